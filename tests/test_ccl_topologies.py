"""The connected-component labelling (csrc/ccl.hip) on the constructed cases of tests/ccl_cases.py against scipy.ndimage.label.

CPU tests: every case holds what its builder claims (ccl_cases.CLAIMS), judged by scipy and by the window arithmetic alone.
GPU tests: every case at 6-, 18- and 26-connectivity, full and members-only, into a label buffer poisoned with -7; labels, component
counts and statistics equal scipy's exactly.  Builders 1, 3 and 4 again under the merge knobs (ccl_merge, ccl_tilecols); builder 5
three times over (the unions race by design, the result may not)."""
import numpy as np
import pytest
from scipy import ndimage

import ccl_cases as cc
from test_top_k_components import STRUCT, scipy_stats

CAP = 4096                      # host records per colour; the device keeps min(CAP, 16384 // K)
POISON = -7
GPU_BUILDERS = list(cc.BUILDERS)
KNOB_BUILDERS = ["long_rows", "long_rows_multi", "tile_seams", "implied_links"]
KNOBS = [("ccl_merge", 1), ("ccl_tilecols", 2), ("ccl_tilecols", 8), ("ccl_tilecols", 64)]
_ref = {}


def reference(case, conn):
    """scipy's (labels, n, bbox, count, sums) per colour; the rgb and the label-volume form of a case share their masks"""
    key = (case[0].rsplit("/", 1)[0], conn)
    if key not in _ref:
        _ref[key] = [scipy_stats(m, conn) for m in cc.masks(case)]
    return _ref[key]


def ncomp(mask, conn):
    return ndimage.label(mask, structure=STRUCT[conn])[1]


def face_degree(mask):
    """the number of face neighbours of every voxel that are members"""
    m = np.pad(mask, 1).astype(np.int8)
    return (m[2:, 1:-1, 1:-1] + m[:-2, 1:-1, 1:-1] + m[1:-1, 2:, 1:-1] + m[1:-1, :-2, 1:-1] + m[1:-1, 1:-1, 2:] + m[1:-1, 1:-1, :-2])


# ---- CPU: the cases are what their names say ---------------------------------------------------------------------------------------
def test_case_names_and_sizes():
    seen = set()
    for b in cc.BUILDERS:
        cs = cc.cases(b)
        assert cs, b
        for name, grid, colours, channels in cs:
            assert name not in seen, name
            seen.add(name)
            assert name in cc.CLAIMS and cc.CLAIMS[name], name
            assert grid.dtype == np.uint8 and grid.ndim == (4 if channels == 3 else 3) and np.prod(grid.shape[:3]) <= cc.MAX_VOXELS, name
            assert 1 <= len(colours) <= 8, name
            ms = cc.masks((name, grid, colours, channels))
            assert all(m.any() for m in ms), name
            background = ~np.any(ms, axis=0)
            other = background & (grid.reshape(grid.shape[:3] + (-1,)).any(-1))
            assert other.any() or background.sum() <= 5, name + ": no voxel of a colour that is not asked for"


@pytest.mark.parametrize("builder", GPU_BUILDERS)
def test_claims(builder):
    by_name = {c[0]: c for c in cc.cases(builder)}
    for name, case in by_name.items():
        claims = cc.CLAIMS[name]
        ms = cc.masks(case)
        m = ms[0]
        A2 = m.shape[2]
        for key, want in claims.items():
            if key in ("n6", "n18", "n26"):
                assert ncomp(m, int(key[1:])) == want, (name, key)
            elif key == "members_eq_n6":
                assert ncomp(m, 6) == int(m.sum()) > 1, name
            elif key == "members":
                assert int(m.sum()) == want, name
            elif key == "ncomp":
                assert [ncomp(x, 6) for x in ms] == want and [ncomp(x, 26) for x in ms] == want, name
                assert want[0] > 16384 // len(ms) >= max(want[1:]), name
            elif key == "edges":                                 # a run over voxels E - 1 and E of some row
                assert want and want[0] == 1024, name
                for E in want:
                    assert (m[:, :, E - 1] & m[:, :, E]).any(), (name, E)
            elif key == "ft":                                    # a pass-through window at these window indices
                pt = cc.passthrough_windows(m)
                for t in want:
                    assert pt[:, t].any(), (name, t)
            elif key == "chunk_through":                         # a run that passes through all sixteen windows of chunk 1
                assert (A2 >= 2048 and bool(cc.passthrough_windows(m)[:, 16:32].all(1).any())) == want, name
            elif key == "abut":                                  # two different colours at E - 1 and E, no gap
                idx = np.zeros(m.shape, np.int8)
                for k, x in enumerate(ms):
                    idx[x] = k + 1
                assert want, name
                for E in want:
                    a, b = idx[:, :, E - 1], idx[:, :, E]
                    assert ((a > 0) & (b > 0) & (a != b)).any(), (name, E)
            elif key == "absent_chunk":
                assert any((x[:, :, :1024].any(2) & ~x[:, :, 1024:2048].any(2) & x[:, :, 2048:3072].any(2)).any() for x in ms), name
            elif key == "segs":
                seg = cc.segments_per_window(m)
                assert set(want) <= set(seg.ravel().tolist()), name
            elif key == "alt89":                                 # windows of 8 and of 9 segments next to each other inside one group of 64
                seg = cc.segments_per_window(m).ravel()[:64]
                assert set(seg.tolist()) == {8, 9} and np.all(seg[1:] != seg[:-1]), name
            elif key == "root_windows":
                got = set(cc.run_start_windows(m).tolist())
                assert got == set(want), name
                assert {1022, 1023, 1024, 1025, 1026} <= got and {252, 253, 255, 256, 257, 1020} <= got, name       # threads 63 | 64, 255 | block 1
            elif key == "group_rows":                            # rows that start an RT-row group, for every RT the knobs give
                P = (A2 + 63) // 64
                for rt in cc._rts(P):
                    if rt > 1 and rt <= m.shape[1] - 1:
                        assert any(g % rt == 0 for g in want), (name, rt)
                assert want, name
            elif key == "implied":
                got = cc.implied_links(m)
                for k2, v in want.items():
                    assert got[k2] == v, (name, k2, got)
                if "apart" not in name:
                    assert got["overlaps"] > 0, name
            elif key == "group_first_rows":                      # overlaps at row 0 and at first rows of RT groups (RT > 1)
                rows = {r for x in range(m.shape[0] - 1) for r in range(m.shape[1]) if (m[x, r] & m[x + 1, r]).any()}
                assert 0 in rows and want, name
                P = (A2 + 63) // 64
                for rt in cc._rts(P):
                    if rt > 1:
                        assert any(r and r % rt == 0 for r in rows), (name, rt)
            elif key == "twin_n6":
                twin = by_name[name.replace("joined", "apart")]
                n_twin = ncomp(cc.masks(twin)[0], 6)
                assert n_twin == want and n_twin - ncomp(m, 6) == want - claims["n6"] > 0, name
            elif key == "path":                                  # one voxel wide: two ends, every other voxel has two neighbours
                deg = face_degree(m)[m]
                assert (deg == 1).sum() == 2 and (deg == 2).sum() == deg.size - 2, name
            elif key == "first_voxel_on_prong":                  # the raster-first voxel of every component is the tip of a prong
                lab, n = ndimage.label(m)
                deg = face_degree(m).ravel()
                first = ndimage.minimum(np.arange(m.size).reshape(m.shape), lab, np.arange(1, n + 1)).astype(np.int64)
                assert np.all(deg[first] == 1), name
            else:
                raise AssertionError(f"{name}: unknown claim {key}")


def test_long_rows_cover_every_length_and_kind():
    names = [c[0] for c in cc.cases("long_rows")]
    for A2 in cc.LONG_A2:
        for kind in ("full", "edge2", "gap", "hole", "cross", "cross_pt", "inner", "bit63"):
            for ch in ("rgb", "lab"):
                assert any(n.startswith(f"long/{A2}/") and kind in n.split("/")[2].split("+") and n.endswith(ch) for n in names), (A2, kind, ch)
    multi = [c[0] for c in cc.cases("long_rows_multi")]
    assert {n.split("/")[2] for n in multi} == {"K2", "K3", "K5", "K8"}
    for K in (2, 3, 5, 8):
        assert f"longmulti/3073/K{K}/rgb" in multi and f"longmulti/4100/K{K}/lab" in multi


def test_rows_per_wave_forms():
    """A2 = 16 .. 1024 gives every rows-per-wave form of k_ccl_init (16, 8, 4, 2, 1 rows), on a row count that is no multiple of 16"""
    forms = set()
    for _, grid, _, _ in cc.cases("rows_per_wave"):
        A0, A1, A2 = grid.shape[:3]
        assert (A0 * A1) % 16
        lgR = 0
        while lgR < 4 and A2 <= (1024 >> (lgR + 1)):
            lgR += 1
        forms.add(lgR)
    assert forms == {0, 1, 2, 3, 4}


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
class Device:
    """a case's grid and a label buffer on the device; run() poisons the buffer, labels, and brings labels and statistics back"""

    def __init__(self, case):
        from pb3d import device as dev
        self.case = case
        self.shape3 = case[1].shape[:3]
        self.d_g = self.d_lab = None
        self.poison = np.full(self.shape3, POISON, np.int32)
        self.d_g = dev.from_numpy(case[1])
        self.d_lab = dev.DeviceBuffer(self.poison.nbytes)

    def run(self, conn, members_only):
        from pb3d.voxel_utils import _label_stats_conn
        self.d_lab.upload(self.poison)
        res = _label_stats_conn(self.d_g, self.shape3, self.case[2], self.d_lab, conn, cap=CAP, members_only=members_only, channels=self.case[3])
        return self.d_lab.download(self.shape3, np.int32), res

    def free(self):
        for b in (self.d_g, self.d_lab):
            if b is not None:
                b.free()


def check(case, conn, members_only, lab, res):
    name = case[0]
    ms = cc.masks(case)
    capacity = min(CAP, 16384 // len(ms))
    anymask = np.zeros(lab.shape, bool)
    for k, (m, (n, bbox, cnt, sums), (rl, rn, rb, rc, rs)) in enumerate(zip(ms, res, reference(case, conn))):
        where = (name, conn, members_only, k)
        anymask |= m
        assert n == rn, where + (n, rn)
        assert np.array_equal(lab[m], rl[m]), where
        if rn > capacity:
            assert bbox is None and cnt is None and sums is None, where
        else:
            assert bbox is not None, where
            assert np.array_equal(bbox, rb) and np.array_equal(cnt, rc) and np.array_equal(sums, rs), where
    rest = lab[~anymask]
    if members_only:
        assert np.all((rest == POISON) | (rest == 0)), (name, conn)
    else:
        assert not rest.any(), (name, conn)


def same_result(a, b):
    (la, ra), (lb, rb) = a, b
    if not np.array_equal(la, lb) or len(ra) != len(rb):
        return False
    for x, y in zip(ra, rb):
        if x[0] != y[0] or (x[1] is None) != (y[1] is None):
            return False
        if x[1] is not None and not all(np.array_equal(p, q) for p, q in zip(x[1:], y[1:])):
            return False
    return True


@pytest.mark.gpu
@pytest.mark.parametrize("builder", GPU_BUILDERS)
def test_labelling(pb3d_gpu, builder):
    from pb3d import device as dev
    from pb3d.voxel_carving_utils import _component_stats, _label
    for case in cc.cases(builder):
        d = Device(case)
        d_full = None
        try:
            for conn in (6, 18, 26):
                for members_only in (False, True):
                    lab, res = d.run(conn, members_only)
                    check(case, conn, members_only, lab, res)
            if case[3] == 3:            # the plain 6-connected entry (no statistics), and the separate statistics pass on its volume
                d_full = dev.DeviceBuffer(d.poison.nbytes)
                for colour, (rl, rn, rb, rc, rs) in zip(case[2], reference(case, 6)):
                    d_full.upload(d.poison)
                    n = _label(d.d_g, d.shape3, colour, d_full)
                    assert n == rn, case[0]
                    assert np.array_equal(d_full.download(d.shape3, np.int32), rl), case[0]
                    bbox, cnt, sums = _component_stats(d_full, d.shape3, n)
                    assert np.array_equal(bbox, rb) and np.array_equal(cnt, rc) and np.array_equal(sums, rs), case[0]
        finally:
            d.free()
            if d_full is not None:
                d_full.free()


@pytest.mark.gpu
@pytest.mark.parametrize("knob", KNOBS, ids=lambda k: f"{k[0]}{k[1]}")
@pytest.mark.parametrize("builder", KNOB_BUILDERS)
def test_merge_knobs(pb3d_gpu, builder, knob):
    """the pairwise merge and the tile merge at every RT give the default form's bytes, and scipy's labels"""
    set_tuning = pb3d_gpu._lib.set_tuning
    try:
        for case in cc.cases(builder):
            d = Device(case)
            try:
                for conn in (6, 18, 26):
                    for members_only in (False, True):
                        set_tuning("ccl_merge", 0); set_tuning("ccl_tilecols", 0)
                        base = d.run(conn, members_only)
                        set_tuning(*knob)
                        got = d.run(conn, members_only)
                        check(case, conn, members_only, *got)
                        assert same_result(base, got), (case[0], conn, members_only, knob)
            finally:
                d.free()
    finally:
        set_tuning("ccl_merge", 0); set_tuning("ccl_tilecols", 0)


@pytest.mark.gpu
def test_repeat_runs_identical(pb3d_gpu):
    for case in cc.cases("shapes"):
        d = Device(case)
        try:
            for conn in (6, 18, 26):
                runs = [d.run(conn, False) for _ in range(3)]
                check(case, conn, False, *runs[0])
                assert same_result(runs[0], runs[1]) and same_result(runs[0], runs[2]), (case[0], conn)
        finally:
            d.free()
