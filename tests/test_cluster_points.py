"""cluster_points, radius_neighbor_counts, select_points and keep_largest_clusters (pb3d/cluster.py, csrc/cluster.hip) against the NumPy
restatement of tests/cluster_restate.py, and that restatement against scikit-learn.  Every comparison is np.array_equal on integers
and booleans: include/pb3d.h states the result to the bit, so there is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import cluster_restate as cr

gpu = pytest.mark.gpu

CASES = cr.constructed_cases()
NAMES = [c[0] for c in CASES]
DTYPES = (np.float64, np.float32)


def case(name):
    return next(c for c in CASES if c[0] == name)


# =====================================================================================================================
# CPU: the restatement is scikit-learn's DBSCAN; exports; validation
# =====================================================================================================================

@pytest.mark.parametrize("name", NAMES + ["sfm"])
def test_restatement_is_sklearn(name):
    skc = pytest.importorskip("sklearn.cluster")
    pts, eps, ms = (cr.sfm_cloud(), cr.SFM_EPS, cr.SFM_MIN_SAMPLES) if name == "sfm" else case(name)[1:]
    for dt in DTYPES if name != "sfm" else (np.float64,):
        labels, core, counts, sizes = cr.reference(name, dt)
        # the k-d tree compares (dx*dx + dy*dy) + dz*dz with eps*eps and prunes by exact box gaps.  "brute" expands |x|^2 - 2 x.y + |y|^2
        # and loses the offset cloud's digits; "ball_tree" prunes by rounded centroid distances and drops exact ties of the chain
        for algorithm in ("kd_tree", "auto"):
            d = skc.DBSCAN(eps=eps, min_samples=ms, algorithm=algorithm).fit(pts.astype(dt).astype(np.float64))
            assert np.array_equal(d.labels_, labels), (name, dt, algorithm)
            assert np.array_equal(d.core_sample_indices_, np.flatnonzero(core)), (name, dt, algorithm)


def test_restatement_on_the_sfm_sample():
    labels, core, counts, sizes = cr.reference("sfm")
    assert len(sizes) == 36 and labels.max() == 35
    assert sorted(sizes.tolist(), reverse=True)[:5] == [8883, 3072, 1867, 1443, 1359]
    assert int((labels == -1).sum()) == 222
    assert int(core.sum()) == 19017
    assert int(((labels >= 0) & ~core).sum()) == 761
    assert int(sizes.sum()) == 20000 - 222
    assert np.array_equal(core, counts >= cr.SFM_MIN_SAMPLES)


def test_restatement_rules_on_the_bridge():
    """the bridge point is not core and takes the label of the blob that comes first in the input, whichever that is"""
    for order in ("ab-", "ba-", "-ba", "a-b"):
        labels, core, counts, sizes = cr.reference(f"bridge/{order}")
        b = {"ab-": 54, "ba-": 54, "-ba": 0, "a-b": 27}[order]
        assert not core[b] and counts[b] == 3 and labels[b] == 0 and core.sum() == 54
        assert sizes.tolist() == [28, 27]


def test_exports():
    import pb3d
    for n in ("radius_neighbor_counts", "cluster_points", "select_points", "keep_largest_clusters"):
        assert callable(getattr(pb3d, n)) and callable(getattr(pb3d, n + "_resident")), n
        assert n in pb3d.cluster.__all__ and n + "_resident" in pb3d.cluster.__all__
    for n in ("pb3d_radius_count_resident", "pb3d_cluster_points_resident", "pb3d_points_select_resident", "pb3d_labels_member_resident",
              "pb3d_cluster_last"):
        assert n in pb3d._lib.EXPORTED_SYMBOLS


def test_validation_needs_no_device():
    import pb3d
    ok = np.zeros((4, 3))
    for bad in (np.nan, np.inf, -np.inf):
        p = ok.copy()
        p[2, 1] = bad
        for fn in (lambda: pb3d.cluster_points(p, 0.1, 2), lambda: pb3d.radius_neighbor_counts(p, 0.1),
                   lambda: pb3d.keep_largest_clusters(p, 0.1, 2)):
            with pytest.raises(ValueError, match="NaN or infinity"):
                fn()
    for eps in (0.0, -1.0, np.nan, np.inf):
        for fn in (lambda: pb3d.cluster_points(ok, eps, 2), lambda: pb3d.radius_neighbor_counts(ok, eps),
                   lambda: pb3d.keep_largest_clusters(ok, eps, 2), lambda: pb3d.cluster_points_resident(None, 4, eps, 2),
                   lambda: pb3d.radius_neighbor_counts_resident(None, 4, eps)):
            with pytest.raises(ValueError, match="eps must be finite and > 0"):
                fn()
    for ms in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="min_samples must be an integer >= 1"):
            pb3d.cluster_points(ok, 0.1, ms)
        with pytest.raises(ValueError, match="min_samples must be an integer >= 1"):
            pb3d.cluster_points_resident(None, 4, 0.1, ms)
    with pytest.raises(ValueError, match="k must be an integer >= 1"):
        pb3d.keep_largest_clusters(ok, 0.1, 2, k=0)
    huge = np.broadcast_to(np.zeros((1, 3), np.float32), (2 ** 31, 3))         # a view: no memory behind it
    for fn in (lambda: pb3d.cluster_points(huge, 0.1, 2), lambda: pb3d.radius_neighbor_counts(huge, 0.1),
               lambda: pb3d.select_points(huge, np.zeros(1, bool)), lambda: pb3d.keep_largest_clusters(huge, 0.1, 2),
               lambda: pb3d.cluster_points_resident(None, 2 ** 31, 0.1, 2), lambda: pb3d.select_points_resident(None, 2 ** 31, None)):
        with pytest.raises(ValueError, match="at most 2\\^31 - 1 points"):
            fn()
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        pb3d.cluster_points(np.zeros((4, 2)), 0.1, 2)
    with pytest.raises(ValueError, match="keep must be"):
        pb3d.select_points(ok, np.zeros(3, bool))
    with pytest.raises(ValueError, match="keep must be"):
        pb3d.select_points(ok, np.zeros(4, np.float64))
    # n = 0: empty arrays, no device
    for dt in DTYPES:
        e = np.zeros((0, 3), dt)
        labels, core, counts, sizes = pb3d.cluster_points(e, 0.1, 2)
        assert labels.shape == (0,) and labels.dtype == np.int64 and core.dtype == bool and counts.dtype == np.int64 and sizes.shape == (0,)
        assert pb3d.radius_neighbor_counts(e, 0.1).shape == (0,)
        kept, idx = pb3d.select_points(e, np.zeros(0, bool))
        assert kept.shape == (0, 3) and kept.dtype == dt and idx.shape == (0,)
        kept, idx = pb3d.keep_largest_clusters(e, 0.1, 2, return_index=True)
        assert kept.shape == (0, 3) and kept.dtype == dt and idx.shape == (0,)


def test_cabi_refusals_need_no_device():
    import pb3d
    L = pb3d._lib
    lib = L.load()
    one = C.c_void_p(256)
    nc = C.c_int64(7)

    def refused(rc, text):
        assert rc == -1 and text in lib.pb3d_last_error().decode(), (rc, lib.pb3d_last_error())

    refused(lib.pb3d_cluster_points_resident(None, one, 1, -1, 0.1, 2, one, one, one, one, C.byref(nc)), "0 <= n")
    refused(lib.pb3d_cluster_points_resident(None, one, 1, 5, 0.0, 2, one, one, one, one, C.byref(nc)), "eps must be finite")
    refused(lib.pb3d_cluster_points_resident(None, one, 1, 5, float("nan"), 2, one, one, one, one, C.byref(nc)), "eps must be finite")
    refused(lib.pb3d_cluster_points_resident(None, one, 1, 5, float("inf"), 2, one, one, one, one, C.byref(nc)), "eps must be finite")
    refused(lib.pb3d_cluster_points_resident(None, one, 1, 5, 0.1, 0, one, one, one, one, C.byref(nc)), "min_samples must be >= 1")
    refused(lib.pb3d_cluster_points_resident(None, None, 1, 5, 0.1, 2, one, one, one, one, C.byref(nc)), "null buffer")
    refused(lib.pb3d_cluster_points_resident(None, one, 1, 5, 0.1, 2, one, one, one, one, None), "null argument")
    refused(lib.pb3d_cluster_points_resident(None, one, 1, 5, 0.1, 2, one, one, one, one, C.byref(nc)), "null context")
    refused(lib.pb3d_radius_count_resident(None, one, 1, 5, -2.0, one), "eps must be finite")
    refused(lib.pb3d_radius_count_resident(None, one, 1, 5, 0.1, one), "null context")
    refused(lib.pb3d_points_select_resident(None, one, 1, -1, one, one, None, one), "0 <= n")
    refused(lib.pb3d_points_select_resident(None, one, 1, 5, None, one, None, one), "null buffer")
    refused(lib.pb3d_points_select_resident(None, one, 1, 5, one, one, None, None), "null argument")
    refused(lib.pb3d_points_select_resident(None, one, 1, 5, one, one, None, one), "null context")
    refused(lib.pb3d_labels_member_resident(None, one, 5, None, 3, one), "null argument")
    refused(lib.pb3d_labels_member_resident(None, one, 5, None, 0, one), "null context")
    refused(lib.pb3d_cluster_last(None, None, None), "null argument")


# =====================================================================================================================
# GPU
# =====================================================================================================================

def via_numpy(pb3d, pts, eps, ms):
    return pb3d.cluster_points(pts, eps, ms)


def via_resident(pb3d, pts, eps, ms):
    """the resident entry on an uploaded cloud, downloaded into the NumPy form's types"""
    n = len(pts)
    d_p = pb3d.device.from_numpy(pts)
    try:
        d_lab, d_core, d_cnt, d_sizes, nc = pb3d.cluster_points_resident(d_p, n, eps, ms, f64=pts.dtype == np.float64)
        try:
            return (d_lab.download((n,), np.int32).astype(np.int64), d_core.download((n,), np.uint8) != 0,
                    d_cnt.download((n,), np.uint32).astype(np.int64), d_sizes.download((nc,), np.int64))
        finally:
            for b in (d_lab, d_core, d_cnt, d_sizes):
                b.free()
    finally:
        d_p.free()


def same(got, want, what):
    for g, w, part in zip(got, want, ("labels", "core", "counts", "sizes")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, part, g.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (what, part, int(np.flatnonzero(g != w)[0]), int((g != w).sum()))


def check_case(pb3d, name, pts64, eps, ms, dtypes=DTYPES):
    for dt in dtypes:
        pts = np.ascontiguousarray(pts64.astype(dt))
        want = cr.reference(name, dt)
        same(via_numpy(pb3d, pts, eps, ms), want, (name, dt.__name__, "numpy"))
        same(via_resident(pb3d, pts, eps, ms), want, (name, dt.__name__, "resident"))
        counts = pb3d.radius_neighbor_counts(pts, eps)
        assert counts.dtype == np.int64 and np.array_equal(counts, want[2]), (name, dt.__name__, "radius_neighbor_counts")


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_constructed(pb3d_gpu, name):
    _, pts, eps, ms = case(name)
    check_case(pb3d_gpu, name, pts, eps, ms)


@gpu
def test_chain_labels_follow_the_minimum_index(pb3d_gpu):
    """three chains in shuffled order: cluster c is the chain whose smallest input position is the c-th smallest"""
    _, pts, eps, ms = case("chain/cut-shuffled")
    labels = pb3d_gpu.cluster_points(pts, eps, ms)[0]
    firsts = [int(np.flatnonzero(labels == c)[0]) for c in range(3)]
    assert firsts == sorted(firsts) and firsts[0] == 0 and set(labels.tolist()) == {0, 1, 2}
    pos = np.rint(pts[:, 0] * 32.0).astype(np.int64)                 # the position along the chain
    for c in range(3):
        run = np.sort(pos[labels == c])
        assert np.array_equal(run, np.arange(run[0], run[0] + len(run))), c


@gpu
def test_sfm_sample(pb3d_gpu):
    check_case(pb3d_gpu, "sfm", cr.sfm_cloud(), cr.SFM_EPS, cr.SFM_MIN_SAMPLES)


@gpu
def test_both_cell_edges_give_the_same_result(pb3d_gpu):
    """knob cluster_cell: the index with two points per cell (1) and with cells wider than eps (2); no result depends on it"""
    L = pb3d_gpu._lib
    lib, ctx = L.load(), L.ctx()
    names = ["lattice/eps=sqrt2/ms=4", "lattice/eps=2/ms=7", "chain/cut-shuffled", "degenerate/eps>diagonal", "degenerate/offset",
             "degenerate/flat", "size/257", "sfm"]
    cells = {}
    try:
        for knob in (1, 2, 0):
            L.set_tuning("cluster_cell", knob)
            for name in names:
                pts, eps, ms = (cr.sfm_cloud(), cr.SFM_EPS, cr.SFM_MIN_SAMPLES) if name == "sfm" else case(name)[1:]
                same(via_numpy(pb3d_gpu, pts, eps, ms), cr.reference(name), (name, "cluster_cell", knob))
                c = (C.c_int64 * 3)()
                L.check(lib.pb3d_cluster_last(ctx, c, None))
                cells[knob, name] = tuple(c)
    finally:
        L.set_tuning("cluster_cell", 0)
    # the two grids differ where eps exceeds the two-points-per-cell edge: the dense lattice at eps 2 (extent 11: at most 5 cells per
    # axis), and eps beyond the diagonal (one cell, against every ring of the finer grid).  Under 2 and 0 every cell is wider than eps
    assert cells[2, "degenerate/eps>diagonal"] == (1, 1, 1) and int(np.prod(cells[1, "degenerate/eps>diagonal"])) > 27
    assert max(cells[2, "lattice/eps=2/ms=7"]) <= 5 < max(cells[1, "lattice/eps=2/ms=7"])
    for name in names:
        pts, eps = (cr.sfm_cloud(), cr.SFM_EPS) if name == "sfm" else case(name)[1:3]
        for knob in (2, 0):
            assert all(c == 1 or e / c > eps for e, c in zip(np.ptp(pts, axis=0), cells[knob, name])), (name, knob, cells[knob, name])
            assert all(c2 <= c1 for c1, c2 in zip(cells[1, name], cells[knob, name])), (name, knob)
    with pytest.raises(ValueError, match="not timed"):
        L.check(lib.pb3d_cluster_last(ctx, (C.c_int64 * 3)(), (C.c_double * 5)()))


@gpu
def test_determinism(pb3d_gpu):
    """the same call five times: identical bytes (the union-find's roots are component minima whatever the interleaving)"""
    for name in ("sfm", "chain/shuffled", "lattice/eps=sqrt2/ms=4"):
        pts, eps, ms = (cr.sfm_cloud(), cr.SFM_EPS, cr.SFM_MIN_SAMPLES) if name == "sfm" else case(name)[1:]
        first = [a.tobytes() for a in via_resident(pb3d_gpu, pts, eps, ms)]
        for _ in range(4):
            assert [a.tobytes() for a in via_resident(pb3d_gpu, pts, eps, ms)] == first, name


@gpu
def test_select_points(pb3d_gpu):
    rng = np.random.default_rng(77)
    for n in (1, 255, 256, 257, 5000):
        for dt in DTYPES:
            pts = rng.standard_normal((n, 3)).astype(dt)
            pts[rng.random(n) < 0.05] = np.nan                       # rows are copied byte for byte, never through arithmetic
            for keep in (rng.random(n) < 0.4, np.ones(n, bool), np.zeros(n, bool), rng.integers(0, 3, n).astype(np.uint8),
                         (rng.integers(-1, 2, n) * 256).astype(np.int32)):
                got, idx = pb3d_gpu.select_points(pts, keep)
                want = pts[keep != 0]
                assert got.dtype == dt and np.array_equal(got.view(np.uint8), want.view(np.uint8)), (n, dt, keep.dtype)
                assert idx.dtype == np.intp and np.array_equal(idx, np.flatnonzero(keep)), (n, dt, keep.dtype)


def largest(sizes, k):
    return sorted(sorted(range(len(sizes)), key=lambda c: (-int(sizes[c]), c))[:k])


@gpu
def test_keep_largest_clusters(pb3d_gpu):
    two_blobs = {o: cr.bridge_cloud(o) for o in ("ab", "ba")}             # sizes 27 and 27: the tie goes to label 0, the first in the input
    jobs = [("sfm", cr.sfm_cloud(), cr.SFM_EPS, cr.SFM_MIN_SAMPLES, cr.reference("sfm")),
            ("lattice", *case("lattice/eps=1/ms=4")[1:], cr.reference("lattice/eps=1/ms=4"))]
    jobs += [(f"tie/{o}", p, 1.0, 4, cr.restate(p, 1.0, 4)) for o, p in two_blobs.items()]
    for name, pts, eps, ms, (labels, core, counts, sizes) in jobs:
        if name.startswith("tie"):
            assert sizes.tolist() == [27, 27]
        for k in (1, 3, len(sizes), len(sizes) + 5):
            chosen = largest(sizes, k)
            mask = np.isin(labels, chosen)
            for dt in DTYPES if name != "sfm" else (np.float64,):
                p = np.ascontiguousarray(pts.astype(dt))
                got, idx = pb3d_gpu.keep_largest_clusters(p, eps, ms, k=k, return_index=True)
                assert got.dtype == dt and np.array_equal(got, p[mask]), (name, k, dt)
                assert np.array_equal(idx, np.flatnonzero(mask)), (name, k, dt)
                assert np.array_equal(pb3d_gpu.keep_largest_clusters(p, eps, ms, k=k), p[mask]), (name, k, dt)
        if name.startswith("tie"):
            assert np.array_equal(pb3d_gpu.keep_largest_clusters(pts, eps, ms), pts[:27]), name
    # the resident form: the cloud stays on the device, the chosen labels come back
    pts = cr.sfm_cloud()
    labels, _, _, sizes = cr.reference("sfm")
    d_p = pb3d_gpu.device.from_numpy(pts)
    try:
        d_out, d_idx, count, chosen = pb3d_gpu.keep_largest_clusters_resident(d_p, len(pts), cr.SFM_EPS, cr.SFM_MIN_SAMPLES, k=3)
        try:
            mask = np.isin(labels, largest(sizes, 3))
            assert count == int(mask.sum()) and chosen.tolist() == largest(sizes, 3)
            assert np.array_equal(d_out.download((count, 3), np.float64), pts[mask])
            assert np.array_equal(d_idx.download((count,), np.int32), np.flatnonzero(mask))
        finally:
            d_out.free(); d_idx.free()
    finally:
        d_p.free()


# ---- buffers that do not start where the allocator put them -----------------------------------------------------------------------------
GUARD = 256
IN_FILL, OUT_FILL = 0xFF, 0xA5


class Arena:
    """a payload at GUARD + off bytes inside a 256-byte aligned allocation, guard bytes on both sides"""

    def __init__(self, pb3d, nbytes, off, fill, payload=None):
        self.off, self.n, self.fill = int(off), int(nbytes), fill
        total = GUARD + self.off + self.n + GUARD
        total += -total % 256
        self.buf = pb3d.device.DeviceBuffer(total)
        assert self.buf.ptr % 256 == 0
        self.host = np.full(total, fill, np.uint8)
        if payload is not None:
            self.host[GUARD + self.off:GUARD + self.off + self.n] = np.ascontiguousarray(payload).view(np.uint8).reshape(-1)
        self.buf.upload(self.host)
        self.ptr = self.buf.at(GUARD + self.off)

    def payload(self, dtype):
        """the payload, after checking that both guards still hold the fill"""
        got = self.buf.download((self.buf.nbytes,))
        lo, hi = GUARD + self.off, GUARD + self.off + self.n
        assert (got[:lo] == self.fill).all() and (got[hi:] == self.fill).all(), "a guard zone was written"
        return got[lo:hi].copy().view(dtype)


@gpu
def test_buffers_at_odd_offsets(pb3d_gpu):
    """every buffer of the three entries one or three elements (any byte for the byte buffers) off its allocation; the index reads the
    rows element by element and the outputs are stored by element, so nothing may depend on the base address"""
    L = pb3d_gpu._lib
    lib, ctx = L.load(), L.ctx()
    name = "size/257"
    _, pts64, eps, ms = case(name)
    for dt in DTYPES:
        pts = np.ascontiguousarray(pts64.astype(dt))
        n, w = len(pts), pts.dtype.itemsize
        want = cr.reference(name, dt)
        keep = (want[0] == int(np.argmax(want[3]))).astype(np.uint8)
        for elems, byte in ((0, 0), (1, 1), (3, 3), (1, 64)):
            arenas = []

            def arena(nbytes, off, fill, payload=None):
                arenas.append(Arena(pb3d_gpu, nbytes, off, fill, payload))
                return arenas[-1]

            try:
                a_p = arena(pts.nbytes, elems * w, IN_FILL, pts)
                a_lab, a_core, a_cnt, a_sz = (arena(n * 4, elems * 4, OUT_FILL), arena(n, byte, OUT_FILL), arena(n * 4, elems * 4, OUT_FILL),
                                              arena(n * 8, elems * 8, OUT_FILL))
                nc = C.c_int64(0)
                L.check(lib.pb3d_cluster_points_resident(ctx, a_p.ptr, int(w == 8), n, eps, ms, a_lab.ptr, a_core.ptr, a_cnt.ptr, a_sz.ptr,
                                                         C.byref(nc)))
                got = (a_lab.payload(np.int32).astype(np.int64), a_core.payload(np.uint8) != 0, a_cnt.payload(np.uint32).astype(np.int64),
                       a_sz.payload(np.int64)[:nc.value])
                same(got, want, (name, dt.__name__, "offsets", elems, byte))
                assert (a_sz.payload(np.uint8)[nc.value * 8:] == OUT_FILL).all(), "sizes past the cluster count were written"
                a_rc = arena(n * 4, elems * 4, OUT_FILL)
                L.check(lib.pb3d_radius_count_resident(ctx, a_p.ptr, int(w == 8), n, eps, a_rc.ptr))
                assert np.array_equal(a_rc.payload(np.uint32), want[2])
                a_keep = arena(n, byte, IN_FILL, keep)
                a_out, a_idx, a_count = arena(pts.nbytes, elems * w, OUT_FILL), arena(n * 4, elems * 4, OUT_FILL), arena(8, elems * 8, OUT_FILL)
                L.check(lib.pb3d_points_select_resident(ctx, a_p.ptr, int(w == 8), n, a_keep.ptr, a_out.ptr, a_idx.ptr, a_count.ptr))
                k = int(a_count.payload(np.int64)[0])
                assert k == int(keep.sum())
                assert np.array_equal(a_out.payload(dt)[:3 * k].reshape(k, 3), pts[keep != 0])
                assert (a_out.payload(np.uint8)[k * 3 * w:] == OUT_FILL).all(), "rows past the count were written"
                assert np.array_equal(a_idx.payload(np.int32)[:k], np.flatnonzero(keep))
                assert np.array_equal(a_p.payload(dt).reshape(n, 3), pts) and np.array_equal(a_keep.payload(np.uint8), keep)
            finally:
                for a in arenas:
                    a.buf.free()
