"""voxel_downsample (pb3d/downsample.py, csrc/downsample.hip) against the NumPy restatement of tests/downsample_restate.py, and that
restatement against a plain Python loop.  Every comparison is np.array_equal: include/pb3d.h states the result to the bit, so there is
no tolerance anywhere."""
import ctypes as C
import functools

import numpy as np
import pytest

import downsample_restate as dr

gpu = pytest.mark.gpu

CASES = dr.constructed_cases()
DTYPES = (np.float64, np.float32)
REDUCES = ("centroid", "first")
PARTS = ("out", "index", "inverse", "counts")
SFM_SIZES = (0.5, 0.05)


@functools.lru_cache(maxsize=None)
def sfm(order="forward"):
    p = dr.sfm_cloud()
    if order == "reversed":
        p = p[::-1]
    elif order == "shuffled":
        p = p[np.random.default_rng(2024).permutation(len(p))]
    p = np.ascontiguousarray(p)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def _want(name, f32, reduce):
    """the restatement of a constructed case or of 'sfm/<order>/<voxel_size>', computed once and shared"""
    if name.startswith("sfm/"):
        _, order, vs = name.split("/")
        pts, vs, origin = sfm(order), float(vs), None
    else:
        pts, vs, origin = CASES[name]
    got = dr.restate(pts.astype(np.float32 if f32 else np.float64), vs, origin, reduce)
    for a in got:
        a.setflags(write=False)
    return got


def want(name, dtype, reduce="centroid"):
    return _want(name, dtype == np.float32, reduce)


def same(got, ref, what):
    for g, w, part in zip(got, ref, PARTS):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, part, g.dtype, w.dtype, g.shape, w.shape)
        if not np.array_equal(g.view(np.uint8) if part == "out" else g, w.view(np.uint8) if part == "out" else w):
            bad = np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1))
            raise AssertionError((what, part, "first differing row", int(bad[0]), "rows differing", len(bad), "of", len(g)))


# =====================================================================================================================
# CPU: the restatement against a loop, its invariants, the pinned counts; exports; validation
# =====================================================================================================================

@pytest.mark.parametrize("name", list(CASES))
def test_restatement_is_the_loop(name):
    pts, vs, origin = CASES[name]
    for dt, reduce in ((np.float64, "centroid"), (np.float32, "centroid"), (np.float64, "first")):
        same(want(name, dt, reduce), dr.loop(pts.astype(dt), vs, origin, reduce), (name, dt.__name__, reduce))


@pytest.mark.parametrize("name", list(CASES) + [f"sfm/forward/{vs}" for vs in SFM_SIZES])
def test_restatement_invariants(name):
    for dt in DTYPES:
        out, index, inverse, counts = want(name, dt)
        m, n = len(index), len(inverse)
        assert out.shape == (m, 3) and counts.shape == (m,)
        assert np.array_equal(inverse[index], np.arange(m))
        assert (np.diff(index) > 0).all()
        assert int(counts.sum()) == n and np.array_equal(np.bincount(inverse, minlength=m), counts)
        first = want(name, dt, "first")
        assert all(np.array_equal(a, b) for a, b in zip(first[1:], (index, inverse, counts)))


def test_restatement_on_the_constructed_clouds():
    out, index, inverse, counts = want("faces/lattice", np.float64)
    assert len(index) == 64 and (counts == 8).all()                 # every point on a face: it belongs to the upper voxel
    for a in range(3):
        c = dr.cells(dr.nextafter_points(a), 0.1, (0.0, 0.0, 0.0))[:, a]
        assert int((c == np.arange(1, 200)).sum()) == 12               # quotients that round up to the integer
        assert ((c == np.arange(1, 200)) | (c == np.arange(0, 199))).all()
    assert len(want("keywidth", np.float32)[1]) == len(CASES["keywidth"][0]) == 8
    assert len(want("onevoxel/70001", np.float32)[1]) == 1
    for layout in ("cx", "cz", "random"):
        for dt in DTYPES:
            assert len(want(f"distinct/{layout}", dt)[1]) == 2 ** 17 + 3


def test_run_boundaries_case_tells_orders_apart():
    """the populations are dr.RUN_LENGTHS (as a multiset: voxels are numbered by first appearance), and in float64 the centroid of some
    voxel of 65 or more points changes bits when its points are added in reversed order -- else the case could not catch a wrong order"""
    pts, vs, origin = CASES["runs/boundaries"]
    out, index, inverse, counts = want("runs/boundaries", np.float64)
    assert len(pts) == 772 and sorted(counts.tolist()) == sorted(dr.RUN_LENGTHS)
    differing = 0
    for v in np.flatnonzero(counts >= 65):
        rows = pts[inverse == v].tolist()
        fwd, rev = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
        for r, q in zip(rows, rows[::-1]):
            for a in range(3):
                fwd[a] = fwd[a] + r[a]
                rev[a] = rev[a] + q[a]
        k = float(counts[v])
        assert np.array([s / k for s in fwd]).tobytes() == out[v].tobytes()
        differing += [s / k for s in fwd] != [s / k for s in rev]
    assert differing >= 1


def test_pinned_counts_on_the_sfm_sample():
    for vs, m, largest in ((0.5, 127, 743), (0.05, 5217, 22)):
        counts = want(f"sfm/forward/{vs}", np.float64)[3]
        assert len(counts) == m and int(counts.max()) == largest
    # the order of the additions is part of the result: most centroids change with it
    for vs, sums_changed, rows_changed in ((0.5, 112, 107), (0.05, 2025, 1898)):
        out, index, inverse, counts = want(f"sfm/forward/{vs}", np.float64)
        forward, backward = np.zeros((len(index), 3)), np.zeros((len(index), 3))
        np.add.at(forward, inverse, sfm())
        np.add.at(backward, inverse[::-1], sfm()[::-1])
        assert np.array_equal(forward / counts[:, None], out)
        assert int((backward != forward).any(axis=1).sum()) == sums_changed
        assert int((backward / counts[:, None] != out).any(axis=1).sum()) == rows_changed


def test_exports():
    import pb3d
    for n in ("voxel_downsample", "voxel_downsample_resident"):
        assert callable(getattr(pb3d, n)) and n in pb3d.downsample.__all__
    assert "pb3d_voxel_downsample_resident" in pb3d._lib.EXPORTED_SYMBOLS


def test_validation_needs_no_device():
    import pb3d
    ok = np.zeros((4, 3))
    for bad in (np.nan, np.inf, -np.inf):
        p = ok.copy()
        p[2, 1] = bad
        with pytest.raises(ValueError, match="Input points contains NaN or infinity."):
            pb3d.voxel_downsample(p, 0.1)
    for vs in (0.0, -1.0, np.nan, np.inf):
        for fn in (lambda: pb3d.voxel_downsample(ok, vs), lambda: pb3d.voxel_downsample_resident(None, 4, vs)):
            with pytest.raises(ValueError, match="voxel_size must be finite and > 0"):
                fn()
    for origin in ((0.0, np.nan, 0.0), (np.inf, 0.0, 0.0), (0.0, 0.0), 1.0):
        for fn in (lambda: pb3d.voxel_downsample(ok, 0.1, origin=origin), lambda: pb3d.voxel_downsample_resident(None, 4, 0.1, origin=origin)):
            with pytest.raises(ValueError, match="origin must be three finite values"):
                fn()
    for reduce in ("mean", "", None, 0):
        for fn in (lambda: pb3d.voxel_downsample(ok, 0.1, reduce=reduce), lambda: pb3d.voxel_downsample_resident(None, 4, 0.1, reduce=reduce)):
            with pytest.raises(ValueError, match="reduce must be 'centroid' or 'first'"):
                fn()
    huge = np.broadcast_to(np.zeros((1, 3), np.float32), (2 ** 31, 3))         # a view: no memory behind it
    for fn in (lambda: pb3d.voxel_downsample(huge, 0.1), lambda: pb3d.voxel_downsample_resident(None, 2 ** 31, 0.1)):
        with pytest.raises(ValueError, match="at most 2\\^31 - 1 points"):
            fn()
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        pb3d.voxel_downsample(np.zeros((4, 2)), 0.1)


def test_empty_cloud_needs_no_device():
    import pb3d
    for dt in DTYPES:
        e = np.zeros((0, 3), dt)
        for reduce in REDUCES:
            out = pb3d.voxel_downsample(e, 0.1, reduce=reduce)
            assert out.shape == (0, 3) and out.dtype == dt
            out, index, inverse, counts = pb3d.voxel_downsample(e, 0.1, reduce=reduce, return_index=True, return_inverse=True, return_counts=True)
            assert out.shape == (0, 3) and out.dtype == dt
            assert index.shape == inverse.shape == counts.shape == (0,)
            assert index.dtype == np.intp and inverse.dtype == np.intp and counts.dtype == np.int64
            same((out, index, inverse, counts), dr.restate(e, 0.1, None, reduce), ("empty", dt.__name__, reduce))
    out, counts = pb3d.voxel_downsample(np.zeros((0, 3), np.int32), 0.1, return_counts=True)
    assert out.dtype == np.float64 and counts.shape == (0,)


def test_cabi_refusals_need_no_device():
    import pb3d
    lib = pb3d._lib.load()
    one = C.c_void_p(256)
    m = C.c_int64(7)
    good = (C.c_double * 3)(0.0, 0.0, 0.0)
    fn = lib.pb3d_voxel_downsample_resident

    def refused(rc, text):
        assert rc == -1 and text in lib.pb3d_last_error().decode(), (rc, lib.pb3d_last_error())

    refused(fn(None, one, 1, -1, 0.1, None, 0, one, one, one, one, C.byref(m)), "0 <= n")
    refused(fn(None, one, 1, 2 ** 31, 0.1, None, 0, one, one, one, one, C.byref(m)), "0 <= n")
    for vs in (0.0, -0.5, float("nan"), float("inf")):
        refused(fn(None, one, 1, 5, vs, None, 0, one, one, one, one, C.byref(m)), "voxel_size must be finite and > 0")
    for bad in (float("nan"), float("inf"), float("-inf")):
        for a in range(3):
            o = (C.c_double * 3)(0.0, 0.0, 0.0)
            o[a] = bad
            refused(fn(None, one, 1, 5, 0.1, o, 0, one, one, one, one, C.byref(m)), "origin must be finite")
    for reduce in (-1, 2):
        refused(fn(None, one, 1, 5, 0.1, good, reduce, one, one, one, one, C.byref(m)), "reduce must be 0 (centroid) or 1 (first)")
    refused(fn(None, one, 1, 5, 0.1, good, 0, one, one, one, one, None), "null argument")
    refused(fn(None, None, 1, 5, 0.1, good, 0, one, one, one, one, C.byref(m)), "null buffer")
    refused(fn(None, one, 1, 5, 0.1, good, 0, None, one, one, one, C.byref(m)), "null buffer")
    refused(fn(None, one, 1, 5, 0.1, good, 1, one, None, one, one, C.byref(m)), "null buffer")
    refused(fn(None, one, 1, 5, 0.1, good, 0, one, one, None, None, C.byref(m)), "null context")      # inverse and counts may be NULL
    assert m.value == 7                                                # a refusal writes nothing
    refused(fn(None, None, 0, 0, 0.1, None, 1, None, None, None, None, C.byref(m)), "null context")      # n = 0 needs no buffers
    assert m.value == 7


# =====================================================================================================================
# GPU
# =====================================================================================================================

def via_numpy(pb3d, pts, vs, origin, reduce):
    return pb3d.voxel_downsample(pts, vs, origin=origin, reduce=reduce, return_index=True, return_inverse=True, return_counts=True)


def via_resident(pb3d, pts, vs, origin, reduce):
    """the resident entry on an uploaded cloud, downloaded into the NumPy form's types"""
    n = len(pts)
    d_p = pb3d.device.from_numpy(pts)
    try:
        d_out, d_index, d_inverse, d_counts, m = pb3d.voxel_downsample_resident(d_p, n, vs, origin=origin, reduce=reduce, f64=pts.dtype == np.float64)
        try:
            return (d_out.download((m, 3), pts.dtype), d_index.download((m,), np.int32).astype(np.intp),
                    d_inverse.download((n,), np.int32).astype(np.intp), d_counts.download((m,), np.uint32).astype(np.int64))
        finally:
            for b in (d_out, d_index, d_inverse, d_counts):
                b.free()
    finally:
        d_p.free()


def check(pb3d, name, pts64, vs, origin, dtypes=DTYPES, reduces=REDUCES, forms=(via_numpy, via_resident)):
    for dt in dtypes:
        pts = np.ascontiguousarray(pts64.astype(dt))
        for reduce in reduces:
            ref = want(name, dt, reduce)
            for form in forms:
                same(form(pb3d, pts, vs, origin, reduce), ref, (name, dt.__name__, reduce, form.__name__))
            if reduce == "first":
                out = pb3d.voxel_downsample(pts, vs, origin=origin, reduce="first")
                assert out.tobytes() == pts[ref[1]].tobytes(), (name, dt.__name__, "first rows")


@gpu
@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("faces/")])
def test_faces(pb3d_gpu, name):
    check(pb3d_gpu, name, *CASES[name])


@gpu
@pytest.mark.parametrize("vs", SFM_SIZES)
def test_order(pb3d_gpu, vs):
    """forward, reversed and shuffled: three different sets of centroids, each the restatement's; one order twice gives equal bytes"""
    rows = {}
    for order in ("forward", "reversed", "shuffled"):
        name = f"sfm/{order}/{vs}"
        check(pb3d_gpu, name, sfm(order), vs, None, reduces=("centroid",))
        rows[order] = {r.tobytes() for r in want(name, np.float64)[0]}
    assert rows["forward"] != rows["reversed"] and rows["forward"] != rows["shuffled"] and rows["reversed"] != rows["shuffled"]
    pts = sfm("shuffled")
    once = [a.tobytes() for a in via_resident(pb3d_gpu, pts, vs, None, "centroid")]
    assert [a.tobytes() for a in via_resident(pb3d_gpu, pts, vs, None, "centroid")] == once


@gpu
def test_one_voxel(pb3d_gpu):
    out, index, inverse, counts = via_numpy(pb3d_gpu, sfm(), 100.0, None, "centroid")
    same((out, index, inverse, counts), dr.restate(sfm(), 100.0), "sfm/100")
    assert counts.tolist() == [20000] and index.tolist() == [0] and not inverse.any()
    check(pb3d_gpu, "onevoxel/70001", *CASES["onevoxel/70001"])


@gpu
def test_run_boundaries(pb3d_gpu):
    """voxels of 1, 2, 63, 64, 65, 127, 128, 129 and 193 points: every tail length of the ordered wavefront sum (csrc/ordered_sum.h)"""
    check(pb3d_gpu, "runs/boundaries", *CASES["runs/boundaries"])


@gpu
@pytest.mark.parametrize("layout", ("cx", "cz", "random"))
def test_all_distinct(pb3d_gpu, layout):
    name = f"distinct/{layout}"
    check(pb3d_gpu, name, *CASES[name], forms=(via_resident,))
    check(pb3d_gpu, name, *CASES[name], dtypes=(np.float32,), reduces=("centroid",), forms=(via_numpy,))


@gpu
def test_key_width(pb3d_gpu):
    pts, vs, origin = CASES["keywidth"]
    check(pb3d_gpu, "keywidth", pts, vs, origin)
    for dt in DTYPES:
        assert len(pb3d_gpu.voxel_downsample(pts.astype(dt), vs, origin=origin)) == len(pts)
        for a in range(3):
            p = pts.astype(dt).copy()
            p[3, a] = 2.0 ** 21 + 0.5                                   # cell 2^21
            with pytest.raises(ValueError, match="voxel_size.*origin"):
                pb3d_gpu.voxel_downsample(p, vs, origin=origin)
            o = [0.0, 0.0, 0.0]
            o[a] = 1.0                                                  # above the cloud's minimum: cell -1
            with pytest.raises(ValueError, match="voxel_size.*origin"):
                pb3d_gpu.voxel_downsample(pts.astype(dt), vs, origin=o)
    with pytest.raises(ValueError, match="voxel_size.*origin"):        # the default origin, and a voxel too small for the extent
        pb3d_gpu.voxel_downsample(pts, 0.5)


@gpu
@pytest.mark.parametrize("n", (1, 2, 255, 256, 257, 65537))
def test_seams(pb3d_gpu, n):
    check(pb3d_gpu, f"seams/{n}", *CASES[f"seams/{n}"])


def scan_segments_cloud(n):
    """n points whose first-appearance flags differ from one 1024-flag segment of the rank scan to the next: 3 * 1024 points in cells of
    their own (segments of all ones), 5 * 1024 copies of them (segments of all zeros), then a random mix of new and seen cells; the two
    small sizes get half and half"""
    rng = np.random.default_rng(1026)
    cell = rng.integers(0, 96, (n, 3))
    k = min(n // 2, 3 * 1024)
    cell[:k] = np.stack([np.arange(k) % 96, np.arange(k) // 96, np.full(k, 200)], axis=1)
    copies = min(n - k - 1, 5 * 1024)                   # (the last point is always a random one)
    cell[k:k + copies] = cell[np.arange(copies) % k]
    return cell + rng.choice([0.25, 0.5, 0.75], (n, 3))


@gpu
@pytest.mark.parametrize("n", (1024, 1025, 1024 * 1024 + 1025))
def test_scan_segments(pb3d_gpu, n):
    """The rank scan (pb3d_scan_counts) is given the n first-appearance flags, so its one-workgroup pass over the segment totals
    (k_scan_totals, csrc/wave.h's group_scan_array) sees ceil(n / 1024) of them: one, two, and 1026 -- two per thread of its 1024
    threads with a ragged last thread, the only size at which a thread's run is longer than one.  Both reductions, to the bit."""
    pts = scan_segments_cloud(n)
    for reduce in REDUCES:
        same(via_numpy(pb3d_gpu, pts, 1.0, (0.0, 0.0, 0.0), reduce), dr.restate(pts, 1.0, (0.0, 0.0, 0.0), reduce), (n, reduce))


# ---- buffers that do not start where the allocator put them, and the optional outputs ---------------------------------------------------
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
def test_nulls_and_offsets(pb3d_gpu):
    """the cloud one element (4 or 8 bytes) into its buffer, the outputs one element into theirs; d_inverse and d_counts NULL; entries
    past the voxel count stay untouched"""
    L = pb3d_gpu._lib
    lib, ctx = L.load(), L.ctx()
    name = "seams/257"
    pts64, vs, origin = CASES[name]
    for dt in DTYPES:
        pts = np.ascontiguousarray(pts64.astype(dt))
        n, w = len(pts), pts.dtype.itemsize
        for reduce in REDUCES:
            ref = want(name, dt, reduce)
            m = len(ref[1])
            for elems, extras in ((1, True), (1, False), (0, False)):
                arenas = []

                def arena(nbytes, off, fill, payload=None):
                    arenas.append(Arena(pb3d_gpu, nbytes, off, fill, payload))
                    return arenas[-1]

                try:
                    a_p = arena(pts.nbytes, elems * w, IN_FILL, pts)
                    a_out, a_idx = arena(pts.nbytes, elems * w, OUT_FILL), arena(n * 4, elems * 4, OUT_FILL)
                    a_inv, a_cnt = (arena(n * 4, elems * 4, OUT_FILL), arena(n * 4, elems * 4, OUT_FILL)) if extras else (None, None)
                    got_m = C.c_int64(-1)
                    L.check(lib.pb3d_voxel_downsample_resident(ctx, a_p.ptr, int(w == 8), n, vs, None, dr_reduce(reduce), a_out.ptr, a_idx.ptr,
                                                               a_inv.ptr if extras else None, a_cnt.ptr if extras else None, C.byref(got_m)))
                    what = (name, dt.__name__, reduce, elems, extras)
                    assert got_m.value == m, what
                    got = [a_out.payload(dt)[:3 * m].reshape(m, 3), a_idx.payload(np.int32)[:m].astype(np.intp)]
                    if extras:
                        got += [a_inv.payload(np.int32).astype(np.intp), a_cnt.payload(np.uint32)[:m].astype(np.int64)]
                        assert (a_cnt.payload(np.uint8)[m * 4:] == OUT_FILL).all(), "counts past the voxel count were written"
                    same(got, ref, what)
                    assert (a_out.payload(np.uint8)[m * 3 * w:] == OUT_FILL).all(), "rows past the voxel count were written"
                    assert (a_idx.payload(np.uint8)[m * 4:] == OUT_FILL).all(), "index entries past the voxel count were written"
                    assert np.array_equal(a_p.payload(dt).reshape(n, 3), pts)
                finally:
                    for a in arenas:
                        a.buf.free()


def dr_reduce(reduce):
    return {"centroid": 0, "first": 1}[reduce]


@gpu
def test_host_waits(pb3d_gpu):
    """two host waits a call once the scratch is warm (the bounding box and the voxel count), whichever the reduction"""
    L = pb3d_gpu._lib
    lib, ctx = L.load(), L.ctx()
    pts = np.ascontiguousarray(CASES["seams/65537"][0])
    n = len(pts)
    d_p = pb3d_gpu.device.from_numpy(pts)
    bufs = [pb3d_gpu.device.DeviceBuffer(n * w) for w in (24, 4, 4, 4)]
    try:
        for reduce in (0, 1):
            for rep in range(2):
                before = pb3d_gpu.device.sync_count()
                m = C.c_int64(0)
                L.check(lib.pb3d_voxel_downsample_resident(ctx, C.c_void_p(d_p.ptr), 1, n, 0.25, None, reduce, *(C.c_void_p(b.ptr) for b in bufs),
                                                           C.byref(m)))
                waits = pb3d_gpu.device.sync_count() - before
            assert waits == 2 and m.value == len(want("seams/65537", np.float64)[1]), (reduce, waits)
        before, m = pb3d_gpu.device.sync_count(), C.c_int64(5)          # n = 0: no buffers, no wait
        L.check(lib.pb3d_voxel_downsample_resident(ctx, None, 1, 0, 0.25, None, 0, None, None, None, None, C.byref(m)))
        assert m.value == 0 and pb3d_gpu.device.sync_count() == before
    finally:
        for b in [d_p] + bufs:
            b.free()


@gpu
def test_chain_stays_resident(pb3d_gpu):
    """keep_largest_clusters -> voxel_downsample -> icp_align with the cloud on the device throughout (only counts come back in between)
    equals the same chain through the NumPy forms"""
    pb3d = pb3d_gpu
    src = sfm()
    eps, ms, vs = 0.06, 10, 0.05
    ang = 0.03
    R = np.array([[np.cos(ang), -np.sin(ang), 0.0], [np.sin(ang), np.cos(ang), 0.0], [0.0, 0.0, 1.0]])
    target = np.ascontiguousarray(src[::3] @ R.T + np.array([0.02, -0.01, 0.015]))
    kept = pb3d.keep_largest_clusters(src, eps, ms)
    thin, counts = pb3d.voxel_downsample(kept, vs, return_counts=True)
    T_host = pb3d.icp_align(thin, target, max_iterations=5)
    same((thin, counts), (lambda r: (r[0], r[3]))(dr.restate(kept, vs)), "chain/numpy")

    d_src, d_tgt = pb3d.device.from_numpy(src), pb3d.device.from_numpy(target)
    held = [d_src, d_tgt]
    try:
        d_kept, d_idx, count, _ = pb3d.keep_largest_clusters_resident(d_src, len(src), eps, ms)
        held += [d_kept, d_idx]
        d_thin, d_index, d_inverse, d_counts, m = pb3d.voxel_downsample_resident(d_kept, count, vs)
        held += [d_thin, d_index, d_inverse, d_counts]
        T_dev = pb3d.icp_align_resident(d_thin, m, d_tgt, len(target), max_iterations=5)
        assert count == len(kept) and m == len(thin)
        assert np.array_equal(T_dev, T_host)
        assert np.array_equal(d_thin.download((m, 3), np.float64), thin)
    finally:
        for b in held:
            b.free()
