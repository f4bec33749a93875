"""icp_align / transform_points (pb3d/preprocess_helpers.py on csrc/icp.hip): rigid ICP with both clouds resident on the device.

There is no upstream text to be exact against, so the chain of evidence is: include/pb3d.h states the arithmetic; tests/icp_restate.py
restates it in NumPy; the CPU tests below pin the restatement (its sums against exact sums with a bound that follows from the float
width, its correspondences against cKDTree, its loop against a motion it must recover); the GPU tests demand the restatement's BYTES
from the device -- counts, all 16 sums, every transform and rmse of a whole alignment."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

import icp_restate as ir

gpu = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -53


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@functools.lru_cache(maxsize=None)
def restated_alignment(degrees, dtype_name, gate):
    """one restated alignment per case, shared by the CPU and the GPU tests (read-only)"""
    s, t, M, extent = ir.recovery_case(degrees, np.dtype(dtype_name).type)
    T, hist, Ts = ir.icp_align(s, t, max_distance=None if gate is None else gate * extent)
    for a in (s, t, M, T, *Ts):
        a.setflags(write=False)
    return s, t, M, extent, T, hist, Ts


# ---- CPU: the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 257, 5000, 65537])
def test_restated_sums_against_exact_sums(n):
    """any summation order of n terms errs by at most n * 2^-53 * sum|term| (each of the n - 1 additions adds a relative 2^-53 of a
    partial sum that is itself bounded by sum|term|): derived, not measured"""
    rng = np.random.default_rng(n)
    src = rng.normal(size=(n, 3)) * (3.0, 1.0, 0.2) + (10.0, -4.0, 0.5)
    tgt = rng.normal(size=(97, 3)) * (3.0, 1.0, 0.2) + (10.0, -4.0, 0.5)
    T = np.eye(4)
    T[:3, :3] = ir.rotation((0.3, -1.0, 0.2), 7.0)
    T[:3, 3] = (0.1, -0.2, 0.05)
    cp, cq = np.array([9.5, -4.25, 0.4]), np.array([10.25, -3.5, 0.6])
    _, used, t = ir.pairs(src, tgt, T, 2.0, cp, cq)
    assert 0 < used.sum() <= n and (n < 255 or used.sum() < n)       # the gate drops some pairs of the larger clouds
    got = ir.ordered_sum(t)
    for c in range(16):
        exact = math.fsum(t[:, c].tolist())
        bound = n * U * math.fsum(np.abs(t[:, c]).tolist())
        print(f"n={n} term {c}: |restated - exact| = {abs(got[c] - exact):.3e}, bound {bound:.3e}")
        assert abs(got[c] - exact) <= bound, (n, c)
    count, sums = ir.step(src, tgt, T, 2.0, cp, cq)
    assert count == int(used.sum()) and same_bytes(sums, got)


def test_restated_correspondences_are_ckdtrees():
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(5)
    tgt = rng.random((4000, 3))
    src = rng.random((3000, 3)) * 1.2 - 0.1
    j, d2 = ir.nearest(src, tgt)
    dist, idx = cKDTree(tgt).query(src)
    assert np.array_equal(j, idx)
    assert same_bytes(np.sqrt(d2), dist)


def test_reflection_case():
    """a planar cloud: H has rank 2 and the sign of the third singular pair is free, so the plain V U^T is a reflection for one of the
    two in-plane motions below (a mirror image, a proper rotation); the d = -1 branch must repair it"""
    from pb3d import best_fit_transform_from_sums
    rng = np.random.default_rng(11)
    P = np.zeros((200, 3))
    P[:, :2] = rng.normal(size=(200, 2)) * (2.0, 0.7)
    zero = np.zeros(3)
    branch = 0
    for A in (np.diag([-1.0, 1.0, 1.0]), ir.rotation((0.0, 0.0, 1.0), 33.0)):
        Q = P @ A.T + (0.5, -0.25, 0.0)
        t = np.empty((len(P), 16))
        t[:, 0:3], t[:, 3:6] = P, Q
        t[:, 6:15] = (P[:, :, None] * Q[:, None, :]).reshape(-1, 9)
        t[:, 15] = 0.0
        sums = ir.ordered_sum(t)
        H = sums[6:15].reshape(3, 3) - np.outer(sums[0:3], sums[3:6]) / len(P)
        Us, _, Vt = np.linalg.svd(H)
        branch += np.linalg.det(Vt.T @ Us.T) < 0
        M = best_fit_transform_from_sums(len(P), sums, zero, zero)
        R = M[:3, :3]
        assert abs(np.linalg.det(R) - 1.0) <= 1e-14
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-14
        assert np.array_equal(M[3], (0.0, 0.0, 0.0, 1.0))
        assert np.abs(P @ R.T + M[:3, 3] - Q).max() <= 1e-12       # the planar points land on their partners either way
    assert branch >= 1


RECOVERY = [(5.0, "float64", None), (5.0, "float32", None), (10.0, "float64", None), (5.0, "float64", 0.1)]


@pytest.mark.parametrize("degrees,dtype_name,gate", RECOVERY)
def test_restated_loop_recovers_a_known_motion(degrees, dtype_name, gate):
    """A plain cKDTree ICP of the 5-degree case converges in 15 iterations with max|R - R0| = 1.5e-15 on float64 clouds and 5e-10 on
    clouds rounded to float32; asserted three and two orders above that"""
    s, t, M, extent, T, hist, Ts = restated_alignment(degrees, dtype_name, gate)
    assert s.dtype == np.dtype(dtype_name) and len(s) == 1500 and len(t) == 3000
    err = np.abs(T[:3, :3] - M[:3, :3]).max()
    print(f"{degrees} deg {dtype_name} gate {gate}: {len(hist)} iterations, max|R - R0| = {err:.3e}, rmse {hist[-1][1]:.3e}")
    assert len(hist) <= 30 and len(hist) == len(Ts)
    assert err <= (1e-12 if dtype_name == "float64" else 1e-7)
    assert hist[-1][0] == 1500
    assert np.array_equal(T[3], (0.0, 0.0, 0.0, 1.0))


# ---- CPU: argument checks (no device is touched before they run) -----------------------------------------------------------------------
def test_exports():
    import pb3d
    from pb3d import preprocess_helpers as ph
    for n in ("icp_align", "icp_align_resident", "transform_points", "transform_points_resident", "best_fit_transform_from_sums"):
        assert n in ph.__all__ and getattr(pb3d, n) is getattr(ph, n)
    for n in ("pb3d_transform_points_resident", "pb3d_icp_index_resident", "pb3d_icp_step_resident"):
        assert n in pb3d._lib.EXPORTED_SYMBOLS


def test_argument_checks():
    import pb3d
    rng = np.random.default_rng(2)
    ok = rng.random((10, 3))
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        pb3d.icp_align(rng.random((10, 2)), ok)
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        pb3d.icp_align(ok, rng.random(30))
    with pytest.raises(TypeError, match="unsupported dtype"):
        pb3d.icp_align(ok.astype(np.complex128), ok)
    with pytest.raises(TypeError, match="unsupported dtype"):
        pb3d.transform_points(ok.astype(str), np.eye(4))
    for bad in (np.eye(3), np.zeros((4, 3)), np.zeros(12), np.eye(4)[None]):
        with pytest.raises(ValueError, match="3 x 4 or 4 x 4"):
            pb3d.transform_points(ok, bad)
        with pytest.raises(ValueError, match="3 x 4 or 4 x 4"):
            pb3d.icp_align(ok, ok, init=bad)
    with pytest.raises(ValueError, match="last row"):
        pb3d.transform_points(ok, np.full((4, 4), 0.5))
    with pytest.raises(ValueError, match="NaN or infinity"):
        pb3d.transform_points(ok, np.full((3, 4), np.nan))
    nan = ok.copy()
    nan[3, 1] = np.nan
    inf = ok.astype(np.float32)
    inf[0, 0] = np.inf
    for s, t in ((nan, ok), (ok, nan), (inf, ok), (ok, inf)):
        with pytest.raises(ValueError, match="NaN or infinity"):
            pb3d.icp_align(s, t)
    with pytest.raises(ValueError, match="target cloud is empty"):
        pb3d.icp_align(ok, np.zeros((0, 3)))
    with pytest.raises(ValueError, match="at least 3 point pairs"):
        pb3d.icp_align(ok[:2], ok)
    for kw in ({"max_iterations": 0}, {"max_iterations": 2.5}, {"tolerance": -1.0}, {"tolerance": float("nan")}, {"max_distance": -0.1},
               {"max_distance": float("inf")}):
        with pytest.raises(ValueError):
            pb3d.icp_align(ok, ok, **kw)
    assert pb3d.transform_points(np.zeros((0, 3), np.float32), np.eye(4)).shape == (0, 3)
    with pytest.raises(ValueError, match="at least 3 point pairs"):
        pb3d.best_fit_transform_from_sums(2, np.zeros(16), np.zeros(3), np.zeros(3))
    # the restated loop on a gate nothing passes
    with pytest.raises(ValueError, match="only 0 point pairs"):
        ir.icp_align(ok + 100.0, ok, max_distance=1.0)


def test_cabi_argument_checks():
    """the entries refuse bad counts and null arguments before they look at the context"""
    import pb3d
    L = pb3d._lib
    lib = L.load()
    T = np.eye(4)[:3].reshape(12).copy()
    z = np.zeros(3)
    out = np.zeros(17)
    one = C.c_void_p(out.ctypes.data)       # never dereferenced: every call below is refused first

    def refused(rc, text):
        assert rc == -1 and text in lib.pb3d_last_error().decode(), (rc, lib.pb3d_last_error())

    refused(lib.pb3d_icp_step_resident(None, one, 1, 5, one, 1, 0, L.p_dbl(T), -1.0, L.p_dbl(z), L.p_dbl(z), one), "the target is empty")
    refused(lib.pb3d_icp_step_resident(None, one, 1, -1, one, 1, 4, L.p_dbl(T), -1.0, L.p_dbl(z), L.p_dbl(z), one), "negative point count")
    refused(lib.pb3d_icp_step_resident(None, one, 1, 1 << 31, one, 1, 4, L.p_dbl(T), -1.0, L.p_dbl(z), L.p_dbl(z), one), "2^31 - 1")
    refused(lib.pb3d_icp_step_resident(None, one, 1, 5, one, 1, 4, L.p_dbl(T), float("nan"), L.p_dbl(z), L.p_dbl(z), one), "NaN")
    refused(lib.pb3d_icp_step_resident(None, one, 1, 5, one, 1, 4, None, -1.0, L.p_dbl(z), L.p_dbl(z), one), "null argument")
    refused(lib.pb3d_icp_step_resident(None, None, 1, 5, one, 1, 4, L.p_dbl(T), -1.0, L.p_dbl(z), L.p_dbl(z), one), "null buffer")
    refused(lib.pb3d_icp_step_resident(None, one, 1, 5, one, 1, 4, L.p_dbl(T), -1.0, L.p_dbl(z), L.p_dbl(z), one), "null context")
    refused(lib.pb3d_icp_index_resident(None, one, 1, 0, None), "1 <= nt")
    refused(lib.pb3d_icp_index_resident(None, None, 1, 5, None), "null buffer")
    refused(lib.pb3d_icp_index_resident(None, one, 1, 5, None), "null context")
    refused(lib.pb3d_transform_points_resident(None, one, 1, -2, L.p_dbl(T), one), "0 <= n")
    refused(lib.pb3d_transform_points_resident(None, one, 1, 2, None, one), "null transform")
    refused(lib.pb3d_transform_points_resident(None, one, 1, 2, L.p_dbl(T), None), "null buffer")
    refused(lib.pb3d_transform_points_resident(None, one, 1, 2, L.p_dbl(T), one), "null context")
    assert lib.pb3d_transform_points_resident(None, None, 1, 0, L.p_dbl(T), None) == 0        # n = 0: nothing to do


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
class Clouds:
    """source / target uploaded once; step() runs the device step and returns (count, sums)"""

    def __init__(self, pb3d, src, tgt, index=True):
        from pb3d.eval_helpers import _cloud
        self.pb3d, self.ph = pb3d, pb3d.preprocess_helpers
        self.src, self.sf = _cloud(src, "source")
        self.tgt, self.tf = _cloud(tgt, "target")
        self.d_s = pb3d.device.from_numpy(self.src) if len(self.src) else pb3d.device.DeviceBuffer(8)
        self.d_t = pb3d.device.from_numpy(self.tgt) if len(self.tgt) else pb3d.device.DeviceBuffer(8)
        self.box = self.index() if index else None

    def index(self):
        return self.ph.icp_index_resident(self.d_t, len(self.tgt), self.tf)

    def step(self, T, max_dist2, cp, cq):
        d_out = self.ph.icp_step_resident(self.d_s, len(self.src), self.d_t, len(self.tgt), T, max_dist2, cp, cq, self.sf, self.tf)
        try:
            raw = d_out.download((17,), np.float64)
        finally:
            d_out.free()
        return int(raw[:1].view(np.int64)[0]), raw[1:].copy()

    def free(self):
        self.d_s.free()
        self.d_t.free()


def check_step(pb3d, src, tgt, T, max_dist2, cp, cq, what):
    c = Clouds(pb3d, src, tgt)
    try:
        got = c.step(T, max_dist2, cp, cq)
    finally:
        c.free()
    want = ir.step(src, tgt, T, max_dist2, cp, cq)
    assert got[0] == want[0], (what, got[0], want[0])
    assert same_bytes(got[1], want[1]), (what, got[1], want[1])
    return got


@gpu
@pytest.mark.parametrize("sdt,tdt", [("float64", "float64"), ("float64", "float32"), ("float32", "float64"), ("float32", "float32")])
def test_step_sums_and_counts_by_point_count(pb3d_gpu, sdt, tdt):
    """65 537 = 256 workgroups of 256 and one point: the last pass takes a second partial row in thread 0"""
    rng = np.random.default_rng(17)
    T = np.eye(4)
    c = np.zeros(3)
    for nt in (1, 2, 500):
        tgt = (rng.normal(size=(nt, 3)) * (1.0, 0.5, 0.25)).astype(tdt)
        for ns in (1, 63, 64, 65, 255, 256, 257, 1000, 65537):
            src = (rng.normal(size=(ns, 3)) * (1.1, 0.6, 0.3)).astype(sdt)
            count, _ = check_step(pb3d_gpu, src, tgt, T, -1.0, c, c, (sdt, tdt, ns, nt))
            assert count == ns


@gpu
def test_step_transform_and_pivots(pb3d_gpu):
    rng = np.random.default_rng(23)
    src = rng.normal(size=(777, 3)) * (2.0, 1.0, 0.5) + (3.0, -1.0, 7.0)
    tgt = rng.normal(size=(400, 3)) * (2.0, 1.0, 0.5) + (3.1, -0.9, 7.2)
    T = np.eye(4)
    T[:3, :3] = ir.rotation((0.3, -1.0, 0.2), 7.0)          # inexact entries
    T[:3, 3] = (0.1, -1.0 / 3.0, math.pi / 50)
    cp, cq = np.array([2.9, -1.1, 6.7]), np.array([3.3, -0.7, 7.1])
    for md2 in (-1.0, 1.0 / 3.0):
        count, _ = check_step(pb3d_gpu, src, tgt, T, md2, cp, cq, ("pivots", md2))
        assert (count == 777) == (md2 < 0) and count > 100
    check_step(pb3d_gpu, src.astype(np.float32), tgt.astype(np.float32), T, 0.3, cp, cq, "pivots float32")


@gpu
def test_gate(pb3d_gpu):
    """integer lattices: source point (3, 4, 0) is exactly 5 from its nearest target (0, 0, 0); every other source point sits on a target"""
    tgt = np.array([[x, y, z] for x in (0, 20, 40) for y in (0, 20) for z in (0, 20)], np.float64)
    src = np.concatenate([tgt[1:8], [[3.0, 4.0, 0.0]]])
    T, c = np.eye(4), np.array([20.0, 10.0, 10.0])
    at5 = check_step(pb3d_gpu, src, tgt, T, 5.0 * 5.0, c, c, "gate at 5")
    assert at5[0] == 8 and at5[1][15] == 25.0
    below = float(np.nextafter(5.0, 0.0))
    under = check_step(pb3d_gpu, src, tgt, T, below * below, c, c, "gate just under 5")
    assert under[0] == 7 and under[1][15] == 0.0
    # a gate that rejects everything: count 0, every sum +0.0 (sign bit included), and the alignment refuses
    far = src + (7.0, 0.0, 0.0)
    none = check_step(pb3d_gpu, far, tgt, T, 1.0, c, c, "gate rejects all")
    assert none[0] == 0 and not none[1].view(np.uint64).any()
    with pytest.raises(ValueError, match="only 0 point pairs"):
        pb3d_gpu.icp_align(far, tgt, max_distance=1.0)
    # an empty source needs no index and gives zeros
    empty = check_step(pb3d_gpu, np.zeros((0, 3)), tgt, T, -1.0, c, c, "empty source")
    assert empty[0] == 0 and not empty[1].view(np.uint64).any()


@gpu
def test_ties_go_to_the_lowest_index(pb3d_gpu):
    c = np.zeros(3)
    # a query equidistant from two targets (and from four): Q = q_j - 0 names the winner
    tgt = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0], [9.0, 9.0, 9.0]])
    for order in ([0, 1, 2, 3, 4], [1, 0, 3, 2, 4], [4, 3, 2, 1, 0]):
        t = tgt[order]
        src = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.5], [4.0, 4.0, 4.0]])
        for k, s in enumerate(src):
            j, _, _ = ir.pairs(s[None], t, np.eye(4), -1.0, c, c)
            count, sums = check_step(pb3d_gpu, s[None], t, np.eye(4), -1.0, c, c, ("tie", order, k))
            assert count == 1 and same_bytes(sums[3:6], t[j[0]])
            if k < 2:
                assert j[0] == min(i for i in range(5) if np.abs(t[i]).sum() == 1.0)
    # duplicated target rows: every copy ties at the same d2, the first copy wins
    rng = np.random.default_rng(3)
    base = rng.integers(-5, 6, (40, 3)).astype(np.float64)
    t = np.concatenate([base, base[::-1], base])
    src = base + rng.normal(size=base.shape) * 0.01
    j, _, _ = ir.pairs(src, t, np.eye(4), -1.0, c, c)
    assert (j < 40).all()
    check_step(pb3d_gpu, src, t, np.eye(4), -1.0, c, c, "duplicates")
    check_step(pb3d_gpu, src.astype(np.float32), t.astype(np.float32), np.eye(4), -1.0, c, c, "duplicates float32")


@gpu
def test_determinism_and_index_reuse(pb3d_gpu):
    rng = np.random.default_rng(31)
    src = rng.normal(size=(5000, 3))
    tgt = rng.normal(size=(3000, 3))
    other = rng.normal(size=(700, 3))
    T = np.eye(4)
    T[:3, :3] = ir.rotation((1.0, 1.0, 0.0), 3.0)
    cc = np.array([0.1, 0.2, 0.3])
    a = Clouds(pb3d_gpu, src, tgt)
    b = Clouds(pb3d_gpu, src, other, index=False)
    try:
        assert np.array_equal(a.box, np.concatenate([tgt.min(0), tgt.max(0)]))
        first = a.step(T, 0.5, cc, cc)
        again = a.step(T, 0.5, cc, cc)
        assert first[0] == again[0] and same_bytes(first[1], again[1])
        # an unrelated search in between uses slots of its own: the index is still there and the step's bytes do not change
        pb3d_gpu.nn_distances(other, src[:900])
        pb3d_gpu.knn(other, other, 3)
        third = a.step(T, 0.5, cc, cc)
        assert first[0] == third[0] and same_bytes(first[1], third[1])
        want = ir.step(src, tgt, T, 0.5, cc, cc)
        assert first[0] == want[0] and same_bytes(first[1], want[1])
        # a step against a target the index was not built for is refused, never rebuilt behind the caller's back
        with pytest.raises(ValueError, match="built for another target"):
            b.step(T, 0.5, cc, cc)
        with pytest.raises(ValueError, match="built for another target"):       # same pointer, another count
            a.ph.icp_step_resident(a.d_s, len(src), a.d_t, len(tgt) - 1, T, 0.5, cc, cc)
        with pytest.raises(ValueError, match="built for another target"):       # same pointer, another width
            a.ph.icp_step_resident(a.d_s, len(src), a.d_t, len(tgt), T, 0.5, cc, cc, True, False)
        b.index()                                                               # an explicit rebuild for the other target ...
        got = b.step(T, 0.5, cc, cc)
        want_b = ir.step(src, other, T, 0.5, cc, cc)
        assert got[0] == want_b[0] and same_bytes(got[1], want_b[1])
        with pytest.raises(ValueError, match="built for another target"):       # ... retires the first
            a.step(T, 0.5, cc, cc)
        a.index()
        back = a.step(T, 0.5, cc, cc)
        assert first[0] == back[0] and same_bytes(first[1], back[1])
    finally:
        a.free()
        b.free()


@gpu
def test_transform_points(pb3d_gpu):
    rng = np.random.default_rng(41)
    T4 = np.eye(4)
    T4[:3, :3] = ir.rotation((0.2, 0.9, -0.4), 123.0) * 1.0000001
    T4[:3, 3] = (1.0 / 3.0, -2.5, 1e3)
    for dt in (np.float32, np.float64):
        for n in (0, 1, 257):
            P = (rng.normal(size=(n, 3)) * (10.0, 1.0, 0.1)).astype(dt)
            for T in (T4, T4[:3]):
                got = pb3d_gpu.transform_points(P, T)
                assert got.dtype == np.float64 and same_bytes(got, ir.transform(P, T[:3])), (dt, n, T.shape)
    ints = rng.integers(-9, 10, (33, 3))
    assert same_bytes(pb3d_gpu.transform_points(ints, T4), ir.transform(ints, T4[:3]))


def check_alignment(pb3d, src, tgt, want, **kw):
    T, hist, Ts = pb3d.icp_align(src, tgt, return_history=True, **kw)
    wT, whist, wTs = want
    assert len(hist) == len(whist) and len(Ts) == len(wTs)
    for i, ((c, r), (wc, wr)) in enumerate(zip(hist, whist)):
        assert c == wc and same_bytes([r], [wr]), (i, c, wc, r, wr)
    for i, (a, b) in enumerate(zip(Ts, wTs)):
        assert same_bytes(a, b), (i, a, b)
    assert same_bytes(T, wT) and same_bytes(T, Ts[-1])
    assert same_bytes(pb3d.icp_align(src, tgt, **kw), wT)       # without the history: the matrix alone
    return T, hist


@gpu
@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
def test_alignment_synthetic(pb3d_gpu, dtype_name):
    s, t, M, extent, wT, whist, wTs = restated_alignment(5.0, dtype_name, None)
    T, hist = check_alignment(pb3d_gpu, s, t, (wT, whist, wTs))
    assert len(hist) <= 30
    assert np.abs(T[:3, :3] - M[:3, :3]).max() <= (1e-12 if dtype_name == "float64" else 1e-7)
    # the same through the resident entry, with a gate, an initial guess and an iteration limit
    init = ir.motion(4.0, extent)
    want = ir.icp_align(s, t, max_iterations=4, max_distance=0.1 * extent, init=init)
    check_alignment(pb3d_gpu, s, t, want, max_iterations=4, max_distance=0.1 * extent, init=init[:3])


@gpu
def test_alignment_real_cloud(pb3d_gpu):
    """the first four iterations only: the brute-force restatement costs a second per iteration on 5 000 x 20 000 points (the whole
    alignment takes 34), and four already cut the rmse from 0.28 to 0.15"""
    with np.load(os.path.join(GOLDEN, "inter_sfm20k.npz"), allow_pickle=False) as z:
        tgt = np.ascontiguousarray(z["sfm"])
    extent = float((tgt.max(0) - tgt.min(0)).max())
    M = ir.motion(5.0, extent)
    pick = np.sort(np.random.default_rng(7).choice(len(tgt), 5000, replace=False))
    src = np.ascontiguousarray(ir.moved_back(tgt[pick], M))
    want = ir.icp_align(src, tgt, max_iterations=4)
    T, hist = check_alignment(pb3d_gpu, src, tgt, want, max_iterations=4)
    before = pb3d_gpu.chamfer_distance(src, tgt)
    after = pb3d_gpu.chamfer_distance(pb3d_gpu.transform_points(src, T), tgt)
    print(f"real cloud: {len(hist)} iterations, rmse {hist[0][1]:.4e} -> {hist[-1][1]:.4e}, chamfer {before:.4e} -> {after:.4e}")
    assert after < before
