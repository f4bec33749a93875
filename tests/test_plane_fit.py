"""fit_plane_ransac / crop_to_box / symmetric_completion (pb3d/preprocess_helpers.py on csrc/plane.hip): steps 2-4 of the inter-method
preprocessing with the cloud resident on the device.

There is no upstream text to be exact against, so the chain of evidence is the one of tests/test_icp.py: include/pb3d.h states the
arithmetic; tests/plane_restate.py restates it in NumPy from the header; the CPU tests below pin the restatement (its sums against
exact sums with a bound that follows from the float width, its hypotheses against np.cross, its loop against a plane it must recover
and against the stored SfM cloud); the GPU tests demand the restatement's BYTES and integers from the device."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

import icp_restate as ir
import plane_restate as pr

gpu = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -53
NAN_BITS = np.uint64(0x7FF8000000000000)


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def bits_one_nan(a):
    """the bit patterns of a float64 array with every NaN mapped to one pattern"""
    a = np.ascontiguousarray(a, np.float64)
    out = a.view(np.uint64).copy()
    out[np.isnan(a)] = NAN_BITS
    return out


def sfm_cloud(dtype_name):
    with np.load(os.path.join(GOLDEN, "inter_sfm20k.npz"), allow_pickle=False) as z:
        return np.ascontiguousarray(z["sfm"].astype(dtype_name))


@functools.lru_cache(maxsize=None)
def restated_fit(case, dtype_name):
    """one restated fit per case, shared by the CPU and the GPU tests (read-only): (points, tau, K, result of pr.fit)"""
    if case == "slab":
        P, tau, K = pr.slab_case(np.dtype(dtype_name).type), 0.01, 256
    else:
        P = sfm_cloud(dtype_name)
        lo, hi = P.min(0).astype(np.float64), P.max(0).astype(np.float64)
        tau, K = 0.01 * float((hi - lo).max()), 1024
    P.setflags(write=False)
    return P, tau, K, pr.fit(P, tau, K=K, seed=0, refits=2)


# ---- CPU: the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 257, 5000, 65537])
def test_restated_moments_against_exact_sums(n):
    """any summation order of n terms errs by at most n * 2^-53 * sum|term| (the argument of
    test_icp.test_restated_sums_against_exact_sums): derived, not measured"""
    rng = np.random.default_rng(n)
    P = rng.normal(size=(n, 3)) * (3.0, 1.0, 0.2) + (10.0, -4.0, 0.5)
    plane = (0.1, -0.05, 0.99, -1.695)                      # passes through the cloud's centre (10, -4, 0.5)
    pivot = np.array([9.5, -4.25, 0.4])
    used, t = pr.moment_terms(P, plane, 0.25, pivot)
    assert n < 255 or 0 < used.sum() < n                     # the threshold drops some points of the larger clouds
    got = ir.ordered_sum(t)
    for c in range(11):
        exact = math.fsum(t[:, c].tolist())
        bound = n * U * math.fsum(np.abs(t[:, c]).tolist())
        print(f"n={n} term {c}: |restated - exact| = {abs(got[c] - exact):.3e}, bound {bound:.3e}")
        assert abs(got[c] - exact) <= bound, (n, c)
    count, sums = pr.moments(P, plane, 0.25, pivot)
    assert count == int(used.sum()) and same_bytes(sums, got)


def hypothesis_case(n=500, K=300, dtype=np.float64, seed=3):
    """(points, triplets, rows that must be NaN): points 0..2 are an exactly collinear integer triplet; rows 0..5 of the triplets are
    a repeated index (three ways), the collinear triplet and two out-of-range indices; the rest are random (some repeat an index)"""
    rng = np.random.default_rng(seed)
    P = rng.normal(size=(n, 3)) * (2.0, 1.0, 0.5) + (1.0, -2.0, 3.0)
    P[0], P[1], P[2] = (1.0, 2.0, 3.0), (3.0, 5.0, 7.0), (7.0, 11.0, 15.0)        # b - a = (2, 3, 4), c - a = 3 (b - a)
    P = np.ascontiguousarray(P.astype(dtype))
    t = rng.integers(0, n, size=(K, 3), dtype=np.int64)
    special = np.array([[5, 5, 9], [5, 9, 5], [9, 5, 5], [0, 1, 2], [3, n, 4], [-1, 3, 4]], np.int64)[:K]
    t[:len(special)] = special
    if K > 10:
        t[10] = (2, 0, 1)                                                          # the collinear points in another order
    rep = (t[:, 0] == t[:, 1]) | (t[:, 0] == t[:, 2]) | (t[:, 1] == t[:, 2])
    col = np.array([sorted(r.tolist()) == [0, 1, 2] for r in t])
    oob = ((t < 0) | (t >= n)).any(1)
    return P, t, rep | col | oob


def test_restated_hypotheses_against_cross_and_norm():
    """the finite rows against np.cross / np.linalg.norm: the two differ only in how |w| is summed and rounded (relative 2 * 2^-53 on
    L), so 4 * 2^-53 absolute on a unit normal's components and 8 * 2^-53 * sum|n_i a_i| on d"""
    for dtype in (np.float64, np.float32):
        P, t, must_nan = hypothesis_case(dtype=dtype)
        got = pr.hypotheses(P, t)
        nan_rows = np.isnan(got).any(1)
        assert np.array_equal(nan_rows, must_nan) and must_nan.sum() >= 7
        assert np.isnan(got[nan_rows]).all()
        p = P.astype(np.float64)
        for k in np.flatnonzero(~nan_rows):
            a, b, c = p[t[k]]
            w = np.cross(b - a, c - a)
            nrm = w / np.linalg.norm(w)
            assert np.abs(got[k, :3] - nrm).max() <= 4 * U, k
            assert abs(got[k, 3] + nrm @ a) <= 8 * U * np.abs(nrm * a).sum(), k
            assert abs(np.linalg.norm(got[k, :3]) - 1.0) <= 4 * U


def test_plane_from_moments():
    import pb3d
    # exact integer-coordinate points of the plane 2x - y + 2z = 6 (normal (2, -1, 2) / 3): every sum is an exact integer
    g = np.array([[x, y] for x in range(-6, 7, 2) for y in range(-4, 5, 2)], np.float64)
    P = np.stack([g[:, 0], g[:, 1] + 2 * g[:, 0], 3.0 - g[:, 0] + 0.5 * (g[:, 1] + 2 * g[:, 0])], axis=1)
    assert np.array_equal(P, np.round(P)) and np.array_equal(2 * P[:, 0] - P[:, 1] + 2 * P[:, 2], np.full(len(P), 6.0))
    pivot = np.array([1.0, -2.0, 3.0])
    count, sums = pr.moments(P, (0.0, 0.0, 0.0, 0.0), 1.0, pivot)       # the zero "plane": every point is an inlier
    assert count == len(P)
    nrm, d, ev = pb3d.plane_from_moments(count, sums, pivot)
    want = np.array([2.0, -1.0, 2.0]) / 3.0
    print(f"normal error {np.abs(nrm - want).max():.3e}, d error {abs(d + 2.0):.3e}, eigenvalues {ev}")
    assert np.abs(nrm - want).max() <= 1e-14 and abs(d + 2.0) <= 1e-13
    assert ev.shape == (3,) and abs(ev[0]) <= 1e-12 * ev[2] and ev[0] <= ev[1] <= ev[2]
    # the sign rule where the two largest components tie: the planes x + y = 0 and x - y = 0 have the normals +-(1, +-1, 0) / sqrt 2
    zero = np.zeros(3)
    for s in (1.0, -1.0):
        Q = np.array([[x, -s * x, z] for x in range(-3, 4) for z in range(-2, 3)], np.float64)
        c2, s2 = pr.moments(Q, (0.0, 0.0, 0.0, 0.0), 1.0, zero)
        n2, d2, _ = pb3d.plane_from_moments(c2, s2, zero)
        assert np.abs(np.abs(n2) - np.array([1.0, 1.0, 0.0]) / math.sqrt(2.0)).max() <= 1e-14 and abs(d2) <= 1e-14
        assert n2[int(np.argmax(np.abs(n2)))] > 0.0 and n2[0] * n2[1] * s > 0.0
        if abs(n2[0]) == abs(n2[1]):                            # an exact tie: the lowest axis is the positive one
            assert n2[0] > 0.0
    with pytest.raises(ValueError, match="at least 3 points"):
        pb3d.plane_from_moments(2, np.zeros(11), zero)


def test_plane_alignment_transform():
    import pb3d
    rng = np.random.default_rng(4)
    normals = [pr.SLAB_NORMAL, np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0]), np.array([0.6, 0.0, -0.8]), np.array([0.0, 0.0, -1.0]),
               np.array([1e-9, 0.0, -1.0])] + [v / np.linalg.norm(v) for v in rng.normal(size=(20, 3))]
    for nrm in normals:
        nrm = nrm / np.linalg.norm(nrm)
        M = pb3d.plane_alignment_transform(nrm, 0.75)
        R = M[:3, :3]
        assert M.dtype == np.float64 and M.shape == (4, 4) and np.array_equal(M[3], (0.0, 0.0, 0.0, 1.0))
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(R) - 1.0) <= 1e-14, nrm
        assert np.abs(R @ nrm - (0.0, 0.0, 1.0)).max() <= 1e-15, (nrm, R @ nrm)
        assert M[0, 3] == 0.0 and M[1, 3] == 0.0 and abs(M[2, 3] - 0.75) <= 2 * U       # d / |normal|, |normal| = 1 to an ulp
    assert np.array_equal(pb3d.plane_alignment_transform((0.0, 0.0, -1.0), 2.0)[:3], [[1, 0, 0, 0], [0, -1, 0, 0], [0, 0, -1, 2.0]])
    assert np.array_equal(pb3d.plane_alignment_transform((0.0, 0.0, 2.0), 3.0), np.array([[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 1.5], [0, 0, 0, 1]]))
    with pytest.raises(ValueError):
        pb3d.plane_alignment_transform((0.0, 0.0, 0.0), 1.0)


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
def test_restated_fit_recovers_a_known_plane(dtype_name):
    """3000 points of a slab (normal ~ (0.2, -0.1, 0.97), offset 0.3, thickness sigma 0.002, extent +-1) among 2000 uniform outliers,
    K = 256, tau = 0.01.  A NumPy run gave an angle error of 0.0043 degrees and an offset error of 4e-5 (sigma / (spread sqrt M) gives
    0.0036 degrees); asserted at ten times those.  Four hypotheses tie for the best count, so the case pins the tie rule too."""
    P, tau, K, (nrm, d, count, h) = restated_fit("slab", dtype_name)
    assert P.dtype == np.dtype(dtype_name) and len(P) == 5000 and K == 256 and len(h["refits"]) == 2
    angle = math.degrees(math.acos(min(1.0, abs(float(nrm @ pr.SLAB_NORMAL)))))
    off = abs(d * np.sign(nrm @ pr.SLAB_NORMAL) - pr.SLAB_OFFSET)
    tied = np.flatnonzero(h["counts"] == h["counts"].max())
    print(f"{dtype_name}: angle error {angle:.4f} deg, offset error {off:.2e}, {count} inliers, best {h['best']} of the tied {tied.tolist()}")
    assert angle <= 0.043 and off <= 4e-4
    assert len(tied) >= 2 and h["best"] == tied[0]
    assert 2900 <= count <= 3200
    assert nrm[int(np.argmax(np.abs(nrm)))] > 0.0 and abs(np.linalg.norm(nrm) - 1.0) <= 4 * U


def test_restated_fit_ties_go_to_the_lowest_hypothesis():
    """every point on one plane: each non-degenerate hypothesis counts all of them, the first such row wins"""
    g = np.array([[x, y, 5.0] for x in range(8) for y in range(8)], np.float64)
    nrm, d, count, h = pr.fit(g, 0.0, K=64, seed=1, refits=1)
    finite = np.flatnonzero(~np.isnan(h["planes"][:, 0]))
    assert 0 < len(finite) < 64 and (h["counts"][finite] == 64).all() and h["best"] == finite[0] and count == 64
    assert np.abs(np.abs(nrm) - (0.0, 0.0, 1.0)).max() <= 1e-15 and abs(abs(d) - 5.0) <= 1e-14


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
def test_restated_fit_on_the_stored_sfm_cloud(dtype_name):
    """tests/golden/inter_sfm20k.npz, tau = 1 % of the extent, K = 1024, seed 0: the restated fit gives the normal
    (0.0237, 0.1572, 0.9873) with 6383 inliers, 31.9 % of the 20 000 points (float32 rows: the same to the digits shown); the whole
    52 032-point cloud gave z = 0.987 and 32 %"""
    P, tau, K, (nrm, d, count, h) = restated_fit("sfm", dtype_name)
    print(f"{dtype_name}: normal {nrm}, d {d:.6f}, {count} inliers = {count / len(P):.4f}, best hypothesis {h['best']} with {h['counts'][h['best']]}")
    assert len(P) == 20000 and nrm[2] > 0.95 and 0.2 <= count / len(P) <= 0.45


def test_exports():
    import pb3d
    from pb3d import preprocess_helpers as ph
    for n in ("fit_plane_ransac", "fit_plane_ransac_resident", "plane_from_moments", "plane_alignment_transform", "crop_to_box",
              "crop_to_box_resident", "symmetric_completion", "symmetric_completion_resident", "plane_hypotheses_resident", "plane_score_resident",
              "plane_moments_resident"):
        assert n in ph.__all__ and getattr(pb3d, n) is getattr(ph, n)
    for n in ("pb3d_plane_hypotheses_resident", "pb3d_plane_score_resident", "pb3d_plane_moments_resident", "pb3d_points_crop_box_resident"):
        assert n in pb3d._lib.EXPORTED_SYMBOLS


def test_argument_checks():
    import pb3d
    ok = np.random.default_rng(2).random((10, 3))
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        pb3d.fit_plane_ransac(ok[:, :2], 0.1)
    with pytest.raises(TypeError, match="unsupported dtype"):
        pb3d.fit_plane_ransac(ok.astype(np.complex128), 0.1)
    with pytest.raises(ValueError, match="at least 3 points"):
        pb3d.fit_plane_ransac(ok[:2], 0.1)
    for tau in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="inlier_threshold"):
            pb3d.fit_plane_ransac(ok, tau)
    for K in (0, 4097, 2.5, True):
        with pytest.raises(ValueError, match="num_hypotheses"):
            pb3d.fit_plane_ransac(ok, 0.1, num_hypotheses=K)
    with pytest.raises(ValueError, match="refine_iterations"):
        pb3d.fit_plane_ransac(ok, 0.1, refine_iterations=-1)
    bad = ok.copy()
    bad[4, 2] = np.inf
    with pytest.raises(ValueError, match="NaN or infinity"):
        pb3d.fit_plane_ransac(bad, 0.1)
    with pytest.raises(ValueError, match="NaN or infinity"):
        pb3d.symmetric_completion(bad)
    with pytest.raises(ValueError, match="NaN"):
        pb3d.crop_to_box(ok, (0.0, float("nan"), 0.0), (1.0, 1.0, 1.0))
    assert pb3d.symmetric_completion(np.zeros((0, 3), np.float32)).shape == (0, 3)
    out, idx = pb3d.crop_to_box(np.zeros((0, 3), np.float32), np.zeros(3), np.ones(3), return_index=True)
    assert out.shape == (0, 3) and out.dtype == np.float32 and idx.shape == (0,)


def test_cabi_argument_checks():
    """the entries refuse bad counts, thresholds and null arguments before they look at the context"""
    import pb3d
    L = pb3d._lib
    lib = L.load()
    z3, p4 = np.zeros(3), np.zeros(4)
    buf = np.zeros(64)
    one = C.c_void_p(buf.ctypes.data)       # never dereferenced: every call below is refused first

    def refused(rc, text):
        assert rc == -1 and text in lib.pb3d_last_error().decode(), (rc, lib.pb3d_last_error())

    for K in (0, 4097):
        refused(lib.pb3d_plane_hypotheses_resident(None, one, 1, 5, one, K, one), "1 <= K <= 4096")
        refused(lib.pb3d_plane_score_resident(None, one, 1, 5, one, K, 0.5, one), "1 <= K <= 4096")
    refused(lib.pb3d_plane_hypotheses_resident(None, one, 1, -1, one, 4, one), "0 <= n")
    refused(lib.pb3d_plane_hypotheses_resident(None, one, 1, 1 << 31, one, 4, one), "2^31 - 1")
    refused(lib.pb3d_plane_hypotheses_resident(None, one, 1, 5, None, 4, one), "null buffer")
    refused(lib.pb3d_plane_hypotheses_resident(None, one, 1, 5, one, 4, None), "null buffer")
    refused(lib.pb3d_plane_hypotheses_resident(None, None, 1, 5, one, 4, one), "null buffer")
    refused(lib.pb3d_plane_hypotheses_resident(None, one, 1, 5, one, 4, one), "null context")
    refused(lib.pb3d_plane_score_resident(None, one, 1, -1, one, 4, 0.5, one), "0 <= n")
    for tau in (-0.5, float("nan")):
        refused(lib.pb3d_plane_score_resident(None, one, 1, 5, one, 4, tau, one), "threshold")
        refused(lib.pb3d_plane_moments_resident(None, one, 1, 5, L.p_dbl(p4), tau, L.p_dbl(z3), one), "threshold")
    refused(lib.pb3d_plane_score_resident(None, one, 1, 5, None, 4, 0.5, one), "null buffer")
    refused(lib.pb3d_plane_score_resident(None, one, 1, 5, one, 4, 0.5, None), "null buffer")
    refused(lib.pb3d_plane_score_resident(None, None, 1, 5, one, 4, 0.5, one), "null buffer")
    refused(lib.pb3d_plane_score_resident(None, one, 1, 5, one, 4, 0.5, one), "null context")
    refused(lib.pb3d_plane_moments_resident(None, one, 1, -3, L.p_dbl(p4), 0.5, L.p_dbl(z3), one), "0 <= n")
    refused(lib.pb3d_plane_moments_resident(None, one, 1, 5, None, 0.5, L.p_dbl(z3), one), "null argument")
    refused(lib.pb3d_plane_moments_resident(None, one, 1, 5, L.p_dbl(p4), 0.5, None, one), "null argument")
    refused(lib.pb3d_plane_moments_resident(None, one, 1, 5, L.p_dbl(p4), 0.5, L.p_dbl(z3), None), "null argument")
    refused(lib.pb3d_plane_moments_resident(None, None, 1, 5, L.p_dbl(p4), 0.5, L.p_dbl(z3), one), "null buffer")
    refused(lib.pb3d_plane_moments_resident(None, one, 1, 5, L.p_dbl(p4), 0.5, L.p_dbl(z3), one), "null context")
    refused(lib.pb3d_points_crop_box_resident(None, one, 1, -1, L.p_dbl(z3), L.p_dbl(z3), one, None, one), "0 <= n")
    refused(lib.pb3d_points_crop_box_resident(None, one, 1, 5, None, L.p_dbl(z3), one, None, one), "null argument")
    refused(lib.pb3d_points_crop_box_resident(None, one, 1, 5, L.p_dbl(z3), L.p_dbl(z3), one, None, None), "null argument")
    refused(lib.pb3d_points_crop_box_resident(None, None, 1, 5, L.p_dbl(z3), L.p_dbl(z3), one, None, one), "null buffer")
    refused(lib.pb3d_points_crop_box_resident(None, one, 1, 5, L.p_dbl(z3), L.p_dbl(z3), None, None, one), "null buffer")
    refused(lib.pb3d_points_crop_box_resident(None, one, 1, 5, L.p_dbl(z3), L.p_dbl(z3), one, None, one), "null context")


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
class Cloud:
    """a cloud uploaded once, optionally `shift` elements behind the start of its allocation (an odd element offset)"""

    def __init__(self, pb3d, P, shift=0):
        from pb3d.eval_helpers import _cloud
        self.pb3d, self.ph, self.dev = pb3d, pb3d.preprocess_helpers, pb3d.device
        self.P, self.f64 = _cloud(P, "points")
        self.n = len(self.P)
        off = shift * self.P.dtype.itemsize
        self.buf = self.dev.DeviceBuffer(max(8, self.P.nbytes) + off)
        if self.n:
            self.buf.upload(self.P, off)
        self.ptr = self.buf.at(off)

    def hypotheses(self, triplets):
        K = len(triplets)
        d_t = self.dev.from_numpy(np.ascontiguousarray(triplets, np.int64))
        d_out = self.ph.plane_hypotheses_resident(self.ptr, self.n, d_t, K, self.f64)
        try:
            return d_out.download((K, 4), np.float64)
        finally:
            d_out.free()
            d_t.free()

    def score(self, planes, tau, out=None):
        planes = np.ascontiguousarray(planes, np.float64).reshape(-1, 4)
        d_p = self.dev.from_numpy(planes)
        d_out = self.ph.plane_score_resident(self.ptr, self.n, d_p, len(planes), tau, self.f64, out=out)
        try:
            return d_out.download((len(planes),), np.int64)
        finally:
            if out is None:
                d_out.free()
            d_p.free()

    def moments(self, plane, tau, pivot):
        d_out = self.ph.plane_moments_resident(self.ptr, self.n, plane, tau, pivot, self.f64)
        try:
            raw = d_out.download((12,), np.float64)
        finally:
            d_out.free()
        return int(raw[:1].view(np.int64)[0]), raw[1:].copy()

    def free(self):
        self.buf.free()


@gpu
@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
def test_hypotheses(pb3d_gpu, dtype_name):
    for K in (1, 65, 300):
        P, t, must_nan = hypothesis_case(n=500, K=K, dtype=np.dtype(dtype_name).type, seed=K)
        c = Cloud(pb3d_gpu, P)
        try:
            got = c.hypotheses(t)
        finally:
            c.free()
        want = pr.hypotheses(P, t)
        assert np.array_equal(np.isnan(got).any(1), must_nan) and must_nan[0]
        assert np.array_equal(bits_one_nan(got), bits_one_nan(want)), (dtype_name, K)


def random_planes(P, K, seed):
    """K plane rows through random triplets of the cloud (for n < 3 or repeated indices: NaN rows), the last one NaN on purpose"""
    rng = np.random.default_rng(seed)
    n = len(P)
    planes = pr.hypotheses(P, rng.integers(0, n, size=(K, 3), dtype=np.int64))
    bad = np.isnan(planes[:, 0])
    if bad.any():                                           # fill most degenerate rows with planes through the cloud's centre
        m = ir.widen(P).mean(0)
        v = rng.normal(size=(K, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        fill = np.concatenate([v, -(v @ m)[:, None]], axis=1)
        planes[bad] = fill[bad]
    if K > 1:
        planes[K - 1] = np.nan
    return planes


@gpu
@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
def test_score_by_point_and_plane_count(pb3d_gpu, dtype_name):
    """a cloud with fewer tiles of 1024 points than 8 workgroups per compute unit splits the K rows over the grid's y as well, in
    at most ceil(K / 64) chunks: every K > 64 here runs chunked (4096: 64 chunks of 64; 301: chunks of 61, 61, 61, 61, 57), every
    smaller K in one chunk; test_score_second_tile is the other side, where the tiles alone fill the grid"""
    rng = np.random.default_rng(19)
    for n in (1, 63, 64, 65, 255, 257, 5000):
        P = (rng.normal(size=(n, 3)) * (1.0, 0.5, 0.25)).astype(dtype_name)
        for shift in ((0, 1) if n in (65, 5000) else (0,)):             # 1: the base pointer one element past its allocation
            c = Cloud(pb3d_gpu, P, shift)
            try:
                for K in (1, 7, 64, 4096) + ((301,) if n in (65, 5000) else ()):   # 301: five ragged chunks of plane rows (see below)
                    planes = random_planes(P, K, n + K)
                    got = c.score(planes, 0.2)
                    want = pr.score(P, planes, 0.2)
                    assert np.array_equal(got, want), (dtype_name, n, K, shift)
                    assert K == 1 or (got[K - 1] == 0 and got.max() > 0)
            finally:
                c.free()
    empty = Cloud(pb3d_gpu, np.zeros((0, 3), dtype_name))
    try:
        assert np.array_equal(empty.score(np.ones((5, 4)), 1.0), np.zeros(5, np.int64))
    finally:
        empty.free()


@gpu
@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
def test_score_second_tile(pb3d_gpu, dtype_name):
    """k_plane_score runs min(tiles, 8 * compute units) workgroups of 256 lanes x 4 points: a tile is 1024 points and workgroup b takes
    tiles b, b + grid, ...  With n = 8 * CUs * 1024 + 1024 + 77 there are grid + 2 tiles: workgroups 0 and 1 take a second tile (the
    last one ragged) and add to an LDS table that already holds their first tile's counts."""
    cus = pb3d_gpu.device.device_info()["compute_units"]
    n = 8 * cus * 1024 + 1024 + 77
    rng = np.random.default_rng(23)
    P = (rng.random(size=(n, 3)) * (4.0, 2.0, 1.0)).astype(dtype_name)
    planes = random_planes(P, 16, 5)
    c = Cloud(pb3d_gpu, P)
    try:
        got = c.score(planes, 0.05)
        got7 = c.score(planes[:7], 0.05)
    finally:
        c.free()
    want = pr.score(P, planes, 0.05)
    assert np.array_equal(got, want) and np.array_equal(got7, want[:7])
    assert want[:15].min() > 1000 and want[15] == 0


@gpu
def test_score_boundary_nan_and_overwrite(pb3d_gpu):
    """integer coordinates, plane z = 5, tau = 2: z = 3 and z = 7 count, the next float64 beyond either does not"""
    z = [5.0, 3.0, 7.0, np.nextafter(3.0, -np.inf), np.nextafter(7.0, np.inf), 4.0, 6.0, 2.0, 8.0, np.nan]
    P = np.array([[i, 2 * i, v] for i, v in enumerate(z)], np.float64)
    P[5, 0] = np.nan                                        # a NaN coordinate the plane does not even weigh: 0 * NaN is NaN
    planes = np.array([[0.0, 0.0, 1.0, -5.0], [np.nan] * 4, [0.0, 0.0, 1.0, np.nan], [0.0, 0.0, -1.0, 5.0]])
    c = Cloud(pb3d_gpu, P)
    d_counts = pb3d_gpu.device.DeviceBuffer(4 * 8)
    try:
        d_counts.upload(np.full(4, 12345, np.int64))        # overwritten, not accumulated
        first = c.score(planes, 2.0, out=d_counts)
        again = c.score(planes, 2.0, out=d_counts)
        exact = c.score(planes[:1], 0.0)
    finally:
        d_counts.free()
        c.free()
    assert first.tolist() == [4, 0, 0, 4] and np.array_equal(first, again)     # z = 5, 3, 7, 6 (z = 4 sits in the NaN row)
    assert np.array_equal(first, pr.score(P, planes, 2.0))
    assert exact.tolist() == [1]
    P32 = np.array([[0, 0, 3.0], [0, 0, 7.0], [0, 0, np.nextafter(np.float32(3.0), np.float32(-9))],
                    [0, 0, np.nextafter(np.float32(7.0), np.float32(9))]], np.float32)
    c = Cloud(pb3d_gpu, P32)
    try:
        assert c.score(planes[:1], 2.0).tolist() == [2]
    finally:
        c.free()


@gpu
@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
def test_moments(pb3d_gpu, dtype_name):
    """65 537 = 256 workgroups of 256 and one point: the last pass takes a second partial row in thread 0"""
    plane = (0.1, -0.05, 0.99, -1.695)
    pivot = np.array([9.5, -4.25, 0.4])
    for n in (1, 255, 257, 5000, 65537):
        rng = np.random.default_rng(n)
        P = (rng.normal(size=(n, 3)) * (3.0, 1.0, 0.2) + (10.0, -4.0, 0.5)).astype(dtype_name)
        c = Cloud(pb3d_gpu, P, shift=1 if n == 257 else 0)
        try:
            got = c.moments(plane, 0.25, pivot)
            again = c.moments(plane, 0.25, pivot)
            none = c.moments(plane, 0.0, pivot) if n == 5000 else None
        finally:
            c.free()
        want = pr.moments(P, plane, 0.25, pivot)
        assert got[0] == want[0] and same_bytes(got[1], want[1]), (dtype_name, n, got, want)
        assert again[0] == got[0] and same_bytes(again[1], got[1])
        assert n < 255 or 0 < got[0] < n
        if none is not None:                                # nobody within 0 of an inexact plane: count 0 and eleven +0.0, sign bit included
            assert none[0] == 0 and not none[1].view(np.uint64).any()
    empty = Cloud(pb3d_gpu, np.zeros((0, 3), dtype_name))
    try:
        e = empty.moments(plane, 0.25, pivot)
    finally:
        empty.free()
    assert e[0] == 0 and not e[1].view(np.uint64).any()


def crop_device(pb3d, P, lo, hi, with_index, shift=0):
    """(rows the entry wrote, tail of d_out behind them, index or None, count) with d_out pre-filled with a sentinel"""
    c = Cloud(pb3d, P, shift)
    n, row = c.n, 3 * c.P.dtype.itemsize
    d_out = pb3d.device.DeviceBuffer(n * row)
    d_idx = pb3d.device.DeviceBuffer(n * 4) if with_index else None
    try:
        d_out.upload(np.full(n * row, 0xA5, np.uint8))
        if d_idx is not None:
            d_idx.upload(np.full(n, -7, np.int32))
        _, count = c.ph.crop_to_box_resident(c.ptr, n, lo, hi, c.f64, out=d_out, index=d_idx)
        raw = d_out.download((n * row,), np.uint8)
        idx = d_idx.download((n,), np.int32) if with_index else None
    finally:
        c.free()
        d_out.free()
        if d_idx is not None:
            d_idx.free()
    return raw[:count * row], raw[count * row:], idx, count


@gpu
@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
def test_crop(pb3d_gpu, dtype_name):
    rng = np.random.default_rng(29)
    lo, hi = np.array([-0.5, -0.25, -1.0]), np.array([0.75, 0.5, 0.125])       # exact in float32 too
    for n in (1, 63, 64, 65, 255, 256, 257, 70001):
        P = (rng.normal(size=(n, 3)) * (1.0, 0.5, 0.7)).astype(dtype_name)
        if n >= 63:
            P[3], P[7] = lo, hi                              # on the corners of the closed box: kept
            P[11] = (lo[0], hi[1], 0.0)
            P[13] = (0.0, np.nan, 0.0)                       # inside but for one NaN coordinate: rejected
            P[n - 1] = (0.0, 0.0, 0.0)                       # the last row is kept
        boxes = [("all", np.full(3, -np.inf), np.full(3, np.inf)), ("none", np.full(3, 50.0), np.full(3, 60.0)), ("part", lo, hi),
                 ("empty box", hi, lo)]
        for what, blo, bhi in boxes:
            mask = pr.crop_mask(P, blo, bhi)
            if n >= 63:
                assert not mask[13] and (what != "part" or (mask[3] and mask[7] and mask[11] and mask[n - 1] and 0 < mask.sum() < n))
            for with_index in (True, False):
                rows, tail, idx, count = crop_device(pb3d_gpu, P, blo, bhi, with_index, shift=1 if n == 257 else 0)
                assert count == int(mask.sum()), (dtype_name, n, what, count)
                assert np.array_equal(rows, P[mask].view(np.uint8).reshape(-1)), (dtype_name, n, what)
                assert (tail == 0xA5).all(), (dtype_name, n, what)
                if with_index:
                    assert np.array_equal(idx[:count], np.flatnonzero(mask)) and (idx[count:] == -7).all()
    # the NumPy-signature wrapper
    P = (rng.normal(size=(1000, 3))).astype(dtype_name)
    mask = pr.crop_mask(P, lo, hi)
    out, idx = pb3d_gpu.crop_to_box(P, lo, hi, return_index=True)
    assert out.dtype == P.dtype and np.array_equal(out, P[mask]) and np.array_equal(idx, np.flatnonzero(mask))
    assert np.array_equal(pb3d_gpu.crop_to_box(P, lo, hi), P[mask])
    assert pb3d_gpu.crop_to_box(P, hi, lo).shape == (0, 3)


def check_fit(pb3d, P, tau, K, want):
    nrm, d, count, h = pb3d.fit_plane_ransac(P, tau, num_hypotheses=K, seed=0, refine_iterations=2, return_history=True)
    wn, wd, wcount, wh = want
    assert np.array_equal(h["triplets"], wh["triplets"])
    assert np.array_equal(bits_one_nan(h["planes"]), bits_one_nan(wh["planes"]))
    assert np.array_equal(h["counts"], wh["counts"]) and h["best"] == wh["best"]
    assert len(h["refits"]) == len(wh["refits"]) == 2
    for i, ((c, s, n_, d_), (wc, ws, wn_, wd_)) in enumerate(zip(h["refits"], wh["refits"])):
        assert c == wc and same_bytes(s, ws) and same_bytes(n_, wn_) and same_bytes([d_], [wd_]), (i, c, wc)
    assert same_bytes(nrm, wn) and same_bytes([d], [wd]) and count == wcount
    short = pb3d.fit_plane_ransac(P, tau, num_hypotheses=K, seed=0, refine_iterations=2)
    assert len(short) == 3 and same_bytes(short[0], wn) and same_bytes([short[1]], [wd]) and short[2] == wcount
    return nrm, d, count


@gpu
@pytest.mark.parametrize("case", ["slab", "sfm"])
@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
def test_whole_fit(pb3d_gpu, case, dtype_name):
    P, tau, K, want = restated_fit(case, dtype_name)
    nrm, d, count = check_fit(pb3d_gpu, P, tau, K, want)
    # no refit: the best hypothesis and its count
    n0, d0, c0 = pb3d_gpu.fit_plane_ransac(P, tau, num_hypotheses=K, seed=0, refine_iterations=0)
    h = want[3]
    assert same_bytes(n0, h["planes"][h["best"], :3]) and same_bytes([d0], [h["planes"][h["best"], 3]]) and c0 == h["counts"][h["best"]]
    # alignment: the fitted plane's inliers land within tau of z = 0 (the transform's own rounding: a few ulps of the extent)
    inl = P[pr.inliers(P, (*nrm, d), tau)]
    assert len(inl) == count
    moved = pb3d_gpu.transform_points(inl, pb3d_gpu.plane_alignment_transform(nrm, d))
    extent = float((ir.widen(P).max(0) - ir.widen(P).min(0)).max())
    print(f"{case} {dtype_name}: max |z| of the aligned inliers {np.abs(moved[:, 2]).max():.6e}, tau {tau:.6e}")
    assert np.abs(moved[:, 2]).max() <= tau + 64 * U * extent


@gpu
def test_fit_ties_and_too_few_inliers(pb3d_gpu):
    g = np.array([[x, y, 5.0] for x in range(8) for y in range(8)], np.float64)
    want = pr.fit(g, 0.0, K=64, seed=1, refits=1)
    nrm, d, count, h = pb3d_gpu.fit_plane_ransac(g, 0.0, num_hypotheses=64, seed=1, refine_iterations=1, return_history=True)
    assert h["best"] == want[3]["best"] and np.array_equal(h["counts"], want[3]["counts"]) and count == 64
    assert same_bytes(nrm, want[0]) and same_bytes([d], [want[1]])
    # three copies of one point: every hypothesis is degenerate, the best count is 0
    with pytest.raises(ValueError, match="0 inliers"):
        pb3d_gpu.fit_plane_ransac(np.ones((3, 3)), 0.5, num_hypotheses=8)


@gpu
def test_symmetric_completion(pb3d_gpu):
    rng = np.random.default_rng(37)
    for dtype_name in ("float64", "float32"):
        P = (rng.normal(size=(1000, 3)) * (2.0, 1.0, 0.5) + (3.0, -1.0, 7.0)).astype(dtype_name)
        for centre in (None, (2.5, 7.25)):
            got = pb3d_gpu.symmetric_completion(P, centre)
            assert got.dtype == np.float64 and got.shape == (4000, 3)
            assert same_bytes(got, pr.completion(P, centre)), (dtype_name, centre)
            assert same_bytes(got[:1000], P.astype(np.float64))                # copy 0 is the input
            assert same_bytes(got[:, 1].reshape(4, 1000), np.tile(P[:, 1].astype(np.float64), (4, 1)))
    # small integers: copy 1's rule applied four times gives back the input exactly, and the completed box is symmetric about the centre
    ints = rng.integers(-20, 21, size=(1000, 3)).astype(np.float64)
    centre = (3.0, -4.0)
    got = pb3d_gpu.symmetric_completion(ints, centre)
    assert same_bytes(got, pr.completion(ints, centre))
    q = ints
    for _ in range(4):
        q = pb3d_gpu.symmetric_completion(q, centre)[1000:2000]
    assert np.array_equal(q, ints)
    lo, hi = got.min(0), got.max(0)
    assert lo[0] + hi[0] == 2 * centre[0] and lo[2] + hi[2] == 2 * centre[1]
    assert hi[0] - lo[0] == hi[2] - lo[2]
