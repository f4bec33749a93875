"""Trimmed and scaled icp_align, and the exact k-th selection under it (pb3d/preprocess_helpers.py, pb3d/selection.py on csrc/icp.hip
and csrc/select.hip).

The chain of evidence is the one of tests/test_icp.py: include/pb3d.h states the arithmetic; tests/icp_trim_restate.py restates it in
NumPy on top of icp_restate; the CPU tests pin the restatement (its 17 sums against exact sums with a derived bound, its tau against
np.partition, the similarity solve against transforms it must recover, its loop against a motion and a scale it must recover); the GPU
tests demand the restatement's BYTES from the device -- the selected element, all 20 words of a step, every transform, count, rmse,
candidate count and tau of a whole alignment."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

import icp_restate as ir
import icp_trim_restate as tr

gpu = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -53
QNAN = np.array([0x7FF8000000000000], np.uint64).view(np.float64)[0]


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def case_clouds(name):
    """(source, target, M, extent, scale, kwargs) of the named whole-alignment case"""
    if name == "X":
        return (*tr.clutter_case(), 1.0, {"trim_fraction": 0.75})
    if name == "X untrimmed":
        return (*tr.clutter_case(), 1.0, {})
    scale = float(name.split()[1])
    if name.endswith("clutter"):
        return (*tr.scale_case(scale, clutter=True), {"trim_fraction": 0.75, "with_scale": True})
    return (*tr.scale_case(scale), {"with_scale": True})


@functools.lru_cache(maxsize=None)
def restated_alignment(name):
    """one restated alignment per case, shared by the CPU and the GPU tests (read-only)"""
    s, t, M, extent, scale, kw = case_clouds(name)
    T, hist, Ts = tr.icp_align(s, t, **kw)
    for a in (s, t, M, T, *Ts):
        a.setflags(write=False)
    return s, t, M, scale, kw, T, hist, Ts


def scale_of(T):
    return float(np.cbrt(np.linalg.det(T[:3, :3])))


# ---- CPU: the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 257, 5000, 65537])
def test_restated_sums_against_exact_sums(n):
    """any summation order of n terms errs by at most n * 2^-53 * sum|term| (each of the n - 1 additions adds a relative 2^-53 of a
    partial sum that is itself bounded by sum|term|): derived, not measured -- the bound of test_icp.py, now over 17 sums"""
    rng = np.random.default_rng(n)
    src = rng.normal(size=(n, 3)) * (3.0, 1.0, 0.2) + (10.0, -4.0, 0.5)
    tgt = rng.normal(size=(97, 3)) * (3.0, 1.0, 0.2) + (10.0, -4.0, 0.5)
    T = np.eye(4)
    T[:3, :3] = ir.rotation((0.3, -1.0, 0.2), 7.0)
    T[:3, 3] = (0.1, -0.2, 0.05)
    cp, cq = np.array([9.5, -4.25, 0.4]), np.array([10.25, -3.5, 0.6])
    used, t, m, tau = tr.pairs(src, tgt, T, 2.0, 0.6, cp, cq)
    assert 0 < used.sum() <= m <= n and (n < 255 or used.sum() < m < n)     # the gate and the trim both drop pairs of the larger clouds
    assert used.sum() >= tr.trim_k(m, 0.6)
    got = ir.ordered_sum(t)
    assert got.shape == (17,)
    for c in range(17):
        exact = math.fsum(t[:, c].tolist())
        bound = n * U * math.fsum(np.abs(t[:, c]).tolist())
        print(f"n={n} term {c}: |restated - exact| = {abs(got[c] - exact):.3e}, bound {bound:.3e}")
        assert abs(got[c] - exact) <= bound, (n, c)
    count, sums, m2, tau2 = tr.step(src, tgt, T, 2.0, 0.6, cp, cq)
    assert count == int(used.sum()) and same_bytes(sums, got) and m2 == m and same_bytes([tau2], [tau])
    # with rho = 1 the first 16 sums and the count are the plain step's
    c1, s1, m1, tau1 = tr.step(src, tgt, T, 2.0, 1.0, cp, cq)
    c0, s0 = ir.step(src, tgt, T, 2.0, cp, cq)
    assert c1 == c0 == m1 and same_bytes(s1[:16], s0)


@pytest.mark.parametrize("rho", [1e-9, 1.0 / 3.0, 0.5, 0.75, float(np.nextafter(1.0, 0.0)), 1.0])
def test_restated_tau_against_partition(rho):
    rng = np.random.default_rng(8)
    src = rng.normal(size=(3001, 3))
    tgt = rng.normal(size=(200, 3))
    c = np.zeros(3)
    for md2 in (-1.0, 0.3):
        d2, valid, _ = tr.prepare(src, tgt, np.eye(4), c, c)
        used, t, m, tau = tr.finish((d2, valid, _), md2, rho)
        cand = d2 <= md2 if md2 >= 0 else np.ones(len(d2), bool)
        assert m == cand.sum() and (md2 < 0) == (m == len(src))
        k = m if rho >= 1.0 else min(m, math.ceil(rho * m))
        assert k == tr.trim_k(m, rho) and 1 <= k <= m and (rho > 1e-9 or k == 1) and (rho < 0.9 or k >= m - 1)
        assert tau == np.partition(d2[cand], k - 1)[k - 1]
        assert used.sum() == (d2[cand] <= tau).sum() >= k
        # the totalOrder selection over the keys (sentinels above every candidate) names the same element
        assert same_bytes([tr.kth(tr.keys(d2, cand), k - 1)], [tau])
    # kth on the special values: totalOrder, the element's own bytes
    v = np.array([np.inf, 0.0, -0.0, QNAN, -1.0, 5e-324, -np.inf, 1.0, -5e-324])
    want = [-np.inf, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, np.inf, QNAN]
    for r, w in enumerate(want):
        assert same_bytes([tr.kth(v, r)], [w]), (r, w)


def exact_sums(P, Q, cp, cq):
    t = np.empty((len(P), 17))
    Pc, Qc = P - cp, Q - cq
    t[:, 0:3], t[:, 3:6] = Pc, Qc
    t[:, 6:15] = (Pc[:, :, None] * Qc[:, None, :]).reshape(-1, 9)
    t[:, 15] = 0.0
    t[:, 16] = (Pc * Pc).sum(axis=1)
    return ir.ordered_sum(t)


@pytest.mark.parametrize("s0", [0.5, 1.05, 3.0])
def test_similarity_solve_recovers_exact_correspondences(s0):
    from pb3d import best_fit_similarity_from_sums, best_fit_transform_from_sums
    rng = np.random.default_rng(13)
    P = rng.normal(size=(300, 3)) * (2.0, 0.7, 0.4) + (1.0, -2.0, 0.5)
    R0 = ir.rotation((0.4, -0.2, 1.0), 37.0)
    t0 = np.array([0.5, -0.25, 2.0])
    Q = s0 * (P @ R0.T) + t0
    cp, cq = np.array([0.9, -1.8, 0.4]), np.array([1.2, 0.1, 2.2])
    sums = exact_sums(P, Q, cp, cq)
    M = best_fit_similarity_from_sums(len(P), sums, cp, cq)
    err_s, err_R, err_t = abs(scale_of(M) - s0), np.abs(M[:3, :3] / s0 - R0).max(), np.abs(M[:3, 3] - t0).max()
    print(f"s0={s0}: |s - s0| = {err_s:.3e}, max|A/s0 - R0| = {err_R:.3e}, max|t - t0| = {err_t:.3e}")
    assert err_s <= 1e-12 and err_R <= 1e-12 and err_t <= 1e-12
    assert np.array_equal(M[3], (0.0, 0.0, 0.0, 1.0))
    assert np.abs(P @ M[:3, :3].T + M[:3, 3] - Q).max() <= 1e-12
    # with_scale=False is the rigid solve, byte for byte
    assert same_bytes(best_fit_similarity_from_sums(len(P), sums, cp, cq, with_scale=False),
                      best_fit_transform_from_sums(len(P), sums[:16], cp, cq))


def test_similarity_solve_reflection_case_and_refusals():
    """the planar cloud of test_icp.test_reflection_case, scaled: the d = -1 branch must repair the reflection AND enter the scale"""
    from pb3d import best_fit_similarity_from_sums
    rng = np.random.default_rng(11)
    P = np.zeros((200, 3))
    P[:, :2] = rng.normal(size=(200, 2)) * (2.0, 0.7)
    zero = np.zeros(3)
    branch = 0
    for A in (np.diag([-1.0, 1.0, 1.0]), ir.rotation((0.0, 0.0, 1.0), 33.0)):
        Q = 1.7 * (P @ A.T) + (0.5, -0.25, 0.0)
        sums = exact_sums(P, Q, zero, zero)
        H = sums[6:15].reshape(3, 3) - np.outer(sums[0:3], sums[3:6]) / len(P)
        Us, _, Vt = np.linalg.svd(H)
        branch += np.linalg.det(Vt.T @ Us.T) < 0
        M = best_fit_similarity_from_sums(len(P), sums, zero, zero)
        s = scale_of(M)
        R = M[:3, :3] / s
        assert abs(s - 1.7) <= 1e-12 and abs(np.linalg.det(R) - 1.0) <= 1e-12
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12
        assert np.abs(P @ M[:3, :3].T + M[:3, 3] - Q).max() <= 1e-12       # the planar points land on their partners either way
    assert branch >= 1
    # var = 0: all source points equal
    same = np.tile([[1.0, 2.0, 3.0]], (10, 1))
    Q = rng.normal(size=(10, 3))
    with pytest.raises(ValueError, match="not all equal"):
        best_fit_similarity_from_sums(10, exact_sums(same, Q, zero, zero), zero, zero)
    with pytest.raises(ValueError, match="at least 3 point pairs"):
        best_fit_similarity_from_sums(2, np.zeros(17), zero, zero)
    with pytest.raises(ValueError, match="at least 3 point pairs"):
        best_fit_similarity_from_sums(2, np.zeros(17), zero, zero, with_scale=False)
    nan = exact_sums(P, Q[:1].repeat(200, 0), zero, zero)
    nan[16] = np.nan
    with pytest.raises(ValueError, match="not all equal"):
        best_fit_similarity_from_sums(200, nan, zero, zero)


ALIGNMENTS = ["X", "scale 1.05", "scale 0.9", "scale 1.05 clutter", "scale 0.9 clutter"]


def check_recovery(name, T, hist, M, scale):
    A = T[:3, :3]
    s = scale_of(T)
    err_s, err_R = abs(s - scale), np.abs(A / s - M[:3, :3]).max()
    print(f"{name}: {len(hist)} iterations, s = {s!r}, |s - s0| = {err_s:.3e}, max|A/s - R0| = {err_R:.3e}, count {hist[-1][0]} of m {hist[-1][2]}")
    assert len(hist) <= (30 if name == "X" else 50)
    assert err_s <= 1e-12 and err_R <= 1e-12
    assert hist[-1][0] == 1500
    assert np.array_equal(T[3], (0.0, 0.0, 0.0, 1.0))


@pytest.mark.parametrize("name", ALIGNMENTS)
def test_restated_loop_recovers_motion_and_scale(name):
    """Measured with this restatement: X with rho = 0.75 takes 15 iterations to max|R - R0| = 1.8e-15; scale 1.05 takes 31 iterations to
    |s - s0| = 8.9e-16 and max|A/s - R0| = 1.5e-15, scale 0.9 takes 16 to 3.3e-16 and 1.7e-15, with and without clutter.  Asserted
    three orders above that, as test_icp.py does."""
    s, t, M, scale, kw, T, hist, Ts = restated_alignment(name)
    assert len(t) == 3000 and len(s) == (2000 if "clutter" in name or name == "X" else 1500) and len(hist) == len(Ts)
    check_recovery(name, T, hist, M, scale)
    if name == "X":
        assert np.abs(T[:3, :3] - M[:3, :3]).max() <= 1e-12 and hist[-1][2] == 2000


def test_restated_loop_untrimmed_fails_on_clutter():
    s, t, M, scale, kw, T, hist, Ts = restated_alignment("X untrimmed")
    err = np.abs(T[:3, :3] - M[:3, :3]).max()
    print(f"X untrimmed: {len(hist)} iterations, max|R - R0| = {err:.3e}")
    assert err > 0.1 and hist[-1][0] == hist[-1][2] == 2000
    # and rho = None on the trimmed path is the plain loop: the same transforms
    wT, whist, wTs = ir.icp_align(s, t)
    assert same_bytes(T, wT) and [h[:2] for h in hist] == whist


# ---- CPU: argument checks (no device is touched before they run) -----------------------------------------------------------------------
def test_exports():
    import pb3d
    from pb3d import preprocess_helpers as ph
    from pb3d import selection as sel
    for n in ("best_fit_similarity_from_sums", "icp_step_trimmed_resident", "icp_align", "icp_align_resident"):
        assert n in ph.__all__ and getattr(pb3d, n) is getattr(ph, n)
    for n in ("kth_smallest", "kth_smallest_resident"):
        assert n in sel.__all__ and getattr(pb3d, n) is getattr(sel, n)
    for n in ("pb3d_kth_smallest_resident", "pb3d_icp_step_trimmed_resident"):
        assert n in pb3d._lib.EXPORTED_SYMBOLS


def test_argument_checks():
    import pb3d
    rng = np.random.default_rng(2)
    ok = rng.random((10, 3))
    for bad in (0, 0.0, -0.5, 1.5, float("nan"), float("inf"), "0.5", True, 1j, [0.5]):
        with pytest.raises(ValueError, match="trim_fraction"):
            pb3d.icp_align(ok, ok, trim_fraction=bad)
    for bad in (1, 0, "yes", None, 1.0):
        with pytest.raises(ValueError, match="with_scale"):
            pb3d.icp_align(ok, ok, with_scale=bad)
    # the earlier checks still come first on the new path
    with pytest.raises(ValueError, match="target cloud is empty"):
        pb3d.icp_align(ok, np.zeros((0, 3)), trim_fraction=0.5)
    with pytest.raises(ValueError, match="at least 3 point pairs"):
        pb3d.icp_align(ok[:2], ok, with_scale=True)
    for bad in (-1, 3, 2.0, True, None):
        with pytest.raises(ValueError, match="rank"):
            pb3d.kth_smallest([3.0, 1.0, 2.0], bad)
    with pytest.raises(ValueError, match="at least one value"):
        pb3d.kth_smallest([], 0)
    with pytest.raises(TypeError, match="unsupported dtype"):
        pb3d.kth_smallest(np.array([1j, 2j]), 0)
    with pytest.raises(ValueError, match="rank"):
        pb3d.kth_smallest_resident(None, 5, 5)
    # the restated loop on a gate nothing passes
    with pytest.raises(ValueError, match="only 0 point pairs"):
        tr.icp_align(ok + 100.0, ok, max_distance=1.0, trim_fraction=0.5)


def test_cabi_argument_checks():
    """the entries refuse bad fractions, ranks, counts and null arguments before they look at the context"""
    import pb3d
    L = pb3d._lib
    lib = L.load()
    T = np.eye(4)[:3].reshape(12).copy()
    z = np.zeros(3)
    out = np.zeros(20)
    one = C.c_void_p(out.ctypes.data)       # never dereferenced: every call below is refused first

    def refused(rc, text):
        assert rc == -1 and text in lib.pb3d_last_error().decode(), (rc, lib.pb3d_last_error())

    def trimmed(src=one, ns=5, tgt=one, nt=4, t=T, md2=-1.0, rho=0.5, cp=z, cq=z, o=one):
        return lib.pb3d_icp_step_trimmed_resident(None, src, 1, ns, tgt, 1, nt, None if t is None else L.p_dbl(t), md2, rho, L.p_dbl(cp), L.p_dbl(cq), o)

    for rho in (0.0, -1.0, 1.5, float("nan"), float("inf")):
        refused(trimmed(rho=rho), "trim fraction")
    refused(trimmed(nt=0), "the target is empty")
    refused(trimmed(ns=-1), "negative point count")
    refused(trimmed(ns=1 << 31), "2^31 - 1")
    refused(trimmed(md2=float("nan")), "NaN")
    refused(trimmed(t=None), "null argument")
    refused(trimmed(o=None), "null argument")
    refused(trimmed(src=None), "null buffer")
    refused(trimmed(tgt=None), "null buffer")
    refused(trimmed(), "null context")
    refused(trimmed(rho=1.0), "null context")
    refused(trimmed(ns=0), "null context")
    for n, rank in ((5, 5), (5, -1), (1, 1), (5, 1 << 40)):
        refused(lib.pb3d_kth_smallest_resident(None, one, n, rank, one), "0 <= rank < n")
    refused(lib.pb3d_kth_smallest_resident(None, one, 0, 0, one), "1 <= n")
    refused(lib.pb3d_kth_smallest_resident(None, one, -3, 0, one), "1 <= n")
    refused(lib.pb3d_kth_smallest_resident(None, one, 1 << 31, 0, one), "2^31 - 1")
    refused(lib.pb3d_kth_smallest_resident(None, None, 5, 2, one), "null buffer")
    refused(lib.pb3d_kth_smallest_resident(None, one, 5, 2, None), "null buffer")
    refused(lib.pb3d_kth_smallest_resident(None, one, 5, 2, one), "null context")


# ---- GPU: the selection -----------------------------------------------------------------------------------------------------------------
def from_bits(b):
    return np.ascontiguousarray(b, dtype=np.uint64).view(np.float64)


def family(name, n, rng):
    if name == "all equal":
        return np.full(n, 1.5)
    if name == "one ulp apart":
        return rng.choice([1.0, np.nextafter(1.0, 2.0)], n)
    if name == "lowest digit":
        return from_bits(np.uint64(0x3FE5555555555500) | rng.integers(0, 256, n).astype(np.uint64))
    if name == "highest digit":       # sign and seven exponent bits vary; the low exponent bits are 0, so no inf and no NaN
        return from_bits((rng.integers(0, 256, n).astype(np.uint64) << np.uint64(56)) | np.uint64(0x000123456789AB))
    if name == "signed zeros":
        return rng.choice([0.0, -0.0], n)
    if name == "negatives":
        return -np.abs(rng.normal(size=n)) * 10.0 ** rng.integers(-30, 30, n)
    if name == "subnormals":
        return from_bits(rng.integers(1, 1 << 52, n).astype(np.uint64) | (rng.integers(0, 2, n).astype(np.uint64) << np.uint64(63)))
    if name == "infinities":
        return rng.choice([np.inf, -np.inf, 1.0, -1.0], n)
    if name == "nan above inf":
        return from_bits(rng.choice(np.array([0x7FF0000000000000, 0x7FF8000000000000, 0x3FF0000000000000, 0x7FEFFFFFFFFFFFFF], np.uint64), n))
    assert name == "normals"
    return rng.normal(size=n)


FAMILIES = ["all equal", "one ulp apart", "lowest digit", "highest digit", "signed zeros", "negatives", "subnormals", "infinities", "nan above inf",
            "normals"]
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 4097, 65537]


@gpu
@pytest.mark.parametrize("name", FAMILIES)
def test_kth_matches_the_restatement(pb3d_gpu, name):
    rng = np.random.default_rng(FAMILIES.index(name))
    d_out = pb3d_gpu.device.DeviceBuffer(8)
    try:
        for n in SIZES:
            v = family(name, n, rng)
            srt = np.sort(tr.order_keys(v))
            d_v = pb3d_gpu.device.from_numpy(v)
            try:
                for rank in sorted({0, n // 2, n - 1}):
                    pb3d_gpu.kth_smallest_resident(d_v, n, rank, out=d_out)
                    got = d_out.download((1,), np.float64)
                    want = tr.kth(v, rank)
                    assert same_bytes(got, [want]), (name, n, rank, got, want)
                    assert tr.order_keys(got)[0] == srt[rank]
            finally:
                d_v.free()
    finally:
        d_out.free()
    # the host-array form
    v = family(name, 1000, rng)
    assert same_bytes([pb3d_gpu.kth_smallest(v, 333)], [tr.kth(v, 333)])


@gpu
def test_kth_state_is_cleared_and_repeatable(pb3d_gpu):
    """65 537 values, then 300: histograms left over from the first call would shift the second's bins.  Every rank of a small list.
    A list that starts 8 bytes past a 16-byte boundary (the kernel reads aligned pairs between a head and a tail element)."""
    rng = np.random.default_rng(77)
    big, small = rng.normal(size=65537), rng.normal(size=300) * 1e-3
    a = pb3d_gpu.kth_smallest(big, 40000)
    b = pb3d_gpu.kth_smallest(small, 17)
    assert same_bytes([a], [tr.kth(big, 40000)]) and same_bytes([b], [tr.kth(small, 17)])
    assert same_bytes([pb3d_gpu.kth_smallest(big, 40000)], [a]) and same_bytes([pb3d_gpu.kth_smallest(small, 17)], [b])
    ints = rng.integers(-4, 5, 41).astype(np.float64)
    assert same_bytes([pb3d_gpu.kth_smallest(ints, r) for r in range(41)], np.sort(ints))
    small_ints = rng.integers(0, 9, 50)
    assert same_bytes([pb3d_gpu.kth_smallest(small_ints, 49)], [float(small_ints.max())])        # an integer array is taken as float64
    for n in (1, 2, 3, 64, 129, 1000, 4098):
        v = rng.normal(size=n + 1)
        d_v = pb3d_gpu.device.from_numpy(v)
        try:
            for rank in sorted({0, n // 2, n - 1}):
                d_out = pb3d_gpu.kth_smallest_resident(d_v.at(8), n, rank)
                try:
                    assert same_bytes(d_out.download((1,), np.float64), [tr.kth(v[1:], rank)]), (n, rank)
                finally:
                    d_out.free()
        finally:
            d_v.free()


# ---- GPU: the step ---------------------------------------------------------------------------------------------------------------------
class Clouds:
    """source / target uploaded once; trimmed() and plain() run the device steps and return their words"""

    def __init__(self, pb3d, src, tgt):
        from pb3d.eval_helpers import _cloud
        self.pb3d, self.ph = pb3d, pb3d.preprocess_helpers
        self.src, self.sf = _cloud(src, "source")
        self.tgt, self.tf = _cloud(tgt, "target")
        self.d_s = pb3d.device.from_numpy(self.src) if len(self.src) else pb3d.device.DeviceBuffer(8)
        self.d_t = pb3d.device.from_numpy(self.tgt)
        self.d_out = pb3d.device.DeviceBuffer(20 * 8)
        self.ph.icp_index_resident(self.d_t, len(self.tgt), self.tf)

    def trimmed(self, T, max_dist2, rho, cp, cq):
        """the 20 words as uint64; the buffer is filled with ones first, so a word the step does not write shows"""
        self.d_out.upload(np.full(20, 0xFFFFFFFFFFFFFFFF, np.uint64))
        self.ph.icp_step_trimmed_resident(self.d_s, len(self.src), self.d_t, len(self.tgt), T, max_dist2, rho, cp, cq, self.sf, self.tf, out=self.d_out)
        return self.d_out.download((20,), np.uint64)

    def plain(self, T, max_dist2, cp, cq):
        self.ph.icp_step_resident(self.d_s, len(self.src), self.d_t, len(self.tgt), T, max_dist2, cp, cq, self.sf, self.tf, out=self.d_out)
        return self.d_out.download((17,), np.uint64)

    def free(self):
        for b in (self.d_s, self.d_t, self.d_out):
            b.free()


def check_steps(pb3d, src, tgt, T, gates_rhos, cp, cq, what):
    """every (max_dist2, rho) of gates_rhos on one pair of clouds: all 20 words against the restatement"""
    c = Clouds(pb3d, src, tgt)
    got = []
    try:
        with np.errstate(over="ignore", invalid="ignore"):
            prepared = tr.prepare(src, tgt, T, cp, cq)
        for md2, rho in gates_rhos:
            g = c.trimmed(T, md2, rho, cp, cq)
            w = tr.words(tr.result(*tr.finish(prepared, md2, rho)))
            assert np.array_equal(g, w), (what, md2, rho, g, w)
            got.append(g)
    finally:
        c.free()
    return got


RHOS = [1e-9, 1.0 / 3.0, 0.5, float(np.nextafter(1.0, 0.0)), 1.0]


@gpu
@pytest.mark.parametrize("nt", [1, 500])
def test_step_words_by_point_count(pb3d_gpu, nt):
    """nt = 1 at the origin with T = I: d2 = (x*x + y*y) + z*z of the source, so the source's small integer coordinates choose the keys
    (many ties at every tau).  65 537 = 256 workgroups of 256 and one point."""
    rng = np.random.default_rng(19 + nt)
    T, c = np.eye(4), np.zeros(3)
    tgt = np.zeros((1, 3)) if nt == 1 else rng.normal(size=(nt, 3)) * (1.0, 0.5, 0.25)
    for ns in (1, 63, 64, 65, 255, 256, 257, 1000, 65537):
        src = rng.integers(-6, 7, (ns, 3)).astype(np.float64) if nt == 1 else rng.normal(size=(ns, 3)) * (1.1, 0.6, 0.3)
        got = check_steps(pb3d_gpu, src, tgt, T, [(-1.0, rho) for rho in RHOS], c, c, (ns, nt))
        for g, rho in zip(got, RHOS):
            assert int(g[18]) == ns and int(g[0]) >= tr.trim_k(ns, rho)
        assert int(got[0][0]) >= 1 and int(got[-1][0]) == ns
        if nt == 1:
            d2 = (src[:, 0] * src[:, 0] + src[:, 1] * src[:, 1]) + src[:, 2] * src[:, 2]
            assert got[0][19:].view(np.float64)[0] == d2.min() and got[-1][19:].view(np.float64)[0] == d2.max()
            assert int(got[0][0]) == (d2 == d2.min()).sum()


@gpu
@pytest.mark.parametrize("sdt,tdt", [("float64", "float64"), ("float64", "float32"), ("float32", "float64"), ("float32", "float32")])
def test_step_words_by_dtype(pb3d_gpu, sdt, tdt):
    rng = np.random.default_rng(23)
    src = (rng.normal(size=(1000, 3)) * (2.0, 1.0, 0.5) + (3.0, -1.0, 7.0)).astype(sdt)
    tgt = (rng.normal(size=(500, 3)) * (2.0, 1.0, 0.5) + (3.1, -0.9, 7.2)).astype(tdt)
    T = np.eye(4)
    T[:3, :3] = ir.rotation((0.3, -1.0, 0.2), 7.0) * 1.03          # inexact entries, not rigid
    T[:3, 3] = (0.1, -1.0 / 3.0, math.pi / 50)
    cp, cq = np.array([2.9, -1.1, 6.7]), np.array([3.3, -0.7, 7.1])
    got = check_steps(pb3d_gpu, src, tgt, T, [(md2, rho) for md2 in (-1.0, 1.0 / 3.0) for rho in RHOS], cp, cq, (sdt, tdt))
    assert int(got[4][18]) == 1000 and 100 < int(got[9][18]) < 1000


@gpu
def test_full_fraction_is_the_plain_step(pb3d_gpu):
    """rho = 1 against pb3d_icp_step_resident on the same input: independent of the restatement"""
    rng = np.random.default_rng(29)
    src = rng.normal(size=(4099, 3))
    tgt = rng.normal(size=(700, 3))
    T = np.eye(4)
    T[:3, :3] = ir.rotation((1.0, 1.0, 0.0), 3.0)
    cc = np.array([0.1, 0.2, 0.3])
    c = Clouds(pb3d_gpu, src, tgt)
    try:
        for md2 in (-1.0, 0.05):
            old = c.plain(T, md2, cc, cc)
            new = c.trimmed(T, md2, 1.0, cc, cc)
            assert np.array_equal(new[:17], old) and new[18] == old[0]
            _, d2 = ir.nearest(ir.transform(src, T[:3]), tgt)
            assert new[19:].view(np.float64)[0] == (d2[d2 <= md2].max() if md2 >= 0 else d2.max())
            assert (int(old[0]) == len(src)) == (md2 < 0)
    finally:
        c.free()


@gpu
def test_ties_gate_and_overflow(pb3d_gpu):
    T, zero = np.eye(4), np.zeros(3)
    # ties at tau: candidate d2 values {0, 1, 1, 1, 4, 25} and k = 2 -> tau = 1, all three pairs at 1 are used
    origin = np.zeros((1, 3))
    src = np.array([[0.0, 0, 0], [1.0, 0, 0], [0, -1.0, 0], [0, 0, 1.0], [0, 2.0, 0], [3.0, 4.0, 0]])
    (g,) = check_steps(pb3d_gpu, src, origin, T, [(-1.0, 1.0 / 3.0)], zero, zero, "ties")
    assert tr.trim_k(6, 1.0 / 3.0) == 2
    assert int(g[0]) == 4 and int(g[18]) == 6 and g[19:].view(np.float64)[0] == 1.0
    assert g[1:18].view(np.float64)[15] == 3.0                          # sum of the used d2: 0 + 1 + 1 + 1
    # the lattice of test_icp.test_gate: (3, 4, 0) is exactly 5 from its nearest target, the seven others sit on theirs
    tgt = np.array([[x, y, z] for x in (0, 20, 40) for y in (0, 20) for z in (0, 20)], np.float64)
    src = np.concatenate([tgt[1:8], [[3.0, 4.0, 0.0]]])
    c = np.array([20.0, 10.0, 10.0])
    below = float(np.nextafter(5.0, 0.0))
    at5, under = check_steps(pb3d_gpu, src, tgt, T, [(25.0, 1.0), (below * below, 1.0)], c, c, "gate")
    assert (int(at5[0]), int(at5[18]), at5[19:].view(np.float64)[0]) == (8, 8, 25.0)
    assert (int(under[0]), int(under[18]), under[19:].view(np.float64)[0]) == (7, 7, 0.0)
    # k follows m, not ns: twelve more source points the gate rejects leave k and tau where they were
    more = np.concatenate([src, tgt[:12] + (7.0, 0.0, 0.0)])
    half8, half20 = check_steps(pb3d_gpu, src, tgt, T, [(25.0, 0.9)], c, c, "k of 8")[0], check_steps(pb3d_gpu, more, tgt, T, [(25.0, 0.9)], c, c, "k of 20")[0]
    assert tr.trim_k(8, 0.9) == 8 and tr.trim_k(20, 0.9) == 18
    assert (int(half20[0]), int(half20[18]), half20[19]) == (8, 8, half8[19]) and half8[19:].view(np.float64)[0] == 25.0
    # a gate that rejects everything: twenty zero words, and the alignment refuses
    far = src + (7.0, 0.0, 0.0)
    (none,) = check_steps(pb3d_gpu, far, tgt, T, [(1.0, 0.5)], c, c, "gate rejects all")
    assert not none.any()
    with pytest.raises(ValueError, match="only 0 point pairs"):
        pb3d_gpu.icp_align(far, tgt, max_distance=1.0, trim_fraction=0.5)
    # an empty source needs no index and gives twenty zero words
    (empty,) = check_steps(pb3d_gpu, np.zeros((0, 3)), tgt, T, [(-1.0, 0.5)], c, c, "empty source")
    assert not empty.any()
    # overflow: large finite entries send ONE source point to infinity; it is no candidate and is not counted in m
    big = np.eye(4)
    big[0, 0] = 1e300
    src = np.zeros((5, 3))
    src[:, 1] = [0.0, 1.0, 2.0, 3.0, 4.0]
    src[2, 0] = 1e10
    for rho in (0.5, 1.0):
        (g,) = check_steps(pb3d_gpu, src, origin, big, [(-1.0, rho)], zero, zero, ("overflow", rho))
        assert int(g[18]) == 4 and int(g[0]) == (2 if rho < 1 else 4)
        assert g[19:].view(np.float64)[0] == (1.0 if rho < 1 else 16.0)


@gpu
def test_index_refusal_slot_reuse_and_determinism(pb3d_gpu):
    rng = np.random.default_rng(31)
    src, tgt = rng.normal(size=(5000, 3)), rng.normal(size=(3000, 3))
    T = np.eye(4)
    T[:3, :3] = ir.rotation((1.0, 1.0, 0.0), 3.0)
    cc = np.array([0.1, 0.2, 0.3])
    a = Clouds(pb3d_gpu, src, tgt)
    try:
        first = a.trimmed(T, 0.5, 0.7, cc, cc)
        assert np.array_equal(first, tr.words(tr.step(src, tgt, T, 0.5, 0.7, cc, cc)))
        # a step with 300 points after one with 5 000: the key slot keeps its size, the step reads its own ns keys only
        b = Clouds(pb3d_gpu, src[:300], tgt)
        try:
            small = b.trimmed(T, 0.5, 0.7, cc, cc)
            assert np.array_equal(small, tr.words(tr.step(src[:300], tgt, T, 0.5, 0.7, cc, cc)))
            # b's index (same target values, another buffer) retired a's: refused, never rebuilt behind the caller's back
            with pytest.raises(ValueError, match="built for another target"):
                a.trimmed(T, 0.5, 0.7, cc, cc)
        finally:
            b.free()
        a.ph.icp_index_resident(a.d_t, len(tgt), a.tf)
        pb3d_gpu.kth_smallest(rng.normal(size=1000), 5)                 # a selection of its own in between
        assert np.array_equal(a.trimmed(T, 0.5, 0.7, cc, cc), first)
    finally:
        a.free()


# ---- GPU: whole alignments -------------------------------------------------------------------------------------------------------------
def check_alignment(pb3d, src, tgt, want, **kw):
    T, hist, Ts = pb3d.icp_align(src, tgt, return_history=True, **kw)
    wT, whist, wTs = want
    assert len(hist) == len(whist) and len(Ts) == len(wTs)
    for i, ((c, r, m, tau), (wc, wr, wm, wtau)) in enumerate(zip(hist, whist)):
        assert c == wc and m == wm and same_bytes([r, tau], [wr, wtau]), (i, c, wc, m, wm, r, wr, tau, wtau)
    for i, (a, b) in enumerate(zip(Ts, wTs)):
        assert same_bytes(a, b), (i, a, b)
    assert same_bytes(T, wT) and same_bytes(T, Ts[-1])
    return T, hist


@gpu
@pytest.mark.parametrize("name", ["X", "scale 1.05", "scale 1.05 clutter"])
def test_alignment_synthetic(pb3d_gpu, name):
    s, t, M, scale, kw, wT, whist, wTs = restated_alignment(name)
    T, hist = check_alignment(pb3d_gpu, s, t, (wT, whist, wTs), **kw)
    check_recovery(name, T, hist, M, scale)
    assert same_bytes(pb3d_gpu.icp_align(s, t, **kw), wT)               # without the history: the matrix alone


@gpu
def test_alignment_full_fraction_is_the_plain_alignment(pb3d_gpu):
    s, t, M, extent = ir.recovery_case(5.0)
    old, ohist, oTs = pb3d_gpu.icp_align(s, t, return_history=True)
    new, nhist, nTs = pb3d_gpu.icp_align(s, t, trim_fraction=1.0, return_history=True)
    assert same_bytes(new, old) and len(nTs) == len(oTs) and all(same_bytes(a, b) for a, b in zip(nTs, oTs))
    assert [h[:2] for h in nhist] == ohist and all(len(h) == 2 for h in ohist) and all(h[2] == 1500 for h in nhist)


@gpu
def test_alignment_real_cloud(pb3d_gpu):
    """three iterations only: the brute-force restatement costs about a second per iteration on 6 000 x 20 000 points"""
    with np.load(os.path.join(GOLDEN, "inter_sfm20k.npz"), allow_pickle=False) as z:
        tgt = np.ascontiguousarray(z["sfm"])
    extent = float((tgt.max(0) - tgt.min(0)).max())
    M = ir.motion(5.0, extent)
    rng = np.random.default_rng(7)
    pick = np.sort(rng.choice(len(tgt), 5000, replace=False))
    clutter = rng.normal(size=(1000, 3)) * 0.05 * extent + (tgt.max(0) + 0.5 * extent)
    src = np.ascontiguousarray(ir.moved_back(np.concatenate([tgt[pick], clutter]), M))
    want = tr.icp_align(src, tgt, max_iterations=3, trim_fraction=0.8)
    T, hist = check_alignment(pb3d_gpu, src, tgt, want, max_iterations=3, trim_fraction=0.8)
    print(f"real cloud: {len(hist)} iterations, rmse {hist[0][1]:.4e} -> {hist[-1][1]:.4e}, count {hist[-1][0]} of {hist[-1][2]}, tau {hist[-1][3]:.4e}")
    assert len(hist) == 3 and hist[-1][1] < hist[0][1] and all(h[0] >= 4800 and h[2] == 6000 for h in hist)
