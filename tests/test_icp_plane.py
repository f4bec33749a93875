"""Point-to-plane icp_align and the point-cloud normals under it (pb3d/preprocess_helpers.py on csrc/icp.hip and csrc/normals.hip).

The chain of evidence is the one of tests/test_icp.py and tests/test_icp_trimmed.py: include/pb3d.h states the arithmetic;
tests/icp_plane_restate.py restates it in NumPy on top of icp_restate and icp_trim_restate; the CPU tests pin the restatement (its 29
sums against exact sums with a derived bound, its normals against np.linalg.eigh of a long-double covariance, the 6 x 6 solve against
motions it must recover, its loop against the point-to-point loop on a surface that one cannot register); the GPU tests demand the
restatement's BYTES from the device -- every normal, all 32 words of a step, every transform, count, both RMSEs, rank, candidate count
and tau of a whole alignment."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import icp_plane_restate as pr
import icp_restate as ir
import icp_trim_restate as tr

gpu = pytest.mark.gpu
U = 2.0 ** -53


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def unit_rows(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def step_case(n, nt=97):
    """source, target, target normals, T, pivot of the step tests: an anisotropic cloud off the origin, an inexact transform"""
    rng = np.random.default_rng(1000 * nt + n)
    src = rng.normal(size=(n, 3)) * (3.0, 1.0, 0.2) + (10.0, -4.0, 0.5)
    tgt = rng.normal(size=(nt, 3)) * (3.0, 1.0, 0.2) + (10.0, -4.0, 0.5)
    T = np.eye(4)
    T[:3, :3] = ir.rotation((0.3, -1.0, 0.2), 7.0)
    T[:3, 3] = (0.1, -0.2, 0.05)
    return src, tgt, unit_rows(rng, nt), T, np.array([9.5, -4.25, 0.4])


# ---- CPU: the restated step -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 257, 5000, 65537])
def test_restated_sums_against_exact_sums(n):
    """any summation order of n terms errs by at most n * 2^-53 * sum|term| (each of the n - 1 additions adds a relative 2^-53 of a
    partial sum that is itself bounded by sum|term|): derived, not measured -- the bound of test_icp.py, now over 29 sums"""
    src, tgt, nrm, T, c = step_case(n)
    prepared = pr.prepare(src, tgt, nrm, T, c)
    used, t, m, tau = pr.finish(prepared, 2.0, 0.6)
    assert 0 < used.sum() <= m <= n and (n < 255 or used.sum() < m < n)     # the gate and the trim both drop pairs of the larger clouds
    assert used.sum() >= tr.trim_k(m, 0.6)
    got = ir.ordered_sum(t)
    assert got.shape == (29,)
    for col in range(29):
        exact = math.fsum(t[:, col].tolist())
        bound = n * U * math.fsum(np.abs(t[:, col]).tolist())
        print(f"n={n} term {col}: |restated - exact| = {abs(got[col] - exact):.3e}, bound {bound:.3e}")
        assert abs(got[col] - exact) <= bound, (n, col)
    count, sums, m2, tau2 = pr.step(src, tgt, nrm, T, 2.0, 0.6, c)
    assert count == int(used.sum()) and same_bytes(sums, got) and m2 == m and same_bytes([tau2], [tau])
    # no trim and the full fraction use the same pairs: count and sums agree bytewise; only m and tau tell them apart
    c0, s0, m0, tau0 = pr.step(src, tgt, nrm, T, 2.0, -1.0, c)
    c1, s1, m1, tau1 = pr.step(src, tgt, nrm, T, 2.0, 1.0, c)
    assert c0 == c1 == m1 and same_bytes(s0, s1) and m0 == 0 and same_bytes([tau0], [0.0])
    assert pr.step(src, tgt, nrm, T, 2.0, None, c)[0] == c0
    # term 28 is the point-to-point step's sum of squared distances
    cp, sp = ir.step(src, tgt, T, 2.0, c, c)
    assert cp == c0 and same_bytes(s0[28:], sp[15:])
    # every term is even in the normal
    flipped = np.where(np.arange(len(nrm))[:, None] % 2 == 0, -nrm, nrm)
    for other in (-nrm, flipped):
        assert np.array_equal(pr.words(pr.step(src, tgt, other, T, 2.0, 0.6, c)), pr.words((count, sums, m2, tau2)))


# ---- CPU: the restated normals ----------------------------------------------------------------------------------------------------------
GAP_FLOOR = 0.05        # (w1 - w0) / w2 of every neighbourhood of the lattice sheet; measured minimum 0.113 (k = 3)
ANGLE_K = 7.5           # 8 x the largest angle / (k * 2^-53 / gap) the restatement shows on the lattice sheet: 0.93 (k = 3)


@functools.lru_cache(maxsize=None)
def lattice():
    pts = pr.lattice_sheet()
    pts.setflags(write=False)
    return pts


@pytest.mark.parametrize("k", [3, 16, 32])
def test_restated_normals_against_eigh(k):
    """The normal is the eigenvector of the smallest eigenvalue of a covariance whose entries carry a relative error of about k * 2^-53;
    first-order perturbation theory turns that into an angle of about k * 2^-53 / gap, gap = (w1 - w0) / w2.  The reference is
    np.linalg.eigh of the covariance formed in np.longdouble (its own error is of the same kind, and inside the measured ratio).
    Measured on this sheet (1 600 points, offset (3, -2, 5) from the origin): ratio 0.93 at k = 3, 0.24 at k = 16, 0.16 at k = 32;
    minimum gap 0.113, 0.221, 0.214."""
    pts = lattice()
    assert len(pts) == 1600 and np.abs(pts.mean(0)).min() > 1.0
    rows = pr.knn_rows(pts, k)
    assert np.array_equal(rows[:, 0], np.arange(len(pts)))                  # no duplicates: a point is its own first neighbour
    got = pr.normals(pts, rows)
    x = pts[rows].astype(np.longdouble)
    y = x - x.mean(axis=1, keepdims=True)
    cov = np.einsum("nka,nkb->nab", y, y).astype(np.float64)
    w, V = np.linalg.eigh(cov)
    gap = (w[:, 1] - w[:, 0]) / w[:, 2]
    print(f"k={k}: minimum gap {gap.min():.4f}")
    assert gap.min() > GAP_FLOOR
    ref = V[:, :, 0]
    angle = np.arctan2(np.linalg.norm(np.cross(got, ref), axis=1), np.abs(np.einsum("na,na->n", got, ref)))
    ratio = angle / (k * U / gap)
    print(f"k={k}: largest angle {angle.max():.3e}, largest angle / (k * 2^-53 / gap) = {ratio.max():.3f}")
    assert (angle <= ANGLE_K * k * U / gap).all()
    length = np.sqrt((got * got).sum(axis=1))
    assert np.abs(length - 1.0).max() <= 4 * U
    # the sheet is a graph over (u, v): its normals have a dominant z, so the default sign makes z positive
    assert (got[:, 2] > 0.5).all()


def test_restated_sign_rules_and_duplicates():
    pts = lattice()[:400]
    rows = pr.knn_rows(pts, 8)
    free = pr.normals(pts, rows)
    lead = np.abs(free).argmax(axis=1)
    assert (free[np.arange(len(free)), lead] > 0).all()
    for view in ((3.0, -2.0, 50.0), (3.0, -2.0, -50.0), (2.25, -2.0, 5.15)):      # the last lies in the sheet's hollow: both signs
        n = pr.normals(pts, rows, view)
        d = ((np.array(view) - pts) * n).sum(axis=1)
        assert (d > 0).all()
        flipped = (n != free).any(axis=1)
        assert same_bytes(np.where(flipped[:, None], -n, n), free)          # the same direction, sign apart
        assert (flipped.all(), flipped.any()) == ((True, True) if view[2] < 0 else (False, view[2] < 6))
    # a tie of the largest magnitude goes to the lowest component: spread along (1, 1, 0) and along z leaves the normal (a, -a, 0),
    # whose first component decides
    line = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 0.0], [2.0, 2.0, 0.0], [1.0, 1.0, 1.0], [1.0, 1.0, -1.0]])
    n = pr.normals(line, np.tile(np.arange(5), (5, 1)))
    assert same_bytes(n, np.tile(n[0], (5, 1))) and n[0, 0] > 0 and n[0, 0] == -n[0, 1] and n[0, 2] == 0.0
    # k coincident points: zero covariance, no rotation, column 0 of the identity
    dup = np.tile([[0.3, -1.7, 2.9]], (6, 1))
    assert same_bytes(pr.normals(dup, np.tile(np.arange(6), (6, 1))), np.tile([[1.0, 0.0, 0.0]], (6, 1)))
    assert same_bytes(pr.normals(dup, np.tile(np.arange(6), (6, 1)), (-5.0, 0.0, 0.0)), np.tile([[-1.0, -0.0, -0.0]], (6, 1)))     # negated whole
    assert np.array_equal(pr.knn_rows(dup, 4), np.tile(np.arange(4), (6, 1)))       # ties at d2 = 0: ascending index


# ---- CPU: the host solve ----------------------------------------------------------------------------------------------------------------
def exact_pair_sums(P, Q, N, c):
    """the 29 sums of the pairs (P_i, Q_i) with normals N_i, no search"""
    d = P - Q
    Pc = P - c
    r = (d * N).sum(axis=1)
    J = np.concatenate([np.cross(Pc, N), N], axis=1)
    t = np.empty((len(P), 29))
    iu = np.triu_indices(6)
    t[:, :21] = J[:, iu[0]] * J[:, iu[1]]
    t[:, 21:27] = J * r[:, None]
    t[:, 27] = r * r
    t[:, 28] = (d * d).sum(axis=1)
    return ir.ordered_sum(t)


def test_plane_step_recovers_a_small_motion_and_flat_rank():
    from pb3d import plane_step_from_sums
    rng = np.random.default_rng(17)
    Q = rng.normal(size=(400, 3)) * (2.0, 1.0, 0.5) + (4.0, -1.0, 2.0)
    N = unit_rows(rng, 400)
    c = np.array([3.8, -0.9, 2.2])
    errs = []
    for deg in (1e-3, 1e-5):
        M = np.eye(4)
        M[:3, :3] = ir.rotation((0.2, 1.0, -0.4), deg)
        M[:3, 3] = np.array([2.0, -1.0, 3.0]) * math.radians(deg)
        P = ir.moved_back(Q, M)
        step, rank = plane_step_from_sums(400, exact_pair_sums(P, Q, N, c), c)
        err = np.abs(step - M).max()
        errs.append(err)
        th = math.radians(deg)
        print(f"{deg} degrees: rank {rank}, max|step - M| = {err:.3e}, theta^2 = {th * th:.3e}")
        # one linearised step: the error is second order in the motion (constant: a few times the cloud's radius)
        assert rank == 6 and err <= 40.0 * th * th + 1e-14
        assert np.array_equal(step[3], (0.0, 0.0, 0.0, 1.0)) and np.abs(step[:3, :3] @ step[:3, :3].T - np.eye(3)).max() <= 4 * U
    assert errs[1] < errs[0]
    # a flat target: one normal for all pairs leaves rotations about it and translations across it undetermined
    n = ir.rotation((1.0, -1.0, 0.5), 25.0)[:, 2]
    Qf = Q - ((Q - c) @ n)[:, None] * n                                     # Q dropped into the plane through c
    M = np.eye(4)
    M[:3, :3] = ir.rotation((2.0, 1.0, -1.0), 0.01)
    M[:3, 3] = (1e-4, 2e-4, -1e-4)
    P = ir.moved_back(Qf, M)
    step, rank = plane_step_from_sums(400, exact_pair_sums(P, Qf, np.tile(n, (400, 1)), c), c)
    moved = P @ step[:3, :3].T + step[:3, 3]
    off = np.abs((moved - c) @ n).max()
    print(f"flat: rank {rank}, largest distance to the plane after the step {off:.3e} (before {np.abs((P - c) @ n).max():.3e})")
    assert rank == 3 and off <= 1e-7
    # the identity for sums of zero, a refusal below six pairs and for a short vector
    step, rank = plane_step_from_sums(6, np.zeros(29), c)
    assert rank == 0 and np.array_equal(step, np.eye(4))
    with pytest.raises(ValueError, match="at least 6 point pairs"):
        plane_step_from_sums(5, np.zeros(29), c)
    with pytest.raises(ValueError, match="27 sums"):
        plane_step_from_sums(10, np.zeros(16), c)
    # a rotation vector below the switch: I + K
    tiny = np.zeros(29)
    tiny[np.flatnonzero(np.triu_indices(6)[0] == np.triu_indices(6)[1])] = 1.0      # A = I
    tiny[21:27] = (-1e-13, 2e-13, 0.0, -0.5, 0.0, 0.25)                             # g = -x
    step, rank = plane_step_from_sums(6, tiny, np.zeros(3))
    assert rank == 6 and same_bytes(step[:3], [[1.0, 0.0, -2e-13, 0.5], [0.0, 1.0, -1e-13, 0.0], [2e-13, 1e-13, 1.0, -0.25]])


# ---- CPU: the restated loop -------------------------------------------------------------------------------------------------------------
def case_clouds(name):
    """(source, target, normals or None, kwargs) of the named whole-alignment case"""
    kind, how = name.split()
    if kind == "flat":
        s, t, n, _ = pr.flat_case()
        nrm, kw = np.tile(n, (len(t), 1)), {}
    else:
        s, t, nrm, _ = pr.sheet_case(clutter=500 if kind == "clutter" else 0)
        kw = {"trim_fraction": 0.6} if kind == "clutter" else {}
        if name == "clutter estimated":
            kw["max_iterations"] = 6        # the trimmed set keeps flipping by a pair at the 1e-9 level; six iterations pin every word
    return s, t, (nrm if how == "given" else None), kw


@functools.lru_cache(maxsize=None)
def restated_alignment(name):
    """one restated alignment per case, shared by the CPU and the GPU tests (read-only)"""
    s, t, nrm, kw = case_clouds(name)
    T, hist, Ts = pr.icp_align(s, t, target_normals=nrm, **kw)
    for a in (s, t, T, *Ts) + (() if nrm is None else (nrm,)):
        a.setflags(write=False)
    return s, t, nrm, kw, T, hist, Ts


@functools.lru_cache(maxsize=None)
def point_to_point_on_the_sheet():
    s, t, _, _ = pr.sheet_case()
    return ir.icp_align(s, t)


@pytest.mark.parametrize("how", ["given", "estimated"])
def test_restated_loop_registers_the_sheet(how):
    """Measured with this restatement (4 000 target, 1 000 source points, 4 degrees and (0.05, -0.04, 0.03)): point-to-plane stops by
    tolerance after 9 iterations 3.3e-4 off with the sheet's own normals, after 7 iterations 5.9e-4 off with estimated ones (the floor is
    the target's sampling: the tangent plane at the nearest sample is not the surface); point-to-point stops after 31 iterations 7.1e-2
    off, its pairs holding each cloud to the other's samples."""
    s, t, nrm, kw, T, hist, Ts = restated_alignment(f"sheet {how}")
    M = pr.sheet_motion()
    Tp, hp, _ = point_to_point_on_the_sheet()
    err, errp = np.abs(T - M).max(), np.abs(Tp - M).max()
    print(f"sheet, normals {how}: {len(hist)} iterations, max|T - M| = {err:.3e}; point-to-point: {len(hp)} iterations, {errp:.3e}")
    assert len(hist) < 50 and abs(hist[-2][1] - hist[-1][1]) < 1e-9          # stopped by tolerance
    assert err < 0.1 * errp
    assert all(h[0] == 1000 and h[3] == 6 and len(h) == 4 for h in hist)
    assert hist[-1][1] < 0.02 * hist[0][1] and hist[-1][2] > 50 * hist[-1][1]     # the plane distance collapses, the point distance is the sampling's
    assert np.array_equal(T[3], (0.0, 0.0, 0.0, 1.0))


@pytest.mark.parametrize("how", ["given", "estimated"])
def test_restated_loop_drops_the_source_into_a_flat_target(how):
    s, t, nrm, kw, T, hist, Ts = restated_alignment(f"flat {how}")
    _, _, n, offset = pr.flat_case()
    rms = float(np.sqrt(np.mean((ir.transform(s, T) @ n - offset) ** 2)))
    before = float(np.sqrt(np.mean((s @ n - offset) ** 2)))
    print(f"flat, normals {how}: {len(hist)} iterations, ranks {[h[3] for h in hist]}, RMS distance to the plane {before:.3e} -> {rms:.3e}")
    assert len(hist) < 10 and all(h[3] == 3 for h in hist)
    assert rms <= 1e-14 and before > 1e-3


def test_restated_loop_trims_clutter():
    s, t, nrm, kw, T, hist, Ts = restated_alignment("clutter given")
    err = np.abs(T - pr.sheet_motion()).max()
    print(f"clutter, trim 0.6: {len(hist)} iterations, max|T - M| = {err:.3e}, last entry {hist[-1]}")
    assert len(s) == 1500 and len(hist) < 50 and err < 1e-3
    assert all(len(h) == 6 and h[4] == 1500 and h[0] >= 900 and h[5] > 0 for h in hist)


# ---- CPU: argument checks (no device is touched before they run) -----------------------------------------------------------------------
def test_exports():
    import pb3d
    from pb3d import preprocess_helpers as ph
    for n in ("estimate_normals", "estimate_normals_resident", "icp_step_plane_resident", "plane_step_from_sums"):
        assert n in ph.__all__ and getattr(pb3d, n) is getattr(ph, n)
    for n in ("pb3d_point_normals_resident", "pb3d_icp_step_plane_resident"):
        assert n in pb3d._lib.EXPORTED_SYMBOLS


def test_argument_errors_before_device_work(monkeypatch):
    import pb3d
    from pb3d import _lib
    monkeypatch.setattr(_lib, "ctx", lambda: (_ for _ in ()).throw(AssertionError("device touched")))
    rng = np.random.default_rng(2)
    ok = rng.random((40, 3))
    for k in (2, 0, -1, pb3d.eval_helpers.KNN_MAX_K + 1):
        with pytest.raises(ValueError, match="k must be in"):
            pb3d.estimate_normals(ok, k=k)
        with pytest.raises(ValueError, match="k must be in"):
            pb3d.estimate_normals_resident(None, 40, k=k)
    for k in (True, 3.0, "3", None):
        with pytest.raises(ValueError, match="k must be an integer"):
            pb3d.estimate_normals(ok, k=k)
    with pytest.raises(ValueError, match="need at least 20 points"):
        pb3d.estimate_normals(ok[:19])
    with pytest.raises(ValueError, match="need at least 3 points"):
        pb3d.estimate_normals_resident(None, 2, k=3)
    for bad in (np.nan, np.inf):
        p = ok.copy()
        p[7, 1] = bad
        with pytest.raises(ValueError, match="NaN or infinity"):
            pb3d.estimate_normals(p)
    for bad in ((1.0, 2.0), "up", (0.0, np.nan, 0.0), [[0.0, 0.0, 1.0]]):
        with pytest.raises(ValueError, match="orient_towards"):
            pb3d.estimate_normals(ok, orient_towards=bad)
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        pb3d.estimate_normals(ok[:, :2])
    # icp_align
    with pytest.raises(ValueError, match="method"):
        pb3d.icp_align(ok, ok, method="plane")
    with pytest.raises(ValueError, match="with_scale"):
        pb3d.icp_align(ok, ok, method="point_to_plane", with_scale=True)
    for bad in (ok[:39], ok[:, :2], np.zeros((40, 3), complex)):
        with pytest.raises(ValueError, match="target_normals must be"):
            pb3d.icp_align(ok, ok, method="point_to_plane", target_normals=bad)
    nan = ok.copy()
    nan[3, 0] = np.nan
    with pytest.raises(ValueError, match="NaN or infinity"):
        pb3d.icp_align(ok, ok, method="point_to_plane", target_normals=nan)
    with pytest.raises(ValueError, match="only read with"):
        pb3d.icp_align(ok, ok, target_normals=ok)
    with pytest.raises(ValueError, match="k must be in"):
        pb3d.icp_align(ok, ok, method="point_to_plane", normals_k=2)
    with pytest.raises(ValueError, match="need at least 20 points"):
        pb3d.icp_align(ok, ok[:10], method="point_to_plane")
    # the earlier checks still come first on the new path
    with pytest.raises(ValueError, match="trim_fraction"):
        pb3d.icp_align(ok, ok, method="point_to_plane", trim_fraction=0.0)
    with pytest.raises(ValueError, match="target cloud is empty"):
        pb3d.icp_align(ok, np.zeros((0, 3)), method="point_to_plane")
    with pytest.raises(ValueError, match="method"):
        pb3d.icp_align_resident(None, 40, None, 40, method="p2p")
    with pytest.raises(ValueError, match="with_scale"):
        pb3d.icp_align_resident(None, 40, None, 40, method="point_to_plane", with_scale=True)
    # the restated loop on a gate nothing passes
    with pytest.raises(ValueError, match="only 0 point pairs"):
        pr.icp_align(ok + 100.0, ok, max_distance=1.0, target_normals=unit_rows(rng, 40))


def test_c_entries_refuse_bad_arguments():
    """the entries refuse bad fractions, counts, k and null arguments before they look at the context"""
    import pb3d
    L = pb3d._lib
    lib = L.load()
    T = np.eye(4)[:3].reshape(12).copy()
    z = np.zeros(3)
    out = np.zeros(32)
    one = C.c_void_p(out.ctypes.data)       # never dereferenced: every call below is refused first

    def refused(rc, text):
        assert rc == -1 and text in lib.pb3d_last_error().decode(), (rc, lib.pb3d_last_error())

    def plane(src=one, ns=5, tgt=one, nt=4, nrm=one, t=T, md2=-1.0, rho=0.5, c=z, o=one):
        return lib.pb3d_icp_step_plane_resident(None, src, 1, ns, tgt, 1, nt, nrm, None if t is None else L.p_dbl(t), md2, rho,
                                                None if c is None else L.p_dbl(c), o)

    for rho in (0.0, 1.5, float("nan"), float("inf")):
        refused(plane(rho=rho), "trim fraction")
    refused(plane(nt=0), "the target is empty")
    refused(plane(ns=-1), "negative point count")
    refused(plane(ns=1 << 31), "2^31 - 1")
    refused(plane(md2=float("nan")), "NaN")
    refused(plane(t=None), "null argument")
    refused(plane(c=None), "null argument")
    refused(plane(o=None), "null argument")
    refused(plane(src=None), "null buffer")
    refused(plane(tgt=None), "null buffer")
    refused(plane(nrm=None), "null buffer")
    for rho in (0.5, 1.0, -1.0, -0.25, float("-inf")):
        refused(plane(rho=rho), "null context")
    refused(plane(ns=0, nrm=None), "null context")

    def normals(pts=one, n=40, idx=one, k=20, view=None, o=one):
        return lib.pb3d_point_normals_resident(None, pts, 1, n, idx, k, None if view is None else L.p_dbl(np.asarray(view, np.float64)), o)

    for k in (2, 0, -3, 33):
        refused(normals(k=k), "k must be in [3, 32]")
    refused(normals(n=-1), "0 <= n <= 2^31 - 1")
    refused(normals(n=1 << 31), "0 <= n <= 2^31 - 1")
    refused(normals(n=19), "k = 20 neighbours of 19 points")
    refused(normals(view=(0.0, float("nan"), 0.0)), "viewpoint is not finite")
    refused(normals(pts=None), "null buffer")
    refused(normals(idx=None), "null buffer")
    refused(normals(o=None), "null buffer")
    refused(normals(), "null context")
    refused(normals(view=(1.0, 2.0, 3.0)), "null context")
    assert lib.pb3d_point_normals_resident(None, None, 1, 0, None, 3, None, None) == 0          # nothing to do


# ---- GPU: the normals -------------------------------------------------------------------------------------------------------------------
def normals_cloud(n, dtype):
    """n points of the sheet over random (u, v); the float32 cloud is the float64 one rounded"""
    rng = np.random.default_rng(40 + n)
    return np.ascontiguousarray(pr.sheet(rng.uniform(-1.0, 1.0, (n, 2)))[0].astype(dtype))


@gpu
@pytest.mark.parametrize("n", [3, 255, 257, 5000])
def test_estimate_normals_bytes(pb3d_gpu, n):
    views = (None, (3.5, -1.0, 9.0), (3.8, -2.0, 5.1))          # the last lies in the sheet's hollow: both signs occur
    for dtype in ("float64", "float32"):
        pts = normals_cloud(n, dtype)
        for k in (3, 16, 32):
            if k > n:
                with pytest.raises(ValueError, match="need at least"):
                    pb3d_gpu.estimate_normals(pts, k=k)
                continue
            rows = pr.knn_rows(pts, k)
            for view in views:
                got = pb3d_gpu.estimate_normals(pts, k=k, orient_towards=view)
                want = pr.normals(pts, rows, view)
                assert got.dtype == np.float64 and same_bytes(got, want), (n, dtype, k, view, np.flatnonzero((got != want).any(axis=1))[:5])
            if n >= 255:
                flipped = (pr.normals(pts, rows, views[2]) != pr.normals(pts, rows)).any(axis=1)
                assert 0 < flipped.sum() < n


@gpu
def test_estimate_normals_lattice_with_duplicates(pb3d_gpu):
    """an integer lattice (ties in every row, flat neighbourhoods, equal diagonal entries) with every fourth point listed twice and one
    point eight times: rows of coincident points give (1, 0, 0)"""
    g = np.stack(np.meshgrid(np.arange(9.0), np.arange(7.0), np.arange(3.0), indexing="ij"), -1).reshape(-1, 3)
    pts = np.concatenate([g, g[::4], np.tile(g[100], (7, 1))])
    for dtype in ("float64", "float32"):
        p = np.ascontiguousarray(pts.astype(dtype))
        for k in (3, 8, 20):
            rows = pr.knn_rows(p, k)
            for view in (None, (4.0, 3.0, 30.0)):
                assert same_bytes(pb3d_gpu.estimate_normals(p, k=k, orient_towards=view), pr.normals(p, rows, view)), (dtype, k, view)
        n8 = pb3d_gpu.estimate_normals(p, k=8)
        assert same_bytes(n8[100], [1.0, 0.0, 0.0]) and same_bytes(n8[-7:], np.tile([[1.0, 0.0, 0.0]], (7, 1)))


@gpu
def test_normals_resident_entry_and_bad_rows(pb3d_gpu):
    pts = normals_cloud(257, "float64")
    d_p = pb3d_gpu.device.from_numpy(pts)
    try:
        d_n = pb3d_gpu.estimate_normals_resident(d_p, 257, 16)
        try:
            assert same_bytes(d_n.download((257, 3), np.float64), pb3d_gpu.estimate_normals(pts, k=16))
        finally:
            d_n.free()
        # float32 points 4 bytes, rows 4 bytes and normals 8 bytes past an aligned base: the entry reads and writes by element
        p32 = pts.astype(np.float32)
        rows16 = pr.knn_rows(p32, 16).astype(np.int32)
        d_p32 = pb3d_gpu.device.from_numpy(np.concatenate([[np.float32(7.0)], p32.reshape(-1)]))
        d_rows = pb3d_gpu.device.from_numpy(np.concatenate([[np.int32(-9)], rows16.reshape(-1)]))
        d_off = pb3d_gpu.device.DeviceBuffer(8 + 257 * 24)
        try:
            d_off.upload(np.full(1 + 257 * 3, 5.5))
            pb3d_gpu._lib.check(pb3d_gpu._lib.load().pb3d_point_normals_resident(pb3d_gpu._lib.ctx(), d_p32.at(4), 0, 257, d_rows.at(4), 16, None, d_off.at(8)))
            back = d_off.download((1 + 257 * 3,), np.float64)
            assert back[0] == 5.5 and same_bytes(back[1:].reshape(257, 3), pr.normals(p32, rows16))
        finally:
            for b in (d_p32, d_rows, d_off):
                b.free()
        rows = pr.knn_rows(pts, 3).astype(np.int32)
        for bad in (257, -1):
            rows[200, 2] = bad
            d_idx = pb3d_gpu.device.from_numpy(rows)
            d_out = pb3d_gpu.device.DeviceBuffer(257 * 24)
            try:
                rc = pb3d_gpu._lib.load().pb3d_point_normals_resident(pb3d_gpu._lib.ctx(), C.c_void_p(d_p.ptr), 1, 257, C.c_void_p(d_idx.ptr), 3, None,
                                                                      C.c_void_p(d_out.ptr))
                assert rc == -6
                with pytest.raises(IndexError, match="index out of bounds"):
                    pb3d_gpu._lib.check(rc)
            finally:
                d_idx.free()
                d_out.free()
    finally:
        d_p.free()


# ---- GPU: the step ---------------------------------------------------------------------------------------------------------------------
class Clouds:
    """source / target / normals uploaded once; plane() and plain() run the device steps and return their words"""

    def __init__(self, pb3d, src, tgt, nrm, index=True):
        from pb3d.eval_helpers import _cloud
        self.pb3d, self.ph = pb3d, pb3d.preprocess_helpers
        self.src, self.sf = _cloud(src, "source")
        self.tgt, self.tf = _cloud(tgt, "target")
        self.d_s = pb3d.device.from_numpy(self.src) if len(self.src) else pb3d.device.DeviceBuffer(8)
        self.d_t = pb3d.device.from_numpy(self.tgt)
        self.d_n = pb3d.device.from_numpy(np.ascontiguousarray(nrm, np.float64))
        self.d_out = pb3d.device.DeviceBuffer(32 * 8)
        if index:
            self.index()

    def index(self):
        self.ph.icp_index_resident(self.d_t, len(self.tgt), self.tf)

    def set_normals(self, nrm):
        self.d_n.upload(np.ascontiguousarray(nrm, np.float64))

    def plane(self, T, max_dist2, rho, c):
        """the 32 words as uint64; the buffer is filled with ones first, so a word the step does not write shows"""
        self.d_out.upload(np.full(32, 0xFFFFFFFFFFFFFFFF, np.uint64))
        self.ph.icp_step_plane_resident(self.d_s, len(self.src), self.d_t, len(self.tgt), self.d_n, T, max_dist2, rho, c, self.sf, self.tf, out=self.d_out)
        return self.d_out.download((32,), np.uint64)

    def plain(self, T, max_dist2, cp, cq):
        self.ph.icp_step_resident(self.d_s, len(self.src), self.d_t, len(self.tgt), T, max_dist2, cp, cq, self.sf, self.tf, out=self.d_out)
        return self.d_out.download((17,), np.uint64)

    def free(self):
        for b in (self.d_s, self.d_t, self.d_n, self.d_out):
            b.free()


GATES_TRIMS = [(md2, rho) for md2 in (-1.0, 2.0) for rho in (-1.0, 0.6, 1.0)]


def check_steps(pb3d, src, tgt, nrm, T, c, what):
    """ungated and gated, untrimmed and two fractions, then the negated normals: all 32 words against the restatement"""
    cl = Clouds(pb3d, src, tgt, nrm)
    got = []
    try:
        prepared = pr.prepare(src, tgt, nrm, T, c)
        for md2, rho in GATES_TRIMS:
            g = cl.plane(T, md2, rho, c)
            w = pr.words(tr.result(*pr.finish(prepared, md2, rho)))
            assert np.array_equal(g, w), (what, md2, rho, g, w)
            got.append(g)
        cl.set_normals(-np.asarray(nrm))
        for (md2, rho), g in zip(GATES_TRIMS, got):
            assert np.array_equal(cl.plane(T, md2, rho, c), g), (what, "negated normals", md2, rho)
    finally:
        cl.free()
    return got


@gpu
@pytest.mark.parametrize("nt", [97, 5000])
@pytest.mark.parametrize("ns", [1, 255, 257, 65537])
def test_step_words_by_point_count(pb3d_gpu, ns, nt):
    """65 537 = 256 workgroups of 256 and one point: the final pass adds a second partial row in thread 0.  The dtype mix walks with the
    case, so every mix meets a one-workgroup and a many-workgroup step"""
    src, tgt, nrm, T, c = step_case(ns, nt)
    sdt, tdt = [("float64", "float64"), ("float32", "float64"), ("float64", "float32"), ("float32", "float32")][([1, 255, 257, 65537].index(ns) + (nt > 97)) % 4]
    got = check_steps(pb3d_gpu, src.astype(sdt), tgt.astype(tdt), nrm, T, c, (ns, nt, sdt, tdt))
    for (md2, rho), g in zip(GATES_TRIMS, got):
        count, m = int(g[0]), int(g[30])
        assert (m == 0 and g[31] == 0) if rho < 0 else (count >= tr.trim_k(m, rho) and (m == ns if md2 < 0 else m <= ns))
        assert md2 >= 0 or rho == 0.6 or count == ns
    assert ns < 255 or int(got[3][0]) < ns                                  # the gate drops pairs


@gpu
@pytest.mark.parametrize("sdt,tdt", [("float64", "float64"), ("float64", "float32"), ("float32", "float64"), ("float32", "float32")])
def test_step_words_by_dtype(pb3d_gpu, sdt, tdt):
    src, tgt, nrm, T, c = step_case(1000, 500)
    T[:3, :3] *= 1.03                                                       # inexact entries, not rigid
    check_steps(pb3d_gpu, src.astype(sdt), tgt.astype(tdt), nrm, T, c, (sdt, tdt))


@gpu
def test_plane_step_between_plain_steps_and_empty_source(pb3d_gpu):
    src, tgt, nrm, T, c = step_case(4099, 700)
    cl = Clouds(pb3d_gpu, src, tgt, nrm)
    try:
        plain = cl.plain(T, 2.0, c, c)
        assert np.array_equal(plain, np.concatenate([[np.uint64(ir.step(src, tgt, T, 2.0, c, c)[0])], ir.step(src, tgt, T, 2.0, c, c)[1].view(np.uint64)]))
        for rho in (-1.0, 0.6):
            g = cl.plane(T, 2.0, rho, c)
            assert np.array_equal(g, pr.words(pr.step(src, tgt, nrm, T, 2.0, rho, c))), rho
            assert np.array_equal(cl.plain(T, 2.0, c, c), plain)            # same index, the partial-row slot resized in between
        full = cl.plane(T, 2.0, 1.0, c)                                     # term 28 without a trim is the plain step's d2 sum
        assert cl.plane(T, 2.0, -1.0, c)[29] == plain[16] and full[29] == plain[16] and full[0] == full[30] == plain[0]
        assert np.array_equal(cl.plane(T, 2.0, 0.6, c), g)                  # two calls, the same bytes
    finally:
        cl.free()
    # an empty source needs no index and gives thirty-two zero words
    e = Clouds(pb3d_gpu, np.zeros((0, 3)), tgt, nrm, index=False)
    try:
        for rho in (-1.0, 0.5):
            assert not e.plane(T, -1.0, rho, c).any()
    finally:
        e.free()


@gpu
def test_stale_index_is_refused(pb3d_gpu):
    src, tgt, nrm, T, c = step_case(300, 200)
    a = Clouds(pb3d_gpu, src, tgt, nrm)
    try:
        want = pr.words(pr.step(src, tgt, nrm, T, -1.0, -1.0, c))
        assert np.array_equal(a.plane(T, -1.0, -1.0, c), want)
        b = Clouds(pb3d_gpu, src, tgt, nrm)                                 # the same values in another buffer: a's index is retired
        try:
            assert np.array_equal(b.plane(T, -1.0, -1.0, c), want)
            for rho in (-1.0, 0.5):
                with pytest.raises(ValueError, match="built for another target"):
                    a.plane(T, -1.0, rho, c)
        finally:
            b.free()
        a.index()
        assert np.array_equal(a.plane(T, -1.0, -1.0, c), want)
    finally:
        a.free()


# ---- GPU: whole alignments -------------------------------------------------------------------------------------------------------------
def check_history(hist, whist):
    assert len(hist) == len(whist)
    for i, (h, w) in enumerate(zip(hist, whist)):
        assert len(h) == len(w) and h[0] == w[0] and h[3] == w[3] and same_bytes(h[1:3], w[1:3]), (i, h, w)
        assert len(h) == 4 or (h[4] == w[4] and same_bytes([h[5]], [w[5]])), (i, h, w)


ALIGNMENTS = ["sheet given", "sheet estimated", "flat given", "flat estimated", "clutter given", "clutter estimated"]


@gpu
@pytest.mark.parametrize("name", ALIGNMENTS)
def test_alignment_matches_the_restatement(pb3d_gpu, name):
    s, t, nrm, kw, wT, whist, wTs = restated_alignment(name)
    T, hist, Ts = pb3d_gpu.icp_align(s, t, method="point_to_plane", target_normals=nrm, return_history=True, **kw)
    check_history(hist, whist)
    assert len(Ts) == len(wTs) and all(same_bytes(a, b) for a, b in zip(Ts, wTs))
    assert same_bytes(T, wT) and same_bytes(T, Ts[-1])
    assert same_bytes(pb3d_gpu.icp_align(s, t, method="point_to_plane", target_normals=nrm, **kw), wT)     # without the history
    if name.startswith("sheet"):
        assert np.abs(T - pr.sheet_motion()).max() < 1e-3 and len(hist) < 50


@gpu
def test_resident_and_numpy_entries_agree(pb3d_gpu):
    s, t, nrm, kw, wT, whist, wTs = restated_alignment("clutter given")
    dev = pb3d_gpu.device
    s32 = np.ascontiguousarray(s.astype(np.float32))
    d_s, d_s32, d_t, d_n = dev.from_numpy(s), dev.from_numpy(s32), dev.from_numpy(t), dev.from_numpy(nrm)
    try:
        T, hist, Ts = pb3d_gpu.icp_align_resident(d_s, len(s), d_t, len(t), return_history=True, method="point_to_plane", target_normals=d_n, **kw)
        check_history(hist, whist)
        assert same_bytes(T, wT)
        # estimated normals, a float32 source, a gate: the two entries against each other
        a = pb3d_gpu.icp_align_resident(d_s32, len(s), d_t, len(t), max_distance=0.5, max_iterations=4, s_f64=False, method="point_to_plane",
                                        normals_k=12, return_history=True)
        b = pb3d_gpu.icp_align(s32, t, max_distance=0.5, max_iterations=4, method="point_to_plane", normals_k=12, return_history=True)
        assert same_bytes(a[0], b[0]) and a[1] == b[1] and len(a[1]) == 4 and a[1][0][0] < len(s)
        # the default method is untouched by the new arguments' defaults
        assert same_bytes(pb3d_gpu.icp_align(s[:1000], t, max_iterations=3), ir.icp_align(s[:1000], t, max_iterations=3)[0])
    finally:
        for b_ in (d_s, d_s32, d_t, d_n):
            b_.free()
