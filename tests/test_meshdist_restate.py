"""CPU: the ground the GPU checks of tests/test_mesh_target.py stand on.  include/pb3d.h states the point-to-mesh distance and the mesh
sampler to the bit; tests/meshdist_restate.py and tests/meshsample_restate.py restate them in NumPy; here the restatements are held
against geometry (dense barycentric samples, segment minima, np.longdouble), and the new C entries' argument checks run without a
device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
sys.path.insert(0, HERE)
import meshdist_restate as mr  # noqa: E402
import meshsample_restate as ms  # noqa: E402

import pb3d  # noqa: E402

M = 40      # barycentric sample: (M + 1)(M + 2) / 2 = 861 points per triangle


def cols(P):
    return tuple(P[..., k] for k in range(3))


def lattice_triangles(rng, n, lim=6):
    """n non-degenerate triangles with integer corners in [-lim, lim]"""
    out = []
    while len(out) < n:
        t = rng.integers(-lim, lim + 1, (3, 3)).astype(np.float64)
        if np.any(np.cross(t[1] - t[0], t[2] - t[0])):
            out.append(t)
    return np.array(out)


def degenerate_triangles(rng, n, lim=6):
    """the four kinds in turn: a = b, b = c, collinear (distinct), all three equal"""
    out = []
    for i in range(n):
        a, b = rng.integers(-lim, lim + 1, (2, 3))
        if np.array_equal(a, b):
            b = a + 1
        kind = i % 4
        if kind == 0:
            t = [a, a, b]
        elif kind == 1:
            t = [a, b, b]
        elif kind == 2:
            k = int(rng.integers(2, 4))
            t = [a, a + k * (b - a), b] if i % 8 < 4 else [a, b, a + k * (b - a)]     # c between a and b, or beyond b
        else:
            t = [a, a, a]
        out.append(np.array(t, np.float64))
    return np.array(out)


def test_restatement_against_dense_barycentric_samples():
    """20 000 lattice triangles, one lattice query each: the restated distance never exceeds the best of 861 barycentric samples (they
    are points of the triangle) beyond rounding, and is not below it by more than the sample spacing (longest edge / 40: every point of
    the triangle is that close to a sample).  Rounding slack: both sides are a few dozen float64 operations on values below
    3 * 15^2, so 64 * 2^-53 * 675 on d2."""
    rng = np.random.default_rng(1)
    T = lattice_triangles(rng, 20000)
    Q = rng.integers(-9, 10, (len(T), 3)).astype(np.float64)
    d2, cp = mr.closest(cols(Q), cols(T[:, 0]), cols(T[:, 1]), cols(T[:, 2]))
    i, j = np.meshgrid(np.arange(M + 1), np.arange(M + 1), indexing="ij")
    keep = i + j <= M
    v, w = i[keep] / M, j[keep] / M
    assert len(v) == 861
    S = T[:, 0, None, :] + (T[:, 1] - T[:, 0])[:, None, :] * v[None, :, None] + (T[:, 2] - T[:, 0])[:, None, :] * w[None, :, None]
    best = ((Q[:, None, :] - S) ** 2).sum(-1).min(1)
    edges = np.stack([T[:, 1] - T[:, 0], T[:, 2] - T[:, 1], T[:, 0] - T[:, 2]], 1)
    spacing = np.sqrt((edges ** 2).sum(-1)).max(1) / M
    slack = 64 * 2.0 ** -53 * 675
    print("largest d2 - sample best:", (d2 - best).max(), " smallest (sqrt(d2) + spacing - sqrt(best)):", (np.sqrt(d2) + spacing - np.sqrt(best)).min())
    assert (d2 <= best + slack).all()
    assert (np.sqrt(d2) >= np.sqrt(best) - spacing - 1e-12).all()
    # the closest point is a point of the triangle: its distance to the query is d2, and it lies in the plane and inside the corners' box
    P = np.stack(cp, 1)
    assert np.array_equal(((Q - P)[:, 0] ** 2 + (Q - P)[:, 1] ** 2) + (Q - P)[:, 2] ** 2, d2)
    n = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])
    off = np.abs(((P - T[:, 0]) * n).sum(1)) / np.sqrt((n ** 2).sum(1))
    print("largest offset of a closest point from its triangle's plane:", off.max())
    assert off.max() <= 1e-13
    assert (P >= T.min(1) - 1e-13).all() and (P <= T.max(1) + 1e-13).all()


def test_degenerate_faces_equal_segment_minimum():
    """a = b, b = c, collinear, a = b = c: d2 equals the minimum over the three segments, computed in np.longdouble, to 1e-12; and the
    shortcut the header warns against (the region walk with 0/0 -> 0) is indeed wrong on some of them"""
    rng = np.random.default_rng(2)
    T = degenerate_triangles(rng, 4000)
    Q = rng.integers(-9, 10, (len(T), 3)).astype(np.float64)
    a, b, c = cols(T[:, 0]), cols(T[:, 1]), cols(T[:, 2])
    assert mr.degenerate(a, b, c).all()
    d2, cp = mr.closest(cols(Q), a, b, c)
    L = np.longdouble
    ref = np.full(len(T), np.inf, L)
    for s0, s1 in ((0, 1), (1, 2), (2, 0)):
        p0, e = T[:, s0].astype(L), (T[:, s1] - T[:, s0]).astype(L)
        dd = (e * e).sum(1)
        t = np.clip(((Q.astype(L) - p0) * e).sum(1) / np.where(dd == 0, 1, dd), 0, 1)
        ref = np.minimum(ref, ((Q.astype(L) - (p0 + e * t[:, None])) ** 2).sum(1))
    err = np.abs(d2.astype(L) - ref).max()
    print("largest |d2 - segment minimum|:", float(err))
    assert err <= 1e-12
    with np.errstate(all="ignore"):
        walk = mr.region_closest(cols(Q), a, b, c)[0]
    print("share of degenerate faces where the bare region walk is wrong:", float((np.abs(walk - d2) > 1e-9).mean()))
    assert (np.abs(walk - d2) > 1e-9).any()


def test_vectorised_brute_force_equals_scalar_loop():
    """bit for bit, on a lattice mesh with degenerate faces (ties between faces everywhere) and on a random one"""
    rng = np.random.default_rng(3)
    T = np.concatenate([lattice_triangles(rng, 40, 3), degenerate_triangles(rng, 12, 3)])
    v = T.reshape(-1, 3)
    f = np.arange(len(v)).reshape(-1, 3)
    for V, Q in ((v, rng.integers(-4, 5, (60, 3)).astype(np.float64)), (v + rng.normal(0, 0.3, v.shape), rng.uniform(-5, 5, (60, 3)))):
        got, want = mr.brute_force(Q, V, f, chunk=7), mr.brute_force_scalar(Q, V, f)
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
    assert (np.diff(np.sort(mr.brute_force(rng.integers(-4, 5, (60, 3)), v, f)[0])) == 0).any()        # ties are present


def sliver_triangles(rng, n, lo, hi):
    """n triangles whose aspect (smallest height over longest edge) is log-uniform in [lo, hi), longest edge 1 .. 200, coordinates
    within 1e3, with 8 queries each"""
    L = rng.uniform(1, 200, n)
    asp = 10 ** rng.uniform(np.log10(lo), np.log10(hi), n)
    flat = np.zeros((n, 3, 3))
    flat[:, 1, 0] = L
    flat[:, 2, 0] = rng.uniform(0, 1, n) * L
    flat[:, 2, 1] = asp * L
    R = np.linalg.qr(rng.normal(size=(n, 3, 3)))[0]
    T = flat @ R.transpose(0, 2, 1) + rng.uniform(-700, 700, (n, 1, 3))
    ab, ac = T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]
    # four queries round the triangle (every region of the walk) ...
    q0 = (T[:, None, 0] + ab[:, None] * rng.uniform(-0.5, 1.5, (n, 4, 1))
          + rng.normal(size=(n, 4, 3)) * (L * 10 ** rng.uniform(-3, 0, n))[:, None, None])
    # ... and four above its interior, 1e-4 .. 1 edge lengths off the plane: the barycentric branch, where a sliver hurts
    s, r = np.sqrt(rng.uniform(0, 1, (n, 4, 1))), rng.uniform(0, 1, (n, 4, 1))
    nrm = np.cross(ab, ac)
    nrm /= np.sqrt((nrm ** 2).sum(1))[:, None]
    q1 = (T[:, None, 0] + ab[:, None] * (s * (1 - r)) + ac[:, None] * (s * r)
          + nrm[:, None] * (L[:, None] * 10 ** rng.uniform(-4, 0, (n, 4)))[:, :, None])
    q = np.concatenate([q0, q1], 1)
    assert np.abs(T).max() <= 1e3 and np.abs(q).max() <= 2e3
    return T, q


def test_accuracy_bound_and_sliver_table():
    """On triangles of aspect >= 1e-3 with coordinates up to 1e3 the restated distance exceeds the same algorithm in np.longdouble by at
    most 4 ulps of the coordinate magnitude (np.spacing(1e3) = 1.14e-13); measured by the author of the arithmetic: 0.41 ulp, the cap
    is ten times that since the draw changes.  Below that aspect the overshoot grows -- Ericson's barycentric quotients lose accuracy
    -- and is printed, not asserted: a stated limitation of the arithmetic.  Measured with this draw (2 000 triangles x 8 queries per
    row; aspect in [row, 10 row); overshoot of the distance in ulps of 1e3, and relative to the distance):

        aspect   1e-1     1e-2     1e-3     1e-4     1e-5     1e-6     1e-7     1e-8
        ulps     1.25     1.07     0.98     7.5      5.7e4    9.3e8    1.4e12   2.2e14
        relative 3.5e-10  2.4e-10  3.1e-10  9.5e-11  3.9e-7   5.4e-3   9.8      4.3e2

    (the relative figure is large where the query is close to the face: half of the queries sit 1e-4 .. 1 edge lengths above the
    face's interior, the barycentric branch; the other half lie round the triangle and reach every region of the walk)
    """
    assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble must be wider than float64 (x86's 80-bit format) to serve as the yardstick"
    rng = np.random.default_rng(4)
    ulp = np.spacing(1e3)
    worst = 0.0
    for k in range(1, 9):
        T, q = sliver_triangles(rng, 2000, 10.0 ** -k, 10.0 ** (1 - k))
        args = (cols(q), cols(T[:, None, 0]), cols(T[:, None, 1]), cols(T[:, None, 2]))
        d64 = np.sqrt(mr.closest(*args)[0])
        dl = np.sqrt(mr.closest(*args, dt=np.longdouble)[0])
        over = (d64.astype(np.longdouble) - dl).astype(np.float64)
        rel = over / np.maximum(dl.astype(np.float64), 1e-300)
        print(f"aspect 1e-{k}: overshoot {over.max() / ulp:9.3g} ulps of 1e3, relative {rel.max():9.3g}; undershoot {-over.min() / ulp:9.3g} ulps")
        if k <= 3:
            worst = max(worst, over.max() / ulp)
    assert worst <= 4.0


def test_closest_points_stay_in_their_face_box_on_needles():
    """The premise under the device search (csrc/meshdist.hip): a face is listed in the cells of its corners' box, and the walk may
    skip a cell only because the cell's box is too far -- so every computed closest point has to lie in its face's box up to the
    walk's margin tol = 1e-12 (|lo| + |hi| + |q|) per axis.  Every (query, face) pair of the giant-and-needles case (aspect 1e-6, where
    the barycentric branch is at its worst) is checked; the largest excursion is printed as a share of tol."""
    import mesh_cases as mc
    v, f, q = mc.giant_and_needles()
    a, b, c = mr.corners(v, f)
    lo = tuple(np.minimum(np.minimum(a[k], b[k]), c[k])[None, :] for k in range(3))
    hi = tuple(np.maximum(np.maximum(a[k], b[k]), c[k])[None, :] for k in range(3))
    worst = 0.0
    for s in range(0, len(q), 128):
        Q = tuple(q[s:s + 128, k][:, None] for k in range(3))
        cp = mr.closest(Q, tuple(x[None, :] for x in a), tuple(x[None, :] for x in b), tuple(x[None, :] for x in c))[1]
        for k in range(3):
            tol = 1e-12 * (abs(v[:, k].min()) + abs(v[:, k].max()) + np.abs(Q[k]))
            worst = max(worst, float((np.maximum(lo[k] - cp[k], cp[k] - hi[k]) / tol).max()))
    print("largest excursion of a closest point from its face's box, in units of tol:", worst)
    assert worst <= 1.0


def test_needle_case_overflows_the_entry_cap():
    """what the GPU test of the coarsening path stands on: on the grid sized from the face count the giant-and-needles case has more
    than 8 entries per face, and two halvings of the cells per axis bring it under the cap (one does not)"""
    import mesh_cases as mc
    v, f, _ = mc.giant_and_needles()
    counts = [mc.index_entries(v, f, h) for h in range(3)]
    print(counts, "cap", 8 * len(f))
    assert counts[0][1] > 8 * len(f) and counts[1][1] > 8 * len(f) and counts[2][1] <= 8 * len(f)
    assert mc.index_entries(v, f[1:2001], 0)[1] <= 8 * 2000                      # the small faces alone need no coarsening


# ---- the sampler's restatement ---------------------------------------------------------------------------------------------------------
def mc_mesh():
    with np.load(os.path.join(GOLD, "surface_mc_f32.npz")) as z:
        return z["vertices"], z["faces"]


def test_sampler_restatement_properties():
    v, f = mc_mesh()
    f = f.copy()
    f[[0, 100, 5000, len(f) - 1], 2] = f[[0, 100, 5000, len(f) - 1], 1]      # zero-area faces at the start, inside and at the end
    A = ms.face_areas(v, f)
    assert (A[[0, 100, 5000, -1]] == 0).all() and (A > 0).sum() == len(f) - 4
    cum = ms.cumulative_areas(A)
    assert (np.diff(cum) >= 0).all() and cum[0] == A[0] and cum[-1] > 0
    assert abs(cum[-1] - A.sum()) <= 1e-12 * A.sum()
    n = 20000
    for seed in (0, 7):
        r = ms.unit_randoms(seed, n)
        assert r.shape == (n, 3) and (r >= 0).all() and (r < 1).all()
        assert np.array_equal(r[5], [(ms.mix(ms.mix(seed) + 15 + j) >> 11) * 2.0 ** -53 for j in range(3)])
        assert 0.49 < r.mean() < 0.51
        pts, face, w = ms.sample(v, f, n, seed)
        assert (A[face] > 0).all()                                          # no zero-area face is chosen
        assert (np.diff(face) >= 0).all()                                   # stratified: consecutive samples, consecutive faces
        dev = np.abs(np.bincount(face, minlength=len(f)) - n * A / cum[-1])
        print("seed", seed, "largest |count - n A / total|:", dev.max())
        assert dev.max() <= 2
        assert (w >= 0).all() and (np.abs(w.sum(1) - 1) <= 2 * 2.0 ** -52).all()      # on the face: a convex combination
        a, b, c = ms.corners(v, f)
        lo, hi = np.minimum(np.minimum(a, b), c)[face], np.maximum(np.maximum(a, b), c)[face]
        assert (pts >= lo - 1e-12).all() and (pts <= hi + 1e-12).all()
    assert ms.mix(0) == 0xE220A8397B1DCDAF                                  # SplitMix64's first output for seed 0


def test_prefix_blocks_cross_seams():
    """the blocked running sum is what the header says at nf = 1, 1024, 1025, 2049: a scalar loop gives the same bits"""
    rng = np.random.default_rng(5)
    for nf in (1, 1023, 1024, 1025, 2049):
        A = rng.uniform(0, 1, nf)
        want, off, nb = np.empty(nf), 0.0, 0
        for s in range(0, nf, 1024):
            acc = None
            for i in range(s, min(nf, s + 1024)):
                acc = A[i] if acc is None else acc + A[i]
                want[i] = off + acc
            off = off + acc
        assert np.array_equal(ms.cumulative_areas(A), want)


# ---- the new entries without a device ----------------------------------------------------------------------------------------------------
def test_c_entries_refuse_bad_arguments():
    """argument checks come before any device work (and before the context is looked at)"""
    from pb3d import _lib
    lib = _lib.load()
    for n in ("pb3d_mesh_dist_resident", "pb3d_mesh_grid_shape", "pb3d_mesh_sample_resident"):
        assert n in _lib.EXPORTED_SYMBOLS
    fake, out = C.c_void_p(0x1000), C.c_void_p(0x2000)

    def dist(q=fake, nq=4, v=fake, nv=8, f=fake, nf=4, d=out, fa=out, cp=out):
        return lib.pb3d_mesh_dist_resident(None, q, 1, nq, v, 0, nv, f, 0, nf, d, fa, cp)

    for kw, msg in (({"nq": -1}, b"0 <= nq"), ({"nq": 1 << 31}, b"2^31 - 1"), ({"nf": 0}, b"at least one face"), ({"nv": 0}, b"at least one face"),
                    ({"nf": -3}, b"negative"), ({"nv": -1}, b"negative"), ({"nf": 1 << 31}, b"2^31 - 1"), ({"nv": 1 << 31}, b"2^31 - 1"),
                    ({"q": None}, b"null buffer"), ({"v": None}, b"null buffer"), ({"f": None}, b"null buffer"), ({"d": None}, b"null buffer"),
                    ({}, b"null context"), ({"fa": None, "cp": None}, b"null context")):
        assert dist(**kw) == -1, kw
        assert msg in lib.pb3d_last_error(), (kw, lib.pb3d_last_error())
    assert dist(nq=0, q=None, nf=0, f=None) == 0

    def samp(v=fake, nv=8, f=fake, nf=4, n=10, seed=3, p=out, fa=out):
        return lib.pb3d_mesh_sample_resident(None, v, 1, nv, f, 1, nf, n, seed, p, fa)

    for kw, msg in (({"n": -1}, b"0 <= n"), ({"n": 1 << 31}, b"2^31 - 1"), ({"nf": 0}, b"at least one face"), ({"nv": 0}, b"at least one face"),
                    ({"nf": -1}, b"negative"), ({"nf": 1 << 31}, b"2^31 - 1"), ({"v": None}, b"null buffer"), ({"f": None}, b"null buffer"),
                    ({"p": None}, b"null buffer"), ({}, b"null context"), ({"fa": None}, b"null context")):
        assert samp(**kw) == -1, kw
        assert msg in lib.pb3d_last_error(), (kw, lib.pb3d_last_error())
    assert samp(n=0, v=None, f=None, nf=0) == 0

    cells, e = (C.c_int64 * 3)(), C.c_int64(0)
    assert lib.pb3d_mesh_grid_shape(None, cells, C.byref(e), None) == -1 and b"null argument" in lib.pb3d_last_error()


def test_python_argument_errors_before_device_work(monkeypatch):
    from pb3d import _lib
    monkeypatch.setattr(_lib, "ctx", lambda: (_ for _ in ()).throw(AssertionError("device touched")))
    rng = np.random.default_rng(0)
    v, P = rng.uniform(0, 1, (10, 3)), rng.uniform(0, 1, (5, 3))
    f = np.array([[0, 1, 2], [2, 3, 4]])
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        pb3d.point_to_mesh_distances(P[:, :2], v, f)
    with pytest.raises(ValueError, match=r"\(m, 3\)"):
        pb3d.point_to_mesh_distances(P, v, f[:, :2])
    with pytest.raises(IndexError):
        pb3d.point_to_mesh_distances(P, v, f.astype(np.float64))
    with pytest.raises(ValueError, match="no faces"):
        pb3d.point_to_mesh_distances(P, v, np.zeros((0, 3), np.int64))
    with pytest.raises(ValueError, match="no faces"):
        pb3d.sample_mesh_points(v, np.zeros((0, 3), np.int64), 5)
    for bad in (np.nan, np.inf):
        w = v.copy()
        w[3, 1] = bad
        with pytest.raises(ValueError, match="NaN or infinity"):
            pb3d.point_to_mesh_distances(P, w, f)
        with pytest.raises(ValueError, match="NaN or infinity"):
            pb3d.point_to_mesh_distances(w, v, f)
        with pytest.raises(ValueError, match="NaN or infinity"):
            pb3d.sample_mesh_points(w, f, 5)
    with pytest.raises(ValueError, match="n must be"):
        pb3d.sample_mesh_points(v, f, -1)
    with pytest.raises(ValueError, match="seed must be"):
        pb3d.sample_mesh_points(v, f, 5, seed=-1)
    with pytest.raises(TypeError):
        pb3d.sample_mesh_points(v, f, 2.5)
    # empty requests need no device either
    assert pb3d.point_to_mesh_distances(np.zeros((0, 3)), v, f).shape == (0,)
    d, fa, cp = pb3d.point_to_mesh_distances(np.zeros((0, 3)), v, f, return_faces=True, return_closest=True)
    assert d.shape == (0,) and fa.dtype == np.int32 and cp.shape == (0, 3)
    pts, fa = pb3d.sample_mesh_points(v, f, 0, return_faces=True)
    assert pts.shape == (0, 3) and pts.dtype == np.float64 and fa.shape == (0,) and fa.dtype == np.int32
