"""cast_rays, rays_occluded and points_visible_from (pb3d/raycast.py, csrc/raycast.hip) against the brute-force NumPy restatement of
tests/raycast_restate.py, that restatement against closed forms and against render_mesh's restatement, and the bit equality with
render_mesh that the shared face test exists for.  Every comparison of t, face, bary and hit is np.array_equal on the bytes:
include/pb3d.h states the result to the bit, so there is no tolerance."""
import ctypes as C
import functools

import numpy as np
import pytest

import raycast_restate as cr
import render_restate as rr
from test_points_in_mesh import blob_mask

import pb3d
import pb3d.raycast  # noqa: F401  (without the feature every test of this file fails here)

gpu = pytest.mark.gpu
F = np.float64
POISON = 0xA5
PINNED_BLOB_RAY = ((7.0, 5.5, 1.0), (0.0, 1.0, 1.0))        # two faces at t = -0.0 in adjacent layers: the case of the early exit


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint64)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def float_mesh(name, vdtype):
    """(vertices in vdtype, int64 faces) of the octahedron of radius 4 or the 320-face icosphere of radius 3, rotated"""
    v, f = cr.octahedron((0, 0, 0), 4) if name == "octahedron" else cr.icosphere(2)
    scale = 1.0 if name == "octahedron" else 3.0
    v = ((scale * v) @ cr.rotation(21).T + np.array([0.3, -0.2, 0.1])).astype(vdtype)
    return frozen(np.ascontiguousarray(v), f)


def all_rays(verts, faces, seed, rdtype=np.float64):
    """the five families of raycast_restate.families in one list of 2000 rays, in rdtype"""
    fam = cr.families(verts, faces, seed)
    o = np.concatenate([fam[k][0] for k in fam]).astype(rdtype)
    d = np.concatenate([fam[k][1] for k in fam]).astype(rdtype)
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


@functools.lru_cache(maxsize=None)
def float_case(name, vdtype, rdtype, ranged):
    """(origins, directions, vertices, faces, t_min, t_max, restated (t, face, bary, hits, bad))"""
    v, f = float_mesh(name, vdtype)
    o, d = all_rays(v, f, 5, rdtype)
    t_min, t_max = (1e-3, 1.0) if ranged else (0.0, np.inf)
    return frozen(o, d) + (v, f, t_min, t_max, cr.restate(o, d, v, f, t_min, t_max))


# ---- the device entry on arrays ---------------------------------------------------------------------------------------------------------
def device_cast(o, d, verts, faces, t_min=0.0, t_max=np.inf, any_hit=False, bary=True, offset=0, expect=0, force_outputs=False):
    """pb3d_cast_rays_resident on uploaded arrays.  First hit: (t, face, bary or None); any hit: the bool flags.  offset: the byte offset of
    every list and output inside its allocation.  The outputs are poisoned first; expect: the return code awaited, and with another
    one than 0 the outputs come back as they are.  force_outputs: hand d_t, d_face and d_bary to the any-hit mode too"""
    from pb3d import device as dev
    L = pb3d._lib
    o, d, v, fc = (np.ascontiguousarray(a) for a in (o, d, verts, faces))
    assert o.dtype == d.dtype and o.dtype in (np.float32, np.float64) and v.dtype in (np.float32, np.float64) and fc.dtype in (np.int32, np.int64)
    n = len(o)
    ins = [dev.DeviceBuffer(max(1, a.nbytes) + offset) for a in (o, d, v, fc)]
    outs = [dev.DeviceBuffer(max(1, k * n) + offset) for k in (8, 4, 24, 1)]
    try:
        for b, a in zip(ins, (o, d, v, fc)):
            if a.nbytes:
                b.upload(a, offset)
        for b in outs:
            L.check(L.load().pb3d_dev_memset(L.ctx(), C.c_void_p(b.ptr), POISON, b.nbytes))
        first = not any_hit or force_outputs
        rc = L.load().pb3d_cast_rays_resident(L.ctx(), ins[0].at(offset), ins[1].at(offset), int(o.dtype == np.float64), n, ins[2].at(offset),
                                              int(v.dtype == np.float64), len(v), ins[3].at(offset), int(fc.dtype == np.int64), len(fc),
                                              float(t_min), float(t_max), int(any_hit), outs[0].at(offset) if first else None,
                                              outs[1].at(offset) if first else None, outs[2].at(offset) if first and bary else None,
                                              outs[3].at(offset) if any_hit else None)
        assert rc == expect, (rc, L.load().pb3d_last_error())
        if n == 0:
            return np.zeros(0, bool) if any_hit else (np.zeros(0), np.zeros(0, np.int32), np.zeros((0, 3)))
        got = (outs[0].download((n,), F, offset), outs[1].download((n,), np.int32, offset), outs[2].download((n, 3), F, offset),
               outs[3].download((n,), np.uint8, offset))
        if expect != 0:
            return got
        return got[3] != 0 if any_hit else (got[0], got[1], got[2] if bary else None)
    finally:
        for b in ins + outs:
            b.free()


def same(got, ref, what):
    t, fa, ba = got
    assert np.array_equal(bits(t), bits(ref[0])), (what, "t", np.flatnonzero(bits(t) != bits(ref[0]))[:4].tolist())
    assert fa.dtype == np.int32 and np.array_equal(fa, ref[1]), (what, "face", np.flatnonzero(fa != ref[1])[:4].tolist())
    if ba is not None:
        assert np.array_equal(bits(ba), bits(ref[2])), (what, "bary", np.argwhere(bits(ba) != bits(ref[2]))[:4].tolist())


def check(o, d, v, f, t_min=0.0, t_max=np.inf, what="", ref=None):
    """first hit and any hit of the device against the restatement, byte for byte; the restatement"""
    ref = cr.restate(o, d, v, f, t_min, t_max) if ref is None else ref
    same(device_cast(o, d, v, f, t_min, t_max), ref, what)
    assert np.array_equal(device_cast(o, d, v, f, t_min, t_max, any_hit=True), ref[1] >= 0), (what, "any hit")
    return ref


class counted:
    """knob "raycast_stats" for the calls inside"""

    def __enter__(self):
        pb3d._lib.set_tuning("raycast_stats", 1)

    def __exit__(self, *exc):
        pb3d._lib.set_tuning("raycast_stats", 0)


# ---- CPU: the restatement against closed forms ------------------------------------------------------------------------------------------
def test_restatement_box_axis_rays():
    v, f = cr.box((2, 3, 1), (6, 7, 5))         # the side x = 2 is faces 0 = (v0, v1, v3) and 1 = (v0, v3, v2); its diagonal is y - 3 == z - 1
    ys, zs = np.meshgrid(np.arange(3.0, 7.5, 0.5), np.arange(1.0, 5.5, 0.5), indexing="ij")
    y, z = ys.ravel(), zs.ravel()
    for x0 in (0.0, 0.5, -3.0):
        o = np.column_stack([np.full_like(y, x0), y, z])
        t, face, bary, hits, bad = cr.restate(o, np.tile([1.0, 0.0, 0.0], (len(o), 1)), v, f)
        assert np.array_equal(bits(t), bits(2.0 - o[:, 0])) and not bad.any()
        assert np.array_equal(face, np.where(z - 1 >= y - 3, 0, 1))         # on the diagonal both hit: the lower number
        assert np.array_equal(hits[(z - 1 == y - 3) & (y > 3) & (y < 7)], np.full(7, 4))
        assert np.allclose(bary.sum(axis=1), 1.0, atol=1e-15) and (bary >= 0).all()
    # from inside, and backwards from beyond: the far side
    o = np.column_stack([np.full_like(y, 4.0), y, z])
    assert np.array_equal(bits(cr.restate(o, np.tile([1.0, 0.0, 0.0], (len(o), 1)), v, f)[0]), bits(np.full(len(o), 2.0)))
    o[:, 0] = 8.5
    assert np.array_equal(bits(cr.restate(o, np.tile([-2.0, 0.0, 0.0], (len(o), 1)), v, f)[0]), bits(np.full(len(o), 1.25)))     # t in units of |d|
    # a ray in the plane y = 3 of a side: det == 0 there, and the perpendicular sides are hit on their edges
    o1, d1 = np.array([[0.0, 3.0, 2.5]]), np.array([[1.0, 0.0, 0.0]])
    t, face, _, hits, _ = cr.restate(o1, d1, v, f)
    in_plane = np.flatnonzero((v[f][:, :, 1] == 3).all(axis=1))
    assert len(in_plane) == 2
    kx, ky, kz, Sx, Sy, Sz = cr.ray_setup(d1)
    with np.errstate(all="ignore"):
        det = cr.evaluate(v[f[:, 0]], v[f[:, 1]], v[f[:, 2]], o1, (Sx, Sy, Sz), (int(kx[0]), int(ky[0]), int(kz[0])))[3]
    assert (det[in_plane] == 0).all()
    assert t[0] == 2.0 and face[0] == 0 and hits[0] == 2


def test_restatement_integer_octahedron():
    v, f = cr.octahedron((0, 0, 0), 4)
    q = np.arange(-20, 21) / 4.0
    a, b = (g.ravel() for g in np.meshgrid(q, q, indexing="ij"))
    for axis in range(3):                       # along the axes: hit iff |a| + |b| <= 4, at t = 6 - (4 - |a| - |b|), exactly
        o = np.zeros((len(a), 3))
        o[:, axis], o[:, (axis + 1) % 3], o[:, (axis + 2) % 3] = -6.0, a, b
        d = np.zeros((len(a), 3))
        d[:, axis] = 1.0
        t, face, _, hits, _ = cr.restate(o, d, v, f)
        through = np.abs(a) + np.abs(b) <= 4
        assert np.array_equal(face >= 0, through)
        assert np.array_equal(bits(t[through]), bits(2.0 + np.abs(a[through]) + np.abs(b[through])))
        assert not (hits & 1).any()             # all arithmetic is exact here: a closed mesh is hit an even number of times
        t2, face2, _, hits2, _ = cr.restate(o, d, v, f[:, ::-1])
        assert np.array_equal(bits(t2), bits(t)) and np.array_equal(face2, face) and np.array_equal(hits2, hits)
    for d0 in ((1, 1, 0), (1, -1, 0), (-1, 1, 0), (-1, -1, 0), (1, 1, 1)):       # diagonals: ties in |d|, so kz is the first largest
        d0 = np.array(d0, F)
        o = np.column_stack([a, b, np.zeros_like(a)])[np.abs(a) + np.abs(b) <= 6] - 7.0 * d0
        d = np.tile(d0, (len(o), 1))
        t, face, _, hits, _ = cr.restate(o, d, v, f)
        assert (face >= 0).sum() > 100             # (a ray ALONG an edge has det == 0 in both of its faces: no parity is claimed here)
        p = o[face >= 0] + t[face >= 0, None] * d0
        assert np.abs(np.abs(p).sum(axis=1) - 4.0).max() < 1e-12
        t2, face2, _, _, _ = cr.restate(o, d, v, f[:, ::-1])
        assert np.array_equal(bits(t2), bits(t)) and np.array_equal(face2, face)


def test_restatement_minus_zero_at_a_vertex_is_a_hit():
    v, f = cr.octahedron((0, 0, 0), 4)
    dirs = np.array([(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)], F)
    o = np.repeat(v, len(dirs), axis=0)
    d = np.tile(dirs, (len(v), 1))
    t, face, _, hits, _ = cr.restate(o, d, v, f, t_min=0.0)
    assert (face >= 0).all() and (t == 0).all()                 # the origin is a corner of four faces: every one hits at +-0
    assert np.signbit(t).any() and (~np.signbit(t)).any()       # -0.0 >= 0.0 holds; both signs occur
    assert not (cr.restate(o, d, v, f, t_min=1e-300)[0] == 0).any()


def test_restatement_equals_render_restatement():
    """RENDER of the header on the CPU: o = cam, R = identity, d = (sx, sy, 1) gives render_mesh's restated depth and face bit for bit"""
    v, f = rr.icosphere(2, dtype=np.float32)
    cam, view = np.array([1.0, -2.5, -40.0]), dict(f=100.0, cx=37.75, cy=30.25, H=61, W=77)
    depth, face, bary, _, _ = rr.restate(v, f, rr.IDENTITY, cam, **view)
    sx, sy = rr.rays(view["f"], view["cx"], view["cy"], view["H"], view["W"])
    assert np.abs(sx).max() < 1 and np.abs(sy).max() < 1
    d = np.column_stack([sx, sy, np.ones_like(sx)])
    t, fa, ba, _, _ = cr.restate(np.tile(cam, (len(d), 1)), d, v, f, t_min=1e-6)
    assert (fa >= 0).sum() > 500
    assert np.array_equal(bits(t), bits(depth.ravel())) and np.array_equal(fa, face.ravel()) and np.array_equal(bits(ba), bits(bary.reshape(-1, 3)))


def test_python_validation():
    v, f = cr.box((0, 0, 0), (1, 1, 1))
    o, d = np.zeros((2, 3)), np.ones((2, 3))
    with pytest.raises(ValueError):
        pb3d.cast_rays(o, np.ones((3, 3)), v, f)
    with pytest.raises(ValueError):
        pb3d.cast_rays(o, d, v, f, t_min=1.0, t_max=0.5)
    with pytest.raises(ValueError):
        pb3d.cast_rays(o, d, v, f, t_min=-np.inf)
    with pytest.raises(ValueError):
        pb3d.rays_occluded(o, d, v, f, t_max=np.nan)
    with pytest.raises(TypeError):
        pb3d.points_visible_from(o, (0, 0, 5), v, f)            # t_min has no default
    with pytest.raises(IndexError):
        pb3d.cast_rays(o, d, v, f.astype(np.uint32) + 8)
    oo, dd = pb3d.camera_rays((0.0, 0.0, -5.0), (0.0, 0.0, 0.0), 10.0, 1.0, 1.0, 3, 4)
    assert oo.shape == dd.shape == (12, 3) and oo.dtype == dd.dtype == np.float64
    assert np.array_equal(dd[1 * 4 + 1], [0.0, 0.0, 1.0]) and np.array_equal(dd[0], [-0.1, 0.1, 1.0]) and (oo == [0.0, 0.0, -5.0]).all()


# ---- GPU: device against restatement ------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("ranged", [False, True])
@pytest.mark.parametrize("rdtype", [np.float32, np.float64])
@pytest.mark.parametrize("fdtype", [np.int32, np.int64])
@pytest.mark.parametrize("vdtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", ["octahedron", "icosphere"])
def test_float_meshes(pb3d_gpu, name, vdtype, fdtype, rdtype, ranged):
    o, d, v, f, t_min, t_max, ref = float_case(name, vdtype, rdtype, ranged)
    assert 500 < (ref[1] >= 0).sum() < len(o) - 300 and (ref[3] > 1).sum() > 200  # the case holds hits, misses and rays that meet several faces
    check(o, d, v, f.astype(fdtype), t_min, t_max, (name, vdtype, fdtype, rdtype, ranged), ref)


@functools.lru_cache(maxsize=None)
def blob_mesh():
    v, f = pb3d.isosurface(blob_mask().astype(np.float32), 0.5)         # lattice order (a0, a1, a2): no frame conversion enters
    assert len(f) == 1430
    return frozen(np.ascontiguousarray(v), np.ascontiguousarray(f))


@gpu
@pytest.mark.parametrize("ranged", [False, True])
def test_blob_marching_cubes_mesh(pb3d_gpu, ranged):
    """faces, edges and vertices on cell boundaries; the pinned ray hits two faces at t = -0.0, one in each of two adjacent layers"""
    v, f = blob_mesh()
    o, d = all_rays(v, f, 6)
    o, d = np.concatenate([[PINNED_BLOB_RAY[0]], o]), np.concatenate([[PINNED_BLOB_RAY[1]], d])
    ref = check(o, d, v, f, *((1e-3, 1.0) if ranged else (0.0, np.inf)), what=("blob", ranged))
    if not ranged:
        assert ref[1][0] >= 0 and ref[0][0] == 0 and ref[3][0] >= 2, "the pinned ray starts on the surface"
    o32, d32 = o.astype(np.float32), d.astype(np.float32)
    check(o32, d32, v, f, what=("blob float32 rays", ranged))


def first_grid_entries_3d(verts, faces):
    """the (cell, face) entries of the index's FIRST 3-axis grid, before any halving, by the searches' sizing rule (cell edge h with
    h^3 = volume of the box / (nf / 2), ceil(extent / h) cells per axis); for meshes whose box has a positive extent on every axis"""
    v = np.asarray(verts, F)
    f = cr.wrapped(faces, len(v))
    lo, ext = v.min(axis=0), v.max(axis=0) - v.min(axis=0)
    h = np.exp((np.log(ext).sum() - np.log(max(1.0, len(f) / 2.0))) / 3.0)
    n = np.maximum(np.ceil(ext / h), 1.0)
    inv = np.where(n > 1, n / ext, 0.0)
    cell = lambda p: np.clip(np.floor((p - lo) * inv), 0, n - 1)      # noqa: E731
    t = v[f]
    return int((cell(t.max(axis=1)) - cell(t.min(axis=1)) + 1).prod(axis=1).sum())


@gpu
def test_wall_among_small_coarsens(pb3d_gpu):
    v, f = cr.wall_among_small()
    assert first_grid_entries_3d(v, f) > 8 * len(f)             # the first grid breaks the cap of 8 entries per face
    o, d = all_rays(v, f, 7)
    with counted():
        check(o, d, v, f, what="wall")
        stats = pb3d.cast_rays_last()
    assert 0 < stats["entries"] <= 8 * len(f), stats            # so the index halved its cells: the stats show it
    check(o, d, v.astype(np.float32), f.astype(np.int32), 1e-3, 1.0, what="wall float32 ranged")


@gpu
def test_planar_mesh_and_single_triangle(pb3d_gpu):
    """one cell along an axis: rays along that axis, in the plane and oblique (the families hold all three)"""
    quad = (np.array([[0, 0, 2.0], [4, 0, 2], [4, 3, 2], [0, 3, 2], [2, 1.5, 2]]), np.array([[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4]], np.int32))
    tri = (np.array([[0, 0, 0.0], [4, 0, 1], [0, 4, 2]], np.float32), np.array([[0, 1, 2]], np.int64))
    for name, (v, f) in (("planar", quad), ("triangle", tri)):
        o, d = all_rays(v, f, 8)
        if name == "planar":        # in the plane z = 2, from outside the quad: edge-on, det == 0 for every face
            o = np.concatenate([o, [[-1.0, 1.0, 2.0], [-1.0, 1.5, 2.0], [2.0, -2.0, 2.0]]])
            d = np.concatenate([d, [[1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]])
        for rng in ((0.0, np.inf), (1e-3, 1.0)):
            ref = check(o, d, v, f, *rng, what=(name, rng))
        if name == "planar":
            assert (ref[1][-3:] == -1).all()


@gpu
def test_points_visible_from(pb3d_gpu):
    v, f = float_mesh("icosphere", np.float64)
    eye = np.array([9.0, 4.0, -6.0])
    for t_min in (1e-9, 0.0):
        got = pb3d.points_visible_from(v, eye, v, f, t_min)
        ref = cr.restate(v, eye[None, :] - v, v, f, t_min, 1.0)[1] < 0
        assert got.dtype == np.bool_ and np.array_equal(got, ref)
    vis = pb3d.points_visible_from(v, eye, v, f, 1e-9)
    assert 40 < vis.sum() < len(v) - 40                          # the near side is seen, the far side is not
    assert not pb3d.points_visible_from(v, eye, v, f, 0.0).any()     # with t_min = 0 every vertex is occluded by its own faces


@functools.lru_cache(maxsize=None)
def watertight_rays(vdtype):
    """from outside at EVERY vertex and edge midpoint of the closed convex icosphere, three origins each.  The origin stands off the
    target along the outward direction tilted by at most 0.5 (the ray meets the surface at more than 60 degrees from grazing), so the
    exact ray enters the interior; a ray that only touches a silhouette edge in one point may miss by a rounding and is no claim"""
    v, f = float_mesh("icosphere", vdtype)
    verts, mids = cr.mesh_parts(v, f)
    targets = np.tile(np.concatenate([verts, mids]), (3, 1))
    rng = np.random.default_rng(11)
    out = targets - np.array([0.3, -0.2, 0.1])
    out /= np.linalg.norm(out, axis=1, keepdims=True)
    u = rng.normal(size=targets.shape)
    u *= 0.5 / np.linalg.norm(u, axis=1, keepdims=True)
    o = targets + rng.uniform(4.0, 9.0, (len(targets), 1)) * (out + u)
    return frozen(o, targets - o)


@gpu
@pytest.mark.parametrize("vdtype", [np.float32, np.float64])
def test_watertight_on_the_convex_icosphere(pb3d_gpu, vdtype):
    v, f = float_mesh("icosphere", vdtype)
    o, d = watertight_rays(vdtype)
    assert len(o) == 3 * (162 + 3 * 320)
    ref = check(o, d, v, f, what=("watertight", vdtype))
    assert (ref[1] >= 0).all()                                  # ... in the restatement, and so (check) on the device
    t, face = pb3d.cast_rays(o, d, v, f)
    assert (face >= 0).all() and np.isfinite(t).all()


@gpu
def test_identity_with_render_mesh(pb3d_gpu):
    """RENDER of the header: an unrotated camera off the origin, 48 x 64, no pixel with |sx| or |sy| >= 1"""
    v, f = rr.icosphere(2, dtype=np.float32)
    cam = (1.25, -2.5, -30.0)
    view = dict(f=40.0, cx=31.5, cy=23.5, H=48, W=64)
    R = pb3d.render._camera(cam, (cam[0], cam[1], cam[2] + 1.0), view["f"], view["cx"], view["cy"], view["H"], view["W"], 1e-6)[0]
    assert np.array_equal(R, np.eye(3))
    depth, face = pb3d.render_mesh(v, f, cam, (cam[0], cam[1], cam[2] + 1.0), **view)
    sx, sy = rr.rays(view["f"], view["cx"], view["cy"], view["H"], view["W"])
    assert np.abs(sx).max() < 1 and np.abs(sy).max() < 1
    d = np.column_stack([sx, sy, np.ones_like(sx)])
    t, fa = pb3d.cast_rays(np.tile(np.array(cam), (len(d), 1)), d, v, f, t_min=1e-6)
    assert (fa >= 0).sum() > 300 and (fa < 0).sum() > 300
    assert np.array_equal(bits(t), bits(depth.ravel())) and np.array_equal(fa, face.ravel())


@gpu
def test_bad_rays(pb3d_gpu):
    v, f = float_mesh("icosphere", np.float64)
    o = np.tile([0.3, -0.2, 0.1], (8, 1))
    d = np.tile([0.0, 0.0, 1.0], (8, 1))
    d[1] = 0.0
    d[2, 1] = np.nan
    d[3, 0] = np.inf
    o[4, 2] = np.nan
    o[5, 0] = -np.inf
    d[6] = (-0.0, 0.0, -0.0)
    with counted():
        t, face, bary = device_cast(o, d, v, f)
        stats = pb3d.cast_rays_last()
    assert face[0] >= 0 and face[7] == face[0] and (face[1:7] == -1).all()
    assert np.isposinf(t[1:7]).all() and np.array_equal(bits(bary[1:7]), np.zeros((6, 3), np.uint64))
    assert stats["bad_rays"] == 6 and stats["hits"] == 2
    same((t, face, bary), cr.restate(o, d, v, f), "bad rays")
    assert not device_cast(o, d, v, f, any_hit=True)[1:7].any()
    o32, d32 = o.astype(np.float32), d.astype(np.float32)
    same(device_cast(o32, d32, v, f), cr.restate(o32, d32, v, f), "bad float32 rays")


@gpu
def test_argument_cases(pb3d_gpu):
    v, f = float_mesh("octahedron", np.float32)
    o, d = all_rays(v, f, 9)
    o, d = o[::5], d[::5]
    ref = cr.restate(o, d, v, f)
    neg = np.where(np.arange(f.size).reshape(f.shape) % 2 == 0, f - len(v), f)          # negative face indices wrap
    same(device_cast(o, d, v, neg), ref, "negative indices")
    same(device_cast(o, d, v, neg.astype(np.int32)), ref, "negative int32 indices")
    poison_t = np.frombuffer(bytes([POISON]) * 8, F)[0]
    for bad_f, bad_v, rc in ((np.where(np.arange(f.size).reshape(f.shape) == 7, len(v), f), v, -6),
                             (np.where(np.arange(f.size).reshape(f.shape) == 7, -len(v) - 1, f), v, -6),
                             (f, np.where(np.arange(v.size).reshape(v.shape) == 4, np.float32(np.nan), v), -1),
                             (f, np.where(np.arange(v.size).reshape(v.shape) == 4, np.float32(np.inf), v), -1)):
        for any_hit in (False, True):
            t, face, bary, hit = device_cast(o, d, bad_v, bad_f, any_hit=any_hit, expect=rc)
            assert np.array_equal(bits(t), bits(np.full(len(o), poison_t))) and (face.view(np.uint8) == POISON).all()
            assert (bary.view(np.uint8) == POISON).all() and (hit == POISON).all()      # nothing written
    with pytest.raises(IndexError):
        pb3d.cast_rays(o, d, v, np.where(np.arange(f.size).reshape(f.shape) == 7, len(v), f))
    with pytest.raises(ValueError):
        pb3d.rays_occluded(o, d, np.where(np.arange(v.size).reshape(v.shape) == 4, np.float32(np.nan), v), f)
    # outputs of the first-hit mode handed to the any-hit mode, a bad range, a hit buffer in the first-hit mode: refused, nothing written
    t, face, bary, hit = device_cast(o, d, v, f, any_hit=True, force_outputs=True, expect=-1)
    assert (face.view(np.uint8) == POISON).all() and (hit == POISON).all()
    device_cast(o, d, v, f, t_min=2.0, t_max=1.0, expect=-1)
    device_cast(o, d, v, f, t_min=-np.inf, expect=-1)
    # no face: every ray misses; no ray: nothing happens
    t, face, bary = device_cast(o, d, v, f[:0])
    assert np.isposinf(t).all() and (face == -1).all() and not bary.any()
    assert not device_cast(o, d, v, f[:0], any_hit=True).any()
    t, face, bary = device_cast(o, d, v[:0], f[:0])
    assert np.isposinf(t).all() and (face == -1).all()
    t, face = pb3d.cast_rays(o[:0], d[:0], v, f)
    assert t.shape == (0,) and t.dtype == np.float64 and face.shape == (0,) and face.dtype == np.int32
    assert pb3d.rays_occluded(o[:0], d[:0], v, f).shape == (0,)
    assert device_cast(o[:0], d[:0], v, f)[0].shape == (0,)
    # bases aligned to 8 bytes but not to 16
    same(device_cast(o, d, v.astype(np.float64), f, offset=8), ref, "lists and outputs 8 bytes off")
    assert np.array_equal(device_cast(o, d, v.astype(np.float64), f, any_hit=True, offset=8), ref[1] >= 0)
    # the Python forms: dtypes kept, bary on request
    t, face, bary = pb3d.cast_rays(o.astype(np.float32), d.astype(np.float32), v, f.astype(np.int32), return_bary=True)
    same((t, face, bary), cr.restate(o.astype(np.float32), d.astype(np.float32), v, f), "python float32")
    assert np.array_equal(pb3d.rays_occluded(o, d, v, f, 1e-3, 1.0), cr.restate(o, d, v, f, 1e-3, 1.0)[1] >= 0)


@gpu
def test_pruning_is_a_walk(pb3d_gpu):
    """face tests per ray stay below nf / 4: the walk is a walk, not a loop over all faces"""
    for name, (v, f) in (("icosphere", float_mesh("icosphere", np.float64)), ("blob", blob_mesh())):
        o, d = all_rays(v, f, 5)
        with counted():
            device_cast(o, d, v, f)
            stats = pb3d.cast_rays_last()
        per_ray = stats["face_tests"] / len(o)
        print(name, "faces", len(f), "face tests per ray", per_ray, "cells per ray", stats["cells"] / len(o), stats)
        assert 0 < per_ray < len(f) / 4, (name, stats)
        assert stats["hits"] == (cr.restate(o, d, v, f)[1] >= 0).sum() and stats["bad_rays"] == 0
    with pytest.raises(ValueError):
        device_cast(o, d, v, f)
        pb3d.cast_rays_last()                                   # the last call was not counted


@gpu
def test_two_calls_give_the_same_bytes(pb3d_gpu):
    v, f = blob_mesh()
    o, d = all_rays(v, f, 10)
    a, b = device_cast(o, d, v, f), device_cast(o, d, v, f)
    for x, y in zip(a, b):
        assert np.array_equal(bits(x) if x.dtype == F else x, bits(y) if y.dtype == F else y)
    pb3d._lib.set_tuning("raycast_timing", 1)
    try:
        same(device_cast(o, d, v, f), a, "timed")
        ms = pb3d.cast_rays_last(timed=True)
        assert ms[0] > 0 and ms[1] > 0
    finally:
        pb3d._lib.set_tuning("raycast_timing", 0)
    with pytest.raises(ValueError):
        device_cast(o, d, v, f)
        pb3d.cast_rays_last(timed=True)
