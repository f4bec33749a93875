"""pointcloud_to_voxel_grid (reference utils/eval_helpers.py:178-189) on the device: csrc/density.hip behind
pb3d_density_grid_resident, against fixtures captured from the reference's own function (tools/gen_golden_density.py) and against the
NumPy restatement of tests/density_restate.py, which is itself checked against scipy.ndimage.gaussian_filter.  Every comparison is
np.array_equal on the uint32 views of the float32 volumes."""
import ctypes as C
import glob
import os
import types

import numpy as np
import pytest

import density_restate as dr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def fixtures():
    return sorted(os.path.basename(p)[len("density_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "density_*.npz")))


def load_fixture(name):
    with np.load(os.path.join(GOLDEN, f"density_{name}.npz"), allow_pickle=False) as z:
        return z["points"], int(z["grid_size"]), float(z["sigma"]), z["expected"]


# ---- CPU: the restatement against the real filter ------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,sigma", [(8, 1.0), (16, 1.0), (33, 0.7), (32, 2.5), (7, 2.0), (5, 1.5), (16, 0.874), (16, 0.876)])
def test_restatement_is_the_real_gaussian_filter(G, sigma):
    from scipy.ndimage import gaussian_filter
    rng = np.random.default_rng(G * 1000 + int(sigma * 1000))
    vol = np.zeros(G ** 3, np.float32)
    hit = rng.integers(0, G ** 3, 3 * G * G)
    np.add.at(vol, hit, 1)
    vol[hit[:5]] += np.float32(1 << 20)         # large next to small: the order of the float64 additions shows
    vol = vol.reshape(G, G, G)
    for v in (vol, rng.random((G, G, G)).astype(np.float32)):
        assert same_bits(dr.gaussian_filter_restate(v, sigma), gaussian_filter(v, sigma=sigma)), (G, sigma)


def test_radius_steps_between_the_two_sigmas():
    assert dr.gaussian_weights(0.874)[0] == 3 and dr.gaussian_weights(0.876)[0] == 4
    assert dr.gaussian_weights(2.0)[0] == 8 and dr.gaussian_weights(1.5)[0] == 6       # wider than the 7- and 5-voxel axes
    r, w = dr.gaussian_weights(1.0)
    assert r == 4 and len(w) == 9 and np.array_equal(w, w[::-1])


def test_fixtures_exist():
    names = fixtures()
    assert len(names) >= 10
    for name in names:
        pts, G, sigma, exp = load_fixture(name)
        assert G <= 33 and exp.shape == (G, G, G) and exp.dtype == np.float32 and pts.ndim == 2 and pts.shape[1] == 3


@pytest.mark.parametrize("name", fixtures())
def test_fixture_equals_restatement_with_mirror_normalisation(name):
    from pb3d.preprocess_helpers import normalize_preserve_aspect
    pts, G, sigma, exp = load_fixture(name)
    assert same_bits(dr.voxel_grid_restate(pts, G, sigma, normalize=normalize_preserve_aspect), exp)
    assert same_bits(dr.voxel_grid_restate(pts, G, sigma), exp)                 # ... and with the restatement's own normalisation


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", dr.KINDS)
def test_normalize_preserve_aspect(kind, dtype):
    from pb3d.preprocess_helpers import normalize_preserve_aspect
    p = dr.make_cloud(kind, 501, dtype, 11)
    keep = p.copy()
    norm = normalize_preserve_aspect(p)
    assert np.array_equal(p, keep)
    assert norm.dtype == dtype and norm.shape == p.shape
    assert norm[:, 1].max() == 0 and norm[:, 1].min() >= -1     # -1 itself where scale + 1e-8 rounds to scale (float32)
    assert norm[:, [0, 2]].min() == 0 and norm.max() <= 1
    lo = p.min(0)
    scale = (p.max(0) - lo).max()
    assert scale.dtype == dtype
    want = (p - lo) / (scale + dtype(1e-8))             # one rounding per operation, all in the point dtype
    want[:, 1] -= want[:, 1].max()
    assert want.dtype == dtype and np.array_equal(norm, want)
    assert np.array_equal(norm, dr.normalize_preserve_aspect(p))
    # the constant the device kernel subtracts: division is monotone, so the y maximum is the quotient of the y extent
    assert (p[:, 1].max() - lo[1]) / (scale + dtype(1e-8)) == ((p - lo) / (scale + dtype(1e-8)))[:, 1].max()


def test_cloud_kinds_differ_in_their_y_planes():
    planes = {}
    for kind in dr.KINDS:
        idx = dr.voxel_indices(dr.normalize_preserve_aspect(dr.make_cloud(kind, 4097, np.float64, 1)), 16)
        planes[kind] = set(idx[:, 1].tolist())
    assert planes["flat_y"] == {0}
    assert planes["tall_y"] == {0} | set(range(2, 16))     # trunc(-14.x) = -14 -> plane 2; plane 1 would need norm = -1 exactly
    assert planes["cubic"] != planes["flat_y"]


def test_flip_y_axis():
    from pb3d.preprocess_helpers import flip_y_axis
    for dtype in (np.float32, np.float64):
        c = dr.make_cloud("cubic", 100, dtype, 12)
        keep = c.copy()
        f = flip_y_axis(c)
        assert np.array_equal(c, keep) and f is not c and f.dtype == dtype
        y = keep[:, 1]
        assert np.array_equal(f[:, 1], y.max() - (y - y.min())) and np.array_equal(f[:, [0, 2]], keep[:, [0, 2]])
        assert f[np.argmin(y), 1] == y.max() and np.argmin(f[:, 1]) == np.argmax(y)
    lst = [[0.0, 1.0, 2.0], [3.0, 5.0, 4.0]]
    assert np.array_equal(flip_y_axis(lst), [[0.0, 5.0, 2.0], [3.0, 1.0, 4.0]]) and lst[0][1] == 1.0


def test_exported():
    import pb3d
    from pb3d import eval_helpers as eh, preprocess_helpers as ph
    for n in ("pointcloud_to_voxel_grid", "density_grid_resident"):
        assert n in eh.__all__ and getattr(pb3d, n) is getattr(eh, n)
    assert pb3d.normalize_preserve_aspect is ph.normalize_preserve_aspect and pb3d.flip_y_axis is ph.flip_y_axis
    assert "pb3d_density_grid_resident" in pb3d._lib.EXPORTED_SYMBOLS
    assert "pointcloud_to_voxel_grid" in pb3d._PATCH["eval_helpers"]


def test_entry_refuses_bad_arguments():
    """argument checks come before any device work (and before the context is looked at)"""
    from pb3d import _lib
    lib = _lib.load()
    fake = C.c_void_p(0x1000)
    out = C.c_void_p(0x2000)
    w = np.ones(9) / 9

    def call(pts=fake, f64=1, n=5, G=8, wts=w, r=4, o=out):
        return lib.pb3d_density_grid_resident(None, pts, f64, n, G, None if wts is None else _lib.p_dbl(wts), r, o)

    for kw, msg in (({"G": 0}, b"grid_size"), ({"G": -3}, b"grid_size"), ({"G": 1025}, b"grid_size"), ({"r": -1}, b"radius"),
                    ({"r": 65}, b"radius"), ({"n": 0}, b"1 <= n"), ({"n": -2}, b"1 <= n"), ({"n": 1 << 31}, b"2^31 - 1"),
                    ({"pts": None}, b"null buffer"), ({"o": None}, b"null buffer"), ({"wts": None}, b"null buffer"),
                    ({}, b"null context"), ({"G": 1024, "r": 64, "f64": 0}, b"null context"),
                    ({"wts": None, "r": 0}, b"null context"), ({"G": 1, "r": 0}, b"null context")):
        assert call(**kw) == -1, kw
        assert msg in lib.pb3d_last_error(), (kw, lib.pb3d_last_error())


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
SIGMAS = (0, 0.7, 1.0, 1.5, 2.0, 2.5)
COUNTS = (1, 2, 63, 64, 65, 4097, 20000)


def resident_volume(pb3d, d_pts, n, G, sigma, f64):
    d_out = pb3d.density_grid_resident(d_pts, n, G, sigma, f64=f64)
    try:
        return d_out.download((G, G, G), np.float32)
    finally:
        d_out.free()


@pytest.mark.gpu
@pytest.mark.parametrize("G", [1, 2, 3, 5, 7, 8, 16, 33, 64])
def test_sweep_matches_restatement(pb3d_gpu, G):
    """every (sigma, n, dtype) at this grid size, the cloud kinds in rotation; sigma 1.5 .. 2.5 give radii beyond the small axes"""
    from pb3d import device as dev
    case = 0
    for n in COUNTS:
        for dtype in (np.float32, np.float64):
            kind = dr.KINDS[case % 3]
            case += 1
            p = dr.make_cloud(kind, n, dtype, G)
            counts = dr.count_volume(dr.normalize_preserve_aspect(p), G)
            d_p = dev.from_numpy(p)
            try:
                for sigma in SIGMAS:
                    got = resident_volume(pb3d_gpu, d_p, n, G, sigma, dtype == np.float64)
                    assert same_bits(got, dr.finish(counts, sigma)), (G, n, dtype.__name__, kind, sigma)
            finally:
                d_p.free()


@pytest.mark.gpu
@pytest.mark.parametrize("name", fixtures())
def test_fixtures(pb3d_gpu, name):
    pts, G, sigma, exp = load_fixture(name)
    keep = pts.copy()
    got = pb3d_gpu.pointcloud_to_voxel_grid(pts, grid_size=G, sigma=sigma)
    assert got.dtype == np.float32 and same_bits(got, exp) and np.array_equal(pts, keep)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", dr.KINDS)
def test_cloud_shapes(pb3d_gpu, kind, dtype):
    p = dr.make_cloud(kind, 4097, dtype, 21)
    for G, sigma in ((16, 1.0), (33, 0.0), (33, 0.7)):
        assert same_bits(pb3d_gpu.pointcloud_to_voxel_grid(p, G, sigma), dr.voxel_grid_restate(p, G, sigma)), (kind, G, sigma)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_one_voxel_contention(pb3d_gpu, dtype):
    n = 200000
    p = dr.one_voxel_cloud(n, dtype)
    idx = dr.voxel_indices(dr.normalize_preserve_aspect(p), 8)
    assert len(np.unique(idx[:n], axis=0)) == 1 and tuple(idx[0]) == (2, 5, 4)
    raw = pb3d_gpu.pointcloud_to_voxel_grid(p, 8, 0)
    assert raw[2, 5, 4] == n and raw.sum() == n                # the two corners land on faces
    assert same_bits(raw, dr.voxel_grid_restate(p, 8, 0))
    assert same_bits(pb3d_gpu.pointcloud_to_voxel_grid(p, 8, 1.0), dr.voxel_grid_restate(p, 8, 1.0))


@pytest.mark.gpu
def test_saturation_at_two_to_the_24(pb3d_gpu):
    """2^24 + 5 points in one interior cell: np.add.at on float32 stops at 16 777 216, and so does the device value"""
    from pb3d.preprocess_helpers import normalize_preserve_aspect
    n, G = (1 << 24) + 5, 4
    p = np.empty((n + 2, 3), np.float32)
    p[:] = (0.5, 0.2, 0.5)
    p[n], p[n + 1] = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    idx = (normalize_preserve_aspect(p) * (G - 1)).astype(int)          # the reference's expressions, once
    want = np.zeros((G, G, G), np.float32)
    np.add.at(want, (idx[:, 0], idx[:, 1], idx[:, 2]), 1)
    assert tuple(idx[0]) == (1, -2, 1) and want[1, 2, 1] == np.float32(1 << 24)
    dr.zero_faces(want)
    got = pb3d_gpu.pointcloud_to_voxel_grid(p, G, 0)
    assert same_bits(got, want) and got[1, 2, 1] == 16777216.0


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_offset_buffers(pb3d_gpu, dtype):
    """points based one element past an allocation (4 bytes for float32, 8 for float64), the output 4 bytes past one"""
    from pb3d import device as dev
    G, n = 16, 4097
    p = dr.make_cloud("tall_y", n, dtype, 31)
    item = np.dtype(dtype).itemsize
    d_p = dev.DeviceBuffer(p.nbytes + 64)
    d_o = dev.DeviceBuffer(G ** 3 * 4 + 64)
    try:
        d_p.upload(p, byte_offset=item)
        for sigma in (0, 1.0):
            d_o.upload(np.full(G ** 3 + 16, 0x7fc00123, np.uint32))
            ret = pb3d_gpu.density_grid_resident(types.SimpleNamespace(ptr=d_p.ptr + item), n, G, sigma, f64=dtype == np.float64,
                                                 out=types.SimpleNamespace(ptr=d_o.ptr + 4))
            assert ret.ptr == d_o.ptr + 4
            assert same_bits(d_o.download((G, G, G), np.float32, byte_offset=4), dr.voxel_grid_restate(p, G, sigma)), sigma
            guard = d_o.download((G ** 3 + 16,), np.uint32)
            assert guard[0] == 0x7fc00123 and (guard[G ** 3 + 1:] == 0x7fc00123).all()        # nothing written around the volume
    finally:
        d_p.free()
        d_o.free()


@pytest.mark.gpu
def test_scratch_reuse_and_guard(pb3d_gpu):
    """two grid sizes in sequence on one context, then the first again; a labelling call in between changes nothing"""
    from pb3d import device as dev
    p = dr.make_cloud("cubic", 20000, np.float32, 41)
    d_p = dev.from_numpy(p)
    try:
        first = resident_volume(pb3d_gpu, d_p, len(p), 16, 1.0, False)
        other = resident_volume(pb3d_gpu, d_p, len(p), 33, 2.0, False)
        again = resident_volume(pb3d_gpu, d_p, len(p), 16, 1.0, False)
        assert same_bits(first, again) and same_bits(first, dr.voxel_grid_restate(p, 16, 1.0))
        assert same_bits(other, dr.voxel_grid_restate(p, 33, 2.0))
        rng = np.random.default_rng(5)
        grid = np.zeros((24, 20, 24, 3), np.uint8)
        grid[rng.random((24, 20, 24)) < 0.3] = (200, 10, 10)
        labelled = pb3d_gpu.extract_top_k_components(grid, (200, 10, 10), k=2)
        after = resident_volume(pb3d_gpu, d_p, len(p), 16, 1.0, False)
        assert same_bits(first, after)
        assert np.array_equal(labelled, pb3d_gpu.extract_top_k_components(grid, (200, 10, 10), k=2))      # ... in either direction
    finally:
        d_p.free()


@pytest.mark.gpu
def test_api_paths_agree(pb3d_gpu):
    from pb3d import device as dev
    G, sigma = 33, 1.5
    p = dr.make_cloud("tall_y", 4097, np.float64, 51)
    via_numpy = pb3d_gpu.pointcloud_to_voxel_grid(p, G, sigma)
    d_p = dev.from_numpy(p)
    d_o = dev.DeviceBuffer(G ** 3 * 4)
    try:
        assert same_bits(resident_volume(pb3d_gpu, d_p, len(p), G, sigma, True), via_numpy)
        assert pb3d_gpu.density_grid_resident(d_p, len(p), G, sigma, f64=True, out=d_o) is d_o
        assert same_bits(d_o.download((G, G, G), np.float32), via_numpy)
    finally:
        d_p.free()
        d_o.free()
    assert same_bits(via_numpy, dr.voxel_grid_restate(p, G, sigma))
    # the existing dtype rule: integers and float16 become float64, lists too
    ints = np.random.default_rng(6).integers(-50, 50, (500, 3)).astype(np.int16)
    assert same_bits(pb3d_gpu.pointcloud_to_voxel_grid(ints, 8), dr.voxel_grid_restate(ints.astype(np.float64), 8, 1.0))
    assert same_bits(pb3d_gpu.pointcloud_to_voxel_grid(ints.tolist(), 8), dr.voxel_grid_restate(ints.astype(np.float64), 8, 1.0))
    # defaults: grid_size 128, sigma 1.0
    full = pb3d_gpu.pointcloud_to_voxel_grid(p.astype(np.float32))
    assert full.shape == (128, 128, 128) and same_bits(full, dr.voxel_grid_restate(p.astype(np.float32), 128, 1.0))


@pytest.mark.gpu
def test_python_refusals(pb3d_gpu):
    from pb3d import device as dev
    p = dr.make_cloud("cubic", 100, np.float64, 61)
    with pytest.raises(ValueError):
        pb3d_gpu.pointcloud_to_voxel_grid(np.zeros((0, 3)), 8)
    for bad in (np.nan, np.inf, -np.inf):
        q = p.copy()
        q[17, 2] = bad
        with pytest.raises(ValueError, match="NaN or infinity"):
            pb3d_gpu.pointcloud_to_voxel_grid(q, 8)
    for G in (0, -1, 1025):
        with pytest.raises(ValueError, match="grid_size"):
            pb3d_gpu.pointcloud_to_voxel_grid(p, G)
    with pytest.raises(TypeError):
        pb3d_gpu.pointcloud_to_voxel_grid(p, 8.0)
    with pytest.raises(ValueError, match="radius 64"):
        pb3d_gpu.pointcloud_to_voxel_grid(p, 8, sigma=16.2)
    for shape in ((100, 2), (300,), (10, 10, 3)):
        with pytest.raises(ValueError, match=r"\(n, 3\)"):
            pb3d_gpu.pointcloud_to_voxel_grid(np.zeros(shape), 8)
    with pytest.raises(TypeError):
        pb3d_gpu.pointcloud_to_voxel_grid(p.astype(np.complex128), 8)
    # the resident entry: limits before any allocation, and bounds that are not finite after the device pass
    d_p = dev.from_numpy(p)
    q = p.copy()
    q[3, 0] = np.inf
    d_q = dev.from_numpy(q)
    try:
        with pytest.raises(ValueError, match="grid_size"):
            pb3d_gpu.density_grid_resident(d_p, len(p), 2000)
        with pytest.raises(ValueError, match="radius 64"):
            pb3d_gpu.density_grid_resident(d_p, len(p), 8, sigma=100.0)
        with pytest.raises(ValueError, match="1 <= n"):
            pb3d_gpu.density_grid_resident(d_p, 0, 8)
        with pytest.raises(ValueError, match="not finite"):
            pb3d_gpu.density_grid_resident(d_q, len(q), 8)
        # sigma = 16.1 is the widest filter: radius 64
        assert same_bits(resident_volume(pb3d_gpu, d_p, len(p), 8, 16.1, True), dr.voxel_grid_restate(p, 8, 16.1))
    finally:
        d_p.free()
        d_q.free()
