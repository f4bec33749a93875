"""The isosurface of a float32 volume (pb3d_iso_*, csrc/mesh.hip; pb3d.isosurface, pb3d.device.isosurface,
pb3d.get_marching_cubes_mesh) against the NumPy restatement of the rule of include/pb3d.h (tests/iso_restate.py): vertices and faces
bit for bit, dtype and shape included.

The CPU tests state why the GPU tests are not vacuous: on 0/1 volumes the restatement is the binary marching cubes of
tests/mesh_restate.py on lattices that hold every (case, zbits) pair; every float input has the binary restatement's faces on its sign
mask and is closed; the tie input holds t == 0 vertices and zero-area faces, the seam input faces that name vertices of an earlier
256-cube block, the subnormal input subnormal values on crossed edges; and the C entries refuse bad arguments without a device."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import density_restate as dr
import iso_restate as ir
import mesh_restate as mr
import meshify_cases as mc


def exact(got, want):
    assert len(got) == len(want) == 2
    for what, g, w in zip(("verts", "faces"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, g.dtype, w.dtype, g.shape, w.shape)
        gb, wb = (g.view(np.uint32), w.view(np.uint32)) if g.dtype == np.float32 else (g, w)
        assert np.array_equal(gb, wb), f"{what}: {int(np.any(gb != wb, axis=-1).sum())} of {len(w)} rows differ"


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def with_border(vol, value):
    vol = np.array(vol, np.float32)
    vol[[0, -1]] = value
    vol[:, [0, -1]] = value
    vol[:, :, [0, -1]] = value
    return vol


@functools.lru_cache(maxsize=None)
def float_volumes():
    """name -> (volume, levels)"""
    rng = np.random.default_rng(77)
    a = with_border(rng.normal(size=(9, 10, 11)), -1)
    b = with_border(rng.normal(size=(5, 9, 70)), -1)            # 2 208 cubes: nine 256-cube blocks
    out = {"normal_9x10x11": (a, (0.0, 0.37, -0.5)), "normal_5x9x70": (b, (0.0, 0.37, -0.5))}
    # a row longer than two 64-bit words; the vertices on its axis lie on the edges that start at k = 63, 64, 127 and 128
    w = with_border(-0.25 - rng.random((3, 3, 130)), -1)
    for k in (5, 6, 64, 128):
        w[1, 1, k] = 0.5 + rng.random()
    out["word_seam_3x3x130"] = (w, (0.0,))
    # values on the half-integer lattice: many equal the level
    out["ties_9x10x11"] = (with_border(np.round(a * 2) / 2, -1), (0.0, 0.5))
    # magnitudes 1e-30 .. 1e30: level - va and vb - va round in float64
    mag = (rng.choice([-1.0, 1.0], (7, 8, 9)) * 10.0 ** rng.uniform(-30, 30, (7, 8, 9))).astype(np.float32)
    out["magnitudes_7x8x9"] = (with_border(mag, -1), (0.0, 2.5e-7))
    # subnormal float32 values of either sign
    sub = (rng.choice([-1.0, 1.0], (6, 7, 8)) * rng.integers(1, 1 << 22, (6, 7, 8))).astype(np.float32) * np.float32(2.0 ** -149)
    sub = np.ascontiguousarray(sub, np.float32)
    out["subnormal_6x7x8"] = (with_border(sub, -np.float32(2.0 ** -140)), (0.0,))
    # one voxel holds float32(0.1), which is above the float64 level 0.1 and not above float32(0.1)
    t = np.zeros((4, 5, 6), np.float32)
    t[1, 2, 3] = np.float32(0.1)
    t[2, 2, 2] = 1.0
    out["tenth_4x5x6"] = (t, (0.1,))
    return out


FLOAT_CASES = [(name, lv) for name, (_, levels) in float_volumes().items() for lv in levels]
FLOAT_IDS = [f"{n}@{lv}" for n, lv in FLOAT_CASES]


@functools.lru_cache(maxsize=None)
def restated(name, level, divisor=1.0):
    return ir.isosurface(float_volumes()[name][0], level, divisor)


@functools.lru_cache(maxsize=None)
def binary_lattices():
    """name -> 0/1 lattice: every (case, zbits) pair (the corner lattices apart) and the block seams"""
    out = {name: occ for name, (occ, _) in mc.coverage_cases().items() if not name.startswith("corner")}
    out.update(mc.seam_lattices())
    return out


@functools.lru_cache(maxsize=None)
def binary_restated(name):
    return ir.isosurface(binary_lattices()[name].astype(np.float32), 0.5)


def end_to_end_cases():
    return [(12, 300, 1.0, np.float32), (12, 300, 0, np.float64), (16, 2000, 1.0, np.float64), (16, 2000, 0, np.float32),
            (24, 2000, 1.0, np.float32), (24, 2000, 0, np.float64)]


@functools.lru_cache(maxsize=None)
def end_to_end_restated(G, n, sigma, dtype):
    cloud = dr.make_cloud("cubic", n, dtype, 7 * G)
    vol = dr.voxel_grid_restate(cloud, G, sigma)
    return cloud, vol, ir.isosurface(vol, 0.1, G)


# ---- CPU --------------------------------------------------------------------------------------------------------------------------------
def test_binary_volumes_restate_the_binary_marching_cubes():
    """(mask.astype(float32), 0.5) is marching_cubes_binary(mask) in verts and faces, on lattices that hold every (case, zbits) pair"""
    seen = set()
    lattices = dict(binary_lattices())
    lattices.update({f"corner{i}": occ for i, occ in enumerate(mc.corner_lattices())})
    for name, occ in lattices.items():
        v, f = binary_restated(name) if name in binary_lattices() else ir.isosurface(occ.astype(np.float32), 0.5)
        bv, bf, _ = mr.marching_cubes_binary(occ)
        exact((v, f), (bv, bf))
        seen |= mc.case_zbits_pairs(occ)
    assert len(seen) == 254 * 8


@pytest.mark.parametrize("name,level", FLOAT_CASES, ids=FLOAT_IDS)
def test_float_inputs_have_the_sign_masks_faces_and_are_closed(name, level):
    vol = float_volumes()[name][0]
    v, f = restated(name, level)
    mask = ir.inside_mask(vol, level)
    bv, bf, _ = mr.marching_cubes_binary(mask)
    assert len(f) > 0 and np.array_equal(f, bf) and len(v) == len(bv)
    assert ir.border_below(vol, level) and ir.is_closed(f)
    # every edge vertex lies on its lattice edge: within half a step of the binary mesh's midpoint, the centre vertices on it
    assert (np.abs(v.astype(np.float64) - bv) <= 0.5).all()


def test_tie_input_holds_lattice_point_vertices_and_zero_area_faces():
    vol = float_volumes()["ties_9x10x11"][0]
    for level in (0.0, 0.5):
        assert (vol == level).sum() > 20
        v, f, t = ir.isosurface(vol, level, return_t=True)
        assert (t == 0).sum() > 5 and ((t >= 0) | np.isnan(t)).all() and ((t <= 1) | np.isnan(t)).all()
        assert (v[t == 0] == np.floor(v[t == 0])).all()
        assert ir.zero_area_faces(v, f) > 5 and ir.is_closed(f)
        assert len(np.unique(v, axis=0)) < len(v)           # several vertices at one position


def test_seam_inputs_name_vertices_of_an_earlier_block():
    vol = float_volumes()["normal_5x9x70"][0]
    for level in (0.0, 0.37, -0.5):
        refs = mc.seam_references(ir.inside_mask(vol, level), restated("normal_5x9x70", level)[1])
        assert len(refs) == 8 and sum(r > 0 for r in refs) >= 3, refs
    for name, occ in mc.seam_lattices().items():
        n = (occ.shape[0] - 1) * (occ.shape[1] - 1) * (occ.shape[2] - 1)
        refs = mc.seam_references(occ, binary_restated(name)[1])
        assert len(refs) == (n - 1) // 256 and all(r > 0 for r in refs), (name, refs)


def test_word_seam_input_crosses_at_the_word_seams():
    v, _ = restated("word_seam_3x3x130", 0.0)
    on_row = v[(v[:, 0] == 1) & (v[:, 1] == 1)][:, 2]
    assert {63, 64, 127, 128} <= set(np.floor(on_row).astype(int).tolist()) and ((on_row != np.floor(on_row)).all())


def test_subnormal_input_has_subnormal_values_on_crossed_edges():
    vol = float_volumes()["subnormal_6x7x8"][0]
    ends = ir.crossed_edge_values(vol, 0.0)
    tiny = np.finfo(np.float32).tiny
    assert len(ends) > 100 and (ends != 0).all() and (np.abs(ends) < tiny).all()
    v, f, t = ir.isosurface(vol, 0.0, return_t=True)
    assert np.isfinite(v).all() and ((t[~np.isnan(t)] > 0) & (t[~np.isnan(t)] < 1)).all()


def test_magnitude_input_rounds_in_float64():
    vol = float_volumes()["magnitudes_7x8x9"][0].astype(np.float64)
    d = vol[:, :, 1:] - vol[:, :, :-1]
    inexact = (d - vol[:, :, 1:]) != -vol[:, :, :-1]
    assert inexact.sum() > 50 and np.abs(vol).max() > 1e25 and np.abs(vol).min() < 1e-25


def test_level_one_tenth_is_not_rounded_to_float32():
    vol = float_volumes()["tenth_4x5x6"][0]
    assert float(vol[1, 2, 3]) > 0.1 and not vol[1, 2, 3] > np.float32(0.1)
    assert ir.inside_mask(vol, 0.1)[1, 2, 3] and ir.inside_mask(vol, 0.1).sum() == 2
    v, f = restated("tenth_4x5x6", 0.1)
    lone = ir.isosurface(np.where(vol == 1.0, np.float32(0), vol), 0.1)
    assert len(lone[0]) == 6 and len(lone[1]) == 8 and len(v) == 12


def test_end_to_end_inputs_are_closed_meshes_of_a_test_size():
    for G, n, sigma, dtype in end_to_end_cases():
        _, vol, (v, f) = end_to_end_restated(G, n, sigma, dtype)
        assert ir.border_below(vol, 0.1) and ir.is_closed(f) and 100 < len(v) < 20000 and v.max() < 1.0, (G, n, sigma, len(v))
        assert np.array_equal(f, mr.marching_cubes_binary(ir.inside_mask(vol, 0.1))[1])


def test_exported():
    import pb3d
    from pb3d import device, eval_helpers as eh
    for n in ("isosurface", "get_marching_cubes_mesh", "marching_cubes_mesh_resident"):
        assert n in eh.__all__ and getattr(pb3d, n) is getattr(eh, n)
    assert "get_marching_cubes_mesh" in pb3d._PATCH["eval_helpers"] and callable(device.isosurface)
    for n in ("pb3d_iso_count_resident", "pb3d_iso_fill_resident", "pb3d_iso_count", "pb3d_iso_fill", "pb3d_iso_last"):
        assert n in pb3d._lib.EXPORTED_SYMBOLS


def test_entries_refuse_bad_arguments():
    """argument checks come before any device work and before the context is looked at"""
    from pb3d import _lib
    if not os.path.exists(_lib.LIB_PATH):      # fresh checkout: hipcc cross-compiles gfx950 without a GPU
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    fake, out = C.c_void_p(0x1000), C.c_void_p(0x2000)
    nv, nf = C.c_int64(-1), C.c_int64(-1)

    def count(entry, vol=fake, shape=(4, 5, 6), level=0.1, divisor=1.0, pn=C.byref(nv), pm=C.byref(nf)):
        return entry(None, vol, *shape, level, divisor, pn, pm)

    def fill(vol=fake, shape=(4, 5, 6), level=0.1, divisor=1.0, n=3, m=1, v=out, f=out):
        return lib.pb3d_iso_fill_resident(None, vol, *shape, level, divisor, n, m, v, f)

    bad = (({"shape": (1, 5, 6)}, b"at least 2x2x2"), ({"shape": (4, 5, 1)}, b"at least 2x2x2"), ({"shape": (4, 0, 6)}, b"at least 2x2x2"),
           ({"shape": (4, 1 << 24, 6)}, b"< 2^24"), ({"level": np.nan}, b"level must be finite"), ({"level": np.inf}, b"level must be finite"),
           ({"divisor": 0.0}, b"divisor must be finite and > 0"), ({"divisor": -2.0}, b"divisor must be finite and > 0"),
           ({"divisor": np.inf}, b"divisor must be finite and > 0"), ({"divisor": np.nan}, b"divisor must be finite and > 0"),
           ({"vol": None}, b"null volume"), ({}, b"null context"))
    for entry in (lib.pb3d_iso_count_resident, lib.pb3d_iso_count):
        for kw, msg in bad:
            assert count(entry, **kw) == -1, kw
            assert msg in lib.pb3d_last_error(), (kw, lib.pb3d_last_error())
        assert count(entry, pn=None) == -1 and b"null argument" in lib.pb3d_last_error()
        assert count(entry, pm=None) == -1 and b"null argument" in lib.pb3d_last_error()
    assert nv.value == 0 and nf.value == 0            # the counts are cleared before anything is refused
    for kw, msg in bad + (({"n": -1}, b"negative size"), ({"m": -1}, b"negative size")):
        assert fill(**kw) == -1, kw
        assert msg in lib.pb3d_last_error(), (kw, lib.pb3d_last_error())
    assert lib.pb3d_iso_fill(None, 3, 1, out, out) == -1 and b"null context" in lib.pb3d_last_error()
    assert lib.pb3d_iso_last(None, None) == -1 and b"null argument" in lib.pb3d_last_error()


def test_python_refusals_need_no_device():
    from pb3d import device
    for shape in ((4, 5), (4, 5, 6, 1), (1, 5, 6)):
        with pytest.raises(ValueError):
            device.iso_check(shape, 0.1, 1.0)
    for level, divisor in ((np.nan, 1.0), (np.inf, 1.0), (0.1, 0.0), (0.1, -1.0), (0.1, np.inf), (0.1, 1e39), (0.1, 1e-46)):
        with pytest.raises(ValueError):
            device.iso_check((4, 5, 6), level, divisor)
    assert device.iso_check((4, 5, 6), 0.1, 24) == ((4, 5, 6), 0.1, 24.0)


# ---- GPU --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_corner_lattices_match_restatement(pb3d_gpu):
    """one cube, zbits 7, every case"""
    for occ in mc.corner_lattices():
        vol = occ.astype(np.float32)
        exact(pb3d_gpu.isosurface(vol, 0.5), ir.isosurface(vol, 0.5))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(binary_lattices()))
def test_binary_volumes_match_restatement(pb3d_gpu, name):
    """0/1 volumes at level 0.5: every (case, zbits) pair and the block seams; the same mesh as meshify's lattice mesh"""
    occ = binary_lattices()[name]
    got = pb3d_gpu.isosurface(occ.astype(np.float32), 0.5)
    exact(got, binary_restated(name))
    grid = occ.astype(np.uint8)[..., None] * np.uint8(255)
    mv, mf = pb3d_gpu.meshify_colored_voxel_grid(grid)[:2]
    lattice = np.stack([grid.shape[2] - mv[:, 2], mv[:, 1], mv[:, 0]], -1)          # meshify hands out (a2, a1, shape[2] - a0)
    assert np.array_equal(mf, got[1]) and np.array_equal(lattice, got[0])


@pytest.mark.gpu
@pytest.mark.parametrize("name,level", FLOAT_CASES, ids=FLOAT_IDS)
def test_float_volumes_match_restatement(pb3d_gpu, name, level):
    vol = float_volumes()[name][0]
    keep = vol.copy()
    exact(pb3d_gpu.isosurface(vol, level), restated(name, level))
    assert np.array_equal(vol.view(np.uint32), keep.view(np.uint32))


@pytest.mark.gpu
def test_level_out_of_range_is_empty(pb3d_gpu):
    from pb3d import device as dev
    vol = float_volumes()["normal_9x10x11"][0]
    inner = vol.copy()
    inner[0, 0, 0] = vol.max()           # the maximum on the border too
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    for v, level in ((vol, float(vol.max())), (vol, float(vol.max()) + 1.0), (vol, float(vol.min()) - 1.0), (inner, float(inner.max())),
                     (np.full((3, 4, 5), 2.0, np.float32), 1.0), (np.full((3, 4, 5), 2.0, np.float32), 2.0)):
        assert len(ir.isosurface(v, level)[0]) == 0
        exact(pb3d_gpu.isosurface(v, level), empty)
        d_v = dev.from_numpy(v)
        try:
            exact(dev.isosurface(d_v, v.shape, level), empty)
            (dv, df), counts = dev.isosurface(d_v, v.shape, level, download=False)
            assert counts == (0, 0)
            dv.free(); df.free()
        finally:
            d_v.free()
    # the level at the minimum: the minimum itself is outside, everything above it inside
    exact(pb3d_gpu.isosurface(vol, float(vol.min())), ir.isosurface(vol, float(vol.min())))


@pytest.mark.gpu
@pytest.mark.parametrize("divisor", [12, 24, 128])
def test_divisors_match_float32_division(pb3d_gpu, divisor):
    for name in ("normal_9x10x11", "normal_5x9x70"):
        want = restated(name, 0.37, divisor)
        plain = restated(name, 0.37)
        assert np.array_equal(want[0], plain[0] / np.float32(divisor)) and want[0].dtype == np.float32
        if divisor != 128:           # ... and a reciprocal multiply would show
            assert np.any(want[0] != plain[0] * (np.float32(1) / np.float32(divisor)))
        exact(pb3d_gpu.isosurface(float_volumes()[name][0], 0.37, divisor=divisor), want)


@pytest.mark.gpu
def test_dtypes_and_python_refusals(pb3d_gpu):
    vol = float_volumes()["normal_9x10x11"][0]
    want = restated("normal_9x10x11", 0.0)
    exact(pb3d_gpu.isosurface(vol.astype(np.float64), 0.0), want)           # float32 values survive the round trip
    exact(pb3d_gpu.isosurface(np.asfortranarray(vol), 0.0), want)
    exact(pb3d_gpu.isosurface(vol.tolist(), np.float32(0.0), divisor=np.int64(1)), want)
    ints = np.zeros((3, 3, 3), np.int16)
    ints[1, 1, 1] = 2
    exact(pb3d_gpu.isosurface(ints, 1), ir.isosurface(ints.astype(np.float32), 1.0))
    for bad in (np.nan, np.inf, -np.inf):
        q = vol.copy()
        q[4, 5, 6] = bad
        with pytest.raises(ValueError, match="NaN or infinity"):
            pb3d_gpu.isosurface(q, 0.0)
    with pytest.raises(TypeError):
        pb3d_gpu.isosurface(vol.astype(np.complex64), 0.0)
    for shape in ((9, 10), (1, 10, 11), (9, 10, 11, 1)):
        with pytest.raises(ValueError):
            pb3d_gpu.isosurface(np.zeros(shape, np.float32), 0.0)
    for kw in ({"level": np.nan}, {"level": 0.0, "divisor": 0}, {"level": 0.0, "divisor": -3.0}):
        with pytest.raises(ValueError):
            pb3d_gpu.isosurface(vol, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("G,n,sigma,dtype", end_to_end_cases(), ids=[f"G{c[0]}-n{c[1]}-s{c[2]}-{c[3].__name__}" for c in end_to_end_cases()])
def test_get_marching_cubes_mesh(pb3d_gpu, G, n, sigma, dtype):
    cloud, vol, want = end_to_end_restated(G, n, sigma, dtype)
    keep = cloud.copy()
    got_vol = pb3d_gpu.pointcloud_to_voxel_grid(cloud, G, sigma)
    assert np.array_equal(got_vol.view(np.uint32), vol.view(np.uint32))
    got = pb3d_gpu.get_marching_cubes_mesh(cloud, grid_size=G, sigma=sigma, level=0.1)
    exact(got, ir.isosurface(got_vol, 0.1, G))
    exact(got, want)
    assert np.array_equal(cloud, keep) and ir.is_closed(got[1])
    metrics = pb3d_gpu.compute_surface_metrics(*got)
    assert len(metrics) == 3 and all(np.isfinite(x) for x in metrics.values())


@pytest.mark.gpu
def test_get_marching_cubes_mesh_defaults_and_empty(pb3d_gpu):
    cloud = dr.make_cloud("tall_y", 20000, np.float32, 3)
    v, f = pb3d_gpu.get_marching_cubes_mesh(cloud)
    vol = pb3d_gpu.pointcloud_to_voxel_grid(cloud)
    assert vol.shape == (128,) * 3 and v.dtype == np.float32 and f.dtype == np.int32 and len(v) > 1000 and ir.is_closed(f)
    exact((v, f), pb3d_gpu.isosurface(vol, 0.1, divisor=128))           # the restatement is compared at the small sizes above
    assert v.min() >= 0 and v.max() < 1
    exact(pb3d_gpu.get_marching_cubes_mesh(cloud, 16, 1.0, level=1e9), (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)))
    with pytest.raises(ValueError):
        pb3d_gpu.get_marching_cubes_mesh(cloud, grid_size=1)
    with pytest.raises(ValueError):
        pb3d_gpu.get_marching_cubes_mesh(np.zeros((0, 3)), 16)


@pytest.mark.gpu
def test_resident_path(pb3d_gpu):
    """download=False, downloaded, is the host path; count + fill wait for the stream once"""
    from pb3d import device as dev
    vol = float_volumes()["normal_5x9x70"][0]
    want = restated("normal_5x9x70", 0.37, 24)
    d_v = dev.from_numpy(vol)
    try:
        for b in dev.isosurface(d_v, vol.shape, 0.37, 24, download=False)[0]:          # scratch and pool warm
            b.free()
        s0 = dev.sync_count()
        (dv, df), (n, m) = dev.isosurface(d_v, vol.shape, 0.37, 24, download=False)
        assert dev.sync_count() - s0 == 1
        got = dv.download((n, 3), np.float32), df.download((m, 3), np.int32)
        dv.free(); df.free()
        exact(got, want)
        exact(dev.isosurface(d_v, vol.shape, 0.37, divisor=24), want)
        exact(pb3d_gpu.isosurface(vol, 0.37, divisor=24), want)
        # the resident form of get_marching_cubes_mesh leaves the same mesh on the device
        cloud, _, e2e = end_to_end_restated(16, 2000, 1.0, np.float64)
        d_c = dev.from_numpy(cloud)
        try:
            (dv, df), (n, m) = pb3d_gpu.marching_cubes_mesh_resident(d_c, len(cloud), 16, 1.0, 0.1, f64=True)
            got = dv.download((n, 3), np.float32), df.download((m, 3), np.int32)
            dv.free(); df.free()
            exact(got, e2e)
        finally:
            d_c.free()
    finally:
        d_v.free()


@pytest.mark.gpu
def test_pair_guard_refuses_a_stale_fill(pb3d_gpu):
    """a fill after an intervening meshify count, or with other arguments, is refused, not served; and a meshify fill after an
    intervening isosurface count likewise"""
    from pb3d import _lib, device as dev
    lib, ctx = _lib.load(), _lib.ctx()
    vol = float_volumes()["normal_9x10x11"][0]
    want = restated("normal_9x10x11", 0.0)
    grid = (np.random.default_rng(9).random((8, 9, 10, 3)) < 0.4).astype(np.uint8) * np.uint8(200)
    d_v, d_g = dev.from_numpy(vol), dev.from_numpy(grid)
    bufs = []
    try:
        nv, nf, gv, gf = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)

        def iso_count(level=0.0):
            _lib.check(lib.pb3d_iso_count_resident(ctx, _lib._ptr(d_v), *vol.shape, level, 1.0, C.byref(nv), C.byref(nf)))

        def mesh_count():
            _lib.check(lib.pb3d_mesh_count_dev(ctx, _lib._ptr(d_g), *grid.shape[:3], 3, 1, C.byref(gv), C.byref(gf)))

        iso_count()
        n, m = nv.value, nf.value
        assert (n, m) == (len(want[0]), len(want[1]))
        dv, df = dev.DeviceBuffer(n * 12), dev.DeviceBuffer(m * 12)
        bufs += [dv, df]

        def iso_fill(level=0.0, divisor=1.0, n_=n, m_=m, shape=vol.shape):
            return lib.pb3d_iso_fill_resident(ctx, _lib._ptr(d_v), *shape, level, divisor, n_, m_, _lib._ptr(dv), _lib._ptr(df))

        dv.zero(); df.zero()
        # other arguments
        for kw in ({"level": 0.37}, {"divisor": 2.0}, {"n_": n + 1}, {"m_": m - 1}, {"shape": (9, 11, 10)}, {"level": -0.0}):
            assert iso_fill(**kw) == -1, kw
            assert b"arguments differ" in lib.pb3d_last_error(), (kw, lib.pb3d_last_error())
        # an intervening meshify count
        mesh_count()
        assert iso_fill() == -1 and b"overwritten by another call" in lib.pb3d_last_error()
        assert not dv.download((n, 3), np.float32).any() and not df.download((m, 3), np.int32).any()          # nothing was served
        # ... and the other way round
        mv = [dev.DeviceBuffer(gv.value * 12), dev.DeviceBuffer(gf.value * 12), dev.DeviceBuffer(gv.value * 12)]
        bufs += mv
        iso_count()
        rc = lib.pb3d_mesh_fill_dev(ctx, _lib._ptr(d_g), *grid.shape[:3], 3, 1, gv.value, gf.value, _lib._ptr(mv[0]), _lib._ptr(mv[1]),
                                    _lib._ptr(mv[2]), None)
        assert rc == -1 and b"overwritten by another call" in lib.pb3d_last_error()
        # the pending isosurface pair is intact, and a count at another level ends it
        assert iso_fill() == 0
        exact((dv.download((n, 3), np.float32), df.download((m, 3), np.int32)), want)
        iso_count(0.37)
        assert iso_fill() == -1 and b"arguments differ" in lib.pb3d_last_error()
        # the host pair: sizes that do not match the count, then a fill without a count
        hv, hf = C.c_int64(0), C.c_int64(0)
        _lib.check(lib.pb3d_iso_count(ctx, vol.ctypes.data_as(C.c_void_p), *vol.shape, 0.0, 1.0, C.byref(hv), C.byref(hf)))
        assert (hv.value, hf.value) == (n, m)
        v, f = np.zeros((n, 3), np.float32), np.zeros((m, 3), np.int32)
        ptrs = v.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p)
        assert lib.pb3d_iso_fill(ctx, n + 1, m, *ptrs) == -1 and b"sizes do not match the count" in lib.pb3d_last_error()
        assert lib.pb3d_iso_fill(ctx, n, m, *ptrs) == 0
        exact((v, f), want)
        assert lib.pb3d_iso_fill(ctx, n, m, *ptrs) == -1 and b"call pb3d_iso_count first" in lib.pb3d_last_error()
    finally:
        for b in bufs + [d_v, d_g]:
            b.free()


@pytest.mark.gpu
def test_meshify_is_unchanged_by_an_isosurface_call(pb3d_gpu):
    grid, s, want = mc.reference("cube")
    before = pb3d_gpu.meshify_colored_voxel_grid(grid, stride=s)
    vol = float_volumes()["normal_5x9x70"][0]
    exact(pb3d_gpu.isosurface(vol, 0.0), restated("normal_5x9x70", 0.0))
    after = pb3d_gpu.meshify_colored_voxel_grid(grid, stride=s)
    for b, a, w in zip(before, after, want):
        assert b.dtype == a.dtype == w.dtype and b.tobytes() == a.tobytes() == w.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("off_in,off_out", [(4, 0), (0, 4), (12, 4), (4, 12)])
def test_buffers_at_odd_element_offsets(pb3d_gpu, off_in, off_out):
    """the volume, the vertices and the faces as windows into larger buffers, one and three elements off their bases: the kernels
    read and store float32 / int32 by element, so any 4-byte aligned address serves; the bytes around the windows stay"""
    from pb3d import _lib, device as dev
    lib, ctx = _lib.load(), _lib.ctx()
    vol = float_volumes()["word_seam_3x3x130"][0]
    want = restated("word_seam_3x3x130", 0.0, 24)
    n, m = len(want[0]), len(want[1])
    guard = 64
    arena = np.full(vol.size + 2 * guard, np.nan, np.float32)           # NaN slack: outside at any level, loud if it leaked into a vertex
    lo = guard + off_in // 4
    arena[lo:lo + vol.size] = vol.ravel()
    d_in = dev.from_numpy(arena)
    d_v, d_f = dev.DeviceBuffer((3 * n + 2 * guard) * 4), dev.DeviceBuffer((3 * m + 2 * guard) * 4)
    try:
        for b in (d_v, d_f):
            _lib.check(lib.pb3d_dev_memset(ctx, C.c_void_p(b.ptr), 0xA5, b.nbytes))
        p_in, start = d_in.at(lo * 4), guard * 4 + off_out
        nv, nf = C.c_int64(0), C.c_int64(0)
        _lib.check(lib.pb3d_iso_count_resident(ctx, p_in, *vol.shape, 0.0, 24.0, C.byref(nv), C.byref(nf)))
        assert (nv.value, nf.value) == (n, m)
        _lib.check(lib.pb3d_iso_fill_resident(ctx, p_in, *vol.shape, 0.0, 24.0, n, m, d_v.at(start), d_f.at(start)))
        exact((d_v.download((n, 3), np.float32, start), d_f.download((m, 3), np.int32, start)), want)
        for b, rows in ((d_v, n), (d_f, m)):
            raw = b.download((b.nbytes,), np.uint8)
            assert (raw[:start] == 0xA5).all() and (raw[start + rows * 12:] == 0xA5).all()
        assert np.array_equal(d_in.download(arena.shape, np.float32).view(np.uint32), arena.view(np.uint32))
    finally:
        for b in (d_in, d_v, d_f):
            b.free()
