"""voxelize_mesh, grid_overlap_counts and mesh_grid_iou (pb3d/voxelize.py, csrc/voxelize.hip) against the NumPy restatement of
tests/voxelize_restate.py, that restatement against a plain Python loop, and the round trip voxelize(marching_cubes(mask)) == mask that
the tie rule exists for.  Every comparison is np.array_equal: include/pb3d.h states the result to the bit, so there is no tolerance."""
import functools
import os

import numpy as np
import pytest

import mesh_restate as mr
import voxelize_restate as vr

import pb3d
import pb3d.voxelize  # noqa: F401  (without the feature every test of this file fails here)

gpu = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = vr.constructed_cases()
TRIPS = {f"trip{k}": t for k, t in enumerate(vr.ROUND_TRIPS)}
FIXTURE_SHAPE = (32, 32, 40)


# the two obvious wrong tie rules: every edge closed, every edge open
def all_closed(E, pos):
    return E >= 0 if pos else E <= 0


def all_open(E, pos):
    return E > 0 if pos else E < 0


@functools.lru_cache(maxsize=None)
def trip(name):
    """(mask, marching-cubes vertices in lattice order, faces) of a round-trip grid, computed once"""
    shape, density, seed = TRIPS[name]
    mask = vr.random_mask(shape, density, seed)
    v, f, _ = mr.marching_cubes_binary(mask)
    for a in (mask, v, f):
        a.setflags(write=False)
    return mask, v, f


@functools.lru_cache(maxsize=None)
def trip_meshify(name):
    """(RGB grid, vertices in meshify's frame, faces): the same mask coloured at random, through mesh_restate.meshify"""
    mask = trip(name)[0]
    grid = np.random.default_rng(11).integers(1, 256, mask.shape + (3,), dtype=np.uint8) * mask[..., None].astype(np.uint8)
    v, f = mr.meshify(grid)[:2]
    for a in (grid, v, f):
        a.setflags(write=False)
    return grid, v, f


@functools.lru_cache(maxsize=None)
def fixture(name):
    """a committed surface scaled into FIXTURE_SHAPE: its longest side spans 29 voxels from (1.5, 1.25, 1.125), in the fixture's dtype"""
    with np.load(os.path.join(GOLD, f"surface_{name}.npz")) as z:
        v, f = np.ascontiguousarray(z["vertices"]), np.ascontiguousarray(z["faces"])
    lo, hi = v.min(axis=0), v.max(axis=0)
    v = ((v - lo) * v.dtype.type(29.0 / float((hi - lo).max())) + np.array([1.5, 1.25, 1.125], v.dtype)).astype(v.dtype)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


def case(name):
    """(verts, faces, shape, keyword arguments)"""
    if name.startswith("fixture/"):
        return (*fixture(name[8:]), FIXTURE_SHAPE, {})
    if name.startswith("trip"):
        if name.endswith("/meshify"):
            grid, v, f = trip_meshify(name[:-8])
            return v, f, grid.shape[:3], dict(frame="meshify")
        mask, v, f = trip(name)
        return v, f, mask.shape, {}
    return CASES[name]


@functools.lru_cache(maxsize=None)
def want(name):
    """the restatement of one case, computed once and shared"""
    v, f, shape, kw = case(name)
    occ, stats = vr.restate(v, f, shape, **kw)
    occ.setflags(write=False)
    return occ, stats


def same(got, ref, what):
    assert got.dtype == np.uint8 and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    if not np.array_equal(got, ref):
        bad = np.argwhere(got != ref)
        raise AssertionError((what, "first differing voxel", bad[0].tolist(), "voxels differing", len(bad), "of", ref.size))


# ---- CPU: the rules themselves ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(set(CASES) - {"many_columns"}))        # that one is 17 M voxels of the same rules
def test_restatement_equals_loop(name):
    v, f, shape, kw = CASES[name]
    occ, stats = vr.loop(v, f, shape, **kw)
    same(occ, want(name)[0], name)
    assert stats == want(name)[1]


def test_pinned_box():
    occ, stats = want("pinned_box")
    ref = np.zeros((9, 10, 8), np.uint8)
    ref[3:7, 3:7, 1:5] = 1
    same(occ, ref, "pinned box")
    # the eight flat faces are the box's four sides parallel to the ray
    assert stats == dict(crossings=32, occupied=64, open_columns=0, flat_faces=8)


@pytest.mark.parametrize("axis", (0, 1, 2))
@pytest.mark.parametrize("name", sorted(TRIPS))
def test_round_trip_restated(name, axis):
    """restate(marching_cubes_binary(mask)) == mask with the ray along each axis: the mesh's columns and the grid's axes permuted alike"""
    mask, v, f = trip(name)
    perm = [a for a in range(3) if a != axis] + [axis]
    occ, stats = vr.restate(v[:, perm], f, tuple(mask.shape[a] for a in perm))
    same(occ.transpose(np.argsort(perm)), mask.astype(np.uint8), (name, axis))
    assert stats["open_columns"] == 0 and stats["occupied"] == int(mask.sum())


@pytest.mark.parametrize("name", sorted(TRIPS))
def test_round_trip_restated_meshify_frame(name):
    grid, v, f = trip_meshify(name)
    assert v.dtype == np.float32
    same(want(name + "/meshify")[0], np.any(grid > 0, axis=-1).astype(np.uint8), name)


def test_wrong_tie_rules_break_the_round_trip():
    """the teeth: with every edge closed, or every edge open, the 12 x 11 x 13 mesh does not give its mask back"""
    mask, v, f = trip("trip1")
    assert mask.shape == (12, 11, 13)
    for rule in (all_closed, all_open):
        occ, _ = vr.restate(v, f, mask.shape, accept=rule)
        assert np.count_nonzero(occ != mask) > 0, rule.__name__


def test_argument_errors_need_no_device():
    v, f = CASES["pinned_box"][:2]
    ok = (9, 10, 8)
    for shape in ((9, 10), (9, 10, 0), (9, 10, -1), (9.0, 10, 8), (True, 10, 8), 5, (2 ** 11, 2 ** 10, 2 ** 10)):
        with pytest.raises(ValueError):
            pb3d.voxelize_mesh(v, f, shape)
    for vs in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="voxel_size"):
            pb3d.voxelize_mesh(v, f, ok, voxel_size=vs)
    for origin in ((0, 0), (0, 0, float("nan")), (0, float("inf"), 0)):
        with pytest.raises(ValueError, match="origin"):
            pb3d.voxelize_mesh(v, f, ok, origin=origin)
    for frame in ("world", None, 1):
        with pytest.raises(ValueError, match="frame"):
            pb3d.voxelize_mesh(v, f, ok, frame=frame)
    with pytest.raises(ValueError, match="depth"):
        pb3d.voxelize_mesh(v, f, ok, frame="meshify", depth=float("nan"))
    for value in (256, -1, (1, 2), (1, 2, 300), 1.5, (1.0, 2.0, 3.0)):
        with pytest.raises(ValueError, match="value"):
            pb3d.voxelize_mesh(v, f, ok, value=value)
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        pb3d.voxelize_mesh(v[:, :2], f, ok)
    with pytest.raises(ValueError, match=r"\(m, 3\)"):
        pb3d.voxelize_mesh(v, f[:, :2], ok)
    with pytest.raises(IndexError):
        pb3d.voxelize_mesh(v, f.astype(np.float64), ok)
    with pytest.raises(IndexError):
        pb3d.voxelize_mesh(v, f.astype(np.uint32) + np.uint32(len(v)), ok)
    with pytest.raises(IndexError):
        pb3d.voxelize_mesh(np.zeros((0, 3)), f, ok)
    with pytest.raises(ValueError, match="differ in shape"):
        pb3d.grid_overlap_counts(np.zeros((2, 3, 4), np.uint8), np.zeros((2, 3, 5, 3), np.uint8))
    with pytest.raises(TypeError):
        pb3d.grid_overlap_counts(np.zeros((2, 3, 4), np.float32), np.zeros((2, 3, 4), np.uint8))
    with pytest.raises(ValueError, match="shape"):
        pb3d.grid_overlap_counts(np.zeros((2, 3), np.uint8), np.zeros((2, 3), np.uint8))
    with pytest.raises(ValueError, match="shape"):
        pb3d.mesh_grid_iou(v, f, np.zeros((2, 3, 4, 2), np.uint8))


# ---- GPU: device == restatement, bytes and stats -------------------------------------------------------------------------------------
def run(pb, name, vdtype=None, fdtype=None, **more):
    v, f, shape, kw = case(name)
    v = v if vdtype is None else v.astype(vdtype)
    f = f if fdtype is None else f.astype(fdtype)
    return pb.voxelize_mesh(v, f, shape, return_stats=True, **kw, **more)


def check(pb, name, **how):
    occ, stats = run(pb, name, **how)
    same(occ, want(name)[0], (name, how))
    assert stats == want(name)[1], (name, how, stats, want(name)[1])


@gpu
@pytest.mark.parametrize("name", sorted(TRIPS))
def test_round_trip_lattice_frame(pb3d_gpu, name):
    mask = trip(name)[0]
    check(pb3d_gpu, name, vdtype=np.float32, fdtype=np.int32)
    check(pb3d_gpu, name, vdtype=np.float64, fdtype=np.int64)
    same(want(name)[0], mask.astype(np.uint8), name)


@gpu
@pytest.mark.parametrize("name", sorted(TRIPS))
def test_round_trip_meshify_frame(pb3d_gpu, name):
    check(pb3d_gpu, name + "/meshify", fdtype=np.int64)
    check(pb3d_gpu, name + "/meshify", vdtype=np.float64, fdtype=np.int32)


@gpu
@pytest.mark.parametrize("fdtype", (np.int32, np.int64))
def test_wrapped_negative_indices(pb3d_gpu, fdtype):
    mask, v, f = trip("trip3")
    neg = np.random.default_rng(5).random(f.shape) < 0.5
    wrapped = np.where(neg, f.astype(np.int64) - len(v), f).astype(fdtype)
    assert wrapped.min() < 0 <= wrapped.max()
    occ, stats = pb3d_gpu.voxelize_mesh(v, wrapped, mask.shape, return_stats=True)
    same(occ, mask.astype(np.uint8), "wrapped")
    assert stats == want("trip3")[1]


@gpu
@pytest.mark.parametrize("name", ("pinned_box", "octahedron", "octahedron_box"))
def test_ties(pb3d_gpu, name):
    check(pb3d_gpu, name)
    check(pb3d_gpu, name, vdtype=np.float32, fdtype=np.int32)


@gpu
@pytest.mark.parametrize("name", ("sphere_f32", "sphere_f64", "sphere_scaled", "fixture/mc_f32", "fixture/sphere_f64"))
def test_irrational_coordinates(pb3d_gpu, name):
    assert want(name)[1]["occupied"] > 0 and want(name)[1]["open_columns"] == 0
    check(pb3d_gpu, name)


@gpu
@pytest.mark.parametrize("n2", vr.WORD_DEPTHS)
def test_word_boundaries(pb3d_gpu, n2):
    check(pb3d_gpu, f"words_{n2}")


@gpu
@pytest.mark.parametrize("name", ("tall_2100", "tall_4133"))
def test_columns_longer_than_a_wavefront(pb3d_gpu, name):
    """more than 64 dwords per column: the scan's other path, a wavefront per column with a carry between its chunks"""
    assert want(name)[1]["occupied"] > 2048
    check(pb3d_gpu, name)
    v, f, shape, kw = CASES[name]
    same(pb3d_gpu.voxelize_mesh(v, f, shape, value=(1, 2, 3), **kw), want(name)[0][..., None] * np.array([1, 2, 3], np.uint8), name)


@gpu
@pytest.mark.parametrize("name", ("slabs", "twice"))
def test_contention(pb3d_gpu, name):
    check(pb3d_gpu, name)
    if name == "twice":
        v, f, shape, _ = CASES[name]
        once = vr.restate(v, f[:len(f) // 2], shape)[1]
        occ, stats = want(name)
        assert not occ.any() and stats["crossings"] == 2 * once["crossings"] > 0


@gpu
def test_imbalance(pb3d_gpu):
    """a box of 12 triangles over all 40 x 40 columns beside 20 000 triangles of a column or two, in one face list"""
    check(pb3d_gpu, "imbalance")


@gpu
def test_more_wide_faces_than_workgroups(pb3d_gpu):
    assert len(CASES["many_wide"][1]) > 256 * 8         # the workgroups that walk listed faces: 8 per CU
    check(pb3d_gpu, "many_wide")


@gpu
def test_more_faces_than_one_round_of_lanes(pb3d_gpu):
    """1.1 M faces, more than the capped grid of the lane pass takes in one round (16 workgroups of 256 lanes on each of 256 CUs).  The
    added faces repeat one vertex: area == 0, so by the rule they add nothing but their number to the flat faces, wherever they stand"""
    v, f, shape, kw = CASES["imbalance"]
    n, half = 1_100_000, len(f) // 2
    assert n > 16 * 256 * 256
    faces = np.concatenate([f[:half], np.full((n, 3), 5, np.int64), f[half:]]).astype(np.int32)
    occ, stats = pb3d_gpu.voxelize_mesh(v, faces, shape, return_stats=True, **kw)
    same(occ, want("imbalance")[0], "imbalance + flat faces")
    ref = dict(want("imbalance")[1])
    ref["flat_faces"] += n
    assert stats == ref


@gpu
def test_more_columns_than_one_round_of_wavefronts(pb3d_gpu):
    """130 x 127 x 1025: above the other grids of this file because the scan's capped grid (16 workgroups on each of 256 CUs, a column
    of 33 dwords per wavefront) starts its second round only past 16 384 columns; the overlap sweep's begins past 524 288 voxels"""
    v, f, shape, kw = CASES["many_columns"]
    assert shape[0] * shape[1] > 16 * 256 * 4
    occ = want("many_columns")[0]
    check(pb3d_gpu, "many_columns")
    rgb = pb3d_gpu.voxelize_mesh(v, f, shape, value=(3, 0, 250), **kw)
    same(rgb, occ[..., None] * np.array([3, 0, 250], np.uint8), "many_columns rgb")
    other = np.roll(occ, 7, axis=0)
    ref = (int((occ & other).sum()), int(occ.sum()), int(other.sum()))
    assert pb3d_gpu.grid_overlap_counts(rgb, other) == ref


@gpu
def test_mesh_partly_outside(pb3d_gpu):
    occ = want("outside")[0]
    assert all(occ.take(i, axis=a).any() for a in range(3) for i in (0, -1))       # it leaves the grid on every side
    check(pb3d_gpu, "outside")


@gpu
@pytest.mark.parametrize("name", ("triangle", "hemisphere"))
def test_open_mesh(pb3d_gpu, name):
    assert want(name)[1]["open_columns"] > 0
    check(pb3d_gpu, name)


@gpu
def test_no_faces(pb3d_gpu):
    v = CASES["pinned_box"][0]
    for verts in (v, np.zeros((0, 3), np.float32)):
        occ, stats = pb3d_gpu.voxelize_mesh(verts, np.zeros((0, 3), np.int32), (5, 6, 33), return_stats=True)
        same(occ, np.zeros((5, 6, 33), np.uint8), "nf = 0")
        assert stats == dict(crossings=0, occupied=0, open_columns=0, flat_faces=0)


@gpu
def test_bad_index_leaves_the_output_untouched(pb3d_gpu):
    from pb3d import device as dev
    v, f, shape, _ = CASES["pinned_box"]
    v32, n = v.astype(np.float32), int(np.prod(shape))
    for bad in (len(v), -len(v) - 1):
        fb = f.astype(np.int32)
        fb[7, 1] = bad
        d_v, d_f, d_out = dev.from_numpy(v32), dev.from_numpy(fb), dev.from_numpy(np.full(n, 0xAB, np.uint8))
        try:
            with pytest.raises(IndexError):
                pb3d_gpu.voxelize_mesh_resident(d_v, len(v), d_f, len(f), shape, out=d_out)
            assert np.array_equal(d_out.download((n,)), np.full(n, 0xAB, np.uint8))
        finally:
            for b in (d_v, d_f, d_out):
                b.free()
        with pytest.raises(IndexError):
            pb3d_gpu.voxelize_mesh(v, fb, shape)


@gpu
@pytest.mark.parametrize("bad", (np.nan, np.inf, -np.inf))
def test_non_finite_vertex(pb3d_gpu, bad):
    v, f, shape, _ = CASES["pinned_box"]
    for dtype in (np.float32, np.float64):
        vb = v.astype(dtype)
        vb[5, 2] = bad
        with pytest.raises(ValueError, match="not finite"):
            pb3d_gpu.voxelize_mesh(vb, f, shape)


@gpu
def test_label_and_rgb_values(pb3d_gpu):
    for name in ("octahedron_box", "words_33", "words_64"):      # the last: 16-byte stores
        v, f, shape, kw = CASES[name]
        occ = want(name)[0]
        same(pb3d_gpu.voxelize_mesh(v, f, shape, value=7, **kw), occ * np.uint8(7), (name, "label"))
        rgb, stats = pb3d_gpu.voxelize_mesh(v, f, shape, value=(200, 0, 31), return_stats=True, **kw)
        same(rgb, occ[..., None] * np.array([200, 0, 31], np.uint8), (name, "rgb"))
        assert stats == want(name)[1]


@gpu
def test_resident_with_out(pb3d_gpu):
    from pb3d import device as dev
    v, f, shape, kw = CASES["sphere_scaled"]
    n = int(np.prod(shape))
    d_v, d_f, d_out = dev.from_numpy(v), dev.from_numpy(f), dev.from_numpy(np.full(n, 0xCD, np.uint8))
    try:
        got, stats = pb3d_gpu.voxelize_mesh_resident(d_v, len(v), d_f, len(f), shape, return_stats=True, verts_f64=True, faces_i64=True,
                                                     out=d_out, **kw)
        assert got is d_out
        same(d_out.download(shape), want("sphere_scaled")[0], "resident")
        assert stats == want("sphere_scaled")[1]
    finally:
        for b in (d_v, d_f, d_out):
            b.free()


@gpu
@pytest.mark.parametrize("value", (1, (9, 8, 7)))
def test_output_at_an_odd_address(pb3d_gpu, value):
    """n2 = 64 into a buffer that starts 3 bytes into an allocation: the byte-store path, and nothing outside the grid is written"""
    from pb3d import device as dev
    v, f, shape, kw = CASES["words_64"]
    ch = np.size(value)
    n = int(np.prod(shape)) * ch
    d_v, d_f, d_buf = dev.from_numpy(v), dev.from_numpy(f), dev.from_numpy(np.full(n + 8, 0xEE, np.uint8))
    try:
        pb3d_gpu.voxelize_mesh_resident(d_v, len(v), d_f, len(f), shape, value=value, verts_f64=True, faces_i64=True, out=d_buf.at(3), **kw)
        got = d_buf.download((n + 8,))
        assert np.array_equal(got[:3], np.full(3, 0xEE, np.uint8)) and np.array_equal(got[n + 3:], np.full(5, 0xEE, np.uint8))
        ref = want("words_64")[0][..., None] * np.atleast_1d(np.array(value, np.uint8))
        same(got[3:n + 3].reshape(ref.shape), ref, "odd address")
    finally:
        for b in (d_v, d_f, d_buf):
            b.free()


@gpu
def test_two_runs_give_equal_bytes(pb3d_gpu):
    a, sa = run(pb3d_gpu, "imbalance")
    b, sb = run(pb3d_gpu, "imbalance")
    assert np.array_equal(a, b) and sa == sb


@gpu
def test_grid_overlap_counts(pb3d_gpu):
    rng = np.random.default_rng(3)
    shape = (7, 9, 11)                                  # 693 voxels: no multiple of 64
    a = (rng.random(shape) < 0.4).astype(np.uint8) * rng.integers(1, 256, shape, dtype=np.uint8)
    b = rng.integers(0, 256, shape + (3,), dtype=np.uint8) * (rng.random(shape + (1,)) < 0.5).astype(np.uint8)
    b[0, 0, 0] = (0, 0, 9)                              # non-zero in its last channel alone
    oa, ob = a > 0, np.any(b > 0, axis=-1)
    ref = lambda x, y: (int((x & y).sum()), int(x.sum()), int(y.sum()))     # noqa: E731
    assert pb3d_gpu.grid_overlap_counts(a, b) == ref(oa, ob)
    assert pb3d_gpu.grid_overlap_counts(b, a) == ref(ob, oa)
    assert pb3d_gpu.grid_overlap_counts(a, a) == ref(oa, oa)
    assert pb3d_gpu.grid_overlap_counts(b, b) == ref(ob, ob)
    big = (rng.random((40, 40, 70)) < 0.5).astype(np.uint8)
    assert pb3d_gpu.grid_overlap_counts(big, big[::-1].copy()) == ref(big > 0, big[::-1] > 0)


@gpu
def test_mesh_grid_iou(pb3d_gpu):
    mask, v, f = trip("trip1")
    assert pb3d_gpu.mesh_grid_iou(v, f, mask.astype(np.uint8)) == 1.0
    grid, vm, fm = trip_meshify("trip1")
    assert pb3d_gpu.mesh_grid_iou(vm, fm, grid, frame="meshify") == 1.0
    half = mask.astype(np.uint8)
    half[:6] = 0
    inter, union = int((half > 0).sum()), int(mask.sum())
    assert pb3d_gpu.mesh_grid_iou(v, f, half) == np.float64(inter) / np.float64(union)
    assert pb3d_gpu.mesh_grid_iou(v[:0], f[:0], np.zeros(mask.shape, np.uint8)) == 0.0


@gpu
def test_resident_chain_meshify_to_voxelize(pb3d_gpu, golden):
    """pb3d.device.meshify(download=False) of a carved fixture grid, then voxelize_mesh_resident(frame="meshify"): the grid's occupancy
    comes back, nothing but the result leaving the device.  The 20 x 18 x 24 fixture is padded to 24 x 20 x 28, so its border is empty"""
    from pb3d import device as dev
    carved = golden("pcarve_synth")["views9/out"]
    grid = np.zeros((24, 20, 28, 3), np.uint8)
    grid[2:-2, 1:-1, 2:-2] = carved
    occ = np.any(grid > 0, axis=-1).astype(np.uint8)
    assert occ.any()
    d_grid = dev.from_numpy(grid)
    bufs = [d_grid]
    try:
        (dv, df, dn, dc), (n, m) = dev.meshify(d_grid, grid.shape, download=False)
        bufs += [dv, df, dn, dc]
        d_out, stats = pb3d_gpu.voxelize_mesh_resident(dv, n, df, m, grid.shape[:3], frame="meshify", return_stats=True)
        bufs.append(d_out)
        same(d_out.download(grid.shape[:3]), occ, "chain")
        assert stats["occupied"] == int(occ.sum()) and stats["open_columns"] == 0
        assert pb3d_gpu.grid_overlap_counts_resident(d_out, 1, d_grid, 3, occ.size) == (int(occ.sum()),) * 3
    finally:
        for b in bufs:
            b.free()
