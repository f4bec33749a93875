"""Edge cases of the deformation kernels (csrc/deform.hip): pb3d_deform_count[_dev] / pb3d_deform_fill[_dev], pb3d_deform_paint_dev,
pb3d_scatter_colors_dev and pb3d_deform_iou_batch_dev against the NumPy restatement tests/deform_restate.py and the reference
closures' recorded results (tests/golden/deform_edges.*: rounding ties, sign(0), fused multiply-add and float32 sensitive clouds,
rounded means, duplicates, the six faces of a 5 x 7 x 9 grid, paint order).  tests/test_deform_host.py shows on the CPU that these
cases tell the right arithmetic from round-half-away, a contracted multiply-add, float32, sign(0) = 1 and a shared centre.

Every comparison is exact equality.  Device buffers sit between guard bytes (test_pointer_offsets.Run).  The batch runs its pass loop
(more tuples than fit one pass: 8192, or 256 MiB / pixels), and every grid-stride loop of the file takes a second trip (300,000 and
80,000 points, 600,000 rows).

With n == 0 points the batch gives inter = nvalid = 0 and uni = the image's pixels of the colour: what the reference's empty projection
gives (its union is the image part alone), not zero."""
import ctypes as C

import numpy as np
import pytest

import deform_restate as dr
from test_pointer_offsets import Run

gpu = pytest.mark.gpu
PATTERN_SEED = 77


@pytest.fixture(scope="module")
def fixtures():
    return dr.load()


def _f32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _cam_struct(pb3d, cam):
    """the pb3d_camera evaluate_part_deform_batch builds: float32 points, the camera's own dtypes"""
    from pb3d.camera_estimation import CameraObjective
    from pb3d.projection_utils import camera_args
    _, _, R, pos, prec = camera_args(np.zeros((1, 3), np.float32), cam["cam_pos"], cam["target"], cam["f"], cam["cx"], cam["cy"])
    c = np.zeros(1, CameraObjective._CAM)
    c["R"][0] = R.reshape(9); c["cam"][0] = pos; c["f"][0] = float(cam["f"]); c["cx"][0] = float(cam["cx"]); c["cy"][0] = float(cam["cy"])
    c["prec"][0] = list(prec)
    return c


def _batch(pb3d, pts, A, sc, image, cam, colour, what="batch", prefill=-7):
    """pb3d_deform_iou_batch_dev on guarded device buffers -> (rc, inter, uni, nvalid); the points and the image must not change"""
    L = pb3d._lib
    run = Run(pb3d, what)
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    image = np.ascontiguousarray(image, np.uint8)
    H, W = image.shape[:2]
    d_pts = run.inp(pts, 0) if len(pts) else None
    d_img = run.inp(image, 0) if image.size else None
    sc = np.ascontiguousarray(sc, np.float64).reshape(-1, 5)
    K = len(sc)
    out = [np.full(K + 2, prefill, np.int64) for _ in range(3)]             # one spare element on each side of the K outputs
    c = _cam_struct(pb3d, cam)
    col = np.ascontiguousarray(colour, np.uint8)
    rc = run.lib.pb3d_deform_iou_batch_dev(run.ctx, d_pts, len(pts), L.p_dbl(sc), K, A[0], A[1], A[2], c.ctypes.data_as(C.c_void_p), H, W, d_img,
                                           L.p_u8(col), *(o[1:].ctypes.data_as(L.i64p) for o in out))
    run.finish()
    for o in out:
        assert o[0] == prefill and o[-1] == prefill, what
    return (rc,) + tuple(o[1:-1] for o in out)


def _seg_image(H, W, colour, seed, p=0.4, other=(1, 220, 5)):
    """an image whose pixels hold `colour` with probability p, black with 0.1, else another colour"""
    r = np.random.default_rng(seed).random((H, W))
    img = np.empty((H, W, 3), np.uint8)
    img[:] = np.uint8(other)
    img[r < p] = np.uint8(colour)
    img[r > 0.9] = 0
    return img


def _count_fill_dev(pb3d, pts, sc, what):
    """count, then fill, on guarded device buffers -> int64 rows"""
    run = Run(pb3d, what)
    d_pts = run.inp(np.ascontiguousarray(pts, np.float32), 0)
    nu = C.c_int64(-3)
    run.ok(run.lib.pb3d_deform_count_dev(run.ctx, d_pts, len(pts), *sc, C.byref(nu)))
    out = run.out(nu.value * 24, 0)
    run.ok(run.lib.pb3d_deform_fill_dev(run.ctx, nu.value, out.ptr))
    return run.finish()[0].view(np.int64).reshape(-1, 3)


def _pattern(shape):
    return np.random.default_rng(PATTERN_SEED).integers(1, 256, tuple(shape) + (3,), dtype=np.uint8)


def _paint_dev(pb3d, calls, A, what, init=None):
    """pb3d_deform_paint_dev for every (pts, scalars, rgb) of `calls`, in order, on one guarded grid prefilled with a pattern"""
    run = Run(pb3d, what)
    init = _pattern(A) if init is None else init
    g = run.out(init.nbytes, 0, init=init)
    rcs = []
    for pts, sc, rgb in calls:
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
        d_pts = run.inp(pts, 0) if len(pts) else None
        rcs.append(run.lib.pb3d_deform_paint_dev(run.ctx, d_pts, len(pts), *sc, A[0], A[1], A[2], pb3d._lib.p_u8(np.ascontiguousarray(rgb, np.uint8)), g.ptr))
    return rcs, run.finish()[0].reshape(init.shape)


def _painted(A, calls, init=None):
    """the restatement: the pattern with every call's unique in-bounds rows set to its colour, in order"""
    out = _pattern(A) if init is None else init.copy()
    for pts, sc, rgb in calls:
        if len(pts) == 0:
            continue
        cd = np.unique(dr.rounded(pts, sc)[0], axis=0)
        cd = cd[dr.in_bounds(cd, A)]
        if len(cd):
            dr.paint(out, cd, dr.pair_colors(np.repeat(np.uint8([rgb]), len(pts), axis=0), len(cd)))
    return out


# =====================================================================================================================
# The constructed cases, by every route
# =====================================================================================================================

@gpu
def test_clouds_deform_coords(pb3d_gpu, fixtures):
    """pb3d.deform_coords (host pair) and count -> fill on device buffers == the closures' rows; three runs agree"""
    clouds, _ = fixtures
    for name, (c, rows) in clouds.items():
        got = pb3d_gpu.deform_coords(c["pts"], c["image_shape"], c["voxel_shape"], c["deform"])
        assert got.dtype == np.int64 and np.array_equal(got, rows), name
        sc = dr.scalars(c["image_shape"], c["voxel_shape"], c["deform"])
        for rep in range(3 if c["kind"] in ("tie", "fma") else 1):
            assert np.array_equal(_count_fill_dev(pb3d_gpu, c["pts"], sc, name), rows), (name, rep)


@gpu
def test_scenes_by_the_python_routes(pb3d_gpu, fixtures):
    """deform_part, evaluate_part_deform, evaluate_part_deform_batch and build_deformed_grid == the closures' results"""
    _, scenes = fixtures
    for name, (sc, parts, out) in scenes.items():
        grid, labels, image, cam = sc["grid"], sc["labels"], sc["image"], sc["cam"]
        ishape = image.shape[:2]
        for part, (rows, iou) in parts.items():
            d = sc["saved"][part]
            pts, cols = pb3d_gpu.get_voxel_points_by_parts(grid, labels, [part])
            assert np.array_equal(pb3d_gpu.deform_coords(pts, ishape, grid.shape[:3], d), rows), (name, part)
            cd, ccols = pb3d_gpu.deform_part(grid, labels, part, d, ishape)
            keep = rows[dr.in_bounds(rows, grid.shape[:3])]
            assert np.array_equal(cd, keep) and np.array_equal(ccols, dr.pair_colors(cols, len(keep))), (name, part)
            proj, got = pb3d_gpu.evaluate_part_deform(grid, labels, part, d, image, cam)
            assert got == iou, (name, part, got, iou)
            inter, uni, nv = dr.iou_counts(pts, grid.shape[:3], d, image, cam, labels[part])
            hit = np.all(proj == np.uint8(labels[part]), axis=-1)
            gt = np.all(image == np.uint8(labels[part]), axis=-1)
            assert (int((hit & gt).sum()), int((hit | gt).sum())) == (inter, uni), (name, part)
            ious, nvalid = pb3d_gpu.evaluate_part_deform_batch(grid, labels, part, [d, dr.D(), d], image, cam)
            assert int(nvalid[0]) == nv == int(nvalid[2]) and int(nvalid[1]) == 7 * len(pts), (name, part)
            assert ious[0] == ious[2] == (iou if nv > 0 else 0.0), (name, part)
        full = pb3d_gpu.build_deformed_grid(grid, labels, {p: {"deform": d} for p, d in sc["saved"].items()}, ishape)
        assert full.dtype == np.uint8 and np.array_equal(full, out), name


# =====================================================================================================================
# pb3d_deform_paint_dev
# =====================================================================================================================

@gpu
def test_paint_dev_clouds(pb3d_gpu, fixtures):
    """every cloud painted into a patterned, guarded grid: the unique in-bounds rows take the colour, nothing else changes"""
    clouds, _ = fixtures
    untouched = 0
    for name, (c, rows) in clouds.items():
        A = c["voxel_shape"]
        calls = [(c["pts"], dr.scalars(c["image_shape"], A, c["deform"]), (9, 200, 31))]
        rcs, got = _paint_dev(pb3d_gpu, calls, A, name)
        want = _painted(A, calls)
        assert rcs == [0] and np.array_equal(got, want), name
        keep = rows[dr.in_bounds(rows, A)]
        assert int((want != _pattern(A)).any(axis=-1).sum()) == len(keep), name
        untouched += len(keep) == 0
    assert untouched >= 4                                                   # the all-out-of-bounds clouds leave the grid as it was


@gpu
def test_paint_dev_sequence_and_empty(pb3d_gpu, fixtures):
    """two paints in sequence: the later colour on the overlap; n == 0 and a grid without voxels are no-ops"""
    clouds, _ = fixtures
    a, b = clouds["bounds_stretch"][0], clouds["bounds_all_in"][0]
    A = a["voxel_shape"]
    calls = [(a["pts"], dr.scalars(a["image_shape"], A, a["deform"]), (250, 1, 2)), (b["pts"], dr.scalars(b["image_shape"], A, b["deform"]), (3, 4, 251))]
    rcs, got = _paint_dev(pb3d_gpu, calls, A, "sequence")
    want = _painted(A, calls)
    assert rcs == [0, 0] and np.array_equal(got, want)
    first, second = (np.all(want == np.uint8(c[2]), axis=-1) for c in calls)
    alone = _painted(A, calls[:1])
    assert first.any() and second.any() and (np.all(alone == np.uint8((250, 1, 2)), axis=-1) & second).any()      # there is an overlap
    rcs, got = _paint_dev(pb3d_gpu, calls[::-1], A, "sequence reversed")
    assert rcs == [0, 0] and np.array_equal(got, _painted(A, calls[::-1])) and not np.array_equal(got, want)
    rcs, got = _paint_dev(pb3d_gpu, [(np.zeros((0, 3), np.float32), (1.0, 1.0, 0.0, 0.0, 0.0), (1, 2, 3))], A, "n == 0")
    assert rcs == [0] and np.array_equal(got, _pattern(A))
    L = pb3d_gpu._lib
    run = Run(pb3d_gpu, "empty grid")
    d_pts = run.inp(a["pts"], 0)
    g = run.out(64, 0)
    rc = run.lib.pb3d_deform_paint_dev(run.ctx, d_pts, len(a["pts"]), 1.0, 1.0, 0.0, 0.0, 0.0, 5, 0, 9, L.p_u8(np.uint8([1, 2, 3])), g.ptr)
    assert rc == 0 and (run.finish()[0] == 0xA5).all()


# =====================================================================================================================
# pb3d_scatter_colors_dev
# =====================================================================================================================

def _scatter(pb3d, rows, cols, A, what, init=None):
    run = Run(pb3d, what)
    init = _pattern(A) if init is None else init
    g = run.out(init.nbytes, 0, init=init)
    rows = np.ascontiguousarray(rows, np.int64).reshape(-1, 3)
    cols = np.ascontiguousarray(cols, np.uint8).reshape(-1, 3)
    d_rows = run.inp(rows, 0) if len(rows) else None
    d_cols = run.inp(cols, 0) if len(rows) else None
    rc = run.lib.pb3d_scatter_colors_dev(run.ctx, d_rows, d_cols, len(rows), A[0], A[1], A[2], g.ptr)
    return rc, run.finish()[0].reshape(init.shape)


def _unique_rows(A, m, seed):
    """m distinct in-bounds (x, y, z) rows in a shuffled order, and a colour for each"""
    rng = np.random.default_rng(seed)
    flat = rng.permutation(A[0] * A[1] * A[2])[:m]
    z, y, x = np.unravel_index(flat, A)
    return np.stack([x, y, z], axis=1).astype(np.int64), rng.integers(0, 256, (m, 3), dtype=np.uint8)


@gpu
@pytest.mark.parametrize("A, m", [((5, 7, 9), 1), ((5, 7, 9), 255), ((5, 7, 9), 315), ((9, 11, 13), 256), ((9, 11, 13), 257), ((96, 96, 96), 600000)])
def test_scatter_colors(pb3d_gpu, A, m):
    """grid[z, y, x] = cols for unique in-bounds rows: m around the block size, every voxel of a 5 x 7 x 9 grid, and 600,000 rows (a
    second trip of the grid-stride loop: 256 CUs x 8 blocks x 256 threads = 524,288)"""
    rows, cols = _unique_rows(A, m, 1000 + m)
    rc, got = _scatter(pb3d_gpu, rows, cols, A, f"scatter {m}")
    want = _pattern(A)
    want[rows[:, 2], rows[:, 1], rows[:, 0]] = cols
    assert rc == 0 and np.array_equal(got, want)
    assert int((want != _pattern(A)).any(axis=-1).sum()) > 0.9 * m


@gpu
def test_scatter_colors_refusals_and_empty(pb3d_gpu):
    """one row outside each of the six faces: PB3D_EINVAL, and (one row: nothing else could be written) the grid as it was; among good
    rows: PB3D_EINVAL, every voxel holds its old bytes or its row's colour, nothing outside the grid is written; m == 0 is a no-op"""
    A = (5, 7, 9)
    L = pb3d_gpu._lib
    for row in ([-1, 3, 2], [9, 3, 2], [4, -1, 2], [4, 7, 2], [4, 3, -1], [4, 3, 5]):
        rc, got = _scatter(pb3d_gpu, [row], [[1, 2, 3]], A, f"oob {row}")
        assert rc == -1 and "out of bounds" in L.load().pb3d_last_error().decode() and np.array_equal(got, _pattern(A)), row
        rows, cols = _unique_rows(A, 40, 5)
        rows[17] = row
        rc, got = _scatter(pb3d_gpu, rows, cols, A, f"oob among good rows {row}")
        assert rc == -1, row
        want = _pattern(A)
        good = np.delete(np.arange(40), 17)
        old = want[rows[good, 2], rows[good, 1], rows[good, 0]]
        new = got[rows[good, 2], rows[good, 1], rows[good, 0]]
        assert (np.all(new == old, axis=1) | np.all(new == cols[good], axis=1)).all(), row
        want[rows[good, 2], rows[good, 1], rows[good, 0]] = new
        assert np.array_equal(got, want), row
    rc, got = _scatter(pb3d_gpu, np.zeros((0, 3), np.int64), np.zeros((0, 3), np.uint8), A, "m == 0")
    assert rc == 0 and np.array_equal(got, _pattern(A))
    rows, cols = _unique_rows(A, 20, 6)                                     # the entry works after the refusals
    rc, got = _scatter(pb3d_gpu, rows, cols, A, "after refusals")
    want = _pattern(A)
    want[rows[:, 2], rows[:, 1], rows[:, 0]] = cols
    assert rc == 0 and np.array_equal(got, want)


# =====================================================================================================================
# pb3d_deform_iou_batch_dev
# =====================================================================================================================

@gpu
def test_batch_mixed_lists(pb3d_gpu, fixtures):
    """every cloud with a list that mixes ordinary tuples, its own constructed tuple, the tie tuples, one that puts the part outside
    and one clipping at each face: inter, uni and nvalid per tuple, float32 and float64 cameras, an ordinary colour, a colour the image
    does not hold and black"""
    clouds, _ = fixtures
    colour = (190, 0, 255)
    for i, (name, (c, _)) in enumerate(clouds.items()):
        A = dr.batch_bounds(c)
        H, W = c["image_shape"]
        image = _seg_image(H, W, colour, 500 + i)
        sc = dr.mixed_batch(c)
        for dtype in (np.float32, np.float64):
            cam = dr.front_camera(A, H, W, dtype)
            for col in (colour, (7, 7, 7), (0, 0, 0)):
                rc, inter, uni, nv = _batch(pb3d_gpu, c["pts"], A, sc, image, cam, col, name)
                want = dr.iou_counts_sc(c["pts"], A, sc, image, cam, col)
                assert rc == 0, name
                for g, w, what in zip((inter, uni, nv), want, ("inter", "uni", "nvalid")):
                    assert np.array_equal(g, w), (name, dtype.__name__, col, what, g, w)
                if col == (7, 7, 7):
                    assert not inter.any()
                if col == (0, 0, 0):
                    assert (uni == H * W).all() and (inter == int(np.all(image == 0, axis=-1).sum())).all()


def _multipass(fixtures):
    clouds, _ = fixtures
    pts = clouds["tie_n8_m0"][0]["pts"]
    sc = dr.lattice(8197, {0: dr.TIE_SC[0], 8191: dr.TIE_SC[1], 8192: dr.TIE_SC[2], 8196: dr.TIE_SC[3]})
    A, colour = (16, 16, 16), (63, 138, 173)
    return pts, sc, A, colour, _seg_image(16, 16, colour, 900), dr.front_camera(A, 16, 16)


@gpu
def test_batch_multipass_8192(pb3d_gpu, fixtures):
    """8192 + 5 distinct tuples on a 16 x 16 image: two passes of the pass loop (8192 tuples, then 5), the constructed tie tuples at
    the seams; every tuple against the restatement, three runs agree"""
    pts, sc, A, colour, image, cam = _multipass(fixtures)
    want = dr.iou_counts_sc(pts, A, sc, image, cam, colour)
    assert len({tuple(int(w[k]) for w in want) for k in range(len(sc))}) > 500         # a shifted offset would show
    for rep in range(3):
        rc, inter, uni, nv = _batch(pb3d_gpu, pts, A, sc, image, cam, colour, "multipass 8192")
        assert rc == 0
        for g, w, what in zip((inter, uni, nv), want, ("inter", "uni", "nvalid")):
            bad = np.flatnonzero(g != w)
            assert len(bad) == 0, (rep, what, bad[:8], g[bad[:8]], w[bad[:8]])


@gpu
def test_batch_multipass_256(pb3d_gpu, fixtures):
    """a 1024 x 1024 image holds 256 tuples per pass: 258 tuples run two passes.  The restatement forms the union as
    |image part| + |pixels hit| - inter"""
    clouds, _ = fixtures
    pts = clouds["dup_half"][0]["pts"]
    A, colour = (16, 16, 16), (63, 138, 173)
    sc = dr.lattice(258, {0: dr.TIE_SC[0], 255: dr.TIE_SC[1], 256: dr.TIE_SC[2], 257: dr.TIE_SC[3]})
    image = _seg_image(1024, 1024, colour, 901)
    cam = dr.front_camera(A, 1024, 1024, np.float64)
    want = dr.iou_counts_sc(pts, A, sc, image, cam, colour, dense=False)
    rc, inter, uni, nv = _batch(pb3d_gpu, pts, A, sc, image, cam, colour, "multipass 256")
    assert rc == 0
    for g, w, what in zip((inter, uni, nv), want, ("inter", "uni", "nvalid")):
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, (what, bad[:8], g[bad[:8]], w[bad[:8]])
    assert len(np.unique(inter)) > 30


@gpu
def test_batch_zero_sizes(pb3d_gpu, fixtures):
    """ntuples == 0: no output element is written; npix == 0: the outputs are zero; n == 0: inter and nvalid are zero and uni is the
    image's part alone (the reference's empty projection).  The buffers passed are unchanged (guards, inputs)."""
    clouds, _ = fixtures
    c = clouds["tie_n8_m0"][0]
    A, colour = (16, 16, 16), (190, 0, 255)
    image = _seg_image(16, 16, colour, 902)
    cam = dr.front_camera(A, 16, 16)
    rc, inter, uni, nv = _batch(pb3d_gpu, c["pts"], A, np.zeros((0, 5)), image, cam, colour, "ntuples == 0")
    assert rc == 0 and len(inter) == len(uni) == len(nv) == 0
    sc = dr.mixed_batch(c)
    rc, inter, uni, nv = _batch(pb3d_gpu, c["pts"], A, sc, np.zeros((0, 16, 3), np.uint8), cam, colour, "npix == 0")
    assert rc == 0 and not inter.any() and not uni.any() and not nv.any()
    rc, inter, uni, nv = _batch(pb3d_gpu, np.zeros((0, 3), np.float32), A, sc, image, cam, colour, "n == 0")
    gt = int(np.all(image == np.uint8(colour), axis=-1).sum())
    assert rc == 0 and not inter.any() and not nv.any() and gt > 0 and (uni == gt).all()


# =====================================================================================================================
# Second trips of the grid-stride loops
# =====================================================================================================================

BIG_A = (96, 96, 96)
BIG_D = dr.D(1.25, 0.75, 2.0, -3.0)


@pytest.fixture(scope="module")
def big_cloud():
    """300,000 integer points in a 96^3 box (k_deform_sum loops past 262,144 points, the 7n kernels past 74,898) and the restatement's
    rows, computed once"""
    pts = np.random.default_rng(96).integers(0, 96, (300000, 3)).astype(np.float32)
    sc = dr.scalars(BIG_A[:2], BIG_A, BIG_D)
    return pts, sc, np.unique(dr.rounded(pts, sc)[0], axis=0)


@gpu
def test_second_trip_deform_coords(pb3d_gpu, big_cloud):
    pts, sc, rows = big_cloud
    assert np.array_equal(pb3d_gpu.deform_coords(pts, BIG_A[:2], BIG_A, BIG_D), rows)
    assert np.array_equal(_count_fill_dev(pb3d_gpu, pts, sc, "big count -> fill"), rows)


@gpu
def test_second_trip_paint(pb3d_gpu, big_cloud):
    pts, sc, rows = big_cloud
    rcs, got = _paint_dev(pb3d_gpu, [(pts, sc, (9, 200, 31))], BIG_A, "big paint")
    want = _pattern(BIG_A)
    keep = rows[dr.in_bounds(rows, BIG_A)]
    assert 0 < len(keep) < len(rows)
    want[keep[:, 2], keep[:, 1], keep[:, 0]] = (9, 200, 31)
    assert rcs == [0] and np.array_equal(got, want)


@gpu
def test_second_trip_batch(pb3d_gpu):
    """80,000 points in a 3-tuple batch: 560,000 evaluations per tuple over at most 1366 blocks, so lanes of one wave leave the loop
    at different trips"""
    pts = np.random.default_rng(97).integers(0, 64, (80000, 3)).astype(np.float32)
    A, colour = (64, 64, 64), (190, 0, 255)
    sc = np.array([(1.25, 0.75, 2.0, -3.0, 2.0), (0.5, 1.5, -1.25, 2.5, -1.25), (1.0, 1.0, 0.0, 30.0, 0.0)])
    image = _seg_image(96, 96, colour, 903)
    cam = dr.front_camera(A, 96, 96)
    want = dr.iou_counts_sc(pts, A, sc, image, cam, colour)
    rc, inter, uni, nv = _batch(pb3d_gpu, pts, A, sc, image, cam, colour, "big batch")
    assert rc == 0
    for g, w, what in zip((inter, uni, nv), want, ("inter", "uni", "nvalid")):
        assert np.array_equal(g, w), (what, g, w)
    assert (nv > 0).all() and (nv < 7 * len(pts)).all() and (inter > 0).all()


# =====================================================================================================================
# Non-finite deform scalars are refused
# =====================================================================================================================

BAD = [(0, "sxz", np.nan), (1, "sy", np.inf), (2, "kx", -np.inf), (3, "ky", np.nan), (4, "kz", np.inf)]


def _pending_count(pb3d, pts, sc):
    """a count whose fill has not run yet -> n_unique"""
    nu = C.c_int64(0)
    pb3d._lib.check(pb3d._lib.load().pb3d_deform_count(pb3d._lib.ctx(), _f32p(pts), len(pts), *sc, C.byref(nu)))
    return nu.value


def _fill_refused(pb3d, n_unique):
    out = np.full((n_unique, 3), -7, np.int64)
    with pytest.raises(ValueError, match="pb3d_deform_fill: call pb3d_deform_count first"):
        pb3d._lib.check(pb3d._lib.load().pb3d_deform_fill(pb3d._lib.ctx(), n_unique, out.ctypes.data_as(pb3d._lib.i64p)))
    assert (out == -7).all()


@gpu
def test_non_finite_scalars_are_refused(pb3d_gpu, fixtures):
    """count (host and device), paint and the batch return PB3D_EINVAL for a non-finite scalar and name it (the batch: the tuple too);
    their outputs are untouched, a pending count -> fill pair is dropped, and the entries work afterwards"""
    clouds, _ = fixtures
    c, rows = clouds["tie_n8_m0"]
    pts, A = c["pts"], c["voxel_shape"]
    good = dr.scalars(c["image_shape"], A, c["deform"])
    L, lib = pb3d_gpu._lib, pb3d_gpu._lib.load()
    err = lambda: lib.pb3d_last_error().decode()
    image = _seg_image(16, 16, (190, 0, 255), 904)
    cam = dr.front_camera(A, 16, 16)
    for a, name, v in BAD:
        sc = list(good)
        sc[a] = v
        # count, host flavour
        n0 = _pending_count(pb3d_gpu, pts, good)
        nu = C.c_int64(123)
        assert lib.pb3d_deform_count(L.ctx(), _f32p(pts), len(pts), *sc, C.byref(nu)) == -1
        assert err() == f"pb3d_deform_count: {name} is not finite" and nu.value == 123
        _fill_refused(pb3d_gpu, n0)
        # count, device flavour
        n0 = _pending_count(pb3d_gpu, pts, good)
        run = Run(pb3d_gpu, "count refused")
        d_pts = run.inp(pts, 0)
        assert run.lib.pb3d_deform_count_dev(run.ctx, d_pts, len(pts), *sc, C.byref(nu)) == -1
        run.finish()
        assert err() == f"pb3d_deform_count: {name} is not finite" and nu.value == 123
        _fill_refused(pb3d_gpu, n0)
        # paint
        n0 = _pending_count(pb3d_gpu, pts, good)
        rcs, got = _paint_dev(pb3d_gpu, [(pts, sc, (1, 2, 3))], A, "paint refused")
        assert rcs == [-1] and err() == f"pb3d_deform_paint: {name} is not finite" and np.array_equal(got, _pattern(A))
        _fill_refused(pb3d_gpu, n0)
        # the batch: the bad tuple is not the first
        n0 = _pending_count(pb3d_gpu, pts, good)
        tuples = dr.mixed_batch(c)
        tuples[5] = sc
        rc, inter, uni, nv = _batch(pb3d_gpu, pts, A, tuples, image, cam, (190, 0, 255), "batch refused")
        assert rc == -1 and err() == f"pb3d_deform_iou_batch: tuple 5: {name} is not finite"
        assert (inter == -7).all() and (uni == -7).all() and (nv == -7).all()
        _fill_refused(pb3d_gpu, n0)
        with pytest.raises(ValueError, match="pb3d_deform_count: k?[sxyz]+ is not finite"):
            pb3d_gpu.deform_coords(pts, c["image_shape"], A, {**c["deform"], {0: "scale_xz", 1: "scale_y", 2: "shift_xz", 3: "shift_y", 4: "shift_xz"}[a]: v})
    # a finite call after the refusals
    assert np.array_equal(pb3d_gpu.deform_coords(pts, c["image_shape"], A, c["deform"]), rows)
    assert np.array_equal(_count_fill_dev(pb3d_gpu, pts, good, "after refusals"), rows)
    rcs, got = _paint_dev(pb3d_gpu, [(pts, good, (1, 2, 3))], A, "paint after refusals")
    assert rcs == [0] and np.array_equal(got, _painted(A, [(pts, good, (1, 2, 3))]))
    sc = dr.mixed_batch(c)
    rc, inter, uni, nv = _batch(pb3d_gpu, pts, A, sc, image, cam, (190, 0, 255), "batch after refusals")
    want = dr.iou_counts_sc(pts, A, sc, image, cam, (190, 0, 255))
    assert rc == 0 and all(np.array_equal(g, w) for g, w in zip((inter, uni, nv), want))
