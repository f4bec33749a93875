"""distance_transform, the ball morphology and grid_surface_metrics (pb3d/distance.py, csrc/edt.hip) against the NumPy restatement of
tests/edt_restate.py, and that restatement against a brute force over all (voxel, target) pairs and against scipy.ndimage.  Every
comparison is np.array_equal: include/pb3d.h states the result in integers, so there is no tolerance.

The constants of csrc/edt.hip the shapes are chosen around: the row pass ballots ROW_WORD = 64 voxels into a word and names the
non-empty words of a row in masks of ROW_GROUP = 64 words = 4096 voxels; the column passes have no tile, band or stack segment (a
column's stack lies at the column's own voxels, as long as the column), so the lengths that matter there are COLUMN_GROUP = 256, the
columns a workgroup takes at a time, and MAX_AXIS = 16384, where the 14-bit packing of a stack level and int32 end."""
import functools
import math

import numpy as np
import pytest
import scipy.ndimage as ndi

import edt_restate as er

import pb3d
import pb3d.distance as pd  # noqa: F401  (without the feature every test of this file fails here)

gpu = pytest.mark.gpu

ROW_WORD, ROW_GROUP, COLUMN_GROUP, MAX_AXIS = 64, 4096, 256, pd.MAX_AXIS
SMALL = (9, 7, 11)
MID = (40, 33, 70)
SMALL_CASES = er.contents(SMALL)
MID_CASES = er.contents(MID)
R_SQ = (1, 2, 3, 5, 9)


@functools.lru_cache(maxsize=None)
def restated(case, to, border, shape=MID):
    """(sq, index) of a constructed content by the restatement, computed once"""
    mask = er.contents(shape)[case]
    res = er.edt_grid(er.grid_for(mask, to), to, border)
    for a in res:
        a.setflags(write=False)
    return res


def rgb_of(grid, seed=3):
    """an RGB grid with the occupancy of `grid`, random colours, some voxels with only the last byte set"""
    rng = np.random.default_rng(seed)
    rgb = rng.integers(1, 256, grid.shape + (3,), dtype=np.uint8)
    rgb[rng.random(grid.shape) < 0.3, :2] = 0
    return rgb * (grid != 0)[..., None].astype(np.uint8)


def labels_of(grid, seed=4):
    return (np.random.default_rng(seed).integers(1, 12, grid.shape, dtype=np.uint8) * (grid != 0)).astype(np.uint8)


# ---- CPU: the rules --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SMALL, (1, 1, 9), (6, 1, 4), (5, 8, 1)])
def test_restatement_equals_brute_force(shape):
    for name, mask in er.contents(shape).items():
        for to in er.TARGETS:
            t = er.target_mask(er.grid_for(mask, to), to)
            for border in (False, True):
                sq, idx = er.edt(t, border)
                bsq, bidx = er.brute(t, border)
                assert np.array_equal(sq, bsq), (name, to, border)
                assert np.array_equal(idx, bidx), (name, to, border)


@pytest.mark.parametrize("name", sorted(SMALL_CASES))
def test_restated_distances_are_scipys(name):
    x = er.grid_for(SMALL_CASES[name], "background")
    sq, idx = er.edt_grid(x, "background")
    if not (x == 0).any():
        assert (sq == er.NONE).all() and (idx == -1).all() and np.isinf(er.distances(sq)).all()
        return
    ref = ndi.distance_transform_edt(x)
    assert np.array_equal(er.distances(sq), ref)
    # every restated index is A nearest target by SciPy's distances
    t = np.stack(np.unravel_index(idx, x.shape), axis=-1)
    v = np.stack(np.indices(x.shape), axis=-1)
    assert (x.reshape(-1)[idx.reshape(-1)] == 0).all()
    assert np.array_equal(np.sqrt(((t - v) ** 2).sum(axis=-1).astype(np.float64)), ref)


@pytest.mark.parametrize("r_sq", R_SQ)
def test_ball_identities(r_sq):
    for name in ("random_0.5", "random_0.995", "random_0.005", "checkerboard", "slab_axis1", "pairs_all_axes"):
        occ = SMALL_CASES[name]
        b = er.ball(r_sq)
        if occ.any():
            assert np.array_equal(ndi.binary_dilation(occ, b), er.edt(occ)[0] <= r_sq), name
        assert np.array_equal(ndi.binary_erosion(occ, b, border_value=0), er.edt(~occ, border=True)[0] > r_sq), name
        assert np.array_equal(er.occupancy(er.dilate(occ.astype(np.uint8), r_sq)), ndi.binary_dilation(occ, b) if occ.any() else occ), name
        assert np.array_equal(er.occupancy(er.erode(occ.astype(np.uint8), r_sq)), ndi.binary_erosion(occ, b, border_value=0)), name


def test_tie_rule_is_not_vacuous():
    """on er.tie_case() the largest-index rule and SciPy's own indices both differ from the stated rule"""
    t = er.tie_case()
    _, idx = er.edt(t)
    assert np.array_equal(idx, er.brute(t)[1])
    assert (er.brute(t, rule="largest")[1] != idx).any()
    _, ind = ndi.distance_transform_edt(~t, return_indices=True)
    scipy_idx = (ind[0] * t.shape[1] + ind[1]) * t.shape[2] + ind[2]
    assert (scipy_idx != idx).any()


def test_radius_rule():
    assert [pd._radius_sq(r) for r in (0, 1, 1.5, 2, math.sqrt(2), math.sqrt(3), 2.9999)] == [0, 1, 2, 4, 2, 2, 8]
    assert all(pd._radius_sq(r) == er.radius_sq(r) for r in (0.0, 0.37, 1.0, 1.5, 2.5, 7.3))


def test_closing_fixture_by_the_restatement():
    grid, box = closing_fixture()
    assert np.array_equal(er.close(grid, 1)[5, 5, 5], grid[4, 5, 5])
    assert np.array_equal(er.occupancy(er.close(grid, 2)), box)


def test_argument_validation_needs_no_device():
    g = np.zeros((4, 5, 6), np.uint8)
    with pytest.raises(ValueError):
        pb3d.distance_transform(np.zeros((4, 5), np.uint8))
    with pytest.raises(ValueError):
        pb3d.distance_transform(np.zeros((4, 5, 6, 2), np.uint8))
    with pytest.raises(ValueError):
        pb3d.distance_transform(np.zeros((4, 0, 6), np.uint8))
    with pytest.raises(TypeError):
        pb3d.distance_transform(g.astype(np.float32))
    with pytest.raises(TypeError):
        pb3d.distance_transform(g, dtype=np.int32)
    with pytest.raises(ValueError):
        pb3d.distance_transform(g, to="edges")
    with pytest.raises(ValueError):
        pb3d.distance_transform(g, voxel_size=0.0)
    with pytest.raises(ValueError):
        pb3d.distance_transform(g, return_indices=True, border=True)
    with pytest.raises(ValueError):
        pb3d.distance_transform(g, return_distances=False)
    for shape in ((MAX_AXIS + 1, 1, 1), (1, MAX_AXIS + 1, 1), (1, 1, MAX_AXIS + 1)):
        with pytest.raises(ValueError):
            pb3d.distance_transform(np.zeros(shape, np.uint8))
        with pytest.raises(ValueError):
            pb3d.dilate_grid(np.zeros(shape, np.uint8), 1)
    for fn in (pb3d.dilate_grid, pb3d.erode_grid, pb3d.close_grid, pb3d.open_grid):
        with pytest.raises(ValueError):
            fn(g, -1)
        with pytest.raises(ValueError):
            fn(g, math.nan)
        with pytest.raises(TypeError):
            fn(g, "1")
        with pytest.raises(TypeError):
            fn(g.astype(np.int32), 1)
    with pytest.raises(ValueError):
        pb3d.grid_surface_metrics(g, g, thresholds=tuple(range(1, 10)))
    with pytest.raises(ValueError):
        pb3d.grid_surface_metrics(g, g, thresholds=(-1.0,))
    with pytest.raises(ValueError):
        pb3d.grid_surface_metrics(g, np.zeros((4, 5, 7), np.uint8))
    with pytest.raises(ValueError):
        pb3d.grid_surface_metrics(g, g, voxel_size=-1.0)
    with pytest.raises(TypeError):
        pb3d.distance_transform_resident(g)


# ---- GPU: the device against the restatement ----------------------------------------------------------------------------------------
def device_edt(grid, to, border=False, index=True):
    res = pb3d.distance_transform(grid, to=to, border=border, return_indices=index, squared=True)
    return res if index else (res, None)


def check_all_kinds(mask, what):
    """sq and index of a target mask, all three kinds, with and without border, index asked for and not"""
    for to in er.TARGETS:
        grid = er.grid_for(mask, to)
        esq, eidx = er.edt_grid(grid, to)
        sq, idx = device_edt(grid, to)
        assert np.array_equal(sq, esq), (what, to)
        assert np.array_equal(idx, eidx), (what, to)
        assert np.array_equal(device_edt(grid, to, index=False)[0], esq), (what, to)
        assert np.array_equal(device_edt(grid, to, border=True, index=False)[0], er.edt_grid(grid, to, True)[0]), (what, to)


def seam_mask(n2):
    """rows with targets either side of every word seam and at both ends, and a plane of rows without any in between"""
    m = np.zeros((3, 5, n2), bool)
    seams = [s for s in range(ROW_WORD // 2, n2 + 1, ROW_WORD // 2)]
    m[0, 0, [0, n2 - 1]] = True
    m[0, 1, [s - 1 for s in seams if s - 1 < n2]] = True
    m[0, 2, [s for s in seams if s < n2]] = True
    m[0, 3, n2 - 1] = True
    m[0, 4, 0] = True
    m[2] = np.random.default_rng(n2).random((5, n2)) < 0.05
    m[2, 2] = False
    return m


@gpu
@pytest.mark.parametrize("n2", [1, 31, 32, 33, 63, 64, 65, 70, 129])
def test_row_seams(n2):
    check_all_kinds(seam_mask(n2), n2)


@gpu
def test_row_group_seam():
    """a row longer than ROW_GROUP voxels: the nearest target lies in another 64-word group, whole empty words and groups in between"""
    n2 = ROW_GROUP + ROW_WORD + 40
    m = np.zeros((1, 3, n2), bool)
    m[0, 0, [10, n2 - 10]] = True
    m[0, 1, [ROW_GROUP - 1]] = True
    m[0, 2, [ROW_GROUP]] = True
    for to in ("occupied", "background"):
        grid = er.grid_for(m, to)
        esq, eidx = er.edt_grid(grid, to)
        sq, idx = device_edt(grid, to)
        assert np.array_equal(sq, esq) and np.array_equal(idx, eidx), to


@gpu
@pytest.mark.parametrize("shape", [(1, 1, 37), (37, 1, 1), (1, 37, 1), (1, 5, 7), (5, 1, 7), (5, 7, 1), (1, 1, 1)])
def test_degenerate_shapes(shape):
    for seed, density in enumerate((0.3, 0.05, 1.0, 0.0)):
        check_all_kinds(np.random.default_rng(seed).random(shape) < density, (shape, density))


@gpu
@pytest.mark.parametrize("axis", [0, 1])
def test_long_columns(axis):
    """columns of COLUMN_GROUP + 47 voxels, the other axes small: targets at the two ends and one off the middle, so the envelope holds
    parabolas from both ends and the answers of most voxels come from far away"""
    shape = [5, 5, 70]
    shape[axis] = n = COLUMN_GROUP + 47
    m = np.zeros(shape, bool)
    sl = [slice(None)] * 3
    for pos, k in ((0, 3), (n - 1, 40), (n // 2 + 5, 69), (COLUMN_GROUP - 1, 41), (COLUMN_GROUP, 42)):
        sl[axis] = pos
        m[tuple(sl)][2, k] = True
    check_all_kinds(m, axis)


@gpu
def test_longest_column():
    """an axis of MAX_AXIS voxels: stack levels at s, t up to 16383, squares up to 16383^2.  Expected by the pairs themselves"""
    shape = (MAX_AXIS, 1, 3)
    T = np.array([[0, 0, 0], [MAX_AXIS - 1, 0, 0], [8000, 0, 2]], np.int64)
    grid = np.zeros(shape, np.uint8)
    grid[tuple(T.T)] = 1
    v = np.stack(np.indices(shape), axis=-1).reshape(-1, 1, 3).astype(np.int64)
    d = ((v - T[None]) ** 2).sum(axis=-1)
    lin = (T[:, 0] * shape[1] + T[:, 1]) * shape[2] + T[:, 2]
    sq, idx = device_edt(grid, "occupied")
    assert np.array_equal(sq.reshape(-1), d.min(axis=1))
    assert np.array_equal(idx.reshape(-1), lin[d.argmin(axis=1)])       # T is in index order: the first minimum is the smallest index


@gpu
@pytest.mark.parametrize("case", sorted(MID_CASES))
def test_contents(case):
    for to in er.TARGETS:
        grid = er.grid_for(MID_CASES[case], to)
        esq, eidx = restated(case, to, False)
        d_grid = pb3d.device.DeviceGrid(pb3d.device.from_numpy(grid), grid.shape)
        try:
            d_sq, d_idx, stats = pb3d.distance_transform_resident(d_grid, to=to, return_indices=True, squared=True, return_stats=True)
            sq, idx = d_sq.download(grid.shape, np.int32), d_idx.download(grid.shape, np.int32)
            d_sq.free()
            d_idx.free()
        finally:
            d_grid.free()
        assert np.array_equal(sq, esq), to
        assert np.array_equal(idx, eidx), to
        finite = esq[esq != er.NONE]
        assert stats == {"targets": int(er.target_mask(grid, to).sum()), "max_sq": int(finite.max()) if len(finite) else -1}, to
        assert np.array_equal(device_edt(grid, to, index=False)[0], esq), to
        assert np.array_equal(device_edt(grid, to, border=True, index=False)[0], restated(case, to, True)[0]), to


@gpu
@pytest.mark.parametrize("case", ["random_0.5", "random_0.995", "pairs_all_axes", "none"])
def test_three_channels(case):
    """RGB grids, a third of the voxels with only the last byte set: the result is that of the occupancy"""
    for to in er.TARGETS:
        rgb = rgb_of(er.grid_for(MID_CASES[case], to))
        esq, eidx = restated(case, to, False)
        sq, idx = device_edt(rgb, to)
        assert np.array_equal(sq, esq) and np.array_equal(idx, eidx), to
        assert np.array_equal(device_edt(rgb, to, border=True, index=False)[0], restated(case, to, True)[0]), to


@gpu
def test_index_with_border_raises():
    g = er.grid_for(MID_CASES["random_0.5"], "background")
    with pytest.raises(ValueError):
        pb3d.distance_transform(g, border=True, return_indices=True)
    d = pb3d.device.from_numpy(g)
    sq = pb3d.device.DeviceBuffer(4 * g.size)
    try:
        rc = pb3d._lib.load().pb3d_edt_resident(pb3d._lib.ctx(), pd._ptr(d), 1, *g.shape, 0, 1, pd._ptr(sq), pd._ptr(sq), None)
        assert rc == -1
    finally:
        d.free()
        sq.free()


@gpu
@pytest.mark.parametrize("voxel_size", [1.0, 0.37])
def test_distances(voxel_size):
    for case in ("random_0.005", "corner", "none", "checkerboard"):
        grid = er.grid_for(MID_CASES[case], "background")
        esq = restated(case, "background", False)[0]
        want = np.sqrt(esq.astype(np.float64)) * voxel_size
        want[esq == er.NONE] = np.inf
        d64 = pb3d.distance_transform(grid, voxel_size=voxel_size)
        d32 = pb3d.distance_transform(grid, voxel_size=voxel_size, dtype=np.float32)
        assert d64.dtype == np.float64 and d32.dtype == np.float32
        assert np.array_equal(d64, want), case
        assert np.array_equal(d32, want.astype(np.float32)), case
        if voxel_size == 1.0 and (grid == 0).any():
            assert np.array_equal(d64, ndi.distance_transform_edt(grid)), case


def closing_fixture():
    """a solid box with a one-voxel pinhole and a two-voxel gap inside, labelled; and the box"""
    box = np.zeros((12, 13, 14), bool)
    box[2:10, 2:11, 2:12] = True
    grid = labels_of(box)
    grid[5, 5, 5] = 0
    grid[7, 7, 4:6] = 0
    return grid, box


MORPH_SHAPE = (20, 17, 36)


@functools.lru_cache(maxsize=None)
def morph_grid(kind):
    occ = ndi.binary_dilation(np.random.default_rng(5).random(MORPH_SHAPE) < 0.01, er.ball(5))
    occ &= np.random.default_rng(6).random(MORPH_SHAPE) < 0.97          # pinholes
    g = rgb_of(occ) if kind == "rgb" else labels_of(occ)
    g.setflags(write=False)
    return g


@gpu
@pytest.mark.parametrize("kind", ["rgb", "label"])
@pytest.mark.parametrize("radius", [1, 1.5, 3])
def test_morphology(kind, radius):
    g = morph_grid(kind)
    occ, r_sq, b = er.occupancy(g), er.radius_sq(radius), er.ball(er.radius_sq(radius))
    dil, ero, clo, ope = pb3d.dilate_grid(g, radius), pb3d.erode_grid(g, radius), pb3d.close_grid(g, radius), pb3d.open_grid(g, radius)
    assert np.array_equal(dil, er.dilate(g, r_sq))                      # the colours of the restated nearest voxel
    assert np.array_equal(ero, er.erode(g, r_sq))
    assert np.array_equal(clo, er.close(g, r_sq))
    assert np.array_equal(ope, er.open_(g, r_sq))
    assert np.array_equal(pb3d.erode_grid(g, radius, border=False), er.erode(g, r_sq, border=False))
    assert np.array_equal(er.occupancy(dil), ndi.binary_dilation(occ, b))
    assert np.array_equal(er.occupancy(ero), ndi.binary_erosion(occ, b, border_value=0))
    assert np.array_equal(er.occupancy(clo), ndi.binary_erosion(ndi.binary_dilation(occ, b), b, border_value=1))
    assert np.array_equal(er.occupancy(ope), ndi.binary_dilation(ndi.binary_erosion(occ, b, border_value=0), b))


@gpu
@pytest.mark.parametrize("kind", ["rgb", "label"])
def test_morphology_in_place(kind):
    g = morph_grid(kind)
    for fn, ref in ((pb3d.dilate_grid_resident, er.dilate), (pb3d.erode_grid_resident, er.erode), (pb3d.close_grid_resident, er.close),
                    (pb3d.open_grid_resident, er.open_)):
        d = pb3d.device.DeviceGrid(pb3d.device.from_numpy(g), g.shape)
        try:
            assert fn(d, 1.5, out=d) is d
            assert np.array_equal(d.numpy(), ref(g, 2)), fn.__name__
        finally:
            d.free()


@gpu
def test_closing_pinhole_and_gap():
    grid, box = closing_fixture()
    c1, c2 = pb3d.close_grid(grid, 1), pb3d.close_grid(grid, 1.5)
    assert c1[5, 5, 5] == grid[4, 5, 5]                                 # the pinhole takes its nearest voxel's label: the smallest index
    assert np.array_equal(c1, er.close(grid, 1)) and np.array_equal(c2, er.close(grid, 2))
    assert (c2[7, 7, 4:6] != 0).all()
    assert np.array_equal(c2 != 0, box) and np.array_equal((c1 != 0) | box, box)       # the outer boundary is unchanged
    assert np.array_equal(c2[grid != 0], grid[grid != 0])


def two_boxes():
    a, b = np.zeros((16, 15, 20), np.uint8), np.zeros((16, 15, 20), np.uint8)
    a[2:8, 3:9, 4:10] = 1
    b[2:8, 3:9, 7:13] = 1                                               # a moved by 3 along the last axis
    return a, b


TWO_BOX_SUMS = [152, 9, 452, 60, 92, 152]      # surface voxels, max sq, sum sq, #(sq <= 0), #(sq <= 1), #(sq <= 9)


def test_two_boxes_by_hand():
    """Two 6^3 boxes, b = a moved by 3 along axis 2 (a: k = 4..9, b: k = 7..12).  A 6^3 box has 6^3 - 4^3 = 152 surface voxels: two faces
    of 36 and four planes of 20 rim voxels.  a's surface against b's shell, plane by plane: k = 4 (a's face, 36 voxels) looks straight
    at b's face k = 7: sq 9; the rims of k = 5 and k = 6 (20 each): sq 4 and 1; the rims of k = 7, 8 and of the face k = 9 are voxels
    of b's rim: sq 0 (60 voxels); the 16 inner voxels of a's face k = 9 lie inside b, two planes behind its face k = 7: the 12 next
    to a side face have sq 1, the middle 4 have sq 4.  Sum 36*9 + 20*4 + 20*1 + 12*1 + 4*4 = 452; 60 + 20 + 12 = 92 within 1.  The
    mirror k -> 16 - k swaps the boxes, so b against a gives the same numbers."""
    a, b = two_boxes()
    assert er.surface_sums(a, b, [0, 1, 9]) == TWO_BOX_SUMS and er.surface_sums(b, a, [0, 1, 9]) == TWO_BOX_SUMS


@gpu
def test_surface_metrics_two_boxes():
    """the hand-derived sums of test_two_boxes_by_hand"""
    a, b = two_boxes()
    m = pb3d.grid_surface_metrics(a, b, thresholds=(0.0, 1.0, 3.0))
    n = np.float64(152)
    rms = float(np.sqrt(np.float64(452) / n))
    p = [float(np.float64(c) / n) for c in TWO_BOX_SUMS[3:]]
    assert m == {"hausdorff": 3.0, "hausdorff_ab": 3.0, "hausdorff_ba": 3.0, "rms_ab": rms, "rms_ba": rms, "surface_voxels_a": 152,
                 "surface_voxels_b": 152, "precision": p, "recall": p, "fscore": [2 * q * q / (q + q) for q in p]}
    assert m == er.surface_metrics(a, b, (0.0, 1.0, 3.0))


@gpu
def test_surface_metrics_self_and_empty():
    a, _ = two_boxes()
    rgb = rgb_of(a)
    m = pb3d.grid_surface_metrics(rgb, a, thresholds=(1.0, 2.0))
    assert m["hausdorff"] == m["rms_ab"] == m["rms_ba"] == 0.0
    assert m["precision"] == m["recall"] == m["fscore"] == [1.0, 1.0]
    e = np.zeros_like(a)
    m = pb3d.grid_surface_metrics(a, e)
    assert m == er.surface_metrics(a, e)
    assert m["precision"] == m["recall"] == m["fscore"] == [0.0]
    assert m["hausdorff_ab"] == math.inf and m["hausdorff_ba"] == 0.0 and m["surface_voxels_b"] == 0
    m = pb3d.grid_surface_metrics(e, e)
    assert m == er.surface_metrics(e, e) and m["hausdorff"] == 0.0


@gpu
@pytest.mark.parametrize("voxel_size", [1.0, 0.25])
def test_surface_metrics_random_pair(voxel_size):
    shape = (21, 18, 37)
    a = ndi.binary_dilation(np.random.default_rng(8).random(shape) < 0.004, er.ball(9)).astype(np.uint8)
    b = ndi.binary_dilation(np.random.default_rng(9).random(shape) < 0.004, er.ball(5)).astype(np.uint8)
    thr = (0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 4.0, 8.0)
    assert pb3d.grid_surface_metrics(a, rgb_of(b), thr, voxel_size) == er.surface_metrics(a, b, thr, voxel_size)


@gpu
def test_surface_extraction_at_faces_edges_corners():
    """a full grid: its surface is the grid's shell; with one inner voxel removed, also that voxel's six neighbours"""
    shape = (6, 5, 7)
    full = np.ones(shape, np.uint8)
    sq = pb3d.distance_transform(full, to="surface", squared=True)
    assert np.array_equal(sq, er.edt(er.surface(full != 0))[0])
    shell = np.ones(shape, bool)
    shell[1:-1, 1:-1, 1:-1] = False
    assert np.array_equal(sq == 0, shell)
    m = pb3d.grid_surface_metrics(full, full)
    assert m["surface_voxels_a"] == int(shell.sum()) == 6 * 5 * 7 - 4 * 3 * 5
    full[2, 2, 3] = 0
    assert pb3d.grid_surface_metrics(full, full)["surface_voxels_a"] == int(shell.sum()) + 6
    for shape in ((1, 1, 1), (1, 4, 5), (2, 2, 2)):
        assert pb3d.grid_surface_metrics(np.ones(shape, np.uint8), np.ones(shape, np.uint8))["surface_voxels_a"] == int(np.prod(shape))


@gpu
@pytest.mark.parametrize("offset", [1, 3])
@pytest.mark.parametrize("channels", [1, 3])
def test_odd_byte_offsets(offset, channels):
    """the grid (and the apply's output) start `offset` bytes into their allocation, guard bytes either side"""
    guard = 256
    occ = er.grid_for(MID_CASES["random_0.5"], "occupied")[:12, :9, :70]
    g = np.ascontiguousarray(rgb_of(occ) if channels == 3 else labels_of(occ))
    n, s = occ.size, occ.shape
    dev, lib, ctx = pb3d.device, pb3d._lib.load(), pb3d._lib.ctx()
    arena_in, arena_out = dev.DeviceBuffer(g.nbytes + 2 * guard + 8), dev.DeviceBuffer(g.nbytes + 2 * guard + 8)
    try:
        arena_in.upload(np.full(arena_in.nbytes, 0xFF, np.uint8))
        arena_in.upload(g, guard + offset)
        arena_out.upload(np.full(arena_out.nbytes, 0xA5, np.uint8))
        p_in, p_out = arena_in.at(guard + offset), arena_out.at(guard + offset)
        for to in range(3):
            d_sq, d_ix = pd._edt(p_in, channels, s, to, False, True)
            esq, eidx = er.edt_grid(g, er.TARGETS[to])
            assert np.array_equal(d_sq.download(s, np.int32), esq) and np.array_equal(d_ix.download(s, np.int32), eidx), to
            if to == 1:
                pd._apply(p_in, channels, n, d_sq, d_ix, pd.FILL, 2, p_out)
                out = arena_out.download((arena_out.nbytes,))
                assert np.array_equal(out[guard + offset:guard + offset + g.nbytes].reshape(g.shape), er.dilate(g, 2))
                assert (out[:guard + offset] == 0xA5).all() and (out[guard + offset + g.nbytes:] == 0xA5).all()
                out8 = (pb3d._lib.C.c_int64 * 11)()
                pb3d._lib.check(lib.pb3d_grid_surface_stats_resident(ctx, p_in, channels, *s, pd._ptr(d_sq), None, 0, out8))
                assert list(out8[:3]) == [int(er.surface(occ != 0).sum()), 0, 0]
            d_sq.free()
            d_ix.free()
        back = arena_in.download((arena_in.nbytes,))
        assert np.array_equal(back[guard + offset:guard + offset + g.nbytes].reshape(g.shape), g)
        assert (back[:guard + offset] == 0xFF).all() and (back[guard + offset + g.nbytes:] == 0xFF).all()
    finally:
        arena_in.free()
        arena_out.free()


@gpu
def test_resident_chain():
    """voxelize_mesh_resident -> close_grid_resident -> grid_overlap_counts_resident: the only downloads are the three counts"""
    dev = pb3d.device
    shape = (14, 15, 16)
    corners = np.array([[x, y, z] for x in (2.0, 10.0) for y in (3.0, 11.0) for z in (2.0, 12.0)])
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    faces = np.array([t for a, b, c, e in quads for t in ((a, b, c), (a, c, e))], np.int32)
    solid = pb3d.voxelize_mesh(corners, faces, shape)         # a box two voxels or more from every side of the grid
    holes = solid.copy()
    holes[5, 6, 7] = holes[8, 8, 5:7] = 0
    d_v, d_f, d_h = dev.from_numpy(corners), dev.from_numpy(faces), dev.from_numpy(holes)
    d_m = d_c = None
    try:
        d_m = pb3d.voxelize_mesh_resident(d_v, 8, d_f, 12, shape, verts_f64=True)
        pb3d.close_grid_resident(dev.DeviceGrid(d_h, shape), 1.5).free()       # warms the scratch slots
        before = dev.sync_count()
        d_c = pb3d.close_grid_resident(dev.DeviceGrid(d_h, shape), 1.5)
        assert dev.sync_count() == before                   # the closing only enqueues
        inter, na, nb = pb3d.grid_overlap_counts_resident(d_m, 1, d_c.buf, 1, solid.size)
        assert inter == na == nb == int(solid.sum())
        assert np.array_equal(d_c.numpy(), er.close(holes, 2))
    finally:
        for b in (d_v, d_f, d_h, d_m, d_c):
            if b is not None:
                b.free()
