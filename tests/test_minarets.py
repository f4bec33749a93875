"""Minaret extraction and keypoints (reference utils/camera_estimation.py:20-50, :176-216, :247-325, :329-344) and the member pass under
them (pb3d_component_members_dev).

Expected values come from tests/golden/f14_minarets.json (the reference's own extract_minaret_voxels_by_label and
extract_top_bottom_voxel_points, captured by tools/gen_golden_minarets.py) and from restatements with scipy.ndimage.label here.  The mask
side cannot be captured from the reference (it needs skimage): its restatement labels with structure=np.ones((3, 3)) -- skimage's
default 8-connectivity -- and takes areas and centroids from bincount."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MONUMENTS = ["Akbar", "Bibi", "Charminar", "Itimad", "Taj"]
FRONT, BACK = (0, 0, 255), (5, 223, 223)
sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _fixture():
    with open(os.path.join(GOLDEN, "f14_minarets.json")) as f:
        return json.load(f)


def _grid(mon):
    return np.load(os.path.join(GOLDEN, f"stored_{mon}_voxel_grid.npz"))["voxel_grid"]


def _mask(mon, view):
    from PIL import Image
    return np.array(Image.open(os.path.join(GOLDEN, f"data_{mon}_{view}_mask.png")).convert("RGB"))


# ---- restatements --------------------------------------------------------------------------------------------------------------------
def ref_voxels(grid, colors):
    """the reference's :176-216 with the per-component argwhere taken inside the component's box and np.ptp for ndarray.ptp"""
    comps = []
    for color in colors:
        mask = np.all(grid == np.asarray(color), axis=-1)
        lab, n = ndimage.label(mask)
        for cid, sl in enumerate(ndimage.find_objects(lab), 1):
            coords = np.argwhere(lab[sl] == cid) + np.array([s.start for s in sl])
            comps.append((coords.mean(axis=0), np.ptp(coords[:, 1]), coords))
    if len(comps) < 4:
        raise ValueError(f"Expected ≥4 minarets, found {len(comps)}")
    top4 = sorted(comps, key=lambda x: -x[1])[:4]
    centroids = np.stack([c[0] for c in top4])
    sets = [c[2] for c in top4]
    order_x = np.argsort(centroids[:, 0])
    left = sorted(order_x[:2], key=lambda i: centroids[i, 2])
    right = sorted(order_x[2:], key=lambda i: centroids[i, 2])
    return {"LM1": sets[left[0]], "LM2": sets[left[1]], "RM1": sets[right[0]], "RM2": sets[right[1]]}


def ref_masks(image, colors, min_area=50):
    rgb = image[:, :, :3]
    regions = []
    for ci, color in enumerate(colors):
        m = np.all(rgb == np.asarray(color), axis=-1)
        lab, n = ndimage.label(m, structure=np.ones((3, 3)))
        f = lab.ravel()
        rr, cc = np.indices(m.shape).reshape(2, -1)
        area = np.bincount(f, minlength=n + 1)
        sr = np.bincount(f, weights=rr, minlength=n + 1)
        sc = np.bincount(f, weights=cc, minlength=n + 1)
        for lbl in range(1, n + 1):
            if area[lbl] < min_area:
                continue
            regions.append({"ci": ci, "centroid": (sr[lbl] / area[lbl], sc[lbl] / area[lbl]), "mask": (lab == lbl).astype(np.uint8)})
    if len(regions) < 2:
        raise ValueError("Not enough minarets for camera alignment")
    regions.sort(key=lambda r: r["centroid"][1])
    mid = len(regions) // 2

    def pick(rs):
        if len(rs) == 1:
            return rs[0], None
        rs = sorted(rs, key=lambda r: (r["ci"], r["centroid"][0]))
        return rs[0], rs[1]

    lm1, lm2 = pick(regions[:mid])
    rm1, rm2 = pick(regions[mid:])
    return {k: r["mask"] for k, r in (("LM1", lm1), ("RM1", rm1), ("LM2", lm2), ("RM2", rm2)) if r is not None}


def ref_image_kps(masks):
    out = {}
    for name, mask in masks.items():
        ys, xs = np.nonzero(mask)
        out[f"{name}_top"] = (xs[ys == ys.min()].mean(), ys.min())
        out[f"{name}_bottom"] = (xs[ys == ys.max()].mean(), ys.max())
    return out


def _same_parts(got, want):
    assert list(got) == list(want)
    for k in want:
        assert got[k].dtype == np.int64 and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k


def _same_masks(got, want):
    assert list(got) == list(want)
    for k in want:
        assert got[k].dtype == np.uint8 and np.array_equal(got[k], want[k]), k


# ---- CPU -----------------------------------------------------------------------------------------------------------------------------
def test_fixture_matches_restatement_akbar():
    """the fixture pins the reference; the restatement used by the GPU tests below must agree with it"""
    fx = _fixture()["Akbar"]
    parts = ref_voxels(_grid("Akbar"), [FRONT, BACK])
    assert list(parts) == fx["keys"] == ["LM1", "LM2", "RM1", "RM2"]
    for k, v in parts.items():
        assert list(v.shape) == fx["parts"][k]["shape"] and sha(v) == fx["parts"][k]["sha256"]
        ys = v[:, 1]
        assert [float(x).hex() for x in v[ys == ys.min()].mean(axis=0)] == fx["kps"][f"{k}_bottom"]
        assert [float(x).hex() for x in v[ys == ys.max()].mean(axis=0)] == fx["kps"][f"{k}_top"]


def test_keypoint_helpers_on_host_arrays():
    """extract_top_bottom_*_points run on host arrays; the image sense of top (smallest y) is the opposite of the voxel one"""
    import pb3d
    vox = {"LM1": np.array([[1, 2, 3], [3, 2, 5], [0, 7, 1]], np.int64)}
    kv = pb3d.extract_top_bottom_voxel_points(vox)
    assert list(kv) == ["LM1_bottom", "LM1_top"]
    assert np.array_equal(kv["LM1_bottom"], [2.0, 2.0, 4.0]) and np.array_equal(kv["LM1_top"], [0.0, 7.0, 1.0])
    m = np.zeros((6, 5), np.uint8); m[1, 1:4] = 1; m[4, 0] = 1; m[4, 3] = 1
    ki = pb3d.extract_top_bottom_image_points({"RM2": m})
    assert list(ki) == ["RM2_top", "RM2_bottom"]
    assert ki["RM2_top"] == (2.0, 1) and ki["RM2_bottom"] == (1.5, 4)
    assert isinstance(ki["RM2_top"][0], np.float64) and isinstance(ki["RM2_top"][1], np.integer)


def test_install_patches_minaret_names():
    """install() rebinds the five names wherever the package holds them (camera_estimation and its star-importers)"""
    import sys
    import types
    import pb3d
    names = ["extract_minaret_voxels_by_label", "extract_minaret_masks_by_label", "extract_top_bottom_voxel_points",
             "extract_top_bottom_image_points", "extract_minaret_kps_for_view"]
    pkg = types.ModuleType("fakeutils_m")
    ce = types.ModuleType("fakeutils_m.camera_estimation"); ev = types.ModuleType("fakeutils_m.eval_helpers_intra")
    for n in names:
        setattr(ce, n, lambda *a: "old")
    ev.extract_minaret_voxels_by_label = ce.extract_minaret_voxels_by_label
    ev.extract_minaret_masks_by_label = ce.extract_minaret_masks_by_label
    ce.launch_smart_aligner = lambda *a: "kept"
    sys.modules["fakeutils_m"] = pkg; sys.modules["fakeutils_m.camera_estimation"] = ce; sys.modules["fakeutils_m.eval_helpers_intra"] = ev
    try:
        patched = pb3d.install(pkg)
        for n in names:
            assert ("fakeutils_m.camera_estimation", n) in patched and getattr(ce, n) is getattr(pb3d, n)
        assert ("fakeutils_m.eval_helpers_intra", "extract_minaret_masks_by_label") in patched
        assert ev.extract_minaret_voxels_by_label is pb3d.extract_minaret_voxels_by_label and ce.launch_smart_aligner() == "kept"
    finally:
        for m in ("fakeutils_m", "fakeutils_m.camera_estimation", "fakeutils_m.eval_helpers_intra"):
            del sys.modules[m]


# ---- GPU: the five stored grids ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mon", MONUMENTS)
def test_stored_grids_match_reference(pb3d_gpu, mon):
    fx = _fixture()[mon]
    parts = pb3d_gpu.extract_minaret_voxels_by_label(_grid(mon), [FRONT, BACK])
    assert list(parts) == fx["keys"]
    for k, v in parts.items():
        assert v.dtype == np.int64 and list(v.shape) == fx["parts"][k]["shape"] and sha(v) == fx["parts"][k]["sha256"], k
    kps = pb3d_gpu.extract_top_bottom_voxel_points(parts)
    assert list(kps) == list(fx["kps"])
    for k, v in kps.items():
        assert v.dtype == np.float64 and [float(x).hex() for x in v] == fx["kps"][k], k


# ---- GPU: synthetic fragments --------------------------------------------------------------------------------------------------------
A, B = (10, 20, 30), (40, 50, 60)


def _columns(shape, cols):
    """grid with axis-1 columns: cols = [(colour, a0, a2, y0, y1, w)], a w x w square section over rows [y0, y1)"""
    g = np.zeros(shape + (3,), np.uint8)
    for color, a0, a2, y0, y1, w in cols:
        g[a0:a0 + w, y0:y1, a2:a2 + w] = color
    return g


@pytest.mark.gpu
def test_more_components_than_records(pb3d_gpu):
    """2304 single voxels besides the minarets: the statistics overflow their records and the fallback decides"""
    g = _columns((96, 40, 96), [(A, 10, 10, 5, 35, 3), (A, 10, 80, 6, 36, 2), (A, 80, 10, 4, 30, 3), (A, 80, 80, 5, 33, 4)])
    g[0::2, 0, 0::2] = A
    assert ndimage.label(np.all(g == A, axis=-1))[1] > 2048
    _same_parts(pb3d_gpu.extract_minaret_voxels_by_label(g, [A, B]), ref_voxels(g, [A, B]))


@pytest.mark.gpu
def test_equal_heights_rank_colour_then_label(pb3d_gpu):
    g = _columns((40, 30, 40), [(B, 2, 2, 0, 20, 2), (A, 30, 30, 5, 25, 2), (A, 2, 30, 3, 23, 3), (A, 30, 2, 1, 21, 2), (B, 15, 15, 2, 22, 2)])
    got = pb3d_gpu.extract_minaret_voxels_by_label(g, [A, B])
    _same_parts(got, ref_voxels(g, [A, B]))
    # the three of A (colour first), then B's first label (raster order: the one at a0 = 2)
    firsts = sorted(tuple(v[0]) for v in got.values())
    assert firsts == sorted([(2, 0, 2), (30, 5, 30), (2, 3, 30), (30, 1, 2)])


@pytest.mark.gpu
def test_fewer_than_four_raises(pb3d_gpu):
    g = _columns((20, 20, 20), [(A, 1, 1, 0, 10, 2), (B, 10, 10, 0, 10, 2), (A, 15, 1, 0, 5, 2)])
    with pytest.raises(ValueError, match="Expected ≥4 minarets, found 3"):
        pb3d_gpu.extract_minaret_voxels_by_label(g, [A, B])
    with pytest.raises(ValueError, match="found 0"):
        pb3d_gpu.extract_minaret_voxels_by_label(np.zeros((0, 4, 4, 3), np.uint8), [A, B])


@pytest.mark.gpu
def test_duplicated_and_out_of_range_colours(pb3d_gpu):
    g = _columns((30, 30, 30), [(A, 2, 2, 0, 20, 2), (A, 20, 20, 3, 18, 3)])
    for colors in ([A, A], [A, (300, 0, 0), A], [(-1, 20, 30), A, A]):
        _same_parts(pb3d_gpu.extract_minaret_voxels_by_label(g, colors), ref_voxels(g, colors))
    with pytest.raises(ValueError, match="found 2"):
        pb3d_gpu.extract_minaret_voxels_by_label(g, [A, (256, 20, 30)])


@pytest.mark.gpu
def test_edge_and_corner_contacts_stay_apart(pb3d_gpu):
    """6-connectivity: columns touching along an edge or at a corner are separate components"""
    g = _columns((24, 30, 24), [(A, 4, 4, 0, 20, 2), (A, 6, 6, 2, 25, 2), (A, 14, 4, 0, 10, 2), (A, 14, 14, 0, 12, 2)])
    g[16, 12, 16] = A          # touches the last column only at a corner
    g[13, 3, 3] = A            # and one voxel along an edge of the third
    got = pb3d_gpu.extract_minaret_voxels_by_label(g, [A])
    _same_parts(got, ref_voxels(g, [A]))
    assert sorted(len(v) for v in got.values()) == [40, 48, 80, 92]


@pytest.mark.gpu
def test_device_grid_and_many_colours(pb3d_gpu):
    """a DeviceGrid gives what the NumPy grid gives (and is left as it was); ten colours are labelled in two chunks, and minarets taken
    from both chunks re-make the earlier labelling"""
    from pb3d import device as dev
    cols = [(i * 20, 7, 9) for i in range(10)]
    heights = [10, 17, 24, 31, 13, 20, 27, 12, 16, 35]          # the tallest is in the second chunk, the next three in the first
    g = _columns((60, 40, 60), [(cols[i], 5 * i, (13 * i) % 50, 0, heights[i], 2) for i in range(10)])
    want = ref_voxels(g, cols)
    d = dev.DeviceGrid(dev.from_numpy(g), g.shape)
    try:
        _same_parts(pb3d_gpu.extract_minaret_voxels_by_label(d, cols), want)
        assert np.array_equal(d.numpy(), g)
    finally:
        d.free()
    _same_parts(pb3d_gpu.extract_minaret_voxels_by_label(g, cols), want)
    _same_parts(pb3d_gpu.extract_minaret_voxels_by_label(g[:, :, :53], cols), ref_voxels(g[:, :, :53], cols))


def _box_filling_component(shape):
    """One 6-connected component whose bounding box is the whole grid, with 4096-voxel blocks of its box that hold every voxel, none,
    and something in between: a spine along axis 0 with three lines from the origin, ten full slices, twenty comb slices (a wall at
    a2 = 0 and every third row to a varying length) and a full last slice behind a slice that holds the spine alone."""
    A0, A1, A2 = shape
    m = np.zeros(shape, bool)
    m[:, 0, 0] = m[0, :, 0] = m[0, 0, :] = True
    m[10:20] = True
    a1 = np.arange(0, A1, 3)
    for a0 in range(40, 60):
        m[a0, :, 0] = True
        m[a0, a1] |= np.arange(A2)[None, :] < ((a0 * 7 + a1 * 13) % A2)[:, None]
    m[A0 - 1] = True
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("shape, nblocks", [((168, 168, 168), 1158), ((128, 128, 256), 1024)])
def test_members_of_a_box_of_many_blocks(pb3d_gpu, shape, nblocks):
    """The member pass scans its per-block counts in one 1024-thread workgroup (k_members_scan, csrc/wave.h's group_scan_array).  A box
    of 168^3 voxels is 1158 blocks of 4096 -- two per thread with a ragged last thread and a ragged last block -- and one of
    128 x 128 x 256 is exactly 1024, one per thread with no slack.  The big component's colour is labelled in the first chunk of eight
    colours and the three small ones in the second, so its box is a launch of its own.  Coordinates in np.argwhere order, exactly."""
    big = (250, 7, 9)
    small = [(i * 20, 7, 9) for i in (8, 9, 10)]
    colours = [big] + [(i * 20, 7, 9) for i in range(1, 8)] + small          # 1 .. 7 colour nothing
    m = _box_filling_component(shape)
    per_block = np.add.reduceat(m.ravel().astype(np.int64), np.arange(0, m.size, 4096))          # the box is the grid: box raster = grid raster
    assert len(per_block) == nblocks and per_block.min() == 0 and per_block.max() == 4096 and ((per_block > 0) & (per_block < 4096)).any()
    g = np.zeros(shape + (3,), np.uint8)
    g[m] = big
    for i, c in enumerate(small):
        g[100:102, 50:55 + i, 60 + 10 * i:62 + 10 * i] = c
    assert ndimage.label(np.all(g == big, axis=-1))[1] == 1
    got = pb3d_gpu.extract_minaret_voxels_by_label(g, colours)
    assert list(got) == ["LM1", "LM2", "RM1", "RM2"]
    seen = set()
    for name, v in got.items():
        colour = tuple(int(x) for x in g[tuple(v[0])])
        seen.add(colour)
        want = np.argwhere(np.all(g == colour, axis=-1))
        assert v.dtype == np.int64 and v.shape == want.shape and np.array_equal(v, want), (name, colour)
    assert seen == {big, *small}


# ---- GPU: masks ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("view", ["front", "drone"])
@pytest.mark.parametrize("mon", MONUMENTS)
def test_real_masks(pb3d_gpu, mon, view):
    img = _mask(mon, view)
    want = ref_masks(img, [FRONT, BACK])
    _same_masks(pb3d_gpu.extract_minaret_masks_by_label(img, [FRONT, BACK]), want)
    if (mon, view) == ("Taj", "drone"):        # four front regions, two of them single pixels that min_area drops, and one back region
        assert list(want) == ["LM1", "RM1", "RM2"]


def _blobs(shape, blobs):
    img = np.zeros(shape + (3,), np.uint8)
    for color, r0, r1, c0, c1 in blobs:
        img[r0:r1, c0:c1] = color
    return img


@pytest.mark.gpu
def test_mask_edge_cases(pb3d_gpu):
    img = _blobs((40, 60), [(A, 2, 12, 2, 7), (A, 20, 30, 40, 45), (B, 5, 15, 20, 25)])
    # RGBA: the alpha channel is ignored
    rgba = np.concatenate([img, np.full((40, 60, 1), 7, np.uint8)], axis=-1)
    _same_masks(pb3d_gpu.extract_minaret_masks_by_label(rgba, [A, B]), ref_masks(img, [A, B]))
    # area == min_area is kept, min_area - 1 dropped (each blob has 50 pixels)
    assert len(pb3d_gpu.extract_minaret_masks_by_label(img, [A, B], min_area=50)) == 3
    with pytest.raises(ValueError, match="Not enough minarets for camera alignment"):
        pb3d_gpu.extract_minaret_masks_by_label(img, [A, B], min_area=51)
    # three regions: the odd split puts one on the left and two on the right
    got = pb3d_gpu.extract_minaret_masks_by_label(img, [A, B])
    assert list(got) == ["LM1", "RM1", "RM2"]
    _same_masks(got, ref_masks(img, [A, B]))
    # a single region
    with pytest.raises(ValueError, match="Not enough minarets"):
        pb3d_gpu.extract_minaret_masks_by_label(_blobs((40, 60), [(A, 2, 12, 2, 7)]), [A, B])
    # diagonal-only contact joins at 8-connectivity: two squares meeting at a corner are one region
    diag = _blobs((40, 60), [(A, 2, 9, 2, 9), (A, 9, 16, 9, 16), (B, 20, 30, 40, 50)])
    got = pb3d_gpu.extract_minaret_masks_by_label(diag, [A, B])
    _same_masks(got, ref_masks(diag, [A, B]))
    assert int(got["LM1"].sum()) == 98
    # a repeated colour and one out of range
    for colors in ([A, A, B], [(300, 0, 0), B, A]):
        _same_masks(pb3d_gpu.extract_minaret_masks_by_label(img, colors), ref_masks(img, colors))


# ---- GPU: end to end -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_kps_for_view_taj_front(pb3d_gpu):
    grid, img = _grid("Taj"), _mask("Taj", "front")
    vs, im = pb3d_gpu.extract_minaret_kps_for_view(grid, img, [FRONT, BACK])
    parts = ref_voxels(grid, [FRONT, BACK])
    masks = ref_masks(img, [FRONT, BACK])
    common = [k for k in ("LM1", "LM2", "RM1", "RM2") if k in masks]
    keys = [f"{m}_{e}" for m in common for e in ("bottom", "top") if "1" in m or e == "top"]
    assert list(vs) == keys and list(im) == keys
    ik = ref_image_kps(masks)
    for k in keys:
        m, e = k.split("_")
        v = parts[m]
        ys = v[:, 1]
        want = v[ys == (ys.min() if e == "bottom" else ys.max())].mean(axis=0)
        assert vs[k].dtype == np.float64 and [float(x).hex() for x in vs[k]] == [float(x).hex() for x in want], k
        assert float(im[k][0]).hex() == float(ik[k][0]).hex() and im[k][1] == ik[k][1], k
        assert isinstance(im[k][0], np.float64) and isinstance(im[k][1], np.integer)
    # the voxel keypoints are those of the coordinate sets
    fx = _fixture()["Taj"]["kps"]
    assert all([float(x).hex() for x in vs[k]] == fx[k] for k in keys)


@pytest.mark.gpu
def test_kps_for_view_errors(pb3d_gpu):
    g = _columns((40, 30, 40), [(A, 2, 2, 0, 20, 2), (A, 30, 30, 5, 25, 2), (A, 2, 30, 3, 23, 3), (A, 30, 2, 1, 21, 2)])
    with pytest.raises(ValueError, match="Not enough minarets for camera alignment"):
        pb3d_gpu.extract_minaret_kps_for_view(g, _blobs((40, 60), [(A, 2, 12, 2, 7)]), [A, B])
    # two front regions: LM1 and RM1, both keypoints of each
    vs, im = pb3d_gpu.extract_minaret_kps_for_view(g, _blobs((40, 60), [(A, 2, 12, 2, 7), (A, 2, 12, 40, 45)]), [A, B])
    assert list(vs) == ["LM1_bottom", "LM1_top", "RM1_bottom", "RM1_top"] == list(im)


# ---- GPU: the C entry ----------------------------------------------------------------------------------------------------------------
def _members_call(lib, ctx, d_g, shape, d_lab, colors, labels, bbox, counts, outputs, d_coords, d_rows, d_masks, channels=3):
    nsel = len(labels)
    cols = np.ascontiguousarray(np.asarray(colors, np.uint8).reshape(-1))
    lab = np.ascontiguousarray(labels, np.int32)
    bb = np.ascontiguousarray(np.asarray(bbox, np.int64).reshape(-1))
    cnt = None if counts is None else np.ascontiguousarray(counts, np.int64)
    import pb3d
    p = lambda b: None if b is None else C.c_void_p(b.ptr)
    return lib.pb3d_component_members_dev(ctx, p(d_g), *shape, channels, p(d_lab), nsel, pb3d._lib.p_u8(cols) if cols.size else None,
                                          lab.ctypes.data_as(C.POINTER(C.c_int32)), bb.ctypes.data_as(pb3d._lib.i64p),
                                          None if cnt is None else cnt.ctypes.data_as(pb3d._lib.i64p), outputs, p(d_coords), p(d_rows),
                                          p(d_masks))


@pytest.mark.gpu
def test_members_entry_direct(pb3d_gpu):
    """output (c) of a 26-connected (1, H, W) labelling, all three outputs together, and the PB3D_EINVAL cases"""
    from pb3d import device as dev
    from pb3d.voxel_utils import _label_stats_conn
    lib, ctx = pb3d_gpu._lib.load(), pb3d_gpu._lib.ctx()
    rng = np.random.default_rng(5)
    img = np.where(rng.random((37, 71, 1)) < 0.45, np.array(A, np.uint8), np.array(B, np.uint8)).astype(np.uint8)
    shape = (1, 37, 71)
    d_g = dev.from_numpy(img); d_lab = dev.DeviceBuffer(37 * 71 * 4)
    d_coords = dev.DeviceBuffer(37 * 71 * 24); d_rows = dev.DeviceBuffer(8 * 64); d_masks = dev.DeviceBuffer(8 * 37 * 71)
    try:
        st = _label_stats_conn(d_g, shape, [A, B], d_lab, 26, cap=4096, members_only=True)
        ref = {c: ndimage.label(np.all(img == c, axis=-1), structure=np.ones((3, 3))) for c in (A, B)}
        sel = [(A, 1), (B, 1), (A, ref[A][1]), (B, ref[B][1])]
        recs = {A: st[0], B: st[1]}
        bbox = [recs[c][1][l - 1] for c, l in sel]
        counts = [int(recs[c][2][l - 1]) for c, l in sel]
        assert _members_call(lib, ctx, d_g, shape, d_lab, [c for c, _ in sel], [l for _, l in sel], bbox, counts, 7, d_coords, d_rows, d_masks) == 0
        masks = d_masks.download((4, 37, 71), np.uint8)
        rows = d_rows.download((4, 2, 4), np.int64)
        xyz = d_coords.download((sum(counts), 3), np.int64)
        off = 0
        for q, (c, l) in enumerate(sel):
            want = (ref[c][0] == l).astype(np.uint8)
            assert np.array_equal(masks[q], want), q
            coords = np.argwhere(want[None])
            assert np.array_equal(xyz[off:off + counts[q]], coords), q
            off += counts[q]
            for e, r in ((0, coords[:, 1].min()), (1, coords[:, 1].max())):
                on = coords[coords[:, 1] == r]
                assert rows[q, e, 0] == len(on) and list(rows[q, e, 1:]) == list(on.sum(axis=0)), (q, e)
        # refused: more than eight selections, a box outside the grid, a requested output without its buffer
        nine = [A] * 9
        assert _members_call(lib, ctx, d_g, shape, d_lab, nine, [1] * 9, [bbox[0]] * 9, [counts[0]] * 9, 4, None, None, d_masks) == -1
        assert "at most 8" in lib.pb3d_last_error().decode()
        for bad in ([0, 0, 0, 1, 38, 71], [0, -1, 0, 1, 5, 5], [0, 0, 0, 2, 1, 1], [0, 5, 0, 1, 4, 1]):
            assert _members_call(lib, ctx, d_g, shape, d_lab, [A], [1], [bad], [1], 4, None, None, d_masks) == -1
            assert "outside the grid" in lib.pb3d_last_error().decode()
        for outputs, bufs in ((1, (None, d_rows, d_masks)), (2, (d_coords, None, d_masks)), (4, (d_coords, d_rows, None))):
            assert _members_call(lib, ctx, d_g, shape, d_lab, [A], [1], [bbox[0]], [counts[0]], outputs, *bufs) == -1
            assert "null buffer" in lib.pb3d_last_error().decode()
        assert _members_call(lib, ctx, d_g, shape, d_lab, [A], [1], [bbox[0]], None, 1, d_coords, None, None) == -1
        dev.sync()
    finally:
        for b in (d_g, d_lab, d_coords, d_rows, d_masks):
            b.free()
