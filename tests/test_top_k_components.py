"""extract_top_k_components (reference utils/voxel_utils.py:24-33) and the 6-, 18- and 26-connected labelling under it.

Expected values come from tests/golden/f13_top_k_components.json (captured from the reference by tools/gen_golden_topk.py) and from
scipy.ndimage.label called here."""
import hashlib
import json
import os

import numpy as np
import pytest
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
STRUCT = {6: ndimage.generate_binary_structure(3, 1), 18: ndimage.generate_binary_structure(3, 2), 26: ndimage.generate_binary_structure(3, 3)}
sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
_grids = {}


def _fixture():
    with open(os.path.join(GOLDEN, "f13_top_k_components.json")) as f:
        return json.load(f)


def _grid(mon):
    if mon not in _grids:
        _grids.clear()
        _grids[mon] = np.load(os.path.join(GOLDEN, f"stored_{mon}_voxel_grid.npz"))["voxel_grid"]
    return _grids[mon]


def ref_top_k(grid, color, k):
    """the reference's seven lines, restated (heights from find_objects instead of an argwhere per component)"""
    mask = np.all(grid == color, axis=-1)
    labeled, n = ndimage.label(mask, structure=np.ones((3, 3, 3)))
    heights = [(i + 1, s[1].stop - 1 - s[1].start) for i, s in enumerate(ndimage.find_objects(labeled))]
    top_ids = [idx for idx, _ in sorted(heights, key=lambda x: -x[1])[:k]]
    out = grid.copy()
    out[mask & ~np.isin(labeled, top_ids)] = 0
    return out


def scipy_stats(mask, conn):
    lab, n = ndimage.label(mask, structure=STRUCT[conn])
    bbox = np.array([[s[0].start, s[1].start, s[2].start, s[0].stop, s[1].stop, s[2].stop] for s in ndimage.find_objects(lab)], np.int64).reshape(-1, 6)
    f = lab.ravel()
    cnt = np.bincount(f, minlength=n + 1)[1:].astype(np.int64)
    idx = np.indices(mask.shape).reshape(3, -1)
    sums = np.stack([np.bincount(f, weights=idx[a], minlength=n + 1)[1:] for a in range(3)], 1).astype(np.int64)
    return lab, n, bbox, cnt, sums


# ---- CPU: the fixture against the restatement --------------------------------------------------------------------------------------
def test_fixture_matches_restatement_akbar():
    """the fixture pins the reference; the restatement used by the GPU tests below must agree with it"""
    import pb3d
    fx = _fixture()
    grid = _grid("Akbar")
    cases = [key for key in fx if key.startswith("Akbar/")]
    assert cases
    for key in cases:
        _, part, kk = key.split("/")
        color = pb3d.PART_COLORS[part]
        out = ref_top_k(grid, color, int(kk[1:]))
        assert sha(out) == fx[key]["sha256"], key
        mask = np.all(grid == color, axis=-1)
        assert ndimage.label(mask, structure=np.ones((3, 3, 3)))[1] == fx[key]["n26"], key


def test_fixture_full_building_needs_diagonals():
    """the full_building cases of Akbar, Bibi and Charminar: fewer 26-connected components than 6-connected ones"""
    import pb3d
    fx = _fixture()
    for mon in ("Akbar", "Bibi", "Charminar"):
        mask = np.all(_grid(mon) == pb3d.PART_COLORS["full_building"], axis=-1)
        assert ndimage.label(mask)[1] > fx[f"{mon}/full_building/k4"]["n26"], mon


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
def gpu_label(pb3d, grid, colors, conn, members_only=False, channels=3, cap=1024):
    from pb3d import device as dev
    from pb3d.voxel_utils import _label_stats_conn
    shape3 = grid.shape[:3]
    d_g = dev.from_numpy(grid); d_lab = dev.DeviceBuffer(max(1, int(np.prod(shape3))) * 4)
    try:
        if not members_only:
            d_lab.zero()
        res = _label_stats_conn(d_g, shape3, colors, d_lab, conn, cap=cap, members_only=members_only, channels=channels)
        lab = d_lab.download(shape3, np.int32) if np.prod(shape3) else np.zeros(shape3, np.int32)
        return lab, res
    finally:
        d_g.free(); d_lab.free()


def check_labelling(pb3d, grid, colors, conn, members_only=False, channels=3):
    lab, res = gpu_label(pb3d, grid, colors, conn, members_only, channels)
    anymask = np.zeros(grid.shape[:3], bool)
    for c, (n, bbox, cnt, sums) in zip(colors, res):
        mask = grid == c if channels == 1 else np.all(grid == np.asarray(c, np.uint8), axis=-1)
        anymask |= mask
        rl, rn, rb, rc, rs = scipy_stats(mask, conn)
        assert n == rn, (conn, n, rn)
        assert np.array_equal(lab[mask], rl[mask]), conn
        if rn <= 1024:
            assert np.array_equal(bbox, rb) and np.array_equal(cnt, rc) and np.array_equal(sums, rs), conn
    if not members_only:
        assert not np.any(lab[~anymask]), conn


@pytest.mark.gpu
@pytest.mark.parametrize("conn", [6, 18, 26])
def test_labelling_noise(pb3d_gpu, conn):
    rng = np.random.default_rng(130 + conn)
    col = np.array([253, 248, 96], np.uint8)
    for density in (0.05, 0.1, 0.2, 0.3):
        for shape in ((20, 24, 70), (7, 9, 130), (33, 17, 64)):
            g = np.zeros(shape + (3,), np.uint8)
            g[rng.random(shape) < density] = col
            check_labelling(pb3d_gpu, g, [col], conn)


@pytest.mark.gpu
@pytest.mark.parametrize("conn", [18, 26])
def test_labelling_constructed(pb3d_gpu, conn):
    col = np.array([1, 220, 5], np.uint8)
    cases = []
    # diagonal staircases across the 64-voxel window edges, along a1 and along a0
    for A2 in (64, 65, 128, 130):
        g = np.zeros((6, 6, A2, 3), np.uint8)
        for s in range(6):
            g[0, s, min(60 + s, A2 - 1)] = col
            g[s, 0, min(61 + s, A2 - 1)] = col
            g[s, s, (62 + s) % A2] = col
        cases.append(g)
    # rows whose runs are one empty voxel apart, against a run in the neighbour row that spans the gap (and the reverse)
    g = np.zeros((3, 3, 80, 3), np.uint8)
    g[0, 0, 10:20] = col; g[0, 0, 21:30] = col; g[0, 1, 19:22] = col
    g[1, 1, 40:44] = col; g[1, 1, 45:50] = col; g[2, 2, 44] = col
    g[0, 2, 60:63] = col; g[0, 2, 64:66] = col; g[1, 1, 63] = col
    cases.append(g)
    # contacts at a2 = 0 and a2 = A2 - 1 (and nothing past them)
    for A2 in (1, 2, 63, 64, 65):
        g = np.zeros((3, 3, A2, 3), np.uint8)
        g[0, 0, 0] = col; g[1, 1, 0] = col; g[0, 1, min(1, A2 - 1)] = col
        g[2, 2, A2 - 1] = col; g[1, 2, max(A2 - 2, 0)] = col; g[2, 0, A2 - 1] = col
        cases.append(g)
    for g in cases:
        check_labelling(pb3d_gpu, g, [col], conn)
        check_labelling(pb3d_gpu, g, [col], conn, members_only=True)


@pytest.mark.gpu
@pytest.mark.parametrize("A2", [1, 63, 64, 65, 130, 2049, 3000, 4096])
def test_labelling_row_lengths(pb3d_gpu, A2):
    """A2 > 2048 takes the generic face merge, the shorter rows the tile form: the diagonal links follow either"""
    rng = np.random.default_rng(A2)
    col = np.array([63, 138, 173], np.uint8)
    shape = (5, 6, A2)
    g = np.zeros(shape + (3,), np.uint8)
    g[rng.random(shape) < 0.15] = col
    for conn in (6, 18, 26):
        check_labelling(pb3d_gpu, g, [col], conn)


@pytest.mark.gpu
def test_labelling_degenerate_axes(pb3d_gpu):
    rng = np.random.default_rng(7)
    col = np.array([190, 0, 255], np.uint8)
    for shape in ((1, 1, 200), (200, 1, 1), (1, 200, 1), (1, 40, 70), (40, 1, 70), (40, 70, 1)):
        g = np.zeros(shape + (3,), np.uint8)
        g[rng.random(shape) < 0.4] = col
        for conn in (18, 26):
            check_labelling(pb3d_gpu, g, [col], conn)
    for shape in ((0, 5, 5, 3), (5, 0, 5, 3)):
        g = np.zeros(shape, np.uint8)
        assert pb3d_gpu.extract_top_k_components(g, col, k=1).shape == shape


@pytest.mark.gpu
@pytest.mark.parametrize("conn", [6, 18, 26])
def test_labelling_multi_colour_and_label_volume(pb3d_gpu, conn):
    rng = np.random.default_rng(40 + conn)
    pal = np.array([[253, 248, 96], [0, 0, 255], [255, 120, 230]], np.uint8)
    shape = (24, 19, 90)
    lab = rng.integers(0, 5, shape).astype(np.uint8)          # labels 0..4: 0 and 4 are not asked for
    table = np.concatenate([np.zeros((1, 3), np.uint8), pal, [[5, 223, 223]]]).astype(np.uint8)
    rgb = table[lab]
    check_labelling(pb3d_gpu, rgb, list(pal), conn)
    check_labelling(pb3d_gpu, rgb, list(pal), conn, members_only=True)
    check_labelling(pb3d_gpu, lab, [1, 2, 3], conn, channels=1)
    check_labelling(pb3d_gpu, lab, [2], conn, members_only=True, channels=1)


# ---- top-k semantics -----------------------------------------------------------------------------------------------------------
def scene(rng, shape=(40, 48, 90), nblobs=14):
    """boxes of one colour (heights with ties), diagonal-only joins, other colours around them"""
    col = np.array([253, 248, 96], np.uint8)
    g = np.zeros(shape + (3,), np.uint8)
    g[rng.random(shape) < 0.03] = (0, 0, 255)
    for _ in range(nblobs):
        h = int(rng.choice([1, 3, 3, 5, 8]))
        a0, a1, a2 = (int(rng.integers(0, s - 6)) for s in shape)
        g[a0:a0 + 3, a1:a1 + h, a2:a2 + 4] = col
        if rng.random() < 0.5:                                     # a diagonal neighbour: joins at 26 only
            g[min(a0 + 3, shape[0] - 1), min(a1 + h, shape[1] - 1), min(a2 + 4, shape[2] - 1)] = col
    g[rng.random(shape) < 0.01] = col
    return g, col


@pytest.mark.gpu
def test_top_k_semantics(pb3d_gpu):
    rng = np.random.default_rng(2024)
    for trial in range(3):
        g, col = scene(rng)
        n = ndimage.label(np.all(g == col, -1), structure=np.ones((3, 3, 3)))[1]
        before = g.copy()
        for k in (0, 1, 4, -1, -n, n, n + 5, -n - 3, 10 ** 30, -10 ** 30):
            got = pb3d_gpu.extract_top_k_components(g, col, k=k)
            assert got.flags.c_contiguous and got.dtype == np.uint8
            assert np.array_equal(got, ref_top_k(g, col, k)), (trial, k)
        assert np.array_equal(g, before)
    assert np.array_equal(pb3d_gpu.extract_top_k_components(g, col), ref_top_k(g, col, 4))       # k defaults to 4


@pytest.mark.gpu
def test_top_k_colours(pb3d_gpu):
    rng = np.random.default_rng(5)
    g, col = scene(rng)
    for c in ((1, 220, 5), (300, 0, 0), (-1, 0, 0), (0, 0, 0), (0, 0, 255), np.array([253, 248, 96])):
        for k in (0, 2):
            got = pb3d_gpu.extract_top_k_components(g, c, k=k)
            assert np.array_equal(got, ref_top_k(g, c, k)), (c, k)
            assert got is not g


@pytest.mark.gpu
def test_top_k_non_contiguous_input(pb3d_gpu):
    rng = np.random.default_rng(9)
    g, col = scene(rng)
    for view in (g.transpose(2, 1, 0, 3), np.flip(g, axis=1), g[::2, :, ::-1]):
        before = view.copy()
        got = pb3d_gpu.extract_top_k_components(view, col, k=2)
        assert np.array_equal(got, ref_top_k(np.ascontiguousarray(view), col, 2))
        assert np.array_equal(view, before)


@pytest.mark.gpu
def test_top_k_resident_and_labels(pb3d_gpu):
    from pb3d import device as dev
    from pb3d.labels import Palette, extract_top_k_components_labels, label_to_rgb, rgb_to_label
    rng = np.random.default_rng(11)
    g, col = scene(rng)
    pal = Palette.from_part_colors(pb3d_gpu.PART_COLORS)
    lab = rgb_to_label(g, pal)
    for k in (0, 3, -2):
        want = ref_top_k(g, col, k)
        dg = dev.DeviceGrid(dev.from_numpy(g), g.shape)
        try:
            out = pb3d_gpu.extract_top_k_components(dg, col, k=k)
            assert isinstance(out, dev.DeviceGrid) and out.shape == g.shape
            assert np.array_equal(out.numpy(), want) and np.array_equal(dg.numpy(), g)
            out.free()
        finally:
            dg.free()
        got = extract_top_k_components_labels(lab, pal.label_of("full_building"), k=k)
        assert np.array_equal(label_to_rgb(got, pal), want), k
    assert np.array_equal(extract_top_k_components_labels(lab, 300, k=0), lab)


@pytest.mark.gpu
def test_top_k_many_components(pb3d_gpu):
    """32 768 isolated voxels: more than the device records hold (the host decides); 3 000 components: past 2 048, decided on the device"""
    col = np.array([180, 140, 255], np.uint8)
    g = np.zeros((64, 64, 64, 3), np.uint8)
    g[::2, ::2, ::2] = col
    for k in (4, -1, 0, 40000):
        assert np.array_equal(pb3d_gpu.extract_top_k_components(g, col, k=k), ref_top_k(g, col, k)), k
    rng = np.random.default_rng(3)
    g = np.zeros((60, 64, 64, 3), np.uint8)
    g[::2, ::2, ::2][rng.random((30, 32, 32)) < 3000 / 30720] = col
    g[10:20:2, 10:14, 10] = col                                  # a few taller ones
    n = ndimage.label(np.all(g == col, -1), structure=np.ones((3, 3, 3)))[1]
    assert n > 2048
    for k in (100, -100, 1):
        assert np.array_equal(pb3d_gpu.extract_top_k_components(g, col, k=k), ref_top_k(g, col, k)), k


@pytest.mark.gpu
@pytest.mark.parametrize("mon", ["Akbar", "Bibi", "Charminar", "Itimad", "Taj"])
def test_top_k_golden(pb3d_gpu, mon):
    from pb3d import device as dev
    from pb3d.labels import Palette, extract_top_k_components_labels, label_to_rgb, rgb_to_label
    fx = _fixture()
    grid = _grid(mon)
    pal = Palette.from_part_colors(pb3d_gpu.PART_COLORS)
    lab = rgb_to_label(grid, pal)
    dg = dev.DeviceGrid(dev.from_numpy(grid), grid.shape)
    try:
        cases = [key for key in fx if key.startswith(mon + "/")]
        assert cases
        for key in cases:
            _, part, kk = key.split("/")
            k = int(kk[1:])
            color = pb3d_gpu.PART_COLORS[part]
            assert sha(pb3d_gpu.extract_top_k_components(grid, color, k=k)) == fx[key]["sha256"], key
            assert sha(label_to_rgb(extract_top_k_components_labels(lab, pal.label_of(part), k=k), pal)) == fx[key]["sha256"], key + " (labels)"
            out = pb3d_gpu.extract_top_k_components(dg, color, k=k)
            try:
                assert sha(out.numpy()) == fx[key]["sha256"], key + " (resident)"
            finally:
                out.free()
    finally:
        dg.free()


@pytest.mark.gpu
def test_labelling_26_at_1024(pb3d_gpu):
    """one 26-connected labelling of the synthetic 1024^3 carved grid's colour equals scipy's labels at the member voxels"""
    from pb3d import device as dev
    from pb3d.voxel_utils import _label_stats_conn
    S = 1024
    d_bhw = dev.DeviceBuffer(S * S); d_rgb = dev.DeviceBuffer(S * S * 3); d_mwh = dev.DeviceBuffer(S * S)
    d_col = dev.DeviceBuffer(S ** 3 * 3); d_lab = dev.DeviceBuffer(S ** 3 * 4)
    try:
        dev.synth_mask16(S, d_binary_hw=d_bhw, d_rgb_hw3=d_rgb, d_binary_wh=d_mwh)
        dev.global_carve(d_bhw, d_rgb, S, S, 90, d_col)
        col = np.array(pb3d_gpu.PART_COLORS["full_building"], np.uint8)
        n = _label_stats_conn(d_col, (S, S, S), [col], d_lab, 26, members_only=True)[0][0]
        mask = np.all(d_col.download((S, S, S, 3)) == col, axis=-1)
        d_col.free()
        lab = d_lab.download((S, S, S), np.int32)
        d_lab.free()
        ref, rn = ndimage.label(mask, structure=np.ones((3, 3, 3)))
        assert n == rn and rn > 0
        assert np.array_equal(lab[mask], ref[mask])
    finally:
        for b in (d_bhw, d_rgb, d_mwh, d_col, d_lab):
            b.free()
