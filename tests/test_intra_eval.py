"""Notebook 4 (intra-method analysis, reference utils/eval_helpers_intra.py:287-748) and the grid-direct visibility kernels under it
(csrc/visibility.hip).

tests/golden/n4_intra_tables.json holds the three tables as notebook 4's saved outputs print them (and the "Mask resized" lines).  The
restatement below is the reference's arithmetic in NumPy (float32 points and camera as load_camera_json casts them, OpenCV's nearest
index rule, the int64 minaret sets of np.argwhere); on the CPU it reproduces the Akbar cells, on the GPU pb3d must reproduce every cell
from the fixtures alone."""
import ctypes as C
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MONUMENTS = ["Taj", "Bibi", "Itimad", "Akbar", "Charminar"]
SHORT = {"Taj": "TM", "Bibi": "BkM", "Itimad": "IuD", "Akbar": "AT", "Charminar": "CM"}
MINARETS = ["LM1", "RM1", "LM2", "RM2"]
PARTS = ["dome", "chhatris", "main_door", "windows", "plinth"]
BACK_TOP_ONLY = {"Itimad": True, "Akbar": True, "Charminar": True, "Taj": False, "Bibi": False}


def _tables():
    with open(os.path.join(GOLDEN, "n4_intra_tables.json"), encoding="utf-8") as f:
        return json.load(f)


def _grid(mon, deformed=False):
    name = f"stored_{mon}_deformed_voxel_grid.npz" if deformed else f"stored_{mon}_voxel_grid.npz"
    with np.load(os.path.join(GOLDEN, name)) as f:
        return f["voxel_grid"]


def _cam(mon, tag, view="front"):
    with open(os.path.join(GOLDEN, f"stored_{mon}_camera_params_{tag}.json")) as f:
        c = json.load(f)[view]
    return {"cam_pos": np.array(c["cam_pos"], np.float32), "target": np.array(c["target"], np.float32), "f": float(c["f"]),
            "cx": float(c["cx"]), "cy": float(c["cy"])}


def _raw_mask(mon, view="front"):
    from PIL import Image
    return np.array(Image.open(os.path.join(GOLDEN, f"data_{mon}_{view}_mask.png")).convert("RGB"))


def _resized_mask(mon, grid_shape, view="front"):
    """cv2.resize(..., INTER_NEAREST) to round(side * max(grid) / max(mask))"""
    m = _raw_mask(mon, view)
    h, w = m.shape[:2]
    s = max(grid_shape[:3]) / max(h, w)
    nw, nh = int(round(w * s)), int(round(h * s))
    xs = np.minimum(np.floor(np.arange(nw) * (1.0 / (nw / float(w)))).astype(np.int64), w - 1)
    ys = np.minimum(np.floor(np.arange(nh) * (1.0 / (nh / float(h)))).astype(np.int64), h - 1)
    return np.ascontiguousarray(m[ys][:, xs])


# ---- NumPy restatement of the reference's visibility (:134-190) ------------------------------------------------------------------------
def _look_at(eye, target):
    from pb3d.camera_geometry import look_at_rotation       # host NumPy, the reference's :3-14 line for line
    return look_at_rotation(eye, target)


def _project(pts, cam, H, W):
    R = _look_at(cam["cam_pos"], cam["target"])
    X, Y, Z = ((pts - cam["cam_pos"]) @ R.T).T
    valid = Z > 1e-6
    X, Y, Z = X[valid], Y[valid], Z[valid]
    ui = np.round((X / Z) * cam["f"] + cam["cx"]).astype(int)
    vi = np.round(-(Y / Z) * cam["f"] + cam["cy"]).astype(int)
    inside = (ui >= 0) & (ui < W) & (vi >= 0) & (vi < H)
    return ui[inside], vi[inside], Z[inside]


def ref_zbuf(grid, cam, H, W):
    z, y, x = np.where(np.any(grid > 0, axis=-1))
    ui, vi, Z = _project(np.stack([x, y, z], axis=1).astype(np.float32), cam, H, W)
    zb = np.full((H, W), np.inf, np.float32)
    np.minimum.at(zb, (vi, ui), Z.astype(np.float32))
    return zb


def ref_visible(pts, cam, zbuf, H, W, eps=1e-3):
    ui, vi, Z = _project(pts, cam, H, W)
    m = np.zeros((H, W), bool)
    m[vi[np.abs(Z - zbuf[vi, ui]) < eps], ui[np.abs(Z - zbuf[vi, ui]) < eps]] = True
    return m


def _part_pts(grid, colours):
    mask = np.zeros(grid.shape[:3], bool)
    for c in colours:
        mask |= np.all(grid == c, axis=-1)
    z, y, x = np.where(mask)
    return np.stack([x, y, z], axis=1).astype(np.float32)


def _iou(a, b):
    inter, union = np.logical_and(a, b).sum(), np.logical_or(a, b).sum()
    return inter / union if union > 0 else np.nan


def ref_part_cells(mon, PC):
    gi, gd = _grid(mon), _grid(mon, True)
    mask = _resized_mask(mon, gi.shape)
    H, W = mask.shape[:2]
    cam = _cam(mon, "final")
    zi, zd = ref_zbuf(gi, cam, H, W), ref_zbuf(gd, cam, H, W)
    cells = {}
    for part in PARTS:
        gt = np.all(mask == PC[part], axis=-1)
        pi, pd = _part_pts(gi, [PC[part]]), _part_pts(gd, [PC[part]])
        if gt.sum() == 0 or len(pi) == 0:
            cells[part] = "--"
            continue
        cells[part] = f"{_iou(gt, ref_visible(pi, cam, zi, H, W)):.3f}→{_iou(gt, ref_visible(pd, cam, zd, H, W)):.3f}"
    mc = [PC["front_minarets"], PC["back_minarets"]]
    pm = _part_pts(gi, mc)
    gt = np.all(mask == mc[0], axis=-1) | np.all(mask == mc[1], axis=-1)
    cells["minarets"] = f"{_iou(gt, ref_visible(pm, cam, zi, H, W)):.3f}→{_iou(gt, ref_visible(pm, cam, zd, H, W)):.3f}"
    cols = np.unique(gi.reshape(-1, 3), axis=0)
    cols = cols[~np.all(cols == 0, axis=1)]
    gt = np.zeros((H, W), bool)
    for c in cols:
        gt |= np.all(mask == c, axis=-1)
    occ_i = np.stack(np.where(np.any(gi > 0, axis=-1))[::-1], axis=1).astype(np.float32)
    occ_d = np.stack(np.where(np.any(gd > 0, axis=-1))[::-1], axis=1).astype(np.float32)
    cells["whole"] = f"{_iou(gt, ref_visible(occ_i, cam, zi, H, W)):.3f}→{_iou(gt, ref_visible(occ_d, cam, zd, H, W)):.3f}"
    return cells


def ref_minaret_parts(mon, PC):
    from test_minarets import ref_masks, ref_voxels
    g = _grid(mon)
    mask = _resized_mask(mon, g.shape)
    mc = [PC["front_minarets"], PC["back_minarets"]]
    return g, mask, ref_voxels(g, mc), ref_masks(mask, mc)


def ref_iou_cells(mon, PC):
    g, mask, vox, msk = ref_minaret_parts(mon, PC)
    H, W = mask.shape[:2]
    iou = {m: {} for m in MINARETS}
    for tag in ("init", "kp", "final"):
        cam = _cam(mon, tag)
        zb = ref_zbuf(g, cam, H, W)
        pr_all = ref_visible(np.vstack([vox[m] for m in MINARETS]), cam, zb, H, W)
        for m in MINARETS:
            iou[m][tag] = _iou(msk[m].astype(bool) & pr_all, ref_visible(vox[m], cam, zb, H, W))
    cells = {m: f"{iou[m]['init']:.3f}→{iou[m]['kp']:.3f}→{iou[m]['final']:.3f}" for m in MINARETS}
    cells["Average"] = "→".join(f"{np.mean([iou[m][t] for m in MINARETS]):.3f}" for t in ("init", "kp", "final"))
    return cells


def ref_kp_cells(mon, PC):
    from pb3d.camera_geometry import project
    from test_minarets import ref_image_kps
    _, _, vox, msk = ref_minaret_parts(mon, PC)
    vkp = {}
    for name, v in vox.items():
        ys = v[:, 1]
        vkp[f"{name}_bottom"] = v[ys == ys.min()].mean(axis=0)
        vkp[f"{name}_top"] = v[ys == ys.max()].mean(axis=0)
    ikp = ref_image_kps(msk)
    err = {}
    for tag in ("init", "kp"):
        cam = _cam(mon, tag)
        proj = {k: project(p, cam["cam_pos"], cam["target"], cam["f"], cam["cx"], cam["cy"]) for k, p in vkp.items()}
        err[tag] = {}
        for m in MINARETS:
            e = [np.linalg.norm(np.array(ikp[f"{m}_top"]) - np.array(proj[f"{m}_top"]))]
            if not (m in ["LM2", "RM2"] and BACK_TOP_ONLY[mon]):
                e.append(np.linalg.norm(np.array(ikp[f"{m}_bottom"]) - np.array(proj[f"{m}_bottom"])))
            err[tag][m] = np.mean(e)
    cells = {m: f"{err['init'][m]:.2f}→{err['kp'][m]:.2f}" for m in MINARETS}
    cells["Average"] = f"{np.mean(list(err['init'].values())):.2f}→{np.mean(list(err['kp'].values())):.2f}"
    return cells


def _want(table, mon):
    t = _tables()[table]["rows"]
    return {row: t[row][SHORT[mon]] for row in t}


# ---- CPU -----------------------------------------------------------------------------------------------------------------------------
def test_restatement_reproduces_akbar_tables():
    from pb3d.config import PART_COLORS as PC
    assert ref_kp_cells("Akbar", PC) == _want("minaret_kp", "Akbar")
    assert ref_iou_cells("Akbar", PC) == _want("minaret_iou", "Akbar")
    assert ref_part_cells("Akbar", PC) == _want("part_minaret_binary", "Akbar")


def test_resize_mask_to_voxel_grid_lines(capsys):
    from pb3d import eval_helpers_intra as ev
    lines = []
    for mon in MONUMENTS:
        g = _grid(mon)
        got = ev.resize_mask_to_voxel_grid(_raw_mask(mon), g)
        lines.append(capsys.readouterr().out.strip())
        assert np.array_equal(got, _resized_mask(mon, g.shape))
    assert lines == _tables()["mask_resized"]
    assert lines[0] == "Mask resized: (660,1214) → (278,512) | scale=0.422"


def test_loaders_and_iou_helper(tmp_path):
    from pb3d import eval_helpers_intra as ev
    cam = ev.load_camera_json(os.path.join(GOLDEN, "stored_Bibi_camera_params_init.json"), "front")
    assert cam["cam_pos"].dtype == np.float32 and cam["target"].dtype == np.float32 and type(cam["f"]) is float
    with pytest.raises(KeyError):
        ev.load_camera_json(os.path.join(GOLDEN, "stored_Bibi_camera_params_init.json"), "side")
    with pytest.raises(FileNotFoundError):
        ev.load_camera_json(str(tmp_path / "missing.json"), "front")
    assert np.isnan(ev._iou_bool(np.zeros(4, bool), np.zeros(4, bool)))
    assert ev._iou_bool(np.array([1, 1, 0], bool), np.array([1, 0, 0], bool)) == 0.5
    assert np.array_equal(ev.load_voxel_grid(os.path.join(GOLDEN, "stored_Akbar_voxel_grid.npz")), _grid("Akbar"))


def test_install_names():
    import pb3d
    names = pb3d._PATCH["eval_helpers_intra"]
    for n in ("run_minaret_kp_evaluation", "run_minaret_iou_evaluation", "run_part_minaret_binary_iou", "compute_binary_gt",
              "resize_mask_to_voxel_grid", "load_camera_json", "project_keypoints"):
        assert n in names and callable(getattr(pb3d.eval_helpers_intra, n))
    assert "load_mask" not in names          # utils.mask_utils.load_mask has another signature


def _cabi():
    import pb3d
    return pb3d._lib.load(), pb3d._lib


def _err(lib):
    return lib.pb3d_last_error().decode()


def test_cabi_refuses_bad_arguments():
    """argument errors come before any device work (and before the context is looked at): no GPU needed"""
    lib, L = _cabi()
    R = np.eye(3).ravel(); cp = np.zeros(3); prec = (C.c_int * 4)(0, 0, 0, 0)
    cols = np.ones(32 * 3, np.uint8)
    fake = C.c_void_p(16)
    args = (L.p_dbl(R), L.p_dbl(cp), 1.0, 0.0, 0.0, prec)
    assert lib.pb3d_grid_depth_buffer_dev(None, fake, 4, 4, 4, 2, *args, 4, 4, fake) == -1 and "C must be" in _err(lib)
    assert lib.pb3d_grid_visible_bits_dev(None, fake, 4, 4, 4, 3, L.p_u8(cols), 32, *args, fake, 4, 4, 4, 4, 1e-3, 1, fake) == -1
    assert "at most 31 colours" in _err(lib)
    assert lib.pb3d_grid_visible_bits_dev(None, fake, 4, 4, 4, 4, L.p_u8(cols), 2, *args, fake, 4, 4, 4, 4, 1e-3, 1, fake) == -1
    assert "C must be" in _err(lib)
    assert lib.pb3d_grid_visible_bits_dev(None, fake, 4, 4, 4, 3, L.p_u8(cols), 2, *args, fake, 5, 4, 4, 4, 1e-3, 1, fake) == -1
    assert "zbuf is 5x4" in _err(lib)
    z = np.zeros(6, np.uint8)
    assert lib.pb3d_grid_visible_bits_dev(None, fake, 4, 4, 4, 3, L.p_u8(z), 2, *args, fake, 4, 4, 4, 4, 1e-3, 1, fake) == -1
    assert "black" in _err(lib)
    assert lib.pb3d_grid_visible_bits_dev(None, fake, 4, 4, 4, 3, L.p_u8(cols), 2, *args, fake, 4, 4, 4, 4, 1e-3, 1, fake) == -1
    assert "null context" in _err(lib)
    big = (64, 1 << 20, 1 << 22)        # 2^40 walk items: more than 2^31 blocks of 256, refused by the shape alone
    assert lib.pb3d_grid_depth_buffer_dev(None, fake, *big, 3, *args, 4, 4, fake) == -1 and "too large" in _err(lib)
    assert lib.pb3d_grid_visible_bits_dev(None, fake, *big, 3, L.p_u8(cols), 2, *args, fake, 4, 4, 4, 4, 1e-3, 1, fake) == -1
    assert "too large" in _err(lib)
    ptrs = (C.c_void_p * 32)(*([16] * 32)); counts = np.ones(32, np.int64)
    assert lib.pb3d_points_visible_bits_dev(None, ptrs, counts.ctypes.data_as(L.i64p), 32, 2, *args, fake, 4, 4, 4, 4, 1e-3, 0, fake) == -1
    assert "at most 31 point lists" in _err(lib)
    assert lib.pb3d_points_visible_bits_dev(None, ptrs, counts.ctypes.data_as(L.i64p), 2, 3, *args, fake, 4, 4, 4, 4, 1e-3, 0, fake) == -1
    assert lib.pb3d_points_visible_bits_dev(None, ptrs, counts.ctypes.data_as(L.i64p), 2, 2, *args, fake, 4, 3, 4, 4, 1e-3, 0, fake) == -1
    assert "zbuf is 4x3" in _err(lib)
    assert lib.pb3d_color_presence_dev(None, fake, 64, 2, fake, None, 0, None) == -1 and "C must be" in _err(lib)
    assert lib.pb3d_color_presence_dev(None, fake, 64, 3, fake, L.p_u8(cols), 32, fake) == -1 and "at most 31" in _err(lib)
    assert lib.pb3d_mask_bits_dev(None, fake, 16, L.p_u8(cols), 32, None, fake) == -1 and "at most 31" in _err(lib)
    rows = (L.IouRow * 33)()
    assert lib.pb3d_iou_rows_dev(None, C.cast(rows, C.c_void_p), 33, 16, fake) == -1 and "at most 32 rows" in _err(lib)


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------
def _layout(tmp_path):
    """the reference's results/ and data/ layout, linked to the fixtures"""
    dirs = {k: tmp_path / k for k in ("vox", "def", "cam", "masks")}
    for d in dirs.values():
        d.mkdir()
    for mon in MONUMENTS:
        os.symlink(os.path.join(GOLDEN, f"stored_{mon}_voxel_grid.npz"), dirs["vox"] / f"{mon}_voxel_grid.npz")
        os.symlink(os.path.join(GOLDEN, f"stored_{mon}_deformed_voxel_grid.npz"), dirs["def"] / f"{mon}_deformed_voxel_grid.npz")
        for tag in ("init", "kp", "final"):
            os.symlink(os.path.join(GOLDEN, f"stored_{mon}_camera_params_{tag}.json"), dirs["cam"] / f"{mon}_camera_params_{tag}.json")
        (dirs["masks"] / mon / "masks").mkdir(parents=True)
        os.symlink(os.path.join(GOLDEN, f"data_{mon}_front_mask.png"), dirs["masks"] / mon / "masks" / f"{mon}_front_mask.png")
    return dirs


def _table_of(out):
    return "\n".join(l for l in out.splitlines() if l.startswith("+") or l.startswith("|"))


@pytest.mark.gpu
@pytest.mark.parametrize("table", ["minaret_kp", "minaret_iou", "part_minaret_binary"])
def test_notebook4_tables(pb3d_gpu, tmp_path, capsys, table):
    ev = pb3d_gpu.eval_helpers_intra
    d = _layout(tmp_path)
    PC = pb3d_gpu.PART_COLORS
    if table == "minaret_kp":
        df = ev.run_minaret_kp_evaluation(MONUMENTS, "front", d["vox"], d["masks"], d["cam"], PC, visualize=False)
    elif table == "minaret_iou":
        df = ev.run_minaret_iou_evaluation(MONUMENTS, "front", d["vox"], d["masks"], d["cam"], PC, visualize=False)
    else:
        df = ev.run_part_minaret_binary_iou(MONUMENTS, "front", d["vox"], d["def"], d["masks"], d["cam"], PC, visualize=False)
    out = capsys.readouterr().out
    want = _tables()[table]
    got = {r: {c: df.loc[r, c] for c in df.columns} for r in df.index}
    assert list(df.columns) == want["columns"]
    assert got == want["rows"]
    assert _table_of(out) == _table_of(_tables()["stdout"][table])


@pytest.mark.gpu
def test_cells_helpers_return_plain_dicts(pb3d_gpu, tmp_path):
    ev = pb3d_gpu.eval_helpers_intra
    d = _layout(tmp_path)
    cells = ev.part_minaret_binary_cells("Akbar", "front", d["vox"], d["def"], d["masks"], d["cam"], pb3d_gpu.PART_COLORS)
    assert type(cells) is dict and cells == _want("part_minaret_binary", "Akbar")


def _label_grid(g):
    """a C = 1 grid with the occupancy of the RGB grid g"""
    lab = ((g[..., 0].astype(np.int64) * 7 + g[..., 1] * 3 + g[..., 2]) % 250 + 1).astype(np.uint8)
    return np.where(np.any(g > 0, axis=-1), lab, 0).astype(np.uint8)


def _view_size(mon, view, grid_shape):
    return _resized_mask(mon, grid_shape, view).shape[:2]


@pytest.mark.gpu
@pytest.mark.parametrize("mon", ["Akbar", "Bibi", "Charminar", "Itimad", "Taj"])
def test_grid_depth_buffer_bit_identical(pb3d_gpu, mon):
    for deformed in (False, True):
        g = _grid(mon, deformed)
        lab = _label_grid(g)
        for view in ("front", "drone"):
            H, W = _view_size(mon, view, g.shape)
            cam = _cam(mon, "final", view)
            want = pb3d_gpu.compute_global_depth_buffer(g, cam, H, W)
            for grid in (g, lab):
                got = pb3d_gpu.grid_depth_buffer(grid, cam, H, W)
                assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (mon, deformed, view, grid.ndim)
    cam64 = {k: (v.astype(np.float64) if isinstance(v, np.ndarray) else v) for k, v in _cam(mon, "final").items()}
    g = _grid(mon)
    H, W = _view_size(mon, "front", g.shape)
    want = pb3d_gpu.compute_global_depth_buffer(g, cam64, H, W)
    assert np.array_equal(pb3d_gpu.grid_depth_buffer(g, cam64, H, W).view(np.uint32), want.view(np.uint32))


def _bits_want(pb3d, grid, colours, cam, zbuf, H, W):
    want = np.zeros((H, W), np.uint32)
    for k, c in enumerate(colours):
        pts, _ = pb3d.get_voxel_points_by_parts(grid, {"c": tuple(c)}, ["c"])
        want |= pb3d.project_part_visible(pts, cam, zbuf, H, W).astype(np.uint32) << k
    z, y, x = np.where(np.any(grid > 0, axis=-1))
    occ = np.stack([x, y, z], axis=1).astype(np.float32)
    want |= pb3d.project_part_visible(occ, cam, zbuf, H, W).astype(np.uint32) << 31
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("mon", ["Akbar", "Itimad", "Charminar"])
def test_grid_visible_bits_match_per_colour_masks(pb3d_gpu, mon):
    PC = pb3d_gpu.PART_COLORS
    colours = [PC[p] for p in PARTS] + [PC["front_minarets"], PC["back_minarets"]]
    gi, gd = _grid(mon), _grid(mon, True)
    for view in ("front", "drone"):
        cam = _cam(mon, "final", view)
        H, W = _view_size(mon, view, gi.shape)
        zi = pb3d_gpu.compute_global_depth_buffer(gi, cam, H, W)
        zd = pb3d_gpu.compute_global_depth_buffer(gd, cam, H, W)
        for grid, zb in ((gi, zi), (gd, zd), (gi, zd)):        # (gi, zd): the minarets row's init voxels against the deformed z-buffer
            got = pb3d_gpu.grid_visible_bits(grid, colours, cam, zb, H, W)
            assert np.array_equal(got, _bits_want(pb3d_gpu, grid, colours, cam, zb, H, W)), (mon, view)
    # labels: colour k of a C = 1 grid is a label value
    lab = _label_grid(gi)
    cam = _cam(mon, "final")
    H, W = _view_size(mon, "front", gi.shape)
    zb = pb3d_gpu.compute_global_depth_buffer(gi, cam, H, W)
    vals = [int(v) for v in np.unique(lab)[1:6]]
    got = pb3d_gpu.grid_visible_bits(lab, np.array(vals, np.uint8).reshape(-1, 1), cam, zb, H, W)
    want = np.zeros((H, W), np.uint32)
    for k, v in enumerate(vals):
        z, y, x = np.where(lab == v)
        want |= pb3d_gpu.project_part_visible(np.stack([x, y, z], 1).astype(np.float32), cam, zb, H, W).astype(np.uint32) << k
    z, y, x = np.where(lab > 0)
    want |= pb3d_gpu.project_part_visible(np.stack([x, y, z], 1).astype(np.float32), cam, zb, H, W).astype(np.uint32) << 31
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_points_visible_bits_int64_lists(pb3d_gpu):
    PC = pb3d_gpu.PART_COLORS
    g = _grid("Taj")
    vox = pb3d_gpu.extract_minaret_voxels_by_label(g, [PC["front_minarets"], PC["back_minarets"]])
    H, W = _view_size("Taj", "front", g.shape)
    for tag in ("init", "kp", "final"):
        cam = _cam("Taj", tag)
        zb = pb3d_gpu.compute_global_depth_buffer(g, cam, H, W)
        got = pb3d_gpu.points_visible_bits([vox[m] for m in MINARETS], cam, zb, H, W)
        want = np.zeros((H, W), np.uint32)
        for j, m in enumerate(MINARETS):
            want |= pb3d_gpu.project_part_visible(vox[m], cam, zb, H, W).astype(np.uint32) << j
        assert np.array_equal(got, want), tag


def _synthetic(shape, seed, ncolours=8, fill=0.3):
    rng = np.random.default_rng(seed)
    pal = rng.integers(1, 256, (ncolours, 3), dtype=np.uint8)
    g = pal[rng.integers(0, ncolours, shape)]
    g[rng.random(shape) > fill] = 0
    return g, pal


def _check_grid(pb3d, g, pal, cam, H, W):
    want = pb3d.compute_global_depth_buffer(g, cam, H, W)
    got = pb3d.grid_depth_buffer(g, cam, H, W)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    bits = pb3d.grid_visible_bits(g, pal, cam, want, H, W)
    assert np.array_equal(bits, _bits_want(pb3d, g, pal, cam, want, H, W))
    return want


@pytest.mark.gpu
def test_edge_cases(pb3d_gpu):
    # odd shape (unaligned rows: the byte-load path)
    g, pal = _synthetic((355, 512, 355), 1, fill=0.05)
    cam = {"cam_pos": np.array([177.0, 256.0, -600.0], np.float32), "target": np.array([177.0, 256.0, 177.0], np.float32),
           "f": 600.0, "cx": 256.0, "cy": 256.0}
    _check_grid(pb3d_gpu, g, pal, cam, 512, 512)
    # the camera inside the grid: voxels behind it (Z <= 1e-6) are dropped
    g, pal = _synthetic((64, 48, 40), 2)
    inside = {"cam_pos": np.array([20.0, 24.0, 32.0], np.float32), "target": np.array([20.0, 24.0, 90.0], np.float32),
              "f": 40.0, "cx": 50.0, "cy": 40.0}
    zb = _check_grid(pb3d_gpu, g, pal, inside, 80, 100)
    assert np.isfinite(zb).any() and np.isinf(zb).any()
    # looking along a2 (x): every a0 step of a column moves the pixel
    side = {"cam_pos": np.array([-200.0, 24.0, 32.0], np.float32), "target": np.array([20.0, 24.0, 32.0], np.float32),
            "f": 300.0, "cx": 60.0, "cy": 50.0}
    _check_grid(pb3d_gpu, g, pal, side, 100, 120)
    # an empty grid, and a zero-sized one
    e = np.zeros((16, 16, 16, 3), np.uint8)
    assert np.isinf(pb3d_gpu.grid_depth_buffer(e, cam, 8, 8)).all()
    assert not pb3d_gpu.grid_visible_bits(e, pal, cam, np.full((8, 8), np.inf, np.float32), 8, 8).any()
    assert np.isinf(pb3d_gpu.grid_depth_buffer(np.zeros((0, 4, 4, 3), np.uint8), cam, 8, 8)).all()
    assert len(pb3d_gpu.color_presence(e)) == 0
    with pytest.raises(ValueError, match="zbuf is 8x9"):
        pb3d_gpu.grid_visible_bits(g, pal, cam, np.zeros((8, 9), np.float32), 8, 8)
    with pytest.raises(ValueError, match="at most 31"):
        pb3d_gpu.grid_visible_bits(g, np.ones((32, 3), np.uint8), cam, np.zeros((8, 8), np.float32), 8, 8)


@pytest.mark.gpu
def test_color_presence_matches_unique(pb3d_gpu):
    rng = np.random.default_rng(7)
    pal = rng.integers(0, 256, (5000, 3), dtype=np.uint8)
    g = pal[rng.integers(0, len(pal), (61, 67, 71))]          # odd sizes: the byte-load tail
    g[rng.random(g.shape[:3]) < 0.5] = 0
    want = np.unique(g.reshape(-1, 3), axis=0)
    want = want[~np.all(want == 0, axis=1)]
    got = pb3d_gpu.color_presence(g)
    assert len(want) > 3000 and np.array_equal(got, want)
    g2 = np.ascontiguousarray(g[:, :, :64])                   # aligned rows: the dword path
    want2 = np.unique(g2.reshape(-1, 3), axis=0)
    assert np.array_equal(pb3d_gpu.color_presence(g2), want2[~np.all(want2 == 0, axis=1)])
    lab = rng.integers(0, 256, (40, 40, 40)).astype(np.uint8)
    assert np.array_equal(pb3d_gpu.color_presence(lab), np.unique(lab)[np.unique(lab) > 0])
    # compute_binary_gt against the reference's np.unique form
    mask = pal[rng.integers(0, len(pal), (50, 60))]
    gt = np.zeros(mask.shape[:2], bool)
    for c in want:
        gt |= np.all(mask == c, axis=-1)
    assert np.array_equal(pb3d_gpu.compute_binary_gt(mask, g), gt)
