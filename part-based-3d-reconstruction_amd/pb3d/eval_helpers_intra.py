"""Notebook 4 (intra-method analysis): reference utils/eval_helpers_intra.py.

Z-buffer visibility of a voxel grid under a pinhole camera (row N5): compute_global_depth_buffer (:134-163) and project_part_visible
(:168-190) on point lists, one atomicMin z-buffer kernel and one compare kernel (csrc/project.hip).

The three evaluations of notebook 4 (row N6): run_minaret_kp_evaluation (:287-424), run_minaret_iou_evaluation (:427-557) and
run_part_minaret_binary_iou (:560-748), with the loaders and small helpers they use (:19-84, :269-285).  Upstream makes a point list
per part, camera and grid (np.where over the grid) and walks it in a Python loop; here every z-buffer and visibility pass reads the
resident grid directly (csrc/visibility.hip), each pass writes one uint32 bit image (bit k = colour k, bit 31 = any occupied voxel),
and all IoU rows of a monument come back in one download of counts."""
import ctypes as C
import json
import os
import warnings

import numpy as np

from . import _lib, device as dev, mask_utils
from ._args import _cam, _colour_table, _eps_f32, _grid, _on_device
from ._lib import _ptr
from .projection_utils import camera_args

__all__ = ["compute_global_depth_buffer", "project_part_visible", "load_voxel_grid", "load_mask", "resize_mask_to_voxel_grid",
           "load_camera_json", "project_keypoints", "compute_binary_gt", "run_minaret_kp_evaluation", "run_minaret_iou_evaluation",
           "run_part_minaret_binary_iou", "grid_depth_buffer", "grid_visible_bits", "points_visible_bits", "color_presence",
           "minaret_kp_cells", "minaret_iou_cells", "part_minaret_binary_cells"]


def compute_global_depth_buffer(voxel_grid, cam, H, W):
    """(H,W) float32 depth of the nearest occupied voxel per pixel, +inf where none."""
    grid = _lib.as_u8(voxel_grid, "voxel_grid")
    if grid.ndim != 4:
        raise ValueError("voxel_grid must be (A0,A1,A2,3)")
    A0, A1, A2, Cc = grid.shape
    lib, ctx = _lib.load(), _lib.ctx()
    with dev.Scope() as sc:
        d_grid = sc.upload(grid) or sc.alloc(0)
        d_z = sc.alloc(int(H) * int(W) * 4)
        n = C.c_int64(0)
        _lib.check(lib.pb3d_points_count_dev(ctx, C.c_void_p(d_grid.ptr), A0, A1, A2, Cc, None, 0, 1, C.byref(n)))
        d_pts = sc.alloc(max(1, n.value) * 12); d_pc = sc.alloc(max(1, n.value) * Cc)
        _lib.check(lib.pb3d_points_fill_dev(ctx, C.c_void_p(d_grid.ptr), A0, A1, A2, Cc, None, 0, 1, n.value, C.c_void_p(d_pts.ptr),
                                            C.c_void_p(d_pc.ptr)))
        _, _, R, cp, prec = camera_args(np.zeros((1, 3), np.float32), cam["cam_pos"], cam["target"], cam["f"], cam["cx"], cam["cy"])
        _lib.check(lib.pb3d_depth_buffer_dev(ctx, C.c_void_p(d_pts.ptr), 0, n.value, _lib.p_dbl(R), _lib.p_dbl(cp), float(cam["f"]),
                                             float(cam["cx"]), float(cam["cy"]), prec, int(H), int(W), C.c_void_p(d_z.ptr)))
        return d_z.download((int(H), int(W)), np.float32)


def project_part_visible(pts3d, cam, zbuf, H, W, eps=1e-3):
    """(H,W) bool: pixels where some point of the part lies on the depth buffer (within eps)."""
    p, pf64, R, cp, prec = camera_args(pts3d, cam["cam_pos"], cam["target"], cam["f"], cam["cx"], cam["cy"])
    zb = np.ascontiguousarray(zbuf, np.float32)
    if zb.shape != (int(H), int(W)):
        raise IndexError("zbuf shape does not match (H, W)")
    with dev.Scope() as sc:
        d_p = sc.upload(p)
        d_zb = sc.upload(zb) or sc.alloc(0); d_m = sc.alloc(int(H) * int(W))
        _lib.check(_lib.load().pb3d_visible_mask_dev(_lib.ctx(), None if d_p is None else C.c_void_p(d_p.ptr), pf64, len(p), _lib.p_dbl(R),
                                                     _lib.p_dbl(cp), float(cam["f"]), float(cam["cx"]), float(cam["cy"]), prec,
                                                     C.c_void_p(d_zb.ptr), int(H), int(W), float(eps), _eps_f32(prec, eps), C.c_void_p(d_m.ptr)))
        return d_m.download((int(H), int(W))).astype(bool)


# ---- loaders and small helpers (reference :19-84, :269-285) -------------------------------------------------------------------------
MINARETS = ["LM1", "RM1", "LM2", "RM2"]
PARTS = ["dome", "chhatris", "main_door", "windows", "plinth"]
MONUMENT_SHORT = {"Taj": "TM", "Bibi": "BkM", "Itimad": "IuD", "Akbar": "AT", "Charminar": "CM"}
BACK_TOP_ONLY = {"Itimad": True, "Akbar": True, "Charminar": True, "Taj": False, "Bibi": False}
_ANY = 1 << 31


def load_voxel_grid(npz_path):
    with np.load(npz_path) as data:
        return data["voxel_grid"]


def load_mask(mask_path):
    """(H, W, 3) uint8 RGB of a mask file (not pb3d.load_mask, which is utils/mask_utils.py's)"""
    return mask_utils._read_rgb(mask_path)


def resize_mask_to_voxel_grid(mask_img, voxel_grid):
    """nearest resize so the mask's longer side is the grid's largest dimension; prints upstream's line.  voxel_grid: anything with
    the grid's .shape (a NumPy grid or a DeviceGrid)"""
    H, W = mask_img.shape[:2]
    scale = max(voxel_grid.shape[:3]) / max(H, W)
    new_W, new_H = int(round(W * scale)), int(round(H * scale))
    resized = mask_utils.resize_nearest(mask_img, new_W, new_H)
    print(f"Mask resized: ({H},{W}) → ({new_H},{new_W}) | scale={scale:.3f}")
    return resized


def load_camera_json(path, view):
    if not os.path.exists(path):
        raise FileNotFoundError(path)
    with open(path, "r") as f:
        data = json.load(f)
    if view not in data:
        raise KeyError(f"View '{view}' not found in {os.path.basename(path)}")
    cam = data[view]
    return {"cam_pos": np.array(cam["cam_pos"], dtype=np.float32), "target": np.array(cam["target"], dtype=np.float32),
            "f": float(cam["f"]), "cx": float(cam["cx"]), "cy": float(cam["cy"])}


def project_keypoints(voxel_kps, cam):
    from .camera_geometry import project
    return {k: project(pt, cam["cam_pos"], cam["target"], cam["f"], cam["cx"], cam["cy"]) for k, pt in voxel_kps.items()}


def _iou_bool(a, b):
    inter = np.logical_and(a, b).sum()
    union = np.logical_or(a, b).sum()
    return inter / union if union > 0 else np.nan


def _iou_counts(inter, union):
    """_iou_bool from counts (NumPy int64 division, nan for an empty union)"""
    return np.int64(inter) / np.int64(union) if union > 0 else np.nan


# ---- device passes ----------------------------------------------------------------------------------------------------------------
def depth_buffer_resident(d_grid, shape, cam, H, W, out=None):
    """pb3d_grid_depth_buffer_dev: the float32 (H, W) z-buffer of a resident grid in a DeviceBuffer"""
    A0, A1, A2, Cc = shape
    R, cp, prec = _cam(cam, np.float32)
    with dev.Scope() as sc:
        d_z = sc.result(out, max(1, int(H) * int(W)) * 4)
        _lib.check(_lib.load().pb3d_grid_depth_buffer_dev(_lib.ctx(), _ptr(d_grid), A0, A1, A2, Cc, _lib.p_dbl(R), _lib.p_dbl(cp), float(cam["f"]),
                                                          float(cam["cx"]), float(cam["cy"]), prec, int(H), int(W), C.c_void_p(d_z.ptr)))
        return d_z


def visible_bits_resident(d_grid, shape, colors, cam, d_zbuf, zshape, H, W, eps=1e-3, out=None):
    """pb3d_grid_visible_bits_dev into a (H, W) uint32 DeviceBuffer"""
    A0, A1, A2, Cc = shape
    R, cp, prec = _cam(cam, np.float32)
    tab = _colour_table(colors, Cc)
    with dev.Scope() as sc:
        d_b = sc.result(out, max(1, int(H) * int(W)) * 4)
        _lib.check(_lib.load().pb3d_grid_visible_bits_dev(_lib.ctx(), _ptr(d_grid), A0, A1, A2, Cc, _lib.p_u8(tab), len(tab), _lib.p_dbl(R),
                                                          _lib.p_dbl(cp), float(cam["f"]), float(cam["cx"]), float(cam["cy"]), prec,
                                                          C.c_void_p(d_zbuf.ptr), int(zshape[0]), int(zshape[1]), int(H), int(W), float(eps),
                                                          _eps_f32(prec, eps), C.c_void_p(d_b.ptr)))
        return d_b


def points_visible_bits_resident(lists, cam, d_zbuf, zshape, H, W, eps=1e-3, out=None):
    """pb3d_points_visible_bits_dev: bit k = some point of lists[k] ((n, 3) arrays of one dtype: float32, float64 or int64) is visible.
    The camera's precision follows NumPy's promotion of the points' dtype (int64 - float32 is float64)."""
    arrs = [np.asarray(a) for a in lists]
    dt = np.result_type(*arrs) if arrs else np.dtype(np.float32)
    kinds = {np.dtype(np.float32): 0, np.dtype(np.float64): 1, np.dtype(np.int64): 2}
    if dt not in kinds or any(a.dtype != dt for a in arrs):
        raise TypeError("point lists must all be float32, float64 or int64")
    for a in arrs:
        if a.ndim != 2 or a.shape[1] != 3:
            raise ValueError("point lists must be (n, 3)")
    R, cp, prec = _cam(cam, dt)
    counts = np.array([len(a) for a in arrs] or [0], np.int64)
    with dev.Scope() as sc:     # (the context's pool hands a freed block out again only behind this stream's work)
        bufs = [sc.upload(a) for a in arrs]
        ptrs = (C.c_void_p * max(1, len(arrs)))(*[None if b is None else b.ptr for b in bufs])
        d_b = sc.result(out, max(1, int(H) * int(W)) * 4)
        _lib.check(_lib.load().pb3d_points_visible_bits_dev(_lib.ctx(), ptrs, counts.ctypes.data_as(_lib.i64p), len(arrs), kinds[dt],
                                                            _lib.p_dbl(R), _lib.p_dbl(cp), float(cam["f"]), float(cam["cx"]), float(cam["cy"]),
                                                            prec, C.c_void_p(d_zbuf.ptr), int(zshape[0]), int(zshape[1]), int(H), int(W),
                                                            float(eps), _eps_f32(prec, eps), C.c_void_p(d_b.ptr)))
        return d_b


def presence_resident(d_grid, shape, colors, d_present=None, out=None):
    """pb3d_color_presence_dev: the 2^24-bit colour bitmap of a resident grid (a DeviceBuffer); d_present (8 bytes) gets the bits
    of the table's colours that occur"""
    A0, A1, A2, Cc = shape
    tab = _colour_table(colors, Cc)
    with dev.Scope() as sc:
        d_bm = sc.result(out, _lib.PRESENCE_BYTES)
        _lib.check(_lib.load().pb3d_color_presence_dev(_lib.ctx(), _ptr(d_grid), A0 * A1 * A2, Cc, C.c_void_p(d_bm.ptr), _lib.p_u8(tab), len(tab),
                                                       _ptr(d_present)))
        return d_bm


def mask_bits_resident(d_mask, npix, colors, d_bitmap=None, out=None):
    """pb3d_mask_bits_dev of a resident (H, W, 3) RGB mask"""
    tab = _colour_table(colors, 3)
    with dev.Scope() as sc:
        d_b = sc.result(out, max(1, int(npix)) * 4)
        _lib.check(_lib.load().pb3d_mask_bits_dev(_lib.ctx(), C.c_void_p(d_mask.ptr), int(npix), _lib.p_u8(tab), len(tab), _ptr(d_bitmap),
                                                  C.c_void_p(d_b.ptr)))
        return d_b


def iou_rows_resident(rows, npix, d_counts, byte_offset=0):
    """pb3d_iou_rows_dev: rows = [(pred buffer, pred bits, gt buffer, gt bits, gate buffer or None, gate bits)]; (inter, union) of row r
    land at d_counts int64 [2r, 2r + 1] from byte_offset on"""
    arr = (_lib.IouRow * max(1, len(rows)))()
    for r, (pb, pm, gb, gm, kb, km) in enumerate(rows):
        arr[r] = _lib.IouRow(None if pb is None else pb.ptr, None if gb is None else gb.ptr, None if kb is None else kb.ptr,
                             pm & 0xffffffff, gm & 0xffffffff, km & 0xffffffff)
    _lib.check(_lib.load().pb3d_iou_rows_dev(_lib.ctx(), C.cast(arr, C.c_void_p), len(rows), int(npix), C.c_void_p(d_counts.ptr + byte_offset)))


def grid_depth_buffer(voxel_grid, cam, H, W):
    """compute_global_depth_buffer read straight from the grid (NumPy (A0,A1,A2,3) / (A0,A1,A2) labels or DeviceGrid): (H, W) float32"""
    g, shape = _grid(voxel_grid)
    with dev.Scope() as sc:
        d_z = sc.adopt(depth_buffer_resident(_on_device(sc, g), shape, cam, H, W))
        return d_z.download((int(H), int(W)), np.float32)


def grid_visible_bits(voxel_grid, colors, cam, zbuf, H, W, eps=1e-3):
    """(H, W) uint32: bit k = project_part_visible of the voxels of colors[k] against zbuf (which may come from another grid), bit 31
    = of every occupied voxel"""
    zb = np.ascontiguousarray(zbuf, np.float32)
    g, shape = _grid(voxel_grid)
    with dev.Scope() as sc:
        d_g, d_zb = _on_device(sc, g), sc.upload(zb) or sc.alloc(0)
        d_b = sc.adopt(visible_bits_resident(d_g, shape, colors, cam, d_zb, zb.shape if zb.ndim == 2 else (-1, -1), H, W, eps))
        return d_b.download((int(H), int(W)), np.uint32)


def points_visible_bits(lists, cam, zbuf, H, W, eps=1e-3):
    """(H, W) uint32: bit k = project_part_visible(lists[k], cam, zbuf, H, W, eps)"""
    zb = np.ascontiguousarray(zbuf, np.float32)
    with dev.Scope() as sc:
        d_zb = sc.upload(zb) or sc.alloc(0)
        d_b = sc.adopt(points_visible_bits_resident(lists, cam, d_zb, zb.shape if zb.ndim == 2 else (-1, -1), H, W, eps))
        return d_b.download((int(H), int(W)), np.uint32)


def color_presence(voxel_grid):
    """the distinct non-zero values of a grid, as np.unique(axis=0) orders them ((n, 3) uint8 colours, or (n,) labels)"""
    g, shape = _grid(voxel_grid)
    with dev.Scope() as sc:
        d_bm = sc.adopt(presence_resident(_on_device(sc, g), shape, []))
        words = d_bm.download((_lib.PRESENCE_BYTES // 4,), np.uint32)
    keys = np.flatnonzero(np.unpackbits(words.view(np.uint8), bitorder="little"))
    if shape[3] == 1:
        return keys.astype(np.uint8)
    rgb = np.stack([keys & 0xff, (keys >> 8) & 0xff, keys >> 16], axis=1).astype(np.uint8)
    return rgb[np.lexsort(rgb.T[::-1])]


def compute_binary_gt(mask_img, voxel_grid):
    """mask pixels whose colour occurs (non-black) in the grid (reference :274-284): the grid's colour set is a device bitmap"""
    m = np.ascontiguousarray(np.asarray(mask_img)[:, :, :3], np.uint8)
    H, W = m.shape[:2]
    g, shape = _grid(voxel_grid)
    if shape[3] != 3:
        raise ValueError("compute_binary_gt takes an RGB grid")
    with dev.Scope() as sc:
        d_g, d_m = _on_device(sc, g), sc.upload(m)
        d_bm = sc.adopt(presence_resident(d_g, shape, []))
        if d_m is None:
            return np.zeros((H, W), bool)
        d_b = sc.adopt(mask_bits_resident(d_m, H * W, [], d_bm))
        return d_b.download((H, W), np.uint32) != 0


# ---- the three evaluations, per monument (plain dicts of table cells) -----------------------------------------------------------------
def _paths(root, *parts):
    return os.path.join(str(root), *parts)


def _load_mask_for(root_masks, monument, view, grid):
    return resize_mask_to_voxel_grid(load_mask(_paths(root_masks, monument, "masks", f"{monument}_{view}_mask.png")), grid)


def _resident_grid(path):
    from .formats import load_voxel_grid as load
    return load(path, on_device=True)


def _vis(name):
    ref = _REF.get("module")
    if ref is None:
        if not _REF.get("warned"):
            warnings.warn("visualize=True: the plots are the reference's own code; call pb3d.install() on an imported reference `utils` "
                          "package to have them (skipped)", stacklevel=3)
            _REF["warned"] = True
        return None
    return getattr(ref, name)


_REF = {}       # "module": the reference's utils.eval_helpers_intra once pb3d.install() has run


def minaret_kp_cells(monument, view, root_voxels, root_masks, cam_dir, part_colors, visualize=False):
    """{minaret or "Average": "init→kp" pixel error} of one monument (reference :340-393)"""
    from .minarets import (extract_minaret_masks_by_label, extract_minaret_voxels_by_label, extract_top_bottom_image_points,
                           extract_top_bottom_voxel_points)
    print(f"\n🏛️ {monument}")
    with dev.Scope() as sc:
        grid = sc.adopt(_resident_grid(_paths(root_voxels, f"{monument}_voxel_grid.npz")))
        mask_img = _load_mask_for(root_masks, monument, view, grid)
        cams = {tag: load_camera_json(_paths(cam_dir, f"{monument}_camera_params_{tag}.json"), view) for tag in ("init", "kp")}
        cams = {"init": cams["init"], "rep": cams["kp"]}
        colours = [part_colors["front_minarets"], part_colors["back_minarets"]]
        vox_parts = extract_minaret_voxels_by_label(grid, colours)
    msk_parts = extract_minaret_masks_by_label(mask_img, colours)
    voxel_kps = extract_top_bottom_voxel_points(vox_parts)
    image_kps = extract_top_bottom_image_points(msk_parts)
    err = {tag: {} for tag in cams}
    for tag, cam in cams.items():
        proj = project_keypoints(voxel_kps, cam)
        if visualize and _vis("visualize_minaret_kp") is not None:
            _vis("visualize_minaret_kp")(monument, tag, cam, mask_img, voxel_kps, image_kps, MINARETS, BACK_TOP_ONLY)
        for m in MINARETS:
            errs = [np.linalg.norm(np.array(image_kps[f"{m}_top"]) - np.array(proj[f"{m}_top"]))]
            if not (m in ["LM2", "RM2"] and BACK_TOP_ONLY[monument]):
                errs.append(np.linalg.norm(np.array(image_kps[f"{m}_bottom"]) - np.array(proj[f"{m}_bottom"])))
            err[tag][m] = np.mean(errs)
    cells = {m: f"{err['init'][m]:.2f}→{err['rep'][m]:.2f}" for m in MINARETS}
    cells["Average"] = f"{np.mean(list(err['init'].values())):.2f}→{np.mean(list(err['rep'].values())):.2f}"
    return cells


def minaret_iou_cells(monument, view, root_voxels, root_masks, cam_dir, part_colors, visualize=False):
    """{minaret or "Average": "init→kp→final" IoU} of one monument (reference :471-532).  Per camera: the init grid's z-buffer, the
    visible bits of the four int64 minaret sets, and four gated rows; the twelve rows come back in one download."""
    from .minarets import extract_minaret_masks_by_label, extract_minaret_voxels_by_label
    print(f"\n🏛️ {monument}")
    with dev.Scope() as sc:
        grid = sc.adopt(_resident_grid(_paths(root_voxels, f"{monument}_voxel_grid.npz")))
        mask_img = _load_mask_for(root_masks, monument, view, grid)
        H, W = mask_img.shape[:2]
        cams = {"init": load_camera_json(_paths(cam_dir, f"{monument}_camera_params_init.json"), view),
                "rep": load_camera_json(_paths(cam_dir, f"{monument}_camera_params_kp.json"), view),
                "final": load_camera_json(_paths(cam_dir, f"{monument}_camera_params_final.json"), view)}
        if visualize and _vis("visualize_minarets_all_3cams") is not None:
            _vis("visualize_minarets_all_3cams")(grid.numpy(), mask_img, cams, H, W, part_colors)
        colours = [part_colors["front_minarets"], part_colors["back_minarets"]]
        vox_parts = extract_minaret_voxels_by_label(grid, colours)
        msk_parts = extract_minaret_masks_by_label(mask_img, colours)
        gt = np.zeros((H, W), np.uint32)
        for j, m in enumerate(MINARETS):
            gt |= msk_parts[m].astype(bool).astype(np.uint32) << j
        d_gt = sc.upload(gt) or sc.alloc(0)
        shape = grid.shape + (() if len(grid.shape) == 4 else (1,))
        rows = []
        for cam in cams.values():
            d_z = sc.adopt(depth_buffer_resident(grid.buf, shape, cam, H, W))
            d_v = sc.adopt(points_visible_bits_resident([vox_parts[m] for m in MINARETS], cam, d_z, (H, W), H, W))
            rows += [(d_v, 1 << j, d_gt, 1 << j, d_v, 0xF) for j in range(len(MINARETS))]
        d_c = sc.alloc(len(rows) * 16)
        iou_rows_resident(rows, H * W, d_c)
        counts = d_c.download((len(rows), 2), np.int64)
    iou = {m: {} for m in MINARETS}
    for c, tag in enumerate(cams):
        for j, m in enumerate(MINARETS):
            iou[m][tag] = _iou_counts(*counts[4 * c + j])
    cells = {m: f"{iou[m]['init']:.3f}→{iou[m]['rep']:.3f}→{iou[m]['final']:.3f}" for m in MINARETS}
    cells["Average"] = (f"{np.mean([iou[m]['init'] for m in MINARETS]):.3f}→{np.mean([iou[m]['rep'] for m in MINARETS]):.3f}→"
                        f"{np.mean([iou[m]['final'] for m in MINARETS]):.3f}")
    return cells


def part_minaret_binary_cells(monument, view, root_voxels, deformed_voxels, root_masks, cam_dir, part_colors, visualize=False):
    """{part, "minarets", "whole": "init→deformed" IoU or "--"} of one monument under its final camera (reference :605-738): two grid
    z-buffers, three visible-bit passes (init and deformed grid against their own z-buffer, the init grid against the deformed one for the
    minarets row), the colour set of the init grid, one ground-truth bit image and one row pass; one download."""
    print(f"\n🏛️ {monument}")
    with dev.Scope() as sc:
        g_i = sc.adopt(_resident_grid(_paths(root_voxels, f"{monument}_voxel_grid.npz")))
        g_d = sc.adopt(_resident_grid(_paths(deformed_voxels, f"{monument}_deformed_voxel_grid.npz")))
        mask_img = _load_mask_for(root_masks, monument, view, g_i)
        H, W = mask_img.shape[:2]
        cam = load_camera_json(_paths(cam_dir, f"{monument}_camera_params_final.json"), view)
        counts, present, images = _part_rows(g_i, g_d, mask_img, cam, part_colors, want_images=visualize)
    cells, r = {}, 0
    for k, part in enumerate(PARTS):
        (i0n, i0u), (i1n, i1u), (_, gt_sum) = counts[r:r + 3]
        r += 3
        if gt_sum == 0 or not (present >> k) & 1:
            cells[part] = "--"
            continue
        i0, i1 = _iou_counts(i0n, i0u), _iou_counts(i1n, i1u)
        if images is not None and _vis("visualize_side_by_side") is not None:
            _vis("visualize_side_by_side")(*images(1 << k, 1 << k, 1 << k, False), part, i0, i1)
        cells[part] = f"{i0:.3f}→{i1:.3f}"
    for name, (pm, title) in (("minarets", (3 << 5, "minarets")), ("whole", (_ANY, "whole (binary)"))):
        (i0n, i0u), (i1n, i1u) = counts[r:r + 2]
        r += 2
        i0, i1 = _iou_counts(i0n, i0u), _iou_counts(i1n, i1u)
        if images is not None and _vis("visualize_side_by_side") is not None:
            _vis("visualize_side_by_side")(*images(pm, pm, pm, name == "minarets"), title, i0, i1)
        cells[name] = f"{i0:.3f}→{i1:.3f}"
    return cells


def _part_rows(g_i, g_d, mask_img, cam, part_colors, bufs=None, want_images=False):
    """the device half of part_minaret_binary_cells: counts (rows, 2) int64 and the init grid's part-presence bits.  `bufs` is not read:
    the buffers live in a scope of this call."""
    with dev.Scope() as sc:
        H, W = mask_img.shape[:2]
        colours = [part_colors[p] for p in PARTS] + [part_colors["front_minarets"], part_colors["back_minarets"]]
        sh_i = g_i.shape + (() if len(g_i.shape) == 4 else (1,))
        sh_d = g_d.shape + (() if len(g_d.shape) == 4 else (1,))
        d_m = sc.upload(mask_img[:, :, :3]) or sc.alloc(0)
        nrows = 3 * len(PARTS) + 4
        d_c = sc.alloc(nrows * 16 + 8)
        d_present = d_c.at(nrows * 16)
        d_bm = sc.adopt(presence_resident(g_i.buf, sh_i, colours, d_present))
        d_gt = sc.adopt(mask_bits_resident(d_m, H * W, colours, d_bm))
        z_i = sc.adopt(depth_buffer_resident(g_i.buf, sh_i, cam, H, W))
        z_d = sc.adopt(depth_buffer_resident(g_d.buf, sh_d, cam, H, W))
        v_ii = sc.adopt(visible_bits_resident(g_i.buf, sh_i, colours, cam, z_i, (H, W), H, W))
        v_dd = sc.adopt(visible_bits_resident(g_d.buf, sh_d, colours, cam, z_d, (H, W), H, W))
        v_id = sc.adopt(visible_bits_resident(g_i.buf, sh_i, colours[len(PARTS):], cam, z_d, (H, W), H, W))
        rows = []
        for k in range(len(PARTS)):
            rows += [(v_ii, 1 << k, d_gt, 1 << k, None, 0), (v_dd, 1 << k, d_gt, 1 << k, None, 0), (None, 0, d_gt, 1 << k, None, 0)]
        rows += [(v_ii, 3 << 5, d_gt, 3 << 5, None, 0), (v_id, 3, d_gt, 3 << 5, None, 0)]
        rows += [(v_ii, _ANY, d_gt, _ANY, None, 0), (v_dd, _ANY, d_gt, _ANY, None, 0)]
        iou_rows_resident(rows, H * W, d_c)
        raw = d_c.download((nrows * 2 + 1,), np.int64)
        images = None
        if want_images:
            host = {k: b.download((H, W), np.uint32) for k, b in (("gt", d_gt), ("ii", v_ii), ("dd", v_dd), ("id", v_id))}

            def images(gm, pm_i, pm_d, minarets):
                return (host["gt"] & gm) != 0, (host["ii"] & pm_i) != 0, (host["id" if minarets else "dd"] & (3 if minarets else pm_d)) != 0
        return raw[:-1].reshape(nrows, 2), int(raw[-1]), images


# ---- the notebook entry points -------------------------------------------------------------------------------------------------------
_KP_HEADER = """
=== Minaret Keypoint Reprojection Error (px) ===
Θinit → Θkp

Rules:
- LM1, RM1: top + bottom
- LM2, RM2:
    * Taj, Bibi: top + bottom
    * Akbar, Charminar, Itimad: top only
"""
_IOU_HEADER = """
=== Minaret IoU (INIT voxel grid)
Visualization: ALL minarets together
Table: per-minaret IoU (visible only)
Cameras: Θinit → Θkp → Θfinal
"""
_PART_HEADER = """
=== Part / Minaret / Binary IoU (init → deformed)
Camera: final (Θ*)
Visibility-aware

Binary row = true whole silhouette IoU
(not average of parts)
"""


def _table(per_monument, rows, monuments, header):
    import pandas as pd
    from tabulate import tabulate
    cells = {r: {m: per_monument[m][r] for m in monuments} for r in rows}
    df = pd.DataFrame.from_dict(cells, orient="index")
    df = df[[m for m in monuments]]
    df.columns = [MONUMENT_SHORT[m] for m in df.columns]
    print(header)
    print(tabulate(df, headers="keys", tablefmt="grid", showindex=True))
    return df


def run_minaret_kp_evaluation(monuments, view, root_voxels, root_masks, cam_dir, part_colors, visualize=True):
    """Minaret keypoint reprojection error, Θinit → Θkp (reference :287-424); prints the table and returns it as a DataFrame."""
    per = {m: minaret_kp_cells(m, view, root_voxels, root_masks, cam_dir, part_colors, visualize) for m in monuments}
    return _table(per, MINARETS + ["Average"], monuments, _KP_HEADER)


def run_minaret_iou_evaluation(monuments, view, root_voxels, root_masks, cam_dir, part_colors, visualize=True):
    """Per-minaret visible IoU, Θinit → Θkp → Θfinal on the init grid (reference :427-557)."""
    per = {m: minaret_iou_cells(m, view, root_voxels, root_masks, cam_dir, part_colors, visualize) for m in monuments}
    return _table(per, MINARETS + ["Average"], monuments, _IOU_HEADER)


def run_part_minaret_binary_iou(monuments, view, root_voxels, deformed_voxels, root_masks, cam_dir, part_colors, visualize=True):
    """Part / minarets / whole IoU, init → deformed grid under the final camera (reference :560-748)."""
    per = {m: part_minaret_binary_cells(m, view, root_voxels, deformed_voxels, root_masks, cam_dir, part_colors, visualize)
           for m in monuments}
    return _table(per, PARTS + ["minarets", "whole"], monuments, _PART_HEADER)
