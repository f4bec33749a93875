"""Camera estimation of notebooks 2 and 3; mirror of reference utils/camera_estimation.py: the per-part IoU (:770-787, the inner
metric of every re-projection loop), the aligner's objective and search loops (:597-725), the bbox camera init (:56-108), the
keypoint fit (:110-170) and the projection-IoU overlays (:346-477)."""
import ctypes as C

import numpy as np

from . import _lib, device as dev, eval_helpers_intra as ev, projection_utils
from ._args import _cam, _colour_table, _grid, _on_device
from ._lib import _ptr
from .minarets import (extract_minaret_kps_for_view, extract_minaret_masks_by_label, extract_minaret_voxels_by_label,  # noqa: F401
                       extract_top_bottom_image_points, extract_top_bottom_voxel_points)

__all__ = ["compute_partwise_iou", "CameraObjective", "projection_iou_by_part", "random_search", "coordinate_descent", "powell_search",
           "auto_compute_initial_params_matching_bbox", "bbox_init_from_bounds", "optimize_camera_with_keypoints", "projection_overlays",
           "visualize_voxel_projection_iou"]

_REF = {}       # install() leaves the reference's own `minimize` here (optimize_camera_with_keypoints)


def partwise_iou_counts(proj_mask, gt_mask, colors):
    a = _lib.as_u8(proj_mask, "proj_mask").reshape(-1, 3)
    b = _lib.as_u8(gt_mask, "gt_mask").reshape(-1, 3)
    if a.shape != b.shape:
        raise ValueError(f"operands could not be broadcast together with shapes {a.shape} {b.shape}")
    cols = np.asarray(colors, np.int64).reshape(-1, 3)
    inter = np.zeros(len(cols), np.int64)
    uni = np.zeros(len(cols), np.int64)
    ok = np.all((cols >= 0) & (cols <= 255), axis=1)
    c8 = np.ascontiguousarray(cols[ok].astype(np.uint8))
    if len(c8):
        i8 = np.zeros(len(c8), np.int64); u8 = np.zeros(len(c8), np.int64)
        for s in range(0, len(c8), 32):
            chunk = np.ascontiguousarray(c8[s:s + 32])
            _lib.check(_lib.load().pb3d_partwise_iou(_lib.ctx(), _lib.p_u8(a), _lib.p_u8(b), a.shape[0], _lib.p_u8(chunk),
                                                     len(chunk), i8[s:].ctypes.data_as(_lib.i64p), u8[s:].ctypes.data_as(_lib.i64p)))
        inter[ok] = i8; uni[ok] = u8
    return inter, uni


def compute_partwise_iou(proj_mask, gt_mask, part_colors):
    """({part: inter/union, or 0.0 when the union is empty}, mean over parts)."""
    names = list(part_colors.keys())
    inter, uni = partwise_iou_counts(proj_mask, gt_mask, [part_colors[n] for n in names])
    per_part = {}
    for name, i, u in zip(names, inter, uni):
        per_part[name] = (i / u) if u > 0 else 0.0
    return per_part, np.mean(list(per_part.values()))


class CameraObjective:
    """The objective of the camera aligner, reference utils/camera_estimation.py:597-603
    (`evaluate(p)` = minus the mean IoU of the selected parts between the projection and the part image),
    with the point cloud, its colours and the image RESIDENT in HBM: the random / coordinate / Powell loops
    (:606-725) re-project the same points hundreds of times and only the nine camera numbers change.

        obj = CameraObjective(voxel_pts, voxel_colors, seg_img, selected_labels)
        value = obj(p)                       # p: dict with cam_pos, target, f, cx, cy (H, W default to the image's)
        values = obj.evaluate_batch([p1, p2, ...])
    """

    def __init__(self, voxel_pts, voxel_colors, seg_img, selected_labels):
        from .projection_utils import points_f64
        self._dev = dev
        pts = np.asarray(voxel_pts)
        self._pf64 = int(points_f64(pts.dtype))
        self._pts_dtype = pts.dtype
        self._pts_host = np.ascontiguousarray(pts, np.float64 if self._pf64 else np.float32)
        if self._pts_host.ndim != 2 or self._pts_host.shape[1] != 3:
            raise ValueError("voxel_pts must be (N,3)")
        cols = np.ascontiguousarray(np.asarray(voxel_colors).astype(np.uint8, copy=False))
        if cols.shape != (len(self._pts_host), 3):
            raise ValueError("voxel_colors must be (N,3)")
        self.n = len(self._pts_host)
        seg = _lib.as_u8(seg_img, "seg_img")
        self.H, self.W = seg.shape[:2]
        self.names = list(selected_labels.keys())
        self._colors = np.ascontiguousarray(np.array([selected_labels[k] for k in self.names], np.uint8).reshape(-1, 3))
        if len(self._colors) > 32:
            raise ValueError("at most 32 parts")
        with dev.Scope() as sc:         # (all four or none: close() frees them)
            self._d_pts, self._d_cols = sc.upload(self._pts_host), sc.upload(cols)
            self._d_seg = sc.upload(seg) or sc.alloc(0)
            self._d_img = sc.alloc(self.H * self.W * 3)
            for b in (self._d_pts, self._d_cols, self._d_seg, self._d_img):
                sc.keep(b)

    def __call__(self, p):
        from .projection_utils import camera_args
        H, W = int(p.get("H", self.H)), int(p.get("W", self.W))
        if (H, W) != (self.H, self.W):
            raise ValueError("operands could not be broadcast together: projection and part image differ in size")
        # only dtypes matter for the promotion flags: a one-row stand-in avoids touching the resident points
        _, _, R, cam, prec = camera_args(np.zeros((1, 3), self._pts_dtype), p["cam_pos"], p["target"], p["f"], p["cx"], p["cy"])
        lib, ctx = _lib.load(), _lib.ctx()
        _lib.check(lib.pb3d_project_dev(ctx, None if not self.n else C.c_void_p(self._d_pts.ptr), self._pf64,
                                        None if not self.n else C.c_void_p(self._d_cols.ptr), self.n, _lib.p_dbl(R), _lib.p_dbl(cam),
                                        float(p["f"]), float(p["cx"]), float(p["cy"]), prec, H, W, C.c_void_p(self._d_img.ptr)))
        inter = np.zeros(len(self._colors), np.int64); uni = np.zeros(len(self._colors), np.int64)
        _lib.check(lib.pb3d_partwise_iou_dev(ctx, C.c_void_p(self._d_img.ptr), C.c_void_p(self._d_seg.ptr), H * W, _lib.p_u8(self._colors),
                                             len(self._colors), inter.ctypes.data_as(_lib.i64p), uni.ctypes.data_as(_lib.i64p)))
        per = [(i / u) if u > 0 else 0.0 for i, u in zip(inter, uni)]
        return -np.mean(per)

    # struct pb3d_camera of include/pb3d.h
    _CAM = np.dtype([("R", np.float64, 9), ("cam", np.float64, 3), ("f", np.float64), ("cx", np.float64), ("cy", np.float64),
                     ("prec", np.int32, 4)], align=True)

    def evaluate_batch(self, params):
        """[obj(p) for p in params] with ONE projection launch, one IoU launch and one counter download for the whole list
        (the random / coordinate stages of the aligner evaluate dozens of cameras around the current one).  Exactly the values
        of the one-at-a-time path: the same point kernel per camera, the same integer counts, the same float64 mean."""
        from .camera_geometry import look_at_rotation_batch
        params = list(params)
        K = len(params)
        if K == 0:
            return []
        for p in params:
            if (int(p.get("H", self.H)), int(p.get("W", self.W))) != (self.H, self.W):
                raise ValueError("operands could not be broadcast together: projection and part image differ in size")
        eyes = [np.asarray(p["cam_pos"]) for p in params]; tgts = [np.asarray(p["target"]) for p in params]
        dts = {a.dtype for a in eyes} | {a.dtype for a in tgts}
        cams = np.zeros(K, self._CAM)
        if len(dts) == 1 and all(a.shape == (3,) for a in eyes) and all(a.shape == (3,) for a in tgts):
            E = np.stack(eyes); T = np.stack(tgts)
            cams["R"] = look_at_rotation_batch(E, T).reshape(K, 9)
            cams["cam"] = E
            t0 = int(np.result_type(self._pts_dtype, E.dtype) == np.float64)     # R has the cameras' dtype (float32 `up` is the narrowest operand)
            t0s = [t0] * K
        else:                                                                    # mixed dtypes: the per-camera NumPy route decides everything
            from .projection_utils import camera_args
            t0s = []
            for k, p in enumerate(params):
                _, _, R, cam, prec = camera_args(np.zeros((1, 3), self._pts_dtype), p["cam_pos"], p["target"], p["f"], p["cx"], p["cy"])
                cams["R"][k] = R.reshape(9); cams["cam"][k] = cam; t0s.append(int(prec[0]))
        for k, p in enumerate(params):
            cams["prec"][k] = projection_utils._promotion_flags(t0s[k], p["f"], p["cx"], p["cy"])
            cams["f"][k] = float(p["f"]); cams["cx"][k] = float(p["cx"]); cams["cy"][k] = float(p["cy"])
        P = len(self._colors)
        inter = np.zeros((K, P), np.int64); uni = np.zeros((K, P), np.int64)
        _lib.check(_lib.load().pb3d_project_iou_batch_dev(
            _lib.ctx(), None if not self.n else C.c_void_p(self._d_pts.ptr), self._pf64, None if not self.n else C.c_void_p(self._d_cols.ptr),
            self.n, cams.ctypes.data_as(C.c_void_p), K, self.H, self.W, C.c_void_p(self._d_seg.ptr), _lib.p_u8(self._colors), P,
            inter.ctypes.data_as(_lib.i64p), uni.ctypes.data_as(_lib.i64p)))
        self.last_counts = (inter, uni)
        with np.errstate(divide="ignore", invalid="ignore"):
            per = np.where(uni > 0, inter / uni, 0.0)
        if 0 < P < 8:
            # fewer than 8 addends: NumPy's reduction is the plain left-to-right sum whichever axis order its iterator
            # picks, so the row-wise mean of the matrix has the bits of np.mean(list) per camera
            return list(-(per.mean(axis=1)))
        return [-np.mean(row) for row in per] if P else [-np.mean([]) for _ in range(K)]

    def projection(self):
        """the image of the last evaluation (H,W,3)"""
        return self._d_img.download((self.H, self.W, 3))

    def close(self):
        for b in (self._d_pts, self._d_cols, self._d_seg, self._d_img):
            if b is not None:
                b.free()


def projection_iou_by_part(voxel_grid, part_colors, image, cam_params):
    """The numbers behind visualize_voxel_projection_iou (reference utils/camera_estimation.py:381-403, :437-452): for every
    part its points are extracted, projected with the camera and compared with the part's pixels of `image`; the
    combined binary IoU compares the union of the projections with every non-background pixel.
    Returns ({part: IoU}, combined_binary_IoU).  The grid is uploaded once and all parts are processed on the device."""
    from .projection_utils import camera_args
    grid = _lib.as_u8(voxel_grid, "voxel_grid")
    img = _lib.as_u8(image, "image")
    H, W = img.shape[:2]
    A0, A1, A2 = grid.shape[:3]
    lib, ctx = _lib.load(), _lib.ctx()
    per = {}
    union_prj = np.zeros((H, W), bool)
    with dev.Scope() as sc:
        d_grid = sc.upload(grid) or sc.alloc(0); d_img = sc.upload(img) or sc.alloc(0); d_proj = sc.alloc(H * W * 3)
        _, _, R, cam, prec = camera_args(np.zeros((1, 3), np.float32), cam_params["cam_pos"], cam_params["target"], cam_params["f"],
                                         cam_params["cx"], cam_params["cy"])
        for part, color in part_colors.items():
            c = np.asarray(color).reshape(-1)
            if c.size != 3 or np.any(c < 0) or np.any(c > 255):
                continue
            c8 = np.ascontiguousarray(c.astype(np.uint8))
            n = C.c_int64(0)
            _lib.check(lib.pb3d_points_count_dev(ctx, C.c_void_p(d_grid.ptr), A0, A1, A2, 3, _lib.p_u8(c8), 1, 1, C.byref(n)))
            if n.value == 0:
                continue
            with dev.Scope() as part_sc:
                d_pts = part_sc.alloc(n.value * 12); d_pc = part_sc.alloc(n.value * 3)
                _lib.check(lib.pb3d_points_fill_dev(ctx, C.c_void_p(d_grid.ptr), A0, A1, A2, 3, _lib.p_u8(c8), 1, 1, n.value,
                                                    C.c_void_p(d_pts.ptr), C.c_void_p(d_pc.ptr)))
                _lib.check(lib.pb3d_project_dev(ctx, C.c_void_p(d_pts.ptr), 0, C.c_void_p(d_pc.ptr), n.value, _lib.p_dbl(R), _lib.p_dbl(cam),
                                                float(cam_params["f"]), float(cam_params["cx"]), float(cam_params["cy"]), prec, H, W,
                                                C.c_void_p(d_proj.ptr)))
                inter = np.zeros(1, np.int64); uni = np.zeros(1, np.int64)
                _lib.check(lib.pb3d_partwise_iou_dev(ctx, C.c_void_p(d_proj.ptr), C.c_void_p(d_img.ptr), H * W, _lib.p_u8(c8), 1,
                                                     inter.ctypes.data_as(_lib.i64p), uni.ctypes.data_as(_lib.i64p)))
                per[part] = (inter[0] / uni[0]) if uni[0] > 0 else 0.0
                union_prj |= np.all(d_proj.download((H, W, 3)) == c8, axis=-1)
        bg = np.array(part_colors.get("background", (0, 0, 0)), dtype=np.uint8)
        gt = np.any(img != bg, axis=-1)
        u = np.logical_or(gt, union_prj).sum()
        return per, ((np.logical_and(gt, union_prj).sum() / u) if u > 0 else 0.0)


# =====================================================================================================
# N4: the search loops of launch_smart_aligner as drivers over CameraObjective.evaluate_batch
# (reference utils/camera_estimation.py:606-650 random, :652-686 coordinate descent, :688-726 Powell).
# A parameter set is the dict get_params() builds there (:528-542): cam_pos / target float64 arrays, f / cx / cy floats.
# =====================================================================================================
_KEYS = ("cam_x", "cam_y", "cam_z", "target_x", "target_y", "target_z", "f", "cx", "cy")        # the slider order (:505-518)


def _snap(p):
    q = dict(p)
    q["cam_pos"] = np.array(p["cam_pos"], copy=True); q["target"] = np.array(p["target"], copy=True)
    return q


def random_search(objective, base, steps, rng=None, lock_xy_equal=False):
    """Random Search button (:606-650): `steps` trials around `base` (never around the best so far), uniform in +-(50, 50, 100) for the
    camera and the target, +-50 for f, +-20 for cx / cy, drawn from `rng` (default: the global np.random, as upstream) in upstream's
    order; the best of base and trials by strict `>`.  ALL trials are ONE projection + IoU launch.  Returns (best_params, best_iou)."""
    rng = np.random if rng is None else rng
    step_cam = np.array([50, 50, 100]); step_tgt = np.array([50, 50, 100])
    trials = []
    for _ in range(int(steps)):
        t = dict(base)
        t["cam_pos"] = base["cam_pos"] + rng.uniform(-1, 1, 3) * step_cam
        t["target"] = base["target"] + rng.uniform(-1, 1, 3) * step_tgt
        t["f"] = base["f"] + rng.uniform(-1, 1) * 50
        t["cx"] = base["cx"] + rng.uniform(-1, 1) * 20
        t["cy"] = base["cy"] + rng.uniform(-1, 1) * 20
        if lock_xy_equal:
            t["cam_pos"][:2] = t["target"][:2]
        trials.append(t)
    vals = objective.evaluate_batch([base] + trials)
    best_iou, best_p = -vals[0], dict(base)
    for t, v in zip(trials, vals[1:]):
        if -v > best_iou:
            best_iou, best_p = -v, dict(t)
    return best_p, best_iou


def coordinate_descent(objective, base, rounds, lock_xy_equal=False):
    """Coordinate Descent button (:652-686): per round the +-20 trials of the nine parameters in slider order, the FIRST improvement
    (strict `>`) becomes the new best and ends the round.  Upstream's trial dicts are shallow copies, so the camera / target ARRAYS
    are shared between the best set and every trial and are stepped in place: the -20 trial of an array entry really moves it, the
    +20 trial moves it back (to fl(fl(x - 20) + 20): the value upstream continues with), and only f / cx / cy are ever tried at
    +20.  That sequence does not depend on the IoUs until an improvement ends it, so a round's trials are laid out first and
    evaluated in ONE launch.  Returns (best_params, best_iou)."""
    best_p = _snap(base)
    best_iou = -objective.evaluate_batch([best_p])[0]
    for _ in range(int(rounds)):
        cam = best_p["cam_pos"].copy(); tgt = best_p["target"].copy()          # the shared arrays as the round steps them
        trials = []
        for k in _KEYS:
            for delta in (-20, 20):
                t = dict(best_p)
                if k.startswith("cam_") and not lock_xy_equal:
                    cam["xyz".index(k[-1])] += delta
                elif k.startswith("target_"):
                    tgt["xyz".index(k[-1])] += delta
                    if lock_xy_equal and k in ("target_x", "target_y"):
                        cam["xyz".index(k[-1])] += delta
                elif k in ("f", "cx", "cy"):
                    t[k] = best_p[k] + delta
                else:
                    continue
                t["cam_pos"] = cam.copy(); t["target"] = tgt.copy()
                trials.append(t)
        vals = objective.evaluate_batch(trials)
        for t, v in zip(trials, vals):
            if -v > best_iou:
                best_iou, best_p = -v, t
                break
        else:
            # no improvement: the arrays keep whatever the in-place steps left in them (the scalars are untouched)
            best_p = dict(best_p); best_p["cam_pos"] = cam; best_p["target"] = tgt
    return best_p, best_iou


def powell_search(objective, base, maxiter, minimize, lock_xy_equal=False):
    """Powell button (:688-726) with the caller's minimiser (upstream: `minimize(obj, x0, method='Powell', options=...)`): the
    objective is CameraObjective.__call__ on from_vector(x) (:586-595).  Sequential by nature -- one camera per evaluation.
    Returns (params, iou)."""
    base = _snap(base)
    if lock_xy_equal:
        x0 = np.array([base["cam_pos"][2], base["target"][2], base["f"], base["cx"], base["cy"]])
        tx, ty = base["target"][0], base["target"][1]
        from_vec = lambda x: {"cam_pos": np.array([tx, ty, x[0]]), "target": np.array([tx, ty, x[1]]), "f": x[2], "cx": x[3], "cy": x[4]}
    else:
        x0 = np.concatenate([base["cam_pos"], base["target"], [base["f"], base["cx"], base["cy"]]])
        from_vec = lambda x: {"cam_pos": x[:3], "target": x[3:6], "f": x[6], "cx": x[7], "cy": x[8]}
    res = minimize(lambda x: objective(from_vec(x)), x0, method="Powell",
                   options={"maxiter": int(maxiter), "maxfev": int(maxiter) * 10, "xtol": 1e-3, "ftol": 1e-3, "disp": False})
    p = from_vec(res.x)
    return p, -objective(p)


# =====================================================================================================
# Notebook 2: the bbox camera init (:56-108), the keypoint fit (:110-170) and the overlays (:346-477)
# =====================================================================================================
def grid_bounds(voxel_grid, colors=None):
    """(count, lo, hi): the number of voxels whose colour (RGB grid) or label ((A0,A1,A2) grid) is in `colors` (None or empty: any
    non-zero voxel; at most 31, none of them zero) and their inclusive int64 bounds (a0, a1, a2) -- np.where(mask) reduced on the
    device in one read of the grid (pb3d_grid_bounds_resident).  count 0: lo and hi are None."""
    g, shape = _grid(voxel_grid)
    A0, A1, A2, Cc = shape
    with dev.Scope() as sc:
        d_g = _on_device(sc, g)
        tab = _colour_table(colors if colors is not None else [], Cc)
        d_o = sc.alloc(7 * 8)
        _lib.check(_lib.load().pb3d_grid_bounds_resident(_lib.ctx(), _ptr(d_g), A0, A1, A2, Cc, _lib.p_u8(tab), len(tab), C.c_void_p(d_o.ptr)))
        out = d_o.download((7,), np.int64)
    if out[0] == 0:
        return 0, None, None
    return int(out[0]), out[1:4].copy(), out[4:7].copy()


def hit_bits_resident(d_grid, shape, colors, cam_params, H, W, out=None):
    """pb3d_grid_hit_bits_resident into a (H, W) uint32 image: `out` (a DeviceBuffer or a ctypes pointer into one) or a new DeviceBuffer"""
    A0, A1, A2, Cc = shape
    R, cp, prec = _cam(cam_params, np.float32)
    tab = _colour_table(colors, Cc)
    with dev.Scope() as sc:
        d_b = sc.result(out, max(1, int(H) * int(W)) * 4)
        _lib.check(_lib.load().pb3d_grid_hit_bits_resident(_lib.ctx(), _ptr(d_grid), A0, A1, A2, Cc, _lib.p_u8(tab), len(tab), _lib.p_dbl(R),
                                                           _lib.p_dbl(cp), float(cam_params["f"]), float(cam_params["cx"]), float(cam_params["cy"]),
                                                           prec, int(H), int(W), _ptr(d_b)))
        return d_b


def grid_hit_bits(voxel_grid, colors, cam_params, H, W):
    """(H, W) uint32: bit k = some voxel of colors[k] (at most 31) projects onto the pixel, i.e.
    np.all(project_colored_voxels(*get_voxel_points_by_parts(grid, .., [part k]), ...) == colors[k], axis=-1) for every k in one sweep"""
    g, shape = _grid(voxel_grid)
    with dev.Scope() as sc:
        d_b = sc.adopt(hit_bits_resident(_on_device(sc, g), shape, colors, cam_params, H, W))
        return d_b.download((int(H), int(W)), np.uint32)


def bbox_init_from_bounds(lo, hi, img_bbox_min, img_bbox_max, H_img, W_img, fov_deg=30):
    """The scalar half of auto_compute_initial_params_matching_bbox (:64-108), host only: `lo` / `hi` are the inclusive voxel bounds
    (a0, a1, a2) of the chosen parts, img_bbox_min / img_bbox_max the (x, y) integer bounds of the image mask.  Upstream's NumPy
    expressions and dtypes: the bounds become the float32 (x, y, z) = (a2, a1, a0) rows that voxel_pts.min / max(axis=0) give.
    `lo` None (the parts have no voxel): the ValueError that voxel_pts.min(axis=0) raises upstream."""
    if lo is None:
        np.empty((0, 3), np.float32).min(axis=0)
    bbox_min = np.array([lo[2], lo[1], lo[0]]).astype(np.float32)
    bbox_max = np.array([hi[2], hi[1], hi[0]]).astype(np.float32)
    voxel_center = (bbox_min + bbox_max) / 2
    voxel_size = np.linalg.norm(bbox_max - bbox_min)
    img_bbox_width = np.linalg.norm(np.asarray(img_bbox_max) - np.asarray(img_bbox_min))
    cam_pos = voxel_center + np.array([0, 0, -voxel_size * 2.0])
    target = voxel_center
    f = H_img / (2 * np.tan(np.deg2rad(fov_deg) / 2))
    approx_voxel_proj_width = (voxel_size * f) / (voxel_size * 2.0)
    scale_factor = img_bbox_width / approx_voxel_proj_width
    f_adjusted = f * scale_factor
    init_params = {"cam_pos": cam_pos, "target": target, "f": f_adjusted, "cx": W_img / 2, "cy": H_img / 2}
    print(f"Estimated scale factor: {scale_factor:.4f}")
    print(f"Adjusted focal length: {f_adjusted:.2f}")
    return init_params


def auto_compute_initial_params_matching_bbox(voxel_grid, image, part_colors, parts_for_alignment, fov_deg=30):
    """Initial camera whose projection roughly matches the bounding box of the image mask (:56-108).  The voxel bounding box comes from
    one device read of the grid (grid_bounds; NumPy grid or DeviceGrid) instead of a point list; the image bbox and the scalars are
    upstream's NumPy expressions on the host.  No voxel of the parts, or no pixel: the ValueError of NumPy's min of an empty array."""
    from .mask_utils import mask_parts_from_image
    image = np.asarray(image)
    H_img, W_img = image.shape[:2]
    cols = []
    for p in parts_for_alignment:
        c = np.asarray(part_colors[p]).reshape(-1)
        if c.size != 3:
            raise ValueError("a part colour is (R, G, B)")
        if np.all((c >= 0) & (c <= 255)) and np.all(c == np.floor(c)):       # any other value never equals a uint8 voxel
            cols.append(tuple(int(v) for v in c))
    cols = list(dict.fromkeys(cols))
    if (0, 0, 0) in cols or len(cols) > 31:
        # black selects the empty voxels and is no colour bit: the point path
        from .voxel_utils import get_voxel_points_by_parts
        grid = voxel_grid.numpy() if hasattr(voxel_grid, "numpy") else voxel_grid
        pts = np.concatenate([get_voxel_points_by_parts(grid, {"p": c}, ["p"])[0] for c in cols])
        lo = pts.min(axis=0)[::-1]; hi = pts.max(axis=0)[::-1]
    else:
        n, lo, hi = grid_bounds(voxel_grid, cols) if cols else (0, None, None)
        if n == 0:                                          # upstream fails on the voxels before it looks at the image
            return bbox_init_from_bounds(None, None, None, None, H_img, W_img, fov_deg)
    seg_img = mask_parts_from_image(image, part_colors, parts_for_alignment)
    mask = np.any(seg_img > 0, axis=-1)
    ys, xs = np.where(mask)
    img_bbox_min = np.array([xs.min(), ys.min()])
    img_bbox_max = np.array([xs.max(), ys.max()])
    return bbox_init_from_bounds(lo, hi, img_bbox_min, img_bbox_max, H_img, W_img, fov_deg)


def optimize_camera_with_keypoints(voxel_keypoints_dict, image_keypoints_dict, image, init_params, loss_type='L2', minimize=None):
    """Fit camera position, target and intrinsics to the keypoints (:110-170); host only.  Upstream's loss term for term over
    pb3d.camera_geometry.project, the same x0 order, bounds, method='L-BFGS-B' and prints.

    `minimize` is the minimiser upstream imports from its optimisation library.  The package itself imports none (as powell_search,
    it takes the caller's): after pb3d.install() the reference's own `minimize` is used; otherwise pass it."""
    from .camera_geometry import project
    if minimize is None:
        minimize = _REF.get("minimize")
    if minimize is None:
        raise TypeError("optimize_camera_with_keypoints needs the L-BFGS-B minimiser: pass minimize=<optimize module>.minimize "
                        "(pb3d.install() takes it from the reference package)")
    H, W = image.shape[:2]
    keys = list(image_keypoints_dict.keys())

    def loss_fn(x):
        cam_x, cam_y, cam_z, target_x, target_y, target_z, f, cx, cy = x
        cam_pos = np.array([cam_x, cam_y, cam_z])
        target = np.array([target_x, target_y, target_z])
        total = 0
        for k in keys:
            proj_pt = project(voxel_keypoints_dict[k], cam_pos, target, f, cx, cy)
            gt_pt = image_keypoints_dict[k]
            error = np.abs(proj_pt - gt_pt) if loss_type == 'L1' else (proj_pt - gt_pt) ** 2
            total += error.sum()
        return total

    x0 = [*init_params['cam_pos'], *init_params['target'], init_params['f'], init_params['cx'], init_params['cy']]
    bounds = [(-W, 2 * W), (-H, 2 * H), (-2000, 100),       # cam_x, cam_y, cam_z
              (-W, 2 * W), (-H, 2 * H), (-2000, 100),       # target_x, target_y, target_z
              (10, 2000),                                   # f
              (0, W), (0, H)]                               # cx, cy
    result = minimize(loss_fn, x0, bounds=bounds, method='L-BFGS-B')
    cam_x, cam_y, cam_z, target_x, target_y, target_z, f, cx, cy = result.x
    final_params = {"cam_pos": np.array([cam_x, cam_y, cam_z]), "target": np.array([target_x, target_y, target_z]), "f": f, "cx": cx,
                    "cy": cy}
    print("\n📷 Optimized Camera Parameters:")
    for k, v in final_params.items():
        print(f"{k}: {v}")
    print(f"📉 Final Reprojection Loss: {result.fun:.2f}")
    return final_params


OVERLAY_MODES = {"part_on_whole": 0, "whole_on_whole": 1, "whole_on_whole_color": 2}      # PB3D_OVERLAY_* of include/pb3d.h
_SWEEP = 31                                                                               # colour bits of one grid sweep


def _iou(inter, union):
    return (inter / union) if union > 0 else 0.0


def _outline_host(vis, gt, prj):
    """outline_projection (:363-367) for a part that took the point path: the 4-neighbour cross, outside the image false"""
    m = gt & prj
    d = m.copy()
    d[1:] |= m[:-1]; d[:-1] |= m[1:]; d[:, 1:] |= m[:, :-1]; d[:, :-1] |= m[:, 1:]
    vis[d & ~m] = [255, 255, 0]
    return vis


def _overlays(voxel_grid, part_colors, image, cam_params, mode):
    """[(part or None, title, vis, iou)] of projection_overlays"""
    g, shape = _grid(voxel_grid)
    with dev.Scope() as sc:
        d_g = _on_device(sc, g)
        if shape[3] != 3:
            raise ValueError("voxel_grid must be (A0,A1,A2,3) RGB")
        img = _lib.as_u8(image, "image")
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError("image must be (H,W,3)")
        H, W = img.shape[:2]
        npix = H * W
        # which parts can be a colour bit, and which of those have voxels (:382-385 skips the others)
        cand, black = [], []
        for part, color in part_colors.items():
            c = np.asarray(color).reshape(-1)
            if c.size != 3:
                raise ValueError("a part colour is (R, G, B)")
            if not (np.all((c >= 0) & (c <= 255)) and np.all(c == np.floor(c))):
                continue                                    # never equals a uint8 voxel: no points upstream
            (cand if np.any(c != 0) else black).append((part, np.ascontiguousarray(c.astype(np.uint8))))
        live = []
        d_present = sc.alloc(8)
        d_bm = sc.alloc(_lib.PRESENCE_BYTES)
        for s in range(0, len(cand), _SWEEP):
            chunk = cand[s:s + _SWEEP]
            ev.presence_resident(d_g, shape, [c for _, c in chunk], d_present, out=d_bm)
            present = int(d_present.download((1,), np.int64)[0])
            live += [pc for k, pc in enumerate(chunk) if (present >> k) & 1]
        # black parts select the empty voxels: the point path (its own projection; the mask is merged on the host)
        host = {}
        if black:
            from .projection_utils import project_colored_voxels
            from .voxel_utils import get_voxel_points_by_parts
            grid_np = voxel_grid.numpy() if isinstance(voxel_grid, dev.DeviceGrid) else np.asarray(voxel_grid)
            for part, c8 in black:
                pts, col = get_voxel_points_by_parts(grid_np, {part: tuple(int(v) for v in c8)}, [part])
                if pts.shape[0] == 0:
                    continue
                proj = project_colored_voxels(pts, col, cam_params["cam_pos"], cam_params["target"], cam_params["f"], cam_params["cx"],
                                              cam_params["cy"], H, W)
                host[part] = (c8, proj, np.all(proj == c8, axis=-1))
        if mode == "part_on_part" and (live or host):
            raise NameError("name 'proj_f' is not defined")             # upstream's :414, at the first part that has voxels
        if mode not in OVERLAY_MODES:
            return []
        if len(live) > 8 * _SWEEP:
            raise ValueError(f"at most {8 * _SWEEP} parts with voxels")
        nplanes = (len(live) + _SWEEP - 1) // _SWEEP
        d_bits = sc.alloc(max(1, nplanes * npix) * 4)
        for s in range(nplanes):
            hit_bits_resident(d_g, shape, [c for _, c in live[s * _SWEEP:(s + 1) * _SWEEP]], cam_params, H, W, out=d_bits.at(s * npix * 4))
        d_img = sc.upload(img) or sc.alloc(1)
        tab = np.ascontiguousarray(np.array([c for _, c in live], np.uint8).reshape(-1, 3))
        bg = np.array(part_colors.get("background", (0, 0, 0)), dtype=np.uint8)
        m = OVERLAY_MODES[mode]
        nimg = len(live) if m == 0 else 1
        ncnt = 2 * len(live) if m == 0 else 2
        d_vis = sc.alloc(max(1, nimg * npix * 3))
        d_cnt = sc.alloc(max(1, ncnt) * 8)
        d_extra = None
        if m == 1 and host:
            extra = np.zeros((H, W), bool)
            for _, _, prj in host.values():
                extra |= prj
            d_extra = sc.upload(extra.view(np.uint8))
        _lib.check(_lib.load().pb3d_overlay_compose_resident(_lib.ctx(), C.c_void_p(d_bits.ptr), nplanes, C.c_void_p(d_img.ptr), H, W, _lib.p_u8(tab),
                                                        len(live), _lib.p_u8(bg), _ptr(d_extra), m, C.c_void_p(d_vis.ptr),
                                                        C.c_void_p(d_cnt.ptr)))
        vis = d_vis.download((nimg, H, W, 3)) if nimg else np.zeros((0, H, W, 3), np.uint8)
        cnt = d_cnt.download((max(1, ncnt),), np.int64)
        if m == 1:
            return [(None, f"Combined Binary | IoU: {_iou(cnt[0], cnt[1]):.3f}", vis[0], _iou(cnt[0], cnt[1]))]
        if m == 2:
            return [(None, "Combined Color Projection Overlay", vis[0], None)]      # a black projection adds nothing to the sum
        done = {part: (vis[j], _iou(cnt[2 * j], cnt[2 * j + 1])) for j, (part, _) in enumerate(live)}
        for part, (c8, proj, prj) in host.items():
            gt = np.all(img == c8, axis=-1)
            v = _outline_host((0.7 * proj + 0.3 * img).astype(np.uint8), gt, prj)
            done[part] = (v, _iou(np.logical_and(gt, prj).sum(), np.logical_or(gt, prj).sum()))
        return [(part, f"{part} | IoU: {done[part][1]:.3f}", done[part][0], done[part][1]) for part in part_colors if part in done]


def projection_overlays(voxel_grid, part_colors, image, cam_params, mode):
    """The images of visualize_voxel_projection_iou (:346-477) without matplotlib: [(title, vis, iou), ...] in upstream's order --
    'part_on_whole': one per part that has voxels; 'whole_on_whole': the combined binary overlay; 'whole_on_whole_color': the combined
    colour overlay (iou None: upstream computes none).  The grid (NumPy or DeviceGrid) is swept ONCE per 31 parts for the bits of
    every part (pb3d_grid_hit_bits_resident) and the images are composed in one launch (pb3d_overlay_compose_resident).
    'part_on_part' cannot run upstream (:414 names proj_f, which does not exist): NameError when any part has voxels, [] otherwise."""
    return [(title, vis, iou) for _, title, vis, iou in _overlays(voxel_grid, part_colors, image, cam_params, mode)]


def visualize_voxel_projection_iou(voxel_grid, part_colors, image, cam_params, mode='part_on_whole', save=False, save_root='visualisation'):
    """Show (and save) the overlays of projection_overlays with upstream's figures, titles, prints and file names (:346-477)."""
    import os

    import matplotlib.pyplot as plt
    if save:
        save_dir = os.path.join(save_root, mode)
        os.makedirs(save_dir, exist_ok=True)
    items = _overlays(voxel_grid, part_colors, image, cam_params, mode)
    if mode == "whole_on_whole":
        print("Visualizing combined binary projection vs. binary ground-truth...")
    if mode == "whole_on_whole_color":
        print("Visualizing full-color projection overlay...")
    names = {"whole_on_whole": "combined_binary_overlay.png", "whole_on_whole_color": "combined_color_overlay.png"}
    for part, title, vis, _ in items:
        plt.figure(figsize=(6, 6))
        plt.imshow(vis)
        plt.title(title)
        plt.axis("off")
        if save:
            path = os.path.join(save_dir, names.get(mode, f"{part}_overlay.png"))
            plt.savefig(path)
            print(f"Saved {path}")
        plt.show()
