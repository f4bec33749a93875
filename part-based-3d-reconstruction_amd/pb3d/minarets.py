"""Minaret extraction and top / bottom keypoints; host mirror of reference utils/camera_estimation.py:20-50 (extract_minaret_kps_for_view),
:176-216 (extract_minaret_voxels_by_label), :247-325 (extract_minaret_masks_by_label) and :329-344 (the keypoints).

The components come from the device labelling (pb3d_label_colors_conn_stats_dev: up to eight colours in one sequence, with per-component
box, count and coordinate sums), and the chosen few are turned into coordinates, masks and extreme-row sums by one walk of their boxes
(pb3d_component_members_dev) -- no pass over the whole grid per component."""
import ctypes as C

import numpy as np

from . import _lib, device as dev, voxel_carving_utils as vcu, voxel_utils as vu
from ._args import _on_device

__all__ = ["extract_minaret_voxels_by_label", "extract_minaret_masks_by_label", "extract_top_bottom_voxel_points",
           "extract_top_bottom_image_points", "extract_minaret_kps_for_view"]

_MAX_SEL = 8                # selections per pb3d_component_members_dev call (PB3D_CCL_MAX_COLORS)
_COORDS, _ROWS, _MASK = 1, 2, 4


class _Labelling:
    """The components of the distinct colours `cols` (uint8 triples) of a resident grid at `connectivity`, labelled into `d_lab` eight colours
    per labelling call.  recs[i] = (n, bbox, count, sums, group) of colour i; `group` names the labelling call whose volume holds its labels,
    and current() re-makes that volume when a later call has overwritten it (labels are numbered per colour, deterministically)."""

    def __init__(self, d_g, shape3, cols, d_lab, connectivity, cap):
        self.d_g, self.shape3, self.cols, self.d_lab, self.conn = d_g, shape3, cols, d_lab, connectivity
        self.recs = [None] * len(cols)
        self.cur = None
        for s in range(0, len(cols), _MAX_SEL):
            chunk = list(range(s, min(s + _MAX_SEL, len(cols))))
            st = vu._label_stats_conn(d_g, shape3, [cols[i] for i in chunk], d_lab, connectivity, cap=cap, members_only=True)
            self.cur = ("chunk", s)
            for i, (n, bbox, cnt, sums) in zip(chunk, st):
                self.recs[i] = (int(n), bbox, cnt, sums, self.cur)
            for i, (n, bbox, cnt, sums) in zip(chunk, st):
                if bbox is not None:
                    continue
                # more components than the records hold: this colour alone, a full label volume, then the statistics pass if still needed
                n, bbox, cnt, sums = vu._label_stats_conn(d_g, shape3, [cols[i]], d_lab, connectivity, cap=min(int(n), vu._RECORDS_MAX))[0]
                if bbox is None:
                    bbox, cnt, sums = vcu._component_stats(d_lab, shape3, int(n))
                self.cur = ("solo", i)
                self.recs[i] = (int(n), bbox, cnt, sums, self.cur)

    def current(self, group):
        if group != self.cur:
            kind, i = group
            idx = list(range(i, min(i + _MAX_SEL, len(self.cols)))) if kind == "chunk" else [i]
            vu._label_stats_conn(self.d_g, self.shape3, [self.cols[j] for j in idx], self.d_lab, self.conn, cap=1, members_only=kind == "chunk")
            self.cur = group


def _distinct(colors):
    """per given colour the index of its distinct uint8 colour (None: a colour no uint8 voxel can equal), and the distinct colours"""
    cols, index, where = [], {}, []
    for c in colors:
        cu8 = vcu._color_u8(c)
        if cu8 is None:
            where.append(None)
            continue
        key = bytes(cu8)
        if key not in index:
            index[key] = len(cols)
            cols.append(cu8)
        where.append(index[key])
    return cols, where


def _members(lab, sel, outputs):
    """pb3d_component_members_dev for the selections sel = [(colour index, label, bbox row, count)], grouped by the labelling that holds
    them.  Returns per selection a dict with "coords" (int64 (n, 3)), "rows" (int64 (2, 4)) and / or "mask" (uint8 (A0, A1, A2))."""
    A0, A1, A2 = lab.shape3
    nvox = A0 * A1 * A2
    out = [dict() for _ in sel]
    groups = {}
    for j, (ci, _, _, _) in enumerate(sel):
        groups.setdefault(lab.recs[ci][4], []).append(j)
    # the labelling made last first: the common case (one labelling holds every selection) re-labels nothing
    for group in sorted(groups, key=lambda g: g != lab.cur):
        js = groups[group]
        lab.current(group)
        k = len(js)
        cols = np.ascontiguousarray(np.stack([lab.cols[sel[j][0]] for j in js]))
        labels = np.ascontiguousarray([sel[j][1] for j in js], np.int32)
        bbox = np.ascontiguousarray(np.stack([sel[j][2] for j in js]), np.int64)
        counts = np.ascontiguousarray([sel[j][3] for j in js], np.int64)
        ntot = int(counts.sum())
        with dev.Scope() as sc:
            d_coords = sc.alloc(max(ntot, 1) * 24) if outputs & _COORDS else None
            d_rows = sc.alloc(k * 64) if outputs & _ROWS else None
            d_masks = sc.alloc(max(k * nvox, 1)) if outputs & _MASK else None
            ptr = lambda b: None if b is None else C.c_void_p(b.ptr)
            _lib.check(_lib.load().pb3d_component_members_dev(
                _lib.ctx(), C.c_void_p(lab.d_g.ptr), A0, A1, A2, 3, C.c_void_p(lab.d_lab.ptr), k, _lib.p_u8(cols),
                labels.ctypes.data_as(C.POINTER(C.c_int32)), bbox.ctypes.data_as(_lib.i64p), counts.ctypes.data_as(_lib.i64p), outputs,
                ptr(d_coords), ptr(d_rows), ptr(d_masks)))
            if d_coords is not None:
                xyz = d_coords.download((ntot, 3), np.int64)
                ends = np.cumsum(counts)
                for q, j in enumerate(js):
                    out[j]["coords"] = xyz[ends[q] - counts[q]:ends[q]]
            if d_rows is not None:
                rows = d_rows.download((k, 2, 4), np.int64)
                for q, j in enumerate(js):
                    out[j]["rows"] = rows[q]
            if d_masks is not None:
                m = d_masks.download((k, A0, A1, A2), np.uint8)
                for q, j in enumerate(js):
                    out[j]["mask"] = m[q]
    return out


def _rgb_grid(grid, what):
    """(the DeviceGrid or the uint8 array to upload, lattice shape) of a NumPy (A0, A1, A2, 3) uint8 grid or a pb3d.device.DeviceGrid"""
    g = grid if isinstance(grid, dev.DeviceGrid) else _lib.as_u8(grid, what)
    if len(g.shape) != 4 or g.shape[3] != 3:
        raise ValueError(f"{what} must be (A0,A1,A2,3)")
    return g, tuple(int(v) for v in g.shape[:3])


def _four_minarets(lab, where):
    """the selections (colour index, label, bbox, count) of LM1, LM2, RM1, RM2 in a labelling of the distinct colours; where[k] = the
    distinct index of the k-th given colour"""
    # one ndimage.label per colour in the order given (a repeated colour counts twice), components in label order
    comps = [(ci, i) for ci in where if ci is not None and lab is not None for i in range(lab.recs[ci][0])]
    if len(comps) < 4:
        raise ValueError(f"Expected ≥4 minarets, found {len(comps)}")
    heights = np.array([lab.recs[ci][1][i, 4] - 1 - lab.recs[ci][1][i, 1] for ci, i in comps], np.int64)
    top4 = [comps[q] for q in np.argsort(-heights, kind="stable")[:4]]
    # coords.mean(axis=0) of integer coordinates: the exact sum over the count
    centroids = np.stack([lab.recs[ci][3][i].astype(np.float64) / lab.recs[ci][2][i] for ci, i in top4])
    order_x = np.argsort(centroids[:, 0])
    left, right = order_x[:2], order_x[2:]
    left = sorted(left, key=lambda i: centroids[i, 2])
    right = sorted(right, key=lambda i: centroids[i, 2])
    sel = [(ci, i + 1, lab.recs[ci][1][i], int(lab.recs[ci][2][i])) for ci, i in top4]
    return [sel[q] for q in (left[0], left[1], right[0], right[1])]


def _minaret_voxels(voxel_grid, minaret_colors, outputs):
    """the four minarets of extract_minaret_voxels_by_label: {"LM1", "LM2", "RM1", "RM2": _members' outputs for that component}"""
    g, shape3 = _rgb_grid(voxel_grid, "voxel_grid")
    with dev.Scope() as sc:
        d_g = _on_device(sc, g)
        cols, where = _distinct(minaret_colors)
        nvox = int(np.prod(shape3, dtype=np.int64))
        d_lab = sc.alloc(max(nvox, 1) * 4) if nvox and cols else None
        lab = _Labelling(d_g, shape3, cols, d_lab, 6, 1024) if d_lab is not None else None
        got = _members(lab, _four_minarets(lab, where), outputs)
        return dict(zip(("LM1", "LM2", "RM1", "RM2"), got))


def extract_minaret_voxels_by_label(voxel_grid, minaret_colors):
    """The four tallest 6-connected components of the minaret colours, as {"LM1", "LM2", "RM1", "RM2": int64 (n, 3) coordinates};
    reference :176-216.

    voxel_grid: uint8 (A0, A1, A2, 3) NumPy array or pb3d.device.DeviceGrid (left unchanged).  Components are those of one
    ndimage.label per colour, in the order the colours are given (a colour listed twice counts twice; one outside 0..255 has no
    members).  Height is the ptp of a component's axis-1 coordinates -- what the reference's `coords[:, 1].ptp()` gives under NumPy 1.x
    (NumPy 2 removed ndarray.ptp; the port computes the NumPy 1.x value).  The first four of a stable sort by -height are split by
    centroid axis 0 (np.argsort) into the left and right pair, each ordered by centroid axis 2.  Coordinates are np.argwhere's: raster
    order, columns in axis order (a0, a1, a2) -- not the (x, y, z) of get_voxel_points_by_parts.  Fewer than four components raise
    ValueError."""
    return {name: r["coords"] for name, r in _minaret_voxels(voxel_grid, minaret_colors, _COORDS).items()}


def _mask_regions(image, minaret_colors, min_area):
    """the chosen regions of extract_minaret_masks_by_label: [(name, region)], region = (colour index, label, bbox, count)"""
    img = _lib.as_u8(image, "image")
    if img.ndim != 3 or img.shape[2] < 3:
        raise ValueError("image must be (H, W, 3) or (H, W, 4)")
    rgb = np.ascontiguousarray(img[:, :, :3])
    H, W = rgb.shape[:2]
    shape3 = (1, H, W)
    cols, where = _distinct(minaret_colors)
    with dev.Scope() as sc:
        d_g = sc.upload(rgb) if cols else None
        d_lab = sc.alloc(H * W * 4) if d_g is not None else None
        # skimage.measure.label's default connectivity is ndim (8 neighbours in 2-D): the 26-connected labelling of the (1, H, W) view
        lab = _Labelling(d_g, shape3, cols, d_lab, 26, 4096) if d_g is not None else None
        regions = []
        for color_idx, ci in enumerate(where):
            if ci is None or lab is None:
                continue
            n, bbox, cnt, sums, _ = lab.recs[ci]
            for i in range(n):
                if cnt[i] < min_area:
                    continue
                centroid = (sums[i, 1] / np.float64(cnt[i]), sums[i, 2] / np.float64(cnt[i]))     # (row, column), regionprops' centroid
                regions.append({"color_idx": color_idx, "centroid": centroid, "sel": (ci, i + 1, bbox[i], int(cnt[i]))})
        if len(regions) < 2:
            raise ValueError("Not enough minarets for camera alignment")
        regions.sort(key=lambda r: r["centroid"][1])
        mid = len(regions) // 2

        def pick_front_back(rs):
            if len(rs) == 1:
                return rs[0], None
            rs = sorted(rs, key=lambda r: (r["color_idx"], r["centroid"][0]))
            return rs[0], rs[1]

        lm1, lm2 = pick_front_back(regions[:mid])
        rm1, rm2 = pick_front_back(regions[mid:])
        chosen = [(name, r) for name, r in (("LM1", lm1), ("RM1", rm1), ("LM2", lm2), ("RM2", rm2)) if r is not None]
        got = _members(lab, [r["sel"] for _, r in chosen], _MASK)
        return {name: g["mask"].reshape(H, W) for (name, _), g in zip(chosen, got)}


def extract_minaret_masks_by_label(image, minaret_colors, min_area=50):
    """{"LM1", "RM1", "LM2", "RM2" (those present, in this order): uint8 (H, W) 0/1 mask}; reference :247-325.

    image: uint8 (H, W, 3) or (H, W, 4) (only the first three channels are read).  Regions are the 8-connected components of each colour
    (skimage.measure.label's default connectivity), in label order -- raster order of their first pixel, which is also skimage's
    numbering -- colour by colour in the order given; regions with area < min_area are skipped.  Fewer than two regions raise ValueError.
    The regions are sorted (stably) by centroid column and split at len // 2 into left and right; on each side the first two by
    (colour index, centroid row) are the front (1) and back (2) minaret."""
    return _mask_regions(image, minaret_colors, min_area)


def extract_top_bottom_voxel_points(voxel_parts):
    """{"<name>_bottom", "<name>_top": float64 (3,) mean of the coordinates on the lowest / highest axis-1 row}; reference :329-335."""
    out = {}
    for name, vox in voxel_parts.items():
        ys = vox[:, 1]
        out[f"{name}_bottom"] = vox[ys == ys.min()].mean(axis=0)
        out[f"{name}_top"] = vox[ys == ys.max()].mean(axis=0)
    return out


def extract_top_bottom_image_points(mask_parts):
    """{"<name>_top", "<name>_bottom": (x mean, y)} of a mask's first / last non-zero row; reference :338-344.  "Top" is the smallest y
    (image rows grow downwards), the opposite sense of the voxel keypoints."""
    out = {}
    for name, mask in mask_parts.items():
        ys, xs = np.nonzero(mask)
        out[f"{name}_top"] = (xs[ys == ys.min()].mean(), ys.min())
        out[f"{name}_bottom"] = (xs[ys == ys.max()].mean(), ys.max())
    return out


def extract_minaret_kps_for_view(voxel_grid, mask_img, minaret_colors, back_top_only=False):
    """(voxel keypoints, image keypoints) of the minarets seen in both the grid and the mask; reference :20-50.

    The voxel keypoints come from the bottom / top row sums of the device (the coordinate sets are not downloaded); they equal
    extract_top_bottom_voxel_points of extract_minaret_voxels_by_label.  Kept: both keypoints of a minaret whose name contains "1", the
    "_top" keypoint of one whose name contains "2".  The reference orders the keys by set iteration (which depends on the string hash
    seed); here the minarets come in the order LM1, LM2, RM1, RM2 and each minaret's "_bottom" before its "_top", in both dicts.
    back_top_only is accepted and unused, as in the reference.  ValueError when fewer than two minarets are common to both or fewer than
    two keypoints survive the filter."""
    voxel_parts = _minaret_voxels(voxel_grid, minaret_colors, _ROWS)
    mask_parts = extract_minaret_masks_by_label(mask_img, minaret_colors)
    common = [k for k in ("LM1", "LM2", "RM1", "RM2") if k in voxel_parts and k in mask_parts]
    if len(common) < 2:
        raise ValueError("Not enough visible minarets")
    voxel_kps = {}
    for name in common:
        rows = voxel_parts[name]["rows"]
        voxel_kps[f"{name}_bottom"] = rows[0, 1:].astype(np.float64) / rows[0, 0]
        voxel_kps[f"{name}_top"] = rows[1, 1:].astype(np.float64) / rows[1, 0]
    image_kps = extract_top_bottom_image_points({k: mask_parts[k] for k in common})
    voxel_sel, image_sel = {}, {}
    for k in voxel_kps:
        m = k.split("_")[0]
        if ("1" in m) or ("2" in m and "top" in k):
            voxel_sel[k] = voxel_kps[k]
            image_sel[k] = image_kps[k]
    if len(voxel_sel) < 2:
        raise ValueError("Not enough keypoints after filtering")
    return voxel_sel, image_sel
