"""NumPy statement of perspective_paint (csrc/ppaint.hip; include/pb3d.h has the semantics) and the cases its fixtures store.

Nothing here is new arithmetic.  The pixel and depth of a voxel, the z-buffer and the visibility test are test_visibility_kernels'
restatement of the reference's compute_global_depth_buffer and project_part_visible (utils/eval_helpers_intra.py:134-190), whose
camera frame is the FMA chain NumPy's gemm evaluates (ref_frame), so the result does not depend on the BLAS of the machine the tests
run on.  tools/gen_golden_paint.py checks, before it writes a fixture, that every case's z-buffers and seen pixels are those of the
reference's own two functions."""
import json
import os

import numpy as np

import perspective_restate as pr
from perspective_restate import GOLDEN, cam_from_record, cam_record, sha  # noqa: F401  (the tests take them from here)

BACKGROUND = (216, 224, 251)        # PART_COLORS["background"]: what the masks hold where there is no part


def keys_of(a, C):
    """r | g << 8 | b << 16 of (..., 3) uint8 colours, or the labels themselves"""
    a = np.asarray(a)
    if C == 1:
        return a.astype(np.uint32)
    return a[..., 0].astype(np.uint32) | (a[..., 1].astype(np.uint32) << 8) | (a[..., 2].astype(np.uint32) << 16)


def zbuffers(grid, views):
    """the float32 (H, W) z-buffer of the grid under every view's camera: compute_global_depth_buffer"""
    from test_visibility_kernels import ref_grid_zbuf
    return [ref_grid_zbuf(grid, cam, *np.asarray(image).shape[:2]) for image, cam in views]


def paint(grid, views, colors=None, skip=(), eps=1e-3, zbufs=None, trace=None):
    """(painted grid, decided int64 (K,)): the views are tried in order, the first that paints a voxel decides its colour.
    zbufs None: the z-buffers of `grid` itself.  trace: a list that gets, per view, (seen, paints, ui, vi) over the subject voxels in
    np.where order (bool, bool, and the pixel where seen)."""
    from test_visibility_kernels import _visible, ref_pixels
    g = np.asarray(grid)
    C = 3 if g.ndim == 4 else 1
    out = np.array(g, copy=True)
    decided = np.zeros(len(views), np.int64)
    if len(views) > 8:
        raise ValueError("at most 8 views")
    pts, (a0, a1, a2) = pr.points_of(pr.subject(g, colors))
    if zbufs is None:
        zbufs = zbuffers(g, views)
    skip_keys = keys_of(np.asarray(list(skip), np.uint8).reshape(-1, C) if C == 3 else np.asarray(list(skip), np.uint8), C).reshape(-1)
    open_ = np.ones(len(pts), bool)
    for k, ((image, cam), zb) in enumerate(zip(views, zbufs)):
        img = np.asarray(image)
        H, W = img.shape[:2]
        assert img.dtype == np.uint8 and img.ndim == (3 if C == 3 else 2) and np.asarray(zb).shape == (H, W)
        ui, vi, Z, idx = ref_pixels(pts, cam, H, W)                 # Z > 1e-6 and the rounded pixel inside the image
        vis = _visible(Z, zb, vi, ui, eps)                          # |Z - zbuf[v, u]| < eps in NumPy's widths
        pix = img[vi, ui]
        key = keys_of(pix, C)
        paints = vis & (key != 0) & ~np.isin(key, skip_keys) & open_[idx]
        hit = idx[paints]
        out[a0[hit], a1[hit], a2[hit]] = pix[paints]
        open_[hit] = False
        decided[k] = int(paints.sum())
        if trace is not None:
            seen, p = np.zeros(len(pts), bool), np.zeros(len(pts), bool)
            seen[idx[vis]] = True; p[hit] = True
            trace.append((seen, p, ui[vis], vi[vis]))
    return out, decided


def changed_sample(grid, out):
    """(flat indices into out[::2, ::2, ::2] of the voxels painting changed, their new values): what the large fixture stores beside
    the digest of the whole grid"""
    g, o = np.asarray(grid)[::2, ::2, ::2], np.asarray(out)[::2, ::2, ::2]
    diff = (g != o).any(axis=-1) if g.ndim == 4 else g != o
    at = np.flatnonzero(diff)
    return at.astype(np.int32), o.reshape((-1, 3) if g.ndim == 4 else (-1,))[at]


# ---- the synthetic cases -----------------------------------------------------------------------------------------------------------
PAINTS = [(200, 30, 40), (10, 220, 90), (255, 255, 255), (1, 0, 0), (0, 0, 7), (90, 90, 200)]


def view_image(H, W, C, p_paint, seed, skip_value, p_black=0.1, cell=1):
    """an image whose cells hold a paint colour / label with probability p_paint, black / 0 with p_black, else skip_value"""
    rng = np.random.default_rng(seed)
    h, w = (H + cell - 1) // cell, (W + cell - 1) // cell
    r = rng.random((h, w))
    which = rng.integers(0, len(PAINTS), (h, w))
    if C == 3:
        img = np.empty((h, w, 3), np.uint8)
        img[:] = np.asarray(skip_value, np.uint8)
        img[r < p_paint] = np.asarray(PAINTS, np.uint8)[which[r < p_paint]]
    else:
        img = np.full((h, w), skip_value, np.uint8)
        img[r < p_paint] = (which[r < p_paint] + 1).astype(np.uint8)      # labels 1 .. 6
    img[r > 1 - p_black] = 0
    return np.ascontiguousarray(img.repeat(cell, 0).repeat(cell, 1)[:H, :W])


def synthetic_cases():
    """name -> {"grid", "views": [(image, cam)], "colors", "skip", "eps", "zbufs": None or [(H, W) float32]}"""
    cases = {}

    def add(name, grid, views, colors=None, skip=(), eps=1e-3, zbufs=None):
        cases[name] = {"grid": grid, "views": views, "colors": colors, "skip": list(skip), "eps": eps, "zbufs": zbufs}

    D = pr.DIRECTIONS
    # ---- walk edges: A0 across the 64-step chunk with a ragged A2 (byte loads and stores), two image sizes, a float32 camera
    g = pr.rgb_grid((70, 9, 13), 0.6, 111)
    sh = g.shape[:3]
    add("walk_rgb_70x9x13", g, [(view_image(150, 61, 3, 0.45, 121, BACKGROUND), pr.orbit_camera(sh, 150, 61, D[1], 2.0)),
                                (view_image(160, 50, 3, 0.6, 122, BACKGROUND, cell=2), pr.orbit_camera(sh, 160, 50, D[3], 2.0))], skip=[BACKGROUND])
    # ---- labels in rows of whole dwords: a float64 camera (np.float64 cam_pos) next to a float32 one, eps an np.float64, a label subset
    g = pr.label_grid((12, 10, 16), 0.6, 112)
    sh = g.shape[:3]
    add("walk_lab_12x10x16", g, [(view_image(41, 47, 1, 0.4, 123, 9), pr.orbit_camera(sh, 41, 47, D[0], 2.5, np.float64)),
                                 (view_image(37, 52, 1, 0.6, 124, 9), pr.orbit_camera(sh, 37, 52, D[4], 2.5))],
        colors=[2, 6, 1, 4], skip=[9], eps=np.float64(1e-3))
    # ---- a small RGB grid of whole dwords (the grid the offset tests move around), a colour subset
    g = pr.rgb_grid((5, 7, 16), 0.7, 113)
    sh = g.shape[:3]
    add("walk_rgb_5x7x16", g, [(view_image(40, 44, 3, 0.4, 125, BACKGROUND), pr.orbit_camera(sh, 40, 44, D[2], 2.5)),
                               (view_image(36, 48, 3, 0.6, 126, BACKGROUND), pr.orbit_camera(sh, 36, 48, D[6], 2.5, np.float64, np.float64))],
        colors=[pr.PALETTE[0], pr.PALETTE[4], pr.PALETTE[2], pr.PALETTE[1]], skip=[BACKGROUND, (1, 0, 0)])
    # ---- eight views in one call, each image of its own size, float32 and float64 cameras in turn; later images paint more
    g = pr.rgb_grid((20, 18, 24), 0.5, 131)
    sh = g.shape[:3]
    views = []
    for k in range(8):
        H, W = 70 + 2 * k, 75 + 5 * k
        views.append((view_image(H, W, 3, 0.14 / (1 - 0.1 * k), 140 + k, BACKGROUND, p_black=0.05),
                      pr.orbit_camera(sh, H, W, D[k], 2.4, np.float64 if k % 3 == 2 else np.float32)))
    add("views8", g, views, skip=[BACKGROUND])
    # ---- the skip list matters: the same call with it and without, where the background paints like any colour
    g = pr.rgb_grid((10, 12, 14), 0.6, 171)
    sh = g.shape[:3]
    v = [(view_image(40, 46, 3, 0.35, 172, BACKGROUND), pr.orbit_camera(sh, 40, 46, (0.4, 0.3, -1), 2.5)),
         (view_image(44, 42, 3, 0.5, 173, BACKGROUND), pr.orbit_camera(sh, 44, 42, (-0.5, 1, 0.6), 2.5))]
    add("skip_on", g, v, skip=[BACKGROUND, PAINTS[1]], eps=np.float64(1e-3))
    add("skip_off", g, v)
    # ---- z-buffers of another grid (the deformed grid of notebook 4): this grid with a slab in front of the first camera filled in
    other = np.array(g, copy=True)
    other[:2, 3:9, 2:9] = PAINTS[0]
    add("zbuf_other", g, v, skip=[BACKGROUND], zbufs=zbuffers(other, v))
    return cases


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------
def eps_record(eps):
    return {"hex": float(eps).hex(), "dtype": str(np.asarray(eps).dtype) if isinstance(eps, np.generic) else "py"}


def eps_from_record(rec):
    v = float.fromhex(rec["hex"])
    return v if rec["dtype"] == "py" else np.dtype(rec["dtype"]).type(v)


def load_synthetic():
    """the committed synthetic cases: name -> (case dict as synthetic_cases gives it, painted grid, decided)"""
    meta = json.load(open(os.path.join(GOLDEN, "ppaint_synth.json")))
    out = {}
    with np.load(os.path.join(GOLDEN, "ppaint_synth.npz"), allow_pickle=False) as z:
        for name, rec in meta["cases"].items():
            views = [(z[f"{name}/image{k}"], cam_from_record(c)) for k, c in enumerate(rec["cams"])]
            zbufs = [z[f"{name}/zbuf{k}"] for k in range(len(views))] if rec["zbufs"] else None
            tup = (lambda c: tuple(c) if isinstance(c, list) else c)
            case = {"grid": z[f"{name}/grid"], "views": views, "colors": None if rec["colors"] is None else [tup(c) for c in rec["colors"]],
                    "skip": [tup(c) for c in rec["skip"]], "eps": eps_from_record(rec["eps"]), "zbufs": zbufs}
            out[name] = (case, z[f"{name}/out"], z[f"{name}/decided"])
    return out


def stored_case(mon):
    """(grid, [(RGB mask, cam)] front then drone) of a stored monument: perspective_restate.stored_case"""
    return pr.stored_case(mon)
