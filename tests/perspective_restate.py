"""NumPy statement of perspective_carve (csrc/pcarve.hip; include/pb3d.h has the semantics) and the cases its fixtures store.

The projection is project_colored_voxels' own text (reference utils/projection_utils.py:5-23) but for the matmul, which is written
as the FMA chain NumPy's gemm evaluates (test_visibility_kernels.ref_frame), so that the result does not depend on the BLAS of the
machine the tests run on.  tools/gen_golden_perspective.py checks, before it writes a fixture, that these pixels reproduce the image
of the reference's own function for every case's points and cameras."""
import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def mask_set(mask):
    """(H, W) bool: a pixel is set where any of its values is non-zero"""
    m = np.asarray(mask)
    return np.any(m != 0, axis=2) if m.ndim == 3 else m != 0


def pixels(pts3d, cam, H, W):
    """(ui, vi, valid) of project_colored_voxels for (N, 3) points; ui, vi are meaningful where valid"""
    from test_visibility_kernels import ref_frame
    f, cx, cy = cam["f"], cam["cx"], cam["cy"]
    with np.errstate(all="ignore"):
        X, Y, Z = ref_frame(pts3d, cam)                 # pts_cam = (pts3d - cam_pos) @ R.T; X, Y, Z = pts_cam.T
        Z = np.where(Z < 1e-8, 1e-8, Z)
        u = (X / Z) * f + cx
        v = -(Y / Z) * f + cy
        ur, vr = np.round(u), np.round(v)
        valid = (ur >= 0) & (ur < W) & (vr >= 0) & (vr < H)     # NaN and values past int64 are outside
    ui = np.where(valid, ur, 0).astype(np.int64)
    vi = np.where(valid, vr, 0).astype(np.int64)
    return ui, vi, valid


def subject(grid, colors=None):
    """(A0, A1, A2) bool: occupied and, with colors, of one of them"""
    g = np.asarray(grid)
    occ = np.any(g != 0, axis=-1) if g.ndim == 4 else g != 0
    if colors is None:
        return occ
    sel = np.zeros(occ.shape, bool)
    for c in colors:
        sel |= np.all(g == np.asarray(c, np.uint8), axis=-1) if g.ndim == 4 else g == np.uint8(c)
    return occ & sel


def points_of(sel):
    """voxel (a0, a1, a2) is the float32 point (a2, a1, a0), in np.where order"""
    a0, a1, a2 = np.where(sel)
    return np.stack([a2, a1, a0], axis=1).astype(np.float32), (a0, a1, a2)


def carve(grid, views, colors=None, outside="carve"):
    """(carved grid, removed int64 (K,)): views apply in order, the first that rejects a voxel zeroes it"""
    assert outside in ("carve", "keep")
    out = np.array(grid, copy=True)
    removed = np.zeros(len(views), np.int64)
    live = subject(out, colors)
    for k, (mask, cam) in enumerate(views):
        m = mask_set(mask)
        H, W = m.shape
        pts, (a0, a1, a2) = points_of(live)
        if len(pts) == 0:
            continue
        ui, vi, valid = pixels(pts, cam, H, W)
        reject = np.where(valid, ~m[vi, ui], outside == "carve")
        out[a0[reject], a1[reject], a2[reject]] = 0
        live[a0[reject], a1[reject], a2[reject]] = False
        removed[k] = int(reject.sum())
    return out, removed


def pack_bits(mask):
    """(H, (W + 31) // 32) uint32: pixel u of a row is bit u & 31 of word u >> 5"""
    m = mask_set(mask)
    H, W = m.shape
    words = np.zeros((H, (W + 31) // 32), np.uint32)
    for u in range(W):
        words[:, u >> 5] |= m[:, u].astype(np.uint32) << np.uint32(u & 31)
    return words


def keep_bits(grid):
    """the occupancy of every second voxel per axis, packed: what the large fixture stores beside the digest of the whole grid"""
    g = np.asarray(grid)
    occ = np.any(g != 0, axis=-1) if g.ndim == 4 else g != 0
    return np.packbits(occ[::2, ::2, ::2].reshape(-1))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- cameras in fixtures: every value as a hex float with its dtype ("py" = a weak Python float) -------------------------------------
def cam_record(cam):
    rec = {}
    for k, v in cam.items():
        dt = str(np.asarray(v).dtype) if isinstance(v, (np.ndarray, np.generic)) else "py"
        rec[k] = {"hex": [float(x).hex() for x in np.asarray(v, np.float64).reshape(-1)], "dtype": dt}
    return rec


def cam_from_record(rec):
    cam = {}
    for k, r in rec.items():
        vals = [float.fromhex(h) for h in r["hex"]]
        if k in ("cam_pos", "target"):
            cam[k] = np.array(vals, dtype=r["dtype"])
        else:
            cam[k] = vals[0] if r["dtype"] == "py" else np.dtype(r["dtype"]).type(vals[0])
    return cam


# ---- the synthetic cases -----------------------------------------------------------------------------------------------------------
PALETTE = [(200, 30, 40), (10, 220, 90), (255, 255, 255), (1, 0, 0), (0, 0, 7)]


def rgb_grid(shape, fill, seed, colours=PALETTE):
    rng = np.random.default_rng(seed)
    g = np.zeros(tuple(shape) + (3,), np.uint8)
    occ = rng.random(shape) < fill
    g[occ] = np.asarray(colours, np.uint8)[rng.integers(0, len(colours), shape)[occ]]
    return g


def label_grid(shape, fill, seed, nlabels=6):
    rng = np.random.default_rng(seed)
    return (rng.integers(1, nlabels + 1, shape) * (rng.random(shape) < fill)).astype(np.uint8)


def blob_mask(H, W, p, seed, cell=3):
    """random cells of cell x cell pixels, set with probability p"""
    rng = np.random.default_rng(seed)
    low = rng.random(((H + cell - 1) // cell, (W + cell - 1) // cell)) < p
    return np.ascontiguousarray(low.repeat(cell, 0).repeat(cell, 1)[:H, :W])


def orbit_camera(shape, H, W, direction, px_per_voxel=1.0, dtype=np.float32, scalar=None):
    """a camera at 3 grid diameters from the grid's centre along `direction` (x, y, z), looking at the centre, with
    `px_per_voxel` pixels per voxel there; scalar: the type of f, cx, cy (None = Python floats)"""
    A0, A1, A2 = shape
    c = np.array([(A2 - 1) / 2, (A1 - 1) / 2, (A0 - 1) / 2])
    d = np.asarray(direction, np.float64)
    dist = 3.0 * max(shape)
    pos = c + d / np.linalg.norm(d) * dist
    wrap = (lambda x: x) if scalar is None else scalar
    return {"cam_pos": pos.astype(dtype), "target": c.astype(dtype), "f": wrap(px_per_voxel * dist), "cx": wrap(W / 2 - 0.25),
            "cy": wrap(H / 2 + 0.25)}


DIRECTIONS = [(0.1, 0.05, -1), (1, 0.2, 0.1), (0.3, 1, 0.2), (-1, 0.1, -0.4), (0.5, -0.3, 1), (-0.6, 0.8, 0.3), (0.2, -1, -0.3),
              (1, 1, 1), (-1, 0.5, 1)]


def synthetic_cases():
    """name -> {"grid", "views": [(mask, cam)], "colors": None or list, "outside", "trivial": bool}"""
    cases = {}

    def add(name, grid, views, colors=None, outside="carve", trivial=False):
        cases[name] = {"grid": grid, "views": views, "colors": colors, "outside": outside, "trivial": trivial}

    # ---- walk edges: A0 across the 64-step chunk with a ragged A2 (byte path); labels with whole dwords; a small RGB grid for offsets
    for name, g in (("walk_rgb_70x9x13", rgb_grid((70, 9, 13), 0.6, 11)), ("walk_lab_12x10x16", label_grid((12, 10, 16), 0.6, 12)),
                    ("walk_rgb_5x7x16", rgb_grid((5, 7, 16), 0.7, 13))):
        sh = g.shape[:3]
        H, W = max(sh) + 5, max(sh) + 9
        add(name, g, [(blob_mask(H, W, 0.8, 21), orbit_camera(sh, H, W, DIRECTIONS[0])),
                      (blob_mask(H + 3, W - 2, 0.8, 22), orbit_camera(sh, H + 3, W - 2, DIRECTIONS[1]))])

    # ---- nine views (the tests run the prefixes K = 0, 1, 3, 9): masks of their own sizes, widths off the 32-pixel word, three dtypes
    g = rgb_grid((20, 18, 24), 0.5, 31)
    views = []
    for k, d in enumerate(DIRECTIONS):
        H, W = 29 + 2 * k, 33 + 5 * k                   # 33 .. 73: one to three words per row, never a whole number of them
        m = blob_mask(H, W, 0.9, 40 + k)
        if k % 3 == 1:
            m = (m * np.random.default_rng(50 + k).integers(2, 256, m.shape)).astype(np.uint8)      # set pixels hold values other than 1
        elif k % 3 == 2:
            rgb = np.zeros(m.shape + (3,), np.uint8)
            rgb[m, np.random.default_rng(60 + k).integers(0, 3, int(m.sum()))] = 9                  # one channel set per pixel
            m = rgb
        views.append((m, orbit_camera(g.shape[:3], H, W, d, 1.2)))
    add("views9", g, views)

    # ---- arithmetic: each promotion path of the camera on one grid
    g = rgb_grid((10, 12, 14), 0.6, 71)
    sh, H, W = g.shape[:3], 21, 27
    m = blob_mask(H, W, 0.7, 72, cell=2)
    add("arith_f32", g, [(m, orbit_camera(sh, H, W, (0.4, 0.3, -1), 1.4))])
    cam = orbit_camera(sh, H, W, (0.4, 0.3, -1), 1.4)
    cam["cx"] = np.float64(cam["cx"])                                                   # float32 up to the shift by cx alone
    add("arith_cx64", g, [(m, cam)])
    cam = orbit_camera(sh, H, W, (0.4, 0.3, -1), 1.4)
    cam["f"] = np.float64(cam["f"]); cam["cy"] = np.float32(cam["cy"])                  # float64 from the scale by f on
    add("arith_f64scale", g, [(m, cam)])
    add("arith_f64cam", g, [(m, orbit_camera(sh, H, W, (0.4, 0.3, -1), 1.4, np.float64, np.float64))])
    # a camera inside the grid looking along +x: voxels behind it have Z < 1e-8 and take the clamp (those on its axis land on (cx, cy))
    cam = {"cam_pos": np.array([6.0, 5.0, 4.0], np.float32), "target": np.array([13.0, 5.5, 4.5], np.float32), "f": 6.0, "cx": 13.0, "cy": 10.0}
    add("arith_inside", g, [(m, cam)])
    # a mask smaller than the projected grid: the voxels outside it go or stay
    small = blob_mask(9, 11, 0.7, 73, cell=2)
    cam = orbit_camera(sh, 9, 11, (0.4, 0.3, -1), 1.4)
    add("outside_carve", g, [(small, cam)], outside="carve")
    add("outside_keep", g, [(small, cam)], outside="keep")
    # rint's half-to-even: an axis-aligned camera at depth 4 of the a0 = 0 plane with f = 2 puts every odd x and y on a .5
    g = rgb_grid((5, 16, 20), 0.8, 74)
    cam = {"cam_pos": np.array([9.0, 7.0, -4.0], np.float32), "target": np.array([9.0, 7.0, 0.0], np.float32), "f": 2.0, "cx": 6.0, "cy": 5.0}
    add("half_even", g, [(np.random.default_rng(75).random((11, 13)) < 0.5, cam)])

    # ---- subject colours: the others stay byte-identical
    g = rgb_grid((9, 11, 12), 0.7, 81)
    sh, H, W = g.shape[:3], 17, 19
    v = [(blob_mask(H, W, 0.6, 82, cell=2), orbit_camera(sh, H, W, (0.2, 0.4, -1), 1.3))]
    add("colors_rgb_none", g, v)
    add("colors_rgb_1", g, v, colors=[PALETTE[3]])
    add("colors_rgb_3", g, v, colors=[PALETTE[0], PALETTE[4], PALETTE[2]])
    g = label_grid((9, 11, 12), 0.7, 83)
    add("colors_lab_none", g, v)
    add("colors_lab_1", g, v, colors=[5])
    add("colors_lab_3", g, v, colors=[2, 6, 1])
    return cases


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------
def load_synthetic():
    """the committed synthetic cases: name -> (case dict as synthetic_cases gives it, carved grid, removed)"""
    meta = json.load(open(os.path.join(GOLDEN, "pcarve_synth.json")))
    out = {}
    with np.load(os.path.join(GOLDEN, "pcarve_synth.npz"), allow_pickle=False) as z:
        for name, rec in meta["cases"].items():
            views = [(z[f"{name}/mask{k}"], cam_from_record(c)) for k, c in enumerate(rec["cams"])]
            case = {"grid": z[f"{name}/grid"], "views": views, "colors": rec["colors"], "outside": rec["outside"], "trivial": rec["trivial"]}
            out[name] = (case, z[f"{name}/out"], z[f"{name}/removed"])
    return out


def stored_case(mon):
    """(grid, [(mask, cam)] front then drone) of a stored monument: its final cameras and its two masks resized to the grid"""
    import contextlib
    import io
    from pb3d import eval_helpers_intra as ev
    grid = np.load(os.path.join(GOLDEN, f"stored_{mon}_voxel_grid.npz"))["voxel_grid"]
    views = []
    for view in ("front", "drone"):
        with contextlib.redirect_stdout(io.StringIO()):
            mask = ev.resize_mask_to_voxel_grid(ev.load_mask(os.path.join(GOLDEN, f"data_{mon}_{view}_mask.png")), grid)
        views.append((np.ascontiguousarray(mask), ev.load_camera_json(os.path.join(GOLDEN, f"stored_{mon}_camera_params_final.json"), view)))
    return grid, views
