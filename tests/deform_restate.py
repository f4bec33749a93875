"""NumPy float64 statement of the notebook-3 deformation closures (csrc/deform.hip; include/pb3d.h has the semantics) and the
constructed cases tests/golden/deform_edges.{npz,json} store.

deform_coords, the bounds filter, the colour pairing, the painted grid and the IoU of one deform tuple are the text of the reference's
closures (utils/deformation_estimation.py:70-98, :100-146, :262-313) in this project's words, written once for K deform tuples at a
time: every operation is an element-wise float64 NumPy operation, so a tuple's values do not depend on its neighbours in the list.  The
projection is perspective_restate.pixels (project_colored_voxels bit for bit, float32 and float64 cameras).
tools/gen_golden_deform.py checks, before it writes a fixture, that every case's rows, IoUs and grids are those of the closures.

`variant` switches ONE detail of the arithmetic to a plausible wrong one; tests/test_deform_host.py uses the variants to show that the
committed cases tell the right arithmetic from each of them.  Nothing else passes a variant."""
import json
import os
from fractions import Fraction

import numpy as np

import perspective_restate as pr
from perspective_restate import GOLDEN, cam_from_record, cam_record  # noqa: F401  (the tests take them from here)

JITTER = np.array([[0, 0, 0], [0.25, 0, 0], [-0.25, 0, 0], [0, 0.25, 0], [0, -0.25, 0], [0, 0, 0.25], [0, 0, -0.25]])
VARIANTS = ("half_away", "fma", "float32", "sign0_plus", "one_centre")


def scalars(image_shape, voxel_shape, deform):
    """(scale_xz, scale_y, kx, ky, kz): one_pass's five scalars, the shifts in voxels, formed with Python floats (:74-81)"""
    H_img, W_img = image_shape
    D, H, W = voxel_shape
    pix2vox_x = W / float(W_img)
    pix2vox_y = H / float(H_img)
    pix2vox_z = D / float(W_img)
    return (float(deform["scale_xz"]), float(deform["scale_y"]), deform["shift_xz"] * pix2vox_x, deform["shift_y"] * pix2vox_y,
            deform["shift_xz"] * pix2vox_z)


def _fma(a, b, c):
    """a * b + c rounded once: exact rational arithmetic, float() rounds to nearest even"""
    a, b, c = np.broadcast_arrays(a, b, c)
    out = np.empty(a.shape, np.float64)
    for i in np.ndindex(a.shape):
        out[i] = float(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
    return out


def values(pts, sc, variant=None):
    """(values before rounding (K, 7, n, 3), centred coordinates (7, n, 3)) for K rows of scalars()"""
    assert variant is None or variant in VARIANTS
    wt = np.float32 if variant == "float32" else np.float64
    sc = np.asarray(sc, np.float64).reshape(-1, 5).astype(wt)
    p = np.asarray(pts, np.float32).reshape(-1, 3)
    jit = (p[None].astype(np.float64) + JITTER[:, None, :]).astype(wt)          # coords + offset, per jitter
    centre = jit.mean(axis=1, keepdims=True)                                    # each jitter's own mean
    if variant == "one_centre":
        centre = np.broadcast_to(centre[:1], centre.shape)
    c = jit - centre
    sign = (lambda v: np.where(v >= 0, 1.0, -1.0).astype(wt)) if variant == "sign0_plus" else np.sign
    sxz, sy, kx, ky, kz = (sc[:, a][:, None, None] for a in range(5))
    if variant == "fma":
        x = _fma(c[..., 0], sxz, kx * sign(c[..., 0]))
        y = _fma(c[..., 1], sy, -ky)
        z = _fma(c[..., 2], sxz, kz * sign(c[..., 2]))
    else:
        x = c[..., 0] * sxz + kx * sign(c[..., 0])
        y = c[..., 1] * sy - ky
        z = c[..., 2] * sxz + kz * sign(c[..., 2])
    return np.stack([x, y, z], axis=-1) + centre, c


def rounded(pts, sc, variant=None):
    """(K, 7n, 3) int64: np.round(...).astype(int) of every (jitter, point), jitters stacked as np.vstack does"""
    v, _ = values(pts, sc, variant)
    r = np.sign(v) * np.floor(np.abs(v) + 0.5) if variant == "half_away" else np.round(v)
    return r.astype(np.int64).reshape(len(v), -1, 3)


def in_bounds(rows, voxel_shape):
    A0, A1, A2 = voxel_shape
    return ((rows[..., 0] >= 0) & (rows[..., 0] < A2) & (rows[..., 1] >= 0) & (rows[..., 1] < A1) &
            (rows[..., 2] >= 0) & (rows[..., 2] < A0))


def deform_coords(pts, image_shape, voxel_shape, deform, variant=None):
    """np.unique(np.vstack(seven passes), axis=0): int64 rows (x, y, z) in lexicographic order"""
    return np.unique(rounded(pts, scalars(image_shape, voxel_shape, deform), variant)[0], axis=0)


def nvalid(pts, image_shape, voxel_shape, deform, variant=None):
    """the (point, jitter) pairs whose deformed coordinate is inside the grid, counted before np.unique"""
    return int(in_bounds(rounded(pts, scalars(image_shape, voxel_shape, deform), variant)[0], voxel_shape).sum())


def part_points(grid, labels, part):
    """get_voxel_points_by_parts for one part: float32 (x, y, z) in np.where order, and the voxels' colours"""
    z, y, x = np.where(np.all(grid == np.asarray(labels[part], grid.dtype), axis=-1))
    return np.stack([x, y, z], axis=1).astype(np.float32), grid[z, y, x]


def pair_colors(colors, m):
    """np.repeat(colors, max(1, int(m / len) + 1), axis=0)[:m]"""
    return np.repeat(colors, repeats=max(1, int(m / len(colors)) + 1), axis=0)[:m]


def deform_part(grid, labels, part, deform, image_shape, variant=None):
    """(in-bounds unique rows, the colours paired with them) of one part; an absent part gives empty arrays"""
    pts, colors = part_points(grid, labels, part)
    if len(pts) == 0:
        return np.zeros((0, 3), np.int64), np.zeros((0, 3), np.uint8)
    cd = deform_coords(pts, image_shape, grid.shape[:3], deform, variant)
    cd = cd[in_bounds(cd, grid.shape[:3])]
    return cd, pair_colors(colors, len(cd))


def paint(out, cd, cols):
    """voxel_def[z, y, x] = colours"""
    out[cd[:, 2], cd[:, 1], cd[:, 0]] = cols
    return out


def build_deformed_grid(grid, labels, saved, image_shape, variant=None):
    """save_deformed_grid: every saved part painted into a zero grid in the order of `labels`"""
    out = np.zeros_like(grid, dtype=np.uint8)
    for part in labels:
        if part not in saved:
            continue
        cd, cols = deform_part(grid, labels, part, saved[part]["deform"], image_shape, variant)
        if cd.size:
            paint(out, cd, cols)
    return out


def iou_counts_sc(pts, voxel_shape, sc, image, cam, colour, variant=None, dense=True):
    """(inter, uni, nvalid) int64 (K,) for K rows of scalars: the in-bounds unique rows of every tuple projected as float32, the image
    of the pixels hit in `colour` compared with `image` as compute_partwise_iou does.  dense=False forms the union as
    |image part| + |pixels hit| - inter without building K images (not for a black colour, which every unhit pixel matches)."""
    image = np.asarray(image)
    H, W = image.shape[:2]
    colour = np.asarray(colour, np.uint8)
    rows = rounded(pts, sc, variant)                                            # (K, 7n, 3)
    K = len(rows)
    ok = in_bounds(rows, voxel_shape)
    nv = ok.sum(axis=1).astype(np.int64)
    k = np.broadcast_to(np.arange(K)[:, None], ok.shape)[ok]
    cd = np.unique(np.column_stack([k, rows[ok]]), axis=0)                      # each tuple's unique in-bounds rows, in order
    ui, vi, valid = pr.pixels(cd[:, 1:].astype(np.float32), cam, H, W)
    k, ui, vi = cd[valid, 0], ui[valid], vi[valid]
    gt = np.all(image == colour, axis=-1)
    if dense:
        proj = np.zeros((K, H, W, 3), np.uint8)
        proj[k, vi, ui] = colour
        hit = np.all(proj == colour, axis=-1)
        return (hit & gt).sum(axis=(1, 2)).astype(np.int64), (hit | gt).sum(axis=(1, 2)).astype(np.int64), nv
    assert colour.any()
    px = np.unique(k * (H * W) + vi * W + ui)
    nhit = np.bincount(px // (H * W), minlength=K)
    inter = np.bincount(px // (H * W), weights=gt.reshape(-1)[px % (H * W)].astype(np.float64), minlength=K).astype(np.int64)
    return inter, int(gt.sum()) + nhit - inter, nv


def iou_counts(pts, voxel_shape, deform, image, cam, colour, variant=None):
    """(inter, uni, nvalid) of one deform dict"""
    sc = scalars(np.asarray(image).shape[:2], voxel_shape, deform)
    return tuple(int(v[0]) for v in iou_counts_sc(pts, voxel_shape, [sc], image, cam, colour, variant))


def iou(inter, uni):
    """compute_partwise_iou's value"""
    return inter / uni if uni > 0 else 0.0


def half_count(v):
    """how many values sit exactly on .5"""
    return int(np.count_nonzero(np.abs(v - np.trunc(v)) == 0.5))


# ---- the constructed clouds -----------------------------------------------------------------------------------------------------------
def D(scale_xz=1.0, scale_y=1.0, shift_xz=0.0, shift_y=0.0):
    return {"scale_y": scale_y, "shift_y": shift_y, "scale_xz": scale_xz, "shift_xz": shift_xz}


def mirrored(n, mean2, seed, spread=6):
    """n points (n even) in mirrored pairs q, 2 * mean - q: the mean is exactly mean2 / 2 per axis"""
    rng = np.random.default_rng(seed)
    q = rng.integers(-spread, spread + 1, (n // 2, 3)) + np.asarray(mean2) // 2
    return np.concatenate([q, np.asarray(mean2) - q]).astype(np.float32)


def fma_pairs():
    """three (axis, c, scale, k) with fl(c * scale) + k on a .5 that the exactly rounded c * scale + k leaves on the side half-to-even
    does not take: found by a search in exact rational arithmetic over small integers c, scales with no finite binary expansion and
    shifts in half voxels.  A cloud {-c, +c} on the axis has the mean 0, so the value before rounding is fl(c * scale) + k itself."""
    found = []
    scales = (1 / 3, 0.7, 1.1, 0.9, 1.3, 0.6)
    for axis in (0, 1, 2):
        for c in range(3, 200):
            for s in scales:
                if any(f[1] == c or f[2] == s for f in found):
                    continue
                prod = float(c) * s
                exact = Fraction(c) * Fraction(s)
                if Fraction(prod) == exact or prod * 2 != np.floor(prod * 2):
                    continue
                for k2 in range(-1, 3):                                # k so that prod + k is -0.5, 0.5, 1.5 or 2.5
                    k = (k2 + 0.5) - prod
                    unfused = np.round(prod + k)
                    fused = np.round(float(exact + Fraction(k)))
                    if prod + k == k2 + 0.5 and unfused != fused:
                        found.append((axis, c, s, k))
                        break
                if len(found) > axis:
                    break
            if len(found) > axis:
                break
    assert len(found) == 3
    return found


def cloud_cases():
    """name -> {"pts" float32 (n, 3), "image_shape", "voxel_shape", "deform", "kind"}"""
    cases = {}

    def add(name, kind, pts, deform, voxel_shape=(16, 16, 16), image_shape=None):
        image_shape = tuple(voxel_shape[1:]) if image_shape is None else image_shape
        cases[name] = {"pts": np.ascontiguousarray(pts, np.float32), "image_shape": tuple(image_shape), "voxel_shape": tuple(voxel_shape),
                       "deform": deform, "kind": kind}

    # ---- ties: dyadic means on both sides of zero (twice the mean is given), dyadic scales, shifts in quarter voxels; pix2vox = 1
    tie_deforms = [D(2.0, 0.5, 0.25, -0.75), D(1.5, 1.5, -1.25, 2.5), D(0.5, 1.0, 0.5, 0.25), D(1.0, 2.0, 1.75, -0.5)]
    for i, n in enumerate((2, 4, 8, 64)):
        for j, mean2 in enumerate(((8, 9, 6), (-7, -10, -5), (0, 1, 0))):
            add(f"tie_n{n}_m{j}", "tie", mirrored(n, mean2, 100 + 10 * i + j), tie_deforms[(i + j) % 4])
    # ---- sign(0): odd symmetric clouds, the middle point on the centre in x, in z, in both, in neither; one point alone
    mid = {"x": [[2, 1, 3], [5, 4, 9], [8, 10, 3]], "z": [[1, 1, 3], [7, 4, 6], [1, 10, 9]], "xz": [[2, 1, 3], [5, 4, 6], [8, 10, 9]],
           "none": [[1, 1, 2], [7, 4, 8], [1, 10, 2]]}
    for which, p in mid.items():
        add(f"sign0_{which}_n3", "sign0", p, D(1.5, 1.0, 2.25, -1.0))
    add("sign0_xz_n5", "sign0", [[0, 0, 2], [3, 9, 5], [4, 2, 6], [5, 1, 7], [8, 3, 10]], D(2.0, 0.5, -1.5, 0.75))
    add("sign0_n1", "sign0", [[3, 5, 2]], D(2.0, 1.5, 3.0, -2.0))
    # ---- fused multiply-add sensitive, one per axis: {-c, +c} on the axis, the other coordinates fixed
    # The +-0.25 jitters of the tied axis land on both neighbours of the tie whatever the tie does, so the other axes are shifted by
    # 0.4 of a voxel: there a jitter moves the rounded value, and the rows (tied value, moved value) exist on one side of the tie only.
    for axis, c, s, k in fma_pairs():
        p = np.array([[1, 2, 3], [1, 2, 3]], np.float64)
        p[:, axis] = (-c, c)
        if axis == 1:
            p[:, 0], p[:, 2] = (2, 4), (3, 5)
            d = D(scale_xz=1.0, scale_y=s, shift_xz=0.4, shift_y=-k)            # y: c * s - ky
        else:
            p[:, 1] = (2, 4)
            d = D(scale_xz=s, scale_y=1.0, shift_xz=k, shift_y=-0.4)            # x, z: c * s + k * sign(c)
        add(f"fma_{'xyz'[axis]}", "fma", p, d)
    # ---- float32 sensitive: coordinates near 2^21, a scale with no finite binary expansion
    rng = np.random.default_rng(7)
    add("f32_near_2p21", "f32", (1 << 21) - rng.integers(1, 40, (9, 3)), D(1.1, 0.9, 3.0, -2.0))
    # ---- the mean is sum / n, rounded
    for n in (3, 7):
        add(f"mean_n{n}", "mean", np.random.default_rng(30 + n).integers(-9, 12, (n, 3)), D(1.1, 1.3, 2.0, -3.0))
    # ---- duplicates: a block halved (many jitters on one voxel), repeated input rows, a far shift, negative coordinates
    blk = np.stack(np.meshgrid(range(4), range(4), range(4), indexing="ij"), -1).reshape(-1, 3)
    add("dup_half", "dup", blk + 3, D(0.5, 0.5, 0.0, 0.0))
    rep = np.array([[1, 2, 3], [4, 0, 2], [1, 2, 3], [7, 7, 1], [4, 0, 2], [1, 2, 3], [0, 5, 5], [7, 7, 1], [1, 2, 3], [4, 0, 2]])
    add("dup_rows", "dup", rep, D(1.5, 1.0, 0.5, -0.25))
    add("far_shift_y", "dup", blk[::3] + 2, D(1.0, 1.0, 0.0, 100000.0))
    add("negative", "dup", -np.random.default_rng(41).integers(1, 30, (12, 3)), D(1.5, 0.5, -40.0, 30.0))
    # ---- bounds on a grid of three lengths: rows at -1, 0, A - 1 and A of every axis (the identity keeps them), then a stretch
    A0, A1, A2 = 5, 7, 9
    faces = np.stack(np.meshgrid([-1, 0, A2 - 1, A2], [-1, 0, A1 - 1, A1], [-1, 0, A0 - 1, A0], indexing="ij"), -1).reshape(-1, 3)
    add("bounds_identity", "bounds", faces, D(), (A0, A1, A2), (14, 18))
    inner = np.stack(np.meshgrid(range(2, 7), range(1, 6), range(1, 4), indexing="ij"), -1).reshape(-1, 3)
    add("bounds_stretch", "bounds", inner, D(2.0, 2.0, 0.0, 0.0), (A0, A1, A2), (14, 18))
    add("bounds_all_in", "bounds", inner, D(), (A0, A1, A2), (14, 18))
    for a, (sh_xz, sh_y) in enumerate(((0.0, 14.0), (0.0, -14.0), (20.0, 0.0))):
        add(f"bounds_push{a}", "bounds", inner, D(1.0, 1.0, sh_xz, sh_y), (A0, A1, A2), (14, 18))
    add("bounds_all_out", "bounds", inner, D(1.0, 1.0, 0.0, 40.0), (A0, A1, A2), (14, 18))
    return cases


# ---- the scenes: a grid of parts, an image, a camera, the deform saved for some parts --------------------------------------------------
COLOURS = {"dome": (190, 0, 255), "plinth": (63, 138, 173), "windows": (255, 120, 230), "chhatris": (1, 220, 5), "main_door": (180, 140, 255)}


def front_camera(shape, Himg, Wimg, dtype=np.float32):
    A0, A1, A2 = shape
    c = np.array([A2 / 2, A1 / 2, A0 / 2])
    return {"cam_pos": (c + [0.5, 0.25, -3.0 * max(shape)]).astype(dtype), "target": c.astype(dtype), "f": 2.5 * Wimg, "cx": Wimg / 2 - 0.25,
            "cy": Himg / 2 + 0.25}


def scene_image(grid, labels, cam, H, W):
    """the image a scene is compared with: the undeformed parts projected, in the order of `labels`"""
    img = np.zeros((H, W, 3), np.uint8)
    for part in labels:
        pts, cols = part_points(grid, labels, part)
        if len(pts):
            ui, vi, valid = pr.pixels(pts, cam, H, W)
            img[vi[valid], ui[valid]] = cols[valid]
    return img


def scenes():
    """name -> {"grid", "labels" (ordered), "image", "cam", "saved": {part: deform}}"""
    out = {}

    def add(name, shape, boxes, saved, image_shape, labels=None, cam_dtype=np.float32):
        grid = np.zeros(tuple(shape) + (3,), np.uint8)
        for part, (z, y, x) in boxes:
            grid[z, y, x] = COLOURS[part]
        labels = {p: COLOURS[p] for p in (labels or [b[0] for b in boxes])}
        cam = front_camera(shape, *image_shape, dtype=cam_dtype)
        out[name] = {"grid": grid, "labels": labels, "image": scene_image(grid, labels, cam, *image_shape), "cam": cam, "saved": saved}

    s = slice
    # ties: blocks of 64, 8 and 2 voxels (dyadic means), dyadic scales, quarter-voxel shifts, pix2vox = 1
    add("ties", (16, 16, 16), [("dome", (s(4, 8), s(5, 9), s(6, 10))), ("plinth", (s(10, 12), s(2, 4), s(1, 3))), ("windows", (s(3, 4), s(12, 13), s(11, 13)))],
        {"dome": D(1.5, 0.5, 0.25, -0.75), "plinth": D(2.0, 1.5, -1.25, 2.5), "windows": D(0.5, 2.0, 1.75, -0.5)}, (16, 16))
    # sign(0): odd blocks whose middle voxel is the centre, one voxel alone, non-zero shift_xz; a float64 camera
    add("sign0", (16, 16, 16), [("dome", (s(5, 8), s(5, 8), s(6, 9))), ("plinth", (s(11, 12), s(3, 4), s(2, 3))), ("windows", (s(2, 3), s(10, 13), s(9, 14)))],
        {"dome": D(2.0, 1.0, 2.25, -1.0), "plinth": D(1.5, 0.5, 3.0, 2.0), "windows": D(1.0, 1.5, -1.5, 0.75)}, (16, 16), cam_dtype=np.float64)
    # bounds: three lengths; stretched and pushed through the faces
    add("bounds_579", (5, 7, 9), [("dome", (s(1, 4), s(1, 6), s(2, 7))), ("plinth", (s(0, 1), s(0, 2), s(0, 3))), ("windows", (s(4, 5), s(5, 7), s(6, 9)))],
        {"dome": D(2.0, 2.0, 0.0, 0.0), "plinth": D(1.0, 1.0, 0.0, 4.0), "windows": D(1.5, 1.0, 6.0, -2.0)}, (14, 18))
    # paint order: three parts whose deformed sets overlap, one that leaves the grid, one never saved
    add("order", (9, 11, 13), [("dome", (s(2, 6), s(2, 7), s(2, 8))), ("plinth", (s(3, 7), s(4, 9), s(6, 11))), ("windows", (s(1, 4), s(6, 10), s(4, 9))),
                               ("chhatris", (s(7, 9), s(0, 2), s(0, 2))), ("main_door", (s(0, 1), s(9, 11), s(11, 13)))],
        {"dome": D(1.25, 1.0, 1.0, 0.0), "plinth": D(1.0, 1.25, -1.0, 1.0), "windows": D(1.5, 1.5, 0.0, -1.0), "chhatris": D(1.0, 1.0, 0.0, 60.0)},
        (22, 26), labels=["windows", "main_door", "plinth", "chhatris", "dome"])
    return out


# ---- tuple lists for pb3d_deform_iou_batch_dev (scalars as scalars() forms them) --------------------------------------------------------
ORDINARY = [(1.1, 0.9, 1.0, 2.0, 1.0), (0.9, 1.2, -0.5, -1.5, -0.5), (1.0, 1.0, 0.0, 0.0, 0.0)]
TIE_SC = [(2.0, 0.5, 0.25, -0.75, 0.25), (1.5, 1.5, -1.25, 2.5, -1.25), (0.5, 1.0, 0.5, 0.25, 0.5), (1.0, 2.0, 1.75, -0.5, 1.75)]


def batch_bounds(case):
    """the grid a cloud's batch is clipped by: the case's own, or for clouds far from the origin a box that ends just past them"""
    p = case["pts"]
    if case["kind"] == "f32":
        return tuple(int(p[:, a].max()) + 2 for a in (2, 1, 0))
    return case["voxel_shape"]


def mixed_batch(case):
    """(K, 5): ordinary tuples, the case's own, the tie tuples, one that puts everything outside, one clipping at each face"""
    A0, A1, A2 = batch_bounds(case)
    own = scalars(case["image_shape"], case["voxel_shape"], case["deform"])
    clip = [(1.0, 1.0, 0.0, float(A1) / 2, 0.0), (1.0, 1.0, 0.0, -float(A1) / 2, 0.0), (1.0, 1.0, A2 / 2.0, 0.0, 0.0), (1.0, 1.0, 0.0, 0.0, A0 / 2.0),
            (3.0, 1.0, 0.0, 0.0, 0.0), (1.0, 3.0, 0.0, 0.0, 0.0)]
    return np.array(ORDINARY[:2] + [own] + TIE_SC + [(1.0, 1.0, 0.0, 1e7, 0.0)] + clip + ORDINARY[2:], np.float64)


def lattice(K, special=()):
    """(K, 5) distinct dyadic tuples (mixed radix 7, 9, 11, 13 over scale_xz, scale_y, kx, ky; kz follows kx) with `special` = {index: tuple}"""
    k = np.arange(K)
    sc = np.stack([0.5 + 0.25 * (k % 7), 0.625 + 0.125 * (k // 7 % 9), -2.625 + 0.5 * (k // 63 % 11), -3.125 + 0.5 * (k // 693 % 13),
                   -2.625 + 0.5 * (k // 63 % 11) + 0.25 * (k % 2)], axis=1)
    for i, t in dict(special).items():
        sc[i] = t
    assert K <= 9009 and len(np.unique(sc, axis=0)) == K
    return sc


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------------
def deform_record(d):
    return {k: float(v).hex() for k, v in d.items()}


def deform_from_record(r):
    return {k: float.fromhex(v) for k, v in r.items()}


def load():
    """the committed cases: (clouds: name -> (case, unique rows), scenes: name -> (scene, {part: (rows, iou)}, deformed grid))"""
    meta = json.load(open(os.path.join(GOLDEN, "deform_edges.json")))
    clouds, scn = {}, {}
    with np.load(os.path.join(GOLDEN, "deform_edges.npz"), allow_pickle=False) as z:
        for name, r in meta["clouds"].items():
            case = {"pts": z[f"cloud/{name}/pts"], "image_shape": tuple(r["image_shape"]), "voxel_shape": tuple(r["voxel_shape"]),
                    "deform": deform_from_record(r["deform"]), "kind": r["kind"]}
            clouds[name] = (case, z[f"cloud/{name}/coords"])
        for name, r in meta["scenes"].items():
            sc = {"grid": z[f"scene/{name}/grid"], "labels": {p: tuple(c) for p, c in r["labels"]}, "image": z[f"scene/{name}/image"],
                  "cam": cam_from_record(r["cam"]), "saved": {p: deform_from_record(d) for p, d in r["saved"].items()}}
            parts = {p: (z[f"scene/{name}/coords/{p}"], float.fromhex(r["iou"][p])) for p in r["saved"]}
            scn[name] = (sc, parts, z[f"scene/{name}/out"])
    return clouds, scn
