"""NumPy restatement of notebook 2's device work (csrc/overlay.hip): the bounds of a colour set, the per-part hit bits of a projection
and the three overlay compositions of visualize_voxel_projection_iou (reference utils/camera_estimation.py:56-108, :346-477).

tools/gen_golden_overlays.py asserts every function here equal to the reference's own output before it writes a fixture; the tests
compare the kernels with it where no fixture is stored.  The projection is project_colored_voxels' arithmetic with NumPy's promotion
rules; as in test_visibility_kernels the matmul is written as the FMA chain NumPy's gemm evaluates (ref_frame)."""
import numpy as np

YELLOW = (255, 255, 0)


def part_mask(grid, colour):
    """voxels of an (A0,A1,A2,3) RGB grid (colour: 3 values) or an (A0,A1,A2) label grid (colour: one value) equal to `colour`"""
    g = np.asarray(grid)
    return np.all(g == np.asarray(colour), axis=-1) if g.ndim == 4 else g == np.asarray(colour).reshape(())


def selection(grid, colours):
    g = np.asarray(grid)
    if not len(colours):
        return np.any(g != 0, axis=-1) if g.ndim == 4 else g != 0
    m = np.zeros(g.shape[:3], bool)
    for c in colours:
        m |= part_mask(g, c)
    return m


def bounds(grid, colours):
    """(count, lo, hi) over np.where of the selection; lo / hi inclusive (a0, a1, a2) int64, or None when the count is 0"""
    idx = np.stack(np.where(selection(grid, colours)), 1)
    if len(idx) == 0:
        return 0, None, None
    return len(idx), idx.min(0).astype(np.int64), idx.max(0).astype(np.int64)


def points_of(mask):
    """voxel (a0, a1, a2) is the float32 point (a2, a1, a0), in np.where order"""
    a0, a1, a2 = np.where(mask)
    return np.stack([a2, a1, a0], axis=1).astype(np.float32)


def hit_mask(pts, cam, H, W):
    """(H, W) bool: the pixels project_colored_voxels paints for these points (Z < 1e-8 clamped, no depth test)"""
    from test_visibility_kernels import ref_frame
    out = np.zeros((H, W), bool)
    if len(pts) == 0:
        return out
    X, Y, Z = ref_frame(pts, cam)
    Z = np.where(Z < 1e-8, 1e-8, Z)
    with np.errstate(all="ignore"):
        u = np.round((X / Z) * cam["f"] + cam["cx"])
        v = np.round(-(Y / Z) * cam["f"] + cam["cy"])
        ok = (u >= 0) & (u < W) & (v >= 0) & (v < H)
    out[v[ok].astype(np.int64), u[ok].astype(np.int64)] = True
    return out


def hit_bits(grid, colours, cam, H, W):
    """(H, W) uint32, bit k = some voxel of colours[k] lands on the pixel"""
    bits = np.zeros((H, W), np.uint32)
    for k, c in enumerate(colours):
        bits |= hit_mask(points_of(part_mask(grid, c)), cam, H, W).astype(np.uint32) << np.uint32(k)
    return bits


def blend(a, b):
    return (0.7 * a + 0.3 * b).astype(np.uint8)


def dilate4(m):
    """one step of the 4-neighbour cross; outside the image is false"""
    d = m.copy()
    d[1:] |= m[:-1]; d[:-1] |= m[1:]; d[:, 1:] |= m[:, :-1]; d[:, :-1] |= m[:, 1:]
    return d


def iou(gt, prj):
    inter, union = np.logical_and(gt, prj).sum(), np.logical_or(gt, prj).sum()
    return inter / union if union > 0 else 0.0


def part_on_whole(painted, colour, image):
    """(vis, iou, outline pixels) of one part: `painted` the pixels its projection paints"""
    c = np.asarray(colour, np.uint8)
    proj = np.zeros_like(image)
    proj[painted] = c
    prj = np.all(proj == c, axis=-1)                 # everything, for a black part
    gt = np.all(image == c, axis=-1)
    vis = blend(proj, image)
    both = gt & prj
    outline = dilate4(both) & ~both
    vis[outline] = YELLOW
    return vis, iou(gt, prj), int(outline.sum())


def whole_on_whole(prj, image, bg):
    gt = np.any(image != np.asarray(bg, np.uint8), axis=-1)
    vis = np.zeros(image.shape, np.uint8)
    vis[gt & ~prj] = (0, 255, 0)
    vis[prj & ~gt] = (255, 0, 0)
    vis[gt & prj] = YELLOW
    return vis, iou(gt, prj)


def whole_on_whole_color(painted_list, colours, image):
    acc = np.zeros(image.shape, np.int64)
    for painted, c in zip(painted_list, colours):
        acc[painted] += np.asarray(c, np.int64)
    return blend(np.clip(acc, 0, 255).astype(np.uint8), image)


def overlays(grid, part_colors, image, cam, mode):
    """[(title, vis, iou)] as the reference emits them; `outlines` of part_on_whole are returned alongside as a list"""
    H, W = image.shape[:2]
    live = []
    for part, colour in part_colors.items():
        pts = points_of(part_mask(grid, colour))
        if len(pts):
            live.append((part, colour, hit_mask(pts, cam, H, W)))
    if mode == "part_on_part" and live:
        raise NameError("name 'proj_f' is not defined")
    out, outlines = [], []
    if mode == "part_on_whole":
        for part, colour, painted in live:
            vis, i, n = part_on_whole(painted, colour, image)
            out.append((f"{part} | IoU: {i:.3f}", vis, i)); outlines.append(n)
    elif mode == "whole_on_whole":
        prj = np.zeros((H, W), bool)
        for _, colour, painted in live:
            prj |= painted if np.any(np.asarray(colour) != 0) else np.ones((H, W), bool)
        vis, i = whole_on_whole(prj, image, part_colors.get("background", (0, 0, 0)))
        out.append((f"Combined Binary | IoU: {i:.3f}", vis, i))
    elif mode == "whole_on_whole_color":
        out.append(("Combined Color Projection Overlay", whole_on_whole_color([p for _, _, p in live], [c for _, c, _ in live], image), None))
    return out, outlines


# ---- the small synthetic cases shared by the generator and the tests ---------------------------------------------------------------
def palette(n, seed):
    """n distinct non-black colours"""
    rng = np.random.default_rng(seed)
    seen, out = set(), []
    while len(out) < n:
        c = tuple(int(v) for v in rng.integers(0, 256, 3))
        if c != (0, 0, 0) and c not in seen:
            seen.add(c); out.append(c)
    return out


def random_grid(shape, colours, fill, seed):
    rng = np.random.default_rng(seed)
    g = np.zeros(tuple(shape) + (3,), np.uint8)
    pick = rng.integers(0, len(colours), shape)
    occ = rng.random(shape) < fill
    g[occ] = np.asarray(colours, np.uint8)[pick[occ]]
    return g


def front_camera(shape, H, W, px_per_voxel=0.5, dtype=np.float32):
    """a camera in front of the grid (looking along +z = a0) at `px_per_voxel` image pixels per voxel at the grid's middle depth"""
    A0, A1, A2 = shape
    dist = 3.0 * max(shape)
    c = np.array([(A2 - 1) / 2, (A1 - 1) / 2, (A0 - 1) / 2])
    cam = {"cam_pos": (c + [0.3, 0.2, -dist]).astype(dtype), "target": c.astype(dtype), "f": px_per_voxel * dist, "cx": W / 2 - 0.5,
           "cy": H / 2 - 0.5}
    return cam


def synthetic_cases():
    """name -> (grid, part_colors, image, cam): the composition cases the fixtures store in full"""
    cases = {}
    # gt == prj reaches all four borders: a full slab seen at 0.5 px / voxel covers the whole 9 x 11 image; the image is the slab's
    # colour but for a hole and a second part in a corner
    cols = palette(3, 1)
    g = np.zeros((3, 24, 28, 3), np.uint8); g[:] = cols[0]; g[1, 2:6, 3:9] = cols[1]
    img = np.zeros((9, 11, 3), np.uint8); img[:] = cols[0]; img[4, 5] = cols[2]; img[0:2, 0:3] = cols[1]
    cases["borders"] = (g, {"slab": cols[0], "patch": cols[1], "none": cols[2], "background": cols[2]}, img, front_camera((3, 24, 28), 9, 11))
    # 33 parts: two sweeps; one more part without voxels, one colour outside uint8
    cols = palette(35, 2)
    pc = {f"p{k}": c for k, c in enumerate(cols[:33])}
    pc["absent"] = cols[33]; pc["wide"] = (300, 0, 0); pc["background"] = cols[34]
    g = random_grid((5, 30, 34), cols[:33], 0.5, 3)
    rng = np.random.default_rng(4)
    img = np.asarray(cols, np.uint8)[rng.integers(0, 35, (8, 9))].repeat(4, 0).repeat(4, 1)[:29, :33]
    cases["pal33"] = (g, pc, np.ascontiguousarray(img), front_camera((5, 30, 34), 29, 33, 0.9))
    # one black part (it selects the empty voxels) and no "background" entry (black is the default)
    cols = palette(2, 5)
    pc = {"a": cols[0], "void": (0, 0, 0), "b": cols[1]}
    g = random_grid((4, 10, 12), cols, 0.4, 6)
    rng = np.random.default_rng(7)
    img = np.asarray(cols + [(0, 0, 0)], np.uint8)[rng.integers(0, 3, (5, 7))]
    cases["black"] = (g, pc, np.ascontiguousarray(img), front_camera((4, 10, 12), 5, 7, 0.4))
    # two parts share a colour
    cols = palette(3, 8)
    pc = {"a": cols[0], "twin": cols[0], "b": cols[1], "background": cols[2]}
    g = random_grid((6, 14, 9), cols[:2], 0.3, 9)
    rng = np.random.default_rng(10)
    img = np.asarray(cols, np.uint8)[rng.integers(0, 3, (12, 10))]
    cases["twins"] = (g, pc, np.ascontiguousarray(img), front_camera((6, 14, 9), 12, 10, 0.8, np.float64))
    return cases
