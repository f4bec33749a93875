"""Constructed scenes for the fused component loop of left_right_guided_carve (csrc/guided.hip), and a plain restatement of the
reference function: NumPy / SciPy only, no GPU.

A scene is a colour grid (W, H, D, 3) of solid boxes of ONE part colour that do not touch, so each box is one 6-connected component
whose bounding box is the box itself.  Every scene is seeded; about 3 % of the voxels are punched out and about 2 % get a foreign
colour, but never one of the eight corners of a box; the semantic mask carries the part colour on about 88 % of its pixels.  What a
scene is there for is a property of its boxes (CLAIMS): the x-z cell count of a crop selects the form of k_crop_chain<NB>
(nbt = ceil(Wc * Dc / 4096): 1 -> <1>, 2 -> <2>, 3 -> <3>, 4 and 5 -> <5>), its height the number of 32-plane groups, its depth the
divisionless (xs, zs) stepping.  scene() checks every claim against scipy.ndimage.label of the grid it built -- the component count,
every bounding box, the nbt classes -- so a builder that degenerates fails before any kernel runs.

restate() is left_right_guided_carve (reference utils/voxel_carving_utils.py:163-210) in plain SciPy: ndimage.label for the
components, affine_transform(order=1, mode="constant", cval=0) with numpy.linalg.inv of the Y rotation and the offset c - M c
(c = shape / 2) for every angle of range(0, 91, angle), the 2-D crop mask after every step, then clear-the-component and
paste-the-survivors.  wrong=True is a deliberately WRONG variant in which a later crop is cut from the grid as carved so far, not
from the original: on a scene whose boxes overlap it must differ, which is what makes that scene able to fail."""
import numpy as np
from scipy import ndimage

from oracle.oracle import PART_COLORS

COLOR = np.array(PART_COLORS["dome"], np.uint8)
FOREIGN = np.array(PART_COLORS["plinth"], np.uint8)
BACKGROUND = np.array(PART_COLORS["background"], np.uint8)
PCN = {k: np.array(v, np.uint8) for k, v in PART_COLORS.items()}

K_MAX_LDS = 150 * 1024          # kMaxLds of csrc/guided.hip
CELLS_PER_NB = 8 * 512          # cells a workgroup of k_crop_chain evaluates per unit of NB


def nbt_of(box):
    """the ceil(Wc * Dc / 4096) that picks k_crop_chain<NB> for a crop (guided.hip, `nbt`)"""
    x0, y0, z0, x1, y1, z1 = box
    return -(-((x1 - x0) * (z1 - z0)) // CELLS_PER_NB)


def fits_lds(box):
    """two LDS planes of (Wc + 1) * (Dc | 1) + 1 dwords and Wc mask words within kMaxLds, offsets within 16 bits (guided.hip)"""
    x0, y0, z0, x1, y1, z1 = box
    Wc, Dc = x1 - x0, z1 - z0
    plane = (Wc + 1) * (Dc | 1) + 1
    return plane < 65536 and (2 * plane + Wc) * 4 <= K_MAX_LDS


def boxes_overlap(a, b):
    return all(a[k] < b[3 + k] and b[k] < a[3 + k] for k in range(3))


# ---- builders: name -> (grid shape (W, H, D), components, seed); a component is a list of slabs (x0, x1, y0, y1, z0, z1) -----------
def _many():
    comps = [[(0, 93, 0, 33, 0, 89)]]
    spots = [(x, z) for z in (90, 94) for x in range(0, 100, 4)] + [(94, z) for z in range(0, 86, 4)]
    hs = (1, 31, 32, 33)
    for k, (x, z) in enumerate(spots):
        comps.append([(x, x + 3, 0, hs[k % 4], z, z + 3)])
    for j, k in enumerate((0, 4, 8)):              # three more above boxes of height 1 (one empty plane between)
        x, z = spots[k]
        comps.append([(x, x + 3, 2, 2 + hs[j], z, z + 3)])
    assert len(comps) == 76
    return comps


SPECS = {
    "nb2": ((72, 36, 70), [[(3, 68, 2, 35, 2, 67)]], 11),
    "nb3_nb2": ((140, 35, 100), [[(1, 93, 1, 34, 4, 95)], [(95, 139, 0, 34, 0, 100)]], 23),
    "nb4": ((116, 33, 116), [[(2, 113, 0, 33, 3, 114)]], 13),
    "nb5_corner": ((137, 40, 137), [[(0, 137, 3, 40, 0, 137)]], 14),
    "thin": ((20, 34, 620), [[(1, 4, 0, 33, 5, 613)], [(6, 19, 33, 34, 0, 620)]], 15),
    "tall": ((70, 140, 66), [[(2, 68, 5, 70, 0, 65)], [(2, 68, 72, 136, 1, 66)]], 16),
    "many": ((100, 34, 100), _many(), 17),
    "ell": ((76, 40, 76), [[(1, 40, 3, 30, 30, 50)], [(5, 72, 5, 38, 3, 8), (68, 72, 5, 38, 3, 73)]], 18),
    "over": ((138, 10, 138), [[(0, 138, 1, 9, 0, 138)]], 19),
    "plate_z": ((30, 40, 9), [[(2, 27, 1, 38, 4, 5)]], 20),
    "plate_x": ((9, 40, 30), [[(4, 5, 1, 38, 2, 27)]], 21),
    # for the odd-base-offset runs of tests/test_pointer_offsets.py only: small, its large box ends at the volume's last voxel
    "corner_small": ((21, 37, 19), [[(0, 1, 0, 3, 0, 2)], [(2, 21, 1, 37, 3, 19)]], 22),
}
NAMES = tuple(n for n in SPECS if n != "corner_small")
FUSED = tuple(n for n in NAMES if n != "over")          # every crop fits the LDS: the fused loop must take them

# what each scene is there for, from its construction alone: crops as (Wc, Hc, Dc) in label order, then properties of them
CLAIMS = {
    "nb2": {"crops": [(65, 33, 65)], "nbt": [2]},
    "nb3_nb2": {"crops": [(92, 33, 91), (44, 34, 100)], "nbt": [3, 2]},
    "nb4": {"crops": [(111, 33, 111)], "nbt": [4]},
    "nb5_corner": {"crops": [(137, 37, 137)], "nbt": [5], "ends_at_last_voxel": True},
    "thin": {"crops": [(3, 33, 608), (13, 1, 620)], "nbt": [1, 2]},
    "tall": {"crops": [(66, 65, 65), (66, 64, 65)], "nbt": [2, 2], "groups": [3, 2], "last_np": [1, 32]},
    "many": {"ncomp": 76, "first_crop": (93, 33, 89), "nbt_max": 3, "disjoint": True},
    "ell": {"crops": [(39, 27, 20), (67, 33, 70)], "nbt": [1, 2], "overlap": True},
    "over": {"crops": [(138, 8, 138)], "fits": False},
    "plate_z": {"crops": [(25, 37, 1)], "nbt": [1]},
    "plate_x": {"crops": [(1, 37, 25)], "nbt": [1]},
    "corner_small": {"crops": [(1, 3, 2), (19, 36, 16)], "nbt": [1, 1], "ends_at_last_voxel": True},
}

# the angle steps every scene is run at, and the additional ones: 1 -> 90 rotation steps, 7 -> 12 steps (the last at 84 degrees),
# 90 -> one step, 120 -> an empty rotation loop; 60 on the overlap scene
ANGLES = {n: (5, 45) for n in NAMES}
ANGLES["nb2"] = (5, 45, 1, 7, 90, 120)
ANGLES["ell"] = (5, 45, 60)


class Scene:
    def __init__(self, name, grid, sem, boxes):
        self.name, self.grid, self.sem, self.boxes = name, grid, sem, boxes       # boxes: (n, 6) int64 lo | hi, in label order
        self.color = COLOR
        self.shape = grid.shape[:3]


def _punch(grid, comps, rng, foreign):
    """about 3 % holes and about 2 % voxels of a foreign colour, never a corner of a slab"""
    shape = grid.shape[:3]
    r = rng.random(shape)
    keep = np.zeros(shape, bool)
    for slabs in comps:
        for x0, x1, y0, y1, z0, z1 in slabs:
            for x in (x0, x1 - 1):
                for y in (y0, y1 - 1):
                    for z in (z0, z1 - 1):
                        keep[x, y, z] = True
    occupied = grid.any(-1)
    grid[(r < 0.03) & ~keep] = 0
    grid[(r >= 0.03) & (r < 0.05) & ~keep & occupied] = foreign


def _sem(rng, H, W, color, share=0.88):
    sem = np.empty((H, W, 3), np.uint8)
    sem[:] = BACKGROUND
    sem[rng.random((H, W)) < share] = color
    return sem


def component_boxes(member):
    """(count, (n, 6) int64 boxes lo | hi in label order) of scipy.ndimage.label of a membership mask"""
    lab, n = ndimage.label(member)
    objs = ndimage.find_objects(lab)
    return n, np.array([[s.start for s in o] + [s.stop for s in o] for o in objs], np.int64).reshape(n, 6)


def _build(name):
    shape, comps, seed = SPECS[name]
    rng = np.random.default_rng(seed)
    W, H, D = shape
    grid = np.zeros(shape + (3,), np.uint8)
    for slabs in comps:
        for x0, x1, y0, y1, z0, z1 in slabs:
            assert 0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H and 0 <= z0 < z1 <= D, (name, slabs)
            grid[x0:x1, y0:y1, z0:z1] = COLOR
    _punch(grid, comps, rng, FOREIGN)
    sem = _sem(rng, H, W, COLOR)
    # ---- the claims, from scipy.ndimage.label of what was built --------------------------------------------------------------
    intended = sorted(tuple(min(s[a] for s in slabs) for a in (0, 2, 4)) + tuple(max(s[a] for s in slabs) for a in (1, 3, 5)) for slabs in comps)
    n, boxes = component_boxes(np.all(grid == COLOR, axis=-1))
    assert n == len(comps), (name, "components", n, len(comps))
    assert sorted(tuple(int(v) for v in b) for b in boxes) == intended, (name, "bounding boxes")
    cl = CLAIMS[name]
    crops = [(int(b[3] - b[0]), int(b[4] - b[1]), int(b[5] - b[2])) for b in boxes]
    if "crops" in cl:
        assert crops == cl["crops"], (name, crops)
    if "nbt" in cl:
        assert [nbt_of(b) for b in boxes] == cl["nbt"], name
    assert all(fits_lds(b) for b in boxes) == cl.get("fits", True), name
    if "groups" in cl:
        assert [(c[1] + 31) // 32 for c in crops] == cl["groups"] and [c[1] - 32 * ((c[1] - 1) // 32) for c in crops] == cl["last_np"], name
    if cl.get("ends_at_last_voxel"):
        assert tuple(boxes[-1][3:]) == shape and grid[-1, -1, -1].any(), name
    if "ncomp" in cl:
        assert n == cl["ncomp"] and crops[0] == cl["first_crop"] and max(nbt_of(b) for b in boxes) == cl["nbt_max"], name
        assert min(c[0] * c[2] for c in crops) == 9 and {c[1] for c in crops[1:]} == {1, 31, 32, 33}, name
    pairs = any(boxes_overlap(boxes[i], boxes[j]) for i in range(n) for j in range(i + 1, n))
    assert pairs == bool(cl.get("overlap", False)), (name, "overlap")
    m = np.all(sem == COLOR, axis=-1).mean()
    assert 0.85 <= m <= 0.90 or H * W < 400, (name, m)
    for a in (grid, sem, boxes):
        a.setflags(write=False)
    return Scene(name, grid, sem, boxes)


_built = {}


def scene(name):
    """the scene, built (and its claims checked) once per process; nobody writes to it"""
    if name not in _built:
        _built[name] = _build(name)
    return _built[name]


def nbt_classes():
    """the nbt classes of every crop of every scene"""
    return {nbt_of(b) for n in NAMES for b in scene(n).boxes}


# ---- the two-part scene of partwise_carve: a 92 x 91 crop of one part colour, a 65 x 65 crop of another, a small third part ----------
TWO_PART_JOBS = [(["dome", "plinth", "main_door"], 120)]             # an angle step beyond 90: part_carve only applies the 2-D mask
TWO_PART_SYMMETRY = {"dome": 5, "plinth": 45, "main_door": 45}
_two = {}


def two_part():
    """(grid, sem, masked, boxes): `masked` is what part_carve(grid, sem, TWO_PART_JOBS) leaves (the columns whose pixel carries one
    of the three colours), boxes[part] the component boxes of that part's colour in it, from scipy"""
    if _two:
        return _two["v"]
    rng = np.random.default_rng(31)
    W, H, D = 96, 70, 100
    slabs = {"dome": (1, 93, 1, 34, 4, 95), "plinth": (3, 68, 36, 69, 2, 67), "main_door": (80, 90, 40, 50, 70, 80)}
    grid = np.zeros((W, H, D, 3), np.uint8)
    for part, (x0, x1, y0, y1, z0, z1) in slabs.items():
        grid[x0:x1, y0:y1, z0:z1] = PCN[part]
    _punch(grid, [[s] for s in slabs.values()], rng, PCN["windows"])
    sem = np.empty((H, W, 3), np.uint8)
    sem[:] = BACKGROUND
    sem[0:35] = PCN["dome"]; sem[35:] = PCN["plinth"]; sem[38:52, 78:92] = PCN["main_door"]
    drop = rng.random((H, W)) < 0.12
    for x0, x1, y0, y1, z0, z1 in slabs.values():                       # the corner columns of every box stay
        for x in (x0, x1 - 1):
            for y in (y0, y1 - 1):
                drop[y, x] = False
    sem[drop] = BACKGROUND
    keep = np.zeros((H, W), bool)
    for part in slabs:
        keep |= np.all(sem == PCN[part], axis=-1)
    masked = grid * keep.T[:, :, None, None].astype(np.uint8)
    boxes = {part: component_boxes(np.all(masked == PCN[part], axis=-1))[1] for part in slabs}
    for part, nbt in (("dome", 3), ("plinth", 2), ("main_door", 1)):
        b = boxes[part]
        x0, x1, y0, y1, z0, z1 = slabs[part]
        assert len(b) >= 1 and tuple(int(v) for v in b[0]) == (x0, y0, z0, x1, y1, z1), (part, b[0])
        assert max(nbt_of(q) for q in b) == nbt_of(b[0]) == nbt and all(fits_lds(q) for q in b), part
    for a in (grid, sem, masked):
        a.setflags(write=False)
    _two["v"] = (grid, sem, masked, boxes)
    return _two["v"]


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def _rotinv(angle):
    a = np.deg2rad(angle)
    c, s = np.cos(a), np.sin(a)
    return np.linalg.inv(np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]))


def process(occ, mask2d, angle):
    """process_voxel_grid (reference :104-126): rotate about Y by 0, angle, 2 angle, ... <= 90 degrees, the 2-D mask after every step"""
    W, H, D = occ.shape
    m = np.asarray(mask2d)
    m = m.T if m.shape[:2] == (H, W) else m
    assert m.shape == (W, H)
    c = np.array(occ.shape) / 2
    out = occ
    for a in range(0, 91, angle):
        M = _rotinv(a)
        out = ndimage.affine_transform(out, M, offset=c - M @ c, order=1, mode="constant", cval=0)
        out = np.where(m[:, :, None], out, 0)
    return out


def restate(grid, sem, color, angle, wrong=False):
    """-> (carved grid, [((x0, y0, z0, x1, y1, z1), carved voxels)] per component in label order), or (copy, None) when the mask
    does not hold the colour.  wrong=True: crops are cut from the grid as carved so far."""
    carved = grid.copy()
    mask2d = np.all(sem == color, axis=-1)
    if not mask2d.any():
        return carved, None
    lab, n = ndimage.label(np.all(grid == color, axis=-1))
    comps = []
    for i in range(1, n + 1):
        m3 = lab == i
        idx = np.argwhere(m3)
        x0, y0, z0 = (int(v) for v in idx.min(axis=0))
        x1, y1, z1 = (int(v) + 1 for v in idx.max(axis=0))
        sub = (carved if wrong else grid)[x0:x1, y0:y1, z0:z1].copy()
        occ = np.any(sub > 0, axis=-1).astype(np.uint8)
        kept = process(occ, mask2d[y0:y1, x0:x1], angle)
        comps.append(((x0, y0, z0, x1, y1, z1), int(np.count_nonzero(kept))))
        paste = sub * kept[:, :, :, None]
        view = carved[x0:x1, y0:y1, z0:z1]
        view[m3[x0:x1, y0:y1, z0:z1]] = 0
        on = np.any(paste > 0, axis=-1)
        view[on] = paste[on]
    return carved, comps


def log_text(color, comps):
    """what the reference prints for these components (:172, :176, :187, :195)"""
    if comps is None:
        return f"[SKIP] No mask for color {color}\n"
    lines = [f"[{color}] 3D components: {len(comps)}"]
    for i, ((x0, y0, z0, x1, y1, z1), count) in enumerate(comps, 1):
        lines.append(f"  - Component {i}: bbox ({x0},{y0},{z0}) → ({x1},{y1},{z1})")
        lines.append(f"    carved voxels: {count}")
    return "\n".join(lines) + "\n"


def crop_masks(sem, color, boxes):
    """the (Wc, Hc) truthiness images of every component's crop of the 2-D mask (reference :189, _mask_to_wh), packed back to back:
    (bytes, offsets)"""
    mask2d = np.all(sem == color, axis=-1)
    parts, offs, o = [], [], 0
    for x0, y0, z0, x1, y1, z1 in (tuple(int(v) for v in b) for b in boxes):
        m = np.ascontiguousarray(mask2d[y0:y1, x0:x1].T).astype(np.uint8)
        assert m.shape == (x1 - x0, y1 - y0)
        parts.append(m.reshape(-1)); offs.append(o); o += m.size
    return np.concatenate(parts), np.array(offs, np.int64)
