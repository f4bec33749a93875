"""Constructed inputs of tests/test_meshify_pinned.py and the CPU probes that say what each of them reaches: lattices in which every
voxel has a colour of its own (a colour names the voxel the nearest search chose), every (cube case, zbits) pair, the 256-cube block
seams of the mesh passes, and the seams of the nearest search of k_mesh_colors (csrc/mesh.hip).  Needs no device."""
import functools

import numpy as np

import mesh_restate as mr

OFF = (255, 254, 253)    # colour of the voxels off the stride lattice: no lattice index reaches it


# ---- grids whose colours name their voxels -----------------------------------------------------------------------------------
def full_shape(lattice, stride, tail=(0, 0, 0)):
    """the smallest full-resolution shape with that lattice, plus tail (< stride) voxels past the last lattice point"""
    assert all(0 <= t < stride for t in tail)
    return tuple((n - 1) * stride + 1 + t for n, t in zip(lattice, tail))


def index_grid(occ, stride=1, tail=(0, 0, 0)):
    """(A0, A1, A2, 3) uint8: lattice voxel t (scan order) of grid[::s, ::s, ::s] is coloured t + 1 (R, G, B = the three bytes) where
    occ is set and black elsewhere; voxels off the lattice are OFF"""
    n = occ.shape
    t = np.arange(occ.size, dtype=np.int64).reshape(n) + 1
    assert t.max() < (OFF[0] << 16)
    lat = (np.stack([t >> 16, (t >> 8) & 255, t & 255], -1) * occ[..., None]).astype(np.uint8)
    grid = np.empty(full_shape(n, stride, tail) + (3,), np.uint8)
    grid[:] = OFF
    grid[::stride, ::stride, ::stride] = lat
    assert grid[::stride, ::stride, ::stride].shape[:3] == n
    return grid


PALETTE = np.array([[16 * k + 9, 255 - 11 * k, 5 + 7 * k] for k in range(14)], np.uint8)   # 14 distinct colours, none black
OFF_LABEL = 14           # label of the voxels off the stride lattice: the lattice uses 1 .. 13


def label_grid(occ, stride=1, tail=(0, 0, 0)):
    """(A0, A1, A2) uint8 labels 1 + (7i + 3j + k) % 13 on the occupied lattice voxels: voxels one step apart on any axis, or five
    steps apart on axis 0 or 1 (the ring-boundary ties), never share a label; voxels off the lattice carry OFF_LABEL"""
    i, j, k = np.indices(occ.shape)
    lat = ((1 + (7 * i + 3 * j + k) % 13) * occ).astype(np.uint8)
    lab = np.full(full_shape(occ.shape, stride, tail), OFF_LABEL, np.uint8)
    lab[::stride, ::stride, ::stride] = lat
    return lab


def label_rgb(lab):
    """the RGB grid a label grid stands for (label 0 black, label k = PALETTE[k - 1])"""
    return np.concatenate([np.zeros((1, 3), np.uint8), PALETTE])[lab]


def voxel_of(colors):
    """the lattice index each colour of an index_grid mesh names"""
    c = np.rint(colors * 255.0).astype(np.int64) if colors.dtype == np.float64 else colors.astype(np.int64)
    return (c[:, 0] << 16) + (c[:, 1] << 8) + c[:, 2] - 1


# ---- the cube layout, restated ------------------------------------------------------------------------------------------------
def case_volume(mask):
    """cube cases as mesh_restate.marching_cubes_binary computes them: bit a0*4 + a1*2 + a2 = corner (c0+a0, c1+a1, c2+a2) occupied"""
    n0, n1, n2 = mask.shape
    m = mask.astype(np.int64)
    cases = np.zeros((n0 - 1, n1 - 1, n2 - 1), np.int64)
    for bit in range(8):
        a0, a1, a2 = (bit >> 2) & 1, (bit >> 1) & 1, bit & 1
        cases |= m[a0:a0 + n0 - 1, a1:a1 + n1 - 1, a2:a2 + n2 - 1] << bit
    return cases


def zbits_volume(shape):
    """per cube: bit a set where the cube's index on axis a is 0 (decides which of its edge vertices a cube owns)"""
    c0, c1, c2 = np.indices(shape)
    return (c0 == 0) | ((c1 == 0) << 1) | ((c2 == 0) << 2)


def case_zbits_pairs(mask):
    """the (case, zbits) pairs of the cubes that hold surface"""
    cases = case_volume(mask)
    z = zbits_volume(cases.shape)
    keep = (cases != 0) & (cases != 255)
    return set(zip(cases[keep].tolist(), z[keep].tolist()))


def cube_layout(mask):
    """per cube in scan order: (first owned vertex, owned vertices, first face, faces), from the restatement's table and ownership
    rule: the vertex and face numbering marching_cubes_binary produces"""
    cases = case_volume(mask)
    nv = np.zeros(cases.size, np.int64)
    nf = np.zeros(cases.size, np.int64)
    for t, c in enumerate(np.ndindex(cases.shape)):
        cs = int(cases[c])
        nf[t] = len(mr.TRIS[cs])
        nv[t] = sum(mr.owns(e, c) for e in mr.ORDER[cs]) if nf[t] else 0
    return np.cumsum(nv) - nv, nv, np.cumsum(nf) - nf, nf


def seam_references(mask, faces, block=256):
    """for every block seam: how many vertex references of the first cube of block b + 1 name a vertex of the last cube of block b"""
    vb, nv, fb, nf = cube_layout(mask)
    out = []
    for t in range(block, len(vb), block):
        f = faces[fb[t]:fb[t] + nf[t]]
        out.append(int(((f >= vb[t - 1]) & (f < vb[t - 1] + nv[t - 1])).sum()))
    return out


# ---- the nearest search, restated with its visiting order -------------------------------------------------------------------
def cell(q, n):
    return int(min(max(np.floor(q + 0.5), 0), n - 1))


def ring_of(mask, q, index):
    """Chebyshev ring of k_mesh_colors in which the row of lattice voxel `index` lies for query q"""
    i, j, _ = np.unravel_index(index, mask.shape)
    return max(abs(i - cell(q[0], mask.shape[0])), abs(j - cell(q[1], mask.shape[1])))


def visiting_order(mask, q):
    """the candidates of k_mesh_colors in the order it meets them, without its pruning: ring by ring around the query's clamped
    cell, rows in loop order (i ascending; all j on the two edge planes of the ring, the two end rows between), and in each row the
    largest occupied k <= floor(q2) before the smallest above it"""
    n0, n1, n2 = mask.shape
    ci, cj, kf = cell(q[0], n0), cell(q[1], n1), int(np.floor(q[2]))
    out = []
    for rho in range(max(n0, n1) + 1):
        for i in range(ci - rho, ci + rho + 1):
            if not 0 <= i < n0:
                continue
            js = range(cj - rho, cj + rho + 1) if abs(i - ci) == rho else (cj - rho, cj + rho)
            for j in js:
                if not 0 <= j < n1:
                    continue
                left, right = np.flatnonzero(mask[i, j, :kf + 1]), np.flatnonzero(mask[i, j, kf + 1:])
                if len(left):
                    out.append((i, j, int(left[-1])))
                if len(right):
                    out.append((i, j, kf + 1 + int(right[0])))
    return out


def nearest_by_rule(mask, queries, rule):
    """lattice index of the nearest occupied voxel of each query under a tie rule: "smallest" (the published one), "largest", or
    "first" (the first candidate of the kernel's visiting order, no index comparison)"""
    out = []
    for q in queries:
        cand = visiting_order(mask, q)
        p = np.array(cand, np.float64)
        d = ((q - p) ** 2).sum(-1)
        flat = np.ravel_multi_index(np.array(cand).T, mask.shape)
        tied = np.flatnonzero(d == d.min())
        out.append({"smallest": flat[tied].min(), "largest": flat[tied].max(), "first": flat[tied[0]]}[rule])
    return np.array(out, np.int64)


def colors_by_rule(grid, stride, verts, rule):
    """the colours meshify would return for those vertices under that tie rule"""
    g = grid[::stride, ::stride, ::stride]
    best = nearest_by_rule(np.any(g > 0, axis=-1), mr.queries(verts, stride), rule)
    cols = g.reshape(-1, g.shape[-1])[best]
    return cols / 255.0 if cols.max() > 1 else cols


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def voxels(shape, *points):
    occ = np.zeros(shape, bool)
    for p in points:
        occ[p] = True
    return occ


def de_bruijn(k, n):
    """the lexicographically least de Bruijn sequence B(k, n) (concatenated Lyndon words)"""
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
            return
        a[t] = a[t - p]
        db(t + 1, p)
        for j in range(a[t - p] + 1, k):
            a[t] = j
            db(t + 1, t)

    db(1, 1)
    return seq


def line_lattice(axis):
    """a lattice 2 x 2 x 257 (the long axis moved to `axis`) whose 2 x 2 slices follow B(16, 2) and its first symbol again: every
    ordered pair of slices, i.e. every cube case, occurs exactly once along the line; the first cube, the only one at index 0 of
    the long axis, is the empty case"""
    seq = de_bruijn(16, 2)
    seq = np.array(seq + seq[:1])
    assert len(seq) == 257 and seq[0] == seq[1] == 0
    occ = np.stack([np.stack([(seq >> (2 * a + b)) & 1 for b in (0, 1)]) for a in (0, 1)]).astype(bool)    # (2, 2, 257)
    return np.ascontiguousarray(np.moveaxis(occ, 2, axis))


def corner_lattices():
    """the 254 lattices 2 x 2 x 2 that hold surface: one cube, zbits 7"""
    return [np.array([(cs >> b) & 1 for b in range(8)], bool).reshape(2, 2, 2) for cs in range(1, 255)]


def random_lattices():
    """seeded lattices at density 0.5: zbits 0 from a 24^3 cube, zbits 1, 2 and 4 from three slabs one cube thick (a face of the
    cube has 484 cubes with one index at 0, too few to draw all 254 cases at random and about 160 come up; a 56 x 56 slab has
    3 025 and costs the restatement less than a larger cube would)"""
    rng = np.random.default_rng(2024)
    out = {"cube": rng.random((24, 24, 24)) < 0.5}
    for axis in range(3):
        shape = [56, 56, 56]
        shape[axis] = 2
        out[f"slab{axis}"] = rng.random(shape) < 0.5
    return out


@functools.lru_cache(maxsize=None)
def coverage_cases():
    """name -> (occupancy lattice, strides): the inputs whose union holds every (case, zbits) pair"""
    out = {f"corner{cs}": (occ, (1,)) for cs, occ in zip(range(1, 255), corner_lattices())}
    out.update({f"line{axis}": (line_lattice(axis), (1, 2)) for axis in range(3)})
    out.update({name: (occ, (1,)) for name, occ in random_lattices().items()})
    return out


@functools.lru_cache(maxsize=None)
def seam_lattices():
    """lattices with 255, 256, 257 cubes in one row, 256 and 258 cubes in two rows and in two planes: at 257 and 258 a second block
    exists, and slice 256 is mixed so that its first cube's faces use vertices the last cube of block 0 owns"""
    rng = np.random.default_rng(31)
    out = {}
    for shape in ((2, 2, 256), (2, 2, 257), (2, 2, 258), (2, 3, 129), (2, 3, 130), (3, 2, 130)):
        occ = rng.random(shape) < 0.5
        m2 = shape[2] - 1
        if (shape[0] - 1) * (shape[1] - 1) * m2 > 256:
            c0, r = divmod(256, (shape[1] - 1) * m2)
            c1, c2 = divmod(r, m2)
            assert c2 > 0
            occ[c0:c0 + 2, c1:c1 + 2, c2 - 1:c2 + 2] = np.array([[[0, 1, 0], [1, 0, 0]], [[1, 0, 1], [1, 1, 0]]], bool)
        out["x".join(map(str, shape))] = occ
    return out


WORD_SEAMS = {64: [(63, 0), (0, 63), (63, 63), (31, 32)],
              65: [(0, 64), (64, 0), (63, 64), (64, 63)],
              128: [(127, 0), (0, 127), (63, 64), (64, 63), (127, 64)],
              129: [(128, 0), (0, 128), (63, 128), (127, 128)],
              130: [(129, 0), (129, 1), (0, 129), (1, 129), (63, 129), (64, 0), (128, 63)]}


def word_seam_cases():
    """(n, 3, n) lattices with two voxels: (0, 1, ks), whose vertices mirror to queries at or just past plane n - 1, and (n - 1, 1, kw),
    the only voxel near them, |ks - kw| steps along the bit row.  (A query whose winner is 128 steps away has its own voxel at
    least that far off on axis 0, so it comes from plane 0 and lands half a step or a step past plane n - 1.)"""
    return {f"words{n}_{ks}_{kw}": voxels((n, 3, n), (0, 1, ks), (n - 1, 1, kw)) for n, pairs in WORD_SEAMS.items() for ks, kw in pairs}


LIMIT_TIES = {"limit_tie_right": ((27, 1, 62), (101, 1, 2), (100, 1, 122)), "limit_tie_left": ((27, 1, 70), (101, 1, 120), (100, 1, 20))}


def limit_tie_cases():
    """(128, 3, 128), voxels (source, ring 0, ring 1).  right: the vertex (27.5, 1, 62) mirrors to the query (100.5, 1, 62);
    (101, 1, 2) in ring 0 and (100, 1, 122) in ring 1 are both 60 steps off along k, and the second lies in the last word the
    right-hand scan may read once the first is known.  left: the query (100.5, 1, 70), (101, 1, 120) in ring 0 and (100, 1, 20)
    in ring 1, 50 steps off, in the last word of the left-hand scan.  Either way the ring-1 voxel ties and has the smaller index."""
    return {name: voxels((128, 3, 128), *pts) for name, pts in LIMIT_TIES.items()}


def ring_tie_cases():
    """axis 0: vertex (8.5, 1, 2) of voxel (8, 1, 2) mirrors to q0 = 3.5, cell 4; (6, 1, 2) lies in ring 2 and (1, 1, 2) in ring 3,
    both 2.5 away.  axis 1: vertex (2, 3.5, 5) of voxel (2, 3, 5) mirrors to (10, 3.5, 5), cell 4 on axis 1; (10, 6, 5) in ring 2
    and (10, 1, 5) in ring 3."""
    return {"ring_tie0": voxels((12, 3, 12), (8, 1, 2), (6, 1, 2), (1, 1, 2)),
            "ring_tie1": voxels((12, 8, 12), (2, 3, 5), (10, 6, 5), (10, 1, 5))}


def long_search_cases():
    """the only voxel near the mirrored queries lies 7 or 8 rings out: along axis 0 from outside the box, along axis 1, and along
    axis 0 from inside"""
    return {"long0_out": voxels((24, 3, 24), (0, 1, 12), (16, 1, 12)),
            "long1": voxels((24, 20, 24), (0, 10, 12), (23, 2, 12)),
            "long0_in": voxels((24, 3, 24), (4, 1, 12), (12, 1, 12))}


def outside_cases():
    """name -> (lattice, tail): stride 3.  below*: shape[0] > shape[2], the vertices of (13, 1, 4) mirror to q0 < 0; plane 0 holds
    (0, 1, 0) four steps off along k, plane 1 holds (1, 1, 4).  above*: shape[0] < shape[2], the vertices of (0, 1, 6) mirror
    to q0 > n0 - 1 = 3; plane 3 holds (3, 1, 0), plane 2 holds (2, 1, 6).  tail sets shape[2] % 3 to 1 or 2."""
    out = {}
    for r in (1, 2):
        out[f"below{r}"] = (voxels((14, 3, 8), (13, 1, 4), (0, 1, 0), (1, 1, 4)), (0, 0, r - 1))
        out[f"above{r}"] = (voxels((4, 3, 14), (0, 1, 6), (3, 1, 0), (2, 1, 6)), (0, 0, r - 1))
    return out


def mirror_tie_cases():
    """dense random lattices, square in axes 0 and 2: the mirrored edge midpoints fall half-way between lattice points"""
    rng = np.random.default_rng(5)
    return {"mirror_s1": (rng.random((7, 6, 7)) < 0.6, 1, (0, 0, 0)), "mirror_s2": (rng.random((6, 5, 6)) < 0.6, 2, (1, 0, 1))}


@functools.lru_cache(maxsize=None)
def tie_cases():
    """name -> (lattice, stride, tail): the constructed cases in which the tie rule decides colours"""
    out = dict(mirror_tie_cases())
    out.update({name: (occ, 1, (0, 0, 0)) for name, occ in ring_tie_cases().items()})
    out.update({name: (occ, 1, (0, 0, 0)) for name, occ in limit_tie_cases().items()})
    return out


@functools.lru_cache(maxsize=None)
def search_cases():
    """name -> (lattice, stride, tail): every constructed case of the nearest search"""
    out = {name: (occ, 1, (0, 0, 0)) for name, occ in word_seam_cases().items()}
    out.update(tie_cases())
    out.update({name: (occ, 1, (0, 0, 0)) for name, occ in long_search_cases().items()})
    out.update({name: (occ, 3, tail) for name, (occ, tail) in outside_cases().items()})
    return out


@functools.lru_cache(maxsize=None)
def reference(name, stride=None):
    """(grid, stride, restatement's (verts, faces, colours, normals)) of a named case, computed once"""
    if name in (cov := coverage_cases()):
        occ, strides = cov[name]
        s = stride or strides[0]
        grid = index_grid(occ, s, (s - 1,) * 3)
    elif name in (seams := seam_lattices()):
        grid, s = index_grid(seams[name]), 1
    else:
        occ, s, tail = search_cases()[name]
        grid = index_grid(occ, s, tail)
    return grid, s, mr.meshify(grid, s)


def winners(name):
    """per vertex of a named case: (query, winner's lattice index, tie set)"""
    grid, s, (v, _, _, _) = reference(name)
    mask = np.any(grid[::s, ::s, ::s] > 0, axis=-1)
    q = mr.queries(v, s)
    best, ties = mr.nearest_filled(mask, q)
    return mask, q, best, ties
