"""NumPy restatement of mesh_vertex_adjacency and smooth_mesh (include/pb3d.h "mesh smoothing") for tests/test_mesh_smooth.py and
tools/opbench.py, a plain Python loop that the restatement is held to, and the constructed meshes of the tests.

np.add.at(s, src, x[nbr]) over the (i, j)-sorted pairs performs s[i] = s[i] + x[j] one pair after the other, unbuffered: exactly the
stated order of the additions, which np.add.reduceat (pairwise inside a run) would not give."""
import numpy as np


def wrapped(faces, nv):
    """int64 (nf, 3) faces with NumPy's negative indices resolved; IndexError outside [-nv, nv)"""
    f = np.asarray(faces)
    if f.dtype.kind not in "iu":
        raise IndexError("arrays used as indices must be of integer (or boolean) type")
    f = f.astype(np.int64).reshape(-1, 3)
    if f.size and (int(f.min()) < -nv or int(f.max()) >= nv):
        raise IndexError(f"face index out of bounds for {nv} vertices")
    return np.where(f < 0, f + nv, f)


def pairs(faces, nv):
    """the directed pairs of PAIRS, in emission order: (sources, targets)"""
    f = wrapped(faces, nv)
    a, b, c = f[:, 0], f[:, 1], f[:, 2]
    src = np.stack([a, b, b, c, c, a], axis=1).reshape(-1)
    dst = np.stack([b, a, c, b, a, c], axis=1).reshape(-1)
    keep = src != dst
    return src[keep], dst[keep]


def adjacency(faces, nv):
    """(starts int64 nv + 1, neighbours int32, multiplicity int64, boundary bool nv)"""
    src, dst = pairs(faces, nv)
    if len(src) == 0:
        return np.zeros(nv + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(nv, bool)
    keys, mult = np.unique(src * nv + dst, return_counts=True)
    i, j = keys // nv, keys % nv
    starts = np.concatenate([[0], np.cumsum(np.bincount(i, minlength=nv))]).astype(np.int64)
    boundary = np.zeros(nv, bool)
    boundary[i[mult == 1]] = True
    boundary[j[mult == 1]] = True
    return starts, j.astype(np.int32), mult.astype(np.int64), boundary


def sources(starts):
    """the first end of every unique pair, from the list starts"""
    return np.repeat(np.arange(len(starts) - 1, dtype=np.int64), np.diff(starts))


def step(x, starts, nbr, src, fixed, f):
    """STEP with factor f on float64 positions x (nv, 3); fixed: bool nv"""
    s = np.zeros_like(x)
    with np.errstate(all="ignore"):
        np.add.at(s, src, x[nbr])
        deg = np.diff(starts)
        move = (deg > 0) & ~fixed
        m = s[move] / deg[move].astype(np.float64)[:, None]
        d = m - x[move]
        out = x.copy()
        out[move] = x[move] + f * d
    return out


def as_vertices(vertices):
    v = np.asarray(vertices)
    return np.ascontiguousarray(v) if v.dtype == np.float32 else np.ascontiguousarray(v, dtype=np.float64)


def factors(method, lamb, mu):
    return (lamb, mu) if method == "taubin" else (lamb,)


def restate(vertices, faces, iterations=10, method="taubin", lamb=0.5, mu=-0.53, fixed=None, fix_boundary=False):
    v = as_vertices(vertices)
    nv = len(v)
    starts, nbr, mult, boundary = adjacency(faces, nv)
    if iterations == 0:
        return v.copy()
    fx = np.zeros(nv, bool) if fixed is None else np.asarray(fixed) != 0
    if fix_boundary:
        fx = fx | boundary
    src = sources(starts)
    x = v.astype(np.float64)
    for _ in range(iterations):
        for f in factors(method, lamb, mu):
            x = step(x, starts, nbr, src, fx, f)
    with np.errstate(all="ignore"):
        return x.astype(v.dtype)


def loop_adjacency(faces, nv):
    """the same four arrays from a plain loop over the faces"""
    count = {}
    for face in np.asarray(faces).reshape(-1, 3).tolist():
        for k in face:
            if not -nv <= k < nv:
                raise IndexError(f"face index out of bounds for {nv} vertices")
        a, b, c = (k + nv if k < 0 else k for k in face)
        for i, j in ((a, b), (b, a), (b, c), (c, b), (c, a), (a, c)):
            if i != j:
                count[(i, j)] = count.get((i, j), 0) + 1
    lists = [[] for _ in range(nv)]
    for i, j in sorted(count):
        lists[i].append(j)
    starts = np.zeros(nv + 1, np.int64)
    for i in range(nv):
        starts[i + 1] = starts[i] + len(lists[i])
    boundary = np.zeros(nv, bool)
    for (i, j), c in count.items():
        if c == 1:
            boundary[i] = boundary[j] = True
    return (starts, np.array([j for l in lists for j in l], np.int32).reshape(-1), np.array([count[k] for k in sorted(count)], np.int64).reshape(-1),
            boundary)


def loop(vertices, faces, iterations=10, method="taubin", lamb=0.5, mu=-0.53, fixed=None, fix_boundary=False):
    """the rules as a plain Python double loop over Python floats (IEEE float64, one rounded operation per operator)"""
    v = as_vertices(vertices)
    nv = len(v)
    starts, nbr, mult, boundary = loop_adjacency(faces, nv)
    if iterations == 0:
        return v.copy()
    starts, nbr = starts.tolist(), nbr.tolist()
    fx = [bool(fixed is not None and fixed[i]) or bool(fix_boundary and boundary[i]) for i in range(nv)]
    x = [[float(c) for c in row] for row in v.tolist()]
    for _ in range(iterations):
        for f in factors(method, lamb, mu):
            new = []
            for i in range(nv):
                lo, hi = starts[i], starts[i + 1]
                if fx[i] or hi == lo:
                    new.append(x[i])
                    continue
                row = []
                for a in range(3):
                    s = 0.0
                    for p in range(lo, hi):
                        s = s + x[nbr[p]][a]
                    m = s / float(hi - lo)
                    d = m - x[i][a]
                    row.append(x[i][a] + f * d)
                new.append(row)
            x = new
    with np.errstate(all="ignore"):
        return np.array(x, np.float64).reshape(nv, 3).astype(v.dtype)


# ---- properties ---------------------------------------------------------------------------------------------------------------------------
def mean_dihedral_deg(vertices, faces):
    """mean angle, in degrees, between the normals of the two faces of every edge that exactly two faces share"""
    v = np.asarray(vertices, np.float64)
    f = wrapped(faces, len(v))
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    n /= np.linalg.norm(n, axis=1)[:, None]
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    face = np.tile(np.arange(len(f)), 3)
    key = e[:, 0] * len(v) + e[:, 1]
    order = np.argsort(key, kind="stable")
    key, face = key[order], face[order]
    uniq, first, cnt = np.unique(key, return_index=True, return_counts=True)
    first = first[cnt == 2]
    cos = np.clip((n[face[first]] * n[face[first + 1]]).sum(axis=1), -1.0, 1.0)
    return float(np.degrees(np.arccos(cos)).mean())


def extent(vertices):
    v = np.asarray(vertices, np.float64)
    return float((v.max(axis=0) - v.min(axis=0)).sum())


# ---- constructed meshes: name -> (vertices float64 (nv, 3), faces int64 (nf, 3)) ------------------------------------------------------------
LANE_DEGREE = 32        # csrc/smooth.hip: above it a vertex is summed by a wavefront, 64 neighbours a time


def fan(rim, hub_last=False):
    """`rim` faces around a hub (degree rim + 1): hub 0 and the rim 1 .. rim + 1, or the hub as the last vertex"""
    k = np.arange(rim, dtype=np.int64)
    if hub_last:
        return np.stack([np.full(rim, rim + 1), k, k + 1], axis=1)
    return np.stack([np.zeros(rim, np.int64), k + 1, k + 2], axis=1)


def strip(nf):
    k = np.arange(nf, dtype=np.int64)
    return np.stack([k, k + 1, k + 2], axis=1)


def grid_faces(rows, cols):
    r, c = np.meshgrid(np.arange(rows - 1), np.arange(cols - 1), indexing="ij")
    a = (r * cols + c).reshape(-1).astype(np.int64)
    return np.concatenate([np.stack([a, a + 1, a + cols], axis=1), np.stack([a + 1, a + cols + 1, a + cols], axis=1)])


def constructed_cases():
    rng = np.random.default_rng(20240611)
    cases = {}

    def add(name, nv, faces):
        cases[name] = (np.ascontiguousarray(rng.normal(size=(nv, 3)) * 10.0), np.asarray(faces, np.int64).reshape(-1, 3))

    add("small/triangle", 3, [[0, 1, 2]])
    add("small/two_triangles", 4, [[0, 1, 2], [2, 1, 3]])
    add("small/tetrahedron", 4, [[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]])
    add("small/no_faces", 5, np.zeros((0, 3), np.int64))
    add("small/one_vertex", 1, [[0, 0, 0]])
    add("fan/hub_first", 4098, fan(4096))
    add("fan/hub_last", 4098, fan(4096, hub_last=True))
    for deg in (LANE_DEGREE, LANE_DEGREE + 1, 64, 65, 128, 129):        # either side of the lane cutoff and of one and two 64-gathers
        add(f"fan/degree_{deg}", deg + 1, fan(deg - 1))
    # 6 nf is never 2048 k: the pair counts that are multiples of 6 nearest to 2048 k - 6, 2048 k and 2048 k + 6, for k = 1, 2
    for nf in (340, 341, 342, 343, 681, 682, 683, 684):
        add(f"seam/{6 * nf}", nf + 2, strip(nf))
    for rows, cols in ((10, 20), (15, 20), (250, 280)):                 # nv = 200, 300, 70 000: one, two and three radix passes
        add(f"radix/{rows * cols}", rows * cols, grid_faces(rows, cols))
    add("awkward/duplicated", 4, [[0, 1, 2], [2, 1, 3], [0, 1, 2], [2, 1, 3]])
    add("awkward/degenerate", 6, [[0, 1, 2], [3, 3, 4], [4, 5, 4], [5, 5, 5], [2, 1, 3], [1, 2, 2]])
    add("awkward/all_degenerate", 4, [[0, 0, 0], [1, 1, 1], [3, 3, 3]])
    add("awkward/isolated", 12, [[2, 3, 5], [5, 3, 8], [8, 9, 5]])
    add("awkward/negative", 5, [[0, 1, -1], [-1, 1, -3], [-5, -4, 3], [4, 2, 3]])
    for v, f in cases.values():
        v.setflags(write=False)
        f.setflags(write=False)
    return cases
