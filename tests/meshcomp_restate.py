"""The rules of mesh_components (include/pb3d.h: RECORDS, EDGES, CONNECT, NUMBERS, COUNTS, MEASURES, TOTALS) restated in NumPy / SciPy, a
plain per-face Python union-find loop that the restatement itself is held to, the composition that keep_mesh_components is, and the
constructed meshes of tests/test_mesh_components.py.

restate(): np.lexsort puts the records in (lo, hi) order, scipy.sparse.csgraph.connected_components finds the components, which are
renumbered by their first face, and every block sum and every total is np.cumsum(...)[-1] behind a leading 0.0 -- cumsum adds one
element after the other, which is the order the header fixes.  loop() walks the faces one by one with dictionaries and Python floats."""
import functools
import math

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

import mesh_restate as mr
import simplify_restate as sr

COUNTS = ("faces", "edges", "boundary_edges", "nonmanifold_edges", "unbalanced_edges")
TOTALS = ("components", "vertices", "edges", "faces", "boundary_edges", "nonmanifold_edges", "unbalanced_edges", "loops")
BLOCK = 256


def _wrapped(faces, n):
    F = np.asarray(faces)
    F = np.ascontiguousarray(F, dtype=np.int32 if F.dtype == np.int32 else np.int64).reshape(-1, 3)
    if F.size and (int(F.min()) < -n or int(F.max()) >= n):
        raise IndexError(f"index out of bounds for {n} entries")
    return np.where(F < 0, F + n, F).astype(np.int64)


def _widened(vertices):
    V = np.asarray(vertices)
    return np.ascontiguousarray(V, dtype=np.float64).reshape(-1, 3)         # float32 widens exactly


def _first_face_numbers(comp_of_face):
    """the components renumbered by their smallest face position"""
    ids, first = np.unique(comp_of_face, return_index=True)
    number = np.empty(int(ids.max()) + 1 if len(ids) else 0, np.int64)
    number[ids[np.argsort(first, kind="stable")]] = np.arange(len(ids))
    return number[comp_of_face]


def _ordered_sum(x):
    return np.cumsum(np.concatenate(([0.0], x)))[-1]


def face_measures(V, W):
    """(A_j, S_j) of every face, one rounded float64 operation a step"""
    a, b, c = V[W[:, 0]], V[W[:, 1]], V[W[:, 2]]
    e1, e2 = b - a, c - a

    def cross(p, q):
        return (p[:, 1] * q[:, 2] - p[:, 2] * q[:, 1], p[:, 2] * q[:, 0] - p[:, 0] * q[:, 2], p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0])

    nx, ny, nz = cross(e1, e2)
    A = 0.5 * np.sqrt((nx * nx + ny * ny) + nz * nz)
    mx, my, mz = cross(b, c)
    S = (a[:, 0] * mx + a[:, 1] * my) + a[:, 2] * mz
    return A, S


def restate(faces, n, vertices=None, connectivity="edge"):
    """dict(face_labels int32, vertex_labels int32, stats {name: array}, totals {name: int})"""
    W = _wrapped(faces, n)
    m = len(W)
    stats = {name: np.zeros(0, np.int64) for name in COUNTS}
    if vertices is not None:
        stats.update(area=np.zeros(0), volume=np.zeros(0))
    if m == 0:
        return dict(face_labels=np.zeros(0, np.int32), vertex_labels=np.full(n, -1, np.int32), stats=stats, totals=dict.fromkeys(TOTALS, 0))
    src, dst = W.reshape(-1), W[:, [1, 2, 0]].reshape(-1)                      # record 3j + a
    lo, hi = np.minimum(src, dst), np.maximum(src, dst)
    rec = np.flatnonzero(src != dst)
    rec = rec[np.lexsort((hi[rec], lo[rec]))]                                  # (lo, hi) order, stable: ascending record within an edge
    head = np.ones(len(rec), bool)
    head[1:] = (lo[rec][1:] != lo[rec][:-1]) | (hi[rec][1:] != hi[rec][:-1])
    edge = np.cumsum(head) - 1
    E = int(head.sum())
    c = np.bincount(edge, minlength=E).astype(np.int64)
    f = np.bincount(edge, weights=(src[rec] == lo[rec]), minlength=E).astype(np.int64)
    if connectivity == "edge":
        later = np.flatnonzero(~head)
        g = coo_matrix((np.ones(len(later)), (rec[later] // 3, rec[later - 1] // 3)), shape=(m, m))
        comp = connected_components(g, directed=False)[1]
    else:
        assert connectivity == "vertex"
        g = coo_matrix((np.ones(2 * m), (np.concatenate([W[:, 0], W[:, 1]]), np.concatenate([W[:, 1], W[:, 2]]))), shape=(n, n))
        comp = connected_components(g, directed=False)[1][W[:, 0]]
    labels = _first_face_numbers(comp)
    nc = int(labels.max()) + 1
    vertex_labels = np.full(n, np.iinfo(np.int64).max)
    np.minimum.at(vertex_labels, W.reshape(-1), np.repeat(labels, 3))
    vertex_labels[vertex_labels == np.iinfo(np.int64).max] = -1
    edge_label = labels[rec[head] // 3]
    boundary, nonmanifold, unbalanced = c == 1, c > 2, 2 * f != c
    stats.update(faces=np.bincount(labels, minlength=nc).astype(np.int64), edges=np.bincount(edge_label, minlength=nc).astype(np.int64),
                 boundary_edges=np.bincount(edge_label[boundary], minlength=nc).astype(np.int64),
                 nonmanifold_edges=np.bincount(edge_label[nonmanifold], minlength=nc).astype(np.int64),
                 unbalanced_edges=np.bincount(edge_label[unbalanced], minlength=nc).astype(np.int64))
    if vertices is not None:
        A, S = face_measures(_widened(vertices), W)
        order = np.argsort(labels, kind="stable")
        starts = np.concatenate(([0], np.cumsum(stats["faces"])))
        area, volume = np.zeros(nc), np.zeros(nc)
        for l in range(nc):
            mine = order[starts[l]:starts[l + 1]]
            area[l] = _ordered_sum(np.array([_ordered_sum(A[mine[s:s + BLOCK]]) for s in range(0, len(mine), BLOCK)]))
            volume[l] = _ordered_sum(np.array([_ordered_sum(S[mine[s:s + BLOCK]]) for s in range(0, len(mine), BLOCK)])) / 6.0
        stats.update(area=area, volume=volume)
    totals = dict(components=nc, vertices=int((vertex_labels >= 0).sum()), edges=E, faces=m, boundary_edges=int(boundary.sum()),
                  nonmanifold_edges=int(nonmanifold.sum()), unbalanced_edges=int(unbalanced.sum()), loops=int((src == dst).sum()))
    return dict(face_labels=labels.astype(np.int32), vertex_labels=vertex_labels.astype(np.int32), stats=stats, totals=totals)


def loop(faces, n, vertices=None, connectivity="edge"):
    """the same result face by face"""
    W = _wrapped(faces, n).tolist()
    m = len(W)
    if m == 0:
        return restate(faces, n, vertices, connectivity)
    parent = list(range(m))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    def union(x, y):
        x, y = find(x), find(y)
        if x != y:
            parent[max(x, y)] = min(x, y)

    edges, seen_vertex, loops = {}, {}, 0
    for j, w in enumerate(W):
        for a in range(3):
            s, d = w[a], w[(a + 1) % 3]
            if s == d:
                loops += 1
                continue
            e = edges.setdefault((min(s, d), max(s, d)), [0, 0, j])
            e[0] += 1
            e[1] += s < d
            if connectivity == "edge":
                union(j, e[2])
        if connectivity == "vertex":
            for v in w:
                union(j, seen_vertex.setdefault(v, j))
    roots = [find(j) for j in range(m)]
    number = {r: k for k, r in enumerate(sorted(set(roots)))}               # a root is its component's smallest face
    labels = [number[r] for r in roots]
    nc = len(number)
    vertex_labels = [-1] * n
    for j, w in enumerate(W):
        for v in w:
            vertex_labels[v] = labels[j] if vertex_labels[v] < 0 else min(vertex_labels[v], labels[j])
    stats = {name: np.zeros(nc, np.int64) for name in COUNTS}
    totals = dict.fromkeys(TOTALS, 0)
    for j in range(m):
        stats["faces"][labels[j]] += 1
    for (c, f, j) in edges.values():
        for name, flag in (("edges", True), ("boundary_edges", c == 1), ("nonmanifold_edges", c > 2), ("unbalanced_edges", 2 * f != c)):
            stats[name][labels[j]] += flag
            totals[name] += flag
    if vertices is not None:
        V = _widened(vertices).tolist()
        mine = [[] for _ in range(nc)]
        for j, (i0, i1, i2) in enumerate(W):
            a, b, c = V[i0], V[i1], V[i2]
            e1, e2 = [b[t] - a[t] for t in range(3)], [c[t] - a[t] for t in range(3)]
            nx, ny, nz = e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]
            mx, my, mz = b[1] * c[2] - b[2] * c[1], b[2] * c[0] - b[0] * c[2], b[0] * c[1] - b[1] * c[0]
            mine[labels[j]].append((0.5 * math.sqrt((nx * nx + ny * ny) + nz * nz), (a[0] * mx + a[1] * my) + a[2] * mz))
        area, volume = np.zeros(nc), np.zeros(nc)
        for l, rows in enumerate(mine):
            ta = ts = 0.0
            for s in range(0, len(rows), BLOCK):
                ba = bs = 0.0
                for A, S in rows[s:s + BLOCK]:
                    ba, bs = ba + A, bs + S
                ta, ts = ta + ba, ts + bs
            area[l], volume[l] = ta, ts / 6.0
        stats.update(area=area, volume=volume)
    totals.update(components=nc, vertices=sum(v >= 0 for v in vertex_labels), faces=m, loops=loops)
    return dict(face_labels=np.array(labels, np.int32), vertex_labels=np.array(vertex_labels, np.int32), stats=stats, totals=totals)


def choose(stats, k=None, min_faces=None, min_area=None, closed_only=False, rank_by="faces"):
    """keep_mesh_components' choice: thresholds, then the k largest by rank_by (volume by absolute value), ties to the lower number"""
    ok = np.ones(len(stats["faces"]), bool)
    if min_faces is not None:
        ok &= stats["faces"] >= min_faces
    if min_area is not None:
        ok &= stats["area"] >= min_area
    if closed_only:
        ok &= stats["unbalanced_edges"] == 0
    cand = [int(l) for l in np.flatnonzero(ok)]
    if k is not None:
        cand = sorted(sorted(cand, key=lambda l: (-abs(float(stats[rank_by][l])), l))[:k])
    return np.array(cand, np.intp)


def select(vertices, faces, keep, colors=None):
    """select_faces in NumPy: (vertices, faces, colors or None, index, inverse, face_index)"""
    V, F = sr._arrays(vertices, faces)
    keep = np.asarray(keep) != 0
    face_index = np.flatnonzero(keep).astype(np.intp)
    if len(face_index) == 0:
        return sr._empty(V, F, colors)
    g = np.where(F < 0, F + len(V), F)[face_index]
    used = np.zeros(len(V), bool)
    used[g.reshape(-1)] = True
    new = np.cumsum(used) - 1
    index = np.flatnonzero(used).astype(np.intp)
    return (V[used].copy(), new[g].astype(F.dtype).reshape(-1, 3), None if colors is None else np.asarray(colors)[index].copy(), index,
            np.where(used, new, -1).astype(np.intp), face_index)


def keep_components(vertices, faces, colors=None, connectivity="edge", **how):
    """keep_mesh_components composed of the restatements: (vertices, faces, colors or None, face_labels, chosen)"""
    V, F = sr._arrays(vertices, faces)
    r = restate(F, len(V), V, connectivity)
    chosen = choose(r["stats"], **how)
    out = select(V, F, np.isin(r["face_labels"], chosen), colors)
    return out[0], out[1], out[2], r["face_labels"], chosen


# ---- constructed meshes ------------------------------------------------------------------------------------------------------------------
TET = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int32)         # closed, every directed edge has its reverse
TET_VERTS = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], np.float32)


def _irrational(n, seed=0.0):
    """n float32 offsets below 0.1 that no short binary fraction holds"""
    i = np.arange(n, dtype=np.float64)
    return np.stack([0.07 * np.sin(1.3 * i + seed), 0.05 * np.cos(1.7 * i + seed), 0.09 * np.sin(0.37 * i + 2.0 + seed)], 1)


def tets_sharing_vertex():
    """two tetrahedra with one common vertex: one component by vertex, two by edge"""
    V = np.concatenate([TET_VERTS, TET_VERTS[3] + np.array([[1.5, 0.2, 0.1], [0.3, 1.25, 0.2], [0.1, 0.4, 1.75]], np.float32)]).astype(np.float32)
    return V, np.concatenate([TET, TET + 3]).astype(np.int32)              # vertex 3 is the second one's corner 0


def tets_sharing_edge():
    """two tetrahedra on either side of the edge (0, 1): one component and one non-manifold edge under both rules"""
    V = np.concatenate([TET_VERTS, [[0.25, -1.0, 0.0], [0.25, 0.0, -1.5]]]).astype(np.float32)
    B = np.array([0, 1, 4, 5], np.int32)[TET]
    return V, np.concatenate([TET, B]).astype(np.int32)


def tet_with_flipped_face():
    F = TET.copy()
    F[2] = F[2][::-1]
    return TET_VERTS.copy(), F


def open_triangle():
    return TET_VERTS[:3].copy(), np.array([[0, 1, 2]], np.int32)


def loop_faces():
    """(a, a, b): one loop and a balanced edge; (a, a, a): three loops, a component of its own by edge"""
    return TET_VERTS.copy(), np.array([[0, 0, 1], [2, 2, 2], [0, 0, 0]], np.int32)


@functools.lru_cache(maxsize=None)
def strip(m):
    """a 1 x m triangle strip, consistently oriented: one chain of m faces over m + 2 float32 vertices with irrational-looking
    coordinates"""
    i = np.arange(m + 2)
    V = (np.stack([(i // 2) * math.sqrt(2.0), (i % 2) * (math.pi / 3.0), np.zeros(m + 2)], 1) + _irrational(m + 2)).astype(np.float32)
    k = np.arange(m)
    F = np.where((k % 2 == 0)[:, None], np.stack([k, k + 1, k + 2], 1), np.stack([k + 1, k, k + 2], 1)).astype(np.int32)
    return sr._frozen(V, F)


@functools.lru_cache(maxsize=None)
def book(m=4097):
    """m faces (0, 1, k) round one edge, every other one reversed: a run of m records that crosses the sort's tiles"""
    k = np.arange(2, m + 2)
    F = np.stack([np.zeros(m, np.int64), np.ones(m, np.int64), k], 1)
    F[1::2] = F[1::2][:, [1, 0, 2]]
    ang = k * 0.001
    V = np.concatenate([[[0.0, 0.0, 0.0], [0.0, 0.0, 1.0]], np.stack([np.cos(ang), np.sin(ang), 0.5 + 0 * ang], 1)]) + _irrational(m + 2, 1.0)
    return sr._frozen(V.astype(np.float32), F.astype(np.int32))


@functools.lru_cache(maxsize=None)
def disjoint_triangles(m=5000):
    F = np.arange(3 * m, dtype=np.int32).reshape(m, 3)
    V = (np.repeat(np.arange(m), 3)[:, None] * np.array([[2.0, 0.0, 0.0]]) + np.tile(TET_VERTS[:3], (m, 1)) + _irrational(3 * m, 2.0))
    return sr._frozen(V.astype(np.float32), F)


@functools.lru_cache(maxsize=None)
def fragments_mesh():
    """folded_mesh()'s construction with default_rng(7) at density 0.2: 2608 vertices, 5352 faces, 43 components"""
    mask = np.zeros((16, 16, 16), bool)
    mask[1:15, 1:15, 1:15] = np.random.default_rng(7).random((14, 14, 14)) < 0.2
    v, f, _ = mr.marching_cubes_binary(mask)
    return sr._frozen(v, f)


def ranked_tets():
    """three closed tetrahedra whose order by faces (a tie: the first), by area and by |volume| differ, the last one inside out: B is
    flat and wide (largest area), C is compact (largest volume, negative)"""
    A = TET_VERTS * 1.0
    B = TET_VERTS * np.array([4.0, 4.0, 0.05], np.float32) + np.float32(10.0)
    C = TET_VERTS * np.float32(2.5) + np.float32(20.0)
    V = (np.concatenate([A, B, C]) + _irrational(12, 3.0)).astype(np.float32)
    F = np.concatenate([TET, TET + 4, (TET + 8)[:, ::-1]]).astype(np.int32)
    return V, F
