"""The rules of simplify_mesh and compact_mesh (include/pb3d.h: CLUSTERS, MAP, COLLAPSED, REPEATED, ORDER, VERTICES, FACES OUT,
ATTRIBUTES, EMPTY) restated in NumPy, a plain per-face Python loop that the restatement itself is held to, and the constructed meshes of
tests/test_simplify_mesh.py.

restate(): the clusters are downsample_restate.restate's voxels of the whole vertex list (voxel_size None: every vertex its own), the
faces are mapped with one fancy index, np.unique over the rotated rows names the first of every run of repeats, and a cumulative sum
renumbers the clusters that stay.  loop() walks the faces one by one with a set of the triples seen so far."""
import functools

import numpy as np

import downsample_restate as dr
import mesh_restate as mr
import meshify_cases as mc

PARTS = ("vertices", "faces", "colors", "index", "inverse", "face_index")


def _arrays(vertices, faces):
    V = np.asarray(vertices)
    V = np.ascontiguousarray(V, dtype=np.float32 if V.dtype == np.float32 else np.float64).reshape(-1, 3)
    F = np.asarray(faces)
    F = np.ascontiguousarray(F, dtype=np.int32 if F.dtype == np.int32 else np.int64).reshape(-1, 3)
    if F.size and (int(F.min()) < -len(V) or int(F.max()) >= len(V)):
        raise IndexError(f"index out of bounds for {len(V)} entries")
    return V, F


def _clusters(V, voxel_size, origin, reduce):
    """(rows, first, inv): one row per cluster, its first vertex, the cluster of every vertex"""
    if voxel_size is None:
        return V, np.arange(len(V), dtype=np.intp), np.arange(len(V), dtype=np.intp)
    rows, first, inv, _ = dr.restate(V, voxel_size, origin, reduce)
    return rows, first, inv


def _empty(V, F, colors):
    return (V[:0].copy(), F[:0].copy(), None if colors is None else np.asarray(colors)[:0].copy(), np.zeros(0, np.intp),
            np.full(len(V), -1, np.intp), np.zeros(0, np.intp))


def restate(vertices, faces, voxel_size=None, origin=None, reduce="centroid", duplicate_faces="drop", colors=None):
    """(vertices, faces, colors or None, index intp, inverse intp, face_index intp); voxel_size None = compact_mesh"""
    V, F = _arrays(vertices, faces)
    nv = len(V)
    if len(F) == 0:
        return _empty(V, F, colors)
    rows, first, inv = _clusters(V, voxel_size, origin, reduce)
    g = inv[np.where(F < 0, F + nv, F)]                                         # MAP
    alive = np.flatnonzero((g[:, 0] != g[:, 1]) & (g[:, 1] != g[:, 2]) & (g[:, 0] != g[:, 2]))     # COLLAPSED
    if duplicate_faces == "drop":                                               # REPEATED
        ga = g[alive]
        k = np.argmin(ga, axis=1)
        rot = np.stack([ga[np.arange(len(ga)), (k + a) % 3] for a in range(3)], axis=1)
        _, firsts = np.unique(rot, axis=0, return_index=True)                   # the first occurrence: the smallest position
        face_index = np.sort(alive[firsts]).astype(np.intp)
    else:
        assert duplicate_faces == "keep"
        face_index = alive.astype(np.intp)
    used = np.zeros(len(first), bool)                                           # VERTICES
    used[g[face_index].reshape(-1)] = True
    new = np.cumsum(used) - 1
    index = first[used].astype(np.intp)
    inverse = np.where(used[inv], new[inv], -1).astype(np.intp)
    out_faces = new[g[face_index]].astype(F.dtype).reshape(-1, 3)               # FACES OUT
    out_colors = None if colors is None else np.asarray(colors)[index].copy()   # ATTRIBUTES
    return rows[used].copy(), out_faces, out_colors, index, inverse, face_index


def loop(vertices, faces, voxel_size=None, origin=None, reduce="centroid", duplicate_faces="drop", colors=None):
    """the same result face by face"""
    V, F = _arrays(vertices, faces)
    nv = len(V)
    if len(F) == 0:
        return _empty(V, F, colors)
    rows, first, inv = _clusters(V, voxel_size, origin, reduce)
    inv = inv.tolist()
    seen, kept, named = set(), [], set()
    for j, corners in enumerate(F.tolist()):
        g = tuple(inv[w + nv if w < 0 else w] for w in corners)
        if g[0] == g[1] or g[1] == g[2] or g[0] == g[2]:
            continue
        if duplicate_faces == "drop":
            k = g.index(min(g))
            r = g[k:] + g[:k]
            if r in seen:
                continue
            seen.add(r)
        kept.append((j, g))
        named.update(g)
    number = {k: t for t, k in enumerate(sorted(named))}
    index = np.array([first[k] for k in sorted(named)], np.intp)
    inverse = np.array([number.get(k, -1) for k in inv], np.intp)
    out_faces = np.array([[number[k] for k in g] for _, g in kept], F.dtype).reshape(-1, 3)
    out_colors = None if colors is None else np.asarray(colors)[index].copy()
    return (rows[sorted(named)].reshape(-1, 3).copy(), out_faces, out_colors, index, inverse, np.array([j for j, _ in kept], np.intp))


def edge_balanced(faces):
    """every directed edge (a, b) of the faces occurs as often as (b, a)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if len(f) == 0:
        return True
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    n = int(f.max()) + 1
    fwd, nfwd = np.unique(a * n + b, return_counts=True)
    bwd, nbwd = np.unique(b * n + a, return_counts=True)
    return np.array_equal(fwd, bwd) and np.array_equal(nfwd, nbwd)


# ---- constructed meshes ------------------------------------------------------------------------------------------------------------------
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def folded_mesh():
    """a closed marching-cubes mesh with thin parts: 4570 float32 vertices, 10648 int32 faces, every directed edge balanced"""
    mask = np.zeros((16, 16, 16), bool)
    mask[1:15, 1:15, 1:15] = np.random.default_rng(3).random((14, 14, 14)) < 0.5
    v, f, _ = mr.marching_cubes_binary(mask)
    return _frozen(v, f)


@functools.lru_cache(maxsize=None)
def ball_mesh():
    """radius^2 < 81 about (11.5, 11.5, 11.5) in 24^3: 1536 vertices, 3068 faces"""
    i = np.indices((24, 24, 24)) - 11.5
    v, f, _ = mr.marching_cubes_binary((i * i).sum(axis=0) < 81)
    return _frozen(v, f)


REPEAT_SIZES = (2047, 2048, 2049, 4097)      # faces: the sort's tile is 2048 pairs
RESERVED = (61, 62, 63)                      # the three vertices of the hand-made faces; the other faces use 0 .. 60
MIRROR_AT, ROTATION_AT = 5, 1031


def repeats_mesh(nf):
    """64 vertices on a 4 x 4 x 4 lattice and nf faces: random triples of the vertices 0 .. 60 (repeats and mirror images among them by
    chance), and by hand (a, b, c) at position 0, its mirror image (a, c, b) at MIRROR_AT, its rotation (b, c, a) at ROTATION_AT and its
    rotation (c, a, b) at nf - 1"""
    rng = np.random.default_rng(nf)
    V = np.stack(np.meshgrid(*[np.arange(4.0)] * 3, indexing="ij"), -1).reshape(-1, 3)
    F = np.stack([rng.permutation(61)[:3] for _ in range(nf)]).astype(np.int32)
    a, b, c = RESERVED
    F[0], F[MIRROR_AT], F[ROTATION_AT], F[nf - 1] = (a, b, c), (a, c, b), (b, c, a), (c, a, b)
    return V, F


SHEET_SIDES = (15, 16, 40, 300)              # 225, 256, 1600 and 90000 clusters: one, two, two and three digit passes per key
SHEET_VOXEL = 0.75                           # below the spacing of 1: every vertex its own cluster


@functools.lru_cache(maxsize=None)
def sheet_mesh(side):
    """side x side vertices on a regular grid of spacing 1, two faces per square, and behind them a few hundred repeats, in another
    rotation, of faces from all over the list"""
    i, j = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    V = np.stack([i, j, np.zeros_like(i)], -1).reshape(-1, 3).astype(np.float32)
    q = (i[:-1, :-1] * side + j[:-1, :-1]).reshape(-1)
    F = np.concatenate([np.stack([q, q + side, q + 1], 1), np.stack([q + 1, q + side, q + side + 1], 1)]).astype(np.int32)
    rng = np.random.default_rng(side)
    src = rng.choice(len(F), min(300, len(F)), replace=False)
    again = np.roll(F[src], 1, axis=1)
    again[::7] = F[src[::7]][:, [0, 2, 1]]                                     # ... and some mirror images, which are no repeats
    return _frozen(V, np.concatenate([F, again]))


def with_unreferenced(V, F, seed=9):
    """the mesh with one extra vertex after every third one: half of them near a vertex of the mesh (they join its cluster and its
    centroid), half far outside (clusters of their own that no face names)"""
    rng = np.random.default_rng(seed)
    nv = len(V)
    extra = np.arange(0, nv, 3)
    pos = V[rng.integers(0, nv, len(extra))] + rng.random((len(extra), 3)).astype(V.dtype) * 0.25
    far = rng.random(len(extra)) < 0.5
    pos[far] += 1000.0
    place = np.arange(nv) + np.searchsorted(extra, np.arange(nv), side="left")     # where each old vertex goes
    out = np.empty((nv + len(extra), 3), V.dtype)
    out[place] = V
    out[np.setdiff1d(np.arange(len(out)), place)] = pos
    return out, place[F].astype(F.dtype)


@functools.lru_cache(maxsize=None)
def colored_mesh():
    """a random 10^3 occupancy as meshify_cases.index_grid colours it, meshed as meshify does: (vertices float32 in meshify's frame,
    faces int32, (n, 3) uint8 colours that name the lattice voxel nearest to each vertex)"""
    occ = np.zeros((10, 10, 10), bool)
    occ[1:9, 1:9, 1:9] = np.random.default_rng(17).random((8, 8, 8)) < 0.55
    grid = mc.index_grid(occ)
    v, f, _ = mr.marching_cubes_binary(occ)
    verts = v[:, [2, 1, 0]].copy()
    verts[:, 2] = grid.shape[2] - verts[:, 2]
    best, _ = mr.nearest_filled(occ, mr.queries(verts, 1))
    return _frozen(np.ascontiguousarray(verts), f, np.ascontiguousarray(grid.reshape(-1, 3)[best]))
