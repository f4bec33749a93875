"""The rules of mesh_orient (include/pb3d.h: PAIR EDGES, PATCHES, ANCHOR, SIGN, FACES OUT, COUNTS, TOTALS) restated in NumPy / SciPy, a
plain breadth-first propagation that the restatement itself is held to, and the constructed meshes of tests/test_mesh_orient.py.

restate(): the records in (lo, hi) order as tests/meshcomp_restate.py puts them; the doubled graph -- node j is face j as it came, node
m + j face j flipped -- through scipy.sparse.csgraph.connected_components; the smallest member of every set by np.minimum.at; every
block sum and every total np.cumsum(...)[-1] behind a leading 0.0.  loop() builds a dictionary of edges, walks every patch breadth
first from its smallest face carrying the flip bit across pair edges, and calls the patch not orientable at the first conflict."""
import collections
import functools

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

import meshcomp_restate as mc
import simplify_restate as sr

COUNTS = ("faces", "pair_edges", "disagreeing_edges", "boundary_edges", "nonmanifold_records", "flipped_faces")
TOTALS = ("patches", "orientable_patches", "pair_edges", "disagreeing_edges", "flipped_faces", "inverted_patches", "boundary_edges",
          "nonmanifold_edges")
BLOCK = 256


def _empty(faces, measured):
    stats = {name: np.zeros(0, np.int64) for name in COUNTS}
    stats.update(orientable=np.zeros(0, bool), inverted=np.zeros(0, bool))
    if measured:
        stats["volume"] = np.zeros(0)
    return dict(flip=np.zeros(0, np.uint8), patch=np.zeros(0, np.int32), faces=np.array(faces, copy=True).reshape(-1, 3), stats=stats,
                totals=dict.fromkeys(TOTALS, 0))


def _wrong(V, volume_sign):
    return V < 0.0 if volume_sign == "positive" else V > 0.0


def _swapped(faces, flip):
    out = np.array(faces, copy=True).reshape(-1, 3)
    k = np.flatnonzero(flip)
    out[k] = out[k][:, [0, 2, 1]]
    return out


def restate(faces, n, vertices=None, volume_sign=None):
    """dict(flip uint8, patch int32, faces (the output rows, input dtype), stats {name: array}, totals {name: int})"""
    assert volume_sign in (None, "positive", "negative") and (volume_sign is None or vertices is not None)
    W = mc._wrapped(faces, n)
    m = len(W)
    if m == 0:
        return _empty(faces, vertices is not None)
    src, dst = W.reshape(-1), W[:, [1, 2, 0]].reshape(-1)                      # record 3j + a
    lo, hi = np.minimum(src, dst), np.maximum(src, dst)
    rec = np.flatnonzero(src != dst)
    rec = rec[np.lexsort((hi[rec], lo[rec]))]
    head = np.ones(len(rec), bool)
    head[1:] = (lo[rec][1:] != lo[rec][:-1]) | (hi[rec][1:] != hi[rec][:-1])
    start = np.flatnonzero(head)
    E = len(start)
    edge = np.cumsum(head) - 1
    c = np.bincount(edge, minlength=E).astype(np.int64)
    fwd = src[rec] == lo[rec]
    f = np.bincount(edge, weights=fwd, minlength=E).astype(np.int64)
    p = start[c == 2]
    a, b, d = rec[p] // 3, rec[p + 1] // 3, (f[c == 2] != 1).astype(np.int64)
    g = coo_matrix((np.ones(2 * len(p)), (np.concatenate([a, a + m]), np.concatenate([b + d * m, b + (1 - d) * m]))), shape=(2 * m, 2 * m))
    nsets, set_of = connected_components(g, directed=False)
    smallest = np.full(nsets, 2 * m)
    np.minimum.at(smallest, set_of, np.arange(2 * m))
    r0, r1 = smallest[set_of[:m]], smallest[set_of[m:]]
    ids, patch = np.unique(np.minimum(r0, r1), return_inverse=True)            # ascending anchors: numbered by smallest face
    P = len(ids)
    orientable = np.ones(P, bool)
    orientable[patch[r0 == r1]] = False
    flip = r0 > r1
    face_of_edge = patch[rec[start] // 3]
    stats = dict(faces=np.bincount(patch, minlength=P), pair_edges=np.bincount(face_of_edge[c == 2], minlength=P),
                 disagreeing_edges=np.bincount(face_of_edge[(c == 2) & (f != 1)], minlength=P),
                 boundary_edges=np.bincount(face_of_edge[c == 1], minlength=P),
                 nonmanifold_records=np.bincount(patch[rec[(c > 2)[edge]] // 3], minlength=P))
    stats = {k: v.astype(np.int64) for k, v in stats.items()}
    inverted = np.zeros(P, bool)
    if vertices is not None:
        _, S = mc.face_measures(mc._widened(vertices), W)
        S = np.where(flip, -S, S)
        order = np.argsort(patch, kind="stable")
        starts = np.concatenate(([0], np.cumsum(stats["faces"])))
        volume = np.zeros(P)
        for l in range(P):
            mine = order[starts[l]:starts[l + 1]]
            volume[l] = mc._ordered_sum(np.array([mc._ordered_sum(S[mine[s:s + BLOCK]]) for s in range(0, len(mine), BLOCK)])) / 6.0
        if volume_sign is not None:
            inverted = orientable & (stats["boundary_edges"] == 0) & _wrong(volume, volume_sign)
        volume = np.where(inverted, -volume, volume)
    flip = flip ^ inverted[patch]
    stats.update(flipped_faces=np.bincount(patch[flip], minlength=P).astype(np.int64), orientable=orientable, inverted=inverted)
    if vertices is not None:
        stats["volume"] = volume
    totals = dict(patches=P, orientable_patches=int(orientable.sum()), pair_edges=int((c == 2).sum()), disagreeing_edges=int(((c == 2) & (f != 1)).sum()),
                  flipped_faces=int(flip.sum()), inverted_patches=int(inverted.sum()), boundary_edges=int((c == 1).sum()),
                  nonmanifold_edges=int((c > 2).sum()))
    return dict(flip=flip.astype(np.uint8), patch=patch.astype(np.int32), faces=_swapped(faces, flip), stats=stats, totals=totals)


def loop(faces, n, vertices=None, volume_sign=None):
    """the same result by a breadth-first walk"""
    W = mc._wrapped(faces, n).tolist()
    m = len(W)
    if m == 0:
        return _empty(faces, vertices is not None)
    edges = {}
    for j, w in enumerate(W):
        for k in range(3):
            s, t = w[k], w[(k + 1) % 3]
            if s != t:
                edges.setdefault((min(s, t), max(s, t)), []).append((j, s < t))
    across = [[] for _ in range(m)]                 # (other face, disagree) over pair edges
    for recs in edges.values():
        if len(recs) == 2:
            (x, fx), (y, fy) = recs
            across[x].append((y, fx == fy))
            across[y].append((x, fx == fy))
    patch, flip, orientable = [-1] * m, [False] * m, []
    for j in range(m):                              # ascending: a patch is met at its smallest face first
        if patch[j] >= 0:
            continue
        l, ok, members = len(orientable), True, [j]
        patch[j] = l
        queue = collections.deque([j])
        while queue:
            x = queue.popleft()
            for y, dis in across[x]:
                if patch[y] < 0:
                    patch[y], flip[y] = l, flip[x] != dis
                    members.append(y)
                    queue.append(y)
                elif flip[y] != (flip[x] != dis):
                    ok = False
        if not ok:
            for y in members:
                flip[y] = False
        orientable.append(ok)
    P = len(orientable)
    stats = {name: np.zeros(P, np.int64) for name in COUNTS}
    totals = dict.fromkeys(TOTALS, 0)
    for j in range(m):
        stats["faces"][patch[j]] += 1
    for recs in edges.values():
        l = patch[recs[0][0]]
        if len(recs) == 2:
            dis = recs[0][1] == recs[1][1]
            stats["pair_edges"][l] += 1
            stats["disagreeing_edges"][l] += dis
            totals["pair_edges"] += 1
            totals["disagreeing_edges"] += dis
        elif len(recs) == 1:
            stats["boundary_edges"][l] += 1
            totals["boundary_edges"] += 1
        else:
            totals["nonmanifold_edges"] += 1
            for j, _ in recs:
                stats["nonmanifold_records"][patch[j]] += 1
    inverted = [False] * P
    if vertices is not None:
        V = mc._widened(vertices).tolist()
        mine = [[] for _ in range(P)]
        for j, (i0, i1, i2) in enumerate(W):
            p0, p1, p2 = V[i0], V[i1], V[i2]
            mx, my, mz = p1[1] * p2[2] - p1[2] * p2[1], p1[2] * p2[0] - p1[0] * p2[2], p1[0] * p2[1] - p1[1] * p2[0]
            S = (p0[0] * mx + p0[1] * my) + p0[2] * mz
            mine[patch[j]].append(-S if flip[j] else S)
        volume = np.zeros(P)
        for l, terms in enumerate(mine):
            total = 0.0
            for s in range(0, len(terms), BLOCK):
                block = 0.0
                for S in terms[s:s + BLOCK]:
                    block += S
                total += block
            vol = total / 6.0
            if volume_sign is not None and orientable[l] and stats["boundary_edges"][l] == 0 and bool(_wrong(vol, volume_sign)):
                inverted[l], vol = True, -vol
            volume[l] = vol
    flip = [fl != inverted[patch[j]] for j, fl in enumerate(flip)]
    for j in range(m):
        stats["flipped_faces"][patch[j]] += flip[j]
    stats.update(orientable=np.array(orientable, bool), inverted=np.array(inverted, bool))
    if vertices is not None:
        stats["volume"] = volume
    totals.update(patches=P, orientable_patches=sum(orientable), flipped_faces=sum(flip), inverted_patches=sum(inverted))
    totals = {k: int(v) for k, v in totals.items()}
    return dict(flip=np.array(flip, np.uint8), patch=np.array(patch, np.int32), faces=_swapped(faces, np.array(flip, bool)), stats=stats, totals=totals)


def same(x, y):
    """two results equal in every output, floats by their bytes"""
    ok = all(np.array_equal(x[k], y[k]) and x[k].dtype == y[k].dtype for k in ("flip", "patch", "faces")) and x["totals"] == y["totals"]
    ok = ok and set(x["stats"]) == set(y["stats"])
    for k in x["stats"]:
        p, q = np.asarray(x["stats"][k]), np.asarray(y["stats"][k])
        ok = ok and p.dtype == q.dtype and (np.array_equal(p.view(np.uint64), q.view(np.uint64)) if p.dtype == np.float64 else np.array_equal(p, q))
    return bool(ok)


# ---- constructed meshes ------------------------------------------------------------------------------------------------------------------
PROJECTIVE_PLANE = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 5], [0, 5, 1], [1, 2, 4], [2, 3, 5], [3, 4, 1], [4, 5, 2], [5, 1, 3]], np.int32)


def band(k, twisted):
    """a closed band of k quads over 2 k vertices, each quad two faces; twisted: the last quad joins vertex 2k - 2 to 1 and 2k - 1 to 0"""
    F = []
    for i in range(k):
        a, b = 2 * i, 2 * i + 1
        c, e = (2 * (i + 1), 2 * (i + 1) + 1) if i + 1 < k else ((1, 0) if twisted else (0, 1))
        F += [[a, c, b], [b, c, e]]
    ang = np.arange(2 * k) // 2 * (2 * np.pi / k)
    V = np.stack([np.cos(ang) * (1.0 + 0.2 * (np.arange(2 * k) % 2)), np.sin(ang), 0.3 * (np.arange(2 * k) % 2)], 1) + mc._irrational(2 * k, 4.0)
    return V.astype(np.float32), np.array(F, np.int32)


@functools.lru_cache(maxsize=None)
def fan(m=4096):
    """m faces round vertex 0, closed: every face shares an edge with the next, and all of them one vertex"""
    k = np.arange(m)
    F = np.stack([np.zeros(m, np.int64), 1 + k, 1 + (k + 1) % m], 1).astype(np.int32)
    ang = k * (2 * np.pi / m)
    V = np.concatenate([[[0.0, 0.0, 1.0]], np.stack([np.cos(ang), np.sin(ang), 0 * ang], 1)]) + mc._irrational(m + 1, 5.0)
    return sr._frozen(V.astype(np.float32), F)


def preswapped(F, seed, fraction=0.5):
    """(faces with a seeded random subset wound the other way, the subset)"""
    k = np.random.default_rng(seed).random(len(F)) < fraction
    G = np.array(F, copy=True)
    G[k] = G[k][:, [0, 2, 1]]
    return G, k
