"""NumPy restatement of meshify_colored_voxel_grid (reference utils/voxel_utils.py:53-96) as csrc/mesh.hip computes it: the
binary case table (tests/golden/mc_binary_table.json, read off scikit-image), the edge-ownership rule, skimage's per-reference
normal accumulation and the exact nearest-occupied-voxel colour.  Needs no device; it is the CPU side of tests/test_meshify.py."""
import json
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLD, "mc_binary_table.json")) as _fh:
    _T = json.load(_fh)
TRIS = _T["tris"]     # per case: triangles (local vertex ids) in emission order, columns as skimage returns them
ORDER = _T["order"]   # per case: vertex creation order
LB = [0, 1, 3, 2, 4, 5, 7, 6]   # Lewiner corner i -> case bit a0*4 + a1*2 + a2


def edge_offsets(e):
    """axis of edge e and the local (a0, a1, a2) offsets of its low end"""
    ax, p, q = e >> 2, (e >> 1) & 1, e & 1
    o = [0, 0, 0]
    others = [a for a in range(3) if a != ax]
    o[others[0]], o[others[1]] = p, q
    return ax, o


def owns(e, c):
    """does cube c own its local vertex e (the lowest-scan-order cube holding the edge)?"""
    if e == 12:
        return True
    ax, o = edge_offsets(e)
    return all(o[a] == 1 or c[a] == 0 for a in range(3) if a != ax)


def contrib(cs, e):
    """skimage's per-reference gradient of vertex e in a cube of case cs, (a0, a1, a2) components"""
    v = [(cs >> LB[i]) & 1 for i in range(8)]
    if e == 12:
        return np.array([0, (v[0] + v[1] + v[4] + v[5]) - (v[2] + v[3] + v[6] + v[7]),
                         (v[0] + v[1] + v[2] + v[3]) - (v[4] + v[5] + v[6] + v[7])])
    vg = [(v[0] - v[1], v[0] - v[3], v[0] - v[4]), (v[0] - v[1], v[1] - v[2], v[1] - v[5]), (v[3] - v[2], v[1] - v[2], v[2] - v[6]),
          (v[3] - v[2], v[0] - v[3], v[3] - v[7]), (v[4] - v[5], v[4] - v[7], v[0] - v[4]), (v[4] - v[5], v[5] - v[6], v[1] - v[5]),
          (v[7] - v[6], v[5] - v[6], v[2] - v[6]), (v[7] - v[6], v[4] - v[7], v[3] - v[7])]
    ax, o = edge_offsets(e)
    i1 = o[0] * 4 + o[1] * 2 + o[2]          # skimage indexes vg (Lewiner order) with the binary corner index
    i2 = i1 + (4, 2, 1)[ax]
    g = np.array(vg[i1]) + np.array(vg[i2])   # x, y, z
    return g[::-1]


def marching_cubes_binary(mask):
    """(verts (a0,a1,a2) float32, faces int32, normals float32) as skimage's marching_cubes(mask.astype(uint8), level=0.5)"""
    n0, n1, n2 = mask.shape
    m = mask.astype(np.int64)
    cases = np.zeros((n0 - 1, n1 - 1, n2 - 1), np.int64)
    for bit in range(8):
        a0, a1, a2 = (bit >> 2) & 1, (bit >> 1) & 1, bit & 1
        cases |= m[a0:a0 + n0 - 1, a1:a1 + n1 - 1, a2:a2 + n2 - 1] << bit
    verts, faces, grads = [], [], []
    index = {}        # (owner cube, local id) -> vertex index
    for c in map(tuple, np.argwhere((cases != 0) & (cases != 255))):
        cs = int(cases[c])
        for e in ORDER[cs]:
            if not owns(e, c):
                continue
            if e == 12:
                pos = [c[0] + 0.5, c[1] + 0.5, c[2] + 0.5]
                g = contrib(cs, 12) * sum(t.count(12) for t in TRIS[cs])
            else:
                ax, o = edge_offsets(e)
                pos = [c[a] + o[a] + (0.5 if a == ax else 0.0) for a in range(3)]
                g = np.zeros(3, np.int64)
                others = [a for a in range(3) if a != ax]
                for dp in (0, 1):
                    for dq in (0, 1):
                        cc = list(c)
                        cc[others[0]] += o[others[0]] - dp
                        cc[others[1]] += o[others[1]] - dq
                        if all(0 <= cc[a] < cases.shape[a] for a in range(3)):
                            cs2 = int(cases[tuple(cc)])
                            e2 = 4 * ax + 2 * dp + dq
                            g = g + contrib(cs2, e2) * sum(t.count(e2) for t in TRIS[cs2])
            index[(c, e)] = len(verts)
            verts.append(pos)
            grads.append(g)
        for t in TRIS[cs]:
            row = []
            for e in t:
                if owns(e, c):
                    row.append(index[(c, e)])
                    continue
                ax, o = edge_offsets(e)
                oc, e2 = list(c), e
                for k, a in enumerate(a for a in range(3) if a != ax):
                    if o[a] == 0 and c[a] > 0:
                        oc[a] -= 1
                        e2 |= 2 >> k
                row.append(index[(tuple(oc), e2)])
            faces.append(row)
    g = np.array(grads, np.float64).reshape(-1, 3)
    ln = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
    nrm = np.zeros(g.shape, np.float32)
    nz = ln > 0
    nrm[nz] = (g[nz] / ln[nz, None]).astype(np.float32)
    return np.array(verts, np.float32).reshape(-1, 3), np.array(faces, np.int32).reshape(-1, 3), nrm


def nearest_filled(mask, queries):
    """Per query (n x 3 float64, lattice units): the scan-order lattice index of the nearest occupied point (ties to the
    smallest index) and the whole tie set."""
    pts = np.argwhere(mask).astype(np.float64)
    flat = np.ravel_multi_index(np.argwhere(mask).T, mask.shape)
    best, ties = [], []
    for q in queries:
        d = ((q - pts) ** 2).sum(-1)
        t = flat[d == d.min()]
        best.append(t.min())
        ties.append(t)
    return np.array(best, np.int64), ties


def queries(verts, stride):
    """the reference's query verts[:, [2,1,0]] / stride (float32 arithmetic), widened to float64"""
    return (verts[:, [2, 1, 0]] / stride).astype(np.float64)


def meshify(grid, stride=1):
    """The whole function: (verts, faces, vertex_colors, normals) with the reference's dtypes (ties to the smallest index)."""
    g = grid[::stride, ::stride, ::stride]
    mask = np.any(g > 0, axis=-1)
    v, f, n = marching_cubes_binary(mask)
    verts = (v * stride)[:, [2, 1, 0]]
    verts[:, 2] = grid.shape[2] - verts[:, 2]
    best, _ = nearest_filled(mask, queries(verts, stride))
    cols = g.reshape(-1, g.shape[-1])[best]
    if cols.max() > 1:
        cols = cols / 255.0
    return verts, f, cols, n
