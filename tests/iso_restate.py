"""NumPy restatement of the isosurface rule of include/pb3d.h (pb3d_iso_*, csrc/mesh.hip), written from the header's text, and the
mesh probes tests/test_isosurface.py uses.  The case table, the ownership rule and the edge numbering are those of
tests/mesh_restate.py; the arithmetic of a vertex is spelled out here with float64 scalars.  Needs no device.

    inside      float64(v) > level (a value equal to the level is outside)
    edge vertex a = the edge's end with the lower index on its axis, b the other: t = (level - va) / (vb - va) in float64, the
                coordinate on the axis float32(float64(ia) + t), the other two the float32 lattice indices
    centre      c + 0.5 on every axis
    output      every coordinate / float32(divisor) in float32"""
import collections

import numpy as np

from mesh_restate import ORDER, TRIS, edge_offsets, owns


def inside_mask(vol, level):
    vol = np.asarray(vol)
    assert vol.dtype == np.float32 and vol.ndim == 3
    return vol.astype(np.float64) > np.float64(level)


def case_volume(mask):
    n0, n1, n2 = mask.shape
    m = mask.astype(np.int64)
    cases = np.zeros((n0 - 1, n1 - 1, n2 - 1), np.int64)
    for bit in range(8):
        a0, a1, a2 = (bit >> 2) & 1, (bit >> 1) & 1, bit & 1
        cases |= m[a0:a0 + n0 - 1, a1:a1 + n1 - 1, a2:a2 + n2 - 1] << bit
    return cases


def edge_vertex(vol, level, c, e):
    """(position in lattice units as three float32, t) of local edge vertex e of cube c"""
    ax, o = edge_offsets(e)
    a = [c[k] + o[k] for k in range(3)]
    b = list(a)
    b[ax] += 1
    va, vb = np.float64(vol[tuple(a)]), np.float64(vol[tuple(b)])
    num = np.float64(level) - va
    den = vb - va
    t = num / den
    pos = [np.float32(a[k]) for k in range(3)]
    pos[ax] = np.float32(np.float64(a[ax]) + t)
    return pos, t


def isosurface(vol, level, divisor=1.0, return_t=False):
    """(verts (n, 3) float32 in (a0, a1, a2) order, faces (m, 3) int32) of a float32 volume; with return_t also the t of every vertex
    (NaN for a centre vertex)"""
    cases = case_volume(inside_mask(vol, level))
    verts, faces, ts = [], [], []
    index = {}        # (owner cube, local id) -> vertex index
    for c in map(tuple, np.argwhere((cases != 0) & (cases != 255))):
        cs = int(cases[c])
        for e in ORDER[cs]:
            if not owns(e, c):
                continue
            if e == 12:
                pos, t = [np.float32(c[k]) + np.float32(0.5) for k in range(3)], np.nan
            else:
                pos, t = edge_vertex(vol, level, c, e)
            index[(c, e)] = len(verts)
            verts.append(pos)
            ts.append(t)
        for tri in TRIS[cs]:
            row = []
            for e in tri:
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
    v = np.array(verts, np.float32).reshape(-1, 3) / np.float32(divisor)
    assert v.dtype == np.float32
    f = np.array(faces, np.int32).reshape(-1, 3)
    return (v, f, np.array(ts, np.float64)) if return_t else (v, f)


# ---- probes -----------------------------------------------------------------------------------------------------------------------------
def is_closed(faces):
    """every directed edge is matched by its reverse the same number of times"""
    f = np.asarray(faces, np.int64)
    count = collections.Counter()
    for a, b in ((0, 1), (1, 2), (2, 0)):
        count.update(zip(f[:, a].tolist(), f[:, b].tolist()))
    return all(count[(j, i)] == n for (i, j), n in count.items())


def zero_area_faces(verts, faces):
    """number of faces whose corners are collinear or coincide (exact in float64: the coordinates are float32)"""
    v = np.asarray(verts, np.float64)
    n = np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])
    return int((n == 0).all(axis=1).sum())


def border_below(vol, level):
    m = inside_mask(vol, level)
    return not (m[[0, -1]].any() or m[:, [0, -1]].any() or m[:, :, [0, -1]].any())


def crossed_edge_values(vol, level):
    """the float32 values at both ends of every sign-changing lattice edge"""
    m = inside_mask(vol, level)
    out = []
    for ax in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        x = m[tuple(lo)] != m[tuple(hi)]
        out += [vol[tuple(lo)][x], vol[tuple(hi)][x]]
    return np.concatenate(out)
