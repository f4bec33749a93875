"""NumPy restatement of pb3d_voxelize_mesh_resident (include/pb3d.h, "mesh -> grid") as csrc/voxelize.hip computes it, and beside it the
same rules as a plain Python loop over faces, columns and bits.  Every product, sum, difference and quotient is one float64 operation,
in the header's order.  Needs no device; it is the CPU side of tests/test_voxelize_mesh.py."""
import math

import numpy as np

STATS = ("crossings", "occupied", "open_columns", "flat_faces")


def tie_rule(E, pos):
    """the header's rule: an edge accepts a column where E >= 0 (pos) or E < 0 (not pos)"""
    return E >= 0 if pos else E < 0


def lattice(verts, origin=(0, 0, 0), voxel_size=1.0, frame="lattice", depth=None):
    """(nv, 3) float64 lattice coordinates; ValueError on a coordinate that is not finite"""
    v = np.asarray(verts)
    v = v.astype(np.float64).reshape(-1, 3)          # float32 widens exactly
    if not np.all(np.isfinite(v)):
        raise ValueError("a vertex coordinate is not finite")
    if frame == "meshify":
        v = np.stack([np.float64(depth) - v[:, 2], v[:, 1], v[:, 0]], axis=1)
    elif frame != "lattice":
        raise ValueError(frame)
    with np.errstate(over="ignore"):
        return (v - np.asarray(origin, np.float64)) / np.float64(voxel_size)


def wrapped(faces, nv):
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    if f.size and (f.min() < -nv or f.max() >= nv):
        raise IndexError("index out of bounds")
    return np.where(f < 0, f + nv, f)


def _column_box(A, B, C, n0, n1):
    """inclusive (i0, i1, j0, j1), clamped in float64 first; None if empty"""
    ilo = max(0.0, float(np.ceil(min(A[0], B[0], C[0]))))           # np.ceil / np.floor: an infinity stays one
    ihi = min(float(n0 - 1), float(np.floor(max(A[0], B[0], C[0]))))
    jlo = max(0.0, float(np.ceil(min(A[1], B[1], C[1]))))
    jhi = min(float(n1 - 1), float(np.floor(max(A[1], B[1], C[1]))))
    if not (ilo <= ihi and jlo <= jhi):
        return None
    return int(ilo), int(ihi), int(jlo), int(jhi)


def _edges(A, B, C, area):
    """per directed edge: (lo, hi, pos)"""
    out = []
    for P, Q in ((A, B), (B, C), (C, A)):
        flipped = (Q[0], Q[1]) < (P[0], P[1])
        lo, hi = (Q, P) if flipped else (P, Q)
        out.append((lo, hi, (area > 0) != flipped))
    return out


def restate(verts, faces, shape, origin=(0, 0, 0), voxel_size=1.0, frame="lattice", depth=None, accept=tie_rule):
    """(occ uint8 of `shape`, stats dict): one NumPy pass per face over the columns of its box"""
    n0, n1, n2 = shape
    L = lattice(verts, origin, voxel_size, frame, n2 if depth is None else depth)
    F = wrapped(faces, len(L))
    flips = np.zeros((n0, n1, n2 + 1), np.uint8)        # [..., n2] = the column's overflow bit
    crossings = flat = 0
    with np.errstate(over="ignore", invalid="ignore"):
        for a, b, c in F:
            A, B, C = L[a], L[b], L[c]
            area = (B[0] - A[0]) * (C[1] - A[1]) - (B[1] - A[1]) * (C[0] - A[0])
            if area == 0:
                flat += 1
                continue
            box = _column_box(A, B, C, n0, n1)
            if box is None:
                continue
            i0, i1, j0, j1 = box
            i = np.arange(i0, i1 + 1, dtype=np.float64)[:, None]
            j = np.arange(j0, j1 + 1, dtype=np.float64)[None, :]
            inside = np.ones((i1 - i0 + 1, j1 - j0 + 1), bool)
            for lo, hi, pos in _edges(A, B, C, area):
                E = (hi[0] - lo[0]) * (j - lo[1]) - (hi[1] - lo[1]) * (i - lo[0])
                inside &= accept(E, pos)
            if not inside.any():
                continue
            nx = (B[1] - A[1]) * (C[2] - A[2]) - (B[2] - A[2]) * (C[1] - A[1])
            ny = (B[2] - A[2]) * (C[0] - A[0]) - (B[0] - A[0]) * (C[2] - A[2])
            z = A[2] - (nx * (i - A[0]) + ny * (j - A[1])) / area
            kz = np.ceil(z)[inside]
            ii, jj = np.nonzero(inside)
            k = np.where(kz <= n2 - 1, np.maximum(kz, 0.0), np.float64(n2))      # a NaN compares false: the overflow bit
            np.bitwise_xor.at(flips, (ii + i0, jj + j0, k.astype(np.int64)), 1)
            crossings += len(ii)
    occ = np.bitwise_xor.accumulate(flips[:, :, :n2], axis=2)
    open_columns = int(np.count_nonzero(occ[:, :, n2 - 1] ^ flips[:, :, n2]))
    return occ, dict(zip(STATS, (crossings, int(occ.sum()), open_columns, flat)))


def loop(verts, faces, shape, origin=(0, 0, 0), voxel_size=1.0, frame="lattice", depth=None):
    """the same rules with nothing but Python floats and loops over faces, columns and bits"""
    n0, n1, n2 = shape
    L = [[float(x) for x in row] for row in lattice(verts, origin, voxel_size, frame, n2 if depth is None else depth)]
    F = wrapped(faces, len(L)).tolist()
    flips = [[[0] * (n2 + 1) for _ in range(n1)] for _ in range(n0)]
    crossings = flat = 0
    for a, b, c in F:
        A, B, C = L[a], L[b], L[c]
        area = (B[0] - A[0]) * (C[1] - A[1]) - (B[1] - A[1]) * (C[0] - A[0])
        if area == 0:
            flat += 1
            continue
        box = _column_box(A, B, C, n0, n1)
        if box is None:
            continue
        edges = _edges(A, B, C, area)
        nx = (B[1] - A[1]) * (C[2] - A[2]) - (B[2] - A[2]) * (C[1] - A[1])
        ny = (B[2] - A[2]) * (C[0] - A[0]) - (B[0] - A[0]) * (C[2] - A[2])
        for i in range(box[0], box[1] + 1):
            for j in range(box[2], box[3] + 1):
                x, y = float(i), float(j)
                ok = True
                for lo, hi, pos in edges:
                    E = (hi[0] - lo[0]) * (y - lo[1]) - (hi[1] - lo[1]) * (x - lo[0])
                    ok = ok and (E >= 0 if pos else E < 0)
                if not ok:
                    continue
                z = A[2] - (nx * (x - A[0]) + ny * (y - A[1])) / area
                if z <= n2 - 1:                        # ceil(z) <= n2 - 1, n2 - 1 being an integer
                    k = 0 if z <= 0 else math.ceil(z)
                else:
                    k = n2
                flips[i][j][k] ^= 1
                crossings += 1
    occ = np.zeros((n0, n1, n2), np.uint8)
    open_columns = 0
    for i in range(n0):
        for j in range(n1):
            p = 0
            for k in range(n2):
                p ^= flips[i][j][k]
                occ[i, j, k] = p
            open_columns += p ^ flips[i][j][n2]
    return occ, dict(zip(STATS, (crossings, int(occ.sum()), open_columns, flat)))


# ---- constructed cases: name -> (verts, faces, shape, keyword arguments) --------------------------------------------------------------
def box(lo, hi):
    """the 12 triangles of the box with corners lo and hi, float64"""
    v = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])], np.float64)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return v, np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int64)


def join(*meshes):
    """one face list over the meshes' vertices"""
    vs, fs, base = [], [], 0
    for v, f in meshes:
        vs.append(np.asarray(v, np.float64))
        fs.append(np.asarray(f, np.int64) + base)
        base += len(v)
    return np.concatenate(vs), np.concatenate(fs)


def octahedron(centre, r):
    c = np.asarray(centre, np.float64)
    v = c + r * np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    return v, np.array(f, np.int64)


def uv_sphere(centre, r, nlat=12, nlon=16, dtype=np.float64):
    """a closed latitude / longitude sphere: its coordinates are irrational, so every product below rounds"""
    th = np.pi * np.arange(1, nlat) / nlat
    ph = 2 * np.pi * np.arange(nlon) / nlon
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones(nlon))], axis=-1)
    v = np.concatenate([[[0, 0, 1.0]], ring.reshape(-1, 3), [[0, 0, -1.0]]])
    f = []
    at = lambda a, b: 1 + a * nlon + b % nlon     # noqa: E731
    last = len(v) - 1
    for b in range(nlon):
        f.append((0, at(0, b), at(0, b + 1)))
        f.append((last, at(nlat - 2, b + 1), at(nlat - 2, b)))
        for a in range(nlat - 2):
            f.append((at(a, b), at(a + 1, b), at(a + 1, b + 1)))
            f.append((at(a, b), at(a + 1, b + 1), at(a, b + 1)))
    return (np.asarray(centre, np.float64) + r * v).astype(dtype), np.array(f, np.int64)


def random_mask(shape, density, seed):
    """a random mask with an empty one-voxel border"""
    m = np.zeros(shape, bool)
    m[1:-1, 1:-1, 1:-1] = np.random.default_rng(seed).random(tuple(n - 2 for n in shape)) < density
    return m


ROUND_TRIPS = (((9, 8, 10), 0.5, 0), ((12, 11, 13), 0.3, 1), ((10, 10, 10), 0.7, 2), ((14, 9, 12), 0.5, 3))
WORD_DEPTHS = (1, 31, 32, 33, 64, 65)


def word_boundary_mesh(n2):
    """boxes whose crossings sit below 0, at k = 31 and 32, at k = n2 - 1 (between samples and exactly on one) and above the grid"""
    return join(box((0.5, 0.5, -3.5), (2.5, 2.5, 30.5)), box((3.5, 0.5, 31.5), (5.5, 2.5, n2 - 1.5)),
                box((0.5, 3.5, n2 - 2.5), (2.5, 5.5, n2 + 3.5)), box((3.5, 3.5, n2 + 1.5), (5.5, 5.5, n2 + 4.5)),
                box((6.5, 6.5, 2.0), (7.5, 7.5, n2 - 1.0)))


def constructed_cases():
    cases = {}
    cases["pinned_box"] = (*box((2, 3, 1), (6, 7, 5)), (9, 10, 8), {})
    cases["octahedron"] = (*octahedron((5, 5, 5), 3), (11, 11, 11), {})         # vertices on samples, edges through samples
    cases["octahedron_box"] = (*join(octahedron((4, 4, 4), 3), box((8, 1, 1), (11, 6, 7))), (13, 9, 9), {})
    cases["sphere_f32"] = (*uv_sphere((9.1, 8.7, 10.2), 5.3, dtype=np.float32), (19, 18, 21), {})
    cases["sphere_f64"] = (*uv_sphere((9.1, 8.7, 10.2), 5.3), (19, 18, 21), {})
    v, f = uv_sphere((9.1, 8.7, 10.2), 5.3)
    origin = (1.3, -0.7, 2.1)
    cases["sphere_scaled"] = (v * 0.37 + np.array(origin), f, (19, 18, 21), dict(origin=origin, voxel_size=0.37))
    for n2 in WORD_DEPTHS:
        cases[f"words_{n2}"] = (*word_boundary_mesh(n2), (8, 8, n2), {})
    # columns longer than one wavefront's 64 dwords: the scan carries across two and three chunks of them
    cases["tall_2100"] = (*join(box((-0.5, 0.5, 100.3), (1.5, 1.5, 2090.2)), octahedron((0.4, 0.3, 2060.2), 30.0)), (2, 3, 2100), {})
    cases["tall_4133"] = (*join(box((0.5, -0.5, 31.5), (1.5, 1.5, 4100.5)), box((-0.5, -0.5, 2047.5), (0.5, 0.5, 4140.0))), (2, 2, 4133), {})
    slabs = [box((0.5, 0.5, 0.75 * t + 0.1), (20.5, 20.5, 0.75 * t + 0.6)) for t in range(40)]
    cases["slabs"] = (*join(*slabs), (22, 22, 32), {})                           # every crossing of a column in one dword
    v, f = join(octahedron((5, 5, 5), 3.5), uv_sphere((5.2, 4.9, 5.1), 3.3))
    cases["twice"] = (v, np.concatenate([f, f]), (11, 11, 11), {})
    rng = np.random.default_rng(7)
    c = rng.random((20000, 1, 3)) * (40, 40, 64)
    small = (c + rng.uniform(-0.8, 0.8, (20000, 3, 3))).reshape(-1, 3)
    v, f = join(box((-0.5, -0.5, -0.5), (39.5, 39.5, 63.5)), (small, np.arange(60000).reshape(-1, 3)))
    cases["imbalance"] = (v.astype(np.float32), f, (40, 40, 64), {})
    # more faces too wide for a lane than the workgroups that walk them
    c = rng.random((3000, 1, 3)) * (40, 40, 64)
    cases["many_wide"] = ((c + rng.uniform(-6.0, 6.0, (3000, 3, 3))).reshape(-1, 3), np.arange(9000).reshape(-1, 3), (40, 40, 64), {})
    # 16 510 columns of 33 dwords, one wavefront each: more than a capped grid of 16 workgroups on each of 256 CUs takes in one round
    cases["many_columns"] = (*join(uv_sphere((60.3, 70.1, 500.7), 55.2), box((2.5, 3.5, 1000.5), (126.5, 120.5, 1030.0)),
                                   box((90.5, 3.5, -4.0), (120.5, 30.5, 31.5))), (130, 127, 1025), {})
    cases["outside"] = (*uv_sphere((6, 6, 6), 9.0, dtype=np.float32), (12, 12, 12), {})
    cases["triangle"] = (np.array([[1.2, 1.1, 3.3], [9.7, 2.2, 5.1], [3.3, 8.8, 1.2]]), np.array([[0, 1, 2]]), (12, 12, 8), {})
    v, f = uv_sphere((6.3, 6.1, 5.7), 4.4)
    cases["hemisphere"] = (v, f[(v[f][:, :, 2] >= 5.7).all(axis=1)], (13, 13, 12), {})
    for v, f, _, _ in cases.values():
        v.setflags(write=False)
        f.setflags(write=False)
    return cases
