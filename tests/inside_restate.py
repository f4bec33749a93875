"""NumPy restatement of pb3d_points_in_mesh_resident (include/pb3d.h, "containment") as csrc/inside.hip computes it: a loop over the
faces, vectorised over the queries.  Every product, sum, difference and quotient is one float64 operation, in the header's order; the
edge rule is the voxelization's own (tests/voxelize_restate.py).  Needs no device; it is the CPU side of tests/test_points_in_mesh.py,
which also takes its constructed meshes and query sets from here."""
import numpy as np

from voxelize_restate import _edges, box, octahedron, wrapped  # noqa: F401  (box and octahedron: the tests' meshes)

STATS = ("inside", "odd_totals", "flat_faces", "outside_box")


def restate(P, verts, faces):
    """(inside bool (n,), counts int32 (n, 2) = (below, total), stats dict).  ValueError on a vertex that is not finite, IndexError on
    a face index outside [-nv, nv); a query with a NaN coordinate is outside with zero counts, as a resident caller's is"""
    q = np.asarray(P).astype(np.float64).reshape(-1, 3)             # float32 widens exactly
    V = np.asarray(verts).astype(np.float64).reshape(-1, 3)
    if not np.all(np.isfinite(V)):
        raise ValueError("a vertex coordinate is not finite")
    F = wrapped(faces, len(V))
    n = len(q)
    below, total = np.zeros(n, np.int32), np.zeros(n, np.int32)
    flat = 0
    q0, q1, q2 = q[:, 0], q[:, 1], q[:, 2]
    with np.errstate(over="ignore", invalid="ignore"):
        if len(F):
            lo, hi = V[:, :2].min(axis=0), V[:, :2].max(axis=0)     # the box of ALL vertices
            boxed = (q0 >= lo[0]) & (q0 <= hi[0]) & (q1 >= lo[1]) & (q1 <= hi[1]) & ~np.isnan(q2)
        else:
            boxed = np.zeros(n, bool)
        for a, b, c in F:
            A, B, C = V[a], V[b], V[c]
            area = (B[0] - A[0]) * (C[1] - A[1]) - (B[1] - A[1]) * (C[0] - A[0])
            if area == 0:
                flat += 1
                continue
            held = boxed & (min(A[0], B[0], C[0]) <= q0) & (q0 <= max(A[0], B[0], C[0])) & \
                (min(A[1], B[1], C[1]) <= q1) & (q1 <= max(A[1], B[1], C[1]))
            idx = np.flatnonzero(held)
            if not idx.size:
                continue
            x, y = q0[idx], q1[idx]
            ok = np.ones(idx.size, bool)
            for elo, ehi, pos in _edges(A, B, C, area):
                E = (ehi[0] - elo[0]) * (y - elo[1]) - (ehi[1] - elo[1]) * (x - elo[0])
                ok &= (E >= 0) if pos else (E < 0)
            idx, x, y = idx[ok], x[ok], y[ok]
            nx = (B[1] - A[1]) * (C[2] - A[2]) - (B[2] - A[2]) * (C[1] - A[1])
            ny = (B[2] - A[2]) * (C[0] - A[0]) - (B[0] - A[0]) * (C[2] - A[2])
            z = A[2] - (nx * (x - A[0]) + ny * (y - A[1])) / area
            total[idx] += 1
            below[idx] += z <= q2[idx]                              # a NaN height counts in total only
    inside = (below & 1).astype(bool)
    stats = dict(zip(STATS, (int(inside.sum()), int((total & 1).sum()), flat, int(n - boxed.sum()))))
    return inside, np.stack([below, total], axis=1), stats


# ---- constructed meshes and query sets -----------------------------------------------------------------------------------------------
def lattice_points(shape, dtype=np.float64):
    """the sample points of a grid of `shape` in the grid's own order: row (i * n1 + j) * n2 + k is (i, j, k)"""
    return np.ascontiguousarray(np.indices(shape).reshape(3, -1).T.astype(dtype))


def quarter_points(r=5):
    """every quarter-integer point of [-r, r]^3 (r = 5: 41^3 = 68 921 of them), exact in float32 and float64"""
    t = np.arange(-4 * r, 4 * r + 1, dtype=np.float64) / 4.0
    return np.ascontiguousarray(np.stack(np.meshgrid(t, t, t, indexing="ij"), axis=-1).reshape(-1, 3))


def icosphere(subdivisions=2):
    """the unit icosphere: 20 * 4^subdivisions faces (2: 320), outward winding, float64"""
    t = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1),
         (-t, 0, 1)]
    v = [np.array(p, np.float64) / np.sqrt(1.0 + t * t) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, out = {}, []

        def middle(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.sqrt(m @ m))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = out
    return np.array(v, np.float64), np.array(f, np.int64)


def inradius(verts, faces):
    """the smallest distance from the origin to a face's plane (a convex mesh around the origin: the largest ball inside it)"""
    a, b, c = (verts[faces[:, k]] for k in range(3))
    n = np.cross(b - a, c - a)
    return float(np.min(np.abs(np.einsum("ij,ij->i", n, a)) / np.linalg.norm(n, axis=1)))


def rotation(seed):
    """a proper rotation with irrational entries, from the QR factorisation of a random matrix"""
    q, r = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else q[:, ::-1]


def tie_queries(verts, faces, seed, per=3):
    """queries whose (q0, q1) are copied from the vertices and the edge midpoints of the mesh, `per` heights each: every one projects
    onto a vertex or an edge.  Computed in the dtype of `verts`, so a float32 mesh gets float32 queries on its own coordinates"""
    v = np.asarray(verts)
    f = wrapped(faces, len(v))
    mids = np.concatenate([(v[f[:, k]] + v[f[:, (k + 1) % 3]]) * v.dtype.type(0.5) for k in range(3)])
    xy = np.concatenate([v[:, :2], mids[:, :2]])
    rng = np.random.default_rng(seed)
    lo, hi = float(v[:, 2].min()) - 0.5, float(v[:, 2].max()) + 0.5
    z = rng.uniform(lo, hi, (len(xy), per)).astype(v.dtype)
    return np.ascontiguousarray(np.concatenate([np.column_stack([xy, z[:, k]]) for k in range(per)]).astype(v.dtype))


def wall_among_small(seed=3, n_small=500):
    """two faces over the whole unit square among n_small faces whose corners scatter 0.15 around their centres: 502 faces get a
    16 x 16 grid (two faces per cell), and a small face spans three or four of its cells of edge 1/16 per axis -- more than the cap of 8
    entries per face on average (tests assert the count) -- so the index must halve its cells.  (In 2-D a wall alone cannot exceed the
    cap: it is listed in every cell, which is nf / 2 entries.)"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.15, 0.85, (n_small, 1, 2))
    xy = (c + rng.uniform(-0.15, 0.15, (n_small, 3, 2))).reshape(-1, 2)
    small = np.column_stack([xy, rng.uniform(0.0, 1.0, len(xy))])
    wall = np.array([[0.0, 0.0, 0.5], [1.0, 0.0, 0.5], [0.0, 1.0, 0.5]])
    wall2 = np.array([[1.0, 1.0, 0.25]])
    v = np.concatenate([wall, wall2, small])
    f = np.concatenate([[[0, 1, 2], [1, 3, 2]], 4 + np.arange(3 * n_small).reshape(-1, 3)])
    return v, f.astype(np.int64)


def first_grid_entries(verts, faces, cap_per_cell=2.0):
    """((cells along a0, cells along a1), (cell, face) entries) of the index's FIRST grid, before any halving: the sizing rule of the
    searches' grid in 2-D (cell edge h with h^2 = area of the box / (nf / 2), ceil(extent / h) cells per axis) and the listing rule
    cell(min corner) .. cell(max corner); for meshes whose box has a positive extent on both axes"""
    v = np.asarray(verts, np.float64)
    f = wrapped(faces, len(v))
    lo, hi = v[:, :2].min(axis=0), v[:, :2].max(axis=0)
    ext = hi - lo
    h = np.exp((np.log(ext).sum() - np.log(max(1.0, len(f) / cap_per_cell))) / 2.0)
    n = np.maximum(np.ceil(ext / h), 1.0)
    inv = np.where(n > 1, n / ext, 0.0)
    cell = lambda p: np.clip(np.floor((p - lo) * inv), 0, n - 1)      # noqa: E731
    t = v[f][:, :, :2]
    area = (t[:, 1, 0] - t[:, 0, 0]) * (t[:, 2, 1] - t[:, 0, 1]) - (t[:, 1, 1] - t[:, 0, 1]) * (t[:, 2, 0] - t[:, 0, 0])
    span = cell(t.max(axis=1)) - cell(t.min(axis=1)) + 1
    return (int(n[0]), int(n[1])), int((span[:, 0] * span[:, 1])[area != 0].sum())


def grid_entries(verts, faces, cells):
    """the (cell, face) entries of the index on a grid of `cells` = (cells along a0, cells along a1) over the (a0, a1) box of ALL
    vertices, by the arithmetic of mesh_cases.index_entries: inv = n / extent (0 on a one-cell axis), cell = clip(floor((p - lo) * inv),
    0, n - 1), a face listed in cell(min corner) .. cell(max corner) per axis -- and a face whose projected area is 0 nowhere.  The
    same float64 operations as the device's, so the count is the device's exactly"""
    v = np.asarray(verts).astype(np.float64)
    f = wrapped(faces, len(v))
    n = np.array(cells, np.int64)
    lo, ext = v[:, :2].min(axis=0), v[:, :2].max(axis=0) - v[:, :2].min(axis=0)
    inv = np.where(n > 1, n / np.where(n > 1, ext, 1.0), 0.0)
    t = v[f][:, :, :2]
    area = (t[:, 1, 0] - t[:, 0, 0]) * (t[:, 2, 1] - t[:, 0, 1]) - (t[:, 1, 1] - t[:, 0, 1]) * (t[:, 2, 0] - t[:, 0, 0])
    first = np.clip(np.floor((t.min(axis=1) - lo) * inv), 0, n - 1)
    last = np.clip(np.floor((t.max(axis=1) - lo) * inv), 0, n - 1)
    return int((last - first + 1).prod(axis=1)[area != 0].sum())
