"""Constructed meshes and query sets shared by tests/test_meshdist_restate.py (CPU) and tests/test_mesh_target.py (GPU)."""
import ctypes as C
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixture_mesh(name):
    """(vertices, faces) of tests/golden/surface_<name>.npz"""
    with np.load(os.path.join(GOLD, f"surface_{name}.npz")) as z:
        return z["vertices"], z["faces"]


def real_mesh_queries(v, seed):
    """the mesh's own vertices (every distance 0), jittered vertices, a uniform cloud in 1.5 x the box, 64 points at 100 x the box:
    2 764 queries at most"""
    rng = np.random.default_rng(seed)
    v = v.astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    mid, half = (lo + hi) / 2, np.maximum((hi - lo) / 2, 1e-3 * (hi - lo).max())
    own = v[rng.choice(len(v), min(len(v), 900), replace=False)]
    jit = v[rng.choice(len(v), 800, replace=False)] + rng.normal(0, 0.01 * (hi - lo).max(), (800, 3))
    cloud = mid + rng.uniform(-1.5, 1.5, (1000, 3)) * half
    far = mid + rng.uniform(-100, 100, (64, 3)) * half
    return own, np.concatenate([jit, cloud, far])


def lattice_mesh():
    """the 13 x 13 x 3 integer lattice: every unit square of every axis-aligned lattice plane, split into two triangles (2 112 faces),
    and every lattice point of a box two steps larger as a query (2 023): nearly every query is equally near several faces"""
    nx, ny, nz = 13, 13, 3
    idx = np.arange(nx * ny * nz).reshape(nx, ny, nz)
    v = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    faces = []
    for p00, p10, p01, p11 in ((idx[:-1, :-1, :], idx[1:, :-1, :], idx[:-1, 1:, :], idx[1:, 1:, :]),
                               (idx[:-1, :, :-1], idx[1:, :, :-1], idx[:-1, :, 1:], idx[1:, :, 1:]),
                               (idx[:, :-1, :-1], idx[:, 1:, :-1], idx[:, :-1, 1:], idx[:, 1:, 1:])):
        faces.append(np.stack([p00.ravel(), p10.ravel(), p11.ravel()], 1))
        faces.append(np.stack([p00.ravel(), p11.ravel(), p01.ravel()], 1))
    f = np.concatenate(faces)
    q = np.stack(np.meshgrid(np.arange(-2, nx + 2), np.arange(-2, ny + 2), np.arange(-2, nz + 2), indexing="ij"), -1).reshape(-1, 3)
    return v, f, q.astype(np.float64)


def giant_and_needles():
    """One triangle spanning the whole 100-box, 2 000 triangles of 1e-3 of its size, 1 500 needles of aspect 1e-6 that run 60 .. 140
    units across the box, clipped to it (the cells of their boxes are what overflows the entry cap: a single giant face is listed
    in every cell, but a grid sized from the face count has only half as many cells as faces), the four degenerate kinds, a
    duplicated face, and vertices no face names, two of them outside everything else (they enlarge the box): (vertices, faces int64,
    queries (2 500, 3))"""
    rng = np.random.default_rng(11)
    tris = [np.array([[0.0, 0.0, 0.0], [100.0, 0.0, 60.0], [0.0, 100.0, 100.0]])]
    c = rng.uniform(1, 99, (2000, 1, 3))
    tris += list(c + rng.uniform(-0.05, 0.05, (2000, 3, 3)))
    for _ in range(1500):
        a = rng.uniform(5, 95, 3)
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        b = np.clip(a + d * rng.uniform(60, 140), 0, 100)
        p = np.cross(b - a, rng.normal(size=3))
        p /= np.linalg.norm(p)
        tris.append(np.array([a, b, (a + b) / 2 + p * 1e-6 * np.linalg.norm(b - a)]))
    a, b = np.array([20.0, 30.0, 40.0]), np.array([60.0, 35.0, 45.0])
    tris += [np.array(t) for t in ([a, a, b], [a, b, b], [a, (a + b) / 2, b], [a, b, a + 2 * (b - a)], [b, b, b])]
    v = np.concatenate(tris)
    f = np.arange(len(v)).reshape(-1, 3)
    f = np.concatenate([f, f[[7]], f[[0]]])                                             # a duplicated small face, the giant again
    v = np.concatenate([v, rng.uniform(0, 100, (10, 3)), [[-10.0, 50.0, 50.0], [110.0, 110.0, 110.0]]])    # unreferenced
    q = np.concatenate([rng.uniform(-30, 130, (1500, 3)), c[:500, 0] + rng.normal(0, 0.2, (500, 3)),
                        tris[0][0] + rng.uniform(0, 1, (500, 1)) * (tris[0][1] - tris[0][0]) * rng.uniform(0, 1, (500, 1))
                        + rng.uniform(0, 0.5, (500, 1)) * (tris[0][2] - tris[0][0]) + rng.normal(0, 0.5, (500, 3))])
    return v, f.astype(np.int64), q


def random_mesh(nf, seed, dtype=np.float64, zero_at=()):
    """nf random triangles over nf // 2 + 3 shared vertices; the faces listed in zero_at get a repeated corner (area 0)"""
    rng = np.random.default_rng(seed)
    nv = nf // 2 + 3
    v = rng.uniform(-3, 5, (nv, 3)).astype(dtype)
    f = np.stack([rng.permutation(nv)[:3] for _ in range(nf)]).astype(np.int64)
    for z in zero_at:
        f[z, 2] = f[z, 0]
    return v, f


def index_entries(v, f, halvings):
    """(cells per axis, (cell, face) entries) of the triangle index as include/pb3d.h describes it, in NumPy: the cell grid
    pb3d_nn_grid_shape gives for the box of ALL vertices and the face count (a host function, no device), its cells per axis halved
    `halvings` times, every face listed in the cells cell(min corner) .. cell(max corner)"""
    from pb3d import _lib
    v = np.asarray(v).astype(np.float64)
    b = np.concatenate([v.min(0), v.max(0)])
    cells = (C.c_int64 * 3)()
    _lib.check(_lib.load().pb3d_nn_grid_shape(_lib.p_dbl(b), len(f), cells))
    n = np.array(list(cells))
    for _ in range(halvings):
        n = (n + 1) // 2
    inv = np.where(n > 1, n / np.where(n > 1, b[3:] - b[:3], 1.0), 0.0)
    t = v[np.asarray(f).astype(np.int64)]
    lo = np.clip(np.floor((t.min(1) - b[:3]) * inv), 0, n - 1)
    hi = np.clip(np.floor((t.max(1) - b[:3]) * inv), 0, n - 1)
    return tuple(int(x) for x in n), int((hi - lo + 1).prod(1).sum())
