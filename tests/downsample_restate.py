"""The rules of voxel_downsample (include/pb3d.h: ORIGIN, CELL, RANGE, VOXELS, INDEX, CENTROID, FIRST) restated in NumPy, a plain
Python loop that the restatement itself is held to, and the constructed clouds of tests/test_voxel_downsample.py.

restate(): the cells as stated, np.unique on the packed key renumbered by first appearance, sums by np.add.at (which adds in input
order, one rounded addition each) and one division.  loop() does the same with a dict and Python floats, point by point."""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CELLS = 2 ** 21


def sfm_cloud():
    with np.load(os.path.join(GOLDEN, "inter_sfm20k.npz"), allow_pickle=False) as z:
        return z["sfm"]


def _widen(points):
    a = np.asarray(points)
    dtype = np.float32 if a.dtype == np.float32 else np.float64
    return np.ascontiguousarray(a, dtype=dtype), np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 3)


def cells(P64, voxel_size, origin=None):
    """(n, 3) int64 cells; ValueError where RANGE fails"""
    vs = np.float64(voxel_size)
    if origin is None:
        o = P64.min(axis=0) - np.float64(0.5) * vs
    else:
        o = np.asarray(origin, np.float64)
    c = np.floor((P64 - o) / vs)
    if len(c) and not ((c >= 0) & (c < CELLS)).all():
        raise ValueError("voxel_size / origin: a cell outside [0, 2^21)")
    return c.astype(np.int64)


def restate(points, voxel_size, origin=None, reduce="centroid"):
    """(out, index intp, inverse intp, counts int64)"""
    P, P64 = _widen(points)
    n = len(P64)
    if n == 0:
        return P.reshape(0, 3).copy(), np.zeros(0, np.intp), np.zeros(0, np.intp), np.zeros(0, np.int64)
    c = cells(P64, voxel_size, origin)
    key = (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
    _, first, inv, counts = np.unique(key, return_index=True, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    order = np.argsort(first, kind="stable")              # sorted-key number -> first-appearance number
    renumber = np.empty(len(order), np.intp)
    renumber[order] = np.arange(len(order))
    index = first[order].astype(np.intp)
    inverse = renumber[inv].astype(np.intp)
    counts = counts[order].astype(np.int64)
    if reduce == "first":
        return P[index].copy(), index, inverse, counts
    assert reduce == "centroid"
    sums = np.zeros((len(index), 3), np.float64)
    np.add.at(sums, inverse, P64)
    return (sums / counts[:, None].astype(np.float64)).astype(P.dtype), index, inverse, counts


def loop(points, voxel_size, origin=None, reduce="centroid"):
    """the same result point by point: Python floats are float64, and every operation below rounds once"""
    P, P64 = _widen(points)
    n = len(P64)
    vs = float(voxel_size)
    o = [float(v) for v in origin] if origin is not None else [float(P64[:, a].min()) - 0.5 * vs for a in range(3)] if n else [0.0] * 3
    number, index, inverse, counts, sums = {}, [], [], [], []
    for i, p in enumerate(P64.tolist()):
        c = (math.floor((p[0] - o[0]) / vs), math.floor((p[1] - o[1]) / vs), math.floor((p[2] - o[2]) / vs))
        if not all(0 <= v < CELLS for v in c):
            raise ValueError("voxel_size / origin: a cell outside [0, 2^21)")
        v = number.setdefault(c, len(number))
        if v == len(index):
            index.append(i); counts.append(0); sums.append([0.0, 0.0, 0.0])
        inverse.append(v)
        counts[v] += 1
        for a in range(3):
            sums[v][a] = sums[v][a] + p[a]
    index, inverse, counts = np.array(index, np.intp), np.array(inverse, np.intp), np.array(counts, np.int64)
    if reduce == "first":
        return P[index].reshape(-1, 3).copy(), index, inverse, counts
    out = np.array([[s[a] / float(k) for a in range(3)] for s, k in zip(sums, counts)], np.float64).reshape(-1, 3)
    return out.astype(P.dtype), index, inverse, counts


# ---- constructed clouds: name -> (points float64, voxel_size, origin or None) ----------------------------------------------------------
def face_lattice():
    g = np.arange(8) * 0.25
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def nextafter_points(axis):
    """nextafter(k * 0.1, -inf), k = 1 .. 199, on one axis: just below a voxel face of voxel_size 0.1, origin 0"""
    p = np.zeros((199, 3))
    p[:, axis] = np.nextafter(np.arange(1, 200) * 0.1, -np.inf)
    return p


def key_width_cells():
    top = CELLS - 1
    c = [(top, 0, 0), (0, top, 0), (0, 0, top), (0, 0, 0)]
    for a in range(3):                                     # pairs that differ only in bit 20 of one axis
        lo, hi = [5, 6, 7], [5, 6, 7]
        hi[a] += 1 << 20
        c += [tuple(lo), tuple(hi)]
    return np.array(sorted(set(c), key=c.index), np.int64)


def duplicated(n, seed):
    """n points, about half of them an earlier point moved by less than 0.01"""
    rng = np.random.default_rng(seed)
    base = rng.random((n, 3)) * 40.0
    src = np.where(rng.random(n) < 0.5, (rng.random(n) * np.arange(n)).astype(np.int64), np.arange(n))      # itself, or an earlier point
    return base[src] + rng.random((n, 3)) * 0.01 * (src != np.arange(n))[:, None]


def all_distinct(layout, n=2 ** 17 + 3):
    p = np.full((n, 3), 0.5)
    if layout == "cx":
        p[:, 0] += np.arange(n)
    elif layout == "cz":
        p[:, 2] += np.arange(n)
    else:
        rng = np.random.default_rng(11)
        flat = rng.choice(128 ** 3, n, replace=False)
        p += np.stack([flat // (128 * 128), flat // 128 % 128, flat % 128], -1)
    return p


RUN_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 193)       # voxel populations on both sides of the centroid kernel's 64-row rounds


def run_boundaries(seed=7):
    """772 points: voxel k (cell k on x, voxel_size 1e5, origin 0) holds RUN_LENGTHS[k] of them, interleaved by a seeded permutation.
    Inside a voxel the offsets span seven decades, so the order of the additions shows in the centroid's bits."""
    rng = np.random.default_rng(seed)
    voxel = np.repeat(np.arange(len(RUN_LENGTHS)), RUN_LENGTHS)
    p = rng.random((len(voxel), 3)) * 10.0 ** rng.integers(-3, 4, (len(voxel), 3))
    p[:, 0] += voxel * 1e5
    return p[rng.permutation(len(voxel))]


def constructed_cases():
    cases = {"faces/lattice": (face_lattice(), 0.5, (0.0, 0.0, 0.0))}
    for a in range(3):
        cases[f"faces/nextafter/{'xyz'[a]}"] = (nextafter_points(a), 0.1, (0.0, 0.0, 0.0))
    cases["keywidth"] = (key_width_cells() + 0.5, 1.0, (0.0, 0.0, 0.0))
    for n in (1, 2, 255, 256, 257, 65537):
        cases[f"seams/{n}"] = (duplicated(n, n), 0.25, None)
    rng = np.random.default_rng(5)
    cases["onevoxel/70001"] = (rng.random((70001, 3)) * 3.0 + 10.0, 8.0, (8.0, 8.0, 8.0))
    for layout in ("cx", "cz", "random"):
        cases[f"distinct/{layout}"] = (all_distinct(layout), 1.0, (0.0, 0.0, 0.0))
    cases["runs/boundaries"] = (run_boundaries(), 1e5, (0.0, 0.0, 0.0))
    return cases
