"""NumPy statement of the ICP step and loop (csrc/icp.hip; include/pb3d.h has the semantics), independent of the device code.

Every float64 operation below is one NumPy elementwise operation, so it is rounded exactly where the header says the kernel rounds:
the transform, the squared distance, the terms, and the additions of the stated summation order.  The search is a brute-force argmin
over (d2, index) -- np.argmin returns the first, i.e. lowest, index of the minimum.  The host loop is written again here; only
best_fit_transform_from_sums is the library's own (it is host NumPy and has a test of its own)."""
import math

import numpy as np

from pb3d.preprocess_helpers import best_fit_transform_from_sums

LANE = np.arange(64)


def widen(P):
    return np.ascontiguousarray(np.asarray(P), dtype=np.float64).reshape(-1, 3)


def transform(P, T):
    """p_h = ((T[h,0]*x + T[h,1]*y) + T[h,2]*z) + T[h,3] on the widened points"""
    s = widen(P)
    T = np.asarray(T, np.float64)
    x, y, z = s[:, 0], s[:, 1], s[:, 2]
    return np.stack([((T[h, 0] * x + T[h, 1] * y) + T[h, 2] * z) + T[h, 3] for h in range(3)], axis=1)


def nearest(p, q, chunk_elems=1 << 17):
    """(j, d2): for every row of p the lowest index of the smallest d2 = (dx*dx + dy*dy) + dz*dz over the rows of q, and that d2
    (brute force, in chunks that stay in cache; the in-place operations round exactly as the expression does)"""
    n, m = len(p), len(q)
    j = np.zeros(n, np.int64)
    d2 = np.zeros(n, np.float64)
    step = max(1, chunk_elems // max(m, 1))
    qx, qy, qz = (np.ascontiguousarray(q[:, a])[None, :] for a in range(3))
    for a in range(0, n, step):
        c = p[a:a + step]
        dx, dy, dz = c[:, 0:1] - qx, c[:, 1:2] - qy, c[:, 2:3] - qz
        dx *= dx
        dy *= dy
        dx += dy            # dx*dx + dy*dy
        dz *= dz
        dx += dz            # (dx*dx + dy*dy) + dz*dz
        jj = np.argmin(dx, axis=1)
        j[a:a + step] = jj
        d2[a:a + step] = dx[np.arange(len(c)), jj]
    return j, d2


def terms(p, qj, d2, max_dist2, cp, cq):
    """(used (n,) bool, terms (n, 16)): P (3), Q (3), P_a * Q_b row-major (9), d2 (1); +0.0 in every term of an unused pair"""
    used = np.ones(len(p), bool) if max_dist2 < 0 else d2 <= max_dist2
    P = p - np.asarray(cp, np.float64)
    Q = qj - np.asarray(cq, np.float64)
    t = np.empty((len(p), 16), np.float64)
    t[:, 0:3] = P
    t[:, 3:6] = Q
    for a in range(3):
        for b in range(3):
            t[:, 6 + 3 * a + b] = P[:, a] * Q[:, b]
    t[:, 15] = d2
    t[~used] = 0.0
    return used, t


def _workgroups(v):
    """(k, 256, c) -> (k, c): per wave the butterfly v += v[lane ^ off] for off = 32 ... 1, then ((w0 + w1) + w2) + w3"""
    k, _, c = v.shape
    v = v.reshape(k, 4, 64, c)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, LANE ^ off, :]
    w = v[:, :, 0, :]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def _pad256(a):
    k = -(-len(a) // 256)
    out = np.zeros((k * 256,) + a.shape[1:], np.float64)
    out[:len(a)] = a
    return out, k


def ordered_sum(t):
    """the stated order over the rows of t (n, c): one partial row per 256 consecutive points, then thread t of one workgroup adds
    partial rows t, t + 256, ... in ascending order from +0.0, and the 256 values are reduced like a workgroup's"""
    t = np.asarray(t, np.float64)
    c = t.shape[1]
    padded, k = _pad256(t)
    rows = _workgroups(padded.reshape(k, 256, c))
    padded, k2 = _pad256(rows)
    acc = np.zeros((256, c), np.float64)
    for i in range(k2):
        acc = acc + padded[256 * i:256 * (i + 1)]
    return _workgroups(acc[None])[0]


def pairs(source, target, T, max_dist2, cp, cq):
    """(j, used, terms) of one step"""
    p = transform(source, np.asarray(T, np.float64)[:3])
    q = widen(target)
    j, d2 = nearest(p, q)
    used, t = terms(p, q[j], d2, max_dist2, cp, cq)
    return j, used, t


def step(source, target, T, max_dist2, cp, cq):
    """(count, sums (16,)) of one step"""
    if len(source) == 0:
        return 0, np.zeros(16, np.float64)
    if len(target) == 0:
        raise ValueError("the target is empty")
    _, used, t = pairs(source, target, T, max_dist2, cp, cq)
    return int(used.sum()), ordered_sum(t)


def box_centre(target):
    q = widen(target)
    return 0.5 * (q.min(0) + q.max(0))


def icp_align(source, target, max_iterations=50, tolerance=1e-9, max_distance=None, init=None):
    """(T, [(count, rmse)], [T per iteration]) -- the loop of pb3d.preprocess_helpers.icp_align_resident, restated"""
    md2 = -1.0 if max_distance is None else float(max_distance) * float(max_distance)
    T = np.eye(4)
    if init is not None:
        T[:3] = np.asarray(init, np.float64)[:3]
    c = box_centre(target)
    history, Ts, prev = [], [], None
    for _ in range(max_iterations):
        count, sums = step(source, target, T, md2, c, c)
        if count < 3:
            raise ValueError(f"only {count} point pairs")
        rmse = math.sqrt(sums[15] / count)
        T = best_fit_transform_from_sums(count, sums, c, c) @ T
        history.append((count, rmse))
        Ts.append(T)
        if prev is not None and abs(prev - rmse) < tolerance:
            break
        prev = rmse
    return T, history, Ts


# ---- the constructed clouds of tests/test_icp.py -------------------------------------------------------------------------------------
def rotation(axis, degrees):
    """Rodrigues' formula"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    th = math.radians(degrees)
    return np.eye(3) + math.sin(th) * K + (1.0 - math.cos(th)) * (K @ K)


def motion(degrees, extent):
    M = np.eye(4)
    M[:3, :3] = rotation((1.0, 2.0, 3.0), degrees)
    M[:3, 3] = np.array([0.02, -0.03, 0.01]) * extent
    return M


def moved_back(points, M):
    """the points moved by the inverse of M: icp_align of the result onto `points` recovers M"""
    return (np.asarray(points, np.float64) - M[:3, 3]) @ M[:3, :3]      # R^T (q - t), row form


def recovery_case(degrees=5.0, dtype=np.float64):
    """(source, target, M, extent): a two-blob cloud and every second point of it moved by the inverse of M"""
    rng = np.random.default_rng(0)
    target = np.concatenate([rng.normal(size=(2000, 3)) * (1.0, 0.6, 0.3), rng.normal(size=(1000, 3)) * 0.2 + (0.9, 0.5, -0.4)])
    extent = float((target.max(0) - target.min(0)).max())
    M = motion(degrees, extent)
    source = moved_back(target[::2], M)
    return np.ascontiguousarray(source.astype(dtype)), np.ascontiguousarray(target.astype(dtype)), M, extent
