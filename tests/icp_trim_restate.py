"""NumPy statement of the trimmed ICP step, its loop and the totalOrder selection (csrc/icp.hip, csrc/select.hip; include/pb3d.h has
the semantics), independent of the device code.  Built on icp_restate: the transform, the brute-force search, the 16 terms and the
stated summation order are its own.  Only best_fit_similarity_from_sums is the library's (host NumPy, with a test of its own)."""
import math

import numpy as np

import icp_restate as ir
from pb3d.preprocess_helpers import best_fit_similarity_from_sums

SENTINEL = np.uint64(0x7FF8000000000000)        # what a pair that is no candidate enters the selection as


# ---- the selection ---------------------------------------------------------------------------------------------------------------------
def order_keys(values):
    """key = bits ^ (bits >> 63 ? ~0 : 1 << 63): unsigned order of the keys = totalOrder of the float64 values"""
    b = np.ascontiguousarray(values, dtype=np.float64).reshape(-1).view(np.uint64)
    flip = np.where(b >> np.uint64(63) != 0, np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(1) << np.uint64(63))
    return b ^ flip


def kth(values, rank):
    """the element at 0-based position `rank` in totalOrder, with its own bytes (a float64 scalar)"""
    v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
    if not 0 <= rank < len(v):
        raise ValueError("rank out of range")
    k = np.sort(order_keys(v))[rank:rank + 1]
    back = np.where(k >> np.uint64(63) != 0, k ^ (np.uint64(1) << np.uint64(63)), ~k)
    return back.view(np.float64)[0]


# ---- the step --------------------------------------------------------------------------------------------------------------------------
def candidates(p, q):
    """(j, d2, valid): the search of icp_restate; a moved point that is not finite has no nearest point"""
    valid = np.isfinite(p).all(axis=1)
    j = np.zeros(len(p), np.int64)
    d2 = np.zeros(len(p), np.float64)
    if valid.any():
        j[valid], d2[valid] = ir.nearest(p[valid], q)
    return j, d2, valid


def keys(d2, cand):
    """the float64 list the device selects from: d2 of a candidate, the sentinel NaN of any other pair"""
    k = np.full(len(d2), SENTINEL, np.uint64)
    k[cand] = d2[cand].view(np.uint64)
    return k.view(np.float64)


def trim_k(m, rho):
    """k = (rho >= 1.0) ? m : min(m, ceil(rho * (double)m)): one rounded product, then ceil"""
    return m if rho >= 1.0 else min(m, int(math.ceil(rho * float(m))))


def prepare(source, target, T, cp, cq):
    """(d2, valid, terms (n, 17)) of every pair before the gate and the trim: what the steps of one (source, target, T) share"""
    p = ir.transform(source, np.asarray(T, np.float64)[:3])
    q = ir.widen(target)
    j, d2, valid = candidates(p, q)
    P = p - np.asarray(cp, np.float64)
    Q = q[j] - np.asarray(cq, np.float64)
    t = np.empty((len(p), 17), np.float64)
    t[:, 0:3] = P
    t[:, 3:6] = Q
    for a in range(3):
        for b in range(3):
            t[:, 6 + 3 * a + b] = P[:, a] * Q[:, b]
    t[:, 15] = d2
    t[:, 16] = (P[:, 0] * P[:, 0] + P[:, 1] * P[:, 1]) + P[:, 2] * P[:, 2]
    return d2, valid, t


def finish(prepared, max_dist2, rho):
    """(used (n,) bool, terms (n, 17), m, tau): the gate, k, tau and the used pairs; +0.0 in every term of an unused pair"""
    d2, valid, t = prepared
    cand = valid & (np.ones(len(d2), bool) if max_dist2 < 0 else d2 <= max_dist2)
    m = int(cand.sum())
    k = trim_k(m, rho)
    tau = np.float64(0.0) if m == 0 else np.sort(d2[cand])[k - 1]
    if m:
        assert kth(keys(d2, cand), k - 1).tobytes() == tau.tobytes()       # the selection the device runs names the same element
    used = cand & (d2 <= tau)
    t = t.copy()
    t[~used] = 0.0
    return used, t, m, tau


def pairs(source, target, T, max_dist2, rho, cp, cq):
    """(used, terms, m, tau) of one trimmed step"""
    return finish(prepare(source, target, T, cp, cq), max_dist2, rho)


def result(used, t, m, tau):
    """(count, sums (17,), m, tau) in the stated summation order"""
    return int(used.sum()), ir.ordered_sum(t), m, tau


def step(source, target, T, max_dist2, rho, cp, cq):
    """(count, sums (17,), m, tau) of one trimmed step"""
    if len(source) == 0:
        return 0, np.zeros(17, np.float64), 0, np.float64(0.0)
    if len(target) == 0:
        raise ValueError("the target is empty")
    with np.errstate(over="ignore", invalid="ignore"):
        return result(*pairs(source, target, T, max_dist2, rho, cp, cq))


def words(result):
    """the 20 words of d_out as uint64"""
    count, sums, m, tau = result
    w = np.empty(20, np.uint64)
    w[0] = count
    w[1:18] = np.ascontiguousarray(sums, np.float64).view(np.uint64)
    w[18] = m
    w[19] = np.float64(tau).view(np.uint64)
    return w


# ---- the loop ------------------------------------------------------------------------------------------------------------------------
def icp_align(source, target, max_iterations=50, tolerance=1e-9, max_distance=None, init=None, trim_fraction=None, with_scale=False):
    """(T, [(count, rmse, m, tau)], [T per iteration]) -- the trimmed path of pb3d.preprocess_helpers.icp_align_resident, restated"""
    md2 = -1.0 if max_distance is None else float(max_distance) * float(max_distance)
    rho = 1.0 if trim_fraction is None else float(trim_fraction)
    T = np.eye(4)
    if init is not None:
        T[:3] = np.asarray(init, np.float64)[:3]
    c = ir.box_centre(target)
    history, Ts, prev = [], [], None
    for _ in range(max_iterations):
        count, sums, m, tau = step(source, target, T, md2, rho, c, c)
        if count < 3:
            raise ValueError(f"only {count} point pairs")
        rmse = math.sqrt(sums[15] / count)
        T = best_fit_similarity_from_sums(count, sums, c, c, with_scale) @ T
        history.append((count, rmse, m, float(tau)))
        Ts.append(T)
        if prev is not None and abs(prev - rmse) < tolerance:
            break
        prev = rmse
    return T, history, Ts


# ---- the constructed clouds of tests/test_icp_trimmed.py ----------------------------------------------------------------------------
def clutter_case():
    """case X: the 5-degree recovery case with 500 clutter points well outside the target appended to its 1 500 source points"""
    s, t, M, extent = ir.recovery_case(5.0)
    rng = np.random.default_rng(1)
    clutter = rng.normal(size=(500, 3)) * 0.3 + (t.max(0) + 1.5 * extent * np.array([1.0, 0.5, -0.7]))
    return np.ascontiguousarray(np.concatenate([s, ir.moved_back(clutter, M)])), t, M, extent


def scale_case(scale, clutter=False):
    """(source, target, M, extent, scale): the source of the recovery case (of case X) shrunk by 1 / scale about the origin, so that
    the similarity that registers it is  q = scale * R0 s + t0"""
    s, t, M, extent = clutter_case() if clutter else ir.recovery_case(5.0)
    return np.ascontiguousarray(s / scale), t, M, extent, scale
