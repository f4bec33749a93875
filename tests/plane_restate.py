"""NumPy statement of the plane hypotheses, scoring, refit moments, box crop, RANSAC loop and four-way completion (csrc/plane.hip;
include/pb3d.h has the semantics), independent of the device code and written from the header.

Every float64 operation below is one NumPy elementwise operation, so it is rounded exactly where the header says the kernel rounds.
The summation order of the moments is icp_restate.ordered_sum (the header states the ICP step's order for them).  The host loop is
written again here; only plane_from_moments and the exact 0 / +-1 transforms of the completion are the library's own (host NumPy, with
CPU tests of their own)."""
import numpy as np

import icp_restate as ir
from pb3d.preprocess_helpers import plane_from_moments, quarter_turn_transforms


def hypotheses(P, triplets):
    """(K, 4): row k = (w / L, d) of the points a, b, c at triplets[k]; four NaNs where L is not a finite number above 0 or an index is
    outside [0, n)"""
    p = ir.widen(P)
    t = np.asarray(triplets, np.int64).reshape(-1, 3)
    n = len(p)
    ok = ((t >= 0) & (t < n)).all(1)
    out = np.full((len(t), 4), np.nan)
    ts = t[ok]
    if len(ts) == 0:
        return out
    a, b, c = p[ts[:, 0]], p[ts[:, 1]], p[ts[:, 2]]
    u, v = b - a, c - a
    with np.errstate(all="ignore"):
        wx = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
        wy = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
        wz = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
        L = np.sqrt((wx * wx + wy * wy) + wz * wz)
        nx, ny, nz = wx / L, wy / L, wz / L
        d = -((nx * a[:, 0] + ny * a[:, 1]) + nz * a[:, 2])
    rows = np.stack([nx, ny, nz, d], axis=1)
    rows[~(np.isfinite(L) & (L > 0.0))] = np.nan
    out[ok] = rows
    return out


def residuals(P, plane):
    """r = ((a*x + b*y) + c*z) + d of every widened point"""
    p = ir.widen(P)
    a, b, c, d = (float(v) for v in plane)
    with np.errstate(invalid="ignore", over="ignore"):
        return ((a * p[:, 0] + b * p[:, 1]) + c * p[:, 2]) + d


def inliers(P, plane, tau):
    with np.errstate(invalid="ignore"):
        return np.abs(residuals(P, plane)) <= tau                    # a NaN residual compares False


def score(P, planes, tau, chunk_elems=1 << 22):
    """(K,) int64: the number of points with fabs(r) <= tau per plane row"""
    p = ir.widen(P)
    planes = np.asarray(planes, np.float64).reshape(-1, 4)
    K, n = len(planes), len(p)
    counts = np.zeros(K, np.int64)
    if n == 0:
        return counts
    x, y, z = (np.ascontiguousarray(p[:, a])[None, :] for a in range(3))
    step = max(1, chunk_elems // n)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(0, K, step):
            q = planes[k:k + step]
            r = q[:, 0:1] * x
            r += q[:, 1:2] * y              # a*x + b*y
            r += q[:, 2:3] * z              # (a*x + b*y) + c*z
            r += q[:, 3:4]                  # ... + d
            np.abs(r, out=r)
            counts[k:k + step] = (r <= tau).sum(1)
    return counts


def moment_terms(P, plane, tau, pivot):
    """(used (n,) bool, terms (n, 11)): P = p - pivot (3), P.x*P.x, P.x*P.y, P.x*P.z, P.y*P.y, P.y*P.z, P.z*P.z, r, r*r; +0.0 in every term
    of a point that is not an inlier"""
    p = ir.widen(P)
    r = residuals(p, plane)
    with np.errstate(invalid="ignore"):
        used = np.abs(r) <= tau
    Q = p - np.asarray(pivot, np.float64)
    t = np.empty((len(p), 11), np.float64)
    t[:, 0:3] = Q
    for c, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        t[:, 3 + c] = Q[:, i] * Q[:, j]
    t[:, 9] = r
    t[:, 10] = r * r
    t[~used] = 0.0
    return used, t


def moments(P, plane, tau, pivot):
    """(count, sums (11,)) in the stated order"""
    if len(P) == 0:
        return 0, np.zeros(11, np.float64)
    used, t = moment_terms(P, plane, tau, pivot)
    return int(used.sum()), ir.ordered_sum(t)


def crop_mask(P, lo, hi):
    p = ir.widen(P)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    with np.errstate(invalid="ignore"):
        return ((lo <= p) & (p <= hi)).all(1)


def box_centre(P):
    p = ir.widen(P)
    return 0.5 * (p.min(0) + p.max(0))


def fit(P, tau, K=1024, seed=0, refits=2):
    """(normal, d, inlier_count, history) -- the loop of pb3d.preprocess_helpers.fit_plane_ransac_resident, restated"""
    n = len(P)
    triplets = np.random.default_rng(seed).integers(0, n, size=(K, 3), dtype=np.int64)
    planes = hypotheses(P, triplets)
    counts = score(P, planes, tau)
    best = 0
    for k in range(K):                                              # the highest count, ties to the lowest k
        if counts[k] > counts[best]:
            best = k
    if counts[best] < 3:
        raise ValueError(f"the best hypothesis has {int(counts[best])} inliers")
    normal, d, count = planes[best, :3].copy(), float(planes[best, 3]), int(counts[best])
    log = []
    if refits:
        pivot = box_centre(P)
        for _ in range(refits):
            c, sums = moments(P, (*normal, d), tau, pivot)
            if c < 3:
                raise ValueError(f"a refit found only {c} inliers")
            normal, d, _ = plane_from_moments(c, sums, pivot)
            log.append((c, sums, normal, d))
        count = int(inliers(P, (*normal, d), tau).sum())
    return normal, d, count, {"triplets": triplets, "planes": planes, "counts": counts, "best": best, "refits": log}


def completion(P, centre=None):
    """(4n, 3): copy q = transform of the widened cloud by q quarter turns about the Y-parallel axis through centre"""
    p = ir.widen(P)
    if centre is None:
        c = box_centre(p)
        centre = (c[0], c[2])
    return np.concatenate([ir.transform(p, T[:3]) for T in quarter_turn_transforms(centre)])


# ---- the constructed cloud of tests/test_plane_fit.py ------------------------------------------------------------------------------------
SLAB_NORMAL = np.array([0.2, -0.1, 0.97]) / np.linalg.norm([0.2, -0.1, 0.97])
SLAB_OFFSET = 0.3


def slab_case(dtype=np.float64):
    """3000 points on the plane SLAB_NORMAL . p + SLAB_OFFSET = 0 within +-1 (Gaussian thickness 0.002) and 2000 uniform outliers,
    shuffled"""
    rng = np.random.default_rng(0)
    nrm = SLAB_NORMAL
    e1 = np.cross(nrm, (0.0, 1.0, 0.0))
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(nrm, e1)
    uv = rng.uniform(-1.0, 1.0, size=(3000, 2))
    on = uv[:, :1] * e1 + uv[:, 1:] * e2 - SLAB_OFFSET * nrm + rng.normal(size=(3000, 1)) * 0.002 * nrm
    out = rng.uniform(-1.0, 1.0, size=(2000, 3))
    pts = np.concatenate([on, out])
    rng.shuffle(pts)
    return np.ascontiguousarray(pts.astype(dtype))
