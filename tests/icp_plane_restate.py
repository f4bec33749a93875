"""NumPy statement of the point-cloud normals, the point-to-plane ICP step and its loop (csrc/normals.hip, csrc/icp.hip; include/pb3d.h
has the semantics), independent of the device code.  Built on icp_restate and icp_trim_restate: the transform, the brute-force search,
the candidate / k / tau rules and the stated summation order are theirs.  Every
float64 operation below is one NumPy elementwise operation, rounded where the header says the kernels round.  Only
plane_step_from_sums is the library's (host NumPy, with tests of its own)."""
import math

import numpy as np

import icp_restate as ir
import icp_trim_restate as tr
from pb3d.preprocess_helpers import plane_step_from_sums

PAIRS = ((0, 1, 2), (0, 2, 1), (1, 2, 0))       # (p, q, r) of the cyclic Jacobi sweep


# ---- normals -----------------------------------------------------------------------------------------------------------------------------
def jacobi3(A):
    """(diagonal (n, 3), V (n, 3, 3)) of the symmetric (n, 3, 3) stack A: the solve of csrc/jacobi3.h for all n at once.  A matrix whose
    sweep rotates nothing is finished; running the remaining sweeps on it changes nothing (every off-diagonal entry is then 0 and is
    skipped), so the loop needs no per-matrix break."""
    a = np.array(A, np.float64)
    n = len(a)
    v = np.zeros((n, 3, 3))
    v[:, 0, 0] = v[:, 1, 1] = v[:, 2, 2] = 1.0
    with np.errstate(all="ignore"):
        for _ in range(8):
            for p, q, r in PAIRS:
                apq = a[:, p, q].copy()
                nz = apq != 0.0
                rot = nz & (np.abs(apq) > 2.0 ** -70 * np.sqrt(np.abs(a[:, p, p] * a[:, q, q])))
                tau = (a[:, q, q] - a[:, p, p]) / (2.0 * apq)
                t = np.copysign(1.0, tau) / (np.abs(tau) + np.sqrt(1.0 + tau * tau))
                c = 1.0 / np.sqrt(1.0 + t * t)
                s = t * c
                app, aqq = a[:, p, p] - t * apq, a[:, q, q] + t * apq
                arp, arq = a[:, r, p].copy(), a[:, r, q].copy()
                nrp, nrq = c * arp - s * arq, s * arp + c * arq
                a[:, p, p] = np.where(rot, app, a[:, p, p])
                a[:, q, q] = np.where(rot, aqq, a[:, q, q])
                a[:, r, p] = a[:, p, r] = np.where(rot, nrp, arp)
                a[:, r, q] = a[:, q, r] = np.where(rot, nrq, arq)
                for x in range(3):
                    vp, vq = v[:, x, p].copy(), v[:, x, q].copy()
                    v[:, x, p] = np.where(rot, c * vp - s * vq, vp)
                    v[:, x, q] = np.where(rot, s * vp + c * vq, vq)
                a[:, p, q] = a[:, q, p] = np.where(nz, 0.0, apq)
    return np.stack([a[:, 0, 0], a[:, 1, 1], a[:, 2, 2]], axis=1), v


def covariance(points, idx):
    """(n, 3, 3): mean and the six sums in row order, each from +0.0, no divisor"""
    x = ir.widen(points)[np.asarray(idx)]       # (n, k, 3)
    n, k, _ = x.shape
    m = np.zeros((n, 3))
    for j in range(k):
        m = m + x[:, j]
    m = m / float(k)
    C = np.zeros((n, 3, 3))
    for j in range(k):
        y = x[:, j] - m
        for a in range(3):
            for b in range(a, 3):
                C[:, a, b] = C[:, a, b] + y[:, a] * y[:, b]
    for a in range(3):
        for b in range(a):
            C[:, a, b] = C[:, b, a]
    return C


def normals(points, idx, viewpoint=None):
    """(n, 3) float64 unit normals from the (n, k) neighbour rows idx"""
    pts = ir.widen(points)
    d, V = jacobi3(covariance(pts, idx))
    c1 = d[:, 1] < d[:, 0]
    d01 = np.where(c1, d[:, 1], d[:, 0])
    c2 = d[:, 2] < d01
    col = np.where(c2, 2, np.where(c1, 1, 0))
    nv = V[np.arange(len(pts)), :, col]
    length = np.sqrt((nv[:, 0] * nv[:, 0] + nv[:, 1] * nv[:, 1]) + nv[:, 2] * nv[:, 2])
    nv = nv / length[:, None]
    if viewpoint is None:
        a = np.abs(nv)
        b1 = a[:, 1] > a[:, 0]
        b2 = a[:, 2] > np.where(b1, a[:, 1], a[:, 0])
        lead = np.where(b2, nv[:, 2], np.where(b1, nv[:, 1], nv[:, 0]))
        flip = lead < 0.0
    else:
        v = np.asarray(viewpoint, np.float64)
        flip = ((v[0] - pts[:, 0]) * nv[:, 0] + (v[1] - pts[:, 1]) * nv[:, 1]) + (v[2] - pts[:, 2]) * nv[:, 2] < 0.0
    return np.where(flip[:, None], -nv, nv)


def knn_rows(points, k, chunk=256):
    """(n, k) int64: for every point the k points with the smallest (d2, index), d2 = (dx*dx + dy*dy) + dz*dz, in that order (the
    rows of the exact search on the set itself).  Brute force; only the entries up to the k-th smallest d2 of a row are sorted."""
    pts = ir.widen(points)
    rows = np.empty((len(pts), k), np.int64)
    for s in range(0, len(pts), chunk):
        q = pts[s:s + chunk]
        dx, dy, dz = (q[:, None, a] - pts[None, :, a] for a in range(3))
        d = (dx * dx + dy * dy) + dz * dz
        kth = np.partition(d, k - 1, axis=1)[:, k - 1]
        for i in range(len(q)):
            cand = np.flatnonzero(d[i] <= kth[i])                               # ascending index
            rows[s + i] = cand[np.argsort(d[i, cand], kind="stable")][:k]       # stable: equal d2 stay in index order
    return rows


def estimate_normals(points, k, viewpoint=None):
    return normals(points, knn_rows(points, k), viewpoint)


# ---- the step --------------------------------------------------------------------------------------------------------------------------
def prepare(source, target, tnormals, T, c):
    """(d2, valid, terms (n, 29)) of every pair before the gate and the trim"""
    p = ir.transform(source, np.asarray(T, np.float64)[:3])
    q = ir.widen(target)
    j, d2, valid = tr.candidates(p, q)
    nrm = np.asarray(tnormals, np.float64)[j]
    qj = q[j]
    dx, dy, dz = p[:, 0] - qj[:, 0], p[:, 1] - qj[:, 1], p[:, 2] - qj[:, 2]
    P = p - np.asarray(c, np.float64)
    n0, n1, n2 = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    r = (dx * n0 + dy * n1) + dz * n2
    J = [P[:, 1] * n2 - P[:, 2] * n1, P[:, 2] * n0 - P[:, 0] * n2, P[:, 0] * n1 - P[:, 1] * n0, n0, n1, n2]
    t = np.empty((len(p), 29), np.float64)
    col = 0
    for u in range(6):
        for v in range(u, 6):
            t[:, col] = J[u] * J[v]
            col += 1
    for u in range(6):
        t[:, 21 + u] = J[u] * r
    t[:, 27] = r * r
    t[:, 28] = d2
    return d2, valid, t


def finish(prepared, max_dist2, rho):
    """(used, terms, m, tau).  rho < 0: untrimmed -- a pair is used when it passes the gate, m = 0 and tau = +0.0; otherwise the
    candidate, k and tau rules of the trimmed step (icp_trim_restate.finish)"""
    if rho >= 0:
        return tr.finish(prepared, max_dist2, rho)
    d2, valid, t = prepared
    used = valid & (np.ones(len(d2), bool) if max_dist2 < 0 else d2 <= max_dist2)
    t = t.copy()
    t[~used] = 0.0
    return used, t, 0, np.float64(0.0)


def step(source, target, tnormals, T, max_dist2, rho, c):
    """(count, sums (29,), m, tau) of one point-to-plane step; rho < 0 or None: untrimmed"""
    rho = -1.0 if rho is None else float(rho)
    if len(source) == 0:
        return 0, np.zeros(29, np.float64), 0, np.float64(0.0)
    if len(target) == 0:
        raise ValueError("the target is empty")
    return tr.result(*finish(prepare(source, target, tnormals, T, c), max_dist2, rho))


def words(result):
    """the 32 words of d_out as uint64"""
    count, sums, m, tau = result
    w = np.empty(32, np.uint64)
    w[0] = count
    w[1:30] = np.ascontiguousarray(sums, np.float64).view(np.uint64)
    w[30] = m
    w[31] = np.float64(tau).view(np.uint64)
    return w


# ---- the loop ------------------------------------------------------------------------------------------------------------------------
def icp_align(source, target, max_iterations=50, tolerance=1e-9, max_distance=None, init=None, trim_fraction=None, target_normals=None,
              normals_k=20):
    """(T, [(count, rmse_plane, rmse_point, rank[, m, tau])], [T per iteration]) -- the point-to-plane path of
    pb3d.preprocess_helpers.icp_align_resident, restated"""
    md2 = -1.0 if max_distance is None else float(max_distance) * float(max_distance)
    T = np.eye(4)
    if init is not None:
        T[:3] = np.asarray(init, np.float64)[:3]
    nrm = estimate_normals(target, normals_k) if target_normals is None else np.asarray(target_normals, np.float64)
    c = ir.box_centre(target)
    history, Ts, prev = [], [], None
    for _ in range(max_iterations):
        count, sums, m, tau = step(source, target, nrm, T, md2, trim_fraction, c)
        if count < 6:
            raise ValueError(f"only {count} point pairs")
        rmse_plane, rmse_point = math.sqrt(sums[27] / count), math.sqrt(sums[28] / count)
        M, rank = plane_step_from_sums(count, sums, c)
        T = M @ T
        entry = (count, rmse_plane, rmse_point, rank)
        history.append(entry if trim_fraction is None else entry + (m, float(tau)))
        Ts.append(T)
        if prev is not None and abs(prev - rmse_plane) < tolerance:
            break
        prev = rmse_plane
    return T, history, Ts


# ---- the constructed clouds of tests/test_icp_plane.py -------------------------------------------------------------------------------
def sheet(uv):
    """points of a gently curved sheet over the (u, v) rows, offset from the origin, and its unit normals there"""
    u, v = uv[:, 0], uv[:, 1]
    z = 0.2 * u * u - 0.15 * v * v + 0.1 * u * v + 0.03 * np.sin(3.0 * u) * np.cos(2.0 * v)
    zu = 0.4 * u + 0.1 * v + 0.09 * np.cos(3.0 * u) * np.cos(2.0 * v)
    zv = -0.3 * v + 0.1 * u - 0.06 * np.sin(3.0 * u) * np.sin(2.0 * v)
    n = np.stack([-zu, -zv, np.ones_like(u)], axis=1)
    n /= np.linalg.norm(n, axis=1)[:, None]
    return np.stack([u, v, z], axis=1) + SHEET_CENTRE, n


SHEET_CENTRE = np.array([3.0, -2.0, 5.0])


def lattice_sheet(nu=40, nv=40, jitter=0.1, seed=9):
    """nu x nv points of the sheet over a lattice whose gaps alternate (0.8, 1.2 along u; 0.9, 1.3 along v), each moved by up to `jitter`
    of the mean gap: every point has ONE nearest neighbour along each axis, so even three neighbours span a plane well"""
    rng = np.random.default_rng(seed)
    axes = []
    for n, (g0, g1) in ((nu, (0.8, 1.2)), (nv, (0.9, 1.3))):
        a = np.concatenate([[0.0], np.cumsum(np.where(np.arange(n - 1) % 2 == 0, g0, g1))])
        axes.append(2.0 * a / a[-1] - 1.0)
    uv = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 2)
    h = 2.0 / (nu - 1)
    return sheet(uv + rng.uniform(-jitter * h, jitter * h, uv.shape))[0]


def sheet_motion():
    """4 degrees about the axis (1, 2, 3) through the sheet's centre, then the shift (0.05, -0.04, 0.03)"""
    M = np.eye(4)
    M[:3, :3] = ir.rotation((1.0, 2.0, 3.0), 4.0)
    M[:3, 3] = np.array([0.05, -0.04, 0.03]) + SHEET_CENTRE - M[:3, :3] @ SHEET_CENTRE
    return M


def sheet_case(clutter=0):
    """(source, target, target normals, M): 4 000 target points of the sheet; 1 000 OTHER points of its inner part, moved by the inverse of M
    (icp_align of the source onto the target recovers M), and `clutter` points well off the sheet appended to them"""
    rng = np.random.default_rng(5)
    target, nrm = sheet(rng.uniform(-1.0, 1.0, (4000, 2)))
    inner, _ = sheet(rng.uniform(-0.75, 0.75, (1000, 2)))
    M = sheet_motion()
    if clutter:
        inner = np.concatenate([inner, rng.normal(size=(clutter, 3)) * 0.2 + SHEET_CENTRE + (0.0, 0.0, 2.5)])
    return np.ascontiguousarray(ir.moved_back(inner, M)), np.ascontiguousarray(target), np.ascontiguousarray(nrm), M


def flat_case():
    """(source, target, unit normal, offset): 3 000 target points of a tilted plane n . x = offset and 800 other points of it, moved by 2 degrees
    and a shift"""
    rng = np.random.default_rng(6)
    R = ir.rotation((1.0, -1.0, 0.5), 25.0)
    e1, e2, n = R[:, 0], R[:, 1], R[:, 2]
    o = np.array([1.0, 2.0, -0.5])
    ab = rng.uniform(-1.0, 1.0, (3000, 2))
    target = o + ab[:, :1] * e1 + ab[:, 1:] * e2
    ab = rng.uniform(-0.7, 0.7, (800, 2))
    inner = o + ab[:, :1] * e1 + ab[:, 1:] * e2
    M = np.eye(4)
    M[:3, :3] = ir.rotation((2.0, 1.0, -1.0), 2.0)
    M[:3, 3] = (0.02, 0.01, -0.03)
    return np.ascontiguousarray(ir.moved_back(inner, M)), np.ascontiguousarray(target), n, float(n @ o)
