"""NumPy restatements for tests/test_surface_metrics.py and tools/gen_golden_surface.py (reference utils/eval_helpers.py:198-245):
the brute-force k nearest neighbours under pb3d's tie rule, the two normal functions in scalar operations in NumPy's order, and the
per-vertex quantities of compute_surface_metrics in any float type (float64 in the tests, np.longdouble for the fixtures' yardstick).
Needs no device."""
import numpy as np


# ---- k nearest neighbours, ascending by (squared distance as computed, index) --------------------------------------------------------
def brute_knn(Q, R, k, chunk=512):
    """(d2, idx): for each row of Q the k smallest (dx*dx + dy*dy) + dz*dz over R in float64, ties by ascending index"""
    Q = np.asarray(Q, dtype=np.float64)
    R = np.asarray(R, dtype=np.float64)
    d2 = np.empty((len(Q), k), np.float64)
    idx = np.empty((len(Q), k), np.int64)
    for s in range(0, len(Q), chunk):
        q = Q[s:s + chunk]
        dx = q[:, None, 0] - R[None, :, 0]
        dy = q[:, None, 1] - R[None, :, 1]
        dz = q[:, None, 2] - R[None, :, 2]
        d = (dx * dx + dy * dy) + dz * dz
        o = np.argsort(d, axis=1, kind="stable")[:, :k]        # stable: equal d2 stay in index order
        idx[s:s + chunk] = o
        d2[s:s + chunk] = np.take_along_axis(d, o, axis=1)
    return d2, idx


def relative_gaps(V, k, chunk=512):
    """(d(k+1) - d(k)) / d(k) per vertex of the set V queried on itself, and d(k)"""
    d2, _ = brute_knn(V, V, k + 1, chunk)
    d = np.sqrt(d2)
    return (d[:, k] - d[:, k - 1]) / d[:, k - 1], d[:, k - 1]


# ---- normals in scalar operations, NumPy's order ---------------------------------------------------------------------------------------
def triangle_normals_scalar(vertices, faces):
    """compute_triangle_normals one operation at a time in the vertex dtype: each cross component one rounded product minus one
    rounded product; the norm sqrt((x*x + y*y) + z*z); 1e-8 rounded to the dtype"""
    T = vertices.dtype.type
    v0, v1, v2 = (vertices[faces[:, c]] for c in range(3))
    a, b = v1 - v0, v2 - v0
    n = np.empty_like(a)
    n[:, 0] = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
    n[:, 1] = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
    n[:, 2] = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    d = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]) + T(1e-8)
    return n / d[:, None]


def vertex_normals_scalar(vertices, faces):
    """compute_vertex_normals: per vertex the face normals added one by one in ascending (face, corner) order from 0, in the vertex
    dtype, then the same normalisation"""
    T = vertices.dtype.type
    tn = triangle_normals_scalar(vertices, faces)
    acc = [[T(0), T(0), T(0)] for _ in range(len(vertices))]
    for i in range(len(faces)):
        for j in range(3):
            a = acc[faces[i, j]]
            a[0] = a[0] + tn[i, 0]
            a[1] = a[1] + tn[i, 1]
            a[2] = a[2] + tn[i, 2]
    s = np.array(acc, dtype=vertices.dtype).reshape(len(vertices), 3)
    d = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]) + T(1e-8)
    return s / d[:, None]


# ---- per-vertex metrics in a float type F ----------------------------------------------------------------------------------------------
def jacobi3(A):
    """cyclic Jacobi on a stack of symmetric 3 x 3 matrices (n, 3, 3): (diagonal (n, 3), rotations' product (n, 3, 3))"""
    A = A.copy()
    F = A.dtype.type
    V = np.zeros_like(A)
    V[:, 0, 0] = V[:, 1, 1] = V[:, 2, 2] = 1
    for _ in range(12):
        moved = False
        for p, q in ((0, 1), (0, 2), (1, 2)):
            r = 3 - p - q
            apq = A[:, p, q].copy()
            act = np.abs(apq) > F(2.0) ** -70 * np.sqrt(np.abs(A[:, p, p] * A[:, q, q]))
            act &= apq != 0
            if act.any():
                moved = True
                with np.errstate(all="ignore"):
                    tau = (A[:, q, q] - A[:, p, p]) / (F(2) * apq)
                    t = np.where(tau < 0, F(-1), F(1)) / (np.abs(tau) + np.sqrt(F(1) + tau * tau))
                t = np.where(act, t, F(0))
                c = F(1) / np.sqrt(F(1) + t * t)
                s = t * c
                A[:, p, p] -= t * apq
                A[:, q, q] += t * apq
                arp, arq = A[:, r, p].copy(), A[:, r, q].copy()
                A[:, r, p] = A[:, p, r] = c * arp - s * arq
                A[:, r, q] = A[:, q, r] = s * arp + c * arq
                vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
                V[:, :, p] = c[:, None] * vp - s[:, None] * vq
                V[:, :, q] = s[:, None] * vp + c[:, None] * vq
            A[:, p, q] = A[:, q, p] = 0
        if not moved:
            break
    return np.stack([A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]], 1), V


def surface_metrics_restate(vertices, normals, idx, F=np.float64, frames=3):
    """The loop body of compute_surface_metrics (:221-239) for every vertex at once, every operation in the float type F on the given
    neighbour rows idx (n, k): (normal angle std in degrees, eigenvalues of the neighbours' covariance ascending (n, 3), |neighbour
    mean - vertex|).  The covariance is solved `frames` times, the second and later times in the eigenvector frame found so far, so
    the smallest eigenvalue keeps its relative accuracy."""
    P = np.asarray(vertices).astype(F)
    N = np.asarray(normals).astype(F)
    k = idx.shape[1]
    pi = F(4) * np.arctan(F(1))
    dot = np.clip((N[idx] * N[:, None, :]).sum(-1), F(-1), F(1))
    ang = np.arccos(dot) * (F(180) / pi)
    dev = ang - (ang.sum(1) / F(k))[:, None]
    std = np.sqrt((dev * dev).sum(1) / F(k))
    nb = P[idx]
    mean = nb.sum(1) / F(k)
    lap = mean - P
    curv = np.sqrt((lap * lap).sum(1))
    X = nb - mean[:, None, :]
    V = np.zeros((len(P), 3, 3), F)
    V[:, 0, 0] = V[:, 1, 1] = V[:, 2, 2] = 1
    for _ in range(frames):
        Y = X @ V
        lam, R = jacobi3(np.swapaxes(Y, 1, 2) @ Y)
        V = V @ R
    lam = np.sort(np.maximum(lam, F(0)), axis=1) / F(k - 1)
    return std, lam, curv


def split_hi_lo(x):
    """a longdouble array as two float64 arrays whose sum is x to ~2^-106"""
    hi = x.astype(np.float64)
    return hi, (x - hi.astype(x.dtype)).astype(np.float64)


def error_over_scale(got, hi, lo, scale):
    """max_i |got_i - (hi_i + lo_i)| / scale_i, evaluated in np.longdouble"""
    L = np.longdouble
    e = np.abs((np.asarray(got).astype(L) - hi.astype(L)) - lo.astype(L)) / scale.astype(L)
    return float(e.max())
