"""NumPy statement of the point-to-mesh distance (csrc/meshdist.hip; include/pb3d.h has the semantics), independent of the device code
and written from the header: Ericson's closest point on a triangle (Real-Time Collision Detection 5.1.5) in its order of tests, a
degenerate face by its three segments, every product / sum / quotient one rounded operation, and a brute force over ALL faces with
ties to the lowest face index.

Coordinates travel as tuples of three arrays (x, y, z) that broadcast against each other, so the same text serves a scalar, a
(queries, faces) block and np.longdouble (closest(..., dt=np.longdouble): the accuracy yardstick)."""
import numpy as np


def _dot(x, y):
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]


def _sub(x, y):
    return (x[0] - y[0], x[1] - y[1], x[2] - y[2])


def _div0(x, y):
    """x / y, 0 where y == 0"""
    zero = y == 0
    return np.where(zero, 0, x / np.where(zero, 1, y))


def _d2(q, cp):
    d = _sub(q, cp)
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def segment_closest(q, s0, s1):
    """(d2, cp) of the segment s0 -> s1"""
    e = _sub(s1, s0)
    dd = _dot(e, e)
    t = _dot(_sub(q, s0), e)
    t = np.where(dd == 0, 0, np.minimum(np.maximum(_div0(t, dd), 0), 1))
    cp = tuple(s0[k] + e[k] * t for k in range(3))
    return _d2(q, cp), cp


def degenerate(a, b, c):
    """dot(n, n) == 0 for n = cross(b - a, c - a)"""
    ab, ac = _sub(b, a), _sub(c, a)
    n = (ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0])
    return _dot(n, n) == 0


def degenerate_closest(q, a, b, c):
    """the best of AB, BC, CA in that order, a later segment only if strictly nearer"""
    best, cp = segment_closest(q, a, b)
    for s0, s1 in ((b, c), (c, a)):
        d, alt = segment_closest(q, s0, s1)
        win = d < best
        best = np.where(win, d, best)
        cp = tuple(np.where(win, alt[k], cp[k]) for k in range(3))
    return best, cp


def region_closest(q, a, b, c):
    """(d2, cp) by the region walk; meaningless (but harmless) for a degenerate face"""
    ab, ac = _sub(b, a), _sub(c, a)
    ap = _sub(q, a)
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    bp = _sub(q, b)
    d3, d4 = _dot(ab, bp), _dot(ac, bp)
    vc = d1 * d4 - d3 * d2
    cq = _sub(q, c)
    d5, d6 = _dot(ab, cq), _dot(ac, cq)
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    u1, u2 = d4 - d3, d5 - d6
    conds = [(d1 <= 0) & (d2 <= 0),
             (d3 >= 0) & (d4 <= d3),
             (vc <= 0) & (d1 >= 0) & (d3 <= 0),
             (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0),
             (va <= 0) & (u1 >= 0) & (u2 >= 0)]
    v_ab = _div0(d1, d1 - d3)
    w_ac = _div0(d2, d2 - d6)
    w_bc = _div0(u1, u1 + u2)
    den = _div0(1, (va + vb) + vc)
    v, w = vb * den, vc * den
    bc = _sub(c, b)
    cp = []
    for k in range(3):
        shape = np.broadcast(d1, a[k]).shape
        cands = [a[k], b[k], a[k] + ab[k] * v_ab, c[k], a[k] + ac[k] * w_ac, b[k] + bc[k] * w_bc]
        cp.append(np.select(conds, [np.broadcast_to(x, shape) for x in cands], (a[k] + ab[k] * v) + ac[k] * w))
    cp = tuple(cp)
    return _d2(q, cp), cp


def closest(q, a, b, c, dt=np.float64):
    """(d2, cp) of the points q against the faces (a, b, c); each a tuple of three broadcastable arrays (or scalars)"""
    q, a, b, c = (tuple(np.asarray(x, dtype=dt) for x in p) for p in (q, a, b, c))
    with np.errstate(all="ignore"):
        d2, cp = region_closest(q, a, b, c)
        deg = degenerate(a, b, c)
        if np.any(deg):
            dd, dcp = degenerate_closest(q, a, b, c)
            d2 = np.where(deg, dd, d2)
            cp = tuple(np.where(deg, dcp[k], cp[k]) for k in range(3))
    return d2, cp


def closest_scalar(q, a, b, c):
    """the same statement one Python float at a time (the order the kernel follows): (d2, (x, y, z))"""
    q, a, b, c = ([float(v) for v in p] for p in (q, a, b, c))

    def dot(x, y):
        return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]

    def sub(x, y):
        return [x[0] - y[0], x[1] - y[1], x[2] - y[2]]

    def div0(x, y):
        return 0.0 if y == 0 else x / y

    def d2of(cp):
        d = sub(q, cp)
        return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]

    def segment(s0, s1):
        e = sub(s1, s0)
        dd, t = dot(e, e), dot(sub(q, s0), e)
        t = 0.0 if dd == 0 else min(max(t / dd, 0.0), 1.0)
        cp = [s0[k] + e[k] * t for k in range(3)]
        return d2of(cp), cp

    ab, ac = sub(b, a), sub(c, a)
    n = [ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]]
    if dot(n, n) == 0:
        best, cp = segment(a, b)
        for s0, s1 in ((b, c), (c, a)):
            d, alt = segment(s0, s1)
            if d < best:
                best, cp = d, alt
        return best, tuple(cp)
    ap = sub(q, a)
    d1, d2 = dot(ab, ap), dot(ac, ap)
    if d1 <= 0 and d2 <= 0:
        return d2of(a), tuple(a)
    bp = sub(q, b)
    d3, d4 = dot(ab, bp), dot(ac, bp)
    if d3 >= 0 and d4 <= d3:
        return d2of(b), tuple(b)
    vc = d1 * d4 - d3 * d2
    if vc <= 0 and d1 >= 0 and d3 <= 0:
        v = div0(d1, d1 - d3)
        cp = [a[k] + ab[k] * v for k in range(3)]
        return d2of(cp), tuple(cp)
    cq = sub(q, c)
    d5, d6 = dot(ab, cq), dot(ac, cq)
    if d6 >= 0 and d5 <= d6:
        return d2of(c), tuple(c)
    vb = d5 * d2 - d1 * d6
    if vb <= 0 and d2 >= 0 and d6 <= 0:
        w = div0(d2, d2 - d6)
        cp = [a[k] + ac[k] * w for k in range(3)]
        return d2of(cp), tuple(cp)
    va = d3 * d6 - d5 * d4
    u1, u2 = d4 - d3, d5 - d6
    if va <= 0 and u1 >= 0 and u2 >= 0:
        w = div0(u1, u1 + u2)
        cp = [b[k] + (c[k] - b[k]) * w for k in range(3)]
        return d2of(cp), tuple(cp)
    den = div0(1.0, (va + vb) + vc)
    v, w = vb * den, vc * den
    cp = [(a[k] + ab[k] * v) + ac[k] * w for k in range(3)]
    return d2of(cp), tuple(cp)


def _columns(P):
    return tuple(np.ascontiguousarray(P[:, k]) for k in range(3))


def corners(vertices, faces):
    """(a, b, c) as tuples of three (nf,) float64 arrays; negative indices wrap as NumPy's do"""
    v = np.asarray(vertices).astype(np.float64)
    f = np.asarray(faces).astype(np.int64)
    return tuple(_columns(v[f[:, j]]) for j in range(3))


def brute_force(Q, vertices, faces, chunk=None):
    """(dist, face int32, closest (nq, 3)) of the queries against ALL faces: the minimum of d2 as computed, the lowest face on a tie
    (np.argmin returns the first minimum), sqrt at the end.  Vectorised over (queries, faces) blocks of about 2^18 pairs."""
    Q = np.asarray(Q).astype(np.float64)
    a, b, c = corners(vertices, faces)
    nf = len(a[0])
    if chunk is None:
        chunk = max(1, (1 << 18) // nf)
    face = np.empty(len(Q), np.int32)
    d2 = np.empty(len(Q), np.float64)
    cp = np.empty((len(Q), 3), np.float64)
    for s in range(0, len(Q), chunk):
        q = tuple(Q[s:s + chunk, k][:, None] for k in range(3))
        dd, cc = closest(q, tuple(x[None, :] for x in a), tuple(x[None, :] for x in b), tuple(x[None, :] for x in c))
        j = np.argmin(dd, axis=1)
        rows = np.arange(len(j))
        face[s:s + chunk] = j
        d2[s:s + chunk] = dd[rows, j]
        for k in range(3):
            cp[s:s + chunk, k] = np.broadcast_to(cc[k], dd.shape)[rows, j]
    return np.sqrt(d2), face, cp


def brute_force_scalar(Q, vertices, faces):
    """brute_force one pair at a time"""
    v = np.asarray(vertices).astype(np.float64)
    f = np.asarray(faces).astype(np.int64)
    Q = np.asarray(Q).astype(np.float64)
    dist, face, cp = np.empty(len(Q)), np.empty(len(Q), np.int32), np.empty((len(Q), 3))
    for i, q in enumerate(Q):
        best = (np.inf, -1, None)
        for j, (ia, ib, ic) in enumerate(f):
            d, p = closest_scalar(q, v[ia], v[ib], v[ic])
            if d < best[0]:
                best = (d, j, p)
        dist[i], face[i], cp[i] = np.sqrt(best[0]), best[1], best[2]
    return dist, face, cp
