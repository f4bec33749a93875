"""NumPy restatement of include/pb3d.h's distance-transform section: exact, in integers, separable -- one broadcast minimum per axis with the
lexicographic tie rule and the PB3D_EDT_NONE sentinel -- next to a brute force over all (voxel, target) pairs, the ball morphology and
the surface sums built on it, and the constructed contents the tests run.  No device, no pb3d import."""
import math

import numpy as np

NONE = 2 ** 31 - 1          # PB3D_EDT_NONE
_BIG = np.int64(1) << 40    # "no target" inside the int64 minima: larger than any sum of three squares below 16384^2
TARGETS = ("background", "occupied", "surface")


def occupancy(grid):
    """(n0, n1, n2) bool: any channel non-zero"""
    g = np.asarray(grid)
    return g != 0 if g.ndim == 3 else (g != 0).any(axis=-1)


def surface(occ):
    """occupied voxels with at least one of their 6 neighbours empty or outside the grid"""
    p = np.pad(occ, 1, constant_values=False)
    inner = (p[:-2, 1:-1, 1:-1] & p[2:, 1:-1, 1:-1] & p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1] & p[1:-1, 1:-1, :-2] & p[1:-1, 1:-1, 2:])
    return occ & ~inner


def target_mask(grid, to):
    occ = occupancy(grid)
    return {"background": ~occ, "occupied": occ, "surface": surface(occ)}[to]


def _border_sq(shape):
    """min over the axes a of (v_a + 1)^2 and (n_a - v_a)^2"""
    ax = [np.minimum(np.arange(n) + 1, n - np.arange(n)).astype(np.int64) for n in shape]
    b = np.minimum(np.minimum(ax[0][:, None, None], ax[1][None, :, None]), ax[2][None, None, :])
    return b * b


def _axis_pass(g, f, axis, mult):
    """out[x] = min over s of g[s] + (x - s)^2 along `axis`, the smallest s among equal totals; f[x] = s * mult + f[s]"""
    g, f = np.moveaxis(g, axis, -1), np.moveaxis(f, axis, -1)
    shape, m = g.shape, g.shape[-1]
    G, F = g.reshape(-1, m), f.reshape(-1, m)
    x = np.arange(m, dtype=np.int64)
    par = (x[:, None] - x[None, :]) ** 2                    # [x, s]
    out, idx = np.empty_like(G), np.empty_like(F)
    step = max(1, (1 << 22) // (m * m))                     # lines per broadcast: bounded memory for a long axis
    for a in range(0, len(G), step):
        cost = G[a:a + step, None, :] + par[None]
        s = cost.argmin(axis=-1)                            # the first minimum: the smallest s
        out[a:a + step] = np.take_along_axis(cost, s[..., None], -1)[..., 0]
        idx[a:a + step] = s * mult + np.take_along_axis(F[a:a + step], s, -1)
    none = out >= _BIG
    out[none], idx[none] = _BIG, -1
    return np.moveaxis(out.reshape(shape), -1, axis), np.moveaxis(idx.reshape(shape), -1, axis)


def edt(targets, border=False):
    """(sq int32, index int32) of a bool target mask; index is all -1 with border (the entry refuses it there)"""
    t = np.asarray(targets, dtype=bool)
    n0, n1, n2 = t.shape
    g, f = np.where(t, np.int64(0), _BIG), np.zeros(t.shape, np.int64)
    g, f = _axis_pass(g, f, 2, 1)                           # rows: the smaller t2 of an equidistant pair
    g, f = _axis_pass(g, f, 1, n2)                          # the smallest t1 among equal totals
    g, f = _axis_pass(g, f, 0, n1 * n2)                     # the smallest t0
    if border:
        g = np.minimum(g, _border_sq(t.shape))
        f = np.full(t.shape, -1, np.int64)
    return np.where(g >= _BIG, NONE, g).astype(np.int32), f.astype(np.int32)


def edt_grid(grid, to="background", border=False):
    return edt(target_mask(grid, to), border)


def brute(targets, border=False, rule="smallest"):
    """the same by every (voxel, target) pair: per voxel the squared distances to all targets, listed in linear-index order.
    rule: which of the nearest targets the index names -- 'smallest' (the stated rule) or 'largest' (a wrong one, for the tests)"""
    t = np.asarray(targets, dtype=bool)
    shape = t.shape
    T = np.argwhere(t).astype(np.int64)                     # lexicographic = ascending linear index
    lin = (T[:, 0] * shape[1] + T[:, 1]) * shape[2] + T[:, 2]
    sq, idx = np.full(shape, NONE, np.int64), np.full(shape, -1, np.int64)
    bsq = _border_sq(shape)
    for v in np.ndindex(*shape):
        if len(T):
            d = ((T - np.array(v)) ** 2).sum(axis=1)
            m = d.min()
            near = np.flatnonzero(d == m)
            sq[v], idx[v] = m, lin[near[0] if rule == "smallest" else near[-1]]
        if border:
            sq[v], idx[v] = min(sq[v], bsq[v]), -1
    return sq.astype(np.int32), idx.astype(np.int32)


def distances(sq, voxel_size=1.0, dtype=np.float64):
    """sqrt((double)sq) * voxel_size, +inf at the sentinel, rounded once more for float32"""
    with np.errstate(over="ignore"):
        d = np.sqrt(sq.astype(np.float64)) * np.float64(voxel_size)
    d[sq == NONE] = np.inf
    return d.astype(dtype)


def radius_sq(radius):
    """the largest integer q with q <= radius * radius in float64"""
    return int(math.floor(float(radius) * float(radius)))


def ball(r_sq):
    """the structuring element of the lattice points with squared norm <= r_sq"""
    r = int(math.isqrt(r_sq))
    x = np.arange(-r, r + 1)
    return (x[:, None, None] ** 2 + x[None, :, None] ** 2 + x[None, None, :] ** 2) <= r_sq


def dilate(grid, r_sq):
    g = np.asarray(grid)
    occ = occupancy(g)
    sq, idx = edt(occ)
    out = g.copy()
    fill = ~occ & (sq <= r_sq)
    flat = g.reshape(occ.size, -1)
    out.reshape(occ.size, -1)[fill.reshape(-1)] = flat[idx[fill]]
    return out


def erode(grid, r_sq, border=True):
    g = np.asarray(grid)
    sq, _ = edt(~occupancy(g), border)
    keep = sq > r_sq
    return np.where(keep if g.ndim == 3 else keep[..., None], g, 0).astype(np.uint8)


def close(grid, r_sq):
    return erode(dilate(grid, r_sq), r_sq, border=False)


def open_(grid, r_sq):
    return dilate(erode(grid, r_sq, border=True), r_sq)


def surface_sums(a, b, thresholds_sq):
    """[surface voxels of a, max sq, sum sq, #(sq <= t) per t] of a's surface against b's, Python integers; max is -1 without a voxel"""
    sa = surface(occupancy(a))
    s = edt(surface(occupancy(b)))[0][sa].astype(np.int64)
    return [int(sa.sum()), int(s.max()) if len(s) else -1, int(s.sum())] + [int((s <= t).sum()) for t in thresholds_sq]


def surface_metrics(a, b, thresholds=(1.0,), voxel_size=1.0):
    """the dict of grid_surface_metrics from the integer sums"""
    vs = np.float64(voxel_size)
    thr = [radius_sq(float(t) / float(voxel_size)) for t in thresholds]
    ab, ba = surface_sums(a, b, thr), surface_sums(b, a, thr)
    na, nb = ab[0], ba[0]

    def directed(r, n_from, n_to):
        if n_from == 0:
            return 0.0, 0.0
        if n_to == 0:
            return math.inf, math.inf
        return float(np.sqrt(np.float64(r[1])) * vs), float(np.sqrt(np.float64(r[2]) / np.float64(n_from)) * vs)

    (h_ab, rms_ab), (h_ba, rms_ba) = directed(ab, na, nb), directed(ba, nb, na)
    res = {"hausdorff": max(h_ab, h_ba), "hausdorff_ab": h_ab, "hausdorff_ba": h_ba, "rms_ab": rms_ab, "rms_ba": rms_ba,
           "surface_voxels_a": na, "surface_voxels_b": nb, "precision": [], "recall": [], "fscore": []}
    for k in range(len(thr)):
        p = float(np.float64(ab[3 + k]) / np.float64(na)) if na and nb else 0.0
        r = float(np.float64(ba[3 + k]) / np.float64(nb)) if na and nb else 0.0
        res["precision"].append(p)
        res["recall"].append(r)
        res["fscore"].append(0.0 if (p + r) == 0 else 2 * p * r / (p + r))
    return res


# ---- constructed contents: bool TARGET masks of a shape -------------------------------------------------------------------------------
def contents(shape, seed=0):
    """name -> bool mask: the contents the issue lists, at any shape"""
    n0, n1, n2 = shape
    rng = np.random.default_rng(seed)
    z = lambda: np.zeros(shape, bool)                       # noqa: E731
    out = {"random_0.5": rng.random(shape) < 0.5, "random_0.995": rng.random(shape) < 0.995, "random_0.005": rng.random(shape) < 0.005}
    c = z()
    c[0, 0, 0] = True
    out["corner"] = c
    c = z()
    c[-1, -1, -1] = True
    out["far_corner"] = c
    i, j, k = np.indices(shape)
    out["checkerboard"] = (i + j + k) % 2 == 0
    p = z()
    p[n0 // 2] = True
    out["plane_axis0"] = p
    p = z()
    p[:, :, n2 // 3] = True
    out["plane_axis2"] = p
    s = z()
    s[:, n1 // 3:n1 // 3 + 3] = True
    out["slab_axis1"] = s
    m = (n0 // 2, n1 // 2, n2 // 2)
    for a in range(3):                                      # two targets symmetric about voxel m on axis a: the tie rule alone
        if shape[a] >= 3:
            t = z()
            d = min(m[a], shape[a] - 1 - m[a], 3)
            lo, hi = list(m), list(m)
            lo[a] -= d
            hi[a] += d
            t[tuple(lo)] = t[tuple(hi)] = True
            out[f"pair_axis{a}"] = t
    if min(shape) >= 3:
        t = z()
        for sgn in [(a, b, c) for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)]:
            t[m[0] + sgn[0], m[1] + sgn[1], m[2] + sgn[2]] = True
        out["pairs_all_axes"] = t
    out["none"] = z()
    out["all"] = ~z()
    return out


def grid_for(mask, to):
    """a uint8 grid whose targets of kind `to` are (for 'surface': come from) the mask"""
    return (~mask if to == "background" else mask).astype(np.uint8)


TIE_CASE_SHAPE = (9, 7, 11)     # the case on which SciPy's own indices and the largest-index rule both differ from the stated rule


def tie_case():
    return np.random.default_rng(7).random(TIE_CASE_SHAPE) < 0.06
