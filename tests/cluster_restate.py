"""The rules of cluster_points (include/pb3d.h: NEIGHBOUR, COUNTS, CORE, CLUSTERS, BORDER, NOISE, SIZES) restated in NumPy by brute
force, and the constructed clouds that tests/test_cluster_points.py runs on the CPU (against scikit-learn) and on the device.

restate() compares every point with every point whose x lies within eps of its own: d2 <= eps2 implies dx*dx <= eps2 (adding
non-negative terms never lowers a rounded sum), so the window, taken a little wider than eps, drops no neighbour.  It works through
the cloud in chunks of rows sorted by x and never holds an n x n array.  Components come from the core-core pairs by repeated
hooking of the larger root under the smaller and full path compression, so a root is its component's smallest index."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _pairs(a, eps, chunk):
    """yields (I, J): the neighbour pairs (both directions, i == j included) of one chunk of rows, as positions in a"""
    n = len(a)
    eps2 = eps * eps
    order = np.argsort(a[:, 0], kind="stable")
    xs = a[order, 0]
    reach = eps * (1.0 + 1e-9) + 4.0 * np.spacing(np.abs(xs).max() + eps)
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        lo = np.searchsorted(xs, xs[s] - reach, "left")
        hi = np.searchsorted(xs, xs[e - 1] + reach, "right")
        I, J = order[s:e], order[lo:hi]
        dx = a[I, 0][:, None] - a[J, 0][None, :]
        dy = a[I, 1][:, None] - a[J, 1][None, :]
        dz = a[I, 2][:, None] - a[J, 2][None, :]
        d2 = (dx * dx + dy * dy) + dz * dz
        r, c = np.nonzero(d2 <= eps2)
        yield I[r], J[c]


def restate(points, eps, min_samples, chunk=512):
    """(labels int64, core bool, counts int64, sizes int64) of an (n, 3) cloud; float32 is widened, anything else becomes float64"""
    a = np.asarray(points)
    a = np.ascontiguousarray(a, dtype=np.float64)
    n = len(a)
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, bool), np.zeros(0, np.int64), np.zeros(0, np.int64)
    eps = np.float64(eps)
    counts = np.zeros(n, np.int64)
    for I, _ in _pairs(a, eps, chunk):
        counts += np.bincount(I, minlength=n)
    core = counts >= min_samples
    ei, ej, bi, bj = [], [], [], []
    for I, J in _pairs(a, eps, chunk):
        cj = core[J]
        m = cj & core[I] & (J < I)
        ei.append(I[m]); ej.append(J[m])
        m = cj & ~core[I]
        bi.append(I[m]); bj.append(J[m])
    ei, ej, bi, bj = (np.concatenate(v) for v in (ei, ej, bi, bj))
    parent = np.arange(n)
    while True:
        ri, rj = parent[ei], parent[ej]
        m = ri != rj
        if not m.any():
            break
        np.minimum.at(parent, np.maximum(ri, rj)[m], np.minimum(ri, rj)[m])
        while True:
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
    roots = np.flatnonzero(core & (parent == np.arange(n)))
    rank = np.full(n, -1, np.int64)
    rank[roots] = np.arange(len(roots))
    labels = np.full(n, -1, np.int64)
    labels[core] = rank[parent[core]]
    border = np.full(n, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(border, bi, labels[bj])
    hit = ~core & (border != np.iinfo(np.int64).max)
    labels[hit] = border[hit]
    sizes = np.bincount(labels[labels >= 0], minlength=len(roots)).astype(np.int64)
    return labels, core, counts, sizes


# ---- the constructed clouds ------------------------------------------------------------------------------------------------------------
def lattice_cloud():
    """400 of the 12^3 integer sites: every distance is the root of an integer, so eps in {1, sqrt 2, sqrt 3, 2} puts many pairs exactly
    at (or one rounding away from) the threshold"""
    rng = np.random.default_rng(1203)
    sites = rng.choice(12 ** 3, 400, replace=False)
    return np.stack(np.unravel_index(sites, (12, 12, 12)), axis=1).astype(np.float64)


def chain_cloud(n=3000, gaps=()):
    """n points spaced exactly eps = 7/64 apart along (2, 3, 6)/64: d2 of two neighbours is 49/4096 = eps*eps to the bit, in float32
    as well.  gaps: positions left out, which cut the chain into several"""
    i = np.array([k for k in range(n + len(gaps)) if k not in set(gaps)], np.float64)
    return i[:, None] * (np.array([2.0, 3.0, 6.0]) / 64.0)[None, :]


CHAIN_EPS = 7.0 / 64.0


def bridge_cloud(order):
    """two 3x3x3 unit-lattice blobs, x in 0..2 and x in 4..6, and the point (3, 1, 1) between them.  eps = 1, min_samples = 4: every
    blob point is core (a corner has 3 neighbours and itself), the bridge has 2 neighbours and itself, both core, one in each blob.
    order: the blocks 'a', 'b' and the bridge '-' in input order"""
    g = np.stack(np.meshgrid(np.arange(3.0), np.arange(3.0), np.arange(3.0), indexing="ij"), axis=-1).reshape(-1, 3)
    part = {"a": g, "b": g + np.array([4.0, 0.0, 0.0]), "-": np.array([[3.0, 1.0, 1.0]])}
    return np.concatenate([part[c] for c in order])


def _unit(seed, n):
    return np.random.default_rng(seed).random((n, 3))


def constructed_cases():
    """[(name, float64 cloud, eps, min_samples)], small enough for a few seconds each in both dtypes"""
    cases = []
    lat = lattice_cloud()
    for en, eps in (("1", 1.0), ("sqrt2", float(np.sqrt(2.0))), ("sqrt3", float(np.sqrt(3.0))), ("2", 2.0)):
        for ms in (1, 4, 7):
            cases.append((f"lattice/eps={en}/ms={ms}", lat, eps, ms))
    chain = chain_cloud()
    rng = np.random.default_rng(3000)
    cases.append(("chain/forward", chain, CHAIN_EPS, 2))
    cases.append(("chain/reversed", chain[::-1].copy(), CHAIN_EPS, 2))
    cases.append(("chain/shuffled", chain[rng.permutation(len(chain))], CHAIN_EPS, 2))
    cut = chain_cloud(3000, gaps=(700, 701, 1900))
    cases.append(("chain/cut-shuffled", cut[rng.permutation(len(cut))], CHAIN_EPS, 2))
    for order in ("ab-", "ba-", "-ba", "a-b"):
        cases.append((f"bridge/{order}", bridge_cloud(order), 1.0, 4))
    cases.append(("singletons", _unit(2500, 2500), 1e-6, 1))        # 2500 roots: the rank scan crosses two segment seams (1024)
    cases.append(("degenerate/eps>diagonal", _unit(31, 300), 10.0, 5))
    cases.append(("degenerate/identical", np.tile(np.array([[0.3, -1.2, 5.0]]), (200, 1)), 0.1, 3))
    flat = _unit(32, 500)
    flat[:, 2] = 2.0
    cases.append(("degenerate/flat", flat, 0.08, 4))
    cases.append(("degenerate/offset", _unit(33, 500) + 1e6, 0.12, 4))
    for n in (1, 255, 256, 257):
        cases.append((f"size/{n}", _unit(100 + n, n), 0.15, 3))
    return cases


SFM_EPS, SFM_MIN_SAMPLES = 0.06, 10


def sfm_cloud():
    with np.load(os.path.join(GOLDEN, "inter_sfm20k.npz"), allow_pickle=False) as z:
        return z["sfm"]


@functools.lru_cache(maxsize=None)
def _reference(name, f32):
    if name == "sfm":
        pts, eps, ms = sfm_cloud(), SFM_EPS, SFM_MIN_SAMPLES
    else:
        pts, eps, ms = next((p, e, m) for n, p, e, m in constructed_cases() if n == name)
    if f32:
        pts = pts.astype(np.float32)
    out = restate(pts, eps, ms)
    for a in out:
        a.setflags(write=False)
    return out


def reference(name, dtype=np.float64):
    """restate() of a constructed case (or "sfm") cast to dtype: computed once per process, read-only"""
    return _reference(name, np.dtype(dtype) == np.float32)
