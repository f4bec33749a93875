"""NumPy restatement of cast_rays (include/pb3d.h, "rays against a mesh"): brute force, every ray against every face, no index, no
walk, no margins.  Every operation is one NumPy float64 operation in the header's order, so t, face and bary must equal the device's
bit for bit.  Needs no device; it is the CPU side of tests/test_cast_rays.py, which also takes its ray families from here."""
import numpy as np

from inside_restate import box, icosphere, octahedron, rotation, wall_among_small, wrapped  # noqa: F401  (the tests' meshes)

F = np.float64


def ray_setup(d):
    """(kx, ky, kz) int arrays and (Sx, Sy, Sz) of finite, non-zero directions d (n, 3): RAY of the header"""
    a = np.abs(d)
    kz = np.where(a[:, 1] > a[:, 0], 1, 0)
    big = np.where(a[:, 1] > a[:, 0], a[:, 1], a[:, 0])
    kz = np.where(a[:, 2] > big, 2, kz)
    kx, ky = (kz + 1) % 3, (kz + 2) % 3
    r = np.arange(len(d))
    dz = d[r, kz]
    return kx, ky, kz, d[r, kx] / dz, d[r, ky] / dz, F(1.0) / dz


def evaluate(A, B, C, o, S, k):
    """U, V, W, det, t of faces with corners A, B, C (m, 3) against rays with origins o (n, 3), shears S = (Sx, Sy, Sz) (n,) each and the
    ONE permutation k = (kx, ky, kz): arrays (m, n).  FACE against RAY of the header, operation for operation"""
    kx, ky, kz = k
    Sx, Sy, Sz = S
    Ax, Ay, Az = (A[:, j][:, None] - o[:, j][None, :] for j in (kx, ky, kz))
    Bx, By, Bz = (B[:, j][:, None] - o[:, j][None, :] for j in (kx, ky, kz))
    Cx, Cy, Cz = (C[:, j][:, None] - o[:, j][None, :] for j in (kx, ky, kz))
    ax, ay = Ax - Sx * Az, Ay - Sy * Az
    bx, by = Bx - Sx * Bz, By - Sy * Bz
    cx, cy = Cx - Sx * Cz, Cy - Sy * Cz
    U = cx * by - cy * bx
    V = ax * cy - ay * cx
    W = bx * ay - by * ax
    det = (U + V) + W
    T = (U * (Sz * Az) + V * (Sz * Bz)) + W * (Sz * Cz)
    return U, V, W, det, T / det


def restate(origins, directions, verts, faces, t_min=0.0, t_max=np.inf, chunk=128):
    """(t float64 (n,), face int32 (n,), bary float64 (n, 3), hits int64 (n,) = the number of faces hitting each ray, bad bool (n,)).
    ValueError on a vertex that is not finite, IndexError on a face index outside [-nv, nv)"""
    o = np.asarray(origins).astype(F).reshape(-1, 3)                # float32 widens exactly
    d = np.asarray(directions).astype(F).reshape(-1, 3)
    V = np.asarray(verts).astype(F).reshape(-1, 3)
    fc = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    if fc.size and (fc.min() < -len(V) or fc.max() >= len(V)):
        raise IndexError("a face index is out of bounds")
    if not np.all(np.isfinite(V)):
        raise ValueError("a vertex coordinate is not finite")
    fc = wrapped(fc, len(V))
    t_min, t_max = F(t_min), F(t_max)
    n = len(o)
    best_t = np.full(n, np.inf)
    best_f = np.full(n, -1, np.int64)
    bary = np.zeros((n, 3))
    hits = np.zeros(n, np.int64)
    bad = ~(np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1)) | (d == 0).all(axis=1)
    good = np.flatnonzero(~bad)
    with np.errstate(all="ignore"):
        kx, ky, kz, Sx, Sy, Sz = ray_setup(d[good])
        for k in range(3):                                          # the rays of one permutation together
            sel = kz == k
            idx = good[sel]
            if not idx.size:
                continue
            perm = ((k + 1) % 3, (k + 2) % 3, k)
            S = (Sx[sel], Sy[sel], Sz[sel])
            cols = np.arange(idx.size)
            bt, bf, bb, bh = best_t[idx], best_f[idx], bary[idx], hits[idx]
            for s in range(0, len(fc), chunk):
                c = fc[s:s + chunk]
                U, Vv, W, det, t = evaluate(V[c[:, 0]], V[c[:, 1]], V[c[:, 2]], o[idx], S, perm)
                neg = (U < 0) | (Vv < 0) | (W < 0)
                pos = (U > 0) | (Vv > 0) | (W > 0)
                hit = ~(neg & pos) & (det != 0) & (t >= t_min) & (t <= t_max)
                bh += hit.sum(axis=0)
                tt = np.where(hit, t, np.inf)
                tmin = tt.min(axis=0)
                first = np.argmax(hit & (tt == tmin), axis=0)       # the smallest face number at the chunk's minimum (-0.0 == +0.0)
                some = hit.any(axis=0)
                take = some & ((tmin < bt) | (bf < 0))              # a later chunk wins only with a strictly smaller t
                bt = np.where(take, t[first, cols], bt)             # that face's own t: the sign of a zero is the face's
                bf = np.where(take, first + s, bf)
                dd = det[first, cols]
                w = np.stack([U[first, cols] / dd, Vv[first, cols] / dd, W[first, cols] / dd], axis=1)
                bb = np.where(take[:, None], w, bb)
            best_t[idx], best_f[idx], bary[idx], hits[idx] = bt, bf, bb, bh
    return best_t, best_f.astype(np.int32), bary, hits, bad


# ---- ray families ---------------------------------------------------------------------------------------------------------------------
def mesh_parts(verts, faces):
    """(vertices, edge midpoints) of the mesh in float64, the midpoints computed in the dtype of verts"""
    v = np.asarray(verts)
    f = wrapped(faces, len(v))
    mids = np.concatenate([(v[f[:, k]] + v[f[:, (k + 1) % 3]]) * v.dtype.type(0.5) for k in range(3)])
    return v.astype(F), mids.astype(F)


def families(verts, faces, seed, per=400):
    """the five ray families of tests/test_cast_rays.py, `per` rays each, as a dict name -> (origins, directions) in float64:
    uniform   origins uniform in the box of the mesh grown by a quarter (inside the mesh included), normal directions
    aimed     from outside (three box diagonals away) at vertices and edge midpoints: d = target - o as computed
    axis      axis-parallel rays through vertices: the origin is the vertex moved along one axis, so two coordinates are the vertex's
    ties      rays through vertices with direction components in {-1, 0, 1} (not all zero): ties in |d| for kz
    far       the aimed family with the origins scaled by 1e6"""
    rng = np.random.default_rng(seed)
    v, mids = mesh_parts(verts, faces)
    lo, hi = v.min(axis=0), v.max(axis=0)
    ext = np.where(hi > lo, hi - lo, 1.0)
    centre, diag = (lo + hi) / 2, float(np.linalg.norm(ext))
    out = {}
    out["uniform"] = (rng.uniform(lo - ext / 4, hi + ext / 4, (per, 3)), rng.normal(size=(per, 3)))
    targets = np.concatenate([v, mids])[rng.integers(0, len(v) + len(mids), per)]
    u = rng.normal(size=(per, 3))
    o = centre + 3 * diag * u / np.linalg.norm(u, axis=1, keepdims=True)
    out["aimed"] = (o, targets - o)
    pv = v[rng.integers(0, len(v), per)]
    ax = rng.integers(0, 3, per)
    step = np.zeros((per, 3))
    step[np.arange(per), ax] = rng.choice([-1.0, 1.0], per)
    out["axis"] = (pv - step * rng.choice([0.0, 0.5, 2.0], per)[:, None] * diag, step)
    d = rng.integers(-1, 2, (per, 3)).astype(F)
    d[(d == 0).all(axis=1)] = (1.0, -1.0, 1.0)
    pv2 = v[rng.integers(0, len(v), per)]
    out["ties"] = (pv2 - d * rng.choice([0.0, 1.0, 0.25], per)[:, None], d)
    of = o * 1e6
    out["far"] = (of, targets - of)
    return out

