"""NumPy restatement of render_mesh (include/pb3d.h, "mesh -> image"): brute force over faces x pixels, no pruning, no boxes, no tiles.
Every operation is one NumPy float64 operation in the header's order, so the images must equal the device's bit for bit.  Also a plain
Python loop (per pixel, per face) the restatement is checked against, the shading rule, and the builders of the constructed cases."""
import numpy as np


def camera_coords(verts, R, cam, frame=0, depth=0.0):
    """(nv, 3) float64 camera coordinates: p = v or (v0, v1, depth - v2); q = p - cam; X = (R0*q0 + R1*q1) + R2*q2, ..."""
    v = np.asarray(verts).astype(np.float64)
    R = np.asarray(R, np.float64).reshape(9)
    cam = np.asarray(cam, np.float64)
    p2 = (np.float64(depth) - v[:, 2]) if frame else v[:, 2]
    q0, q1, q2 = v[:, 0] - cam[0], v[:, 1] - cam[1], p2 - cam[2]
    with np.errstate(all="ignore"):
        return np.stack([(R[3 * r] * q0 + R[3 * r + 1] * q1) + R[3 * r + 2] * q2 for r in range(3)], axis=1)


def wrapped(faces, nv):
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    assert f.size == 0 or (f.min() >= -nv and f.max() < nv)
    return np.where(f < 0, f + nv, f)


def evaluate(P, f, sx, sy, near):
    """U, V, W, det, t, hit of faces f (k, 3) against rays (sx, sy) (n,): arrays (k, n)"""
    A, B, C = P[f[:, 0]][:, None, :], P[f[:, 1]][:, None, :], P[f[:, 2]][:, None, :]
    xa, ya = A[..., 0] - sx * A[..., 2], A[..., 1] - sy * A[..., 2]
    xb, yb = B[..., 0] - sx * B[..., 2], B[..., 1] - sy * B[..., 2]
    xc, yc = C[..., 0] - sx * C[..., 2], C[..., 1] - sy * C[..., 2]
    U = xc * yb - yc * xb
    V = xa * yc - ya * xc
    W = xb * ya - yb * xa
    det = (U + V) + W
    T = (U * A[..., 2] + V * B[..., 2]) + W * C[..., 2]
    t = T / det
    neg = (U < 0) | (V < 0) | (W < 0)
    pos = (U > 0) | (V > 0) | (W > 0)
    hit = ~(neg & pos) & (det != 0) & (t >= near)
    return U, V, W, det, t, hit


def rays(f, cx, cy, H, W):
    u = np.tile(np.arange(W, dtype=np.float64), H)
    v = np.repeat(np.arange(H, dtype=np.float64), W)
    return (u - np.float64(cx)) / np.float64(f), -((v - np.float64(cy)) / np.float64(f))


def restate(verts, faces, R, cam, f, cx, cy, H, W, near=1e-6, frame=0, depth=0.0, chunk=64):
    """(depth (H, W) float64, face (H, W) int32, bary (H, W, 3) float64, hits (H, W) int64 = the number of faces hitting each pixel,
    ties (H, W) int64 = the number of them at the pixel's depth)"""
    P = camera_coords(verts, R, cam, frame, depth)
    fc = wrapped(faces, len(P))
    sx, sy = rays(f, cx, cy, H, W)
    n = H * W
    best_t = np.full(n, np.inf)
    best_f = np.full(n, -1, np.int64)
    bary = np.zeros((n, 3))
    hits = np.zeros(n, np.int64)
    ties = np.zeros(n, np.int64)
    cols = np.arange(n)
    with np.errstate(all="ignore"):
        for s in range(0, len(fc), chunk):
            U, V, W_, det, t, hit = evaluate(P, fc[s:s + chunk], sx, sy, np.float64(near))
            hits += hit.sum(axis=0)
            tt = np.where(hit, t, np.inf)
            tmin = tt.min(axis=0)
            first = np.argmax(hit & (tt == tmin), axis=0)           # the smallest face number at the chunk's minimum
            some = hit.any(axis=0)
            take = some & ((tmin < best_t) | (best_f < 0))          # a later chunk wins only with a strictly smaller t
            at_min = (hit & (tt == tmin)).sum(axis=0)
            ties = np.where(take, at_min, np.where(some & (tmin == best_t), ties + at_min, ties))
            best_t = np.where(take, tmin, best_t)
            best_f = np.where(take, first + s, best_f)
            d = det[first, cols]
            w = np.stack([U[first, cols] / d, V[first, cols] / d, W_[first, cols] / d], axis=1)
            bary = np.where(take[:, None], w, bary)
    return best_t.reshape(H, W), best_f.astype(np.int32).reshape(H, W), bary.reshape(H, W, 3), hits.reshape(H, W), ties.reshape(H, W)


def loop(verts, faces, R, cam, f, cx, cy, H, W, near=1e-6, frame=0, depth=0.0):
    """the same rule, one float64 scalar operation at a time: per pixel, per face"""
    F = np.float64
    P = camera_coords(verts, R, cam, frame, depth)
    fc = wrapped(faces, len(P))
    dep = np.full((H, W), np.inf)
    fac = np.full((H, W), -1, np.int32)
    bar = np.zeros((H, W, 3))
    hits = np.zeros((H, W), np.int64)
    with np.errstate(all="ignore"):
        for v in range(H):
            for u in range(W):
                sx = (F(u) - F(cx)) / F(f)
                sy = -((F(v) - F(cy)) / F(f))
                for k, (ia, ib, ic) in enumerate(fc):
                    (Xa, Ya, Za), (Xb, Yb, Zb), (Xc, Yc, Zc) = P[ia], P[ib], P[ic]
                    xa, ya = Xa - sx * Za, Ya - sy * Za
                    xb, yb = Xb - sx * Zb, Yb - sy * Zb
                    xc, yc = Xc - sx * Zc, Yc - sy * Zc
                    U = xc * yb - yc * xb
                    V = xa * yc - ya * xc
                    Wt = xb * ya - yb * xa
                    det = (U + V) + Wt
                    t = ((U * Za + V * Zb) + Wt * Zc) / det
                    mixed = min(U, V, Wt) < 0 and max(U, V, Wt) > 0
                    if mixed or not det != 0 or not t >= F(near):
                        continue
                    hits[v, u] += 1
                    if fac[v, u] < 0 or t < dep[v, u]:
                        dep[v, u], fac[v, u] = t, k
                        bar[v, u] = (U / det, V / det, Wt / det)
    return dep, fac, bar, hits


def shade(face, bary, faces, attr, background):
    """image[v, u] = attr[faces[face][m]], m the first corner with the largest weight; background where face is -1"""
    attr = np.asarray(attr)
    fc = wrapped(faces, len(attr))
    m = np.zeros(face.shape, np.int64)
    best = bary[..., 0]
    for k in (1, 2):
        up = bary[..., k] > best
        m = np.where(up, k, m)
        best = np.where(up, bary[..., k], best)
    hit = face >= 0
    img = np.empty(face.shape + attr.shape[1:], np.uint8)
    img[...] = np.asarray(background, np.uint8)
    if hit.any():
        img[hit] = attr[fc[face[hit], m[hit]]]
    return img


def bits(depth):
    return np.ascontiguousarray(depth, dtype=np.float64).view(np.uint64)


# ---- cameras ------------------------------------------------------------------------------------------------------------------------------
def look_at(cam_pos, target):
    """(R (3, 3) float64, cam (3,) float64) as render_mesh takes them: the host's look_at_rotation in float64"""
    from pb3d.camera_geometry import look_at_rotation
    cam = np.array(cam_pos, np.float64)
    return np.asarray(look_at_rotation(cam.copy(), np.array(target, np.float64)), np.float64), cam


IDENTITY = np.eye(3)


# ---- meshes -------------------------------------------------------------------------------------------------------------------------------
def icosphere(levels=3, scale=(9.0, 7.0, 11.5), centre=(1.5, -2.25, 3.0), dtype=np.float64):
    """a subdivided icosahedron (20 * 4^levels faces, consistently wound, vertices shared), scaled unevenly"""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1),
         (-g, 0, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(levels):
        mid = {}

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        nxt = []
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nxt += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nxt
    verts = (np.array(v) * np.array(scale) + np.array(centre)).astype(dtype)
    return verts, np.array(f, np.int32)


SPHERE_CAMERAS = [((40.0, 5.0, -30.0), (1.0, -2.0, 3.0)), ((-35.0, 22.0, 9.0), (2.0, -2.0, 2.5)), ((3.0, 48.0, 7.0), (1.5, -2.25, 3.0)),
                  ((-12.0, -30.0, 38.0), (1.0, -3.0, 3.5))]
SPHERE_INSIDE = ((1.0, -2.0, 3.5), (7.0, 1.0, 9.0))
SPHERE_VIEW = dict(f=100.0, cx=37.75, cy=30.25, H=61, W=77)
INSIDE_VIEW = dict(f=20.0, cx=37.75, cy=30.25, H=61, W=77)


def lattice_quad():
    """the exact-lattice quad split along its diagonal: (verts, faces, view) with R = I, cam = 0; pixel (u, v) is the point (u, 8 - v, 8)"""
    verts = np.array([(0, 0, 8), (8, 0, 8), (8, 8, 8), (0, 8, 8)], np.float64)
    faces = np.array([(0, 1, 2), (0, 2, 3)], np.int32)
    return verts, faces, dict(R=IDENTITY, cam=np.zeros(3), f=8.0, cx=0.0, cy=8.0, H=9, W=9)


def near_fan(near=2.0 ** -3, n=48):
    """n small faces parallel to the image plane (R = I, cam = 0), each over its own pixel of a 12-wide image, face k at
    Z = near * (1 + (k - n / 2) * 2^-52): a few ulps on either side of near, and exactly near in the middle"""
    f, cx, cy, W = 16.0, 5.5, 1.5, 12
    H = (n + W - 1) // W
    verts, faces = [], []
    for k in range(n):
        z = near * (1.0 + (k - n // 2) * 2.0 ** -52)
        u, v = k % W, k // W
        x, y = (u - cx) / f * z, -((v - cy) / f) * z
        r = 0.3 / f * z
        verts += [(x - r, y - r, z), (x + r, y - r, z), (x, y + r, z)]
        faces.append((3 * k, 3 * k + 1, 3 * k + 2))
    return np.array(verts, np.float64), np.array(faces, np.int32), dict(R=IDENTITY, cam=np.zeros(3), f=f, cx=cx, cy=cy, H=H, W=W, near=near)


def facing_triangles(points, R, cam, f, radius_px=1.5, lift=1e-3):
    """one camera-facing triangle around each point, its inscribed circle of projected radius radius_px pixels, moved `lift` towards
    the camera: (verts (3n, 3) float64, faces (n, 3) int32)"""
    P = np.asarray(points, np.float64)
    R = np.asarray(R, np.float64).reshape(3, 3)
    right, up, fwd = R[0], R[1], R[2]
    Z = (P - cam) @ fwd
    rin = radius_px * Z / f                                     # world radius of the inscribed circle at the point's depth
    c = P - lift * fwd
    corners = []
    for ang in (90.0, 210.0, 330.0):                            # an equilateral triangle: circumradius = 2 * inradius
        a = np.deg2rad(ang)
        corners.append(c + (2.0 * rin)[:, None] * (np.cos(a) * right + np.sin(a) * up))
    verts = np.stack(corners, axis=1).reshape(-1, 3)
    return verts, np.arange(3 * len(P), dtype=np.int32).reshape(-1, 3)
