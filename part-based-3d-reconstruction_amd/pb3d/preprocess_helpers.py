"""The two normalisation helpers of the reference's utils/preprocess_helpers.py that its evaluation code calls (the file itself is
missing upstream; utils/eval_helpers.py:11 imports normalize_preserve_aspect from it).  Host NumPy, dtype-preserving: a float32 cloud
is normalised in float32, as NumPy's own promotion rules (NEP 50) do with the Python constants below.

normalize_preserve_aspect maps a cloud into the unit cube with one scale for all three axes, then shifts the y column so that its
maximum is exactly 0: y ends in [-1, 0] (-1 itself only where scale + 1e-8 rounds to scale).  pb3d.eval_helpers.pointcloud_to_voxel_grid evaluates the same expressions on the device
(csrc/density.hip).

icp_align is the registration the inter-method metrics assume ("Align all reconstructions" of the reference's inter-method README):
rigid point-to-point ICP with both clouds resident on the device.  There is no upstream text to follow, so include/pb3d.h states the
arithmetic to the bit: per iteration the device transforms the source, finds every point's exact nearest target point against an
index built once per alignment (csrc/icp.hip on the search of csrc/nn.hip, ties to the lowest index) and reduces the pairs to a
count and 16 float64 sums in a fixed order; the host downloads those 17 values, solves the 3 x 3 problem
(best_fit_transform_from_sums) and composes the transform.  With trim_fraction the device also finds, per iteration and without a host
wait, the exact k-th smallest pair distance (csrc/select.hip) and sums only the pairs up to it; with with_scale the host solve
estimates Umeyama's scale from one more sum (best_fit_similarity_from_sums).  With method="point_to_plane" the device step gathers the
target's normals (given, or estimated once on the device: estimate_normals on the exact k-neighbour rows of csrc/nn.hip, csrc/normals.hip)
and sums the 29 terms of the 6 x 6 normal equations; the host solves them with a cut-off pseudo-inverse (plane_step_from_sums).

crop_to_box, fit_plane_ransac + plane_alignment_transform and symmetric_completion are steps 2-4 of the same README: crop the dense
cloud to the sparse cloud's box, estimate the dominant facade plane and turn it onto the Z axis, and the naive four-way completion.
Again include/pb3d.h states the arithmetic (csrc/plane.hip): the device builds K plane hypotheses from K point triplets, scores all
of them against the resident cloud in one sweep with exact integer counts, and reduces the inliers of a plane to a count and 11
float64 sums in the ICP step's fixed order; the host draws the triplets, picks the best row, and solves the 3 x 3 eigen problem of a
refit (plane_from_moments).  Segmenting the SfM cloud, step 1, is pb3d/cluster.py (cluster_points, keep_largest_clusters: exact DBSCAN
on the device).  Thinning a cloud to an even density before registration is pb3d/downsample.py (voxel_downsample: a voxel-grid filter
on the device).  What is still not mirrored: loading the SfM cloud, and the CAD model."""
import math

import numpy as np

from . import _lib, device as dev
from ._lib import _ptr
from ._args import _cloud

__all__ = ["normalize_preserve_aspect", "flip_y_axis", "transform_points", "transform_points_resident", "best_fit_transform_from_sums",
           "best_fit_similarity_from_sums", "icp_align", "icp_align_resident", "icp_index_resident", "icp_step_resident",
           "icp_step_trimmed_resident", "icp_step_plane_resident", "plane_step_from_sums", "estimate_normals",
           "estimate_normals_resident", "plane_hypotheses_resident", "plane_score_resident",
           "plane_moments_resident", "crop_to_box_resident", "plane_from_moments", "fit_plane_ransac", "fit_plane_ransac_resident",
           "plane_alignment_transform", "crop_to_box", "symmetric_completion", "symmetric_completion_resident"]


def normalize_preserve_aspect(points):
    pts = np.asarray(points)
    min_val = pts.min(0)
    size = pts.max(0) - min_val
    scale = size.max()
    norm = (pts - min_val) / (scale + 1e-8)
    norm[:, 1] -= norm[:, 1].max()
    return norm


def flip_y_axis(coords):
    c = np.array(coords, copy=True)
    y = c[:, 1]
    c[:, 1] = y.max() - (y - y.min())
    return c


# ---- rigid ICP ---------------------------------------------------------------------------------------------------------------------------
def _finite(a, what):
    if not np.isfinite(a).all():
        raise ValueError(f"Input {what} contains NaN or infinity.")


def _transform(T, what="T"):
    """float64 4 x 4 of a 3 x 4 or 4 x 4 matrix (a 4 x 4 must end in the row 0 0 0 1)"""
    t = np.asarray(T)
    if t.shape not in ((3, 4), (4, 4)) or t.dtype.kind not in "fiu":
        raise ValueError(f"{what} must be a real 3 x 4 or 4 x 4 matrix (got shape {t.shape}, dtype {t.dtype})")
    t = np.ascontiguousarray(t, dtype=np.float64)
    _finite(t, what)
    if t.shape == (4, 4) and not np.array_equal(t[3], (0.0, 0.0, 0.0, 1.0)):
        raise ValueError(f"{what}: the last row of a 4 x 4 transform must be 0 0 0 1")
    out = np.eye(4)
    out[:3] = t[:3]
    return out


def _t12(T):
    return np.ascontiguousarray(T[:3], dtype=np.float64).reshape(12)


def transform_points_resident(d_P, n, T, f64=True, out=None):
    """pb3d_transform_points_resident: a DeviceBuffer of n x 3 float64, T applied to the resident (n, 3) list d_P (float64 rows, or
    float32 with f64 False)"""
    t = _t12(_transform(T))
    with dev.Scope() as sc:
        d_out = sc.result(out, max(1, int(n)) * 24)
        _lib.check(_lib.load().pb3d_transform_points_resident(_lib.ctx(), _ptr(d_P), int(bool(f64)), int(n), _lib.p_dbl(t), _ptr(d_out)))
        return d_out


def transform_points(P, T):
    """float64 (n, 3): row i = ((T[h,0]*x + T[h,1]*y) + T[h,2]*z) + T[h,3] of point i, for a 3 x 4 or 4 x 4 T, on the device"""
    p, pf = _cloud(P, "P")
    t = _transform(T)
    if len(p) == 0:
        return np.zeros((0, 3), np.float64)
    with dev.Scope() as sc:
        d_out = sc.adopt(transform_points_resident(sc.upload(p), len(p), t, pf))
        return d_out.download((len(p), 3), np.float64)


def best_fit_transform_from_sums(count, sums, cp, cq):
    """The 4 x 4 rigid transform (rotation of determinant +1, no scale) that best maps the used source points onto their partners in
    the least-squares sense, from the count and the 16 sums of a step: sums[0:3] = sum(p - cp), sums[3:6] = sum(q - cq),
    sums[6:15] = sum((p - cp)(q - cq)^T) row-major (sums[15], the squared distances, is not read)."""
    count = int(count)
    sums = np.asarray(sums, np.float64).reshape(16)
    cp = np.asarray(cp, np.float64).reshape(3)
    cq = np.asarray(cq, np.float64).reshape(3)
    if count < 3:
        raise ValueError(f"a rigid fit needs at least 3 point pairs (got {count})")
    Sp, Sq, Spq = sums[0:3], sums[3:6], sums[6:15].reshape(3, 3)
    H = Spq - np.outer(Sp, Sq) / count
    U, S, Vt = np.linalg.svd(H)
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    t = (Sq / count + cq) - R @ (Sp / count + cp)
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = t
    return M


def best_fit_similarity_from_sums(count, sums, cp, cq, with_scale=True):
    """The 4 x 4 similarity transform (upper 3 x 3 = s R, R a rotation of determinant +1, s > 0: Umeyama's estimate) that best maps the
    used source points onto their partners, from the count and the 17 sums of a trimmed step: the 16 of best_fit_transform_from_sums
    and sums[16] = sum |p - cp|^2.  H, its SVD, d and R are the rigid solve's;
        var = sums[16] - ((Sp0*Sp0 + Sp1*Sp1) + Sp2*Sp2) / count,   s = ((S0 + S1) + d*S2) / var,   t = (Sq/count + cq) - s R (Sp/count + cp).
    with_scale=False: exactly best_fit_transform_from_sums(count, sums[:16], cp, cq)."""
    sums = np.asarray(sums, np.float64).reshape(17)
    if not with_scale:
        return best_fit_transform_from_sums(count, sums[:16], cp, cq)
    count = int(count)
    cp = np.asarray(cp, np.float64).reshape(3)
    cq = np.asarray(cq, np.float64).reshape(3)
    if count < 3:
        raise ValueError(f"a similarity fit needs at least 3 point pairs (got {count})")
    Sp, Sq, Spq = sums[0:3], sums[3:6], sums[6:15].reshape(3, 3)
    H = Spq - np.outer(Sp, Sq) / count
    U, S, Vt = np.linalg.svd(H)
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    var = sums[16] - ((Sp[0] * Sp[0] + Sp[1] * Sp[1]) + Sp[2] * Sp[2]) / count
    if not (math.isfinite(var) and var > 0.0):
        raise ValueError(f"a similarity fit needs source points that are not all equal (their summed squared spread is {var})")
    s = ((S[0] + S[1]) + d * S[2]) / var
    if not (math.isfinite(s) and s > 0.0):
        raise ValueError(f"the similarity fit found no positive finite scale (got {s})")
    A = s * R
    t = (Sq / count + cq) - A @ (Sp / count + cp)
    M = np.eye(4)
    M[:3, :3] = A
    M[:3, 3] = t
    return M


def icp_index_resident(d_target, nt, f64=True):
    """pb3d_icp_index_resident: bin the resident (nt, 3) target for the steps that follow; returns its exact box (min 3, max 3)"""
    b = np.zeros(6, np.float64)
    _lib.check(_lib.load().pb3d_icp_index_resident(_lib.ctx(), _ptr(d_target), int(bool(f64)), int(nt), _lib.p_dbl(b)))
    return b


def icp_step_resident(d_source, ns, d_target, nt, T, max_dist2, cp, cq, s_f64=True, t_f64=True, out=None):
    """pb3d_icp_step_resident: a DeviceBuffer of 17 x 8 bytes -- the int64 count of used pairs and the 16 float64 sums of one step with
    the 4 x 4 (or 3 x 4) T against the index icp_index_resident built for this target.  max_dist2 < 0: no gate."""
    t = _t12(np.asarray(T, np.float64))
    cp = np.ascontiguousarray(cp, dtype=np.float64).reshape(3)
    cq = np.ascontiguousarray(cq, dtype=np.float64).reshape(3)
    with dev.Scope() as sc:
        d_out = sc.result(out, 17 * 8)
        _lib.check(_lib.load().pb3d_icp_step_resident(_lib.ctx(), _ptr(d_source), int(bool(s_f64)), int(ns), _ptr(d_target), int(bool(t_f64)),
                                                      int(nt), _lib.p_dbl(t), float(max_dist2), _lib.p_dbl(cp), _lib.p_dbl(cq), _ptr(d_out)))
        return d_out


def icp_step_trimmed_resident(d_source, ns, d_target, nt, T, max_dist2, trim_fraction, cp, cq, s_f64=True, t_f64=True, out=None):
    """pb3d_icp_step_trimmed_resident: a DeviceBuffer of 20 x 8 bytes -- the int64 count of used pairs, 17 float64 sums (the 16 of
    icp_step_resident and sum |p - cp|^2), the int64 number of candidate pairs m and the float64 tau, the k-th smallest candidate
    squared distance with k = ceil(trim_fraction * m): the pairs with d2 <= tau are used.  The 4 x 4 (or 3 x 4) T need not be rigid."""
    t = _t12(np.asarray(T, np.float64))
    cp = np.ascontiguousarray(cp, dtype=np.float64).reshape(3)
    cq = np.ascontiguousarray(cq, dtype=np.float64).reshape(3)
    with dev.Scope() as sc:
        d_out = sc.result(out, 20 * 8)
        _lib.check(_lib.load().pb3d_icp_step_trimmed_resident(_lib.ctx(), _ptr(d_source), int(bool(s_f64)), int(ns), _ptr(d_target),
                                                              int(bool(t_f64)), int(nt), _lib.p_dbl(t), float(max_dist2), float(trim_fraction),
                                                              _lib.p_dbl(cp), _lib.p_dbl(cq), _ptr(d_out)))
        return d_out


def icp_step_plane_resident(d_source, ns, d_target, nt, d_normals, T, max_dist2, trim_fraction, c, s_f64=True, t_f64=True, out=None):
    """pb3d_icp_step_plane_resident: a DeviceBuffer of 32 x 8 bytes -- the int64 count of used pairs, the 29 float64 sums of one
    point-to-plane step (the upper triangle of sum J J^T, sum J r, sum r r, sum d2) against the index of icp_index_resident and the
    resident (nt, 3) float64 target normals, the int64 number of candidate pairs m and the float64 tau.  trim_fraction < 0 (or None):
    untrimmed, m and tau are 0.  c: the pivot of the rotation."""
    t = _t12(np.asarray(T, np.float64))
    c = np.ascontiguousarray(c, dtype=np.float64).reshape(3)
    rho = -1.0 if trim_fraction is None else float(trim_fraction)
    with dev.Scope() as sc:
        d_out = sc.result(out, 32 * 8)
        _lib.check(_lib.load().pb3d_icp_step_plane_resident(_lib.ctx(), _ptr(d_source), int(bool(s_f64)), int(ns), _ptr(d_target),
                                                            int(bool(t_f64)), int(nt), _ptr(d_normals), _lib.p_dbl(t), float(max_dist2), rho,
                                                            _lib.p_dbl(c), _ptr(d_out)))
        return d_out


def plane_step_from_sums(count, sums, c, cutoff=1e-12):
    """(4 x 4 step, rank): the small rigid motion about the pivot c that minimises the linearised point-to-plane error, from the count
    and the sums of a point-to-plane step (sums[0:21] = the upper triangle of A = sum J J^T row-major, sums[21:27] = g = sum J r; later
    entries are not read).  w, V = eigh(A); the eigenpairs with w > cutoff * w[-1] are kept (rank of them: a flat target leaves 3)
    and x = -V_keep diag(1 / w_keep) V_keep^T g.  omega = x[:3] becomes R by Rodrigues' formula (I + K below |omega| = 1e-12), t = x[3:],
    and the step is [R | c + t - R c]."""
    count = int(count)
    sums = np.asarray(sums, np.float64).reshape(-1)
    c = np.asarray(c, np.float64).reshape(3)
    if sums.size < 27:
        raise ValueError(f"a point-to-plane solve needs the 27 sums of A and g (got {sums.size})")
    if count < 6:
        raise ValueError(f"a point-to-plane fit needs at least 6 point pairs (got {count})")
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = sums[:21]
    A = A + np.triu(A, 1).T
    g = sums[21:27]
    w, V = np.linalg.eigh(A)
    keep = w > cutoff * w[-1]
    rank = int(keep.sum())
    M = np.eye(4)
    if rank == 0:           # A = 0: nothing to solve
        return M, 0
    Vk = V[:, keep]
    x = -(Vk @ ((Vk.T @ g) / w[keep]))
    om, t = x[:3], x[3:]
    th = float(np.sqrt((om[0] * om[0] + om[1] * om[1]) + om[2] * om[2]))
    K = np.array([[0.0, -om[2], om[1]], [om[2], 0.0, -om[0]], [-om[1], om[0], 0.0]])
    if th < 1e-12:
        R = np.eye(3) + K
    else:
        K = K / th
        R = np.eye(3) + math.sin(th) * K + (1.0 - math.cos(th)) * (K @ K)
    M[:3, :3] = R
    M[:3, 3] = c + t - R @ c
    return M, rank


def _normals_k(k, n):
    """k of estimate_normals for n points: a plane needs three neighbours, the search has its limit, and a row needs k points"""
    from .eval_helpers import KNN_MAX_K
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)):
        raise ValueError(f"k must be an integer (got {k!r})")
    if k < 3 or k > KNN_MAX_K:
        raise ValueError(f"k must be in [3, {KNN_MAX_K}] (got {k})")
    if n < k:
        raise ValueError(f"estimate_normals: k = {k} neighbours need at least {k} points (got {n})")
    return int(k)


def _viewpoint(orient_towards):
    if orient_towards is None:
        return None
    v = np.asarray(orient_towards)
    if v.shape != (3,) or v.dtype.kind not in "fiu":
        raise ValueError(f"orient_towards must be three real numbers, or None (got {orient_towards!r})")
    v = np.ascontiguousarray(v, dtype=np.float64)
    _finite(v, "orient_towards")
    return v


def estimate_normals_resident(d_points, n, k=20, orient_towards=None, f64=True, out=None):
    """pb3d_point_normals_resident on the rows of pb3d_knn_dev: a DeviceBuffer of n x 3 float64 unit normals of the resident (n, 3) list
    (float64 rows, or float32 with f64 False; finite).  Two host waits: the search's box and the index check."""
    from .eval_helpers import knn_resident
    n = int(n)
    k = _normals_k(k, n)
    v = _viewpoint(orient_towards)
    with dev.Scope() as sc:
        _, d_idx = sc.adopt(knn_resident(d_points, n, d_points, n, k, f64, f64, dist=False))
        d_out = sc.result(out, n * 24)
        _lib.check(_lib.load().pb3d_point_normals_resident(_lib.ctx(), _ptr(d_points), int(bool(f64)), n, _ptr(d_idx), k,
                                                           None if v is None else _lib.p_dbl(v), _ptr(d_out)))
        return d_out


def estimate_normals(points, k=20, orient_towards=None):
    """float64 (n, 3): a unit normal per point of the cloud, the direction of least spread of its k nearest points (itself included;
    exact search, ties to the lowest index), on the device.  include/pb3d.h states the arithmetic to the bit.  orient_towards=None: the
    component of largest magnitude is positive; orient_towards=v: the normal points into the half space of the viewpoint v.
    ValueError for k < 3, k > KNN_MAX_K, fewer than k points or non-finite input.  float32 clouds stay float32 on the device."""
    p, pf = _cloud(points, "points")
    _normals_k(k, len(p))
    _viewpoint(orient_towards)
    _finite(p, "points")
    with dev.Scope() as sc:
        d_out = sc.adopt(estimate_normals_resident(sc.upload(p), len(p), k, orient_towards, pf))
        return d_out.download((len(p), 3), np.float64)


METHODS = ("point_to_point", "point_to_plane")


def _method_args(method, with_scale, normals_k, nt, have_normals):
    """True for the plane method, after its checks"""
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS} (got {method!r})")
    if method == "point_to_point":
        if have_normals:
            raise ValueError("target_normals are only read with method='point_to_plane'")
        return False
    if with_scale:
        raise ValueError("with_scale=True needs method='point_to_point': the point-to-plane step is rigid")
    if not have_normals:
        _normals_k(normals_k, nt)
    return True


def _trim_args(trim_fraction, with_scale):
    """(rho or None, with_scale): both defaults -> (None, False), today's path"""
    if not isinstance(with_scale, (bool, np.bool_)):
        raise ValueError(f"with_scale must be a bool (got {with_scale!r})")
    if trim_fraction is None:
        return None, bool(with_scale)
    if isinstance(trim_fraction, (bool, np.bool_)) or not isinstance(trim_fraction, (int, float, np.integer, np.floating)):
        raise ValueError(f"trim_fraction must be a real number in (0, 1], or None (got {trim_fraction!r})")
    rho = float(trim_fraction)
    if not (0.0 < rho <= 1.0):
        raise ValueError(f"trim_fraction must be in (0, 1], or None (got {trim_fraction})")
    return rho, bool(with_scale)


def _icp_args(ns, nt, max_iterations, tolerance, max_distance, init):
    if isinstance(max_iterations, (bool, np.bool_)) or not isinstance(max_iterations, (int, np.integer)) or max_iterations < 1:
        raise ValueError(f"max_iterations must be a positive integer (got {max_iterations!r})")
    tolerance = float(tolerance)
    if not tolerance >= 0.0:
        raise ValueError(f"tolerance must be >= 0 (got {tolerance})")
    if max_distance is None:
        md2 = -1.0
    else:
        md = float(max_distance)
        if not (md >= 0.0 and math.isfinite(md)):
            raise ValueError(f"max_distance must be finite and >= 0, or None (got {max_distance})")
        md2 = md * md
    T = np.eye(4) if init is None else _transform(init, "init")
    if nt == 0:
        raise ValueError("icp_align: the target cloud is empty")
    if ns < 3:
        raise ValueError(f"icp_align: a rigid fit needs at least 3 point pairs (the source has {ns} points)")
    return int(max_iterations), tolerance, md2, T


def icp_align_resident(d_source, ns, d_target, nt, max_iterations=50, tolerance=1e-9, max_distance=None, init=None, return_history=False,
                       s_f64=True, t_f64=True, trim_fraction=None, with_scale=False, method="point_to_point", target_normals=None,
                       normals_k=20):
    """icp_align on resident (ns, 3) / (nt, 3) lists (DeviceBuffers; float64 rows, or float32 with s_f64 / t_f64 False).  The target
    is binned once; every iteration enqueues one step and downloads its 17 values (20 with trim_fraction or with_scale: the trimmed
    step, whose history entries are (count, rmse, candidates, tau)).  method="point_to_plane": target_normals is a DeviceBuffer of nt x 3
    float64, or None to estimate them here from the normals_k nearest neighbours; an iteration downloads 32 values."""
    max_iterations, tolerance, md2, T = _icp_args(int(ns), int(nt), max_iterations, tolerance, max_distance, init)
    rho, with_scale = _trim_args(trim_fraction, with_scale)
    if _method_args(method, with_scale, normals_k, int(nt), target_normals is not None):
        return _icp_plane(d_source, ns, d_target, nt, max_iterations, tolerance, md2, T, return_history, s_f64, t_f64, rho, target_normals,
                          normals_k)
    trimmed = rho is not None or with_scale
    box = icp_index_resident(d_target, nt, t_f64)               # the only index build of the alignment
    c = 0.5 * (box[:3] + box[3:])
    words = 20 if trimmed else 17
    history, Ts, prev = [], [], None
    with dev.Scope() as sc:
        d_out = sc.alloc(words * 8)
        for _ in range(max_iterations):
            if trimmed:
                icp_step_trimmed_resident(d_source, ns, d_target, nt, T, md2, 1.0 if rho is None else rho, c, c, s_f64, t_f64, out=d_out)
            else:
                icp_step_resident(d_source, ns, d_target, nt, T, md2, c, c, s_f64, t_f64, out=d_out)
            raw = d_out.download((words,), np.float64)
            count, sums = int(raw[:1].view(np.int64)[0]), raw[1:words - 2] if trimmed else raw[1:]
            if count < 3:
                raise ValueError(f"icp_align: only {count} point pairs within max_distance (a rigid fit needs 3)")
            rmse = math.sqrt(sums[15] / count)
            if trimmed:
                T = best_fit_similarity_from_sums(count, sums, c, c, with_scale) @ T
                history.append((count, rmse, int(raw[18:19].view(np.int64)[0]), float(raw[19])))
            else:
                T = best_fit_transform_from_sums(count, sums, c, c) @ T
                history.append((count, rmse))
            Ts.append(T)
            if prev is not None and abs(prev - rmse) < tolerance:
                break
            prev = rmse
    return (T, history, Ts) if return_history else T


def _icp_plane(d_source, ns, d_target, nt, max_iterations, tolerance, md2, T, return_history, s_f64, t_f64, rho, d_normals, normals_k):
    """the point-to-plane loop of icp_align_resident, its arguments checked"""
    history, Ts, prev = [], [], None
    with dev.Scope() as sc:
        if d_normals is None:
            d_normals = sc.adopt(estimate_normals_resident(d_target, nt, normals_k, None, t_f64))     # once per alignment
        box = icp_index_resident(d_target, nt, t_f64)
        c = 0.5 * (box[:3] + box[3:])
        d_out = sc.alloc(32 * 8)
        for _ in range(max_iterations):
            icp_step_plane_resident(d_source, ns, d_target, nt, d_normals, T, md2, rho, c, s_f64, t_f64, out=d_out)
            raw = d_out.download((32,), np.float64)
            count, sums = int(raw[:1].view(np.int64)[0]), raw[1:30]
            if count < 6:
                raise ValueError(f"icp_align: only {count} point pairs within max_distance (a point-to-plane fit needs 6)")
            rmse_plane, rmse_point = math.sqrt(sums[27] / count), math.sqrt(sums[28] / count)
            step, rank = plane_step_from_sums(count, sums, c)
            T = step @ T
            entry = (count, rmse_plane, rmse_point, rank)
            history.append(entry if rho is None else entry + (int(raw[30:31].view(np.int64)[0]), float(raw[31])))
            Ts.append(T)
            if prev is not None and abs(prev - rmse_plane) < tolerance:
                break
            prev = rmse_plane
    return (T, history, Ts) if return_history else T


def _target_normals(target_normals, nt):
    """float64 (nt, 3), finite, or None"""
    if target_normals is None:
        return None
    n = np.asarray(target_normals)
    if n.shape != (nt, 3) or n.dtype.kind not in "fiu":
        raise ValueError(f"target_normals must be a real ({nt}, 3) array, one row per target point (got shape {n.shape}, dtype {n.dtype})")
    n = np.ascontiguousarray(n, dtype=np.float64)
    _finite(n, "target_normals")
    return n


def icp_align(source, target, max_iterations=50, tolerance=1e-9, max_distance=None, init=None, return_history=False, trim_fraction=None,
              with_scale=False, method="point_to_point", target_normals=None, normals_k=20):
    """Rigid point-to-point ICP: the float64 4 x 4 T that moves `source` onto `target` (transform_points(source, T) ~ target).

    Every iteration pairs each transformed source point with its exact nearest target point (ties to the lowest index), drops the pairs
    farther apart than max_distance (None: keeps all), fits the best rigid motion of the pairs and composes it: T = step @ T.  It stops
    after the update once the pairs' RMS distance changed by less than `tolerance` from the iteration before, or after max_iterations.
    ValueError when an iteration has fewer than 3 pairs.  return_history=True: (T, [(count, rmse) per iteration], [T per iteration]).
    Both clouds are uploaded once and the target is indexed once; an iteration moves 17 numbers to the host.  float32 clouds stay
    float32 on the device (widened there), other real dtypes become float64; the arithmetic is float64 throughout.

    trim_fraction (a real number in (0, 1]): trimmed ICP for a source that carries clutter or overlaps the target only partly.  Of the
    m pairs that pass max_distance an iteration uses the k = ceil(trim_fraction * m) closest, and every pair tied with the k-th; the
    k-th smallest squared distance tau is found exactly on the device, with no host wait.  with_scale=True: a similarity fit -- each
    iteration also estimates one scale (Umeyama), and the upper 3 x 3 of T is s R.  A similarity fit needs a sensible `init`: trimmed
    pairs plus a free scale can shrink a badly placed source onto a few target points.  With either argument an iteration moves 20
    numbers, and the history entries are (count, rmse, candidates, tau); with both left at their defaults nothing changes.

    method="point_to_plane": every iteration minimises the pairs' distances along the TARGET's normals instead of the distances
    themselves, so two samplings of one smooth surface may slide along each other: a facade registers in a handful of iterations
    where point-to-point pairs creep.  target_normals: a finite (nt, 3) array, one row per target point, of any orientation (the step
    is even in the normal); None: estimated once on the device from the normals_k nearest target points (estimate_normals).  Each
    iteration moves 32 numbers, solves a 6 x 6 system with a cut-off pseudo-inverse (plane_step_from_sums: a flat target leaves rank 3
    and the source is moved into the plane, not along it) and stops once the RMS plane distance changed by less than `tolerance`.
    History entries are (count, rmse_plane, rmse_point, rank), with (candidates, tau) appended under trim_fraction.  The method is
    rigid: with_scale=True is a ValueError.  An iteration needs 6 pairs."""
    s, sf = _cloud(source, "source")
    t, tf = _cloud(target, "target")
    _finite(s, "source")
    _finite(t, "target")
    _icp_args(len(s), len(t), max_iterations, tolerance, max_distance, init)
    _, scaled = _trim_args(trim_fraction, with_scale)
    _method_args(method, scaled, normals_k, len(t), target_normals is not None)
    nrm = _target_normals(target_normals, len(t))
    with dev.Scope() as sc:
        d_s = sc.upload(s)
        d_t = d_s if target is source else sc.upload(t)
        d_n = None if nrm is None else sc.upload(nrm)
        return icp_align_resident(d_s, len(s), d_t, len(t), max_iterations, tolerance, max_distance, init, return_history, sf, tf,
                                  trim_fraction, with_scale, method, d_n, normals_k)


# ---- facade plane, box crop, four-way completion ---------------------------------------------------------------------------------------
MAX_HYPOTHESES = 4096


def plane_hypotheses_resident(d_P, n, d_triplets, K, f64=True, out=None):
    """pb3d_plane_hypotheses_resident: a DeviceBuffer of K x 4 float64, row k the plane (unit normal, d) through the three points of the
    resident (n, 3) list that the resident int64 triplet k names; four NaNs for a degenerate or out-of-range triplet"""
    with dev.Scope() as sc:
        d_out = sc.result(out, max(1, int(K)) * 32)
        _lib.check(_lib.load().pb3d_plane_hypotheses_resident(_lib.ctx(), _ptr(d_P), int(bool(f64)), int(n), _ptr(d_triplets), int(K), _ptr(d_out)))
        return d_out


def plane_score_resident(d_P, n, d_planes, K, tau, f64=True, out=None):
    """pb3d_plane_score_resident: a DeviceBuffer of K int64, the number of points within tau of each of the K resident plane rows"""
    with dev.Scope() as sc:
        d_out = sc.result(out, max(1, int(K)) * 8)
        _lib.check(_lib.load().pb3d_plane_score_resident(_lib.ctx(), _ptr(d_P), int(bool(f64)), int(n), _ptr(d_planes), int(K), float(tau), _ptr(d_out)))
        return d_out


def plane_moments_resident(d_P, n, plane, tau, pivot, f64=True, out=None):
    """pb3d_plane_moments_resident: a DeviceBuffer of 12 x 8 bytes -- the int64 count of the points within tau of `plane` (a, b, c, d)
    and the 11 float64 sums of a refit about `pivot`"""
    plane = np.ascontiguousarray(plane, dtype=np.float64).reshape(4)
    pivot = np.ascontiguousarray(pivot, dtype=np.float64).reshape(3)
    with dev.Scope() as sc:
        d_out = sc.result(out, 12 * 8)
        _lib.check(_lib.load().pb3d_plane_moments_resident(_lib.ctx(), _ptr(d_P), int(bool(f64)), int(n), _lib.p_dbl(plane), float(tau),
                                                           _lib.p_dbl(pivot), _ptr(d_out)))
        return d_out


def _box(lo, hi):
    lo = np.ascontiguousarray(lo, dtype=np.float64).reshape(3)
    hi = np.ascontiguousarray(hi, dtype=np.float64).reshape(3)
    if np.isnan(lo).any() or np.isnan(hi).any():
        raise ValueError("crop_to_box: a box corner is NaN")
    return lo, hi


def crop_to_box_resident(d_P, n, lo, hi, f64=True, out=None, index=None):
    """pb3d_points_crop_box_resident: (d_out, count) -- the rows of the resident (n, 3) list inside the closed box [lo, hi], in their
    order and dtype, at the front of d_out (a DeviceBuffer of n rows; allocated when `out` is None).  index: a DeviceBuffer of n int32
    that receives the surviving rows' positions, or None.  The count is downloaded (the one host wait)."""
    lo, hi = _box(lo, hi)
    row = 24 if f64 else 12
    with dev.Scope() as sc:
        d_out = sc.result(out, max(1, int(n)) * row)
        d_count = sc.alloc(8)
        _lib.check(_lib.load().pb3d_points_crop_box_resident(_lib.ctx(), _ptr(d_P), int(bool(f64)), int(n), _lib.p_dbl(lo), _lib.p_dbl(hi),
                                                             _ptr(d_out), _ptr(index), _ptr(d_count)))
        return d_out, int(d_count.download((1,), np.int64)[0])


def crop_to_box(points, lo, hi, return_index=False):
    """points[mask] for mask = all(lo <= p) & all(p <= hi) per row (the box is closed, a NaN coordinate fails), compacted on the device;
    float32 clouds stay float32, other real dtypes become float64.  return_index=True: (cropped, np.flatnonzero(mask))."""
    p, pf = _cloud(points, "points")
    lo, hi = _box(lo, hi)
    n = len(p)
    if n == 0:
        return (p.copy(), np.zeros(0, np.intp)) if return_index else p.copy()
    with dev.Scope() as sc:
        d_p = sc.upload(p)
        d_idx = sc.alloc(n * 4) if return_index else None
        d_out, count = crop_to_box_resident(d_p, n, lo, hi, pf, index=d_idx)
        sc.adopt(d_out)
        out = d_out.download((count, 3), p.dtype) if count else np.zeros((0, 3), p.dtype)
        if not return_index:
            return out
        idx = d_idx.download((count,), np.int32) if count else np.zeros(0, np.int32)
        return out, idx.astype(np.intp)


def plane_from_moments(count, sums, pivot):
    """(normal, d, eigenvalues) of the least-squares plane of the points a refit summed: sums[0:3] = sum(p - pivot), sums[3:9] =
    sum of (P.x*P.x, P.x*P.y, P.x*P.z, P.y*P.y, P.y*P.z, P.z*P.z) (later values are not read).  m = S / count,
    Cov = (S2 - outer(S, S) / count) / count; the normal is np.linalg.eigh's eigenvector of the smallest eigenvalue, signed so that its
    component of largest magnitude (the lowest axis on a tie) is positive; d = -normal . (m + pivot).  Eigenvalues ascending."""
    count = int(count)
    sums = np.asarray(sums, np.float64).reshape(-1)
    pivot = np.asarray(pivot, np.float64).reshape(3)
    if count < 3:
        raise ValueError(f"a plane fit needs at least 3 points (got {count})")
    S = sums[0:3]
    xx, xy, xz, yy, yz, zz = sums[3:9]
    S2 = np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]])
    m = S / count
    cov = (S2 - np.outer(S, S) / count) / count
    ev, vec = np.linalg.eigh(cov)
    nrm = vec[:, 0].copy()
    if nrm[int(np.argmax(np.abs(nrm)))] < 0.0:
        nrm = -nrm
    c = m + pivot
    d = -((nrm[0] * c[0] + nrm[1] * c[1]) + nrm[2] * c[2])
    return nrm, float(d), ev


def _ransac_args(n, inlier_threshold, num_hypotheses, refine_iterations):
    tau = float(inlier_threshold)
    if not (tau >= 0.0 and math.isfinite(tau)):
        raise ValueError(f"inlier_threshold must be finite and >= 0 (got {inlier_threshold})")
    for name, v, lo in (("num_hypotheses", num_hypotheses, 1), ("refine_iterations", refine_iterations, 0)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < lo:
            raise ValueError(f"{name} must be an integer >= {lo} (got {v!r})")
    if num_hypotheses > MAX_HYPOTHESES:
        raise ValueError(f"num_hypotheses must be in [1, {MAX_HYPOTHESES}] (got {num_hypotheses})")
    if n < 3:
        raise ValueError(f"fit_plane_ransac: a plane needs at least 3 points (got {n})")
    return tau, int(num_hypotheses), int(refine_iterations)


def fit_plane_ransac_resident(d_P, n, inlier_threshold, num_hypotheses=1024, seed=0, refine_iterations=2, return_history=False, f64=True):
    """fit_plane_ransac on a resident (n, 3) list (a DeviceBuffer; float64 rows, or float32 with f64 False).  One upload of the
    triplets, the hypotheses and score entries, one download of K planes and K counts; then per refit one moments call about the box
    centre (pb3d_points_bounds_dev, once) and a download of its 12 numbers.  The coordinates must be finite (not checked here)."""
    n = int(n)
    tau, K, refits = _ransac_args(n, inlier_threshold, num_hypotheses, refine_iterations)
    triplets = np.random.default_rng(seed).integers(0, n, size=(K, 3), dtype=np.int64)
    with dev.Scope() as sc:
        d_trip = sc.upload(triplets)
        d_pc = sc.alloc(K * 40)                                     # K x 4 planes, then K counts: one download
        plane_hypotheses_resident(d_P, n, d_trip, K, f64, out=d_pc.at(0))
        plane_score_resident(d_P, n, d_pc.at(0), K, tau, f64, out=d_pc.at(K * 32))
        raw = d_pc.download((K * 5,), np.float64)
        planes, counts = raw[:4 * K].reshape(K, 4).copy(), raw[4 * K:].view(np.int64).copy()
        best = int(np.argmax(counts))                               # the first maximum: ties go to the lowest k
        if counts[best] < 3:
            raise ValueError(f"fit_plane_ransac: the best hypothesis has {int(counts[best])} inliers (a plane needs 3)")
        normal, d, inliers = planes[best, :3].copy(), float(planes[best, 3]), int(counts[best])
        refit_log = []
        if refits:
            d_box = sc.alloc(48)
            _lib.check(_lib.load().pb3d_points_bounds_dev(_lib.ctx(), _ptr(d_P), int(bool(f64)), n, _ptr(d_box)))
            box = d_box.download((6,), np.float64)
            pivot = 0.5 * (box[:3] + box[3:])
            d_mom = sc.alloc(12 * 8)
            for _ in range(refits):
                plane_moments_resident(d_P, n, (normal[0], normal[1], normal[2], d), tau, pivot, f64, out=d_mom)
                raw = d_mom.download((12,), np.float64)
                count, sums = int(raw[:1].view(np.int64)[0]), raw[1:].copy()
                if count < 3:
                    raise ValueError(f"fit_plane_ransac: a refit found only {count} inliers (a plane needs 3)")
                normal, d, _ = plane_from_moments(count, sums, pivot)
                refit_log.append((count, sums, normal, d))
            # the inliers of the plane that is returned: one more sweep, of one plane
            d_one = sc.upload(np.array([normal[0], normal[1], normal[2], d], np.float64))
            plane_score_resident(d_P, n, d_one, 1, tau, f64, out=d_pc.at(K * 32))
            inliers = int(d_pc.download((1,), np.int64, K * 32)[0])
    if return_history:
        return normal, d, inliers, {"triplets": triplets, "planes": planes, "counts": counts, "best": best, "refits": refit_log}
    return normal, d, inliers


def fit_plane_ransac(points, inlier_threshold, num_hypotheses=1024, seed=0, refine_iterations=2, return_history=False):
    """The dominant plane of a cloud by RANSAC: (normal, d, inlier_count) with normal . p + d = 0, |normal| = 1.

    num_hypotheses planes through the point triplets np.random.default_rng(seed).integers(0, n, size=(K, 3), dtype=np.int64) are
    scored by the number of points within inlier_threshold of them (all K in one sweep of the resident cloud); the best has the highest
    count, ties to the lowest k.  Each of the refine_iterations refits replaces the plane by the least-squares plane of its inliers
    (plane_from_moments of the device's sums about the box centre).  inlier_count is the number of points within the threshold of the
    plane that is returned.  return_history=True adds a dict: triplets, planes (K x 4, NaN rows for degenerate triplets), counts, best
    and refits = [(count, sums, normal, d) per refit].  ValueError for fewer than 3 points, a threshold that is negative or not finite,
    K outside [1, 4096], points that are not finite, or fewer than 3 inliers at any stage.  float32 clouds stay float32 on the device."""
    p, pf = _cloud(points, "points")
    _ransac_args(len(p), inlier_threshold, num_hypotheses, refine_iterations)
    _finite(p, "points")
    with dev.Scope() as sc:
        return fit_plane_ransac_resident(sc.upload(p), len(p), inlier_threshold, num_hypotheses, seed, refine_iterations, return_history, pf)


def plane_alignment_transform(normal, d):
    """float64 4 x 4 [R | t]: R is the rotation about normal x (0, 0, 1) (Rodrigues) that takes `normal` to (0, 0, 1), t = (0, 0, d),
    so the plane normal . p + d = 0 lands on z = 0 (apply it with transform_points).  A normal of exactly (0, 0, -1) takes the half
    turn about x.  The normal is normalised first (and d with it)."""
    nrm = np.asarray(normal, np.float64).reshape(3)
    L = math.sqrt(float((nrm[0] * nrm[0] + nrm[1] * nrm[1]) + nrm[2] * nrm[2]))
    d = float(d)
    if not (L > 0.0 and math.isfinite(L) and math.isfinite(d)):
        raise ValueError("plane_alignment_transform: the plane must be finite with a non-zero normal")
    x, y, z = (float(v) / L for v in nrm)
    M = np.eye(4)
    s2 = x * x + y * y
    if s2 == 0.0 and z < 0.0:
        M[1, 1] = M[2, 2] = -1.0
    else:
        a, b = y, -x                                # v = normal x (0, 0, 1) = (a, b, 0); R = I + [v]x + [v]x^2 / (1 + z)
        h = 1.0 / (1.0 + z) if z >= 0.0 else (1.0 - z) / s2      # the same number, without the cancellation next to z = -1
        M[:3, :3] = [[1.0 - h * b * b, h * a * b, b], [h * a * b, 1.0 - h * a * a, -a], [-b, a, z]]
    M[2, 3] = d / L
    return M


_QUARTER = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])       # a quarter turn about +Y: (x, y, z) -> (z, y, -x)


def quarter_turn_transforms(centre):
    """the four float64 4 x 4 of symmetric_completion: R_q = q quarter turns about Y (entries exactly 0 / +-1), t = c - R_q c for
    c = (cx, 0, cz)"""
    cx, cz = (float(v) for v in np.asarray(centre, np.float64).reshape(2))
    if not (math.isfinite(cx) and math.isfinite(cz)):
        raise ValueError("symmetric_completion: the centre must be finite")
    c = np.array([cx, 0.0, cz])
    out, R = [], np.eye(3)
    for _ in range(4):
        M = np.eye(4)
        M[:3, :3] = R + 0.0                         # + 0.0: no -0.0 entries
        M[:3, 3] = c - M[:3, :3] @ c
        out.append(M)
        R = _QUARTER @ R
    return out


def symmetric_completion_resident(d_P, n, centre=None, f64=True):
    """symmetric_completion on a resident (n, 3) list: a DeviceBuffer of 4n x 3 float64 (four transform_points_resident calls)"""
    n = int(n)
    if centre is None:
        if n < 1:
            raise ValueError("symmetric_completion: an empty cloud has no box; give a centre")
        with dev.Scope() as sc:
            d_box = sc.alloc(48)
            _lib.check(_lib.load().pb3d_points_bounds_dev(_lib.ctx(), _ptr(d_P), int(bool(f64)), n, _ptr(d_box)))
            box = d_box.download((6,), np.float64)
        centre = (0.5 * (box[0] + box[3]), 0.5 * (box[2] + box[5]))
    Ts = quarter_turn_transforms(centre)
    with dev.Scope() as sc:
        d_out = sc.result(None, max(1, 4 * n) * 24)
        for q, T in enumerate(Ts):
            transform_points_resident(d_P, n, T, f64, out=d_out.at(q * n * 24))
        return d_out


def symmetric_completion(points, centre=None):
    """The naive four-way completion of a facade cloud: float64 (4n, 3), rows [q n, (q + 1) n) the cloud turned by q quarter turns about
    the axis parallel to Y through centre = (cx, cz) (default: the x / z centre of the cloud's box).  Copy 0 is the input widened to
    float64 (a -0.0 coordinate comes out as +0.0)."""
    p, pf = _cloud(points, "points")
    _finite(p, "points")
    n = len(p)
    if n == 0:
        return np.zeros((0, 3), np.float64)
    with dev.Scope() as sc:
        d_out = sc.adopt(symmetric_completion_resident(sc.upload(p), n, centre, pf))
        return d_out.download((4 * n, 3), np.float64)
