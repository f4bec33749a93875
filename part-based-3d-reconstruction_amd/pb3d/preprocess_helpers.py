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
(best_fit_transform_from_sums) and composes the transform.  The SfM preprocessing, the facade-plane fit and the symmetric completion
of that file are not mirrored."""
import ctypes as C
import math

import numpy as np

from . import _lib

__all__ = ["normalize_preserve_aspect", "flip_y_axis", "transform_points", "transform_points_resident", "best_fit_transform_from_sums",
           "icp_align", "icp_align_resident", "icp_index_resident", "icp_step_resident"]


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
def _cloud(P, what):
    from .eval_helpers import _cloud as cloud
    return cloud(P, what)


def _finite(a, what):
    if not np.isfinite(a).all():
        raise ValueError(f"Input {what} contains NaN or infinity.")


def _ptr(b):
    return None if b is None else C.c_void_p(b.ptr)


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
    from . import device as dev
    t = _t12(_transform(T))
    d_out = out if out is not None else dev.DeviceBuffer(max(1, int(n)) * 24)
    _lib.check(_lib.load().pb3d_transform_points_resident(_lib.ctx(), _ptr(d_P), int(bool(f64)), int(n), _lib.p_dbl(t), _ptr(d_out)))
    return d_out


def transform_points(P, T):
    """float64 (n, 3): row i = ((T[h,0]*x + T[h,1]*y) + T[h,2]*z) + T[h,3] of point i, for a 3 x 4 or 4 x 4 T, on the device"""
    from . import device as dev
    p, pf = _cloud(P, "P")
    t = _transform(T)
    if len(p) == 0:
        return np.zeros((0, 3), np.float64)
    d_p = dev.from_numpy(p)
    try:
        d_out = transform_points_resident(d_p, len(p), t, pf)
        try:
            return d_out.download((len(p), 3), np.float64)
        finally:
            d_out.free()
    finally:
        d_p.free()


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


def icp_index_resident(d_target, nt, f64=True):
    """pb3d_icp_index_resident: bin the resident (nt, 3) target for the steps that follow; returns its exact box (min 3, max 3)"""
    b = np.zeros(6, np.float64)
    _lib.check(_lib.load().pb3d_icp_index_resident(_lib.ctx(), _ptr(d_target), int(bool(f64)), int(nt), _lib.p_dbl(b)))
    return b


def icp_step_resident(d_source, ns, d_target, nt, T, max_dist2, cp, cq, s_f64=True, t_f64=True, out=None):
    """pb3d_icp_step_resident: a DeviceBuffer of 17 x 8 bytes -- the int64 count of used pairs and the 16 float64 sums of one step with
    the 4 x 4 (or 3 x 4) T against the index icp_index_resident built for this target.  max_dist2 < 0: no gate."""
    from . import device as dev
    t = _t12(np.asarray(T, np.float64))
    cp = np.ascontiguousarray(cp, dtype=np.float64).reshape(3)
    cq = np.ascontiguousarray(cq, dtype=np.float64).reshape(3)
    d_out = out if out is not None else dev.DeviceBuffer(17 * 8)
    _lib.check(_lib.load().pb3d_icp_step_resident(_lib.ctx(), _ptr(d_source), int(bool(s_f64)), int(ns), _ptr(d_target), int(bool(t_f64)),
                                                  int(nt), _lib.p_dbl(t), float(max_dist2), _lib.p_dbl(cp), _lib.p_dbl(cq), _ptr(d_out)))
    return d_out


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
                       s_f64=True, t_f64=True):
    """icp_align on resident (ns, 3) / (nt, 3) lists (DeviceBuffers; float64 rows, or float32 with s_f64 / t_f64 False).  The target
    is binned once; every iteration enqueues one step and downloads its 17 values."""
    from . import device as dev
    max_iterations, tolerance, md2, T = _icp_args(int(ns), int(nt), max_iterations, tolerance, max_distance, init)
    box = icp_index_resident(d_target, nt, t_f64)               # the only index build of the alignment
    c = 0.5 * (box[:3] + box[3:])
    d_out = dev.DeviceBuffer(17 * 8)
    history, Ts, prev = [], [], None
    try:
        for _ in range(max_iterations):
            icp_step_resident(d_source, ns, d_target, nt, T, md2, c, c, s_f64, t_f64, out=d_out)
            raw = d_out.download((17,), np.float64)
            count, sums = int(raw[:1].view(np.int64)[0]), raw[1:]
            if count < 3:
                raise ValueError(f"icp_align: only {count} point pairs within max_distance (a rigid fit needs 3)")
            rmse = math.sqrt(sums[15] / count)
            T = best_fit_transform_from_sums(count, sums, c, c) @ T
            history.append((count, rmse))
            Ts.append(T)
            if prev is not None and abs(prev - rmse) < tolerance:
                break
            prev = rmse
    finally:
        d_out.free()
    return (T, history, Ts) if return_history else T


def icp_align(source, target, max_iterations=50, tolerance=1e-9, max_distance=None, init=None, return_history=False):
    """Rigid point-to-point ICP: the float64 4 x 4 T that moves `source` onto `target` (transform_points(source, T) ~ target).

    Every iteration pairs each transformed source point with its exact nearest target point (ties to the lowest index), drops the pairs
    farther apart than max_distance (None: keeps all), fits the best rigid motion of the pairs and composes it: T = step @ T.  It stops
    after the update once the pairs' RMS distance changed by less than `tolerance` from the iteration before, or after max_iterations.
    ValueError when an iteration has fewer than 3 pairs.  return_history=True: (T, [(count, rmse) per iteration], [T per iteration]).
    Both clouds are uploaded once and the target is indexed once; an iteration moves 17 numbers to the host.  float32 clouds stay
    float32 on the device (widened there), other real dtypes become float64; the arithmetic is float64 throughout."""
    from . import device as dev
    s, sf = _cloud(source, "source")
    t, tf = _cloud(target, "target")
    _finite(s, "source")
    _finite(t, "target")
    _icp_args(len(s), len(t), max_iterations, tolerance, max_distance, init)
    d_s = dev.from_numpy(s)
    d_t = d_s if target is source else dev.from_numpy(t)
    try:
        return icp_align_resident(d_s, len(s), d_t, len(t), max_iterations, tolerance, max_distance, init, return_history, sf, tf)
    finally:
        d_s.free()
        if d_t is not d_s:
            d_t.free()
