"""Pinhole scatter projection of coloured voxels; host mirror of reference utils/projection_utils.py:5-23."""
import ctypes as C

import numpy as np

from . import _lib
from .camera_geometry import look_at_rotation, project  # noqa: F401

__all__ = ["project_colored_voxels"]


def _promotes_to_f64(v):
    """NumPy-2 promotion: Python scalars are weak, NumPy scalars / arrays carry their dtype."""
    if isinstance(v, (np.generic, np.ndarray)):
        return np.result_type(v, np.float32) == np.float64
    return False


def _promotion_flags(t0, f, cx, cy):
    """(t0, tm, tu, tv): the float64 flags of the projection's stages -- (p - cam) @ R.T, the scale by f, the shifts by cx
    and cy -- given t0, the flag of the first; each later stage is float64 if the one before it is or its scalar is."""
    tm = int(t0 or _promotes_to_f64(f))
    return int(t0), tm, int(tm or _promotes_to_f64(cx)), int(tm or _promotes_to_f64(cy))


def points_f64(dtype):
    """True for the point dtypes the kernels read as float64: float64 itself and the 32- and 64-bit integers, which NumPy
    promotes with any float camera to float64 (float32 would round their values from 2^24 on).  Narrower types are exact
    in float32."""
    return np.result_type(dtype, np.float32) == np.float64


def camera_args(pts3d, cam_pos, target, f, cx, cy):
    """Everything the projection kernels need from the caller's camera: the look-at rotation (host NumPy, same
    dtypes as upstream), the points in a float width that holds their values and the NumPy-2 promotion flags of each stage."""
    pts3d = np.asarray(pts3d)
    cam_pos = np.asarray(cam_pos)
    target = np.asarray(target)
    R = look_at_rotation(cam_pos, target)
    prec = (C.c_int * 4)(*_promotion_flags(np.result_type(pts3d, cam_pos, R) == np.float64, f, cx, cy))
    pf64 = int(points_f64(pts3d.dtype))
    return (np.ascontiguousarray(pts3d, np.float64 if pf64 else np.float32), pf64, np.ascontiguousarray(R, np.float64),
            np.ascontiguousarray(cam_pos, np.float64), prec)


def project_colored_voxels(pts3d, colors, cam_pos, target, f, cx, cy, H, W):
    """(H,W,3) uint8 image of the points seen from cam_pos looking at target; among points that
    land on one pixel the last in input order wins (NumPy fancy-assignment semantics)."""
    p, pf64, Rd, cd, prec = camera_args(pts3d, cam_pos, target, f, cx, cy)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("pts3d must be (N,3)")
    cols = np.ascontiguousarray(np.asarray(colors).astype(np.uint8, copy=False))
    if cols.shape != (p.shape[0], 3):
        raise ValueError("colors must be (N,3)")
    img = np.empty((int(H), int(W), 3), np.uint8)
    _lib.check(_lib.load().pb3d_project(_lib.ctx(), p.ctypes.data_as(C.c_void_p), pf64, _lib.p_u8(cols), p.shape[0],
                                        _lib.p_dbl(Rd), _lib.p_dbl(cd), float(f), float(cx), float(cy), prec,
                                        int(H), int(W), _lib.p_u8(img)))
    return img
