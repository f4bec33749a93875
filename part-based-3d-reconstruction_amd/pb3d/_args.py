"""The argument checks more than one module of the package uses.  Nothing here touches the device: a wrapper runs its checks first, so an
argument error is raised before any device work.  Two checks are one only where they accept and reject the same inputs with the same
exception and message; where they differ both stand here, each saying who needs it."""
import math

import numpy as np

from . import _lib, projection_utils
from .device import DeviceGrid

MAX_POINTS = 2 ** 31 - 1
MAX_VERTICES = 2 ** 31 - 1
MAX_FACES = (2 ** 31 - 1) // 6


# ---- point clouds ------------------------------------------------------------------------------------------------------------------------
def _cloud(P, what="points"):
    """(n, 3) array the kernels read: float32 stays float32 (widened on the device), anything else real becomes float64 -- what the
    trees do with it.  Integer coordinates must satisfy |v| < 2^53 to convert exactly."""
    a = np.asarray(P)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError(f"{what} must be an (n, 3) array (got shape {a.shape})")
    if a.dtype == np.float32:
        return np.ascontiguousarray(a), 0
    if a.dtype.kind not in "fiu" or a.dtype.itemsize > 8:
        raise TypeError(f"{what}: unsupported dtype {a.dtype}")
    return np.ascontiguousarray(a, dtype=np.float64), 1


def _count(n):
    n = int(n)
    if not 0 <= n <= MAX_POINTS:
        raise ValueError(f"a point list holds at most 2^31 - 1 points (got {n})")
    return n


def _sized_cloud(points):
    """_cloud with the size checked on the shape, before any copy (select_points: the cloud may hold non-finite rows)"""
    shape = np.shape(points)
    if len(shape) == 2 and shape[1] == 3:
        _count(shape[0])
    return _cloud(points, "points")


def _finite_cloud(points):
    """_sized_cloud of a finite cloud (cluster_points and its kin, voxel_downsample)"""
    p, pf = _sized_cloud(points)
    if not np.isfinite(p).all():
        raise ValueError("Input points contains NaN or infinity.")
    return p, pf


def _voxel_size(voxel_size):
    vs = float(voxel_size)
    if not math.isfinite(vs) or vs <= 0.0:
        raise ValueError(f"voxel_size must be finite and > 0 (got {voxel_size!r})")
    return vs


# ---- meshes ------------------------------------------------------------------------------------------------------------------------------
def _counts(nv, nf):
    nv, nf = int(nv), int(nf)
    if not 0 <= nv <= MAX_VERTICES:
        raise ValueError(f"a mesh holds at most 2^31 - 1 vertices (got {nv})")
    if not 0 <= nf <= MAX_FACES:
        raise ValueError(f"a mesh holds at most (2^31 - 1) / 6 faces (got {nf})")
    return nv, nf


def _faces(faces, nv):
    """(contiguous (nf, 3) int32 or int64 array, i64 flag); int32 and int64 go as they are, other integer types become int64"""
    f = np.asarray(faces)
    if f.dtype.kind not in "iu":
        raise IndexError("arrays used as indices must be of integer (or boolean) type")
    if f.ndim != 2 or f.shape[1] != 3:
        raise ValueError(f"faces must be an (m, 3) array (got shape {f.shape})")
    _counts(nv, f.shape[0])
    if f.dtype.kind == "u" and f.size and int(f.max()) >= nv:           # before the cast to int64 could wrap it
        raise IndexError(f"index {int(f.max())} is out of bounds for axis 0 with size {nv}")
    if f.dtype == np.int32:
        return np.ascontiguousarray(f), 0
    return np.ascontiguousarray(f, dtype=np.int64), 1


def _mesh(vertices, faces):
    """(vertices, f64 flag, faces, i64 flag) of a mesh (voxelize_mesh, mesh_grid_iou, render_mesh, mesh_projection_iou)"""
    v, vf = _cloud(vertices, "vertices")
    f, fi = _faces(faces, len(v))
    if len(v) == 0 and len(f):
        raise IndexError(f"index {int(f.reshape(-1)[0])} is out of bounds for axis 0 with size 0")
    return v, vf, f, fi


# ---- voxel grids: three checks that differ in what they return -----------------------------------------------------------------------------
def _grid_channels(g, what):
    """(channels, lattice shape) of a uint8 (n0, n1, n2[, 1 or 3]) array or DeviceGrid, TypeError on another dtype (voxelize.py,
    distance.py)"""
    if not isinstance(g, DeviceGrid) and np.asarray(g).dtype != np.uint8:
        raise TypeError(f"{what} must be a uint8 array (got {np.asarray(g).dtype})")
    shape = tuple(g.shape if isinstance(g, DeviceGrid) else np.shape(g))
    if len(shape) not in (3, 4) or (len(shape) == 4 and shape[3] not in (1, 3)):
        raise ValueError(f"{what} must have shape (n0, n1, n2) or (n0, n1, n2, 3) (got {shape})")
    return (shape[3] if len(shape) == 4 else 1), shape[:3]


def _grid_shape(voxel_grid):
    """the shape as given, (A0, A1, A2, 3) or (A0, A1, A2), of an array of any dtype or a DeviceGrid (perspective.py, before its other
    checks)"""
    grid_shape = tuple(voxel_grid.shape if isinstance(voxel_grid, DeviceGrid) else np.shape(voxel_grid))
    if len(grid_shape) not in (3, 4) or (len(grid_shape) == 4 and grid_shape[3] != 3):
        raise ValueError("voxel_grid must be (A0,A1,A2,3) RGB or (A0,A1,A2) labels")
    return grid_shape


def _grid(voxel_grid):
    """(the DeviceGrid itself or the contiguous uint8 array to upload, (A0, A1, A2, C)) of a NumPy grid ((A0,A1,A2,3) RGB or (A0,A1,A2)
    labels) or a DeviceGrid (eval_helpers_intra.py, perspective.py, minarets.py); _on_device puts it there"""
    g = voxel_grid if isinstance(voxel_grid, DeviceGrid) else _lib.as_u8(voxel_grid, "voxel_grid")
    shape = tuple(g.shape)
    if len(shape) == 3:
        shape = shape + (1,)
    if len(shape) != 4 or shape[3] not in (1, 3):
        raise ValueError("voxel_grid must be (A0,A1,A2,3) RGB or (A0,A1,A2) labels")
    return g, tuple(int(v) for v in shape)


def _on_device(sc, g):
    """the buffer of a checked grid: a DeviceGrid's own, which stays its owner's, or an upload the scope `sc` owns (None for an empty
    array)"""
    return g.buf if isinstance(g, DeviceGrid) else sc.upload(g)


# ---- colour tables and cameras of the grid passes (eval_helpers_intra.py, perspective.py) --------------------------------------------------
def _colour_table(colors, C):
    t = np.ascontiguousarray(np.asarray(colors, dtype=np.int64).reshape(-1, C) if len(colors) else np.zeros((0, C), np.int64))
    if t.size and (t.min() < 0 or t.max() > 255):
        raise ValueError("colours are uint8 values")
    return np.ascontiguousarray(t.astype(np.uint8))


def _cam(cam, pts_dtype):
    _, _, R, cp, prec = projection_utils.camera_args(np.zeros((1, 3), pts_dtype), cam["cam_pos"], cam["target"], cam["f"], cam["cx"], cam["cy"])
    return R, cp, prec


def _eps_f32(prec, eps):
    return int((not prec[0]) and not projection_utils._promotes_to_f64(eps))
