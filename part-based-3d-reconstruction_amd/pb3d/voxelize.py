"""Mesh -> grid: exact solid voxelization of a triangle mesh on the device, and the volume overlap of two grids.  It is the conversion the
package lacked: with it a mesh (a CAD model, a smoothed marching-cubes mesh) becomes an occupancy, label or RGB grid that perspective_carve,
perspective_paint, the labelling, the point extraction and notebook 3's deformation loop take as it is, and it can be compared volume
against volume with a carved grid (mesh_grid_iou).

include/pb3d.h states the result to the bit.  Voxel (i, j, k) is the sample point origin + voxel_size * (i, j, k); a ray along the last
axis through each column (i, j) is crossed by the faces whose projection holds the column, ties on edges and vertices decided by a
symbolic rule (the sample moved by the infinitesimal (-eps^2, +eps)), and a voxel is inside when the number of crossings at or below it is
odd.  All arithmetic is float64, one rounded operation each.  On marching-cubes output at unit voxel size every operation is exact, so
voxelize_mesh(*marching_cubes(mask)) gives the mask back (wherever the mask's border is empty: marching cubes leaves the surface open
there).  frame="meshify" reads vertices in the frame meshify_colored_voxel_grid hands out.

csrc/voxelize.hip: crossings are integer XOR atomics of single bits in a bit volume, a second pass scans each column and writes the
bytes -- no floating-point atomics, the result is a function of the input alone.  The NumPy forms upload the mesh and download the grid;
the *_resident twins take and return device handles (pb3d.device.DeviceBuffer)."""
import ctypes as C
import math

import numpy as np

from . import _lib, device as dev
from ._args import _counts, _grid_channels, _mesh, _on_device
from ._lib import _ptr

__all__ = ["voxelize_mesh", "voxelize_mesh_resident", "grid_overlap_counts", "grid_overlap_counts_resident", "mesh_grid_iou"]

MAX_VOXELS = 2 ** 31 - 1
FRAMES = ("lattice", "meshify")
STATS = ("crossings", "occupied", "open_columns", "flat_faces")


def _shape(shape):
    try:
        s = tuple(shape)
    except TypeError:
        raise ValueError(f"shape must be three integers (got {shape!r})") from None
    if len(s) != 3 or any(isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) for v in s):
        raise ValueError(f"shape must be three integers (got {shape!r})")
    s = tuple(int(v) for v in s)
    if min(s) < 1:
        raise ValueError(f"every axis of the grid must be >= 1 (got {s})")
    if s[0] * s[1] * s[2] > MAX_VOXELS:
        raise ValueError(f"a grid holds at most 2^31 - 1 voxels (got {s})")
    return s


def _placement(origin, voxel_size, frame, depth, shape):
    """(origin as three float64, voxel_size, frame number, depth) as the entry takes them"""
    o = np.asarray(origin, dtype=np.float64)
    if o.shape != (3,) or not np.all(np.isfinite(o)):
        raise ValueError(f"origin must be three finite numbers (got {origin!r})")
    vs = float(voxel_size)
    if not math.isfinite(vs) or vs <= 0.0:
        raise ValueError(f"voxel_size must be finite and > 0 (got {voxel_size!r})")
    if not isinstance(frame, str) or frame not in FRAMES:
        raise ValueError(f"frame must be 'lattice' or 'meshify' (got {frame!r})")
    d = float(shape[2] if depth is None else depth)
    if not math.isfinite(d):
        raise ValueError(f"depth must be finite (got {depth!r})")
    return np.ascontiguousarray(o), vs, FRAMES.index(frame), d


def _value(value):
    """the bytes inside voxels take: a scalar (one channel) or a triple (RGB)"""
    v = np.asarray(value)
    if v.shape not in ((), (3,)) or v.dtype.kind not in "iu":
        raise ValueError(f"value must be an integer in [0, 255] or a triple of them (got {value!r})")
    v = np.atleast_1d(v).astype(np.int64)
    if v.min() < 0 or v.max() > 255:
        raise ValueError(f"value must be an integer in [0, 255] or a triple of them (got {value!r})")
    return np.ascontiguousarray(v, dtype=np.uint8)


def voxelize_mesh_resident(d_verts, n_vertices, d_faces, n_faces, shape, origin=(0, 0, 0), voxel_size=1.0, frame="lattice", depth=None,
                           value=1, return_stats=False, verts_f64=False, faces_i64=False, out=None):
    """pb3d_voxelize_mesh_resident: a DeviceBuffer of shape[0] * shape[1] * shape[2] (x 3 when `value` is a triple) bytes, written whole --
    pb3d.device.meshify(..., download=False) hands out float32 vertices and int32 faces in frame="meshify".  With return_stats also the
    dict of crossings, occupied, open_columns and flat_faces (one more download).  Everything is enqueued behind the check of the indices
    (IndexError) and of the coordinates (ValueError on one that is not finite); `out` is untouched when it fails."""
    nv, nf = _counts(n_vertices, n_faces)
    s = _shape(shape)
    o, vs, fr, d = _placement(origin, voxel_size, frame, depth, s)
    val = _value(value)
    stats = (C.c_int64 * 4)() if return_stats else None
    with dev.Scope() as sc:
        d_out = sc.result(out, s[0] * s[1] * s[2] * len(val))
        _lib.check(_lib.load().pb3d_voxelize_mesh_resident(_lib.ctx(), _ptr(d_verts), int(bool(verts_f64)), nv, _ptr(d_faces), int(bool(faces_i64)),
                                                           nf, s[0], s[1], s[2], _lib.p_dbl(o), vs, fr, d, len(val), _lib.p_u8(val), _ptr(d_out),
                                                           stats))
        if return_stats:
            return d_out, dict(zip(STATS, (int(v) for v in stats)))
        return d_out


def voxelize_mesh(vertices, faces, shape, origin=(0, 0, 0), voxel_size=1.0, frame="lattice", depth=None, value=1, return_stats=False):
    """The solid an (n, 3) vertex array and an (m, 3) integer face array enclose, sampled at the points origin + voxel_size * (i, j, k) of a
    grid of `shape`: a uint8 array of `shape` holding `value` inside and 0 outside, or of shape + (3,) when `value` is an RGB triple.
    float32 vertices stay float32 (the arithmetic is float64), other real dtypes become float64; negative face indices wrap as NumPy's
    do.  frame="meshify" takes the vertices as meshify_colored_voxel_grid returns them (`depth` = the grid's last axis, default
    shape[2]).  return_stats adds the dict of crossings, occupied voxels, open_columns (columns whose crossings do not pair up: the mesh
    leaks there or leaves the grid's side) and flat_faces (faces the rays run parallel to)."""
    s = _shape(shape)
    _placement(origin, voxel_size, frame, depth, s)
    val = _value(value)
    v, vf, f, fi = _mesh(vertices, faces)
    with dev.Scope() as sc:
        res = voxelize_mesh_resident(sc.upload(v), len(v), sc.upload(f), len(f), s, origin, voxel_size, frame, depth, value, return_stats, vf, fi)
        d_out, stats = res if return_stats else (res, None)
        grid = sc.adopt(d_out).download(s if len(val) == 1 else s + (3,))
        return (grid, stats) if return_stats else grid


def grid_overlap_counts_resident(d_a, channels_a, d_b, channels_b, n_voxels):
    """pb3d_grid_overlap_resident: (inter, count_a, count_b) of two resident grids of n_voxels voxels, 1 or 3 bytes per voxel each"""
    out = (C.c_int64 * 3)()
    _lib.check(_lib.load().pb3d_grid_overlap_resident(_lib.ctx(), _ptr(d_a), int(channels_a), _ptr(d_b), int(channels_b), int(n_voxels), out))
    return int(out[0]), int(out[1]), int(out[2])


def grid_overlap_counts(a, b):
    """(inter, count_a, count_b): the voxels non-zero in both grids, in a and in b, where non-zero means any channel > 0.  a, b: uint8
    arrays or DeviceGrids of one lattice shape, each (n0, n1, n2) or (n0, n1, n2, 3)."""
    (ca, sa), (cb, sb) = _grid_channels(a, "a"), _grid_channels(b, "b")
    if sa != sb:
        raise ValueError(f"the grids differ in shape: {sa} and {sb}")
    with dev.Scope() as sc:
        return grid_overlap_counts_resident(_on_device(sc, a), ca, _on_device(sc, b), cb, sa[0] * sa[1] * sa[2])


def mesh_grid_iou(vertices, faces, grid, origin=(0, 0, 0), voxel_size=1.0, frame="lattice"):
    """Intersection over union of the solid a mesh encloses and the occupied voxels of `grid` (a uint8 array or DeviceGrid, (n0, n1, n2) or
    (n0, n1, n2, 3)), on the grid's lattice: voxelize_mesh and grid_overlap_counts composed, the voxelized mesh never leaving the
    device.  inter / union as one float64 division; 0.0 for an empty union."""
    v, vf, f, fi = _mesh(vertices, faces)
    ch, shape = _grid_channels(grid, "grid")
    with dev.Scope() as sc:
        d_g = _on_device(sc, grid)
        s = _shape(shape)
        d_m = sc.adopt(voxelize_mesh_resident(sc.upload(v), len(v), sc.upload(f), len(f), s, origin, voxel_size, frame, None, 1, False, vf, fi))
        inter, na, nb = grid_overlap_counts_resident(d_m, 1, d_g, ch, s[0] * s[1] * s[2])
        union = na + nb - inter
        return float(np.float64(inter) / np.float64(union)) if union else 0.0
