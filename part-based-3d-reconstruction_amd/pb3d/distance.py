"""Grid -> distance: the exact Euclidean distance transform of a voxel grid with its feature transform (the nearest voxel's index), and
what it gives a grid: dilation, erosion, closing and opening by a Euclidean ball (new voxels take the colour or label of the nearest
voxel) and the surface distances of two grids (Hausdorff, RMS, precision / recall / F-score), the volume-against-volume counterparts of
cloud_to_mesh_metrics.

include/pb3d.h states the result to the bit.  Squared distances on a lattice are integers: sq is int32, computed without a single
floating-point operation, and among the targets at the minimum squared distance the index is the smallest linear index.
SciPy's ndimage.distance_transform_edt(x) is sqrt(sq) of to="background" bit for bit; SciPy's return_indices follows no tie rule and is
not reproduced.  A radius r becomes the integer r_sq = the largest q with q <= r * r in float64 (_radius_sq), and a ball is sq <= r_sq.

csrc/edt.hip: a row pass on occupancy bits (clz / ctz), then Meijster's lower envelope along axis 1 and axis 0, one lane per column.
The NumPy forms upload the grid and download the result; the *_resident twins take and return device handles
(pb3d.device.DeviceGrid / DeviceBuffer) and the intermediate grids of close_grid / open_grid never leave the device."""
import ctypes as C
import math

import numpy as np

from . import _lib, device as dev
from ._args import _grid_channels, _on_device, _voxel_size
from ._lib import _ptr

__all__ = ["distance_transform", "distance_transform_resident", "dilate_grid", "dilate_grid_resident", "erode_grid", "erode_grid_resident",
           "close_grid", "close_grid_resident", "open_grid", "open_grid_resident", "grid_surface_metrics", "grid_surface_metrics_resident"]

MAX_AXIS = 16384            # PB3D_EDT_MAX_AXIS: 3 * 16383^2 < 2^31
MAX_VOXELS = 2 ** 31 - 1
MAX_THRESHOLDS = 8
NONE = 2 ** 31 - 1          # PB3D_EDT_NONE
TARGETS = ("background", "occupied", "surface")
FILL, KEEP = 0, 1


def _lattice(shape, what):
    """the lattice shape of a grid as the entries take it"""
    s = tuple(int(v) for v in shape)
    if min(s) < 1:
        raise ValueError(f"every axis of {what} must be >= 1 (got {s})")
    if max(s) > MAX_AXIS:
        raise ValueError(f"every axis of {what} must be <= {MAX_AXIS} (got {s})")
    if s[0] * s[1] * s[2] > MAX_VOXELS:
        raise ValueError(f"{what} holds at most 2^31 - 1 voxels (got {s})")
    return s


def _target(to):
    if not isinstance(to, str) or to not in TARGETS:
        raise ValueError(f"to must be 'background', 'occupied' or 'surface' (got {to!r})")
    return TARGETS.index(to)


def _radius_sq(radius, what="radius"):
    """the largest integer q with q <= radius * radius, the product rounded once in float64"""
    if isinstance(radius, (bool, np.bool_)) or not isinstance(radius, (int, float, np.integer, np.floating)):
        raise TypeError(f"{what} must be a real number (got {radius!r})")
    r = float(radius)
    if not math.isfinite(r) or r < 0.0:
        raise ValueError(f"{what} must be finite and >= 0 (got {radius!r})")
    return min(int(math.floor(r * r)), 2 ** 62)


def _out_dtype(dtype):
    dt = np.dtype(dtype)
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise TypeError(f"dtype must be float32 or float64 (got {dt})")
    return dt


def _thresholds_sq(thresholds, vs):
    try:
        ts = [t for t in thresholds]
    except TypeError:
        raise TypeError(f"thresholds must be a sequence of numbers (got {thresholds!r})") from None
    if len(ts) > MAX_THRESHOLDS:
        raise ValueError(f"at most {MAX_THRESHOLDS} thresholds (got {len(ts)})")
    out = []
    for t in ts:
        _radius_sq(t, "a threshold")
        out.append(_radius_sq(float(t) / vs, "a threshold"))
    return ts, out


def _edt(d_grid, ch, s, target, border, want_index, want_stats=False):
    """pb3d_edt_resident into fresh buffers: (d_sq, d_index or None[, stats])"""
    n = s[0] * s[1] * s[2]
    with dev.Scope() as sc:
        d_sq = sc.result(None, 4 * n)
        d_ix = sc.result(None, 4 * n) if want_index else None
        stats = (C.c_int64 * 2)() if want_stats else None
        _lib.check(_lib.load().pb3d_edt_resident(_lib.ctx(), _ptr(d_grid), ch, s[0], s[1], s[2], target, int(bool(border)), _ptr(d_sq), _ptr(d_ix),
                                                 stats))
        if want_stats:
            return d_sq, d_ix, {"targets": int(stats[0]), "max_sq": int(stats[1])}
        return d_sq, d_ix


def _check_transform(grid, to, border, return_distances, return_indices, voxel_size, dtype):
    ch, shape = _grid_channels(grid, "grid")
    s = _lattice(shape, "grid")
    target = _target(to)
    if not return_distances and not return_indices:
        raise ValueError("at least one of return_distances and return_indices must be set")
    if return_indices and border:
        raise ValueError("return_indices with border=True: a border plane has no index")
    return ch, s, target, _voxel_size(voxel_size), _out_dtype(dtype)


def distance_transform_resident(grid, to="background", border=False, return_distances=True, return_indices=False, squared=False, voxel_size=1.0,
                                dtype=np.float64, return_stats=False):
    """distance_transform of a DeviceGrid with the results left on the device: DeviceBuffers of n0 * n1 * n2 values -- distances
    (float64 / float32, or the int32 sq with squared=True), indices (int32), in that order, one or a tuple as asked for.  With
    return_stats also the dict of targets (their number) and max_sq (the largest sq, -1 when there is no target): one host wait."""
    if not isinstance(grid, dev.DeviceGrid):
        raise TypeError(f"grid must be a DeviceGrid (got {type(grid).__name__})")
    ch, s, target, vs, dt = _check_transform(grid, to, border, return_distances, return_indices, voxel_size, dtype)
    n = s[0] * s[1] * s[2]
    out = []
    with dev.Scope() as sc:
        res = _edt(grid.buf, ch, s, target, border, return_indices, return_stats)
        d_sq, d_ix = sc.adopt(res[:2])
        if return_distances and not squared:
            d_d = sc.alloc(n * dt.itemsize)
            _lib.check(_lib.load().pb3d_edt_distances_resident(_lib.ctx(), _ptr(d_sq), n, vs, int(dt.itemsize == 8), _ptr(d_d)))
            out.append(d_d)
        elif return_distances:
            out.append(d_sq)
        if return_indices:
            out.append(d_ix)
        for b in out:
            sc.keep(b)
    if return_stats:
        out.append(res[2])
    return out[0] if len(out) == 1 else tuple(out)


def distance_transform(grid, to="background", border=False, return_distances=True, return_indices=False, squared=False, voxel_size=1.0,
                       dtype=np.float64):
    """The exact Euclidean distance of every voxel of `grid` (a uint8 array or DeviceGrid, (n0, n1, n2) or (n0, n1, n2, 3); a voxel is
    occupied when any channel is non-zero) to the nearest target voxel: to="background" the empty voxels (SciPy's convention),
    "occupied" the occupied ones, "surface" the occupied ones with an empty or missing 6-neighbour.  border=True counts the six planes
    just outside the grid as targets (border_value=0 of SciPy's morphology).  Returns an (n0, n1, n2) array of sqrt(sq) * voxel_size in
    `dtype` (float64: one correctly rounded root and one product; float32: that rounded once more), +inf where there is no target; with
    squared=True the int32 sq itself (2^31 - 1 where there is no target).  return_indices adds the int32 linear index into the lattice
    of a nearest target -- among equidistant ones the smallest index -- and -1 where there is none; np.unravel_index(index, shape) gives
    coordinates.  With voxel_size 1 and float64 the distances are SciPy's ndimage.distance_transform_edt's bit for bit."""
    _check_transform(grid, to, border, return_distances, return_indices, voxel_size, dtype)
    ch, s = _grid_channels(grid, "grid")
    with dev.Scope() as sc:
        d_g = _on_device(sc, grid)
        res = sc.adopt(distance_transform_resident(dev.DeviceGrid(d_g, s + ((3,) if ch == 3 else ())), to, border, return_distances, return_indices,
                                                   squared, voxel_size, dtype))
        bufs = res if isinstance(res, tuple) else (res,)
        out = []
        if return_distances:
            out.append(bufs[0].download(s, np.int32 if squared else np.dtype(dtype)))
        if return_indices:
            out.append(bufs[-1].download(s, np.int32))
        return out[0] if len(out) == 1 else tuple(out)


def _apply(d_grid, ch, n, d_sq, d_ix, mode, r_sq, d_out):
    _lib.check(_lib.load().pb3d_edt_apply_resident(_lib.ctx(), _ptr(d_grid), ch, n, _ptr(d_sq), _ptr(d_ix), mode, r_sq, _ptr(d_out)))


def _morph(grid, steps, out=None):
    """steps: (FILL or KEEP, r_sq, border) in turn on a DeviceGrid; a new DeviceGrid (or `out`, which may be `grid`)"""
    if not isinstance(grid, dev.DeviceGrid):
        raise TypeError(f"grid must be a DeviceGrid (got {type(grid).__name__})")
    ch, shape = _grid_channels(grid, "grid")
    s = _lattice(shape, "grid")
    n = s[0] * s[1] * s[2]
    if out is not None and (not isinstance(out, dev.DeviceGrid) or out.shape != grid.shape):
        raise ValueError("out must be a DeviceGrid of the grid's shape")
    with dev.Scope() as sc:
        d_res = sc.result(None if out is None else out.buf, n * ch)
        src = grid.buf
        for mode, r_sq, border in steps:
            with dev.Scope() as step:
                d_sq, d_ix = step.adopt(_edt(src, ch, s, 1 if mode == FILL else 0, border, mode == FILL))
                _apply(src, ch, n, d_sq, d_ix, mode, r_sq, d_res)
            src = d_res                                     # the next step runs in place on the result
        return out if out is not None else dev.DeviceGrid(d_res, grid.shape)


def dilate_grid_resident(grid, radius, out=None):
    """dilate_grid of a DeviceGrid -> DeviceGrid (`out` may be `grid`: in place)"""
    return _morph(grid, [(FILL, _radius_sq(radius), False)], out)


def erode_grid_resident(grid, radius, border=True, out=None):
    """erode_grid of a DeviceGrid -> DeviceGrid (`out` may be `grid`: in place)"""
    return _morph(grid, [(KEEP, _radius_sq(radius), bool(border))], out)


def close_grid_resident(grid, radius, out=None):
    """close_grid of a DeviceGrid -> DeviceGrid; the dilated grid never leaves the device"""
    r = _radius_sq(radius)
    return _morph(grid, [(FILL, r, False), (KEEP, r, False)], out)


def open_grid_resident(grid, radius, out=None):
    """open_grid of a DeviceGrid -> DeviceGrid; the eroded grid never leaves the device"""
    r = _radius_sq(radius)
    return _morph(grid, [(KEEP, r, True), (FILL, r, False)], out)


def _host_form(resident, grid, *args):
    _lattice(_grid_channels(grid, "grid")[1], "grid")
    if isinstance(grid, dev.DeviceGrid):
        return resident(grid, *args)
    with dev.Scope() as sc:
        return sc.adopt(resident(dev.DeviceGrid(_on_device(sc, grid), np.shape(grid)), *args)).numpy()


def dilate_grid(grid, radius):
    """Dilation of an occupancy, label or RGB grid (uint8 array -> array, DeviceGrid -> DeviceGrid) by the Euclidean ball of `radius`
    voxels: an occupied voxel keeps its bytes, an empty voxel within the radius of an occupied one (sq <= r_sq, r_sq the largest
    integer <= radius * radius in float64) takes the bytes of the nearest occupied voxel, the smallest linear index among equidistant
    ones.  Its occupancy is SciPy's ndimage.binary_dilation by the ball."""
    _radius_sq(radius)
    return _host_form(dilate_grid_resident, grid, radius)


def erode_grid(grid, radius, border=True):
    """Erosion by the Euclidean ball of `radius` voxels: a voxel keeps its bytes when every voxel within the radius (sq <= r_sq) is
    occupied, otherwise it becomes zero.  border=True counts the outside of the grid as empty (SciPy's ndimage.binary_erosion's
    border_value=0), border=False as occupied."""
    _radius_sq(radius)
    return _host_form(erode_grid_resident, grid, radius, border)


def close_grid(grid, radius):
    """erode_grid(dilate_grid(grid, radius), radius, border=False): closes pinholes and gaps narrower than the ball; the filled voxels
    carry the colour or label of the nearest voxel."""
    _radius_sq(radius)
    return _host_form(close_grid_resident, grid, radius)


def open_grid(grid, radius):
    """dilate_grid(erode_grid(grid, radius, border=True), radius): removes what is thinner than the ball"""
    _radius_sq(radius)
    return _host_form(open_grid_resident, grid, radius)


def _directed(d_a, ch_a, d_b, ch_b, s, thr_sq):
    """surface of a against the surface of b: (surface voxels of a, max sq, sum sq, counts per threshold), surface voxels of b"""
    with dev.Scope() as sc:
        d_sq, _, st = _edt(d_b, ch_b, s, 2, False, False, True)
        sc.adopt(d_sq)
        out = (C.c_int64 * (3 + MAX_THRESHOLDS))()
        thr = (C.c_int64 * MAX_THRESHOLDS)(*thr_sq)
        _lib.check(_lib.load().pb3d_grid_surface_stats_resident(_lib.ctx(), _ptr(d_a), ch_a, s[0], s[1], s[2], _ptr(d_sq), thr, len(thr_sq), out))
    return [int(v) for v in out[:3 + len(thr_sq)]], st["targets"]


def _metrics_from_sums(ab, ba, thresholds, voxel_size):
    """the dict of grid_surface_metrics from the two directed integer results (surface voxels, max sq, sum sq, counts per threshold)"""
    vs = np.float64(voxel_size)
    na, nb = ab[0], ba[0]

    def directed(r, n_from, n_to):
        if n_from == 0:
            return 0.0, 0.0
        if n_to == 0:
            return math.inf, math.inf
        return float(np.sqrt(np.float64(r[1])) * vs), float(np.sqrt(np.float64(r[2]) / np.float64(n_from)) * vs)

    h_ab, rms_ab = directed(ab, na, nb)
    h_ba, rms_ba = directed(ba, nb, na)
    res = {"hausdorff": max(h_ab, h_ba), "hausdorff_ab": h_ab, "hausdorff_ba": h_ba, "rms_ab": rms_ab, "rms_ba": rms_ba,
           "surface_voxels_a": na, "surface_voxels_b": nb, "precision": [], "recall": [], "fscore": []}
    for k in range(len(thresholds)):
        if na == 0 or nb == 0:
            p = r = 0.0
        else:
            p = float(np.float64(ab[3 + k]) / np.float64(na))
            r = float(np.float64(ba[3 + k]) / np.float64(nb))
        res["precision"].append(p)
        res["recall"].append(r)
        res["fscore"].append(0.0 if (p + r) == 0 else 2 * p * r / (p + r))
    return res


def grid_surface_metrics_resident(a, b, thresholds=(1.0,), voxel_size=1.0):
    """grid_surface_metrics of two DeviceGrids (what it does for grids that are already resident)"""
    for g, what in ((a, "a"), (b, "b")):
        if not isinstance(g, dev.DeviceGrid):
            raise TypeError(f"{what} must be a DeviceGrid (got {type(g).__name__})")
    return grid_surface_metrics(a, b, thresholds, voxel_size)


def grid_surface_metrics(a, b, thresholds=(1.0,), voxel_size=1.0):
    """Surface distances of two grids of one lattice shape (uint8 arrays or DeviceGrids, (n0, n1, n2) or (n0, n1, n2, 3)).  The surface
    of a grid is its occupied voxels with an empty or missing 6-neighbour; every surface voxel of a is measured against the nearest
    surface voxel of b and the other way round (two "surface" transforms, two integer reductions on the device).  Returns a dict:
    hausdorff_ab, hausdorff_ba (the largest such distance) and hausdorff, their maximum; rms_ab, rms_ba (sqrt(sum sq / n)); per
    threshold t, in lists: precision (the share of a's surface voxels with sq <= floor((t / voxel_size)^2), the quotient rounded once
    in float64 and floored as a radius is), recall (the same from b) and fscore, formed as fscore_with_threshold forms them; and
    surface_voxels_a, surface_voxels_b.  Distances are sqrt(integer) * voxel_size in float64.  Where a surface is empty precision,
    recall and fscore are 0.0, the distances from the empty surface are 0.0 and those to it are inf (both empty: all 0.0).
    The mean (non-squared) surface distance is left out on purpose: a sum of square roots has no order-free exact form on the device;
    take it from distance_transform(b, to="surface") on the host if it is needed."""
    ca, sa = _grid_channels(a, "a")
    cb, sb = _grid_channels(b, "b")
    if sa != sb:
        raise ValueError(f"the grids differ in shape: {sa} and {sb}")
    s = _lattice(sa, "a")
    vs = _voxel_size(voxel_size)
    ts, thr_sq = _thresholds_sq(thresholds, vs)
    with dev.Scope() as sc:
        d_a, d_b = _on_device(sc, a), _on_device(sc, b)
        ab, nb = _directed(d_a, ca, d_b, cb, s, thr_sq)
        ba, na = _directed(d_b, cb, d_a, ca, s, thr_sq)
        assert ab[0] == na and ba[0] == nb, "the two surface counts of a grid differ"
        return _metrics_from_sums(ab, ba, ts, vs)
