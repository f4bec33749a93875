"""Thinning a point cloud to an even density on the device: the voxel-grid filter every point-cloud toolkit puts between segmentation and
registration.  A random pick (the reference's _downsample) keeps the density bias of its source; one point per occupied voxel does not,
and the nearest-neighbour metrics, estimate_normals and icp_align all weight dense regions more.

include/pb3d.h states the result to the bit: the grid starts at `origin`, or half a voxel below the cloud's minimum (then the voxel
membership is Open3D's voxel_down_sample); c = floor((p - origin) / voxel_size) in float64 per axis; points with equal cells share a voxel;
voxels are numbered in order of first appearance in the input; a voxel's centroid is the sum of its points in input order, each widened
to float64, divided once by their number (reduce="first" keeps the voxel's first point instead).  The result is a function of the input
and its order: permuting the input may renumber the voxels and change the last bits of the centroids, never the partition.

csrc/downsample.hip: a hash table of 63-bit cell keys finds the voxels, a scan of the first-appearance flags numbers them, and a stable
radix sort of (voxel, position) pairs puts every voxel's points in input order for the sums -- no floating-point atomics.  The NumPy
form uploads the cloud and downloads the arrays; the *_resident twin takes and returns device handles (pb3d.device.DeviceBuffer)."""
import ctypes as C

import numpy as np

from . import _lib, device as dev
from ._args import _count, _finite_cloud, _voxel_size
from ._lib import _ptr

__all__ = ["voxel_downsample", "voxel_downsample_resident"]

REDUCE = {"centroid": 0, "first": 1}


def _origin(origin):
    if origin is None:
        return None
    o = np.array(origin, dtype=np.float64).reshape(-1)
    if o.shape != (3,) or not np.isfinite(o).all():
        raise ValueError(f"origin must be three finite values (got {origin!r})")
    return o


def _reduce(reduce):
    if not isinstance(reduce, str) or reduce not in REDUCE:
        raise ValueError(f"reduce must be 'centroid' or 'first' (got {reduce!r})")
    return REDUCE[reduce]


def voxel_downsample_resident(d_P, n, voxel_size, origin=None, reduce="centroid", f64=True):
    """pb3d_voxel_downsample_resident: (d_out, d_index, d_inverse, d_counts, m) -- DeviceBuffers of n rows in the input's dtype (float64,
    or float32 with f64 False), n int32 first positions, n int32 voxel numbers and n uint32 counts; the first m entries of d_out, d_index
    and d_counts are written.  m is the call's one download.  The caller frees the four buffers.  ValueError when a point's cell leaves
    [0, 2^21) on an axis (voxel_size too small for the extent, or an origin above the cloud)."""
    n, voxel_size, o, r = _count(n), _voxel_size(voxel_size), _origin(origin), _reduce(reduce)
    m = C.c_int64(0)
    with dev.Scope() as sc:
        bufs = [sc.result(None, max(1, n) * w) for w in (24 if f64 else 12, 4, 4, 4)]
        _lib.check(_lib.load().pb3d_voxel_downsample_resident(_lib.ctx(), _ptr(d_P), int(bool(f64)), n, voxel_size,
                                                              None if o is None else _lib.p_dbl(o), r, _ptr(bufs[0]), _ptr(bufs[1]),
                                                              _ptr(bufs[2]), _ptr(bufs[3]), C.byref(m)))
        return bufs[0], bufs[1], bufs[2], bufs[3], int(m.value)


def voxel_downsample(points, voxel_size, origin=None, reduce="centroid", return_index=False, return_inverse=False, return_counts=False):
    """One point per occupied voxel of an (n, 3) cloud, voxels in order of first appearance: the centroid of the voxel's points, or with
    reduce="first" its first point.  float32 clouds stay float32 (sums and quotient in float64, rounded once), other real dtypes become
    float64.  Extras in np.unique's order: index (intp, the first position of each voxel), inverse (intp, the voxel of each point),
    counts (int64)."""
    voxel_size, o, _ = _voxel_size(voxel_size), _origin(origin), _reduce(reduce)
    p, pf = _finite_cloud(points)
    n = len(p)

    def pack(out, index, inverse, counts):
        extras = [a for a, want in ((index, return_index), (inverse, return_inverse), (counts, return_counts)) if want]
        return (out, *extras) if extras else out

    if n == 0:
        return pack(p.copy(), np.zeros(0, np.intp), np.zeros(0, np.intp), np.zeros(0, np.int64))
    with dev.Scope() as sc:
        *bufs, m = voxel_downsample_resident(sc.upload(p), n, voxel_size, o, reduce, pf)
        sc.adopt(bufs)
        out = bufs[0].download((m, 3), p.dtype)
        index = bufs[1].download((m,), np.int32).astype(np.intp) if return_index else None
        inverse = bufs[2].download((n,), np.int32).astype(np.intp) if return_inverse else None
        counts = bufs[3].download((m,), np.uint32).astype(np.int64) if return_counts else None
        return pack(out, index, inverse, counts)
