"""Segmenting a point cloud on the device: exact DBSCAN (cluster_points), the fixed-radius neighbour counts it starts from, and the
order-keeping selection that turns labels into a smaller cloud.  This is the step the inter-method preprocessing begins with: an SfM
cloud holds the monument, the ground around it and stray points, and every later step (crop_to_box, icp_align, the metrics) assumes
the monument alone.

include/pb3d.h states the result to the bit, and it is scikit-learn's: q is a neighbour of p iff (dx*dx + dy*dy) + dz*dz <= eps*eps in
float64 (a point is its own neighbour); counts[p] is the number of neighbours; core[p] = counts[p] >= min_samples; clusters are the
connected components of the neighbour graph on core points, numbered by their smallest core index; a non-core point takes the smallest
label among its core neighbours, or -1 (noise).  labels equal sklearn.cluster.DBSCAN(eps, min_samples).fit(points).labels_ and
np.flatnonzero(core) equals its core_sample_indices_, for every algorithm= of scikit-learn's and every order of the input.

csrc/cluster.hip: the cloud is binned against itself in the cell index of the exact searches (csrc/nn.hip), one walk per point counts,
a second unites core neighbours in a lock-free union-find whose roots are component minima by construction, a scan ranks the roots
and a third, short walk labels the border points.  The NumPy-signature functions upload the cloud and download the arrays; the
*_resident twins take and return device handles (pb3d.device.DeviceBuffer) and leave the cloud where it is."""
import ctypes as C
import math

import numpy as np

from . import _lib, device as dev
from ._args import MAX_POINTS, _count, _finite_cloud, _sized_cloud  # noqa: F401
from ._lib import _ptr

__all__ = ["radius_neighbor_counts", "radius_neighbor_counts_resident", "cluster_points", "cluster_points_resident", "select_points",
           "select_points_resident", "keep_largest_clusters", "keep_largest_clusters_resident"]

def _eps(eps):
    e = float(eps)
    if not (math.isfinite(e) and e > 0.0):
        raise ValueError(f"eps must be finite and > 0 (got {eps!r})")
    return e


def _at_least_one(v, name):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < 1:
        raise ValueError(f"{name} must be an integer >= 1 (got {v!r})")
    return int(v)


# ---- resident forms ----------------------------------------------------------------------------------------------------------------------
def radius_neighbor_counts_resident(d_P, n, eps, f64=True, out=None):
    """pb3d_radius_count_resident: a DeviceBuffer of n uint32 -- for every point of the resident (n, 3) list (float64 rows, or float32
    with f64 False; finite) the number of points within eps of it, itself included"""
    n, eps = _count(n), _eps(eps)
    with dev.Scope() as sc:
        d_out = sc.result(out, max(1, n) * 4)
        _lib.check(_lib.load().pb3d_radius_count_resident(_lib.ctx(), _ptr(d_P), int(bool(f64)), n, eps, _ptr(d_out)))
        return d_out


def cluster_points_resident(d_P, n, eps, min_samples, f64=True):
    """pb3d_cluster_points_resident: (d_labels, d_core, d_counts, d_sizes, nclusters) -- DeviceBuffers of n int32 labels (-1 = noise),
    n core bytes (0 / 1), n uint32 neighbour counts and int64 cluster sizes (the first nclusters of n entries are written).  The
    number of clusters is the call's one download.  The caller frees the four buffers."""
    n, eps, min_samples = _count(n), _eps(eps), _at_least_one(min_samples, "min_samples")
    nc = C.c_int64(0)
    with dev.Scope() as sc:
        bufs = [sc.result(None, max(1, n) * w) for w in (4, 1, 4, 8)]
        _lib.check(_lib.load().pb3d_cluster_points_resident(_lib.ctx(), _ptr(d_P), int(bool(f64)), n, eps, min_samples, _ptr(bufs[0]),
                                                            _ptr(bufs[1]), _ptr(bufs[2]), _ptr(bufs[3]), C.byref(nc)))
        return bufs[0], bufs[1], bufs[2], bufs[3], int(nc.value)


def select_points_resident(d_P, n, d_keep, f64=True, out=None, index=None):
    """pb3d_points_select_resident: (d_out, d_idx, count) -- the rows of the resident (n, 3) list whose byte in d_keep (n bytes on the
    device) is not 0, in their order and dtype, at the front of d_out (n rows), and their positions in the input at the front of d_idx
    (n int32).  Both are allocated unless given.  The count is downloaded (the one host wait)."""
    n = _count(n)
    row = 24 if f64 else 12
    with dev.Scope() as sc:
        d_out = sc.result(out, max(1, n) * row)
        d_idx = sc.result(index, max(1, n) * 4)
        d_count = sc.alloc(8)
        _lib.check(_lib.load().pb3d_points_select_resident(_lib.ctx(), _ptr(d_P), int(bool(f64)), n, _ptr(d_keep), _ptr(d_out), _ptr(d_idx),
                                                           _ptr(d_count)))
        return d_out, d_idx, int(d_count.download((1,), np.int64)[0])


def _largest(sizes, k):
    """the labels of the k largest clusters: by size, ties to the lower label; all of them when k exceeds their number"""
    sizes = np.asarray(sizes, np.int64)
    order = np.lexsort((np.arange(len(sizes)), -sizes))
    return np.sort(order[:k])


def keep_largest_clusters_resident(d_P, n, eps, min_samples, k=1, f64=True):
    """cluster_points_resident, the k largest sizes picked on the host (ties to the lower label), and select_points_resident on the
    device's flags `label is one of them`: (d_out, d_idx, count, chosen labels).  Only the sizes and two counts leave the device."""
    k = _at_least_one(k, "k")
    n = _count(n)
    with dev.Scope() as sc:
        *bufs, nc = cluster_points_resident(d_P, n, eps, min_samples, f64)
        d_lab, _, _, d_sizes = sc.adopt(bufs)
        sizes = d_sizes.download((nc,), np.int64) if nc else np.zeros(0, np.int64)
        chosen = _largest(sizes, k)
        table = np.zeros(max(1, nc), np.uint8)
        table[chosen] = 1
        d_keep = sc.alloc(max(1, n))
        _lib.check(_lib.load().pb3d_labels_member_resident(_lib.ctx(), _ptr(d_lab), n, _lib.p_u8(table), nc, _ptr(d_keep)))
        d_out, d_idx, count = select_points_resident(d_P, n, d_keep, f64)
        return d_out, d_idx, count, chosen


# ---- NumPy forms ------------------------------------------------------------------------------------------------------------------------
def radius_neighbor_counts(points, eps):
    """int64 (n,): the number of points within eps of each point, itself included (d2 <= eps*eps as in the module text).  Radius outlier
    removal is points[radius_neighbor_counts(points, eps) >= m]."""
    eps = _eps(eps)
    p, pf = _finite_cloud(points)
    n = len(p)
    if n == 0:
        return np.zeros(0, np.int64)
    with dev.Scope() as sc:
        d_out = sc.adopt(radius_neighbor_counts_resident(sc.upload(p), n, eps, pf))
        return d_out.download((n,), np.uint32).astype(np.int64)


def cluster_points(points, eps, min_samples):
    """(labels int64 (n,), core bool (n,), counts int64 (n,), sizes int64 (clusters,)): DBSCAN of an (n, 3) cloud, float32 (widened) or
    any other real dtype (as float64).  labels == sklearn.cluster.DBSCAN(eps=eps, min_samples=min_samples).fit(points).labels_."""
    eps, min_samples = _eps(eps), _at_least_one(min_samples, "min_samples")
    p, pf = _finite_cloud(points)
    n = len(p)
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, bool), np.zeros(0, np.int64), np.zeros(0, np.int64)
    with dev.Scope() as sc:
        *bufs, nc = cluster_points_resident(sc.upload(p), n, eps, min_samples, pf)
        sc.adopt(bufs)
        labels = bufs[0].download((n,), np.int32).astype(np.int64)
        core = bufs[1].download((n,), np.uint8) != 0
        counts = bufs[2].download((n,), np.uint32).astype(np.int64)
        sizes = bufs[3].download((nc,), np.int64).copy() if nc else np.zeros(0, np.int64)
        return labels, core, counts, sizes


def _keep_flags(keep, n):
    k = np.asarray(keep)
    if k.shape != (n,) or k.dtype.kind not in "biu":
        raise ValueError(f"keep must be a boolean or integer array of shape ({n},) (got shape {k.shape}, dtype {k.dtype})")
    return _lib.truth_u8(k)


def select_points(points, keep):
    """(points[keep != 0], np.flatnonzero(keep)) compacted on the device, in input order; float32 clouds stay float32, other real
    dtypes become float64.  keep: one boolean or integer per point."""
    p, pf = _sized_cloud(points)
    n = len(p)
    flags = _keep_flags(keep, n)
    if n == 0:
        return p.copy(), np.zeros(0, np.intp)
    with dev.Scope() as sc:
        d_out, d_idx, count = select_points_resident(sc.upload(p), n, sc.upload(flags), pf)
        sc.adopt((d_out, d_idx))
        return _download_selection(d_out, d_idx, count, p.dtype)


def _download_selection(d_out, d_idx, count, dtype):
    out = d_out.download((count, 3), dtype) if count else np.zeros((0, 3), dtype)
    idx = d_idx.download((count,), np.int32) if count else np.zeros(0, np.int32)
    return out, idx.astype(np.intp)


def keep_largest_clusters(points, eps, min_samples, k=1, return_index=False):
    """The points of the k largest DBSCAN clusters (core and border points; ties in size go to the lower label; all clusters when k
    exceeds their number), in input order.  return_index=True: (kept, their positions in the input)."""
    eps, min_samples, k = _eps(eps), _at_least_one(min_samples, "min_samples"), _at_least_one(k, "k")
    p, pf = _finite_cloud(points)
    n = len(p)
    if n == 0:
        return (p.copy(), np.zeros(0, np.intp)) if return_index else p.copy()
    with dev.Scope() as sc:
        d_out, d_idx, count, _ = keep_largest_clusters_resident(sc.upload(p), n, eps, min_samples, k, pf)
        sc.adopt((d_out, d_idx))
        out, idx = _download_selection(d_out, d_idx, count, p.dtype)
        return (out, idx) if return_index else out
