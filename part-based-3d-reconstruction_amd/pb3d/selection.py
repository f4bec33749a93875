"""Exact order statistics of a float64 list on the device (csrc/select.hip; include/pb3d.h has the contract): the element at a given
0-based rank in IEEE totalOrder, found by a radix selection over the ordered keys with integer counters only -- no sort, no host
round trip, and the same bytes on every call.  The trimmed ICP step (pb3d.preprocess_helpers) is its first user."""
import numpy as np

from . import _lib, device as dev
from ._lib import _ptr

__all__ = ["kth_smallest", "kth_smallest_resident"]


def kth_smallest_resident(d_vals, n, rank, out=None):
    """pb3d_kth_smallest_resident: a DeviceBuffer of 8 bytes holding the element at 0-based position `rank` of the n resident float64
    values d_vals, sorted by totalOrder (negatives < -0.0 < +0.0 < positives < +inf < NaN).  Enqueued: nothing waits for the host."""
    n, rank = int(n), int(rank)
    if n < 1 or not 0 <= rank < n:          # before any allocation; the entry states the same refusals
        raise ValueError(f"kth_smallest: need n >= 1 and 0 <= rank < n (got rank {rank} of {n})")
    with dev.Scope() as sc:
        d_out = sc.result(out, 8)
        _lib.check(_lib.load().pb3d_kth_smallest_resident(_lib.ctx(), _ptr(d_vals), n, rank, _ptr(d_out)))
        return d_out


def kth_smallest(values, rank):
    """The element at 0-based position `rank` of `values` (any real array, flattened, taken as float64) in totalOrder, as a NumPy
    float64 scalar with the exact bytes of that element"""
    v = np.asarray(values)
    if v.dtype.kind not in "fiub":
        raise TypeError(f"kth_smallest: unsupported dtype {v.dtype}")
    v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
    if isinstance(rank, (bool, np.bool_)) or not isinstance(rank, (int, np.integer)):
        raise ValueError(f"kth_smallest: rank must be an integer (got {rank!r})")
    if len(v) == 0 or not 0 <= rank < len(v):
        raise ValueError(f"kth_smallest: need at least one value and 0 <= rank < {len(v)} (got rank {rank})")
    with dev.Scope() as sc:
        d_out = sc.adopt(kth_smallest_resident(sc.upload(v), len(v), rank))
        return d_out.download((1,), np.float64)[0]
