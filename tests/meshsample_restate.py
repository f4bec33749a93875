"""NumPy statement of the stratified area-weighted mesh sampler (csrc/meshdist.hip, pb3d_mesh_sample_resident; include/pb3d.h has the
semantics), independent of the device code and written from the header."""
import numpy as np

BLOCK = 1024
M64 = (1 << 64) - 1


def mix(x):
    """SplitMix64's output function on Python integers, uint64 wrap-around"""
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def mix_array(x):
    """mix on a uint64 array"""
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def unit_randoms(seed, n):
    """(n, 3) float64: r_j(i) = (mix(mix(seed) + 3 i + j) >> 11) * 2^-53"""
    key = np.uint64(mix(int(seed)))
    with np.errstate(over="ignore"):
        idx = key + np.uint64(3) * np.arange(n, dtype=np.uint64)[:, None] + np.arange(3, dtype=np.uint64)[None, :]
    return (mix_array(idx) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def corners(vertices, faces):
    v = np.asarray(vertices).astype(np.float64)
    f = np.asarray(faces).astype(np.int64)
    return v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]


def face_areas(vertices, faces):
    a, b, c = corners(vertices, faces)
    ab, ac = b - a, c - a
    n0 = ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1]
    n1 = ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2]
    n2 = ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]
    return 0.5 * np.sqrt((n0 * n0 + n1 * n1) + n2 * n2)


def cumulative_areas(areas):
    """cum[f] = O_b + local[f]: running sums inside blocks of 1024 faces (np.cumsum of float64 adds left to right), a running sum of
    the block totals with O_0 = 0"""
    cum = np.empty(len(areas), np.float64)
    offset = 0.0
    for s in range(0, len(areas), BLOCK):
        local = np.cumsum(areas[s:s + BLOCK])
        cum[s:s + BLOCK] = offset + local
        offset = offset + local[-1]
    return cum


def sample(vertices, faces, n, seed=0):
    """(points (n, 3) float64, faces (n,) int32, barycentric weights (n, 3))"""
    a, b, c = corners(vertices, faces)
    cum = cumulative_areas(face_areas(vertices, faces))
    total = cum[-1]
    assert np.isfinite(total) and total > 0
    r = unit_randoms(seed, n)
    u = (np.arange(n, dtype=np.float64) + r[:, 0]) / np.float64(n) * total
    f = np.minimum(np.searchsorted(cum, u, "right"), len(cum) - 1)
    s = np.sqrt(r[:, 1])
    wa, wb, wc = 1.0 - s, s * (1.0 - r[:, 2]), s * r[:, 2]
    pts = (a[f] * wa[:, None] + b[f] * wb[:, None]) + c[f] * wc[:, None]
    return pts, f.astype(np.int32), np.stack([wa, wb, wc], 1)
