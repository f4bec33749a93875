"""NumPy restatement of pointcloud_to_voxel_grid (reference utils/eval_helpers.py:178-189) for tests/test_density_grid.py and
tools/gen_golden_density.py, and the clouds both use.

The Gaussian filter is restated operation by operation: per axis (0, 1, 2), float32 in and out, and per output element in float64
    tmp = in[l] * w[r];  for jj = -r .. -1:  tmp += (in[l + jj] + in[l - jj]) * w[r + jj]
with out-of-range indices reflected about the edges (d c b a | a b c d | d c b a, period 2n).  NumPy's element-wise multiply and add
are separate roundings, which is what the compiled filter does.  tests/test_density_grid.py checks the restatement against
scipy.ndimage.gaussian_filter bit for bit.  The counts use np.bincount, capped at 2^24 where a float32 cell of np.add.at stops."""
import numpy as np

FLOAT_CAP = 1 << 24


def normalize_preserve_aspect(points):
    """the stated arithmetic, written independently of pb3d.preprocess_helpers"""
    pts = np.asarray(points)
    lo = pts.min(axis=0)
    scale = (pts.max(axis=0) - lo).max()
    norm = (pts - lo) / (scale + 1e-8)
    norm[:, 1] = norm[:, 1] - norm[:, 1].max()
    return norm


def gaussian_weights(sigma):
    """(radius, 2 * radius + 1 float64 weights)"""
    sd = float(sigma)
    radius = int(4.0 * sd + 0.5)
    x = np.arange(-radius, radius + 1)
    w = np.exp(-0.5 / (sd * sd) * x ** 2)
    return radius, w / w.sum()


def reflect_index(i, n):
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def filter_axis(vol, axis, w, r):
    a = np.moveaxis(np.asarray(vol, dtype=np.float32), axis, 0).astype(np.float64)
    n = a.shape[0]
    l = np.arange(n)
    tmp = a * w[r]
    for jj in range(-r, 0):
        tmp = tmp + (a[reflect_index(l + jj, n)] + a[reflect_index(l - jj, n)]) * w[r + jj]
    return np.ascontiguousarray(np.moveaxis(tmp.astype(np.float32), 0, axis))


def gaussian_filter_restate(vol, sigma):
    r, w = gaussian_weights(sigma)
    out = np.asarray(vol, dtype=np.float32)
    for axis in range(out.ndim):
        out = filter_axis(out, axis, w, r)
    return out


def voxel_indices(norm, G):
    """(n, 3) int64 indices in [0, G) after NumPy's wrap of negative ones"""
    idx = (norm * (G - 1)).astype(int)
    assert (idx >= -G).all() and (idx < G).all()
    return np.where(idx < 0, idx + G, idx)


def count_volume(norm, G):
    idx = voxel_indices(norm, G)
    flat = (idx[:, 0] * G + idx[:, 1]) * G + idx[:, 2]
    counts = np.bincount(flat, minlength=G ** 3)
    return np.minimum(counts, FLOAT_CAP).astype(np.float32).reshape(G, G, G)


def zero_faces(vol):
    vol[[0, -1], :, :] = 0
    vol[:, [0, -1], :] = 0
    vol[:, :, [0, -1]] = 0
    return vol


def finish(counts, sigma):
    """filter (sigma > 0) and zero faces of a float32 count volume; the count volume is left unchanged"""
    vol = gaussian_filter_restate(counts, sigma) if sigma > 0 else counts.copy()
    return zero_faces(vol)


def voxel_grid_restate(points, G, sigma, normalize=normalize_preserve_aspect):
    return finish(count_volume(normalize(points), G), sigma)


# ---- clouds ---------------------------------------------------------------------------------------------------------------------------
KINDS = ("cubic", "flat_y", "tall_y")


def make_cloud(kind, n, dtype, seed):
    """(n, 3) cloud off the origin.  cubic: equal extents; flat_y: the y extent is 2 % of the largest, so every y index is 0;
    tall_y: y is the largest extent, so the y indices run over -(G - 1) .. 0 and wrap to every plane."""
    rng = np.random.default_rng([seed, n, KINDS.index(kind)])
    ext = {"cubic": (1.0, 1.0, 1.0), "flat_y": (1.0, 0.02, 0.7), "tall_y": (0.3, 1.0, 0.45)}[kind]
    p = rng.random((n, 3)) * np.array(ext) * 37.5 + np.array([-3.25, 11.0, 0.125])
    return np.ascontiguousarray(p.astype(dtype))


def one_voxel_cloud(n, dtype):
    """n points inside one interior voxel of a unit box, plus the box's two corners"""
    rng = np.random.default_rng(n)
    p = np.array([0.40, 0.45, 0.62]) + rng.random((n, 3)) * 1e-3
    return np.ascontiguousarray(np.concatenate([p, [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]]).astype(dtype))
