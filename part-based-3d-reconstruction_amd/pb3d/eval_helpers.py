"""Inter-method point-cloud metrics (row I5): reference utils/eval_helpers.py.

Every metric of the file compares two clouds through one primitive, the distance from each point of A to its nearest (or, for
compute_nn_stats, second-nearest) point of B.  Upstream takes it from cKDTree / NearestNeighbors on clouds downsampled to 20 k or 50 k
points; here it is pb3d_nn_dist_dev (csrc/nn.hip): an exact search over a uniform cell index on the device, bit for bit the value
those trees return (sqrt((dx*dx + dy*dy) + dz*dz) in float64, float32 widened first), so full-resolution clouds are affordable too.

The downsampling draws np.random.choice / np.random.default_rng(seed).choice exactly as the reference does, in the same order, so a
seeded notebook gets the same subsets and leaves the global RNG in the same state.  Distances come back to the host, and the means,
thresholds and F1 run there with the reference's own NumPy expressions.  voxel_iou's occupancy, dilation and counts run on the device
(pb3d_voxel_iou_counts_dev) after the host has computed bounds_min, step and iters with the reference's expressions from the exact
device bounding box.  pca_shape_similarity and filter_mesh are host NumPy.

Not mirrored: get_marching_cubes_mesh and pointcloud_to_voxel_grid (marching cubes and the missing
utils.preprocess_helpers upstream) and compute_surface_metrics."""
import ctypes as C

import numpy as np

from . import _lib

__all__ = ["filter_mesh", "chamfer_distance", "fscore_with_threshold", "pca_shape_similarity", "voxel_iou", "compute_nn_stats",
           "compute_nn_distances", "f1_curve_from_distances", "compute_f1_curve", "nn_distances", "nn_distances_resident",
           "points_bounds_resident", "voxel_iou_counts_resident", "voxel_iou_counts"]


# ---- geometry helpers (:18-22) ---------------------------------------------------------------------------------------------------------
def filter_mesh(vertices, faces, y_thresh=0.2):
    mask = vertices[:, 1] <= y_thresh
    valid_idx = np.where(mask)[0]
    face_mask = np.all(np.isin(faces, valid_idx), axis=1)
    return vertices[mask], faces[face_mask]


# ---- point lists on the device -----------------------------------------------------------------------------------------------------------
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


def _ptr(b):
    return None if b is None else C.c_void_p(b.ptr)


def nn_distances_resident(d_A, nA, d_B, nB, k=1, a_f64=True, b_f64=True, out=None):
    """pb3d_nn_dist_dev: a DeviceBuffer of nA float64 -- the k-th smallest distance (k = 1 or 2) from each point of the resident
    (nA, 3) list d_A to the resident (nB, 3) list d_B (float64 rows, or float32 with a_f64 / b_f64 False).  With k = 2 and d_A the
    same list as d_B a point's own copy counts (distance 0), as NearestNeighbors(2).kneighbors(X) of X itself does."""
    from . import device as dev
    d_out = out if out is not None else dev.DeviceBuffer(max(1, int(nA)) * 8)
    _lib.check(_lib.load().pb3d_nn_dist_dev(_lib.ctx(), _ptr(d_A), int(bool(a_f64)), int(nA), _ptr(d_B), int(bool(b_f64)), int(nB), int(k),
                                            _ptr(d_out)))
    return d_out


def points_bounds_resident(d_P, n, f64=True, out=None):
    """pb3d_points_bounds_dev: a DeviceBuffer of 6 float64, the exact min (3) and max (3) of a resident (n, 3) list"""
    from . import device as dev
    d_out = out if out is not None else dev.DeviceBuffer(6 * 8)
    _lib.check(_lib.load().pb3d_points_bounds_dev(_lib.ctx(), _ptr(d_P), int(bool(f64)), int(n), _ptr(d_out)))
    return d_out


def voxel_iou_counts_resident(d_A, nA, d_B, nB, bounds_min, step, resolution, iters, a_f64=True, b_f64=True, calc_f32=False, out=None):
    """pb3d_voxel_iou_counts_dev: a DeviceBuffer of 2 int64, (#(occA & occB), #(occA | occB)) of voxel_iou's dilated occupancies"""
    from . import device as dev
    d_out = out if out is not None else dev.DeviceBuffer(2 * 8)
    lo = np.ascontiguousarray(np.asarray(bounds_min, dtype=np.float64).reshape(3))
    _lib.check(_lib.load().pb3d_voxel_iou_counts_dev(_lib.ctx(), _ptr(d_A), int(bool(a_f64)), int(nA), _ptr(d_B), int(bool(b_f64)), int(nB),
                                                     _lib.p_dbl(lo), float(step), int(bool(calc_f32)), int(resolution), int(iters),
                                                     _ptr(d_out)))
    return d_out


def nn_distances(A, B, k=1):
    """float64 (len(A),) array: the k-th nearest distance (k = 1 or 2) from each point of A to B, bit for bit
    cKDTree(B).query(A, k)[0] (its last column when k = 2)."""
    from . import device as dev
    a, af = _cloud(A, "A")
    b, bf = _cloud(B, "B")
    if len(a) == 0:
        return np.zeros(0, np.float64)
    d_a = dev.from_numpy(a)
    d_b = d_a if B is A else dev.from_numpy(b)
    try:
        d_out = nn_distances_resident(d_a, len(a), d_b, len(b), k, af, bf)
        try:
            return d_out.download((len(a),), np.float64)
        finally:
            d_out.free()
    finally:
        d_a.free()
        if d_b is not d_a:
            d_b.free()


# ---- accuracy metrics (:29-70) ---------------------------------------------------------------------------------------------------------
def _downsample(P, n=20000):
    if len(P) <= n:
        return P
    idx = np.random.choice(len(P), n, replace=False)
    return P[idx]


def chamfer_distance(A, B, max_points=20000, squared=True):
    A = _downsample(A, max_points)
    B = _downsample(B, max_points)

    dA = nn_distances(A, B)
    dB = nn_distances(B, A)

    if squared:
        return float(np.mean(dA**2) + np.mean(dB**2))
    else:
        return float(np.mean(dA) + np.mean(dB))


def fscore_with_threshold(A, B, tau=0.03, max_points=20000):
    A = _downsample(A, max_points)
    B = _downsample(B, max_points)

    d_AB = nn_distances(A, B)
    precision = float(np.mean(d_AB < tau))

    d_BA = nn_distances(B, A)
    recall = float(np.mean(d_BA < tau))

    f1 = 0.0 if (precision + recall) == 0 else (
        2 * precision * recall / (precision + recall)
    )
    return f1, precision, recall


def _explained_variance_ratio(X):
    """PCA(n_components=3).fit(X).explained_variance_ratio_ of (n, 3) data: the eigenvalues of the centred covariance, largest first,
    over their sum.  scikit-learn picks its covariance-eigh solver for tall 3-column data; this centred form agrees with it to ~1e-15."""
    X = np.asarray(X, dtype=np.float64)
    Xc = X - X.mean(axis=0)
    ev = np.linalg.eigvalsh(Xc.T @ Xc / (len(X) - 1))[::-1]
    ev = np.maximum(ev, 0.0)
    return ev / ev.sum()


def pca_shape_similarity(A, B):
    return 1.0 - np.sum(
        np.abs(_explained_variance_ratio(A) -
               _explained_variance_ratio(B))
    )


# ---- completeness metrics (:77-111) ----------------------------------------------------------------------------------------------------
def _iou_inputs(A, B):
    """(A, B) as the kernels read them, their flags, and the dtype of the reference's np.vstack([A, B])"""
    A = np.asarray(A)
    B = np.asarray(B)
    dt = np.result_type(A.dtype, B.dtype)
    if dt == np.float32:            # float32 arithmetic (NEP 50); every dtype that promotes to float32 converts to it exactly
        conv = np.float32
    elif dt == np.float64 or dt.kind in "iu":
        conv = np.float64           # integers: exact for |v| < 2^53
    else:
        raise TypeError(f"voxel_iou: unsupported dtype {dt}")
    out = []
    for P, what in ((A, "A"), (B, "B")):
        if P.ndim != 2 or P.shape[1] != 3:
            raise ValueError(f"voxel_iou: {what} must be an (n, 3) array (got shape {P.shape})")
        out.append(np.ascontiguousarray(P, dtype=conv))
    return out[0], out[1], int(conv is np.float64), dt


def voxel_iou_counts(A, B, resolution=96, dilate_frac=0.01):
    """(inter, union) of voxel_iou: the occupancy of both clouds in resolution^3 voxels of their joint box, each dilated `iters`
    times; bounds, step and iters are the reference's expressions (:84-102) on the exact device bounds."""
    from . import device as dev
    a, b, f64, dt = _iou_inputs(A, B)
    if len(a) + len(b) == 0:
        np.vstack([np.asarray(A), np.asarray(B)]).min(0)        # the reference's error on two empty clouds
    bufs = []
    try:
        d_pts, bb = [], []
        for P in (a, b):
            d_p = dev.from_numpy(P) if len(P) else None
            d_pts.append(d_p)
            if d_p is not None:
                bufs.append(d_p)
                d_bb = points_bounds_resident(d_p, len(P), f64)
                bufs.append(d_bb)
                bb.append(d_bb.download((6,), np.float64))
        bb = np.array(bb)
        bounds_min = bb[:, :3].min(0).astype(dt)
        bounds_max = bb[:, 3:].max(0).astype(dt)
        step = (bounds_max - bounds_min).max() / resolution
        iters = 0
        if dilate_frac > 0:
            iters = max(1, int(round(
                (dilate_frac * np.linalg.norm(bounds_max - bounds_min)) / step
            )))
        d_c = voxel_iou_counts_resident(d_pts[0], len(a), d_pts[1], len(b), bounds_min, step, resolution, iters, f64, f64,
                                        calc_f32=not f64)
        bufs.append(d_c)
        inter, union = (int(v) for v in d_c.download((2,), np.int64))
        return inter, union
    finally:
        for buf in bufs:
            buf.free()


def voxel_iou(A, B, resolution=96, dilate_frac=0.01):
    inter, union = voxel_iou_counts(A, B, resolution, dilate_frac)
    return inter / union if union > 0 else np.nan


# ---- regularity metrics (:118-130) -----------------------------------------------------------------------------------------------------
def compute_nn_stats(pts, max_points=50000):
    if len(pts) > max_points:
        pts = pts[np.random.choice(len(pts), max_points, replace=False)]

    nn = nn_distances(pts, pts, k=2)        # distances[:, 1] of NearestNeighbors(n_neighbors=2) on the set itself
    return {
        "NN Mean ↓": nn.mean(),
        "NN Std ↓": nn.std(),
        "NN CV ↓": nn.std() / (nn.mean() + 1e-8)
    }


# ---- F1 curve (:214-263) ---------------------------------------------------------------------------------------------------------------
def compute_nn_distances(A, B, max_points=50000, seed=0):
    """
    Downsample + compute nearest-neighbor distances A->B and B->A.
    Returns (d_AB, d_BA).
    """
    rng = np.random.default_rng(seed)

    if len(A) > max_points:
        A = A[rng.choice(len(A), max_points, replace=False)]
    if len(B) > max_points:
        B = B[rng.choice(len(B), max_points, replace=False)]

    return nn_distances(A, B), nn_distances(B, A)


def f1_curve_from_distances(d_AB, d_BA, thresholds):
    """
    Compute precision, recall, and F1 for a sweep of thresholds.
    """
    precs, recs, f1s = [], [], []

    for t in thresholds:
        prec = float(np.mean(d_AB < t))
        rec  = float(np.mean(d_BA < t))
        f1   = 0.0 if (prec + rec) == 0 else (2 * prec * rec) / (prec + rec)

        precs.append(prec)
        recs.append(rec)
        f1s.append(f1)

    return (
        np.asarray(recs),
        np.asarray(precs),
        np.asarray(f1s),
    )


def compute_f1_curve(A, B, thresholds, max_points=50000, seed=0):
    """
    End-to-end F1(τ) curve between two point clouds.
    """
    d_AB, d_BA = compute_nn_distances(
        A, B, max_points=max_points, seed=seed
    )
    return f1_curve_from_distances(d_AB, d_BA, thresholds)
