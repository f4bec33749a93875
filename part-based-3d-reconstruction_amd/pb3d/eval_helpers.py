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

The mesh regularity block (:198-245) runs on the device too (csrc/surface.hip): compute_triangle_normals and compute_vertex_normals
bit for bit NumPy's, in the vertex dtype; compute_surface_metrics on the exact k nearest neighbours of pb3d_knn_dev (csrc/nn.hip, rows
ordered by (squared distance, index): sklearn breaks ties by traversal order, so the two agree wherever every vertex's k-th and
(k+1)-th distances differ) with the per-vertex spread of normal angles, smallest PCA eigenvalue and mean offset in float64; the last
np.mean of each is the reference's own, on the downloaded per-vertex arrays.

pointcloud_to_voxel_grid (:178-189) runs on the device as well (csrc/density.hip, pb3d_density_grid_resident): the normalisation of
pb3d.preprocess_helpers in the point dtype from the exact device bounds, integer counts by atomics (exact in any order; a float32
cell of np.add.at stops at 2^24, so the value is min(count, 2^24)), then the reference's Gaussian filter restated pass by pass -- its
float64 summation order per output, float32 between the passes, reflect boundary, no FMA -- and the zero faces.  The volume is bit
for bit the reference's at any point count, so full-resolution clouds and finer grids need no downsampling.

point_to_mesh_distances, sample_mesh_points and cloud_to_mesh_metrics have no upstream text (the reference's README names the step,
"load and align a CAD reference model", and ships no code for it): a mesh as the other side of the comparison.  csrc/meshdist.hip finds
the exact nearest point of the surface for every point of a cloud on the cell index of the NN search, with triangles in the cells, and
draws stratified area-weighted samples that turn a mesh into a cloud for every metric above and for icp_align; include/pb3d.h states
both to the bit.

get_marching_cubes_mesh (:191-195) runs on the device too: the resident density volume, then the isosurface of csrc/mesh.hip
(pb3d_iso_*), whose rule -- inside iff float64(v) > level, meshify's binary case table, ownership and order, edge vertices
interpolated in float64, the centre vertex at the cube centre -- is the project's own and is stated to the bit in include/pb3d.h.
There is no scikit-image here to compare float-level meshes with, and none is claimed equal: skimage's Lewiner variant decides
ambiguous faces and interiors from the values, so vertex and face counts can differ on ambiguous cubes.  On a 0/1 volume at level
0.5 the rule gives meshify_colored_voxel_grid's lattice mesh, which is skimage's, byte for byte."""
import ctypes as C
import operator

import numpy as np

from . import _hostmem, _lib, device as dev
from ._args import _cloud  # noqa: F401  (the cloud check; tests and tools take it from here)
from ._lib import _ptr

__all__ = ["filter_mesh", "chamfer_distance", "fscore_with_threshold", "pca_shape_similarity", "voxel_iou", "compute_nn_stats",
           "compute_nn_distances", "f1_curve_from_distances", "compute_f1_curve", "nn_distances", "nn_distances_resident",
           "points_bounds_resident", "voxel_iou_counts_resident", "voxel_iou_counts", "knn", "knn_resident", "compute_triangle_normals",
           "compute_vertex_normals", "compute_surface_metrics", "surface_metrics_per_vertex", "triangle_normals_resident",
           "vertex_normals_resident", "surface_metrics_resident", "KNN_MAX_K", "pointcloud_to_voxel_grid", "density_grid_resident",
           "point_to_mesh_distances", "point_to_mesh_distances_resident", "mesh_grid_shape", "sample_mesh_points",
           "sample_mesh_points_resident", "cloud_to_mesh_metrics", "isosurface", "get_marching_cubes_mesh",
           "marching_cubes_mesh_resident"]

KNN_MAX_K = 32      # PB3D_KNN_MAX_K
DENSITY_MAX_GRID = 1024     # the limits of pb3d_density_grid_resident
DENSITY_MAX_RADIUS = 64


# ---- geometry helpers (:18-22) ---------------------------------------------------------------------------------------------------------
def filter_mesh(vertices, faces, y_thresh=0.2):
    mask = vertices[:, 1] <= y_thresh
    valid_idx = np.where(mask)[0]
    face_mask = np.all(np.isin(faces, valid_idx), axis=1)
    return vertices[mask], faces[face_mask]


# ---- point lists on the device -----------------------------------------------------------------------------------------------------------
def nn_distances_resident(d_A, nA, d_B, nB, k=1, a_f64=True, b_f64=True, out=None):
    """pb3d_nn_dist_dev: a DeviceBuffer of nA float64 -- the k-th smallest distance (k = 1 or 2) from each point of the resident
    (nA, 3) list d_A to the resident (nB, 3) list d_B (float64 rows, or float32 with a_f64 / b_f64 False).  With k = 2 and d_A the
    same list as d_B a point's own copy counts (distance 0), as NearestNeighbors(2).kneighbors(X) of X itself does."""
    with dev.Scope() as sc:
        d_out = sc.result(out, max(1, int(nA)) * 8)
        _lib.check(_lib.load().pb3d_nn_dist_dev(_lib.ctx(), _ptr(d_A), int(bool(a_f64)), int(nA), _ptr(d_B), int(bool(b_f64)), int(nB), int(k),
                                                _ptr(d_out)))
        return d_out


def points_bounds_resident(d_P, n, f64=True, out=None):
    """pb3d_points_bounds_dev: a DeviceBuffer of 6 float64, the exact min (3) and max (3) of a resident (n, 3) list"""
    with dev.Scope() as sc:
        d_out = sc.result(out, 6 * 8)
        _lib.check(_lib.load().pb3d_points_bounds_dev(_lib.ctx(), _ptr(d_P), int(bool(f64)), int(n), _ptr(d_out)))
        return d_out


def voxel_iou_counts_resident(d_A, nA, d_B, nB, bounds_min, step, resolution, iters, a_f64=True, b_f64=True, calc_f32=False, out=None):
    """pb3d_voxel_iou_counts_dev: a DeviceBuffer of 2 int64, (#(occA & occB), #(occA | occB)) of voxel_iou's dilated occupancies"""
    lo = np.ascontiguousarray(np.asarray(bounds_min, dtype=np.float64).reshape(3))
    with dev.Scope() as sc:
        d_out = sc.result(out, 2 * 8)
        _lib.check(_lib.load().pb3d_voxel_iou_counts_dev(_lib.ctx(), _ptr(d_A), int(bool(a_f64)), int(nA), _ptr(d_B), int(bool(b_f64)), int(nB),
                                                         _lib.p_dbl(lo), float(step), int(bool(calc_f32)), int(resolution), int(iters),
                                                         _ptr(d_out)))
        return d_out


def nn_distances(A, B, k=1):
    """float64 (len(A),) array: the k-th nearest distance (k = 1 or 2) from each point of A to B, bit for bit
    cKDTree(B).query(A, k)[0] (its last column when k = 2)."""
    a, af = _cloud(A, "A")
    b, bf = _cloud(B, "B")
    if len(a) == 0:
        return np.zeros(0, np.float64)
    with dev.Scope() as sc:
        d_a = sc.upload(a)
        d_b = d_a if B is A else sc.upload(b)
        d_out = sc.adopt(nn_distances_resident(d_a, len(a), d_b, len(b), k, af, bf))
        return d_out.download((len(a),), np.float64)


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
    a, b, f64, dt = _iou_inputs(A, B)
    if len(a) + len(b) == 0:
        np.vstack([np.asarray(A), np.asarray(B)]).min(0)        # the reference's error on two empty clouds
    with dev.Scope() as sc:
        d_pts, bb = [], []
        for P in (a, b):
            d_p = sc.upload(P)
            d_pts.append(d_p)
            if d_p is not None:
                bb.append(sc.adopt(points_bounds_resident(d_p, len(P), f64)).download((6,), np.float64))
        bb = np.array(bb)
        bounds_min = bb[:, :3].min(0).astype(dt)
        bounds_max = bb[:, 3:].max(0).astype(dt)
        step = (bounds_max - bounds_min).max() / resolution
        iters = 0
        if dilate_frac > 0:
            iters = max(1, int(round(
                (dilate_frac * np.linalg.norm(bounds_max - bounds_min)) / step
            )))
        d_c = sc.adopt(voxel_iou_counts_resident(d_pts[0], len(a), d_pts[1], len(b), bounds_min, step, resolution, iters, f64, f64,
                                                 calc_f32=not f64))
        inter, union = (int(v) for v in d_c.download((2,), np.int64))
        return inter, union


def voxel_iou(A, B, resolution=96, dilate_frac=0.01):
    inter, union = voxel_iou_counts(A, B, resolution, dilate_frac)
    return inter / union if union > 0 else np.nan


# ---- density volume (:178-189) ---------------------------------------------------------------------------------------------------------
def _density_args(grid_size, sigma):
    """(grid_size, radius, weights): the limits of pb3d_density_grid_resident checked before anything is allocated, and the Gaussian
    kernel as the reference's Gaussian filter builds it (float64, radius = int(4 * sigma + 0.5), normalised by its own sum)"""
    G = operator.index(grid_size)
    if not 1 <= G <= DENSITY_MAX_GRID:
        raise ValueError(f"grid_size must be in [1, {DENSITY_MAX_GRID}] (got {G})")
    if not sigma > 0:
        return G, 0, None
    sd = float(sigma)
    radius = int(4.0 * sd + 0.5)
    if radius > DENSITY_MAX_RADIUS:
        raise ValueError(f"sigma = {sd} gives a filter radius of {radius}; the device filter is limited to radius {DENSITY_MAX_RADIUS} "
                         f"(sigma < {(DENSITY_MAX_RADIUS + 0.5) / 4.0})")
    x = np.arange(-radius, radius + 1)
    phi_x = np.exp(-0.5 / (sd * sd) * x ** 2)
    return G, radius, np.ascontiguousarray(phi_x / phi_x.sum())


def density_grid_resident(d_pts, n, grid_size=128, sigma=1.0, f64=True, out=None):
    """pb3d_density_grid_resident: a DeviceBuffer of grid_size^3 float32, pointcloud_to_voxel_grid of the resident (n, 3) list d_pts
    (float64 rows, or float32 with f64 False), bit for bit the reference's volume.  The coordinates must be finite."""
    G, radius, w = _density_args(grid_size, sigma)
    with dev.Scope() as sc:
        d_out = sc.result(out, G ** 3 * 4)
        _lib.check(_lib.load().pb3d_density_grid_resident(_lib.ctx(), _ptr(d_pts), int(bool(f64)), int(n), G,
                                                          None if w is None else _lib.p_dbl(w), radius, _ptr(d_out)))
        return d_out


def pointcloud_to_voxel_grid(points, grid_size=128, sigma=1.0):
    """float32 (grid_size,) * 3 density volume, bit for bit the reference's: the cloud normalised by
    pb3d.preprocess_helpers.normalize_preserve_aspect in its own dtype (float32 stays float32, other reals become float64), the points
    counted per voxel trunc(norm * (grid_size - 1)) -- the y indices are <= 0 and wrap to the far planes, as NumPy's do -- smoothed by
    the reference's Gaussian filter when sigma > 0, and the six faces set to 0."""
    p, f64 = _cloud(points)
    G, _, _ = _density_args(grid_size, sigma)
    if len(p) == 0:
        raise ValueError("zero-size array to reduction operation minimum which has no identity")
    _finite(p, "points")
    with dev.Scope() as sc:
        d_out = sc.adopt(density_grid_resident(sc.upload(p), len(p), G, sigma, f64))
        return d_out.download((G, G, G), np.float32)


# ---- isosurface of the density volume (:191-195; csrc/mesh.hip, include/pb3d.h states the rule) -----------------------------------------
def isosurface(volume, level, divisor=1.0):
    """(verts (n, 3) float32 in (a0, a1, a2) order, faces (m, 3) int32): the isosurface of a float32 (n0, n1, n2) volume at `level`
    by the rule of include/pb3d.h -- a lattice point is inside iff float64(v) > level; cases, vertex ownership and order are
    meshify_colored_voxel_grid's; an edge vertex sits at ia + (level - va) / (vb - va), in float64, rounded to float32 once; the
    centre vertex of the cases that have one stays at the cube centre; every coordinate is divided by float32(divisor).  A 0/1 volume
    at level 0.5 gives the lattice mesh of meshify_colored_voxel_grid byte for byte.  The mesh is closed and consistently oriented
    wherever the volume's border is outside; zero-area faces (values equal to the level) are kept.  A level outside the data range
    gives empty (0, 3) arrays.  Not skimage's Lewiner mesh on float input: on ambiguous cubes vertex and face counts can differ.
    Other real dtypes are converted to float32; non-finite values are refused (ValueError)."""
    v = np.asarray(volume)
    if v.dtype.kind not in "fiub":
        raise TypeError(f"isosurface takes a real-valued volume (got {v.dtype})")
    v = np.ascontiguousarray(v, dtype=np.float32)
    shape, level, divisor = dev.iso_check(v.shape, level, divisor)
    _finite(v, "volume")
    lib, ctx = _lib.load(), _lib.ctx()
    nv, nf = C.c_int64(0), C.c_int64(0)
    _lib.check(lib.pb3d_iso_count(ctx, v.ctypes.data_as(C.c_void_p), *shape, level, divisor, C.byref(nv), C.byref(nf)))
    verts = _hostmem.empty((nv.value, 3), np.float32)
    faces = _hostmem.empty((nf.value, 3), np.int32)
    _lib.check(lib.pb3d_iso_fill(ctx, nv.value, nf.value, verts.ctypes.data_as(C.c_void_p), faces.ctypes.data_as(C.c_void_p)))
    return verts, faces


def marching_cubes_mesh_resident(d_pts, n, grid_size=128, sigma=1.0, level=0.1, f64=True):
    """get_marching_cubes_mesh of a resident (n, 3) cloud, the mesh left on the device: ((DeviceBuffer of nv x 3 float32 vertices,
    DeviceBuffer of nf x 3 int32 faces), (nv, nf)) as pb3d.device.isosurface(download=False) hands them out -- the density volume
    (density_grid_resident) never leaves the device and is freed before the call returns."""
    with dev.Scope() as sc:
        d_vol = sc.adopt(density_grid_resident(d_pts, n, grid_size, sigma, f64))
        G = operator.index(grid_size)
        return dev.isosurface(d_vol, (G, G, G), level, divisor=G, download=False)


def get_marching_cubes_mesh(points, grid_size=128, sigma=1.0, level=0.1):
    """(verts, faces) of the reference (:191-195): pointcloud_to_voxel_grid's density volume (bit for bit the reference's), its
    isosurface at `level` by the rule of isosurface() -- this project's own, not skimage's Lewiner mesh on float input -- and the
    vertices divided by grid_size in float32, as the reference's verts /= grid_size does.  The cloud goes up once, the volume stays on
    the device, the two arrays come down.  A level outside the volume's range gives empty (0, 3) arrays (skimage raises there)."""
    p, f64 = _cloud(points)
    G, _, _ = _density_args(grid_size, sigma)
    if len(p) == 0:
        raise ValueError("zero-size array to reduction operation minimum which has no identity")
    _finite(p, "points")
    if G < 2:
        raise ValueError("Input array must be at least 2x2x2.")
    with dev.Scope() as sc:
        bufs, (nv, nf) = marching_cubes_mesh_resident(sc.upload(p), len(p), G, sigma, level, f64)
        d_v, d_f = sc.adopt(bufs)
        if nv == 0:
            return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
        return d_v.download((nv, 3), np.float32), d_f.download((nf, 3), np.int32)


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


# ---- exact k nearest neighbours (NearestNeighbors(n_neighbors=k).fit(B).kneighbors(A)) ----------------------------------------------
def _check_k(k, n_fit):
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)):
        raise TypeError(f"n_neighbors does not take {type(k)} value, enter integer value")
    if k < 1 or k > KNN_MAX_K:
        raise ValueError(f"k must be in [1, {KNN_MAX_K}] (got {k})")
    if k > n_fit:
        raise ValueError(f"Expected n_neighbors <= n_samples_fit, but n_neighbors = {k}, n_samples_fit = {n_fit}")
    return int(k)


def _check_k_metrics(k, nv):
    """compute_surface_metrics' k: the neighbour search's limits, and PCA(n_components=3) needs three samples"""
    k = _check_k(k, nv)
    if k < 3:
        raise ValueError(f"n_components=3 must be between 0 and min(n_samples, n_features)={k} with svd_solver='full'")
    return k


def _finite(a, what):
    if not np.isfinite(a).all():
        raise ValueError(f"Input {what} contains NaN or infinity.")


def knn_resident(d_A, nA, d_B, nB, k, a_f64=True, b_f64=True, dist=True):
    """pb3d_knn_dev: (DeviceBuffer of nA x k float64 distances or None, DeviceBuffer of nA x k int32 positions in d_B), each row
    ascending by (squared distance, position)."""
    k = _check_k(k, int(nB))
    with dev.Scope() as sc:
        d_idx = sc.result(None, max(1, int(nA) * k) * 4)
        d_dist = sc.result(None, max(1, int(nA) * k) * 8) if dist else None
        _lib.check(_lib.load().pb3d_knn_dev(_lib.ctx(), _ptr(d_A), int(bool(a_f64)), int(nA), _ptr(d_B), int(bool(b_f64)), int(nB), k,
                                            _ptr(d_dist), _ptr(d_idx)))
        return d_dist, d_idx


def knn(A, B, k):
    """(dist float64 (len(A), k), idx int32 (len(A), k)): the k nearest points of B for each point of A, nearest first; equal
    distances in ascending index order, which also decides who is in the row.  The distances are bit for bit
    NearestNeighbors(n_neighbors=k).fit(B).kneighbors(A)[0]; the indices are too wherever no two candidates tie."""
    a, af = _cloud(A, "A")
    b, bf = _cloud(B, "B")
    k = _check_k(k, len(b))
    _finite(a, "A")
    _finite(b, "B")
    if len(a) == 0:
        return np.zeros((0, k), np.float64), np.zeros((0, k), np.int32)
    with dev.Scope() as sc:
        d_a = sc.upload(a)
        d_b = d_a if B is A else sc.upload(b)
        d_dist, d_idx = sc.adopt(knn_resident(d_a, len(a), d_b, len(b), k, af, bf))
        return d_dist.download((len(a), k), np.float64), d_idx.download((len(a), k), np.int32)


# ---- mesh regularity (:198-245) --------------------------------------------------------------------------------------------------------
def _mesh_arrays(vertices, faces):
    """(vertices, vertex flag, faces int64) as the kernels read them; the reference's dtypes: float32 stays, other reals -> float64"""
    v, vf = _cloud(vertices, "vertices")
    f = np.asarray(faces)
    if f.dtype.kind not in "iu":
        raise IndexError("arrays used as indices must be of integer (or boolean) type")
    if f.ndim != 2 or f.shape[1] != 3:
        raise ValueError(f"faces must be an (m, 3) array (got shape {f.shape})")
    if f.dtype.kind == "u" and f.size and int(f.max()) >= len(v):       # before the cast to int64 could wrap it
        raise IndexError(f"index {int(f.max())} is out of bounds for axis 0 with size {len(v)}")
    return v, vf, np.ascontiguousarray(f, dtype=np.int64)


def triangle_normals_resident(d_verts, nv, d_faces, nf, verts_f64=False, faces_i64=False, out=None):
    """pb3d_triangle_normals_dev: a DeviceBuffer of nf x 3 face normals in the vertex dtype (IndexError on a bad face index)"""
    with dev.Scope() as sc:
        d_out = sc.result(out, max(1, int(nf)) * 3 * (8 if verts_f64 else 4))
        _lib.check(_lib.load().pb3d_triangle_normals_dev(_lib.ctx(), _ptr(d_verts), int(bool(verts_f64)), int(nv), _ptr(d_faces),
                                                         int(bool(faces_i64)), int(nf), _ptr(d_out)))
        return d_out


def vertex_normals_resident(d_verts, nv, d_faces, nf, verts_f64=False, faces_i64=False, out=None):
    """pb3d_vertex_normals_dev: a DeviceBuffer of nv x 3 vertex normals in the vertex dtype (IndexError on a bad face index)"""
    with dev.Scope() as sc:
        d_out = sc.result(out, max(1, int(nv)) * 3 * (8 if verts_f64 else 4))
        _lib.check(_lib.load().pb3d_vertex_normals_dev(_lib.ctx(), _ptr(d_verts), int(bool(verts_f64)), int(nv), _ptr(d_faces),
                                                       int(bool(faces_i64)), int(nf), _ptr(d_out)))
        return d_out


def surface_metrics_resident(d_verts, nv, d_faces, nf, k=20, verts_f64=False, faces_i64=False):
    """The per-vertex quantities of compute_surface_metrics for a resident mesh (pb3d.device.meshify(..., download=False) hands out
    float32 vertices and int32 faces): a DeviceBuffer of 3 x nv float64 -- normal angle spread (degrees), smallest PCA eigenvalue,
    |neighbour mean - vertex| -- from pb3d_vertex_normals_dev, pb3d_knn_dev on the vertices themselves and pb3d_surface_metrics_dev.
    The vertices must be finite."""
    nv = int(nv)
    k = _check_k_metrics(k, nv)
    with dev.Scope() as sc:
        d_n = sc.adopt(vertex_normals_resident(d_verts, nv, d_faces, nf, verts_f64, faces_i64))
        _, d_idx = sc.adopt(knn_resident(d_verts, nv, d_verts, nv, k, verts_f64, verts_f64, dist=False))
        d_out = sc.result(None, max(1, nv) * 3 * 8)
        _lib.check(_lib.load().pb3d_surface_metrics_dev(_lib.ctx(), _ptr(d_verts), _ptr(d_n), int(bool(verts_f64)), nv, _ptr(d_idx), k,
                                                        d_out.at(0), d_out.at(nv * 8), d_out.at(2 * nv * 8)))
        return d_out


def _normals(vertices, faces, per_vertex):
    v, vf, f = _mesh_arrays(vertices, faces)
    n = len(v) if per_vertex else len(f)
    if len(v) == 0 and len(f):
        v[f[:, 0]]                                                      # the reference's IndexError
    if n == 0:
        return np.zeros((0, 3), v.dtype)
    with dev.Scope() as sc:
        d_v, d_f = sc.upload(v), sc.upload(f if len(f) else np.zeros((1, 3), np.int64))
        fn = vertex_normals_resident if per_vertex else triangle_normals_resident
        d_out = sc.adopt(fn(d_v, len(v), d_f, len(f), vf, True))
        return d_out.download((n, 3), v.dtype)


def compute_triangle_normals(vertices, faces):
    """(m, 3) unit face normals in the vertex dtype, bit for bit the reference's (:198-203)"""
    return _normals(vertices, faces, per_vertex=False)


def compute_vertex_normals(vertices, faces):
    """(n, 3) vertex normals in the vertex dtype: the face normals of each vertex added in ascending face order and normalised, bit for
    bit the reference's loop (:206-212)"""
    return _normals(vertices, faces, per_vertex=True)


def surface_metrics_per_vertex(vertices, faces, k=20):
    """(normal_stds, roughness_vals, mean_curvatures): the three per-vertex lists of compute_surface_metrics as float64 arrays"""
    v, vf, f = _mesh_arrays(vertices, faces)
    k = _check_k_metrics(k, len(v))
    _finite(v, "X")
    with dev.Scope() as sc:
        d_v, d_f = sc.upload(v), sc.upload(f if len(f) else np.zeros((1, 3), np.int64))
        d_out = sc.adopt(surface_metrics_resident(d_v, len(v), d_f, len(f), k, vf, True))
        out = d_out.download((3, len(v)), np.float64)
        return out[0], out[1], out[2]


def compute_surface_metrics(vertices, faces, k=20):
    normal_stds, roughness_vals, mean_curvatures = surface_metrics_per_vertex(vertices, faces, k)
    return {
        "Normal StdDev (°)": np.mean(normal_stds),
        "Mean Roughness (λ₃)": np.mean(roughness_vals),
        "Mean Curvature": np.mean(mean_curvatures),
    }


# ---- a triangle mesh as a comparison target (csrc/meshdist.hip; include/pb3d.h states the arithmetic) ---------------------------------
def point_to_mesh_distances_resident(d_P, nP, d_verts, nv, d_faces, nf, p_f64=True, verts_f64=False, faces_i64=False, return_faces=False,
                                     return_closest=False):
    """pb3d_mesh_dist_resident: (DeviceBuffer of nP float64 distances, DeviceBuffer of nP int32 nearest faces or None, DeviceBuffer of
    nP x 3 float64 closest points or None) of the resident (nP, 3) list d_P against the resident mesh (IndexError on a bad face index).
    Points and vertices must be finite."""
    nP = int(nP)
    with dev.Scope() as sc:
        bufs = [sc.result(None, max(1, nP) * 8), sc.result(None, max(1, nP) * 4) if return_faces else None,
                sc.result(None, max(1, nP) * 24) if return_closest else None]
        _lib.check(_lib.load().pb3d_mesh_dist_resident(_lib.ctx(), _ptr(d_P), int(bool(p_f64)), nP, _ptr(d_verts), int(bool(verts_f64)), int(nv),
                                                       _ptr(d_faces), int(bool(faces_i64)), int(nf), *[_ptr(b) for b in bufs]))
        return tuple(bufs)


def mesh_grid_shape():
    """pb3d_mesh_grid_shape: ((cells per axis), entries, halvings) of the triangle index the last point-to-mesh search built"""
    cells, entries, halvings = (C.c_int64 * 3)(), C.c_int64(0), C.c_int64(0)
    _lib.check(_lib.load().pb3d_mesh_grid_shape(_lib.ctx(), cells, C.byref(entries), C.byref(halvings)))
    return tuple(cells), entries.value, halvings.value


def _mesh_on_device(vertices, faces, what):
    """(vertices, flag, faces) validated for the mesh entries: at least one face, finite vertices"""
    v, vf, f = _mesh_arrays(vertices, faces)
    if len(f) == 0:
        raise ValueError(f"{what}: the mesh has no faces")
    if len(v) == 0:
        v[f[:, 0]]                                                      # NumPy's IndexError
    _finite(v, "vertices")
    return v, vf, f


def point_to_mesh_distances(P, vertices, faces, return_faces=False, return_closest=False):
    """float64 (len(P),) array: the distance from each point of P to the nearest point of the mesh surface, exact in the sense of
    include/pb3d.h (Ericson's closest point on every candidate face in float64, the minimum over ALL faces, ties to the lowest face).
    With return_faces also the int32 face index of each point, with return_closest also the (len(P), 3) float64 closest points, in
    that order."""
    p, pf = _cloud(P, "P")
    _finite(p, "P")
    if len(p) == 0:
        out = (np.zeros(0, np.float64),) + ((np.zeros(0, np.int32),) if return_faces else ()) + \
            ((np.zeros((0, 3), np.float64),) if return_closest else ())
        return out if len(out) > 1 else out[0]
    v, vf, f = _mesh_on_device(vertices, faces, "point_to_mesh_distances")
    with dev.Scope() as sc:
        outs = sc.adopt(point_to_mesh_distances_resident(sc.upload(p), len(p), sc.upload(v), len(v), sc.upload(f), len(f), pf, vf, True,
                                                         return_faces, return_closest))
        res = [outs[0].download((len(p),), np.float64)]
        if return_faces:
            res.append(outs[1].download((len(p),), np.int32))
        if return_closest:
            res.append(outs[2].download((len(p), 3), np.float64))
        return tuple(res) if len(res) > 1 else res[0]


def _sample_args(n, seed):
    n, seed = operator.index(n), operator.index(seed)
    if n < 0:
        raise ValueError(f"n must be >= 0 (got {n})")
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f"seed must be in [0, 2^64) (got {seed})")
    return n, seed


def sample_mesh_points_resident(d_verts, nv, d_faces, nf, n, seed=0, verts_f64=False, faces_i64=False, return_faces=True):
    """pb3d_mesh_sample_resident: (DeviceBuffer of n x 3 float64 surface points, DeviceBuffer of n int32 faces or None), stratified by
    area and a function of (mesh, n, seed) alone (ValueError if the mesh's area is 0, IndexError on a bad face index)"""
    n, seed = _sample_args(n, seed)
    with dev.Scope() as sc:
        d_pts = sc.result(None, max(1, n) * 24)
        d_face = sc.result(None, max(1, n) * 4) if return_faces else None
        _lib.check(_lib.load().pb3d_mesh_sample_resident(_lib.ctx(), _ptr(d_verts), int(bool(verts_f64)), int(nv), _ptr(d_faces),
                                                         int(bool(faces_i64)), int(nf), n, seed, _ptr(d_pts), _ptr(d_face)))
        return d_pts, d_face


def sample_mesh_points(vertices, faces, n, seed=0, return_faces=False):
    """(n, 3) float64 points of the mesh surface, area-weighted and stratified: sample i falls in the i-th of n equal slices of the
    cumulative face area, so consecutive samples lie on consecutive faces and every face gets its share to within 2 samples.  The
    same (mesh, n, seed) gives the same bytes.  With return_faces also the int32 face of each sample."""
    n, seed = _sample_args(n, seed)
    if n == 0:
        return (np.zeros((0, 3), np.float64), np.zeros(0, np.int32)) if return_faces else np.zeros((0, 3), np.float64)
    v, vf, f = _mesh_on_device(vertices, faces, "sample_mesh_points")
    with dev.Scope() as sc:
        d_pts, d_face = sc.adopt(sample_mesh_points_resident(sc.upload(v), len(v), sc.upload(f), len(f), n, seed, vf, True, return_faces))
        pts = d_pts.download((n, 3), np.float64)
        return (pts, d_face.download((n,), np.int32)) if return_faces else pts


def cloud_to_mesh_metrics(P, vertices, faces, tau, n_samples=None, seed=0):
    """A cloud against a mesh, both ways: accuracy = mean distance of P to the surface, completeness = mean distance of n_samples
    (default len(P)) area-weighted surface samples to P, precision / recall = the shares of each below tau (strict), and their F1 as
    fscore_with_threshold forms it."""
    d_P = point_to_mesh_distances(P, vertices, faces)
    S = sample_mesh_points(vertices, faces, len(d_P) if n_samples is None else n_samples, seed)
    d_S = nn_distances(S, P)
    precision = float(np.mean(d_P < tau))
    recall = float(np.mean(d_S < tau))
    f1 = 0.0 if (precision + recall) == 0 else (
        2 * precision * recall / (precision + recall)
    )
    return {"accuracy": float(np.mean(d_P)), "completeness": float(np.mean(d_S)), "precision": precision, "recall": recall, "f1": f1}


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
