"""Smoothing a triangle mesh on the device: the step every user takes between marching cubes and anything that measures, samples or
aligns the surface.  meshify_colored_voxel_grid is binary marching cubes, so its vertices sit on a half-voxel lattice and the surface is
a staircase; compute_surface_metrics, point_to_mesh_distances, sample_mesh_points and the point-to-plane icp_align all inherit it.  A few
rounds of Taubin smoothing (trimesh.smoothing.filter_taubin, Open3D's filter_smooth_taubin) remove the staircase without the shrinkage
of plain Laplacian smoothing.

include/pb3d.h states the result to the bit.  Face (a, b, c) gives the directed pairs (a,b) (b,a) (b,c) (c,b) (c,a) (a,c), pairs with
equal ends dropped; N(i) is the ascending set of j with a pair (i, j); the multiplicity of (i, j) is the number of such pairs and a vertex
on a pair of multiplicity 1 is a boundary vertex.  One step with factor f moves every free vertex with a neighbour, per axis in float64:
s = 0.0, s = s + x_j over N(i) ascending, m = s / deg, d = m - x_i, x_i + f * d -- one rounded operation each, all vertices reading the
positions from before the step.  Taubin is a step with `lamb` then a step with `mu` per iteration, Laplacian a step with `lamb`; the
positions are widened once and rounded to the input dtype once.

Smoothing moves vertices and nothing else: the faces and the per-vertex colours of a mesh stay valid beside the new vertices, so
meshify_colored_voxel_grid's other outputs go on being used as they are (its normals describe the old surface: compute_vertex_normals
gives the new ones).

csrc/smooth.hip: the pairs go through two stable radix sorts (csrc/sort_pairs.hip), a scan compacts the unique ones, run lengths are the
multiplicities; a step is one lane per vertex, one wavefront for a vertex of degree above 32 -- no floating-point atomics.  The NumPy
forms upload the mesh and download the arrays; the *_resident twins take and return device handles (pb3d.device.DeviceBuffer)."""
import ctypes as C
import math

import numpy as np

from . import _lib, device as dev
from ._args import MAX_FACES, MAX_VERTICES, _cloud, _counts, _faces  # noqa: F401
from ._lib import _ptr

__all__ = ["mesh_vertex_adjacency", "mesh_vertex_adjacency_resident", "smooth_mesh", "smooth_mesh_resident"]

METHODS = ("taubin", "laplacian")


def _iterations(iterations):
    if isinstance(iterations, (bool, np.bool_)) or not isinstance(iterations, (int, np.integer)) or not 0 <= iterations <= 2 ** 30:
        raise ValueError(f"iterations must be an integer in [0, 2^30] (got {iterations!r})")
    return int(iterations)


def _factors(method, lamb, mu):
    """(lambda, mu) as the entry takes them: mu = NaN selects Laplacian smoothing"""
    if not isinstance(method, str) or method not in METHODS:
        raise ValueError(f"method must be 'taubin' or 'laplacian' (got {method!r})")
    lamb = float(lamb)
    if not math.isfinite(lamb):
        raise ValueError(f"lamb must be finite (got {lamb!r})")
    if method == "laplacian":
        return lamb, math.nan
    mu = float(mu)
    if not math.isfinite(mu):
        raise ValueError(f"mu must be finite (got {mu!r})")
    return lamb, mu


def mesh_vertex_adjacency_resident(d_faces, n_vertices, n_faces, faces_i64=False, multiplicity=False, boundary=False):
    """pb3d_mesh_adjacency_resident: (d_starts, d_neighbours, d_mult, d_boundary, total) -- DeviceBuffers of n_vertices + 1 int64, room for
    6 * n_faces int32 of which the first `total` are written, the same of uint32 (None unless `multiplicity`) and n_vertices bytes (None
    unless `boundary`).  total is the call's one download.  The caller frees the buffers.  IndexError on a face index outside
    [-n_vertices, n_vertices)."""
    nv, nf = _counts(n_vertices, n_faces)
    room = max(1, 6 * nf) * 4
    total = C.c_int64(0)
    with dev.Scope() as sc:
        bufs = [sc.result(None, (nv + 1) * 8), sc.result(None, room), sc.result(None, room) if multiplicity else None,
                sc.result(None, max(1, nv)) if boundary else None]
        _lib.check(_lib.load().pb3d_mesh_adjacency_resident(_lib.ctx(), _ptr(d_faces), int(bool(faces_i64)), nv, nf, _ptr(bufs[0]), _ptr(bufs[1]),
                                                            _ptr(bufs[2]), _ptr(bufs[3]), C.byref(total)))
        return bufs[0], bufs[1], bufs[2], bufs[3], int(total.value)


def mesh_vertex_adjacency(faces, n_vertices, return_multiplicity=False, return_boundary=False):
    """The vertex-to-vertex adjacency of an (m, 3) integer face list over n_vertices vertices, in CSR form: (starts, neighbours) with
    starts (n_vertices + 1 int64) and neighbours (int32) -- the neighbours of vertex i are neighbours[starts[i]:starts[i + 1]], ascending.
    Negative indices wrap as NumPy's do; one outside [-n_vertices, n_vertices) is an IndexError.  Degenerate faces contribute the pairs
    of their distinct corners.  Extras, in this order: multiplicity (int64, beside neighbours: the number of face corners pairs that
    give the directed pair; 1 = an edge of one face), boundary (bool per vertex: it is an end of a pair of multiplicity 1)."""
    nv = _counts(n_vertices, 0)[0]
    f, fi = _faces(faces, nv)
    nf = len(f)
    with dev.Scope() as sc:
        *bufs, total = mesh_vertex_adjacency_resident(sc.upload(f), nv, nf, fi, return_multiplicity, return_boundary)
        sc.adopt(bufs)
        out = [bufs[0].download((nv + 1,), np.int64), bufs[1].download((total,), np.int32)]
        if return_multiplicity:
            out.append(bufs[2].download((total,), np.uint32).astype(np.int64))
        if return_boundary:
            out.append(bufs[3].download((nv,), np.uint8).astype(bool))
        return tuple(out)


def smooth_mesh_resident(d_verts, n_vertices, d_faces, n_faces, iterations=10, method="taubin", lamb=0.5, mu=-0.53, d_fixed=None,
                         fix_boundary=False, verts_f64=False, faces_i64=False, out=None):
    """pb3d_mesh_smooth_resident: a DeviceBuffer of n_vertices x 3 smoothed vertices in the input dtype (float32, or float64 with verts_f64)
    -- pb3d.device.meshify(..., download=False) hands out float32 vertices and int32 faces.  d_fixed: n_vertices bytes, non-zero = the
    vertex stays, or None.  Everything is enqueued behind the index check (IndexError on a bad face index).  `out` may not be d_verts."""
    nv, nf = _counts(n_vertices, n_faces)
    iterations = _iterations(iterations)
    lamb, mu = _factors(method, lamb, mu)
    with dev.Scope() as sc:
        d_out = sc.result(out, max(1, nv) * 3 * (8 if verts_f64 else 4))
        _lib.check(_lib.load().pb3d_mesh_smooth_resident(_lib.ctx(), _ptr(d_verts), int(bool(verts_f64)), nv, _ptr(d_faces), int(bool(faces_i64)), nf,
                                                         iterations, lamb, mu, _ptr(d_fixed), int(bool(fix_boundary)), _ptr(d_out)))
        return d_out


def smooth_mesh(vertices, faces, iterations=10, method="taubin", lamb=0.5, mu=-0.53, fixed=None, fix_boundary=False):
    """`iterations` rounds of Taubin (a step with `lamb`, then one with `mu`) or Laplacian (`method="laplacian"`: a step with `lamb`; `mu`
    is ignored) smoothing of an (n, 3) vertex array over an (m, 3) integer face array, uniform weights.  Returns the new vertices in the
    input dtype: float32 stays float32 (the arithmetic is float64, rounded once at the end), other real dtypes become float64.
    fixed: a mask of n entries, true = the vertex stays; fix_boundary also keeps every vertex on an edge of a single face.
    The faces and the colours of the mesh are untouched by smoothing: meshify_colored_voxel_grid's other outputs stay valid beside the
    new vertices."""
    iterations = _iterations(iterations)
    _factors(method, lamb, mu)
    v, vf = _cloud(vertices, "vertices")
    nv = len(v)
    f, fi = _faces(faces, nv)
    nf = len(f)
    fx = None
    if fixed is not None:
        fx = np.asarray(fixed)
        if fx.shape != (nv,) or fx.dtype.kind not in "biu":
            raise ValueError(f"fixed must be a mask of {nv} entries (got shape {fx.shape}, dtype {fx.dtype})")
        fx = np.ascontiguousarray(fx != 0).view(np.uint8)
    if nv == 0:
        if nf:
            raise IndexError(f"index {int(f.reshape(-1)[0])} is out of bounds for axis 0 with size 0")
        return v.copy()
    with dev.Scope() as sc:
        d_v, d_f = sc.upload(v), sc.upload(f)
        d_x = sc.upload(fx) if fx is not None else None
        d_out = sc.adopt(smooth_mesh_resident(d_v, nv, d_f, nf, iterations, method, lamb, mu, d_x, fix_boundary, vf, fi))
        return d_out.download((nv, 3), v.dtype)
