"""Thinning a triangle mesh on the device: vertex clustering (Rossignac & Borrel; Open3D's simplify_vertex_clustering), the one mesh ->
mesh step that changes the faces.  A stride-1 marching-cubes mesh has a vertex on every crossed lattice edge; render_mesh,
point_to_mesh_distances, sample_mesh_points and smooth_mesh all cost time in proportion to its faces, and re-meshing at a stride loses
thin parts -- and cannot be done to a CAD model or a smoothed mesh at all.

include/pb3d.h states the result to the bit.  The clusters are voxel_downsample's voxels of the whole vertex list (same origin rule, same
cells, numbered by first appearance, centroid or first vertex); a face is mapped to the clusters of its corners, dropped when two of them
are equal and, with duplicate_faces="drop", when an earlier face has the same three clusters in the same cyclic order (the mirror image
is another face and stays); the clusters no remaining face names are dropped and the rest renumbered in order.  Faces keep their order
and their corner order.  colors (uint8, one or three bytes a vertex: meshify's nearest-voxel bytes, a label) follow the first vertex of
each cluster, unblended.  With duplicate_faces="keep" a closed, consistently oriented mesh stays one (every directed edge keeps its
reverse), so voxelize_mesh's crossing parity survives; "drop" may open a thin part that folds onto itself.

compact_mesh is the face half alone, every vertex its own cluster: it removes faces with a repeated corner, repeated faces and
unreferenced vertices, and copies the vertices byte for byte.

This is not quadric-error simplification, no representative is moved to a quadric optimum, and vertices are never welded by coordinate
equality.

csrc/simplify.hip: pb3d_voxel_downsample_resident for the clusters, three stable radix sorts (csrc/sort_pairs.hip) of the rotated
triples for the repeats, two scans and two gathers -- no state per cluster, no floating-point atomics.  The NumPy forms upload the mesh
and download the arrays; the *_resident twins take and return device handles (pb3d.device.DeviceBuffer)."""
import ctypes as C

import numpy as np

from . import _lib, device as dev
from ._args import _counts, _finite_cloud, _mesh, _voxel_size
from ._lib import _ptr
from .downsample import _origin, _reduce

__all__ = ["simplify_mesh", "simplify_mesh_resident", "compact_mesh", "compact_mesh_resident"]

DUPLICATE_FACES = {"drop": 0, "keep": 1}


def _duplicate_faces(duplicate_faces):
    if not isinstance(duplicate_faces, str) or duplicate_faces not in DUPLICATE_FACES:
        raise ValueError(f"duplicate_faces must be 'drop' or 'keep' (got {duplicate_faces!r})")
    return DUPLICATE_FACES[duplicate_faces]


def _channels(channels):
    if channels not in (1, 3):
        raise ValueError(f"channels must be 1 or 3 (got {channels!r})")
    return int(channels)


def _colors(colors, nv):
    """the contiguous (nv, 1 or 3) uint8 array, or None"""
    if colors is None:
        return None
    c = _lib.as_u8(colors, "colors")
    if c.ndim != 2 or c.shape[0] != nv or c.shape[1] not in (1, 3):
        raise ValueError(f"colors must have shape ({nv}, 1) or ({nv}, 3) (got {c.shape})")
    return c


def _resident(call, nv, nf, d_colors, channels, verts_f64, faces_i64):
    """the output buffers of either entry around `call(outputs..., counts)`: (d_vertices, d_faces, d_colors or None, d_index, d_inverse,
    d_face_index, (vertices, faces) written)"""
    counts = (C.c_int64 * 2)(0, 0)
    with dev.Scope() as sc:
        bufs = [sc.result(None, max(1, nv) * (24 if verts_f64 else 12)), sc.result(None, max(1, nf) * (24 if faces_i64 else 12)),
                sc.result(None, max(1, nv) * channels) if d_colors is not None else None, sc.result(None, max(1, nv) * 4),
                sc.result(None, max(1, nv) * 4), sc.result(None, max(1, nf) * 4)]
        _lib.check(call(*(_ptr(b) for b in bufs), counts))
        return (*bufs, (int(counts[0]), int(counts[1])))


def simplify_mesh_resident(d_verts, n_vertices, d_faces, n_faces, voxel_size, origin=None, reduce="centroid", duplicate_faces="drop",
                           d_colors=None, channels=3, verts_f64=False, faces_i64=False):
    """pb3d_mesh_simplify_resident: (d_vertices, d_faces, d_colors, d_index, d_inverse, d_face_index, (n, m)) -- DeviceBuffers with room
    for n_vertices rows of vertices in the input dtype (float32, or float64 with verts_f64), n_faces rows of faces in the input dtype
    (int32, or int64 with faces_i64), n_vertices x channels colour bytes (None unless d_colors is given), n_vertices int32 first
    vertices, n_vertices int32 new numbers (-1: dropped) and n_faces int32 face positions; the first n rows / m rows are written, the
    inverse whole.  pb3d.device.meshify(..., download=False) hands out what this takes: float32 vertices, int32 faces, n x C bytes.
    Host waits: the index check (IndexError on a bad face index, nothing written), voxel_downsample's two, and (n, m).  The caller
    frees the buffers."""
    nv, nf = _counts(n_vertices, n_faces)
    voxel_size, o, r, dup, channels = _voxel_size(voxel_size), _origin(origin), _reduce(reduce), _duplicate_faces(duplicate_faces), _channels(channels)
    lib, ctx = _lib.load(), _lib.ctx()
    return _resident(lambda *out: lib.pb3d_mesh_simplify_resident(ctx, _ptr(d_verts), int(bool(verts_f64)), nv, _ptr(d_faces), int(bool(faces_i64)), nf,
                                                                  voxel_size, None if o is None else _lib.p_dbl(o), r, dup, _ptr(d_colors),
                                                                  channels, *out),
                     nv, nf, d_colors, channels, verts_f64, faces_i64)


def compact_mesh_resident(d_verts, n_vertices, d_faces, n_faces, duplicate_faces="drop", d_colors=None, channels=3, verts_f64=False,
                          faces_i64=False):
    """pb3d_mesh_compact_resident: simplify_mesh_resident's tuple with every vertex its own cluster and the vertices copied byte for
    byte.  Host waits: the index check and (n, m)."""
    nv, nf = _counts(n_vertices, n_faces)
    dup, channels = _duplicate_faces(duplicate_faces), _channels(channels)
    lib, ctx = _lib.load(), _lib.ctx()
    return _resident(lambda *out: lib.pb3d_mesh_compact_resident(ctx, _ptr(d_verts), int(bool(verts_f64)), nv, _ptr(d_faces), int(bool(faces_i64)), nf,
                                                                 dup, _ptr(d_colors), channels, *out),
                     nv, nf, d_colors, channels, verts_f64, faces_i64)


def _numpy_form(resident, v, f, c, want):
    """upload, run `resident(d_verts, nv, d_faces, nf, d_colors, channels)`, download what `want` = (index, inverse, face_index) asks"""
    nv, nf = len(v), len(f)

    def pack(verts, faces, colors, index, inverse, face_index):
        out = [verts, faces] + ([colors] if c is not None else [])
        return tuple(out + [a for a, w in zip((index, inverse, face_index), want) if w])

    if nf == 0:     # nothing stays, and nothing needs the device
        return pack(v[:0].copy(), f[:0].copy(), None if c is None else c[:0].copy(), np.zeros(0, np.intp), np.full(nv, -1, np.intp),
                    np.zeros(0, np.intp))
    with dev.Scope() as sc:
        d_c = sc.upload(c) if c is not None else None
        *bufs, (n, m) = resident(sc.upload(v), nv, sc.upload(f), nf, d_c, c.shape[1] if c is not None else 3)
        sc.adopt(bufs)
        return pack(bufs[0].download((n, 3), v.dtype), bufs[1].download((m, 3), f.dtype),
                    bufs[2].download((n, c.shape[1])) if c is not None else None,
                    bufs[3].download((n,), np.int32).astype(np.intp) if want[0] else None,
                    bufs[4].download((nv,), np.int32).astype(np.intp) if want[1] else None,
                    bufs[5].download((m,), np.int32).astype(np.intp) if want[2] else None)


def simplify_mesh(vertices, faces, voxel_size, origin=None, reduce="centroid", duplicate_faces="drop", colors=None, return_index=False,
                  return_inverse=False, return_face_index=False):
    """Vertex-clustering simplification of an (n, 3) vertex array over an (m, 3) integer face array: (vertices, faces[, colors][, index]
    [, inverse][, face_index]).  The vertices of one voxel of edge `voxel_size` (voxel_downsample's voxels, `origin` and `reduce`
    included) become one vertex; faces with two corners in one cluster are dropped, and with duplicate_faces="drop" so is every later
    face with the same three clusters in the same cyclic order; clusters without a face are dropped.  float32 vertices stay float32,
    other real dtypes become float64; int32 faces stay int32, other integer types become int64; negative indices wrap as NumPy's do
    and one outside [-n, n) is an IndexError.  colors: (n, 1 or 3) uint8, each output vertex gets the bytes of its cluster's first
    vertex.  Extras (intp): index, the first input vertex of each output vertex; inverse, the output vertex of each input vertex or -1;
    face_index, the input position of each output face.  No faces in, or all of them collapsed: (0, 3) and (0, 3)."""
    voxel_size, o, _, _ = _voxel_size(voxel_size), _origin(origin), _reduce(reduce), _duplicate_faces(duplicate_faces)
    v, vf, f, fi = _mesh(vertices, faces)
    _finite_cloud(v)
    c = _colors(colors, len(v))
    return _numpy_form(lambda d_v, nv, d_f, nf, d_c, ch: simplify_mesh_resident(d_v, nv, d_f, nf, voxel_size, o, reduce, duplicate_faces, d_c, ch,
                                                                                vf, fi),
                       v, f, c, (return_index, return_inverse, return_face_index))


def compact_mesh(vertices, faces, duplicate_faces="drop", colors=None, return_index=False, return_inverse=False, return_face_index=False):
    """simplify_mesh with every vertex its own cluster and no arithmetic: faces with a repeated corner, repeated faces
    (duplicate_faces="drop") and unreferenced vertices are removed, and the vertices that stay are copied byte for byte (non-finite
    coordinates included)."""
    _duplicate_faces(duplicate_faces)
    v, vf, f, fi = _mesh(vertices, faces)
    c = _colors(colors, len(v))
    return _numpy_form(lambda d_v, nv, d_f, nf, d_c, ch: compact_mesh_resident(d_v, nv, d_f, nf, duplicate_faces, d_c, ch, vf, fi),
                       v, f, c, (return_index, return_inverse, return_face_index))
