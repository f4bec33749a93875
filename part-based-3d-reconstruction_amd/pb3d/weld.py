"""Welding the vertices of a mesh by exact coordinate equality on the device: trimesh's merge_vertices, Open3D's
remove_duplicated_vertices.  An STL-style triangle soup gives every face three vertices of its own; mesh_components then sees one
component per face, mesh_topology nothing closed, and mesh_vertex_adjacency, smooth_mesh and simplify_mesh(duplicate_faces="drop") no
shared edge.  Our own marching-cubes meshes arrive welded; the CAD model usually does not.

include/pb3d.h states the result to the bit: two vertices are one iff their three coordinates compare equal as IEEE numbers in the
input's dtype (so -0.0 == +0.0); a class's representative is its smallest input position; classes are numbered by first appearance
(voxel_downsample(reduce="first")'s numbering with equality classes for voxels); the output rows are the representatives' rows byte
for byte.  Faces keep their order, corner order and dtype, and every index is wrapped and mapped through `inverse`.  Nothing is dropped:
unreferenced vertices are welded like any other, and a face that becomes degenerate or a repeat stays -- compact_mesh removes those.

csrc/weld.hip: one key word per 32 bits of coordinate, one stable radix sort (csrc/sort_pairs.hip) per word -- three for float32, six
for float64 --, run heads, two scans and the gathers.  No hashing, no per-class state, no atomics.  The NumPy form uploads the mesh and
downloads the arrays; the *_resident twin takes and returns device handles (pb3d.device.DeviceBuffer).  There is no CPU fallback."""
import ctypes as C

import numpy as np

from . import _lib, device as dev
from ._args import _cloud, _counts, _faces
from ._lib import _ptr
from .simplify import _channels, _colors

__all__ = ["weld_vertices", "weld_vertices_resident"]


def weld_vertices_resident(d_verts, n_vertices, d_faces=None, n_faces=0, d_colors=None, channels=3, verts_f64=False, faces_i64=False):
    """pb3d_weld_vertices_resident: (d_vertices, d_faces, d_colors, d_index, d_inverse, d_counts, m) -- DeviceBuffers with room for
    n_vertices rows in the input dtype (float32, or float64 with verts_f64), n_faces rows of faces in the input dtype (int32, or int64
    with faces_i64; None without faces), n_vertices x channels colour bytes (None unless d_colors is given), n_vertices int32
    representatives, n_vertices int32 class numbers and n_vertices uint32 class sizes; the first m entries of d_vertices, d_colors,
    d_index and d_counts are written, d_inverse and d_faces whole.  The vertices must be finite.  Host waits: the index check
    (IndexError on a bad face index, nothing written) and m.  The caller frees the buffers."""
    nv, nf = _counts(n_vertices, 0)[0], int(n_faces)
    if not 0 <= 3 * nf <= 2 ** 31 - 1:
        raise ValueError(f"a face list to weld holds at most (2^31 - 1) / 3 faces (got {nf})")
    channels = _channels(channels)
    m = C.c_int64(0)
    with dev.Scope() as sc:
        bufs = [sc.result(None, max(1, nv) * (24 if verts_f64 else 12)),
                sc.result(None, nf * (24 if faces_i64 else 12)) if nf else None,
                sc.result(None, max(1, nv) * channels) if d_colors is not None else None,
                sc.result(None, max(1, nv) * 4), sc.result(None, max(1, nv) * 4), sc.result(None, max(1, nv) * 4)]
        _lib.check(_lib.load().pb3d_weld_vertices_resident(_lib.ctx(), _ptr(d_verts), int(bool(verts_f64)), nv, _ptr(d_faces) if nf else None,
                                                           int(bool(faces_i64)), nf, _ptr(d_colors), channels, *(_ptr(b) for b in bufs), C.byref(m)))
        return (*bufs, int(m.value))


def _narrowed(out, dtype):
    """the mapped faces in the caller's index dtype; they are class numbers, never above the wrapped index they came from"""
    if out.dtype == dtype:
        return out
    if out.size and int(out.max()) > np.iinfo(dtype).max:
        raise OverflowError(f"a welded index ({int(out.max())}) does not fit the faces' dtype {dtype}: it named a vertex from the end of the list")
    return out.astype(dtype)


def weld_vertices(vertices, faces=None, colors=None, return_index=False, return_inverse=False, return_counts=False):
    """The distinct rows of an (n, 3) vertex array in order of first appearance: vertices, or (vertices[, faces][, colors][, index]
    [, inverse][, counts]) when anything else is asked for or given.  Two vertices are one iff their coordinates compare equal in the
    input's dtype -- float32 stays float32, float64 float64, other real dtypes become float64 first -- so -0.0 and +0.0 are one vertex,
    and the row that stays is the first one's, byte for byte.  A NaN or infinity is a ValueError.  faces: an (m, 3) integer array;
    every index is wrapped as NumPy wraps it and replaced by its vertex's output row, in the same order, corner order and dtype, so
    the output holds no negative index; one outside [-n, n) is an IndexError.  Nothing is removed: unreferenced vertices are welded
    like any other, degenerate and repeated faces stay (compact_mesh removes those).  colors: (n, 1 or 3) uint8, each output vertex
    gets the bytes of its first input vertex, unblended.  Extras in np.unique's order: index (int32, the first position of each output
    vertex), inverse (int32, the output row of each input vertex), counts (int64, the class sizes)."""
    v, vf = _cloud(vertices, "vertices")
    n = len(v)
    _counts(n, 0)
    f = fi = ftype = None
    if faces is not None:
        ftype = np.asarray(faces).dtype
        f, fi = _faces(faces, n)
        if n == 0 and len(f):
            raise IndexError(f"index {int(f.reshape(-1)[0])} is out of bounds for axis 0 with size 0")
        if 3 * len(f) > 2 ** 31 - 1:
            raise ValueError(f"a face list to weld holds at most (2^31 - 1) / 3 faces (got {len(f)})")
    if not np.isfinite(v).all():
        raise ValueError("vertices contain NaN or infinity.")
    c = _colors(colors, n)

    def pack(verts, out_faces, cols, index, inverse, counts):
        out = [verts] + ([out_faces] if f is not None else []) + ([cols] if c is not None else [])
        out += [a for a, want in ((index, return_index), (inverse, return_inverse), (counts, return_counts)) if want]
        return tuple(out) if len(out) > 1 else out[0]

    if n == 0:      # nothing needs the device
        return pack(v.copy(), None if f is None else f.astype(ftype), None if c is None else c.copy(), np.zeros(0, np.int32), np.zeros(0, np.int32),
                    np.zeros(0, np.int64))
    nf = 0 if f is None else len(f)
    with dev.Scope() as sc:
        d_c = sc.upload(c) if c is not None else None
        *bufs, m = weld_vertices_resident(sc.upload(v), n, sc.upload(f) if nf else None, nf, d_c, c.shape[1] if c is not None else 3, vf, fi)
        sc.adopt(bufs)
        out_faces = None
        if f is not None:
            out_faces = _narrowed(bufs[1].download((nf, 3), f.dtype) if nf else f.copy(), ftype)
        return pack(bufs[0].download((m, 3), v.dtype), out_faces, bufs[2].download((m, c.shape[1])) if c is not None else None,
                    bufs[3].download((m,), np.int32) if return_index else None, bufs[4].download((n,), np.int32) if return_inverse else None,
                    bufs[5].download((m,), np.uint32).astype(np.int64) if return_counts else None)
