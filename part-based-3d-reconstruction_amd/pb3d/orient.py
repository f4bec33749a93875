"""A consistent winding for a triangle mesh on the device: trimesh's repair.fix_winding / fix_inversion, Open3D's orient_triangles.  A
welded model with mixed winding is "not closed" by mesh_topology's unbalanced edges, its signed volumes are meaningless and vertex
normals taken from its faces cancel.  (voxelize_mesh, points_in_mesh, render_mesh and cast_rays are winding-independent by their rules.)

include/pb3d.h states the result to the bit.  The records and undirected edges are mesh_components' exactly.  A pair edge has two
records; its faces agree iff the records run in opposite directions.  Edges of one or of more than two records connect nothing: no
winding is carried across a non-manifold edge.  A patch is a connected component of the faces under pair edges alone, numbered by its
smallest face; it is orientable iff a flip bit per face exists that makes every pair edge agree.  In an orientable patch the smallest
face keeps its winding; a patch that is not orientable is left exactly as it came and reported.  With volume_sign "positive" or
"negative", every orientable patch without a boundary edge whose ordered signed volume V (mesh_components' sum, over the patch) has the
other sign is complemented as a whole; V == 0 changes nothing.  The rule is per patch: nested shells are not analysed, so a cavity's
shell ends with the same sign as the outer shell.

One fact about our own meshes: in their own frame the shells that meshify_colored_voxel_grid and get_marching_cubes_mesh produce have
NEGATIVE V and their cavities positive (the 4 x 3 x 3 box mask gives -31.666..., a cavity in it +0.666...).  volume_sign="negative"
therefore restores such a mesh's own winding shell by shell, cavities excepted.

A flipped face (a, b, c) becomes (a, c, b): the first corner stays, so anything keyed to it is unaffected.  Index values are copied
as they came, negative ones included, in the input dtype; vertices are not touched.

csrc/orient.hip on csrc/meshcomp.hip's front half: the same two stable sorts of the 3 m records, the same lock-free min-root
union-find (csrc/union_find.h) on a doubled forest -- node j is face j as it came, node m + j face j flipped --, integer atomics for
the counts and none for the floats.  The NumPy forms upload the mesh and download the arrays; the *_resident twins take and return
device handles (pb3d.device.DeviceBuffer).  There is no CPU fallback."""
import ctypes as C

import numpy as np

from . import _lib, device as dev
from ._args import _counts, _mesh
from ._lib import _ptr
from .meshcomp import _face_list, _finite

__all__ = ["mesh_orientation", "mesh_orientation_resident", "orient_mesh", "orient_mesh_resident"]

VOLUME_SIGN = {None: 0, "positive": 1, "negative": 2}
COUNTS = ("faces", "pair_edges", "disagreeing_edges", "boundary_edges", "nonmanifold_records", "flipped_faces")
FLAGS = ("orientable", "inverted")
TOTALS = ("patches", "orientable_patches", "pair_edges", "disagreeing_edges", "flipped_faces", "inverted_patches", "boundary_edges",
          "nonmanifold_edges")


def _volume_sign(volume_sign, have_vertices):
    if not (volume_sign is None or isinstance(volume_sign, str)) or volume_sign not in VOLUME_SIGN:
        raise ValueError(f"volume_sign must be None, 'positive' or 'negative' (got {volume_sign!r})")
    if volume_sign is not None and not have_vertices:
        raise ValueError("volume_sign needs the vertices")
    return VOLUME_SIGN[volume_sign]


def _empty_stats(measured):
    stats = {name: np.zeros(0, np.int64) for name in COUNTS}
    stats.update({name: np.zeros(0, bool) for name in FLAGS})
    if measured:
        stats["volume"] = np.zeros(0, np.float64)
    return stats


def _download_stats(d_counts, d_volume, npatches):
    stats = _empty_stats(d_volume is not None)
    if npatches:
        c = d_counts.download((8, npatches), np.int64)
        stats.update({name: c[a].copy() for a, name in enumerate(COUNTS)})
        stats.update({name: c[len(COUNTS) + a] != 0 for a, name in enumerate(FLAGS)})
        if d_volume is not None:
            stats["volume"] = d_volume.download((npatches,), np.float64)
    return stats


# ---- resident forms ----------------------------------------------------------------------------------------------------------------------
def mesh_orientation_resident(d_faces, n_faces, n_vertices, d_verts=None, volume_sign=None, verts_f64=False, faces_i64=False, out_faces=False):
    """pb3d_mesh_orient_resident: (d_flip, d_patch, d_out_faces, d_counts, d_volume, totals) -- DeviceBuffers of n_faces flip bytes,
    n_faces int32 patch numbers, n_faces face rows in the input dtype (None without out_faces), eight int64 arrays of
    totals["patches"] entries one behind the other (faces, pair, disagreeing and boundary edges, records on edges of more than two,
    flipped faces, orientable, inverted) and, when d_verts is given, as many float64 volumes (else None).  totals: a dict of the eight
    totals.  Host waits: the index check (IndexError on a bad face index, nothing written) and the totals.  The caller frees the
    buffers."""
    nv, nf = _counts(n_vertices, n_faces)
    sign = _volume_sign(volume_sign, d_verts is not None)
    totals = (C.c_int64 * 8)(*([0] * 8))
    with dev.Scope() as sc:
        d_flip = sc.result(None, max(1, nf))
        d_patch = sc.result(None, max(1, nf) * 4)
        d_out = sc.result(None, max(1, nf) * (24 if faces_i64 else 12)) if out_faces else None
        d_counts = sc.result(None, max(1, nf) * 64)
        d_volume = sc.result(None, max(1, nf) * 8) if d_verts is not None else None
        _lib.check(_lib.load().pb3d_mesh_orient_resident(_lib.ctx(), _ptr(d_verts), int(bool(verts_f64)), nv, _ptr(d_faces), int(bool(faces_i64)), nf,
                                                         sign, _ptr(d_flip), _ptr(d_patch), _ptr(d_out), _ptr(d_counts), _ptr(d_volume), totals))
        return d_flip, d_patch, d_out, d_counts, d_volume, {name: int(x) for name, x in zip(TOTALS, totals)}


def orient_mesh_resident(d_verts, n_vertices, d_faces, n_faces, volume_sign=None, verts_f64=False, faces_i64=False):
    """mesh_orientation_resident with the re-wound face list written: the same tuple, d_out_faces never None"""
    return mesh_orientation_resident(d_faces, n_faces, n_vertices, d_verts, volume_sign, verts_f64, faces_i64, out_faces=True)


# ---- NumPy forms ------------------------------------------------------------------------------------------------------------------------
def _run(v, vf, f, fi, n, volume_sign, out_faces):
    """(flip, patch, faces or None, stats, totals) of a checked face list"""
    m = len(f)
    if m == 0:      # nothing needs the device
        return np.zeros(0, np.uint8), np.zeros(0, np.int32), f.copy() if out_faces else None, _empty_stats(v is not None), dict.fromkeys(TOTALS, 0)
    with dev.Scope() as sc:
        d_v = sc.upload(v) if v is not None else None
        *bufs, totals = mesh_orientation_resident(sc.upload(f), m, n, d_v, volume_sign, vf, fi, out_faces)
        sc.adopt(bufs)
        d_flip, d_patch, d_out, d_counts, d_volume = bufs
        return (d_flip.download((m,), np.uint8), d_patch.download((m,), np.int32), d_out.download((m, 3), f.dtype) if out_faces else None,
                _download_stats(d_counts, d_volume, totals["patches"]), totals)


def mesh_orientation(faces, n_vertices=None, vertices=None, volume_sign=None):
    """(flip uint8 (m,), patch int32 (m,), stats, totals) of an (m, 3) integer face array over n vertices (n_vertices, else
    len(vertices), else the largest index + 1): which faces orient_mesh would re-wind, and the patch of every face.  stats is a dict of
    arrays with one entry per patch: int64 faces, pair_edges, disagreeing_edges (of the input), boundary_edges, nonmanifold_records
    (records of the patch's faces on edges of more than two records) and flipped_faces; bool orientable and inverted (complemented
    by the sign rule); float64 volume when vertices ((n, 3), finite) are given -- of the output winding.  totals: patches,
    orientable_patches, pair_edges, disagreeing_edges, flipped_faces, inverted_patches, boundary_edges, nonmanifold_edges.
    volume_sign: None (the smallest face of every patch keeps its winding), or "positive" / "negative" (needs vertices).  Negative
    indices wrap as NumPy's do and one outside [-n, n) is an IndexError."""
    _volume_sign(volume_sign, vertices is not None)
    v, vf, f, fi, n = _face_list(faces, n_vertices, vertices)
    flip, patch, _, stats, totals = _run(v, vf, f, fi, n, volume_sign, False)
    return flip, patch, stats, totals


def orient_mesh(vertices, faces, volume_sign=None, return_flips=False, return_patches=False, return_stats=False):
    """The face array with every orientable patch consistently wound: faces, or (faces[, flip][, patch][, stats, totals]).  Faces keep
    their order, dtype and index values (negative ones included); a re-wound face (a, b, c) comes back as (a, c, b).  volume_sign None:
    the smallest face of each patch keeps its winding.  "positive" / "negative": every orientable patch without a boundary edge ends
    with a signed volume of that sign (or 0); meshify_colored_voxel_grid's and get_marching_cubes_mesh's own shells are "negative".
    Patches that are not orientable (a Moebius band, a projective plane) come back exactly as they came, and stats["orientable"]
    says which.  flip, patch, stats and totals are mesh_orientation's."""
    _volume_sign(volume_sign, True)
    ftype = np.asarray(faces).dtype
    v, vf, f, fi = _mesh(vertices, faces)
    _finite(v)
    flip, patch, out, stats, totals = _run(v, vf, f, fi, len(v), volume_sign, True)
    out = out.astype(ftype, copy=False)       # the values are the caller's own: they fit
    extras = ([flip] if return_flips else []) + ([patch] if return_patches else []) + ([stats, totals] if return_stats else [])
    return (out, *extras) if extras else out
