"""Containment: which points of a cloud lie inside a triangle mesh, on the device -- and with it signed point-to-mesh distances and
a mesh as a selector for a cloud.  point_to_mesh_distances says how far a point is from the surface; this says on which side.  The
fraction of an SfM cloud outside the mesh of a carved hull measures carving too much; a part's mesh (keep_mesh_components,
select_faces, a per-part meshify) picks the part's points out of a cloud where crop_to_box could only cut a box.

include/pb3d.h states the result to the bit, and it is voxelize_mesh's rule at arbitrary query points: a ray along the last axis
through the query is crossed by the faces whose projection holds (q0, q1), ties on edges and vertices decided by the same symbolic
rule (the query moved by the infinitesimal (-eps^2, +eps)), and the query is inside when the number of crossings at or below it is
odd.  No frame, origin or voxel size is applied.  All arithmetic is float64, one rounded operation each.  points_in_mesh at the
lattice points of a grid equals voxelize_mesh of that grid byte for byte.  An odd number of crossings over a query (`total`) means
the mesh is open there; the answer is still exactly the stated function of the input, and for open or self-intersecting meshes
nothing more is claimed.

csrc/inside.hip: a 2-D cell index of the faces, one lane per query walking the list of its one cell, no atomics on the query side
-- the result is a function of the input alone.  The NumPy forms upload cloud and mesh and download the arrays; the *_resident twins
take and return device handles (pb3d.device.DeviceBuffer)."""
import ctypes as C

import numpy as np

from . import _lib, device as dev
from ._args import _cloud, _count, _counts, _finite_cloud, _mesh
from ._lib import _ptr
from .cluster import _download_selection, select_points_resident
from .eval_helpers import point_to_mesh_distances_resident

__all__ = ["points_in_mesh", "points_in_mesh_resident", "points_in_mesh_last", "signed_point_to_mesh_distances",
           "signed_point_to_mesh_distances_resident", "select_points_in_mesh", "select_points_in_mesh_resident"]

STATS = ("inside", "odd_totals", "flat_faces", "outside_box")


def _finite_mesh(vertices, faces, what):
    """_mesh of a mesh that a distance can be measured to: at least one face, finite vertices"""
    v, vf, f, fi = _mesh(vertices, faces)
    if len(f) == 0:
        raise ValueError(f"{what}: the mesh has no faces")
    if not np.isfinite(v).all():
        raise ValueError("Input vertices contains NaN or infinity.")
    return v, vf, f, fi


# ---- resident forms ----------------------------------------------------------------------------------------------------------------------
def points_in_mesh_resident(d_P, nP, d_verts, n_vertices, d_faces, n_faces, p_f64=True, verts_f64=False, faces_i64=False,
                            return_counts=False, return_stats=False, out=None, counts_out=None):
    """pb3d_points_in_mesh_resident: a DeviceBuffer of nP bytes (1 = inside) for the resident (nP, 3) list d_P (float64 rows, or float32
    with p_f64 False) against the resident mesh; with return_counts also a DeviceBuffer of nP x 2 int32 (crossings at or below the query,
    crossings over it), with return_stats also the dict of inside, odd_totals, flat_faces and outside_box, in that order.  `out` and
    `counts_out` are written instead of new buffers when given, and are untouched when the call fails.  A query with a NaN coordinate
    is outside with zero counts.  Host waits: the check of the face indices (IndexError) and of the vertices (ValueError on one that is
    not finite), the vertices' box, one per count of the index's entries (1 + its halvings), and one more for the stats; the query
    itself is enqueued."""
    nP = _count(nP)
    nv, nf = _counts(n_vertices, n_faces)
    stats = (C.c_int64 * 4)() if return_stats else None
    with dev.Scope() as sc:
        d_out = sc.result(out, max(1, nP))
        d_cnt = sc.result(counts_out, max(1, nP) * 8) if return_counts else None
        _lib.check(_lib.load().pb3d_points_in_mesh_resident(_lib.ctx(), _ptr(d_P), int(bool(p_f64)), nP, _ptr(d_verts), int(bool(verts_f64)), nv,
                                                            _ptr(d_faces), int(bool(faces_i64)), nf, _ptr(d_out), _ptr(d_cnt), stats))
        res = (d_out,) + ((d_cnt,) if return_counts else ()) + ((dict(zip(STATS, (int(v) for v in stats))),) if return_stats else ())
        return res if len(res) > 1 else d_out


def points_in_mesh_last(timed=False):
    """pb3d_points_in_mesh_last: ((cells along a0, cells along a1), entries, halvings) of the index the last containment test built;
    with timed=True also (index ms, query ms) of that call, which must have run under knob "inside_timing" """
    info, ms = (C.c_int64 * 4)(), (C.c_double * 2)()
    _lib.check(_lib.load().pb3d_points_in_mesh_last(_lib.ctx(), info, ms if timed else None))
    res = ((int(info[0]), int(info[1])), int(info[2]), int(info[3]))
    return res + ((float(ms[0]), float(ms[1])),) if timed else res


def signed_point_to_mesh_distances_resident(d_P, nP, d_verts, n_vertices, d_faces, n_faces, p_f64=True, verts_f64=False, faces_i64=False,
                                            return_faces=False, return_closest=False, return_inside=False):
    """(DeviceBuffer of nP float64 signed distances, nearest faces or None, closest points or None, inside bytes or None):
    point_to_mesh_distances_resident, points_in_mesh_resident and pb3d_mesh_dist_sign_resident on the same resident cloud and mesh
    -- negative inside, a point on the surface keeps +0.0.  Points and vertices must be finite, the mesh needs a face.  Host waits:
    those of the two entries; the sign pass is enqueued."""
    nP = _count(nP)
    with dev.Scope() as sc:
        d_dist, d_face, d_closest = sc.adopt(point_to_mesh_distances_resident(d_P, nP, d_verts, n_vertices, d_faces, n_faces, p_f64, verts_f64,
                                                                              faces_i64, return_faces, return_closest))
        d_in = sc.adopt(points_in_mesh_resident(d_P, nP, d_verts, n_vertices, d_faces, n_faces, p_f64, verts_f64, faces_i64))
        _lib.check(_lib.load().pb3d_mesh_dist_sign_resident(_lib.ctx(), _ptr(d_dist), _ptr(d_in), nP, _ptr(d_dist)))
        for b in (d_dist, d_face, d_closest) + ((d_in,) if return_inside else ()):      # they outlive the scope; on a failure it frees them
            if b is not None:
                sc.keep(b)
        return d_dist, d_face, d_closest, (d_in if return_inside else None)


def select_points_in_mesh_resident(d_P, nP, d_verts, n_vertices, d_faces, n_faces, invert=False, p_f64=True, verts_f64=False,
                                   faces_i64=False, out=None, index=None):
    """(d_out, d_idx, count) of select_points_resident on the containment bytes: the rows of the resident cloud inside the mesh (outside
    it with invert), in their order and dtype, and their positions.  The cloud never leaves the device; the count is downloaded."""
    nP = _count(nP)
    with dev.Scope() as sc:
        d_keep = sc.adopt(points_in_mesh_resident(d_P, nP, d_verts, n_vertices, d_faces, n_faces, p_f64, verts_f64, faces_i64))
        if invert:
            _lib.check(_lib.load().pb3d_flags_not_resident(_lib.ctx(), _ptr(d_keep), nP, _ptr(d_keep)))
        return select_points_resident(d_P, nP, d_keep, p_f64, out, index)


# ---- NumPy forms ------------------------------------------------------------------------------------------------------------------------
def points_in_mesh(P, vertices, faces, return_counts=False):
    """bool (len(P),): which points of the (n, 3) cloud P lie inside the mesh of an (nv, 3) vertex array and an (m, 3) integer face
    array, by the crossing parity include/pb3d.h states.  float32 clouds and vertices stay float32 (the arithmetic is float64), other
    real dtypes become float64; int32 faces stay int32, other integer types become int64; negative face indices wrap as NumPy's do and
    one outside [-nv, nv) is an IndexError.  Points and vertices must be finite (ValueError).  With return_counts also an (n, 2) int32
    array: the crossings at or below each point and the crossings over it -- the first decides, an odd second says the mesh is open
    over that point.  No faces: nothing is inside."""
    p, pf = _finite_cloud(P)
    v, vf, f, fi = _mesh(vertices, faces)
    n = len(p)
    if n == 0:
        return (np.zeros(0, bool), np.zeros((0, 2), np.int32)) if return_counts else np.zeros(0, bool)
    with dev.Scope() as sc:
        res = points_in_mesh_resident(sc.upload(p), n, sc.upload(v), len(v), sc.upload(f), len(f), pf, vf, fi, return_counts)
        d_in, d_cnt = sc.adopt(res) if return_counts else (sc.adopt(res), None)
        inside = d_in.download((n,), np.uint8) != 0
        return (inside, d_cnt.download((n, 2), np.int32)) if return_counts else inside


def signed_point_to_mesh_distances(P, vertices, faces, return_faces=False, return_closest=False, return_inside=False):
    """float64 (len(P),): point_to_mesh_distances with the sign of points_in_mesh -- negative inside the mesh, positive outside, and a
    point on the surface keeps +0.0: np.where(inside & (d > 0), -d, d), the mesh uploaded once.  With return_faces also the int32
    nearest face of each point, with return_closest the (n, 3) float64 closest points, with return_inside the bool flags, in that
    order.  The sign means what points_in_mesh means: for a closed mesh inside and outside, for an open one the stated parity."""
    p, pf = _cloud(P, "P")
    if not np.isfinite(p).all():
        raise ValueError("Input P contains NaN or infinity.")
    n = len(p)
    if n == 0:
        out = (np.zeros(0, np.float64),) + ((np.zeros(0, np.int32),) if return_faces else ()) + \
            ((np.zeros((0, 3), np.float64),) if return_closest else ()) + ((np.zeros(0, bool),) if return_inside else ())
        return out if len(out) > 1 else out[0]
    v, vf, f, fi = _finite_mesh(vertices, faces, "signed_point_to_mesh_distances")
    with dev.Scope() as sc:
        d_dist, d_face, d_closest, d_in = sc.adopt(signed_point_to_mesh_distances_resident(
            sc.upload(p), n, sc.upload(v), len(v), sc.upload(f), len(f), pf, vf, fi, return_faces, return_closest, return_inside))
        res = [d_dist.download((n,), np.float64)]
        if return_faces:
            res.append(d_face.download((n,), np.int32))
        if return_closest:
            res.append(d_closest.download((n, 3), np.float64))
        if return_inside:
            res.append(d_in.download((n,), np.uint8) != 0)
        return tuple(res) if len(res) > 1 else res[0]


def select_points_in_mesh(P, vertices, faces, invert=False, return_index=False):
    """P[points_in_mesh(P, vertices, faces)] -- with invert the points outside -- compacted on the device in input order; with
    return_index also their positions, np.flatnonzero of the flags.  The cloud is uploaded once and only the selection comes back."""
    p, pf = _finite_cloud(P)
    v, vf, f, fi = _mesh(vertices, faces)
    n = len(p)
    if n == 0:
        return (p.copy(), np.zeros(0, np.intp)) if return_index else p.copy()
    with dev.Scope() as sc:
        d_out, d_idx, count = select_points_in_mesh_resident(sc.upload(p), n, sc.upload(v), len(v), sc.upload(f), len(f), invert, pf, vf, fi)
        sc.adopt((d_out, d_idx))
        out, idx = _download_selection(d_out, d_idx, count, p.dtype)
        return (out, idx) if return_index else out
