"""Segmenting a triangle mesh on the device: connected components (Open3D's cluster_connected_triangles, trimesh's split), the edge
counts that say whether a mesh is closed, manifold or watertight, ordered float64 area and signed volume per component, and the
order-keeping selection that turns a face mask into a smaller mesh.  An isosurface of an SfM density volume is one building and a crowd
of floating fragments; render_mesh, sample_mesh_points, point_to_mesh_distances, smooth_mesh and simplify_mesh take the fragments as
given, and voxelize_mesh needs every directed edge to have its reverse -- which mesh_topology's `closed` now checks.

include/pb3d.h states the result to the bit.  Face j gives three directed-edge records; a record with equal ends is a loop and takes
no part.  An undirected edge with c records of which f run from its smaller to its larger vertex is boundary iff c == 1, non-manifold
iff c > 2 and unbalanced iff 2 f != c.  connectivity="edge" (the default) connects two faces that have a record on one undirected edge,
"vertex" two faces that name a common vertex.  Components are numbered by their smallest face position.  Area and volume are sums in a
fixed order: a component's faces in blocks of 256, the blocks in order.

csrc/meshcomp.hip: two stable radix sorts of the 3 m records (csrc/sort_pairs.hip), flags and scans for the runs, a lock-free union-find
whose roots are minima (csrc/union_find.h), integer atomics for the counts and none for the floats.  select_faces is compact_mesh's
face tail (csrc/simplify.hip) with the caller's flags.  The NumPy forms upload the mesh and download the arrays; the *_resident twins
take and return device handles (pb3d.device.DeviceBuffer).  There is no CPU fallback."""
import ctypes as C
import math

import numpy as np

from . import _lib, device as dev
from ._args import _cloud, _counts, _faces, _mesh
from ._lib import _ptr
from .simplify import _channels, _colors, _numpy_form, _resident

__all__ = ["mesh_components", "mesh_components_resident", "mesh_topology", "mesh_topology_resident", "select_faces", "select_faces_resident",
           "keep_mesh_components", "keep_mesh_components_resident"]

CONNECTIVITY = {"edge": 0, "vertex": 1}
COUNTS = ("faces", "edges", "boundary_edges", "nonmanifold_edges", "unbalanced_edges")
MEASURES = ("area", "volume")
TOTALS = ("components", "vertices", "edges", "faces", "boundary_edges", "nonmanifold_edges", "unbalanced_edges", "loops")
RANK_BY = ("faces", "area", "volume")


def _connectivity(connectivity):
    if not isinstance(connectivity, str) or connectivity not in CONNECTIVITY:
        raise ValueError(f"connectivity must be 'edge' or 'vertex' (got {connectivity!r})")
    return CONNECTIVITY[connectivity]


def _rank_by(rank_by):
    if not isinstance(rank_by, str) or rank_by not in RANK_BY:
        raise ValueError(f"rank_by must be 'faces', 'area' or 'volume' (got {rank_by!r})")
    return rank_by


def _whole(v, name, least):
    if v is None:
        return None
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < least:
        raise ValueError(f"{name} must be an integer >= {least} (got {v!r})")
    return int(v)


def _min_area(min_area):
    if min_area is None:
        return None
    a = float(min_area)
    if not math.isfinite(a) or a < 0.0:
        raise ValueError(f"min_area must be finite and >= 0 (got {min_area!r})")
    return a


def _keep_flags(keep, m):
    k = np.asarray(keep)
    if k.shape != (m,) or k.dtype.kind not in "biu":
        raise ValueError(f"keep must be a boolean or integer array of shape ({m},) (got shape {k.shape}, dtype {k.dtype})")
    return _lib.truth_u8(k)


def _finite(v):
    if not np.isfinite(v).all():
        raise ValueError("vertices contain NaN or infinity.")


def _totals(t):
    """the dict of the eight totals, the Euler characteristic and the three flags"""
    out = {name: int(x) for name, x in zip(TOTALS, t)}
    out["euler"] = out["vertices"] - out["edges"] + out["faces"]
    out["closed"] = out["unbalanced_edges"] == 0
    out["edge_manifold"] = out["nonmanifold_edges"] == 0
    out["watertight"] = out["closed"] and out["edge_manifold"] and out["boundary_edges"] == 0
    return out


def _empty_stats(measured):
    stats = {name: np.zeros(0, np.int64) for name in COUNTS}
    if measured:
        stats.update({name: np.zeros(0, np.float64) for name in MEASURES})
    return stats


# ---- resident forms ----------------------------------------------------------------------------------------------------------------------
def mesh_components_resident(d_faces, n_faces, n_vertices, d_verts=None, connectivity="edge", verts_f64=False, faces_i64=False,
                             vertex_labels=True, counts=True):
    """pb3d_mesh_components_resident: (d_face_labels, d_vertex_labels, d_counts, d_measures, totals) -- DeviceBuffers of n_faces int32
    labels, n_vertices int32 labels (-1: no face names the vertex; None without vertex_labels), five int64 arrays of totals["components"]
    entries one behind the other (faces, edges, boundary, non-manifold and unbalanced edges per component; None without counts) and,
    when d_verts is given, two float64 arrays of as many (area, volume; else None).  totals: mesh_topology's dict.  Host waits: the index
    check (IndexError on a bad face index, nothing written) and the totals.  The caller frees the buffers."""
    nv, nf = _counts(n_vertices, n_faces)
    conn = _connectivity(connectivity)
    totals = (C.c_int64 * 8)(*([0] * 8))
    with dev.Scope() as sc:
        d_lab = sc.result(None, max(1, nf) * 4)
        d_vlab = sc.result(None, max(1, nv) * 4) if vertex_labels else None
        d_counts = sc.result(None, max(1, nf) * 40) if counts else None
        d_meas = sc.result(None, max(1, nf) * 16) if d_verts is not None else None
        _lib.check(_lib.load().pb3d_mesh_components_resident(_lib.ctx(), _ptr(d_verts), int(bool(verts_f64)), nv, _ptr(d_faces), int(bool(faces_i64)),
                                                             nf, conn, _ptr(d_lab), _ptr(d_vlab), _ptr(d_counts), _ptr(d_meas), totals))
        return d_lab, d_vlab, d_counts, d_meas, _totals(totals)


def mesh_topology_resident(d_faces, n_faces, n_vertices, faces_i64=False):
    """mesh_topology of a resident face list: the totals of pb3d_mesh_components_resident alone (edge connectivity)"""
    with dev.Scope() as sc:
        d_lab, _, _, _, totals = mesh_components_resident(d_faces, n_faces, n_vertices, faces_i64=faces_i64, vertex_labels=False, counts=False)
        sc.adopt(d_lab)
        return totals


def select_faces_resident(d_verts, n_vertices, d_faces, n_faces, d_keep, d_colors=None, channels=3, verts_f64=False, faces_i64=False):
    """pb3d_mesh_select_faces_resident: compact_mesh_resident's tuple for the faces whose byte in d_keep (n_faces bytes) is not 0 --
    (d_vertices, d_faces, d_colors, d_index, d_inverse, d_face_index, (n, m)).  Host waits: the index check and (n, m)."""
    nv, nf = _counts(n_vertices, n_faces)
    channels = _channels(channels)
    lib, ctx = _lib.load(), _lib.ctx()
    return _resident(lambda *out: lib.pb3d_mesh_select_faces_resident(ctx, _ptr(d_verts), int(bool(verts_f64)), nv, _ptr(d_faces), int(bool(faces_i64)),
                                                                      nf, _ptr(d_keep), _ptr(d_colors), channels, *out),
                     nv, nf, d_colors, channels, verts_f64, faces_i64)


def _download_stats(d_counts, d_meas, nc):
    stats = _empty_stats(d_meas is not None)
    if nc:
        c = d_counts.download((5, nc), np.int64)
        stats.update({name: c[a].copy() for a, name in enumerate(COUNTS)})
        if d_meas is not None:
            f = d_meas.download((2, nc), np.float64)
            stats.update({name: f[a].copy() for a, name in enumerate(MEASURES)})
    return stats


def _choose(stats, k, min_faces, min_area, closed_only, rank_by):
    """the components that stay: the thresholds first, then the k largest by rank_by (volume by absolute value), ties to the lower
    number; all that pass when k exceeds their number or is None"""
    ok = np.ones(len(stats["faces"]), bool)
    if min_faces is not None:
        ok &= stats["faces"] >= min_faces
    if min_area is not None:
        ok &= stats["area"] >= min_area
    if closed_only:
        ok &= stats["unbalanced_edges"] == 0
    cand = np.flatnonzero(ok)
    if k is not None:
        score = np.abs(stats[rank_by][cand])
        cand = np.sort(cand[np.lexsort((cand, -score))[:k]])
    return cand.astype(np.intp)


def _keep_args(k, min_faces, min_area, closed_only, rank_by, connectivity):
    _connectivity(connectivity)
    return _whole(k, "k", 1), _whole(min_faces, "min_faces", 0), _min_area(min_area), bool(closed_only), _rank_by(rank_by)


def keep_mesh_components_resident(d_verts, n_vertices, d_faces, n_faces, k=None, min_faces=None, min_area=None, closed_only=False, rank_by="faces",
                                  connectivity="edge", d_colors=None, channels=3, verts_f64=False, faces_i64=False):
    """mesh_components_resident, the choice made on the host from the downloaded stats, pb3d_labels_member_resident on the face labels
    and select_faces_resident on its flags: (select_faces_resident's tuple, d_face_labels, chosen component numbers).  The mesh stays
    where it is; the stats and the counts are all that leaves the device.  The caller frees the buffers."""
    nv, nf = _counts(n_vertices, n_faces)
    k, min_faces, min_area, closed_only, rank_by = _keep_args(k, min_faces, min_area, closed_only, rank_by, connectivity)
    measured = min_area is not None or (k is not None and rank_by != "faces")
    with dev.Scope() as sc:
        d_lab, _, d_counts, d_meas, totals = mesh_components_resident(d_faces, nf, nv, d_verts if measured else None, connectivity, verts_f64,
                                                                      faces_i64, vertex_labels=False)
        sc.adopt((d_lab, d_counts, d_meas))
        nc = totals["components"]
        chosen = _choose(_download_stats(d_counts, d_meas, nc), k, min_faces, min_area, closed_only, rank_by)
        table = np.zeros(max(1, nc), np.uint8)
        table[chosen] = 1
        d_keep = sc.alloc(max(1, nf))
        _lib.check(_lib.load().pb3d_labels_member_resident(_lib.ctx(), _ptr(d_lab), nf, _lib.p_u8(table), nc, _ptr(d_keep)))
        out = select_faces_resident(d_verts, nv, d_faces, nf, d_keep, d_colors, channels, verts_f64, faces_i64)
        return out, sc.keep(d_lab), chosen


# ---- NumPy forms ------------------------------------------------------------------------------------------------------------------------
def _face_list(faces, n_vertices, vertices):
    """(vertices or None, f64 flag, faces, i64 flag, n)"""
    if vertices is not None:
        v, vf, f, fi = _mesh(vertices, faces)
        if n_vertices is not None and int(n_vertices) != len(v):
            raise ValueError(f"n_vertices is {n_vertices!r} but vertices has {len(v)} rows")
        _finite(v)
        return v, vf, f, fi, len(v)
    if n_vertices is None:
        a = np.asarray(faces)
        n_vertices = int(a.max()) + 1 if a.size and a.dtype.kind in "iu" else 0
    n = _counts(n_vertices, 0)[0]
    f, fi = _faces(faces, n)
    if n == 0 and len(f):
        raise IndexError(f"index {int(f.reshape(-1)[0])} is out of bounds for axis 0 with size 0")
    return None, 0, f, fi, n


def mesh_components(faces, n_vertices=None, vertices=None, connectivity="edge", return_vertex_labels=False):
    """(face_labels int32 (m,), stats[, vertex_labels int32 (n,)]) of an (m, 3) integer face array over n vertices (n_vertices, else
    len(vertices), else the largest index + 1).  stats is a dict of arrays with one entry per component: int64 faces, edges,
    boundary_edges, nonmanifold_edges, unbalanced_edges and, when vertices ((n, 3), finite) are given, float64 area and volume.
    int32 faces stay int32, other integer types become int64; negative indices wrap as NumPy's do and one outside [-n, n) is an
    IndexError.  vertex_labels: the smallest label among the faces naming the vertex, -1 for an unreferenced one."""
    _connectivity(connectivity)
    v, vf, f, fi, n = _face_list(faces, n_vertices, vertices)
    m = len(f)
    if m == 0:      # nothing needs the device
        out = (np.zeros(0, np.int32), _empty_stats(v is not None))
        return out + (np.full(n, -1, np.int32),) if return_vertex_labels else out
    with dev.Scope() as sc:
        d_v = sc.upload(v) if v is not None else None
        bufs = mesh_components_resident(sc.upload(f), m, n, d_v, connectivity, vf, fi, vertex_labels=return_vertex_labels)
        d_lab, d_vlab, d_counts, d_meas, totals = bufs
        sc.adopt(bufs[:4])
        out = (d_lab.download((m,), np.int32), _download_stats(d_counts, d_meas, totals["components"]))
        return out + (d_vlab.download((n,), np.int32),) if return_vertex_labels else out


def mesh_topology(faces, n_vertices):
    """The totals of a face list as a dict: components (edge connectivity), vertices (those a face names), edges, faces,
    boundary_edges, nonmanifold_edges, unbalanced_edges, loops; euler = vertices - edges + faces; closed = no unbalanced edge (every
    directed edge has its reverse: what voxelize_mesh needs), edge_manifold = no edge of more than two faces, watertight = closed and
    edge_manifold and no boundary edge."""
    _, _, f, fi, n = _face_list(faces, n_vertices, None)
    if len(f) == 0:
        return _totals([0] * 8)
    with dev.Scope() as sc:
        return mesh_topology_resident(sc.upload(f), len(f), n, fi)


def select_faces(vertices, faces, keep, colors=None, return_index=False, return_inverse=False, return_face_index=False):
    """compact_mesh with the caller's choice of faces: (vertices, faces[, colors][, index][, inverse][, face_index]).  The faces with a
    non-zero `keep` (one boolean or integer per face) stay, in order and in corner order -- degenerate and repeated faces too, nothing
    is deduplicated; the vertices no kept face names go, the rest are renumbered in order and copied byte for byte."""
    v, vf, f, fi = _mesh(vertices, faces)
    flags = _keep_flags(keep, len(f))
    c = _colors(colors, len(v))

    def resident(d_v, nv, d_f, nf, d_c, ch):
        with dev.Scope() as sc:
            return select_faces_resident(d_v, nv, d_f, nf, sc.upload(flags), d_c, ch, vf, fi)

    return _numpy_form(resident, v, f, c, (return_index, return_inverse, return_face_index))


def keep_mesh_components(vertices, faces, k=None, min_faces=None, min_area=None, closed_only=False, rank_by="faces", connectivity="edge",
                         colors=None, return_labels=False):
    """The mesh of the chosen components: (vertices, faces[, colors][, face_labels, chosen]).  Of the components of mesh_components the
    ones with at least min_faces faces, at least min_area area and (closed_only) no unbalanced edge pass; of those the k largest by
    rank_by ("faces", "area", or "volume" by absolute value) stay, ties going to the lower component number; all that pass when k is
    None or exceeds their number.  The rest is select_faces.  return_labels: the int32 label of every input face and the chosen
    component numbers (intp) as well."""
    k, min_faces, min_area, closed_only, rank_by = _keep_args(k, min_faces, min_area, closed_only, rank_by, connectivity)
    v, vf, f, fi = _mesh(vertices, faces)
    _finite(v)
    c = _colors(colors, len(v))
    nv, nf = len(v), len(f)

    def pack(verts, out_faces, cols, labels, chosen):
        out = [verts, out_faces] + ([cols] if c is not None else [])
        return tuple(out + ([labels, chosen] if return_labels else []))

    if nf == 0:     # nothing stays, and nothing needs the device
        return pack(v[:0].copy(), f[:0].copy(), None if c is None else c[:0].copy(), np.zeros(0, np.int32), np.zeros(0, np.intp))
    with dev.Scope() as sc:
        d_c = sc.upload(c) if c is not None else None
        (*bufs, (n, m)), d_lab, chosen = keep_mesh_components_resident(sc.upload(v), nv, sc.upload(f), nf, k, min_faces, min_area, closed_only,
                                                                       rank_by, connectivity, d_c, c.shape[1] if c is not None else 3, vf, fi)
        sc.adopt(bufs)
        sc.adopt(d_lab)
        return pack(bufs[0].download((n, 3), v.dtype), bufs[1].download((m, 3), f.dtype),
                    bufs[2].download((n, c.shape[1])) if c is not None else None,
                    d_lab.download((nf,), np.int32) if return_labels else None, chosen)
