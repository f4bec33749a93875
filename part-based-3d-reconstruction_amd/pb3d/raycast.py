"""Rays against a mesh: what does this ray hit first?  render_mesh casts the rays of one pinhole camera and points_in_mesh rays along
one axis; this casts the rays the caller chooses -- the segment from a point to an eye (occlusion per point, not per pixel), a surface's
normals (distance along the normal, thickness), a bundle of parallel rays (orthographic depths and silhouettes: cast, then reshape).

include/pb3d.h states the result to the bit.  A ray o + t d is tested against a face by the signs of three edge values of the face's
corners sheared along the ray's dominant axis (Woop, Benthin and Wald 2013, all in float64, one rounded operation each): a ray cannot
pass between two faces that share an edge, and nothing is culled by orientation.  A ray takes the hit with the smallest (t, face
number) among those with t_min <= t <= t_max; t is in units of |d|.  With the rays of an unrotated camera the result equals
render_mesh's depth and face images bit for bit.

csrc/raycast.hip: the 3-axis cell index of the faces, one lane per ray walking the layers of cells along the ray's dominant axis, no
atomics -- the result is a function of the input alone.  The NumPy forms upload rays and mesh and download the arrays; the *_resident
twins take and return device handles (pb3d.device.DeviceBuffer)."""
import ctypes as C
import math

import numpy as np

from . import _lib, device as dev
from ._args import _cloud, _count, _counts, _mesh
from ._lib import _ptr

__all__ = ["cast_rays", "cast_rays_resident", "rays_occluded", "rays_occluded_resident", "points_visible_from", "camera_rays",
           "cast_rays_last"]

STATS = ("hits", "bad_rays", "outside_box", "face_tests", "cells", "entries")


def _range(t_min, t_max):
    t_min, t_max = float(t_min), float(t_max)
    if not math.isfinite(t_min) or math.isnan(t_max) or not t_min <= t_max:
        raise ValueError(f"need t_min finite and t_min <= t_max (got {t_min!r}, {t_max!r})")
    return t_min, t_max


def _rays(origins, directions):
    """(origins, directions, f64 flag): two (n, 3) arrays of one float width -- float32 only when both are"""
    o, of = _cloud(origins, "origins")
    d, df = _cloud(directions, "directions")
    if o.shape != d.shape:
        raise ValueError(f"origins and directions must have one shape (got {o.shape} and {d.shape})")
    _count(len(o))
    if of != df:
        o, d = np.ascontiguousarray(o, dtype=np.float64), np.ascontiguousarray(d, dtype=np.float64)
    return o, d, int(of and df)


# ---- resident forms ----------------------------------------------------------------------------------------------------------------------
def cast_rays_resident(d_origins, d_directions, n_rays, d_verts, n_vertices, d_faces, n_faces, t_min=0.0, t_max=np.inf, return_bary=False,
                       rays_f64=True, verts_f64=False, faces_i64=False, t_out=None, face_out=None, bary_out=None):
    """pb3d_cast_rays_resident, first-hit mode: (d_t, d_face[, d_bary]) -- DeviceBuffers of n_rays float64 (+inf: no hit), n_rays int32
    (-1: no hit) and, with return_bary, n_rays x 3 float64 -- for the resident (n_rays, 3) origins and directions (float64 rows, or
    float32 with rays_f64 False) against the resident mesh.  The *_out buffers are written instead of new ones when given, and are
    untouched when the call fails.  Host waits: the check of the face indices (IndexError) and of the vertices (ValueError on one that
    is not finite), the vertices' box, one per count of the index's entries (1 + its halvings); the query itself is enqueued."""
    n = _count(n_rays)
    nv, nf = _counts(n_vertices, n_faces)
    t_min, t_max = _range(t_min, t_max)
    with dev.Scope() as sc:
        d_t, d_face = sc.result(t_out, max(1, n) * 8), sc.result(face_out, max(1, n) * 4)
        d_bary = sc.result(bary_out, max(1, n) * 24) if return_bary else None
        _lib.check(_lib.load().pb3d_cast_rays_resident(_lib.ctx(), _ptr(d_origins), _ptr(d_directions), int(bool(rays_f64)), n, _ptr(d_verts),
                                                       int(bool(verts_f64)), nv, _ptr(d_faces), int(bool(faces_i64)), nf, t_min, t_max, 0,
                                                       _ptr(d_t), _ptr(d_face), _ptr(d_bary), None))
        return (d_t, d_face, d_bary) if return_bary else (d_t, d_face)


def rays_occluded_resident(d_origins, d_directions, n_rays, d_verts, n_vertices, d_faces, n_faces, t_min=0.0, t_max=np.inf, rays_f64=True,
                           verts_f64=False, faces_i64=False, out=None):
    """pb3d_cast_rays_resident, any-hit mode: a DeviceBuffer of n_rays bytes, 1 where some face hits on [t_min, t_max] -- the bytes of
    face >= 0 of cast_rays_resident, found by a walk that stops at the first hit it meets.  Host waits as there."""
    n = _count(n_rays)
    nv, nf = _counts(n_vertices, n_faces)
    t_min, t_max = _range(t_min, t_max)
    with dev.Scope() as sc:
        d_hit = sc.result(out, max(1, n))
        _lib.check(_lib.load().pb3d_cast_rays_resident(_lib.ctx(), _ptr(d_origins), _ptr(d_directions), int(bool(rays_f64)), n, _ptr(d_verts),
                                                       int(bool(verts_f64)), nv, _ptr(d_faces), int(bool(faces_i64)), nf, t_min, t_max, 1,
                                                       None, None, None, _ptr(d_hit)))
        return d_hit


def cast_rays_last(timed=False):
    """pb3d_cast_rays_last: the dict of hits, bad_rays, outside_box (rays that visit no cell), face_tests, cells and entries (of the
    index) of the context's last ray cast, which must have run under knob "raycast_stats"; with timed=True (index ms, query ms) of
    that call instead, which must have run under knob "raycast_timing" """
    if timed:
        ms = (C.c_double * 2)()
        _lib.check(_lib.load().pb3d_cast_rays_last_ms(_lib.ctx(), ms))
        return float(ms[0]), float(ms[1])
    s = (C.c_int64 * 6)()
    _lib.check(_lib.load().pb3d_cast_rays_last(_lib.ctx(), s))
    return dict(zip(STATS, (int(v) for v in s)))


# ---- NumPy forms ------------------------------------------------------------------------------------------------------------------------
def cast_rays(origins, directions, vertices, faces, t_min=0.0, t_max=np.inf, return_bary=False):
    """(t, face[, bary]) of the first hit of each ray origins[r] + t * directions[r] on the mesh of an (nv, 3) vertex array and an
    (m, 3) integer face array, among the hits with t_min <= t <= t_max: t float64 (n,), +inf where nothing hits and otherwise in units
    of |directions[r]|; face int32 (n,), the smaller number among faces hit at the same t, -1 for none; with return_bary the (n, 3)
    float64 weights of the hit face's corners, zeros for none.  Both windings are hit.  A ray with a component that is not finite, or
    with a zero direction, hits nothing.  float32 rays (both arrays) and vertices stay float32 -- the arithmetic is float64 -- other
    real dtypes become float64; int32 faces stay int32; negative face indices wrap as NumPy's do and one outside [-nv, nv) is an
    IndexError; a vertex that is not finite is a ValueError.  No faces: nothing is hit."""
    o, d, rf = _rays(origins, directions)
    v, vf, f, fi = _mesh(vertices, faces)
    t_min, t_max = _range(t_min, t_max)
    n = len(o)
    with dev.Scope() as sc:
        res = sc.adopt(cast_rays_resident(sc.upload(o), sc.upload(d), n, sc.upload(v), len(v), sc.upload(f), len(f), t_min, t_max,
                                          return_bary, rf, vf, fi))
        if n == 0:          # (the mesh has been checked)
            return (np.zeros(0, np.float64), np.zeros(0, np.int32)) + ((np.zeros((0, 3), np.float64),) if return_bary else ())
        out = (res[0].download((n,), np.float64), res[1].download((n,), np.int32))
        return out + (res[2].download((n, 3), np.float64),) if return_bary else out


def rays_occluded(origins, directions, vertices, faces, t_min=0.0, t_max=np.inf):
    """bool (n,): whether ray r hits any face on [t_min, t_max] -- cast_rays(...)[1] >= 0, by a walk that stops at the first hit it
    meets.  With t_max = 1 the ray is the segment from origins[r] to origins[r] + directions[r]."""
    o, d, rf = _rays(origins, directions)
    v, vf, f, fi = _mesh(vertices, faces)
    t_min, t_max = _range(t_min, t_max)
    n = len(o)
    with dev.Scope() as sc:
        d_hit = sc.adopt(rays_occluded_resident(sc.upload(o), sc.upload(d), n, sc.upload(v), len(v), sc.upload(f), len(f), t_min, t_max, rf, vf, fi))
        return d_hit.download((n,), np.uint8) != 0 if n else np.zeros(0, bool)


def points_visible_from(points, eye, vertices, faces, t_min):
    """bool (n,): point p is visible from `eye` iff no face hits the segment p + t (eye - p) on [t_min, 1].  eye - p is taken on the host
    in float64 and both ray arrays go up as float64.  t_min is the fraction of the segment skipped at the point and has no default: a
    point ON the mesh (a vertex, a sample of the surface) hits its own faces at t = 0, and how far to step off them is the caller's
    decision, not a constant of the library."""
    p, _ = _cloud(points, "points")
    e = np.array(eye, dtype=np.float64)
    if e.shape != (3,):
        raise ValueError(f"eye must be three numbers (got {eye!r})")
    t_min, _ = _range(t_min, 1.0)
    p = np.ascontiguousarray(p, dtype=np.float64)
    with np.errstate(all="ignore"):
        d = e[None, :] - p
    return ~rays_occluded(p, d, vertices, faces, t_min, 1.0)


def camera_rays(cam_pos, target, f, cx, cy, H, W):
    """(origins, directions), float64 (H * W, 3) each, row v * W + u the ray through the integer centre of pixel (u, v) of render_mesh's
    camera: origin cam_pos, direction R^T (sx, sy, 1) with sx = (u - cx) / f, sy = -((v - cy) / f) and R the host's look_at_rotation
    in float64, so t is the camera-space Z as in render_mesh.  R^T is applied by a matrix product on the host: cast_rays on these rays
    agrees with render_mesh up to rounding, and bit for bit only in the unrotated case include/pb3d.h states."""
    from .render import _camera
    R, cam, f, cx, cy, H, W, _ = _camera(cam_pos, target, f, cx, cy, H, W, 1.0)
    sx = (np.arange(W, dtype=np.float64) - cx) / f
    sy = -((np.arange(H, dtype=np.float64) - cy) / f)
    s = np.stack([np.broadcast_to(sx[None, :], (H, W)), np.broadcast_to(sy[:, None], (H, W)), np.ones((H, W))], axis=-1).reshape(-1, 3)
    return np.ascontiguousarray(np.broadcast_to(cam, s.shape)), np.ascontiguousarray(s @ R)
