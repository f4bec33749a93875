"""Mesh -> image: the depth, face and colour images of a triangle mesh under the pinhole camera project_colored_voxels uses.  It is the
pair the package lacked: with it the pipeline's last product (the smoothed, coloured marching-cubes mesh, or a CAD model) is compared
with the part masks under the fitted cameras -- projection IoU per part, silhouettes, z-buffers -- without being voxelized again and
splatted, and a model's silhouette becomes a mask for perspective_carve.

include/pb3d.h states the result to the bit.  The ray through the integer centre of pixel (u, v) is tested against every face by the
signs of three edge values of the face's sheared corners (Woop, Benthin and Wald 2013, all in float64, one rounded operation each): a ray
cannot pass between two faces that share an edge, and a face that crosses the camera plane needs no clipping.  A pixel takes the hit
with the smallest (t, face number); t is the camera-space Z.  Shading picks the attribute of the winner's dominant corner: no blending,
part colours stay part colours.

csrc/render.hip: integer minima on the bit patterns of t, then on the face numbers -- no floating-point atomics, the images are a
function of the input alone.  The NumPy forms upload the mesh and download the images; the *_resident twins take and return device
handles (pb3d.device.DeviceBuffer)."""
import ctypes as C
import math

import numpy as np

from . import _lib, device as dev
from ._args import _counts, _mesh
from ._lib import _ptr

__all__ = ["render_mesh", "render_mesh_resident", "render_shade_resident", "mesh_projection_iou", "render_last"]

MAX_PIXELS = 2 ** 31 - 1
FRAMES = ("points", "meshify")
STATS = ("pruned", "small", "large", "tile_jobs")


def _camera(cam_pos, target, f, cx, cy, H, W, near):
    """(R as nine float64, cam as three, f, cx, cy, H, W, near) as the entry takes them; R is look_at_rotation's, taken in float64"""
    from .camera_geometry import look_at_rotation
    cam = np.array(cam_pos, dtype=np.float64)
    tgt = np.array(target, dtype=np.float64)
    if cam.shape != (3,) or tgt.shape != (3,) or not (np.all(np.isfinite(cam)) and np.all(np.isfinite(tgt))):
        raise ValueError(f"cam_pos and target must be three finite numbers each (got {cam_pos!r} and {target!r})")
    f, cx, cy, near = float(f), float(cx), float(cy), float(near)
    if not math.isfinite(f) or f <= 0.0:
        raise ValueError(f"f must be finite and > 0 (got {f!r})")
    if not (math.isfinite(cx) and math.isfinite(cy)):
        raise ValueError(f"cx and cy must be finite (got {cx!r}, {cy!r})")
    if not math.isfinite(near) or near <= 0.0:
        raise ValueError(f"near must be finite and > 0 (got {near!r})")
    for v in (H, W):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(f"H and W must be integers >= 1 (got {H!r}, {W!r})")
    H, W = int(H), int(W)
    if H * W > MAX_PIXELS:
        raise ValueError(f"an image holds at most 2^31 - 1 pixels (got {H} x {W})")
    with np.errstate(all="ignore"):
        R = np.ascontiguousarray(look_at_rotation(cam.copy(), tgt), dtype=np.float64)
    if not np.all(np.isfinite(R)):
        raise ValueError("cam_pos and target must differ: the look-at rotation is not finite")
    return R, np.ascontiguousarray(cam), f, cx, cy, H, W, near


def _frame(frame, depth):
    if not isinstance(frame, str) or frame not in FRAMES:
        raise ValueError(f"frame must be 'points' or 'meshify' (got {frame!r})")
    if frame == "points":
        return 0, 0.0
    if depth is None:
        raise ValueError("frame='meshify' needs depth, the last axis of the grid the mesh came from")
    d = float(depth)
    if not math.isfinite(d):
        raise ValueError(f"depth must be finite (got {depth!r})")
    return 1, d


def _background(background, channels):
    """the `channels` bytes pixels without a hit take: an integer in [0, 255] (every channel) or one per channel"""
    b = np.asarray(background)
    if b.shape not in ((), (channels,)) or b.dtype.kind not in "iu":
        raise ValueError(f"background must be an integer in [0, 255] or {channels} of them (got {background!r})")
    b = np.broadcast_to(b.astype(np.int64), (channels,))
    if b.min() < 0 or b.max() > 255:
        raise ValueError(f"background must be an integer in [0, 255] or {channels} of them (got {background!r})")
    return np.ascontiguousarray(b, dtype=np.uint8)


def _colors(vertex_colors, nv):
    """(contiguous (nv, C) uint8 array, the image's trailing shape): uint8 (nv,), (nv, 1) or (nv, 3) as it is, or the float colour / 255
    form meshify_colored_voxel_grid returns, converted by rint(c * 255)"""
    c = np.asarray(vertex_colors)
    if c.ndim == 1:
        tail, c = (), c.reshape(-1, 1)
    elif c.ndim == 2 and c.shape[1] in (1, 3):
        tail = (c.shape[1],)
    else:
        raise ValueError(f"vertex_colors must have shape (n,), (n, 1) or (n, 3) (got {c.shape})")
    if c.shape[0] != nv:
        raise ValueError(f"vertex_colors has {c.shape[0]} rows for {nv} vertices")
    if c.dtype.kind == "f":
        if c.size and not (np.all(np.isfinite(c)) and c.min() >= 0.0 and c.max() <= 1.0):
            raise ValueError("float vertex_colors must lie in [0, 1] (colour / 255)")
        c = np.rint(c * 255)
    elif c.dtype != np.uint8:
        raise TypeError(f"vertex_colors must be uint8 or float colour / 255 (got {c.dtype})")
    return np.ascontiguousarray(c, dtype=np.uint8), tail


def render_last():
    """pb3d_render_last: of the context's last completed rendering, the dict of faces pruned, on the small (one lane) path, on the large
    (tile job) path, and tile jobs"""
    s = (C.c_int64 * 4)()
    _lib.check(_lib.load().pb3d_render_last(_lib.ctx(), s))
    return dict(zip(STATS, (int(v) for v in s)))


def render_shade_resident(d_face, d_bary, n_pixels, d_faces, n_faces, n_vertices, d_colors, channels, background=0, faces_i64=False, out=None):
    """pb3d_render_shade_resident: a DeviceBuffer of n_pixels * channels bytes -- per pixel the `channels` (1 or 3) bytes that the
    resident (n_vertices, channels) uint8 list d_colors holds for the dominant corner of the pixel's face, `background` where the face
    image holds -1.  Enqueued."""
    channels = int(channels)
    if channels not in (1, 3):
        raise ValueError(f"channels must be 1 or 3 (got {channels})")
    bg = _background(background, channels)
    with dev.Scope() as sc:
        d_out = sc.result(out, max(1, int(n_pixels) * channels))
        _lib.check(_lib.load().pb3d_render_shade_resident(_lib.ctx(), _ptr(d_face), _ptr(d_bary), int(n_pixels), _ptr(d_faces), int(bool(faces_i64)),
                                                          int(n_faces), int(n_vertices), _ptr(d_colors), channels, _lib.p_u8(bg), _ptr(d_out)))
        return d_out


def render_mesh_resident(d_verts, n_vertices, d_faces, n_faces, cam_pos, target, f, cx, cy, H, W, d_colors=None, channels=3, background=0,
                         near=1e-6, frame="points", depth=None, return_bary=False, verts_f64=False, faces_i64=False):
    """render_mesh on DeviceBuffer handles: (d_depth, d_face[, d_image][, d_bary]) -- H * W float64, H * W int32, H * W * channels bytes
    (with d_colors, the resident (n_vertices, channels) uint8 attribute) and H * W * 3 float64 (with return_bary).  It takes what
    pb3d.device.meshify(..., download=False) hands out as it is: float32 vertices, int32 faces, nearest-voxel bytes, frame="meshify".
    Two host waits (the index / finiteness check: IndexError, ValueError; the tile-job count); nothing is returned when it fails."""
    nv, nf = _counts(n_vertices, n_faces)
    R, cam, f, cx, cy, H, W, near = _camera(cam_pos, target, f, cx, cy, H, W, near)
    fr, d = _frame(frame, depth)
    channels = int(channels)
    if d_colors is not None:
        if channels not in (1, 3):
            raise ValueError(f"channels must be 1 or 3 (got {channels})")
        _background(background, channels)
    npix = H * W
    with dev.Scope() as sc:
        d_depth, d_face = sc.result(None, npix * 8), sc.result(None, npix * 4)
        want_bary = return_bary or d_colors is not None
        d_bary = (sc.result(None, npix * 24) if return_bary else sc.alloc(npix * 24)) if want_bary else None
        _lib.check(_lib.load().pb3d_render_mesh_resident(_lib.ctx(), _ptr(d_verts), int(bool(verts_f64)), nv, _ptr(d_faces), int(bool(faces_i64)), nf,
                                                         fr, d, _lib.p_dbl(R), _lib.p_dbl(cam), f, cx, cy, H, W, near, _ptr(d_depth), _ptr(d_face),
                                                         _ptr(d_bary)))
        out = [d_depth, d_face]
        if d_colors is not None:
            out.append(render_shade_resident(d_face, d_bary, npix, d_faces, nf, nv, d_colors, channels, background, faces_i64))
        if return_bary:
            out.append(d_bary)
        return tuple(out)


def render_mesh(vertices, faces, cam_pos, target, f, cx, cy, H, W, vertex_colors=None, background=0, near=1e-6, frame="points", depth=None,
                return_bary=False):
    """The (n, 3) vertex array and (m, 3) integer face array seen from cam_pos looking at target, with project_colored_voxels' camera:
    (depth, face[, image][, bary]).  depth is (H, W) float64, the camera-space Z of the nearest hit and +inf where there is none; face
    (H, W) int32, the number of the face hit (the smaller number among faces hit at the same depth), -1 for none.  With vertex_colors
    -- uint8 (n,), (n, 1) or (n, 3), or the float colour / 255 form of meshify_colored_voxel_grid -- image is (H, W[, 1 or 3]) uint8:
    the colour of the hit face's dominant corner, `background` elsewhere.  return_bary adds the (H, W, 3) float64 weights of the hit
    face's corners.  float32 vertices stay float32 (the arithmetic is float64), other real dtypes become float64; negative face indices
    wrap as NumPy's do.  frame="meshify" takes the vertices as meshify_colored_voxel_grid returns them and needs `depth`, the grid's last
    axis; frame="points" is the (x, y, z) frame of voxel_grid_to_points.  Faces nearer than `near` along the camera axis are not seen."""
    _camera(cam_pos, target, f, cx, cy, H, W, near)
    _frame(frame, depth)
    v, vf, fc, fi = _mesh(vertices, faces)
    cols, tail = (None, None) if vertex_colors is None else _colors(vertex_colors, len(v))
    if cols is not None:
        _background(background, cols.shape[1])
    H, W = int(H), int(W)
    with dev.Scope() as sc:
        d_v, d_f = sc.upload(v), sc.upload(fc)
        d_c = None if cols is None else sc.upload(cols) or sc.alloc(1)      # no vertex: nothing is read, but the handle says "shade"
        res = sc.adopt(render_mesh_resident(d_v, len(v), d_f, len(fc), cam_pos, target, f, cx, cy, H, W, d_c, 3 if cols is None else cols.shape[1],
                                            background, near, frame, depth, return_bary, vf, fi))
        out = [res[0].download((H, W), np.float64), res[1].download((H, W), np.int32)]
        k = 2
        if cols is not None:
            out.append(res[k].download((H, W) + tail))
            k += 1
        if return_bary:
            out.append(res[k].download((H, W, 3), np.float64))
        return tuple(out)


def mesh_projection_iou(vertices, faces, vertex_colors, seg_image, part_colors, cam_pos, target, f, cx, cy, background=0, near=1e-6,
                        frame="points", depth=None):
    """compute_partwise_iou of the rendered mesh against an (H, W, 3) uint8 part image, what it returns: ({part: inter / union, or 0.0
    when the union is empty}, mean over parts).  The mesh is rendered and shaded with its (n, 3) vertex_colors at the image's size and
    compared by pb3d_partwise_iou_dev where it lies: nothing is downloaded but the counts."""
    seg = _lib.as_u8(seg_image, "seg_image")
    if seg.ndim != 3 or seg.shape[2] != 3:
        raise ValueError(f"seg_image must be an (H, W, 3) image (got shape {seg.shape})")
    H, W = seg.shape[:2]
    v, vf, fc, fi = _mesh(vertices, faces)
    cols, _ = _colors(vertex_colors, len(v))
    if cols.shape[1] != 3:
        raise ValueError("vertex_colors must be (n, 3) to be compared with a part image")
    names = list(part_colors.keys())
    pc = np.asarray([part_colors[n] for n in names], np.int64).reshape(-1, 3)
    ok = np.all((pc >= 0) & (pc <= 255), axis=1)
    c8 = np.ascontiguousarray(pc[ok].astype(np.uint8))
    inter, uni = np.zeros(len(pc), np.int64), np.zeros(len(pc), np.int64)
    with dev.Scope() as sc:
        d_v, d_f, d_c, d_seg = (sc.upload(a) for a in (v, fc, cols, seg))
        res = sc.adopt(render_mesh_resident(d_v, len(v), d_f, len(fc), cam_pos, target, f, cx, cy, H, W, d_c or sc.alloc(1), 3, background, near,
                                            frame, depth, False, vf, fi))
        i8, u8 = np.zeros(len(c8), np.int64), np.zeros(len(c8), np.int64)
        for s in range(0, len(c8), 32):
            chunk = np.ascontiguousarray(c8[s:s + 32])
            _lib.check(_lib.load().pb3d_partwise_iou_dev(_lib.ctx(), _ptr(res[2]), _ptr(d_seg), H * W, _lib.p_u8(chunk), len(chunk),
                                                         i8[s:].ctypes.data_as(_lib.i64p), u8[s:].ctypes.data_as(_lib.i64p)))
        inter[ok], uni[ok] = i8, u8
    per_part = {name: ((i / u) if u > 0 else 0.0) for name, i, u in zip(names, inter, uni)}
    return per_part, np.mean(list(per_part.values()))
