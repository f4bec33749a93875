"""Perspective carve and paint: silhouette carving of a voxel grid by pinhole views (csrc/pcarve.hip), and the colours of the views'
images on the voxels they see (csrc/ppaint.hip).

The reference carves by orthographic views only.  With the cameras notebook 2 fits for the front and the aerial image, the next
step is to carve the coloured grid by those views: a voxel goes when it projects onto background in some view.  The pixel of a
voxel is exactly the one project_colored_voxels (reference utils/projection_utils.py:5-23) paints it on; include/pb3d.h states the
semantics to the bit.

perspective_paint is the second half, as apply_colored_mask_to_voxel_grid is for the orthographic carve: a voxel a view sees (the
reference's z-buffer test, utils/eval_helpers_intra.py:134-190) takes the colour of the pixel it is seen at."""
import ctypes as C

import numpy as np

from . import _lib, device as dev
from ._args import _cam, _colour_table, _eps_f32, _grid, _grid_shape, _on_device
from ._lib import _ptr
from .eval_helpers_intra import depth_buffer_resident

__all__ = ["perspective_carve", "perspective_carve_resident", "pack_mask_bits", "perspective_paint", "perspective_paint_resident"]

MAX_COLOURS = 31
MAX_PAINT_VIEWS = 8
MAX_SKIP = 8


def pack_mask_bits(mask):
    """(H, (W + 31) // 32) uint32 bit image of an (H, W) mask of any dtype or an (H, W, 3) one: pixel u of a row is bit u & 31 of
    word u >> 5, set where any value of the pixel is non-zero.  Host NumPy."""
    m = np.asarray(mask)
    if m.ndim == 3 and m.shape[2] == 3:
        m = np.any(m != 0, axis=2)
    elif m.ndim == 2:
        m = m != 0
    else:
        raise ValueError(f"a mask is (H, W) or (H, W, 3), got shape {m.shape}")
    H, W = m.shape
    if H == 0 or W == 0:
        raise ValueError(f"a mask has at least one pixel, got shape {m.shape}")
    padded = np.zeros((H, (W + 31) // 32 * 32), np.uint8)
    padded[:, :W] = m
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view("<u4")


class _DeviceMaskBits:
    """pack_mask_bits of a mask on the device.  perspective_carve_resident makes one per host mask and call; a caller that carves by
    the same masks again and again (tools/pcarvebench.py) makes them once and passes them in place of the masks."""

    def __init__(self, mask):
        bits = pack_mask_bits(mask)
        self.H, self.W = int(bits.shape[0]), int(np.asarray(mask).shape[1])
        self.buf = dev.from_numpy_async(bits)

    def free(self):
        self.buf.free()


def _subject_table(colors, Cc):
    """(uint8 table, ncolors); None selects every occupied voxel"""
    if colors is None:
        return np.zeros((0, Cc), np.uint8), 0
    tab = _colour_table(colors, Cc)
    if len(tab) == 0:
        raise ValueError("colors is None (every occupied voxel) or a list of colours, got an empty list")
    if len(tab) > MAX_COLOURS:
        raise ValueError(f"at most {MAX_COLOURS} subject colours, got {len(tab)}")
    if not tab.any(axis=1).all():
        raise ValueError("a subject colour is black / label 0 (the empty voxel)")
    return tab, len(tab)


def _outside(outside):
    if outside not in ("carve", "keep"):
        raise ValueError(f"outside is 'carve' or 'keep', got {outside!r}")
    return int(outside == "keep")


def _fill_view(rec, cam):
    """the camera of a CarveView / PaintView record; returns the promotion flags"""
    R, cp, prec = _cam(cam, np.float32)
    rec.R[:] = R.reshape(9).tolist(); rec.cam[:] = cp.reshape(3).tolist()
    rec.f, rec.cx, rec.cy = float(cam["f"]), float(cam["cx"]), float(cam["cy"])
    rec.prec[:] = list(prec)
    return prec


def _rewritten(voxel_grid, grid_shape, nviews, return_counts, run):
    """The tail of perspective_carve / perspective_paint, once every argument is checked: run(d_grid, shape, d_out, d_counts) rewrites
    the resident grid into a new buffer; the result is downloaded, or wrapped as a DeviceGrid for a DeviceGrid."""
    g, shape = _grid(voxel_grid)
    with dev.Scope() as sc:
        d_g = _on_device(sc, g)
        d_out = sc.alloc(max(1, int(np.prod(shape, dtype=np.int64))))
        d_cnt = sc.alloc(8 * max(1, nviews)) if return_counts else None
        run(d_g, shape, d_out, d_cnt if nviews else None)
        counts = d_cnt.download((nviews,), np.int64) if return_counts else None
        if isinstance(voxel_grid, dev.DeviceGrid):
            res = dev.DeviceGrid(sc.keep(d_out), grid_shape)
        else:
            res = d_out.download(grid_shape)
    return (res, counts) if return_counts else res


def perspective_carve_resident(d_grid, shape, views, colors=None, outside="carve", out=None, d_removed=None):
    """pb3d_perspective_carve_resident, queued on the context's stream: nothing is downloaded and the host does not wait.
    d_grid: DeviceBuffer (or a pointer into one, DeviceBuffer.at) of the (A0, A1, A2, C) uint8 grid, shape = (A0, A1, A2, C) with
    C = 1 or 3.  views: (mask, cam) pairs, mask a host array or a _DeviceMaskBits, cam a dict with cam_pos, target, f, cx, cy.
    out: DeviceBuffer of the result (it may not overlap the grid), None = in place.  d_removed: DeviceBuffer of len(views) int64 (or
    a pointer into one), None = no counts.  Returns `out` (d_grid when in place)."""
    A0, A1, A2, Cc = (int(v) for v in shape)
    keep = _outside(outside)
    tab, ncol = _subject_table(colors, Cc)
    views = list(views)
    arr = (_lib.CarveView * max(1, len(views)))()
    with dev.Scope() as sc:     # (the context's pool hands a freed block out again only behind this stream's work)
        for k, (mask, cam) in enumerate(views):
            mb = mask if isinstance(mask, _DeviceMaskBits) else sc.adopt(_DeviceMaskBits(mask))
            _fill_view(arr[k], cam)
            arr[k].Himg, arr[k].Wimg, arr[k].d_maskbits = mb.H, mb.W, mb.buf.ptr
        dst = d_grid if out is None else out
        _lib.check(_lib.load().pb3d_perspective_carve_resident(_lib.ctx(), _ptr(d_grid), A0, A1, A2, Cc, _lib.p_u8(tab) if ncol else None, ncol,
                                                               C.cast(arr, C.c_void_p), len(views), keep, _ptr(dst), _ptr(d_removed)))
        return dst


def perspective_carve(voxel_grid, views, colors=None, outside="carve", return_counts=False):
    """Carve a grid by perspective views: a new grid in which every subject voxel that some view rejects is zero.

    voxel_grid: uint8 (A0,A1,A2,3) RGB or (A0,A1,A2) labels, a NumPy array or a DeviceGrid (then the result is a new DeviceGrid).
    Voxel (a0,a1,a2) is the float32 point (x = a2, y = a1, z = a0), occupied where any channel is non-zero.
    views: a sequence of (mask, cam); mask (H,W) of any dtype or (H,W,3), set where any value is non-zero, each view with its own
    size; cam a dict with cam_pos, target, f, cx, cy (the camera JSONs of notebook 2 through load_camera_json).
    colors: None, or at most 31 non-black colours / non-zero labels: only voxels of these are subject, the others are copied.
    A view rejects a subject voxel whose pixel (project_colored_voxels' arithmetic, to the bit) is inside the image on a clear
    mask pixel; a pixel outside the image rejects with outside="carve" and accepts with outside="keep".  Views apply in order and
    the first rejection zeroes the voxel.  return_counts=True also returns the int64 (K,) array of voxels zeroed per view."""
    views = list(views)
    _outside(outside)       # every argument is checked before anything is uploaded
    for mask, _ in views:
        if not isinstance(mask, _DeviceMaskBits):
            m = np.asarray(mask)
            if not (m.ndim == 2 or (m.ndim == 3 and m.shape[2] == 3)) or 0 in m.shape[:2]:
                raise ValueError(f"a mask is a non-empty (H, W) or (H, W, 3) array, got shape {m.shape}")
    grid_shape = _grid_shape(voxel_grid)
    _subject_table(colors, 3 if len(grid_shape) == 4 else 1)
    return _rewritten(voxel_grid, grid_shape, len(views), return_counts, lambda d_g, shape, d_out, d_rem:
                      perspective_carve_resident(d_g, shape, views, colors, outside, out=d_out, d_removed=d_rem))


# ---- perspective paint -------------------------------------------------------------------------------------------------------------
class _DeviceImage:
    """A view's (H, W, 3) RGB or (H, W) label image on the device.  perspective_paint_resident makes one per host image and call; a
    caller whose image is resident already wraps it: _DeviceImage(DeviceBuffer or pointer into one, H, W)."""

    def __init__(self, image, H=None, W=None):
        if H is None:
            img = _lib.as_u8(image, "a view's image")
            self.H, self.W = int(img.shape[0]), int(img.shape[1])
            self.buf, self.owned = dev.from_numpy_async(img), True
        else:
            self.H, self.W, self.buf, self.owned = int(H), int(W), image, False

    def free(self):
        if self.owned:
            self.buf.free()


def _image_shape(image, Cc):
    """(H, W) of a view's image, checked against the grid's channels"""
    if isinstance(image, _DeviceImage):
        H, W = image.H, image.W
    else:
        m = _lib.as_u8(image, "a view's image")
        if m.ndim != (3 if Cc == 3 else 2) or (Cc == 3 and m.shape[2] != 3):
            raise ValueError(f"the image of a view is (H, W, 3) for an RGB grid and (H, W) for a label grid, got shape {m.shape}")
        H, W = m.shape[:2]
    if H <= 0 or W <= 0:
        raise ValueError(f"the image of a view has at least one pixel, got {H} x {W}")
    return int(H), int(W)


def _skip_table(skip, Cc):
    tab = _colour_table(skip, Cc)
    if len(tab) > MAX_SKIP:
        raise ValueError(f"at most {MAX_SKIP} skip colours, got {len(tab)}")
    return tab


def _paint_args(Cc, views, colors, skip):
    """the host-only checks of both entries: (views as a list, [(H, W)], subject table, ncolors, skip table)"""
    views = list(views)
    if len(views) > MAX_PAINT_VIEWS:
        raise ValueError(f"at most {MAX_PAINT_VIEWS} views, got {len(views)}")
    sizes = [_image_shape(image, Cc) for image, _ in views]
    tab, ncol = _subject_table(colors, Cc)
    return views, sizes, tab, ncol, _skip_table(skip, Cc)


def perspective_paint_resident(d_grid, shape, views, d_zbufs, colors=None, skip=(), eps=1e-3, out=None, d_painted=None):
    """pb3d_perspective_paint_resident, queued on the context's stream: nothing is downloaded and the host does not wait.
    d_grid: DeviceBuffer (or a pointer into one, DeviceBuffer.at) of the (A0, A1, A2, C) uint8 grid, shape = (A0, A1, A2, C) with
    C = 1 or 3.  views: (image, cam) pairs, image a host array or a _DeviceImage, cam a dict with cam_pos, target, f, cx, cy.
    d_zbufs: per view the DeviceBuffer (or pointer) of its float32 (H, W) z-buffer, normally depth_buffer_resident of the grid before
    painting.  out: DeviceBuffer of the result (it may not overlap the grid in part), None = in place.  d_painted: DeviceBuffer of
    len(views) int64 (or a pointer into one), None = no counts.  Returns `out` (d_grid when in place)."""
    A0, A1, A2, Cc = (int(v) for v in shape)
    views, sizes, tab, ncol, sk = _paint_args(Cc, views, colors, skip)
    d_zbufs = list(d_zbufs)
    if len(d_zbufs) != len(views):
        raise ValueError(f"{len(views)} views but {len(d_zbufs)} z-buffers")
    arr = (_lib.PaintView * max(1, len(views)))()
    eps_f32 = max([_eps_f32(_fill_view(arr[k], cam), eps) for k, (_, cam) in enumerate(views)], default=0)     # read by float32 cameras only
    with dev.Scope() as sc:     # (the context's pool hands a freed block out again only behind this stream's work)
        for k, ((image, _), (H, W)) in enumerate(zip(views, sizes)):
            im = image if isinstance(image, _DeviceImage) else sc.adopt(_DeviceImage(image))
            arr[k].Himg, arr[k].Wimg, arr[k].d_image, arr[k].d_zbuf = H, W, _ptr(im.buf), _ptr(d_zbufs[k])
        dst = d_grid if out is None else out
        _lib.check(_lib.load().pb3d_perspective_paint_resident(_lib.ctx(), _ptr(d_grid), A0, A1, A2, Cc, _lib.p_u8(tab) if ncol else None, ncol,
                                                               C.cast(arr, C.c_void_p), len(views), _lib.p_u8(sk) if len(sk) else None, len(sk),
                                                               float(eps), eps_f32, _ptr(dst), _ptr(d_painted)))
        return dst


def perspective_paint(voxel_grid, views, colors=None, skip=(), eps=1e-3, zbufs=None, return_counts=False):
    """Paint a grid by perspective views: a new grid in which every subject voxel some view paints has that view's pixel colour.
    include/pb3d.h (pb3d_perspective_paint_resident) states the semantics.

    voxel_grid: uint8 (A0,A1,A2,3) RGB or (A0,A1,A2) labels, a NumPy array or a DeviceGrid (then the result is a new DeviceGrid).
    Voxel (a0,a1,a2) is the float32 point (x = a2, y = a1, z = a0), occupied where any channel is non-zero.
    views: a sequence of at most 8 (image, cam); image uint8 (H,W,3) for an RGB grid, (H,W) for a label grid, each view with its own
    size; cam a dict with cam_pos, target, f, cx, cy whose dtypes decide the float widths as they do for grid_visible_bits.
    colors: None, or at most 31 non-black colours / non-zero labels: only voxels of these are subject, the others are copied.
    skip: at most 8 image colours / labels that never paint (the masks' background); black / label 0 never paints.
    zbufs: None, or per view a float32 (H,W) array or a DeviceBuffer; None = the z-buffer of the input grid under the view's camera.
    A view sees a subject voxel whose pixel is inside the image (Z > 1e-6) with |Z - zbuf[v,u]| < eps, and paints it when the pixel is
    neither black nor in skip.  Views are tried in order, the first that paints a voxel decides its colour, a voxel no view paints
    keeps its own.  return_counts=True also returns the int64 (K,) array of voxels decided per view."""
    grid_shape = _grid_shape(voxel_grid)
    views, sizes, _, _, _ = _paint_args(3 if len(grid_shape) == 4 else 1, views, colors, skip)      # every argument is checked before anything is uploaded
    for _, cam in views:
        _cam(cam, np.float32)
    host_z = [None] * len(views)
    if zbufs is not None:
        zbufs = list(zbufs)
        if len(zbufs) != len(views):
            raise ValueError(f"{len(views)} views but {len(zbufs)} z-buffers")
        for k, (zb, hw) in enumerate(zip(zbufs, sizes)):
            if not isinstance(zb, dev.DeviceBuffer):
                host_z[k] = np.ascontiguousarray(zb, np.float32)
                if host_z[k].shape != hw:
                    raise ValueError(f"the z-buffer of view {k} is {host_z[k].shape}, its image {hw}")
            elif zb.nbytes != 4 * hw[0] * hw[1]:
                raise ValueError(f"the z-buffer of view {k} holds {zb.nbytes} bytes, its {hw[0]} x {hw[1]} image needs {4 * hw[0] * hw[1]}")

    def paint(d_g, shape, d_out, d_cnt):
        with dev.Scope() as sc:         # (the context's pool hands a freed block out again only behind this stream's work)
            d_z = []
            for k, ((_, cam), (H, W)) in enumerate(zip(views, sizes)):
                if zbufs is None:
                    d_z.append(sc.adopt(depth_buffer_resident(d_g, shape, cam, H, W)))
                elif host_z[k] is not None:
                    d_z.append(sc.upload(host_z[k], wait=False))
                else:
                    d_z.append(zbufs[k])
            perspective_paint_resident(d_g, shape, views, d_z, colors, skip, eps, out=d_out, d_painted=d_cnt)

    return _rewritten(voxel_grid, grid_shape, len(views), return_counts, paint)
