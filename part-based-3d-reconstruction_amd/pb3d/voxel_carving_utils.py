"""Orthographic semantic voxel carving on MI355X -- host mirror of the reference interface.

Same function names, argument meaning, return shapes/dtypes and error behaviour as
reference utils/voxel_carving_utils.py; every array operation runs in hand-written HIP
kernels (csrc/*.hip) through the ctypes C-ABI (include/pb3d.h).  Grids are uint8 with axes
(W=x, H=y, D=z[,3]).  There is no CPU fallback.
"""
import ctypes as C

import numpy as np

from . import _hostmem, _lib, device as dev
from .config import PART_COLORS, PART_COLORS_NP  # noqa: F401  (re-exported like upstream)

__all__ = ["carve_voxel_grid_with_masks", "process_voxel_grid", "apply_colored_mask_to_voxel_grid", "part_carve",
           "left_right_guided_carve", "extrude_from_surface", "recolor_backward_components", "global_carve", "partwise_carve"]

# optional visualisation hook (reference utils/visualization.plot_voxel); set by pb3d.install()
plot_voxel = None


def _mask_to_wh(mask, W, H):
    """Orient a 2-D/3-D mask as (W,H[,3]); reference :19-28.  The (H,W) test comes first, so a
    square mask is always transposed."""
    mask = np.asarray(mask)
    if mask.shape[:2] == (H, W):
        return mask.T
    if mask.shape[:2] == (W, H):
        return mask
    raise ValueError(f"Mask shape {mask.shape} incompatible with (W,H)=({W},{H})")


def _rotation_matrix_inv(angle):
    """inv of the Y-rotation by `angle` degrees, bit-identical to the reference's LAPACK result
    for the integer angles 0..90 its loops can produce (reference :65-69; pinned table)."""
    M = np.empty((3, 3), np.float64)
    if int(angle) != angle:
        raise ValueError("only integer angles 0..90 are pinned")
    _lib.check(_lib.load().pb3d_rotinv(int(angle), _lib.p_dbl(M)))
    return M


def _occupancy(grid):
    """any(grid > 0, axis=-1) as uint8; reference :32-33."""
    g = _lib.as_u8(grid, "grid")
    if g.ndim != 4 or g.shape[3] != 3:
        raise ValueError("_occupancy expects a (W,H,D,3) grid")
    out = _hostmem.empty(g.shape[:3], np.uint8)
    _lib.check(_lib.load().pb3d_occupancy(_lib.ctx(), _lib.p_u8(g), out.size, _lib.p_u8(out)))
    return out


def carve_voxel_grid_with_masks(voxel_grid, combined_mask):
    """np.where(mask[x,y], grid, 0) broadcast over z (and channel); reference :76-97."""
    g = np.ascontiguousarray(np.asarray(voxel_grid))
    if g.ndim not in (3, 4):
        raise ValueError(f"voxel_grid must be (W,H,D) or (W,H,D,C), got {g.shape}")
    W, H, D = g.shape[:3]
    mask = _mask_to_wh(combined_mask, W, H)
    if mask.ndim == 2:
        m = _lib.truth_u8(mask)
        if g.dtype == np.uint8 and (g.ndim == 3 or g.shape[3] == 3):
            out = _hostmem.empty_like(g)
            _lib.check(_lib.load().pb3d_carve_mask(_lib.ctx(), _lib.p_u8(g), W, H, D, 3 if g.ndim == 4 else 1,
                                                   _lib.p_u8(m), _lib.p_u8(out)))
            return out
        # Any other numeric dtype / channel count: np.where(mask, grid, 0) keeps the grid's dtype and either copies an element
        # bit for bit or writes a zero, so the op is "zero the bytes of the dropped (x,y) columns" whatever the elements are.
        if g.dtype == np.bool_:
            g = g.astype(np.result_type(g.dtype, 0))          # np.where(mask, bool_grid, 0) is an int64 grid (NumPy's promotion of the Python 0)
        if g.dtype.kind not in "uifc" or np.result_type(g.dtype, 0) != g.dtype:
            raise TypeError(f"voxel_grid dtype {g.dtype} is not supported (np.where would change it); use a numeric dtype")
        col_bytes = int(np.prod(g.shape[2:], dtype=np.int64)) * g.dtype.itemsize
        out = _hostmem.empty(g.shape, g.dtype)
        if g.size:
            _lib.check(_lib.load().pb3d_carve_mask(_lib.ctx(), g.view(np.uint8).ctypes.data_as(_lib.u8p), W, H, col_bytes, 1, _lib.p_u8(m),
                                                   out.view(np.uint8).ctypes.data_as(_lib.u8p)))
        return out
    if mask.ndim == 3 and mask.shape[2] == 3:
        # Upstream's RGB-mask branch (:90-95) selects with a (W,H,1,1) array against a (W,H,D)
        # channel slab; NumPy cannot broadcast that for any non-degenerate shape, so the call
        # always ends in this ValueError.  Mirrored rather than "fixed".
        raise ValueError(f"operands could not be broadcast together with shapes ({W},{H},1,1) ({W},{H},{D}) ()")
    raise ValueError("Unsupported mask shape")


_TYPED_CODES = {"int8": 1, "uint8": 2, "int16": 3, "uint16": 4, "int32": 5, "uint32": 6, "int64": 7, "uint64": 8, "float32": 9,
                "float64": 10, "complex64": 11, "complex128": 12}       # include/pb3d.h PB3D_I8 ..


def process_voxel_grid(voxel_grid, combined_mask, angle_interval=90):
    """for angle in range(0, 91, angle_interval): rotate about Y (trilinear, SciPy semantics) and
    carve; cumulative, never rotated back.  reference :104-126.  The loop runs on the device."""
    g = np.ascontiguousarray(np.asarray(voxel_grid))
    if g.ndim != 3:
        raise ValueError(f"process_voxel_grid rotates occupancy grids (W,H,D); got shape {g.shape}")
    W, H, D = g.shape
    if isinstance(angle_interval, (bool, np.bool_)) or not isinstance(angle_interval, (int, np.integer)):
        raise TypeError(f"'{type(angle_interval).__name__}' object cannot be interpreted as an integer")
    if angle_interval == 0:
        raise ValueError("range() arg 3 must not be zero")
    if angle_interval < 0:
        return g.copy()  # range(0, 91, negative) is empty: upstream returns the input grid
    if g.dtype == np.bool_:
        g = g.astype(np.int64)      # upstream's first np.where(mask, grid, 0) turns a bool grid into int64 (the 0-degree step before it is the identity)
    typed = _TYPED_CODES.get(g.dtype.name) if g.dtype != np.uint8 else None
    if g.dtype != np.uint8 and typed is None:
        # what SciPy's interpolation says to a dtype it does not take (float16, object, strings ...)
        raise RuntimeError("data type not supported")
    mask = _mask_to_wh(combined_mask, W, H)
    if mask.ndim != 2:
        carve_voxel_grid_with_masks(g, combined_mask)  # raises what upstream raises
    m = _lib.truth_u8(mask)
    if typed is not None:
        # any other dtype SciPy's interpolation takes (the reference's loop never looks at it): csrc/rotate_typed.hip
        if g.size == 0:
            return g.copy()
        with dev.Scope() as sc:
            d_g = sc.upload(g.view(np.uint8).reshape(-1)); d_m = sc.upload(m)
            d_o = sc.alloc(g.nbytes); d_t = sc.alloc(g.nbytes)
            _lib.check(_lib.load().pb3d_process_grid_typed_dev(_lib.ctx(), C.c_void_p(d_g.ptr), typed, W, H, D, C.c_void_p(d_m.ptr),
                                                               int(min(angle_interval, 91)), C.c_void_p(d_o.ptr), C.c_void_p(d_t.ptr)))
            return d_o.download((g.nbytes,)).view(g.dtype).reshape(g.shape)
    out = _hostmem.empty_like(g)
    _lib.check(_lib.load().pb3d_process_grid(_lib.ctx(), _lib.p_u8(g), W, H, D, _lib.p_u8(m), int(min(angle_interval, 91)),
                                             _lib.p_u8(out)))
    return out


def _rotate_and_carve(grid, mask, angle_interval):
    """reference :47-60 -- the loop of process_voxel_grid without the progress bar (upstream keeps it next to the public function; unused there)."""
    return process_voxel_grid(grid, mask, angle_interval)


def apply_colored_mask_to_voxel_grid(carved_voxel_grid, colored_mask):
    """out[x,y,z,:] = colored_mask[y,x,:] where carved == 1 else 0; reference :128-136."""
    cv = _lib.as_u8(carved_voxel_grid, "carved_voxel_grid")
    W, H, D = cv.shape
    rgb = np.ascontiguousarray(np.asarray(colored_mask).astype(np.uint8, copy=False))
    if rgb.shape != (H, W, 3):
        raise ValueError(f"colored_mask shape {rgb.shape} does not match (H,W,3)=({H},{W},3)")
    out = _hostmem.empty((W, H, D, 3), np.uint8)
    _lib.check(_lib.load().pb3d_color_apply(_lib.ctx(), _lib.p_u8(cv), W, H, D, _lib.p_u8(rgb), _lib.p_u8(out)))
    return out


# Derived 2-D masks are memoised by CONTENT (xxhash of the image bytes, ~40 us for a 278 x 512 x 3 mask): notebook 1 passes the same
# semantic masks to global_carve, part_carve, partwise_carve and every left_right_guided_carve, and the NumPy work on them (colour
# keys, per-job selections, transposes: ~4 ms per partwise_carve at Taj 512) was half the wall time of the resident chain.  Without
# the xxhash module nothing is memoised.
try:
    import xxhash as _xx
except Exception:       # pragma: no cover - optional accelerator
    _xx = None
_memo = {}


def _digest(a):
    if _xx is None or not isinstance(a, np.ndarray) or a.dtype == object or not a.flags["C_CONTIGUOUS"]:
        return None
    return (_xx.xxh3_128_digest(a), a.shape, a.dtype.str)


def _memo_get(kind, dig, extra=()):
    return None if dig is None else _memo.get((kind, dig, extra))


def _memo_put(kind, dig, extra, value):
    if dig is not None:
        if len(_memo) >= 64:
            _memo.pop(next(iter(_memo)))
        _memo[(kind, dig, extra)] = value
    return value


def _color_key(img_hw3):
    """(H,W) uint32 image r | g << 8 | b << 16 of an (H,W,3) uint8 image: one pass, then every np.all(img == colour, axis=-1)
    is a single integer compare (the per-colour broadcast compare of a 278 x 512 mask costs ~4 ms in NumPy, this ~0.05 ms)."""
    a = np.asarray(img_hw3)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        return None
    dig = _digest(a)
    hit = _memo_get("key", dig)
    if hit is not None:
        return hit
    a4 = np.zeros(a.shape[:2] + (4,), np.uint8)
    a4[..., :3] = a
    key = a4.view("<u4")[..., 0]
    key.flags.writeable = False
    return _memo_put("key", dig, (), key)


def _is_color(img_hw3, key, color):
    """np.all(img == color, axis=-1) (key = _color_key(img) or None)."""
    c = np.asarray(color)
    if key is None or c.shape != (3,) or c.dtype.kind not in "ui" or (c < 0).any() or (c > 255).any():
        return np.all(np.asarray(img_hw3) == color, axis=-1)
    return key == np.uint32(int(c[0]) | (int(c[1]) << 8) | (int(c[2]) << 16))


def _job_masks(semantic_mask, group_jobs, W, H, part_colors):
    """Per job: (mask2d.T as uint8, what _mask_to_wh makes of it, angle, skip) -- reference :143-151."""
    sm = np.asarray(semantic_mask)
    dig = _digest(sm)
    try:
        extra = (W, H, tuple((tuple(names), int(angle)) for names, angle in group_jobs),
                 tuple(tuple(int(v) for v in np.asarray(part_colors[n]).reshape(-1)) for names, _ in group_jobs for n in names))
    except Exception:
        dig, extra = None, ()
    hit = _memo_get("jobs", dig, extra)
    if hit is not None:
        msub, mcarve, ang, sk = hit
        nj1 = len(ang)
        return msub, mcarve, (C.c_int * nj1)(*ang), (C.c_int * nj1)(*sk)       # (the ctypes arrays are the caller's to modify)
    key = _color_key(sm)
    nj = len(group_jobs)
    msub = np.zeros((max(nj, 1), W, H), np.uint8)
    mcarve = np.zeros((max(nj, 1), W, H), np.uint8)
    angles = (C.c_int * max(nj, 1))()
    skip = (C.c_int * max(nj, 1))()
    # the key image transposed ONCE: every job's selection is then formed directly in the grid's (W,H) order (a strided transpose
    # and two strided copies per job were most of this function's 1.4 ms on a 278 x 512 mask)
    keyT = np.ascontiguousarray(key.T) if key is not None else None
    for j, (names, angle) in enumerate(group_jobs):
        if keyT is not None and all(_color_u8(part_colors[n]) is not None for n in names):
            selT = np.zeros(keyT.shape, bool)
            for n in names:
                c = _color_u8(part_colors[n])
                selT |= keyT == np.uint32(int(c[0]) | (int(c[1]) << 8) | (int(c[2]) << 16))
            m = selT.view(np.uint8)
        else:
            sel = np.zeros(sm.shape[:2], bool)
            for n in names:
                sel |= _is_color(sm, key, part_colors[n])
            m = sel.T.astype(np.uint8)
        skip[j] = 0 if m.any() else 1
        angles[j] = int(angle)
        if m.shape != (W, H):
            raise ValueError(f"operands could not be broadcast together: mask {m.shape} vs grid ({W},{H})")
        msub[j] = m
        mcarve[j] = _mask_to_wh(m, W, H)
    msub.flags.writeable = False; mcarve.flags.writeable = False
    _memo_put("jobs", dig, extra, (msub, mcarve, tuple(angles), tuple(skip)))
    return msub, mcarve, angles, skip


def part_carve(colored_grid, semantic_mask, group_jobs, visualize=False):
    """Per part group: select its pixels, carve the group's occupancy with its own symmetry
    angle, overlay the survivors; reference :139-160."""
    resident = isinstance(colored_grid, dev.DeviceGrid)          # device-resident chain: no upload, no download
    g = colored_grid if resident else _lib.as_u8(colored_grid, "colored_grid")
    if len(g.shape) != 4 or g.shape[3] != 3:
        raise ValueError("colored_grid must be (W,H,D,3)")
    W, H, D, _ = g.shape
    msub, mcarve, angles, skip = _job_masks(semantic_mask, group_jobs, W, H, PART_COLORS)
    for j in range(len(group_jobs)):
        if not skip[j] and angles[j] <= 0:
            raise ValueError("range() arg 3 must not be zero" if angles[j] == 0 else "negative angle steps are not supported")
        angles[j] = min(angles[j], 91) if angles[j] > 0 else angles[j]
    if resident:
        with dev.Scope() as sc:
            d_ms = sc.upload(msub) or sc.alloc(0); d_mc = sc.upload(mcarve) or sc.alloc(0)
            d_out = sc.result(None, g.nbytes)
            _lib.check(_lib.load().pb3d_part_carve_dev(_lib.ctx(), C.c_void_p(g.buf.ptr), W, H, D, C.c_void_p(d_ms.ptr), C.c_void_p(d_mc.ptr),
                                                       angles, skip, len(group_jobs), C.c_void_p(d_out.ptr)))
            dev.sync()
            return dev.DeviceGrid(d_out, g.shape)
    out = _hostmem.empty_like(g)
    _lib.check(_lib.load().pb3d_part_carve(_lib.ctx(), _lib.p_u8(g), W, H, D, _lib.p_u8(msub), _lib.p_u8(mcarve), angles, skip,
                                           len(group_jobs), _lib.p_u8(out)))
    return out


def global_carve(binary_mask, semantic_mask_exterior, angle_interval=90, stride=4, visualize=False, on_device=False):
    """ones((w,h,w)) -> process_voxel_grid -> colours; reference :269-298.  Returns (w,h,w,3) uint8
    (on_device=True: a pb3d.device.DeviceGrid that part_carve / partwise_carve take as is)."""
    b = np.asarray(binary_mask)
    if b.ndim != 2:
        raise ValueError("not enough values to unpack" if b.ndim < 2 else "too many values to unpack (expected 2)")
    h, w = b.shape
    if isinstance(angle_interval, (bool, np.bool_)) or not isinstance(angle_interval, (int, np.integer)):
        raise TypeError(f"'{type(angle_interval).__name__}' object cannot be interpreted as an integer")
    if angle_interval == 0:
        raise ValueError("range() arg 3 must not be zero")
    rgb = np.ascontiguousarray(np.asarray(semantic_mask_exterior).astype(np.uint8, copy=False))
    if rgb.shape != (h, w, 3):
        raise ValueError(f"semantic mask shape {rgb.shape} does not match (h,w,3)=({h},{w},3)")
    if angle_interval < 0:
        # empty angle loop: the all-ones grid is coloured as is
        return apply_colored_mask_to_voxel_grid(np.ones((w, h, w), np.uint8), rgb)
    bt = _lib.truth_u8(b)
    if on_device:
        with dev.Scope() as sc:
            d_b = sc.upload(bt) or sc.alloc(0); d_rgb = sc.upload(rgb) or sc.alloc(0)
            d_out = sc.result(None, w * h * w * 3)
            dev.global_carve(d_b, d_rgb, h, w, int(min(angle_interval, 91)), d_out)
            dev.sync()
            return dev.DeviceGrid(d_out, (w, h, w, 3))
    out = _hostmem.empty((w, h, w, 3), np.uint8)
    _lib.check(_lib.load().pb3d_global_carve(_lib.ctx(), _lib.p_u8(bt), _lib.p_u8(rgb), h, w, int(min(angle_interval, 91)),
                                             _lib.p_u8(out)))
    if visualize and plot_voxel is not None:
        from .voxel_utils import voxel_grid_to_points
        pts, cols, _ = voxel_grid_to_points(out, stride=stride)
        if pts.shape[0] > 0:
            plot_voxel(pts, cols, title="After global symmetric carving")
    return out


# =====================================================================================================
# Component-guided symmetry, interior extrusion, back-minaret recolouring, partwise_carve
# (reference :163-266, :302-400).  Connected components are labelled on the device (csrc/components.hip).
# =====================================================================================================
def _color_u8(color):
    """a palette entry as 3 uint8 values, or None if it cannot equal any uint8 voxel"""
    c = np.asarray(color).reshape(-1)
    if c.size != 3 or np.any(c < 0) or np.any(c > 255) or np.any(c != np.round(c)):
        return None
    return np.ascontiguousarray(c.astype(np.uint8))


def _label(d_grid, shape3, color_u8, d_labels):
    A0, A1, A2 = shape3
    n = C.c_int64(0)
    _lib.check(_lib.load().pb3d_label_color_dev(_lib.ctx(), C.c_void_p(d_grid.ptr), A0, A1, A2, _lib.p_u8(color_u8),
                                                C.c_void_p(d_labels.ptr), C.byref(n)))
    return n.value


def _component_stats(d_labels, shape3, n):
    A0, A1, A2 = shape3
    bbox = np.zeros((max(n, 1), 6), np.int64); cnt = np.zeros(max(n, 1), np.int64); sums = np.zeros((max(n, 1), 3), np.int64)
    if n:
        _lib.check(_lib.load().pb3d_component_stats_dev(_lib.ctx(), C.c_void_p(d_labels.ptr), A0, A1, A2, n,
                                                        bbox.ctypes.data_as(_lib.i64p), cnt.ctypes.data_as(_lib.i64p),
                                                        sums.ctypes.data_as(_lib.i64p)))
    return bbox[:n], cnt[:n], sums[:n]


def _label_stats(d_grid, shape3, color_u8, d_labels, cap=1024, members_only=False):
    """_label + _component_stats in one device pass and one host round trip (pb3d_label_color_stats_dev); scenes with more than
    `cap` components take the separate statistics pass.  members_only: d_labels is written at the colour's voxels only (for the
    consumers that walk the labelling's membership bits: the fused component loop and the recolouring)."""
    A0, A1, A2 = shape3
    n = C.c_int64(0); ok = C.c_int(0)
    bbox = np.zeros((cap, 6), np.int64); cnt = np.zeros(cap, np.int64); sums = np.zeros((cap, 3), np.int64)
    if isinstance(color_u8, (int, np.integer)):          # a 1-byte label volume (pb3d.labels): components of one label value
        _lib.check(_lib.load().pb3d_label_value_stats_dev(_lib.ctx(), C.c_void_p(d_grid.ptr), A0, A1, A2, int(color_u8), C.c_void_p(d_labels.ptr),
                                                          C.byref(n), cap, 1 if members_only else 0, bbox.ctypes.data_as(_lib.i64p), cnt.ctypes.data_as(_lib.i64p),
                                                          sums.ctypes.data_as(_lib.i64p), C.byref(ok)))
    else:
        _lib.check(_lib.load().pb3d_label_color_stats_dev(_lib.ctx(), C.c_void_p(d_grid.ptr), A0, A1, A2, _lib.p_u8(color_u8), C.c_void_p(d_labels.ptr),
                                                          C.byref(n), cap, 1 if members_only else 0, bbox.ctypes.data_as(_lib.i64p), cnt.ctypes.data_as(_lib.i64p),
                                                          sums.ctypes.data_as(_lib.i64p), C.byref(ok)))
    if not ok.value:
        if members_only:        # more components than `cap`: the separate statistics pass reads the WHOLE label volume -- label again, in full
            return _label_stats(d_grid, shape3, color_u8, d_labels, cap=cap, members_only=False)
        return (n.value,) + _component_stats(d_labels, shape3, n.value)
    return n.value, bbox[:n.value], cnt[:n.value], sums[:n.value]


def _label_stats_multi(d_grid, shape3, colors, d_labels, cap=1024, members_only=True):
    """The components of SEVERAL colours (or label values) in one labelling sequence and one host round trip
    (pb3d_label_colors_stats_dev: the grid is read once; labels are numbered per colour).  `colors`: a list of 3-byte colours, or of ints
    for a 1-byte label volume.  Returns a list of (n, bbox, count, sums) per colour; an entry is None where the colour has more than
    `cap` components (the caller labels that colour on its own)."""
    A0, A1, A2 = shape3
    K = len(colors)
    lib = _lib.load()
    n = (C.c_int64 * K)(); ok = (C.c_int * K)()
    bbox = np.zeros((K, cap, 6), np.int64); cnt = np.zeros((K, cap), np.int64); sums = np.zeros((K, cap, 3), np.int64)
    if isinstance(colors[0], (int, np.integer)):
        cols = np.ascontiguousarray(np.asarray(colors, np.uint8))
        fn = lib.pb3d_label_values_stats_dev
    else:
        cols = np.ascontiguousarray(np.asarray(colors, np.uint8).reshape(K, 3))
        fn = lib.pb3d_label_colors_stats_dev
    _lib.check(fn(_lib.ctx(), C.c_void_p(d_grid.ptr), A0, A1, A2, _lib.p_u8(cols), K, C.c_void_p(d_labels.ptr), n, cap, 1 if members_only else 0,
                  bbox.ctypes.data_as(_lib.i64p), cnt.ctypes.data_as(_lib.i64p), sums.ctypes.data_as(_lib.i64p), ok))
    return [((n[k], bbox[k, :n[k]], cnt[k, :n[k]], sums[k, :n[k]]) if ok[k] else None) for k in range(K)]


def _check_angle_step(angle):
    if isinstance(angle, (bool, np.bool_)) or not isinstance(angle, (int, np.integer)):
        raise TypeError(f"'{type(angle).__name__}' object cannot be interpreted as an integer")
    if angle == 0:
        raise ValueError("range() arg 3 must not be zero")


def _lrgc_dev(d_col, shape3, mask2d, target_color, angle, label=None, d_lab=None):
    """left_right_guided_carve on a device-resident grid.  Returns the DeviceBuffer that holds the result: d_col itself when the
    fused component loop ran (csrc/guided.hip: in place, one launch pair per batch of components), else a new buffer."""
    W, H, D = shape3
    lib, ctx = _lib.load(), _lib.ctx()
    nbytes = W * H * D * (3 if label is None else 1)      # label: d_col is a 1-byte label volume and `label` the part's label value
    with dev.Scope() as sc:
        if d_lab is None:
            d_lab = sc.alloc(W * H * D * 4)
        d_carved = None
        cu8 = _color_u8(target_color) if label is None else int(label)
        # (labels written at the component voxels only: the fused loop below consults the labelling's membership bits)
        num, bbox, _, _ = _label_stats(d_col, (W, H, D), cu8, d_lab, members_only=True) if cu8 is not None else (0, None, None, None)
        print(f"[{target_color}] 3D components: {num}")
        if not num:
            return d_col
        _check_angle_step(angle)
        # every component's 2-D crop mask goes up in ONE transfer and the "carved voxels" counts come back in one (upstream prints
        # between the steps; the text is the same, it is emitted after the loop)
        packed, offs = _pack_crop_masks(mask2d, bbox)
        counts = None
        if angle > 0:
            bb = np.ascontiguousarray(bbox, np.int64); cn = np.zeros(num, np.int64)
            took = C.c_int(0)
            fn = lib.pb3d_guided_carve_dev if label is None else lib.pb3d_guided_carve_label_dev
            _lib.check(fn(ctx, C.c_void_p(d_col.ptr), C.c_void_p(d_lab.ptr), W, H, D, num, bb.ctypes.data_as(_lib.i64p),
                                                 _lib.p_u8(packed), offs.ctypes.data_as(_lib.i64p), packed.size, int(min(angle, 91)),
                                                 cn.ctypes.data_as(_lib.i64p), C.byref(took)))
            if took.value:
                counts = cn
        if counts is None:
            # a crop too large for the LDS-resident chain (or an empty angle loop): component by component, into a copy -- these entries
            # read labels at every voxel of a crop, so the volume is labelled again, in full
            if label is None:
                _label(d_col, (W, H, D), cu8, d_lab)
            else:
                _label_stats(d_col, (W, H, D), cu8, d_lab, cap=1024, members_only=False)
            crop_fn = lib.pb3d_crop_occupancy_dev if label is None else lib.pb3d_crop_occupancy_label_dev
            paste_fn = lib.pb3d_component_paste_dev if label is None else lib.pb3d_component_paste_label_dev
            d_carved = sc.result(None, nbytes)
            _lib.check(lib.pb3d_d2d(ctx, C.c_void_p(d_carved.ptr), C.c_void_p(d_col.ptr), nbytes))
            vmax = int(max((b[3] - b[0]) * (b[4] - b[1]) * (b[5] - b[2]) for b in bbox))
            d_m = sc.upload(packed)
            d_occ = sc.alloc(vmax); d_out = sc.alloc(vmax); d_tmp = sc.alloc(vmax)
            d_cnt = sc.alloc(8 * num); d_cnt.zero()
            for i in range(1, num + 1):
                x0, y0, z0, x1, y1, z1 = (int(v) for v in bbox[i - 1])
                Wc, Hc, Dc = x1 - x0, y1 - y0, z1 - z0
                lo = (C.c_int64 * 3)(x0, y0, z0); hi = (C.c_int64 * 3)(x1, y1, z1)
                _lib.check(crop_fn(ctx, C.c_void_p(d_col.ptr), W, H, D, lo, hi, C.c_void_p(d_occ.ptr)))
                if angle < 0:
                    src = d_occ     # empty angle loop: the crop's occupancy is returned as is
                else:
                    dev.process_grid(d_occ, Wc, Hc, Dc, d_m.at(int(offs[i - 1])), int(min(angle, 91)), d_out, d_tmp)
                    src = d_out
                _lib.check(lib.pb3d_count_nonzero_dev(ctx, C.c_void_p(src.ptr), Wc * Hc * Dc, d_cnt.at(8 * (i - 1))))
                _lib.check(paste_fn(ctx, C.c_void_p(d_col.ptr), C.c_void_p(d_lab.ptr), i, C.c_void_p(src.ptr), W, H, D, lo, hi, C.c_void_p(d_carved.ptr)))
            counts = d_cnt.download((num,), np.int64)
        print("\n".join(_component_log(num, bbox, counts)))
        dev.sync()
        return d_carved if d_carved is not None else d_col


def _pack_crop_masks(mask2d, bbox):
    """every component's 2-D crop mask (reference :189) in one byte string: (packed, offsets)"""
    masks, offs, o = [], [], 0
    for b in bbox:
        x0, y0, z0, x1, y1, z1 = (int(v) for v in b)
        m = _lib.truth_u8(_mask_to_wh(mask2d[y0:y1, x0:x1], x1 - x0, y1 - y0))
        masks.append(np.ascontiguousarray(m).reshape(-1)); offs.append(o); o += (m.size + 15) & ~15
    packed = np.zeros(max(o, 16), np.uint8)
    for m, off in zip(masks, offs):
        packed[off:off + m.size] = m
    return packed, np.asarray(offs, np.int64)


def _component_log(num, bbox, counts):
    lines = []
    for i in range(1, num + 1):
        x0, y0, z0, x1, y1, z1 = (int(v) for v in bbox[i - 1])
        lines.append(f"  - Component {i}: bbox ({x0},{y0},{z0}) → ({x1},{y1},{z1})")
        lines.append(f"    carved voxels: {int(counts[i - 1])}")
    return lines


class _GuidedParts:
    """left_right_guided_carve for SEVERAL part colours of one grid (the loop of reference :338-346) behind ONE labelling.

    left_right_guided_carve(colour c) only ever clears or restores voxels of colour c (:199-201), so the membership of every OTHER
    colour -- and with it the components, their numbering and their boxes -- is what it was before the loop started: all part colours
    are labelled together on the grid part_carve left (pb3d_label_colors_stats_dev: the grid is read once, ONE host round trip), the
    component loops of all parts are queued behind it in the reference's order (each crop's occupancy is taken from the grid as the
    parts before it left it, like upstream), and the "carved voxels" counts of the printed log come back once, at the end, together
    with the status words of whatever the caller queues behind (the recolouring).  The log text is upstream's, line for line; it is
    emitted by finish()."""
    CAP = 8192          # components whose counts one log buffer holds

    def __init__(self, d_grid, shape3, parts, d_lab, channels=3):
        """parts: list of (printed colour, mask2d (H,W) bool, angle, key) -- key = 3 uint8 (colour grid) or an int label value
        (label volume), None if the colour cannot occur in a uint8 grid."""
        self.dev, self.d_grid, self.shape3, self.d_lab, self.channels = dev, d_grid, shape3, d_lab, channels
        self.items = []           # ("text", line) | ("part", printed colour, num, bbox, offset into the counts)
        self.d_log = dev.DeviceBuffer(8 * (self.CAP + 2))
        self.parts = list(parts)
        self.used = 0

    def status_ptr(self):
        """two device int64 behind the counts: pb3d_recolor_backward_dev's status words come back with the log"""
        return self.d_log.at(8 * self.CAP)

    def _one_by_one(self, d_cur, part):
        target, mask2d, angle, key = part
        d_new = _lrgc_dev(d_cur, self.shape3, mask2d, target, angle, label=None if self.channels == 3 else key, d_lab=self.d_lab)
        if d_new is not d_cur and d_cur is not self.d_grid:
            d_cur.free()            # (a copy an earlier fallback made; the caller's buffer stays the caller's)
        return d_new

    def run(self):
        """queue every part; returns the DeviceBuffer that holds the grid afterwards (d_grid unless a fallback copied it)"""
        lib, ctx = _lib.load(), _lib.ctx()
        W, H, D = self.shape3
        work = [p for p in self.parts if p[1] is not None and np.any(p[1]) and p[3] is not None]
        keys = [(int(p[3]) if isinstance(p[3], (int, np.integer)) else tuple(int(v) for v in p[3])) for p in work]
        one_by_one = len(set(keys)) != len(keys)          # a colour named twice: its second carve sees what the first one left
        groups = [work[i:i + 8] for i in range(0, len(work), 8)]
        where = {}                  # id(part) -> (colour index in its labelling, (n, bbox, count, sums) or None)
        d_cur = self.d_grid
        for part in self.parts:
            target, mask2d, angle, key = part
            if mask2d is None or not np.any(mask2d):
                self.items.append(("text", f"[SKIP] No mask for color {target}"))
                continue
            if one_by_one:
                self.flush()
                d_cur = self._one_by_one(d_cur, part)
                continue
            if key is None:
                self.items.append(("text", f"[{target}] 3D components: 0"))
                continue
            if id(part) not in where:        # the next group of (at most eight) colours: one labelling for all of them
                grp = next(g for g in groups if any(q is part for q in g))
                res = _label_stats_multi(d_cur, (W, H, D), [q[3] for q in grp], self.d_lab, cap=1024, members_only=True)
                for k, q in enumerate(grp):
                    where[id(q)] = (k, res[k])
            k, r = where[id(part)]
            queued = False
            if r is not None and r[0] == 0:
                self.items.append(("text", f"[{target}] 3D components: 0"))
                queued = True
            elif r is not None:
                num, bbox = r[0], r[1]
                if isinstance(angle, (bool, np.bool_)) or not isinstance(angle, (int, np.integer)) or angle == 0:
                    self.items.append(("text", f"[{target}] 3D components: {num}"))
                    self.flush()
                    _check_angle_step(angle)        # raises what upstream's range() raises
                if angle > 0 and self.used + num <= self.CAP:
                    packed, offs = _pack_crop_masks(mask2d, bbox)
                    bb = np.ascontiguousarray(bbox, np.int64)
                    took = C.c_int(0)
                    _lib.check(lib.pb3d_guided_carve_queue_dev(ctx, C.c_void_p(d_cur.ptr), C.c_void_p(self.d_lab.ptr), k, self.channels, W, H, D, num,
                                                               bb.ctypes.data_as(_lib.i64p), _lib.p_u8(packed), offs.ctypes.data_as(_lib.i64p), packed.size,
                                                               int(min(angle, 91)), self.d_log.at(8 * self.used), C.byref(took)))
                    if took.value:
                        self.items.append(("part", target, num, bbox, self.used))
                        self.used += num
                        queued = True
            if not queued:
                # more components than the statistics hold, an empty angle loop, or a crop too large for the LDS-resident chain: this part and
                # the ones after it go one by one (their labellings would overwrite the shared one)
                self.flush()
                one_by_one = True
                d_cur = self._one_by_one(d_cur, part)
        return d_cur

    def _emit(self, log):
        lines = []
        for it in self.items:
            if it[0] == "text":
                lines.append(it[1])
            else:
                _, target, num, bbox, off = it
                lines.append(f"[{target}] 3D components: {num}")
                lines += _component_log(num, bbox, log[off:off + num])
        if lines:
            print("\n".join(lines))
        self.items = []

    def flush(self):
        """emit the log collected so far (waits for the device when a queued part's counts are still there)"""
        log = self.d_log.download((self.used,), np.int64) if any(it[0] == "part" for it in self.items) else None
        self._emit(log)

    def finish(self, with_status=False):
        """ONE download: the counts of every queued part (+ the two status words behind them); emits the log; returns the status"""
        if not with_status:
            self.flush()
            return None
        log = self.d_log.download((self.CAP + 2,), np.int64)
        self._emit(log)
        return log[self.CAP:]

    def free(self):
        if self.d_log is not None:
            self.d_log.free(); self.d_log = None


def left_right_guided_carve(colored_grid, semantic_mask, target_color, angle=60, visualize=False, stride=2):
    """Per 3-D connected component of `target_color`: crop its bounding box, rotate-and-carve the crop's
    occupancy with the part's own angle step against the cropped 2-D mask, clear the component and paste
    what survives; reference :163-210 (prints kept: they are notebook output)."""
    g = _lib.as_u8(colored_grid, "colored_grid")
    if g.ndim != 4 or g.shape[3] != 3:
        raise ValueError("not enough values to unpack (expected 4, got %d)" % g.ndim)
    W, H, D, _ = g.shape
    sm2 = np.asarray(semantic_mask)
    mask2d = _is_color(sm2, _color_key(sm2), target_color)
    if not np.any(mask2d):
        print(f"[SKIP] No mask for color {target_color}")
        return g.copy()
    with dev.Scope() as sc:
        d_col = sc.upload(g) or sc.alloc(0)
        d_carved = _lrgc_dev(d_col, (W, H, D), mask2d, target_color, angle)
        if d_carved is not d_col:
            sc.adopt(d_carved)
        return d_carved.download(g.shape)


def _extrude_args(shape3, mask_2d, axis, direction):
    W, H, D = shape3
    if direction not in ("+", "-"):
        raise ValueError("direction must be '+' or '-'")
    m = np.asarray(mask_2d)
    if axis == 2:
        valid, vw = m.T, H
        if valid.shape != (W, H):
            raise ValueError(f"operands could not be broadcast together with shapes ({W},{H}) {valid.shape}")
    else:
        valid, vw = m, D
        if valid.shape != (H, D):
            raise ValueError(f"operands could not be broadcast together with shapes ({H},{D}) {valid.shape}")
    return _lib.truth_u8(valid), vw


def _extrude_dev(d_in, d_out, shape3, valid_u8, vw, axis, direction, depth, fill_color, d_valid=None, label=False):
    """one extrusion on device buffers; d_out may be d_in (in place).  d_valid: the mask already on the device (a chain of calls
    with one mask uploads it once); the call only queues work."""
    W, H, D = shape3
    fc = None if (fill_color is None or label) else np.ascontiguousarray(np.asarray(fill_color).astype(np.uint8).reshape(3))
    with dev.Scope() as sc:     # (a mask uploaded here goes back to the context's pool; the stream is in order)
        d_v = d_valid if d_valid is not None else sc.upload(valid_u8) or sc.alloc(0)
        if label:       # 1-byte label volume: fill_color is the label value (None clears)
            _lib.check(_lib.load().pb3d_extrude_label_dev(_lib.ctx(), C.c_void_p(d_in.ptr), W, H, D, C.c_void_p(d_v.ptr), vw, int(axis),
                                                          1 if direction == "+" else 0, int(depth), -1 if fill_color is None else int(fill_color),
                                                          C.c_void_p(d_out.ptr)))
            return
        _lib.check(_lib.load().pb3d_extrude_dev(_lib.ctx(), C.c_void_p(d_in.ptr), W, H, D, C.c_void_p(d_v.ptr), vw, int(axis),
                                                1 if direction == "+" else 0, int(depth), None if fc is None else _lib.p_u8(fc),
                                                C.c_void_p(d_out.ptr)))


def extrude_from_surface(grid, mask_2d, axis, direction="+", depth=5, fill_color=None):
    """From the first occupied voxel along `axis` (seen from the `direction` side) paint `depth` cells
    where the 2-D mask allows; reference :213-248 (an empty column starts at index 0, like np.argmax)."""
    g = _lib.as_u8(grid, "grid")
    if g.ndim != 4 or g.shape[3] != 3:
        raise ValueError("extrude_from_surface expects a (W,H,D,3) grid")
    W, H, D, _ = g.shape
    if axis not in (0, 2) or int(depth) <= 0:
        return g.copy()
    vt, vw = _extrude_args((W, H, D), mask_2d, axis, direction)
    with dev.Scope() as sc:
        d_in = sc.upload(g) or sc.alloc(0); d_out = sc.alloc(g.size)
        _extrude_dev(d_in, d_out, (W, H, D), vt, vw, axis, direction, depth, fill_color)
        return d_out.download(g.shape)


def _recolor_dev(d_g, shape3, color, new_color, k, sort_axis, label=False):
    """recolor_backward_components in place on a device-resident (A0,A1,A2,3) grid."""
    A0, A1, A2 = shape3
    cu8 = int(color) if label else _color_u8(color)
    if cu8 is None or A0 * A1 * A2 == 0:
        return
    with dev.Scope() as sc:
        d_lab = sc.alloc(A0 * A1 * A2 * 4)
        n, _, cnt, sums = _label_stats(d_g, (A0, A1, A2), cu8, d_lab, members_only=True)
        if n == 0:
            return
        means = [(i + 1, sums[i, sort_axis] / cnt[i]) for i in range(n)]        # np.mean of an int64 column
        keep = {i for i, _ in sorted(means, key=lambda t: t[1])[:k]}
        flags = np.array([0 if (i + 1) in keep else 1 for i in range(n)], np.uint8)
        # d_lab is what the labelling just wrote: the recolouring walks its membership bits (pb3d_recolor_last_labelled_dev)
        nc = np.array([int(new_color), 0, 0], np.uint8) if label else np.ascontiguousarray(np.asarray(new_color).astype(np.uint8).reshape(3))
        _lib.check(_lib.load().pb3d_recolor_last_labelled_dev(_lib.ctx(), C.c_void_p(d_lab.ptr), A0 * A1 * A2, _lib.p_u8(flags), n,
                                                              _lib.p_u8(nc), C.c_void_p(d_g.ptr), 1 if label else 3))
        dev.sync()


def recolor_backward_components(voxel_grid, color, new_color, k=4, sort_axis=2):
    """Keep the k components of `color` with the smallest mean coordinate on sort_axis, recolour the rest;
    reference :252-266.  Returns a C-contiguous copy (the input is usually a transposed/flipped view)."""
    g = np.ascontiguousarray(_lib.as_u8(voxel_grid, "voxel_grid"))
    if g.ndim != 4 or g.shape[3] != 3:
        raise ValueError("recolor_backward_components expects an (A0,A1,A2,3) grid")
    if g.size == 0:
        return g.copy()
    with dev.Scope() as sc:
        d_g = sc.upload(g)
        d_lab = sc.alloc(g.size // 3 * 4); d_st = sc.alloc(16)
        # labelling, keep decision and painting on the device (pb3d_recolor_backward_dev); the host decides for scenes with more
        # components than that entry takes
        if _recolor_queue(d_g, g.shape[:3], color, new_color, k, sort_axis, d_lab, C.c_void_p(d_st.ptr)) and d_st.download((2,), np.int64)[1]:
            _recolor_dev(d_g, g.shape[:3], color, new_color, k, sort_axis)
        return d_g.download(g.shape)


def _recolor_queue(d_g, shape3, color, new_color, k, sort_axis, d_lab, d_status, label=False):
    """recolor_backward_components queued on the device without a host wait (pb3d_recolor_backward_dev); False if nothing was queued"""
    A0, A1, A2 = shape3
    cu8 = int(color) if label else _color_u8(color)
    if cu8 is None or A0 * A1 * A2 == 0:
        return False
    c3 = np.array([cu8, 0, 0], np.uint8) if label else cu8
    nc = np.array([int(new_color), 0, 0], np.uint8) if label else np.ascontiguousarray(np.asarray(new_color).astype(np.uint8).reshape(3))
    _lib.check(_lib.load().pb3d_recolor_backward_dev(_lib.ctx(), C.c_void_p(d_g.ptr), A0, A1, A2, _lib.p_u8(c3), _lib.p_u8(nc), int(k), int(sort_axis),
                                                     1 if label else 3, C.c_void_p(d_lab.ptr), d_status))
    return True


def partwise_carve(colored_voxel_grid, semantic_mask_exterior, semantic_mask_full, part_colors_np, group_jobs, part_symmetry,
                   extrusion_depths, recolor_back_minarets=True, visualize=False, stride=4):
    """Part-wise refinement after global carving; reference :302-400.  Returns (D,H,W,3) when the
    back-minaret recolouring runs (transposed + flipped, as upstream), else (W,H,D,3).
    The grid stays resident in HBM from the first stage to the last (one upload, one download) and the host waits for the device
    TWICE: for the component boxes of all part colours (one labelling) and for the finished grid -- the printed log (upstream's text,
    line for line) is emitted at the end.  Only with visualize=True are intermediate grids brought back for plotting."""
    resident = isinstance(colored_voxel_grid, dev.DeviceGrid)     # then the result is a DeviceGrid too (the input stays the caller's)
    g = colored_voxel_grid if resident else _lib.as_u8(colored_voxel_grid, "colored_voxel_grid")
    if len(g.shape) != 4 or g.shape[3] != 3:
        raise ValueError("colored_voxel_grid must be (W,H,D,3)")
    W, H, D, _ = g.shape
    lib, ctx = _lib.load(), _lib.ctx()

    def show(d_buf, shape, title):
        if visualize and plot_voxel is not None:
            from .voxel_utils import voxel_grid_to_points
            pts, cols, _ = voxel_grid_to_points(d_buf.download(shape), stride=stride)
            if pts.shape[0] > 0:
                plot_voxel(pts, cols, title=title)

    # 1. global symmetry per part group
    msub, mcarve, angles, skip = _job_masks(semantic_mask_exterior, group_jobs, W, H, PART_COLORS)
    for j in range(len(group_jobs)):
        if not skip[j] and angles[j] <= 0:
            raise ValueError("range() arg 3 must not be zero" if angles[j] == 0 else "negative angle steps are not supported")
        angles[j] = min(angles[j], 91) if angles[j] > 0 else angles[j]
    nb = int(np.prod(g.shape, dtype=np.int64))
    with dev.Scope() as sc:
        d_in = sc.alloc(nb) if resident else sc.upload(g) or sc.alloc(0)       # scratch later on; a resident input is only read
        d_a = sc.alloc(nb)
        d_ms = sc.upload(msub, wait=False) or sc.alloc(0); d_mc = sc.upload(mcarve, wait=False) or sc.alloc(0)
        _lib.check(lib.pb3d_part_carve_dev(ctx, C.c_void_p(g.buf.ptr if resident else d_in.ptr), W, H, D, C.c_void_p(d_ms.ptr), C.c_void_p(d_mc.ptr), angles, skip,
                                           len(group_jobs), C.c_void_p(d_a.ptr)))
        show(d_a, tuple(g.shape), "After part-wise symmetric carving (global symmetry on each part)")
        # 2. component-guided symmetry: ONE labelling for all part colours, the component loops queued behind it
        sm_ext = np.asarray(semantic_mask_exterior)
        key_ext = _color_key(sm_ext)
        d_lab = sc.alloc(W * H * D * 4)
        parts = []
        for part, angle in part_symmetry.items():
            target = part_colors_np[part]
            parts.append((target, _is_color(sm_ext, key_ext, target), angle, _color_u8(target)))
        guided = sc.adopt(_GuidedParts(d_a, (W, H, D), parts, d_lab))
        d_b = guided.run()
        if d_b is not d_a:          # (a part that went component by component works on a copy)
            sc.adopt(d_b)
            sc.free(d_a)
            d_a = d_b
        show(d_a, g.shape, "After part-wise symmetric carving (local symmetry on each part)")
        # 3. interior extrusion: four directions per part, IN PLACE (a column is scanned and painted by one wavefront / thread), the
        #    part's mask uploaded once per axis orientation (staged: no host wait)
        d_b = d_in          # the input copy is no longer needed (the orientation stage below writes into it)
        sm_full = np.asarray(semantic_mask_full)
        key_full = _color_key(sm_full)
        for part, depth in extrusion_depths.items():
            if int(depth) <= 0:
                continue
            mask = _is_color(sm_full, key_full, part_colors_np[part])
            for axis in (2, 0):
                vt, vw = _extrude_args((W, H, D), mask, axis, "+")
                d_v = sc.upload(vt, wait=False) or sc.alloc(0)
                for direction in ("+", "-"):
                    _extrude_dev(d_a, d_a, (W, H, D), vt, vw, axis, direction, depth, part_colors_np[part], d_valid=d_v)
                sc.free(d_v)
        show(d_a, g.shape, "After interior extrusion")
        # 4. orientation + back-minaret recolouring (labelling, keep decision and painting all on the device)
        if recolor_back_minarets:
            _lib.check(lib.pb3d_orient_dev(ctx, C.c_void_p(d_a.ptr), W, H, D, C.c_void_p(d_b.ptr)))
            queued = _recolor_queue(d_b, (D, H, W), part_colors_np["front_minarets"], part_colors_np["back_minarets"], 2, 0, d_lab, guided.status_ptr())
            status = guided.finish(with_status=queued)          # the second (and last) wait: the log's counts + the recolouring's status
            if queued and status[1]:
                # more components than the device decides on: the host path (nothing was painted)
                _recolor_dev(d_b, (D, H, W), part_colors_np["front_minarets"], part_colors_np["back_minarets"], 2, 0)
            show(d_b, (D, H, W, 3), "After back-minaret recoloring")
            if resident:
                return dev.DeviceGrid(sc.keep(d_b), (D, H, W, 3))
            return d_b.download((D, H, W, 3))
        guided.finish()
        if resident:
            return dev.DeviceGrid(sc.keep(d_a), tuple(g.shape))
        return d_a.download(g.shape)
