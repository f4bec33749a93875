"""Grid -> points (ordered stream compaction on the device) and the top-k component filter; host mirror of
reference utils/voxel_utils.py:7-51."""
import ctypes as C

import numpy as np

from . import _hostmem, _lib, device as dev, voxel_carving_utils as vcu

__all__ = ["get_voxel_points_by_parts", "extract_top_k_components", "voxel_grid_to_points", "meshify_colored_voxel_grid"]

_RECORDS_MAX = 16384        # statistics records a single-colour labelling keeps (csrc/ccl.hip)


def _compact(grid, colors, stride):
    g = _lib.as_u8(grid, "grid")
    A0, A1, A2 = g.shape[:3]
    Cc = g.shape[3] if g.ndim == 4 else 1
    if colors is not None and len(colors):
        cols = np.ascontiguousarray(np.asarray(colors, np.int64).reshape(-1, 3))
        # a palette entry outside 0..255 can never equal a uint8 voxel
        ok = np.all((cols >= 0) & (cols <= 255), axis=1)
        cols = np.ascontiguousarray(cols[ok].astype(np.uint8))
        if len(cols) == 0:
            return np.zeros((0, 3), np.float32), np.zeros((0, Cc), np.uint8)
        if len(cols) > 32:
            raise ValueError("at most 32 part colours per call")
        cptr, nc = _lib.p_u8(cols), len(cols)
    else:
        cptr, nc = None, 0
    lib, ctx = _lib.load(), _lib.ctx()
    n = C.c_int64(0)
    _lib.check(lib.pb3d_points_count(ctx, _lib.p_u8(g), A0, A1, A2, Cc, cptr, nc, int(stride), C.byref(n)))
    pts = _hostmem.empty((n.value, 3), np.float32)
    pc = _hostmem.empty((n.value, Cc), np.uint8)
    _lib.check(lib.pb3d_points_fill(ctx, n.value, pts.ctypes.data_as(C.POINTER(C.c_float)), _lib.p_u8(pc)))
    return pts, pc


def get_voxel_points_by_parts(grid, part_colors, part_names):
    """Points (x,y,z) = (a2,a1,a0) float32 and colours of every voxel whose RGB equals one of the
    named parts' colours, in numpy.where order; reference :7-21."""
    grid = np.asarray(grid)
    if grid.ndim != 4 or grid.shape[3] != 3:
        raise ValueError("grid must be (A0,A1,A2,3)")
    cols = [part_colors[name] for name in part_names]
    if not cols:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8)
    return _compact(grid, cols, 1)


def voxel_grid_to_points(grid, axis="z", colormap="viridis", stride=2):
    """Occupied voxels on the [::stride] lattice as points*stride (+ colours); reference :35-51.
    Returns (pts, colors, (H, W, D))."""
    grid = np.asarray(grid)
    W, H, D = grid.shape[:3]
    is_color = grid.ndim == 4 and grid.shape[3] == 3
    if grid.ndim == 4 and not is_color:
        raise ValueError("too many values to unpack (expected 3)")
    pts, pc = _compact(grid, None, stride)
    if is_color:
        return pts, pc, (H, W, D)
    # occupancy grids are coloured by a matplotlib colormap along one axis (visualisation only)
    import matplotlib.pyplot as plt
    xs, ys, zs = (pts[:, k] / np.float32(stride) for k in range(3))
    with np.errstate(divide="ignore", invalid="ignore"):
        vals = {"x": xs, "y": ys, "z": zs}[axis].astype(np.int64) / {"x": W - 1, "y": H - 1, "z": D - 1}[axis]
    colors = (plt.get_cmap(colormap)(vals)[:, :3] * 255).astype(np.uint8)
    return pts, colors, (H, W, D)


# ---- extract_top_k_components (reference :24-33): 26-connected components of one colour, ranked by height ---------------------------
def _label_stats_conn(d_grid, shape3, colors, d_labels, connectivity, cap=1024, members_only=False, channels=3):
    """The components of up to eight colours (channels = 3: 3-byte colours; 1: label values of a 1-byte volume) at 6-, 18- or
    26-connectivity (pb3d_label_colors_conn_stats_dev).  Returns (n, bbox, count, sums) per colour; bbox/count/sums are None for a
    colour with more than the records hold (pb3d_component_stats_dev on a full labelling gives them)."""
    A0, A1, A2 = shape3
    K = len(colors)
    cols = np.ascontiguousarray(np.asarray(colors, np.uint8).reshape(K, channels))
    n = (C.c_int64 * K)(); ok = (C.c_int * K)()
    bbox = np.zeros((K, cap, 6), np.int64); cnt = np.zeros((K, cap), np.int64); sums = np.zeros((K, cap, 3), np.int64)
    _lib.check(_lib.load().pb3d_label_colors_conn_stats_dev(_lib.ctx(), C.c_void_p(d_grid.ptr), A0, A1, A2, _lib.p_u8(cols), K, channels,
                                                            int(connectivity), C.c_void_p(d_labels.ptr), n, cap, 1 if members_only else 0,
                                                            bbox.ctypes.data_as(_lib.i64p), cnt.ctypes.data_as(_lib.i64p),
                                                            sums.ctypes.data_as(_lib.i64p), ok))
    return [(n[k], bbox[k, :n[k]], cnt[k, :n[k]], sums[k, :n[k]]) if ok[k] else (n[k], None, None, None) for k in range(K)]


def _top_k_dev(d_g, shape3, value, k, channels):
    """extract_top_k_components in place on a device buffer; value: 3 uint8 (channels = 3) or a label value (channels = 1)."""
    A0, A1, A2 = shape3
    if A0 * A1 * A2 == 0:
        return
    c3 = np.array([value, 0, 0], np.uint8) if channels == 1 else np.ascontiguousarray(value)
    kk = max(min(int(k), 1 << 62), -(1 << 62))           # any Python int: [:k] of fewer than 2^31 components
    lib, ctx = _lib.load(), _lib.ctx()
    with dev.Scope() as sc:
        d_lab = sc.alloc(A0 * A1 * A2 * 4); d_st = sc.alloc(16)
        # labelling, ranking and zeroing on the device (pb3d_top_k_components_dev); the host decides when the records overflow
        _lib.check(lib.pb3d_top_k_components_dev(ctx, C.c_void_p(d_g.ptr), A0, A1, A2, _lib.p_u8(c3), channels, kk, 26, C.c_void_p(d_lab.ptr),
                                                 C.c_void_p(d_st.ptr)))
        n, over = (int(v) for v in d_st.download((2,), np.int64))
        if not over or n == 0:
            return
        # (more components than the device records hold: nothing was zeroed) -- a full labelling, its statistics, the choice here
        col = [value] if channels == 1 else [c3]
        n, bbox, _, _ = _label_stats_conn(d_g, shape3, col, d_lab, 26, cap=min(n, _RECORDS_MAX), members_only=False, channels=channels)[0]
        if bbox is None:
            bbox = vcu._component_stats(d_lab, shape3, n)[0]
        heights = bbox[:, 4] - 1 - bbox[:, 1]
        top = sorted(range(n), key=lambda i: -heights[i])[:kk]
        flags = np.ones(n, np.uint8)
        flags[np.asarray(top, np.int64)] = 0
        zero = np.zeros(3, np.uint8)
        _lib.check(lib.pb3d_recolor_last_labelled_dev(ctx, C.c_void_p(d_lab.ptr), A0 * A1 * A2, _lib.p_u8(flags), n, _lib.p_u8(zero),
                                                      C.c_void_p(d_g.ptr), channels))
        dev.sync()


def extract_top_k_components(voxel_grid, color, k=4):
    """Keep the k tallest 26-connected components of `color` (height = extent along axis 1; equal heights in label order), zero the
    other voxels of that colour; reference :24-33.  Returns a new C-contiguous uint8 array (the input is not changed), or a new
    pb3d.device.DeviceGrid for a resident grid (the input stays the caller's)."""
    resident = isinstance(voxel_grid, dev.DeviceGrid)
    g = voxel_grid if resident else _lib.as_u8(voxel_grid, "voxel_grid")
    if len(g.shape) != 4 or g.shape[3] != 3:
        raise ValueError("extract_top_k_components expects an (A0,A1,A2,3) grid")
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)):
        raise TypeError("k must be an integer")
    cu8 = vcu._color_u8(color)
    shape3 = tuple(int(v) for v in g.shape[:3])
    nbytes = int(np.prod(g.shape, dtype=np.int64))
    if not resident and (cu8 is None or g.size == 0):       # a colour that no uint8 voxel can equal: nothing is a member
        return np.ascontiguousarray(g).copy()
    with dev.Scope() as sc:
        if resident:
            d_out = sc.result(None, nbytes)
            if nbytes:
                _lib.check(_lib.load().pb3d_d2d(_lib.ctx(), C.c_void_p(d_out.ptr), C.c_void_p(g.buf.ptr), nbytes))
            if cu8 is not None:
                _top_k_dev(d_out, shape3, cu8, k, 3)
            return dev.DeviceGrid(d_out, g.shape)
        d_g = sc.upload(g)
        _top_k_dev(d_g, shape3, cu8, k, 3)
        return d_g.download(g.shape)


# ---- meshify_colored_voxel_grid (reference :53-96): binary marching cubes + nearest-filled-voxel colours (csrc/mesh.hip) ----------
def mesh_check(shape, stride):
    """The reference's argument errors, raised before any device work: stride >= 1 and a lattice grid[::stride, ::stride, ::stride]
    of at least 2 on every axis (skimage: "Input array must be at least 2x2x2.")."""
    stride = int(stride)
    if stride < 1:
        raise ValueError("stride must be >= 1")
    if any(-(-int(n) // stride) < 2 for n in shape[:3]):
        raise ValueError("Input array must be at least 2x2x2.")
    return stride


def mesh_colors(cols):
    """The reference's colour rule: colour / 255.0 (float64) when any colour is > 1, the raw values otherwise."""
    if cols.size and cols.max() > 1:
        return cols / 255.0
    return cols


def _mesh_host(grid, channels, stride):
    """(verts, faces, normals, nearest-voxel bytes) of a uint8 (A0,A1,A2[,channels]) grid through pb3d_mesh_count / _fill."""
    A0, A1, A2 = grid.shape[:3]
    lib, ctx = _lib.load(), _lib.ctx()
    nv, nf = C.c_int64(0), C.c_int64(0)
    _lib.check(lib.pb3d_mesh_count(ctx, _lib.p_u8(grid), A0, A1, A2, channels, stride, C.byref(nv), C.byref(nf)))
    if nv.value == 0:
        # an all-empty or all-full lattice: skimage refuses level 0.5
        raise ValueError("Surface level must be within volume data range.")
    verts = _hostmem.empty((nv.value, 3), np.float32)
    faces = _hostmem.empty((nf.value, 3), np.int32)
    normals = _hostmem.empty((nv.value, 3), np.float32)
    cols = _hostmem.empty((nv.value, channels), np.uint8)
    _lib.check(lib.pb3d_mesh_fill(ctx, nv.value, nf.value, verts.ctypes.data_as(C.c_void_p), faces.ctypes.data_as(C.c_void_p),
                                  normals.ctypes.data_as(C.c_void_p), cols.ctypes.data_as(C.c_void_p)))
    return verts, faces, normals, cols


def meshify_colored_voxel_grid(colored_voxel_grid, stride=1):
    """Surface mesh of the occupied voxels (any channel > 0) of grid[::stride, ::stride, ::stride] with per-vertex colours;
    reference :53-96.  Returns (verts float32 (x, y, z) = (s*a2, s*a1, shape[2] - s*a0), faces int32, vertex_colors, normals
    float32 in skimage's (a0, a1, a2) order): the mesh skimage's Lewiner marching cubes builds at level 0.5, vertex for vertex
    and face for face, and each vertex coloured by its nearest occupied lattice voxel (the reference's mirrored query).
    vertex_colors is colour / 255.0 (float64) when any returned colour is > 1, else the raw uint8 values.
    The grid must be uint8 (A0, A1, A2, C) with C = 1 or 3 (TypeError otherwise); the device reads the lattice in place."""
    g = np.asarray(colored_voxel_grid)
    if g.ndim != 4:
        raise ValueError("colored_voxel_grid must be (A0, A1, A2, C)")
    stride = mesh_check(g.shape, stride)
    if g.dtype != np.uint8 or g.shape[3] not in (1, 3):
        raise TypeError("meshify_colored_voxel_grid takes a uint8 (A0, A1, A2, 1 or 3) grid")
    verts, faces, normals, cols = _mesh_host(np.ascontiguousarray(g), g.shape[3], stride)
    return verts, faces, mesh_colors(cols), normals
