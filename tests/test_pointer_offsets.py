"""The *_dev entries of include/pb3d.h on buffers whose BASE is not where pb3d_dev_alloc put it.

A dozen host-side dispatchers pick a kernel, or a path inside one, from the low bits of a pointer; the rest of the suite
hands over 256-byte aligned allocations only, so only the aligned side of every such condition had ever run.  Here every
buffer of a call is a window into an arena: 256 guard bytes, the payload at 256 + offset, at least 256 guard bytes behind
it.  Input arenas are filled with 0xff (dirty slack: it may neither leak into a voxel nor trip the chain's 0/1 check),
output arenas with 0xA5.  Every case asserts

  * the payload equals the CPU oracle (or NumPy / SciPy where the entry's own test uses them) byte for byte -- the run at
    offset 0 is checked against the oracle like the others, never used as the expectation;
  * both guard zones of every output arena still hold 0xA5 and every input arena is unchanged;
  * after a refusal (PB3D_EINVAL) an aligned call of the same entry on the same context gives the oracle's bytes.

Offsets are multiples of the element size: any byte for uint8 buffers (1: nothing aligned, 4: dword but not 16, 16: 16
but not 128, 64), one and three elements for 4- and 8-byte element buffers.

What the kernels need, per pointer argument, from reading them (csrc/ = part-based-3d-reconstruction_amd/csrc/):

  carve_mask        grid / out: k_carve_tiles casts to 16-byte vectors -> only behind the aligned16 test (carve.hip:508); k_carve_flat
                    uses align-1 vector types, k_carve_bytes bytes.  mask: bytes.
  occupancy         k_occupancy16 behind carve.hip:536, else the byte kernel.
  color_apply       carved through align-1 vectors, out through store48_wave (align-1), rgb_hw3 bytes: any base.
  rotate_carve      90 degrees: every form reads through load_piece (align-1); WF / FLAT store aligned 16-byte pieces relative
                    to `out` and are chosen only for a 128-byte aligned out (rotate_tiled.hip:780); WIDE loads and stores aligned
                    vectors and needs in | out 16-byte aligned (:783); TILE / TILE_RAGGED store align-1.  Generic angle:
                    k_rotate_generic<PACK> stores a dword, only for a 4-byte aligned out (rotate.hip:103).  180 / 270 degrees:
                    k_rotate_perm is a dword kernel, chosen only for 4-byte aligned in | out (rotate_tiled.hip:729, refused at :791
                    otherwise); rotate_carve then takes the bit-sliced step (0/1 data) or k_rotate_generic (rotate.hip:122-129).
  process_grid      slice pass reads align-1 vectors, un-slice stores align-1; the sliced volume is scratch.  d_tmp: as out.
  global_carve      bin_hw / rgb_hw3 bytes; the colour stream stores align-1 vectors (bits90.hip) or bytes: any slab pointer.
  part_carve        the 16-voxel forms behind carve.hip:600 (aligned16 of colored | out), else byte kernels; masks bytes.
  label form        k_rgb_to_label / k_label_to_rgb moved 16-byte vectors through ALIGNED vector types on the caller's pointers
                    with no test in front: they now use the align-1 type like every other sweep (label.hip).  global_carve_label and
                    part_carve_label: the rows above with one byte per voxel (one apply routine, one job loop for both forms;
                    k_label_apply16 behind the aligned16 test of carve.hip:690); orient_label bytes.
  orient            k_orient128 behind components.hip:706, k_orient4 (dword casts) behind :716, else k_orient (bytes).
  points count/fill grid: 16-voxel forms behind points.hip:493; d_pts (float aligned) and d_cols (any byte): the wave-private fill
                    derives head and shift from the address (points.hip:336,341).  points_extract refuses a grid that is not
                    16-byte aligned (:610); synth_sem refuses an output that is not 4-byte aligned (synth.hip:115).
  top_k_components  the labelling reads the grid through an align-1 vector type (ccl.hip:62,108) and writes int32 labels through a
                    4-byte aligned one (:63); k_recolor_bits stores single bytes; d_status: two int64 by element.
  component_members grid bytes, int32 labels and int64 coordinates by element, 8-byte atomics on d_rows (int64 aligned), mask bytes.
  mesh              k_mesh_bits reads grid bytes into a scratch bitmask; verts / normals (float32), faces (int32) and the colour
                    bytes are stored element by element; mesh_colors reads float32 verts by element.
  guided_carve      (all four entries) k_crop_slice loads a voxel's three bytes as ONE dword through an align-1 type and switches to
                    byte loads by `v + 4 <= vol_end` (guided.hip:73): an address-keyed path at the volume's last voxel.  The scene's
                    large box ends there, so that voxel sits against the rear guard.  k_crop_chain clears single bytes in place; int32
                    labels by element (members only: the rest of the arena keeps its fill), the membership bits are scratch, the
                    queued entry's counts are 8-byte atomics on d_counts (int64 aligned).
  extrude, recolor_components, count_nonzero, partwise_iou, label_colors_conn_stats, color_presence
                    byte (grid) and element-typed (int32 labels, uint32 bitmap, int64 counters) accesses only; color_presence
                    reads dwords only behind pb3d_color_presence_dev's `vec` test.  k_extrude_x's 4-byte voxel load uses an align-1 type.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 256
IN_FILL, OUT_FILL = 0xFF, 0xA5
BYTE_OFFS = (1, 4, 16, 64)

# (in, out): the control, then in +0 / out +k, in +k / out +0, in +k / out +k' for every k, and both at +1
COMBOS = [(0, 0)] + [c for i, k in enumerate(BYTE_OFFS) for c in ((0, k), (k, 0), (k, BYTE_OFFS[(i + 1) % 4]))] + [(1, 1)]

# ---- the case table: entry -> (test function, rows of (shape, offset argument(s), branch the row is there for)) -----------------
CASES = {
    "pb3d_carve_mask_dev": ("test_carve_mask", [
        ("64x9x64 C=1,3", "grid, mask, out", "carve.hip:508 k_carve_tiles <-> k_carve_flat"),
        ("33x5x37 C=3", "grid, mask, out", "carve.hip:519 k_carve_flat (odd column)"),
        ("20x7x5 C=1,3", "grid, mask, out", "carve.hip:523 k_carve_bytes (col < 16)")]),
    "pb3d_occupancy_dev": ("test_occupancy", [("nvox 4096, 4099, 7", "rgb, occ", "carve.hip:536 k_occupancy16 + tail <-> tail only")]),
    "pb3d_color_apply_dev": ("test_color_apply", [("12x7x32, 12x7x37, 12x7x5", "carved, rgb, out", "carve.hip:686 pb3d_image_apply_dev (no pointer test: align-1 vectors)")]),
    "pb3d_rotate_carve_dev": ("test_rotate90_forms / test_rotate_generic_and_180", [
        ("355x128x355", "in, mask, out", "rotate_tiled.hip:780-781 WF <-> TILE_RAGGED"),
        ("131x256x131", "in, mask, out", "rotate_tiled.hip:780,782 FLAT <-> TILE_RAGGED"),
        ("256x4x256", "in, mask, out", "rotate_tiled.hip:783 WIDE <-> TILE"),
        ("128x5x128", "in, mask, out", "rotate_tiled.hip:785 TILE"),
        ("100x7x100", "in, mask, out", "rotate_tiled.hip:785 TILE_RAGGED"),
        ("48x9x52 at 45 and 30", "in, mask, out", "rotate.hip:103 packed stores <-> byte stores; rotate.hip:124 sliced step"),
        ("36x5x40 at 180", "in, mask, out", "rotate_tiled.hip:729,791 k_rotate_perm <-> rotate.hip:124-129 sliced step / k_rotate_generic")]),
    "pb3d_process_grid_dev": ("test_process_grid", [
        ("300x16x357, 128x9x128 at 90, 45, 5", "occ, mask, out, tmp", "sliced.hip slice / un-slice on offset bases; rotate_tiled.hip:780-785"),
        ("128x9x128 bytes at 45", "occ, mask, out, tmp", "rotate.hip:170-195 byte chain, rotate.hip:103")]),
    "pb3d_global_carve_dev": ("test_global_carve", [
        ("h 37, w 131 whole", "bin, rgb, out", "bits90.hip colour stream / sliced chain colour stores"),
        ("slabs [5,9) [4,20) [16,131)", "out (slab residue 1, 4, 0 mod 16)", "bits90.hip:303 slab pointer = start of the slab (90); global.hip:47 refusal of a slab at 45")]),
    "pb3d_part_carve_dev": ("test_part_carve", [("40x24x56, 41x24x56", "colored, masks, out", "carve.hip:600 16-voxel forms <-> byte kernels; rotate_tiled.hip:887 fused 90")]),
    "pb3d_rgb_to_label_dev": ("test_label_conversions", [("nvox 4096, 4099, 7", "rgb, label", "label.hip:67,88 (align-1 vectors)")]),
    "pb3d_label_to_rgb_dev": ("test_label_conversions", [("nvox 4096, 4099, 7", "label, rgb", "label.hip:106,124 (align-1 vectors)")]),
    "pb3d_global_carve_label_dev": ("test_global_carve_label", [("h 37, w 131 at 90 and 45", "bin, label_hw, out", "carve.hip:690 k_label_apply16 <-> k_color_apply_generic<1>")]),
    "pb3d_part_carve_label_dev": ("test_part_carve_label", [("40x24x48 mixed jobs", "label, masks, out", "carve.hip part_carve_jobs<1>: 16-voxel forms <-> byte kernels; rotate_tiled.hip fused 90")]),
    "pb3d_orient_label_dev": ("test_orient", [("70x5x66", "grid, out", "components.hip:696 (bytes)")]),
    "pb3d_orient_dev": ("test_orient", [
        ("128x3x128", "grid, out", "components.hip:706 k_orient128 <-> :716 k_orient4 <-> k_orient"),
        ("36x5x40", "grid, out", "components.hip:716 k_orient4 <-> k_orient"),
        ("33x5x37", "grid, out", "components.hip:719 k_orient")]),
    "pb3d_points_count_dev": ("test_points_count_fill", [("45x70x33 C=3, 51x18x77 C=1", "grid +1 / +4", "points.hip:493 16-voxel count <-> byte count")]),
    "pb3d_points_fill_dev": ("test_points_count_fill", [("45x70x33 C=3, 51x18x77 C=1", "grid; pts +4/+8/+12; cols +1/+2/+3", "points.hip:493; points.hip:336,341")]),
    "pb3d_points_extract_dev": ("test_refusals", [("32x16x32", "grid +1 / +4", "points.hip:610 refusal")]),
    "pb3d_synth_sem_dev": ("test_refusals", [("4x8x16", "out +1 / +2", "synth.hip:115 refusal")]),
    "pb3d_extrude_dev": ("test_extrude", [("21x13x18", "grid, valid, out; in place", "components.hip:724-746 (bytes, align-1 voxel load)")]),
    "pb3d_count_nonzero_dev": ("test_count_nonzero_partwise_iou", [("n 4099", "bytes; count +8 / +24", "components.hip:486")]),
    "pb3d_partwise_iou_dev": ("test_count_nonzero_partwise_iou", [("40x30", "a, b", "project.hip:433")]),
    "pb3d_color_presence_dev": ("test_color_presence", [("nvox 4096, 4099", "grid; bitmap +4 / +12; present +8 / +24", "pb3d_color_presence_dev's `vec` test: dword <-> byte reads")]),
    "pb3d_recolor_components_dev": ("test_labelling_and_recolor", [("24x10x27", "labels +4 / +12; grid", "components.hip:127")]),
    "pb3d_top_k_components_dev": ("test_top_k_components", [("20x24x45, k = 1, 4, -1", "grid in place; labels +4 / +12; status +8", "components.hip:658; ccl.hip:108 (align-1 grid reads), components.hip:144 k_recolor_bits")]),
    "pb3d_component_members_dev": ("test_component_members", [("12x10x27, three selections, all outputs", "grid; labels +4 / +12; coords +8 / +24; rows +8; masks +1 / +4 / +16", "members.hip:63,119 (bytes, int32 / int64 by element, 8-byte atomics on d_rows)")]),
    "pb3d_mesh_count_dev": ("test_mesh", [("13x11x9 stride 1, 17x19x16 stride 2", "grid +1 / +4 / +16 / +64", "mesh.hip:159 k_mesh_bits (bytes)")]),
    "pb3d_mesh_fill_dev": ("test_mesh", [("13x11x9 stride 1, 17x19x16 stride 2", "grid; verts / faces / normals +4 / +12; cols +1 / +2 / +3", "mesh.hip:497-507 (float32 / int32 by element)")]),
    "pb3d_mesh_colors_dev": ("test_mesh", [("13x11x9 stride 1, 17x19x16 stride 2", "grid; verts +4 / +12; cols +1 / +3", "mesh.hip:314 k_mesh_colors")]),
    "pb3d_label_colors_conn_stats_dev": ("test_labelling_and_recolor", [("24x10x27, 6 and 26 neighbours", "grid +1 / +4; labels +4 / +12", "ccl.hip (bytes, int32 labels)")]),
    "pb3d_guided_carve_dev": ("test_guided_carve", [("21x37x19 C=3, box ends at the last voxel", "grid in place; labels +4 / +12", "guided.hip:73 dword load <-> byte loads at the volume's last voxel")]),
    "pb3d_guided_carve_label_dev": ("test_guided_carve", [("21x37x19 C=1, box ends at the last voxel", "grid in place; labels +4 / +12", "guided.hip:72 byte loads, :201 one-byte clears")]),
    "pb3d_guided_carve_color_dev": ("test_guided_carve", [("21x37x19 C=3,1, colour index 0", "grid in place; labels +4 / +12", "guided.hip:73; the membership bits of a labelling made on the offset grid")]),
    "pb3d_guided_carve_queue_dev": ("test_guided_carve", [("21x37x19 C=3,1, colour index 0", "grid in place; labels +4 / +12; counts +8 / +24", "guided.hip:73; guided.hip:216 64-bit atomics on d_counts")]),
}

# every other *_dev entry, and why it is not in the table
EXEMPT = {
    "pb3d_project_dev": "point lists at byte offsets: tests/test_projection_edges.py::test_unaligned_ragged_point_lists",
    "pb3d_project_keys_dev": "point lists at byte offsets: test_unaligned_ragged_point_lists",
    "pb3d_depth_buffer_dev": "point lists at byte offsets: test_unaligned_ragged_point_lists",
    "pb3d_visible_mask_dev": "point lists at byte offsets: test_unaligned_ragged_point_lists",
    "pb3d_project_iou_batch_dev": "point lists at byte offsets: test_unaligned_ragged_point_lists",
    "pb3d_project_resolve_keys_dev": "uint64 key image, element accesses only (project.hip); its producer is covered by test_unaligned_ragged_point_lists",
    "pb3d_grid_depth_buffer_dev": "notebook-4 grid walk at byte offsets: tests/test_visibility_kernels.py::test_grid_walk_unaligned_and_medium",
    "pb3d_grid_visible_bits_dev": "notebook-4 grid walk at byte offsets: test_grid_walk_unaligned_and_medium",
    "pb3d_points_visible_bits_dev": "8- / 4-byte element point lists read element-wise (visibility.hip k_points_visible_bits); no address-keyed path",
    "pb3d_mask_bits_dev": "byte mask, uint32 outputs by element (visibility.hip); no address-keyed path",
    "pb3d_iou_rows_dev": "uint32 images and int64 counters by element (visibility.hip); no address-keyed path",
    "pb3d_points_bounds_dev": "4- / 8-byte element lists read element-wise (nn.hip); no address-keyed path",
    "pb3d_nn_dist_dev": "4- / 8-byte element lists read element-wise (nn.hip); no address-keyed path",
    "pb3d_knn_dev": "4- / 8-byte element lists read element-wise (nn.hip); no address-keyed path",
    "pb3d_voxel_iou_counts_dev": "4- / 8-byte element lists read element-wise (nn.hip); no address-keyed path",
    "pb3d_triangle_normals_dev": "vertex / face rows read element-wise (surface.hip); no address-keyed path",
    "pb3d_vertex_normals_dev": "vertex / face rows read element-wise (surface.hip); no address-keyed path",
    "pb3d_surface_metrics_dev": "float64 / int32 rows read element-wise (surface.hip); no address-keyed path",
    "pb3d_process_grid_typed_dev": "typed elements read and stored one by one (rotate_typed.hip); no address-keyed path",
    "pb3d_deform_iou_batch_dev": "float32 points read element-wise (deform.hip); no address-keyed path",
    "pb3d_deform_count_dev": "float32 points read element-wise (deform.hip); no address-keyed path",
    "pb3d_deform_fill_dev": "int64 rows stored element-wise (deform.hip); no address-keyed path",
    "pb3d_deform_paint_dev": "scatter of single bytes (deform.hip); no address-keyed path",
    "pb3d_scatter_colors_dev": "scatter of single bytes (deform.hip); no address-keyed path",
    "pb3d_label_color_dev": "the 6-connected labelling of ccl.hip: same kernels as pb3d_label_colors_conn_stats_dev, which is in the table",
    "pb3d_label_color_stats_dev": "same kernels as pb3d_label_colors_conn_stats_dev (ccl.hip)",
    "pb3d_label_colors_stats_dev": "same kernels as pb3d_label_colors_conn_stats_dev (ccl.hip)",
    "pb3d_label_value_stats_dev": "same kernels as pb3d_label_colors_conn_stats_dev with channels = 1 (ccl.hip)",
    "pb3d_label_values_stats_dev": "same kernels as pb3d_label_colors_conn_stats_dev with channels = 1 (ccl.hip)",
    "pb3d_component_stats_dev": "int32 labels read by element (components.hip k_comp_stats); no address-keyed path",
    "pb3d_crop_occupancy_dev": "byte accesses into a crop box (components.hip k_crop_occ); no address-keyed path",
    "pb3d_crop_occupancy_label_dev": "byte accesses into a crop box (components.hip k_crop_occ); no address-keyed path",
    "pb3d_component_paste_dev": "byte accesses into a crop box (components.hip k_comp_paste); no address-keyed path",
    "pb3d_component_paste_label_dev": "byte accesses into a crop box (components.hip k_comp_paste); no address-keyed path",
    "pb3d_recolor_backward_dev": "labelling of ccl.hip (in the table) + k_recolor_bits: byte stores, int32 labels by element",
    "pb3d_recolor_last_labelled_dev": "k_recolor_bits: byte stores, int32 labels by element (components.hip)",
    "pb3d_recolor_components_label_dev": "pb3d_recolor_components_dev with one channel (same kernel, in the table)",
    "pb3d_extrude_label_dev": "pb3d_extrude_dev with one channel (same kernels, in the table)",
    "pb3d_synth_mask16_dev": "generator with byte stores (synth.hip); no address-keyed path",
    "pb3d_synth_occ_dev": "generator with byte stores (synth.hip); no address-keyed path",
    "pb3d_allgather_dev": "RCCL: needs more than one GPU",
    "pb3d_carve_mask_sharded_dev": "RCCL: needs more than one GPU (its local half is pb3d_carve_mask_dev, in the table)",
    "pb3d_global_carve_sharded_dev": "RCCL: needs more than one GPU (its local half is pb3d_global_carve_dev's slab form, in the table)",
    "pb3d_carve_labels_sharded_dev": "RCCL: needs more than one GPU",
    "pb3d_allreduce_max_u64_dev": "RCCL: needs more than one GPU",
}


def test_every_dev_entry_is_decided():
    """every pb3d_*_dev prototype of include/pb3d.h is in the case table or in EXEMPT with a reason; none is in both"""
    text = open(os.path.join(ROOT, "include", "pb3d.h")).read()
    names = set(re.findall(r"^int\s+(pb3d_\w+_dev)\s*\(", text, re.M))
    assert len(names) > 60
    undecided = sorted(names - set(CASES) - set(EXEMPT))
    assert not undecided, f"new *_dev entries: add offset cases or an EXEMPT reason: {undecided}"
    assert not set(CASES) & set(EXEMPT)
    assert not (set(CASES) | set(EXEMPT)) - names, sorted((set(CASES) | set(EXEMPT)) - names)
    assert all(isinstance(r, str) and len(r) > 10 for r in EXEMPT.values())
    here = open(os.path.abspath(__file__)).read()
    for entry, (fn, rows) in CASES.items():
        assert rows and all(len(r) == 3 for r in rows), entry
        for f in fn.split(" / "):
            assert f"def {f}(" in here, (entry, f)


# =====================================================================================================================
# arenas
# =====================================================================================================================

class Arena:
    def __init__(self, pb3d, nbytes, off, fill, payload=None):
        self.off, self.n, self.fill = int(off), int(nbytes), fill
        total = GUARD + self.off + self.n + GUARD
        total += -total % 256
        self.buf = pb3d.device.DeviceBuffer(total)
        assert self.buf.ptr % 256 == 0
        self.host = np.full(total, fill, np.uint8)
        if payload is not None:
            p = np.ascontiguousarray(payload).view(np.uint8).reshape(-1)
            assert p.size == self.n
            self.host[GUARD + self.off:GUARD + self.off + self.n] = p
        self.buf.upload(self.host)
        self.ptr = self.buf.at(GUARD + self.off)

    def at(self, byte):
        return self.buf.at(GUARD + self.off + int(byte))

    def download(self):
        return self.buf.download((self.buf.nbytes,))


class Run:
    """the buffers of one call; finish() checks what must not have changed and frees them"""

    def __init__(self, pb3d, what):
        self.pb3d, self.lib, self.ctx, self.what = pb3d, pb3d._lib.load(), pb3d._lib.ctx(), what
        self.ins, self.outs = [], []

    def inp(self, array, off):
        a = np.ascontiguousarray(array)
        assert off % a.dtype.itemsize == 0
        ar = Arena(self.pb3d, a.nbytes, off, IN_FILL, a)
        self.ins.append(ar)
        return ar.ptr

    def out(self, nbytes, off, init=None, fill=OUT_FILL):
        ar = Arena(self.pb3d, nbytes, off, fill, init)
        self.outs.append(ar)
        return ar

    def ok(self, rc):
        self.pb3d._lib.check(rc)

    def finish(self, written=None):
        """-> the payloads of the output arenas.  written: {arena index: [(lo, hi)]} byte ranges of the payload the call may write (default all)"""
        self.pb3d.device.sync()
        res = []
        try:
            for ar in self.ins:
                assert np.array_equal(ar.download(), ar.host), (self.what, "an input arena changed")
            for i, ar in enumerate(self.outs):
                got = ar.download()
                lo, hi = GUARD + ar.off, GUARD + ar.off + ar.n
                assert (got[:lo] == ar.fill).all(), (self.what, "front guard of output", i, "touched at", int(np.flatnonzero(got[:lo] != ar.fill)[0]) - lo)
                assert (got[hi:] == ar.fill).all(), (self.what, "rear guard of output", i, "touched at +", int(np.flatnonzero(got[hi:] != ar.fill)[0]))
                pay = got[lo:hi]
                if written is not None and i in written:
                    keep = np.ones(ar.n, bool)
                    for a, b in written[i]:
                        keep[a:b] = False
                    assert np.array_equal(pay[keep], ar.host[lo:hi][keep]), (self.what, "output", i, "written outside its slab")
                res.append(pay.copy())
        finally:
            for ar in self.ins + self.outs:
                ar.buf.free()
        return res


def same(got, want, what):
    want = np.ascontiguousarray(want)
    g = got.view(want.dtype).reshape(want.shape) if got.size else got.reshape(want.shape)
    if not np.array_equal(g.view(np.uint8), want.view(np.uint8)):
        bad = np.flatnonzero(g.view(np.uint8).reshape(-1) != want.view(np.uint8).reshape(-1))
        raise AssertionError((what, f"{bad.size} bytes differ from the oracle, first at {int(bad[0])}"))


def truth(a):
    return np.ascontiguousarray(np.asarray(a) != 0).view(np.uint8)


def wh_mask(mask_hw):
    """(H, W) mask -> the (W, H) uint8 truthiness image the device entries take"""
    return truth(np.asarray(mask_hw).T)


# =====================================================================================================================
# carve, occupancy, colour apply
# =====================================================================================================================

@gpu
def test_carve_mask(pb3d_gpu, oracle):
    rng = np.random.default_rng(482)
    for (W, H, D), chans in (((64, 9, 64), (1, 3)), ((33, 5, 37), (3,)), ((20, 7, 5), (1, 3))):
        mask = rng.random((H, W)) < 0.6
        for ch in chans:
            grid = rng.integers(0, 256, (W, H, D) + ((3,) if ch == 3 else ()), dtype=np.uint8)
            want = oracle.carve_voxel_grid_with_masks(grid, mask)
            for oi, oo in COMBOS:
                r = Run(pb3d_gpu, ("carve_mask", W, H, D, ch, oi, oo))
                o = r.out(grid.nbytes, oo)
                r.ok(r.lib.pb3d_carve_mask_dev(r.ctx, r.inp(grid, oi), W, H, D, ch, r.inp(wh_mask(mask), oi and 1), o.ptr))
                same(r.finish()[0], want, r.what)


@gpu
def test_occupancy(pb3d_gpu, oracle):
    rng = np.random.default_rng(510)
    for nvox in (4096, 4099, 7):
        grid = rng.integers(0, 256, (nvox, 1, 1, 3), dtype=np.uint8) * (rng.random((nvox, 1, 1, 1)) < 0.5)
        grid = grid.astype(np.uint8)
        want = oracle.occupancy(grid)
        for oi, oo in COMBOS:
            r = Run(pb3d_gpu, ("occupancy", nvox, oi, oo))
            o = r.out(nvox, oo)
            r.ok(r.lib.pb3d_occupancy_dev(r.ctx, r.inp(grid, oi), nvox, o.ptr))
            same(r.finish()[0], want, r.what)


@gpu
def test_color_apply(pb3d_gpu, oracle):
    rng = np.random.default_rng(535)
    for W, H, D in ((12, 7, 32), (12, 7, 37), (12, 7, 5)):
        carved = rng.choice(np.array([0, 1, 1, 1, 2, 255], np.uint8), (W, H, D))
        rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        want = oracle.apply_colored_mask_to_voxel_grid(carved, rgb)
        for oi, oo in COMBOS:
            r = Run(pb3d_gpu, ("color_apply", W, H, D, oi, oo))
            o = r.out(want.nbytes, oo)
            r.ok(r.lib.pb3d_color_apply_dev(r.ctx, r.inp(carved, oi), W, H, D, r.inp(rgb, oi and 1), o.ptr))
            same(r.finish()[0], want, r.what)


# =====================================================================================================================
# rotation steps
# =====================================================================================================================

def rot_step(r, grid, M, off, mask_wh, oi, oo):
    L = r.pb3d._lib
    W, H, D = grid.shape
    o = r.out(grid.nbytes, oo)
    M = np.ascontiguousarray(M, np.float64).reshape(9)
    off = np.ascontiguousarray(off, np.float64)
    r.ok(r.lib.pb3d_rotate_carve_dev(r.ctx, r.inp(grid, oi), W, H, D, L.p_dbl(M), L.p_dbl(off), None if mask_wh is None else r.inp(mask_wh, oi and 1), o.ptr))
    return r.finish()[0]


def rot_want(oracle, grid, M, off, mask):
    w = oracle.affine_transform_u8(grid, M, off)
    return w if mask is None else oracle.carve_voxel_grid_with_masks(w, mask)


@gpu
def test_rotate90_forms(pb3d_gpu, oracle):
    """one shape per form of rot90_form (rotate_tiled.hip:764-785); an offset `out` leaves the flat forms, an offset `in` leaves WIDE"""
    rng = np.random.default_rng(780)
    M = oracle.rotation_matrix_inv(90)
    for W, H, D in ((355, 128, 355), (131, 256, 131), (256, 4, 256), (128, 5, 128), (100, 7, 100)):
        off = oracle.affine_offset(M, (W, H, D))
        mask = rng.random((H, W)) < 0.7
        grids = {"binary": (rng.random((W, H, D)) < 0.5).astype(np.uint8), "bytes": rng.integers(0, 256, (W, H, D), dtype=np.uint8)}
        for kind, grid in grids.items():
            for m in (mask, None):
                want = rot_want(oracle, grid, M, off, m)
                assert want.any()
                for oi, oo in COMBOS:
                    r = Run(pb3d_gpu, ("rotate 90", W, H, D, kind, m is not None, oi, oo))
                    same(rot_step(r, grid, M, off, None if m is None else wh_mask(m), oi, oo), want, r.what)


def rotinv180():
    """numpy.linalg.inv of the reference's Y-rotation at 180 degrees (reference utils/voxel_carving_utils.py:65-69), row 1 exact"""
    a = np.deg2rad(180.0)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    M = np.linalg.inv(R)
    M[1] = (0.0, 1.0, 0.0)
    M[0, 1] = M[2, 1] = 0.0
    return M


@gpu
def test_rotate_generic_and_180(pb3d_gpu, oracle):
    rng = np.random.default_rng(103)
    W, H, D = 48, 9, 52
    mask = rng.random((H, W)) < 0.7
    grids = {"binary": (rng.random((W, H, D)) < 0.5).astype(np.uint8), "bytes": rng.integers(0, 256, (W, H, D), dtype=np.uint8)}
    for angle in (45, 30):
        M = oracle.rotation_matrix_inv(angle)
        off = oracle.affine_offset(M, (W, H, D))
        for kind, grid in grids.items():
            for m in (mask, None):
                want = rot_want(oracle, grid, M, off, m)
                assert want.any()
                for oi, oo in COMBOS:
                    r = Run(pb3d_gpu, ("rotate", angle, kind, m is not None, oi, oo))
                    same(rot_step(r, grid, M, off, None if m is None else wh_mask(m), oi, oo), want, r.what)
    # 180 degrees: aligned -> k_rotate_perm; otherwise the bit-sliced table step (0/1) or k_rotate_generic (bytes)
    W, H, D = 36, 5, 40
    M = rotinv180()
    off = oracle.affine_offset(M, (W, H, D))
    mask = rng.random((H, W)) < 0.7
    grids = {"binary": (rng.random((W, H, D)) < 0.5).astype(np.uint8), "bytes": rng.integers(0, 256, (W, H, D), dtype=np.uint8)}
    for kind, grid in grids.items():
        for m in (mask, None):
            want = rot_want(oracle, grid, M, off, m)
            assert want.any()
            for oi, oo in COMBOS:
                r = Run(pb3d_gpu, ("rotate 180", kind, m is not None, oi, oo))
                same(rot_step(r, grid, M, off, None if m is None else wh_mask(m), oi, oo), want, r.what)


@gpu
def test_process_grid(pb3d_gpu, oracle):
    rng = np.random.default_rng(170)
    jobs = [((300, 16, 357), "binary", (90, 45, 5)), ((128, 9, 128), "binary", (90, 45, 5)), ((128, 9, 128), "bytes", (45,))]
    for (W, H, D), kind, angles in jobs:
        grid = (rng.random((W, H, D)) < 0.6).astype(np.uint8) if kind == "binary" else rng.integers(0, 256, (W, H, D), dtype=np.uint8)
        mask = rng.random((H, W)) < 0.8
        for ai in angles:
            want = oracle.process_voxel_grid(grid, mask, ai)
            assert want.any()
            for oi, oo in COMBOS:
                ot = COMBOS[(COMBOS.index((oi, oo)) + 5) % len(COMBOS)][1]          # d_tmp at an offset of its own
                r = Run(pb3d_gpu, ("process_grid", W, H, D, kind, ai, oi, oo, ot))
                o, t = r.out(grid.nbytes, oo), r.out(grid.nbytes, ot)
                r.ok(r.lib.pb3d_process_grid_dev(r.ctx, r.inp(grid, oi), W, H, D, r.inp(wh_mask(mask), oi and 1), ai, o.ptr, t.ptr))
                same(r.finish()[0], want, r.what)


# =====================================================================================================================
# global_carve, part_carve
# =====================================================================================================================

def sem_inputs(pb3d, rng, h, w):
    pal = np.array(list(pb3d.PART_COLORS.values()), np.uint8)
    sem = pal[rng.integers(0, len(pal), ((h + 3) // 4, (w + 3) // 4))].repeat(4, 0).repeat(4, 1)[:h, :w]
    binary = (rng.random((h, w)) < 0.8).astype(np.uint8)
    return pal, np.ascontiguousarray(sem), binary


@gpu
def test_global_carve(pb3d_gpu, oracle):
    rng = np.random.default_rng(269)
    h, w = 37, 131
    pal, sem, binary = sem_inputs(pb3d_gpu, rng, h, w)
    plane = h * w * 3
    for ai in (90, 45):
        want = oracle.global_carve(binary, sem, ai)
        assert want.any()
        for oi, oo in COMBOS:
            r = Run(pb3d_gpu, ("global_carve", ai, oi, oo))
            o = r.out(want.nbytes, oo)
            r.ok(r.lib.pb3d_global_carve_dev(r.ctx, r.inp(binary, oi), r.inp(sem, oi and 1), h, w, ai, 0, w, o.ptr))
            same(r.finish()[0], want, r.what)
        # the slab form: slab pointer = volume + x0 * h * w * 3, residues 1, 4 and 0 mod 16 inside an aligned volume
        for (x0, x1), res in (((5, 9), 1), ((4, 20), 4), ((16, w), 0)):
            assert (x0 * plane) % 16 == res
            r = Run(pb3d_gpu, ("global_carve slab", ai, x0, x1))
            o = r.out(want.nbytes, 0)
            rc = r.lib.pb3d_global_carve_dev(r.ctx, r.inp(binary, 0), r.inp(sem, 0), h, w, ai, x0, x1, o.at(x0 * plane))
            if ai != 90:            # a proper slab exists for the fused 90-degree path only: refused before any device work
                assert rc == -1 and "slab output needs the fused 90-degree path" in last_error(pb3d_gpu), (r.what, rc)
                assert (r.finish()[0] == OUT_FILL).all(), r.what
                continue
            r.ok(rc)
            got = r.finish(written={0: [(x0 * plane, x1 * plane)]})[0]
            same(got[x0 * plane:x1 * plane], want[x0:x1], r.what)
        if ai != 90:                # the context after the refusals
            r = Run(pb3d_gpu, ("global_carve after refusal", ai))
            o = r.out(want.nbytes, 0)
            r.ok(r.lib.pb3d_global_carve_dev(r.ctx, r.inp(binary, 0), r.inp(sem, 0), h, w, ai, 0, w, o.ptr))
            same(r.finish()[0], want, r.what)


def part_job_arrays(oracle, sem, jobs, W, H):
    """the (W, H) job images of pb3d_part_carve_dev as oracle.part_carve derives them (reference :143-151)"""
    nj = len(jobs)
    msub = np.zeros((nj, W, H), np.uint8); mcarve = np.zeros((nj, W, H), np.uint8)
    ang = (C.c_int * nj)(); skip = (C.c_int * nj)()
    for j, (names, angle) in enumerate(jobs):
        m2 = oracle.part_masks(sem, names)
        skip[j] = 0 if m2.any() else 1
        ang[j] = int(angle)
        msub[j] = m2.T.astype(np.uint8)
        mcarve[j] = np.ascontiguousarray(oracle.mask_to_wh(msub[j], W, H))
    return msub, mcarve, ang, skip


def part_inputs(pb3d, oracle, rng, W, H, D):
    names = list(oracle.PART_COLORS)
    pal = np.array([oracle.PART_COLORS[n] for n in names], np.uint8)
    lab_hw = rng.integers(0, len(names), ((H + 3) // 4, (W + 3) // 4)).repeat(4, 0).repeat(4, 1)[:H, :W]
    sem = np.ascontiguousarray(pal[lab_hw])
    colored = np.ascontiguousarray(np.broadcast_to(sem.transpose(1, 0, 2)[:, :, None, :], (W, H, D, 3))) * (rng.random((W, H, D, 1)) < 0.7)
    colored = np.ascontiguousarray(colored.astype(np.uint8))
    six90 = [([n], 90) for n in names[:6]]
    mixed = [([names[0], names[1]], 90), ([names[2]], 45), ([names[3]], 90), ([names[4], names[5]], 45)]
    return names, pal, lab_hw, sem, colored, six90, mixed


@gpu
def test_part_carve(pb3d_gpu, oracle):
    rng = np.random.default_rng(581)
    for W, H, D in ((40, 24, 56), (41, 24, 56)):
        names, pal, lab_hw, sem, colored, six90, mixed = part_inputs(pb3d_gpu, oracle, rng, W, H, D)
        for jobs in (six90, mixed):
            want = oracle.part_carve(colored, sem, jobs)
            assert want.any()
            msub, mcarve, ang, skip = part_job_arrays(oracle, sem, jobs, W, H)
            for oi, oo in COMBOS:
                r = Run(pb3d_gpu, ("part_carve", W, H, D, len(jobs), oi, oo))
                o = r.out(want.nbytes, oo)
                r.ok(r.lib.pb3d_part_carve_dev(r.ctx, r.inp(colored, oi), W, H, D, r.inp(msub, oi and 1), r.inp(mcarve, oi and 4), ang, skip, len(jobs), o.ptr))
                same(r.finish()[0], want, r.what)


# =====================================================================================================================
# label form
# =====================================================================================================================

def to_label(rgb, pal):
    """label 0 <-> black, k <-> pal[k - 1]"""
    key = rgb[..., 0].astype(np.int64) << 16 | rgb[..., 1].astype(np.int64) << 8 | rgb[..., 2]
    pk = np.concatenate([[0], pal[:, 0].astype(np.int64) << 16 | pal[:, 1].astype(np.int64) << 8 | pal[:, 2]])
    order = np.argsort(pk)
    pos = np.searchsorted(pk[order], key)
    assert (pk[order][pos] == key).all()
    return order[pos].astype(np.uint8)


def to_rgb(label, pal):
    return np.concatenate([np.zeros((1, 3), np.uint8), pal])[label]


@gpu
def test_label_conversions(pb3d_gpu):
    L = pb3d_gpu._lib
    rng = np.random.default_rng(66)
    pal = np.array(list(pb3d_gpu.PART_COLORS.values()), np.uint8)
    for nvox in (4096, 4099, 7):
        lab = rng.integers(0, len(pal) + 1, nvox).astype(np.uint8)
        rgb = to_rgb(lab, pal)
        assert np.array_equal(to_label(rgb, pal), lab)
        for oi, oo in COMBOS:
            r = Run(pb3d_gpu, ("rgb_to_label", nvox, oi, oo))
            o = r.out(nvox, oo)
            r.ok(r.lib.pb3d_rgb_to_label_dev(r.ctx, r.inp(rgb, oi), nvox, L.p_u8(pal), len(pal), o.ptr))
            same(r.finish()[0], lab, r.what)
            r = Run(pb3d_gpu, ("label_to_rgb", nvox, oi, oo))
            o = r.out(nvox * 3, oo)
            r.ok(r.lib.pb3d_label_to_rgb_dev(r.ctx, r.inp(lab, oi), nvox, L.p_u8(pal), len(pal), o.ptr))
            same(r.finish()[0], rgb, r.what)


@gpu
def test_global_carve_label(pb3d_gpu, oracle):
    rng = np.random.default_rng(330)
    h, w = 37, 131
    pal, sem, binary = sem_inputs(pb3d_gpu, rng, h, w)
    sem[rng.random((h, w)) < 0.1] = 0
    label_hw = to_label(sem, pal)
    for ai in (90, 45):
        want = to_label(oracle.global_carve(binary, sem, ai), pal)
        assert want.any()
        for oi, oo in COMBOS:
            r = Run(pb3d_gpu, ("global_carve_label", ai, oi, oo))
            o = r.out(want.nbytes, oo)
            r.ok(r.lib.pb3d_global_carve_label_dev(r.ctx, r.inp(binary, oi), r.inp(label_hw, oi and 1), h, w, ai, o.ptr))
            same(r.finish()[0], want, r.what)


@gpu
def test_part_carve_label(pb3d_gpu, oracle):
    rng = np.random.default_rng(368)
    W, H, D = 40, 24, 48
    names, pal, lab_hw, sem, colored, six90, mixed = part_inputs(pb3d_gpu, oracle, rng, W, H, D)
    label = to_label(colored, pal)
    for jobs in (mixed, six90):
        want = to_label(oracle.part_carve(colored, sem, jobs), pal)
        assert want.any()
        msub, mcarve, ang, skip = part_job_arrays(oracle, sem, jobs, W, H)
        for oi, oo in COMBOS:
            r = Run(pb3d_gpu, ("part_carve_label", len(jobs), oi, oo))
            o = r.out(want.nbytes, oo)
            r.ok(r.lib.pb3d_part_carve_label_dev(r.ctx, r.inp(label, oi), W, H, D, r.inp(msub, oi and 1), r.inp(mcarve, oi and 4), ang, skip, len(jobs), o.ptr))
            same(r.finish()[0], want, r.what)


@gpu
def test_orient(pb3d_gpu):
    rng = np.random.default_rng(706)
    for W, H, D in ((128, 3, 128), (36, 5, 40), (33, 5, 37)):
        grid = rng.integers(0, 256, (W, H, D, 3), dtype=np.uint8)
        want = np.ascontiguousarray(np.flip(grid.transpose(2, 1, 0, 3), axis=1))
        for oi, oo in COMBOS:
            r = Run(pb3d_gpu, ("orient", W, H, D, oi, oo))
            o = r.out(want.nbytes, oo)
            r.ok(r.lib.pb3d_orient_dev(r.ctx, r.inp(grid, oi), W, H, D, o.ptr))
            same(r.finish()[0], want, r.what)
    W, H, D = 70, 5, 66
    grid = rng.integers(0, 256, (W, H, D), dtype=np.uint8)
    want = np.ascontiguousarray(np.flip(grid.transpose(2, 1, 0), axis=1))
    for oi, oo in COMBOS:
        r = Run(pb3d_gpu, ("orient_label", oi, oo))
        o = r.out(want.nbytes, oo)
        r.ok(r.lib.pb3d_orient_label_dev(r.ctx, r.inp(grid, oi), W, H, D, o.ptr))
        same(r.finish()[0], want, r.what)


# =====================================================================================================================
# grid -> points
# =====================================================================================================================

@gpu
def test_points_count_fill(pb3d_gpu, oracle):
    L = pb3d_gpu._lib
    rng = np.random.default_rng(493)
    pal = np.array(list(pb3d_gpu.PART_COLORS.values()), np.uint8)
    ga = pal[rng.integers(0, len(pal), (45, 70, 33))] * (rng.random((45, 70, 33, 1)) < 0.3)
    ga = np.ascontiguousarray(ga.astype(np.uint8))
    lab = (rng.integers(0, 16, (51, 18, 77)) * (rng.random((51, 18, 77)) < 0.5)).astype(np.uint8)
    labels = np.array([1, 4, 9, 15], np.uint8)
    cases = []
    for stride in (1, 2):
        cases.append((ga, 3, np.ascontiguousarray(pal[:4]), stride, oracle._points(ga, pal[:4], stride)))
        cases.append((ga, 3, np.zeros((0, 3), np.uint8), stride, oracle._points(ga, None, stride)))
        sub = lab[::stride, ::stride, ::stride]
        a0, a1, a2 = np.nonzero(np.isin(sub, labels))
        cases.append((lab, 1, labels, stride, ((np.stack([a2, a1, a0], axis=1) * stride).astype(np.float32), sub[a0, a1, a2][:, None])))
    # grid, d_pts, d_cols.  The wave-private fill (points.hip:336,341) runs for a 16-byte aligned grid at stride 1 only: every
    # d_pts / d_cols offset appears with such a grid (0, 16, 64) as well as with the byte forms (1, 4)
    offs = [(0, 0, 0), (0, 4, 1), (0, 8, 2), (0, 12, 3), (16, 8, 2), (16, 12, 3), (64, 4, 1), (1, 4, 1), (4, 8, 2), (1, 12, 3), (4, 0, 0)]
    for g, ch, cols, stride, (want_p, want_c) in cases:
        A0, A1, A2 = g.shape[:3]
        assert len(want_p) > 100
        cp = L.p_u8(cols) if len(cols) else None
        for og, op, oc in offs:
            r = Run(pb3d_gpu, ("points", g.shape, len(cols), stride, og, op, oc))
            n = C.c_int64(0)
            dg = r.inp(g, og)
            r.ok(r.lib.pb3d_points_count_dev(r.ctx, dg, A0, A1, A2, ch, cp, len(cols), stride, C.byref(n)))
            assert n.value == len(want_p), r.what
            dp, dc = r.out(n.value * 12, op), r.out(n.value * ch, oc)
            r.ok(r.lib.pb3d_points_fill_dev(r.ctx, dg, A0, A1, A2, ch, cp, len(cols), stride, n.value, dp.ptr, dc.ptr))
            got_p, got_c = r.finish()
            same(got_p, want_p, r.what)
            same(got_c, np.ascontiguousarray(want_c), r.what)


def last_error(pb3d):
    return pb3d._lib.load().pb3d_last_error().decode()


@gpu
def test_refusals(pb3d_gpu, oracle):
    """the entries that need more than the element type's alignment say so before any device work, and the context goes on working"""
    import synth_host
    L = pb3d_gpu._lib
    rng = np.random.default_rng(610)
    pal = np.array(list(pb3d_gpu.PART_COLORS.values()), np.uint8)
    g = np.ascontiguousarray((pal[rng.integers(0, len(pal), (32, 16, 32))] * (rng.random((32, 16, 32, 1)) < 0.3)).astype(np.uint8))
    cols = np.ascontiguousarray(pal[:3])
    want_p, want_c = oracle._points(g, cols, 1)
    for og in (1, 4, 0):
        r = Run(pb3d_gpu, ("points_extract", og))
        n = C.c_int64(-7)
        dp, dc = r.out(len(want_p) * 12, 0), r.out(len(want_p) * 3, 0)
        rc = r.lib.pb3d_points_extract_dev(r.ctx, r.inp(g, og), 32, 16, 32, 3, L.p_u8(cols), 3, len(want_p), dp.ptr, dc.ptr, C.byref(n))
        if og:
            assert rc == -1 and "16-byte aligned grid" in last_error(pb3d_gpu), (og, rc, last_error(pb3d_gpu))
            got_p, got_c = r.finish()
            assert (got_p == OUT_FILL).all() and (got_c == OUT_FILL).all() and n.value == 0
        else:                                       # the aligned call after the refusals, same context
            r.ok(rc)
            got_p, got_c = r.finish()
            assert n.value == len(want_p)
            same(got_p, want_p, r.what)
            same(got_c, want_c, r.what)
    x0, x1, H, D, seed = 3, 7, 8, 16, 12345
    want = synth_host.sem_slab(x0, x1, H, D, seed)
    for oo in (1, 2, 0):
        r = Run(pb3d_gpu, ("synth_sem", oo))
        o = r.out(want.nbytes, oo)
        rc = r.lib.pb3d_synth_sem_dev(r.ctx, x0, x1, H, D, seed, o.ptr)
        if oo:
            assert rc == -1 and "unaligned" in last_error(pb3d_gpu), (oo, rc)
            assert (r.finish()[0] == OUT_FILL).all()
        else:
            r.ok(rc)
            same(r.finish()[0], want, r.what)


# =====================================================================================================================
# extrusion, counters, presence, labelling
# =====================================================================================================================

@gpu
def test_extrude(pb3d_gpu, oracle):
    L = pb3d_gpu._lib
    rng = np.random.default_rng(724)
    W, H, D = 21, 13, 18
    pal = np.array(list(pb3d_gpu.PART_COLORS.values()), np.uint8)
    grid = np.ascontiguousarray((pal[rng.integers(0, len(pal), (W, H, D))] * (rng.random((W, H, D, 1)) < 0.15)).astype(np.uint8))
    fill = np.array([9, 200, 31], np.uint8)
    combos = COMBOS[::2] + [(1, 1)]
    for axis in (2, 0):
        m2 = rng.random((H, W) if axis == 2 else (H, D)) < 0.6
        valid = truth(m2.T) if axis == 2 else truth(m2)
        vw = W if axis == 2 else D
        for direction in ("+", "-"):
            for fc in (fill, None):
                want = oracle.extrude_from_surface(grid, m2, axis, direction, 4, None if fc is None else fc)
                assert not np.array_equal(want, grid) or fc is None
                for oi, oo in combos:
                    r = Run(pb3d_gpu, ("extrude", axis, direction, fc is not None, oi, oo))
                    o = r.out(grid.nbytes, oo)
                    r.ok(r.lib.pb3d_extrude_dev(r.ctx, r.inp(grid, oi), W, H, D, r.inp(valid, oi and 1), vw, axis, int(direction == "+"), 4,
                                                None if fc is None else L.p_u8(fc), o.ptr))
                    same(r.finish()[0], want, r.what)
                    r = Run(pb3d_gpu, ("extrude in place", axis, direction, fc is not None, oo))
                    o = r.out(grid.nbytes, oo, init=grid)
                    r.ok(r.lib.pb3d_extrude_dev(r.ctx, o.ptr, W, H, D, r.inp(valid, oi), vw, axis, int(direction == "+"), 4,
                                                None if fc is None else L.p_u8(fc), o.ptr))
                    same(r.finish()[0], want, r.what)


@gpu
def test_count_nonzero_partwise_iou(pb3d_gpu, oracle):
    L = pb3d_gpu._lib
    rng = np.random.default_rng(486)
    b = (rng.integers(0, 256, 4099) * (rng.random(4099) < 0.4)).astype(np.uint8)
    for ob, oc in ((0, 0), (1, 8), (4, 24), (16, 8), (64, 0)):
        r = Run(pb3d_gpu, ("count_nonzero", ob, oc))
        cnt = r.out(8, oc, init=np.zeros(1, np.int64))
        r.ok(r.lib.pb3d_count_nonzero_dev(r.ctx, r.inp(b, ob), b.size, cnt.ptr))
        same(r.finish()[0], np.array([np.count_nonzero(b)], np.int64), r.what)
    pal = np.array(list(pb3d_gpu.PART_COLORS.values())[:6], np.uint8)
    Hh, Ww = 30, 40
    a_img = pal[rng.integers(0, 6, (Hh, Ww))] * (rng.random((Hh, Ww, 1)) < 0.8).astype(np.uint8)
    b_img = pal[rng.integers(0, 6, (Hh, Ww))] * (rng.random((Hh, Ww, 1)) < 0.8).astype(np.uint8)
    b_img[::2] = a_img[::2]
    wi, wu = oracle.partwise_iou_counts(a_img, b_img, pal)
    assert np.any(np.asarray(wi) > 0)
    for oa, ob in COMBOS:
        r = Run(pb3d_gpu, ("partwise_iou", oa, ob))
        inter, uni = np.zeros(6, np.int64), np.zeros(6, np.int64)
        r.ok(r.lib.pb3d_partwise_iou_dev(r.ctx, r.inp(a_img, oa), r.inp(b_img, ob), Hh * Ww, L.p_u8(pal), 6, inter.ctypes.data_as(L.i64p),
                                         uni.ctypes.data_as(L.i64p)))
        r.finish()
        assert np.array_equal(inter, wi) and np.array_equal(uni, wu), r.what


@gpu
def test_color_presence(pb3d_gpu):
    L = pb3d_gpu._lib
    rng = np.random.default_rng(395)
    pal = np.array(list(pb3d_gpu.PART_COLORS.values()), np.uint8)
    table = np.ascontiguousarray(np.concatenate([pal[:5], [[7, 7, 7]]]).astype(np.uint8))
    for nvox in (4096, 4099):
        grid = np.ascontiguousarray((pal[rng.integers(1, 7, nvox)] * (rng.random((nvox, 1)) < 0.5)).astype(np.uint8))
        keys = np.unique(grid[:, 0].astype(np.int64) | grid[:, 1].astype(np.int64) << 8 | grid[:, 2].astype(np.int64) << 16)
        keys = keys[keys != 0]
        bitmap = np.zeros(L.PRESENCE_BYTES // 4, np.uint32)
        np.bitwise_or.at(bitmap, keys >> 5, np.uint32(1) << (keys & 31).astype(np.uint32))
        tkeys = table[:, 0].astype(np.int64) | table[:, 1].astype(np.int64) << 8 | table[:, 2].astype(np.int64) << 16
        present = np.array([sum(1 << k for k, t in enumerate(tkeys) if t in keys)], np.int64)
        assert 0 < present[0] < (1 << len(table)) - 1
        for og, obm, op in ((0, 0, 0), (1, 4, 8), (4, 12, 24), (16, 4, 0), (64, 0, 8)):
            r = Run(pb3d_gpu, ("color_presence", nvox, og, obm, op))
            bm, pr = r.out(L.PRESENCE_BYTES, obm), r.out(8, op)
            r.ok(r.lib.pb3d_color_presence_dev(r.ctx, r.inp(grid, og), nvox, 3, bm.ptr, L.p_u8(table), len(table), pr.ptr))
            got_bm, got_pr = r.finish()
            same(got_bm, bitmap, r.what)
            same(got_pr, present, r.what)


@gpu
def test_labelling_and_recolor(pb3d_gpu, oracle):
    from scipy import ndimage
    L = pb3d_gpu._lib
    rng = np.random.default_rng(127)
    A0, A1, A2 = 24, 10, 27
    pal = np.array(list(pb3d_gpu.PART_COLORS.values()), np.uint8)
    grid = np.ascontiguousarray(pal[rng.integers(0, 3, (A0, A1, A2))] * (rng.random((A0, A1, A2, 1)) < 0.55).astype(np.uint8))
    col = np.ascontiguousarray(pal[1:2])
    member = np.all(grid == col[0], axis=-1)
    cap = 4096
    for conn, rank in ((6, 1), (26, 3)):
        want, nwant = ndimage.label(member, structure=ndimage.generate_binary_structure(3, rank))
        want = want.astype(np.int32)
        assert nwant > 5
        if conn == 6:
            assert np.array_equal(oracle.label6(member)[0], want)
        for og, ol in ((0, 0), (1, 4), (4, 12), (16, 4), (64, 0)):
            r = Run(pb3d_gpu, ("label_colors_conn_stats", conn, og, ol))
            lab = r.out(member.size * 4, ol)
            n = (C.c_int64 * 1)(); ok = (C.c_int * 1)()
            bbox = np.zeros((cap, 6), np.int64); cnt = np.zeros(cap, np.int64); sums = np.zeros((cap, 3), np.int64)
            r.ok(r.lib.pb3d_label_colors_conn_stats_dev(r.ctx, r.inp(grid, og), A0, A1, A2, L.p_u8(col), 1, 3, conn, lab.ptr, n, cap, 0,
                                                        bbox.ctypes.data_as(L.i64p), cnt.ctypes.data_as(L.i64p), sums.ctypes.data_as(L.i64p), ok))
            same(r.finish()[0], want, r.what)
            assert n[0] == nwant and ok[0] == 1, r.what
            assert np.array_equal(cnt[:nwant], np.bincount(want.ravel(), minlength=nwant + 1)[1:]), r.what
            objs = ndimage.find_objects(want)
            assert np.array_equal(bbox[:nwant], np.array([[s.start for s in o] + [s.stop for s in o] for o in objs])), r.what
    # recolor_components: int32 labels at +4 / +12, the grid in place at byte offsets
    want_lab, nwant = ndimage.label(member)
    want_lab = want_lab.astype(np.int32)
    flags = (rng.random(nwant) < 0.5).astype(np.uint8)
    new = np.array([3, 250, 77], np.uint8)
    want = grid.copy()
    want[(want_lab > 0) & (flags[np.maximum(want_lab, 1) - 1] != 0)] = new
    assert not np.array_equal(want, grid)
    for ol, og in ((0, 0), (4, 1), (12, 4), (4, 16), (0, 64)):
        r = Run(pb3d_gpu, ("recolor_components", ol, og))
        o = r.out(grid.nbytes, og, init=grid)
        r.ok(r.lib.pb3d_recolor_components_dev(r.ctx, r.inp(want_lab, ol), member.size, L.p_u8(flags), nwant, L.p_u8(new), o.ptr))
        same(r.finish()[0], want, r.what)


@gpu
def test_top_k_components(pb3d_gpu):
    from scipy import ndimage
    from test_top_k_components import ref_top_k, scene
    L = pb3d_gpu._lib
    g, col = scene(np.random.default_rng(658), shape=(20, 24, 45), nblobs=8)
    n = ndimage.label(np.all(g == col, -1), structure=np.ones((3, 3, 3)))[1]
    assert n > 6
    for k in (1, 4, -1):
        want = ref_top_k(g, col, k if k >= 0 else n + k)
        assert not np.array_equal(want, g)
        for og, ol, ost in ((0, 0, 0), (1, 4, 8), (4, 12, 8), (16, 4, 0), (64, 12, 8)):
            r = Run(pb3d_gpu, ("top_k_components", k, og, ol, ost))
            dg = r.out(g.nbytes, og, init=g)
            lab, st = r.out(g.size // 3 * 4, ol), r.out(16, ost)          # members-only labels: only their guards are checked
            r.ok(r.lib.pb3d_top_k_components_dev(r.ctx, dg.ptr, 20, 24, 45, L.p_u8(col), 3, k, 26, lab.ptr, st.ptr))
            got, _, status = r.finish()
            same(got, want, r.what)
            same(status, np.array([n, 0], np.int64), r.what)


@gpu
def test_component_members(pb3d_gpu):
    from scipy import ndimage
    L = pb3d_gpu._lib
    rng = np.random.default_rng(63)
    A0, A1, A2 = shape = (12, 10, 27)
    ca, cb = np.array([253, 248, 96], np.uint8), np.array([0, 0, 255], np.uint8)
    grid = np.ascontiguousarray(np.where(rng.random(shape + (1,)) < 0.3, ca, cb).astype(np.uint8))
    lab, n = ndimage.label(np.all(grid == ca, -1), structure=np.ones((3, 3, 3)))
    lab = lab.astype(np.int32)
    assert n >= 3
    objs = ndimage.find_objects(lab)
    sel = [1, 2, n]
    bbox = np.array([[s.start for s in objs[l - 1]] + [s.stop for s in objs[l - 1]] for l in sel], np.int64)
    counts = np.array([(lab == l).sum() for l in sel], np.int64)
    cols = np.ascontiguousarray(np.tile(ca, len(sel)))
    labels = np.array(sel, np.int32)
    want_masks = np.stack([(lab == l) for l in sel]).astype(np.uint8)
    want_xyz = np.concatenate([np.argwhere(lab == l) for l in sel]).astype(np.int64)
    want_rows = np.zeros((len(sel), 2, 4), np.int64)
    for q, l in enumerate(sel):
        xyz = np.argwhere(lab == l)
        for e, row in ((0, bbox[q, 1]), (1, bbox[q, 4] - 1)):
            on = xyz[xyz[:, 1] == row]
            want_rows[q, e] = [len(on), *on.sum(axis=0)]
    for og, ol, oc, orw, om in ((0, 0, 0, 0, 0), (1, 4, 8, 8, 1), (4, 12, 24, 24, 4), (16, 4, 8, 0, 16), (64, 0, 0, 8, 1)):
        r = Run(pb3d_gpu, ("component_members", og, ol, oc, orw, om))
        dc, dr, dm = r.out(want_xyz.nbytes, oc), r.out(want_rows.nbytes, orw), r.out(want_masks.nbytes, om)
        r.ok(r.lib.pb3d_component_members_dev(r.ctx, r.inp(grid, og), A0, A1, A2, 3, r.inp(lab, ol), len(sel), L.p_u8(cols),
                                              labels.ctypes.data_as(C.POINTER(C.c_int32)), bbox.ctypes.data_as(L.i64p), counts.ctypes.data_as(L.i64p), 7,
                                              dc.ptr, dr.ptr, dm.ptr))
        got_c, got_r, got_m = r.finish()
        same(got_c, want_xyz, r.what)
        same(got_r, want_rows, r.what)
        same(got_m, want_masks, r.what)


@gpu
def test_mesh(pb3d_gpu):
    import mesh_restate as mr
    from pb3d.voxel_utils import mesh_colors
    from test_meshify import check_colors, rand_grid
    rng = np.random.default_rng(159)
    for shape, dens, stride in (((13, 11, 9), 0.5, 1), ((17, 19, 16), 0.6, 2)):
        A0, A1, A2 = shape
        grid = np.ascontiguousarray(rand_grid(rng, shape, dens))
        rv, rf, rc, rn = mr.meshify(grid, stride)
        assert rv.dtype == np.float32 and rf.dtype == np.int32 and rn.dtype == np.float32 and len(rv) > 50
        for og, ov, of, on, oc in ((0, 0, 0, 0, 0), (1, 4, 4, 12, 1), (4, 12, 4, 4, 3), (16, 4, 12, 0, 2), (64, 0, 4, 4, 0)):
            r = Run(pb3d_gpu, ("mesh", shape, stride, og, ov, of, on, oc))
            dg = r.inp(grid, og)
            nv, nf = C.c_int64(0), C.c_int64(0)
            r.ok(r.lib.pb3d_mesh_count_dev(r.ctx, dg, A0, A1, A2, 3, stride, C.byref(nv), C.byref(nf)))
            assert (nv.value, nf.value) == (len(rv), len(rf)), r.what
            dv, df, dn, dc = r.out(rv.nbytes, ov), r.out(rf.nbytes, of), r.out(rn.nbytes, on), r.out(len(rv) * 3, oc)
            r.ok(r.lib.pb3d_mesh_fill_dev(r.ctx, dg, A0, A1, A2, 3, stride, nv.value, nf.value, dv.ptr, df.ptr, dn.ptr, dc.ptr))
            gv, gf, gn, gc = r.finish()
            same(gv, rv, r.what)
            same(gf, rf, r.what)
            same(gn, rn, r.what)
            check_colors(grid, stride, rv, mesh_colors(gc.reshape(-1, 3)), rc)
            # the nearest-voxel query on its own, the vertices as an input at an offset
            r = Run(pb3d_gpu, ("mesh_colors", shape, stride, og, ov, oc))
            dc = r.out(len(rv) * 3, oc)
            r.ok(r.lib.pb3d_mesh_colors_dev(r.ctx, r.inp(grid, og), A0, A1, A2, 3, stride, r.inp(rv, ov), len(rv), dc.ptr))
            check_colors(grid, stride, rv, mesh_colors(r.finish()[0].reshape(-1, 3)), rc)


# =====================================================================================================================
# the fused component loop of left_right_guided_carve
# =====================================================================================================================

@gpu
def test_guided_carve(pb3d_gpu, oracle):
    """label (members only, as the package does) and carve in place on a grid at every byte offset; the scene's large box ends at the
    volume's last voxel, so k_crop_slice's dword load of the voxel before it and its byte loads of the last one sit against the guard"""
    import contextlib
    import io
    import guided_scenes as gs
    L = pb3d_gpu._lib
    sc = gs.scene("corner_small")
    W, H, D = sc.shape
    nvox, n, angle, cap = W * H * D, len(sc.boxes), 45, 64
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        want3 = oracle.left_right_guided_carve(sc.grid, sc.sem, sc.color, angle=angle)
    counts = np.array([int(v) for v in re.findall(r"carved voxels: (\d+)", buf.getvalue())], np.int64)
    assert len(counts) == n and not np.array_equal(want3, sc.grid)
    pal = np.ascontiguousarray(np.stack([gs.COLOR, gs.FOREIGN]))
    grid1, want1 = to_label(sc.grid, pal), to_label(want3, pal)
    masks, offs = gs.crop_masks(sc.sem, sc.color, sc.boxes)
    bb = np.ascontiguousarray(sc.boxes)
    i64 = lambda a: a.ctypes.data_as(L.i64p)
    lab_offs = [(0, 0)] + [(k, (4, 12)[i % 2]) for i, k in enumerate(BYTE_OFFS)]
    for ch, grid, want in ((3, sc.grid, want3), (1, grid1, want1)):
        for entry in ("plain", "color", "queue"):
            for og, ol in lab_offs:
                r = Run(pb3d_gpu, ("guided_carve", ch, entry, og, ol))
                g, lab = r.out(grid.nbytes, og, init=grid, fill=IN_FILL), r.out(nvox * 4, ol)         # (the grid is read too: dirty 0xff slack)
                nc = (C.c_int64 * 1)(); ok = (C.c_int * 1)()
                bbox = np.zeros((cap, 6), np.int64); cnt = np.zeros(cap, np.int64); sums = np.zeros((cap, 3), np.int64)
                if ch == 3:
                    r.ok(r.lib.pb3d_label_color_stats_dev(r.ctx, g.ptr, W, H, D, L.p_u8(pal[0]), lab.ptr, nc, cap, 1, i64(bbox), i64(cnt), i64(sums), ok))
                else:
                    r.ok(r.lib.pb3d_label_value_stats_dev(r.ctx, g.ptr, W, H, D, 1, lab.ptr, nc, cap, 1, i64(bbox), i64(cnt), i64(sums), ok))
                assert nc[0] == n and ok[0] == 1 and np.array_equal(bbox[:n], bb), r.what
                cn = np.full(n, -1, np.int64)
                took = C.c_int(-1)
                tail = (n, i64(bb), L.p_u8(masks), i64(offs), masks.size, angle)
                if entry == "plain":
                    fn = r.lib.pb3d_guided_carve_dev if ch == 3 else r.lib.pb3d_guided_carve_label_dev
                    r.ok(fn(r.ctx, g.ptr, lab.ptr, W, H, D, *tail, i64(cn), C.byref(took)))
                elif entry == "color":
                    r.ok(r.lib.pb3d_guided_carve_color_dev(r.ctx, g.ptr, lab.ptr, 0, ch, W, H, D, *tail, i64(cn), C.byref(took)))
                else:
                    dc = r.out(8 * n, (8, 24)[ol % 8 == 4], init=np.full(n, -3, np.int64))
                    r.ok(r.lib.pb3d_guided_carve_queue_dev(r.ctx, g.ptr, lab.ptr, 0, ch, W, H, D, *tail, dc.ptr, C.byref(took)))
                assert took.value == 1, r.what
                outs = r.finish()
                same(outs[0], want, r.what)
                if entry == "queue":
                    same(outs[2], counts, r.what)
                else:
                    assert np.array_equal(cn, counts), r.what
