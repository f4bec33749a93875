// Internal declarations shared by the translation units of libpb3d.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <type_traits>

#include "pb3d.h"

typedef uint8_t u8;
typedef int64_t i64;
typedef uint64_t u64;
typedef uint32_t u32;

// ---- scratch slots ----------------------------------------------------------------------------
// The growable device buffers of a context (pb3d_scratch).  Each has one of three lifetimes:
//   call-local  free again when the entry that requested it returns;
//   pair state  written by a *_count and read by its *_fill (struct pb3d_pair: the fill refuses if the slot was requested in between);
//   cache       kept across calls, keyed by scratch_gen / scratch_slot_gen.
// Two names with one value share the buffer on purpose.  The numbers are fixed: the order and sizes of an op's requests decide when
// a slot regrows, and a regrow synchronises the stream and drops the cached rotation tables (scratch_gen).
enum pb3d_slot : int {
    // call-local, csrc/api_host.hip (and the host flavours in mesh.hip, deform.hip): staged inputs and outputs of the host-pointer
    // entries.  Pair state of the host points / mesh pairs: their count leaves the staged grid in HOST_IN0 for the fill.
    PB3D_SLOT_HOST_IN0 = 0,
    PB3D_SLOT_HOST_OUT0 = 1,
    PB3D_SLOT_HOST_IN1 = 2,
    PB3D_SLOT_HOST_OUT1 = PB3D_SLOT_HOST_IN1,           // pb3d_mesh_fill's faces
    PB3D_SLOT_HOST_IN2 = 3,                             // pb3d_part_carve's carve masks
    PB3D_SLOT_HOST_OUT2 = PB3D_SLOT_HOST_IN2,           // pb3d_points_fill's colours, pb3d_mesh_fill's normals
    PB3D_SLOT_HOST_TMP = PB3D_SLOT_HOST_IN2,            // pb3d_process_grid's ping-pong volume
    // call-local, volume temporaries shared by part_carve (csrc/carve.hip), global_carve (global.hip), the label forms (label.hip),
    // CCL (ccl.hip), component statistics (components.hip), pb3d_try_part_carve90 (rotate_tiled.hip) and pb3d_mesh_fill (mesh.hip)
    PB3D_SLOT_VOL_OCC = 4,                              // occupancy / all-ones volume of a carve chain
    PB3D_SLOT_VOL_CARVED = 5,
    PB3D_SLOT_VOL_TMP = 6,
    PB3D_SLOT_VOL_KEEP = 7,
    PB3D_SLOT_MASK_WH = PB3D_SLOT_VOL_KEEP,             // global_carve / label forms: the transposed (W,H) mask
    PB3D_SLOT_PART90_JOBS = PB3D_SLOT_VOL_CARVED,       // pb3d_try_part_carve90: job bits per (x, y) column
    PB3D_SLOT_CCL_ROOT_BITS = PB3D_SLOT_VOL_CARVED,
    PB3D_SLOT_CCL_CHUNKS = PB3D_SLOT_VOL_TMP,
    PB3D_SLOT_STATS_BOXES = PB3D_SLOT_VOL_TMP,          // pb3d_component_stats_dev
    PB3D_SLOT_STATS_SUMS = PB3D_SLOT_VOL_KEEP,
    PB3D_SLOT_RECOLOR_FLAGS = PB3D_SLOT_VOL_TMP,        // the recolouring's per-component flags
    PB3D_SLOT_SELECT_FLAGS = PB3D_SLOT_VOL_KEEP,        // top-k / backward recolouring: the selection made on the device
    PB3D_SLOT_MESH_HOST_COLS = PB3D_SLOT_VOL_OCC,       // pb3d_mesh_fill's colours
    // call-local, csrc/points.hip: the count pass and its scan
    PB3D_SLOT_BLOCK_COUNTS = 8,
    PB3D_SLOT_SCAN_LOCAL = 11,
    PB3D_SLOT_SCAN_SEGS = 15,
    PB3D_SLOT_PROJ_WINNER = PB3D_SLOT_BLOCK_COUNTS,     // csrc/project.hip: winner images
    PB3D_SLOT_DEFORM_ACC = PB3D_SLOT_SCAN_LOCAL,        // csrc/deform.hip: sums, bounding box, out-of-bounds flag
    // pair state, csrc/points.hip: pb3d_points_count_dev -> pb3d_points_fill_dev (block offsets, 16-voxel selection masks)
    PB3D_SLOT_POINTS_OFFSETS = 9,
    PB3D_SLOT_POINTS_MASKS = 25,
    // call-local, csrc/points.hip: pb3d_points_extract_dev, apart from the pair above (it may run between the pair's halves)
    PB3D_SLOT_EXTRACT_OFFSETS = 24,
    PB3D_SLOT_EXTRACT_MASKS = 26,
    // pair state, csrc/deform.hip: pb3d_deform_count* -> pb3d_deform_fill* (with the points pair, which the count runs on it)
    PB3D_SLOT_DEFORM_MARKS = 12,
    PB3D_SLOT_DEFORM_BATCH_MARKS = PB3D_SLOT_DEFORM_MARKS,  // call-local: pb3d_deform_iou_batch_dev
    // call-local, csrc/deform.hip: pb3d_deform_fill_dev's points
    PB3D_SLOT_DEFORM_PTS = 13,
    PB3D_SLOT_DEFORM_COLS = 14,
    // call-local, csrc/project.hip and deform.hip: the camera / deformation batches
    PB3D_SLOT_PROJ_BATCH_CAMS = 20,
    PB3D_SLOT_PROJ_BATCH_COUNTS = 21,
    PB3D_SLOT_PROJ_BATCH_COLORS = 22,
    PB3D_SLOT_DEFORM_BATCH_TUPLES = PB3D_SLOT_PROJ_BATCH_CAMS,
    PB3D_SLOT_DEFORM_BATCH_COUNTS = PB3D_SLOT_PROJ_BATCH_COUNTS,
    // call-local, csrc/members.hip
    PB3D_SLOT_MEMBERS_COUNTS = 16,
    PB3D_SLOT_MEMBERS_OFFSETS = 17,
    // call-local, csrc/label.hip
    PB3D_SLOT_LABEL_FLAG = 23,
    // call-local, csrc/nn.hip: the cell index of the NN search, the bounds, the voxel IoU's bit grids
    PB3D_SLOT_NN_REF_COUNTS = 18,
    PB3D_SLOT_NN_REF_STARTS = 19,
    PB3D_SLOT_NN_REF_COORDS = 27,
    PB3D_SLOT_NN_QUERY_COUNTS = 28,
    PB3D_SLOT_NN_QUERY_STARTS = 29,
    PB3D_SLOT_NN_ORDER = 30,
    PB3D_SLOT_NN_SCAN_LOCAL = 31,
    PB3D_SLOT_NN_SCAN_SEGS = 33,
    PB3D_SLOT_NN_BOUNDS_PARTIALS = 41,
    PB3D_SLOT_NN_BOUNDS = 47,
    PB3D_SLOT_VIOU_BITS = 44,
    PB3D_SLOT_VIOU_DILATED = 45,
    // cache, csrc/rotate_tiled.hip: the validity table of the last 90-degree step (valid_cache)
    PB3D_SLOT_ROT_VALID_TABLE = 10,
    // call-local, csrc/rotate_tiled.hip: pb3d_try_part_carve90's transposed job bits
    PB3D_SLOT_PART90_JOBS_T = 46,
    // cache, csrc/sliced.hip: the tile programs of the bit-sliced chain (s32_cache)
    PB3D_SLOT_S32_TILE_PROGRAMS = 32,
    // call-local, csrc/sliced.hip
    PB3D_SLOT_SLICED_FLAG = 34,
    PB3D_SLOT_SLICED_MASK_BITS = 35,
    // call-local, csrc/guided.hip
    PB3D_SLOT_GUIDED_DESCS = 36,
    PB3D_SLOT_GUIDED_MASKS = 37,
    PB3D_SLOT_GUIDED_TABLES = 38,
    PB3D_SLOT_GUIDED_COUNTS = 39,
    PB3D_SLOT_GUIDED_SLICES = 43,
    // call-local, csrc/ccl.hip: counts and statistics records of a labelling (read by the caller of pb3d_ccl_label_on_device)
    PB3D_SLOT_CCL_RECORDS = 40,
    // cache, csrc/ccl.hip: the membership bits of the last labelled volume (ccl_last)
    PB3D_SLOT_CCL_MEMBER_BITS = 42,
    // pair state, csrc/mesh.hip: pb3d_mesh_count_dev -> pb3d_mesh_fill_dev (pb3d_mesh_colors_dev rebuilds MESH_BITS), and
    // pb3d_iso_count_resident -> pb3d_iso_fill_resident on the same slots: a count of either requests them, which ends the other's pending pair
    PB3D_SLOT_MESH_BITS = 48,
    PB3D_SLOT_MESH_VERT_OFFSETS = 51,
    PB3D_SLOT_MESH_FACE_OFFSETS = 52,
    // call-local, csrc/mesh.hip
    PB3D_SLOT_MESH_VERT_COUNTS = 49,
    PB3D_SLOT_MESH_FACE_COUNTS = 50,
    PB3D_SLOT_MESH_VSCAN_LOCAL = 53,
    PB3D_SLOT_MESH_VSCAN_SEGS = 54,
    PB3D_SLOT_MESH_FSCAN_LOCAL = 55,
    PB3D_SLOT_MESH_FSCAN_SEGS = 56,
    PB3D_SLOT_MESH_VERT_BASE = 57,
    // call-local, csrc/project.hip: pb3d_partwise_iou_dev's counters.  A slot of their own (they once shared POINTS_OFFSETS):
    // the IoU may run between the halves of a points pair
    PB3D_SLOT_IOU_COUNTS = 58,
    // call-local, csrc/nn.hip: pb3d_knn_dev's original index of each cell-sorted reference point (beside NN_REF_COORDS)
    PB3D_SLOT_KNN_REF_IDS = 59,
    // call-local, csrc/surface.hip: the index check's flag, face normals, the vertex -> incident-face lists and their scan
    PB3D_SLOT_SURF_FLAG = 60,
    PB3D_SLOT_SURF_FACE_NORMALS = 61,
    PB3D_SLOT_SURF_VERT_COUNTS = 62,
    PB3D_SLOT_SURF_VERT_STARTS = 63,
    PB3D_SLOT_SURF_INCIDENT = 64,
    PB3D_SLOT_SURF_SCAN_LOCAL = 65,
    PB3D_SLOT_SURF_SCAN_SEGS = 66,
    // call-local, csrc/density.hip: the bounds read back by the host, the u32 count volume (the filter's second pass writes its float32
    // result over it) and the filter weights.  Slots of their own: the bounds pass inside uses NN_BOUNDS_PARTIALS, nothing else
    PB3D_SLOT_DENSITY_BOUNDS = 67,
    PB3D_SLOT_DENSITY_COUNTS = 68,
    PB3D_SLOT_DENSITY_WEIGHTS = 69,
    // cache, csrc/icp.hip: the target's cell index of an alignment (icp_index) -- cell starts, cell-sorted SoA coordinates and each
    // sorted point's original position.  Slots of their own: the index outlives the call that builds it, and every other search
    // (NN_REF_*) may run between two steps
    PB3D_SLOT_ICP_INDEX_STARTS = 70,
    PB3D_SLOT_ICP_INDEX_COORDS = 71,
    PB3D_SLOT_ICP_INDEX_IDS = 72,
    // call-local, csrc/icp.hip: a step's transformed source points, their nearest target positions and the per-workgroup partial rows
    PB3D_SLOT_ICP_MOVED = 73,
    PB3D_SLOT_ICP_NEAREST = 74,
    PB3D_SLOT_ICP_PARTIALS = 75,
    // call-local, csrc/plane.hip: the per-workgroup partial rows of a plane refit; the crop's per-workgroup survivor counts, their
    // offsets and the two slots of its pb3d_scan_counts
    PB3D_SLOT_PLANE_PARTIALS = 76,
    PB3D_SLOT_CROP_COUNTS = 77,
    PB3D_SLOT_CROP_OFFSETS = 78,
    PB3D_SLOT_CROP_SCAN_LOCAL = 79,
    PB3D_SLOT_CROP_SCAN_SEGS = 80,
    // call-local, csrc/select.hip: the state (prefix, remaining rank) and the eight digit histograms of a k-th selection
    PB3D_SLOT_SELECT = 81,
    // call-local, csrc/icp.hip: a trimmed step's header (candidate count, rank, tau) and the selection keys of its pairs
    PB3D_SLOT_ICP_KEYS = 82,
    // call-local, csrc/meshdist.hip, the triangle index of pb3d_mesh_dist_resident (built by csrc/face_index.hip, as containment's
    // below, each in its caller's slots): the nf x 9 float64 corner table, the vertex box and the
    // entry total read back by the host, per-cell counts (then the scatter's cursors), cell starts, face ids in cell order and the two
    // slots of its pb3d_scan_counts.  The query half and the bounds pass inside use NN_QUERY_*, NN_ORDER, NN_SCAN_* and NN_BOUNDS_PARTIALS
    PB3D_SLOT_MESHD_CORNERS = 83,
    PB3D_SLOT_MESHD_READBACK = 84,
    PB3D_SLOT_MESHD_COUNTS = 85,
    PB3D_SLOT_MESHD_STARTS = 86,
    PB3D_SLOT_MESHD_IDS = 87,
    PB3D_SLOT_MESHD_SCAN_LOCAL = 88,
    PB3D_SLOT_MESHD_SCAN_SEGS = 89,
    // call-local, csrc/meshdist.hip, pb3d_mesh_sample_resident: the nf cumulative areas and the per-block totals / offsets
    PB3D_SLOT_MSAMPLE_CUM = 90,
    PB3D_SLOT_MSAMPLE_BLOCKS = 91,
    // call-local, csrc/cluster.hip, all of them: the cloud's cell index against itself (cell starts, cell-sorted SoA coordinates, each
    // sorted point's position in the caller's list), the union-find's parent per point, the root flags, their ranks (n + 1 int64) and
    // the two slots of that pb3d_scan_counts; the chosen-label table of pb3d_labels_member_resident.  Slots of their own: the index is
    // read by three walks with scans in between, and nothing of another op may sit under it.  The index build and the query order
    // inside use NN_REF_COUNTS, NN_QUERY_*, NN_ORDER, NN_SCAN_*, NN_BOUNDS and NN_BOUNDS_PARTIALS (call-local there as here: NN_ORDER
    // is read by every walk, and no entry of csrc/cluster.hip requests an NN_* slot between its order pass and its last walk)
    PB3D_SLOT_CLUSTER_STARTS = 92,
    PB3D_SLOT_CLUSTER_COORDS = 93,
    PB3D_SLOT_CLUSTER_IDS = 94,
    PB3D_SLOT_CLUSTER_PARENT = 95,
    PB3D_SLOT_CLUSTER_ROOT_FLAGS = 96,
    PB3D_SLOT_CLUSTER_RANKS = 97,
    PB3D_SLOT_CLUSTER_SCAN_LOCAL = 98,
    PB3D_SLOT_CLUSTER_SCAN_SEGS = 99,
    PB3D_SLOT_CLUSTER_CHOSEN = 100,
    // call-local, csrc/downsample.hip, all of them: the cloud's box read back by the host; the hash table (a power of two >= 2 n slots of 16
    // bytes: the 64-bit voxel key, the smallest position and the number of its points); each point's slot; the first-appearance flags (then the counts of a centroid call that was given no d_counts); their ranks
    // (n + 1 int64, then the m + 1 list starts) and the two slots of every pb3d_scan_counts of the call; the (voxel, position) pairs of
    // the stable sort (key, val and their ping-pong twins, n u32 each) and its run table (256 runs per tile of 2048 pairs: int64
    // starts, then u32 counts).  The bounds pass inside uses NN_BOUNDS_PARTIALS
    PB3D_SLOT_DOWNSAMPLE_BOUNDS = 101,
    PB3D_SLOT_DOWNSAMPLE_TABLE = 102,
    PB3D_SLOT_DOWNSAMPLE_POINT_SLOT = 103,
    PB3D_SLOT_DOWNSAMPLE_FLAGS = 104,
    PB3D_SLOT_DOWNSAMPLE_RANKS = 105,
    PB3D_SLOT_DOWNSAMPLE_SCAN_LOCAL = 106,
    PB3D_SLOT_DOWNSAMPLE_SCAN_SEGS = 107,
    PB3D_SLOT_DOWNSAMPLE_SORT_PAIRS = 108,
    PB3D_SLOT_DOWNSAMPLE_SORT_HIST = 109,
    // call-local, csrc/smooth.hip, all of them (P = 6 nf directed pairs): the pairs of the two stable sorts (key, val and their
    // ping-pong twins, P u32 each; the sorted (i, j) columns are read until the adjacency is complete) and the sorts' run table; the
    // "new pair" flags (P + 1 u32; once scanned, the position of every unique pair's first copy takes their place); their ranks
    // (P + 1 int64) and the two slots of every pb3d_scan_counts of the call; starts (nv + 1 int64), neighbours (P int32) and the
    // boundary bytes (nv, then ORed with the caller's fixed mask) of pb3d_mesh_smooth_resident, which pb3d_mesh_adjacency_resident
    // writes into its caller's buffers instead (it takes BOUNDARY only when it needs the bytes for nobody); the vertices above the
    // lane cutoff (a counter, then their numbers) and the two float64 position buffers (nv x 3 each) of the steps.  The index check
    // in front uses SURF_FLAG
    PB3D_SLOT_SMOOTH_PAIRS = 110,
    PB3D_SLOT_SMOOTH_SORT_HIST = 111,
    PB3D_SLOT_SMOOTH_FLAGS = 112,
    PB3D_SLOT_SMOOTH_RANKS = 113,
    PB3D_SLOT_SMOOTH_SCAN_LOCAL = 114,
    PB3D_SLOT_SMOOTH_SCAN_SEGS = 115,
    PB3D_SLOT_SMOOTH_STARTS = 116,
    PB3D_SLOT_SMOOTH_NEIGHBOURS = 117,
    PB3D_SLOT_SMOOTH_BOUNDARY = 118,
    PB3D_SLOT_SMOOTH_HUBS = 119,
    PB3D_SLOT_SMOOTH_POS_A = 120,
    PB3D_SLOT_SMOOTH_POS_B = 121,
    // call-local, csrc/voxelize.hip: the bit volume of pb3d_voxelize_mesh_resident (n0 * n1 columns of ceil(n2 / 32) + 1 dwords: 32
    // planes per dword and the column's overflow bit), the faces too wide for a lane (a counter, then their numbers: nf + 1 u32) and
    // five 64-bit words: the four stats and the flag of the index / finiteness check in front.  The three counts of
    // pb3d_grid_overlap_resident have a slot of their own: mesh_grid_iou runs the two back to back
    PB3D_SLOT_VOXELIZE_BITS = 122,
    PB3D_SLOT_VOXELIZE_LARGE = 123,
    PB3D_SLOT_VOXELIZE_COUNTS = 124,
    PB3D_SLOT_OVERLAP_COUNTS = 125,
    // call-local, csrc/edt.hip: the other half of the passes' ping-pong (the axis-1 pass writes it, the axis-0 pass reads it: one int32
    // per voxel for sq, one more for the partial index when d_index is given), the g values of the envelope stacks (one int32 per
    // voxel, level l of a column at the column's l-th voxel) and the counters (pb3d_edt_resident: targets, max sq + 1;
    // pb3d_grid_surface_stats_resident: its 3 + 8 words)
    PB3D_SLOT_EDT_SQ_TMP = 126,
    PB3D_SLOT_EDT_INDEX_TMP = 127,
    PB3D_SLOT_EDT_STACK = 128,
    PB3D_SLOT_EDT_COUNTS = 129,
    // call-local, csrc/render.hip: the camera coordinates of pb3d_render_mesh_resident (24 bytes per vertex), four 64-bit words (faces
    // pruned, on the small path, on the large path; then the flag of the index / finiteness check, later the tile-job total), the
    // winner image when the caller gave no d_face (one u32 per pixel), the tile jobs per face (nf u32), their offsets (nf + 1 int64)
    // and the two slots of that pb3d_scan_counts
    PB3D_SLOT_RENDER_CAMERA = 130,
    PB3D_SLOT_RENDER_COUNTS = 131,
    PB3D_SLOT_RENDER_WINNER = 132,
    PB3D_SLOT_RENDER_JOBS = 133,
    PB3D_SLOT_RENDER_OFFSETS = 134,
    PB3D_SLOT_RENDER_SCAN_LOCAL = 135,
    PB3D_SLOT_RENDER_SCAN_SEGS = 136,
    // call-local, csrc/simplify.hip, all of them.  What pb3d_voxel_downsample_resident leaves of the clusters (pb3d_mesh_simplify_resident
    // only: nv rows in the vertex dtype, nv int32 first vertices, nv int32 cluster numbers); each face's three clusters in the caller's
    // corner order (nf x 3 u32, read by every pass behind the map); the (key, position) pairs of the three stable sorts (key, val and
    // their ping-pong twins, nf u32 each; PB3D_FACES_DROP only) and the sorts' run table; the "face stays" flags (nf u32) and the
    // "cluster is named" flags (m u32), their ranks (nf + 1 and m + 1 int64) and the two slots of every pb3d_scan_counts of the call;
    // the two totals the host reads back.  The cluster pass inside uses the DOWNSAMPLE_* slots, the index check in front SURF_FLAG
    PB3D_SLOT_SIMPLIFY_CLUSTER_ROWS = 137,
    PB3D_SLOT_SIMPLIFY_CLUSTER_FIRST = 138,
    PB3D_SLOT_SIMPLIFY_CLUSTER_INVERSE = 139,
    PB3D_SLOT_SIMPLIFY_CORNERS = 140,
    PB3D_SLOT_SIMPLIFY_PAIRS = 141,
    PB3D_SLOT_SIMPLIFY_SORT_HIST = 142,
    PB3D_SLOT_SIMPLIFY_KEEP = 143,
    PB3D_SLOT_SIMPLIFY_USED = 144,
    PB3D_SLOT_SIMPLIFY_FACE_RANKS = 145,
    PB3D_SLOT_SIMPLIFY_VERTEX_RANKS = 146,
    PB3D_SLOT_SIMPLIFY_SCAN_LOCAL = 147,
    PB3D_SLOT_SIMPLIFY_SCAN_SEGS = 148,
    PB3D_SLOT_SIMPLIFY_COUNTS = 149,
    // call-local, csrc/meshcomp.hip, all of them (R = 3 nf edge records): each face's wrapped corners (nf x 3 u32); the (key, record)
    // pairs of the two stable sorts (key, val and their ping-pong twins, R u32 each; the measures' (label, face) sort takes the front
    // of them once the edges are counted) and the sorts' run table; the run-head flags and the forward bits (R u32 each), their ranks
    // (R + 1 int64 each) and the position of every edge's first record (R + 1 u32); the union-find's parent (per face under "edge",
    // per vertex under "vertex") and, under "vertex", each root's smallest face; the "first face of a component" flags (nf u32) and
    // their ranks (nf + 1 int64); the vertex labels before -1 is written (nv int32); the u32 face count and block count of every
    // component with their two scans (nf + 1 int64 each); A_j, S_j per face and the block sums (nf x 2 float64 each); the eight totals;
    // the two slots of every pb3d_scan_counts of the call.  The index check in front uses SURF_FLAG
    PB3D_SLOT_MESHCOMP_CORNERS = 150,
    PB3D_SLOT_MESHCOMP_PAIRS = 151,
    PB3D_SLOT_MESHCOMP_SORT_HIST = 152,
    PB3D_SLOT_MESHCOMP_FLAGS = 153,
    PB3D_SLOT_MESHCOMP_RANKS = 154,
    PB3D_SLOT_MESHCOMP_HEADS = 155,
    PB3D_SLOT_MESHCOMP_PARENT = 156,
    PB3D_SLOT_MESHCOMP_MIN_FACE = 157,
    PB3D_SLOT_MESHCOMP_ROOT_FLAGS = 158,
    PB3D_SLOT_MESHCOMP_ROOT_RANKS = 159,
    PB3D_SLOT_MESHCOMP_VERTEX_LABELS = 160,
    PB3D_SLOT_MESHCOMP_SEGMENTS = 161,
    PB3D_SLOT_MESHCOMP_MEASURES = 162,
    PB3D_SLOT_MESHCOMP_TOTALS = 163,
    PB3D_SLOT_MESHCOMP_SCAN_LOCAL = 164,
    PB3D_SLOT_MESHCOMP_SCAN_SEGS = 165,
    // call-local, csrc/inside.hip, all of them: the nf x 9 float64 corner table; eight 64-bit words the host reads back (the vertex box,
    // the entry total, the flag of the index / finiteness check in front); per-cell counts (then the scatter's cursors), cell starts,
    // face ids in cell order and the two slots of its pb3d_scan_counts; four 64-bit words (queries inside, with an odd total, faces
    // with area == 0, queries outside the box) and the three u32 partial counts of every workgroup of the query kernel.  The box
    // pass inside uses NN_BOUNDS_PARTIALS, and under knob "inside_order" = 1 the query order uses NN_QUERY_*, NN_ORDER and NN_SCAN_*
    PB3D_SLOT_INSIDE_CORNERS = 166,
    PB3D_SLOT_INSIDE_READBACK = 167,
    PB3D_SLOT_INSIDE_COUNTS = 168,
    PB3D_SLOT_INSIDE_STARTS = 169,
    PB3D_SLOT_INSIDE_IDS = 170,
    PB3D_SLOT_INSIDE_SCAN_LOCAL = 171,
    PB3D_SLOT_INSIDE_SCAN_SEGS = 172,
    PB3D_SLOT_INSIDE_STATS = 173,
    PB3D_SLOT_INSIDE_PARTIALS = 174,
    PB3D_SLOT_INSIDE_SETUP = 175,                       // knob "inside_table" = 1 only: 184 bytes of finished set-up per face
    // call-local, csrc/raycast.hip, all of them: the seven of its pb3d_face_index_build as above (the eighth read-back word is the flag
    // of the mesh check in front); under knob "raycast_stats" six 64-bit totals and the five u64 partial counts of every workgroup of
    // the query kernel.  The box pass inside uses NN_BOUNDS_PARTIALS
    PB3D_SLOT_RAYCAST_CORNERS = 176,
    PB3D_SLOT_RAYCAST_READBACK = 177,
    PB3D_SLOT_RAYCAST_COUNTS = 178,
    PB3D_SLOT_RAYCAST_STARTS = 179,
    PB3D_SLOT_RAYCAST_IDS = 180,
    PB3D_SLOT_RAYCAST_SCAN_LOCAL = 181,
    PB3D_SLOT_RAYCAST_SCAN_SEGS = 182,
    PB3D_SLOT_RAYCAST_STATS = 183,
    PB3D_SLOT_RAYCAST_PARTIALS = 184,
    // call-local, csrc/orient.hip.  The records, their sorts, flags, ranks and edge starts are csrc/meshcomp.hip's front half in the
    // MESHCOMP_* slots (pb3d_mesh_edge_records), and the signed sums its MESHCOMP_SEGMENTS / MESHCOMP_MEASURES (pb3d_mesh_ordered_sums).
    // Its own: the doubled forest's parent (2 nf int32: node j is face j as it came, node nf + j face j flipped); the "smallest face
    // of its patch" flags and the anchor-rule flip bits (nf u32 each); the flags' ranks (nf + 1 int64); area and volume per patch as
    // the sums leave them (2 nf float64); the eight totals
    PB3D_SLOT_ORIENT_PARENT = 185,
    PB3D_SLOT_ORIENT_FLAGS = 186,
    PB3D_SLOT_ORIENT_RANKS = 187,
    PB3D_SLOT_ORIENT_MEASURES = 188,
    PB3D_SLOT_ORIENT_TOTALS = 189,
    // call-local, csrc/weld.hip, all of them: the (key word, position) pairs of the three or six stable sorts (key, val and their
    // ping-pong twins, nv u32 each) and the sorts' run table; the run-head flags in sorted order and the "representative" flags in
    // input order (nv u32 each); their ranks (nv + 1 int64 each); where every run starts (nv + 1 u32), each vertex's representative
    // (nv int32) and each representative's class size (nv u32); the two slots of every pb3d_scan_counts of the call.  The class count the
    // host reads back is the last rank.  The index check in front uses SURF_FLAG
    PB3D_SLOT_WELD_PAIRS = 190,
    PB3D_SLOT_WELD_SORT_HIST = 191,
    PB3D_SLOT_WELD_FLAGS = 192,
    PB3D_SLOT_WELD_RANKS = 193,
    PB3D_SLOT_WELD_RUNS = 194,
    PB3D_SLOT_WELD_SCAN_LOCAL = 195,
    PB3D_SLOT_WELD_SCAN_SEGS = 196,

    PB3D_SLOT_COUNT = 197
};

// ---- the cell index of the exact nearest-neighbour search (csrc/nn.hip) -----------------------------------
struct pb3d_nn_grid {
    double lo[3], hi[3];      // the reference set's exact bounding box
    double inv[3], h[3];      // cells per unit length (0 on a one-cell axis) and cell width
    int n[3];                 // cells per axis
    i64 ncells;
};
// a reference set binned once and kept in the caller's slots (pb3d_nn_index_build); valid while those slots are
struct pb3d_nn_index {
    pb3d_nn_grid g;
    i64 nr;
    const i64* starts;        // ncells + 1 cell starts
    const double* xs;         // cell-sorted SoA coordinates: xs, xs + nr, xs + 2 nr
    const int* ids;           // position of each sorted point in the caller's list
};
constexpr i64 pb3d_max_points = (1ll << 31) - 1;      // of a point list: sorted positions, query slots and ids are 32-bit
// row i of a float32 or float64 (n, 3) point list, widened to double
template <bool F64>
__device__ __forceinline__ void pb3d_load3(const void* p, i64 i, double* x, double* y, double* z) {
    if (F64) {
        const double* d = (const double*)p + 3 * i;
        *x = d[0]; *y = d[1]; *z = d[2];
    } else {
        const float* f = (const float*)p + 3 * i;
        *x = (double)f[0]; *y = (double)f[1]; *z = (double)f[2];
    }
}
template <bool F64>
__device__ __forceinline__ void pb3d_load3(const void* p, i64 i, double v[3]) { pb3d_load3<F64>(p, i, &v[0], &v[1], &v[2]); }

// What a *_count leaves for its *_fill: the use counters (pb3d_ctx::scratch_use) of the slots the fill reads, taken when the count has
// written them.  The fill's arguments are kept next to it, in the pair's own record of pb3d_ctx.
struct pb3d_pair {
    bool valid;
    int nslots;
    pb3d_slot slot[3];
    u64 use[3];
};

#define PB3D_POOL_SLOTS 64
#define PB3D_POOL_LIVE 4096

struct pb3d_event {
    hipEvent_t ev;
};

struct pb3d_ctx {
    int device;
    int cus;
    hipStream_t stream;
    bool orient_lds_set;        // ... and for the 128-pixel orientation kernel (csrc/components.hip)
    bool guided_lds_set;        // ... and for the crop-chain kernel of left_right_guided_carve (csrc/guided.hip)
    // development knobs, read from the environment ONCE in pb3d_create (never on a launch path)
    // (round 4: every knob has a name -- the numbered "misc" switches of rounds 1-3 are gone; PB3D_KNOBS="name=value,..." sets any of them at pb3d_create)
    int tune_rot90_fill;        // knob "rot90_fill": workgroups per CU in the grid of the 90-degree kernels (0 = the built-in rule)
    int tune_rot90_order;       // knob "rot90_order": 1 = tiles in plain x-fastest order instead of one plane chunk per XCD
    int tune_rot90_flat;        // knob "rot90_flat": 0 = choose, 1 = never the flat (stream) forms: the row-wise tile kernel, 2 = flat only on whole-line streams
    int tune_rot90_mask_block;  // knob "rot90_mask_block": 1 = the 90-degree kernels fetch their mask bytes per plane / segment instead of once into LDS
    int tune_orient_tile;       // knob "orient_tile": 1 = pb3d_orient_dev without its 128-pixel tile kernel
    int tune_global_composed;   // knob "global_composed": 1 = global_carve with other angle steps as ones -> process -> colour (parity tests run both)
    int tune_per_job;           // knob "per_job": 1 = part_carve's jobs one by one, RGB and label form alike (no fused 90-degree sweep, no merged pass); label form of global_carve(90) by the composed pipeline
    int tune_no_table_cache;    // knob "no_table_cache": 1 = validity tables and tile programs are rebuilt on every call
    int tune_part90_inflight;   // knob "part90_inflight": 10 UA + UE, items in flight per thread in the source / output pass of k_part90_plane (0 = 2 / 4)
    int tune_crop_ablate;       // knob "crop_ablate": ablation switches of k_crop_chain (tools/cropabl.py)
    int tune_uncap;             // PB3D_UNCAP=1: every grid-stride kernel gets one workgroup per tile (A/B of the persistent grids)
    int tune_sliced;            // PB3D_SLICED: 0 = rotation steps on 0/1 data run bit-sliced (csrc/sliced.hip), 1 = never (byte chain, arithmetic kernel)
    int tune_rot90_wide;        // PB3D_ROT90_WIDE: 1 = the 256 x 256-tile form of the 90-degree step (development A/B)
    bool rot90w_lds_set;
    bool part90_lds_set;        // k_part90_plane has been given its large dynamic LDS limit
    bool rot90wf_lds_set;       // ... and for its form on the rows' (y, z) streams (odd row lengths)
    int tune_s32_order;         // knob "s32_order": 1 = the slice / un-slice passes walk x fastest (round 3's order; development A/B)
    int tune_s32_fuse_last;     // knob "s32_fuse_last": 1 = the chain's last 90-degree step stays a table step (development A/B)
    int tune_s32_gpw;           // PB3D_S32_GPW: plane groups per workgroup of the sliced step kernel (0 = choose)
    int tune_ccl_blocks;        // knob "ccl_blocks": workgroups per CU of the labelling's last pass (0 = default)
    int tune_ccl_init_blocks;   // knob "ccl_init_blocks": workgroups per CU of the labelling's first pass (0 = 16)
    int tune_ccl_tilecols;      // knob "ccl_tilecols": windows per level of a plane-to-plane merge tile (0 = 32)
    int tune_ccl_merge;         // knob "ccl_merge": 0 = tile kernels where the rows fit, 1 = always the pairwise kernel (development A/B)
    int tune_cluster_cell;      // knob "cluster_cell": cell edge of csrc/cluster.hip's index: 0 = the built-in rule, 1 = make_grid's (2 points per cell), 2 = above eps
    int tune_cluster_timing;    // knob "cluster_timing": 1 = pb3d_cluster_points_resident times its passes with events (one more host wait)
    // the last pb3d_cluster_points_resident / pb3d_radius_count_resident (csrc/cluster.hip) for pb3d_cluster_last: cells per axis of its
    // index, and with cluster_timing the milliseconds of its passes (index, count, union + flatten, ranks, labels)
    struct ClusterLast { bool valid, timed; float ms[5]; i64 cells[3]; } cluster_last;
    int tune_voxelize_timing;   // knob "voxelize_timing": 1 = pb3d_voxelize_mesh_resident times its two passes with events (one more host wait)
    // the last pb3d_voxelize_mesh_resident (csrc/voxelize.hip) for pb3d_voxelize_last: with voxelize_timing the milliseconds of the
    // crossing pass (bit-volume clear included) and of the scan pass
    struct VoxelizeLast { bool valid, timed; float ms[2]; } voxelize_last;
    int tune_render_timing;     // knob "render_timing": 1 = pb3d_render_mesh_resident times its passes with events (one more host wait)
    // the last pb3d_render_mesh_resident (csrc/render.hip) for pb3d_render_last: faces pruned, on the small path, on the large path and
    // tile jobs; with render_timing the milliseconds of its passes (faces depth + scan, tiles depth, faces face, tiles face, resolve)
    struct RenderLast { bool valid, timed; float ms[5]; i64 stats[4]; } render_last;
    int tune_iso_timing;        // knob "iso_timing": 1 = pb3d_iso_count_resident / pb3d_iso_fill_resident time their passes with events (the fill waits once more)
    // the last isosurface pair (csrc/mesh.hip) for pb3d_iso_last: with iso_timing the milliseconds of the bits pass, of the count and
    // its two scans (both stamped by the count), of the vertex pass and of the faces (both stamped by the fill)
    struct IsoLast { bool count_timed, fill_timed; float ms[4]; } iso_last;
    int tune_simplify_timing;   // knob "simplify_timing": 1 = pb3d_mesh_simplify_resident / pb3d_mesh_compact_resident time their passes with events (one more host wait)
    // the last of the two (csrc/simplify.hip) for pb3d_simplify_last: clusters, vertices out, faces out; with simplify_timing the
    // milliseconds of its passes (clusters, map, sorts + repeats, scans, gathers)
    struct SimplifyLast { bool valid, timed; float ms[5]; i64 counts[3]; } simplify_last;
    int tune_inside_timing;     // knob "inside_timing": 1 = pb3d_points_in_mesh_resident times its index build and its query with events (one more host wait)
    int tune_inside_order;      // knob "inside_order": 0 = queries in input order, 1 = in the cell order of the index (csrc/nn.hip's query binning)
    int tune_inside_table;      // knob "inside_table": 0 = the query recomputes a face's set-up from its 72-byte corner row, 1 = it reads a 184-byte row of finished set-ups (development A/B)
    // the last pb3d_points_in_mesh_resident (csrc/inside.hip) for pb3d_points_in_mesh_last: cells along a0 and a1 of its index, (cell, face)
    // entries and halvings, as pb3d_face_index_build reports them; with inside_timing the milliseconds of the index build and of the query
    struct InsideLast { bool valid, timed; float ms[2]; i64 info[4]; } inside_last;
    int tune_raycast_timing;    // knob "raycast_timing": 1 = pb3d_cast_rays_resident times its index build and its query with events (one more host wait)
    int tune_raycast_stats;     // knob "raycast_stats": 1 = pb3d_cast_rays_resident counts hits, bad rays, face tests and cells for pb3d_cast_rays_last (one more host wait)
    // the last pb3d_cast_rays_resident (csrc/raycast.hip) for pb3d_cast_rays_last / _last_ms: the six counts of a call under
    // raycast_stats, the milliseconds of the index build and of the query of a call under raycast_timing
    struct RaycastLast { bool counted, timed; float ms[2]; i64 stats[6]; } raycast_last;
    // Growable device scratch slots, named by enum pb3d_slot (no hipMalloc / hipFree per call once warm).
    void* scratch[PB3D_SLOT_COUNT];
    size_t scratch_bytes[PB3D_SLOT_COUNT];
    // small pinned host area for counters read back from the device; who owns which bytes: pb3d_pinned_* below
    void* pinned;
    size_t pinned_bytes;
    // pinned staging ring of pb3d_h2d_async: small host inputs (2-D masks, descriptors) go up without a host wait
    void* stage;
    size_t stage_bytes, stage_head;
    u64 sync_count;             // host waits on the context's stream so far (pb3d_sync_count: tests bound the waits of a pipeline)
    // count -> fill pairs (pb3d_pair_record / pb3d_pair_check): each count's record and the arguments its fill repeats.  The host
    // flavours' grids are staged in PB3D_SLOT_HOST_IN0; pb3d_deform_count* runs the device points pair on PB3D_SLOT_DEFORM_MARKS.
    // The argument records are compared byte for byte (pb3d_same_args): 8-byte members only, unused colour bytes zero.
    struct PointsArgs { const void* grid; i64 A0, A1, A2, n, C, ncolors, stride; u8 colors[3 * 32]; };
    struct { pb3d_pair pair; PointsArgs a; } pts_dev, pts;
    struct MeshArgs { const void* grid; i64 A0, A1, A2, nv, nf, C, stride; };
    struct { pb3d_pair pair; MeshArgs a; } mesh_dev, mesh;
    // level and divisor by their bits (float64, float32): a record compared byte for byte holds no floating-point member
    struct IsoArgs { const void* vol; i64 n0, n1, n2, nv, nf; u64 level_bits, divisor_bits; };
    struct { pb3d_pair pair; IsoArgs a; } iso_dev, iso;
    struct { pb3d_pair pair; int ox, oy, oz; i64 X, Y, Z, n; } deform;
    struct ValidCache { void* buf; u64 gen; i64 W, D; double p[8]; } valid_cache;   // validity bit table of the last 90-degree step (PB3D_SLOT_ROT_VALID_TABLE)
    // Tile programs of the bit-sliced chain (csrc/sliced.hip, PB3D_SLOT_S32_TILE_PROGRAMS): valid for these steps on this (W, D)
    struct S32Cache { bool valid; u64 gen; i64 W, D; int ns; double p[32 * 8]; } s32_cache;
    hipEvent_t s32_ev;          // recorded behind the slice kernel's "not 0/1" flag copy
    // membership bits of the last labelled volume (csrc/ccl.hip, PB3D_SLOT_CCL_MEMBER_BITS): word row * P + t, bit = voxel is a member
    // of colour k (K colours labelled together, csrc/ccl.hip: their numbering is per colour, so a label needs its colour's bits to mean anything
    // once K > 1).  gen = scratch_slot_gen[PB3D_SLOT_CCL_MEMBER_BITS] when the bits were written: only a reallocation of THAT slot invalidates them.
    struct CclLast { bool valid; const void* labels; const void* bits; i64 rows, A2, P; u64 gen; bool members_only; int K, C; u32 colors[PB3D_CCL_MAX_COLORS]; } ccl_last;
    // the target index of an alignment (csrc/icp.hip, PB3D_SLOT_ICP_INDEX_*): built by pb3d_icp_index_resident for this (pointer, count,
    // width), read by every pb3d_icp_step_resident.  gen = scratch_slot_gen of the three slots when it was written.
    struct IcpIndex { bool valid; const void* tgt; i64 nt; int f64; u64 gen[3]; pb3d_nn_index ix; } icp_index;
    // the triangle index of the last pb3d_mesh_dist_resident (csrc/meshdist.hip, from pb3d_face_index_build), for pb3d_mesh_grid_shape:
    // cells per axis, (cell, face) entries, and how often the grid was coarsened to respect the entry cap
    struct MeshGridLast { bool valid; i64 cells[3], entries, coarsenings; } mesh_grid_last;
    // Device block pool behind pb3d_dev_alloc / pb3d_dev_free: a freed block is kept (no hipFree, no stream synchronisation) and handed
    // to the next request of about its size.  Everything that touches such a block runs on ctx->stream, in order, so a re-used block
    // is never written before its previous reader has finished.  The NumPy-signature API allocates and frees a volume-sized buffer
    // or two per call: with hipMalloc / hipFree (which waits for the device) that was most of a notebook-1 run's wall time.
    struct PoolBlock { void* p; size_t bytes; u64 stamp; };
    PoolBlock pool_free[PB3D_POOL_SLOTS];
    int pool_nfree;
    PoolBlock pool_live[PB3D_POOL_LIVE];
    int pool_nlive;
    size_t pool_cached, pool_cap;       // bytes held in pool_free; its limit (PB3D_DEVICE_POOL_MB, default a quarter of the HBM, 0 = off)
    u64 pool_stamp;
    u64 scratch_gen;            // bumped whenever ANY scratch slot is reallocated (cached tables in other slots may have moved)
    u64 scratch_slot_gen[PB3D_SLOT_COUNT];  // ... and per slot
    u64 scratch_use[PB3D_SLOT_COUNT];       // requests of each slot, regrown or not (struct pb3d_pair)
    // RCCL (loaded lazily with dlopen; see comm.hip)
    void* rccl_lib;
    void* rccl_comm;
    int rank, nranks;
};

// ---- error plumbing -------------------------------------------------------------------------
void pb3d_set_error(const char* fmt, ...);

#define PB3D_HIP(call)                                                                          \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess) {                                                                 \
            pb3d_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return e_ == hipErrorOutOfMemory ? PB3D_ENOMEM : PB3D_ENODEVICE;                    \
        }                                                                                       \
    } while (0)

#define PB3D_TRY(call)                 \
    do {                               \
        int rc_ = (call);              \
        if (rc_ != PB3D_OK) return rc_; \
    } while (0)

#define PB3D_REQUIRE(cond, ...)         \
    do {                                \
        if (!(cond)) {                  \
            pb3d_set_error(__VA_ARGS__); \
            return PB3D_EINVAL;         \
        }                               \
    } while (0)

#define PB3D_CHECK_LAUNCH() PB3D_HIP(hipGetLastError())

// scratch slot `slot` grown to at least `bytes`; counts the request in scratch_use[slot]
int pb3d_scratch(pb3d_ctx* ctx, pb3d_slot slot, size_t bytes, void** out);

// ---- count / fill pairs ---------------------------------------------------------------------
// A count records the slots (at most 3) its fill will read once it has written them; the fill calls pb3d_pair_check before any device work.
void pb3d_pair_record(pb3d_ctx* ctx, pb3d_pair* pr, std::initializer_list<pb3d_slot> slots);
// PB3D_OK if the count's state is still there: recorded, none of its slots requested since, and the fill repeats the count's
// arguments (same_args).  Else PB3D_EINVAL with a message that names the pair.
int pb3d_pair_check(const pb3d_ctx* ctx, const pb3d_pair& pr, bool same_args, const char* fill, const char* count);
template <class Args>
bool pb3d_same_args(const Args& a, const Args& b) {
    static_assert(std::has_unique_object_representations_v<Args>, "an argument record compared byte for byte must have no padding");
    return memcmp(&a, &b, sizeof(Args)) == 0;
}
// the points pair's argument record; colors: ncolors RGB triples, or ncolors 1-byte labels when C == 1 (0 <= ncolors <= 32)
static inline pb3d_ctx::PointsArgs pb3d_points_args(const void* grid, i64 A0, i64 A1, i64 A2, int C, const u8* colors, int ncolors,
                                                    int stride, i64 n) {
    pb3d_ctx::PointsArgs a{grid, A0, A1, A2, n, C, ncolors, stride, {}};
    if (ncolors) memcpy(a.colors, colors, (size_t)(C == 1 ? 1 : 3) * ncolors);
    return a;
}
// hipStreamSynchronize(ctx->stream) + bookkeeping (the staging ring is empty afterwards)
int pb3d_stream_sync(pb3d_ctx* ctx);
// ---- the pinned read-back area (pb3d_ctx::pinned), three disjoint regions:
//   [0, pb3d_pinned_head)                  pb3d_read_back: complete when the call returns, so free again for the next one
//   [pb3d_pinned_ccl, ... - flag)          csrc/ccl.hip's counts and statistics block (it static_asserts that it ends before the flag)
//   the last pb3d_pinned_flag bytes        csrc/sliced.hip's "not 0/1" word: its copy completes behind an event (s32_ev), not behind
//                                          the caller's next wait, so nothing else may ever be written there
constexpr size_t pb3d_pinned_bytes = 1 << 16;
constexpr size_t pb3d_pinned_ccl = 1024;
constexpr size_t pb3d_pinned_head = pb3d_pinned_ccl;
constexpr size_t pb3d_pinned_flag = 64;
// d_src[0, bytes) -> host_dst through the head of the pinned area: one copy, one host wait (pb3d_stream_sync), one memcpy out
int pb3d_read_back(pb3d_ctx* ctx, void* host_dst, const void* d_src, size_t bytes);

// The time stamps of an entry's passes (the *_timing knobs; off: nothing happens): N events, created per call, mark() records the
// next one.  read() wants the stream waited for and gives the milliseconds between consecutive marks; *timed = all N were made.
// finish() is the one more host wait, then read()
template <int N>
struct pb3d_stamps {
    bool on;
    int k;
    hipEvent_t ev[N];
    int mark(pb3d_ctx* ctx) {
        if (!on) return PB3D_OK;
        PB3D_HIP(hipEventCreate(&ev[k]));
        PB3D_HIP(hipEventRecord(ev[k], ctx->stream));
        ++k;
        return PB3D_OK;
    }
    int read(float* ms, bool* timed) {
        if (!on) return PB3D_OK;
        for (int i = 0; i + 1 < k; ++i) PB3D_HIP(hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]));
        *timed = k == N;
        return PB3D_OK;
    }
    int finish(pb3d_ctx* ctx, float* ms, bool* timed) {
        if (!on) return PB3D_OK;
        PB3D_TRY(pb3d_stream_sync(ctx));
        return read(ms, timed);
    }
    ~pb3d_stamps() { for (int i = 0; i < k; ++i) (void)hipEventDestroy(ev[i]); }
};

// grid size for grid-stride streaming kernels: enough blocks to fill 256 CUs, capped
// blocks_per_cu <= 0: no cap -- one workgroup per tile of the stream.  For write-heavy or latency-heavy streams the dispatcher balances
// many small workgroups better than a persistent grid-stride loop does (colour apply 0.84 -> 0.70 ms, float32 projection 1.03 -> 0.90 ms
// at 1024^3); kernels with per-workgroup set-up or flush (component statistics) want the cap.
static inline unsigned pb3d_stream_blocks(const pb3d_ctx* ctx, i64 work_items, int per_block, int blocks_per_cu) {
    i64 need = (work_items + per_block - 1) / per_block;
    i64 cap = (blocks_per_cu > 0 && !ctx->tune_uncap) ? (i64)(ctx->cus > 0 ? ctx->cus : 256) * blocks_per_cu : 0x7fffffffll;
    if (need < 1) need = 1;
    return (unsigned)(need < cap ? need : cap);
}

// blocks per batch item of a (blocks, batch) grid: enough for one item's work, and no more than blocks_per_cu per CU for the
// whole batch together (at least one)
static inline unsigned pb3d_batch_blocks(const pb3d_ctx* ctx, i64 work_items, int per_block, i64 batch, int blocks_per_cu) {
    i64 need = (work_items + per_block - 1) / per_block;
    const i64 cap = ((i64)ctx->cus * blocks_per_cu + batch - 1) / batch;
    if (need > cap) need = cap;
    return (unsigned)(need < 1 ? 1 : need);
}

// ---- exact u32 division by a run-time constant (Granlund-Montgomery round-up form): q = (t + ((n - t) >> sa)) >> sb, t = mulhi(m, n).
// A 64-bit integer division is ~100 vector instructions on gfx950 and the VALU issues one wave instruction per four cycles: kernels
// that turn a linear voxel index into coordinates with / and % are bound by exactly that.
struct pb3d_magic { u32 m; int sa, sb; u32 d; };
static inline pb3d_magic pb3d_make_magic(u32 d) {     // 1 <= d < 2^31
    int L = 0;
    while ((1ull << L) < d) ++L;
    pb3d_magic g;
    g.m = (u32)(((1ull << 32) * ((1ull << L) - d)) / d + 1);
    g.sa = L < 1 ? L : 1;
    g.sb = L > 1 ? L - 1 : 0;
    g.d = d;
    return g;
}
__device__ __forceinline__ u32 pb3d_div(u32 n, const pb3d_magic g) {
    const u32 t = __umulhi(g.m, n);
    return (t + ((n - t) >> g.sa)) >> g.sb;
}

// splitmix64's finaliser.  The generator's step is pb3d_mix64(z + 0x9e3779b97f4a7c15) (csrc/synth.hip, the sampler of csrc/meshdist.hip);
// csrc/downsample.hip hashes its voxel keys with the finaliser alone
__host__ __device__ inline u64 pb3d_mix64(u64 z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// what a labelling leaves on the device (csrc/ccl.hip): total[k] = components of colour k, records[(k * dcap + c) * 64] = 64-byte statistics
// record of component c + 1 {int lo[3], hi[3] (inclusive), pad[2]; u64 count, sum[3]}, valid for c < min(total[k], dcap)
struct pb3d_ccl_dev { const i64* total; const char* records; int dcap; };
int pb3d_ccl_label_on_device(pb3d_ctx* ctx, const uint8_t* d_grid, int64_t A0, int64_t A1, int64_t A2, const uint8_t color[3], int channels, int32_t* d_labels,
                             int64_t cap, pb3d_ccl_dev* dev, int connectivity = 6);

// ---- kernels' host launchers used across translation units ---------------------------------
// exclusive scan of n u32 counts into n + 1 int64 offsets (the last = total) with points.hip's scan kernels; scratch slots local_slot, seg_slot
int pb3d_scan_counts(pb3d_ctx* ctx, const u32* d_counts, i64 n, i64* d_offsets, pb3d_slot local_slot, pb3d_slot seg_slot);
// the two slots grown for a scan of n counts (pb3d_scan_counts does it itself): a caller with several scans ahead reserves for the
// largest first, so that no slot regrows (and waits) midway
int pb3d_scan_reserve(pb3d_ctx* ctx, i64 n, pb3d_slot local_slot, pb3d_slot seg_slot);
// csrc/sort_pairs.hip for csrc/downsample.hip and csrc/smooth.hip: the n >= 1 pairs (key[i], val[i]) sorted stably by key < m
// (2 <= m <= 2^32: with m = 2^32 every bit of the key counts, as csrc/weld.hip's coordinate words need), through
// the ping-pong twins key2 / val2 (four arrays of n u32, none overlapping).  *key_sorted (unless null) and *val_sorted = the two of
// the four that hold the result.  hist_slot takes the run table (256 runs per tile of pb3d_sort_tile pairs: int64 starts, then u32
// counts); the scans inside use scan_local_slot and scan_segs_slot, for pb3d_sort_scan_items(n) counts each.  Enqueued
constexpr int pb3d_sort_tile = 2048;
inline i64 pb3d_sort_scan_items(i64 n) { return 256 * ((n + pb3d_sort_tile - 1) / pb3d_sort_tile); }   // the counts one pass of n pairs scans
int pb3d_sort_pairs(pb3d_ctx* ctx, u32* key, u32* val, u32* key2, u32* val2, i64 n, i64 m, pb3d_slot hist_slot, pb3d_slot scan_local_slot,
                    pb3d_slot scan_segs_slot, const u32** key_sorted, const u32** val_sorted);
// csrc/nn.hip: the exact bounding box of n >= 1 points on the host: bounds kernel into `slot` (>= 6 doubles), pb3d_read_back; one host wait
int pb3d_points_box(pb3d_ctx* ctx, const void* d_pts, int f64, i64 n, pb3d_slot slot, double b[6]);
// csrc/nn.hip for csrc/icp.hip: bin the nr >= 1 reference points (one host wait for the exact box) into the three given slots; then,
// any number of times, the position in the reference list of the nearest point ((d2, position) smallest: pb3d_knn_dev with k = 1) of
// each of nq float64 queries -> d_idx (enqueued; only the query binning is redone)
int pb3d_nn_index_build(pb3d_ctx* ctx, const void* d_r, int r_f64, i64 nr, pb3d_slot starts_slot, pb3d_slot coords_slot, pb3d_slot ids_slot,
                        pb3d_nn_index* ix);
// ... in cells whose edge exceeds min_edge (min_edge <= 0: pb3d_nn_index_build), never more cells than that grid has (csrc/cluster.hip)
int pb3d_nn_index_build_edge(pb3d_ctx* ctx, const void* d_r, int r_f64, i64 nr, double min_edge, pb3d_slot starts_slot, pb3d_slot coords_slot,
                             pb3d_slot ids_slot, pb3d_nn_index* ix);
int pb3d_nn_index_nearest(pb3d_ctx* ctx, const pb3d_nn_index& ix, const double* d_q, i64 nq, int* d_idx);
// csrc/nn.hip for csrc/meshdist.hip: the positions of the nq >= 1 queries in the cell order of grid g -> *order (PB3D_SLOT_NN_ORDER;
// enqueued)
int pb3d_nn_order_queries(pb3d_ctx* ctx, const void* d_q, int q_f64, i64 nq, const pb3d_nn_grid& g, const u32** order);
// csrc/face_index.hip for csrc/meshdist.hip and csrc/inside.hip: the triangle cell index of a mesh (face indices checked; nv, nf >= 1)
// in the caller's slots -- cell starts, face ids in cell order, the nf x 9 float64 corner table -- with the (cell, face) entries and
// the halvings of the grid that the entry cap asked for.  axes: 3, or 2 for one cell along a2; skip_flat: a face without an area in
// (a0, a1) is listed nowhere; d_flat: where those faces are counted, or null.  PB3D_EINVAL "<what>: the vertices must be finite" on a
// box that is not.  Host waits: the box and 1 + halvings entry counts; the rest is enqueued.  The read-back slot takes eight 64-bit
// words: the box at [0, 6), the entry total at [6], and [7] is the caller's
struct pb3d_face_index { pb3d_nn_grid g; const i64* starts; const int* ids; const double* tri; i64 entries, coarsenings; };
struct pb3d_face_index_slots { pb3d_slot corners, readback, counts, starts, ids, scan_local, scan_segs; };
int pb3d_face_index_build(pb3d_ctx* ctx, const char* what, const void* d_verts, int verts_f64, i64 nv, const void* d_faces, int faces_i64, i64 nf,
                          int axes, bool skip_flat, u64* d_flat, const pb3d_face_index_slots& slots, pb3d_face_index* out);
// csrc/select.hip for csrc/icp.hip: pb3d_kth_smallest_resident with the rank read from device memory when the selection runs
// (0 <= *d_rank < n; 1 <= n <= 2^31 - 1; enqueued)
int pb3d_select_kth(pb3d_ctx* ctx, const double* d_vals, i64 n, const i64* d_rank, double* d_out);
// csrc/surface.hip for csrc/normals.hip: PB3D_EINDEX (message "<what>: index out of bounds ...") if any of the n int32 (int64 with
// i64_entries) values of d_idx is outside [lo, hi); the flag is in PB3D_SLOT_SURF_FLAG; one host wait
int pb3d_check_index_range(pb3d_ctx* ctx, const void* d_idx, int i64_entries, i64 n, i64 lo, i64 hi, const char* what);
// csrc/meshcomp.hip for itself and csrc/orient.hip: the edge records of a checked face list (nv, nf >= 1; R = 3 nf), in the MESHCOMP_*
// slots.  _reserve requests them (before the caller enqueues anything, so that no regrow waits midway); _build enqueues k_records,
// the two stable sorts, k_heads, the two scans and k_head_positions.  face_parent (or null): nf entries that k_records sets to their
// own position and k_heads unites across every shared edge (mesh_components under "edge").  loops: where the loop records are added
struct pb3d_edge_records {
    u32* W;                   // nf x 3 wrapped corners
    u32* pairs;               // 4 R u32: the sorts' arrays; `val` is one of them, the other three are spent after _build
    const u32* val;           // R records in (lo, hi, record) order, the loops last
    u32 *head, *fwd;          // R each: first record of its undirected edge; source is lo
    i64 *head_rank, *fwd_rank;  // R + 1 each: exclusive scans of the two; head_rank[R] = the number of edges E
    u32* pos;                 // E + 1: where edge e's records start; pos[E] = behind the last record that is no loop
};
int pb3d_mesh_edge_records_reserve(pb3d_ctx* ctx, i64 nf, pb3d_edge_records* rec);
int pb3d_mesh_edge_records_build(pb3d_ctx* ctx, const void* d_faces, int faces_i64, i64 nf, i64 nv, int* face_parent, unsigned long long* loops,
                                 pb3d_edge_records* rec);
// ... a forest of n entries, each its own root; and every entry replaced by its root (root_flag, or null: 1 where entry == root)
int pb3d_forest_init(pb3d_ctx* ctx, int* parent, i64 n);
int pb3d_forest_flatten(pb3d_ctx* ctx, i64 n, int* parent, u32* root_flag);
// ... the ordered sums of A_j and S_j (include/pb3d.h, mesh_components MEASURES) per label: measures[l] = area, measures[nc + l] =
// volume for the *nc labels that face_labels holds, faces_of[l] faces each.  negate (or null): nf u32, S_j enters with a minus where
// it is not 0.  _reserve requests MESHCOMP_SEGMENTS (extra_bytes more behind its tables, for the caller) and, with `sums`,
// MESHCOMP_MEASURES; the (label, face) sort runs in rec.pairs, which spends rec.val
int pb3d_mesh_ordered_sums_reserve(pb3d_ctx* ctx, i64 nf, bool sums, size_t extra_bytes, void** extra);
int pb3d_mesh_ordered_sums(pb3d_ctx* ctx, const void* d_verts, int verts_f64, const pb3d_edge_records& rec, i64 nf, const int* face_labels,
                           const u32* negate, const unsigned long long* faces_of, const i64* nc, double* measures);
// process_voxel_grid through the bit-sliced chain (csrc/sliced.hip); *took = 0: not applicable, nothing written
int pb3d_process_grid_sliced(pb3d_ctx* ctx, const u8* d_occ, i64 W, i64 H, i64 D, const u8* d_mask_wh, int angle_interval, u8* d_out,
                             int known_binary, int* took);
int pb3d_global_carve_sliced(pb3d_ctx* ctx, const u8* d_mask_wh, const u8* d_rgb_hw3, i64 W, i64 H, i64 D, int angle_interval, u8* d_out_rgb,
                             int* took);
// pb3d_process_grid_dev for callers whose grid is 0/1 by construction (occupancy of a colour grid, all-ones): no host wait
int pb3d_process_grid_binary_dev(pb3d_ctx* ctx, const u8* d_occ, i64 W, i64 H, i64 D, const u8* d_mask_wh, int angle_interval, u8* d_out,
                                 u8* d_tmp);
// one rotation step with the caller's matrix through the bit-sliced path (csrc/sliced.hip); *took = 0: not applicable
int pb3d_rotate_step_sliced(pb3d_ctx* ctx, const u8* d_occ, i64 W, i64 H, i64 D, const double M[9], const double off[3], const u8* d_mask_wh, u8* d_out,
                            int* took);
// the arithmetic kernel (csrc/rotate.hip): any uint8 data, any rotation about Y
int pb3d_launch_rotate_generic(pb3d_ctx* ctx, const u8* d_in, i64 W, i64 H, i64 D, const double M[9],
                               const double off[3], const u8* d_mask_wh, u8* d_out, const u8* d_mask_src);
bool pb3d_is_perm_step(const double M[9], const double off[3], i64 W, i64 D);
int pb3d_perm_valid_table(pb3d_ctx* ctx, const double M[9], const double off[3], i64 W, i64 D, u32** bits, int* nw, int* c0, int* c2, bool* rot90);
bool pb3d_perm_step_ok(const double M[9], const double off[3], i64 W, i64 D, const void* a, const void* b);
int pb3d_launch_rotate_perm(pb3d_ctx* ctx, const u8* d_in, i64 W, i64 H, i64 D, const double M[9], const double off[3],
                            const u8* d_mask_src, const u8* d_mask_dst, u8* d_out);
int pb3d_try_part_carve90(pb3d_ctx* ctx, const u8* d_colored, int C, i64 W, i64 H, i64 D, const u8* d_mask_sub, const u8* d_mask_carve,
                          const int* job_angle, const int* job_skip, int njobs, u8* d_out);
int pb3d_transpose_mask_dev(pb3d_ctx* ctx, const u8* d_hw, i64 h, i64 w, u8* d_wh);
// The RGB (C == 3) and label (C == 1) forms of an op behind their entries' argument checks (nvox > 0, no null buffer):
// csrc/carve.hip: part_carve's jobs on a (W,H,D,C) grid -- the fused 90-degree sweep, then the other jobs merged or one by one
int pb3d_part_carve_jobs(pb3d_ctx* ctx, const u8* d_colored, int C, i64 W, i64 H, i64 D, const u8* d_mask_sub, const u8* d_mask_carve,
                         const int* job_angle, const int* job_skip, int njobs, u8* d_out);
// csrc/carve.hip: out[x,y,z,:] = img[y,x,:] where carved[x,y,z] == 1, else 0, for an (H,W,C) image
int pb3d_image_apply_dev(pb3d_ctx* ctx, const u8* d_carved, i64 W, i64 H, i64 D, const u8* d_img_hwc, int C, u8* d_out);
// csrc/global.hip: global_carve as ones -> process_voxel_grid -> image apply, with the transposed (W,H) mask already in d_mask_wh
int pb3d_global_carve_composed(pb3d_ctx* ctx, const u8* d_mask_wh, const u8* d_img_hwc, int C, i64 W, i64 H, i64 D, int angle_interval, u8* d_out);
int pb3d_part_carve90_planes(pb3d_ctx* ctx, const u8* d_colored, int C, i64 W, i64 H, i64 D, const u32* d_A, const u32* d_AT, int njobs, const u32* d_vbits,
                             int nwv, int c0, int c2, u8* d_out, int* took);
int pb3d_launch_gc90_stream(pb3d_ctx* ctx, const u8* d_bin_hw, const u8* d_rgb_hw3, int C, const u32* d_vbits, int nw, int c0, i64 W, i64 H, i64 D, i64 x0,
                            i64 x1, u8* d_out_slab);
int pb3d_launch_global_carve90(pb3d_ctx* ctx, const u8* d_bin_hw, const u8* d_rgb_hw3, int C, i64 h, i64 w, const double M[9],
                               const double off[3], i64 x0, i64 x1, u8* d_out_slab);
