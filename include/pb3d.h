/*
 * pb3d.h -- C ABI of libpb3d.so: MI355X (gfx950) semantic voxel carving & re-projection.
 *
 * The reference (BarnitaSharma/Part-based-3D-Reconstruction) has no FFI: its boundary for
 * this path is the Python function surface of utils/voxel_carving_utils.py,
 * utils/voxel_utils.py, utils/projection_utils.py and utils/camera_estimation.py, called
 * with NumPy arrays.  This header is what a ctypes binding of those functions binds; each
 * entry point cites the reference function (file:line) it replaces.  INTEGRATION.md shows
 * the reference-side stub.
 *
 * Conventions
 *   - plain C, no C++/torch types; every buffer is caller-owned and C-contiguous;
 *   - grids are uint8, axes (W=x, H=y, D=z[,3]) in C order, exactly the reference's layout;
 *   - every function returns 0 on success or a negative PB3D_E* code; pb3d_last_error()
 *     gives the thread-local message of the last failure;
 *   - "*_dev" entry points take DEVICE pointers, enqueue on the context's HIP stream and
 *     return without synchronising (call pb3d_sync); the un-suffixed entry points take
 *     HOST pointers, stage through device scratch and return when the result is in the
 *     caller's buffer (these are what the NumPy shim calls);
 *   - device pointers need the alignment of their element type and no more (any byte for
 *     uint8_t*, 4 for float* / int32_t* / uint32_t*, 8 for double* / int64_t* / uint64_t*),
 *     unless the entry says otherwise: a view into a larger allocation (a slab, a rank's slot)
 *     is as good as the allocation's base; only speed may depend on the address;
 *   - a context belongs to one GPU and one HIP stream; use it from one thread at a time.
 *   - There is NO CPU fallback: every op fails with PB3D_ENODEVICE when no GPU is present.
 */
#ifndef PB3D_H
#define PB3D_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pb3d_ctx pb3d_ctx;
typedef struct pb3d_event pb3d_event;

enum {
    PB3D_OK = 0,
    PB3D_EINVAL = -1,       /* bad argument (shape, null pointer, angle ...)           */
    PB3D_ENODEVICE = -2,    /* no HIP device / HIP runtime error                        */
    PB3D_ENOMEM = -3,       /* device allocation failed                                  */
    PB3D_EUNSUPPORTED = -4, /* argument combination outside what the path needs          */
    PB3D_ECOMM = -5,        /* RCCL not available / collective failed                    */
    PB3D_EINDEX = -6        /* an index read from a device buffer is out of range        */
};

/* ---- lifecycle, device memory, timing (plumbing) ------------------------------------- */
int pb3d_version(void);
const char* pb3d_last_error(void);
int pb3d_device_count(int* n);
int pb3d_create(int device, pb3d_ctx** out);
void pb3d_destroy(pb3d_ctx* ctx);
/* A context belongs to ONE device; its stream, scratch and pools live there.  HIP's current device is a property of the host THREAD:
 * pb3d_create makes `device` current for the calling thread, so "one thread (or one process) per GPU, each with its own context" needs
 * nothing else.  A single thread that alternates between contexts of different devices calls pb3d_make_current(ctx) before each run of
 * calls on that context (it is hipSetDevice(ctx's device); the entry points do not switch devices themselves). */
int pb3d_make_current(pb3d_ctx* ctx);
int pb3d_device_info(pb3d_ctx* ctx, char* name, int name_cap, int* compute_units, int64_t* hbm_bytes);
int pb3d_sync(pb3d_ctx* ctx);
/* Development knobs (results never depend on them; they select between kernels that are all bit-exact, and the parity tests use them to
 * run both forms of a kernel on the same grids).  Every knob has a name -- "sliced", "rot90_wide", "rot90_flat", "rot90_fill",
 * "rot90_mask_block", "global_composed", "per_job", "orient_tile", "ccl_*", "s32_*", "no_table_cache",
 * "uncap", "crop_ablate" (csrc/ctx.hip lists them with their ranges); an unknown name or a value out of range is PB3D_EINVAL.
 * "per_job" = 1: pb3d_part_carve_dev and pb3d_part_carve_label_dev run every job through the job-by-job passes (no fused sweep of the
 * 90-degree jobs, no merged pass of the others), pb3d_global_carve_label_dev its composed pipeline at 90 degrees too.  Initial
 * values come from the environment, read ONCE in pb3d_create: PB3D_KNOBS="name=value,name=value" (any knob), and PB3D_SLICED,
 * PB3D_ROT90_WIDE, PB3D_S32_GPW, PB3D_UNCAP. */
int pb3d_set_tuning(pb3d_ctx* ctx, const char* name, int value);
int pb3d_dev_alloc(pb3d_ctx* ctx, size_t bytes, void** dptr);
int pb3d_dev_free(pb3d_ctx* ctx, void* dptr);
int pb3d_dev_memset(pb3d_ctx* ctx, void* dptr, int value, size_t bytes);
int pb3d_h2d(pb3d_ctx* ctx, void* dptr, const void* hptr, size_t bytes);
int pb3d_d2h(pb3d_ctx* ctx, void* hptr, const void* dptr, size_t bytes);
/* Host -> device without waiting: the bytes are copied into a pinned ring of the context first, so hptr may be reused when the call
 * returns and the transfer is ordered on the context's stream like a kernel (inputs above 4 MiB take the blocking path of pb3d_h2d).
 * What a resident pipeline uploads between its stages are 2-D masks and descriptors of a few hundred KB. */
int pb3d_h2d_async(pb3d_ctx* ctx, void* dptr, const void* hptr, size_t bytes);
/* number of times the host has waited for the context's stream so far (tests bound the waits of a resident pipeline) */
int64_t pb3d_sync_count(pb3d_ctx* ctx);
int pb3d_d2d(pb3d_ctx* ctx, void* dst, const void* src, size_t bytes);
/* HIP events recorded on the context's stream (the stream every kernel is launched on). */
int pb3d_event_create(pb3d_ctx* ctx, pb3d_event** ev);
int pb3d_event_record(pb3d_ctx* ctx, pb3d_event* ev);
int pb3d_event_elapsed_ms(pb3d_ctx* ctx, pb3d_event* start, pb3d_event* stop, float* ms); /* syncs on stop */
void pb3d_event_destroy(pb3d_event* ev);

/* ---- host shim H1: pinned rotation data ------------------------------------------------
 * Rinv(angle) = numpy.linalg.inv of the Y-rotation, reference utils/voxel_carving_utils.py:65-69
 * (bit patterns pinned for angle = 0..90, see csrc/rotinv_table.inc), and
 * offset = c - Rinv@c with c = shape/2 as NumPy evaluates it (:108,:119; FMA chain). */
int pb3d_rotinv(int angle_deg, double M[9]);
int pb3d_offset(const double M[9], const int64_t shape[3], double off[3]);

/* ---- carve_voxel_grid_with_masks, reference utils/voxel_carving_utils.py:76-87 ----------
 * out = grid where mask_wh[x,y] != 0 else 0, broadcast over z (and channel).  C = 1 or 3.
 * mask_wh is the (W,H) uint8 truthiness image, i.e. after _mask_to_wh (:19-28), which is
 * host logic in the shim.  (The reference's RGB-mask branch :90-95 cannot broadcast for
 * any non-degenerate shape and always raises; the shim raises the same ValueError.) */
int pb3d_carve_mask_dev(pb3d_ctx* ctx, const uint8_t* d_grid, int64_t W, int64_t H, int64_t D, int C,
                        const uint8_t* d_mask_wh, uint8_t* d_out);
int pb3d_carve_mask(pb3d_ctx* ctx, const uint8_t* grid, int64_t W, int64_t H, int64_t D, int C,
                    const uint8_t* mask_wh, uint8_t* out);

/* ---- one rotate-about-Y + carve step = scipy.ndimage.affine_transform(order=1,
 * mode="constant", cval=0) followed by the mask carve; call site
 * reference utils/voxel_carving_utils.py:116-124.  M must have row 1 == [+-0, 1, +-0]
 * and off[1] == 0 (true for every Rinv).  d_mask_wh may be NULL (no carve). */
int pb3d_rotate_carve_dev(pb3d_ctx* ctx, const uint8_t* d_occ, int64_t W, int64_t H, int64_t D,
                          const double M[9], const double off[3], const uint8_t* d_mask_wh, uint8_t* d_out);
int pb3d_rotate_carve(pb3d_ctx* ctx, const uint8_t* occ, int64_t W, int64_t H, int64_t D,
                      const double M[9], const double off[3], const uint8_t* mask_wh, uint8_t* out);

/* ---- process_voxel_grid, reference utils/voxel_carving_utils.py:104-126 ------------------
 * for angle in range(0, 91, angle_interval): rotate-carve; cumulative.  The loop runs on
 * the device.  d_tmp: W*H*D bytes of scratch (ping-pong); d_out may not alias d_occ.
 * Chains of two and more rotation steps (angle_interval <= 45) keep the volume BIT-SLICED between the steps (32 planes per dword,
 * 1/4 B/voxel per middle step instead of 2; csrc/sliced.hip): the first kernel slices and checks that the data is 0 / 1; the whole chain
 * is queued behind it and the call then waits on the host for that ONE kernel's verdict (not for the chain): grids with other values
 * take the byte chain, which overwrites what the queued steps left in d_out -- same results.  Everything else about the call is
 * asynchronous on the context's stream, as for the other *_dev entries. */
int pb3d_process_grid_dev(pb3d_ctx* ctx, const uint8_t* d_occ, int64_t W, int64_t H, int64_t D,
                          const uint8_t* d_mask_wh, int angle_interval, uint8_t* d_out, uint8_t* d_tmp);
int pb3d_process_grid(pb3d_ctx* ctx, const uint8_t* occ, int64_t W, int64_t H, int64_t D,
                      const uint8_t* mask_wh, int angle_interval, uint8_t* out);

/* The same loop for grids that are NOT uint8.  The reference never looks at the dtype: scipy.ndimage.affine_transform(order=1) returns the
 * dtype it was given and np.where(mask, grid, 0) keeps it (float16 and anything else SciPy's interpolation refuses: "data type not
 * supported"; a bool grid becomes int64 in upstream's first np.where, so the host side passes it as PB3D_I64).  A plain
 * kernel per step (csrc/rotate_typed.hip: f64 accumulation in SciPy's tap order, SciPy's store rule of the type, the step's carve in the
 * same store); the notebooks only pass uint8, which keeps its own kernels above.  d_grid / d_out / d_tmp: W*H*D elements of the dtype
 * (complex: interleaved parts), none aliased.  64-bit integers go through a double exactly as in SciPy. */
enum {
    PB3D_I8 = 1, PB3D_U8 = 2, PB3D_I16 = 3, PB3D_U16 = 4, PB3D_I32 = 5, PB3D_U32 = 6, PB3D_I64 = 7, PB3D_U64 = 8,
    PB3D_F32 = 9, PB3D_F64 = 10, PB3D_C64 = 11, PB3D_C128 = 12
};
size_t pb3d_dtype_bytes(int dtype);      /* bytes per element, 0 for an unknown code */
int pb3d_process_grid_typed_dev(pb3d_ctx* ctx, const void* d_grid, int dtype, int64_t W, int64_t H, int64_t D, const uint8_t* d_mask_wh,
                                int angle_interval, void* d_out, void* d_tmp);

/* ---- _occupancy, reference utils/voxel_carving_utils.py:32-33: any(grid > 0, axis=-1) ---- */
int pb3d_occupancy_dev(pb3d_ctx* ctx, const uint8_t* d_grid_rgb, int64_t nvox, uint8_t* d_occ);
int pb3d_occupancy(pb3d_ctx* ctx, const uint8_t* grid_rgb, int64_t nvox, uint8_t* occ);

/* ---- apply_colored_mask_to_voxel_grid, reference utils/voxel_carving_utils.py:128-136 ----
 * out[x,y,z,:] = rgb_hw3[y,x,:] where carved[x,y,z] == 1 else 0. */
int pb3d_color_apply_dev(pb3d_ctx* ctx, const uint8_t* d_carved, int64_t W, int64_t H, int64_t D,
                         const uint8_t* d_rgb_hw3, uint8_t* d_out);
int pb3d_color_apply(pb3d_ctx* ctx, const uint8_t* carved, int64_t W, int64_t H, int64_t D,
                     const uint8_t* rgb_hw3, uint8_t* out);

/* ---- global_carve, reference utils/voxel_carving_utils.py:269-298 -------------------------
 * ones((w,h,w)) -> process_voxel_grid -> colour.  bin_hw: (h,w) truthiness uint8,
 * rgb_hw3: (h,w,3).  out: (w,h,w,3).  The x-range [x0,x1) variant computes only that slab
 * of the output (slab pointer = start of the slab, any byte address), for sharded runs; a
 * proper slab needs angle_interval == 90 (PB3D_EINVAL otherwise). */
int pb3d_global_carve_dev(pb3d_ctx* ctx, const uint8_t* d_bin_hw, const uint8_t* d_rgb_hw3, int64_t h, int64_t w,
                          int angle_interval, int64_t x0, int64_t x1, uint8_t* d_out_slab);
int pb3d_global_carve(pb3d_ctx* ctx, const uint8_t* bin_hw, const uint8_t* rgb_hw3, int64_t h, int64_t w,
                      int angle_interval, uint8_t* out);

/* ---- part_carve, reference utils/voxel_carving_utils.py:139-160 ---------------------------
 * Job j is described by two (W,H) uint8 0/1 images (the shim derives them from the
 * semantic mask, :143-151): mask_sub[j] = mask2d.T gates `sub`; mask_carve[j] =
 * _mask_to_wh(mask2d.T) is what process_voxel_grid uses (differs only when W == H).
 * job_skip[j] != 0 marks jobs whose mask2d is empty (:148).  out is zero where no job keeps. */
int pb3d_part_carve_dev(pb3d_ctx* ctx, const uint8_t* d_colored, int64_t W, int64_t H, int64_t D,
                        const uint8_t* d_mask_sub, const uint8_t* d_mask_carve, const int* job_angle,
                        const int* job_skip, int njobs, uint8_t* d_out);
int pb3d_part_carve(pb3d_ctx* ctx, const uint8_t* colored, int64_t W, int64_t H, int64_t D,
                    const uint8_t* mask_sub, const uint8_t* mask_carve, const int* job_angle,
                    const int* job_skip, int njobs, uint8_t* out);

/* ---- grid -> points: get_voxel_points_by_parts (reference utils/voxel_utils.py:7-21) and
 * voxel_grid_to_points (:35-51).  Grid (A0,A1,A2[,C]); a voxel on the stride lattice is
 * selected if its RGB equals one of colors[ncolors][3] (ncolors > 0, C == 3) or if any of
 * its C channels is non-zero (ncolors == 0).  Points come out in numpy.where order as
 * float32 (a2,a1,a0)*stride plus the voxel's C bytes.  count first, then fill with the same
 * arguments and buffers of exactly n rows.  A fill refuses (PB3D_EINVAL) if another call has
 * reused the state its count left on the context. */
int pb3d_points_count_dev(pb3d_ctx* ctx, const uint8_t* d_grid, int64_t A0, int64_t A1, int64_t A2, int C,
                          const uint8_t* colors, int ncolors, int stride, int64_t* n);
int pb3d_points_fill_dev(pb3d_ctx* ctx, const uint8_t* d_grid, int64_t A0, int64_t A1, int64_t A2, int C,
                         const uint8_t* colors, int ncolors, int stride, int64_t n, float* d_pts, uint8_t* d_cols);
/* count + fill in one call (stride 1, a 16-byte aligned grid), for callers whose output buffers exist before the count is known.
 * capacity = rows d_pts (n x 3 float32) / d_cols (n x C) can take; *n is the number of selected voxels.  If *n <= capacity the
 * buffers hold the points when the call returns; otherwise nothing is written and the call must be repeated with capacity >= *n.
 * It keeps its state apart from pb3d_points_count_dev / pb3d_points_fill_dev: it may run between the two.  Synchronises (returns *n). */
int pb3d_points_extract_dev(pb3d_ctx* ctx, const uint8_t* d_grid, int64_t A0, int64_t A1, int64_t A2, int C, const uint8_t* colors, int ncolors,
                            int64_t capacity, float* d_pts, uint8_t* d_cols, int64_t* n);
int pb3d_points_count(pb3d_ctx* ctx, const uint8_t* grid, int64_t A0, int64_t A1, int64_t A2, int C,
                      const uint8_t* colors, int ncolors, int stride, int64_t* n);
int pb3d_points_fill(pb3d_ctx* ctx, int64_t n, float* pts, uint8_t* cols); /* after pb3d_points_count on the same ctx */

/* ---- meshify_colored_voxel_grid, reference utils/voxel_utils.py:53-96 -------------------
 * Binary marching cubes of the lattice grid[::s, ::s, ::s] (occupied = any of its C channels > 0)
 * in skimage's serial order (Lewiner, level 0.5), plus each vertex's nearest occupied
 * lattice point.  count: builds the lattice bitmask, counts, scans, synchronises once and returns
 * nverts / nfaces (an error if either reaches 2^31, or if the lattice is smaller than 2 on an axis).
 * fill: must follow count with identical grid arguments and the counted sizes on the same context, and
 * refuses (PB3D_EINVAL) if another call has reused the state its count left there; writes verts
 * (nverts x 3 float32: (s*a2, s*a1, shape[2] - s*a0)), faces (nfaces x 3 int32, skimage's column
 * order), normals (nverts x 3 float32, skimage's (a0, a1, a2) order) and, if d_cols is not null,
 * the C bytes of each vertex's nearest occupied lattice voxel.  Enqueue only.
 * colors: that nearest-voxel search on its own for verts of this grid (the query is the
 * reference's verts[:, [2,1,0]] / stride; ties go to the smallest lattice index).  Enqueue only. */
int pb3d_mesh_count_dev(pb3d_ctx* ctx, const uint8_t* d_grid, int64_t A0, int64_t A1, int64_t A2, int C, int stride,
                        int64_t* nverts, int64_t* nfaces);
int pb3d_mesh_fill_dev(pb3d_ctx* ctx, const uint8_t* d_grid, int64_t A0, int64_t A1, int64_t A2, int C, int stride,
                       int64_t nverts, int64_t nfaces, float* d_verts, int32_t* d_faces, float* d_normals, uint8_t* d_cols);
int pb3d_mesh_colors_dev(pb3d_ctx* ctx, const uint8_t* d_grid, int64_t A0, int64_t A1, int64_t A2, int C, int stride,
                         const float* d_verts, int64_t nverts, uint8_t* d_cols);
int pb3d_mesh_count(pb3d_ctx* ctx, const uint8_t* grid, int64_t A0, int64_t A1, int64_t A2, int C, int stride,
                    int64_t* nverts, int64_t* nfaces);
int pb3d_mesh_fill(pb3d_ctx* ctx, int64_t nverts, int64_t nfaces, float* verts, int32_t* faces, float* normals,
                   uint8_t* cols); /* after pb3d_mesh_count on the same ctx; cols may be null */

/* ---- get_marching_cubes_mesh, reference utils/eval_helpers.py:191-195: the isosurface of a float32 volume ----------
 * The reference calls skimage's marching_cubes(volume, level) and divides the vertices by grid_size.  This is a rule of the project's
 * own on the binary case table of meshify_colored_voxel_grid (csrc/mc_binary_table.inc), stated to the bit; on a 0/1 volume at level
 * 0.5 it gives meshify's lattice mesh (skimage's) byte for byte.
 *   Input     a C-contiguous float32 volume (n0, n1, n2), every n >= 2 and < 2^24, all values finite (the caller's business: a NaN
 *             counts as outside, and a non-finite end of a crossed edge gives a non-finite vertex); level, a finite float64; divisor, a finite float32 > 0
 *             (1 = lattice units).
 *   Inside    a lattice point is inside iff (double)v > level.  A value equal to the level is outside.  The level is never
 *             rounded to float32: float32(0.1) > 0.1, so a voxel holding float32(0.1) is inside at level 0.1.
 *   Cases, ownership, order   meshify's at stride 1: case bit a0*4 + a1*2 + a2 = corner (c0+a0, c1+a1, c2+a2) inside; a cube's
 *             triangles are the table's for that case, in table order; an edge vertex belongs to the lowest-scan-order cube that
 *             holds the edge, the centre vertex (id 12) to its cube; a cube creates the vertices it owns in the order its triangle
 *             list first names them; vertices and faces follow cube scan order (a2 fastest).  The triangles depend on the 8 signs
 *             alone, and the table resolves ambiguous faces the same way from both sides: the mesh is closed and consistently
 *             oriented wherever the volume's border is outside.
 *   Edge vertex   between lattice points a (the lower index on the edge's axis, value va) and b (value vb):
 *             t = (level - (double)va) / ((double)vb - (double)va), three float64 operations, each rounded once, no FMA;
 *             0 <= t <= 1.  Its coordinate on the edge's axis is (float)((double)ia + t): one float64 addition, one rounding to
 *             float32.  The other two coordinates are the float32 lattice indices.
 *   Centre vertex   c + 0.5 on every axis, whatever the values.
 *   Output    every coordinate is then divided by the divisor in float32, one correctly rounded division (x / 1.0f is x).
 *             verts: nverts x 3 float32 in (a0, a1, a2) order; faces: nfaces x 3 int32.  No normals, no values.
 *   Allowed   a vertex exactly on a lattice point (t = 0 where va == level), several vertices at one position, zero-area faces
 *             (kept, so the mesh stays closed).  A level outside the data range, or a volume all inside, gives 0 vertices and faces.
 *   Not claimed   equality with skimage on float input: its Lewiner variant decides ambiguous faces and interiors from the values and
 *             places the extra vertex elsewhere, so vertex and face counts can differ on ambiguous cubes.
 * count: the inside bitmask (the one full read of the volume), meshify's count and scans, one host wait; returns nverts / nfaces (an
 * error if either reaches 2^31).  fill: must follow count with identical arguments (the level and the divisor bit for bit) and the
 * counted sizes on the same context; enqueue only.  The pair keeps its state in the scratch slots of pb3d_mesh_count_dev /
 * pb3d_mesh_fill_dev: a count of either ends the other's pending pair, whose fill then refuses (PB3D_EINVAL).  The host forms stage
 * the volume; pb3d_iso_fill waits.  Arguments are checked before the context is looked at.
 * Knob "iso_timing" (pb3d_set_tuning; the fill then waits once) times the passes with events: pb3d_iso_last gives the milliseconds
 * of {bits pass, count and scans, vertex pass, faces} of the last count and fill. */
int pb3d_iso_count_resident(pb3d_ctx* ctx, const float* d_vol, int64_t n0, int64_t n1, int64_t n2, double level, float divisor,
                       int64_t* nverts, int64_t* nfaces);
int pb3d_iso_fill_resident(pb3d_ctx* ctx, const float* d_vol, int64_t n0, int64_t n1, int64_t n2, double level, float divisor,
                      int64_t nverts, int64_t nfaces, float* d_verts, int32_t* d_faces);
int pb3d_iso_count(pb3d_ctx* ctx, const float* vol, int64_t n0, int64_t n1, int64_t n2, double level, float divisor,
                   int64_t* nverts, int64_t* nfaces);
int pb3d_iso_fill(pb3d_ctx* ctx, int64_t nverts, int64_t nfaces, float* verts, int32_t* faces); /* after pb3d_iso_count on the same ctx */
int pb3d_iso_last(pb3d_ctx* ctx, double pass_ms[4]);

/* ---- project_colored_voxels, reference utils/projection_utils.py:5-23 ---------------------
 * R = look_at_rotation(cam, target) (host, reference utils/camera_geometry.py:3-14) is
 * passed in.  pts: (n,3) float32 (pts_f64 = 0) or float64 (1); cols (n,3) uint8.
 * prec[4] = arithmetic width (0 = float32, 1 = float64) of {matmul+divide, *f, +cx, +cy}
 * as NumPy-2 promotion decides it from the caller's types.  img (Himg,Wimg,3) is fully
 * written; among points landing on one pixel the last in input order wins. */
int pb3d_project_dev(pb3d_ctx* ctx, const void* d_pts, int pts_f64, const uint8_t* d_cols, int64_t n,
                     const double R[9], const double cam[3], double f, double cx, double cy, const int prec[4],
                     int Himg, int Wimg, uint8_t* d_img);
int pb3d_project(pb3d_ctx* ctx, const void* pts, int pts_f64, const uint8_t* cols, int64_t n,
                 const double R[9], const double cam[3], double f, double cx, double cy, const int prec[4],
                 int Himg, int Wimg, uint8_t* img);

/* ---- z-buffer visibility (row N5), reference utils/eval_helpers_intra.py:134-190 -------------------------
 * Same pinhole arithmetic as pb3d_project, but points with Z <= 1e-6 are dropped (no clamp).
 * depth_buffer: zbuf[v,u] = min Z of the points landing on the pixel as float32, +inf where none (:134-163).
 * visible_mask: mask[v,u] = 1 where some point has |Z - zbuf[v,u]| < eps (:168-190); eps_f32 != 0 when the
 * comparison is made in float32 (float32 camera and a Python-float eps). */
int pb3d_depth_buffer_dev(pb3d_ctx* ctx, const void* d_pts, int pts_f64, int64_t n, const double R[9], const double cam[3], double f,
                          double cx, double cy, const int prec[4], int Himg, int Wimg, float* d_zbuf);
int pb3d_visible_mask_dev(pb3d_ctx* ctx, const void* d_pts, int pts_f64, int64_t n, const double R[9], const double cam[3], double f,
                          double cx, double cy, const int prec[4], const float* d_zbuf, int Himg, int Wimg, double eps, int eps_f32,
                          uint8_t* d_mask);

/* ---- notebook 4 on the device (row N6), reference utils/eval_helpers_intra.py:287-748 ------------------------------------
 * The z-buffer and visibility passes of run_minaret_iou_evaluation / run_part_minaret_binary_iou without point lists: the
 * (A0,A1,A2,C) uint8 grid (C = 3: RGB, C = 1: labels) is read directly, voxel (a0,a1,a2) being the point (x = a2, y = a1,
 * z = a0) of the reference's np.where (:139-140, :710-717); a voxel is occupied where any channel is non-zero.  The camera
 * arguments and eps / eps_f32 are those of pb3d_depth_buffer_dev / pb3d_visible_mask_dev, with the grid's points float32.
 * Colour tables hold ncolors <= 31 entries of C bytes, none of them 0 (black / label 0 is the empty voxel); a zbuf of
 * another shape than the image, a bad C or too many colours are refused before any device work, and a null context after them.
 * grid_depth_buffer: bit for bit pb3d_depth_buffer_dev on the grid's points (compute_global_depth_buffer, :134-163).
 * grid_visible_bits: bits[v,u] bit k = some voxel of colour k is visible (|Z - zbuf| < eps, :168-190), bit 31 = some occupied
 *   voxel is; d_zbuf may come from another grid (:669-684 tests the init grid's minarets against the deformed grid's z-buffer).
 *   Bit k equals pb3d_visible_mask_dev on get_voxel_points_by_parts(grid, colour k), bit 31 on every occupied voxel (:710-728).
 * points_visible_bits: bit k = some point of list k (counts[k] rows of 3; pts_type 0 float32, 1 float64, 2 int64) is visible
 *   (:509-526: the int64 np.argwhere sets of extract_minaret_voxels_by_label; prec[0] = 1 for them, as NumPy promotes).
 * color_presence: d_bitmap (PB3D_PRESENCE_BYTES, bit r | g << 8 | b << 16, or the label) = the non-zero values of nvox voxels
 *   (compute_binary_gt's np.unique, :274-280); d_present[0] bit k = colour k of the table is among them (may be null when
 *   ncolors == 0).
 * mask_bits: bits[px] bit k = RGB mask pixel px has colour k (np.any(mask_parts_from_image(...) > 0), :650-653), bit 31 = its
 *   colour is in d_bitmap (compute_binary_gt, :281-284; d_bitmap may be null: no bit 31).
 * iou_rows: per row r, pred = pred[px] & pred_bits, gt = gt[px] & gt_bits and (no gate, or gate[px] & gate_bits);
 *   d_counts[2r] = #(pred & gt), d_counts[2r+1] = #(pred | gt) (_iou_bool, :269-272; the gate is :525's gt_m & pr_all).
 *   A null image is all zero.  nrows <= 32. */
#define PB3D_PRESENCE_BYTES ((size_t)1 << 21)
typedef struct pb3d_iou_row {
    const uint32_t* pred;
    const uint32_t* gt;
    const uint32_t* gate;
    uint32_t pred_bits, gt_bits, gate_bits;
} pb3d_iou_row;
int pb3d_grid_depth_buffer_dev(pb3d_ctx* ctx, const uint8_t* d_grid, int64_t A0, int64_t A1, int64_t A2, int C, const double R[9],
                               const double cam[3], double f, double cx, double cy, const int prec[4], int Himg, int Wimg, float* d_zbuf);
int pb3d_grid_visible_bits_dev(pb3d_ctx* ctx, const uint8_t* d_grid, int64_t A0, int64_t A1, int64_t A2, int C, const uint8_t* colors,
                               int ncolors, const double R[9], const double cam[3], double f, double cx, double cy, const int prec[4],
                               const float* d_zbuf, int zH, int zW, int Himg, int Wimg, double eps, int eps_f32, uint32_t* d_bits);
int pb3d_points_visible_bits_dev(pb3d_ctx* ctx, const void* const* d_lists, const int64_t* counts, int nlists, int pts_type, const double R[9],
                                 const double cam[3], double f, double cx, double cy, const int prec[4], const float* d_zbuf, int zH, int zW,
                                 int Himg, int Wimg, double eps, int eps_f32, uint32_t* d_bits);
int pb3d_color_presence_dev(pb3d_ctx* ctx, const uint8_t* d_grid, int64_t nvox, int C, uint32_t* d_bitmap, const uint8_t* colors, int ncolors,
                            int64_t* d_present);
int pb3d_mask_bits_dev(pb3d_ctx* ctx, const uint8_t* d_mask, int64_t npix, const uint8_t* colors, int ncolors, const uint32_t* d_bitmap,
                       uint32_t* d_bits);
int pb3d_iou_rows_dev(pb3d_ctx* ctx, const pb3d_iou_row* rows, int nrows, int64_t npix, int64_t* d_counts);

/* ---- inter-method point-cloud metrics (row I5), reference utils/eval_helpers.py ----------------------------------------------------
 * Point lists are (n, 3) rows of float32 (*_f64 = 0) or float64 (*_f64 = 1); everything is computed in float64 (float32 is widened, as
 * cKDTree and NearestNeighbors widen it).  Counts are limited to 2^31 - 1 points per list.
 * points_bounds: d_out[0..3) = min, d_out[3..6) = max over the n >= 1 points, exact (all_pts.min(0) / .max(0), :84-85).
 * nn_dist: d_out[i] = the k-th smallest (k = 1 or 2, with multiplicity) of sqrt((dx*dx + dy*dy) + dz*dz) from query i to the nr
 *   reference points, bit for bit what cKDTree(r).query(q, k)[0][:, k - 1] and NearestNeighbors(k).fit(r).kneighbors(q) return
 *   (chamfer_distance :38-42, fscore_with_threshold :53-59, compute_nn_stats :120-123 with k = 2 on the set itself, so a point's own
 *   copy counts at 0, compute_nn_distances :223-227).  nr >= k when nq > 0.  Builds a uniform cell index of the reference set in
 *   scratch and waits once for the set's bounding box; the query itself is enqueued.
 * nn_grid_shape: the cells per axis of the index nn_dist builds for nr reference points in this box (no device work).
 * voxel_iou_counts: the occupancy, dilation and counts of voxel_iou (:83-111).  The host computes bounds_min, step (float32 values
 *   when calc_f32: both lists float32, NumPy's float32 arithmetic) and iters with the reference's expressions; the device sets voxel
 *   clip(int((p - bounds_min) / step), 0, resolution - 1) of every point (a NaN or out-of-range quotient gives voxel 0, as NumPy's
 *   cast does on x86), dilates both grids iters times with the 6-neighbour cross and a zero border (binary_dilation) and writes
 *   d_counts[0] = #(A & B), d_counts[1] = #(A | B).  1 <= resolution <= 2048, iters >= 0 (0: no dilation).
 * knn: for each of the nq queries its k nearest reference points (1 <= k <= PB3D_KNN_MAX_K, nr >= k when nq > 0), what
 *   NearestNeighbors(n_neighbors=k).fit(r).kneighbors(q) computes (compute_surface_metrics :217-218).  d_idx: nq x k int32, positions
 *   in d_r; d_dist: nq x k float64 or NULL, the distance expression of nn_dist.  A row is ascending by (squared distance as computed,
 *   then reference index), and the same rule decides which of several equidistant points are in the row, so the result is a function
 *   of the input alone (the trees break ties by traversal order: on tied input only their distances are comparable).  With q the
 *   same list as r a point is its own neighbour at distance 0; exact duplicates tie at 0 and are ordered by index.  Input must be
 *   finite.  Same cell index and one host wait as nn_dist; nn_dist itself (k = 1, 2, distances only) is a separate, lighter path. */
int pb3d_points_bounds_dev(pb3d_ctx* ctx, const void* d_pts, int pts_f64, int64_t n, double* d_out);
int pb3d_nn_dist_dev(pb3d_ctx* ctx, const void* d_q, int q_f64, int64_t nq, const void* d_r, int r_f64, int64_t nr, int k, double* d_out);
#define PB3D_KNN_MAX_K 32
int pb3d_knn_dev(pb3d_ctx* ctx, const void* d_q, int q_f64, int64_t nq, const void* d_r, int r_f64, int64_t nr, int k, double* d_dist,
                 int32_t* d_idx);
int pb3d_nn_grid_shape(const double bounds[6], int64_t nr, int64_t cells[3]);
int pb3d_voxel_iou_counts_dev(pb3d_ctx* ctx, const void* d_a, int a_f64, int64_t na, const void* d_b, int b_f64, int64_t nb,
                              const double bounds_min[3], double step, int calc_f32, int resolution, int iters, int64_t* d_counts);

/* ---- mesh regularity (the surface block of the inter-method evaluation), reference utils/eval_helpers.py:198-245 --------------------
 * Vertices are (nv, 3) rows of float32 (verts_f64 = 0) or float64 (1); faces are (nf, 3) rows of int32 (faces_i64 = 0) or int64 (1).
 * Every entry first checks the face indices on the device: one outside [-nv, nv) is PB3D_EINDEX (NumPy's IndexError) before any
 * kernel gathers through them (one host wait); indices in [-nv, -1] wrap as NumPy's do.
 * triangle_normals (:198-203): d_out nf x 3 in the vertex dtype, bit for bit cross(v1 - v0, v2 - v0) / (norm + 1e-8) as NumPy
 *   evaluates it: every component one product minus one product, each rounded; norm = sqrt((x*x + y*y) + z*z); 1e-8 rounded to the
 *   vertex dtype.
 * vertex_normals (:206-212): d_out nv x 3 in the vertex dtype, bit for bit the reference's double loop: each vertex adds the
 *   normals of its incident faces in ascending face order, starting from 0, in the vertex dtype (a face that names the vertex twice
 *   adds twice), then / (norm + 1e-8); a vertex in no face gives 0.  No floating-point atomics: incidence lists are counted,
 *   scanned, filled and sorted, and one lane adds a vertex's list.  Any vertex degree works; a fan of thousands of faces is slow.
 * surface_metrics (:214-245, the loop body): from the vertices, their normals (vertex dtype) and the nv x k neighbour rows of
 *   pb3d_knn_dev(verts, verts, k) -- 2 <= k <= PB3D_KNN_MAX_K -- three float64 arrays of length nv, all arithmetic in float64 and
 *   compensated where it cancels:  normal_std = np.std of degrees(arccos(clip(n_j . n_i, -1, 1))) over the row;  roughness = the
 *   smallest eigenvalue of the neighbours' covariance (divisor k - 1; PCA(3).explained_variance_[2]), >= 0;  curvature =
 *   |mean(neighbours) - vertex|.  An index outside [0, nv) in d_idx is PB3D_EINDEX.  The reference's np.mean of each is the caller's. */
int pb3d_triangle_normals_dev(pb3d_ctx* ctx, const void* d_verts, int verts_f64, int64_t nv, const void* d_faces, int faces_i64, int64_t nf,
                              void* d_out);
int pb3d_vertex_normals_dev(pb3d_ctx* ctx, const void* d_verts, int verts_f64, int64_t nv, const void* d_faces, int faces_i64, int64_t nf,
                            void* d_out);
int pb3d_surface_metrics_dev(pb3d_ctx* ctx, const void* d_verts, const void* d_normals, int verts_f64, int64_t nv, const int32_t* d_idx, int k,
                             double* d_normal_std, double* d_roughness, double* d_curvature);

/* ---- a triangle mesh as a comparison target: exact point-to-mesh distances and area-weighted surface samples (step 7 of the reference's
 * results/4.Inter-method_3D/README.md, "load and align a CAD reference model": its geometry; there is no upstream text, so the arithmetic
 * below is the specification) -------------------------------------------------------------------------------------------------------
 * Vertices and faces as for the mesh regularity entries: (nv, 3) rows of float32 (verts_f64 = 0) or float64 (1), (nf, 3) rows of int32
 * (faces_i64 = 0) or int64 (1), at most 2^31 - 1 of each, any 4- / 8-byte aligned base.  Both entries first check the face indices on
 * the device: one outside [-nv, nv) is PB3D_EINDEX before any kernel gathers through them (one host wait); indices in [-nv, -1] wrap.
 * All arithmetic is float64 (float32 vertices and queries are widened first, which is exact), every product, sum, difference, quotient
 * and square root ONE correctly rounded operation, no FMA.  dot(x, y) = (x0*y0 + x1*y1) + x2*y2; a cross component is one product
 * minus one product: cross(x, y) = (x1*y2 - x2*y1, x2*y0 - x0*y2, x0*y1 - x1*y0).  div0(x, y) = 0 if y == 0, else x / y.
 *
 * mesh_dist: for each of the nq queries (d_q: (nq, 3) rows, float32 or float64 by q_f64) the nearest point of the mesh surface.
 *   d2(q, face (a, b, c)) and the face's closest point cp:
 *     ab = b - a, ac = c - a, n = cross(ab, ac).
 *     If dot(n, n) == 0 the face is DEGENERATE: cp is the best of the segments a->b, b->c, c->a in that order, a later one only if its
 *       squared distance is strictly smaller.  Segment s0->s1: e = s1 - s0, dd = dot(e, e), t = dot(q - s0, e),
 *       t = dd == 0 ? 0 : min(max(t / dd, 0), 1), cp = s0 + e*t (per component one product, one sum).
 *     Otherwise the region walk of Ericson, Real-Time Collision Detection 5.1.5, in its order; the first test that holds decides:
 *       1. ap = q - a, d1 = dot(ab, ap), d2 = dot(ac, ap);  d1 <= 0 && d2 <= 0                    -> cp = a
 *       2. bp = q - b, d3 = dot(ab, bp), d4 = dot(ac, bp);  d3 >= 0 && d4 <= d3                   -> cp = b
 *       3. vc = d1*d4 - d3*d2;  vc <= 0 && d1 >= 0 && d3 <= 0                                      -> cp = a + ab*div0(d1, d1 - d3)
 *       4. cq = q - c, d5 = dot(ab, cq), d6 = dot(ac, cq);  d6 >= 0 && d5 <= d6                   -> cp = c
 *       5. vb = d5*d2 - d1*d6;  vb <= 0 && d2 >= 0 && d6 <= 0                                      -> cp = a + ac*div0(d2, d2 - d6)
 *       6. va = d3*d6 - d5*d4, u1 = d4 - d3, u2 = d5 - d6;  va <= 0 && u1 >= 0 && u2 >= 0           -> cp = b + (c - b)*div0(u1, u1 + u2)
 *       7. else den = div0(1, (va + vb) + vc)                                                      -> cp = (a + ab*(vb*den)) + ac*(vc*den)
 *     d = q - cp, d2 = (dx*dx + dy*dy) + dz*dz.
 *   The result for q is the face with the smallest (d2 as computed, face index) -- ties go to the lowest index, so the result is a
 *   function of the input alone, as knn's is:  d_dist[i] = sqrt(d2) (nq float64), d_face[i] = that face (nq int32, or NULL),
 *   d_closest[i] = its cp (nq x 3 float64, or NULL).  nq = 0 does nothing; nf = 0 (or nv = 0) with nq > 0 is PB3D_EINVAL.  Queries and
 *   vertices must be finite, and small enough that no product above overflows; vertices that are not finite are refused (PB3D_EINVAL).
 *   Accuracy: d2 is the squared distance to a point OF the face (up to the rounding of cp), so it never undershoots the true distance by
 *   more than a few ulps of the coordinates; on a sliver it can overshoot, because Ericson's barycentric quotients lose accuracy with the
 *   aspect (smallest height over longest edge): at most 4 ulps of the coordinate magnitude for aspect >= 1e-3, growing below.  Measured
 *   overshoot of the distance over the same algorithm in 80-bit long double, coordinates up to 1e3, aspect in [column, 10 x column):
 *       aspect        1e-1     1e-2     1e-3     1e-4     1e-5     1e-6     1e-7     1e-8
 *       ulps of 1e3   1.25     1.07     0.98     7.5      5.7e4    9.3e8    1.4e12   2.2e14
 *       relative      3.5e-10  2.4e-10  3.1e-10  9.5e-11  3.9e-7   5.4e-3   9.8      4.3e2
 *   Index: the cell grid of nn_dist over the exact box of ALL vertices, sized from nf; a face is listed in every cell of the box
 *   cell(min corner) .. cell(max corner) per axis.  While the (cell, face) entries exceed 8 * nf and the grid has more than one cell,
 *   the cells per axis are halved.  Host waits: the index check, the box, and 1 + (number of halvings) for the entry counts; the query
 *   itself is enqueued.  Scratch: 72 bytes per face, 4 bytes per entry, 12 bytes per cell.
 * mesh_grid_shape: the cells per axis, the entry count and (if not NULL) the number of halvings of the index the last mesh_dist call on
 *   this context built (no device work; PB3D_EINVAL before the first such call).
 * mesh_sample: n points of the surface, stratified by area, a function of (mesh, n, seed) alone.  d_pts: n x 3 float64; d_face: the
 *   int32 face of each sample, or NULL.
 *     area    A_f = 0.5 * sqrt(dot(n, n)), n as above.
 *     prefix  in blocks of 1024 faces: local[f] = the left-to-right running sum inside f's block, starting from the block's first area;
 *             O_b = the left-to-right running sum of the totals (last local) of the blocks before b, O_0 = 0;  cum[f] = O_b + local[f];
 *             total = cum[nf - 1].  cum is non-decreasing by construction.
 *     random  mix(x): x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) * 0x94D049BB133111EB;
 *             x ^ x >> 31, in uint64 wrap-around arithmetic;  r_j(i) = (double)(mix(mix(seed) + 3*i + j) >> 11) * 2^-53, in [0, 1).
 *     face    u = ((double)i + r_0) / (double)n * total;  f = the smallest face with cum[f] > u (np.searchsorted(cum, u, 'right')),
 *             clamped to nf - 1.  A zero-area face has cum[f] == cum[f - 1] and is never that smallest face; the clamp is reached only
 *             if u rounds up to total itself.
 *     point   s = sqrt(r_1), wa = 1 - s, wb = s*(1 - r_2), wc = s*r_2;  each coordinate (a*wa + b*wb) + c*wc.
 *   Sample i lies in stratum [i, i + 1) / n of the cumulative area, so the samples of a face differ from n * A_f / total by less than 2.
 *   n = 0 does nothing.  nf = 0 with n > 0, or a total that is 0 or not finite, is PB3D_EINVAL.  Host waits: the index check and the
 *   total.  Scratch: 8 bytes per face. */
int pb3d_mesh_dist_resident(pb3d_ctx* ctx, const void* d_q, int q_f64, int64_t nq, const void* d_verts, int verts_f64, int64_t nv,
                            const void* d_faces, int faces_i64, int64_t nf, double* d_dist /* nq */, int32_t* d_face /* nq or NULL */,
                            double* d_closest /* nq x 3 or NULL */);
int pb3d_mesh_grid_shape(const pb3d_ctx* ctx, int64_t cells[3], int64_t* entries, int64_t* coarsenings /* or NULL */);
int pb3d_mesh_sample_resident(pb3d_ctx* ctx, const void* d_verts, int verts_f64, int64_t nv, const void* d_faces, int faces_i64, int64_t nf,
                              int64_t n, uint64_t seed, double* d_pts /* n x 3 */, int32_t* d_face /* n or NULL */);

/* ---- mesh smoothing: the vertex-to-vertex adjacency of a triangle mesh, and Laplacian / Taubin smoothing on it (csrc/smooth.hip) --------
 * The step between marching cubes and everything that measures or samples the mesh (trimesh.smoothing.filter_taubin, Open3D's
 * filter_smooth_taubin; uniform weights).  There is no upstream text, so the rules below are the specification, and the result is a
 * function of the input alone, to the bit.
 *   INPUT      verts: (nv, 3) rows of float32 (verts_f64 = 0) or float64 (1); faces: (nf, 3) rows of int32 (faces_i64 = 0) or int64 (1)
 *              with entries in [-nv, nv); entries in [-nv, -1] wrap as NumPy's do.  Anything else is PB3D_EINDEX, checked on the device
 *              before any kernel gathers through them (one host wait).  Limits: nv <= 2^31 - 1 and 6 * nf <= 2^31 - 1.
 *   PAIRS      face (a, b, c), after wrapping, emits six directed pairs: (a,b) (b,a) (b,c) (c,b) (c,a) (a,c).  Pairs with equal ends are
 *              dropped.  This rule alone defines what degenerate faces contribute.
 *   ADJACENCY  N(i) = the set of j with a pair (i, j), ascending.  starts: nv + 1 int64, N(i) = neighbours[starts[i] .. starts[i + 1]);
 *              neighbours: int32, total = starts[nv] entries.  The multiplicity of (i, j) is the number of emitted pairs (i, j) (2 for an
 *              edge between two faces that wind alike or not, 1 for an edge of one face, 4 for an edge of a face given twice); mult[r]
 *              belongs to neighbours[r].  A vertex is a BOUNDARY vertex if it is an end of a pair with multiplicity 1.
 *   STEP(f)    all arithmetic float64, each line one rounded IEEE operation, no FMA.  A vertex that is fixed, or has no neighbour,
 *              keeps its coordinates.  Every other vertex i, per axis:
 *                  s = 0.0, then s = s + x_j for j in N(i) ascending
 *                  m = s / deg          (one correctly rounded division, deg converted exactly)
 *                  d = m - x_i
 *                  x_i' = x_i + f * d   (a product, then a sum)
 *              All vertices read the positions from before the step.
 *   ITERATIONS positions are widened once to float64; `iterations` rounds follow: one STEP(lambda) when mu is NaN (Laplacian), otherwise
 *              STEP(lambda) then STEP(mu) (Taubin; mu < -lambda < 0 keeps the volume); one rounding to the input dtype at the end.
 *              iterations = 0 returns the input bytes.  Fixed vertices are the caller's mask (d_fixed: nv uint8, non-zero = fixed, or
 *              NULL), ORed with the boundary vertices when fix_boundary is set.  Non-finite coordinates are not special: they spread as
 *              IEEE arithmetic spreads them.
 * mesh_adjacency: d_starts nv + 1 int64; d_neighbours room for 6 * nf int32, the first *total written; d_mult (or NULL) likewise, uint32;
 *   d_boundary (or NULL) nv bytes, 1 = boundary vertex.  nf = 0: starts all 0, total 0, no boundary.  Host waits: the index check and total.
 * mesh_smooth: d_out nv x 3 in the input dtype; it may not alias d_verts.  nf = 0 (or iterations = 0) copies the input; nv = 0 does
 *   nothing.  PB3D_EINVAL: iterations < 0, lambda not finite, mu infinite.  Host waits: the index check; everything else is enqueued.
 * Neither keeps anything per vertex while it builds the lists: the 6 * nf pairs go through two stable radix sorts (by the second end,
 * then by the first), a scan of the "new pair" flags compacts them, and run lengths are the multiplicities -- a vertex that is in every
 * face is handled like any other.  A step is one lane per vertex; vertices of degree above 32 are summed by one wavefront each, in the
 * same order.  No floating-point atomics.  Scratch: 220 bytes per face (pairs 96, flags 24, ranks 48, scan 27, neighbours 24) and,
 * for a smoothing, 57 bytes per vertex (starts 8, boundary 1, the two position buffers 48). */
int pb3d_mesh_adjacency_resident(pb3d_ctx* ctx, const void* d_faces, int faces_i64, int64_t nv, int64_t nf, int64_t* d_starts /* nv + 1 */,
                                 int32_t* d_neighbours /* 6 * nf entries, the first *total written */, uint32_t* d_mult /* 6 * nf, or NULL */,
                                 uint8_t* d_boundary /* nv, or NULL */, int64_t* total);
int pb3d_mesh_smooth_resident(pb3d_ctx* ctx, const void* d_verts, int verts_f64, int64_t nv, const void* d_faces, int faces_i64, int64_t nf,
                              int iterations, double lambda, double mu /* NaN: Laplacian */, const uint8_t* d_fixed /* or NULL */,
                              int fix_boundary, void* d_out /* nv x 3 in the input dtype; may not alias d_verts */);

/* ---- mesh simplification by vertex clustering, and the compaction of a mesh (csrc/simplify.hip) ------------------------------------------
 * The one mesh -> mesh step that changes the faces (Rossignac & Borrel 1993; Open3D's simplify_vertex_clustering): the vertices of a
 * voxel become one vertex, and the faces are mapped, thinned and renumbered.  There is no upstream text, so the rules below are the
 * specification, and the result is a function of the input and its order alone, to the bit: two runs give the same bytes.
 *   INPUT      verts: (nv, 3) rows of float32 (verts_f64 = 0) or float64 (1); faces: (nf, 3) rows of int32 (faces_i64 = 0) or int64 (1)
 *              with entries in [-nv, nv); entries in [-nv, -1] wrap as NumPy's do.  Anything else is PB3D_EINDEX, checked on the device
 *              before any kernel gathers through them (one host wait), with nothing written.  Limits: 0 <= nv, nf <= 2^31 - 1.
 *              voxel_size, origin (or NULL) and reduce are voxel_downsample's; duplicate_faces is one of the two below.
 *   CLUSTERS   ORIGIN, CELL, RANGE, VOXELS, INDEX, CENTROID and FIRST of the voxel_downsample section, applied to the whole vertex list:
 *              vertices that no face names are included.  c[0 .. m) are those voxels in their numbering by first appearance, inv[i] the
 *              cluster of vertex i, first[k] the first vertex of cluster k.  A RANGE failure is that section's PB3D_EINVAL.
 *   MAP        face j becomes g_j = (inv[w0], inv[w1], inv[w2]) of its wrapped corners, in the caller's corner order.
 *   COLLAPSED  face j is dropped iff two of its three clusters are equal.
 *   REPEATED   (duplicate_faces = PB3D_FACES_DROP) g_j is rotated cyclically so that its smallest cluster comes first; the three are
 *              distinct, so the rotation is unique.  Two surviving faces are repeats iff their rotated triples are equal: the same three
 *              clusters in the opposite orientation are NOT a repeat.  Of each set of repeats the face with the smallest j stays.
 *              With PB3D_FACES_KEEP this step is skipped.
 *   ORDER      the faces that stay keep the caller's order; face_index[t] = the input position of output face t, strictly increasing.
 *   VERTICES   a cluster stays iff a face that stays names it.  The clusters that stay keep their relative order (first appearance) and
 *              are renumbered 0 .. m' - 1.  out_verts[k'] = the CENTROID or FIRST row of that cluster, taken over all its vertices,
 *              named by a face or not, in the input dtype (float32 rounded once, as voxel_downsample does); index[k'] = first[k];
 *              inverse[i] = the new number of vertex i's cluster, -1 when that cluster was dropped.
 *   FACES OUT  the new numbers in the caller's corner order (not the rotated order), in the caller's index dtype.
 *   ATTRIBUTES with d_colors ((nv, channels) uint8, channels 1 or 3): out_colors[k'] = colors[index[k']] byte for byte -- the colour or
 *              label of a cluster is that of its first vertex; nothing is blended.
 *   EMPTY      nf = 0, or every face collapsed: counts = (0, 0), inverse all -1; not an error.  nf = 0 skips CLUSTERS altogether (no
 *              RANGE failure, no host wait).  nv = 0 with nf > 0 is PB3D_EINDEX.
 * CLOSEDNESS.  With PB3D_FACES_KEEP: if every directed edge (a, b) of the input occurs as often as (b, a) -- a closed, consistently
 * oriented mesh, as meshify and the isosurface produce away from the volume border -- then the same holds for the output (MAP sends
 * a balanced multiset of directed edges to a balanced one, and a collapsed face removes either an edge and its reverse, or nothing
 * but loops).  So the crossing parity that pb3d_voxelize_mesh_resident relies on survives.  With PB3D_FACES_DROP the property can be
 * lost wherever a thin part folds onto itself: of two sheets that land on the same triple in the same orientation one is removed and
 * its neighbours keep an edge without a partner.
 * mesh_compact is MAP .. ATTRIBUTES with every vertex its own cluster (inv[i] = i, m = nv) and no arithmetic: vertices are copied byte
 *   for byte.  It removes faces with a repeated corner, repeated faces (the same option) and the vertices no remaining face names.
 * Neither is quadric-error simplification, neither moves a representative to a quadric optimum, and neither welds vertices by
 * coordinate equality (two vertices are merged only by sharing a voxel).  Beyond the cluster membership that the voxel_downsample
 * section documents, no equality with Open3D is claimed.
 * Outputs: d_out_verts room for nv rows and d_out_faces room for nf rows, of which the first counts[0] and counts[1] are written;
 *   d_out_colors (given iff d_colors is) nv x channels; d_index (nv int32, or NULL), d_face_index (nf int32, or NULL) likewise;
 *   d_inverse (nv int32, or NULL) whole.  No output may alias an input.  Host waits: the index check, the two of the cluster pass
 *   (mesh_simplify only) and one read-back of the two counts; everything else is enqueued.
 * The face half keeps no state per cluster or per triple: the rotated triples go through three stable radix sorts of (key, position)
 * pairs, last cluster first, and a face is a repeat iff it equals its predecessor in that order.  Scratch: 46 bytes per face with
 * PB3D_FACES_DROP (clusters 12, pairs 16, flags 4, ranks 8, scan 4, run table 2), 28 with PB3D_FACES_KEEP; 12 bytes per cluster and,
 * for mesh_simplify, 8 + one row per vertex on top of voxel_downsample's own.
 * simplify_last: of the last of the two on this context, counts = (clusters m, vertices out, faces out) and, with pass_ms not NULL, the
 *   milliseconds its passes took (clusters, map, sorts + repeats, scans, gathers) -- recorded only under the development knob
 *   "simplify_timing" (pb3d_set_tuning; one more host wait), else PB3D_EINVAL.  No result depends on the knob. */
#define PB3D_FACES_DROP 0
#define PB3D_FACES_KEEP 1
int pb3d_mesh_simplify_resident(pb3d_ctx* ctx, const void* d_verts, int verts_f64, int64_t nv, const void* d_faces, int faces_i64, int64_t nf,
                                double voxel_size, const double origin[3] /* or NULL */, int reduce /* PB3D_DOWNSAMPLE_* */,
                                int duplicate_faces, const uint8_t* d_colors /* nv x channels, or NULL */, int channels,
                                void* d_out_verts /* nv rows */, void* d_out_faces /* nf rows */, uint8_t* d_out_colors /* or NULL */,
                                int32_t* d_index /* nv, or NULL */, int32_t* d_inverse /* nv, or NULL */,
                                int32_t* d_face_index /* nf, or NULL */, int64_t counts[2] /* vertices, faces written */);
int pb3d_mesh_compact_resident(pb3d_ctx* ctx, const void* d_verts, int verts_f64, int64_t nv, const void* d_faces, int faces_i64, int64_t nf,
                               int duplicate_faces, const uint8_t* d_colors /* nv x channels, or NULL */, int channels,
                               void* d_out_verts /* nv rows */, void* d_out_faces /* nf rows */, uint8_t* d_out_colors /* or NULL */,
                               int32_t* d_index /* nv, or NULL */, int32_t* d_inverse /* nv, or NULL */,
                               int32_t* d_face_index /* nf, or NULL */, int64_t counts[2] /* vertices, faces written */);
int pb3d_simplify_last(pb3d_ctx* ctx, int64_t counts[3], double pass_ms[5] /* or NULL */);

/* ---- mesh components: connected components, edge counts and ordered measures of a triangle mesh (csrc/meshcomp.hip), and the mesh of
 * a face mask (csrc/simplify.hip) ------------------------------------------------------------------------------------------------------
 * The segmentation step for the third shape of data (cluster_points has the clouds, the labelling the grids): Open3D's
 * cluster_connected_triangles + remove_triangles_by_mask, trimesh's split / is_watertight.  There is no upstream text, so the rules
 * below are the specification, and the result is a function of the input and its order alone, to the bit.
 *   INPUT      faces: (nf, 3) rows of int32 (faces_i64 = 0) or int64 (1) with entries in [-nv, nv); entries in [-nv, -1] wrap as NumPy's
 *              do.  Anything else is PB3D_EINDEX, checked on the device before any kernel gathers through them (one host wait), with
 *              nothing written; nv = 0 with nf > 0 is PB3D_EINDEX.  verts (or NULL): (nv, 3) rows of float32 (verts_f64 = 0; widened)
 *              or float64 (1), read only for the measures; they must be finite (the caller's promise: pb3d.mesh_components checks it
 *              on the host), else area and volume are whatever IEEE arithmetic makes of them.  Limits: nv <= 2^31 - 1,
 *              nf <= (2^31 - 1) / 6.
 *   RECORDS    face j with wrapped corners (w0, w1, w2) gives the records 3j, 3j + 1, 3j + 2 for the directed edges (w0, w1), (w1, w2),
 *              (w2, w0).  A record with equal ends is a LOOP and takes no further part.  A record's undirected edge is (lo, hi); the
 *              record is FORWARD iff its source is lo.
 *   EDGES      an undirected edge with c records of which f are forward is BOUNDARY iff c == 1, NON-MANIFOLD iff c > 2, UNBALANCED iff
 *              2 f != c.  Unbalanced includes every boundary edge and every pair traversed twice the same way; no unbalanced edge is
 *              exactly "every directed edge has its reverse", what pb3d_voxelize_mesh_resident's crossing parity needs.
 *   CONNECT    PB3D_MESH_CONNECT_VERTEX: two faces are connected when they name a common vertex.  PB3D_MESH_CONNECT_EDGE: when an
 *              undirected edge has a record of each (Open3D's rule; an edge of many faces connects all of them).  Components are the
 *              classes of the transitive closure.  A face all of whose records are loops is a component of its own under EDGE and in
 *              the component of its vertex under VERTEX.
 *   NUMBERS    components are numbered 0 .. nc - 1 by their smallest face position.  face_labels[j] = the number of face j's component;
 *              vertex_labels[i] = the smallest label among the faces that name vertex i, -1 when none does.
 *   COUNTS     d_counts (or NULL; room for 5 nf int64) holds five arrays of nc, one behind the other: faces, edges, boundary edges,
 *              non-manifold edges, unbalanced edges of every component.  An edge belongs to the component of its faces, which is the
 *              same for all of them under both rules.
 *   MEASURES   d_measures (or NULL; needs verts; room for 2 nf float64) holds two arrays of nc: area, volume.  Per face, with the
 *              corners a, b, c as float64 and every operation below one rounded float64 operation (no FMA):
 *                e1 = b - a, e2 = c - a;  nx = e1y*e2z - e1z*e2y, ny = e1z*e2x - e1x*e2z, nz = e1x*e2y - e1y*e2x;
 *                A_j = 0.5 * sqrt((nx*nx + ny*ny) + nz*nz) with the correctly rounded square root;
 *                m = b x c formed like n;  S_j = (a.x*m.x + a.y*m.y) + a.z*m.z.
 *              A component's faces in ascending position are cut into blocks of 256, counted within the component's own list; a block
 *              sum starts at 0.0 and takes its faces in order; the total starts at 0.0 and takes the block sums in order.
 *              area = the total of A, volume = the total of S divided by 6.0: signed, and meaningful when the component has no
 *              unbalanced edge.
 *   TOTALS     totals[8] = components nc, vertices some face names V, undirected edges E, faces F = nf, boundary, non-manifold and
 *              unbalanced edges, loops.  The Euler characteristic is V - E + F.  Read back once, the call's one host wait behind the
 *              index check; everything else is enqueued.
 *   EMPTY      nf = 0: totals all 0, vertex_labels all -1, no host wait.
 * Nothing is kept per edge and no lane walks along a run of records: the 3 nf records go through two stable radix sorts of (key, record)
 * pairs, by hi and then by lo; run heads and forward bits are flagged and scanned, so c and f are differences at consecutive heads; the
 * components are a lock-free union-find whose roots are minima by construction (csrc/union_find.h); the counts are integer atomics; the
 * measures use no atomics: a stable sort of (label, face), one wavefront per block, one per component.  Scratch: about 170 bytes per
 * face (corners 12; pairs 48, flags 24, ranks 48 and edge starts 12 for its three records; the components' parent, flags and ranks 16;
 * scans and run table), 56 more with measures, 40 more without d_counts, 4 - 12 per vertex.
 * mesh_select_faces is mesh_compact's VERTICES, FACES OUT, ATTRIBUTES and outputs with the caller's flags in place of COLLAPSED and
 *   REPEATED: face j stays iff d_keep[j] != 0 (nf bytes), degenerate and repeated faces included, in order and in corner order; the
 *   vertices no kept face names go, the rest are renumbered in order and copied byte for byte.  Host waits: the index check and counts. */
#define PB3D_MESH_CONNECT_EDGE 0
#define PB3D_MESH_CONNECT_VERTEX 1
int pb3d_mesh_components_resident(pb3d_ctx* ctx, const void* d_verts /* or NULL */, int verts_f64, int64_t nv, const void* d_faces, int faces_i64,
                                  int64_t nf, int connectivity, int32_t* d_face_labels /* nf */, int32_t* d_vertex_labels /* nv, or NULL */,
                                  int64_t* d_counts /* 5 nf, or NULL */, double* d_measures /* 2 nf, or NULL */, int64_t totals[8]);
int pb3d_mesh_select_faces_resident(pb3d_ctx* ctx, const void* d_verts, int verts_f64, int64_t nv, const void* d_faces, int faces_i64, int64_t nf,
                                    const uint8_t* d_keep /* nf */, const uint8_t* d_colors /* nv x channels, or NULL */, int channels,
                                    void* d_out_verts /* nv rows */, void* d_out_faces /* nf rows */, uint8_t* d_out_colors /* or NULL */,
                                    int32_t* d_index /* nv, or NULL */, int32_t* d_inverse /* nv, or NULL */,
                                    int32_t* d_face_index /* nf, or NULL */, int64_t counts[2] /* vertices, faces written */);

/* ---- mesh repair: welding vertices by coordinate equality (csrc/weld.hip) and a consistent winding (csrc/orient.hip) -----------------------
 * What a triangle soup (an STL-style CAD export: three vertices of its own per face) or a mesh of mixed winding needs before
 * mesh_components, mesh_adjacency, mesh_smooth, mesh_simplify and the signed volumes mean anything.  trimesh's merge_vertices and
 * repair.fix_winding / fix_inversion, Open3D's remove_duplicated_vertices and orient_triangles are the relatives; there is no upstream
 * text, so the rules below are the specification, and both results are functions of the input and its order alone, to the bit.
 *
 * weld_vertices
 *   INPUT      verts: (nv, 3) rows of float32 (verts_f64 = 0) or float64 (1), finite (the caller's promise: pb3d.weld_vertices checks
 *              it on the host; a NaN would be compared by its bits).  faces (or NULL with nf = 0): (nf, 3) rows of int32 or int64 with
 *              entries in [-nv, nv), wrapping as NumPy's do; anything else is PB3D_EINDEX, checked before anything is written (one host
 *              wait).  Limits: nv <= 2^31 - 1, 3 nf <= 2^31 - 1.
 *   EQUALITY   two vertices are one iff their three coordinates compare equal as IEEE numbers of the input's width: -0.0 == +0.0,
 *              and nothing else that differs in a bit is equal.
 *   CLASSES    a class's representative is its smallest input position; classes are numbered 0 .. m - 1 in the order of their
 *              representatives (first appearance: voxel_downsample's FIRST numbering with equality classes for voxels).
 *              out_verts[k] = the representative's row byte for byte (a -0.0 stays -0.0); index[k] = its position; inverse[i] = the
 *              class of vertex i; class_counts[k] = the class's size.  A vertex no face names is welded like any other.
 *   FACES      out_faces[j][a] = inverse[wrap(faces[j][a])] in the caller's index dtype, order and corner order: never negative.  A
 *              face that becomes degenerate or a repeat stays (mesh_compact removes those).
 *   ATTRIBUTES with d_colors ((nv, channels) uint8, channels 1 or 3): out_colors[k] = colors[index[k]], unblended.
 *   EMPTY      nv = 0: *classes = 0, no host wait (nf > 0 is then PB3D_EINDEX).
 * Outputs: d_out_verts room for nv rows, d_out_colors (given iff d_colors is) nv x channels, d_index and d_class_counts (nv int32 /
 *   uint32, or NULL) of which the first *classes entries are written; d_inverse (nv int32, or NULL) and d_out_faces (nf rows, NULL iff
 *   nf = 0) whole.  No output may alias an input.  Host waits: the index check (nf > 0) and *classes.
 * One key word per 32 bits of coordinate (the raw bits, -0.0 mapped to +0.0: for finite values key equality is IEEE equality) and
 * one stable radix sort of (word, position) pairs per word, three or six: the positions start ascending, so the first record of every
 * run of equal rows is the class's smallest position.  No hashing, no per-class state, no atomics.  Scratch: about 50 bytes a vertex.
 *
 * mesh_orient
 *   INPUT, RECORDS, EDGES  mesh_components' exactly, limits included.  verts (or NULL) are read for the volumes alone.
 *   PAIR EDGES an undirected edge with c == 2 records is a PAIR EDGE; its two faces AGREE iff exactly one of the records is forward
 *              (f == 1: they traverse the edge in opposite directions) and DISAGREE otherwise.  Edges with c == 1 or c > 2 connect
 *              nothing: no winding is carried across a non-manifold edge.
 *   PATCHES    the classes of the faces under pair edges alone, numbered 0 .. np - 1 by their smallest face position.  A patch is
 *              ORIENTABLE iff a bit per face exists with flip[a] ^ flip[b] == disagree(a, b) on every pair edge; it is then unique
 *              up to complementing the patch.
 *   ANCHOR     in an orientable patch the smallest face keeps its winding (flip = 0), which fixes every other bit.  A patch that is
 *              not orientable keeps every face as it came (flip = 0 throughout) and is reported.
 *   SIGN       volume_sign = PB3D_ORIENT_POSITIVE or _NEGATIVE (needs verts, else PB3D_EINVAL) applies to the orientable patches
 *              without a boundary edge.  V = mesh_components' ordered sum over the patch (its faces in ascending position in blocks
 *              of 256, then the blocks, divided by 6.0) of the terms S_j of the INPUT winding, negated for a face the anchor rule
 *              flips (swapping corners 1 and 2 negates S_j exactly, so this is the S_j of the flipped face).  If V has the wrong sign
 *              (V < 0 under POSITIVE, V > 0 under NEGATIVE) the patch is INVERTED: every flip bit is complemented and V negated.
 *              V == 0 or NaN changes nothing.  The rule is per patch: nested shells are not analysed, a cavity's shell ends with the
 *              same sign as the outer one.  PB3D_ORIENT_KEEP: the anchor rule alone.
 *   FACES OUT  d_out_faces (or NULL): row j as it came, negative entries included, in the caller's index dtype; a flipped face
 *              (a, b, c) becomes (a, c, b), so the first corner stays.  Vertices are not touched.
 *   COUNTS     d_counts (8 nf int64) holds eight arrays of np, one behind the other: faces, pair edges, disagreeing pair edges (of
 *              the input), boundary edges (c == 1, counted for the patch of their face), records of the patch's faces on edges with
 *              c > 2, flipped faces (final), orientable (0 / 1), inverted (0 / 1).  d_volume (or NULL; needs verts; nf float64): V
 *              per patch, computed for every patch whether the sign rule covers it or not.
 *   TOTALS     totals[8] = patches, orientable patches, pair edges, disagreeing pair edges, flipped faces, inverted patches, boundary
 *              edges, non-manifold edges.  Read back once, the call's one host wait behind the index check.
 *   EMPTY      nf = 0: totals all 0, no host wait.
 * Outputs: d_flip (nf uint8) and d_patch (nf int32) whole.  No output may alias an input.
 * The records, sorts, heads and scans are mesh_components' own (one copy).  Orientation is the same min-root union-find on a doubled
 * forest of 2 nf nodes -- node j is "face j as it came", node nf + j "face j flipped" -- in which a pair edge with faces a, b and
 * disagreement d unites a ~ b + d nf and a + nf ~ b + (1 - d) nf.  With r0, r1 the roots of j and nf + j: the patch is not orientable
 * iff r0 == r1, its smallest face is min(r0, r1), and the anchor rule flips j iff r0 > r1 (roots are minima and every nf + k exceeds
 * every face number, so the set that holds the anchor unflipped is rooted at the anchor; DESIGN.md "Mesh repair").  Scratch:
 * mesh_components' and 8 + 16 bytes per face. */
#define PB3D_ORIENT_KEEP 0
#define PB3D_ORIENT_POSITIVE 1
#define PB3D_ORIENT_NEGATIVE 2
int pb3d_weld_vertices_resident(pb3d_ctx* ctx, const void* d_verts, int verts_f64, int64_t nv, const void* d_faces /* or NULL */, int faces_i64,
                                int64_t nf, const uint8_t* d_colors /* nv x channels, or NULL */, int channels, void* d_out_verts /* nv rows */,
                                void* d_out_faces /* nf rows */, uint8_t* d_out_colors /* or NULL */, int32_t* d_index /* nv, or NULL */,
                                int32_t* d_inverse /* nv, or NULL */, uint32_t* d_class_counts /* nv, or NULL */, int64_t* classes);
int pb3d_mesh_orient_resident(pb3d_ctx* ctx, const void* d_verts /* or NULL */, int verts_f64, int64_t nv, const void* d_faces, int faces_i64,
                              int64_t nf, int volume_sign, uint8_t* d_flip /* nf */, int32_t* d_patch /* nf */, void* d_out_faces /* nf rows, or NULL */,
                              int64_t* d_counts /* 8 nf */, double* d_volume /* nf, or NULL */, int64_t totals[8]);

/* ---- mesh -> grid: exact solid voxelization of a triangle mesh by crossing parity, and the overlap of two grids (csrc/voxelize.hip) ------
 * The one conversion the other sections lack: a mesh (a CAD model, a smoothed marching-cubes mesh) becomes an occupancy, label or RGB grid
 * that the carve, paint, points and labelling entries take as it is.  Solid voxelization by crossing parity (Schwarz & Seidel 2010) with a
 * symbolic tie rule.  There is no upstream text, so the rules below are the specification, and the result is a function of the input
 * alone, to the bit: the only shared writes are integer XORs of single bits, which commute.
 *   INPUT      verts: (nv, 3) rows of float32 (verts_f64 = 0) or float64 (1); faces: (nf, 3) rows of int32 (faces_i64 = 0) or int64 (1)
 *              with entries in [-nv, nv), wrapping as NumPy's do.  Anything else is PB3D_EINDEX; a vertex coordinate that is not finite
 *              (of any vertex, used or not) is PB3D_EINVAL.  Both are checked on the device in one sweep before any kernel gathers, at the
 *              price of one host wait, and d_out is untouched when they fail.  Grid n0 x n1 x n2, each >= 1, n0 * n1 * n2 <= 2^31 - 1
 *              (the labelling entries' limit); nv <= 2^31 - 1, 3 * nf <= 2^31 - 1.  origin[3] finite, voxel_size finite and > 0.
 *              Voxel (i, j, k) is the SAMPLE POINT origin + voxel_size * (i, j, k); a caller who means cell centres shifts origin by half
 *              a voxel.
 *   ARITHMETIC all float64; float32 is widened first, which is exact.  Every product, sum, difference and quotient below is one rounded
 *              IEEE operation, no FMA.  As for mesh_dist, coordinates must be small enough that no product overflows.
 *   LATTICE    frame = 0 ("lattice"): L = (v - origin) / voxel_size per axis, the vertex's columns in order (a0, a1, a2).
 *              frame = 1 ("meshify"): first v' = (depth - v[2], v[1], v[0]), one subtraction, then as above: the inverse of the frame
 *              pb3d_mesh_fill_dev hands out (its vertices are (a2, a1, A2 - a0)); depth = n2 is right for stride 1, origin 0, voxel_size 1.
 *   FACE       (A, B, C) in lattice coordinates, rays along a2:
 *              1. area = (B0-A0)*(C1-A1) - (B1-A1)*(C0-A0); area == 0: the face contributes nothing (two equal projected corners give
 *                 exactly 0 by this formula).
 *              2. columns i = max(0, ceil(min(A0,B0,C0))) .. min(n0-1, floor(max(A0,B0,C0))), j likewise on axis 1, both clamped in
 *                 float64 before the conversion to integer.
 *              3. each directed edge (P, Q) of (A,B), (B,C), (C,A): flipped = (Q0, Q1) < (P0, P1) lexicographically; lo, hi = its ends in
 *                 ascending lexicographic order; E = (hi0-lo0)*(j-lo1) - (hi1-lo1)*(i-lo0); pos = (area > 0) != flipped; the edge accepts
 *                 the column if pos ? E >= 0 : E < 0.  The face crosses the column if all three edges accept it.  The two faces of a
 *                 shared edge evaluate the same E bit for bit and exactly one of them owns a column on it: the rule is the sample moved
 *                 by the infinitesimal (-eps^2, +eps), so it is consistent at vertices too, and independent of the faces' winding.
 *              4. nx = (B1-A1)*(C2-A2) - (B2-A2)*(C1-A1); ny = (B2-A2)*(C0-A0) - (B0-A0)*(C2-A2);
 *                 z = A2 - (nx*(i-A0) + ny*(j-A1)) / area; k = ceil(z).  k <= n2-1: the crossing flips bit (i, j, max(k, 0)); otherwise
 *                 (above the grid; also a z that is NaN) it flips the column's overflow bit.
 *   RESULT     occ[i,j,k] = parity of the crossings of column (i, j) at bits 0 .. k.  A sample exactly on the surface is inside where the
 *              ray enters and outside where it leaves.  For a closed mesh in exact arithmetic this is the point-in-solid test of the
 *              displaced samples; for any other input (an open mesh, one that intersects itself, coordinates whose products round) it is
 *              still exactly this function of the input, and nothing more is claimed.  Every operation above is exact when the lattice
 *              coordinates are small multiples of a power of two -- half-integer coordinates, marching-cubes output at unit or
 *              power-of-two voxel_size -- and the round trip voxelize(marching_cubes(mask)) == mask (tests) rests on that.
 *              Pinned: the box with corners (2,3,1) and (6,7,5), 12 triangles, in a 9 x 10 x 8 grid fills i 3..6, j 3..6, k 1..4.
 *   OUTPUT     d_out: n0*n1*n2*channels uint8, channels 1 or 3, written whole: inside voxels take value[0 .. channels), outside 0.
 *   STATS      stats[4] int64 or NULL (not NULL: one more host wait, one download): crossings; occupied voxels; open columns (total
 *              parity, overflow bit included, is odd: the mesh leaks there or leaves the grid's side); faces with area == 0.
 * nf = 0 gives an all-zero grid.  PB3D_EINVAL: a grid axis < 1 or too many voxels, origin / voxel_size / depth not finite,
 * voxel_size <= 0, frame not 0 or 1, channels not 1 or 3.
 * Two passes over a bit volume of n0 * n1 * (ceil(n2 / 32) + 1) dwords (32 planes per dword, one more dword per column for the overflow
 * bit).  Crossings: one lane per face computes the set-up once; a face of at most 16 columns is walked by its lane, a wider one is listed
 * and walked by a workgroup; a crossing is one atomicXor of one bit.  Scan: per column the prefix XOR (shifts inside a dword, a ballot of
 * the dwords' parities across them), then the bytes along a2 (16 voxels per lane in 16-byte stores when n2 is a multiple of 16 and d_out is
 * 16-byte aligned, 64 consecutive bytes per store instruction otherwise: only speed depends on it); the same pass counts the occupied
 * voxels and the open columns.  No floating-point atomics.  Scratch: the bit volume (n2 = 512: 17/128 of a byte per voxel), 4 bytes per face
 * and 40 bytes of counters.  Knob "voxelize_timing" (pb3d_set_tuning; one more host wait) times the two passes with events:
 * pb3d_voxelize_last gives the milliseconds of the crossing pass (the bit volume's clear included) and of the scan pass of the last
 * call, PB3D_EINVAL if it was not timed. */
int pb3d_voxelize_mesh_resident(pb3d_ctx* ctx, const void* d_verts, int verts_f64, int64_t nv, const void* d_faces, int faces_i64, int64_t nf,
                                int64_t n0, int64_t n1, int64_t n2, const double origin[3], double voxel_size, int frame, double depth,
                                int channels, const uint8_t* value /* channels bytes */, uint8_t* d_out /* n0*n1*n2*channels */,
                                int64_t stats[4] /* or NULL */);
int pb3d_voxelize_last(pb3d_ctx* ctx, double pass_ms[2]);
/* Volume overlap of two resident grids of nvox voxels: out = {voxels non-zero in both, in a, in b}, where non-zero means any channel > 0
 * (_occupancy's reading; channels 1 or 3 per grid, the two may differ).  Exact integers; one sweep and one download (one host wait). */
int pb3d_grid_overlap_resident(pb3d_ctx* ctx, const uint8_t* d_a, int channels_a, const uint8_t* d_b, int channels_b, int64_t nvox,
                               int64_t out[3]);

/* ---- containment: which points of a cloud lie inside a triangle mesh, and signed mesh distances (csrc/inside.hip) --------------------
 * The relation the other sections lack: mesh_dist says how far a point is from the surface, not on which side.  The rule is the
 * voxelization's above -- its FACE and RESULT rules with the column (i, j) replaced by the query's (q0, q1), from the same text
 * (csrc/cross_rule.h) -- so at a lattice point the byte is the voxel's, and as there the result is a function of the input alone, to the
 * bit.  There is no upstream text: the rules below are the specification.
 *   INPUT      d_P: (nP, 3) rows of float32 (p_f64 = 0) or float64 (1).  verts, faces: as for the voxelization, with its checks: an
 *              index outside [-nv, nv) is PB3D_EINDEX, a vertex coordinate that is not finite (of any vertex, used or not)
 *              PB3D_EINVAL, both found in one sweep before any kernel gathers (one host wait), and nothing is written when they
 *              fail.  nP, nv and 3 * nf <= 2^31 - 1.  No frame, origin or voxel size is applied: vertices and queries are used as given.
 *   ARITHMETIC all float64; float32 is widened first, which is exact.  Every product, sum, difference and quotient below is one rounded
 *              IEEE operation, no FMA.  Rays run along the third coordinate.
 *   FACE       query q against face (A, B, C):
 *              1. area as in the voxelization's step 1; area == 0: the face contributes nothing.
 *              2. box: the face is considered only if min(A0,B0,C0) <= q0 <= max(A0,B0,C0), and likewise on axis 1.  At integer q this is
 *                 the voxelization's step 2.
 *              3. the three edges as in the voxelization's step 3 with i -> q0, j -> q1: flipped, lo, hi, E, pos and the accept condition
 *                 pos ? E >= 0 : E < 0 unchanged.  The face COVERS the query if the box holds it and all three edges accept it.
 *              4. z = A2 - (nx*(q0-A0) + ny*(q1-A1)) / area with nx, ny as in the voxelization's step 4.
 *   RESULT     total = the number of covering faces; below = the number of covering faces with z <= q2 (a NaN z counts in total only, as
 *              the voxelization's overflow bit does); inside = below & 1.  An odd total means the mesh is open over this query (the
 *              voxelization's open column); the answer is still exactly this function of the input.  As there, nothing more is claimed
 *              for an open mesh, one that intersects itself, or coordinates whose products round.  Pinned: the box with corners (2,3,1)
 *              and (6,7,5), 12 triangles, queried at the 720 lattice points of a 9 x 10 x 8 grid, is inside at i 3..6, j 3..6, k 1..4.
 *   QUERIES    A query with a NaN coordinate compares false everywhere: it is outside with below = total = 0, and counts among the
 *              queries outside the box.  An infinite q2 is a coordinate like any other (+inf: below = total).  The NumPy form refuses
 *              queries that are not finite; a resident caller gets the above.
 *   OUTPUT     d_inside: nP bytes, 0 or 1.  d_counts (or NULL): nP x 2 int32, (below, total) per query.
 *   STATS      stats[4] int64 or NULL (not NULL: one more host wait, one download): queries inside; queries with an odd total; faces
 *              with area == 0; queries outside the (a0, a1) box of the vertices (they are outside, with no face looked at).
 * nP = 0 does nothing beyond the check (stats: four zeros).  nf = 0 gives all outside: zero counts, stats {0, 0, 0, nP}.
 * Index: a 2-D cell grid over the exact (a0, a1) box of ALL vertices, sized from nf by the rule of nn_dist's grid; a face with
 * area != 0 is listed in every cell of cell(min corner) .. cell(max corner) per axis, and because that cell function is monotone a face
 * whose box holds (q0, q1) is listed in the query's cell.  While the (cell, face) entries exceed 8 * nf and the grid has more than one
 * cell, the cells per axis are halved (mesh_dist's defence against one giant face among small ones).  One lane per query walks the list
 * of its one cell; no atomics on the query side, no floating-point atomics anywhere.  Host waits: the check, the box, 1 + (number of
 * halvings) for the entry counts; the query itself is enqueued.  Scratch: 72 bytes per face, 4 bytes per entry, 12 bytes per cell, 12
 * bytes per 256 queries with stats.
 * points_in_mesh_last: info = {cells along a0, cells along a1, (cell, face) entries, halvings} of the index the last call with nP > 0
 *   on this context built (four zeros after nf = 0), PB3D_EINVAL before the first.  pass_ms (or NULL): the milliseconds of the index
 *   build and of the query from the call's own events under knob "inside_timing" (pb3d_set_tuning; one more host wait), PB3D_EINVAL if
 *   the last call was not timed.  Knob "inside_order" = 1 walks the queries in the index's cell order instead of the caller's, knob
 *   "inside_table" = 1 reads each face's finished set-up from a table (184 more bytes of scratch per face) instead of computing it
 *   from the corners; no byte depends on any of the three.
 * mesh_dist_sign: d_out[i] = (d_inside[i] != 0 && d_dist[i] > 0) ? -d_dist[i] : d_dist[i] for i < n -- mesh_dist's distances, signed
 *   by the bytes above: negative inside, and a point on the surface keeps +0.0.  d_out may be d_dist.  Enqueued.
 * flags_not: d_out[i] = d_flags[i] == 0 for i < n, what pb3d_points_select_resident needs to keep the points OUTSIDE a mesh.  d_out may
 *   be d_flags.  Enqueued. */
int pb3d_points_in_mesh_resident(pb3d_ctx* ctx, const void* d_P, int p_f64, int64_t nP, const void* d_verts, int verts_f64, int64_t nv,
                                 const void* d_faces, int faces_i64, int64_t nf, uint8_t* d_inside /* nP */,
                                 int32_t* d_counts /* nP x 2: below, total; or NULL */, int64_t stats[4] /* or NULL */);
int pb3d_points_in_mesh_last(pb3d_ctx* ctx, int64_t info[4], double pass_ms[2] /* or NULL */);
int pb3d_mesh_dist_sign_resident(pb3d_ctx* ctx, const double* d_dist, const uint8_t* d_inside, int64_t n, double* d_out);
int pb3d_flags_not_resident(pb3d_ctx* ctx, const uint8_t* d_flags, int64_t n, uint8_t* d_out);

/* ---- grid -> distance: the exact Euclidean distance transform with its feature transform (csrc/edt.hip) ------------------------------
 * Squared distances on a lattice are integers, so the transform is stated to the bit; there is no upstream text and the rules below are
 * the specification.  scipy.ndimage.distance_transform_edt(x) equals sqrt((double)sq) of PB3D_EDT_TO_BACKGROUND bit for bit (tests).
 *   GRID       (n0, n1, n2) voxels of `channels` (1 or 3) uint8 each, every axis in [1, 16384] (so 3 * 16383^2 < 2^31: every squared
 *              distance fits int32), at most 2^31 - 1 voxels; anything else is PB3D_EINVAL.  A voxel is OCCUPIED when any of its
 *              channels is non-zero (pb3d_grid_overlap_resident's rule).
 *   TARGETS    target = PB3D_EDT_TO_BACKGROUND (0): the voxels that are not occupied (SciPy's convention);
 *              PB3D_EDT_TO_OCCUPIED (1): the occupied voxels;
 *              PB3D_EDT_TO_SURFACE (2): the occupied voxels with at least one of their 6 neighbours not occupied or outside the grid.
 *   SQ         d_sq[v] = min over the targets t of (v0-t0)^2 + (v1-t1)^2 + (v2-t2)^2, int32; 0 on a target.  With border_is_target != 0
 *              the six planes just outside the grid are targets too: sq[v] = min(sq[v], (v_a + 1)^2, (n_a - v_a)^2) over the axes a
 *              (border_value = 0 of SciPy's morphology).  With no target and no border every sq is PB3D_EDT_NONE = INT32_MAX.
 *   NONE       PB3D_EDT_NONE never enters a sum: neither widened nor saturated.  A pass tests a partial result for PB3D_EDT_NONE before
 *              it uses it and leaves such a voxel out of the minimisation (it is no parabola of the envelope); what remains is at most
 *              3 * 16383^2 and no sum or difference of the passes leaves int32.
 *   INDEX      d_index[v] (int32, or NULL: not written) = the linear index (t0 * n1 + t1) * n2 + t2 of a nearest target, -1 where sq is
 *              PB3D_EDT_NONE.  TIE RULE: among the targets at the minimum squared distance, the smallest linear index, which is the
 *              lexicographic minimum of (t0, t1, t2).  The rule is separable: the row pass (axis 2) gives every voxel (i, j, k) the
 *              nearest target of its row, the smaller t2 of an equidistant left / right pair, so R(i, j, k) holds, for row (i, j), the
 *              least (distance, t2).  The axis-1 pass minimises R(i, j', k) + (j - j')^2 over j' and keeps the smallest j' among equal
 *              totals: a target (t1, t2) of plane i at the plane's minimum distance from (j, k) with the smallest t1 is found at
 *              j' = t1, and within row t1 the row pass already kept the smallest t2 at that distance.  The axis-0 pass does the same
 *              with i' and keeps the smallest t0.  So the result is the minimum of (distance, t0, t1, t2) in that order.  SciPy's
 *              return_indices follows no such rule (tests); it serves only to check that an index is A nearest target.
 *              d_index with border_is_target != 0 is PB3D_EINVAL: a border plane has no index.
 *   NO FLOATS  No floating-point operation computes sq or index.  The column passes build the lower envelope of the parabolas
 *              g(j') + (j - j')^2 with Meijster's integer Sep(i, u) = (u^2 - i^2 + g(u) - g(i)) div (2 (u - i)), i < u: the largest x
 *              at which parabola i is not above parabola u, so a tie goes to the smaller index.  The numerator is never negative where
 *              it is evaluated (parabola i is not above u at some x >= 0), so the division is that of non-negative integers.
 *   STATS      stats (host, or NULL) = {number of target voxels (border planes not counted), the largest sq that is not PB3D_EDT_NONE
 *              or -1 when there is none}.  Not NULL: one download and one host wait; NULL: the entry only enqueues.
 * Scratch: 8 bytes per voxel (the other half of the passes' ping-pong and the envelope stacks), 4 more with d_index.
 *
 * pb3d_edt_distances_resident: out[v] = sqrt((double)sq[v]) * voxel_size for n values, one correctly rounded square root and one rounded
 *   product, float64 (out_f64 != 0) or that rounded once more to float32; PB3D_EDT_NONE gives +inf.  voxel_size finite and > 0.
 * pb3d_edt_apply_resident: mode PB3D_EDT_FILL: an occupied voxel keeps its bytes, an empty one with sq[v] <= r_sq takes the bytes of
 *   voxel index[v] (d_sq, d_index: PB3D_EDT_TO_OCCUPIED output), every other voxel becomes zero: dilation by the Euclidean ball of
 *   squared radius r_sq, coloured by the nearest voxel.  mode PB3D_EDT_KEEP: a voxel keeps its bytes when sq[v] > r_sq and becomes zero
 *   otherwise (d_index unused, may be NULL); with PB3D_EDT_TO_BACKGROUND output this is erosion by the ball.  d_out may be d_grid (FILL
 *   gathers only from occupied voxels, which keep their bytes).  r_sq >= 0.
 * pb3d_grid_surface_stats_resident: over the surface voxels v of grid a (PB3D_EDT_TO_SURFACE's rule) with s = d_sq_to_b_surface[v]:
 *   out = {their number, max s (-1 without a surface voxel), sum of s, and per k < nthr the number with s <= thresholds_sq[k]}.  int64
 *   atomic max and add only, one per workgroup of a capped grid: independent of order.  0 <= nthr <= 8.  One download, one host wait. */
#define PB3D_EDT_NONE 2147483647
#define PB3D_EDT_MAX_AXIS 16384
enum { PB3D_EDT_TO_BACKGROUND = 0, PB3D_EDT_TO_OCCUPIED = 1, PB3D_EDT_TO_SURFACE = 2 };
enum { PB3D_EDT_FILL = 0, PB3D_EDT_KEEP = 1 };
int pb3d_edt_resident(pb3d_ctx* ctx, const uint8_t* d_grid, int channels, int64_t n0, int64_t n1, int64_t n2, int target, int border_is_target,
                      int32_t* d_sq, int32_t* d_index /* may be NULL */, int64_t* stats /* host, may be NULL: [0] targets, [1] max finite sq or -1 */);
int pb3d_edt_distances_resident(pb3d_ctx* ctx, const int32_t* d_sq, int64_t n, double voxel_size, int out_f64, void* d_out);
int pb3d_edt_apply_resident(pb3d_ctx* ctx, const uint8_t* d_grid, int channels, int64_t nvox, const int32_t* d_sq, const int32_t* d_index, int mode,
                            int64_t r_sq, uint8_t* d_out);
int pb3d_grid_surface_stats_resident(pb3d_ctx* ctx, const uint8_t* d_a, int channels_a, int64_t n0, int64_t n1, int64_t n2,
                                     const int32_t* d_sq_to_b_surface, const int64_t* thresholds_sq, int nthr /* <= 8 */,
                                     int64_t* out /* host: [0] surface voxels of a, [1] max sq, [2] sum sq, [3+k] #(sq <= thresholds_sq[k]) */);

/* ---- mesh -> image: depth, face and colour images of a triangle mesh under a pinhole camera (csrc/render.hip) --------------------------
 * The pair the other sections lack: a mesh (the smoothed marching-cubes mesh, a CAD model) seen by the camera the projection entries use,
 * as a z-buffer, a face image and a part-colour image that pb3d_partwise_iou_dev and the carve entries take as they are.  There is no
 * upstream text, so the rules below are the specification, and the result is a function of the input alone, to the bit: the only shared
 * writes are integer minima, which commute.  The ray test is Woop, Benthin and Wald 2013 ("Watertight ray/triangle intersection")
 * without their float fallback, because everything here is already double.
 *   ARITHMETIC all float64; float32 input is widened first, which is exact.  Every product, sum, difference and quotient below is one
 *              correctly rounded IEEE operation, no FMA (the build has -ffp-contract=off on host and device).
 *   INPUT      verts: (nv, 3) rows of float32 (verts_f64 = 0) or float64 (1); faces: (nf, 3) rows of int32 (faces_i64 = 0) or int64 (1)
 *              with entries in [-nv, nv), those in [-nv, -1] wrapping as NumPy's do.  Any other index is PB3D_EINDEX; a vertex (used or
 *              not) with a coordinate that is not finite is PB3D_EINVAL.  Both are checked on the device before any kernel gathers
 *              through the indices: the call's one host wait besides the job count below, and no output is written when they fail.
 *              Limits: nv, nf <= 2^31 - 1; Himg, Wimg > 0, Himg * Wimg <= 2^31 - 1; f finite and > 0; cx, cy, cam, R finite; near
 *              finite and > 0; frame 0 or 1 (depth finite with 1); d_depth not NULL and 8-byte aligned.  Anything else is PB3D_EINVAL
 *              before any device work.
 *   FRAME      frame = 0 ("points"): p = v, the (x, y, z) frame pb3d_project_dev sees, where voxel (a0, a1, a2) is (a2, a1, a0).
 *              frame = 1 ("meshify"): p = (v0, v1, depth - v2), one subtraction: the inverse of the frame pb3d_mesh_fill_dev hands out
 *              (its vertices are (a2, a1, A2 - a0); depth = A2), the convention of pb3d_voxelize_mesh_resident's frame = 1.
 *   CAMERA     R[9] row-major, rows x, y, z (the host's look_at_rotation taken in float64); cam[3], f, cx, cy float64.  Once per vertex:
 *              q = p - cam; X = (R0*q0 + R1*q1) + R2*q2; Y = (R3*q0 + R4*q1) + R5*q2; Z = (R6*q0 + R7*q1) + R8*q2.
 *   PIXEL      (u, v) integers, 0 <= u < Wimg, 0 <= v < Himg.  The pixel's ray goes through its integer centre, the pixel
 *              pb3d_project_dev rounds to: sx = ((double)u - cx) / f; sy = -(((double)v - cy) / f).
 *   FACE against PIXEL, corners a, b, c with camera coordinates (Xa, Ya, Za) ...:
 *              sheared corners xa = Xa - sx*Za, ya = Ya - sy*Za (a product, then a difference), b and c likewise;
 *              U = xc*yb - yc*xb; V = xa*yc - ya*xc; W = xb*ya - yb*xa; det = (U + V) + W; T = (U*Za + V*Zb) + W*Zc; t = T / det.
 *              The face HITS the pixel iff it is not the case that some of U, V, W is < 0 while another is > 0, and det != 0, and
 *              t >= near, every comparison IEEE (a NaN fails t >= near).  Both windings hit: no culling by orientation.
 *   RESULT     each pixel takes the hitting face with the smallest (t as computed, face number), compared lexicographically.
 *              depth[v,u] = that t as float64, +inf when nothing hits; face[v,u] = its number as int32, -1 when nothing hits;
 *              bary[v,u] = (U/det, V/det, W/det) of that face, (0, 0, 0) when nothing hits.  t is the camera-space Z of the hit, the
 *              quantity the z-buffers (pb3d_depth_buffer_dev, pb3d_grid_depth_buffer_dev) store.
 *   SHADE      a pass of its own (pb3d_render_shade_resident) on face and bary, a per-vertex attribute of C = 1 or 3 bytes and a
 *              background of C bytes: the corner m is the first of (a, b, c) with the largest weight -- a later corner replaces an
 *              earlier one only if its weight is strictly larger -- and image[v,u] = attr[faces[face][m]], the background where
 *              face is -1.  No blending: part colours and labels stay part colours and labels.  The pass only enqueues; a face
 *              number outside [0, nf) or a corner index outside [-nv, nv) is never followed, the pixel takes the background.
 * Two properties the tests lean on:
 *   SHARED EDGES  The value on an edge (U for edge b-c, V for c-a, W for a-b) is computed from the same two sheared vertices in both
 *              faces that share the edge, so it is the same number up to sign (a*b - c*d and c*d - a*b round to negatives of each
 *              other), and the zero case is inclusive: a ray cannot pass between two faces that share an edge, and a ray exactly on
 *              the edge hits both.  A closed mesh is hit an even number of times by a ray from outside.
 *   NO CLIPPING   A face that crosses the camera plane needs no clipping step: the test is on the ray's line, and t >= near discards
 *              what lies behind.
 *   PRUNE      A face is tested only against the pixels of a box, by exactly these rules (h = near / 2, exact):
 *              1. all three Z < h: the face is dropped.  Where U, V, W do not disagree in sign, the computed t is a quotient of
 *                 same-signed sums bounded by the largest Z up to a few roundings, far below the factor 2, so it cannot reach near.
 *              2. all three Z >= h: the box of the projected corners px = (X/Z)*f + cx, py = (-(Y/Z))*f + cy, from floor(min) - 1 to
 *                 ceil(max) + 1, clamped to the image; a face whose box misses the image is dropped.  With every Z positive the sheared
 *                 corners are Z/f times the pixel offsets, and the sign of a computed U, V or W is the sign of the exact one or zero
 *                 (rounding is monotone), so a pixel a whole pixel outside the corners' box sees them disagree.
 *              3. otherwise (corners on both sides of h, or a NaN among the projected corners): the whole image.  Rare, and correct.
 *              Every double -> int conversion of a box edge happens after the clamp to the image in double: a corner at Z = h projects
 *              to about 1e12 pixels, and converting that, or a NaN, directly is undefined.
 * Passes: camera coordinates and the check in one sweep (24 bytes of scratch per vertex); one lane per face classifies, walks a box of at
 * most 64 pixels itself and counts 8 x 8-pixel tile jobs for any other face; pb3d_scan_counts gives the job offsets, whose total (with
 * the three face counts) is the second host wait; one wavefront per (face, tile) job, one pixel per lane, finds its face by a binary
 * search of the offsets -- a triangle that fills the image is thousands of independent jobs, never one loop.  Depth: atomicMin on the
 * uint64 pattern of t (t >= near > 0, so the patterns order as the doubles do) into d_depth, pre-filled with the pattern of +inf.  Face:
 * the same walk again, a face whose t equals the pixel's depth bit for bit does atomicMin on its number into d_face, pre-filled with
 * 0xffffffff; skipped when neither d_face nor d_bary is asked for.  Resolve (d_bary only): one lane per pixel recomputes U, V, W of the
 * winner.  No floating-point atomics.  Scratch: 24 bytes per vertex, 16 per face (jobs 4, offsets 8, scan 4 and a little), 4 per pixel
 * when d_face is NULL and d_bary is not.
 * pb3d_render_last: of the last completed pb3d_render_mesh_resident of the context, {faces dropped by PRUNE 1 or 2, faces on the small
 * path, faces on the large path, tile jobs}.  Knob "render_timing" (pb3d_set_tuning; one more host wait) times the passes with events:
 * pb3d_render_last_ms gives the milliseconds of {small-path depth with the classification, the scan and its wait; tile depth;
 * small-path face; tile face; resolve} of a call with nf > 0 and a face or bary image, PB3D_EINVAL if the last call was not timed. */
int pb3d_render_mesh_resident(pb3d_ctx* ctx, const void* d_verts, int verts_f64, int64_t nv, const void* d_faces, int faces_i64, int64_t nf,
                              int frame, double depth, const double R[9], const double cam[3], double f, double cx, double cy, int Himg,
                              int Wimg, double near, double* d_depth /* Himg*Wimg */, int32_t* d_face /* Himg*Wimg, or NULL */,
                              double* d_bary /* Himg*Wimg*3, or NULL */);
int pb3d_render_shade_resident(pb3d_ctx* ctx, const int32_t* d_face, const double* d_bary, int64_t npix, const void* d_faces, int faces_i64,
                               int64_t nf, int64_t nv, const uint8_t* d_attr /* nv*C */, int C, const uint8_t* bg /* host, C bytes */,
                               uint8_t* d_image /* npix*C */);
int pb3d_render_last(const pb3d_ctx* ctx, int64_t stats[4]);
int pb3d_render_last_ms(const pb3d_ctx* ctx, double pass_ms[5]);

/* ---- rays against a mesh: the first hit, or any hit, of arbitrary rays on a triangle mesh (csrc/raycast.hip) --------------------------
 * "What does this ray hit first?" for rays the caller chooses: occlusion of the segment from a point to an eye, distances along a normal,
 * orthographic depths, thickness.  There is no upstream text, so the rules below are the specification, and the result is a function
 * of the input alone, to the bit: every output is written once by the one lane that owns the ray, and there are no atomics.  The face test
 * is "mesh -> image"'s (Woop, Benthin and Wald 2013) with the ray's own shear in place of the pixel's.
 *   ARITHMETIC all float64; float32 input is widened first, which is exact.  Every product, sum, difference and quotient below is one
 *              correctly rounded IEEE operation, no FMA.
 *   INPUT      origins o and directions d: (nrays, 3) rows of float32 (rays_f64 = 0) or float64 (1), one flag for both arrays.  verts
 *              and faces exactly as pb3d_render_mesh_resident takes them (float32 / float64, int32 / int64, indices in [-nv, nv)
 *              wrapping; any other index PB3D_EINDEX, a vertex that is not finite PB3D_EINVAL, both checked on the device before anything
 *              gathers: one host wait, and no output is written when they fail).  t_min finite, t_max finite or +inf, t_min <= t_max.
 *              nf == 0 or nrays == 0 is legal: every ray misses, no index is built.  Limits: nv, nf, nrays <= 2^31 - 1; ray buffers
 *              aligned to their element, d_t and d_bary to 8 bytes, d_face to 4.  Anything else is PB3D_EINVAL before any device work.
 *   BAD RAY    a ray with a component of o or d that is not finite, or with d == (0, 0, 0), hits nothing (and is counted).
 *   RAY        once per ray: kz = the axis of the largest |d| (a later axis replaces an earlier one only if it is strictly larger);
 *              kx = (kz + 1) % 3; ky = (kz + 2) % 3; Sx = d[kx] / d[kz]; Sy = d[ky] / d[kz]; Sz = 1.0 / d[kz].  No winding swap:
 *              nothing is culled by orientation.
 *   FACE against RAY, corners a, b, c:  A' = a - o per component, B', C' likewise;
 *              ax = A'[kx] - Sx*A'[kz], ay = A'[ky] - Sy*A'[kz] (a product, then a difference), b and c likewise;
 *              U = cx*by - cy*bx; V = ax*cy - ay*cx; W = bx*ay - by*ax; det = (U + V) + W;
 *              T = (U*(Sz*A'[kz]) + V*(Sz*B'[kz])) + W*(Sz*C'[kz]); t = T / det.
 *              The face HITS iff it is not the case that some of U, V, W is < 0 while another is > 0, and det != 0, and t >= t_min, and
 *              t <= t_max, every comparison an IEEE comparison of doubles: -0.0 >= 0.0 holds, a NaN fails.  The hit point is o + t d;
 *              t is in units of |d|.
 *   RESULT     each ray takes the hitting face with the smallest (t, face number); t is compared as a double, so -0.0 and +0.0 tie and
 *              the face number decides.  t[r] = that face's t as computed, +inf when nothing hits; face[r] = its number as int32, -1
 *              when nothing hits; bary[r] = (U/det, V/det, W/det) of that face, zeros when nothing hits.
 *   ANY HIT    any_hit != 0: hit[r] = 1 iff some face hits, which is face[r] >= 0 of the first-hit mode; the walk may stop at the first
 *              hit it meets, and which face that is is not a function of the input, so d_t, d_face and d_bary must be NULL
 *              (PB3D_EINVAL otherwise).  With any_hit == 0 d_hit must be NULL, d_t and d_face are required and d_bary may be NULL.
 * Two properties the tests lean on:
 *   SHARED EDGES  carries over from "mesh -> image": a sheared corner depends on its vertex and the ray only, so the value on an edge
 *              is the same number up to sign in both faces that share it; a ray cannot pass between two faces that share an edge, and a
 *              ray exactly on the edge hits both.
 *   RENDER     With o = cam for every ray, R the identity and d = (sx, sy, 1) for the pixel's sx, sy with |sx|, |sy| < 1, the operations
 *              are pb3d_render_mesh_resident's (frame 0), one for one: kz = 2, Sx = sx / 1 = sx, Sz = 1, the camera coordinates are
 *              p - cam (the products with the identity's 0 and 1 add zeros), and t_min = near, t_max = +inf.  So t and face equal its
 *              depth and face images bit for bit on any mesh.
 * The walk.  The faces are binned by csrc/face_index.hip over all three axes, nothing skipped: a face is listed in every cell of
 * cell_of(min corner) .. cell_of(max corner) per axis, and cell_of is monotone.  One lane per ray walks the layers of cells along kz, in
 * the ray's direction, over the ray's kz range (o[kz] + t_min d[kz] .. o[kz] + t_max d[kz]) clipped to the box of the vertices.  Per layer
 * it evaluates o[k] + S (z - o[kz]) for k = kx, ky at the layer's two bounding planes (the first and last layers reach the box's exact
 * faces; both planes clipped to the ray's range), widens each interval, skips the layer if an interval misses the box, converts both ends
 * with cell_of and tests every face listed in every cell of that rectangle (|Sx|, |Sy| <= 1: usually 1 - 4 cells).  A face listed in
 * several visited cells is tested again; the minimum is idempotent.
 *   MARGINS    tol = 1e-12 x the largest absolute coordinate among the box corners and the origin.  The ray's kz range is widened by tol
 *              and each kx / ky interval by 4 tol.  Why that is conservative: where U, V, W agree in sign, U/det, V/det, W/det are
 *              weights in [0, 1] up to rounding, t d[kz] is that weighted mean of the corners' A'[kz], and the sheared corners' weighted
 *              mean is zero -- so the point of the EXACT ray at the hit's kz lies in the face's box on all three axes, up to the
 *              rounding of some twenty operations on numbers no larger than |a - o|: a few 1e-16 of the largest coordinate, four
 *              orders below tol.  The plane positions lo + c h and cell_of's own product differ from each other by as little.  Hence the
 *              face is listed in a cell of the rectangle of the layer that holds that point.
 *   EXIT       after a layer the walk stops when the best t so far is STRICTLY below t_far - (2 tol |Sz| + 1e-12 |t_far|), t_far =
 *              (z - o[kz]) Sz of the layer's far plane z as it stands, unwidened: a face not yet tested hits, if at all, at or beyond
 *              that plane up to the same roundings, so its t can neither be smaller nor tie.  (A far plane taken from the widened
 *              interval with a single tol rounds to a tiny positive t for a plane through the origin, and stops one layer early on a
 *              tie at t = -0.0 whose lower face number sits in the next layer.)
 *   FAR ORIGINS  an origin 1e15 box sizes away makes tol exceed the box: every layer visits all its cells.  Slow, and correct.
 * Host waits: the mesh check, the box of the vertices, one per count of the index's entries (1 + its halvings).  Knob "raycast_stats"
 * (pb3d_set_tuning; one more host wait) counts, for pb3d_cast_rays_last, {rays that hit, bad rays, rays that visit no cell (they miss
 * the box), face tests, cells visited, (cell, face) entries of the index}; PB3D_EINVAL if the context's last call was not counted.  Knob
 * "raycast_timing" (one more host wait) times the index build and the query with events for pb3d_cast_rays_last_ms; PB3D_EINVAL if the
 * last call was not timed.  Scratch: 72 bytes per face for the corners, 12 per cell and 4 per entry (at most 8 entries a face). */
int pb3d_cast_rays_resident(pb3d_ctx* ctx, const void* d_origins, const void* d_dirs, int rays_f64, int64_t nrays, const void* d_verts,
                            int verts_f64, int64_t nv, const void* d_faces, int faces_i64, int64_t nf, double t_min, double t_max, int any_hit,
                            double* d_t /* nrays */, int32_t* d_face /* nrays */, double* d_bary /* nrays*3, or NULL */,
                            uint8_t* d_hit /* nrays, any_hit only */);
int pb3d_cast_rays_last(const pb3d_ctx* ctx, int64_t stats[6]);
int pb3d_cast_rays_last_ms(const pb3d_ctx* ctx, double ms[2]);

/* ---- density volume of a point cloud, reference utils/eval_helpers.py:178-189 (pointcloud_to_voxel_grid) ---------------------------
 * d_out: grid_size^3 float32, bit for bit the reference's volume for the resident (n, 3) list d_pts (float32 rows, or float64 with
 * pts_f64 = 1; any 4- / 8-byte aligned base):
 *   norm = (p - min) / ((max - min).max() + 1e-8), its y column shifted so that the maximum is 0 (normalize_preserve_aspect), every
 *   operation rounded in the point dtype; voxel = trunc(norm * (grid_size - 1)), a negative index wrapping to the far planes as NumPy's
 *   does; the value of a voxel is (float)min(count, 2^24), where np.add.at on float32 stops growing.
 *   radius > 0: three passes of the Gaussian filter along axes 0, 1, 2 with the 2 * radius + 1 float64 `weights` (symmetric; the
 *   host builds them, radius = int(4 * sigma + 0.5)), float32 in and out of every pass, per output in float64
 *   tmp = in[l] * w[r]; for jj = -r .. -1: tmp += (in[l + jj] + in[l - jj]) * w[r + jj], reflect boundary, no FMA.  radius = 0: no
 *   filter, weights may be NULL.  Last, the six faces of the cube are 0 (grid_size <= 2: all of it).
 * 1 <= n <= 2^31 - 1, 1 <= grid_size <= 1024, 0 <= radius <= 64.  The coordinates must be finite: the entry computes the exact bounds
 * on the device, waits once for them and refuses bounds that are not finite.  Scratch: one volume of 4 * grid_size^3 bytes. */
int pb3d_density_grid_resident(pb3d_ctx* ctx, const void* d_pts, int pts_f64, int64_t n, int grid_size, const double* weights, int radius,
                               float* d_out);

/* ---- rigid ICP of two point clouds: the registration the inter-method metrics assume ("Align all reconstructions", reference
 * results/4.Inter-method_3D/README.md; its utils/preprocess_helpers.py is not shipped, so the arithmetic below is the specification) --
 * Point lists as for the metrics above: (n, 3) rows of float32 (*_f64 = 0) or float64 (1), at most 2^31 - 1 points, finite.  All
 * arithmetic is float64, every product and sum rounded on its own (no FMA); float32 is widened first.
 * transform_points: d_out (n x 3 float64) row i = T s_i for the row-major 3 x 4 T = [R | t]:
 *     p_h = ((T[h][0] * s.x + T[h][1] * s.y) + T[h][2] * s.z) + T[h][3].          n = 0 is fine (nothing written).
 * icp_index: bins the nt >= 1 target points into a cell index the context keeps (the index of knn above: exact box, cells, cell-sorted
 *   coordinates and ids) and, if bounds is not NULL, writes the target's exact box there (min 3, max 3; host memory).  One host wait.
 *   The index belongs to (d_tgt, nt, tgt_f64) and stays until the next icp_index call on the context; other calls do not disturb it.
 * icp_step: one point-to-point step against the index, enqueued without a host wait.  For every source point s
 *     p = T s (transform_points);   j = the target position with the smallest (d2, j), d2 = (dx*dx + dy*dy) + dz*dz, d = p - q_j
 *         (exactly knn with k = 1 on the transformed points: the lowest position wins a tie);
 *     the pair is USED when max_dist2 < 0 (no gate) or d2 <= max_dist2 (the caller forms max_dist * max_dist once);
 *     a used pair contributes 1 to the count and the 16 terms  P = p - cp (3),  Q = q_j - cq (3),  P_a * Q_b for a, b row-major (9),
 *     d2 (1);  an unused pair contributes 0 and +0.0 sixteen times.
 *   d_out (17 x 8 bytes on the device): the int64 count, then the 16 float64 sums.  Summation order, a function of (ns, i) alone:
 *     point i is lane i % 64 of wave (i / 64) % 4 of workgroup i / 256 (lanes past ns hold +0.0).  A wave adds by the butterfly
 *     v += v[lane ^ off] for off = 32, 16, 8, 4, 2, 1; a workgroup's sum is ((w0 + w1) + w2) + w3 of its wave sums: one partial row
 *     per workgroup.  Then one 256-thread workgroup: thread t starts from +0.0 and adds partial rows t, t + 256, t + 512, ... in
 *     ascending order, and the 256 values are reduced the same way.  No floating-point atomics; two calls on the same input give
 *     the same bytes.
 *   ns = 0: count 0 and sixteen +0.0 (no index needed).  nt = 0 with ns > 0 is PB3D_EINVAL.  A step whose (d_tgt, nt, tgt_f64) is not
 *   what the context's index was built for, or that finds no index, is PB3D_EINVAL: it never rebuilds silently.  A transformed point
 *   that is not finite has no nearest point and is not used. */
int pb3d_transform_points_resident(pb3d_ctx* ctx, const void* d_src, int src_f64, int64_t n, const double T[12], double* d_out);
int pb3d_icp_index_resident(pb3d_ctx* ctx, const void* d_tgt, int tgt_f64, int64_t nt, double bounds[6]);
int pb3d_icp_step_resident(pb3d_ctx* ctx, const void* d_src, int src_f64, int64_t ns, const void* d_tgt, int tgt_f64, int64_t nt,
                           const double T[12], double max_dist2, const double cp[3], const double cq[3], void* d_out);

/* ---- exact k-th smallest of a resident float64 list, and the trimmed ICP step built on it -----------------------------------------
 * kth_smallest: *d_out (one float64 on the device) = the element at 0-based position `rank` of the n values of d_vals (8-byte aligned)
 *   sorted by IEEE totalOrder, i.e. by the unsigned key  key = bits ^ (bits >> 63 ? ~0ull : 1ull << 63):
 *     negatives < -0.0 < +0.0 < positives < +inf < NaNs with a clear sign bit   (NaNs with the sign bit set sort below -inf).
 *   The result has the exact bytes of an input element.  1 <= n <= 2^31 - 1 and 0 <= rank < n, else PB3D_EINVAL.  Enqueued without a
 *   host wait.  A radix selection over the keys with integer counters only: two calls on the same input give the same bytes.
 * icp_step_trimmed: pb3d_icp_step_resident with an order statistic between the search and the sums.  Everything stated there holds
 *   unchanged (the index and its refusals, p = T s, j, d2, no FMA, the summation order, no host wait).  trim_fraction rho must be
 *   finite with 0 < rho <= 1, else PB3D_EINVAL.  On top of that:
 *     a pair is a CANDIDATE when p is finite (so j is valid) and (max_dist2 < 0 or d2 <= max_dist2);  m = the number of candidates.
 *       (The search pairs a p with an infinite coordinate at d2 = +inf, which icp_step leaves to its gate; here it is no candidate.)
 *     k = (rho >= 1.0) ? m : min(m, (int64)ceil(rho * (double)m))    -- one rounded float64 product, then ceil; on the device from m;
 *     tau = the k-th smallest candidate d2 (rank k - 1 of kth_smallest; a pair that is no candidate enters the selection as the quiet
 *       NaN 0x7FF8000000000000, which sorts above every candidate, +inf included);  m = 0: tau = +0.0;
 *     a pair is USED when it is a candidate and d2 <= tau: every pair tied at tau is used, so count >= k (no tie-break by index);
 *     a used pair contributes 1 to the count, the 16 terms of icp_step and a 17th, (P0*P0 + P1*P1) + P2*P2 with P = p - cp; any other
 *     pair contributes 0 and +0.0 seventeen times.  Rows of 17 sums, reduced in the order stated for icp_step.
 *   d_out (20 x 8 bytes on the device): the int64 count, the 17 float64 sums, the int64 m, the float64 tau.
 *   ns = 0: twenty zero words (no index needed).  nt = 0 with ns > 0 is PB3D_EINVAL.
 *   With rho = 1 the count, m and the first 16 sums are the bytes of pb3d_icp_step_resident on the same input, and tau is the largest
 *   candidate d2. */
int pb3d_kth_smallest_resident(pb3d_ctx* ctx, const double* d_vals, int64_t n, int64_t rank, double* d_out);
int pb3d_icp_step_trimmed_resident(pb3d_ctx* ctx, const void* d_src, int src_f64, int64_t ns, const void* d_tgt, int tgt_f64, int64_t nt,
                                   const double T[12], double max_dist2, double trim_fraction, const double cp[3], const double cq[3],
                                   void* d_out /* 20 x 8 bytes */);

/* ---- point-cloud normals and the point-to-plane ICP step built on them ----------------------------------------------------------------
 * point_normals: d_normals (n x 3 float64) = one unit normal per point of the resident (n, 3) list d_pts (float32, or float64 with
 *   pts_f64 = 1; finite), from d_idx, the n x k int32 rows of pb3d_knn_dev on (pts, pts, k) with 3 <= k <= PB3D_KNN_MAX_K and n >= k.  An
 *   index outside [0, n) is PB3D_EINDEX, checked on the device before any gather (one host wait), as surface_metrics checks its rows.
 *   One lane per point, float64 after widening; every product, sum, division and square root below is ONE correctly rounded
 *   operation -- no FMA and, unlike the roughness of surface_metrics, no double-double.  With x_j the row's points in row order:
 *     mean        m_a = (((0 + x_0a) + x_1a) + ... + x_(k-1)a) / k;
 *     covariance  y_j = x_j - m;  C_ab = (((0 + y_0a*y_0b) + y_1a*y_1b) + ...) for the six entries a <= b, no divisor;
 *     Jacobi      the cyclic 3 x 3 solve of the roughness path as it stands (one text, csrc/jacobi3.h): V = I; up to 8 sweeps over
 *                 the pairs (p, q) = (0, 1), (0, 2), (1, 2); a pair with C_pq == 0 is skipped; it is rotated when
 *                 |C_pq| > 2^-70 * sqrt(|C_pp * C_qq|) and set to zero either way; for a rotation
 *                 tau = (C_qq - C_pp) / (2 * C_pq), t = copysign(1, tau) / (|tau| + sqrt(1 + tau*tau)), c = 1 / sqrt(1 + t*t), s = t*c,
 *                 C_pp -= t*C_pq, C_qq += t*C_pq, (C_rp, C_rq) = (c*C_rp - s*C_rq, s*C_rp + c*C_rq), and the same for columns p, q of
 *                 every row of V; a sweep without a rotation is the last;
 *     normal      the column of V whose diagonal entry of C is smallest, the lowest column on a tie, each component divided by
 *                 sqrt((n0*n0 + n1*n1) + n2*n2);
 *     sign        viewpoint NULL: negated when its component of largest magnitude (the lowest on a tie) is negative;
 *                 viewpoint v (3 finite doubles, host): negated when ((v0-x0)*n0 + (v1-x1)*n1) + (v2-x2)*n2 < 0, x the point itself.
 *   k coincident neighbours (zero covariance) give (1, 0, 0) before the sign rule.  n = 0 is fine (nothing written).
 * icp_step_plane: one point-to-plane step against the index of icp_index and d_tgt_normals (nt x 3 float64 on the device, row j the
 *   normal of target point j; finite).  Word for word pb3d_icp_step_resident and pb3d_icp_step_trimmed_resident: the index and its
 *   refusals, p = T s, j and d2, the gate, the candidate, k and tau rules, the summation order, no host wait.  trim_fraction < 0:
 *   untrimmed -- no selection runs, a pair is used as icp_step uses it, and the m and tau words are 0; otherwise it must be in (0, 1]
 *   and a pair is used as icp_step_trimmed uses it.  0 and NaN are PB3D_EINVAL.  One pivot c serves as cp.
 *     A used pair contributes 1 to the count and 29 terms.  With n = row j of the normals, (dx, dy, dz) = p - q_j (the differences
 *     that form d2) and P = p - c:
 *       r  = (dx*n0 + dy*n1) + dz*n2
 *       a0 = P1*n2 - P2*n1,  a1 = P2*n0 - P0*n2,  a2 = P0*n1 - P1*n0;     J = (a0, a1, a2, n0, n1, n2)
 *       terms 0-20: J_u * J_v for u <= v, the upper triangle row-major (00 01 .. 05 11 12 .. 55);  terms 21-26: J_u * r;
 *       term 27: r * r;  term 28: d2.
 *     Any other pair contributes 0 and +0.0 twenty-nine times.  Rows of 29 sums, reduced in the order stated for icp_step.
 *   d_out (32 x 8 bytes on the device): the int64 count, the 29 float64 sums, the int64 m, the float64 tau.  ns = 0: thirty-two zero
 *   words (no index, no normals needed).  Every term is even in n, so negating any or all target normals leaves all 32 words
 *   unchanged: the step does not care how the normals are oriented.  The host solves the 6 x 6 system (A x = -g with A from terms
 *   0-20, g from 21-26, x = (rotation vector, translation) about c). */
int pb3d_point_normals_resident(pb3d_ctx* ctx, const void* d_pts, int pts_f64, int64_t n, const int32_t* d_idx, int k,
                                const double* viewpoint /* 3 doubles or NULL */, double* d_normals /* n x 3 float64 */);
int pb3d_icp_step_plane_resident(pb3d_ctx* ctx, const void* d_src, int src_f64, int64_t ns, const void* d_tgt, int tgt_f64, int64_t nt,
                                 const double* d_tgt_normals /* nt x 3 float64 */, const double T[12], double max_dist2,
                                 double trim_fraction, const double c[3], void* d_out /* 32 x 8 bytes */);

/* ---- facade plane, box crop and the pieces of the four-way completion: steps 2-4 of the inter-method preprocessing (reference
 * results/4.Inter-method_3D/README.md; its utils/preprocess_helpers.py is not shipped, so the arithmetic below is the specification) --
 * Point lists as for ICP: (n, 3) rows of float32 (*_f64 = 0) or float64 (1), n <= 2^31 - 1.  All arithmetic is float64 after widening,
 * every product and sum rounded on its own (no FMA).  Every entry is enqueued without a host wait.
 * The RESIDUAL of a point p = (x, y, z) to a plane row (a, b, c, d) is r = ((a * x + b * y) + c * z) + d; p is an INLIER when
 * fabs(r) <= tau.  A NaN residual (a NaN row, a NaN coordinate) is never an inlier.  tau >= 0 and not NaN, else PB3D_EINVAL.
 * plane_hypotheses: d_planes (K x 4 float64 on the device, 1 <= K <= 4096) row k from the points a, b, c at positions
 *   d_triplets[3k .. 3k + 2] (int64 on the device):
 *     u = b - a, v = c - a;   w = (u.y*v.z - u.z*v.y, u.z*v.x - u.x*v.z, u.x*v.y - u.y*v.x);   L = sqrt((w.x*w.x + w.y*w.y) + w.z*w.z);
 *     nrm = w / L (three divisions);   d = -((nrm.x*a.x + nrm.y*a.y) + nrm.z*a.z);   row = (nrm.x, nrm.y, nrm.z, d).
 *   A row whose L is not a finite number above 0 (a repeated index, an exactly collinear triplet, an overflow) is four NaNs; so is a
 *   row with an index outside [0, n), and nothing is gathered through such an index.
 * plane_score: d_counts[k] (K int64 on the device, overwritten) = the number of inliers of row k of d_planes among the n points.  The
 *   points are read once for all K planes; the counts are exact integers (integer atomics) and a function of the input alone.
 *   n = 0: zeros.  1 <= K <= 4096.
 * plane_moments: d_out (12 x 8 bytes on the device) = the int64 count of the inliers of `plane` (host, 4 values), then 11 float64 sums
 *   over the inliers:  P = p - pivot (3);  P.x*P.x, P.x*P.y, P.x*P.z, P.y*P.y, P.y*P.z, P.z*P.z (6);  r (1);  r*r (1).  A point that is
 *   not an inlier contributes 0 and +0.0 eleven times.  The summation order is the one stated for pb3d_icp_step_resident with n for
 *   ns (point i is lane i % 64 of wave (i / 64) % 4 of workgroup i / 256; butterfly; ((w0 + w1) + w2) + w3; the one-workgroup pass over
 *   the partial rows).  No floating-point atomics; two calls on the same input give the same bytes.  n = 0: count 0 and eleven +0.0.
 * points_crop_box: order-keeping compaction.  Row i survives when lo[a] <= p[a] <= hi[a] on all three axes (the point widened, the box
 *   closed, lo / hi on the host; a NaN coordinate fails).  The surviving rows are copied byte for byte, in the input's dtype and order,
 *   to the front of d_out (capacity n rows; rows past the count are not written), their positions in the input go to d_idx (int32;
 *   may be NULL) and the count to d_count (one int64 on the device).  n = 0: count 0. */
int pb3d_plane_hypotheses_resident(pb3d_ctx* ctx, const void* d_pts, int pts_f64, int64_t n, const int64_t* d_triplets, int K, double* d_planes);
int pb3d_plane_score_resident(pb3d_ctx* ctx, const void* d_pts, int pts_f64, int64_t n, const double* d_planes, int K, double tau,
                              int64_t* d_counts);
int pb3d_plane_moments_resident(pb3d_ctx* ctx, const void* d_pts, int pts_f64, int64_t n, const double plane[4], double tau,
                                const double pivot[3], void* d_out);
int pb3d_points_crop_box_resident(pb3d_ctx* ctx, const void* d_pts, int pts_f64, int64_t n, const double lo[3], const double hi[3], void* d_out,
                                  int32_t* d_idx, int64_t* d_count);

/* ---- cluster_points: exact DBSCAN of a point cloud, the segmentation step of the same preprocessing (csrc/cluster.hip) ----------------
 * Point lists as above: (n, 3) rows of float32 (pts_f64 = 0, widened first) or float64 (1), 0 <= n <= 2^31 - 1, coordinates finite
 * (the caller's duty).  eps finite and > 0, min_samples >= 1, else PB3D_EINVAL.  The result is scikit-learn's
 * DBSCAN(eps, min_samples).labels_ / core_sample_indices_ to the bit, and a function of the input alone:
 *   NEIGHBOUR  q is a neighbour of p iff d2 = (dx*dx + dy*dy) + dz*dz <= eps2, with dx = p.x - q.x and so on in float64, every product
 *              and sum rounded on its own (no FMA), and eps2 = eps * eps one rounded product made once on the host.  d2 has the same
 *              bits with p and q exchanged; a point is its own neighbour (d2 = 0).
 *   COUNTS     counts[p] = the number of neighbours of p, itself included: an exact integer (radius outlier removal is counts >= m).
 *   CORE       core[p] = counts[p] >= min_samples.
 *   CLUSTERS   the connected components of the neighbour graph restricted to core points.  The ROOT of a cluster is its smallest core
 *              position in the caller's list; clusters are numbered 0, 1, ... by increasing root.
 *   BORDER     a non-core point with at least one core neighbour takes the smallest label among its core neighbours.
 *   NOISE      a non-core point with no core neighbour: label -1.
 *   SIZES      sizes[c] = the number of points, core and border, labelled c.
 * radius_count: d_counts (n uint32 on the device) = COUNTS.  One host wait (the cloud's bounding box, for the cell index).
 * cluster_points: d_labels (n int32), d_core (n bytes, 0 / 1), d_counts (n uint32) and d_sizes (int64, capacity n entries; the first
 *   *nclusters are written) on the device, *nclusters on the host.  Two host waits: the bounding box and the number of clusters.
 *   n = 0: *nclusters = 0, nothing written.
 * labels_member: d_keep[i] (n bytes on the device) = 1 when 0 <= d_labels[i] < nlabels and chosen[d_labels[i]] != 0 (chosen: nlabels
 *   bytes on the host, staged: it may be reused on return), else 0.  No host wait.
 * points_select: pb3d_points_crop_box_resident with the predicate d_keep[i] != 0 (n bytes on the device) in the box's place: the
 *   surviving rows byte for byte in the input's dtype and order at the front of d_out (capacity n rows), their positions in d_idx
 *   (int32, may be NULL), the count in d_count (one int64 on the device).  No host wait.
 * cluster_last: the cells per axis of the index of the last radius_count / cluster_points on this context and, with pass_ms not NULL,
 *   the milliseconds its passes took (index, count, union + flatten, ranks, labels) -- recorded only under the development knob
 *   "cluster_timing" (pb3d_set_tuning; one more host wait), else PB3D_EINVAL.  Knob "cluster_cell" picks the index's cell edge
 *   (0: the built-in rule, 1: two points per cell, 2: above eps); no result depends on either knob. */
int pb3d_radius_count_resident(pb3d_ctx* ctx, const void* d_pts, int pts_f64, int64_t n, double eps, uint32_t* d_counts);
int pb3d_cluster_points_resident(pb3d_ctx* ctx, const void* d_pts, int pts_f64, int64_t n, double eps, int64_t min_samples, int32_t* d_labels,
                                 uint8_t* d_core, uint32_t* d_counts, int64_t* d_sizes, int64_t* nclusters);
int pb3d_labels_member_resident(pb3d_ctx* ctx, const int32_t* d_labels, int64_t n, const uint8_t* chosen, int64_t nlabels, uint8_t* d_keep);
int pb3d_points_select_resident(pb3d_ctx* ctx, const void* d_pts, int pts_f64, int64_t n, const uint8_t* d_keep, void* d_out, int32_t* d_idx,
                                int64_t* d_count);
int pb3d_cluster_last(pb3d_ctx* ctx, int64_t cells[3], double pass_ms[5] /* or NULL */);

/* ---- voxel_downsample: voxel-grid downsampling of a point cloud, between segmentation and registration (csrc/downsample.hip) ----------
 * Point lists as above: (n, 3) rows of float32 (pts_f64 = 0, widened first) or float64 (1), 0 <= n <= 2^31 - 1, coordinates finite
 * (the caller's duty).  voxel_size finite and > 0, origin NULL or three finite values, reduce one of the two below, else PB3D_EINVAL.
 * The result is a function of the input and its order alone (two runs give the same bytes):
 *   ORIGIN    the caller's three float64 values when given.  Otherwise o_a = lo_a - h with lo the cloud's exact per-axis minimum and
 *             h = 0.5 * voxel_size: one rounded product made once on the host, one rounded subtraction per axis.  With this default the
 *             voxel membership is Open3D's voxel_down_sample.
 *   CELL      c_a = floor((p_a - o_a) / voxel_size) in float64: one rounded subtraction, one correctly rounded division, then floor.  A
 *             point just below a voxel face whose quotient rounds up to the integer belongs to the upper voxel, as it does in NumPy.
 *   RANGE     every point must have 0 <= c_a < 2^21 on every axis.  The three operations are monotone, so the host decides this from
 *             the cells of the exact bounds; on failure PB3D_EINVAL with a message that names voxel_size and origin, nothing written.
 *   VOXELS    two points share a voxel iff their three cells are equal.  Voxels are numbered 0 .. m - 1 by the position of their first
 *             point in the caller's list: in order of first appearance.
 *   INDEX     index[v] = that first position (strictly increasing); inverse[i] = the voxel of point i; counts[v] = its number of points.
 *   CENTROID  (reduce = PB3D_DOWNSAMPLE_CENTROID) per axis s = 0.0, then s = s + (double)p_a over the voxel's points in ascending
 *             position, one rounded addition each (no FMA); out = s / (double)counts[v], one correctly rounded division; for a float32
 *             cloud that quotient rounded once to float32.
 *   FIRST     (reduce = PB3D_DOWNSAMPLE_FIRST) out[v] = row index[v] of the input, byte for byte.
 * Permuting the input may change the numbering of the voxels and the last bits of the centroids (the order of the additions), never the
 * partition into voxels.
 * d_out (capacity n rows of the input's dtype), d_index (n int32) and, where not NULL, d_counts (n uint32): the first *nvoxels entries
 * are written; d_inverse (n int32, or NULL) whole; *nvoxels on the host.  Two host waits: the bounding box and the number of voxels.
 * n = 0: *nvoxels = 0, nothing written, no host wait.  A non-finite coordinate (which the Python forms refuse) gives a wrong voxel for
 * that point, never an access outside the buffers. */
#define PB3D_DOWNSAMPLE_CENTROID 0
#define PB3D_DOWNSAMPLE_FIRST 1
int pb3d_voxel_downsample_resident(pb3d_ctx* ctx, const void* d_pts, int pts_f64, int64_t n, double voxel_size,
                                   const double origin[3] /* or NULL */, int reduce, void* d_out, int32_t* d_index,
                                   int32_t* d_inverse /* or NULL */, uint32_t* d_counts /* or NULL */, int64_t* nvoxels);

/* ---- notebook 2: bbox camera init and projection overlays, reference utils/camera_estimation.py:56-108, :346-477 ----------------
 * grid_bounds: d_out[0] = the number of voxels of the resident (A0,A1,A2,C) grid whose colour (C = 3) / label (C = 1) is one of the
 *   ncolors <= 31 non-zero `colors` (ncolors = 0: any non-zero voxel), d_out[1..3] = their inclusive minimum (a0, a1, a2), d_out[4..6]
 *   the maximum (7 int64 on the device; count 0 leaves INT64_MAX / -1).  One read of the grid; replaces
 *   get_voxel_points_by_parts(...)[0].min / max(axis=0) of :61-66 (x = a2, y = a1, z = a0) without building the point list.
 * grid_hit_bits: d_bits (Himg x Wimg uint32, cleared first) bit k = some voxel of colors[k] projects onto the pixel with the
 *   arithmetic of project_colored_voxels (utils/projection_utils.py:5-23: Z < 1e-8 clamped, no depth test; voxel (a0,a1,a2) is the
 *   float32 point (a2,a1,a0); R, cam, prec as for pb3d_project_dev).  That is all(proj == colour) of a projection of the part alone
 *   (:387-395), for up to 31 parts in one sweep of the grid.
 * overlay_compose: the images of visualize_voxel_projection_iou from d_bits (nplanes = ceil(nparts / 31) bit images one after the
 *   other; part j is bit j % 31 of plane j / 31), the resident d_image (Himg,Wimg,3) and the parts' RGB `colors` (nparts <= 248).
 *   PB3D_OVERLAY_PART_ON_WHOLE (:394-419): d_vis = nparts images; image j is (0.7 * proj + 0.3 * image).astype(uint8) in float64 with
 *     proj = colour j where bit j is set, then (255,255,0) on binary_dilation(gt & prj) & ~(gt & prj), gt = all(image == colour j)
 *     (the 4-neighbour cross, outside = false); d_counts[2j] = #(gt & prj), d_counts[2j+1] = #(gt | prj).
 *   PB3D_OVERLAY_WHOLE_ON_WHOLE (:433-452): one image, gt = any(image != bg), prj = any bit (or d_extra_prj[px] != 0, an optional
 *     Himg x Wimg uint8 mask of parts projected elsewhere): green gt only, red prj only, yellow both; d_counts[0..1].
 *   PB3D_OVERLAY_WHOLE_ON_WHOLE_COLOR (:462-466): one image, per channel the sum of the colours of the parts whose bit is set,
 *     clipped at 255, blended with the image as above; no counts. */
#define PB3D_OVERLAY_PART_ON_WHOLE 0
#define PB3D_OVERLAY_WHOLE_ON_WHOLE 1
#define PB3D_OVERLAY_WHOLE_ON_WHOLE_COLOR 2
int pb3d_grid_bounds_resident(pb3d_ctx* ctx, const uint8_t* d_grid, int64_t A0, int64_t A1, int64_t A2, int C, const uint8_t* colors, int ncolors,
                         int64_t* d_out);
int pb3d_grid_hit_bits_resident(pb3d_ctx* ctx, const uint8_t* d_grid, int64_t A0, int64_t A1, int64_t A2, int C, const uint8_t* colors,
                           int ncolors, const double R[9], const double cam[3], double f, double cx, double cy, const int prec[4], int Himg,
                           int Wimg, uint32_t* d_bits);
int pb3d_overlay_compose_resident(pb3d_ctx* ctx, const uint32_t* d_bits, int nplanes, const uint8_t* d_image, int Himg, int Wimg,
                             const uint8_t* colors, int nparts, const uint8_t bg[3], const uint8_t* d_extra_prj, int mode, uint8_t* d_vis,
                             int64_t* d_counts);

/* ---- perspective carve: silhouette carving of a resident grid by pinhole views -------------------------------------------------
 * The reference carves by orthographic views only; this applies the pinhole arithmetic of project_colored_voxels (reference
 * utils/projection_utils.py:5-23) to the cameras notebook 2 fits.  Voxel (a0,a1,a2) of the uint8 (A0,A1,A2,C) grid, C = 3 (RGB) or 1
 * (labels), is the float32 point (x = a2, y = a1, z = a0), occupied where any channel is non-zero.  A voxel is SUBJECT when it is
 * occupied and, for ncolors > 0, its colour / label is one of the ncolors <= 31 non-zero `colors`; every other voxel is copied.
 * For a subject voxel and a view the pixel (u, v) is exactly the one project_colored_voxels paints: (p - cam) @ R.T in the float
 * width prec[0] names, Z < 1e-8 clamped to 1e-8, u = (X/Z)*f + cx, v = -(Y/Z)*f + cy with the per-stage widths prec[1..3], rint
 * (half to even), then 0 <= u < Wimg, 0 <= v < Himg (R, cam, prec as for pb3d_project_dev: the host's look_at_rotation and the
 * NumPy promotion flags of float32 points).  The view REJECTS the voxel when the pixel is inside the image and the mask is clear
 * there; a pixel outside the image (NaN included) rejects it too, or accepts it with outside_keep != 0.  d_maskbits: Himg rows of
 * (Wimg + 31) / 32 uint32 words on the device, pixel u of a row is bit u & 31 of word u >> 5.
 * Views apply in order: the first view that rejects a voxel zeroes all its channels and later views are not evaluated for it;
 * d_removed[k] (nviews int64 on the device, zeroed by the entry, may be NULL) counts the voxels view k zeroed.  Hence carving by
 * [a, b] is carving by [a], then its result by [b], with the counts side by side, and carving twice is carving once.
 * d_out != d_grid: every voxel is written (the buffers may not overlap); d_out == d_grid: in place, only zeroed voxels are written.
 * Any base address: rows of whole dwords on 4-byte aligned buffers move as dwords, everything else byte by byte.  Eight views go
 * into one launch; further views carve d_out in place.  nviews = 0 copies.  Axes up to 2^24.  Refused before any device work (and
 * before the context is looked at): C other than 1 or 3, a negative shape, a null grid of a non-empty shape, ncolors > 31 or a black
 * colour, nviews < 0 or a null table, Himg or Wimg <= 0, a null mask, prec flags other than 0 / 1 or narrowing. */
typedef struct pb3d_carve_view {
    double R[9], cam[3], f, cx, cy;
    int prec[4];
    int Himg, Wimg;
    const uint32_t* d_maskbits;
} pb3d_carve_view;
int pb3d_perspective_carve_resident(pb3d_ctx* ctx, const uint8_t* d_grid, int64_t A0, int64_t A1, int64_t A2, int C, const uint8_t* colors,
                                    int ncolors, const pb3d_carve_view* views, int nviews, int outside_keep, uint8_t* d_out,
                                    int64_t* d_removed);

/* ---- perspective paint: the visible voxels of a resident grid take the colours of the pixels the views see them at -------------
 * The perspective counterpart of apply_colored_mask_to_voxel_grid, on the grid conventions of the perspective carve above: voxel
 * (a0,a1,a2) of the uint8 (A0,A1,A2,C) grid is the float32 point (x = a2, y = a1, z = a0), occupied where any channel is non-zero,
 * SUBJECT when it is occupied and, for ncolors > 0, of one of the ncolors <= 31 non-zero `colors`; every other voxel is copied.
 * View k holds a camera (R, cam, f, cx, cy, prec as for pb3d_grid_visible_bits_dev), an image d_image of Himg x Wimg x C bytes (RGB
 * for C = 3, labels for C = 1; any base address) and a z-buffer d_zbuf of Himg x Wimg float32, normally pb3d_grid_depth_buffer_dev
 * of the grid BEFORE painting under the same camera (compute_global_depth_buffer, reference utils/eval_helpers_intra.py:134-160).
 * View k SEES a subject voxel when the arithmetic of that z-buffer accepts its point (Z > 1e-6 and the rounded pixel (u, v) inside
 * the image) and |Z - d_zbuf[v,u]| < eps as project_part_visible (:168-190) evaluates it: in float64 for a float64 camera, else on
 * the float32 difference, compared in float32 when eps_f32 != 0 (eps a weak Python float) and in float64 otherwise.
 * View k PAINTS the voxel when it sees it and d_image[v,u] is neither black / label 0 nor one of the nskip <= 8 `skip` colours /
 * labels (nskip * C bytes; black never paints whether listed or not: it would delete the voxel).
 * The views are tried in order; the first that paints a voxel decides its colour, a voxel no view paints keeps its own.
 * d_painted[k] (nviews int64 on the device, zeroed by the entry, may be NULL) counts the voxels whose colour view k decided, whether
 * or not the value changed.  Painting never changes occupancy, so z-buffers made from the input grid do not depend on the order of
 * the views and the result is the same in place and out of place.
 * d_out != d_grid: every voxel is written (the buffers may not overlap); d_out == d_grid: in place, only decided voxels are written.
 * Any base address: rows of whole dwords on 4-byte aligned buffers move as dwords, everything else byte by byte.  nviews = 0 copies.
 * Axes up to 2^24.  Refused before any device work (and before the context is looked at): C other than 1 or 3, a negative shape, a
 * null grid of a non-empty shape, ncolors > 31 or a black colour, nviews outside 0..8 or a null table, nskip outside 0..8 or a null
 * table, eps_f32 other than 0 / 1, Himg or Wimg <= 0, a null image or z-buffer, prec flags other than 0 / 1 or narrowing, a null
 * output, an output that overlaps the grid in part. */
typedef struct pb3d_paint_view {
    double R[9], cam[3], f, cx, cy;
    int prec[4];
    int Himg, Wimg;
    const uint8_t* d_image;
    const float* d_zbuf;
} pb3d_paint_view;
int pb3d_perspective_paint_resident(pb3d_ctx* ctx, const uint8_t* d_grid, int64_t A0, int64_t A1, int64_t A2, int C, const uint8_t* colors,
                                    int ncolors, const pb3d_paint_view* views, int nviews, const uint8_t* skip, int nskip, double eps,
                                    int eps_f32, uint8_t* d_out, int64_t* d_painted);

/* ---- compute_partwise_iou, reference utils/camera_estimation.py:770-787 -------------------
 * per colour k: inter[k] = #(a==c & b==c), uni[k] = #(a==c | b==c) over npix RGB pixels. */
int pb3d_partwise_iou_dev(pb3d_ctx* ctx, const uint8_t* d_a, const uint8_t* d_b, int64_t npix,
                          const uint8_t* colors, int ncolors, int64_t* inter, int64_t* uni);
int pb3d_partwise_iou(pb3d_ctx* ctx, const uint8_t* a, const uint8_t* b, int64_t npix,
                      const uint8_t* colors, int ncolors, int64_t* inter, int64_t* uni);

/* ---- K cameras per launch (row N4): the objective of the camera aligner, reference utils/camera_estimation.py:597-603
 * (`evaluate` = project_colored_voxels + compute_partwise_iou), as the random / coordinate / Powell loops (:606-725) call it
 * hundreds of times on the same points.  For every camera k: inter[k*ncolors + c], uni[k*ncolors + c] are the counts
 * pb3d_partwise_iou would return for pb3d_project's image of camera k against the (Himg,Wimg,3) part image d_seg.  The K
 * images are never materialised; one counter download per call.  pb3d_look_at_batch is the host half: K look-at rotations
 * (reference utils/camera_geometry.py:3-14) in the caller's float width; dot_mode says how this host's NumPy rounds the
 * 3-element dot product inside numpy.linalg.norm (0: separate multiplies and adds, 1: one FMA chain from the first product,
 * 2: exact products accumulated in double then rounded -- float32 only, 3: the FMA chain from the last product, 4: float32 products
 * accumulated in double -- float32 only, OpenBLAS's sdot tail loop); the Python shim calibrates it against NumPy itself. */
typedef struct pb3d_camera {
    double R[9], cam[3], f, cx, cy;
    int prec[4];
} pb3d_camera;
int pb3d_project_iou_batch_dev(pb3d_ctx* ctx, const void* d_pts, int pts_f64, const uint8_t* d_cols, int64_t n, const pb3d_camera* cams,
                               int ncams, int Himg, int Wimg, const uint8_t* d_seg, const uint8_t* colors, int ncolors, int64_t* inter,
                               int64_t* uni);
int pb3d_look_at_batch(const void* eye, const void* target, int is_f64, int64_t count, int dot_mode, double* R9);
/* K deform tuples per launch: the part-wise grid search of reference utils/deformation_estimation.py:148-258 (the slider loop
 * :100-146 / save_params :262-284 automated).  For tuple k = deforms5[5k .. 5k+4] = (scale_xz, scale_y, kx, ky, kz -- the scalars of
 * pb3d_deform_count): deform_coords of the part's points, the bounds filter against the (A0,A1,A2) grid, the float32 projection
 * with ONE fixed camera and the IoU of the part's colour against the (Himg,Wimg,3) image d_seg.  inter[k] / uni[k] are the counts
 * compute_partwise_iou forms; nvalid[k] counts the in-bounds (point, jitter) evaluations before np.unique (0 <=> upstream's
 * "No deformed voxels within bounds").  Every point of a part carries the part colour, so the projected image is the set of
 * pixels hit and neither np.unique nor the write order can change the counts.  A non-finite scalar in any tuple is refused
 * (PB3D_EINVAL, the message names the tuple and the scalar) before the outputs are written or anything is launched; see below.
 * With n == 0 the projection is empty: inter = nvalid = 0 and uni = the image's pixels of the colour. */
int pb3d_deform_iou_batch_dev(pb3d_ctx* ctx, const float* d_pts, int64_t n, const double* deforms5, int ntuples, int64_t A0, int64_t A1,
                              int64_t A2, const pb3d_camera* cam, int Himg, int Wimg, const uint8_t* d_seg, const uint8_t color[3],
                              int64_t* inter, int64_t* uni, int64_t* nvalid);

/* ---- part-wise deformation, reference utils/deformation_estimation.py:70-98 (deform_coords) -------
 * Seven jitters (0, +-0.25 per axis) of the part's points (voxel indices as float32), each centred on
 * its own mean, x/z scaled by sxz and pushed by kx/kz * sign, y scaled by sy and shifted by -ky (the
 * caller forms kx = shift_xz*W/W_img, ky = shift_y*H/H_img, kz = shift_xz*D/W_img as Python floats, :76-78),
 * rounded half-to-even; the result is np.unique(axis=0): unique rows in lexicographic (x,y,z) order as
 * int64.  count, then fill with a buffer of n_unique rows; a fill refuses (PB3D_EINVAL) if another call has
 * reused the state its count left on the context.  paint writes rgb at grid[z,y,x] of every
 * in-bounds deformed coordinate (:120-124, :306-309 for a uniformly coloured part); scatter_colors is the
 * general grid[z,y,x] = cols[k] assignment for unique rows.  A row outside the grid makes scatter_colors
 * return PB3D_EINVAL (NumPy would raise IndexError) after its launch: nothing outside the grid is written,
 * and each in-bounds row's voxel holds either its old bytes or cols[k].
 * Difference from the reference: a non-finite sxz, sy, kx, ky or kz is refused (PB3D_EINVAL, the message
 * names the scalar) by count, paint and the tuple batch before any launch; the outputs are untouched and a
 * pending count -> fill pair is dropped (its fill then asks for a new count).  Upstream, NumPy turns the NaN
 * into INT64_MIN rows that the bounds filter drops; the conversion is undefined in C++. */
int pb3d_deform_count_dev(pb3d_ctx* ctx, const float* d_pts, int64_t n, double sxz, double sy, double kx, double ky, double kz,
                          int64_t* n_unique);
int pb3d_deform_fill_dev(pb3d_ctx* ctx, int64_t n_unique, int64_t* d_coords);
int pb3d_deform_count(pb3d_ctx* ctx, const float* pts, int64_t n, double sxz, double sy, double kx, double ky, double kz,
                      int64_t* n_unique);
int pb3d_deform_fill(pb3d_ctx* ctx, int64_t n_unique, int64_t* coords);
int pb3d_deform_paint_dev(pb3d_ctx* ctx, const float* d_pts, int64_t n, double sxz, double sy, double kx, double ky, double kz,
                          int64_t A0, int64_t A1, int64_t A2, const uint8_t rgb[3], uint8_t* d_grid);
int pb3d_scatter_colors_dev(pb3d_ctx* ctx, const int64_t* d_coords, const uint8_t* d_cols, int64_t m, int64_t A0, int64_t A1,
                            int64_t A2, uint8_t* d_grid);

/* ---- connected components and the steps built on them (rows N1/N2) ---------------------------------
 * pb3d_label_color_dev: scipy.ndimage.label(all(grid == color, axis=-1)) with the default 6-connected
 * structure (call sites reference utils/voxel_carving_utils.py:175, :254): int32 labels 1..ncomp numbered in
 * raster order of each component's first voxel, 0 elsewhere.  pb3d_component_stats_dev: per component the
 * bounding box (lo inclusive, hi exclusive -- :184-185), voxel count and coordinate sums (for the means of
 * :259), returned in host arrays.  crop_occupancy / component_paste are the per-component steps of
 * left_right_guided_carve (:190-192, :197-201); recolor_components is :263-265; extrude is
 * extrude_from_surface (:213-248): out = grid with `depth` cells from the first occupied voxel along the
 * axis painted fill_color (NULL = zeros) where the 2-D mask allows (axis 2: valid[x*H+y]; axis 0:
 * valid[y*valid_w + z], the upstream indexing of its (H,W) mask). */
int pb3d_label_color_dev(pb3d_ctx* ctx, const uint8_t* d_grid_rgb, int64_t A0, int64_t A1, int64_t A2, const uint8_t color[3],
                         int32_t* d_labels, int64_t* ncomp);
/* label_color + component_stats in one pass and ONE host round trip: the statistics are gathered by the labelling's last kernel
 * (the labels are in registers there).  The host arrays hold `cap` components; *stats_valid = 0 when there are more (only *ncomp and
 * the labels are then valid: call pb3d_component_stats_dev). */
int pb3d_label_color_stats_dev(pb3d_ctx* ctx, const uint8_t* d_grid_rgb, int64_t A0, int64_t A1, int64_t A2, const uint8_t color[3],
                               int32_t* d_labels, int64_t* ncomp, int64_t cap, int members_only, int64_t* bbox_lo_hi, int64_t* count,
                               int64_t* coord_sum, int* stats_valid);
/* members_only = 1: the entries of d_labels at voxels that do NOT carry the colour are left UNSPECIFIED (the zeros are more than half of the
 * labelling's traffic).  Such a volume may only be consumed, before the next pb3d_label_* call on the context, by the entries that
 * consult the labelling's membership bits: pb3d_guided_carve[_label | _color]_dev and pb3d_recolor_last_labelled_dev (and by reading the
 * labels of voxels known to carry the colour).  members_only = 0: a full label volume (0 elsewhere), as pb3d_label_color_dev writes.
 * The bits stay valid until the next pb3d_label_* call on the context (calls that only grow OTHER scratch buffers, e.g.
 * pb3d_component_stats_dev, do not invalidate them). */
/* The components of SEVERAL colours in ONE labelling sequence (reference utils/voxel_carving_utils.py:338 calls :175 once per part colour
 * on a grid whose membership of the OTHER colours left_right_guided_carve never changes: it only clears or restores voxels of its own
 * colour, :199-201): the colour grid is read once, one forest serves every colour (a run = a maximal run of one colour).  colors =
 * ncolors x 3 bytes, pairwise different, 1 <= ncolors <= PB3D_CCL_MAX_COLORS.  ncomp[k], stats_valid[k] per colour; the statistics arrays
 * are [ncolors][cap][...]; labels are numbered PER COLOUR (as one scipy.ndimage.label call per colour numbers them), so the label of a
 * voxel means something only together with its colour: d_labels is for the consumers that take a colour index
 * (pb3d_guided_carve_color_dev) or, with ncolors == 1, for anyone. */
#define PB3D_CCL_MAX_COLORS 8
int pb3d_label_colors_stats_dev(pb3d_ctx* ctx, const uint8_t* d_grid_rgb, int64_t A0, int64_t A1, int64_t A2, const uint8_t* colors, int ncolors,
                                int32_t* d_labels, int64_t* ncomp, int64_t cap, int members_only, int64_t* bbox_lo_hi, int64_t* count,
                                int64_t* coord_sum, int* stats_valid);
int pb3d_component_stats_dev(pb3d_ctx* ctx, const int32_t* d_labels, int64_t A0, int64_t A1, int64_t A2, int64_t ncomp,
                             int64_t* bbox_lo_hi, int64_t* count, int64_t* coord_sum);
int pb3d_crop_occupancy_dev(pb3d_ctx* ctx, const uint8_t* d_grid_rgb, int64_t A0, int64_t A1, int64_t A2, const int64_t lo[3],
                            const int64_t hi[3], uint8_t* d_occ);
int pb3d_component_paste_dev(pb3d_ctx* ctx, const uint8_t* d_colored, const int32_t* d_labels, int32_t id, const uint8_t* d_carved_occ,
                             int64_t A0, int64_t A1, int64_t A2, const int64_t lo[3], const int64_t hi[3], uint8_t* d_carved);
/* The whole component loop of left_right_guided_carve (reference utils/voxel_carving_utils.py:178-201) in one call, IN PLACE on the
 * resident colour grid: for component k + 1 of d_labels with box bbox_lo_hi[6k..] (lo inclusive, hi exclusive) and crop mask
 * masks[mask_off[k] ..] ((Wc,Hc) uint8 truthiness, host memory, mask_bytes in all) the crop's occupancy goes through
 * process_voxel_grid(., crop mask, angle_interval) and the component's voxels that do not survive are cleared; carved_counts[k] (host)
 * = the log's "carved voxels" (:195).  One launch pair per batch of components (all 32-plane slices of all crops resident in LDS for
 * every rotation step).  *took = 0 (nothing done): a crop's slice does not fit the LDS -- run the per-component entries below.
 * The call returns after the device has finished (the counts are host values). */
int pb3d_guided_carve_dev(pb3d_ctx* ctx, uint8_t* d_grid_rgb, const int32_t* d_labels, int64_t W, int64_t H, int64_t D, int64_t ncomp,
                          const int64_t* bbox_lo_hi, const uint8_t* masks, const int64_t* mask_off, int64_t mask_bytes, int angle_interval,
                          int64_t* carved_counts, int* took);
/* ... for colour `color_index` of the last pb3d_label_colors_stats_dev / pb3d_label_values_stats_dev call on the context (d_labels is the
 * volume that call wrote; channels = 3: colour grid, 1: label volume).  PB3D_EINVAL when the labelling's membership bits are gone. */
int pb3d_guided_carve_color_dev(pb3d_ctx* ctx, uint8_t* d_grid, const int32_t* d_labels, int color_index, int channels, int64_t W, int64_t H,
                                int64_t D, int64_t ncomp, const int64_t* bbox_lo_hi, const uint8_t* masks, const int64_t* mask_off,
                                int64_t mask_bytes, int angle_interval, int64_t* carved_counts, int* took);
/* ... QUEUED: the call returns without waiting; the "carved voxels" counts are accumulated in d_counts (device memory, ncomp entries, cleared
 * by the call) and every host argument may be reused on return (they are staged through pb3d_h2d_async's ring).  partwise_carve
 * (reference :338-346) queues the component loops of all its parts behind ONE labelling and reads the counts once, at the end. */
int pb3d_guided_carve_queue_dev(pb3d_ctx* ctx, uint8_t* d_grid, const int32_t* d_labels, int color_index, int channels, int64_t W, int64_t H,
                                int64_t D, int64_t ncomp, const int64_t* bbox_lo_hi, const uint8_t* masks, const int64_t* mask_off,
                                int64_t mask_bytes, int angle_interval, int64_t* d_counts, int* took);
/* recolor_backward_components (reference utils/voxel_carving_utils.py:252-266) on a resident grid WITHOUT a host round trip: the
 * components of `color` are labelled (into d_labels, members only) with their statistics left on the device, the keep_k components with
 * the smallest mean coordinate on sort_axis are kept (float64 means as np.mean gives them; equal means keep their numbering order, as
 * the stable sorted() of :261 does), the others painted new_color -- all queued on the context's stream.  d_status (device, two int64,
 * may be NULL): [0] = number of components, [1] = 1 when the device could not decide (more than 2048 components: nothing was painted;
 * run pb3d_label_color_stats_dev + pb3d_recolor_last_labelled_dev instead).  channels = 3: colour grid; 1: label volume (color[0],
 * new_color[0] are label values). */
int pb3d_recolor_backward_dev(pb3d_ctx* ctx, uint8_t* d_grid, int64_t A0, int64_t A1, int64_t A2, const uint8_t color[3], const uint8_t new_color[3],
                              int keep_k, int sort_axis, int channels, int32_t* d_labels, int64_t* d_status);
/* The rest of the notebook-1 chain on the 1-byte LABEL form of a palette grid (row N3; label 0 = empty, the others index a palette):
 * the same kernels with one byte per voxel -- components of the voxels that carry `value`, the fused component loop, extrusion
 * (fill_label < 0: clear), recolouring and the output orientation.  Expanding a result with the palette gives the bytes of the RGB
 * entry (tests: label chain == RGB chain == the reference's stage digests). */
int pb3d_label_value_stats_dev(pb3d_ctx* ctx, const uint8_t* d_grid_lab, int64_t A0, int64_t A1, int64_t A2, uint8_t value, int32_t* d_labels,
                               int64_t* ncomp, int64_t cap, int members_only, int64_t* bbox_lo_hi, int64_t* count, int64_t* coord_sum,
                               int* stats_valid);
int pb3d_label_values_stats_dev(pb3d_ctx* ctx, const uint8_t* d_grid_lab, int64_t A0, int64_t A1, int64_t A2, const uint8_t* values, int nvalues,
                                int32_t* d_labels, int64_t* ncomp, int64_t cap, int members_only, int64_t* bbox_lo_hi, int64_t* count,
                                int64_t* coord_sum, int* stats_valid);
int pb3d_guided_carve_label_dev(pb3d_ctx* ctx, uint8_t* d_grid_lab, const int32_t* d_labels, int64_t W, int64_t H, int64_t D, int64_t ncomp,
                                const int64_t* bbox_lo_hi, const uint8_t* masks, const int64_t* mask_off, int64_t mask_bytes, int angle_interval,
                                int64_t* carved_counts, int* took);
/* the per-component steps (crops too large for the fused loop) on a label volume */
int pb3d_crop_occupancy_label_dev(pb3d_ctx* ctx, const uint8_t* d_grid_lab, int64_t A0, int64_t A1, int64_t A2, const int64_t lo[3],
                                  const int64_t hi[3], uint8_t* d_occ);
/* The labelling of pb3d_label_colors_stats_dev / pb3d_label_values_stats_dev (same contract, same outputs) at a chosen connectivity:
 * 6, 18 or 26 neighbours, the structures of scipy.ndimage.generate_binary_structure(3, 1 | 2 | 3); 26 is the structure=np.ones((3,3,3))
 * of extract_top_k_components (reference utils/voxel_utils.py:26).  channels = 3: d_grid is a colour grid and `colors` holds 3 bytes per
 * colour; 1: a label volume and `colors` holds label values.  The existing entries stay 6-connected. */
int pb3d_label_colors_conn_stats_dev(pb3d_ctx* ctx, const uint8_t* d_grid, int64_t A0, int64_t A1, int64_t A2, const uint8_t* colors, int ncolors,
                                     int channels, int connectivity, int32_t* d_labels, int64_t* ncomp, int64_t cap, int members_only,
                                     int64_t* bbox_lo_hi, int64_t* count, int64_t* coord_sum, int* stats_valid);
/* extract_top_k_components (reference utils/voxel_utils.py:24-33) in place on a resident grid WITHOUT a host round trip: the components of
 * `color` at `connectivity` (26 in the reference) are labelled into d_labels (members only) with their statistics left on the device,
 * ranked by height (ptp of their axis-1 coordinates; equal heights in label order, as the stable sorted() of :29), the first
 * min(k, n) (k >= 0) or max(n + k, 0) (k < 0) kept -- the [:k] of :29 -- and the other members zeroed (three zero bytes; label 0 when
 * channels = 1, where color[0] is the label value).  All queued on the context's stream.  d_status (device, two int64, may be NULL):
 * [0] = number of components, [1] = 1 when the device could not decide (more than 16384 components, or A1 > 8192: nothing was zeroed;
 * run pb3d_label_colors_conn_stats_dev + pb3d_component_stats_dev + pb3d_recolor_last_labelled_dev instead). */
int pb3d_top_k_components_dev(pb3d_ctx* ctx, uint8_t* d_grid, int64_t A0, int64_t A1, int64_t A2, const uint8_t color[3], int channels, int64_t k,
                              int connectivity, int32_t* d_labels, int64_t* d_status);
/* The members of up to PB3D_CCL_MAX_COLORS chosen components of a labelling just made on the context (pb3d_label_colors_conn_stats_dev
 * or any pb3d_label_*): what extract_minaret_voxels_by_label (reference utils/camera_estimation.py:176-216), extract_minaret_masks_by_label
 * (:247-325) and the keypoints of extract_top_bottom_voxel_points (:329-336) take from `labeled == cid`, without a pass over the grid per
 * component.  d_grid / channels as the labelling had them (3: colour grid; 1: label volume), d_labels the volume it wrote.  Selection k is
 * colour colors[k * channels ..], label labels[k] in THAT colour's numbering, box bbox_lo_hi[6k ..] (lo inclusive, hi exclusive, the
 * labelling's statistics; a box outside (A0, A1, A2) is PB3D_EINVAL); only its box is walked.  A voxel is a member when its grid bytes equal
 * the colour and its label equals labels[k]: the label is read only where the colour matches, so a members_only volume (unspecified
 * entries elsewhere) serves as well as a full one, and the labelling's membership bits are not consulted.  `outputs` ORs:
 *   PB3D_MEMBERS_COORDS  d_coords (device, int64): the members' (a0, a1, a2) in raster order -- np.argwhere(labeled == cid) order --
 *                        selection k in rows [counts[0] + .. + counts[k - 1], + counts[k]) (counts: host, the components' voxel counts);
 *                        at most counts[k] rows are written per selection;
 *   PB3D_MEMBERS_ROWS    d_rows (device, nsel x 8 int64, cleared by the call): {count, sum a0, sum a1, sum a2} of the members on the box's
 *                        bottom axis-1 row (lo[1]), then the same for its top row (hi[1] - 1);
 *   PB3D_MEMBERS_MASK    d_masks (device, nsel x A0*A1*A2 uint8, cleared by the call): 1 at the members, 0 elsewhere (the image form of a
 *                        (1, H, W) labelling is the (H, W) mask).
 * More than PB3D_CCL_MAX_COLORS selections, or a NULL buffer for a requested output, is PB3D_EINVAL.  Queued on the context's stream. */
#define PB3D_MEMBERS_COORDS 1
#define PB3D_MEMBERS_ROWS 2
#define PB3D_MEMBERS_MASK 4
int pb3d_component_members_dev(pb3d_ctx* ctx, const uint8_t* d_grid, int64_t A0, int64_t A1, int64_t A2, int channels, const int32_t* d_labels,
                               int nsel, const uint8_t* colors, const int32_t* labels, const int64_t* bbox_lo_hi, const int64_t* counts, int outputs,
                               int64_t* d_coords, int64_t* d_rows, uint8_t* d_masks);
int pb3d_component_paste_label_dev(pb3d_ctx* ctx, const uint8_t* d_grid_lab, const int32_t* d_labels, int32_t id, const uint8_t* d_carved_occ,
                                   int64_t A0, int64_t A1, int64_t A2, const int64_t lo[3], const int64_t hi[3], uint8_t* d_carved);
int pb3d_extrude_label_dev(pb3d_ctx* ctx, const uint8_t* d_grid_lab, int64_t W, int64_t H, int64_t D, const uint8_t* d_valid, int64_t valid_w,
                           int axis, int plus, int depth, int fill_label, uint8_t* d_out);
int pb3d_recolor_components_label_dev(pb3d_ctx* ctx, const int32_t* d_labels, int64_t nvox, const uint8_t* comp_flag, int64_t ncomp,
                                      uint8_t new_label, uint8_t* d_grid_lab);
int pb3d_orient_label_dev(pb3d_ctx* ctx, const uint8_t* d_grid_lab, int64_t W, int64_t H, int64_t D, uint8_t* d_out);
/* *d_count (a device int64 the caller has zeroed) += number of non-zero bytes of d_bytes[0..n): the "carved voxels" figure of
 * left_right_guided_carve's log (reference utils/voxel_carving_utils.py:197), without a host round trip per component. */
int pb3d_count_nonzero_dev(pb3d_ctx* ctx, const uint8_t* d_bytes, int64_t n, int64_t* d_count);
int pb3d_recolor_components_dev(pb3d_ctx* ctx, const int32_t* d_labels, int64_t nvox, const uint8_t* comp_flag, int64_t ncomp,
                                const uint8_t new_color[3], uint8_t* d_grid_rgb);
/* The same for the label volume the LAST pb3d_label_* call on this context wrote, untouched since (PB3D_EINVAL otherwise): the
 * labelling's 1-bit-per-voxel membership array is still on the device, so only the members' labels are read (9 MB of bits instead of
 * 292 MB of labels at 512 x 278 x 512).  channels = 3: d_grid is a colour grid; 1: a label volume and new_color[0] the new label. */
int pb3d_recolor_last_labelled_dev(pb3d_ctx* ctx, const int32_t* d_labels, int64_t nvox, const uint8_t* comp_flag, int64_t ncomp,
                                   const uint8_t new_color[3], uint8_t* d_grid, int channels);
/* d_out may be d_grid_rgb itself (in place: nothing but the painted cells is written). */
int pb3d_extrude_dev(pb3d_ctx* ctx, const uint8_t* d_grid_rgb, int64_t W, int64_t H, int64_t D, const uint8_t* d_valid, int64_t valid_w,
                     int axis, int plus, int depth, const uint8_t* fill_color, uint8_t* d_out);
/* notebook-1 output orientation, reference utils/voxel_carving_utils.py:384-385:
 * out (D,H,W,3) = flip(grid.transpose(2,1,0,3), axis=1) of the (W,H,D,3) grid, C-contiguous. */
int pb3d_orient_dev(pb3d_ctx* ctx, const uint8_t* d_grid_rgb, int64_t W, int64_t H, int64_t D, uint8_t* d_out);

/* ---- the 1-byte LABEL form of a semantic grid (row N3: what sits either side of the path) -------------------------------------
 * A semantic grid / mask only holds (0,0,0) and the colours of a small palette (reference utils/config.py:29-43, masks from
 * reference utils/mask_utils.py:14-87), so a voxel or pixel is one byte: label 0 <-> (0,0,0), label k <-> palette[k-1]
 * (npal <= 254 distinct non-black colours).  rgb_to_label fails with PB3D_EINVAL on a colour outside palette + black;
 * label_to_rgb on a label above npal.  The carve ops take label volumes as they are:
 *   carve_voxel_grid_with_masks  = pb3d_carve_mask_dev with C = 1 (reference utils/voxel_carving_utils.py:76-87);
 *   global_carve                 = pb3d_global_carve_label_dev: (w,h,w) labels = label_hw[y,x] where the carve keeps (:269-298);
 *   part_carve                   = pb3d_part_carve_label_dev, same job description as pb3d_part_carve_dev (:139-160).
 * Expanding any of their results with pb3d_label_to_rgb_dev gives the bytes of the RGB entry points. */
int pb3d_rgb_to_label_dev(pb3d_ctx* ctx, const uint8_t* d_rgb, int64_t nvox, const uint8_t* palette, int npal, uint8_t* d_label);
int pb3d_label_to_rgb_dev(pb3d_ctx* ctx, const uint8_t* d_label, int64_t nvox, const uint8_t* palette, int npal, uint8_t* d_rgb);
int pb3d_global_carve_label_dev(pb3d_ctx* ctx, const uint8_t* d_bin_hw, const uint8_t* d_label_hw, int64_t h, int64_t w, int angle_interval,
                                uint8_t* d_out);
int pb3d_part_carve_label_dev(pb3d_ctx* ctx, const uint8_t* d_label, int64_t W, int64_t H, int64_t D, const uint8_t* d_mask_sub,
                              const uint8_t* d_mask_carve, const int* job_angle, const int* job_skip, int njobs, uint8_t* d_out);

/* ---- seeded synthetic inputs generated on the device ---------------------
 * mask16: labels (S,S) uint8 in 0..15 by the closed formula scaled from S=1024; binary and
 * rgb derive from it.  Any output pointer may be NULL.  sem grid: palette[label16 of a
 * splitmix64 hash of the voxel index] (kind 0) -- worst case for any sparsity trick.
 * pb3d_synth_sem_dev needs d_slab_rgb 4-byte aligned (it stores dwords) and refuses other
 * pointers with PB3D_EINVAL. */
int pb3d_synth_mask16_dev(pb3d_ctx* ctx, int64_t S, uint8_t* d_label_hw, uint8_t* d_binary_hw, uint8_t* d_rgb_hw3,
                          uint8_t* d_binary_wh);
int pb3d_synth_sem_dev(pb3d_ctx* ctx, int64_t x0, int64_t x1, int64_t H, int64_t D, uint64_t seed, uint8_t* d_slab_rgb);
int pb3d_synth_occ_dev(pb3d_ctx* ctx, int64_t x0, int64_t x1, int64_t H, int64_t D, uint64_t seed, uint8_t* d_slab);
int pb3d_synth_palette16(uint8_t palette[48]);

/* ---- multi-GPU: slab reassembly with ONE RCCL all-gather over xGMI -----------------------
 * One process per GPU.  Rank 0 obtains a 128-byte id, the launcher distributes it, every
 * rank calls pb3d_comm_init.  pb3d_allgather_dev gathers `bytes_per_rank` from each rank's
 * d_send into d_recv[rank * bytes_per_rank ...] (d_send may be the rank's own slot: in place). */
int pb3d_comm_unique_id(uint8_t id[128]);
int pb3d_comm_init(pb3d_ctx* ctx, const uint8_t id[128], int rank, int nranks);
/* what the communicator itself reports (ncclCommUserRank / ncclCommCount): lets a launcher confirm RCCL saw every rank */
int pb3d_comm_info(pb3d_ctx* ctx, int* rank, int* nranks);
int pb3d_allgather_dev(pb3d_ctx* ctx, const void* d_send, void* d_recv, size_t bytes_per_rank);
int pb3d_comm_destroy(pb3d_ctx* ctx);
/* Sharded forms of the carve: one process per GPU, communicator from pb3d_comm_init.  Rank r of n owns the X-planes
 * [r W/n, (r+1) W/n) (W % n == 0): it carves ITS slab (d_grid_slab: planes x H x D x C bytes; d_mask_wh: the full (W,H) mask) into its
 * slot of d_out_full and ONE in-place ncclAllGather leaves the whole carved volume on every rank.  Asynchronous like every *_dev
 * entry.  carve_labels: the same on a label slab (1 B/voxel over xGMI instead of 3), then -- if d_rgb_full is not NULL -- the
 * local expansion of the reassembled label volume to RGB (labels above npal expand to black; no read-back). */
int pb3d_carve_mask_sharded_dev(pb3d_ctx* ctx, const uint8_t* d_grid_slab, int64_t W, int64_t H, int64_t D, int C, const uint8_t* d_mask_wh,
                                uint8_t* d_out_full);
int pb3d_global_carve_sharded_dev(pb3d_ctx* ctx, const uint8_t* d_bin_hw, const uint8_t* d_rgb_hw3, int64_t h, int64_t w, int angle_interval,
                                  uint8_t* d_out_full);
int pb3d_carve_labels_sharded_dev(pb3d_ctx* ctx, const uint8_t* d_label_slab, int64_t W, int64_t H, int64_t D, const uint8_t* d_mask_wh,
                                  uint8_t* d_label_full, const uint8_t* palette, int npal, uint8_t* d_rgb_full);
/* points partition of the projection (project_colored_voxels, reference utils/projection_utils.py:5-23): a rank projects its
 * contiguous range [index_base, index_base + n) of the point list into 64-bit keys (global index + 1) << 24 | rgb (zero = no
 * point); pb3d_allreduce_max_u64_dev (in place, ncclMax) merges the ranks' key images; resolve writes the (H,W,3) image. */
int pb3d_project_keys_dev(pb3d_ctx* ctx, const void* d_pts, int pts_f64, const uint8_t* d_cols, int64_t n, int64_t index_base,
                          const double R[9], const double cam[3], double f, double cx, double cy, const int prec[4], int Himg, int Wimg,
                          uint64_t* d_keys);
int pb3d_project_resolve_keys_dev(pb3d_ctx* ctx, const uint64_t* d_keys, int Himg, int Wimg, uint8_t* d_img);
int pb3d_allreduce_max_u64_dev(pb3d_ctx* ctx, void* d_buf, size_t count);

#ifdef __cplusplus
}
#endif
#endif /* PB3D_H */
