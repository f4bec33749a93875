// The triangle cell index of csrc/meshdist.hip (point-to-mesh distances) and csrc/inside.hip (containment): one build for both.
//
// The grid is the searches' own (csrc/ring_walk.h: make_grid from the exact box of ALL vertices and the face count, two faces per
// cell; an unreferenced vertex only enlarges the box).  With axes == 2 the a2 extent of the box is zeroed first, so the grid has one
// cell along a2 and is the 2-D grid over (a0, a1) that containment walks: there n[2] == 1 and inv[2] == 0, cell_of returns 0 for every
// coordinate, and the three-axis text below lists, counts and halves exactly as a two-axis one would.
// A face is listed in every cell of cell_of(min corner) .. cell_of(max corner) per axis.  cell_of is monotone, so every point of a
// face lies in a cell the face is listed in.  With SKIP_FLAT a face whose projection on (a0, a1) has no area (cross_area == 0) is
// listed nowhere: it crosses no ray along a2.
//   k_face_corners   the corners of every face, widened, into an nf x 9 float64 table: the searches follow one indirection (cell ->
//                    face id -> 72 bytes) whatever the vertex and index dtypes are.  Counts the flat faces when asked to
//   k_face_entries   the (cell, face) entry total of a grid, without touching a cell
//   k_face_bin       counts per cell; then, behind the exclusive scan of csrc/points.hip, the scatter of face ids (order within a cell
//                    is free: integer atomics on the cursors)
// One giant face among small ones would be listed in nearly every cell: while the entries exceed kEntryCap = 8 per face and the grid
// has more than one cell, the cells per axis are halved (coarsen) and the entries recounted.  In 2-D one wall cannot
// break the cap (one entry per cell, nf / 2 in all); a mesh whose typical face is several cells wide does.
// Host waits: the box, and one per count of the entries (1 + the number of halvings).
// Measured against the two copies this file replaced (profiles/face_index_ab.jsonl: the stride-1 mesh of the stored Taj grid, 1 518 156
// faces; whole calls, medians of 5, the parent commit's build and this one alternating, two runs each, the first of two such visits;
// parent / this file):
//   3 axes, nothing skipped   index build + one distance query 0.756, 0.754 / 0.693, 0.672 ms (one atomic per workgroup in the entry
//                             count, where the copy had one per wavefront); all 12.0 M grid points 227.8, 227.9 / 227.6, 227.5 ms
//   2 axes, flat faces out    index build by the call's own events 0.671, 0.676 / 0.667, 0.678 ms; containment of the grid's 72.9 M
//                             sample points 16.99, 17.14 / 16.85, 17.05 ms, of its 12.0 M points 6.37, 6.31 / 6.34, 6.43 ms, of the
//                             20 k SfM sample 0.806, 0.806 / 0.811, 0.808 ms
// Over both visits the 2-axis index build took 0.665 - 0.677 ms in the parent's four runs and 0.666 - 0.678 ms in this file's (the
// 12.0 M-point row's events).  Run-to-run differences of one build reach 0.01 ms there, so a cost of the third loop of length 1 below
// about 1 % of the build cannot be told from none; the whole calls show no side that is consistently slower.
#include <cmath>

#include "cross_rule.h"
#include "pb3d_internal.h"
#include "ring_walk.h"
#include "wave.h"

namespace {

constexpr i64 kEntryCap = 8;            // (cell, face) entries per face the index accepts before it coarsens the grid

// flat: where the faces without a projected area are counted, or null
template <bool VF64, bool I64>
__global__ __launch_bounds__(256) void k_face_corners(const void* __restrict__ verts, i64 nv, const void* __restrict__ faces, i64 nf,
                                                      double* __restrict__ tri, u64* __restrict__ flat) {
    u64 n = 0;
    for (i64 f = (i64)blockIdx.x * 256 + threadIdx.x; f < nf; f += (i64)gridDim.x * 256) {
        double t[9];
#pragma unroll
        for (int c = 0; c < 3; ++c) pb3d_load3<VF64>(verts, wrap(load_index<I64>(faces, 3 * f + c), nv), t + 3 * c);
#pragma unroll
        for (int k = 0; k < 9; ++k) tri[9 * f + k] = t[k];
        if (flat) n += cross_area(t, t + 3, t + 6) == 0.0;
    }
    if (flat) group_add(n, flat);
}

// the cells a face is listed in: cell_of(min corner) .. cell_of(max corner), per axis; false: listed nowhere
template <bool SKIP_FLAT>
__device__ __forceinline__ bool face_cells(const Grid& g, const double* __restrict__ t, int lo[3], int hi[3]) {
    if (SKIP_FLAT && cross_area(t, t + 3, t + 6) == 0.0) return false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        lo[a] = cell_of(g, a, fmin(fmin(t[a], t[3 + a]), t[6 + a]));
        hi[a] = cell_of(g, a, fmax(fmax(t[a], t[3 + a]), t[6 + a]));
    }
    return true;
}

template <bool SKIP_FLAT>
__global__ __launch_bounds__(256) void k_face_entries(const double* __restrict__ tri, i64 nf, Grid g, u64* __restrict__ total) {
    u64 n = 0;
    for (i64 f = (i64)blockIdx.x * 256 + threadIdx.x; f < nf; f += (i64)gridDim.x * 256) {
        int lo[3], hi[3];
        if (face_cells<SKIP_FLAT>(g, tri + 9 * f, lo, hi)) n += (u64)(hi[0] - lo[0] + 1) * (u64)(hi[1] - lo[1] + 1) * (u64)(hi[2] - lo[2] + 1);
    }
    group_add(n, total);
}

// FILL false: counts[cell] += 1 per entry;  FILL true: ids[start[cell] + cursor[cell]++] = face (cursor: zeroed per-cell counters)
template <bool SKIP_FLAT, bool FILL>
__global__ __launch_bounds__(256) void k_face_bin(const double* __restrict__ tri, i64 nf, Grid g, u32* __restrict__ counts,
                                                  const i64* __restrict__ start, int* __restrict__ ids) {
    for (i64 f = (i64)blockIdx.x * 256 + threadIdx.x; f < nf; f += (i64)gridDim.x * 256) {
        int lo[3], hi[3];
        if (!face_cells<SKIP_FLAT>(g, tri + 9 * f, lo, hi)) continue;
        for (int i = lo[0]; i <= hi[0]; ++i)
            for (int j = lo[1]; j <= hi[1]; ++j)
                for (int k = lo[2]; k <= hi[2]; ++k) {
                    const i64 c = cell_index(g, i, j, k);
                    if (FILL) ids[start[c] + atomicAdd(&counts[c], 1u)] = (int)f;
                    else atomicAdd(&counts[c], 1u);
                }
    }
}

// halve the cells per axis (the box stays; a one-cell axis stays one cell)
Grid coarsen(Grid g) {
    g.ncells = 1;
    for (int a = 0; a < 3; ++a) {
        g.n[a] = (g.n[a] + 1) / 2;
        const double ext = g.hi[a] - g.lo[a];
        g.inv[a] = g.n[a] > 1 ? (double)g.n[a] / ext : 0.0;
        g.h[a] = g.n[a] > 1 ? ext / (double)g.n[a] : 0.0;
        g.ncells *= g.n[a];
    }
    return g;
}

// the entries counted (and the cells halved until they respect the cap), then count, scan, scatter
template <bool SKIP_FLAT>
int build(pb3d_ctx* ctx, i64 nf, Grid g, const double* tri, u64* d_total, const pb3d_face_index_slots& s, pb3d_face_index* out) {
    const unsigned nb = pb3d_stream_blocks(ctx, nf, 256, 8);
    u64 total = 0;
    i64 coarsenings = 0;
    for (;;) {
        PB3D_HIP(hipMemsetAsync(d_total, 0, sizeof(u64), ctx->stream));
        hipLaunchKernelGGL(k_face_entries<SKIP_FLAT>, dim3(nb), dim3(256), 0, ctx->stream, tri, nf, g, d_total);
        PB3D_CHECK_LAUNCH();
        PB3D_TRY(pb3d_read_back(ctx, &total, d_total, sizeof(total)));
        if (total <= (u64)(kEntryCap * nf) || g.ncells == 1) break;
        g = coarsen(g);
        ++coarsenings;
    }
    void *cnt, *st, *ids;
    PB3D_TRY(pb3d_scratch(ctx, s.counts, (size_t)g.ncells * sizeof(u32), &cnt));
    PB3D_TRY(pb3d_scratch(ctx, s.starts, (size_t)(g.ncells + 1) * sizeof(i64), &st));
    PB3D_TRY(pb3d_scratch(ctx, s.ids, (size_t)total * sizeof(int), &ids));
    PB3D_HIP(hipMemsetAsync(cnt, 0, (size_t)g.ncells * sizeof(u32), ctx->stream));
    hipLaunchKernelGGL((k_face_bin<SKIP_FLAT, false>), dim3(nb), dim3(256), 0, ctx->stream, tri, nf, g, (u32*)cnt, (const i64*)nullptr,
                       (int*)nullptr);
    PB3D_CHECK_LAUNCH();
    PB3D_TRY(pb3d_scan_counts(ctx, (const u32*)cnt, g.ncells, (i64*)st, s.scan_local, s.scan_segs));
    PB3D_HIP(hipMemsetAsync(cnt, 0, (size_t)g.ncells * sizeof(u32), ctx->stream));      // the scatter's cursors
    hipLaunchKernelGGL((k_face_bin<SKIP_FLAT, true>), dim3(nb), dim3(256), 0, ctx->stream, tri, nf, g, (u32*)cnt, (const i64*)st, (int*)ids);
    PB3D_CHECK_LAUNCH();
    *out = {g, (const i64*)st, (const int*)ids, tri, (i64)total, coarsenings};
    return PB3D_OK;
}

}  // namespace

// face indices checked; nv, nf >= 1.  The read-back slot holds eight 64-bit words: the box at [0, 6), the entry total at [6], and [7]
// left to the caller
int pb3d_face_index_build(pb3d_ctx* ctx, const char* what, const void* d_verts, int verts_f64, i64 nv, const void* d_faces, int faces_i64, i64 nf,
                          int axes, bool skip_flat, u64* d_flat, const pb3d_face_index_slots& s, pb3d_face_index* out) {
    void *tri, *rb;
    PB3D_TRY(pb3d_scratch(ctx, s.corners, (size_t)nf * 9 * sizeof(double), &tri));
    with_mesh_types(verts_f64, faces_i64, [&](auto V, auto I) {
        hipLaunchKernelGGL((k_face_corners<decltype(V)::value, decltype(I)::value>), dim3(pb3d_stream_blocks(ctx, nf, 256, 8)), dim3(256), 0,
                           ctx->stream, d_verts, nv, d_faces, nf, (double*)tri, d_flat);
    });
    PB3D_CHECK_LAUNCH();
    PB3D_TRY(pb3d_scratch(ctx, s.readback, 8 * sizeof(u64), &rb));
    double b[6];
    PB3D_TRY(pb3d_points_box(ctx, d_verts, verts_f64, nv, s.readback, b));
    // (a caller that has checked every coordinate, as containment has, cannot fail here)
    for (int a = 0; a < 6; ++a) PB3D_REQUIRE(std::isfinite(b[a]), "%s: the vertices must be finite", what);
    if (axes == 2) b[2] = b[5] = 0.0;       // one cell along a2
    const Grid g = make_grid(b, nf);
    return skip_flat ? build<true>(ctx, nf, g, (const double*)tri, (u64*)rb + 6, s, out)
                     : build<false>(ctx, nf, g, (const double*)tri, (u64*)rb + 6, s, out);
}
