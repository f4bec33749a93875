// points_in_mesh: containment of arbitrary query points in a triangle mesh by crossing parity, and the sign pass that turns
// pb3d_mesh_dist_resident's distances into signed ones (include/pb3d.h, "containment", has the rule to the bit; DESIGN.md "Containment"
// has the passes and their times).  The rule is csrc/voxelize.hip's, from the one copy in csrc/cross_rule.h, with the column (i, j)
// replaced by the query's (q0, q1): at a lattice point the byte is the voxel's.  What differs is everything around the rule: the
// queries are scattered, so nothing is rasterised and the faces need an index.
//
// Index: csrc/face_index.hip's (the passes are described there), the one csrc/meshdist.hip searches, asked for a 2-D cell grid over the
// exact (a0, a1) box of ALL vertices -- one cell along a2 -- and for the faces with area == 0 to be listed nowhere and counted.
// cell_of is monotone, so a face whose projected box holds (q0, q1) is listed in the query's cell.  The stride-1 mesh of the stored Taj
// grid (1 518 156 faces, 1 112 342 of them flat in projection and listed nowhere) makes 2.78 entries per face in 1167 x 651 cells.
//   k_inside_query     one lane per query.  Outside the vertices' (a0, a1) box, or with a NaN coordinate: outside, no walk.  Otherwise
//                      the list of the query's one cell: per candidate the projected box from six of the nine corner values, then the
//                      three edge set-ups and tests, and only for a covering face the plane and its one division.
//                      below and total live in registers; one byte and, if asked, two int32 are written.  NO atomics: with stats
//                      each workgroup leaves three partial counts and k_inside_totals adds them, so the result is a function of the
//                      input alone.  60-62 VGPRs (46-48 in the table form below), no scratch, no spills
//   k_inside_setup     knob "inside_table" = 1 only: a 184-byte row of finished set-ups per face, from the index's corner table, for
//                      the query to read
// Two choices, both measured on that mesh (profiles/inside_opbench.jsonl, whole calls, variants in turn, medians of 5) and both left
// as knobs that change no byte:
//   * The set-up is recomputed per candidate from the 72-byte corner row.  Reading it from the table instead (some twenty operations
//     saved, 2.5 times the bytes) is slower everywhere: 72.9 M lattice queries in the mesh's frame 17 -> 31 ms, the same in the
//     lattice frame 3.0 -> 4.5 ms, the grid's own 12.0 M points 6.4 -> 15 ms.  The walk waits for memory, not for the VALU.
//   * Queries are walked in input order.  In the index's cell order (knob "inside_order" = 1: csrc/nn.hip's query binning, its time
//     included) a cloud whose order says nothing about its cells gains from about 100 k queries on -- shuffled samples of the grid's
//     points: 20 k 1.04, 100 k 0.97, 1 M 0.74, 12.0 M 0.54 of the input order's time; the 20 k SfM sample 1.1 -- but a cloud that is
//     already coherent loses far more than that: the lattice points of a grid with a2 fastest share (q0, q1) across a wavefront and
//     walk one list together, 3.0 ms in input order against 21 ms once binned and scattered.  The input order never costs more
//     than 1.9 times the better choice, the cell order up to 7 times, and nothing cheap tells the two kinds of cloud apart.
//   k_dist_sign        out = inside && d > 0 ? -d : d
//   k_flags_not        out = flags == 0: the bytes pb3d_points_select_resident takes to keep the points outside
// Host waits per call: the index / finiteness check, the box, one per count of the entries (1 + the number of halvings), one more for
// stats, one more under knob "inside_timing".
#include <cmath>

#include "wave.h"
#include "cross_rule.h"
#include "pb3d_internal.h"
#include "ring_walk.h"

namespace {

constexpr i64 kMaxElems = (1ll << 31) - 1;

// knob "inside_table" = 1: the finished set-up of every face with an area, kSetupRow doubles a face -- the projected box (min0, max0,
// min1, max1), ex, ey, lx, ly, pos, then a0, a1, a2, nx, ny, area -- by the same functions, so the query reads the very doubles it
// would have computed
constexpr int kSetupRow = 23;
__global__ __launch_bounds__(256) void k_inside_setup(const double* __restrict__ tri, i64 nf, double* __restrict__ setup) {
    for (i64 f = (i64)blockIdx.x * 256 + threadIdx.x; f < nf; f += (i64)gridDim.x * 256) {
        const double* t = tri + 9 * f;
        const double area = cross_area(t, t + 3, t + 6);
        if (area == 0.0) continue;              // listed nowhere: its row is never read
        CrossFace c;
        cross_edges(t, t + 3, t + 6, area, &c);
        cross_plane(t, t + 3, t + 6, &c);
        double* r = setup + kSetupRow * f;
        r[0] = fmin(fmin(t[0], t[3]), t[6]); r[1] = fmax(fmax(t[0], t[3]), t[6]);
        r[2] = fmin(fmin(t[1], t[4]), t[7]); r[3] = fmax(fmax(t[1], t[4]), t[7]);
#pragma unroll
        for (int e = 0; e < 3; ++e) { r[4 + e] = c.ex[e]; r[7 + e] = c.ey[e]; r[10 + e] = c.lx[e]; r[13 + e] = c.ly[e]; }
        r[16] = (double)c.pos;
        r[17] = c.a0; r[18] = c.a1; r[19] = c.a2; r[20] = c.nx; r[21] = c.ny; r[22] = c.area;
    }
}

// one candidate face against the query: does it cover (q0, q1), and if so is its height at or below q2
template <bool TABLE>
__device__ __forceinline__ void try_face(const double* __restrict__ tri, const double* __restrict__ setup, i64 face, const double (&qv)[3],
                                         int* below, int* total) {
    CrossFace f;
    if (TABLE) {
        const double* r = setup + kSetupRow * face;
        if (!(r[0] <= qv[0] && qv[0] <= r[1] && r[2] <= qv[1] && qv[1] <= r[3])) return;
#pragma unroll
        for (int e = 0; e < 3; ++e) { f.ex[e] = r[4 + e]; f.ey[e] = r[7 + e]; f.lx[e] = r[10 + e]; f.ly[e] = r[13 + e]; }
        f.pos = (u32)r[16];
        if (!cross_covers(f, qv[0], qv[1])) return;
        f.a0 = r[17]; f.a1 = r[18]; f.a2 = r[19]; f.nx = r[20]; f.ny = r[21]; f.area = r[22];
    } else {
        const double* t = tri + 9 * face;
        const double A[2] = {t[0], t[1]}, B[2] = {t[3], t[4]}, C[2] = {t[6], t[7]};
        if (!(fmin(fmin(A[0], B[0]), C[0]) <= qv[0] && qv[0] <= fmax(fmax(A[0], B[0]), C[0]) &&
              fmin(fmin(A[1], B[1]), C[1]) <= qv[1] && qv[1] <= fmax(fmax(A[1], B[1]), C[1])))
            return;
        cross_edges(A, B, C, cross_area(A, B, C), &f);          // listed: it has an area
        if (!cross_covers(f, qv[0], qv[1])) return;
        cross_plane(t, t + 3, t + 6, &f);
    }
    ++*total;
    *below += cross_height(f, qv[0], qv[1]) <= qv[2];           // a NaN height counts in total only
}

// partials (STATS): per workgroup {queries inside, with an odd total, outside the box}
template <bool QF64, bool ORDERED, bool STATS, bool TABLE>
__global__ __launch_bounds__(256) void k_inside_query(const void* __restrict__ q, i64 nq, const u32* __restrict__ order, Grid g,
                                                      const i64* __restrict__ start, const int* __restrict__ ids, const double* __restrict__ tri,
                                                      const double* __restrict__ setup, u8* __restrict__ inside, int* __restrict__ counts,
                                                      u32* __restrict__ partials) {
    const i64 s = (i64)blockIdx.x * 256 + threadIdx.x;
    u32 in = 0, odd = 0, out = 0;
    if (s < nq) {
        const i64 qi = ORDERED ? (i64)order[s] : s;
        double qv[3];
        pb3d_load3<QF64>(q, qi, qv);
        int below = 0, total = 0;
        // a NaN compares false: outside.  (The comparison with itself is the test of q2, which the box does not see)
        const bool boxed = qv[0] >= g.lo[0] && qv[0] <= g.hi[0] && qv[1] >= g.lo[1] && qv[1] <= g.hi[1] && qv[2] == qv[2];
        if (boxed) {
            const i64 c = cell_index(g, cell_of(g, 0, qv[0]), cell_of(g, 1, qv[1]), 0);
            const i64 e = start[c + 1];
#pragma nounroll
            for (i64 p = start[c]; p < e; ++p) try_face<TABLE>(tri, setup, (i64)ids[p], qv, &below, &total);
        } else {
            out = 1;
        }
        inside[qi] = (u8)(below & 1);
        if (counts) { counts[2 * qi] = below; counts[2 * qi + 1] = total; }
        in = (u32)(below & 1);
        odd = (u32)(total & 1);
    }
    if (STATS) {
        __shared__ u32 w_in[4], w_odd[4], w_out[4];
        u32* dst = partials + 3 * (i64)blockIdx.x;
        group_total<4>(wave_sum(in), w_in, [&](u32 t) { dst[0] = t; });
        group_total<4>(wave_sum(odd), w_odd, [&](u32 t) { dst[1] = t; });
        group_total<4>(wave_sum(out), w_out, [&](u32 t) { dst[2] = t; });
    }
}

// one workgroup: stats[0], [1], [3] = the sums of the nb workgroups' partial counts (stats[2], the flat faces, is the index build's)
__global__ __launch_bounds__(1024) void k_inside_totals(const u32* __restrict__ partials, i64 nb, u64* __restrict__ stats) {
    __shared__ u64 w0[16], w1[16], w2[16];
    u64 a = 0, b = 0, c = 0;
    for (i64 i = threadIdx.x; i < nb; i += 1024) { a += partials[3 * i]; b += partials[3 * i + 1]; c += partials[3 * i + 2]; }
    group_total<16>(wave_sum(a), w0, [&](u64 t) { stats[0] = t; });
    group_total<16>(wave_sum(b), w1, [&](u64 t) { stats[1] = t; });
    group_total<16>(wave_sum(c), w2, [&](u64 t) { stats[3] = t; });
}

__global__ __launch_bounds__(256) void k_dist_sign(const double* dist, const u8* __restrict__ inside, i64 n, double* out) {      // out may be dist
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double d = dist[i];
    out[i] = inside[i] && d > 0.0 ? -d : d;
}

__global__ __launch_bounds__(256) void k_flags_not(const u8* flags, i64 n, u8* out) {       // out may be flags
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = flags[i] == 0;
}

// setup: null unless inside_table
template <bool QF64, bool ORDERED>
void launch_query(pb3d_ctx* ctx, unsigned nb, const void* d_P, i64 nP, const u32* order, const pb3d_face_index& ix, const double* setup,
                  u8* d_inside, int* d_counts, u32* partials) {
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(nb), dim3(256), 0, ctx->stream, d_P, nP, order, ix.g, ix.starts, ix.ids, ix.tri, setup, d_inside, d_counts,
                           partials);
    };
    if (partials && setup) go(k_inside_query<QF64, ORDERED, true, true>);
    else if (partials) go(k_inside_query<QF64, ORDERED, true, false>);
    else if (setup) go(k_inside_query<QF64, ORDERED, false, true>);
    else go(k_inside_query<QF64, ORDERED, false, false>);
}

}  // namespace

extern "C" {

int pb3d_points_in_mesh_resident(pb3d_ctx* ctx, const void* d_P, int p_f64, int64_t nP, const void* d_verts, int verts_f64, int64_t nv,
                                 const void* d_faces, int faces_i64, int64_t nf, uint8_t* d_inside, int32_t* d_counts, int64_t stats[4]) {
    PB3D_REQUIRE(nP >= 0 && nv >= 0 && nf >= 0, "pb3d_points_in_mesh: negative count");
    PB3D_REQUIRE(nP <= kMaxElems && nv <= kMaxElems && nf <= kMaxElems / 3,
                 "pb3d_points_in_mesh: at most 2^31 - 1 queries, vertices and face corners");
    PB3D_REQUIRE((nP == 0 || (d_P && d_inside)) && (nv == 0 || d_verts) && (nf == 0 || d_faces), "pb3d_points_in_mesh: null buffer");
    PB3D_REQUIRE(ctx != nullptr, "pb3d_points_in_mesh: null context");

    void *rb, *sv;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_INSIDE_READBACK, 8 * sizeof(u64), &rb));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_INSIDE_STATS, 4 * sizeof(u64), &sv));
    u64* d_stats = (u64*)sv;
    if (nv > 0 || nf > 0) PB3D_TRY(check_mesh(ctx, "pb3d_points_in_mesh", d_verts, verts_f64, nv, d_faces, faces_i64, nf, (u32*)((u64*)rb + 7)));
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if (nP == 0) return PB3D_OK;
    ctx->inside_last = {true, false, {0.0f, 0.0f}, {0, 0, 0, 0}};
    if (nf == 0) {          // no face, no crossing: everything is outside (and there is no box to be inside of)
        PB3D_HIP(hipMemsetAsync(d_inside, 0, (size_t)nP, ctx->stream));
        if (d_counts) PB3D_HIP(hipMemsetAsync(d_counts, 0, (size_t)nP * 2 * sizeof(int32_t), ctx->stream));
        if (stats) stats[3] = nP;
        return PB3D_OK;
    }

    pb3d_stamps<3> t = {ctx->tune_inside_timing != 0, 0, {}};       // knob "inside_timing"
    PB3D_TRY(t.mark(ctx));
    PB3D_HIP(hipMemsetAsync(d_stats, 0, 4 * sizeof(u64), ctx->stream));
    // the index over (a0, a1), flat faces left out and counted into stats[2]; the mesh is checked, so its box is finite
    const pb3d_face_index_slots slots = {PB3D_SLOT_INSIDE_CORNERS, PB3D_SLOT_INSIDE_READBACK, PB3D_SLOT_INSIDE_COUNTS, PB3D_SLOT_INSIDE_STARTS,
                                         PB3D_SLOT_INSIDE_IDS, PB3D_SLOT_INSIDE_SCAN_LOCAL, PB3D_SLOT_INSIDE_SCAN_SEGS};
    pb3d_face_index ix;
    PB3D_TRY(pb3d_face_index_build(ctx, "pb3d_points_in_mesh", d_verts, verts_f64, nv, d_faces, faces_i64, nf, 2, true, d_stats + 2, slots, &ix));
    ctx->inside_last.info[0] = ix.g.n[0];
    ctx->inside_last.info[1] = ix.g.n[1];
    ctx->inside_last.info[2] = ix.entries;
    ctx->inside_last.info[3] = ix.coarsenings;
    void* setup = nullptr;
    if (ctx->tune_inside_table) {
        PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_INSIDE_SETUP, (size_t)nf * kSetupRow * sizeof(double), &setup));
        hipLaunchKernelGGL(k_inside_setup, dim3(pb3d_stream_blocks(ctx, nf, 256, 8)), dim3(256), 0, ctx->stream, ix.tri, (i64)nf, (double*)setup);
        PB3D_CHECK_LAUNCH();
    }
    PB3D_TRY(t.mark(ctx));
    const unsigned nb = (unsigned)((nP + 255) / 256);
    void* pt = nullptr;
    if (stats) PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_INSIDE_PARTIALS, (size_t)nb * 3 * sizeof(u32), &pt));
    const u32* order = nullptr;
    if (ctx->tune_inside_order) PB3D_TRY(pb3d_nn_order_queries(ctx, d_P, p_f64, nP, ix.g, &order));
    if (order) {
        if (p_f64) launch_query<true, true>(ctx, nb, d_P, nP, order, ix, (const double*)setup, d_inside, (int*)d_counts, (u32*)pt);
        else launch_query<false, true>(ctx, nb, d_P, nP, order, ix, (const double*)setup, d_inside, (int*)d_counts, (u32*)pt);
    } else {
        if (p_f64) launch_query<true, false>(ctx, nb, d_P, nP, order, ix, (const double*)setup, d_inside, (int*)d_counts, (u32*)pt);
        else launch_query<false, false>(ctx, nb, d_P, nP, order, ix, (const double*)setup, d_inside, (int*)d_counts, (u32*)pt);
    }
    PB3D_CHECK_LAUNCH();
    if (stats) {
        hipLaunchKernelGGL(k_inside_totals, dim3(1), dim3(1024), 0, ctx->stream, (const u32*)pt, (i64)nb, d_stats);
        PB3D_CHECK_LAUNCH();
    }
    PB3D_TRY(t.mark(ctx));
    if (stats) PB3D_TRY(pb3d_read_back(ctx, stats, d_stats, 4 * sizeof(i64)));
    return t.finish(ctx, ctx->inside_last.ms, &ctx->inside_last.timed);
}

int pb3d_points_in_mesh_last(pb3d_ctx* ctx, int64_t info[4], double pass_ms[2]) {
    PB3D_REQUIRE(ctx != nullptr && info != nullptr, "pb3d_points_in_mesh_last: null argument");
    PB3D_REQUIRE(ctx->inside_last.valid, "pb3d_points_in_mesh_last: no containment test has run on this context");
    for (int i = 0; i < 4; ++i) info[i] = ctx->inside_last.info[i];
    if (pass_ms) {
        PB3D_REQUIRE(ctx->inside_last.timed, "pb3d_points_in_mesh_last: the last containment test was not timed (knob inside_timing)");
        for (int i = 0; i < 2; ++i) pass_ms[i] = ctx->inside_last.ms[i];
    }
    return PB3D_OK;
}

int pb3d_mesh_dist_sign_resident(pb3d_ctx* ctx, const double* d_dist, const uint8_t* d_inside, int64_t n, double* d_out) {
    PB3D_REQUIRE(n >= 0 && n <= kMaxElems, "pb3d_mesh_dist_sign: need 0 <= n <= 2^31 - 1 (got %lld)", (long long)n);
    if (n == 0) return PB3D_OK;
    PB3D_REQUIRE(d_dist != nullptr && d_inside != nullptr && d_out != nullptr, "pb3d_mesh_dist_sign: null buffer");
    PB3D_REQUIRE(ctx != nullptr, "pb3d_mesh_dist_sign: null context");
    hipLaunchKernelGGL(k_dist_sign, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_dist, d_inside, (i64)n, d_out);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

int pb3d_flags_not_resident(pb3d_ctx* ctx, const uint8_t* d_flags, int64_t n, uint8_t* d_out) {
    PB3D_REQUIRE(n >= 0 && n <= kMaxElems, "pb3d_flags_not: need 0 <= n <= 2^31 - 1 (got %lld)", (long long)n);
    if (n == 0) return PB3D_OK;
    PB3D_REQUIRE(d_flags != nullptr && d_out != nullptr, "pb3d_flags_not: null buffer");
    PB3D_REQUIRE(ctx != nullptr, "pb3d_flags_not: null context");
    hipLaunchKernelGGL(k_flags_not, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_flags, (i64)n, d_out);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

}  // extern "C"
