// A triangle mesh as a comparison target: exact point-to-mesh distances (pb3d_mesh_dist_resident) and stratified area-weighted surface
// samples (pb3d_mesh_sample_resident).  include/pb3d.h states the arithmetic of both to the bit; tests/meshdist_restate.py and
// tests/meshsample_restate.py restate it in NumPy and the kernels must return their bytes.
//
// Distance.  For every query the minimum over all faces of d2(q, face) -- the squared distance to the face's closest point by Ericson's
// region walk (Real-Time Collision Detection 5.1.5), a degenerate face by its three segments -- ties to the lowest face index, one
// __dsqrt_rn at the end.  Float64 throughout, float32 widened first; the Makefile passes -ffp-contract=off, so every product, sum and
// quotient below is one rounded operation.
//
// Index: csrc/face_index.hip's (the passes are described there), the one csrc/inside.hip walks in 2-D: the cell grid of csrc/nn.hip over
// the exact box of the vertices, every face listed in the cells of cell_of(min corner) .. cell_of(max corner) per axis, the cells halved
// while the entries exceed the cap, and the corners of every face gathered once into an nf x 9 float64 table, so the search follows
// one indirection (cell -> face id -> 72 bytes) whatever the vertex and index dtypes are.
// Host waits per call: the index check, the box, and one per count of the entries (1 + the number of coarsenings).
//
// Search: one lane per query, queries in cell order, ring_walk of csrc/ring_walk.h itself with (d2, face) as its Best.  Why the walk's
// bounds, made for points in cells, hold for triangles in cells:
//   * cell_of is monotone, so every point of a face lies in a cell the face is listed in.  A face listed in no cell of the visited
//     box has a cell range disjoint from that box on some axis and therefore lies wholly beyond that face of the box: the walk's
//     lower bound over the cells not yet visited is a lower bound on its distance.
//   * A face listed only in pruned cells has its nearest point in a pruned cell, whose box is provably farther than the best so far.
//   * A face listed in a visited cell is evaluated WHOLE, not clipped to the cell, so its d2 is exact wherever its nearest point lies.
//   * Every candidate closest point is a point of the triangle up to the rounding of a + ab*v + ac*w, a few ulps of the coordinate
//     magnitude, so a computed d2 undershoots the true squared distance by no more than that; the walk's per-axis margin
//     tol = 1e-12 (|lo| + |hi| + |q|) is four orders of magnitude above it (measured on 4 000 needle triangles of aspect down to 1e-8
//     and coordinates up to 1e3 against np.longdouble: the largest undershoot was 9e-5 of tol).
// Inside a cell a face is first tested by its corners' box: the squared distance from the query to that box, every axis gap shrunk by
// the walk's tol, is a lower bound on the face's d2 as computed (its closest point lies in the box up to the rounding tol covers:
// tests/test_meshdist_restate.py checks every pair of the needle case), and the face is skipped only when beyond() proves it
// farther than the best so far -- strictly, so a tie is always evaluated and the lowest-face rule is untouched.  A dozen operations
// spare some 130 for most faces of the neighbouring cells: 270 -> 228 ms on the measurement below.
// A face that spans several visited cells is evaluated once per cell (no "already tried" filter; not timed): harmless to the result,
// since the update rule is a function of (d2, face) alone.  The closest point is recomputed from the winning face after the walk, by
// the same arithmetic, so the walk carries only (d2, face) and the three margins per lane.  k_mesh_query: 132 VGPRs, no scratch, no spills (capping it at
// 128 registers for a fourth wave per SIMD spills 20 bytes per lane, so it is not capped).
// Measured on the 1 518 156-face mesh of the stored Taj grid with its 12 021 844 points as queries (profiles/meshdist_ab.jsonl, two
// alternating runs each, before the box test went in): the corner table 270.7 / 270.2 ms, a gather through int32 faces into float32
// vertices inside the walk 261.6 / 262.6 ms.  The 3 % do not pay for eight instantiations of the walk in place of two, and float64 /
// int64 meshes gather 96 bytes a face where the table reads 72: the table stays.  The box test, the same way: 270.2 / 270.5 ms
// without, 227.7 / 228.1 ms with.
//
// Stated limitation of the arithmetic (it is Ericson's, in float64): on a sliver the barycentric quotients lose accuracy and the
// computed point, still on the triangle, is no longer the closest one.  Overshoot of the computed distance over the same algorithm in
// np.longdouble, coordinates up to 1e3, 2 000 triangles x 8 queries per row, aspect (smallest height over longest edge) in [row, 10 row),
// in ulps of 1e3 (1.14e-13) and relative to the distance (tests/test_meshdist_restate.py::test_accuracy_bound_and_sliver_table prints it
// and asserts the first three rows at 4 ulps):
//     aspect   1e-1     1e-2     1e-3     1e-4     1e-5     1e-6     1e-7     1e-8
//     ulps     1.25     1.07     0.98     7.5      5.7e4    9.3e8    1.4e12   2.2e14
//     relative 3.5e-10  2.4e-10  3.1e-10  9.5e-11  3.9e-7   5.4e-3   9.8      4.3e2
//
// Sampling.  Face areas, a cumulative sum whose order of additions is fixed (blocks of 1024 faces: a running sum inside each block,
// a running sum of the block totals, one addition per face), SplitMix64 numbers keyed by (seed, sample, j), a binary search per
// sample and one weighted sum per coordinate.  Nothing depends on the launch shape: two runs give the same bytes.
#include <cmath>

#include "mesh_index.h"
#include "pb3d_internal.h"
#include "ring_walk.h"

namespace {

constexpr int kPrefixBlock = 1024;      // faces per block of the cumulative area sum (include/pb3d.h)
constexpr int kNoFace = 0x7fffffff;

// the corners of face f, widened: t[0..3) = a, t[3..6) = b, t[6..9) = c
template <bool VF64, bool I64>
__device__ __forceinline__ void load_face(const void* verts, i64 nv, const void* faces, i64 f, double t[9]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) pb3d_load3<VF64>(verts, wrap(load_index<I64>(faces, 3 * f + c), nv), t + 3 * c);
}

// ---- d2(q, face) and the closest point ----------------------------------------------------------------------------------------------
__device__ __forceinline__ double dot3(const double* x, const double* y) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; }
__device__ __forceinline__ double div0(double a, double b) { return b == 0.0 ? 0.0 : __ddiv_rn(a, b); }
__device__ __forceinline__ double dist2(const double (&q)[3], const double* cp) {
    const double dx = q[0] - cp[0], dy = q[1] - cp[1], dz = q[2] - cp[2];
    return (dx * dx + dy * dy) + dz * dz;
}

// the segment s0 -> s1
__device__ __forceinline__ double segment_closest(const double* s0, const double* s1, const double (&q)[3], double cp[3]) {
    double e[3], w[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { e[a] = s1[a] - s0[a]; w[a] = q[a] - s0[a]; }
    const double dd = dot3(e, e);
    double t = dot3(w, e);
    t = dd == 0.0 ? 0.0 : fmin(fmax(__ddiv_rn(t, dd), 0.0), 1.0);
#pragma unroll
    for (int a = 0; a < 3; ++a) cp[a] = s0[a] + e[a] * t;
    return dist2(q, cp);
}

__device__ __forceinline__ double face_closest(const double* t, const double (&q)[3], double cp[3]) {
    const double *a = t, *b = t + 3, *c = t + 6;
    double ab[3], ac[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { ab[k] = b[k] - a[k]; ac[k] = c[k] - a[k]; }
    const double n0 = ab[1] * ac[2] - ab[2] * ac[1], n1 = ab[2] * ac[0] - ab[0] * ac[2], n2 = ab[0] * ac[1] - ab[1] * ac[0];
    if ((n0 * n0 + n1 * n1) + n2 * n2 == 0.0) {         // degenerate: AB, BC, CA, a later segment only if strictly nearer
        double best = segment_closest(a, b, q, cp), alt[3];
        double d = segment_closest(b, c, q, alt);
        if (d < best) { best = d; cp[0] = alt[0]; cp[1] = alt[1]; cp[2] = alt[2]; }
        d = segment_closest(c, a, q, alt);
        if (d < best) { best = d; cp[0] = alt[0]; cp[1] = alt[1]; cp[2] = alt[2]; }
        return best;
    }
    do {        // Ericson's regions in his order; the first that holds decides
        double p[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { p[k] = q[k] - a[k]; cp[k] = a[k]; }
        const double d1 = dot3(ab, p), d2 = dot3(ac, p);
        if (d1 <= 0.0 && d2 <= 0.0) break;                                          // a
#pragma unroll
        for (int k = 0; k < 3; ++k) p[k] = q[k] - b[k];
        const double d3 = dot3(ab, p), d4 = dot3(ac, p);
        if (d3 >= 0.0 && d4 <= d3) {                                                // b
#pragma unroll
            for (int k = 0; k < 3; ++k) cp[k] = b[k];
            break;
        }
        const double vc = d1 * d4 - d3 * d2;
        if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {                                  // edge ab
            const double v = div0(d1, d1 - d3);
#pragma unroll
            for (int k = 0; k < 3; ++k) cp[k] = a[k] + ab[k] * v;
            break;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) p[k] = q[k] - c[k];
        const double d5 = dot3(ab, p), d6 = dot3(ac, p);
        if (d6 >= 0.0 && d5 <= d6) {                                                // c
#pragma unroll
            for (int k = 0; k < 3; ++k) cp[k] = c[k];
            break;
        }
        const double vb = d5 * d2 - d1 * d6;
        if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {                                  // edge ac
            const double w = div0(d2, d2 - d6);
#pragma unroll
            for (int k = 0; k < 3; ++k) cp[k] = a[k] + ac[k] * w;
            break;
        }
        const double va = d3 * d6 - d5 * d4;
        const double u1 = d4 - d3, u2 = d5 - d6;
        if (va <= 0.0 && u1 >= 0.0 && u2 >= 0.0) {                                  // edge bc
            const double w = div0(u1, u1 + u2);
#pragma unroll
            for (int k = 0; k < 3; ++k) cp[k] = b[k] + (c[k] - b[k]) * w;
            break;
        }
        const double den = div0(1.0, (va + vb) + vc);                               // the interior
        const double v = vb * den, w = vc * den;
#pragma unroll
        for (int k = 0; k < 3; ++k) cp[k] = (a[k] + ab[k] * v) + ac[k] * w;
    } while (false);
    return dist2(q, cp);
}

// ---- the search -------------------------------------------------------------------------------------------------------------------------
struct Faces { const int* ids; const double* tri; };       // face ids in cell order, the corner table

// the nearest face so far: (d2 as computed, face), the lower face on equal d2 -- a function of the input alone
struct FaceBest {
    double d2;
    int face;
    double tol[3];      // the walk's per-axis margin, for the box test
    __device__ __forceinline__ double bound() const { return d2; }
    __device__ __forceinline__ void visit(const Faces& fc, i64 s, i64 e, const double (&q)[3]) {
#pragma nounroll
        for (i64 p = s; p < e; ++p) {
            const int f = fc.ids[p];
            const double* t = fc.tri + 9 * (i64)f;
            double lb = 0.0;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double lo = fmin(fmin(t[a], t[3 + a]), t[6 + a]), hi = fmax(fmax(t[a], t[3 + a]), t[6 + a]);
                const double g = fmax(fmax(lo - q[a], q[a] - hi) - tol[a], 0.0);
                lb += g * g;
            }
            if (beyond(lb, d2)) continue;
            double cp[3];
            const double d = face_closest(t, q, cp);
            if (d < d2 || (d == d2 && f < face)) { d2 = d; face = f; }
        }
    }
};

template <bool QF64>
__global__ __launch_bounds__(256) void k_mesh_query(const void* __restrict__ q, i64 nq, const u32* __restrict__ order, Grid g,
                                                    const i64* __restrict__ start, const int* __restrict__ ids, const double* __restrict__ tri,
                                                    double* __restrict__ out_dist, int* __restrict__ out_face, double* __restrict__ out_closest) {
    const i64 s = (i64)blockIdx.x * 256 + threadIdx.x;
    if (s >= nq) return;
    const u32 qi = order[s];
    double qv[3];
    pb3d_load3<QF64>(q, qi, qv);
    FaceBest best = {INFINITY, kNoFace, {0.0, 0.0, 0.0}};
#pragma unroll
    for (int a = 0; a < 3; ++a) best.tol[a] = 1e-12 * (fabs(g.lo[a]) + fabs(g.hi[a]) + fabs(qv[a]));
    const Faces fc = {ids, tri};
    ring_walk(g, start, fc, qv, best);
    const bool found = best.face != kNoFace;        // false only for a query that is not finite (no d2 compares below infinity)
    out_dist[qi] = __dsqrt_rn(best.d2);
    if (out_face) out_face[qi] = found ? best.face : -1;
    if (out_closest) {
        double cp[3] = {NAN, NAN, NAN};
        if (found) face_closest(tri + 9 * (i64)best.face, qv, cp);
        out_closest[3 * (i64)qi] = cp[0]; out_closest[3 * (i64)qi + 1] = cp[1]; out_closest[3 * (i64)qi + 2] = cp[2];
    }
}

// ---- sampling ---------------------------------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ u64 mix64(u64 x) { return pb3d_mix64(x + 0x9e3779b97f4a7c15ull); }
// r_j(i) in [0, 1): 53 bits
__device__ __forceinline__ double unit_random(u64 key, u64 i, u64 j) { return (double)(mix64(key + 3 * i + j) >> 11) * 0x1p-53; }

template <bool VF64, bool I64>
__global__ __launch_bounds__(256) void k_face_area(const void* __restrict__ verts, i64 nv, const void* __restrict__ faces, i64 nf,
                                                   double* __restrict__ area) {
    const i64 f = (i64)blockIdx.x * 256 + threadIdx.x;
    if (f >= nf) return;
    double t[9];
    load_face<VF64, I64>(verts, nv, faces, f, t);
    double ab[3], ac[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { ab[k] = t[3 + k] - t[k]; ac[k] = t[6 + k] - t[k]; }
    const double n0 = ab[1] * ac[2] - ab[2] * ac[1], n1 = ab[2] * ac[0] - ab[0] * ac[2], n2 = ab[0] * ac[1] - ab[1] * ac[0];
    area[f] = 0.5 * __dsqrt_rn((n0 * n0 + n1 * n1) + n2 * n2);
}

// one lane per block of kPrefixBlock faces: the running sum, left to right from the block's first area, in place; the block's total
__global__ __launch_bounds__(64) void k_prefix_local(double* __restrict__ cum, i64 nf, double* __restrict__ block_total) {
    const i64 b = (i64)blockIdx.x * 64 + threadIdx.x;
    const i64 f0 = b * kPrefixBlock;
    if (f0 >= nf) return;
    const i64 f1 = f0 + kPrefixBlock < nf ? f0 + kPrefixBlock : nf;
    double acc = cum[f0];
    for (i64 f = f0 + 1; f < f1; ++f) {
        acc = acc + cum[f];
        cum[f] = acc;
    }
    block_total[b] = acc;
}

// one lane: block totals -> block offsets O_b, the running sum of the totals before b, O_0 = 0
__global__ __launch_bounds__(64) void k_prefix_blocks(double* __restrict__ block, i64 nblocks) {
    if (blockIdx.x || threadIdx.x) return;
    double acc = 0.0;
    for (i64 b = 0; b < nblocks; ++b) {
        const double t = block[b];
        block[b] = acc;
        acc = acc + t;
    }
}

__global__ __launch_bounds__(256) void k_prefix_add(double* __restrict__ cum, i64 nf, const double* __restrict__ block) {
    const i64 f = (i64)blockIdx.x * 256 + threadIdx.x;
    if (f < nf) cum[f] = block[f / kPrefixBlock] + cum[f];
}

template <bool VF64, bool I64>
__global__ __launch_bounds__(256) void k_mesh_sample(const void* __restrict__ verts, i64 nv, const void* __restrict__ faces, i64 nf,
                                                     const double* __restrict__ cum, double total, i64 n, u64 key, double* __restrict__ pts,
                                                     int* __restrict__ out_face) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double r0 = unit_random(key, (u64)i, 0), r1 = unit_random(key, (u64)i, 1), r2 = unit_random(key, (u64)i, 2);
    const double u = __ddiv_rn((double)i + r0, (double)n) * total;
    i64 lo = 0, hi = nf;        // the smallest f with cum[f] > u
    while (lo < hi) {
        const i64 mid = lo + ((hi - lo) >> 1);
        if (cum[mid] > u) hi = mid;
        else lo = mid + 1;
    }
    const i64 f = lo < nf - 1 ? lo : nf - 1;
    double t[9];
    load_face<VF64, I64>(verts, nv, faces, f, t);
    const double s = __dsqrt_rn(r1);
    const double wa = 1.0 - s, wb = s * (1.0 - r2), wc = s * r2;
#pragma unroll
    for (int k = 0; k < 3; ++k) pts[3 * i + k] = (t[k] * wa + t[3 + k] * wb) + t[6 + k] * wc;
    if (out_face) out_face[i] = (int)f;
}

int require_mesh(const char* what, const void* d_verts, i64 nv, const void* d_faces, i64 nf) {
    PB3D_REQUIRE(nv >= 0 && nf >= 0, "%s: negative count", what);
    PB3D_REQUIRE(nv <= pb3d_max_points && nf <= pb3d_max_points, "%s: at most 2^31 - 1 vertices and faces", what);
    PB3D_REQUIRE(nf >= 1 && nv >= 1, "%s: the mesh needs at least one face and one vertex (got %lld faces, %lld vertices)", what, (long long)nf,
                 (long long)nv);
    PB3D_REQUIRE(d_verts != nullptr && d_faces != nullptr, "%s: null buffer", what);
    return PB3D_OK;
}

}  // namespace

extern "C" {

int pb3d_mesh_dist_resident(pb3d_ctx* ctx, const void* d_q, int q_f64, int64_t nq, const void* d_verts, int verts_f64, int64_t nv,
                            const void* d_faces, int faces_i64, int64_t nf, double* d_dist, int32_t* d_face, double* d_closest) {
    PB3D_REQUIRE(nq >= 0 && nq <= pb3d_max_points, "pb3d_mesh_dist: need 0 <= nq <= 2^31 - 1 queries (got %lld)", (long long)nq);
    if (nq == 0) return PB3D_OK;
    PB3D_TRY(require_mesh("pb3d_mesh_dist", d_verts, nv, d_faces, nf));
    PB3D_REQUIRE(d_q != nullptr && d_dist != nullptr, "pb3d_mesh_dist: null buffer");
    PB3D_REQUIRE(ctx != nullptr, "pb3d_mesh_dist: null context");
    PB3D_TRY(pb3d_check_index_range(ctx, d_faces, faces_i64, 3 * nf, -nv, nv, "pb3d_mesh_dist"));
    const pb3d_face_index_slots slots = {PB3D_SLOT_MESHD_CORNERS, PB3D_SLOT_MESHD_READBACK, PB3D_SLOT_MESHD_COUNTS, PB3D_SLOT_MESHD_STARTS,
                                         PB3D_SLOT_MESHD_IDS, PB3D_SLOT_MESHD_SCAN_LOCAL, PB3D_SLOT_MESHD_SCAN_SEGS};
    pb3d_face_index ix;
    const u32* order;
    PB3D_TRY(pb3d_face_index_build(ctx, "pb3d_mesh_dist", d_verts, verts_f64, nv, d_faces, faces_i64, nf, 3, false, nullptr, slots, &ix));
    ctx->mesh_grid_last = {true, {ix.g.n[0], ix.g.n[1], ix.g.n[2]}, ix.entries, ix.coarsenings};
    PB3D_TRY(pb3d_nn_order_queries(ctx, d_q, q_f64, nq, ix.g, &order));
    hipLaunchKernelGGL((q_f64 ? k_mesh_query<true> : k_mesh_query<false>), dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, ctx->stream, d_q,
                       (i64)nq, order, ix.g, ix.starts, ix.ids, ix.tri, d_dist, (int*)d_face, d_closest);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

int pb3d_mesh_grid_shape(const pb3d_ctx* ctx, int64_t cells[3], int64_t* entries, int64_t* coarsenings) {
    PB3D_REQUIRE(ctx != nullptr && cells != nullptr && entries != nullptr, "pb3d_mesh_grid_shape: null argument");
    PB3D_REQUIRE(ctx->mesh_grid_last.valid, "pb3d_mesh_grid_shape: no pb3d_mesh_dist_resident call has built an index on this context");
    for (int a = 0; a < 3; ++a) cells[a] = ctx->mesh_grid_last.cells[a];
    *entries = ctx->mesh_grid_last.entries;
    if (coarsenings) *coarsenings = ctx->mesh_grid_last.coarsenings;
    return PB3D_OK;
}

int pb3d_mesh_sample_resident(pb3d_ctx* ctx, const void* d_verts, int verts_f64, int64_t nv, const void* d_faces, int faces_i64, int64_t nf,
                              int64_t n, uint64_t seed, double* d_pts, int32_t* d_face) {
    PB3D_REQUIRE(n >= 0 && n <= pb3d_max_points, "pb3d_mesh_sample: need 0 <= n <= 2^31 - 1 samples (got %lld)", (long long)n);
    if (n == 0) return PB3D_OK;
    PB3D_TRY(require_mesh("pb3d_mesh_sample", d_verts, nv, d_faces, nf));
    PB3D_REQUIRE(d_pts != nullptr, "pb3d_mesh_sample: null buffer");
    PB3D_REQUIRE(ctx != nullptr, "pb3d_mesh_sample: null context");
    PB3D_TRY(pb3d_check_index_range(ctx, d_faces, faces_i64, 3 * nf, -nv, nv, "pb3d_mesh_sample"));
    const i64 nblocks = (nf + kPrefixBlock - 1) / kPrefixBlock;
    void *cum, *blk;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_MSAMPLE_CUM, (size_t)nf * sizeof(double), &cum));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_MSAMPLE_BLOCKS, (size_t)nblocks * sizeof(double), &blk));
    with_mesh_types(verts_f64, faces_i64, [&](auto V, auto I) {
        hipLaunchKernelGGL((k_face_area<decltype(V)::value, decltype(I)::value>), dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, ctx->stream,
                           d_verts, (i64)nv, d_faces, (i64)nf, (double*)cum);
    });
    PB3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_prefix_local, dim3((unsigned)((nblocks + 63) / 64)), dim3(64), 0, ctx->stream, (double*)cum, (i64)nf, (double*)blk);
    PB3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_prefix_blocks, dim3(1), dim3(64), 0, ctx->stream, (double*)blk, nblocks);
    PB3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_prefix_add, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, ctx->stream, (double*)cum, (i64)nf, (const double*)blk);
    PB3D_CHECK_LAUNCH();
    double total;
    PB3D_TRY(pb3d_read_back(ctx, &total, (const double*)cum + (nf - 1), sizeof(total)));
    PB3D_REQUIRE(std::isfinite(total) && total > 0.0, "pb3d_mesh_sample: the mesh's total area must be finite and positive (got %g)", total);
    with_mesh_types(verts_f64, faces_i64, [&](auto V, auto I) {
        hipLaunchKernelGGL((k_mesh_sample<decltype(V)::value, decltype(I)::value>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream,
                           d_verts, (i64)nv, d_faces, (i64)nf, (const double*)cum, total, (i64)n, mix64(seed), d_pts, (int*)d_face);
    });
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

}  // extern "C"
