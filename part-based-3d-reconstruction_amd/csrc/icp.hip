// Rigid ICP of two point clouds, the device half: transform, exact nearest target point, and the 16 float64 sums a point-to-point step
// needs (include/pb3d.h has the semantics to the bit; pb3d/preprocess_helpers.py runs the 3 x 3 solve and the loop on the host).
//
// An alignment bins its target ONCE (pb3d_icp_index_resident -> pb3d_nn_index_build of csrc/nn.hip: exact box, cell counts, scan, cell-
// sorted SoA coordinates and ids in the PB3D_SLOT_ICP_INDEX_* slots, one host wait) and then runs any number of steps against it.  A step
//   k_icp_transform   p = T s in float64, the source widened first                         -> PB3D_SLOT_ICP_MOVED
//   the search        pb3d_nn_index_nearest: bins the moved points (only the query side of the index changes between steps) and runs
//                     k_knn_query<8> with k = 1: the position j of the target point with the smallest (d2, j) -> PB3D_SLOT_ICP_NEAREST
//   k_icp_terms       one point per thread in the ORIGINAL order, 256 consecutive points per workgroup: gathers target row j, forms the
//                     16 terms (+0.0 for a pair the gate rejects and for the lanes past the end) and reduces them to one partial row
//                     per workgroup                                                        -> PB3D_SLOT_ICP_PARTIALS
//   pb3d_k_rows_final one 256-thread workgroup: thread t adds partial rows t, t + 256, ... in ascending order, then the same reduction
//                     (csrc/reduce_rows.h, shared with csrc/plane.hip)
// and nothing waits for the host.  The summation order is a function of (ns, point index) alone: no floating-point atomics, and the
// cell-sorted query order of the search (free within a cell) never reaches a sum, because the terms are formed from the index array in
// the caller's order.  The Makefile passes -ffp-contract=off: every product and sum below is one rounded operation.
#include <cmath>

#include "pb3d_internal.h"
#include "reduce_rows.h"

namespace {

constexpr int kSums = 16;
constexpr int kRow = kSums + 1;              // a partial row and the result: the int64 count, then the 16 float64 sums

struct Xf { double t[12]; };                 // row-major 3 x 4 [R | t]
struct Pivots { double cp[3], cq[3]; };

template <bool F64>
__global__ __launch_bounds__(256) void k_icp_transform(const void* __restrict__ src, i64 n, Xf T, double* __restrict__ out) {
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) {
        double x, y, z;
        pb3d_load3<F64>(src, i, &x, &y, &z);
#pragma unroll
        for (int h = 0; h < 3; ++h) out[3 * i + h] = ((T.t[4 * h] * x + T.t[4 * h + 1] * y) + T.t[4 * h + 2] * z) + T.t[4 * h + 3];
    }
}

template <bool TF64>
__global__ __launch_bounds__(256) void k_icp_terms(const double* __restrict__ moved, const int* __restrict__ nearest, i64 ns,
                                                   const void* __restrict__ tgt, i64 nt, double max_dist2, Pivots pv, double* __restrict__ part) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    double v[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) v[c] = 0.0;
    i64 cnt = 0;
    if (i < ns) {
        const i64 j = nearest[i];
        if (j >= 0 && j < nt) {                 // a moved point that is not finite found nobody: not used (and nothing is gathered)
            const double p[3] = {moved[3 * i], moved[3 * i + 1], moved[3 * i + 2]};
            double q[3];
            pb3d_load3<TF64>(tgt, j, q);
            const double dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            if (max_dist2 < 0.0 || d2 <= max_dist2) {
                double P[3], Q[3];
#pragma unroll
                for (int a = 0; a < 3; ++a) { P[a] = p[a] - pv.cp[a]; Q[a] = q[a] - pv.cq[a]; }
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    v[a] = P[a];
                    v[3 + a] = Q[a];
#pragma unroll
                    for (int b = 0; b < 3; ++b) v[6 + 3 * a + b] = P[a] * Q[b];
                }
                v[15] = d2;
                cnt = 1;
            }
        }
    }
    pb3d_reduce_row<kSums>(v, cnt, part + (i64)blockIdx.x * kRow);
}

int launch_transform(pb3d_ctx* ctx, const void* d_src, int f64, i64 n, const double T[12], double* d_out) {
    Xf x;
    memcpy(x.t, T, sizeof(x.t));
    const dim3 grid(pb3d_stream_blocks(ctx, n, 256, 8));
    if (f64) hipLaunchKernelGGL(k_icp_transform<true>, grid, dim3(256), 0, ctx->stream, d_src, n, x, d_out);
    else hipLaunchKernelGGL(k_icp_transform<false>, grid, dim3(256), 0, ctx->stream, d_src, n, x, d_out);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

const pb3d_slot kIndexSlots[3] = {PB3D_SLOT_ICP_INDEX_STARTS, PB3D_SLOT_ICP_INDEX_COORDS, PB3D_SLOT_ICP_INDEX_IDS};

}  // namespace

extern "C" {

int pb3d_transform_points_resident(pb3d_ctx* ctx, const void* d_src, int src_f64, int64_t n, const double T[12], double* d_out) {
    PB3D_REQUIRE(n >= 0 && n <= pb3d_max_points, "pb3d_transform_points: need 0 <= n <= 2^31 - 1 points (got %lld)", (long long)n);
    PB3D_REQUIRE(T != nullptr, "pb3d_transform_points: null transform");
    if (n == 0) return PB3D_OK;
    PB3D_REQUIRE(d_src != nullptr && d_out != nullptr, "pb3d_transform_points: null buffer");
    PB3D_REQUIRE(ctx != nullptr, "pb3d_transform_points: null context");
    return launch_transform(ctx, d_src, src_f64, n, T, d_out);
}

int pb3d_icp_index_resident(pb3d_ctx* ctx, const void* d_tgt, int tgt_f64, int64_t nt, double bounds[6]) {
    PB3D_REQUIRE(nt >= 1 && nt <= pb3d_max_points, "pb3d_icp_index: need 1 <= nt <= 2^31 - 1 target points (got %lld)", (long long)nt);
    PB3D_REQUIRE(d_tgt != nullptr, "pb3d_icp_index: null buffer");
    PB3D_REQUIRE(ctx != nullptr, "pb3d_icp_index: null context");
    pb3d_ctx::IcpIndex& ii = ctx->icp_index;
    ii.valid = false;
    PB3D_TRY(pb3d_nn_index_build(ctx, d_tgt, tgt_f64, nt, kIndexSlots[0], kIndexSlots[1], kIndexSlots[2], &ii.ix));
    ii.tgt = d_tgt;
    ii.nt = nt;
    ii.f64 = tgt_f64 ? 1 : 0;
    for (int s = 0; s < 3; ++s) ii.gen[s] = ctx->scratch_slot_gen[kIndexSlots[s]];
    ii.valid = true;
    if (bounds)
        for (int a = 0; a < 3; ++a) { bounds[a] = ii.ix.g.lo[a]; bounds[3 + a] = ii.ix.g.hi[a]; }
    return PB3D_OK;
}

int pb3d_icp_step_resident(pb3d_ctx* ctx, const void* d_src, int src_f64, int64_t ns, const void* d_tgt, int tgt_f64, int64_t nt,
                           const double T[12], double max_dist2, const double cp[3], const double cq[3], void* d_out) {
    PB3D_REQUIRE(ns >= 0 && nt >= 0, "pb3d_icp_step: negative point count");
    PB3D_REQUIRE(ns <= pb3d_max_points && nt <= pb3d_max_points, "pb3d_icp_step: at most 2^31 - 1 points per set");
    PB3D_REQUIRE(T != nullptr && cp != nullptr && cq != nullptr && d_out != nullptr, "pb3d_icp_step: null argument");
    PB3D_REQUIRE(max_dist2 == max_dist2, "pb3d_icp_step: the squared gate is NaN");
    PB3D_REQUIRE(ns == 0 || nt >= 1, "pb3d_icp_step: the target is empty");
    PB3D_REQUIRE(ns == 0 || (d_src != nullptr && d_tgt != nullptr), "pb3d_icp_step: null buffer");
    PB3D_REQUIRE(ctx != nullptr, "pb3d_icp_step: null context");
    if (ns == 0) {
        PB3D_HIP(hipMemsetAsync(d_out, 0, kRow * 8, ctx->stream));
        return PB3D_OK;
    }
    const pb3d_ctx::IcpIndex& ii = ctx->icp_index;
    bool live = ii.valid && ii.tgt == d_tgt && ii.nt == nt && ii.f64 == (tgt_f64 ? 1 : 0);
    for (int s = 0; s < 3; ++s) live = live && ii.gen[s] == ctx->scratch_slot_gen[kIndexSlots[s]];
    PB3D_REQUIRE(live, "pb3d_icp_step: the target index is gone or was built for another target; call pb3d_icp_index_resident first");
    const i64 nrows = (ns + 255) / 256;
    void *moved, *nearest, *part;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_ICP_MOVED, (size_t)ns * 3 * sizeof(double), &moved));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_ICP_NEAREST, (size_t)ns * sizeof(int), &nearest));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_ICP_PARTIALS, (size_t)nrows * kRow * 8, &part));
    PB3D_TRY(launch_transform(ctx, d_src, src_f64, ns, T, (double*)moved));
    PB3D_TRY(pb3d_nn_index_nearest(ctx, ii.ix, (const double*)moved, ns, (int*)nearest));
    Pivots pv;
    memcpy(pv.cp, cp, sizeof(pv.cp));
    memcpy(pv.cq, cq, sizeof(pv.cq));
    if (tgt_f64) hipLaunchKernelGGL(k_icp_terms<true>, dim3((unsigned)nrows), dim3(256), 0, ctx->stream, (const double*)moved, (const int*)nearest,
                                    (i64)ns, d_tgt, (i64)nt, max_dist2, pv, (double*)part);
    else hipLaunchKernelGGL(k_icp_terms<false>, dim3((unsigned)nrows), dim3(256), 0, ctx->stream, (const double*)moved, (const int*)nearest,
                            (i64)ns, d_tgt, (i64)nt, max_dist2, pv, (double*)part);
    PB3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(pb3d_k_rows_final<kSums>, dim3(1), dim3(256), 0, ctx->stream, (const double*)part, nrows, (double*)d_out);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

}  // extern "C"
