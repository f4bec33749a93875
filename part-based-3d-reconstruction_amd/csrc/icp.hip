// Rigid ICP of two point clouds, the device half: transform, exact nearest target point, and the 16 (trimmed: 17) float64 sums a
// point-to-point step needs, or the 29 of a point-to-plane step (include/pb3d.h has the semantics to the bit; pb3d/preprocess_helpers.py runs the 3 x 3 solve and the
// loop on the host).
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
// and nothing waits for the host.  A TRIMMED step (pb3d_icp_step_trimmed_resident) puts three things between the search and the terms:
//   k_icp_keys        one point per thread: d2 of a candidate pair, the sentinel NaN of any other, and the candidate count m
//   k_icp_rank        k from m and the trim fraction, on the device                       } -> PB3D_SLOT_ICP_KEYS (header, then keys)
//   pb3d_select_kth   tau = the k-th smallest key (csrc/select.hip), its rank read from the header
// and its terms kernel (the same template, 17 sums) uses the candidates with d2 <= tau.  A POINT-TO-PLANE step
// (pb3d_icp_step_plane_resident) is the same chain with another set of terms: the kernel also gathers row j of the target's float64
// normals and forms the 29 terms of the 6 x 6 normal equations (the upper triangle of J J^T, J r, r r, d2); its trim is optional.
// The summation order is a function of (ns, point index) alone: no floating-point atomics, and the cell-sorted query order of the
// search (free within a cell) never reaches a sum, because the terms are formed from the index array in the caller's order.  The
// Makefile passes -ffp-contract=off: every product and sum below is one rounded operation.
#include <cmath>

#include "pb3d_internal.h"
#include "wave.h"
#include "reduce_rows.h"

namespace {

constexpr int kSums = 16;
constexpr int kPlaneSums = 29;

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

// the pair of point i: p = the moved point, q = its nearest target point, d2 = the search's own expression.  true when the pair is a
// CANDIDATE: j valid (a moved point with a NaN found nobody, and nothing is gathered for it) and the gate passes.  FINITE (the trimmed
// step): a moved point with an infinite coordinate is no candidate either -- the search pairs it at d2 = +inf, which the plain step
// has always left to its gate
template <bool TF64, bool FINITE>
__device__ __forceinline__ bool icp_pair(const double* __restrict__ moved, const int* __restrict__ nearest, i64 i, const void* __restrict__ tgt, i64 nt,
                                         double max_dist2, double p[3], double q[3], double* d2) {
    const i64 j = nearest[i];
    if (j < 0 || j >= nt) return false;
    p[0] = moved[3 * i]; p[1] = moved[3 * i + 1]; p[2] = moved[3 * i + 2];
    if (FINITE && !(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]))) return false;
    pb3d_load3<TF64>(tgt, j, q);
    const double dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
    *d2 = (dx * dx + dy * dy) + dz * dz;
    return max_dist2 < 0.0 || *d2 <= max_dist2;
}

// what a trimmed step keeps on the device in front of its keys (PB3D_SLOT_ICP_KEYS)
struct TrimHeader {
    i64 m;                    // candidates, counted by k_icp_keys
    i64 rank;                 // k - 1 (0 when m = 0), from k_icp_rank
    double tau;               // the selection's result (a sentinel NaN when m = 0: read through trim_tau)
    i64 pad;
};
constexpr u64 kNotCandidate = 0x7FF8000000000000ull;      // sorts above every candidate, +inf included
__device__ __forceinline__ double trim_tau(const TrimHeader* h) { return h->m == 0 ? 0.0 : h->tau; }

// one point per thread: the selection key of its pair (d2 of a candidate, else the sentinel) and the number of candidates
template <bool TF64>
__global__ __launch_bounds__(256) void k_icp_keys(const double* __restrict__ moved, const int* __restrict__ nearest, i64 ns,
                                                  const void* __restrict__ tgt, i64 nt, double max_dist2, TrimHeader* __restrict__ hdr,
                                                  u64* __restrict__ keys) {
    __shared__ int wc[4];
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    bool cand = false;
    if (i < ns) {
        double p[3], q[3], d2 = 0.0;
        cand = icp_pair<TF64, true>(moved, nearest, i, tgt, nt, max_dist2, p, q, &d2);
        keys[i] = cand ? (u64)__double_as_longlong(d2) : kNotCandidate;
    }
    group_total<4>((int)__popcll(__ballot(cand)), wc, [&](int tot) {
        if (tot) atomicAdd((unsigned long long*)&hdr->m, (unsigned long long)tot);      // integer: exact in any order
    });
}

// k = (rho >= 1) ? m : min(m, ceil(rho * m)): one rounded product, then ceil; the selection's rank is k - 1
__global__ void k_icp_rank(TrimHeader* __restrict__ hdr, double rho) {
    const i64 m = hdr->m;
    i64 k = m;
    if (!(rho >= 1.0)) {
        const double c = ceil(rho * (double)m);
        k = c < (double)m ? (i64)c : m;
    }
    hdr->rank = k > 0 ? k - 1 : 0;
}

// W = 16: the plain step.  TAU: a trimmed step -- a candidate is used when d2 <= tau, there is a 17th term |P|^2, and workgroup 0
// writes the candidate count and tau behind the 18 words of the final row pass.  PLANE (W = 29): the point-to-plane terms from row j
// of nrm, pivot pv.cp; the two words behind the row are always written (0 and +0.0 without TAU)
template <bool TF64, int W, bool TAU, bool PLANE>
__global__ __launch_bounds__(256) void k_icp_terms(const double* __restrict__ moved, const int* __restrict__ nearest, i64 ns,
                                                   const void* __restrict__ tgt, i64 nt, double max_dist2, Pivots pv, const TrimHeader* __restrict__ hdr,
                                                   const double* __restrict__ nrm, double* __restrict__ part, double* __restrict__ out) {
    static_assert(W == (PLANE ? kPlaneSums : TAU ? 17 : 16), "the point-to-plane step has 29 sums, the trimmed step 17, the plain step 16");
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    double v[W];
#pragma unroll
    for (int c = 0; c < W; ++c) v[c] = 0.0;
    i64 cnt = 0;
    double tau = 0.0;
    if (TAU) tau = trim_tau(hdr);
    if ((TAU || PLANE) && i == 0) {
        ((i64*)out)[W + 1] = TAU ? hdr->m : 0;
        out[W + 2] = tau;
    }
    if (i < ns) {
        double p[3], q[3], d2 = 0.0;
        if (icp_pair<TF64, TAU>(moved, nearest, i, tgt, nt, max_dist2, p, q, &d2) && (!TAU || d2 <= tau)) {
            double P[3], Q[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) { P[a] = p[a] - pv.cp[a]; Q[a] = q[a] - pv.cq[a]; }
            if (PLANE) {
                const double* n = nrm + 3 * (i64)nearest[i];
                const double dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];       // the differences d2 was formed from
                const double r = (dx * n[0] + dy * n[1]) + dz * n[2];
                const double J[6] = {P[1] * n[2] - P[2] * n[1], P[2] * n[0] - P[0] * n[2], P[0] * n[1] - P[1] * n[0], n[0], n[1], n[2]};
                int c = 0;
#pragma unroll
                for (int a = 0; a < 6; ++a)
#pragma unroll
                    for (int b = a; b < 6; ++b) v[c++] = J[a] * J[b];
#pragma unroll
                for (int a = 0; a < 6; ++a) v[21 + a] = J[a] * r;
                v[27] = r * r;
                v[28] = d2;
            } else {
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    v[a] = P[a];
                    v[3 + a] = Q[a];
#pragma unroll
                    for (int b = 0; b < 3; ++b) v[6 + 3 * a + b] = P[a] * Q[b];
                }
                v[15] = d2;
                if (TAU) v[W - 1] = (P[0] * P[0] + P[1] * P[1]) + P[2] * P[2];
            }
            cnt = 1;
        }
    }
    pb3d_reduce_row<W>(v, cnt, part + (i64)blockIdx.x * (W + 1));
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


// the argument checks of both step entries, before the context check (the refusals can be tested without a device)
int step_args(const pb3d_ctx* ctx, const char* who, const void* d_src, i64 ns, const void* d_tgt, i64 nt, const double* T, double max_dist2,
              const double* cp, const double* cq, const void* d_out) {
    PB3D_REQUIRE(ns >= 0 && nt >= 0, "%s: negative point count", who);
    PB3D_REQUIRE(ns <= pb3d_max_points && nt <= pb3d_max_points, "%s: at most 2^31 - 1 points per set", who);
    PB3D_REQUIRE(T != nullptr && cp != nullptr && cq != nullptr && d_out != nullptr, "%s: null argument", who);
    PB3D_REQUIRE(max_dist2 == max_dist2, "%s: the squared gate is NaN", who);
    PB3D_REQUIRE(ns == 0 || nt >= 1, "%s: the target is empty", who);
    PB3D_REQUIRE(ns == 0 || (d_src != nullptr && d_tgt != nullptr), "%s: null buffer", who);
    PB3D_REQUIRE(ctx != nullptr, "%s: null context", who);
    return PB3D_OK;
}

// transform, search, [keys, rank, selection,] terms, final row pass.  TRIM: 17 sums and the two words behind them.  PLANE: the 29
// point-to-plane sums against the normals d_nrm, the two words always, the selection only with TRIM
template <bool TRIM, bool PLANE>
int run_step(pb3d_ctx* ctx, const char* who, const void* d_src, int src_f64, i64 ns, const void* d_tgt, int tgt_f64, i64 nt, const double* d_nrm,
             const double T[12], double max_dist2, double rho, const double cp[3], const double cq[3], void* d_out) {
    constexpr int W = PLANE ? kPlaneSums : TRIM ? kSums + 1 : kSums;
    if (ns == 0) {
        PB3D_HIP(hipMemsetAsync(d_out, 0, (W + 1 + (TRIM || PLANE ? 2 : 0)) * 8, ctx->stream));
        return PB3D_OK;
    }
    const pb3d_ctx::IcpIndex& ii = ctx->icp_index;
    bool live = ii.valid && ii.tgt == d_tgt && ii.nt == nt && ii.f64 == (tgt_f64 ? 1 : 0);
    for (int s = 0; s < 3; ++s) live = live && ii.gen[s] == ctx->scratch_slot_gen[kIndexSlots[s]];
    PB3D_REQUIRE(live, "%s: the target index is gone or was built for another target; call pb3d_icp_index_resident first", who);
    const i64 nrows = (ns + 255) / 256;
    void *moved, *nearest, *part, *keybuf = nullptr;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_ICP_MOVED, (size_t)ns * 3 * sizeof(double), &moved));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_ICP_NEAREST, (size_t)ns * sizeof(int), &nearest));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_ICP_PARTIALS, (size_t)nrows * (W + 1) * 8, &part));
    if (TRIM) PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_ICP_KEYS, sizeof(TrimHeader) + (size_t)ns * 8, &keybuf));
    PB3D_TRY(launch_transform(ctx, d_src, src_f64, ns, T, (double*)moved));
    PB3D_TRY(pb3d_nn_index_nearest(ctx, ii.ix, (const double*)moved, ns, (int*)nearest));
    Pivots pv;
    memcpy(pv.cp, cp, sizeof(pv.cp));
    memcpy(pv.cq, cq, sizeof(pv.cq));
    TrimHeader* hdr = (TrimHeader*)keybuf;
    const dim3 grid((unsigned)nrows), wg(256);
    if (TRIM) {
        u64* keys = (u64*)(hdr + 1);
        PB3D_HIP(hipMemsetAsync(hdr, 0, sizeof(TrimHeader), ctx->stream));
        if (tgt_f64) hipLaunchKernelGGL(k_icp_keys<true>, grid, wg, 0, ctx->stream, (const double*)moved, (const int*)nearest, ns, d_tgt, nt, max_dist2, hdr, keys);
        else hipLaunchKernelGGL(k_icp_keys<false>, grid, wg, 0, ctx->stream, (const double*)moved, (const int*)nearest, ns, d_tgt, nt, max_dist2, hdr, keys);
        PB3D_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_icp_rank, dim3(1), dim3(1), 0, ctx->stream, hdr, rho);
        PB3D_CHECK_LAUNCH();
        PB3D_TRY(pb3d_select_kth(ctx, (const double*)keys, ns, &hdr->rank, &hdr->tau));
    }
    if (tgt_f64) hipLaunchKernelGGL((k_icp_terms<true, W, TRIM, PLANE>), grid, wg, 0, ctx->stream, (const double*)moved, (const int*)nearest, ns, d_tgt,
                                    nt, max_dist2, pv, (const TrimHeader*)hdr, d_nrm, (double*)part, (double*)d_out);
    else hipLaunchKernelGGL((k_icp_terms<false, W, TRIM, PLANE>), grid, wg, 0, ctx->stream, (const double*)moved, (const int*)nearest, ns, d_tgt,
                            nt, max_dist2, pv, (const TrimHeader*)hdr, d_nrm, (double*)part, (double*)d_out);
    PB3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(pb3d_k_rows_final<W>, dim3(1), dim3(256), 0, ctx->stream, (const double*)part, nrows, (double*)d_out);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

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
    PB3D_TRY(step_args(ctx, "pb3d_icp_step", d_src, ns, d_tgt, nt, T, max_dist2, cp, cq, d_out));
    return run_step<false, false>(ctx, "pb3d_icp_step", d_src, src_f64, ns, d_tgt, tgt_f64, nt, nullptr, T, max_dist2, 1.0, cp, cq, d_out);
}

int pb3d_icp_step_trimmed_resident(pb3d_ctx* ctx, const void* d_src, int src_f64, int64_t ns, const void* d_tgt, int tgt_f64, int64_t nt,
                                   const double T[12], double max_dist2, double trim_fraction, const double cp[3], const double cq[3],
                                   void* d_out) {
    PB3D_REQUIRE(trim_fraction > 0.0 && trim_fraction <= 1.0, "pb3d_icp_step_trimmed: the trim fraction must be in (0, 1] (got %g)", trim_fraction);
    PB3D_TRY(step_args(ctx, "pb3d_icp_step_trimmed", d_src, ns, d_tgt, nt, T, max_dist2, cp, cq, d_out));
    return run_step<true, false>(ctx, "pb3d_icp_step_trimmed", d_src, src_f64, ns, d_tgt, tgt_f64, nt, nullptr, T, max_dist2, trim_fraction, cp, cq,
                                 d_out);
}

int pb3d_icp_step_plane_resident(pb3d_ctx* ctx, const void* d_src, int src_f64, int64_t ns, const void* d_tgt, int tgt_f64, int64_t nt,
                                 const double* d_tgt_normals, const double T[12], double max_dist2, double trim_fraction, const double c[3],
                                 void* d_out) {
    const char* who = "pb3d_icp_step_plane";
    PB3D_REQUIRE(trim_fraction < 0.0 || (trim_fraction > 0.0 && trim_fraction <= 1.0),
                 "%s: the trim fraction must be in (0, 1], or negative for no trim (got %g)", who, trim_fraction);
    PB3D_REQUIRE(ns <= 0 || d_tgt_normals != nullptr, "%s: null buffer", who);
    PB3D_TRY(step_args(ctx, who, d_src, ns, d_tgt, nt, T, max_dist2, c, c, d_out));
    if (trim_fraction < 0.0)
        return run_step<false, true>(ctx, who, d_src, src_f64, ns, d_tgt, tgt_f64, nt, d_tgt_normals, T, max_dist2, 1.0, c, c, d_out);
    return run_step<true, true>(ctx, who, d_src, src_f64, ns, d_tgt, tgt_f64, nt, d_tgt_normals, T, max_dist2, trim_fraction, c, c, d_out);
}

}  // extern "C"
