// The facade-plane fit and the box crop of the inter-method preprocessing, the device half (include/pb3d.h has the semantics to the bit;
// pb3d/preprocess_helpers.py draws the triplets, picks the best hypothesis, runs the 3 x 3 eigen problem of a refit and builds the
// four-way completion from transform_points).
//   k_plane_hyp      one thread per hypothesis: gathers the three points of its triplet and writes (unit normal, d), or four NaNs
//   k_plane_score    RANSAC scoring, K planes against n resident points in ONE sweep of the points.  A workgroup of 256 lanes takes
//                    tiles of 1024 points, four per lane widened in registers, and walks the K plane rows at a wave-uniform address
//                    (scalar loads); per (plane, point slot) a ballot and a popcount accumulate in scalar registers, one lane adds
//                    the wave's count to a u32 table in the LDS, and after its last tile the workgroup flushes the non-zero entries
//                    with 64-bit integer atomics: the counts are exact and a function of the input alone.  6 float64 operations per
//                    (point, plane) against 12 or 24 bytes per point: bound by the vector FP64 rate, not by HBM.
//   k_plane_terms    a refit's 11 terms per point in the caller's order, reduced per workgroup of 256 consecutive points, then
//                    pb3d_k_rows_final<11> (csrc/reduce_rows.h: the summation order of the ICP step, no floating-point atomics)
//   k_crop_count / k_crop_fill   order-keeping stream compaction: survivors per 256 consecutive points, pb3d_scan_counts, and a fill
//                    that ranks a survivor by ballots (lower lanes of its wave + the lower waves of its workgroup).  One shell
//                    (compact_points) for every per-point predicate: the closed box of crop_to_box, the byte flags of select_points
// Nothing here waits for the host.  The Makefile passes -ffp-contract=off: every product and sum below is one rounded operation.
#include <algorithm>
#include <cmath>

#include "pb3d_internal.h"
#include "wave.h"
#include "reduce_rows.h"

namespace {

constexpr int kMaxPlanes = 4096;             // the LDS table of k_plane_score: 16 KB of u32
constexpr int kSums = 11;
constexpr int kRow = kSums + 1;              // a refit's partial row and result: the int64 count, then the 11 float64 sums
constexpr int kSlots = 4;                    // points per lane of a score tile
constexpr int kTile = 256 * kSlots;
constexpr int kScoreBlocksPerCu = 8;         // grid of k_plane_score: min(tiles, CUs * 8) workgroups, each walking tiles b, b + grid, ...
                                             // (8 x 16 KB of LDS and 8 waves per SIMD: 2.95 ms against 3.6 ms at 4 on 12 M points x 1024 planes)

struct Plane { double p[4]; };
struct Box { double lo[3], hi[3]; };
struct Pivot { double c[3]; };

template <bool F64>
__global__ __launch_bounds__(256) void k_plane_hyp(const void* __restrict__ pts, i64 n, const i64* __restrict__ trip, int K,
                                                   double* __restrict__ planes) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    const double nan = __builtin_nan("");
    double out[4] = {nan, nan, nan, nan};
    const i64 ia = trip[3 * k], ib = trip[3 * k + 1], ic = trip[3 * k + 2];
    if (ia >= 0 && ia < n && ib >= 0 && ib < n && ic >= 0 && ic < n) {        // nothing is gathered through an index outside [0, n)
        double a[3], b[3], c[3];
        pb3d_load3<F64>(pts, ia, a);
        pb3d_load3<F64>(pts, ib, b);
        pb3d_load3<F64>(pts, ic, c);
        const double ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2];
        const double vx = c[0] - a[0], vy = c[1] - a[1], vz = c[2] - a[2];
        const double wx = uy * vz - uz * vy, wy = uz * vx - ux * vz, wz = ux * vy - uy * vx;
        const double L = sqrt((wx * wx + wy * wy) + wz * wz);
        if (L > 0.0 && L <= 1.7976931348623157e308) {                         // finite and above 0 (a NaN fails both)
            const double nx = wx / L, ny = wy / L, nz = wz / L;
            out[0] = nx; out[1] = ny; out[2] = nz;
            out[3] = -((nx * a[0] + ny * a[1]) + nz * a[2]);
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) planes[4 * (i64)k + c] = out[c];
}

template <bool F64>
__global__ __launch_bounds__(256) void k_plane_score(const void* __restrict__ pts, i64 n, const double* __restrict__ planes, int K, int kchunk,
                                                     double tau, unsigned long long* __restrict__ counts) {
    __shared__ u32 tbl[kMaxPlanes];
    const int k0 = blockIdx.y * kchunk, k1 = min(K, k0 + kchunk);              // this workgroup's plane rows
    for (int k = k0 + threadIdx.x; k < k1; k += 256) tbl[k] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const i64 ntiles = (n + kTile - 1) / kTile;
    const double nan = __builtin_nan("");
    for (i64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        double x[kSlots], y[kSlots], z[kSlots];
#pragma unroll
        for (int s = 0; s < kSlots; ++s) {
            const i64 i = tile * kTile + s * 256 + threadIdx.x;
            x[s] = y[s] = z[s] = nan;                                          // a slot past the end is never an inlier
            if (i < n) pb3d_load3<F64>(pts, i, &x[s], &y[s], &z[s]);
        }
        for (int k = k0; k < k1; ++k) {                                        // k is wave-uniform: the row comes through the scalar path
            const double a = planes[4 * k], b = planes[4 * k + 1], c = planes[4 * k + 2], d = planes[4 * k + 3];
            u32 cnt = 0;
#pragma unroll
            for (int s = 0; s < kSlots; ++s) {
                const double r = ((a * x[s] + b * y[s]) + c * z[s]) + d;
                cnt += (u32)__popcll(__ballot(fabs(r) <= tau));
            }
            if (lane == 0 && cnt) atomicAdd(&tbl[k], cnt);
        }
    }
    __syncthreads();
    for (int k = k0 + threadIdx.x; k < k1; k += 256) {
        const u32 c = tbl[k];
        if (c) atomicAdd(&counts[k], (unsigned long long)c);
    }
}

template <bool F64>
__global__ __launch_bounds__(256) void k_plane_terms(const void* __restrict__ pts, i64 n, Plane pl, double tau, Pivot pv, double* __restrict__ part) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    double v[kSums];
#pragma unroll
    for (int c = 0; c < kSums; ++c) v[c] = 0.0;
    i64 cnt = 0;
    if (i < n) {
        double p[3];
        pb3d_load3<F64>(pts, i, p);
        const double r = ((pl.p[0] * p[0] + pl.p[1] * p[1]) + pl.p[2] * p[2]) + pl.p[3];
        if (fabs(r) <= tau) {
            const double P[3] = {p[0] - pv.c[0], p[1] - pv.c[1], p[2] - pv.c[2]};
            v[0] = P[0]; v[1] = P[1]; v[2] = P[2];
            v[3] = P[0] * P[0]; v[4] = P[0] * P[1]; v[5] = P[0] * P[2];
            v[6] = P[1] * P[1]; v[7] = P[1] * P[2]; v[8] = P[2] * P[2];
            v[9] = r;
            v[10] = r * r;
            cnt = 1;
        }
    }
    pb3d_reduce_row<kSums>(v, cnt, part + (i64)blockIdx.x * kRow);
}

// ---- the order-keeping compaction shell: one text for every per-point predicate ------------------------------------------------------
// Keep(i) says whether row i survives.  InBox: the closed box of crop_to_box; Flagged: the caller's byte per point (select_points).
template <bool F64>
struct InBox {
    const void* pts;
    Box bx;
    __device__ __forceinline__ bool operator()(i64 i) const {
        double p[3];
        pb3d_load3<F64>(pts, i, p);
        bool keep = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) keep = keep && bx.lo[a] <= p[a] && p[a] <= bx.hi[a];      // a NaN coordinate fails
        return keep;
    }
};
struct Flagged {
    const u8* keep;
    __device__ __forceinline__ bool operator()(i64 i) const { return keep[i] != 0; }
};

template <class Keep>
__global__ __launch_bounds__(256) void k_crop_count(i64 n, Keep pred, u32* __restrict__ counts) {
    __shared__ u32 wsum[4];
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    const bool keep = i < n && pred(i);
    const u32 c = (u32)__popcll(__ballot(keep));
    group_total<4>(c, wsum, [&](u32 tot) { counts[blockIdx.x] = tot; });
}

template <bool F64, class Keep>
__global__ __launch_bounds__(256) void k_crop_fill(const void* __restrict__ pts, i64 n, Keep pred, const i64* __restrict__ offsets, i64 nblocks,
                                                   void* __restrict__ out, int* __restrict__ idx, i64* __restrict__ count) {
    __shared__ u32 wsum[4];
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    const bool keep = i < n && pred(i);
    const unsigned long long m = __ballot(keep);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) wsum[w] = (u32)__popcll(m);
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x == 0) *count = offsets[nblocks];
    if (!keep) return;
    i64 pos = offsets[blockIdx.x] + __popcll(m & ((1ull << lane) - 1));
    for (int j = 0; j < w; ++j) pos += wsum[j];
    if (F64) {                                                                 // the row's bytes as they are, never through arithmetic
        const u64* s = (const u64*)pts + 3 * i;
        u64* d = (u64*)out + 3 * pos;
        d[0] = s[0]; d[1] = s[1]; d[2] = s[2];
    } else {
        const u32* s = (const u32*)pts + 3 * i;
        u32* d = (u32*)out + 3 * pos;
        d[0] = s[0]; d[1] = s[1]; d[2] = s[2];
    }
    if (idx) idx[pos] = (int)i;
}

// count per 256 consecutive points, scan, fill: the n >= 1 rows that pred keeps -> the front of d_out, their positions -> d_idx (may be
// null), their number -> d_count.  Enqueue only.
template <bool F64, class Keep>
int compact_points(pb3d_ctx* ctx, const void* d_pts, i64 n, const Keep& pred, void* d_out, int* d_idx, i64* d_count) {
    const i64 nb = (n + 255) / 256;
    void *cnt, *off;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_CROP_COUNTS, (size_t)nb * sizeof(u32), &cnt));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_CROP_OFFSETS, (size_t)(nb + 1) * sizeof(i64), &off));
    const dim3 grid((unsigned)nb);
    hipLaunchKernelGGL(k_crop_count<Keep>, grid, dim3(256), 0, ctx->stream, n, pred, (u32*)cnt);
    PB3D_CHECK_LAUNCH();
    PB3D_TRY(pb3d_scan_counts(ctx, (const u32*)cnt, nb, (i64*)off, PB3D_SLOT_CROP_SCAN_LOCAL, PB3D_SLOT_CROP_SCAN_SEGS));
    hipLaunchKernelGGL((k_crop_fill<F64, Keep>), grid, dim3(256), 0, ctx->stream, d_pts, n, pred, (const i64*)off, nb, d_out, d_idx, d_count);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

}  // namespace

extern "C" {

int pb3d_plane_hypotheses_resident(pb3d_ctx* ctx, const void* d_pts, int pts_f64, int64_t n, const int64_t* d_triplets, int K, double* d_planes) {
    PB3D_REQUIRE(n >= 0 && n <= pb3d_max_points, "pb3d_plane_hypotheses: need 0 <= n <= 2^31 - 1 points (got %lld)", (long long)n);
    PB3D_REQUIRE(K >= 1 && K <= kMaxPlanes, "pb3d_plane_hypotheses: need 1 <= K <= %d hypotheses (got %d)", kMaxPlanes, K);
    PB3D_REQUIRE(d_triplets != nullptr && d_planes != nullptr, "pb3d_plane_hypotheses: null buffer");
    PB3D_REQUIRE(n == 0 || d_pts != nullptr, "pb3d_plane_hypotheses: null buffer");
    PB3D_REQUIRE(ctx != nullptr, "pb3d_plane_hypotheses: null context");
    const dim3 grid((unsigned)((K + 255) / 256));
    if (pts_f64) hipLaunchKernelGGL(k_plane_hyp<true>, grid, dim3(256), 0, ctx->stream, d_pts, (i64)n, (const i64*)d_triplets, K, d_planes);
    else hipLaunchKernelGGL(k_plane_hyp<false>, grid, dim3(256), 0, ctx->stream, d_pts, (i64)n, (const i64*)d_triplets, K, d_planes);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

int pb3d_plane_score_resident(pb3d_ctx* ctx, const void* d_pts, int pts_f64, int64_t n, const double* d_planes, int K, double tau,
                              int64_t* d_counts) {
    PB3D_REQUIRE(n >= 0 && n <= pb3d_max_points, "pb3d_plane_score: need 0 <= n <= 2^31 - 1 points (got %lld)", (long long)n);
    PB3D_REQUIRE(K >= 1 && K <= kMaxPlanes, "pb3d_plane_score: need 1 <= K <= %d planes (got %d)", kMaxPlanes, K);
    PB3D_REQUIRE(tau >= 0.0, "pb3d_plane_score: the threshold must be >= 0 and not NaN");
    PB3D_REQUIRE(d_planes != nullptr && d_counts != nullptr, "pb3d_plane_score: null buffer");
    PB3D_REQUIRE(n == 0 || d_pts != nullptr, "pb3d_plane_score: null buffer");
    PB3D_REQUIRE(ctx != nullptr, "pb3d_plane_score: null context");
    PB3D_HIP(hipMemsetAsync(d_counts, 0, (size_t)K * sizeof(int64_t), ctx->stream));
    if (n == 0) return PB3D_OK;
    // min(tiles, CUs * kScoreBlocksPerCu) workgroups along x, each walking tiles b, b + grid, ...; a cloud with fewer tiles than that
    // splits the K rows over y as well (at most ceil(K / 64) chunks), so that a small cloud still fills the device
    const unsigned gx = pb3d_stream_blocks(ctx, n, kTile, kScoreBlocksPerCu);
    const int want = (ctx->cus > 0 ? ctx->cus : 256) * kScoreBlocksPerCu;
    int chunks = 1;
    if ((i64)gx < want) chunks = (int)std::min<i64>((want + gx - 1) / gx, (K + 63) / 64);
    const int kchunk = (K + chunks - 1) / chunks;
    const dim3 grid(gx, (unsigned)((K + kchunk - 1) / kchunk));
    unsigned long long* c = (unsigned long long*)d_counts;
    if (pts_f64) hipLaunchKernelGGL(k_plane_score<true>, grid, dim3(256), 0, ctx->stream, d_pts, (i64)n, d_planes, K, kchunk, tau, c);
    else hipLaunchKernelGGL(k_plane_score<false>, grid, dim3(256), 0, ctx->stream, d_pts, (i64)n, d_planes, K, kchunk, tau, c);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

int pb3d_plane_moments_resident(pb3d_ctx* ctx, const void* d_pts, int pts_f64, int64_t n, const double plane[4], double tau,
                                const double pivot[3], void* d_out) {
    PB3D_REQUIRE(n >= 0 && n <= pb3d_max_points, "pb3d_plane_moments: need 0 <= n <= 2^31 - 1 points (got %lld)", (long long)n);
    PB3D_REQUIRE(tau >= 0.0, "pb3d_plane_moments: the threshold must be >= 0 and not NaN");
    PB3D_REQUIRE(plane != nullptr && pivot != nullptr && d_out != nullptr, "pb3d_plane_moments: null argument");
    PB3D_REQUIRE(n == 0 || d_pts != nullptr, "pb3d_plane_moments: null buffer");
    PB3D_REQUIRE(ctx != nullptr, "pb3d_plane_moments: null context");
    if (n == 0) {
        PB3D_HIP(hipMemsetAsync(d_out, 0, kRow * 8, ctx->stream));
        return PB3D_OK;
    }
    const i64 nrows = (n + 255) / 256;
    void* part;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_PLANE_PARTIALS, (size_t)nrows * kRow * 8, &part));
    Plane pl;
    Pivot pv;
    memcpy(pl.p, plane, sizeof(pl.p));
    memcpy(pv.c, pivot, sizeof(pv.c));
    if (pts_f64) hipLaunchKernelGGL(k_plane_terms<true>, dim3((unsigned)nrows), dim3(256), 0, ctx->stream, d_pts, (i64)n, pl, tau, pv, (double*)part);
    else hipLaunchKernelGGL(k_plane_terms<false>, dim3((unsigned)nrows), dim3(256), 0, ctx->stream, d_pts, (i64)n, pl, tau, pv, (double*)part);
    PB3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(pb3d_k_rows_final<kSums>, dim3(1), dim3(256), 0, ctx->stream, (const double*)part, nrows, (double*)d_out);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

int pb3d_points_crop_box_resident(pb3d_ctx* ctx, const void* d_pts, int pts_f64, int64_t n, const double lo[3], const double hi[3], void* d_out,
                                  int32_t* d_idx, int64_t* d_count) {
    PB3D_REQUIRE(n >= 0 && n <= pb3d_max_points, "pb3d_points_crop_box: need 0 <= n <= 2^31 - 1 points (got %lld)", (long long)n);
    PB3D_REQUIRE(lo != nullptr && hi != nullptr && d_count != nullptr, "pb3d_points_crop_box: null argument");
    PB3D_REQUIRE(n == 0 || (d_pts != nullptr && d_out != nullptr), "pb3d_points_crop_box: null buffer");
    PB3D_REQUIRE(ctx != nullptr, "pb3d_points_crop_box: null context");
    if (n == 0) {
        PB3D_HIP(hipMemsetAsync(d_count, 0, sizeof(int64_t), ctx->stream));
        return PB3D_OK;
    }
    Box bx;
    memcpy(bx.lo, lo, sizeof(bx.lo));
    memcpy(bx.hi, hi, sizeof(bx.hi));
    if (pts_f64) return compact_points<true>(ctx, d_pts, (i64)n, InBox<true>{d_pts, bx}, d_out, (int*)d_idx, (i64*)d_count);
    return compact_points<false>(ctx, d_pts, (i64)n, InBox<false>{d_pts, bx}, d_out, (int*)d_idx, (i64*)d_count);
}

int pb3d_points_select_resident(pb3d_ctx* ctx, const void* d_pts, int pts_f64, int64_t n, const uint8_t* d_keep, void* d_out, int32_t* d_idx,
                                int64_t* d_count) {
    PB3D_REQUIRE(n >= 0 && n <= pb3d_max_points, "pb3d_points_select: need 0 <= n <= 2^31 - 1 points (got %lld)", (long long)n);
    PB3D_REQUIRE(d_count != nullptr, "pb3d_points_select: null argument");
    PB3D_REQUIRE(n == 0 || (d_pts != nullptr && d_keep != nullptr && d_out != nullptr), "pb3d_points_select: null buffer");
    PB3D_REQUIRE(ctx != nullptr, "pb3d_points_select: null context");
    if (n == 0) {
        PB3D_HIP(hipMemsetAsync(d_count, 0, sizeof(int64_t), ctx->stream));
        return PB3D_OK;
    }
    if (pts_f64) return compact_points<true>(ctx, d_pts, (i64)n, Flagged{d_keep}, d_out, (int*)d_idx, (i64*)d_count);
    return compact_points<false>(ctx, d_pts, (i64)n, Flagged{d_keep}, d_out, (int*)d_idx, (i64*)d_count);
}

}  // extern "C"
