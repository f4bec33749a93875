// smooth_mesh: the vertex-to-vertex adjacency of a triangle mesh and Laplacian / Taubin smoothing on it (include/pb3d.h has the rules
// to the bit; DESIGN.md "Mesh smoothing" has the passes and their times).
//
// Adjacency = the unique directed pairs (i, j) of the faces' edges, ordered by (i, j).  Nothing in the build is kept per vertex, so a
// vertex that is in every face is handled like any other:
//   k_emit_pairs      face (a, b, c) -> (a,b) (b,a) (b,c) (c,b) (c,a) (a,c), key = second end, value = first end; a pair with equal
//                     ends becomes (nv, nv), which sorts behind everything
//   pb3d_sort_pairs   twice (csrc/sort_pairs.hip, stable): by the second end, then -- key and value change roles -- by the first
//   k_adj_flags       flag[p] = pair p differs from pair p - 1 and is no sentinel
//   pb3d_scan_counts  rank[p] = flags below p: where a unique pair goes; rank[P] = total (read back by the adjacency entry only)
//   k_adj_compact     a flagged pair writes its second end to neighbours[rank] and its position to first[rank]; the last pair that is
//                     no sentinel closes the list: first[total] = its position + 1
//   k_adj_starts      starts[v] = rank[the first position whose first end is >= v], by bisection of the sorted column
//   k_adj_runs        multiplicity of unique pair r = first[r + 1] - first[r]; a run of one marks both ends in the boundary bytes
//                     (plain stores of 1: every writer of a byte writes the same value)
// A step reads one float64 position buffer and writes the other:
//   k_smooth_step     one lane per vertex walks its ascending list: s = 0.0, s = s + x_j; m = s / deg; d = m - x; x + f * d -- one
//                     rounded operation each (-ffp-contract=off, __ddiv_rn).  Fixed vertices and vertices without a neighbour copy
//   k_smooth_hubs     the vertices whose degree exceeds kLaneDegree (listed once, k_hub_list), one wavefront each: the ordered
//                     wavefront sum of csrc/ordered_sum.h -- the same additions in the same order as the lane form, so the cutoff
//                     changes the time and never the bits
// The last step stores in the caller's dtype: the one rounding to float32.
#include <algorithm>
#include <cmath>

#include "mesh_index.h"
#include "ordered_sum.h"
#include "pb3d_internal.h"

namespace {

constexpr i64 kMaxVerts = (1ll << 31) - 1, kMaxPairs = (1ll << 31) - 1;
constexpr int kLaneDegree = 32;                     // above it a vertex is summed by a wavefront

// ---- adjacency ------------------------------------------------------------------------------------------------------------------------
template <bool I64>
__global__ __launch_bounds__(256) void k_emit_pairs(const void* __restrict__ faces, i64 nf, i64 nv, u32* __restrict__ key, u32* __restrict__ val) {
    const i64 f = (i64)blockIdx.x * 256 + threadIdx.x;
    if (f >= nf) return;
    const u32 c[3] = {(u32)wrap(load_index<I64>(faces, 3 * f), nv), (u32)wrap(load_index<I64>(faces, 3 * f + 1), nv),
                      (u32)wrap(load_index<I64>(faces, 3 * f + 2), nv)};
    const u32 none = (u32)nv;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const u32 a = c[k], b = c[(k + 1) % 3];
        const bool self = a == b;
        const i64 p = 6 * f + 2 * k;
        key[p] = self ? none : b;     val[p] = self ? none : a;         // (a, b)
        key[p + 1] = self ? none : a; val[p + 1] = self ? none : b;     // (b, a)
    }
}

// the pair at p opens a run: it is no sentinel and differs from its predecessor
__device__ __forceinline__ bool opens_run(const u32* __restrict__ I, const u32* __restrict__ J, i64 p, u32 none) {
    const u32 i = I[p];
    return i != none && (p == 0 || I[p - 1] != i || J[p - 1] != J[p]);
}

__global__ __launch_bounds__(256) void k_adj_flags(const u32* __restrict__ I, const u32* __restrict__ J, i64 P, u32 none, u32* __restrict__ flag) {
    const i64 p = (i64)blockIdx.x * 256 + threadIdx.x;
    if (p < P) flag[p] = opens_run(I, J, p, none) ? 1u : 0u;
}

// first: P + 1 entries
__global__ __launch_bounds__(256) void k_adj_compact(const u32* __restrict__ I, const u32* __restrict__ J, i64 P, u32 none,
                                                     const i64* __restrict__ rank, int* __restrict__ neighbours, u32* __restrict__ first) {
    const i64 p = (i64)blockIdx.x * 256 + threadIdx.x;
    if (p >= P || I[p] == none) return;
    if (opens_run(I, J, p, none)) {
        const i64 r = rank[p];
        neighbours[r] = (int)J[p];
        first[r] = (u32)p;
    }
    if (p == P - 1 || I[p + 1] == none) first[rank[P]] = (u32)(p + 1);
}

__global__ __launch_bounds__(256) void k_adj_starts(const u32* __restrict__ I, i64 P, i64 nv, const i64* __restrict__ rank, i64* __restrict__ starts) {
    const i64 v = (i64)blockIdx.x * 256 + threadIdx.x;
    if (v > nv) return;
    i64 lo = 0, hi = P;                 // the first position whose first end is >= v (the sentinels hold nv)
    while (lo < hi) {
        const i64 mid = lo + (hi - lo) / 2;
        if ((i64)I[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    starts[v] = rank[lo];
}

// mult and boundary may each be null
__global__ __launch_bounds__(256) void k_adj_runs(const u32* __restrict__ I, const u32* __restrict__ J, i64 P, u32 none, const i64* __restrict__ rank,
                                                  const u32* __restrict__ first, u32* __restrict__ mult, u8* __restrict__ boundary) {
    const i64 p = (i64)blockIdx.x * 256 + threadIdx.x;
    if (p >= P || !opens_run(I, J, p, none)) return;
    const i64 r = rank[p];
    const u32 len = first[r + 1] - (u32)p;
    if (mult) mult[r] = len;
    if (boundary && len == 1) { boundary[I[p]] = 1; boundary[J[p]] = 1; }
}

// ---- steps ----------------------------------------------------------------------------------------------------------------------------
template <bool F64>
__global__ __launch_bounds__(256) void k_widen(const void* __restrict__ in, i64 n, double* __restrict__ out) {
    for (i64 e = (i64)blockIdx.x * 256 + threadIdx.x; e < n; e += (i64)gridDim.x * 256)
        out[e] = F64 ? ((const double*)in)[e] : (double)((const float*)in)[e];
}

__global__ __launch_bounds__(256) void k_fixed_merge(u8* __restrict__ fixed, const u8* __restrict__ more, i64 nv) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i < nv && more[i]) fixed[i] = 1;
}

// hubs[0] = their number (zeroed before), hubs[1 ...] = the vertices, in whatever order the integer atomics give: each is summed on its own
__global__ __launch_bounds__(256) void k_hub_list(const i64* __restrict__ starts, i64 nv, u32* __restrict__ hubs) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i < nv && starts[i + 1] - starts[i] > kLaneDegree) hubs[1 + atomicAdd(&hubs[0], 1u)] = (u32)i;
}

template <bool F32OUT>
__device__ __forceinline__ void store_coord(void* out, i64 e, double x) {
    if (F32OUT) ((float*)out)[e] = (float)x;        // the one rounding to float32
    else ((double*)out)[e] = x;
}

// STEP of include/pb3d.h for the vertices of degree <= kLaneDegree; fixed may be null
template <bool F32OUT>
__global__ __launch_bounds__(256) void k_smooth_step(const double* __restrict__ pos, i64 nv, const i64* __restrict__ starts,
                                                     const int* __restrict__ neighbours, const u8* __restrict__ fixed, double f,
                                                     void* __restrict__ out) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    const i64 s = starts[i], e = starts[i + 1];
    double x[3] = {pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]};
    if (e > s && !(fixed && fixed[i])) {
        if (e - s > kLaneDegree) return;            // k_smooth_hubs writes it
        double sum[3] = {0.0, 0.0, 0.0};
        for (i64 p = s; p < e; ++p) {
            const double* q = pos + 3 * (i64)neighbours[p];
            sum[0] = sum[0] + q[0];
            sum[1] = sum[1] + q[1];
            sum[2] = sum[2] + q[2];
        }
        const double deg = (double)(e - s);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double m = __ddiv_rn(sum[a], deg);
            const double d = m - x[a];
            x[a] = x[a] + f * d;
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) store_coord<F32OUT>(out, 3 * i + a, x[a]);
}

// the same STEP for the listed vertices, one wavefront each: however long the list, it is walked 64 a time
template <bool F32OUT>
__global__ __launch_bounds__(256) void k_smooth_hubs(const double* __restrict__ pos, const u32* __restrict__ hubs, const i64* __restrict__ starts,
                                                     const int* __restrict__ neighbours, const u8* __restrict__ fixed, double f,
                                                     void* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const i64 nwaves = (i64)gridDim.x * 4, nhubs = (i64)hubs[0];
    for (i64 h = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) + (i64)blockIdx.x * 4; h < nhubs; h += nwaves) {
        const i64 v = __builtin_amdgcn_readfirstlane((int)hubs[1 + h]);
        if (fixed && fixed[v]) continue;            // k_smooth_step has copied it
        const i64 s = starts[v], e = starts[v + 1];
        double sum[3];
        ordered_sum(s, e, [&](i64 p, double* row) {
            const double* q = pos + 3 * (i64)neighbours[p];
            row[0] = q[0]; row[1] = q[1]; row[2] = q[2];
        }, sum);
        if (lane < 3) {
            const double x = pos[3 * v + lane];
            const double m = __ddiv_rn(lane == 0 ? sum[0] : lane == 1 ? sum[1] : sum[2], (double)(e - s));
            const double d = m - x;
            store_coord<F32OUT>(out, 3 * v + lane, x + f * d);
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
inline dim3 grid_for(i64 n) { return dim3((unsigned)((n + 255) / 256)); }

// where the adjacency of a call goes: the entry's buffers, or the slots of a smoothing
struct AdjOut { i64* starts; int* neighbours; u32* mult; u8* boundary; };

// nv >= 1, nf >= 1, checked indices.  Everything is enqueued; *d_total = where the number of unique pairs stands on the device
int build_adjacency(pb3d_ctx* ctx, const void* d_faces, int faces_i64, i64 nv, i64 nf, const AdjOut& o, const i64** d_total) {
    const i64 P = 6 * nf;
    const u32 none = (u32)nv;
    void *kv, *fl, *rk;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_SMOOTH_PAIRS, (size_t)P * 4 * sizeof(u32), &kv));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_SMOOTH_FLAGS, (size_t)(P + 1) * sizeof(u32), &fl));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_SMOOTH_RANKS, (size_t)(P + 1) * sizeof(i64), &rk));
    // the scans of the call are the sorts' run tables and the flags': size both scan slots for the largest now, so that none regrows
    // (and waits) midway
    PB3D_TRY(pb3d_scan_reserve(ctx, std::max<i64>(P, pb3d_sort_scan_items(P)), PB3D_SLOT_SMOOTH_SCAN_LOCAL, PB3D_SLOT_SMOOTH_SCAN_SEGS));
    u32* a = (u32*)kv;
    u32 *key = a, *val = a + P, *key2 = a + 2 * P, *val2 = a + 3 * P;
    hipLaunchKernelGGL((faces_i64 ? k_emit_pairs<true> : k_emit_pairs<false>), grid_for(nf), dim3(256), 0, ctx->stream, d_faces, nf, nv, key, val);
    PB3D_CHECK_LAUNCH();
    const u32 *by_j, *ends_i;       // sorted by the second end: that column and the first ends beside it
    PB3D_TRY(pb3d_sort_pairs(ctx, key, val, key2, val2, P, nv + 1, PB3D_SLOT_SMOOTH_SORT_HIST, PB3D_SLOT_SMOOTH_SCAN_LOCAL,
                             PB3D_SLOT_SMOOTH_SCAN_SEGS, &by_j, &ends_i));
    // the roles change: the first ends are the keys now, and the other two arrays are the twins
    u32 *k1 = (u32*)ends_i, *v1 = (u32*)by_j, *k2 = k1 == val ? val2 : val, *v2 = v1 == key ? key2 : key;
    const u32 *I, *J;
    PB3D_TRY(pb3d_sort_pairs(ctx, k1, v1, k2, v2, P, nv + 1, PB3D_SLOT_SMOOTH_SORT_HIST, PB3D_SLOT_SMOOTH_SCAN_LOCAL, PB3D_SLOT_SMOOTH_SCAN_SEGS,
                             &I, &J));
    u32* flags = (u32*)fl;
    i64* rank = (i64*)rk;
    hipLaunchKernelGGL(k_adj_flags, grid_for(P), dim3(256), 0, ctx->stream, I, J, P, none, flags);
    PB3D_CHECK_LAUNCH();
    PB3D_TRY(pb3d_scan_counts(ctx, flags, P, rank, PB3D_SLOT_SMOOTH_SCAN_LOCAL, PB3D_SLOT_SMOOTH_SCAN_SEGS));
    // the flags are spent: the position of every unique pair's first copy takes their place
    hipLaunchKernelGGL(k_adj_compact, grid_for(P), dim3(256), 0, ctx->stream, I, J, P, none, (const i64*)rank, o.neighbours, flags);
    PB3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_adj_starts, grid_for(nv + 1), dim3(256), 0, ctx->stream, I, P, nv, (const i64*)rank, o.starts);
    PB3D_CHECK_LAUNCH();
    if (o.mult || o.boundary) {
        if (o.boundary) PB3D_HIP(hipMemsetAsync(o.boundary, 0, (size_t)nv, ctx->stream));
        hipLaunchKernelGGL(k_adj_runs, grid_for(P), dim3(256), 0, ctx->stream, I, J, P, none, (const i64*)rank, (const u32*)flags, o.mult, o.boundary);
        PB3D_CHECK_LAUNCH();
    }
    *d_total = rank + P;
    return PB3D_OK;
}

int require_faces(const char* what, const void* d_faces, i64 nv, i64 nf) {
    PB3D_REQUIRE(nv >= 0 && nf >= 0, "%s: negative count", what);
    PB3D_REQUIRE(nv <= kMaxVerts && nf <= kMaxPairs / 6, "%s: at most 2^31 - 1 vertices and 2^31 - 1 directed pairs (6 per face)", what);
    PB3D_REQUIRE(nf == 0 || d_faces != nullptr, "%s: null buffer", what);
    return PB3D_OK;
}

template <bool F32OUT>
int launch_step(pb3d_ctx* ctx, const double* pos, i64 nv, const i64* starts, const int* neighbours, const u8* fixed, double f, const u32* hubs,
                i64 max_hubs, void* out) {
    hipLaunchKernelGGL(k_smooth_step<F32OUT>, grid_for(nv), dim3(256), 0, ctx->stream, pos, nv, starts, neighbours, fixed, f, out);
    PB3D_CHECK_LAUNCH();
    if (max_hubs > 0) {
        hipLaunchKernelGGL(k_smooth_hubs<F32OUT>, dim3(pb3d_stream_blocks(ctx, max_hubs, 4, 8)), dim3(256), 0, ctx->stream, pos, hubs, starts, neighbours,
                           fixed, f, out);
        PB3D_CHECK_LAUNCH();
    }
    return PB3D_OK;
}

}  // namespace

extern "C" {

int pb3d_mesh_adjacency_resident(pb3d_ctx* ctx, const void* d_faces, int faces_i64, int64_t nv, int64_t nf, int64_t* d_starts,
                                 int32_t* d_neighbours, uint32_t* d_mult, uint8_t* d_boundary, int64_t* total) {
    PB3D_TRY(require_faces("pb3d_mesh_adjacency", d_faces, nv, nf));
    PB3D_REQUIRE(total != nullptr, "pb3d_mesh_adjacency: null argument");
    PB3D_REQUIRE(d_starts != nullptr && (nf == 0 || d_neighbours != nullptr), "pb3d_mesh_adjacency: null buffer");
    PB3D_REQUIRE(ctx != nullptr, "pb3d_mesh_adjacency: null context");
    PB3D_TRY(pb3d_check_index_range(ctx, d_faces, faces_i64, 3 * nf, -nv, nv, "pb3d_mesh_adjacency"));
    *total = 0;
    if (nf == 0) {
        PB3D_HIP(hipMemsetAsync(d_starts, 0, (size_t)(nv + 1) * sizeof(i64), ctx->stream));
        if (d_boundary && nv > 0) PB3D_HIP(hipMemsetAsync(d_boundary, 0, (size_t)nv, ctx->stream));
        return PB3D_OK;
    }
    const i64* d_total;
    PB3D_TRY(build_adjacency(ctx, d_faces, faces_i64, nv, nf, AdjOut{d_starts, d_neighbours, d_mult, d_boundary}, &d_total));
    return pb3d_read_back(ctx, total, d_total, sizeof(i64));
}

int pb3d_mesh_smooth_resident(pb3d_ctx* ctx, const void* d_verts, int verts_f64, int64_t nv, const void* d_faces, int faces_i64, int64_t nf,
                              int iterations, double lambda, double mu, const uint8_t* d_fixed, int fix_boundary, void* d_out) {
    PB3D_TRY(require_faces("pb3d_mesh_smooth", d_faces, nv, nf));
    PB3D_REQUIRE(iterations >= 0, "pb3d_mesh_smooth: iterations must be >= 0 (got %d)", iterations);
    PB3D_REQUIRE(std::isfinite(lambda), "pb3d_mesh_smooth: lambda must be finite (got %g)", lambda);
    PB3D_REQUIRE(!std::isinf(mu), "pb3d_mesh_smooth: mu must be finite, or NaN for Laplacian smoothing (got %g)", mu);
    PB3D_REQUIRE(nv == 0 || (d_verts != nullptr && d_out != nullptr), "pb3d_mesh_smooth: null buffer");
    PB3D_REQUIRE(nv == 0 || d_verts != d_out, "pb3d_mesh_smooth: d_out may not alias d_verts");
    PB3D_REQUIRE(ctx != nullptr, "pb3d_mesh_smooth: null context");
    PB3D_TRY(pb3d_check_index_range(ctx, d_faces, faces_i64, 3 * nf, -nv, nv, "pb3d_mesh_smooth"));
    if (nv == 0) return PB3D_OK;
    if (nf == 0 || iterations == 0) {       // the input bytes
        PB3D_HIP(hipMemcpyAsync(d_out, d_verts, (size_t)nv * 3 * (verts_f64 ? sizeof(double) : sizeof(float)), hipMemcpyDeviceToDevice, ctx->stream));
        return PB3D_OK;
    }
    const i64 P = 6 * nf, hub_room = P / (kLaneDegree + 1), max_hubs = hub_room < nv ? hub_room : nv;
    void *st, *nb, *bd = nullptr, *hb = nullptr, *pa, *pb;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_SMOOTH_STARTS, (size_t)(nv + 1) * sizeof(i64), &st));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_SMOOTH_NEIGHBOURS, (size_t)P * sizeof(int), &nb));
    if (fix_boundary) PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_SMOOTH_BOUNDARY, (size_t)nv, &bd));
    if (max_hubs > 0) PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_SMOOTH_HUBS, (size_t)(max_hubs + 1) * sizeof(u32), &hb));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_SMOOTH_POS_A, (size_t)nv * 3 * sizeof(double), &pa));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_SMOOTH_POS_B, (size_t)nv * 3 * sizeof(double), &pb));
    const i64* d_total;
    PB3D_TRY(build_adjacency(ctx, d_faces, faces_i64, nv, nf, AdjOut{(i64*)st, (int*)nb, nullptr, (u8*)bd}, &d_total));

    const u8* fixed = d_fixed;
    if (fix_boundary) {
        if (d_fixed) {
            hipLaunchKernelGGL(k_fixed_merge, grid_for(nv), dim3(256), 0, ctx->stream, (u8*)bd, d_fixed, (i64)nv);
            PB3D_CHECK_LAUNCH();
        }
        fixed = (const u8*)bd;
    }
    if (max_hubs > 0) {
        PB3D_HIP(hipMemsetAsync(hb, 0, sizeof(u32), ctx->stream));
        hipLaunchKernelGGL(k_hub_list, grid_for(nv), dim3(256), 0, ctx->stream, (const i64*)st, (i64)nv, (u32*)hb);
        PB3D_CHECK_LAUNCH();
    }
    const unsigned wb = pb3d_stream_blocks(ctx, 3 * nv, 256, 8);
    hipLaunchKernelGGL((verts_f64 ? k_widen<true> : k_widen<false>), dim3(wb), dim3(256), 0, ctx->stream, d_verts, 3 * (i64)nv, (double*)pa);
    PB3D_CHECK_LAUNCH();

    const bool taubin = !std::isnan(mu);
    const i64 steps = (i64)iterations * (taubin ? 2 : 1);
    double *src = (double*)pa, *dst = (double*)pb;
    for (i64 k = 0; k < steps; ++k) {
        const double f = taubin && (k & 1) ? mu : lambda;
        if (k + 1 < steps) {
            PB3D_TRY(launch_step<false>(ctx, src, nv, (const i64*)st, (const int*)nb, fixed, f, (const u32*)hb, max_hubs, dst));
            double* t = src; src = dst; dst = t;
        } else if (verts_f64) {
            PB3D_TRY(launch_step<false>(ctx, src, nv, (const i64*)st, (const int*)nb, fixed, f, (const u32*)hb, max_hubs, d_out));
        } else {
            PB3D_TRY(launch_step<true>(ctx, src, nv, (const i64*)st, (const int*)nb, fixed, f, (const u32*)hb, max_hubs, d_out));
        }
    }
    return PB3D_OK;
}

}  // extern "C"
