// I5: the inter-method point-cloud metrics (reference utils/eval_helpers.py) -- exact nearest-neighbour distances and voxel_iou counts.
//
// Every metric of eval_helpers.py rests on one primitive: for each point of A, the distance to its nearest (k = 1) or second-nearest
// (k = 2) point of B.  The reference takes it from cKDTree.query / NearestNeighbors.kneighbors, which on float64 (float32 is widened
// first) return exactly sqrt((dx*dx + dy*dy) + dz*dz) of the nearest point, with no FMA.  Ties and which neighbour was picked never
// reach a metric, so a search that finds the minimum of that expression is bit-exact.  The Makefile passes -ffp-contract=off: the
// squared distance is three separate multiplies and two adds, in this order, and one correctly rounded sqrt at the end (__dsqrt_rn).
//
// Index: a uniform grid of cells over the reference set's bounding box (exact min / max, k_bounds_*), cell size
// chosen on the host from the box and the point count for about kPerCell points per cell; the points are binned by a count pass, the
// exclusive scan of csrc/points.hip and a scatter into cell-sorted SoA float64 arrays (order within a cell is free: atomics).
// Query: the queries are binned the same way and processed in cell order (the lanes of a wave walk the same cells); each searches
// Chebyshev rings of growing radius around its cell, clamped to the grid, pruning (x) planes and z-runs of cells whose box is farther
// than the current k-th best, and stops once the lower bound on the distance to every cell not yet visited exceeds the k-th best.
// The bound counts only faces of the visited box that still have cells beyond them, adds the query's distance to the grid box along
// the other axes (queries far outside the box), and is shrunk by a relative margin, so a point that rounding put in a neighbouring
// cell can never be missed; the final comparison is strict with a margin, never an exact tie.
#include <cmath>

#include "pb3d_internal.h"
#include "wave.h"
#include "ring_walk.h"      // the cell grid (Grid, make_grid, cell_of, cell_index) and ring_walk with its bounds

namespace {

constexpr int kBoundsBlocks = 512;
constexpr int kMaxResolution = 2048;         // voxel_iou: two (res^3 / 8)-byte bit grids plus a ping-pong copy

// ---- exact bounding box: per-block min / max, then one block over the partials -> out[0..3) = min, out[3..6) = max -------------------
template <bool F64>
__global__ __launch_bounds__(256) void k_bounds_partial(const void* __restrict__ pts, i64 n, double* __restrict__ part) {
    __shared__ double red[6][4];
    double m[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) {
        double x, y, z;
        pb3d_load3<F64>(pts, i, &x, &y, &z);
        m[0] = fmin(m[0], x); m[1] = fmin(m[1], y); m[2] = fmin(m[2], z);
        m[3] = fmax(m[3], x); m[4] = fmax(m[4], y); m[5] = fmax(m[5], z);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        const double v = c < 3 ? wave_min(m[c]) : wave_max(m[c]);
        if (lane == 0) red[c][w] = v;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int c = threadIdx.x;
        double v = red[c][0];
        for (int k = 1; k < 4; ++k) v = c < 3 ? fmin(v, red[c][k]) : fmax(v, red[c][k]);
        part[(i64)blockIdx.x * 6 + c] = v;
    }
}

__global__ __launch_bounds__(64) void k_bounds_final(const double* __restrict__ part, int nblocks, double* __restrict__ out) {
    if (threadIdx.x >= 6) return;
    const int c = threadIdx.x;
    double v = c < 3 ? INFINITY : -INFINITY;
    for (int b = 0; b < nblocks; ++b) v = c < 3 ? fmin(v, part[b * 6 + c]) : fmax(v, part[b * 6 + c]);
    out[c] = v;
}

// d_out: 6 doubles; PB3D_SLOT_NN_BOUNDS_PARTIALS holds the partials
int launch_bounds(pb3d_ctx* ctx, const void* d_pts, int f64, i64 n, double* d_out) {
    const unsigned need = pb3d_stream_blocks(ctx, n, 256, 2);
    const unsigned nb = need < (unsigned)kBoundsBlocks ? need : (unsigned)kBoundsBlocks;
    void* part;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_NN_BOUNDS_PARTIALS, (size_t)kBoundsBlocks * 6 * sizeof(double), &part));
    if (f64) hipLaunchKernelGGL(k_bounds_partial<true>, dim3(nb), dim3(256), 0, ctx->stream, d_pts, n, (double*)part);
    else hipLaunchKernelGGL(k_bounds_partial<false>, dim3(nb), dim3(256), 0, ctx->stream, d_pts, n, (double*)part);
    PB3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_bounds_final, dim3(1), dim3(64), 0, ctx->stream, (const double*)part, (int)nb, d_out);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

template <bool F64>
__global__ __launch_bounds__(256) void k_cell_count(const void* __restrict__ pts, i64 n, Grid g, u32* __restrict__ counts) {
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) {
        double x, y, z;
        pb3d_load3<F64>(pts, i, &x, &y, &z);
        atomicAdd(&counts[cell_index(g, cell_of(g, 0, x), cell_of(g, 1, y), cell_of(g, 2, z))], 1u);
    }
}

// reference points -> cell-sorted SoA (xs, ys, zs) and, where ids is given, each sorted point's position in the caller's list;
// cursor: zeroed per-cell counters
template <bool F64>
__global__ __launch_bounds__(256) void k_cell_scatter_ref(const void* __restrict__ pts, i64 n, Grid g, const i64* __restrict__ start,
                                                          u32* __restrict__ cursor, double* __restrict__ xs, double* __restrict__ ys,
                                                          double* __restrict__ zs, int* __restrict__ ids) {
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) {
        double x, y, z;
        pb3d_load3<F64>(pts, i, &x, &y, &z);
        const i64 c = cell_index(g, cell_of(g, 0, x), cell_of(g, 1, y), cell_of(g, 2, z));
        const i64 pos = start[c] + atomicAdd(&cursor[c], 1u);
        xs[pos] = x; ys[pos] = y; zs[pos] = z;
        if (ids) ids[pos] = (int)i;
    }
}

// query indices in cell order
template <bool F64>
__global__ __launch_bounds__(256) void k_cell_scatter_query(const void* __restrict__ pts, i64 n, Grid g, const i64* __restrict__ start,
                                                            u32* __restrict__ cursor, u32* __restrict__ order) {
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) {
        double x, y, z;
        pb3d_load3<F64>(pts, i, &x, &y, &z);
        const i64 c = cell_index(g, cell_of(g, 0, x), cell_of(g, 1, y), cell_of(g, 2, z));
        order[start[c] + atomicAdd(&cursor[c], 1u)] = (u32)i;
    }
}

// ---- the searches: what the cells hold and what each keeps (the walk itself: csrc/ring_walk.h) -------------------------------------
struct Sorted { const double *xs, *ys, *zs; const int* ids; };     // the cell-sorted arrays (ids: null in the distance-only search)

// the distance-only search (K = 1 or 2): the two smallest squared distances seen; whose they are never reaches a metric
template <int K>
struct NearBest {
    double m1, m2;
    __device__ __forceinline__ double bound() const { return K == 1 ? m1 : m2; }
    __device__ __forceinline__ void visit(const Sorted& pts, i64 s, i64 e, const double (&q)[3]) {
        for (i64 p = s; p < e; ++p) {
            const double dx = q[0] - pts.xs[p], dy = q[1] - pts.ys[p], dz = q[2] - pts.zs[p];
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            if (K == 2) m2 = fmin(m2, fmax(m1, d2));    // (m1, m2) = the two smallest of (m1, m2, d2)
            m1 = fmin(m1, d2);
        }
    }
};

template <int K, bool F64>
__global__ __launch_bounds__(256) void k_nn_query(const void* __restrict__ q, i64 nq, const u32* __restrict__ order, Grid g,
                                                  const i64* __restrict__ start, const double* __restrict__ xs, const double* __restrict__ ys,
                                                  const double* __restrict__ zs, double* __restrict__ out) {
    const i64 s = (i64)blockIdx.x * 256 + threadIdx.x;
    if (s >= nq) return;
    const u32 qi = order[s];
    double qv[3];
    pb3d_load3<F64>(q, qi, qv);
    NearBest<K> best = {INFINITY, INFINITY};
    const Sorted pts = {xs, ys, zs, nullptr};
    ring_walk(g, start, pts, qv, best);
    out[qi] = __dsqrt_rn(best.bound());
}

// ---- exact k nearest neighbours with indices (compute_surface_metrics, reference utils/eval_helpers.py:217-218) --------------------
// The same index and the same ring_walk as k_nn_query: the cell-sorted arrays carry each point's position in the caller's array
// (ids), and every lane keeps its k best (squared distance as computed, reference index) pairs.  The list is a register array that
// is only ever indexed by unrolled loops (KC = 8, 20 or 32 slots, the first k in use; a run-time index would put it in scratch
// memory): slot 0 holds the WORST of the k, so the pruning bound is d2[0] whatever k is, and an insertion shifts the worse
// entries towards slot 0.  Order and membership under ties are decided by (d2, index) alone, so the scatter's order within a cell
// and the order cells are visited in do not reach the result.
__device__ __forceinline__ bool knn_less(double d2a, int ia, double d2b, int ib) { return d2a < d2b || (d2a == d2b && ia < ib); }

template <int KC>
struct KBest {
    int k;              // 1 <= k <= KC slots in use
    double d2[KC];      // slot 0: the k-th best (the worst kept); slot k - 1: the nearest
    int id[KC];
    __device__ __forceinline__ void init(int k_) {
        k = k_;
#pragma unroll
        for (int j = 0; j < KC; ++j) { d2[j] = INFINITY; id[j] = 0x7fffffff; }
    }
    // (d, i) beats slot 0: drop slot 0, move the entries worse than (d, i) one slot down, put (d, i) above them
    __device__ __forceinline__ void insert(double d, int i) {
        bool here = true;                       // (d, i) beats slot j
#pragma unroll
        for (int j = 0; j < KC; ++j) {
            const int u = j + 1 < KC ? j + 1 : j;       // the slot above (a constant once unrolled)
            const bool above = j + 1 < KC && j + 1 < k && knn_less(d, i, d2[u], id[u]);
            d2[j] = above ? d2[u] : (here ? d : d2[j]);
            id[j] = above ? id[u] : (here ? i : id[j]);
            here = above;
        }
    }
    __device__ __forceinline__ double bound() const { return d2[0]; }
    __device__ __forceinline__ void visit(const Sorted& pts, i64 s, i64 e, const double (&q)[3]) {
#pragma nounroll
        for (i64 p = s; p < e; ++p) {
            const double dx = q[0] - pts.xs[p], dy = q[1] - pts.ys[p], dz = q[2] - pts.zs[p];
            const double dd = (dx * dx + dy * dy) + dz * dz;
            const int i = pts.ids[p];
            if (knn_less(dd, i, d2[0], id[0])) insert(dd, i);
        }
    }
};

template <int KC, bool F64>
__global__ __launch_bounds__(256) void k_knn_query(const void* __restrict__ q, i64 nq, const u32* __restrict__ order, Grid g,
                                                   const i64* __restrict__ start, const double* __restrict__ xs, const double* __restrict__ ys,
                                                   const double* __restrict__ zs, const int* __restrict__ ids, int k,
                                                   double* __restrict__ out_dist, int* __restrict__ out_idx) {
    const i64 s = (i64)blockIdx.x * 256 + threadIdx.x;
    if (s >= nq) return;
    const u32 qi = order[s];
    double qv[3];
    pb3d_load3<F64>(q, qi, qv);
    KBest<KC> best;
    best.init(k);
    const Sorted pts = {xs, ys, zs, ids};
    ring_walk(g, start, pts, qv, best);
    // row qi, nearest first: slot k - 1 - j
#pragma unroll
    for (int j = 0; j < KC; ++j) {
        if (j < k) {
            const i64 o = (i64)qi * k + (k - 1 - j);
            out_idx[o] = best.id[j];
            if (out_dist) out_dist[o] = __dsqrt_rn(best.d2[j]);
        }
    }
}

// ---- voxel_iou: occupancy bits, 6-neighbour dilation, intersection / union counts -------------------------------------------------
// Bit grid of one cloud: word (x * res + y) * W + z / 32, bit z % 32, W = ceil(res / 32); bits at z >= res stay 0.
struct Occ {
    int res, W;
    double lo[3];      // bounds_min (as float32 values when F32)
    double step;
};

// ((p - bounds_min) / step).astype(int), clipped to [0, res - 1]: the cast of a NaN or out-of-range value gives INT64_MIN (x86
// cvttsd2si, what NumPy's cast compiles to), i.e. 0 after the clip.
__device__ __forceinline__ int occ_index(double t, int res) {
    if (!(t >= -9223372036854775808.0 && t < 9223372036854775808.0)) return 0;
    const i64 i = (i64)t;
    return i < 0 ? 0 : (i > res - 1 ? res - 1 : (int)i);
}

template <bool PF64, bool F32>
__global__ __launch_bounds__(256) void k_occ_bits(const void* __restrict__ pts, i64 n, Occ o, u32* __restrict__ bits) {
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) {
        double v[3];
        pb3d_load3<PF64>(pts, i, v);
        int idx[3];
        for (int a = 0; a < 3; ++a) {
            double t;
            if (F32) t = (double)__fdiv_rn(__fsub_rn((float)v[a], (float)o.lo[a]), (float)o.step);   // NumPy float32 arithmetic
            else t = (v[a] - o.lo[a]) / o.step;
            idx[a] = occ_index(t, o.res);
        }
        atomicOr(&bits[((i64)idx[0] * o.res + idx[1]) * o.W + (idx[2] >> 5)], 1u << (idx[2] & 31));
    }
}

// one binary_dilation pass with the 6-neighbour cross and a zero border, on `grids` bit grids stored one after the other
__global__ __launch_bounds__(256) void k_dilate6(const u32* __restrict__ in, u32* __restrict__ out, int res, int W, i64 words, u32 lastmask) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= words) return;
    const int w = (int)(i % W);
    const i64 rowi = i / W;                     // grid * res^2 + x * res + y
    const int y = (int)(rowi % res);
    const int x = (int)((rowi / res) % res);
    const u32 v = in[i];
    u32 r = v | (v << 1) | (v >> 1);
    if (w > 0) r |= in[i - 1] >> 31;
    if (w < W - 1) r |= in[i + 1] << 31;
    if (y > 0) r |= in[i - W];
    if (y < res - 1) r |= in[i + W];
    if (x > 0) r |= in[i - (i64)res * W];
    if (x < res - 1) r |= in[i + (i64)res * W];
    if (w == W - 1) r &= lastmask;
    out[i] = r;
}

__global__ __launch_bounds__(256) void k_iou_count(const u32* __restrict__ a, const u32* __restrict__ b, i64 words,
                                                   unsigned long long* __restrict__ counts) {
    __shared__ unsigned long long red[2][4];
    unsigned long long ci = 0, cu = 0;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < words; i += (i64)gridDim.x * 256) {
        const u32 x = a[i], y = b[i];
        ci += __popc(x & y);
        cu += __popc(x | y);
    }
    ci = wave_sum(ci); cu = wave_sum(cu);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { red[0][w] = ci; red[1][w] = cu; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const unsigned long long s = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
        atomicAdd(&counts[threadIdx.x], s);
    }
}

template <bool F32>
int launch_occ(pb3d_ctx* ctx, const void* d_pts, int f64, i64 n, const Occ& o, u32* bits) {
    if (n == 0) return PB3D_OK;
    const unsigned nb = pb3d_stream_blocks(ctx, n, 256, 8);
    if (f64) hipLaunchKernelGGL((k_occ_bits<true, F32>), dim3(nb), dim3(256), 0, ctx->stream, d_pts, n, o, bits);
    else hipLaunchKernelGGL((k_occ_bits<false, F32>), dim3(nb), dim3(256), 0, ctx->stream, d_pts, n, o, bits);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

template <bool F64>
int bin_points(pb3d_ctx* ctx, const void* d_pts, i64 n, const Grid& g, pb3d_slot count_slot, pb3d_slot start_slot, u32** counts, i64** start) {
    void *c, *s;
    PB3D_TRY(pb3d_scratch(ctx, count_slot, (size_t)g.ncells * sizeof(u32), &c));
    PB3D_TRY(pb3d_scratch(ctx, start_slot, (size_t)(g.ncells + 1) * sizeof(i64), &s));
    PB3D_HIP(hipMemsetAsync(c, 0, (size_t)g.ncells * sizeof(u32), ctx->stream));
    hipLaunchKernelGGL(k_cell_count<F64>, dim3(pb3d_stream_blocks(ctx, n, 256, 8)), dim3(256), 0, ctx->stream, d_pts, n, g, (u32*)c);
    PB3D_CHECK_LAUNCH();
    PB3D_TRY(pb3d_scan_counts(ctx, (const u32*)c, g.ncells, (i64*)s, PB3D_SLOT_NN_SCAN_LOCAL, PB3D_SLOT_NN_SCAN_SEGS));
    PB3D_HIP(hipMemsetAsync(c, 0, (size_t)g.ncells * sizeof(u32), ctx->stream));      // the scatter's cursors
    *counts = (u32*)c;
    *start = (i64*)s;
    return PB3D_OK;
}

// the reference set's exact box, read back once, and the cell grid made from it
int grid_of(pb3d_ctx* ctx, const void* d_r, int r_f64, i64 nr, Grid* g) {
    double b[6];
    PB3D_TRY(pb3d_points_box(ctx, d_r, r_f64, nr, PB3D_SLOT_NN_BOUNDS, b));
    *g = make_grid(b, nr);
    return PB3D_OK;
}

// The host pipeline of a search is grid_of, then two halves.  The reference half bins the reference list on the grid of ix and scatters
// it into cell-sorted arrays in the caller's slots (ids_slot null: no ids) -> the rest of ix.
template <bool F64>
int index_reference_t(pb3d_ctx* ctx, const void* d_r, i64 nr, pb3d_slot starts_slot, pb3d_slot coords_slot, const pb3d_slot* ids_slot,
                      pb3d_nn_index* ix) {
    u32* rc;
    i64* rs;
    void *soa, *idbuf = nullptr;
    PB3D_TRY(bin_points<F64>(ctx, d_r, nr, ix->g, PB3D_SLOT_NN_REF_COUNTS, starts_slot, &rc, &rs));
    PB3D_TRY(pb3d_scratch(ctx, coords_slot, (size_t)nr * 3 * sizeof(double), &soa));
    if (ids_slot) PB3D_TRY(pb3d_scratch(ctx, *ids_slot, (size_t)nr * sizeof(int), &idbuf));
    double* xs = (double*)soa;
    hipLaunchKernelGGL(k_cell_scatter_ref<F64>, dim3(pb3d_stream_blocks(ctx, nr, 256, 8)), dim3(256), 0, ctx->stream, d_r, nr, ix->g,
                       (const i64*)rs, rc, xs, xs + nr, xs + 2 * nr, (int*)idbuf);
    PB3D_CHECK_LAUNCH();
    ix->nr = nr;
    ix->starts = rs;
    ix->xs = xs;
    ix->ids = (const int*)idbuf;
    return PB3D_OK;
}
int index_reference(pb3d_ctx* ctx, const void* d_r, int r_f64, i64 nr, pb3d_slot starts_slot, pb3d_slot coords_slot, const pb3d_slot* ids_slot,
                    pb3d_nn_index* ix) {
    return r_f64 ? index_reference_t<true>(ctx, d_r, nr, starts_slot, coords_slot, ids_slot, ix)
                 : index_reference_t<false>(ctx, d_r, nr, starts_slot, coords_slot, ids_slot, ix);
}

// The query half: the queries' positions in the cell order of grid g -> PB3D_SLOT_NN_ORDER
template <bool F64>
int order_queries_t(pb3d_ctx* ctx, const void* d_q, i64 nq, const Grid& g, const u32** order) {
    u32* qc;
    i64* qs;
    void* o;
    PB3D_TRY(bin_points<F64>(ctx, d_q, nq, g, PB3D_SLOT_NN_QUERY_COUNTS, PB3D_SLOT_NN_QUERY_STARTS, &qc, &qs));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_NN_ORDER, (size_t)nq * sizeof(u32), &o));
    hipLaunchKernelGGL(k_cell_scatter_query<F64>, dim3(pb3d_stream_blocks(ctx, nq, 256, 8)), dim3(256), 0, ctx->stream, d_q, nq, g,
                       (const i64*)qs, qc, (u32*)o);
    PB3D_CHECK_LAUNCH();
    *order = (const u32*)o;
    return PB3D_OK;
}
int order_queries(pb3d_ctx* ctx, const void* d_q, int q_f64, i64 nq, const Grid& g, const u32** order) {
    return q_f64 ? order_queries_t<true>(ctx, d_q, nq, g, order) : order_queries_t<false>(ctx, d_q, nq, g, order);
}

// one lane per query, in the cell order
template <int K>
int launch_nn(pb3d_ctx* ctx, const pb3d_nn_index& ix, const void* d_q, int q_f64, i64 nq, const u32* order, double* d_out) {
    hipLaunchKernelGGL((q_f64 ? k_nn_query<K, true> : k_nn_query<K, false>), dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, ctx->stream,
                       d_q, nq, order, ix.g, ix.starts, ix.xs, ix.xs + ix.nr, ix.xs + 2 * ix.nr, d_out);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}
template <int KC>
int launch_knn(pb3d_ctx* ctx, const pb3d_nn_index& ix, const void* d_q, int q_f64, i64 nq, const u32* order, int k, double* d_dist,
               int* d_idx) {
    hipLaunchKernelGGL((q_f64 ? k_knn_query<KC, true> : k_knn_query<KC, false>), dim3((unsigned)((nq + 255) / 256)), dim3(256), 0,
                       ctx->stream, d_q, nq, order, ix.g, ix.starts, ix.xs, ix.xs + ix.nr, ix.xs + 2 * ix.nr, ix.ids, k, d_dist, d_idx);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

}  // namespace

int pb3d_points_box(pb3d_ctx* ctx, const void* d_pts, int f64, i64 n, pb3d_slot slot, double b[6]) {
    void* bb;
    PB3D_TRY(pb3d_scratch(ctx, slot, 6 * sizeof(double), &bb));
    PB3D_TRY(launch_bounds(ctx, d_pts, f64, n, (double*)bb));
    return pb3d_read_back(ctx, b, bb, 6 * sizeof(double));
}

// ---- the index kept between calls (csrc/icp.hip): pb3d_knn_dev's two halves, the reference half into the caller's slots ------------
int pb3d_nn_index_build(pb3d_ctx* ctx, const void* d_r, int r_f64, i64 nr, pb3d_slot starts_slot, pb3d_slot coords_slot, pb3d_slot ids_slot,
                        pb3d_nn_index* ix) {
    return pb3d_nn_index_build_edge(ctx, d_r, r_f64, nr, 0.0, starts_slot, coords_slot, ids_slot, ix);
}

// ... with cells whose edge exceeds min_edge where min_edge > 0 (coarsen_grid; csrc/cluster.hip: the radius of a fixed-radius search)
int pb3d_nn_index_build_edge(pb3d_ctx* ctx, const void* d_r, int r_f64, i64 nr, double min_edge, pb3d_slot starts_slot, pb3d_slot coords_slot,
                             pb3d_slot ids_slot, pb3d_nn_index* ix) {
    PB3D_TRY(grid_of(ctx, d_r, r_f64, nr, &ix->g));
    if (min_edge > 0.0) coarsen_grid(ix->g, min_edge);
    return index_reference(ctx, d_r, r_f64, nr, starts_slot, coords_slot, &ids_slot, ix);
}

int pb3d_nn_index_nearest(pb3d_ctx* ctx, const pb3d_nn_index& ix, const double* d_q, i64 nq, int* d_idx) {
    const u32* order;
    PB3D_TRY(order_queries(ctx, d_q, 1, nq, ix.g, &order));
    return launch_knn<8>(ctx, ix, d_q, 1, nq, order, 1, nullptr, d_idx);
}

// the query half alone, on the caller's grid (csrc/meshdist.hip: its cells hold triangles, its queries are ordered like any other)
int pb3d_nn_order_queries(pb3d_ctx* ctx, const void* d_q, int q_f64, i64 nq, const pb3d_nn_grid& g, const u32** order) {
    return order_queries(ctx, d_q, q_f64, nq, g, order);
}

extern "C" {

int pb3d_points_bounds_dev(pb3d_ctx* ctx, const void* d_pts, int pts_f64, int64_t n, double* d_out) {
    PB3D_REQUIRE(n >= 1 && n <= pb3d_max_points, "pb3d_points_bounds: need 1 <= n <= 2^31 - 1 points (got %lld)", (long long)n);
    PB3D_REQUIRE(d_pts != nullptr && d_out != nullptr, "pb3d_points_bounds: null buffer");
    PB3D_REQUIRE(ctx != nullptr, "pb3d_points_bounds: null context");
    return launch_bounds(ctx, d_pts, pts_f64, n, d_out);
}

int pb3d_nn_dist_dev(pb3d_ctx* ctx, const void* d_q, int q_f64, int64_t nq, const void* d_r, int r_f64, int64_t nr, int k, double* d_out) {
    PB3D_REQUIRE(k == 1 || k == 2, "pb3d_nn_dist: k must be 1 or 2 (got %d)", k);
    PB3D_REQUIRE(nq >= 0 && nr >= 0, "pb3d_nn_dist: negative point count");
    PB3D_REQUIRE(nq <= pb3d_max_points && nr <= pb3d_max_points, "pb3d_nn_dist: at most 2^31 - 1 points per set");
    if (nq == 0) return PB3D_OK;
    PB3D_REQUIRE(nr >= k, "pb3d_nn_dist: the reference set needs at least k = %d points (got %lld)", k, (long long)nr);
    PB3D_REQUIRE(d_q != nullptr && d_r != nullptr && d_out != nullptr, "pb3d_nn_dist: null buffer");
    PB3D_REQUIRE(ctx != nullptr, "pb3d_nn_dist: null context");
    pb3d_nn_index ix;
    const u32* order;
    PB3D_TRY(grid_of(ctx, d_r, r_f64, nr, &ix.g));
    PB3D_TRY(index_reference(ctx, d_r, r_f64, nr, PB3D_SLOT_NN_REF_STARTS, PB3D_SLOT_NN_REF_COORDS, nullptr, &ix));
    PB3D_TRY(order_queries(ctx, d_q, q_f64, nq, ix.g, &order));
    return k == 1 ? launch_nn<1>(ctx, ix, d_q, q_f64, nq, order, d_out) : launch_nn<2>(ctx, ix, d_q, q_f64, nq, order, d_out);
}

int pb3d_knn_dev(pb3d_ctx* ctx, const void* d_q, int q_f64, int64_t nq, const void* d_r, int r_f64, int64_t nr, int k, double* d_dist,
                 int32_t* d_idx) {
    PB3D_REQUIRE(k >= 1 && k <= PB3D_KNN_MAX_K, "pb3d_knn: k must be in [1, %d] (got %d)", PB3D_KNN_MAX_K, k);
    PB3D_REQUIRE(nq >= 0 && nr >= 0, "pb3d_knn: negative point count");
    PB3D_REQUIRE(nq <= pb3d_max_points && nr <= pb3d_max_points, "pb3d_knn: at most 2^31 - 1 points per set");
    if (nq == 0) return PB3D_OK;
    PB3D_REQUIRE(nr >= k, "pb3d_knn: the reference set needs at least k = %d points (got %lld)", k, (long long)nr);
    PB3D_REQUIRE(d_q != nullptr && d_r != nullptr && d_idx != nullptr, "pb3d_knn: null buffer");
    PB3D_REQUIRE(ctx != nullptr, "pb3d_knn: null context");
    pb3d_nn_index ix;
    const u32* order;
    PB3D_TRY(pb3d_nn_index_build(ctx, d_r, r_f64, nr, PB3D_SLOT_NN_REF_STARTS, PB3D_SLOT_NN_REF_COORDS, PB3D_SLOT_KNN_REF_IDS, &ix));
    PB3D_TRY(order_queries(ctx, d_q, q_f64, nq, ix.g, &order));
    if (k <= 8) return launch_knn<8>(ctx, ix, d_q, q_f64, nq, order, k, d_dist, d_idx);
    if (k <= 20) return launch_knn<20>(ctx, ix, d_q, q_f64, nq, order, k, d_dist, d_idx);
    return launch_knn<32>(ctx, ix, d_q, q_f64, nq, order, k, d_dist, d_idx);
}

// the index size of the last pb3d_nn_dist_dev-shaped call on nr reference points with this box (cells per axis; tools/opbench.py)
int pb3d_nn_grid_shape(const double bounds[6], int64_t nr, int64_t cells[3]) {
    PB3D_REQUIRE(bounds != nullptr && cells != nullptr && nr >= 1, "pb3d_nn_grid_shape: bad argument");
    const Grid g = make_grid(bounds, nr);
    for (int a = 0; a < 3; ++a) cells[a] = g.n[a];
    return PB3D_OK;
}

int pb3d_voxel_iou_counts_dev(pb3d_ctx* ctx, const void* d_a, int a_f64, int64_t na, const void* d_b, int b_f64, int64_t nb,
                              const double bounds_min[3], double step, int calc_f32, int resolution, int iters, int64_t* d_counts) {
    PB3D_REQUIRE(resolution >= 1 && resolution <= kMaxResolution, "pb3d_voxel_iou_counts: resolution must be in [1, %d] (got %d)",
                 kMaxResolution, resolution);
    PB3D_REQUIRE(iters >= 0, "pb3d_voxel_iou_counts: iters must be >= 0 (got %d)", iters);
    PB3D_REQUIRE(na >= 0 && nb >= 0, "pb3d_voxel_iou_counts: negative point count");
    PB3D_REQUIRE(na <= pb3d_max_points && nb <= pb3d_max_points, "pb3d_voxel_iou_counts: at most 2^31 - 1 points per set");
    PB3D_REQUIRE((na == 0 || d_a) && (nb == 0 || d_b) && bounds_min && d_counts, "pb3d_voxel_iou_counts: null buffer");
    PB3D_REQUIRE(!calc_f32 || (!a_f64 && !b_f64), "pb3d_voxel_iou_counts: float32 arithmetic needs float32 points");
    PB3D_REQUIRE(ctx != nullptr, "pb3d_voxel_iou_counts: null context");
    Occ o;
    o.res = resolution;
    o.W = (resolution + 31) / 32;
    for (int a = 0; a < 3; ++a) o.lo[a] = bounds_min[a];
    o.step = step;
    const i64 gw = (i64)resolution * resolution * o.W;      // words of one bit grid
    void *buf, *tmp;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_VIOU_BITS, (size_t)gw * 2 * sizeof(u32), &buf));
    u32* bits = (u32*)buf;
    PB3D_HIP(hipMemsetAsync(bits, 0, (size_t)gw * 2 * sizeof(u32), ctx->stream));
    if (calc_f32) {
        PB3D_TRY(launch_occ<true>(ctx, d_a, a_f64, na, o, bits));
        PB3D_TRY(launch_occ<true>(ctx, d_b, b_f64, nb, o, bits + gw));
    } else {
        PB3D_TRY(launch_occ<false>(ctx, d_a, a_f64, na, o, bits));
        PB3D_TRY(launch_occ<false>(ctx, d_b, b_f64, nb, o, bits + gw));
    }
    // the dilated set is the L1 ball of radius iters clipped to the grid: it stops changing after 3 (res - 1) passes
    const int passes = iters < 3 * (resolution - 1) ? iters : 3 * (resolution - 1);
    if (passes > 0) {
        PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_VIOU_DILATED, (size_t)gw * 2 * sizeof(u32), &tmp));
        const u32 lastmask = (resolution & 31) ? (1u << (resolution & 31)) - 1u : 0xffffffffu;
        u32 *src = bits, *dst = (u32*)tmp;
        for (int p = 0; p < passes; ++p) {
            hipLaunchKernelGGL(k_dilate6, dim3((unsigned)((2 * gw + 255) / 256)), dim3(256), 0, ctx->stream, (const u32*)src, dst, resolution,
                               o.W, 2 * gw, lastmask);
            PB3D_CHECK_LAUNCH();
            u32* t = src; src = dst; dst = t;
        }
        bits = src;
    }
    PB3D_HIP(hipMemsetAsync(d_counts, 0, 2 * sizeof(int64_t), ctx->stream));
    hipLaunchKernelGGL(k_iou_count, dim3(pb3d_stream_blocks(ctx, gw, 256, 4)), dim3(256), 0, ctx->stream, (const u32*)bits,
                       (const u32*)(bits + gw), gw, (unsigned long long*)d_counts);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

}  // extern "C"
