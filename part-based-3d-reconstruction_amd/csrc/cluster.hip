// cluster_points: exact DBSCAN of a point cloud, and the fixed-radius neighbour counts it starts from (include/pb3d.h has the semantics
// to the bit; DESIGN.md "Clustering" has the determinism argument).  The segmentation step of the inter-method preprocessing.
//
// The cloud is indexed against itself with the cell index of csrc/nn.hip, and every pass is one ring_walk (csrc/ring_walk.h) per point in
// cell order with a constant pruning bound, eps * eps:
//   k_radius_count     counts[p] = #{q : d2(p, q) <= eps2} (p itself included), core[p] = counts[p] >= min_samples, parent[p] = p
//   k_cluster_union    a core point unites itself with every core neighbour of smaller position in a lock-free union-find over parent[]
//                      (the larger root always goes under the smaller, atomicMin): runs after ALL core flags are written
//   k_cluster_flatten  parent[p] = root of p; flag[p] = p is a core root
//   pb3d_scan_counts   rank[p] = number of core roots below p: the cluster number of root p; rank[n] = the number of clusters (read
//                      back: the call's second host wait, after the index's bounding box)
//   k_cluster_labels   core: rank[parent[p]].  Non-core with counts > 1: a third walk for the smallest root among its core neighbours
//                      (rank order is root order), else -1.  sizes by integer atomics, one per run of equal labels in a wave.
// d2 is (dx*dx + dy*dy) + dz*dz in float64 with dx = p.x - q.x: the Makefile passes -ffp-contract=off, and the expression gives the
// same bits with p and q exchanged, so the neighbour relation is symmetric as computed.  The walk's pruning is strict with a margin
// (ring_walk.h: beyond), so a pair exactly at the threshold, or a point that rounding put in the next cell, is never skipped.
#include <cmath>

#include "pb3d_internal.h"
#include "ring_walk.h"
#include "union_find.h"

namespace {

struct Sorted { const double *xs, *ys, *zs; const int* ids; };     // the cell-sorted arrays of the index

// ---- what each walk keeps.  bound() is the constant eps2 for all three: the walk visits every cell that can hold a neighbour ----------
struct CountBest {
    double eps2;
    u32 cnt;
    __device__ __forceinline__ double bound() const { return eps2; }
    __device__ __forceinline__ void visit(const Sorted& pts, i64 s, i64 e, const double (&q)[3]) {
        for (i64 p = s; p < e; ++p) {
            const double dx = q[0] - pts.xs[p], dy = q[1] - pts.ys[p], dz = q[2] - pts.zs[p];
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            cnt += d2 <= eps2 ? 1u : 0u;
        }
    }
};

struct UnionBest {
    double eps2;
    int me;                 // the walking core point's position in the caller's list
    const u8* core;
    int* parent;
    __device__ __forceinline__ double bound() const { return eps2; }
    __device__ __forceinline__ void visit(const Sorted& pts, i64 s, i64 e, const double (&q)[3]) {
#pragma nounroll
        for (i64 p = s; p < e; ++p) {
            const double dx = q[0] - pts.xs[p], dy = q[1] - pts.ys[p], dz = q[2] - pts.zs[p];
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            if (d2 <= eps2) {
                const int j = pts.ids[p];
                if (j < me && core[j]) uf_union(parent, me, j);
            }
        }
    }
};

struct BorderBest {
    double eps2;
    const u8* core;
    const int* root;        // the flattened forest
    int best;               // the smallest root among the core neighbours so far
    __device__ __forceinline__ double bound() const { return eps2; }
    __device__ __forceinline__ void visit(const Sorted& pts, i64 s, i64 e, const double (&q)[3]) {
        for (i64 p = s; p < e; ++p) {
            const double dx = q[0] - pts.xs[p], dy = q[1] - pts.ys[p], dz = q[2] - pts.zs[p];
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            if (d2 <= eps2) {
                const int j = pts.ids[p];
                if (core[j]) best = min(best, root[j]);
            }
        }
    }
};

struct Index { Grid g; const i64* start; Sorted pts; };

// core == null: the counts alone (pb3d_radius_count_resident)
template <bool F64>
__global__ __launch_bounds__(256) void k_radius_count(const void* __restrict__ q, i64 n, const u32* __restrict__ order, Index ix, double eps2,
                                                      i64 min_samples, u32* __restrict__ counts, u8* __restrict__ core, int* __restrict__ parent) {
    const i64 s = (i64)blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    const u32 qi = order[s];
    double qv[3];
    pb3d_load3<F64>(q, qi, qv);
    CountBest best = {eps2, 0u};
    ring_walk(ix.g, ix.start, ix.pts, qv, best);
    counts[qi] = best.cnt;
    if (core) {
        core[qi] = (i64)best.cnt >= min_samples ? 1 : 0;
        parent[qi] = (int)qi;
    }
}

template <bool F64>
__global__ __launch_bounds__(256) void k_cluster_union(const void* __restrict__ q, i64 n, const u32* __restrict__ order, Index ix, double eps2,
                                                       const u8* __restrict__ core, int* parent) {
    const i64 s = (i64)blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    const u32 qi = order[s];
    if (!core[qi]) return;
    double qv[3];
    pb3d_load3<F64>(q, qi, qv);
    UnionBest best = {eps2, (int)qi, core, parent};
    ring_walk(ix.g, ix.start, ix.pts, qv, best);
}

// Every entry of the forest becomes its root.  The stores race with other lanes' searches, but each is an ancestor of its point and
// the last one is the root, so the result is the same whatever the order.
__global__ __launch_bounds__(256) void k_cluster_flatten(i64 n, const u8* __restrict__ core, int* parent, u32* __restrict__ root_flag) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    u32 flag = 0;
    if (core[i]) {
        int r = (int)i;
        for (int p = ld(&parent[r]); p != r; p = ld(&parent[r])) r = p;
        st(&parent[i], r);
        flag = r == (int)i;
    }
    root_flag[i] = flag;
}

// one 64-bit add per run of lanes that hold the first active lane's label, one per lane otherwise (a wave of one cluster's interior
// adds once).  Called where every lane that has not left the kernel is active.
__device__ __forceinline__ void add_size(unsigned long long* sizes, int lab) {
    if (lab < 0) return;
    const unsigned long long active = __ballot(1);
    const int first = __shfl(lab, __ffsll(active) - 1);
    const unsigned long long same = __ballot(lab == first);
    if (lab != first) atomicAdd(&sizes[lab], 1ull);
    else if ((int)(threadIdx.x & 63) == __ffsll(same) - 1) atomicAdd(&sizes[lab], (unsigned long long)__popcll(same));
}

template <bool F64>
__global__ __launch_bounds__(256) void k_cluster_labels(const void* __restrict__ q, i64 n, const u32* __restrict__ order, Index ix, double eps2,
                                                        const u8* __restrict__ core, const u32* __restrict__ counts, const int* __restrict__ root,
                                                        const i64* __restrict__ rank, int* __restrict__ labels, unsigned long long* sizes) {
    const i64 s = (i64)blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    const u32 qi = order[s];
    int r = 0x7fffffff;
    if (core[qi]) {
        r = root[qi];
    } else if (counts[qi] > 1u) {
        double qv[3];
        pb3d_load3<F64>(q, qi, qv);
        BorderBest best = {eps2, core, root, 0x7fffffff};
        ring_walk(ix.g, ix.start, ix.pts, qv, best);
        r = best.best;
    }
    const int lab = r == 0x7fffffff ? -1 : (int)rank[r];
    labels[qi] = lab;
    add_size(sizes, lab);
}

__global__ __launch_bounds__(256) void k_labels_member(const int* __restrict__ labels, i64 n, const u8* __restrict__ table, i64 nlabels,
                                                       u8* __restrict__ keep) {
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) {
        const int l = labels[i];
        keep[i] = l >= 0 && l < nlabels && table[l] ? 1 : 0;
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
// The index of the cloud against itself and the walk order.  Cell edge (knob "cluster_cell"): above eps where that is coarser than
// make_grid's two points per cell (a walk ends with the 27 cells around the query), unless the knob asks for make_grid's.
int build_index(pb3d_ctx* ctx, const void* d_pts, int f64, i64 n, double eps, Index* ix, const u32** order) {
    pb3d_nn_index nx;
    const double min_edge = ctx->tune_cluster_cell == 1 ? 0.0 : eps;
    PB3D_TRY(pb3d_nn_index_build_edge(ctx, d_pts, f64, n, min_edge, PB3D_SLOT_CLUSTER_STARTS, PB3D_SLOT_CLUSTER_COORDS, PB3D_SLOT_CLUSTER_IDS, &nx));
    PB3D_TRY(pb3d_nn_order_queries(ctx, d_pts, f64, n, nx.g, order));
    ix->g = nx.g;
    ix->start = nx.starts;
    ix->pts = {nx.xs, nx.xs + n, nx.xs + 2 * n, nx.ids};
    ctx->cluster_last.valid = true;
    ctx->cluster_last.timed = false;
    for (int a = 0; a < 3; ++a) ctx->cluster_last.cells[a] = nx.g.n[a];
    return PB3D_OK;
}

int check_args(const char* who, const void* d_pts, i64 n, double eps) {
    PB3D_REQUIRE(n >= 0 && n <= pb3d_max_points, "%s: need 0 <= n <= 2^31 - 1 points (got %lld)", who, (long long)n);
    PB3D_REQUIRE(eps > 0.0 && std::isfinite(eps), "%s: eps must be finite and > 0 (got %g)", who, eps);
    PB3D_REQUIRE(n == 0 || d_pts != nullptr, "%s: null buffer", who);
    return PB3D_OK;
}

}  // namespace

extern "C" {

int pb3d_radius_count_resident(pb3d_ctx* ctx, const void* d_pts, int pts_f64, int64_t n, double eps, uint32_t* d_counts) {
    PB3D_TRY(check_args("pb3d_radius_count", d_pts, n, eps));
    PB3D_REQUIRE(n == 0 || d_counts != nullptr, "pb3d_radius_count: null buffer");
    PB3D_REQUIRE(ctx != nullptr, "pb3d_radius_count: null context");
    if (n == 0) return PB3D_OK;
    Index ix;
    const u32* order;
    PB3D_TRY(build_index(ctx, d_pts, pts_f64, n, eps, &ix, &order));
    const double eps2 = eps * eps;
    hipLaunchKernelGGL((pts_f64 ? k_radius_count<true> : k_radius_count<false>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_pts,
                       (i64)n, order, ix, eps2, (i64)1, d_counts, (u8*)nullptr, (int*)nullptr);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

int pb3d_cluster_points_resident(pb3d_ctx* ctx, const void* d_pts, int pts_f64, int64_t n, double eps, int64_t min_samples, int32_t* d_labels,
                                 uint8_t* d_core, uint32_t* d_counts, int64_t* d_sizes, int64_t* nclusters) {
    PB3D_TRY(check_args("pb3d_cluster_points", d_pts, n, eps));
    PB3D_REQUIRE(min_samples >= 1, "pb3d_cluster_points: min_samples must be >= 1 (got %lld)", (long long)min_samples);
    PB3D_REQUIRE(nclusters != nullptr, "pb3d_cluster_points: null argument");
    PB3D_REQUIRE(n == 0 || (d_labels != nullptr && d_core != nullptr && d_counts != nullptr && d_sizes != nullptr),
                 "pb3d_cluster_points: null buffer");
    PB3D_REQUIRE(ctx != nullptr, "pb3d_cluster_points: null context");
    *nclusters = 0;
    if (n == 0) return PB3D_OK;
    pb3d_stamps<6> t = {ctx->tune_cluster_timing != 0, 0, {}};       // knob "cluster_timing"
    Index ix;
    const u32* order;
    void *parent, *flags, *ranks;
    PB3D_TRY(t.mark(ctx));
    PB3D_TRY(build_index(ctx, d_pts, pts_f64, n, eps, &ix, &order));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_CLUSTER_PARENT, (size_t)n * sizeof(int), &parent));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_CLUSTER_ROOT_FLAGS, (size_t)n * sizeof(u32), &flags));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_CLUSTER_RANKS, (size_t)(n + 1) * sizeof(i64), &ranks));
    const double eps2 = eps * eps;
    const dim3 grid((unsigned)((n + 255) / 256));
    PB3D_TRY(t.mark(ctx));
    hipLaunchKernelGGL((pts_f64 ? k_radius_count<true> : k_radius_count<false>), grid, dim3(256), 0, ctx->stream, d_pts, (i64)n, order, ix, eps2,
                       (i64)min_samples, d_counts, d_core, (int*)parent);
    PB3D_CHECK_LAUNCH();
    PB3D_TRY(t.mark(ctx));
    hipLaunchKernelGGL((pts_f64 ? k_cluster_union<true> : k_cluster_union<false>), grid, dim3(256), 0, ctx->stream, d_pts, (i64)n, order, ix, eps2,
                       (const u8*)d_core, (int*)parent);
    PB3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_cluster_flatten, grid, dim3(256), 0, ctx->stream, (i64)n, (const u8*)d_core, (int*)parent, (u32*)flags);
    PB3D_CHECK_LAUNCH();
    PB3D_TRY(t.mark(ctx));
    PB3D_TRY(pb3d_scan_counts(ctx, (const u32*)flags, n, (i64*)ranks, PB3D_SLOT_CLUSTER_SCAN_LOCAL, PB3D_SLOT_CLUSTER_SCAN_SEGS));
    i64 nc;
    PB3D_TRY(pb3d_read_back(ctx, &nc, (const i64*)ranks + n, sizeof(i64)));
    PB3D_TRY(t.mark(ctx));
    if (nc > 0) PB3D_HIP(hipMemsetAsync(d_sizes, 0, (size_t)nc * sizeof(int64_t), ctx->stream));
    hipLaunchKernelGGL((pts_f64 ? k_cluster_labels<true> : k_cluster_labels<false>), grid, dim3(256), 0, ctx->stream, d_pts, (i64)n, order, ix, eps2,
                       (const u8*)d_core, (const u32*)d_counts, (const int*)parent, (const i64*)ranks, (int*)d_labels,
                       (unsigned long long*)d_sizes);
    PB3D_CHECK_LAUNCH();
    PB3D_TRY(t.mark(ctx));
    PB3D_TRY(t.finish(ctx, ctx->cluster_last.ms, &ctx->cluster_last.timed));
    *nclusters = nc;
    return PB3D_OK;
}

int pb3d_labels_member_resident(pb3d_ctx* ctx, const int32_t* d_labels, int64_t n, const uint8_t* chosen, int64_t nlabels, uint8_t* d_keep) {
    PB3D_REQUIRE(n >= 0 && n <= pb3d_max_points, "pb3d_labels_member: need 0 <= n <= 2^31 - 1 labels (got %lld)", (long long)n);
    PB3D_REQUIRE(nlabels >= 0 && nlabels <= pb3d_max_points, "pb3d_labels_member: need 0 <= nlabels <= 2^31 - 1 (got %lld)", (long long)nlabels);
    PB3D_REQUIRE(nlabels == 0 || chosen != nullptr, "pb3d_labels_member: null argument");
    PB3D_REQUIRE(n == 0 || (d_labels != nullptr && d_keep != nullptr), "pb3d_labels_member: null buffer");
    PB3D_REQUIRE(ctx != nullptr, "pb3d_labels_member: null context");
    if (n == 0) return PB3D_OK;
    void* table;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_CLUSTER_CHOSEN, (size_t)(nlabels > 0 ? nlabels : 1), &table));
    PB3D_TRY(pb3d_h2d_async(ctx, table, chosen, (size_t)nlabels));
    hipLaunchKernelGGL(k_labels_member, dim3(pb3d_stream_blocks(ctx, n, 256, 8)), dim3(256), 0, ctx->stream, (const int*)d_labels, (i64)n,
                       (const u8*)table, (i64)nlabels, (u8*)d_keep);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

int pb3d_cluster_last(pb3d_ctx* ctx, int64_t cells[3], double pass_ms[5]) {
    PB3D_REQUIRE(ctx != nullptr && cells != nullptr, "pb3d_cluster_last: null argument");
    PB3D_REQUIRE(ctx->cluster_last.valid, "pb3d_cluster_last: no clustering has run on this context");
    for (int a = 0; a < 3; ++a) cells[a] = ctx->cluster_last.cells[a];
    if (pass_ms) {
        PB3D_REQUIRE(ctx->cluster_last.timed, "pb3d_cluster_last: the last clustering was not timed (knob cluster_timing)");
        for (int i = 0; i < 5; ++i) pass_ms[i] = ctx->cluster_last.ms[i];
    }
    return PB3D_OK;
}

}  // extern "C"
