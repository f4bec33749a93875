// voxel_downsample: voxel-grid downsampling of a point cloud (include/pb3d.h has the rules to the bit; DESIGN.md "Voxel downsampling"
// has why a hash and not a sort of the keys, and why voxels are numbered by first appearance).
//
// A voxel is a sparse 63-bit key (cx << 42) | (cy << 21) | cz, so nothing here bins densely: one path serves every voxel size.
//   k_voxel_insert    every point finds or claims the slot of its key in an open-addressing table (64-bit atomicCAS, linear probing,
//                     load <= 1/2), remembers the slot, and the slot keeps the smallest position (atomicMin) and the number (atomicAdd)
//                     of its points -- integers, so the order of the atomics leaves no trace.  Key, position and number share one
//                     16-byte record: the table is far larger than the caches and every touch of it is a random line
//   k_voxel_flags     flag[i] = point i is its slot's smallest position: the voxel's first appearance
//   pb3d_scan_counts  rank[i] = flags below i: the voxel number of a first point; rank[n] = m (read back: the second host wait, after
//                     the bounding box that RANGE is decided from)
//   k_voxel_number    inverse[i] = rank[first[slot[i]]]; a first point also writes index, counts and, for reduce = first, its row
// reduce = centroid adds each voxel's points in ascending position, which no atomic can do.  The (voxel, position) pairs, in position
// order to begin with, go through a stable LSD radix sort on the voxel number (pb3d_sort_pairs, csrc/sort_pairs.hip: 8-bit digits over
// the bits m - 1 needs, one pass for up to 256 voxels, four at most), which leaves every voxel's positions ascending and the voxels in
// order, with no per-voxel state: a voxel that holds the whole cloud is sorted like any other.
//   k_voxel_centroid  one wavefront per voxel: the ordered wavefront sum of csrc/ordered_sum.h (which states the order of the additions)
//                     over the voxel's positions, then one correctly rounded division
// No floating-point atomic anywhere, and -ffp-contract=off (Makefile) keeps the additions apart.
#include <algorithm>
#include <cmath>

#include "ordered_sum.h"
#include "pb3d_internal.h"

namespace {

constexpr double kCells = 2097152.0;                // 2^21 cells per axis
constexpr u64 kEmpty = ~0ull;                       // no key has bit 63

struct Vox { double o[3], size; };
// one slot of the table: the three words a point touches share a 16-byte record, so an insertion lands in one cache line
struct alignas(16) Slot { u64 key; u32 first, cnt; };   // the voxel's key, the smallest position and the number of its points

// CELL, clamped into [0, 2^21): the host has refused every cloud whose finite points leave that range, so the clamp moves nothing
// it accepted; a NaN (a resident caller's) fails the first comparison and lands in cell 0 -- a wrong answer, never a wild key
__device__ __forceinline__ u64 cell_of(double p, double o, double size) {
    double c = floor(__ddiv_rn(p - o, size));
    if (!(c >= 0.0)) c = 0.0;
    if (c > kCells - 1.0) c = kCells - 1.0;
    return (u64)c;
}

__global__ __launch_bounds__(256) void k_table_clear(Slot* table, u64 cap) {
    for (u64 s = (u64)blockIdx.x * 256 + threadIdx.x; s < cap; s += (u64)gridDim.x * 256) table[s] = {kEmpty, 0xffffffffu, 0u};
}

// cap: a power of two >= 2 n, so at most half the slots are ever claimed and a probe always ends
template <bool F64>
__global__ __launch_bounds__(256) void k_voxel_insert(const void* __restrict__ pts, i64 n, Vox vx, Slot* table, u64 cap, u32* __restrict__ slot_of) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double p[3];
    pb3d_load3<F64>(pts, i, p);
    const u64 key = (cell_of(p[0], vx.o[0], vx.size) << 42) | (cell_of(p[1], vx.o[1], vx.size) << 21) | cell_of(p[2], vx.o[2], vx.size);
    u64 s = pb3d_mix64(key) & (cap - 1);
    while (true) {
        u64 cur = __hip_atomic_load(&table[s].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == kEmpty) cur = atomicCAS((unsigned long long*)&table[s].key, (unsigned long long)kEmpty, (unsigned long long)key);
        if (cur == kEmpty || cur == key) break;
        s = (s + 1) & (cap - 1);
    }
    slot_of[i] = (u32)s;
    // one pair of atomics per run of neighbouring lanes in one slot.  Lanes ascend in position, so a run's first lane holds its smallest;
    // the lanes that left above (i >= n) are the wave's last, so the active ones are lanes 0 .. popc(active) - 1.  A cloud that comes
    // in scan order (a voxel grid's points, a depth image's) sends one pair for 2 to 64 points, a shuffled one loses nothing
    const int lane = threadIdx.x & 63;
    const unsigned long long active = __ballot(1);
    const u32 prev = (u32)__shfl_up((int)(u32)s, 1);
    const bool head = lane == 0 || prev != (u32)s;
    const unsigned long long heads = __ballot(head);
    if (head) {
        const unsigned long long above = heads & ~((2ull << lane) - 1ull);     // the heads after this lane
        const int next = above ? __ffsll(above) - 1 : __popcll(active);
        atomicMin(&table[s].first, (u32)i);
        atomicAdd(&table[s].cnt, (u32)(next - lane));
    }
}

__global__ __launch_bounds__(256) void k_voxel_flags(i64 n, const u32* __restrict__ slot_of, const Slot* __restrict__ table, u32* __restrict__ flag) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i < n) flag[i] = table[slot_of[i]].first == (u32)i ? 1u : 0u;
}

// inverse, counts, out, key and val may each be null (not asked for).  T is the row type: rows are copied element by element, so
// neither list needs more than its element's alignment
template <class T>
__global__ __launch_bounds__(256) void k_voxel_number(const T* __restrict__ pts, i64 n, const u32* __restrict__ slot_of,
                                                      const Slot* __restrict__ table, const i64* __restrict__ rank, int* __restrict__ index,
                                                      int* __restrict__ inverse, u32* __restrict__ counts, T* __restrict__ out,
                                                      u32* __restrict__ key, u32* __restrict__ val) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const Slot slot = table[slot_of[i]];
    const u32 f = slot.first;
    const i64 v = rank[f];
    if (inverse) inverse[i] = (int)v;
    if (key) { key[i] = (u32)v; val[i] = (u32)i; }
    if (f == (u32)i) {
        index[v] = (int)i;
        if (counts) counts[v] = slot.cnt;
        if (out)
            for (int a = 0; a < 3; ++a) out[3 * v + a] = pts[3 * i + a];
    }
}

// ---- centroids --------------------------------------------------------------------------------------------------------------------------
// start[v] .. start[v + 1]: voxel v's run of pos[], ascending positions.  However long the run, the wavefront walks it 64 a time
template <bool F64>
__global__ __launch_bounds__(256) void k_voxel_centroid(const void* __restrict__ pts, const u32* __restrict__ pos, const i64* __restrict__ start, i64 m,
                                                        void* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const i64 v = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) + (i64)blockIdx.x * 4;
    if (v >= m) return;
    const i64 s = start[v], e = start[v + 1];
    double sum[3];
    ordered_sum(s, e, [&](i64 p, double* row) { pb3d_load3<F64>(pts, (i64)pos[p], row); }, sum);
    if (lane < 3) {
        const double q = __ddiv_rn(sum[lane], (double)(e - s));
        if (F64) ((double*)out)[3 * v + lane] = q;
        else ((float*)out)[3 * v + lane] = (float)q;      // the one rounding to float32
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------------
double host_cell(double p, double o, double size) { return std::floor((p - o) / size); }

template <class T>
int launch_number(pb3d_ctx* ctx, const void* d_pts, i64 n, const u32* slot_of, const Slot* table, const i64* rank, int* index, int* inverse,
                  u32* counts, void* out, u32* key, u32* val) {
    hipLaunchKernelGGL(k_voxel_number<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (const T*)d_pts, n, slot_of, table, rank, index,
                       inverse, counts, (T*)out, key, val);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

}  // namespace

extern "C" int pb3d_voxel_downsample_resident(pb3d_ctx* ctx, const void* d_pts, int pts_f64, int64_t n, double voxel_size, const double origin[3],
                                              int reduce, void* d_out, int32_t* d_index, int32_t* d_inverse, uint32_t* d_counts,
                                              int64_t* nvoxels) {
    PB3D_REQUIRE(n >= 0 && n <= pb3d_max_points, "pb3d_voxel_downsample: need 0 <= n <= 2^31 - 1 points (got %lld)", (long long)n);
    PB3D_REQUIRE(voxel_size > 0.0 && std::isfinite(voxel_size), "pb3d_voxel_downsample: voxel_size must be finite and > 0 (got %g)", voxel_size);
    PB3D_REQUIRE(origin == nullptr || (std::isfinite(origin[0]) && std::isfinite(origin[1]) && std::isfinite(origin[2])),
                 "pb3d_voxel_downsample: origin must be finite");
    PB3D_REQUIRE(reduce == PB3D_DOWNSAMPLE_CENTROID || reduce == PB3D_DOWNSAMPLE_FIRST,
                 "pb3d_voxel_downsample: reduce must be 0 (centroid) or 1 (first) (got %d)", reduce);
    PB3D_REQUIRE(nvoxels != nullptr, "pb3d_voxel_downsample: null argument");
    PB3D_REQUIRE(n == 0 || (d_pts != nullptr && d_out != nullptr && d_index != nullptr), "pb3d_voxel_downsample: null buffer");
    PB3D_REQUIRE(ctx != nullptr, "pb3d_voxel_downsample: null context");
    *nvoxels = 0;
    if (n == 0) return PB3D_OK;

    // the exact bounds (first host wait) decide ORIGIN and RANGE: subtraction, division and floor are monotone, so the cells of lo and
    // hi enclose every point's
    double b[6];
    PB3D_TRY(pb3d_points_box(ctx, d_pts, pts_f64, n, PB3D_SLOT_DOWNSAMPLE_BOUNDS, b));
    Vox vx;
    vx.size = voxel_size;
    const double h = 0.5 * voxel_size;
    for (int a = 0; a < 3; ++a) {
        vx.o[a] = origin ? origin[a] : b[a] - h;
        const double c0 = host_cell(b[a], vx.o[a], voxel_size), c1 = host_cell(b[3 + a], vx.o[a], voxel_size);
        PB3D_REQUIRE(c0 >= 0.0 && c0 < kCells && c1 >= 0.0 && c1 < kCells,
                     "pb3d_voxel_downsample: the cloud leaves cells [0, 2^21) of the voxel grid on axis %d (its cells span %g .. %g): "
                     "choose a larger voxel_size, or an origin at or below the cloud's minimum", a, c0, c1);
    }

    u64 cap = 64;
    while (cap < 2 * (u64)n) cap <<= 1;
    const bool centroid = reduce == PB3D_DOWNSAMPLE_CENTROID;
    void *tab, *slot_of, *flags, *ranks;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_DOWNSAMPLE_TABLE, (size_t)cap * sizeof(Slot), &tab));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_DOWNSAMPLE_POINT_SLOT, (size_t)n * sizeof(u32), &slot_of));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_DOWNSAMPLE_FLAGS, (size_t)n * sizeof(u32), &flags));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_DOWNSAMPLE_RANKS, (size_t)(n + 1) * sizeof(i64), &ranks));
    if (centroid)       // the largest scan of the call may be the sort's: size both scan slots for it now, so none regrows (and waits) midway
        PB3D_TRY(pb3d_scan_reserve(ctx, std::max<i64>(n, pb3d_sort_scan_items(n)), PB3D_SLOT_DOWNSAMPLE_SCAN_LOCAL, PB3D_SLOT_DOWNSAMPLE_SCAN_SEGS));
    Slot* table = (Slot*)tab;
    hipLaunchKernelGGL(k_table_clear, dim3(pb3d_stream_blocks(ctx, (i64)cap, 256, 8)), dim3(256), 0, ctx->stream, table, cap);
    PB3D_CHECK_LAUNCH();
    const dim3 grid((unsigned)((n + 255) / 256));
    hipLaunchKernelGGL((pts_f64 ? k_voxel_insert<true> : k_voxel_insert<false>), grid, dim3(256), 0, ctx->stream, d_pts, (i64)n, vx, table, cap,
                       (u32*)slot_of);
    PB3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_voxel_flags, grid, dim3(256), 0, ctx->stream, (i64)n, (const u32*)slot_of, (const Slot*)table, (u32*)flags);
    PB3D_CHECK_LAUNCH();
    PB3D_TRY(pb3d_scan_counts(ctx, (const u32*)flags, n, (i64*)ranks, PB3D_SLOT_DOWNSAMPLE_SCAN_LOCAL, PB3D_SLOT_DOWNSAMPLE_SCAN_SEGS));
    i64 m;
    PB3D_TRY(pb3d_read_back(ctx, &m, (const i64*)ranks + n, sizeof(i64)));

    // the flags are spent: a centroid call without d_counts keeps its counts there
    u32* counts = d_counts ? d_counts : centroid ? (u32*)flags : nullptr;
    u32* pairs = nullptr;
    if (centroid) {
        void* kv;
        PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_DOWNSAMPLE_SORT_PAIRS, (size_t)n * 4 * sizeof(u32), &kv));
        pairs = (u32*)kv;
    }
    void* first_rows = centroid ? nullptr : d_out;
    if (pts_f64)
        PB3D_TRY(launch_number<double>(ctx, d_pts, n, (const u32*)slot_of, table, (const i64*)ranks, d_index, d_inverse, counts, first_rows, pairs,
                                       pairs ? pairs + n : nullptr));
    else
        PB3D_TRY(launch_number<float>(ctx, d_pts, n, (const u32*)slot_of, table, (const i64*)ranks, d_index, d_inverse, counts, first_rows, pairs,
                                      pairs ? pairs + n : nullptr));
    if (centroid) {
        // the ranks are spent too: the list starts (m + 1 <= n + 1 int64) take their place
        PB3D_TRY(pb3d_scan_counts(ctx, counts, m, (i64*)ranks, PB3D_SLOT_DOWNSAMPLE_SCAN_LOCAL, PB3D_SLOT_DOWNSAMPLE_SCAN_SEGS));
        const u32* sorted;
        PB3D_TRY(pb3d_sort_pairs(ctx, pairs, pairs + n, pairs + 2 * n, pairs + 3 * n, n, m, PB3D_SLOT_DOWNSAMPLE_SORT_HIST,
                                 PB3D_SLOT_DOWNSAMPLE_SCAN_LOCAL, PB3D_SLOT_DOWNSAMPLE_SCAN_SEGS, nullptr, &sorted));
        hipLaunchKernelGGL((pts_f64 ? k_voxel_centroid<true> : k_voxel_centroid<false>), dim3((unsigned)((m + 3) / 4)), dim3(256), 0, ctx->stream, d_pts,
                           sorted, (const i64*)ranks, m, d_out);
        PB3D_CHECK_LAUNCH();
    }
    *nvoxels = m;
    return PB3D_OK;
}
