// distance_transform: the exact Euclidean distance transform of a grid with its feature transform, the ball morphology built on it and
// the surface-distance sums of two grids (include/pb3d.h has the rules to the bit; DESIGN.md "Grid to distance" has the method).
//
// Integer arithmetic only.  Three separable passes, sq and the partial index ping-ponging between the caller's buffers and scratch:
//   k_edt_rows      axis 2.  A wavefront takes a row: it ballots 64 voxels at a time into occupancy words (for PB3D_EDT_TO_SURFACE also
//                   the AND of the four neighbouring rows' occupancy, and the row's own words shifted by one bit either way), keeps
//                   the row's target words in LDS, and every voxel finds the nearest set bit at or below and at or above it with
//                   clz / ctz: in its own word, else in the nearest non-empty word, which a 64-bit "word is not empty" mask per 64
//                   words names without a walk.  An equidistant pair goes to the left (smaller t2).  Writes (t2 - k)^2 and t2
//   k_edt_columns   axis 1, then axis 0.  One lane per column, lanes on consecutive voxels of the contiguous axis, so every load and
//                   store of the pass is coalesced.  Meijster's two scans: the forward scan keeps the lower envelope of the parabolas
//                   g(s) + (x - s)^2 on a stack of (s, t, g(s)), the backward scan reads the envelope off.  The stack of a column lies
//                   at the column's own voxels -- level l at voxel l: (s, t) packed in the OUTPUT buffer, g(s) in a scratch buffer --
//                   so it coalesces like the data.  The backward scan at voxel u holds a stack of at most u + 1 levels (t is strictly
//                   increasing from t[0] = 0, so level q has t >= q) and has its top in registers, so writing the result of voxel u
//                   never destroys a level still to be read.  Work is O(voxels) whatever the content: every voxel is pushed and popped
//                   at most once.  Ties go to the smaller s (Sep's floor), the stated tie rule.  A voxel whose g is PB3D_EDT_NONE is
//                   no parabola and is skipped, so PB3D_EDT_NONE never enters a sum.  The last pass applies the border and takes the
//                   maximum
//   k_edt_distances sqrt((double)sq) * voxel_size
//   k_edt_apply     PB3D_EDT_FILL / PB3D_EDT_KEEP
//   k_surface_stats count, max, sum and threshold counts of sq over the surface voxels of a grid
// Counts are integer atomics (add, max), one per workgroup of a capped grid.  No floating-point atomics anywhere.
#include <algorithm>
#include <cmath>

#include "pb3d_internal.h"
#include "wave.h"

namespace {

constexpr i64 kMaxVoxels = (1ll << 31) - 1;
constexpr int kNone = PB3D_EDT_NONE;
constexpr int kRowWords = PB3D_EDT_MAX_AXIS / 64;   // the 64-voxel words of the longest row
constexpr int kRowGroups = kRowWords / 64;          // ... and the 64-word groups of its "not empty" masks
constexpr int kAhead = 8;                           // g values a column lane requests ahead of its envelope
constexpr int kColLanes = 64;                       // columns per workgroup of the column passes: one wavefront, many workgroups per CU
constexpr int kAxisBits = 14;                       // s and t of a stack level are < 16384
static_assert((1 << kAxisBits) == PB3D_EDT_MAX_AXIS, "a stack level packs s and t in 14 bits each");

template <int CH>
__device__ __forceinline__ bool occupied(const u8* g, i64 v) {
    if (CH == 1) return g[v] != 0;
    const u8* p = g + 3 * v;
    return (p[0] | p[1] | p[2]) != 0;
}

// the largest w' < w (smallest w' > w) whose bit is set in the masks nz[0 .. kRowGroups), or -1
__device__ __forceinline__ int prev_word(const u64* nz, int w) {
    int g = w >> 6;
    u64 m = nz[g] & ((1ull << (w & 63)) - 1);
    while (true) {
        if (m) return g * 64 + 63 - __clzll((long long)m);
        if (--g < 0) return -1;
        m = nz[g];
    }
}
__device__ __forceinline__ int next_word(const u64* nz, int w) {
    int g = w >> 6;
    u64 m = (w & 63) == 63 ? 0 : nz[g] & (~0ull << ((w & 63) + 1));
    while (true) {
        if (m) return g * 64 + __ffsll((unsigned long long)m) - 1;
        if (++g >= kRowGroups) return -1;
        m = nz[g];
    }
}

// counts[0] += the targets.  sq: (t2 - k)^2 of the row's nearest target, feat: its t2
template <int CH, bool IDX>
__global__ __launch_bounds__(256) void k_edt_rows(const u8* __restrict__ grid, i64 n0, i64 n1, i64 n2, int target, int* __restrict__ sq,
                                                  int* __restrict__ feat, u64* __restrict__ counts) {
    __shared__ u64 occ[4][kRowWords], tgt[4][kRowWords], nzs[4][kRowGroups];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const i64 nrows = n0 * n1;
    const int nw = (int)((n2 + 63) >> 6);
    u64 ntargets = 0;
    // every wavefront of a workgroup makes the same number of rounds (the barriers), a wavefront past the last row idles in them
    for (i64 first = (i64)blockIdx.x * 4; first < nrows; first += (i64)gridDim.x * 4) {
        const i64 row = first + wave;
        const bool live = row < nrows;
        const i64 i = row / n1, j = row - i * n1;
        if (live) {
            for (int w = 0; w < nw; ++w) {
                const i64 k = (i64)w * 64 + lane;
                const bool in = k < n2;
                const u64 ow = __ballot(in && occupied<CH>(grid, row * n2 + k));
                u64 nb = 0;
                if (target == PB3D_EDT_TO_SURFACE)
                    nb = __ballot(in && i > 0 && i + 1 < n0 && j > 0 && j + 1 < n1 && occupied<CH>(grid, (row - n1) * n2 + k) &&
                                  occupied<CH>(grid, (row + n1) * n2 + k) && occupied<CH>(grid, (row - 1) * n2 + k) &&
                                  occupied<CH>(grid, (row + 1) * n2 + k));
                if (lane == 0) {
                    occ[wave][w] = ow;
                    tgt[wave][w] = nb;
                }
            }
        }
        __syncthreads();
        if (live) {
            for (int g = 0; g < kRowGroups; ++g) {
                const int w = g * 64 + lane;
                u64 T = 0;
                if (w < nw) {
                    const u64 O = occ[wave][w];
                    const u64 valid = (w == nw - 1 && (n2 & 63)) ? (1ull << (n2 & 63)) - 1 : ~0ull;
                    if (target == PB3D_EDT_TO_BACKGROUND) T = ~O & valid;
                    else if (target == PB3D_EDT_TO_OCCUPIED) T = O;
                    else {
                        // the occupancy of the voxel below and above along the row; outside the row: empty
                        const u64 lo = (O << 1) | (w > 0 ? occ[wave][w - 1] >> 63 : 0);
                        const u64 hi = (O >> 1) | (w + 1 < nw ? occ[wave][w + 1] << 63 : 0);
                        T = O & ~(tgt[wave][w] & lo & hi);
                    }
                    tgt[wave][w] = T;
                    ntargets += (u64)__popcll(T);
                }
                const u64 nz = __ballot(T != 0);
                if (lane == 0) nzs[wave][g] = nz;
            }
        }
        __syncthreads();
        if (live) {
            for (int w = 0; w < nw; ++w) {
                const int k = w * 64 + lane;
                if (k >= n2) continue;
                const u64 T = tgt[wave][w];
                int tl = -1, tr = -1;
                const u64 ml = T & (~0ull >> (63 - lane)), mr = T & (~0ull << lane);
                if (ml) tl = w * 64 + 63 - __clzll((long long)ml);
                else {
                    const int p = prev_word(nzs[wave], w);
                    if (p >= 0) tl = p * 64 + 63 - __clzll((long long)tgt[wave][p]);
                }
                if (mr) tr = w * 64 + __ffsll((unsigned long long)mr) - 1;
                else {
                    const int p = next_word(nzs[wave], w);
                    if (p >= 0) tr = p * 64 + __ffsll((unsigned long long)tgt[wave][p]) - 1;
                }
                // an equidistant pair goes to the left: the smaller t2
                const int t = (tl >= 0 && (tr < 0 || k - tl <= tr - k)) ? tl : tr;
                const i64 v = row * n2 + k;
                sq[v] = t < 0 ? kNone : (t - k) * (t - k);
                if (IDX) feat[v] = t;
            }
        }
        __syncthreads();
    }
    group_add(ntargets, &counts[0]);
}

struct Cols {
    const int* gin;     // the pass's input sq; never the same buffer as gout
    const int* fin;     // ... and partial index (IDX)
    int* gout;          // the output sq; until a column's backward scan passes them, its voxels hold the stack's (s, t)
    int* fout;
    int* stackg;        // g(s) of the stack levels, laid out like gout
    i64 ncols, inner;   // columns, and the distance in elements between two voxels of a column
    int m;              // voxels per column
    int border, n1, n2; // LAST: the border rule and the lattice (a column is (j, k) = (c / n2, c % n2), its voxel u is i)
    pb3d_magic n2m;
};

// LAST: counts[1] = max(counts[1], sq + 1) over the sq that are not PB3D_EDT_NONE
template <bool IDX, bool LAST>
__global__ __launch_bounds__(kColLanes) void k_edt_columns(Cols a, u64* __restrict__ counts) {
    u64 best = 0;
    const int m = a.m;
    const i64 inner = a.inner;
    for (i64 c = (i64)blockIdx.x * kColLanes + threadIdx.x; c < a.ncols; c += (i64)gridDim.x * kColLanes) {
        const i64 o = c / inner, base = o * m * inner + (c - o * inner);
        const int* gin = a.gin + base;
        int* gout = a.gout + base;
        int* sg = a.stackg + base;
        // forward: the lower envelope.  Level q is parabola s, lowest from x = t on; the top level is in (s, t, g)
        int q = -1, s = 0, t = 0, g = 0;
        // the column's g values arrive kAhead at a time, the next batch requested before this one is used: the envelope's own loads
        // (a popped level) depend on what was just read, these do not, and a lane has nothing else to hide their latency with
        int cur[kAhead], nxt[kAhead];
#pragma unroll
        for (int b = 0; b < kAhead; ++b) cur[b] = b < m ? gin[b * inner] : kNone;
        for (int u0 = 0; u0 < m; u0 += kAhead) {
#pragma unroll
            for (int b = 0; b < kAhead; ++b) nxt[b] = u0 + kAhead + b < m ? gin[(u0 + kAhead + b) * inner] : kNone;
#pragma unroll
            for (int b = 0; b < kAhead; ++b) {
                const int u = u0 + b, gu = cur[b];
                if (gu == kNone) continue;                        // no parabola (and the filler past the column's end)
                while (q >= 0) {
                    const int ds = t - s, du = t - u;
                    if (ds * ds + g <= du * du + gu) break;       // s is not above u at t: it keeps [t, Sep]; a tie stays with s < u
                    if (--q >= 0) {
                        const int e = gout[q * inner];
                        s = e & (PB3D_EDT_MAX_AXIS - 1);
                        t = e >> kAxisBits;
                        g = sg[q * inner];
                    }
                }
                int w = 0;
                if (q >= 0) w = 1 + (int)((u32)((u - s) * (u + s) + (gu - g)) / (u32)(2 * (u - s)));   // 1 + Sep(s, u), numerator >= 0
                if (w < m) {
                    ++q;
                    s = u; t = w; g = gu;
                    gout[q * inner] = s | (t << kAxisBits);
                    sg[q * inner] = g;
                }
            }
#pragma unroll
            for (int b = 0; b < kAhead; ++b) cur[b] = nxt[b];
        }
        // backward: read the envelope off
        int bj = 0;
        if (LAST && a.border) {
            const int j = (int)pb3d_div((u32)c, a.n2m), k = (int)c - j * a.n2;
            bj = min(min(j + 1, a.n1 - j), min(k + 1, a.n2 - k));
        }
        int fs = -1;
        if (IDX && q >= 0) fs = (int)(s * inner) + a.fin[base + s * inner];
        for (int u = m - 1; u >= 0; --u) {
            int val = kNone;
            if (q >= 0) val = (u - s) * (u - s) + g;
            if (LAST && a.border) {
                const int b = min(bj, min(u + 1, m - u));
                val = min(val, b * b);
            }
            gout[u * inner] = val;
            if (IDX) a.fout[base + u * inner] = fs;
            if (LAST && val != kNone) best = max(best, (u64)val + 1);
            if (q > 0 && u == t) {
                --q;
                const int e = gout[q * inner];
                s = e & (PB3D_EDT_MAX_AXIS - 1);
                t = e >> kAxisBits;
                g = sg[q * inner];
                if (IDX) fs = (int)(s * inner) + a.fin[base + s * inner];
            }
        }
    }
    if (LAST) {                                             // one wavefront per workgroup: its maximum is the workgroup's
        best = wave_max(best);
        if (threadIdx.x == 0 && best) atomicMax((unsigned long long*)&counts[1], (unsigned long long)best);
    }
}

template <bool F64>
__global__ __launch_bounds__(256) void k_edt_distances(const int* __restrict__ sq, i64 n, double voxel_size, void* __restrict__ out) {
    for (i64 v = (i64)blockIdx.x * 256 + threadIdx.x; v < n; v += (i64)gridDim.x * 256) {
        const int s = sq[v];
        const double d = s == kNone ? (double)INFINITY : __dsqrt_rn((double)s) * voxel_size;
        if (F64) ((double*)out)[v] = d;
        else ((float*)out)[v] = (float)d;
    }
}

template <int CH>
__global__ __launch_bounds__(256) void k_edt_apply(const u8* grid, i64 nvox, const int* __restrict__ sq, const int* __restrict__ index, int mode,
                                                   i64 r_sq, u8* out) {
    for (i64 v = (i64)blockIdx.x * 256 + threadIdx.x; v < nvox; v += (i64)gridDim.x * 256) {
        i64 src = -1;                                       // the voxel whose bytes v takes, -1: zero
        if (mode == PB3D_EDT_KEEP) {
            if ((i64)sq[v] > r_sq) src = v;
        } else if (occupied<CH>(grid, v)) {
            src = v;
        } else if ((i64)sq[v] <= r_sq) {
            const i64 t = index[v];
            if (t >= 0 && t < nvox) src = t;
        }
#pragma unroll
        for (int ch = 0; ch < CH; ++ch) {
            const u8 b = src < 0 ? (u8)0 : grid[src * CH + ch];
            out[v * CH + ch] = b;
        }
    }
}

struct Thresholds { i64 t[8]; int n; };

// counts: surface voxels, max(sq + 1), sum of sq, then the voxels with sq <= t[k]
template <int CH>
__global__ __launch_bounds__(256) void k_surface_stats(const u8* __restrict__ a, int n0, int n1, int n2, pb3d_magic n1m, pb3d_magic n2m,
                                                       const int* __restrict__ sq, Thresholds th, u64* __restrict__ counts) {
    u64 cnt = 0, best = 0, sum = 0, within[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const i64 nvox = (i64)n0 * n1 * n2, plane = (i64)n1 * n2;
    for (i64 v = (i64)blockIdx.x * 256 + threadIdx.x; v < nvox; v += (i64)gridDim.x * 256) {
        if (!occupied<CH>(a, v)) continue;
        const u32 r = pb3d_div((u32)v, n2m);
        const int k = (int)((u32)v - r * (u32)n2), i = (int)pb3d_div(r, n1m), j = (int)(r - (u32)i * (u32)n1);
        const bool inner = i > 0 && i + 1 < n0 && j > 0 && j + 1 < n1 && k > 0 && k + 1 < n2 && occupied<CH>(a, v - plane) &&
                           occupied<CH>(a, v + plane) && occupied<CH>(a, v - n2) && occupied<CH>(a, v + n2) && occupied<CH>(a, v - 1) &&
                           occupied<CH>(a, v + 1);
        if (inner) continue;
        const i64 s = sq[v];
        ++cnt;
        best = max(best, (u64)s + 1);
        sum += (u64)s;
#pragma unroll
        for (int t = 0; t < 8; ++t) within[t] += (t < th.n && s <= th.t[t]) ? 1 : 0;
    }
    group_add(cnt, &counts[0]);
    group_max(best, &counts[1]);
    group_add(sum, &counts[2]);
#pragma unroll
    for (int t = 0; t < 8; ++t)
        if (t < th.n) group_add(within[t], &counts[3 + t]);
}

bool grid_ok(i64 n0, i64 n1, i64 n2) {
    return n0 >= 1 && n1 >= 1 && n2 >= 1 && n0 <= PB3D_EDT_MAX_AXIS && n1 <= PB3D_EDT_MAX_AXIS && n2 <= PB3D_EDT_MAX_AXIS && n0 * n1 * n2 <= kMaxVoxels;
}

}  // namespace

extern "C" {

int pb3d_edt_resident(pb3d_ctx* ctx, const uint8_t* d_grid, int channels, int64_t n0, int64_t n1, int64_t n2, int target, int border_is_target,
                      int32_t* d_sq, int32_t* d_index, int64_t* stats) {
    PB3D_REQUIRE(grid_ok(n0, n1, n2), "pb3d_edt: every axis must be in [1, %d] and the grid at most 2^31 - 1 voxels (got %lld x %lld x %lld)",
                 PB3D_EDT_MAX_AXIS, (long long)n0, (long long)n1, (long long)n2);
    PB3D_REQUIRE(channels == 1 || channels == 3, "pb3d_edt: channels must be 1 or 3 (got %d)", channels);
    PB3D_REQUIRE(target >= PB3D_EDT_TO_BACKGROUND && target <= PB3D_EDT_TO_SURFACE, "pb3d_edt: target must be 0, 1 or 2 (got %d)", target);
    PB3D_REQUIRE(!(border_is_target && d_index), "pb3d_edt: no index with border_is_target: a border plane has no index");
    PB3D_REQUIRE(d_grid && d_sq, "pb3d_edt: null buffer");
    PB3D_REQUIRE((uintptr_t)d_sq % 4 == 0 && (uintptr_t)d_index % 4 == 0, "pb3d_edt: d_sq and d_index must be 4-byte aligned");
    PB3D_REQUIRE(ctx != nullptr, "pb3d_edt: null context");

    const i64 nvox = n0 * n1 * n2;
    void *cn, *st, *sqt, *ixt = nullptr;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_EDT_SQ_TMP, (size_t)nvox * sizeof(int), &sqt));
    if (d_index) PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_EDT_INDEX_TMP, (size_t)nvox * sizeof(int), &ixt));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_EDT_STACK, (size_t)nvox * sizeof(int), &st));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_EDT_COUNTS, 2 * sizeof(u64), &cn));
    u64* counts = (u64*)cn;
    PB3D_HIP(hipMemsetAsync(cn, 0, 2 * sizeof(u64), ctx->stream));

    const dim3 rows(pb3d_stream_blocks(ctx, n0 * n1, 4, 8));
    auto row_pass = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, rows, dim3(256), 0, ctx->stream, d_grid, (i64)n0, (i64)n1, (i64)n2, target, (int*)d_sq, (int*)d_index, counts);
    };
    if (channels == 1 && d_index) row_pass(k_edt_rows<1, true>);
    else if (channels == 1) row_pass(k_edt_rows<1, false>);
    else if (d_index) row_pass(k_edt_rows<3, true>);
    else row_pass(k_edt_rows<3, false>);
    PB3D_CHECK_LAUNCH();

    const Cols c1 = {(const int*)d_sq, (const int*)d_index, (int*)sqt, (int*)ixt, (int*)st, n0 * n2, n2, (int)n1, 0, (int)n1, (int)n2, pb3d_make_magic((u32)n2)};
    const Cols c0 = {(const int*)sqt, (const int*)ixt, (int*)d_sq, (int*)d_index, (int*)st, n1 * n2, n1 * n2, (int)n0, border_is_target != 0, (int)n1, (int)n2,
                     pb3d_make_magic((u32)n2)};
    const dim3 g1(pb3d_stream_blocks(ctx, c1.ncols, kColLanes, 32)), g0(pb3d_stream_blocks(ctx, c0.ncols, kColLanes, 32));
    if (d_index) {
        hipLaunchKernelGGL((k_edt_columns<true, false>), g1, dim3(kColLanes), 0, ctx->stream, c1, counts);
        hipLaunchKernelGGL((k_edt_columns<true, true>), g0, dim3(kColLanes), 0, ctx->stream, c0, counts);
    } else {
        hipLaunchKernelGGL((k_edt_columns<false, false>), g1, dim3(kColLanes), 0, ctx->stream, c1, counts);
        hipLaunchKernelGGL((k_edt_columns<false, true>), g0, dim3(kColLanes), 0, ctx->stream, c0, counts);
    }
    PB3D_CHECK_LAUNCH();
    if (stats) {
        PB3D_TRY(pb3d_read_back(ctx, stats, counts, 2 * sizeof(i64)));
        stats[1] -= 1;                                      // the device keeps max(sq + 1), 0 = no sq but PB3D_EDT_NONE
    }
    return PB3D_OK;
}

int pb3d_edt_distances_resident(pb3d_ctx* ctx, const int32_t* d_sq, int64_t n, double voxel_size, int out_f64, void* d_out) {
    PB3D_REQUIRE(n >= 0 && n <= kMaxVoxels, "pb3d_edt_distances: n must be in [0, 2^31 - 1] (got %lld)", (long long)n);
    PB3D_REQUIRE(std::isfinite(voxel_size) && voxel_size > 0.0, "pb3d_edt_distances: voxel_size must be finite and > 0 (got %g)", voxel_size);
    PB3D_REQUIRE(n == 0 || (d_sq && d_out), "pb3d_edt_distances: null buffer");
    PB3D_REQUIRE((uintptr_t)d_sq % 4 == 0 && (uintptr_t)d_out % (out_f64 ? 8 : 4) == 0, "pb3d_edt_distances: misaligned buffer");
    PB3D_REQUIRE(ctx != nullptr, "pb3d_edt_distances: null context");
    if (n == 0) return PB3D_OK;
    const dim3 grid(pb3d_stream_blocks(ctx, n, 256, 0));
    if (out_f64) hipLaunchKernelGGL(k_edt_distances<true>, grid, dim3(256), 0, ctx->stream, (const int*)d_sq, (i64)n, voxel_size, d_out);
    else hipLaunchKernelGGL(k_edt_distances<false>, grid, dim3(256), 0, ctx->stream, (const int*)d_sq, (i64)n, voxel_size, d_out);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

int pb3d_edt_apply_resident(pb3d_ctx* ctx, const uint8_t* d_grid, int channels, int64_t nvox, const int32_t* d_sq, const int32_t* d_index, int mode,
                            int64_t r_sq, uint8_t* d_out) {
    PB3D_REQUIRE(nvox >= 0 && nvox <= kMaxVoxels, "pb3d_edt_apply: nvox must be in [0, 2^31 - 1] (got %lld)", (long long)nvox);
    PB3D_REQUIRE(channels == 1 || channels == 3, "pb3d_edt_apply: channels must be 1 or 3 (got %d)", channels);
    PB3D_REQUIRE(mode == PB3D_EDT_FILL || mode == PB3D_EDT_KEEP, "pb3d_edt_apply: mode must be 0 (fill) or 1 (keep), got %d", mode);
    PB3D_REQUIRE(r_sq >= 0, "pb3d_edt_apply: r_sq must be >= 0 (got %lld)", (long long)r_sq);
    PB3D_REQUIRE(nvox == 0 || (d_grid && d_sq && d_out && (mode == PB3D_EDT_KEEP || d_index)), "pb3d_edt_apply: null buffer");
    PB3D_REQUIRE((uintptr_t)d_sq % 4 == 0 && (uintptr_t)d_index % 4 == 0, "pb3d_edt_apply: d_sq and d_index must be 4-byte aligned");
    PB3D_REQUIRE(ctx != nullptr, "pb3d_edt_apply: null context");
    if (nvox == 0) return PB3D_OK;
    const dim3 grid(pb3d_stream_blocks(ctx, nvox, 256, 0));
    if (channels == 1)
        hipLaunchKernelGGL(k_edt_apply<1>, grid, dim3(256), 0, ctx->stream, d_grid, (i64)nvox, (const int*)d_sq, (const int*)d_index, mode, (i64)r_sq, d_out);
    else
        hipLaunchKernelGGL(k_edt_apply<3>, grid, dim3(256), 0, ctx->stream, d_grid, (i64)nvox, (const int*)d_sq, (const int*)d_index, mode, (i64)r_sq, d_out);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

int pb3d_grid_surface_stats_resident(pb3d_ctx* ctx, const uint8_t* d_a, int channels_a, int64_t n0, int64_t n1, int64_t n2,
                                     const int32_t* d_sq_to_b_surface, const int64_t* thresholds_sq, int nthr, int64_t* out) {
    PB3D_REQUIRE(grid_ok(n0, n1, n2), "pb3d_grid_surface_stats: every axis must be in [1, %d] and the grid at most 2^31 - 1 voxels (got %lld x %lld x %lld)",
                 PB3D_EDT_MAX_AXIS, (long long)n0, (long long)n1, (long long)n2);
    PB3D_REQUIRE(channels_a == 1 || channels_a == 3, "pb3d_grid_surface_stats: channels must be 1 or 3 (got %d)", channels_a);
    PB3D_REQUIRE(nthr >= 0 && nthr <= 8, "pb3d_grid_surface_stats: nthr must be in [0, 8] (got %d)", nthr);
    PB3D_REQUIRE(out != nullptr && (nthr == 0 || thresholds_sq != nullptr), "pb3d_grid_surface_stats: null argument");
    PB3D_REQUIRE(d_a && d_sq_to_b_surface, "pb3d_grid_surface_stats: null buffer");
    PB3D_REQUIRE((uintptr_t)d_sq_to_b_surface % 4 == 0, "pb3d_grid_surface_stats: d_sq_to_b_surface must be 4-byte aligned");
    PB3D_REQUIRE(ctx != nullptr, "pb3d_grid_surface_stats: null context");
    Thresholds th = {{0, 0, 0, 0, 0, 0, 0, 0}, nthr};
    for (int t = 0; t < nthr; ++t) th.t[t] = thresholds_sq[t];
    void* cn;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_EDT_COUNTS, 11 * sizeof(u64), &cn));
    PB3D_HIP(hipMemsetAsync(cn, 0, 11 * sizeof(u64), ctx->stream));
    const dim3 grid(pb3d_stream_blocks(ctx, n0 * n1 * n2, 256, 8));
    const pb3d_magic n1m = pb3d_make_magic((u32)n1), n2m = pb3d_make_magic((u32)n2);
    if (channels_a == 1)
        hipLaunchKernelGGL(k_surface_stats<1>, grid, dim3(256), 0, ctx->stream, d_a, (int)n0, (int)n1, (int)n2, n1m, n2m, (const int*)d_sq_to_b_surface, th,
                           (u64*)cn);
    else
        hipLaunchKernelGGL(k_surface_stats<3>, grid, dim3(256), 0, ctx->stream, d_a, (int)n0, (int)n1, (int)n2, n1m, n2m, (const int*)d_sq_to_b_surface, th,
                           (u64*)cn);
    PB3D_CHECK_LAUNCH();
    i64 got[11];
    PB3D_TRY(pb3d_read_back(ctx, got, cn, 11 * sizeof(i64)));
    got[1] -= 1;
    for (int t = 0; t < 3 + nthr; ++t) out[t] = got[t];
    return PB3D_OK;
}

}  // extern "C"
