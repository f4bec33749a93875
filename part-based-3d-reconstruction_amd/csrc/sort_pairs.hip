// pb3d_sort_pairs: the stable LSD radix sort of (key, value) pairs of u32 that voxel_downsample (csrc/downsample.hip) orders its
// (voxel, position) pairs with and mesh smoothing (csrc/smooth.hip) its directed edges.  8-bit digits over the bits m - 1 needs: one
// pass for up to 256 keys, four at most.  No per-key state: a key that holds every pair is sorted like any other.
//   k_sort_hist       per tile of 2048 pairs, the digit histogram (LDS integer atomics) -> hist[digit][tile]
//   pb3d_scan_counts  that table in digit-major order = where each (digit, tile) run starts
//   k_sort_scatter    the tile again, 256 pairs a round in input order: a pair's place is its run's start + same-digit pairs of earlier
//                     rounds + of earlier waves + of lower lanes (ballot matching), which is what makes the pass stable
#include "pb3d_internal.h"

namespace {

constexpr int kTile = pb3d_sort_tile, kRounds = kTile / 256;  // pairs per workgroup of a sort pass

// ---- the stable radix pass --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sort_hist(const u32* __restrict__ key, i64 n, int shift, i64 ntiles, u32* __restrict__ hist) {
    __shared__ u32 h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const i64 base = (i64)blockIdx.x * kTile;
    for (int r = 0; r < kRounds; ++r) {
        const i64 i = base + r * 256 + threadIdx.x;
        if (i < n) atomicAdd(&h[(key[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(i64)threadIdx.x * ntiles + blockIdx.x] = h[threadIdx.x];
}

__global__ __launch_bounds__(256) void k_sort_scatter(const u32* __restrict__ key, const u32* __restrict__ val, i64 n, int shift, i64 ntiles,
                                                      const i64* __restrict__ start, u32* __restrict__ key_out, u32* __restrict__ val_out) {
    __shared__ u32 before[256];        // pairs of each digit in the tile's earlier rounds
    __shared__ u32 wave[4][256];       // ... in each wavefront of this round
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    before[t] = 0;
    for (int k = 0; k < 4; ++k) wave[k][t] = 0;
    __syncthreads();
    const i64 base = (i64)blockIdx.x * kTile;
    for (int r = 0; r < kRounds; ++r) {
        const i64 i = base + r * 256 + t;
        const bool valid = i < n;
        const u32 k = valid ? key[i] : 0u;
        const u32 d = (k >> shift) & 255u;
        unsigned long long match = __ballot(valid);     // the lanes of this wavefront that hold digit d
        for (int b = 0; b < 8; ++b) {
            const unsigned long long bal = __ballot((d >> b) & 1u);
            match &= ((d >> b) & 1u) ? bal : ~bal;
        }
        const u32 below = (u32)__popcll(match & ((1ull << lane) - 1ull));
        if (valid && below == 0) wave[w][d] = (u32)__popcll(match);
        __syncthreads();
        if (valid) {
            u32 ahead = before[d] + below;
            for (int k2 = 0; k2 < w; ++k2) ahead += wave[k2][d];
            const i64 dst = start[(i64)d * ntiles + blockIdx.x] + ahead;
            key_out[dst] = k;
            val_out[dst] = val[i];
        }
        __syncthreads();
        for (int k2 = 0; k2 < 4; ++k2) { before[t] += wave[k2][t]; wave[k2][t] = 0; }
        __syncthreads();
    }
}

}  // namespace

int pb3d_sort_pairs(pb3d_ctx* ctx, u32* key, u32* val, u32* key2, u32* val2, i64 n, i64 m, pb3d_slot hist_slot, pb3d_slot scan_local_slot,
                    pb3d_slot scan_segs_slot, const u32** key_sorted, const u32** val_sorted) {
    const i64 ntiles = (n + kTile - 1) / kTile, nruns = pb3d_sort_scan_items(n);
    int bits = 1;
    while (bits < 32 && ((u64)(m - 1) >> bits) != 0) ++bits;
    void* hist;
    PB3D_TRY(pb3d_scratch(ctx, hist_slot, (size_t)(nruns + 1) * sizeof(i64) + (size_t)nruns * sizeof(u32), &hist));
    i64* starts = (i64*)hist;
    u32* counts = (u32*)(starts + nruns + 1);
    for (int shift = 0; shift < bits; shift += 8) {
        hipLaunchKernelGGL(k_sort_hist, dim3((unsigned)ntiles), dim3(256), 0, ctx->stream, (const u32*)key, n, shift, ntiles, counts);
        PB3D_CHECK_LAUNCH();
        PB3D_TRY(pb3d_scan_counts(ctx, counts, nruns, starts, scan_local_slot, scan_segs_slot));
        hipLaunchKernelGGL(k_sort_scatter, dim3((unsigned)ntiles), dim3(256), 0, ctx->stream, (const u32*)key, (const u32*)val, n, shift, ntiles,
                           (const i64*)starts, key2, val2);
        PB3D_CHECK_LAUNCH();
        u32* t = key; key = key2; key2 = t;
        t = val; val = val2; val2 = t;
    }
    if (key_sorted) *key_sorted = key;
    *val_sorted = val;
    return PB3D_OK;
}
