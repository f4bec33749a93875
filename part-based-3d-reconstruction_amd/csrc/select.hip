// Exact k-th smallest of a resident float64 list (include/pb3d.h has the contract): most-significant-digit radix selection over the
// totalOrder keys  key = bits ^ (bits >> 63 ? ~0 : 1 << 63),  eight passes of eight bits.  Pass p
//   k_select_hist   counts digit p (bits 63 - 8p .. 56 - 8p) of every element whose p higher digits equal the prefix found so far: a
//                   256-bin LDS histogram per workgroup, flushed with one integer global atomic per non-empty bin
//   k_select_scan   one 256-thread workgroup: scans the 256 bins, fixes digit p (the bin the remaining rank falls into) and takes the
//                   bins below it off the rank; after the last pass the prefix IS the key, and its value goes to d_out
// and the state (prefix, remaining rank) never leaves the device: nothing waits for the host.  Only integer atomics, so the counts are
// exact in any arrival order and two calls on the same input give the same bytes.  The state and the eight histograms live in
// PB3D_SLOT_SELECT and are cleared in-stream on every call.
//
// Squared distances of a roughly aligned cloud share sign and exponent: in the first passes a whole wave hits one counter.  The wave
// shortcut below turns that into one LDS add of a popcount; mixed waves fall back to per-lane LDS atomics.  Later passes read every
// element (16 bytes per lane where the base allows) but count only those under the prefix.
#include <cstddef>

#include "pb3d_internal.h"
#include "wave.h"

namespace {

constexpr int kPasses = 8, kBins = 256;

struct SelState {
    u64 prefix;               // the digits fixed so far, in place (lower bits 0)
    i64 rank;                 // the rank that remains among the elements under the prefix (valid after pass 0's scan)
    u32 hist[kPasses][kBins];
    i64 host_rank;            // where the exported entry places its rank (not cleared with the rest: it is written first)
};
constexpr size_t kClearBytes = offsetof(SelState, host_rank);

__device__ __forceinline__ u64 key_of(double v) {
    const u64 b = (u64)__double_as_longlong(v);
    return b ^ ((b >> 63) ? ~0ull : 1ull << 63);
}

// one element per lane into the workgroup's histogram; `valid` lanes carry `digit`
__device__ __forceinline__ void count_digit(u32* lds, bool valid, u32 digit) {
    const u64 act = __ballot(valid);
    if (act == 0) return;                                   // wave-uniform
    const int leader = __ffsll((unsigned long long)act) - 1;
    const u32 d0 = __shfl(digit, leader);
    const u64 same = __ballot(valid && digit == d0);
    if (same == act) {
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(&lds[d0], (u32)__popcll(act));
    } else if (valid) {
        atomicAdd(&lds[digit], 1u);
    }
}

__global__ __launch_bounds__(256) void k_select_hist(const double* __restrict__ vals, i64 n, SelState* __restrict__ st, int pass) {
    __shared__ u32 lds[kBins];
    lds[threadIdx.x] = 0;
    __syncthreads();
    const u64 prefix = pass ? st->prefix : 0;
    const int hi = 64 - 8 * pass, lo = 56 - 8 * pass;       // hi == 64 only in pass 0, where every element counts
    auto under = [&](u64 k) { return pass == 0 || ((k ^ prefix) >> hi) == 0; };
    // [0, head): up to the first 16-byte boundary; then npairs aligned pairs; then at most one element
    const i64 head = (((uintptr_t)vals & 8) && n > 0) ? 1 : 0;
    const i64 npairs = (n - head) / 2;
    const double2* pairs = (const double2*)(vals + head);
    for (i64 base = (i64)blockIdx.x * 256; base < npairs; base += (i64)gridDim.x * 256) {      // workgroup-uniform trip count
        const i64 i = base + threadIdx.x;
        const bool ok = i < npairs;
        double2 v = make_double2(0.0, 0.0);
        if (ok) v = pairs[i];
        const u64 k0 = key_of(v.x), k1 = key_of(v.y);
        count_digit(lds, ok && under(k0), (u32)(k0 >> lo) & 255u);
        count_digit(lds, ok && under(k1), (u32)(k1 >> lo) & 255u);
    }
    if (blockIdx.x == 0 && threadIdx.x < 2) {               // the two ends, at most one element each
        const i64 tail = head + 2 * npairs;
        const i64 i = threadIdx.x == 0 ? (head ? 0 : -1) : (tail < n ? tail : -1);
        if (i >= 0) {
            const u64 k = key_of(vals[i]);
            if (under(k)) atomicAdd(&lds[(u32)(k >> lo) & 255u], 1u);
        }
    }
    __syncthreads();
    const u32 c = lds[threadIdx.x];
    if (c) atomicAdd(&st->hist[pass][threadIdx.x], c);
}

__global__ __launch_bounds__(256) void k_select_scan(SelState* __restrict__ st, const i64* __restrict__ rank0, int pass, double* __restrict__ out) {
    __shared__ i64 wsum[4];
    const int t = threadIdx.x;
    const i64 c = st->hist[pass][t];
    const i64 rank = pass ? st->rank : *rank0;
    const u64 prefix = pass ? st->prefix : 0;
    const i64 excl = group_excl_scan<256>(c, wsum);         // (its barriers: every thread has read the state before the one below rewrites it)
    const i64 incl = excl + c;
    if (excl <= rank && rank < incl) {                      // exactly one bin: 0 <= rank < the total
        const u64 p = prefix | ((u64)t << (56 - 8 * pass));
        st->prefix = p;
        st->rank = rank - excl;
        if (pass == kPasses - 1) {
            const u64 bits = (p >> 63) ? p ^ (1ull << 63) : ~p;
            *(u64*)out = bits;
        }
    }
}

__global__ void k_select_put_rank(SelState* __restrict__ st, i64 rank) { st->host_rank = rank; }

}  // namespace

int pb3d_select_kth(pb3d_ctx* ctx, const double* d_vals, i64 n, const i64* d_rank, double* d_out) {
    void* buf;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_SELECT, sizeof(SelState), &buf));
    SelState* st = (SelState*)buf;
    PB3D_HIP(hipMemsetAsync(st, 0, kClearBytes, ctx->stream));
    if (!d_rank) d_rank = &st->host_rank;
    const dim3 grid(pb3d_stream_blocks(ctx, (n + 1) / 2, 256, 4));
    for (int pass = 0; pass < kPasses; ++pass) {
        hipLaunchKernelGGL(k_select_hist, grid, dim3(256), 0, ctx->stream, d_vals, n, st, pass);
        PB3D_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_select_scan, dim3(1), dim3(256), 0, ctx->stream, st, d_rank, pass, d_out);
        PB3D_CHECK_LAUNCH();
    }
    return PB3D_OK;
}

extern "C" int pb3d_kth_smallest_resident(pb3d_ctx* ctx, const double* d_vals, int64_t n, int64_t rank, double* d_out) {
    PB3D_REQUIRE(n >= 1 && n <= pb3d_max_points, "pb3d_kth_smallest: need 1 <= n <= 2^31 - 1 values (got %lld)", (long long)n);
    PB3D_REQUIRE(rank >= 0 && rank < n, "pb3d_kth_smallest: need 0 <= rank < n (got rank %lld of %lld)", (long long)rank, (long long)n);
    PB3D_REQUIRE(d_vals != nullptr && d_out != nullptr, "pb3d_kth_smallest: null buffer");
    PB3D_REQUIRE(ctx != nullptr, "pb3d_kth_smallest: null context");
    void* buf;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_SELECT, sizeof(SelState), &buf));
    hipLaunchKernelGGL(k_select_put_rank, dim3(1), dim3(1), 0, ctx->stream, (SelState*)buf, (i64)rank);
    PB3D_CHECK_LAUNCH();
    return pb3d_select_kth(ctx, d_vals, n, nullptr, d_out);
}
