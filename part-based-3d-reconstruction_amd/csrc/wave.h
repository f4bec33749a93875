// Sums, minima, maxima and scans over a 64-lane wavefront and over a workgroup of whole wavefronts: the one copy of each (DESIGN.md,
// "Wave and workgroup primitives").  gfx950 only: a wavefront is 64 lanes, a workgroup is one-dimensional and a multiple of 64 threads,
// so lane = threadIdx.x & 63 and wave = threadIdx.x >> 6.  Every lane of the wavefront (every thread of the workgroup, for the
// group_* forms) makes the call: the shuffles read all 64 lanes and the group_* forms contain barriers.
//   wave_sum / wave_min / wave_max   all lanes end with the result
//   wave_incl_scan                   lane l ends with the sum over lanes 0 .. l
//   group_total<N>                   sum of the wave totals of an N-wave workgroup, through the caller's LDS, to thread 0
//   group_add / group_max            a 256-thread workgroup's sum / maximum into memory by ONE integer atomic
//   group_excl_scan<THREADS>         exclusive scan over the threads of a workgroup (256 or 1024), and its total
//   group_scan_array                 one 1024-thread workgroup scans an array of any length
// LDS stays with the kernel: a helper that needs it takes a pointer.  Only group_add and group_max own theirs, and therefore end with
// the barrier that lets them be called again.
#pragma once
#include "pb3d_internal.h"

template <typename T> __device__ __forceinline__ T wave_min2(T a, T b) {
    if constexpr (std::is_floating_point<T>::value) return fmin(a, b); else return a < b ? a : b;
}
template <typename T> __device__ __forceinline__ T wave_max2(T a, T b) {
    if constexpr (std::is_floating_point<T>::value) return fmax(a, b); else return a > b ? a : b;
}

// The xor butterfly, off = 32, 16, 8, 4, 2, 1.  For double this ORDER IS PUBLISHED (include/pb3d.h, "Summation order"; reduce_rows.h
// and the box reduction of nn.hip rest on it): lane l adds lane l ^ off at every step, so all lanes end with the same bits (IEEE
// addition commutes) and those bits are a function of the 64 inputs alone.  Changing the order changes results.
template <typename T> __device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
template <typename T> __device__ __forceinline__ T wave_min(T v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = wave_min2(v, (T)__shfl_xor(v, off));
    return v;
}
template <typename T> __device__ __forceinline__ T wave_max(T v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = wave_max2(v, (T)__shfl_xor(v, off));
    return v;
}

// inclusive scan of an integer over the lanes of the wavefront; lane 63 ends with the wave's total
template <typename T> __device__ __forceinline__ T wave_incl_scan(T v) {
    static_assert(std::is_integral<T>::value, "integer scans only: a float scan would need a stated order");
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const T t = __shfl_up(v, off); if (lane >= off) v += t; }
    return v;
}

// The sum of the N wave totals of an N-wave workgroup, handed to use(total) on thread 0 alone: one thread stores or sends a
// workgroup's count.  wave_total is the wave's own (uniform over its lanes), wsum is N elements of LDS.  Integers, added wave 0
// first.  There is no barrier after the read: a kernel that writes wsum again puts one in between.
template <int N, typename T, typename Use> __device__ __forceinline__ void group_total(T wave_total, T* wsum, Use use) {
    static_assert(std::is_integral<T>::value, "integer totals only: reduce_rows.h owns the ordered float64 form");
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = wave_total;
    __syncthreads();
    if (threadIdx.x == 0) {
        T t = wsum[0];
#pragma unroll
        for (int k = 1; k < N; ++k) t += wsum[k];
        use(t);
    }
}

// *dst += the sum (group_max: *dst = max(*dst, the maximum)) of c over a 256-thread workgroup, by one atomic; nothing is sent for 0.
// One per workgroup of a capped grid, not one per wavefront: tens of thousands of atomics on one address were what the passes waited for
__device__ __forceinline__ void group_add(u64 c, u64* dst) {
    __shared__ u64 part[4];
    group_total<4>(wave_sum(c), part, [&](u64 t) { if (t) atomicAdd((unsigned long long*)dst, (unsigned long long)t); });
    __syncthreads();
}
__device__ __forceinline__ void group_max(u64 c, u64* dst) {
    __shared__ u64 part[4];
    c = wave_max(c);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        const u64 t = wave_max2(wave_max2(part[0], part[1]), wave_max2(part[2], part[3]));
        if (t) atomicMax((unsigned long long*)dst, (unsigned long long)t);
    }
    __syncthreads();
}

// Exclusive scan of v over the THREADS threads of the workgroup, in thread order; *total (when asked for) = the workgroup's sum, on
// every thread.  wsum is THREADS / 64 elements of LDS, free again on return (the closing barrier), so calls may follow each other.
template <int THREADS, typename T> __device__ __forceinline__ T group_excl_scan(T v, T* wsum, T* total = nullptr) {
    static_assert(THREADS == 256 || THREADS == 1024, "a workgroup of 4 or 16 wavefronts");
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const T inc = wave_incl_scan(v);
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    T before = inc - v;
    for (int k = 0; k < wv; ++k) before += wsum[k];
    if (total) {
        T t = wsum[0];
#pragma unroll
        for (int k = 1; k < THREADS / 64; ++k) t += wsum[k];
        *total = t;
    }
    __syncthreads();
    return before;
}

// One 1024-thread workgroup: out[i] = in[0] + ... + in[i - 1] for i < n, accumulated as Acc, and *total (when asked for) = the sum of
// all n.  Thread t sums its run of ceil(n / 1024) consecutive elements, wavefront 0 scans the 1024 partial sums (16 per lane), and
// every thread rewrites its run.  part is 1024 Acc of LDS.  in and out may not overlap.
template <typename Acc, typename In, typename Out, typename Tot>
__device__ __forceinline__ void group_scan_array(const In* __restrict__ in, i64 n, Out* __restrict__ out, Tot* __restrict__ total, Acc* part) {
    const i64 per = (n + 1023) / 1024;
    const i64 b = (i64)threadIdx.x * per, e = b + per < n ? b + per : n;
    Acc s = 0;
    for (i64 i = b; i < e; ++i) s += (Acc)in[i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x < 64) {
        Acc loc[16], sum = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) { loc[k] = part[16 * threadIdx.x + k]; sum += loc[k]; }
        Acc run = wave_incl_scan(sum) - sum;
#pragma unroll
        for (int k = 0; k < 16; ++k) { part[16 * threadIdx.x + k] = run; run += loc[k]; }
        if (total && threadIdx.x == 63) *total = (Tot)run;
    }
    __syncthreads();
    Acc run = part[threadIdx.x];
    for (i64 i = b; i < e; ++i) { out[i] = (Out)run; run += (Acc)in[i]; }
}
