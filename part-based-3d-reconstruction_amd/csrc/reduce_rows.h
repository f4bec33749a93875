// The fixed-order reduction of (int64 count, W float64 sums) rows that csrc/icp.hip and csrc/plane.hip share (include/pb3d.h states the
// order: "Summation order" of pb3d_icp_step_resident).  A row is W + 1 8-byte values: the count, then the sums.
//   pb3d_reduce_row<W>     the 256 (count, W values) of a workgroup -> one row
//   pb3d_k_rows_final<W>   one 256-thread workgroup: thread t adds partial rows t, t + 256, ... in ascending order, then the same reduction
// No floating-point atomics; the Makefile's -ffp-contract=off keeps every addition one rounded operation.
#pragma once
#include "pb3d_internal.h"
#include "wave.h"

// The workgroup's 256 (count, W values) -> row[0] = count, row[1 + c] = sum c: per wave the butterfly v += shfl_xor(v, off) for
// off = 32 ... 1 (wave.h's wave_sum; every lane ends with the same bits: IEEE addition commutes), then the four wave sums added left to right.
template <int W>
__device__ __forceinline__ void pb3d_reduce_row(double v[W], i64 cnt, double* __restrict__ row) {
    __shared__ double red[4][W];
    __shared__ i64 redc[4];
    cnt = wave_sum(cnt);
#pragma unroll
    for (int c = 0; c < W; ++c) v[c] = wave_sum(v[c]);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < W; ++c) red[w][c] = v[c];
        redc[w] = cnt;
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < W) row[1 + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
    if (t == W) ((i64*)row)[0] = redc[0] + redc[1] + redc[2] + redc[3];
}

template <int W>
__global__ __launch_bounds__(256) void pb3d_k_rows_final(const double* __restrict__ part, i64 nrows, double* __restrict__ out) {
    double v[W];
#pragma unroll
    for (int c = 0; c < W; ++c) v[c] = 0.0;
    i64 cnt = 0;
    for (i64 r = threadIdx.x; r < nrows; r += 256) {
        const double* row = part + r * (W + 1);
        cnt += ((const i64*)row)[0];
#pragma unroll
        for (int c = 0; c < W; ++c) v[c] += row[1 + c];
    }
    pb3d_reduce_row<W>(v, cnt, out);
}
