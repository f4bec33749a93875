// The count reduction of csrc/voxelize.hip and csrc/render.hip: one integer atomic per 256-thread workgroup.
#pragma once
#include "pb3d_internal.h"

__device__ __forceinline__ u64 wave_sum(u64 c) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d);
    return c;
}

// *dst += the sum of c over a 256-thread workgroup, by one atomic (every thread of the workgroup calls it).  One per workgroup of a
// capped grid, not one per wavefront: tens of thousands of atomics on one address were what the passes waited for
__device__ __forceinline__ void group_add(u64 c, u64* dst) {
    __shared__ u64 part[4];
    c = wave_sum(c);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        const u64 t = (part[0] + part[1]) + (part[2] + part[3]);
        if (t) atomicAdd((unsigned long long*)dst, (unsigned long long)t);
    }
    __syncthreads();
}
