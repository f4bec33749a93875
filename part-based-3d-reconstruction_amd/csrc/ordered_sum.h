// The ordered wavefront sum of voxel centroids (csrc/downsample.hip) and hub vertices (csrc/smooth.hip).
//
// The contract: sum[a] starts at 0.0 and takes rows s, s + 1, ..., e - 1 by one rounded addition each, in that order, in every lane --
// exactly what a single lane looping over the rows computes (-ffp-contract=off, Makefile).  So whether a list is summed by one lane or
// by a wavefront changes the time and never the bits, however long the list is.  Any change to the order or the grouping of the
// additions here changes the results of both callers.
#pragma once
#include "pb3d_internal.h"

__device__ __forceinline__ double from_lane(double x, int j) {      // lane j's x in every lane (j is the same in all of them)
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), j), hi = __builtin_amdgcn_readlane(__double2hiint(x), j);
    return __hiloint2double(hi, lo);
}

// For a whole wavefront (every lane calls it with the same s and e): load(p, v) fetches row p into v[3].  64 rows a time are loaded,
// one per lane, and the next 64 are in flight while every lane adds the current 64 in ascending order by readlane.  Rows at or beyond
// e are never loaded and never added
template <class Load>
__device__ __forceinline__ void ordered_sum(i64 s, i64 e, Load load, double sum[3]) {
    const int lane = threadIdx.x & 63;
    // acc, not sum: adding into the caller's array kept a second copy of the sums around the inner loop (6 more VGPRs in both kernels)
    double acc[3] = {0.0, 0.0, 0.0}, cur[3] = {0.0, 0.0, 0.0}, nxt[3];
    if (s + lane < e) load(s + lane, cur);
    for (i64 p = s; p < e; p += 64) {
        nxt[0] = nxt[1] = nxt[2] = 0.0;
        if (p + 64 + lane < e) load(p + 64 + lane, nxt);
        const int c = (int)(e - p < 64 ? e - p : 64);
        for (int j = 0; j < c; ++j) {
            acc[0] = acc[0] + from_lane(cur[0], j);
            acc[1] = acc[1] + from_lane(cur[1], j);
            acc[2] = acc[2] + from_lane(cur[2], j);
        }
        for (int a = 0; a < 3; ++a) cur[a] = nxt[a];
    }
    for (int a = 0; a < 3; ++a) sum[a] = acc[a];
}
