// The edge records of csrc/meshcomp.hip and csrc/orient.hip, and how their counting kernels keep integer atomics few: one copy.
#pragma once
#include "pb3d_internal.h"

struct Rec { u32 src, dst; };
// record r = 3j + a is the directed edge (corner a, corner a + 1 mod 3) of face j
__device__ __forceinline__ Rec load_rec(const u32* __restrict__ W, u32 r) {
    const u32 a = r % 3u;
    return Rec{W[r], a == 2u ? W[r - 2u] : W[r + 1u]};
}
__device__ __forceinline__ bool is_loop(const Rec& e) { return e.src == e.dst; }
__device__ __forceinline__ u32 lo_of(const Rec& e) { return e.src < e.dst ? e.src : e.dst; }
__device__ __forceinline__ u32 hi_of(const Rec& e) { return e.src < e.dst ? e.dst : e.src; }

// ---- counting by integer atomics, few of them ------------------------------------------------------------------------------------------
// The counting kernels walk their items in a grid-stride loop whose trip count is the same in every lane of a wavefront (wave_base),
// and keep what they count in wave-uniform registers: an atomic on one word costs about as much as a whole wavefront of plain work, and
// a mesh that is mostly one component would send every wavefront's count to the same word.
__device__ __forceinline__ i64 wave_base() { return (i64)blockIdx.x * 256 + (threadIdx.x & ~63u); }
__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63u); }

// a total: the lanes with `flag`, added up per wavefront and flushed once
struct WaveTotal {
    unsigned long long n = 0;
    __device__ __forceinline__ void add(bool flag) { n += (unsigned long long)__popcll(__ballot(flag)); }
    __device__ __forceinline__ void flush(unsigned long long* dst) const { if (n && lane_id() == 0) atomicAdd(dst, n); }
};
// a count per label, add_size of csrc/cluster.hip carried across the loop: the lanes that hold the first counting lane's label go to
// the run (flushed when that label changes, and at the end), every other counting lane adds on its own.  lab < 0 or !flag: no count
struct RunCount {
    int lab = -1;
    unsigned long long n = 0;
    __device__ __forceinline__ void flush(unsigned long long* sizes) {
        if (n && lane_id() == 0) atomicAdd(&sizes[lab], n);
        n = 0;
    }
    __device__ __forceinline__ void add(unsigned long long* sizes, int l, bool flag) {
        const bool counts = flag && l >= 0;
        const unsigned long long active = __ballot(counts);
        if (!active) return;
        const int first = __shfl(l, __ffsll(active) - 1);
        if (first != lab) { flush(sizes); lab = first; }
        n += (unsigned long long)__popcll(__ballot(counts && l == first));
        if (counts && l != first) atomicAdd(&sizes[l], 1ull);
    }
};
