// Shared by visibility.hip and overlay.hip: the walk of a resident (A0, A1, A2, C) uint8 grid, C = 1 (labels) or 3 (RGB), and the
// colour table that turns a voxel into bits.
//
// A lane owns four consecutive a2 columns of one a1 row and walks them along a0 for up to kChunk steps, loading the four voxels with
// dword loads where the rows allow it (lanes of a wave take consecutive a2).  Voxel (a0, a1, a2) is the point (x = a2, y = a1, z = a0).
#pragma once
#include "pb3d_internal.h"

namespace pb3d_walk {

constexpr int kMaxColours = 31;           // bits 0..30: colours / labels / lists; bit 31: any occupied voxel
constexpr u32 kAnyBit = 0x80000000u;
constexpr int kChunk = 64;                // a0 steps per lane

struct Walk {
    const u8* grid;
    i64 A0, A1, A2, ngx, nitems;
    int vec;                              // rows of whole dwords: 4 voxels of a lane = 1 (C = 1) or 3 (C = 3) aligned dword loads
};

struct Colours {
    u32 key[kMaxColours];                 // r | g << 8 | b << 16 (C = 3) or the label (C = 1); never 0
    int n;
};

__device__ __forceinline__ u32 colour_bits(const Colours& c, u32 key) {
    u32 b = 0;
    for (int k = 0; k < c.n; ++k) b |= (u32)(c.key[k] == key) << k;
    return b;
}

// the four voxels (a0, a1, a2 .. a2 + 3) as keys; columns past A2 read as 0 (empty)
template <int C>
__device__ __forceinline__ void load4(const Walk& w, i64 a0, i64 a1, i64 a2, u32 v[4]) {
    const u8* p = w.grid + ((a0 * w.A1 + a1) * w.A2 + a2) * C;
    if (w.vec) {
        if (C == 1) {
            const u32 x = *(const u32*)p;
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = (x >> (8 * k)) & 0xffu;
        } else {
            const u32 x0 = ((const u32*)p)[0], x1 = ((const u32*)p)[1], x2 = ((const u32*)p)[2];
            v[0] = x0 & 0xffffffu;
            v[1] = (x0 >> 24) | ((x1 & 0xffffu) << 8);
            v[2] = (x1 >> 16) | ((x2 & 0xffu) << 16);
            v[3] = x2 >> 8;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k] = 0;
            if (a2 + k < w.A2) v[k] = C == 1 ? (u32)p[k] : (u32)p[3 * k] | ((u32)p[3 * k + 1] << 8) | ((u32)p[3 * k + 2] << 16);
        }
    }
}

__device__ __forceinline__ void flush_or(u32* __restrict__ bits, i64 px, u32 b) {
    if (px >= 0 && b && (b & ~__hip_atomic_load(&bits[px], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) atomicOr(&bits[px], b);
}

// ---- host helpers -------------------------------------------------------------------------------
inline int grid_args(const char* fn, const uint8_t* d_grid, i64 A0, i64 A1, i64 A2, int C) {
    PB3D_REQUIRE(C == 1 || C == 3, "%s: C must be 1 (labels) or 3 (RGB), got %d", fn, C);
    PB3D_REQUIRE(A0 >= 0 && A1 >= 0 && A2 >= 0, "%s: bad grid shape", fn);
    PB3D_REQUIRE(A0 * A1 * A2 == 0 || d_grid, "%s: null grid", fn);
    return PB3D_OK;
}

inline int colour_args(const char* fn, const uint8_t* colors, int ncolors, int C, Colours* out) {
    PB3D_REQUIRE(ncolors >= 0 && ncolors <= kMaxColours, "%s: at most %d colours (bit 31 is 'any'), got %d", fn, kMaxColours, ncolors);
    PB3D_REQUIRE(ncolors == 0 || colors, "%s: null colour table", fn);
    memset(out, 0, sizeof(*out));
    out->n = ncolors;
    for (int k = 0; k < ncolors; ++k) {
        const uint8_t* c = colors + (i64)k * C;
        out->key[k] = C == 1 ? c[0] : (u32)c[0] | ((u32)c[1] << 8) | ((u32)c[2] << 16);
        PB3D_REQUIRE(out->key[k] != 0, "%s: colour %d is black / label 0 (the empty voxel)", fn, k);
    }
    return PB3D_OK;
}

inline Walk make_walk(const uint8_t* d_grid, i64 A0, i64 A1, i64 A2, int C) {
    Walk w;
    w.grid = d_grid; w.A0 = A0; w.A1 = A1; w.A2 = A2;
    w.ngx = (A2 + 3) / 4;
    w.nitems = w.ngx * A1 * ((A0 + kChunk - 1) / kChunk);
    w.vec = (A2 % 4 == 0) && ((((uintptr_t)d_grid) & 3u) == 0);
    (void)C;
    return w;
}

}  // namespace pb3d_walk
