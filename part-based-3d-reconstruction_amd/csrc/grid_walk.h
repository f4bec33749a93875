// Shared by visibility.hip, overlay.hip, pcarve.hip and ppaint.hip: the walk of a resident (A0, A1, A2, C) uint8 grid, C = 1 (labels)
// or 3 (RGB), the colour table that turns a voxel into bits, the shell of the kernels that rewrite the grid view by view
// (rewrite_walk) and the launch of a walking kernel (launch_walk).
//
// A lane owns four consecutive a2 columns of one a1 row (walk_item) and walks them along a0 for up to kChunk steps, loading the four
// voxels with dword loads where the rows allow it (lanes of a wave take consecutive a2).  Voxel (a0, a1, a2) is the point (x = a2, y = a1, z = a0).
#pragma once
#include "pb3d_internal.h"
#include "wave.h"
#include "project_point.h"

namespace pb3d_walk {

constexpr int kMaxColours = 31;           // bits 0..30: colours / labels / lists; bit 31: any occupied voxel
constexpr u32 kAnyBit = 0x80000000u;
constexpr int kChunk = 64;                // a0 steps per lane
constexpr i64 kMaxAxis = (i64)1 << 24;    // entries that project voxel coordinates as float32 points: exact below 2^24

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

// item t of the walk: columns a2 .. a2 + 3 of row a1, steps a0s .. a0e - 1; false past the last item
__device__ __forceinline__ bool walk_item(const Walk& w, i64 t, i64* a2, i64* a1, i64* a0s, i64* a0e) {
    if (t >= w.nitems) return false;
    const i64 r = t / w.ngx;
    *a2 = (t % w.ngx) * 4; *a1 = r % w.A1; *a0s = (r / w.A1) * kChunk;
    *a0e = *a0s + kChunk < w.A0 ? *a0s + kChunk : w.A0;
    return true;
}

// the four voxels at p, voxels i .. i + 3 of a row of n, as keys: whole aligned dwords where vec, else bytes; voxels past n read as
// 0 (empty)
template <int C>
__device__ __forceinline__ void load4(const u8* p, int vec, i64 i, i64 n, u32 v[4]) {
    if (vec) {
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
            if (i + k < n) v[k] = C == 1 ? (u32)p[k] : (u32)p[3 * k] | ((u32)p[3 * k + 1] << 8) | ((u32)p[3 * k + 2] << 16);
        }
    }
}

// the four voxels (a0, a1, a2 .. a2 + 3); columns past A2 read as 0
template <int C>
__device__ __forceinline__ void load4(const Walk& w, i64 a0, i64 a1, i64 a2, u32 v[4]) {
    load4<C>(w.grid + ((a0 * w.A1 + a1) * w.A2 + a2) * C, w.vec, a2, w.A2, v);
}

// load4's inverse into `out`, a grid of w's shape: the voxels of write_mask (bit k: column a2 + k) that lie inside A2; where w.vec,
// whole dwords, and then every voxel of the four is written
template <int C>
__device__ __forceinline__ void store4(const Walk& w, u8* out, i64 a0, i64 a1, i64 a2, const u32 v[4], u32 write_mask) {
    u8* o = out + ((a0 * w.A1 + a1) * w.A2 + a2) * C;
    if (w.vec) {
        if (C == 1) {
            *(u32*)o = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
        } else {
            ((u32*)o)[0] = v[0] | (v[1] << 24);
            ((u32*)o)[1] = (v[1] >> 8) | (v[2] << 16);
            ((u32*)o)[2] = (v[2] >> 16) | (v[3] << 8);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (a2 + k >= w.A2 || !((write_mask >> k) & 1u)) continue;
            if (C == 1) {
                o[k] = (u8)v[k];
            } else {
                o[3 * k] = (u8)v[k]; o[3 * k + 1] = (u8)(v[k] >> 8); o[3 * k + 2] = (u8)(v[k] >> 16);
            }
        }
    }
}

__device__ __forceinline__ void flush_or(u32* __restrict__ bits, i64 px, u32 b) {
    if (b && (b & ~__hip_atomic_load(&bits[px], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) atomicOr(&bits[px], b);
}

// ---- the run shell (k_grid_depth, k_grid_visible_bits, k_grid_hit_bits) ---------------------------------------------------------
// The body of a kernel that folds the voxels landing on a pixel into that pixel.  Under a front camera a column along a0 lands on a
// handful of pixels, so each column keeps a run while its pixel stays the same and flushes it with one atomic when the pixel
// changes or the walk ends.  Run has: MODE (the rule of project_xyz), State, take(voxel, &b) (is the voxel projected at all, and what
// add gets of it), open(pixel, &state), add(&state, b, z) and flush(pixel, state) for pixel >= 0.  The folds are order-free.
template <int C, class Run>
__device__ __forceinline__ void run_walk(const Walk& w, const pb3d_proj::ProjParams& P, const Run& run) {
    i64 a2, a1, a0s, a0e;
    if (!walk_item(w, (i64)blockIdx.x * blockDim.x + threadIdx.x, &a2, &a1, &a0s, &a0e)) return;
    i64 px[4] = {-1, -1, -1, -1};
    typename Run::State st[4] = {};
    for (i64 a0 = a0s; a0 < a0e; ++a0) {
        u32 v[4];
        load4<C>(w, a0, a1, a2, v);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            u32 b;
            if (!run.take(v[k], &b)) continue;
            const double p[3] = {(double)(a2 + k), (double)a1, (double)a0};      // exact in float32 where the entry bounds the axes by 2^24
            int ui, vi;
            double z = 0.0;
            if (!pb3d_proj::project_xyz<Run::MODE>(P, p, &ui, &vi, &z)) continue;
            const i64 q = (i64)vi * P.Wimg + ui;
            if (q != px[k]) {
                if (px[k] >= 0) run.flush(px[k], st[k]);
                px[k] = q;
                run.open(q, &st[k]);
            }
            run.add(&st[k], b, z);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (px[k] >= 0) run.flush(px[k], st[k]);
}

// ---- the decide-and-rewrite shell (k_pcarve, k_ppaint) -------------------------------------------------------------------------
// The body of a kernel that rewrites the subject voxels of a grid view by view.  An empty voxel or one outside the colour set costs
// nothing.  A subject voxel, as the float32 point p, runs through views 0 .. nviews - 1 (at most 8) in order and stops at the first
// for which decide(j, p, &key) is true; it then becomes `key`.  INPLACE: out is the walked grid and only decided voxels are written;
// else every voxel of the lane is.  Counts: a lane tallies its decisions per view in 16-bit fields (at most 4 * kChunk = 256 each),
// the wave adds them up with shuffles and issues one 64-bit atomic per view that decided anything.
template <int C, bool INPLACE, class Decide>
__device__ __forceinline__ void rewrite_walk(const Walk& w, const Colours& cols, int nviews, const Decide& decide, u8* out,
                                             unsigned long long* __restrict__ counts) {
    u64 tally[2] = {0, 0};                // view j: bits 16 * (j & 3) .. + 15 of tally[j >> 2] (in registers: no scratch)
    i64 a2, a1, a0s, a0e;
    if (walk_item(w, (i64)blockIdx.x * blockDim.x + threadIdx.x, &a2, &a1, &a0s, &a0e)) {
        for (i64 a0 = a0s; a0 < a0e; ++a0) {
            u32 v[4];
            load4<C>(w, a0, a1, a2, v);
            u32 decided = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!v[k] || (cols.n && !colour_bits(cols, v[k]))) continue;
                const double p[3] = {(double)(a2 + k), (double)a1, (double)a0};      // exact in float32: the entry bounds the axes by 2^24
                for (int j = 0; j < nviews; ++j) {
                    u32 key;
                    if (!decide(j, p, &key)) continue;
                    tally[j >> 2] += (u64)1 << (16 * (j & 3));
                    decided |= 1u << k;
                    v[k] = key;
                    break;
                }
            }
            if (INPLACE && !decided) continue;
            store4<C>(w, out, a0, a1, a2, v, INPLACE ? decided : 0xfu);
        }
    }
    if (!counts) return;                  // wave-uniform; below, every lane of the wave takes part in the shuffles
    for (int j = 0; j < nviews; ++j) {
        const int c = wave_sum((int)((tally[j >> 2] >> (16 * (j & 3))) & 0xffffu));
        if (__lane_id() == 0 && c) atomicAdd(&counts[j], (unsigned long long)c);
    }
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

// one thread per item
inline int walk_fits(const char* fn, const Walk& w) {
    PB3D_REQUIRE((w.nitems + 255) / 256 <= 0x7fffffff, "%s: grid too large for one launch", fn);
    return PB3D_OK;
}

// k1 (C = 1) or k3 (C = 3) over the items of w, with (w, args...) as arguments
template <class K, class... A>
int launch_walk(const char* fn, pb3d_ctx* ctx, const Walk& w, int C, K k1, K k3, A... args) {
    PB3D_TRY(walk_fits(fn, w));
    hipLaunchKernelGGL(C == 1 ? k1 : k3, dim3((unsigned)((w.nitems + 255) / 256)), dim3(256), 0, ctx->stream, w, args...);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

// a view of the carve or the paint: its size and its `what` ("mask", "image")
inline int view_args(const char* fn, int k, int Himg, int Wimg, const char* what, const void* d_data) {
    PB3D_REQUIRE(Himg > 0 && Wimg > 0, "%s: view %d has a %d x %d %s", fn, k, Himg, Wimg, what);
    PB3D_REQUIRE(d_data, "%s: view %d has a null %s", fn, k, what);
    return PB3D_OK;
}

}  // namespace pb3d_walk
