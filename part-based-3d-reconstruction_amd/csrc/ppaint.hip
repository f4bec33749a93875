// Painting of a resident grid by pinhole views: a subject voxel takes the colour of the pixel the first view sees it at.
//
// The perspective counterpart of apply_colored_mask_to_voxel_grid.  Nothing here is new arithmetic: voxel (a0, a1, a2) is the
// float32 point (x = a2, y = a1, z = a0), its pixel and depth are project_xyz<1>'s (the z-buffer functions of the reference,
// utils/eval_helpers_intra.py:134-190: Z <= 1e-6 dropped, rint, bounds test), and a view sees it when |Z - zbuf[v, u]| < eps in the
// widths of visibility.hip's visible().  The z-buffers are the caller's (pb3d_grid_depth_buffer_dev of the grid before painting).
//
// Grid walk (grid_walk.h): a lane owns four consecutive a2 columns of one a1 row and walks them along a0 for up to kChunk steps.
// An empty voxel or one outside the colour set costs no projection.  A subject voxel runs through the views in order and stops at
// the first that paints it.  The image and the z-buffer of a view are read only behind a true project_xyz<1>: that test is the
// bounds check of both reads.  Images are read byte by byte at (v * W + u) * C, so any base address will do.
// Counts: a lane tallies its decisions per view in 16-bit fields (at most 4 * kChunk = 256 each), the wave adds them up with
// shuffles and issues one 64-bit atomic per view that decided anything.
#include "pb3d_internal.h"
#include "grid_walk.h"
#include "project_point.h"

namespace {

using namespace pb3d_proj;
using namespace pb3d_walk;

constexpr int kMaxViews = 8;              // views of a call (kernel arguments)
constexpr int kMaxSkip = 8;               // image colours / labels that never paint
constexpr i64 kMaxAxis = (i64)1 << 24;    // voxel coordinates are float32 points: exact below 2^24

struct View {
    ProjParams P;
    const u8* image;                      // P.Himg x P.Wimg x C bytes
    const float* zbuf;                    // P.Himg x P.Wimg
};

struct Views {
    View v[kMaxViews];
    int n;
};

struct Skip {
    u32 key[kMaxSkip];                    // r | g << 8 | b << 16 (C = 3) or the label (C = 1)
    int n;
};

// visibility.hip's visible(), word for word: float64 for a float64 camera, else a float32 difference compared in float32 when eps
// is a weak Python float
__device__ __forceinline__ bool visible(double z, float zb, int t0, double eps, int eps_f32) {
    if (t0) return fabs(__dsub_rn(z, (double)zb)) < eps;
    const float dz = fabsf(__fsub_rn((float)z, zb));
    return eps_f32 ? dz < (float)eps : (double)dz < eps;
}

__device__ __forceinline__ bool skipped(const Skip& s, u32 key) {
    bool b = false;
    for (int k = 0; k < s.n; ++k) b |= s.key[k] == key;
    return b;
}

template <int C>
__device__ __forceinline__ void store4_vec(u8* p, const u32 v[4]) {
    if (C == 1) {
        *(u32*)p = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
    } else {
        ((u32*)p)[0] = v[0] | (v[1] << 24);
        ((u32*)p)[1] = (v[1] >> 8) | (v[2] << 16);
        ((u32*)p)[2] = (v[2] >> 16) | (v[3] << 8);
    }
}

// INPLACE: out is the walked grid and only decided voxels are written; else every voxel of the lane is
template <int C, bool INPLACE>
__global__ __launch_bounds__(256) void k_ppaint(Walk w, Colours cols, Views V, Skip skip, double eps, int eps_f32, u8* out,
                                                unsigned long long* __restrict__ painted) {
    const i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    u64 tally[2] = {0, 0};                // view j: bits 16 * (j & 3) .. + 15 of tally[j >> 2]
    if (t < w.nitems) {
        const i64 a2 = (t % w.ngx) * 4, r = t / w.ngx, a1 = r % w.A1, a0s = (r / w.A1) * kChunk;
        const i64 a0e = a0s + kChunk < w.A0 ? a0s + kChunk : w.A0;
        for (i64 a0 = a0s; a0 < a0e; ++a0) {
            u32 v[4];
            load4<C>(w, a0, a1, a2, v);
            u32 decided = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!v[k] || (cols.n && !colour_bits(cols, v[k]))) continue;
                const double p[3] = {(double)(a2 + k), (double)a1, (double)a0};      // exact in float32: the entry bounds the axes by 2^24
                for (int j = 0; j < V.n; ++j) {
                    const View& vw = V.v[j];
                    int ui, vi;
                    double z;
                    if (!project_xyz<1>(vw.P, p, &ui, &vi, &z)) continue;            // below: 0 <= ui < Wimg, 0 <= vi < Himg
                    const i64 q = (i64)vi * vw.P.Wimg + ui;
                    if (!visible(z, vw.zbuf[q], vw.P.t0, eps, eps_f32)) continue;
                    const u8* px = vw.image + q * C;
                    const u32 key = C == 1 ? (u32)px[0] : (u32)px[0] | ((u32)px[1] << 8) | ((u32)px[2] << 16);
                    if (!key || skipped(skip, key)) continue;
                    const u64 one = (u64)1 << (16 * (j & 3));
                    tally[0] += (j >> 2) ? 0 : one;
                    tally[1] += (j >> 2) ? one : 0;
                    decided |= 1u << k;
                    v[k] = key;
                    break;
                }
            }
            if (INPLACE && !decided) continue;
            u8* o = out + ((a0 * w.A1 + a1) * w.A2 + a2) * C;
            if (w.vec) {
                store4_vec<C>(o, v);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (a2 + k >= w.A2 || (INPLACE && !((decided >> k) & 1u))) continue;
                    if (C == 1) {
                        o[k] = (u8)v[k];
                    } else {
                        o[3 * k] = (u8)v[k]; o[3 * k + 1] = (u8)(v[k] >> 8); o[3 * k + 2] = (u8)(v[k] >> 16);
                    }
                }
            }
        }
    }
    if (!painted) return;                 // wave-uniform; below, every lane of the wave takes part in the shuffles
    for (int j = 0; j < V.n; ++j) {
        int c = (int)(((j >> 2) ? tally[1] : tally[0]) >> (16 * (j & 3))) & 0xffff;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d);
        if (__lane_id() == 0 && c) atomicAdd(&painted[j], (unsigned long long)c);
    }
}

template <int C>
void launch(pb3d_ctx* ctx, const Walk& w, const Colours& cols, const Views& V, const Skip& skip, double eps, int eps_f32, u8* out,
            unsigned long long* painted) {
    const unsigned blocks = (unsigned)((w.nitems + 255) / 256);
    if (w.grid == out)
        hipLaunchKernelGGL((k_ppaint<C, true>), dim3(blocks), dim3(256), 0, ctx->stream, w, cols, V, skip, eps, eps_f32, out, painted);
    else
        hipLaunchKernelGGL((k_ppaint<C, false>), dim3(blocks), dim3(256), 0, ctx->stream, w, cols, V, skip, eps, eps_f32, out, painted);
}

}  // namespace

extern "C" {

int pb3d_perspective_paint_resident(pb3d_ctx* ctx, const uint8_t* d_grid, int64_t A0, int64_t A1, int64_t A2, int C, const uint8_t* colors,
                                    int ncolors, const pb3d_paint_view* views, int nviews, const uint8_t* skip, int nskip, double eps,
                                    int eps_f32, uint8_t* d_out, int64_t* d_painted) {
    PB3D_TRY(grid_args("pb3d_perspective_paint", d_grid, A0, A1, A2, C));
    Colours cols;
    PB3D_TRY(colour_args("pb3d_perspective_paint", colors, ncolors, C, &cols));
    PB3D_REQUIRE(A0 <= kMaxAxis && A1 <= kMaxAxis && A2 <= kMaxAxis, "pb3d_perspective_paint: an axis is longer than 2^24 (float32 coordinates)");
    PB3D_REQUIRE(nviews >= 0 && nviews <= kMaxViews, "pb3d_perspective_paint: 0 to %d views, got %d", kMaxViews, nviews);
    PB3D_REQUIRE(nviews == 0 || views, "pb3d_perspective_paint: null view table");
    PB3D_REQUIRE(nskip >= 0 && nskip <= kMaxSkip, "pb3d_perspective_paint: at most %d skip colours, got %d", kMaxSkip, nskip);
    PB3D_REQUIRE(nskip == 0 || skip, "pb3d_perspective_paint: null skip table");
    PB3D_REQUIRE(eps_f32 == 0 || eps_f32 == 1, "pb3d_perspective_paint: eps_f32 must be 0 or 1");
    Views V;
    memset(&V, 0, sizeof(V));
    V.n = nviews;
    for (int k = 0; k < nviews; ++k) {
        const pb3d_paint_view& s = views[k];
        PB3D_REQUIRE(s.Himg > 0 && s.Wimg > 0, "pb3d_perspective_paint: view %d has a %d x %d image", k, s.Himg, s.Wimg);
        PB3D_REQUIRE(s.d_image, "pb3d_perspective_paint: view %d has a null image", k);
        PB3D_REQUIRE(s.d_zbuf, "pb3d_perspective_paint: view %d has a null z-buffer", k);
        PB3D_TRY(fill_proj(&V.v[k].P, 0, s.R, s.cam, s.f, s.cx, s.cy, s.prec, s.Himg, s.Wimg));
        V.v[k].image = s.d_image;
        V.v[k].zbuf = s.d_zbuf;
    }
    Skip sk;
    memset(&sk, 0, sizeof(sk));
    sk.n = nskip;
    for (int k = 0; k < nskip; ++k) {
        const uint8_t* c = skip + (i64)k * C;
        sk.key[k] = C == 1 ? c[0] : (u32)c[0] | ((u32)c[1] << 8) | ((u32)c[2] << 16);
    }
    const i64 nvox = A0 * A1 * A2;
    PB3D_REQUIRE(nvox == 0 || d_out, "pb3d_perspective_paint: null output");
    PB3D_REQUIRE(nvox == 0 || d_out == d_grid || d_out + nvox * C <= d_grid || d_grid + nvox * C <= d_out,
                 "pb3d_perspective_paint: the output overlaps the grid in part");
    PB3D_REQUIRE(ctx, "pb3d_perspective_paint: null context");
    if (d_painted && nviews) PB3D_HIP(hipMemsetAsync(d_painted, 0, (size_t)nviews * sizeof(int64_t), ctx->stream));
    if (nvox == 0) return PB3D_OK;
    if (nviews == 0) {
        if (d_out != d_grid) PB3D_HIP(hipMemcpyAsync(d_out, d_grid, (size_t)nvox * C, hipMemcpyDeviceToDevice, ctx->stream));
        return PB3D_OK;
    }
    PB3D_REQUIRE(((A2 + 3) / 4 * A1 * ((A0 + kChunk - 1) / kChunk) + 255) / 256 <= 0x7fffffff, "pb3d_perspective_paint: grid too large for one launch");
    Walk w = make_walk(d_grid, A0, A1, A2, C);
    w.vec = w.vec && ((((uintptr_t)d_out) & 3u) == 0);
    if (C == 1) launch<1>(ctx, w, cols, V, sk, eps, eps_f32, d_out, (unsigned long long*)d_painted);
    else launch<3>(ctx, w, cols, V, sk, eps, eps_f32, d_out, (unsigned long long*)d_painted);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

}  // extern "C"
