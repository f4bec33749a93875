// Silhouette carving of a resident grid by pinhole views: a voxel goes when it projects onto background in some view.
//
// The reference has no perspective carving; what it has is the pinhole arithmetic of project_colored_voxels
// (utils/projection_utils.py:5-23), and that is the whole of the geometry here: voxel (a0, a1, a2) is the float32 point
// (x = a2, y = a1, z = a0), its pixel is project_xyz<0>'s (Z < 1e-8 clamped, rint, bounds test), bit for bit the pixel the
// reference would paint it on.
//
// Grid walk (grid_walk.h): a lane owns four consecutive a2 columns of one a1 row and walks them along a0 for up to kChunk steps.
// An empty voxel or one outside the colour set costs no projection.  A subject voxel runs through the views of the launch in
// order and stops at the first that rejects it, so the per-view counts are those of carving by one view after the other.
// Masks are bit images (one uint32 word per 32 pixels of a row): a 512 x 355 mask is 22 KB and stays in cache.
// Counts: a lane tallies its rejections per view in 16-bit fields (at most 4 * kChunk = 256 each), the wave adds them up with
// shuffles and issues one 64-bit atomic per view that rejected anything.
#include "pb3d_internal.h"
#include "grid_walk.h"
#include "project_point.h"

namespace {

using namespace pb3d_proj;
using namespace pb3d_walk;

constexpr int kMaxViews = 8;              // views of one launch (kernel arguments); the entry runs further views in place
constexpr i64 kMaxAxis = (i64)1 << 24;    // voxel coordinates are float32 points: exact below 2^24

struct View {
    ProjParams P;
    const u32* bits;                      // P.Himg rows of (P.Wimg + 31) / 32 words, bit u & 31 of word u >> 5
};

struct Views {
    View v[kMaxViews];
    int n, keep;                          // keep: a pixel outside the image accepts the voxel (else it rejects it)
};

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

// INPLACE: out is the walked grid and only zeroed voxels are written; else every voxel of the lane is
template <int C, bool INPLACE>
__global__ __launch_bounds__(256) void k_pcarve(Walk w, Colours cols, Views V, u8* out, unsigned long long* __restrict__ removed) {
    const i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    u64 tally[2] = {0, 0};                // view j: bits 16 * (j & 3) .. + 15 of tally[j >> 2]
    if (t < w.nitems) {
        const i64 a2 = (t % w.ngx) * 4, r = t / w.ngx, a1 = r % w.A1, a0s = (r / w.A1) * kChunk;
        const i64 a0e = a0s + kChunk < w.A0 ? a0s + kChunk : w.A0;
        for (i64 a0 = a0s; a0 < a0e; ++a0) {
            u32 v[4];
            load4<C>(w, a0, a1, a2, v);
            u32 gone = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!v[k] || (cols.n && !colour_bits(cols, v[k]))) continue;
                const double p[3] = {(double)(a2 + k), (double)a1, (double)a0};      // exact in float32: the entry bounds the axes by 2^24
                for (int j = 0; j < V.n; ++j) {
                    const View& vw = V.v[j];
                    int ui, vi;
                    bool reject = !V.keep;
                    if (project_xyz<0>(vw.P, p, &ui, &vi))
                        reject = !((vw.bits[(i64)vi * ((vw.P.Wimg + 31) >> 5) + (ui >> 5)] >> (ui & 31)) & 1u);
                    if (reject) {
                        tally[j >> 2] += (u64)1 << (16 * (j & 3));
                        gone |= 1u << k;
                        v[k] = 0;
                        break;
                    }
                }
            }
            if (INPLACE && !gone) continue;
            u8* o = out + ((a0 * w.A1 + a1) * w.A2 + a2) * C;
            if (w.vec) {
                store4_vec<C>(o, v);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (a2 + k >= w.A2 || (INPLACE && !((gone >> k) & 1u))) continue;
                    if (C == 1) {
                        o[k] = (u8)v[k];
                    } else {
                        o[3 * k] = (u8)v[k]; o[3 * k + 1] = (u8)(v[k] >> 8); o[3 * k + 2] = (u8)(v[k] >> 16);
                    }
                }
            }
        }
    }
    if (!removed) return;                 // wave-uniform; below, every lane of the wave takes part in the shuffles
    for (int j = 0; j < V.n; ++j) {
        int c = (int)((tally[j >> 2] >> (16 * (j & 3))) & 0xffffu);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d);
        if (__lane_id() == 0 && c) atomicAdd(&removed[j], (unsigned long long)c);
    }
}

template <int C>
void launch(pb3d_ctx* ctx, const Walk& w, const Colours& cols, const Views& V, u8* out, unsigned long long* removed) {
    const unsigned blocks = (unsigned)((w.nitems + 255) / 256);
    if (w.grid == out) hipLaunchKernelGGL((k_pcarve<C, true>), dim3(blocks), dim3(256), 0, ctx->stream, w, cols, V, out, removed);
    else hipLaunchKernelGGL((k_pcarve<C, false>), dim3(blocks), dim3(256), 0, ctx->stream, w, cols, V, out, removed);
}

}  // namespace

extern "C" {

int pb3d_perspective_carve_resident(pb3d_ctx* ctx, const uint8_t* d_grid, int64_t A0, int64_t A1, int64_t A2, int C, const uint8_t* colors,
                                    int ncolors, const pb3d_carve_view* views, int nviews, int outside_keep, uint8_t* d_out,
                                    int64_t* d_removed) {
    PB3D_TRY(grid_args("pb3d_perspective_carve", d_grid, A0, A1, A2, C));
    Colours cols;
    PB3D_TRY(colour_args("pb3d_perspective_carve", colors, ncolors, C, &cols));
    PB3D_REQUIRE(A0 <= kMaxAxis && A1 <= kMaxAxis && A2 <= kMaxAxis, "pb3d_perspective_carve: an axis is longer than 2^24 (float32 coordinates)");
    PB3D_REQUIRE(nviews >= 0, "pb3d_perspective_carve: %d views", nviews);
    PB3D_REQUIRE(nviews == 0 || views, "pb3d_perspective_carve: null view table");
    for (int k = 0; k < nviews; ++k) {
        PB3D_REQUIRE(views[k].Himg > 0 && views[k].Wimg > 0, "pb3d_perspective_carve: view %d has a %d x %d mask", k, views[k].Himg, views[k].Wimg);
        PB3D_REQUIRE(views[k].d_maskbits, "pb3d_perspective_carve: view %d has a null mask", k);
        ProjParams P;
        PB3D_TRY(fill_proj(&P, 0, views[k].R, views[k].cam, views[k].f, views[k].cx, views[k].cy, views[k].prec, views[k].Himg, views[k].Wimg));
    }
    PB3D_REQUIRE(ctx, "pb3d_perspective_carve: null context");
    const i64 nvox = A0 * A1 * A2;
    PB3D_REQUIRE(nvox == 0 || d_out, "pb3d_perspective_carve: null output");
    if (d_removed && nviews) PB3D_HIP(hipMemsetAsync(d_removed, 0, (size_t)nviews * sizeof(int64_t), ctx->stream));
    if (nvox == 0) return PB3D_OK;
    if (nviews == 0) {
        if (d_out != d_grid) PB3D_HIP(hipMemcpyAsync(d_out, d_grid, (size_t)nvox * C, hipMemcpyDeviceToDevice, ctx->stream));
        return PB3D_OK;
    }
    PB3D_REQUIRE(((A2 + 3) / 4 * A1 * ((A0 + kChunk - 1) / kChunk) + 255) / 256 <= 0x7fffffff, "pb3d_perspective_carve: grid too large for one launch");
    for (int base = 0; base < nviews; base += kMaxViews) {
        Views V;
        memset(&V, 0, sizeof(V));
        V.n = nviews - base < kMaxViews ? nviews - base : kMaxViews;
        V.keep = outside_keep ? 1 : 0;
        for (int k = 0; k < V.n; ++k) {
            const pb3d_carve_view& s = views[base + k];
            PB3D_TRY(fill_proj(&V.v[k].P, 0, s.R, s.cam, s.f, s.cx, s.cy, s.prec, s.Himg, s.Wimg));
            V.v[k].bits = s.d_maskbits;
        }
        // the first launch reads the caller's grid; the views past kMaxViews carve its result in place
        Walk w = make_walk(base == 0 ? d_grid : d_out, A0, A1, A2, C);
        w.vec = w.vec && ((((uintptr_t)d_out) & 3u) == 0);
        unsigned long long* rem = d_removed ? (unsigned long long*)d_removed + base : nullptr;
        if (C == 1) launch<1>(ctx, w, cols, V, d_out, rem);
        else launch<3>(ctx, w, cols, V, d_out, rem);
        PB3D_CHECK_LAUNCH();
    }
    return PB3D_OK;
}

}  // extern "C"
