// Painting of a resident grid by pinhole views: a subject voxel takes the colour of the pixel the first view sees it at.
//
// The perspective counterpart of apply_colored_mask_to_voxel_grid.  Nothing here is new arithmetic: voxel (a0, a1, a2) is the
// float32 point (x = a2, y = a1, z = a0), its pixel and depth are project_xyz<1>'s (the z-buffer functions of the reference,
// utils/eval_helpers_intra.py:134-190: Z <= 1e-6 dropped, rint, bounds test), and a view sees it when |Z - zbuf[v, u]| < eps in the
// widths of visible() (project_point.h).  The z-buffers are the caller's (pb3d_grid_depth_buffer_dev of the grid before painting).
//
// The kernel is the decide-and-rewrite shell of grid_walk.h (rewrite_walk: the walk, the subject test, the view loop, the stores and
// the per-view counts); what is here is what a view decides.  A subject voxel runs through the views in order and stops at the
// first that paints it.  The image and the z-buffer of a view are read only behind a true project_xyz<1>: that test is the bounds
// check of both reads.  Images are read byte by byte at (v * W + u) * C, so any base address will do.
#include "pb3d_internal.h"
#include "grid_walk.h"

namespace {

using namespace pb3d_proj;
using namespace pb3d_walk;

constexpr int kMaxViews = 8;              // views of a call (kernel arguments)
constexpr int kMaxSkip = 8;               // image colours / labels that never paint

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

__device__ __forceinline__ bool skipped(const Skip& s, u32 key) {
    bool b = false;
    for (int k = 0; k < s.n; ++k) b |= s.key[k] == key;
    return b;
}

// view j paints the voxel it sees (project_xyz<1> and visible()) on a pixel that is neither black nor skipped: the pixel's key
template <int C, bool INPLACE>
__global__ __launch_bounds__(256) void k_ppaint(Walk w, Colours cols, Views V, Skip skip, double eps, int eps_f32, u8* out,
                                                unsigned long long* __restrict__ painted) {
    rewrite_walk<C, INPLACE>(w, cols, V.n, [&](int j, const double p[3], u32* key) {
        const View& vw = V.v[j];
        int ui, vi;
        double z;
        if (!project_xyz<1>(vw.P, p, &ui, &vi, &z)) return false;                    // below: 0 <= ui < Wimg, 0 <= vi < Himg
        const i64 q = (i64)vi * vw.P.Wimg + ui;
        if (!visible(z, vw.zbuf[q], vw.P.t0, eps, eps_f32)) return false;
        const u8* px = vw.image + q * C;
        *key = C == 1 ? (u32)px[0] : (u32)px[0] | ((u32)px[1] << 8) | ((u32)px[2] << 16);
        return *key && !skipped(skip, *key);
    }, out, painted);
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
        PB3D_TRY(view_args("pb3d_perspective_paint", k, s.Himg, s.Wimg, "image", s.d_image));
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
    Walk w = make_walk(d_grid, A0, A1, A2, C);
    w.vec = w.vec && ((((uintptr_t)d_out) & 3u) == 0);
    unsigned long long* cnt = (unsigned long long*)d_painted;
    if (d_out == d_grid)
        return launch_walk("pb3d_perspective_paint", ctx, w, C, k_ppaint<1, true>, k_ppaint<3, true>, cols, V, sk, eps, eps_f32, d_out, cnt);
    return launch_walk("pb3d_perspective_paint", ctx, w, C, k_ppaint<1, false>, k_ppaint<3, false>, cols, V, sk, eps, eps_f32, d_out, cnt);
}

}  // extern "C"
