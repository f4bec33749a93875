// Silhouette carving of a resident grid by pinhole views: a voxel goes when it projects onto background in some view.
//
// The reference has no perspective carving; what it has is the pinhole arithmetic of project_colored_voxels
// (utils/projection_utils.py:5-23), and that is the whole of the geometry here: voxel (a0, a1, a2) is the float32 point
// (x = a2, y = a1, z = a0), its pixel is project_xyz<0>'s (Z < 1e-8 clamped, rint, bounds test), bit for bit the pixel the
// reference would paint it on.
//
// The kernel is the decide-and-rewrite shell of grid_walk.h (rewrite_walk: the walk, the subject test, the view loop, the stores and
// the per-view counts); what is here is what a view decides.  A subject voxel runs through the views of the launch in order and
// stops at the first that rejects it, so the per-view counts are those of carving by one view after the other.
// Masks are bit images (one uint32 word per 32 pixels of a row): a 512 x 355 mask is 22 KB and stays in cache.
#include "pb3d_internal.h"
#include "grid_walk.h"
#include <exception>
#include <vector>

namespace {

using namespace pb3d_proj;
using namespace pb3d_walk;

constexpr int kMaxViews = 8;              // views of one launch (kernel arguments); the entry runs further views in place

struct View {
    ProjParams P;
    const u32* bits;                      // P.Himg rows of (P.Wimg + 31) / 32 words, bit u & 31 of word u >> 5
};

struct Views {
    View v[kMaxViews];
    int n, keep;                          // keep: a pixel outside the image accepts the voxel (else it rejects it)
};

// view j rejects the voxel whose pixel is clear in its mask, or outside its image unless V.keep; a rejected voxel becomes 0
template <int C, bool INPLACE>
__global__ __launch_bounds__(256) void k_pcarve(Walk w, Colours cols, Views V, u8* out, unsigned long long* __restrict__ removed) {
    rewrite_walk<C, INPLACE>(w, cols, V.n, [&](int j, const double p[3], u32* key) {
        const View& vw = V.v[j];
        int ui, vi;
        *key = 0;
        if (!project_xyz<0>(vw.P, p, &ui, &vi)) return !V.keep;
        return !((vw.bits[(i64)vi * ((vw.P.Wimg + 31) >> 5) + (ui >> 5)] >> (ui & 31)) & 1u);
    }, out, removed);
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
    std::vector<Views> launches;                                                     // kMaxViews views to a launch
    try {
        launches.resize(((size_t)nviews + kMaxViews - 1) / kMaxViews);               // zeroed
    } catch (const std::exception&) {
        pb3d_set_error("pb3d_perspective_carve: no host memory for %d views", nviews);
        return PB3D_ENOMEM;
    }
    for (int k = 0; k < nviews; ++k) {
        const pb3d_carve_view& s = views[k];
        Views& V = launches[k / kMaxViews];
        View& v = V.v[V.n++];
        PB3D_TRY(view_args("pb3d_perspective_carve", k, s.Himg, s.Wimg, "mask", s.d_maskbits));
        PB3D_TRY(fill_proj(&v.P, 0, s.R, s.cam, s.f, s.cx, s.cy, s.prec, s.Himg, s.Wimg));
        v.bits = s.d_maskbits;
        V.keep = outside_keep ? 1 : 0;
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
    for (size_t l = 0; l < launches.size(); ++l) {
        // the first launch reads the caller's grid; the views past kMaxViews carve its result in place
        Walk w = make_walk(l == 0 ? d_grid : d_out, A0, A1, A2, C);
        w.vec = w.vec && ((((uintptr_t)d_out) & 3u) == 0);
        unsigned long long* rem = d_removed ? (unsigned long long*)d_removed + l * kMaxViews : nullptr;
        if (w.grid == d_out)
            PB3D_TRY(launch_walk("pb3d_perspective_carve", ctx, w, C, k_pcarve<1, true>, k_pcarve<3, true>, cols, launches[l], d_out, rem));
        else
            PB3D_TRY(launch_walk("pb3d_perspective_carve", ctx, w, C, k_pcarve<1, false>, k_pcarve<3, false>, cols, launches[l], d_out, rem));
    }
    return PB3D_OK;
}

}  // extern "C"
