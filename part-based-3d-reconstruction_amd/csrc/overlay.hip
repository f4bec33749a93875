// Notebook 2 (reference utils/camera_estimation.py:56-108 and :346-477) on the device: the bounding box of the voxels of a colour set,
// the per-part hit bits of a projection straight from the grid, and the overlay images of visualize_voxel_projection_iou.
//
// The reference projects every part on its own (get_voxel_points_by_parts + project_colored_voxels) and keeps all(proj == colour):
// a per-part projection paints one constant colour, so that mask is "some voxel of the colour lands on the pixel" -- one bit per
// colour and pixel, and one sweep of the grid gives the bit of every part (k_grid_hit_bits, run_walk of grid_walk.h with
// project_xyz<0>: Z < 1e-8 is clamped, there is no depth test).  The images are then composed per pixel from the bit image and the
// resident RGB image (k_overlay_compose).
//
// The blend (0.7 * proj + 0.3 * image).astype(np.uint8) is float64 in NumPy: two multiplies, one add, truncation.  It is evaluated
// here with __dmul_rn / __dadd_rn (and the build has -ffp-contract=off), so every byte is NumPy's.
#include "pb3d_internal.h"
#include "wave.h"
#include "grid_walk.h"

namespace {

using namespace pb3d_proj;
using namespace pb3d_walk;

constexpr int kMaxParts = 8 * kMaxColours;      // parts of one compose launch: part j is bit j % 31 of plane j / 31

// ---- (a) count and inclusive bounds of the selected voxels ---------------------------------------------------------------------
// out[0] = count, out[1..3] = min (a0, a1, a2), out[4..6] = max.  A lane keeps its own box, the wave reduces with shuffles, the four
// waves of a block meet in LDS and one lane issues the block's (at most seven) atomics.
__global__ void k_bounds_init(long long* __restrict__ out) {
    out[0] = 0;
    for (int k = 0; k < 3; ++k) { out[1 + k] = 0x7fffffffffffffffll; out[4 + k] = -1; }
}

template <int C>
__global__ __launch_bounds__(256) void k_grid_bounds(Walk w, Colours cols, long long* __restrict__ out) {
    __shared__ int s_box[4][7];
    const i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    int cnt = 0, lo0 = 0x7fffffff, lo1 = 0x7fffffff, lo2 = 0x7fffffff, hi0 = -1, hi1 = -1, hi2 = -1;
    i64 a2, a1, a0s, a0e;
    if (walk_item(w, t, &a2, &a1, &a0s, &a0e)) {
        u32 cols_hit = 0;
        for (i64 a0 = a0s; a0 < a0e; ++a0) {
            u32 v[4];
            load4<C>(w, a0, a1, a2, v);
            u32 m = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) m |= (u32)(v[k] && (cols.n == 0 || colour_bits(cols, v[k]))) << k;
            if (m) {
                cnt += __popc(m);
                cols_hit |= m;
                lo0 = lo0 < (int)a0 ? lo0 : (int)a0;
                hi0 = (int)a0;                              // a0 ascends
            }
        }
        if (cols_hit) {
            lo1 = hi1 = (int)a1;
            lo2 = (int)a2 + (__ffs(cols_hit) - 1);
            hi2 = (int)a2 + (31 - __clz(cols_hit));
        }
    }
    cnt = wave_sum(cnt);
    lo0 = wave_min(lo0); lo1 = wave_min(lo1); lo2 = wave_min(lo2);
    hi0 = wave_max(hi0); hi1 = wave_max(hi1); hi2 = wave_max(hi2);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_box[wave][0] = cnt;
        s_box[wave][1] = lo0; s_box[wave][2] = lo1; s_box[wave][3] = lo2;
        s_box[wave][4] = hi0; s_box[wave][5] = hi1; s_box[wave][6] = hi2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        long long n = 0;
        int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {-1, -1, -1};
        for (int q = 0; q < 4; ++q) {
            n += s_box[q][0];
            for (int k = 0; k < 3; ++k) {
                lo[k] = min(lo[k], s_box[q][1 + k]);
                hi[k] = max(hi[k], s_box[q][4 + k]);
            }
        }
        if (n) {
            atomicAdd((unsigned long long*)&out[0], (unsigned long long)n);
            for (int k = 0; k < 3; ++k) {
                if (__hip_atomic_load(&out[1 + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > lo[k]) atomicMin(&out[1 + k], (long long)lo[k]);
                if (__hip_atomic_load(&out[4 + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < hi[k]) atomicMax(&out[4 + k], (long long)hi[k]);
            }
        }
    }
}

// ---- (b) bits[v, u] |= 1 << k for every voxel of colour k whose projection lands on (u, v) --------------------------------------
struct HitRun {
    static constexpr int MODE = 0;
    typedef u32 State;
    const Colours& cols;
    u32* __restrict__ bits;
    __device__ __forceinline__ bool take(u32 v, u32* b) const {       // an empty voxel, which most are, costs no colour loop
        *b = v ? colour_bits(cols, v) : 0;
        return *b != 0;
    }
    __device__ __forceinline__ void open(i64, u32* br) const { *br = 0; }
    __device__ __forceinline__ void add(u32* br, u32 b, double) const { *br |= b; }
    __device__ __forceinline__ void flush(i64 px, u32 br) const { flush_or(bits, px, br); }
};

template <int C>
__global__ __launch_bounds__(256) void k_grid_hit_bits(Walk w, ProjParams P, Colours cols, u32* __restrict__ bits) {
    run_walk<C>(w, P, HitRun{cols, bits});
}

// ---- (c) the overlay images ------------------------------------------------------------------------------------------------------
struct Parts {
    u32 key[kMaxParts];                   // r | g << 8 | b << 16
    int n;
};

// (0.7 * a + 0.3 * b).astype(np.uint8) of two uint8 values, in float64
__device__ __forceinline__ u8 blend(u32 a, u32 b) {
    return (u8)(int)__dadd_rn(__dmul_rn(0.7, (double)a), __dmul_rn(0.3, (double)b));
}

__device__ __forceinline__ u32 pixel_key(const u8* __restrict__ img, i64 px) {
    return (u32)img[3 * px] | ((u32)img[3 * px + 1] << 8) | ((u32)img[3 * px + 2] << 16);
}

__device__ __forceinline__ void store_rgb(u8* __restrict__ o, u32 r, u32 g, u32 b) {
    o[0] = (u8)r; o[1] = (u8)g; o[2] = (u8)b;
}

// one wave-wide tally of (inter, union) into counts[2 * row], counts[2 * row + 1]; every lane of the wave calls it
__device__ __forceinline__ void tally(bool gt, bool prj, int row, unsigned long long* __restrict__ counts) {
    const u64 bi = __ballot(gt && prj), bu = __ballot(gt || prj);
    if (__lane_id() == 0 && bu) {
        if (bi) atomicAdd(&counts[2 * row], (unsigned long long)__popcll(bi));
        atomicAdd(&counts[2 * row + 1], (unsigned long long)__popcll(bu));
    }
}

// mode 0, part_on_whole (:394-419): per part its blended projection with the yellow outline of gt & prj; counts per part
__global__ __launch_bounds__(256) void k_overlay_parts(const u32* __restrict__ bits, const u8* __restrict__ img, int H, int W, Parts parts,
                                                       u8* __restrict__ vis, unsigned long long* __restrict__ counts) {
    const i64 npix = (i64)H * W, px = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = px < npix;
    const int y = in ? (int)(px / W) : 0, x = in ? (int)(px - (i64)y * W) : 0;
    // the pixel and its 4 neighbours (the cross of binary_dilation; outside the image counts as false)
    const i64 nb[4] = {y > 0 ? px - W : -1, y + 1 < H ? px + W : -1, x > 0 ? px - 1 : -1, x + 1 < W ? px + 1 : -1};
    u32 key = 0, nkey[4] = {0, 0, 0, 0};
    if (in) {
        key = pixel_key(img, px);
#pragma unroll
        for (int d = 0; d < 4; ++d)
            if (nb[d] >= 0) nkey[d] = pixel_key(img, nb[d]);
    }
    const u32 ir = key & 0xffu, ig = (key >> 8) & 0xffu, ib = key >> 16;
    const int nplanes = (parts.n + kMaxColours - 1) / kMaxColours;
    for (int s = 0; s < nplanes; ++s) {
        u32 word = 0, nword[4] = {0, 0, 0, 0};
        if (in) {
            word = bits[(i64)s * npix + px];
#pragma unroll
            for (int d = 0; d < 4; ++d)
                if (nb[d] >= 0) nword[d] = bits[(i64)s * npix + nb[d]];
        }
        const int jend = parts.n - s * kMaxColours < kMaxColours ? parts.n - s * kMaxColours : kMaxColours;
        for (int b = 0; b < jend; ++b) {
            const int j = s * kMaxColours + b;
            const u32 c = parts.key[j];
            const bool prj = in && ((word >> b) & 1u), gt = in && key == c;
            tally(gt, prj, j, counts);
            if (!in) continue;
            bool near = false;
#pragma unroll
            for (int d = 0; d < 4; ++d) near |= nb[d] >= 0 && ((nword[d] >> b) & 1u) && nkey[d] == c;
            u8* o = vis + ((i64)j * npix + px) * 3;
            if (near && !(gt && prj)) store_rgb(o, 255, 255, 0);
            else store_rgb(o, blend(prj ? c & 0xffu : 0, ir), blend(prj ? (c >> 8) & 0xffu : 0, ig), blend(prj ? c >> 16 : 0, ib));
        }
    }
}

// modes 1 and 2: whole_on_whole (:433-452: green = image only, red = projection only, yellow = both; one count pair) and
// whole_on_whole_color (:462-466: the sum of the colours of the parts that hit the pixel, clipped at 255, blended)
__global__ __launch_bounds__(256) void k_overlay_whole(const u32* __restrict__ bits, const u8* __restrict__ img, i64 npix, Parts parts, u32 bgkey,
                                                       const u8* __restrict__ extra_prj, int mode, u8* __restrict__ vis,
                                                       unsigned long long* __restrict__ counts) {
    const i64 px = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = px < npix;
    const int nplanes = (parts.n + kMaxColours - 1) / kMaxColours;
    u32 sr = 0, sg = 0, sb = 0;
    bool prj = false;
    if (in) {
        for (int s = 0; s < nplanes; ++s) {
            const int jend = parts.n - s * kMaxColours < kMaxColours ? parts.n - s * kMaxColours : kMaxColours;
            u32 word = bits[(i64)s * npix + px] & ((1u << jend) - 1u);      // jend <= 31
            prj |= word != 0;
            if (mode == 2)
                for (; word; word &= word - 1) {
                    const u32 c = parts.key[s * kMaxColours + __ffs(word) - 1];
                    sr += c & 0xffu; sg += (c >> 8) & 0xffu; sb += c >> 16;
                }
        }
        if (extra_prj && extra_prj[px]) prj = true;
    }
    const u32 key = in ? pixel_key(img, px) : 0;
    if (mode == 1) {
        const bool gt = in && key != bgkey;
        tally(gt, prj, 0, counts);
        if (in) store_rgb(vis + 3 * px, prj ? 255 : 0, gt ? 255 : 0, 0);
    } else if (in) {
        store_rgb(vis + 3 * px, blend(sr < 255 ? sr : 255, key & 0xffu), blend(sg < 255 ? sg : 255, (key >> 8) & 0xffu),
                  blend(sb < 255 ? sb : 255, key >> 16));
    }
}

}  // namespace

extern "C" {

int pb3d_grid_bounds_resident(pb3d_ctx* ctx, const uint8_t* d_grid, int64_t A0, int64_t A1, int64_t A2, int C, const uint8_t* colors, int ncolors,
                         int64_t* d_out) {
    PB3D_TRY(grid_args("pb3d_grid_bounds", d_grid, A0, A1, A2, C));
    Colours cols;
    PB3D_TRY(colour_args("pb3d_grid_bounds", colors, ncolors, C, &cols));
    PB3D_REQUIRE(A0 <= 0x7fffffff && A1 <= 0x7fffffff && A2 <= 0x7fffffff - 4, "pb3d_grid_bounds: an axis is longer than 2^31 - 5");
    PB3D_REQUIRE(ctx, "pb3d_grid_bounds: null context");
    PB3D_REQUIRE(d_out, "pb3d_grid_bounds: null buffer");
    hipLaunchKernelGGL(k_bounds_init, dim3(1), dim3(1), 0, ctx->stream, (long long*)d_out);
    PB3D_CHECK_LAUNCH();
    const Walk w = make_walk(d_grid, A0, A1, A2, C);
    if (w.nitems == 0) return PB3D_OK;
    return launch_walk("pb3d_grid_bounds", ctx, w, C, k_grid_bounds<1>, k_grid_bounds<3>, cols, (long long*)d_out);
}

int pb3d_grid_hit_bits_resident(pb3d_ctx* ctx, const uint8_t* d_grid, int64_t A0, int64_t A1, int64_t A2, int C, const uint8_t* colors,
                           int ncolors, const double R[9], const double cam[3], double f, double cx, double cy, const int prec[4], int Himg,
                           int Wimg, uint32_t* d_bits) {
    PB3D_TRY(grid_args("pb3d_grid_hit_bits", d_grid, A0, A1, A2, C));
    Colours cols;
    PB3D_TRY(colour_args("pb3d_grid_hit_bits", colors, ncolors, C, &cols));
    PB3D_REQUIRE(A0 <= kMaxAxis && A1 <= kMaxAxis && A2 <= kMaxAxis, "pb3d_grid_hit_bits: an axis is longer than 2^24 (float32 coordinates)");
    PB3D_REQUIRE(R && cam && prec && Himg >= 0 && Wimg >= 0, "pb3d_grid_hit_bits: bad argument");
    PB3D_REQUIRE(ctx, "pb3d_grid_hit_bits: null context");
    const i64 npix = (i64)Himg * Wimg;
    if (npix == 0) return PB3D_OK;
    PB3D_REQUIRE(d_bits, "pb3d_grid_hit_bits: null buffer");
    ProjParams P;
    PB3D_TRY(fill_proj(&P, 0, R, cam, f, cx, cy, prec, Himg, Wimg));
    PB3D_HIP(hipMemsetAsync(d_bits, 0, (size_t)npix * 4, ctx->stream));
    const Walk w = make_walk(d_grid, A0, A1, A2, C);
    if (w.nitems == 0 || ncolors == 0) return PB3D_OK;
    return launch_walk("pb3d_grid_hit_bits", ctx, w, C, k_grid_hit_bits<1>, k_grid_hit_bits<3>, P, cols, d_bits);
}

int pb3d_overlay_compose_resident(pb3d_ctx* ctx, const uint32_t* d_bits, int nplanes, const uint8_t* d_image, int Himg, int Wimg,
                             const uint8_t* colors, int nparts, const uint8_t bg[3], const uint8_t* d_extra_prj, int mode, uint8_t* d_vis,
                             int64_t* d_counts) {
    PB3D_REQUIRE(mode >= PB3D_OVERLAY_PART_ON_WHOLE && mode <= PB3D_OVERLAY_WHOLE_ON_WHOLE_COLOR, "pb3d_overlay_compose: mode is 0, 1 or 2, got %d",
                 mode);
    PB3D_REQUIRE(nparts >= 0 && nparts <= kMaxParts, "pb3d_overlay_compose: at most %d parts, got %d", kMaxParts, nparts);
    PB3D_REQUIRE(nplanes == (nparts + kMaxColours - 1) / kMaxColours, "pb3d_overlay_compose: %d parts take %d bit planes, got %d", nparts,
                 (nparts + kMaxColours - 1) / kMaxColours, nplanes);
    PB3D_REQUIRE(nparts == 0 || colors, "pb3d_overlay_compose: null colour table");
    PB3D_REQUIRE(Himg >= 0 && Wimg >= 0 && (mode != PB3D_OVERLAY_WHOLE_ON_WHOLE || bg), "pb3d_overlay_compose: bad argument");
    PB3D_REQUIRE(ctx, "pb3d_overlay_compose: null context");
    const i64 npix = (i64)Himg * Wimg;
    const int ncounts = mode == PB3D_OVERLAY_PART_ON_WHOLE ? 2 * nparts : mode == PB3D_OVERLAY_WHOLE_ON_WHOLE ? 2 : 0;
    PB3D_REQUIRE(ncounts == 0 || d_counts, "pb3d_overlay_compose: null buffer");
    if (ncounts) PB3D_HIP(hipMemsetAsync(d_counts, 0, (size_t)ncounts * sizeof(int64_t), ctx->stream));
    if (npix == 0 || (mode == PB3D_OVERLAY_PART_ON_WHOLE && nparts == 0)) return PB3D_OK;
    PB3D_REQUIRE(d_image && d_vis && (nparts == 0 || d_bits), "pb3d_overlay_compose: null buffer");
    PB3D_REQUIRE((npix + 255) / 256 <= 0x7fffffff, "pb3d_overlay_compose: image too large for one launch");
    Parts parts;
    memset(&parts, 0, sizeof(parts));
    parts.n = nparts;
    for (int j = 0; j < nparts; ++j) parts.key[j] = (u32)colors[3 * j] | ((u32)colors[3 * j + 1] << 8) | ((u32)colors[3 * j + 2] << 16);
    const unsigned blocks = (unsigned)((npix + 255) / 256);
    if (mode == PB3D_OVERLAY_PART_ON_WHOLE) {
        hipLaunchKernelGGL(k_overlay_parts, dim3(blocks), dim3(256), 0, ctx->stream, d_bits, d_image, Himg, Wimg, parts, d_vis,
                           (unsigned long long*)d_counts);
    } else {
        const u32 bgkey = bg ? (u32)bg[0] | ((u32)bg[1] << 8) | ((u32)bg[2] << 16) : 0;
        hipLaunchKernelGGL(k_overlay_whole, dim3(blocks), dim3(256), 0, ctx->stream, d_bits, d_image, npix, parts, bgkey, d_extra_prj, mode,
                           d_vis, (unsigned long long*)d_counts);
    }
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

}  // extern "C"
