// Notebook 4 (intra-method evaluation, reference utils/eval_helpers_intra.py:287-748) on the device: z-buffers and visible-part bits
// straight from a voxel grid, visible bits of several point lists, the colour set of a grid, and per-row IoU counts.
//
// The reference builds every z-buffer and visibility mask from a point list (np.where over the grid, then a Python loop per point);
// the point path of project.hip does the same on the device (count + fill + scatter).  Here the grid itself is walked: voxel
// (a0, a1, a2) is the point (x = a2, y = a1, z = a0), projected by the same project_xyz<1> as the point path, so every pixel and depth
// is the point path's bit for bit.
//
// Grid walk (grid_walk.h): a lane owns four consecutive a2 columns of one a1 row and walks them along a0 for up to kChunk steps, loading the four
// voxels with dword loads where the rows allow it (lanes of a wave take consecutive a2).  Under a front camera a column along a0 lands
// on a handful of pixels, so each column keeps a run: the minimum depth (or the OR of visible bits) while its pixel stays the same,
// flushed with one atomic when the pixel changes or the walk ends.  The run is exact: float32 min and bit OR are order-free.
// That loop is run_walk of grid_walk.h; k_grid_depth and k_grid_visible_bits are a policy each (what a run holds and how it is flushed).
#include "pb3d_internal.h"
#include "grid_walk.h"

namespace {

using namespace pb3d_proj;
using namespace pb3d_walk;      // Walk, walk_item, Colours, colour_bits, load4, flush_or, launch_walk and the argument checks (grid_walk.h)

constexpr int kMaxRows = 32;

// (a) zbits[v, u] = float32 bits of the minimum Z over the occupied voxels landing on (u, v).  Every Z is positive and finite, so a
// run opens at +inf and the order of the bits is the order of the depths.
struct DepthRun {
    static constexpr int MODE = 1;
    typedef u32 State;
    u32* __restrict__ zbits;
    __device__ __forceinline__ bool take(u32 v, u32* b) const { *b = 0; return v != 0; }
    __device__ __forceinline__ void open(i64, u32* zr) const { *zr = 0x7f800000u; }
    __device__ __forceinline__ void add(u32* zr, u32, double z) const { *zr = min(*zr, __float_as_uint((float)z)); }
    __device__ __forceinline__ void flush(i64 px, u32 zr) const {
        if (__hip_atomic_load(&zbits[px], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > zr) atomicMin(&zbits[px], zr);
    }
};

template <int C>
__global__ __launch_bounds__(256) void k_grid_depth(Walk w, ProjParams P, u32* __restrict__ zbits) {
    run_walk<C>(w, P, DepthRun{zbits});
}

// (b) bits[v, u] |= (1 << k) for a visible voxel of colour k, | kAnyBit for any visible occupied voxel.  A run keeps its pixel's depth.
struct VisibleRun {
    static constexpr int MODE = 1;
    struct State { u32 br; float zr; };
    const float* __restrict__ zbuf;
    double eps;
    int eps_f32, t0;
    const Colours& cols;
    u32* __restrict__ bits;
    __device__ __forceinline__ bool take(u32 v, u32* b) const { *b = v; return v != 0; }
    __device__ __forceinline__ void open(i64 px, State* s) const { s->br = 0; s->zr = zbuf[px]; }
    __device__ __forceinline__ void add(State* s, u32 v, double z) const {
        if (visible(z, s->zr, t0, eps, eps_f32)) s->br |= kAnyBit | colour_bits(cols, v);
    }
    __device__ __forceinline__ void flush(i64 px, const State& s) const { flush_or(bits, px, s.br); }
};

template <int C>
__global__ __launch_bounds__(256) void k_grid_visible_bits(Walk w, ProjParams P, const float* __restrict__ zbuf, double eps, int eps_f32,
                                                           Colours cols, u32* __restrict__ bits) {
    run_walk<C>(w, P, VisibleRun{zbuf, eps, eps_f32, P.t0, cols, bits});
}

// (c) bits[v, u] |= 1 << list for a visible point of list `list` (blockIdx.y)
struct Lists {
    const void* p[kMaxColours];
    i64 n[kMaxColours];
    int type;                             // 0 float32, 1 float64, 2 int64
};

__global__ __launch_bounds__(256) void k_points_visible_bits(Lists L, ProjParams P, const float* __restrict__ zbuf, double eps, int eps_f32,
                                                             u32* __restrict__ bits) {
    const int list = blockIdx.y;
    const i64 n = L.n[list];
    const u32 mine = 1u << list;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x) {
        double p[3];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            p[k] = L.type == 2 ? (double)((const long long*)L.p[list])[3 * i + k]
                 : L.type == 1 ? ((const double*)L.p[list])[3 * i + k] : (double)((const float*)L.p[list])[3 * i + k];
        int ui, vi;
        double z;
        if (!project_xyz<1>(P, p, &ui, &vi, &z)) continue;
        const i64 q = (i64)vi * P.Wimg + ui;
        if (visible(z, zbuf[q], P.t0, eps, eps_f32)) flush_or(bits, q, mine);
    }
}

// (d, pass one) bitmap bit `key` for every non-zero voxel value.  A lane sends a key only when it differs from its previous one and
// its bit is not set yet, and the wave sends each distinct key once (leader loop).
__device__ __forceinline__ void send_keys(u32 cand, u32* __restrict__ bitmap) {
    if (cand && ((bitmap[cand >> 5] >> (cand & 31)) & 1u)) cand = 0;      // already known (a plain, mostly L1-hit load)
    u64 pend = __ballot(cand != 0);
    while (pend) {
        const int leader = __ffsll((unsigned long long)pend) - 1;
        const u32 k = (u32)__shfl((int)cand, leader);
        if (cand == k) {
            if ((int)__lane_id() == leader) flush_or(bitmap, (i64)(k >> 5), 1u << (k & 31));
            cand = 0;
        }
        pend = __ballot(cand != 0);
    }
}

template <int C>
__global__ __launch_bounds__(256) void k_color_presence(const u8* __restrict__ grid, i64 nvox, int vec, u32* __restrict__ bitmap) {
    const i64 ng = (nvox + 3) / 4, stride = (i64)gridDim.x * blockDim.x;
    // wave-uniform trip count: every lane of a wave takes part in each ballot of send_keys
    const i64 wave0 = ((i64)blockIdx.x * blockDim.x + threadIdx.x) & ~(i64)63;
    u32 last = 0;
    for (i64 base = wave0; base < ng; base += stride) {
        const i64 g = base + __lane_id();
        u32 v[4] = {0, 0, 0, 0};
        if (g < ng) load4<C>(grid + g * 4 * C, vec, g * 4, nvox, v);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const u32 cand = v[k] && v[k] != last ? v[k] : 0u;
            if (v[k]) last = v[k];
            send_keys(cand, bitmap);
        }
    }
}

// present[0] bit k = colour k is in the bitmap
__global__ void k_presence_probe(const u32* __restrict__ bitmap, Colours cols, i64* __restrict__ present) {
    i64 b = 0;
    for (int k = 0; k < cols.n; ++k) b |= (i64)((bitmap[cols.key[k] >> 5] >> (cols.key[k] & 31)) & 1u) << k;
    *present = b;
}

// (d, pass two, and the part ground truths) bits[px] = colour matches of an RGB mask pixel, | kAnyBit where its colour is in the bitmap
__global__ __launch_bounds__(256) void k_mask_bits(const u8* __restrict__ mask, i64 npix, Colours cols, const u32* __restrict__ bitmap,
                                                   u32* __restrict__ bits) {
    for (i64 px = (i64)blockIdx.x * blockDim.x + threadIdx.x; px < npix; px += (i64)gridDim.x * blockDim.x) {
        const u32 key = (u32)mask[3 * px] | ((u32)mask[3 * px + 1] << 8) | ((u32)mask[3 * px + 2] << 16);
        u32 b = colour_bits(cols, key);
        if (bitmap && key && ((bitmap[key >> 5] >> (key & 31)) & 1u)) b |= kAnyBit;
        bits[px] = b;
    }
}

// (e) per row: pred = pred[px] & pred_bits, gt = gt[px] & gt_bits [& gate[px] & gate_bits]; counts[2r] += |pred & gt|,
// counts[2r + 1] += |pred | gt|.  Lane r of a wave keeps row r's tally (the ballots are wave-uniform); one atomic per wave and row.
struct Rows {
    pb3d_iou_row r[kMaxRows];
    int n;
};

__device__ __forceinline__ bool hit(const uint32_t* img, uint32_t m, i64 px, bool in) {
    return in && img && (img[px] & m);
}

__global__ __launch_bounds__(256) void k_iou_rows(Rows R, i64 npix, unsigned long long* __restrict__ counts) {
    const int lane = __lane_id();
    const i64 stride = (i64)gridDim.x * blockDim.x;
    unsigned long long ai = 0, au = 0;
    for (i64 base = ((i64)blockIdx.x * blockDim.x + threadIdx.x) & ~(i64)63; base < npix; base += stride) {
        const i64 px = base + lane;
        const bool in = px < npix;
        for (int r = 0; r < R.n; ++r) {
            const pb3d_iou_row& row = R.r[r];
            const bool pr = hit(row.pred, row.pred_bits, px, in);
            const bool gt = hit(row.gt, row.gt_bits, px, in) && (!row.gate || hit(row.gate, row.gate_bits, px, in));
            const unsigned long long ni = __popcll(__ballot(pr && gt)), nu = __popcll(__ballot(pr || gt));
            if (lane == r) { ai += ni; au += nu; }
        }
    }
    if (lane < R.n && au) {
        atomicAdd(&counts[2 * lane], ai);
        atomicAdd(&counts[2 * lane + 1], au);
    }
}

}  // namespace

extern "C" {

int pb3d_grid_depth_buffer_dev(pb3d_ctx* ctx, const uint8_t* d_grid, int64_t A0, int64_t A1, int64_t A2, int C, const double R[9],
                               const double cam[3], double f, double cx, double cy, const int prec[4], int Himg, int Wimg, float* d_zbuf) {
    PB3D_TRY(grid_args("pb3d_grid_depth_buffer", d_grid, A0, A1, A2, C));
    PB3D_REQUIRE(R && cam && prec && Himg >= 0 && Wimg >= 0, "pb3d_grid_depth_buffer: bad argument");
    const Walk w = make_walk(d_grid, A0, A1, A2, C);
    PB3D_TRY(walk_fits("pb3d_grid_depth_buffer", w));      // here as well as in launch_walk: refused without a context, like the rest
    PB3D_REQUIRE(ctx, "pb3d_grid_depth_buffer: null context");
    const i64 npix = (i64)Himg * Wimg;
    if (npix == 0) return PB3D_OK;
    PB3D_REQUIRE(d_zbuf, "pb3d_grid_depth_buffer: null buffer");
    ProjParams P;
    PB3D_TRY(fill_proj(&P, 0, R, cam, f, cx, cy, prec, Himg, Wimg));
    PB3D_HIP(hipMemsetD32Async((hipDeviceptr_t)d_zbuf, 0x7f800000, (size_t)npix, ctx->stream));   // +inf
    if (w.nitems == 0) return PB3D_OK;
    return launch_walk("pb3d_grid_depth_buffer", ctx, w, C, k_grid_depth<1>, k_grid_depth<3>, P, (u32*)d_zbuf);
}

int pb3d_grid_visible_bits_dev(pb3d_ctx* ctx, const uint8_t* d_grid, int64_t A0, int64_t A1, int64_t A2, int C, const uint8_t* colors,
                               int ncolors, const double R[9], const double cam[3], double f, double cx, double cy, const int prec[4],
                               const float* d_zbuf, int zH, int zW, int Himg, int Wimg, double eps, int eps_f32, uint32_t* d_bits) {
    PB3D_TRY(grid_args("pb3d_grid_visible_bits", d_grid, A0, A1, A2, C));
    Colours cols;
    PB3D_TRY(colour_args("pb3d_grid_visible_bits", colors, ncolors, C, &cols));
    PB3D_REQUIRE(R && cam && prec && Himg >= 0 && Wimg >= 0, "pb3d_grid_visible_bits: bad argument");
    PB3D_REQUIRE(zH == Himg && zW == Wimg, "pb3d_grid_visible_bits: zbuf is %dx%d, the image %dx%d", zH, zW, Himg, Wimg);
    const Walk w = make_walk(d_grid, A0, A1, A2, C);
    PB3D_TRY(walk_fits("pb3d_grid_visible_bits", w));      // as in pb3d_grid_depth_buffer_dev
    PB3D_REQUIRE(ctx, "pb3d_grid_visible_bits: null context");
    const i64 npix = (i64)Himg * Wimg;
    if (npix == 0) return PB3D_OK;
    PB3D_REQUIRE(d_zbuf && d_bits, "pb3d_grid_visible_bits: null buffer");
    ProjParams P;
    PB3D_TRY(fill_proj(&P, 0, R, cam, f, cx, cy, prec, Himg, Wimg));
    PB3D_HIP(hipMemsetAsync(d_bits, 0, (size_t)npix * 4, ctx->stream));
    if (w.nitems == 0) return PB3D_OK;
    return launch_walk("pb3d_grid_visible_bits", ctx, w, C, k_grid_visible_bits<1>, k_grid_visible_bits<3>, P, d_zbuf, eps, eps_f32, cols, d_bits);
}

int pb3d_points_visible_bits_dev(pb3d_ctx* ctx, const void* const* d_lists, const int64_t* counts, int nlists, int pts_type, const double R[9],
                                 const double cam[3], double f, double cx, double cy, const int prec[4], const float* d_zbuf, int zH, int zW,
                                 int Himg, int Wimg, double eps, int eps_f32, uint32_t* d_bits) {
    PB3D_REQUIRE(nlists >= 0 && nlists <= kMaxColours, "pb3d_points_visible_bits: at most %d point lists, got %d", kMaxColours, nlists);
    PB3D_REQUIRE(pts_type >= 0 && pts_type <= 2, "pb3d_points_visible_bits: pts_type is 0 (float32), 1 (float64) or 2 (int64)");
    PB3D_REQUIRE(nlists == 0 || (d_lists && counts), "pb3d_points_visible_bits: null list table");
    PB3D_REQUIRE(R && cam && prec && Himg >= 0 && Wimg >= 0, "pb3d_points_visible_bits: bad argument");
    PB3D_REQUIRE(zH == Himg && zW == Wimg, "pb3d_points_visible_bits: zbuf is %dx%d, the image %dx%d", zH, zW, Himg, Wimg);
    Lists L;
    memset(&L, 0, sizeof(L));
    L.type = pts_type;
    i64 nmax = 0;
    for (int k = 0; k < nlists; ++k) {
        PB3D_REQUIRE(counts[k] >= 0 && (counts[k] == 0 || d_lists[k]), "pb3d_points_visible_bits: bad list %d", k);
        L.p[k] = d_lists[k]; L.n[k] = counts[k];
        nmax = counts[k] > nmax ? counts[k] : nmax;
    }
    PB3D_REQUIRE(ctx, "pb3d_points_visible_bits: null context");
    const i64 npix = (i64)Himg * Wimg;
    if (npix == 0) return PB3D_OK;
    PB3D_REQUIRE(d_zbuf && d_bits, "pb3d_points_visible_bits: null buffer");
    ProjParams P;
    PB3D_TRY(fill_proj(&P, pts_type == 1, R, cam, f, cx, cy, prec, Himg, Wimg));
    PB3D_HIP(hipMemsetAsync(d_bits, 0, (size_t)npix * 4, ctx->stream));
    if (nmax == 0) return PB3D_OK;
    hipLaunchKernelGGL(k_points_visible_bits, dim3(pb3d_batch_blocks(ctx, nmax, 256, nlists, 8), nlists), dim3(256), 0, ctx->stream, L, P,
                       d_zbuf, eps, eps_f32, d_bits);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

int pb3d_color_presence_dev(pb3d_ctx* ctx, const uint8_t* d_grid, int64_t nvox, int C, uint32_t* d_bitmap, const uint8_t* colors, int ncolors,
                            int64_t* d_present) {
    PB3D_TRY(grid_args("pb3d_color_presence", d_grid, nvox, 1, 1, C));
    Colours cols;
    PB3D_TRY(colour_args("pb3d_color_presence", colors, ncolors, C, &cols));
    PB3D_REQUIRE(ctx, "pb3d_color_presence: null context");
    PB3D_REQUIRE(d_bitmap && (ncolors == 0 || d_present), "pb3d_color_presence: null buffer");
    PB3D_HIP(hipMemsetAsync(d_bitmap, 0, PB3D_PRESENCE_BYTES, ctx->stream));
    if (nvox > 0) {
        const int vec = (nvox % 4 == 0) && ((((uintptr_t)d_grid) & 3u) == 0);
        const unsigned blocks = pb3d_stream_blocks(ctx, (nvox + 3) / 4, 256, 8);
        if (C == 1) hipLaunchKernelGGL(k_color_presence<1>, dim3(blocks), dim3(256), 0, ctx->stream, d_grid, nvox, vec, d_bitmap);
        else hipLaunchKernelGGL(k_color_presence<3>, dim3(blocks), dim3(256), 0, ctx->stream, d_grid, nvox, vec, d_bitmap);
        PB3D_CHECK_LAUNCH();
    }
    if (d_present) {
        hipLaunchKernelGGL(k_presence_probe, dim3(1), dim3(1), 0, ctx->stream, (const u32*)d_bitmap, cols, (i64*)d_present);
        PB3D_CHECK_LAUNCH();
    }
    return PB3D_OK;
}

int pb3d_mask_bits_dev(pb3d_ctx* ctx, const uint8_t* d_mask, int64_t npix, const uint8_t* colors, int ncolors, const uint32_t* d_bitmap,
                       uint32_t* d_bits) {
    Colours cols;
    PB3D_TRY(colour_args("pb3d_mask_bits", colors, ncolors, 3, &cols));
    PB3D_REQUIRE(npix >= 0, "pb3d_mask_bits: bad argument");
    PB3D_REQUIRE(ctx, "pb3d_mask_bits: null context");
    if (npix == 0) return PB3D_OK;
    PB3D_REQUIRE(d_mask && d_bits, "pb3d_mask_bits: null buffer");
    hipLaunchKernelGGL(k_mask_bits, dim3(pb3d_stream_blocks(ctx, npix, 256, 8)), dim3(256), 0, ctx->stream, d_mask, npix, cols,
                       (const u32*)d_bitmap, d_bits);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

int pb3d_iou_rows_dev(pb3d_ctx* ctx, const pb3d_iou_row* rows, int nrows, int64_t npix, int64_t* d_counts) {
    PB3D_REQUIRE(nrows >= 0 && nrows <= kMaxRows, "pb3d_iou_rows: at most %d rows, got %d", kMaxRows, nrows);
    PB3D_REQUIRE(npix >= 0 && (nrows == 0 || rows), "pb3d_iou_rows: bad argument");
    PB3D_REQUIRE(ctx, "pb3d_iou_rows: null context");
    if (nrows == 0) return PB3D_OK;
    PB3D_REQUIRE(d_counts, "pb3d_iou_rows: null buffer");
    Rows R;
    memset(&R, 0, sizeof(R));
    R.n = nrows;
    for (int k = 0; k < nrows; ++k) R.r[k] = rows[k];
    PB3D_HIP(hipMemsetAsync(d_counts, 0, (size_t)nrows * 2 * sizeof(int64_t), ctx->stream));
    if (npix == 0) return PB3D_OK;
    hipLaunchKernelGGL(k_iou_rows, dim3(pb3d_stream_blocks(ctx, npix, 256, 4)), dim3(256), 0, ctx->stream, R, npix,
                       (unsigned long long*)d_counts);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

}  // extern "C"
