// The density volume of the inter-method evaluation: pointcloud_to_voxel_grid (reference utils/eval_helpers.py:178-189), bit for bit.
//
// The reference normalises the cloud into the unit cube (normalize_preserve_aspect: (p - min) / (max extent + 1e-8), then the y column
// shifted so that its maximum is 0), truncates norm * (G - 1) to integers, counts the points per voxel with np.add.at on a float32
// volume (NumPy wraps the y indices, which are <= 0, to the far planes), smooths with scipy.ndimage.gaussian_filter and zeroes the six
// faces.  Here:
//   k_density_scatter   the normalisation in the point dtype, one correctly rounded operation per NumPy operation, and one atomic add
//                       per point into a zeroed u32 count volume.  Integer counts do not depend on the order of the additions; a
//                       float32 cell stops growing at 2^24, so the value the filter reads is (float)min(count, 2^24).
//   k_density_filter    one pass per axis, SciPy's correlate1d for a symmetric kernel: per output, in float64 and in this order,
//                       tmp = in[l] * w[r]; for jj = -r .. -1: tmp += (in[l + jj] + in[l - jj]) * w[r + jj]; the result rounded to float32.
//                       Indices outside the axis reflect about the edges (d c b a | a b c d | d c b a), repeatedly when r >= n.  The
//                       Makefile passes -ffp-contract=off and every add and multiply is spelled __dadd_rn / __dmul_rn: no FMA.
// One lane per output element in the volume's linear order, so the lanes of a wave run along axis 2 and every load and store is
// coalesced whichever axis is filtered (neighbouring taps of axes 0 and 1 are whole rows apart, of axis 2 one element apart).  The first
// pass converts the counts, the last one writes the zero faces.  Passes: counts -> out (axis 0), out -> scratch (axis 1), scratch -> out
// (axis 2); the scratch volume of pass 1 is the count volume, which pass 0 has finished with.
#include <cmath>

#include "pb3d_internal.h"

namespace {

constexpr int kMaxGrid = 1024;               // G^3 <= 2^30: a voxel's linear index fits u32
constexpr int kMaxRadius = 64;               // int(4 * sigma + 0.5) for sigma up to 16
constexpr u32 kFloatCap = 1u << 24;          // where repeated "+ 1" stops changing a float32

template <class T>
struct Norm {
    T lo[3];        // pts.min(0)
    T denom;        // (pts.max(0) - pts.min(0)).max() + 1e-8
    T ymax;         // norm[:, 1].max() = (ymax - ymin) / denom
    T gm1;          // grid_size - 1
};

__device__ __forceinline__ float sub_rn(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ double sub_rn(double a, double b) { return __dsub_rn(a, b); }
__device__ __forceinline__ float div_rn(float a, float b) { return __fdiv_rn(a, b); }
__device__ __forceinline__ double div_rn(double a, double b) { return __ddiv_rn(a, b); }
__device__ __forceinline__ float mul_rn(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ double mul_rn(double a, double b) { return __dmul_rn(a, b); }

// voxel index along one axis: trunc(t) wrapped as NumPy wraps a negative index; -1 when t is not inside (-G, G) (NaN input)
template <class T>
__device__ __forceinline__ int wrap_index(T t, int G) {
    if (!(t > -(T)G && t < (T)G)) return -1;
    const int i = (int)t;
    return i < 0 ? i + G : i;
}

template <class T>
__global__ __launch_bounds__(256) void k_density_scatter(const T* __restrict__ pts, i64 n, Norm<T> c, int G, u32* __restrict__ counts) {
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) {
        const T* p = pts + 3 * i;
        const T nx = div_rn(sub_rn(p[0], c.lo[0]), c.denom);
        const T ny = sub_rn(div_rn(sub_rn(p[1], c.lo[1]), c.denom), c.ymax);
        const T nz = div_rn(sub_rn(p[2], c.lo[2]), c.denom);
        const int ix = wrap_index(mul_rn(nx, c.gm1), G), iy = wrap_index(mul_rn(ny, c.gm1), G), iz = wrap_index(mul_rn(nz, c.gm1), G);
        if ((ix | iy | iz) < 0) continue;
        atomicAdd(&counts[((u32)ix * (u32)G + (u32)iy) * (u32)G + (u32)iz], 1u);      // result unused: an atomic without return
    }
}

__device__ __forceinline__ double load_value(const u32* in, u32 e) {
    const u32 c = in[e];
    return (double)(c < kFloatCap ? c : kFloatCap);
}
__device__ __forceinline__ double load_value(const float* in, u32 e) { return (double)in[e]; }

// SciPy's "reflect" for any i: period 2n
__device__ __forceinline__ int reflect(int i, int n) {
    const int p = 2 * n;
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - 1 - m;
}

// AXIS 0..2: one filter pass; AXIS -1: no filter, the converted counts.  LAST: the six faces are written as 0.
template <int AXIS, bool LAST, class In>
__global__ __launch_bounds__(256) void k_density_filter(const In* __restrict__ in, float* __restrict__ out, int G, pb3d_magic mg, u32 total, int r,
                                                        const double* __restrict__ w) {
    const u32 e = blockIdx.x * 256u + threadIdx.x;
    if (e >= total) return;
    const u32 xy = pb3d_div(e, mg), x = pb3d_div(xy, mg);
    const int z = (int)(e - xy * (u32)G), y = (int)(xy - x * (u32)G);
    if (LAST) {
        const int last = G - 1;
        if (x == 0 || (int)x == last || y == 0 || y == last || z == 0 || z == last) {
            out[e] = 0.0f;
            return;
        }
    }
    if (AXIS < 0) {
        out[e] = (float)load_value(in, e);
        return;
    }
    const int l = AXIS == 0 ? (int)x : AXIS == 1 ? y : z;
    const u32 stride = AXIS == 0 ? (u32)G * (u32)G : AXIS == 1 ? (u32)G : 1u;
    const u32 base = e - (u32)l * stride;
    double tmp = __dmul_rn(load_value(in, e), w[r]);
    if (l - r >= 0 && l + r < G) {
        for (int jj = -r; jj < 0; ++jj) {
            const double a = load_value(in, base + (u32)(l + jj) * stride), b = load_value(in, base + (u32)(l - jj) * stride);
            tmp = __dadd_rn(tmp, __dmul_rn(__dadd_rn(a, b), w[r + jj]));
        }
    } else {
        for (int jj = -r; jj < 0; ++jj) {
            const double a = load_value(in, base + (u32)reflect(l + jj, G) * stride), b = load_value(in, base + (u32)reflect(l - jj, G) * stride);
            tmp = __dadd_rn(tmp, __dmul_rn(__dadd_rn(a, b), w[r + jj]));
        }
    }
    out[e] = __double2float_rn(tmp);
}

template <int AXIS, bool LAST, class In>
int launch_filter(pb3d_ctx* ctx, const In* in, float* out, int G, int r, const double* w) {
    const u32 total = (u32)G * (u32)G * (u32)G;
    hipLaunchKernelGGL((k_density_filter<AXIS, LAST, In>), dim3((total + 255u) / 256u), dim3(256), 0, ctx->stream, in, out, G,
                       pb3d_make_magic((u32)G), total, r, w);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

// the constants of the normalisation in the point dtype, from the exact bounds (float32 bounds are exact in the doubles that carry them)
template <class T>
Norm<T> make_norm(const double b[6], int G) {
    Norm<T> c;
    T scale = (T)0;
    for (int k = 0; k < 3; ++k) {
        c.lo[k] = (T)b[k];
        const T size = (T)b[3 + k] - (T)b[k];
        if (k == 0 || size > scale) scale = size;
    }
    c.denom = scale + (T)1e-8;
    c.ymax = ((T)b[4] - (T)b[1]) / c.denom;
    c.gm1 = (T)(G - 1);
    return c;
}

template <class T>
int launch_scatter(pb3d_ctx* ctx, const void* d_pts, i64 n, const double b[6], int G, u32* counts) {
    hipLaunchKernelGGL(k_density_scatter<T>, dim3(pb3d_stream_blocks(ctx, n, 256, 8)), dim3(256), 0, ctx->stream, (const T*)d_pts, n,
                       make_norm<T>(b, G), G, counts);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

}  // namespace

extern "C" int pb3d_density_grid_resident(pb3d_ctx* ctx, const void* d_pts, int pts_f64, int64_t n, int grid_size, const double* weights,
                                          int radius, float* d_out) {
    PB3D_REQUIRE(grid_size >= 1 && grid_size <= kMaxGrid, "pb3d_density_grid: grid_size must be in [1, %d] (got %d)", kMaxGrid, grid_size);
    PB3D_REQUIRE(radius >= 0 && radius <= kMaxRadius, "pb3d_density_grid: the filter radius must be in [0, %d] (got %d)", kMaxRadius, radius);
    PB3D_REQUIRE(n >= 1 && n <= pb3d_max_points, "pb3d_density_grid: need 1 <= n <= 2^31 - 1 points (got %lld)", (long long)n);
    PB3D_REQUIRE(d_pts != nullptr && d_out != nullptr && (radius == 0 || weights != nullptr), "pb3d_density_grid: null buffer");
    PB3D_REQUIRE(ctx != nullptr, "pb3d_density_grid: null context");

    const int G = grid_size;
    const size_t vol_bytes = (size_t)G * G * G * sizeof(u32);
    void *vol, *wtab;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_DENSITY_COUNTS, vol_bytes, &vol));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_DENSITY_WEIGHTS, (size_t)(kMaxRadius + 1) * sizeof(double), &wtab));
    // in front of the box, so that it is done under the box's host wait and not after it.  The bounds kernel right behind the fill runs
    // some 6 us longer than behind anything else (53 -> 59 us on 12 M points, profiles/onecopy_bounds_after_fill.txt)
    PB3D_HIP(hipMemsetAsync(vol, 0, vol_bytes, ctx->stream));
    double b[6];
    PB3D_TRY(pb3d_points_box(ctx, d_pts, pts_f64, n, PB3D_SLOT_DENSITY_BOUNDS, b));
    for (int k = 0; k < 6; ++k)
        PB3D_REQUIRE(std::isfinite(b[k]), "pb3d_density_grid: the points' bounds are not finite (NaN or infinite coordinates)");

    u32* counts = (u32*)vol;
    if (pts_f64) PB3D_TRY(launch_scatter<double>(ctx, d_pts, n, b, G, counts));
    else PB3D_TRY(launch_scatter<float>(ctx, d_pts, n, b, G, counts));
    if (radius == 0) return launch_filter<-1, true>(ctx, (const u32*)counts, d_out, G, 0, (const double*)nullptr);
    // w[0 .. r] is all a symmetric kernel needs: the pass reads w[r + jj] for jj = -r .. 0
    PB3D_TRY(pb3d_h2d_async(ctx, wtab, weights, (size_t)(radius + 1) * sizeof(double)));
    float* tmp = (float*)vol;
    PB3D_TRY((launch_filter<0, false>(ctx, (const u32*)counts, d_out, G, radius, (const double*)wtab)));
    PB3D_TRY((launch_filter<1, false>(ctx, (const float*)d_out, tmp, G, radius, (const double*)wtab)));
    return launch_filter<2, true>(ctx, (const float*)tmp, d_out, G, radius, (const double*)wtab);
}
