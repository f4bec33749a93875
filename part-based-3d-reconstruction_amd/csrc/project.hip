// K7 pinhole scatter projection (deterministic last-writer-wins) and K8 per-part IoU counts.
//
// reference utils/projection_utils.py:5-23:  pc = (p - cam) @ R.T ; Z<1e-8 -> 1e-8 ;
//   u = (X/Z)*f + cx ; v = -(Y/Z)*f + cy ; rint ; bounds ; img[v,u] = colour.
// NumPy's fancy assignment resolves duplicate pixels by "last in input order wins"; that is
// reproduced with an atomicMax on (point index + 1) per pixel followed by a resolve pass, so the
// image is identical from run to run and to the CPU path.
// Arithmetic: each component of pc is the FMA chain fma(d2,r2, fma(d1,r1, d0*r0)) NumPy's gemm
// produces (float32 or float64 per prec[0]); the later stages are separate IEEE ops whose width is
// prec[1..3].  float32 +,-,*,/ are evaluated in double and rounded once (exact since 53 >= 2*24+2);
// the float32 FMA chain uses the hardware's single-rounded v_fma_f32.
#include "pb3d_internal.h"
#include "project_point.h"

namespace {

using namespace pb3d_proj;

__global__ __launch_bounds__(256) void k_project_resolve(const u32* __restrict__ winner, const u8* __restrict__ cols,
                                                         u8* __restrict__ img, i64 npix) {
    for (i64 px = (i64)blockIdx.x * blockDim.x + threadIdx.x; px < npix; px += (i64)gridDim.x * blockDim.x) {
        const u32 w = winner[px];
        u8 r = 0, g = 0, b = 0;
        if (w) {
            const u8* c = cols + (i64)(w - 1) * 3;
            r = c[0]; g = c[1]; b = c[2];
        }
        img[3 * px] = r; img[3 * px + 1] = g; img[3 * px + 2] = b;
    }
}

__global__ __launch_bounds__(256) void k_resolve_keys(const unsigned long long* __restrict__ keys, u8* __restrict__ img, i64 npix) {
    for (i64 px = (i64)blockIdx.x * blockDim.x + threadIdx.x; px < npix; px += (i64)gridDim.x * blockDim.x) {
        const unsigned long long k = keys[px];
        img[3 * px] = (u8)(k & 0xff); img[3 * px + 1] = (u8)((k >> 8) & 0xff); img[3 * px + 2] = (u8)((k >> 16) & 0xff);
    }
}

// ------------------------------------------------------------------------------------------------
// Sinks: what a projected point does to its pixel, one per operation, shared by the generic kernel (one point at a time,
// i64 pixel index) and the float32 kernel (groups of four, u32 pixel index).
//   peek(ok, px)               the plain load of the pixel's current value; for a point that missed the image (!ok) a
//                              value that makes commit do nothing
//   commit(ok, cur, i, px, z)  the conditional atomic or store of point i (depth z) given what peek saw
// MODE is the projection rule (project_xyz / project_f32); REVERSE visits the point list last-first.
// ------------------------------------------------------------------------------------------------

// Last writer wins: an atomicMax of (i + 1) per pixel.  Points are visited from the LAST index down: the winner of a pixel
// is its largest point index, so once the high indices have claimed their pixels the remaining points mostly lose on the
// plain read and skip the atomic.
struct WinnerSink {
    static constexpr int MODE = 0;
    static constexpr bool REVERSE = true;
    u32* __restrict__ winner;
    __device__ __forceinline__ void shift(i64 off) { winner += off; }
    template <class I>
    __device__ __forceinline__ u32 peek(bool ok, I px) const {
        return ok ? __hip_atomic_load(&winner[px], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0xffffffffu;
    }
    template <class I, class Z>
    __device__ __forceinline__ void commit(bool, u32 cur, i64 i, I px, Z) const {
        if (cur < (u32)(i + 1)) atomicMax(&winner[px], (u32)(i + 1));
    }
};

// Sharded form of the scatter (points partition): every rank projects its contiguous range of the
// point list into a private image of 64-bit keys ((global index + 1) << 24 | b << 16 | g << 8 | r); the last-writer-wins
// rule is a max over the key, so ONE all-reduce(max) over the ranks followed by a local resolve gives every rank the
// image the unsharded call produces, with no colour look-up across ranks.  Indices are distinct, so the index part decides.
struct KeySink {
    static constexpr int MODE = 0;
    static constexpr bool REVERSE = true;
    const u8* __restrict__ cols;
    i64 index_base;
    unsigned long long* __restrict__ keys;
    template <class I>
    __device__ __forceinline__ unsigned long long peek(bool ok, I px) const {
        return ok ? __hip_atomic_load(&keys[px], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : ~0ull;
    }
    template <class I, class Z>
    __device__ __forceinline__ void commit(bool, unsigned long long cur, i64 i, I px, Z) const {
        const unsigned long long mine = (unsigned long long)(index_base + i + 1) << 24;      // the colour bits are read only to store
        if (cur < mine)
            atomicMax(&keys[px], mine | ((unsigned long long)cols[3 * i + 2] << 16) | ((unsigned long long)cols[3 * i + 1] << 8) | (unsigned long long)cols[3 * i]);
    }
};

// z-buffer: nearest depth per pixel.  Depths are positive, so float32 order == order of their bit patterns and
// the sequential "if z < zbuf: zbuf = z" loop of the reference equals an atomicMin on the float32 bits of z
// (for float64 cameras the stored value is float32(z); float32 rounding is monotone, so min and rounding commute).
struct DepthSink {
    static constexpr int MODE = 1;
    static constexpr bool REVERSE = false;
    u32* __restrict__ zbits;
    template <class I>
    __device__ __forceinline__ u32 peek(bool ok, I px) const {
        return ok ? __hip_atomic_load(&zbits[px], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    }
    template <class I, class Z>
    __device__ __forceinline__ void commit(bool, u32 cur, i64, I px, Z z) const {
        if (cur > __float_as_uint((float)z)) atomicMin(&zbits[px], __float_as_uint((float)z));
    }
};

// visible where |z - zbuf| < eps (visible(), project_point.h).  Only the generic kernel, whose z is a double, sees a float64 camera
// (t0); a float32 z widened and narrowed again is itself.
struct VisibleSink {
    static constexpr int MODE = 1;
    static constexpr bool REVERSE = false;
    const float* __restrict__ zbuf;
    double eps;
    int eps_f32, t0;
    u8* __restrict__ mask;
    template <class I>
    __device__ __forceinline__ float peek(bool ok, I px) const { return ok ? zbuf[px] : 0.0f; }
    template <class I, class Z>
    __device__ __forceinline__ void commit(bool ok, float zb, i64, I px, Z z) const {
        if (ok && visible((double)z, zb, sizeof(Z) == sizeof(double) && t0, eps, eps_f32)) mask[px] = 1;
    }
};

// The camera of a launch: ONE camera travels by value in the kernel arguments; a batch of K cameras (grid y = K) reads
// cams[blockIdx.y] and moves the sink to that camera's image, blockIdx.y * npix further on.
template <class T>
struct CamBatch {
    const T* cams;
    i64 npix;
};
template <class T, class Sink>
__device__ __forceinline__ T camera(const T& P, Sink&) { return P; }
template <class T, class Sink>
__device__ __forceinline__ T camera(const CamBatch<T>& B, Sink& sink) {
    sink.shift((i64)blockIdx.y * B.npix);
    return B.cams[blockIdx.y];
}

// generic path: any precision combination, one point per thread
template <class Cam, class Sink>
__global__ __launch_bounds__(256) void k_project(const void* __restrict__ pts, i64 n, Cam cam, Sink sink) {
    const ProjParams P = camera(cam, sink);
    for (i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (i64)gridDim.x * blockDim.x) {
        const i64 i = Sink::REVERSE ? n - 1 - t : t;
        int ui, vi;
        double z = 0.0;
        if (project_point<Sink::MODE>(P, pts, i, &ui, &vi, &z)) {
            const i64 px = (i64)vi * P.Wimg + ui;
            sink.commit(true, sink.peek(true, px), i, px, z);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// All-float32 fast path (float32 points, float32 camera: prec = {0,0,0,0} -- what notebooks 2/3 pass).
// Every stage of project_point is then one IEEE float32 operation, so it is evaluated directly in
// float32 (v_fma_f32 chains, correctly rounded v_div sequence) instead of "double, rounded once":
// ~3x fewer VALU cycles, which is what bounded the generic kernel.  Points are read four at a time as
// three 16-byte loads per lane.
// ------------------------------------------------------------------------------------------------
struct ProjF32 {
    float R[9], cam[3], f, cx, cy;
    int Himg, Wimg;
};
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int MODE>
__device__ __forceinline__ bool project_f32(const ProjF32& P, float x, float y, float z, int* ui, int* vi, float* zout) {
    const float d0 = __fsub_rn(x, P.cam[0]), d1 = __fsub_rn(y, P.cam[1]), d2 = __fsub_rn(z, P.cam[2]);
    float pc[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) pc[r] = __fmaf_rn(d2, P.R[3 * r + 2], __fmaf_rn(d1, P.R[3 * r + 1], __fmul_rn(d0, P.R[3 * r])));
    float Z = pc[2];
    if (MODE == 0) {
        if (Z < 1e-8f) Z = 1e-8f;
    } else {
        if (!(Z > 1e-6f)) return false;
        *zout = Z;
    }
    const float qx = __fdiv_rn(pc[0], Z), qy = -__fdiv_rn(pc[1], Z);
    const float u = __fadd_rn(__fmul_rn(qx, P.f), P.cx), v = __fadd_rn(__fmul_rn(qy, P.f), P.cy);
    // 0 <= r < n as ONE unsigned compare of float bit patterns: for r >= +0 the patterns order like the values, negative
    // values / NaN / inf have patterns above every finite n; "+ 0.0f" turns the legitimate -0.0 (u in [-0.5, -0]) into +0.0
    const float ur = __fadd_rn(rintf(u), 0.0f), vr = __fadd_rn(rintf(v), 0.0f);
    if (!(__float_as_uint(ur) < __float_as_uint((float)P.Wimg) && __float_as_uint(vr) < __float_as_uint((float)P.Himg))) return false;
    *ui = (int)ur; *vi = (int)vr;
    return true;
}

// One group of four points (i0 = index of the group's first point): the four projections are finished and all four
// pixels peeked before the first commit, so the four dependent image reads / atomics are issued back to back instead of
// one L2 round trip after another.  Commits go in visiting order (k = 3..0 in a reverse sweep).
template <class Sink>
__device__ __forceinline__ void group_f32(const ProjF32& P, const float q[12], int live, i64 i0, const Sink& sink) {
    bool ok[4]; u32 px[4]; float z[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int ui = 0, vi = 0;
        z[k] = 0.0f;
        ok[k] = k < live && project_f32<Sink::MODE>(P, q[3 * k], q[3 * k + 1], q[3 * k + 2], &ui, &vi, &z[k]);
        px[k] = (u32)vi * (u32)P.Wimg + (u32)ui;
    }
    decltype(sink.peek(true, px[0])) cur[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) cur[k] = sink.peek(ok[k], px[k]);
    if (Sink::REVERSE) {
#pragma unroll
        for (int k = 3; k >= 0; --k) sink.commit(ok[k], cur[k], i0 + k, px[k], z[k]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) sink.commit(ok[k], cur[k], i0 + k, px[k], z[k]);
    }
}

template <class Sink>
__device__ __forceinline__ void sweep_f32(const float* __restrict__ pts, i64 n, const ProjF32& P, bool vec, const Sink& sink) {
    constexpr bool REVERSE = Sink::REVERSE;
    const i64 nfull = n >> 2;                      // groups of four whole points
    const i64 gtid = (i64)blockIdx.x * blockDim.x + threadIdx.x, gsz = (i64)gridDim.x * blockDim.x;
    float q[12];
    if (REVERSE && gtid == 0 && (n & 3)) {        // the ragged tail holds the highest indices: first in a reverse sweep
#pragma unroll
        for (int k = 0; k < 12; ++k) q[k] = k < 3 * (int)(n & 3) ? pts[12 * nfull + k] : 0.0f;
        group_f32(P, q, (int)(n & 3), 4 * nfull, sink);
    }
    if (vec) {
        // the next group's three vectors are requested before this group is projected (software prefetch)
        f32x4 nx[3];
        auto fetch = [&](i64 t) {
            const i64 c = REVERSE ? nfull - 1 - t : t;
            const f32x4* g = (const f32x4*)(pts + 12 * c);
#pragma unroll
            for (int k = 0; k < 3; ++k) nx[k] = g[k];   // plain loads: each 128-byte line is shared by three instructions (nontemporal: 1.4x slower)
        };
        if (gtid < nfull) fetch(gtid);
        for (i64 t = gtid; t < nfull; t += gsz) {
            const i64 c = REVERSE ? nfull - 1 - t : t;
#pragma unroll
            for (int k = 0; k < 3; ++k) { q[4 * k] = nx[k].x; q[4 * k + 1] = nx[k].y; q[4 * k + 2] = nx[k].z; q[4 * k + 3] = nx[k].w; }
            if (t + gsz < nfull) fetch(t + gsz);
            group_f32(P, q, 4, 4 * c, sink);
        }
    } else {
        for (i64 t = gtid; t < nfull; t += gsz) {
            const i64 c = REVERSE ? nfull - 1 - t : t;
#pragma unroll
            for (int k = 0; k < 12; ++k) q[k] = pts[12 * c + k];
            group_f32(P, q, 4, 4 * c, sink);
        }
    }
    if (!REVERSE && gtid == 0 && (n & 3)) {
#pragma unroll
        for (int k = 0; k < 12; ++k) q[k] = k < 3 * (int)(n & 3) ? pts[12 * nfull + k] : 0.0f;
        group_f32(P, q, (int)(n & 3), 4 * nfull, sink);
    }
}

template <class Cam, class Sink>
__global__ __launch_bounds__(256) void k_project_f32(const float* __restrict__ pts, i64 n, Cam cam, int vec, Sink sink) {
    const ProjF32 P = camera(cam, sink);
    sweep_f32(pts, n, P, vec != 0, sink);
}

// the fast path applies when nothing in the call is float64
bool f32_path(const ProjParams& P, ProjF32* F) {
    if (P.pts_f64 || P.t0 || P.tm || P.tu || P.tv || P.Himg >= (1 << 24) || P.Wimg >= (1 << 24) || (i64)P.Himg * P.Wimg > 0xffffffffll) return false;
    for (int k = 0; k < 9; ++k) F->R[k] = (float)P.R[k];
    for (int k = 0; k < 3; ++k) F->cam[k] = (float)P.cam[k];
    F->f = (float)P.f; F->cx = (float)P.cx; F->cy = (float)P.cy;
    F->Himg = P.Himg; F->Wimg = P.Wimg;
    return true;
}
inline int vec_ok(const void* p) { return (((uintptr_t)p) & 15u) == 0; }
inline unsigned f32_blocks(pb3d_ctx* ctx, i64 n) { return pb3d_stream_blocks(ctx, n / 4 + 1, 256, 0); }      // one workgroup per 1024 points

// scatter the n points of one camera into the sink's image: the float32 kernel when f32_path accepts P, else the generic one
template <class Sink>
int project_scatter(pb3d_ctx* ctx, const void* d_pts, i64 n, const ProjParams& P, const Sink& sink) {
    if (n == 0) return PB3D_OK;
    ProjF32 F;
    if (f32_path(P, &F))
        hipLaunchKernelGGL((k_project_f32<ProjF32, Sink>), dim3(f32_blocks(ctx, n)), dim3(256), 0, ctx->stream, (const float*)d_pts, n, F,
                           vec_ok(d_pts), sink);
    else
        hipLaunchKernelGGL((k_project<ProjParams, Sink>), dim3(pb3d_stream_blocks(ctx, n, 256, 8)), dim3(256), 0, ctx->stream, d_pts, n, P, sink);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

// Per-colour intersection / union pixel counts of image a against the RGB image b: colour_a(px, c) writes pixel px's
// colour in a to c[0..2].  One ballot per colour and wave; lane 0 adds the popcounts to the block's LDS tally (acc[2k] =
// intersection, acc[2k + 1] = union) and the block adds its tally to counts[0 .. 2 * ncolors) once.
template <class ColourA>
__device__ __forceinline__ void iou_counts(ColourA colour_a, const u8* __restrict__ b, i64 npix, int ncolors, const u8* colors,
                                           unsigned long long* __restrict__ counts) {
    __shared__ u32 acc[64];
    if (threadIdx.x < 64) acc[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const i64 stride = (i64)gridDim.x * blockDim.x;
    const i64 nloop = (npix + stride - 1) / stride;  // same trip count for every lane: ballots stay convergent
    for (i64 it = 0; it < nloop; ++it) {
        const i64 px = it * stride + (i64)blockIdx.x * blockDim.x + threadIdx.x;
        const bool live = px < npix;
        u8 a[3] = {0, 0, 0}, b0 = 0, b1 = 0, b2 = 0;
        if (live) {
            colour_a(px, a);
            b0 = b[3 * px]; b1 = b[3 * px + 1]; b2 = b[3 * px + 2];
        }
        for (int k = 0; k < ncolors; ++k) {
            const u8 c0 = colors[3 * k], c1 = colors[3 * k + 1], c2 = colors[3 * k + 2];
            const bool ma = live && a[0] == c0 && a[1] == c1 && a[2] == c2;
            const bool mb = live && b0 == c0 && b1 == c1 && b2 == c2;
            const u32 ni = (u32)__popcll(__ballot(ma && mb)), nu = (u32)__popcll(__ballot(ma || mb));
            if (lane == 0) {
                if (ni) atomicAdd(&acc[2 * k], ni);
                if (nu) atomicAdd(&acc[2 * k + 1], nu);
            }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < 2 * ncolors && acc[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)acc[threadIdx.x]);
}

struct IouParams {
    int ncolors;
    u8 colors[3 * 32];
};

__global__ __launch_bounds__(256) void k_partwise_iou(const u8* __restrict__ a, const u8* __restrict__ b, i64 npix,
                                                      IouParams P, unsigned long long* __restrict__ counts) {
    iou_counts([&](i64 px, u8 c[3]) { c[0] = a[3 * px]; c[1] = a[3 * px + 1]; c[2] = a[3 * px + 2]; }, b, npix, P.ncolors, P.colors, counts);
}


// ------------------------------------------------------------------------------------------------
// Row N4: K cameras per launch.  The camera aligner (reference utils/camera_estimation.py:597-603 `evaluate`, driven by the
// random / coordinate / Powell loops :606-725) re-projects the SAME resident points for every candidate camera and keeps only
// the per-part IoU against the part image.  One launch projects all K cameras (blockIdx.y = camera; private winner image per
// camera), a second one resolves every camera's winners to colours on the fly and counts intersections / unions against the
// part image -- the K projected images are never written -- and ONE copy brings the K x P counters back.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_iou_winners_batch(const u32* __restrict__ winners, const u8* __restrict__ cols, const u8* __restrict__ seg,
                                                           i64 npix, int ncolors, const u8* __restrict__ colors, unsigned long long* __restrict__ counts) {
    __shared__ u8 cl[96];                          // written before iou_counts' first barrier
    if (threadIdx.x < 96) cl[threadIdx.x] = (int)threadIdx.x < 3 * ncolors ? colors[threadIdx.x] : (u8)0;
    const u32* winner = winners + (i64)blockIdx.y * npix;
    iou_counts([&](i64 px, u8 c[3]) {
                   const u32 w = winner[px];
                   if (w) { const u8* s = cols + (i64)(w - 1) * 3; c[0] = s[0]; c[1] = s[1]; c[2] = s[2]; }
               },
               seg, npix, ncolors, cl, counts + (i64)blockIdx.y * 64);
}

}  // namespace

extern "C" {

int pb3d_project_dev(pb3d_ctx* ctx, const void* d_pts, int pts_f64, const uint8_t* d_cols, int64_t n,
                     const double R[9], const double cam[3], double f, double cx, double cy, const int prec[4],
                     int Himg, int Wimg, uint8_t* d_img) {
    PB3D_REQUIRE(ctx && R && cam && prec, "pb3d_project: null argument");
    PB3D_REQUIRE(n >= 0 && n < 0xffffffffll, "pb3d_project: point count out of range");
    PB3D_REQUIRE(Himg >= 0 && Wimg >= 0, "pb3d_project: bad image shape");
    const i64 npix = (i64)Himg * Wimg;
    if (npix == 0) return PB3D_OK;
    PB3D_REQUIRE(d_img && (n == 0 || (d_pts && d_cols)), "pb3d_project: null buffer");
    ProjParams P;
    PB3D_TRY(fill_proj(&P, pts_f64, R, cam, f, cx, cy, prec, Himg, Wimg));
    void* winner;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_PROJ_WINNER, (size_t)npix * sizeof(u32), &winner));
    PB3D_HIP(hipMemsetAsync(winner, 0, (size_t)npix * sizeof(u32), ctx->stream));
    PB3D_TRY(project_scatter(ctx, d_pts, n, P, WinnerSink{(u32*)winner}));
    hipLaunchKernelGGL(k_project_resolve, dim3(pb3d_stream_blocks(ctx, npix, 256, 8)), dim3(256), 0, ctx->stream,
                       (const u32*)winner, d_cols, d_img, npix);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

int pb3d_project_keys_dev(pb3d_ctx* ctx, const void* d_pts, int pts_f64, const uint8_t* d_cols, int64_t n, int64_t index_base,
                          const double R[9], const double cam[3], double f, double cx, double cy, const int prec[4], int Himg, int Wimg,
                          uint64_t* d_keys) {
    PB3D_REQUIRE(ctx && R && cam && prec && n >= 0 && index_base >= 0 && Himg >= 0 && Wimg >= 0, "pb3d_project_keys: bad argument");
    PB3D_REQUIRE(index_base + n < (1ll << 39), "pb3d_project_keys: point index does not fit the key");
    const i64 npix = (i64)Himg * Wimg;
    if (npix == 0) return PB3D_OK;
    PB3D_REQUIRE(d_keys && (n == 0 || (d_pts && d_cols)), "pb3d_project_keys: null buffer");
    ProjParams P;
    PB3D_TRY(fill_proj(&P, pts_f64, R, cam, f, cx, cy, prec, Himg, Wimg));
    PB3D_HIP(hipMemsetAsync(d_keys, 0, (size_t)npix * sizeof(uint64_t), ctx->stream));
    return project_scatter(ctx, d_pts, n, P, KeySink{d_cols, index_base, (unsigned long long*)d_keys});
}

int pb3d_project_resolve_keys_dev(pb3d_ctx* ctx, const uint64_t* d_keys, int Himg, int Wimg, uint8_t* d_img) {
    PB3D_REQUIRE(ctx && Himg >= 0 && Wimg >= 0, "pb3d_project_resolve_keys: bad argument");
    const i64 npix = (i64)Himg * Wimg;
    if (npix == 0) return PB3D_OK;
    PB3D_REQUIRE(d_keys && d_img, "pb3d_project_resolve_keys: null buffer");
    hipLaunchKernelGGL(k_resolve_keys, dim3(pb3d_stream_blocks(ctx, npix, 256, 8)), dim3(256), 0, ctx->stream,
                       (const unsigned long long*)d_keys, d_img, npix);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

int pb3d_depth_buffer_dev(pb3d_ctx* ctx, const void* d_pts, int pts_f64, int64_t n, const double R[9], const double cam[3], double f,
                          double cx, double cy, const int prec[4], int Himg, int Wimg, float* d_zbuf) {
    PB3D_REQUIRE(ctx && R && cam && prec && n >= 0 && Himg >= 0 && Wimg >= 0, "pb3d_depth_buffer: bad argument");
    const i64 npix = (i64)Himg * Wimg;
    if (npix == 0) return PB3D_OK;
    PB3D_REQUIRE(d_zbuf && (n == 0 || d_pts), "pb3d_depth_buffer: null buffer");
    ProjParams P;
    PB3D_TRY(fill_proj(&P, pts_f64, R, cam, f, cx, cy, prec, Himg, Wimg));
    PB3D_HIP(hipMemsetD32Async((hipDeviceptr_t)d_zbuf, 0x7f800000, (size_t)npix, ctx->stream));   // +inf
    return project_scatter(ctx, d_pts, n, P, DepthSink{(u32*)d_zbuf});
}

int pb3d_visible_mask_dev(pb3d_ctx* ctx, const void* d_pts, int pts_f64, int64_t n, const double R[9], const double cam[3], double f,
                          double cx, double cy, const int prec[4], const float* d_zbuf, int Himg, int Wimg, double eps, int eps_f32,
                          uint8_t* d_mask) {
    PB3D_REQUIRE(ctx && R && cam && prec && n >= 0 && Himg >= 0 && Wimg >= 0, "pb3d_visible_mask: bad argument");
    const i64 npix = (i64)Himg * Wimg;
    if (npix == 0) return PB3D_OK;
    PB3D_REQUIRE(d_zbuf && d_mask && (n == 0 || d_pts), "pb3d_visible_mask: null buffer");
    ProjParams P;
    PB3D_TRY(fill_proj(&P, pts_f64, R, cam, f, cx, cy, prec, Himg, Wimg));
    PB3D_HIP(hipMemsetAsync(d_mask, 0, (size_t)npix, ctx->stream));
    return project_scatter(ctx, d_pts, n, P, VisibleSink{d_zbuf, eps, eps_f32, P.t0, d_mask});
}

int pb3d_partwise_iou_dev(pb3d_ctx* ctx, const uint8_t* d_a, const uint8_t* d_b, int64_t npix,
                          const uint8_t* colors, int ncolors, int64_t* inter, int64_t* uni) {
    PB3D_REQUIRE(ctx && inter && uni, "pb3d_partwise_iou: null argument");
    PB3D_REQUIRE(ncolors >= 0 && ncolors <= 32 && npix >= 0, "pb3d_partwise_iou: bad sizes");
    for (int k = 0; k < ncolors; ++k) inter[k] = uni[k] = 0;
    if (ncolors == 0 || npix == 0) return PB3D_OK;
    PB3D_REQUIRE(d_a && d_b && colors, "pb3d_partwise_iou: null buffer");
    void* counts;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_IOU_COUNTS, 64 * sizeof(unsigned long long), &counts));
    PB3D_HIP(hipMemsetAsync(counts, 0, 64 * sizeof(unsigned long long), ctx->stream));
    IouParams P;
    P.ncolors = ncolors;
    memset(P.colors, 0, sizeof(P.colors));
    memcpy(P.colors, colors, (size_t)3 * ncolors);
    hipLaunchKernelGGL(k_partwise_iou, dim3(pb3d_stream_blocks(ctx, npix, 256, 4)), dim3(256), 0, ctx->stream, d_a, d_b, npix, P,
                       (unsigned long long*)counts);
    PB3D_CHECK_LAUNCH();
    unsigned long long h[64];
    PB3D_TRY(pb3d_read_back(ctx, h, counts, sizeof(h)));
    for (int k = 0; k < ncolors; ++k) { inter[k] = (int64_t)h[2 * k]; uni[k] = (int64_t)h[2 * k + 1]; }
    return PB3D_OK;
}


int pb3d_project_iou_batch_dev(pb3d_ctx* ctx, const void* d_pts, int pts_f64, const uint8_t* d_cols, int64_t n, const pb3d_camera* cams, int ncams,
                               int Himg, int Wimg, const uint8_t* d_seg, const uint8_t* colors, int ncolors, int64_t* inter, int64_t* uni) {
    PB3D_REQUIRE(ctx && (ncams == 0 || (cams && inter && uni)), "pb3d_project_iou_batch: null argument");
    PB3D_REQUIRE(ncams >= 0 && n >= 0 && n < 0xffffffffll && Himg >= 0 && Wimg >= 0, "pb3d_project_iou_batch: bad sizes");
    PB3D_REQUIRE(ncolors >= 0 && ncolors <= 32, "pb3d_project_iou_batch: at most 32 colours");
    for (i64 k = 0; k < (i64)ncams * ncolors; ++k) inter[k] = uni[k] = 0;
    const i64 npix = (i64)Himg * Wimg;
    if (ncams == 0 || ncolors == 0 || npix == 0) return PB3D_OK;
    PB3D_REQUIRE(d_seg && colors && (n == 0 || (d_pts && d_cols)), "pb3d_project_iou_batch: null buffer");
    // cameras per pass: winner images of one pass stay below 512 MiB, the grid's y dimension below 65536
    i64 kc = (512ll << 20) / (npix * (i64)sizeof(u32));
    kc = kc < 1 ? 1 : (kc > 4096 ? 4096 : kc);
    if (kc > ncams) kc = ncams;
    void *winners, *dcams, *counts, *dcolors;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_PROJ_WINNER, (size_t)(kc * npix) * sizeof(u32), &winners));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_PROJ_BATCH_CAMS, (size_t)kc * sizeof(ProjParams), &dcams));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_PROJ_BATCH_COUNTS, (size_t)kc * 64 * sizeof(unsigned long long), &counts));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_PROJ_BATCH_COLORS, 128, &dcolors));
    PB3D_HIP(hipMemcpyAsync(dcolors, colors, (size_t)3 * ncolors, hipMemcpyHostToDevice, ctx->stream));
    ProjParams* hp = (ProjParams*)malloc((size_t)kc * sizeof(ProjParams));
    ProjF32* hf = (ProjF32*)malloc((size_t)kc * sizeof(ProjF32));
    unsigned long long* hc = (unsigned long long*)malloc((size_t)kc * 64 * sizeof(unsigned long long));
    if (!hp || !hf || !hc) { free(hp); free(hf); free(hc); pb3d_set_error("pb3d_project_iou_batch: out of host memory"); return PB3D_ENOMEM; }
    int rc = PB3D_OK;
    for (i64 k0 = 0; k0 < ncams && rc == PB3D_OK; k0 += kc) {
        const i64 kn = ncams - k0 < kc ? ncams - k0 : kc;
        bool all_f32 = true;                             // the float32 kernel runs a pass only when it takes every camera of it
        for (i64 k = 0; k < kn && rc == PB3D_OK; ++k) {
            const pb3d_camera* c = cams + k0 + k;
            rc = fill_proj(&hp[k], pts_f64, c->R, c->cam, c->f, c->cx, c->cy, c->prec, Himg, Wimg);
            if (rc == PB3D_OK && !f32_path(hp[k], &hf[k])) all_f32 = false;
        }
        if (rc != PB3D_OK) break;
        auto hipok = [&](hipError_t e, const char* what) {
            if (e != hipSuccess && rc == PB3D_OK) { pb3d_set_error("%s failed: %s", what, hipGetErrorString(e)); rc = PB3D_ENODEVICE; }
        };
        hipok(hipMemcpyAsync(dcams, all_f32 ? (const void*)hf : (const void*)hp, (size_t)kn * (all_f32 ? sizeof(ProjF32) : sizeof(ProjParams)),
                             hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync");
        hipok(hipMemsetAsync(winners, 0, (size_t)(kn * npix) * sizeof(u32), ctx->stream), "hipMemsetAsync");
        hipok(hipMemsetAsync(counts, 0, (size_t)kn * 64 * sizeof(unsigned long long), ctx->stream), "hipMemsetAsync");
        if (rc != PB3D_OK) break;
        if (n > 0) {
            // enough blocks per camera to fill the chip between them, never more than the points need
            if (all_f32)
                hipLaunchKernelGGL((k_project_f32<CamBatch<ProjF32>, WinnerSink>), dim3(pb3d_batch_blocks(ctx, n / 4 + 1, 256, kn, 16), (unsigned)kn),
                                   dim3(256), 0, ctx->stream, (const float*)d_pts, n, CamBatch<ProjF32>{(const ProjF32*)dcams, npix}, vec_ok(d_pts),
                                   WinnerSink{(u32*)winners});
            else
                hipLaunchKernelGGL((k_project<CamBatch<ProjParams>, WinnerSink>), dim3(pb3d_batch_blocks(ctx, n, 256, kn, 16), (unsigned)kn), dim3(256),
                                   0, ctx->stream, d_pts, n, CamBatch<ProjParams>{(const ProjParams*)dcams, npix}, WinnerSink{(u32*)winners});
            hipok(hipGetLastError(), "k_project batch");
        }
        hipLaunchKernelGGL(k_iou_winners_batch, dim3(pb3d_batch_blocks(ctx, npix, 256, kn, 8), (unsigned)kn), dim3(256), 0, ctx->stream,
                           (const u32*)winners, d_cols, d_seg, npix, ncolors, (const u8*)dcolors, (unsigned long long*)counts);
        hipok(hipGetLastError(), "k_iou_winners_batch");
        hipok(hipMemcpyAsync(hc, counts, (size_t)kn * 64 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync");
        ++ctx->sync_count; hipok(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
        if (rc != PB3D_OK) break;
        for (i64 k = 0; k < kn; ++k)
            for (int c = 0; c < ncolors; ++c) {
                inter[(k0 + k) * ncolors + c] = (int64_t)hc[k * 64 + 2 * c];
                uni[(k0 + k) * ncolors + c] = (int64_t)hc[k * 64 + 2 * c + 1];
            }
    }
    free(hp); free(hf); free(hc);
    return rc;
}

}  // extern "C"
