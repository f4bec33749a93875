// render_mesh: depth, face and barycentric images of a triangle mesh under a pinhole camera, and the shading pass on top of them
// (include/pb3d.h has the rule to the bit; DESIGN.md "Mesh to image" has the passes and their times).
//
//   k_render_setup    one sweep: the face indices against [-nv, nv) (bit 0 of the flag), and per vertex the finiteness of its coordinates
//                     (bit 1) and its camera coordinates (X, Y, Z), 24 bytes in PB3D_SLOT_RENDER_CAMERA.  Nothing gathers through an index
//                     before the host has read the flag: the entry's first host wait
//   k_render_faces    one lane per face: the pruning rules and the conservative pixel box.  A face whose box holds at most kLanePixels
//                     pixels (every face of a marching-cubes mesh at the usual image sizes) is walked by its lane; any other face is
//                     counted as (x1/8 - x0/8 + 1) * (y1/8 - y0/8 + 1) tile jobs, pb3d_scan_counts turns the counts into job offsets, and
//                     their total (with the three face counts) is the entry's second host wait
//   k_render_tiles    one wavefront per (face, 8 x 8-pixel tile) job, one pixel per lane.  The job's face is found by a binary search of
//                     the job offsets (a wavefront-uniform walk of at most 31 steps), not read from a filled job list: filling the list
//                     of a triangle that covers the image would be the serial loop the jobs are there to avoid
//   both walk twice:  PASS 0 atomicMin on the uint64 pattern of t (t >= near > 0: the patterns order as the doubles do) into the depth
//                     image, which is pre-filled with the pattern of +inf; PASS 1 atomicMin of the face number where t equals the pixel's
//                     depth bit for bit, into the face image pre-filled with 0xffffffff (-1 as int32).  Integer minima commute: the images
//                     are a function of the input alone.  Both passes evaluate a (face, pixel) pair with the same ray_face()
//   k_render_resolve  one lane per pixel: U, V, W of the winner again, bary = (U, V, W) / det, zeros where nothing hit
//   k_render_shade    one lane per pixel: the attribute bytes of the winner's dominant corner, or the background
// No floating-point atomics anywhere.
#include <algorithm>
#include <cmath>

#include "wave.h"
#include "cross_rule.h"         // report_mesh_flag: the flag k_render_setup raises is k_check_mesh's
#include "mesh_index.h"
#include "pb3d_internal.h"

namespace {

constexpr i64 kMaxElems = (1ll << 31) - 1;
constexpr int kLanePixels = 64;                     // above it a face's box is walked by tile jobs
constexpr u64 kInfBits = 0x7ff0000000000000ull;

struct Cam { double R[9], c[3], f, cx, cy, near, depth; int meshify, H, W; };
struct Box { int x0, x1, y0, y1; };                 // inclusive, inside the image

template <bool VF64, bool I64>
__global__ __launch_bounds__(256) void k_render_setup(const void* __restrict__ verts, i64 nv, const void* __restrict__ faces, i64 nf, Cam cam,
                                                      double* __restrict__ P, u32* __restrict__ flag) {
    u32 bad = 0;
    const i64 t0 = (i64)blockIdx.x * 256 + threadIdx.x, step = (i64)gridDim.x * 256;
    for (i64 e = t0; e < 3 * nf; e += step) {
        const i64 v = load_index<I64>(faces, e);
        if (v < -nv || v >= nv) bad |= 1u;
    }
    for (i64 v = t0; v < nv; v += step) {
        double p[3];
        pb3d_load3<VF64>(verts, v, p);
        if (!(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]))) bad |= 2u;
        const double q0 = p[0] - cam.c[0], q1 = p[1] - cam.c[1], q2 = (cam.meshify ? cam.depth - p[2] : p[2]) - cam.c[2];
        P[3 * v] = (cam.R[0] * q0 + cam.R[1] * q1) + cam.R[2] * q2;
        P[3 * v + 1] = (cam.R[3] * q0 + cam.R[4] * q1) + cam.R[5] * q2;
        P[3 * v + 2] = (cam.R[6] * q0 + cam.R[7] * q1) + cam.R[8] * q2;
    }
    if (bad) atomicOr(flag, bad);
}

template <bool I64>
__device__ __forceinline__ void load_face(const double* P, i64 nv, const void* faces, i64 f, double A[3], double B[3], double C[3]) {
    const double* a = P + 3 * wrap(load_index<I64>(faces, 3 * f), nv);
    const double* b = P + 3 * wrap(load_index<I64>(faces, 3 * f + 1), nv);
    const double* c = P + 3 * wrap(load_index<I64>(faces, 3 * f + 2), nv);
    A[0] = a[0]; A[1] = a[1]; A[2] = a[2];
    B[0] = b[0]; B[1] = b[1]; B[2] = b[2];
    C[0] = c[0]; C[1] = c[1]; C[2] = c[2];
}

// PRUNE of include/pb3d.h.  false: no pixel can be hit.  Every value converted to int has been clamped to [0, W - 1] or [0, H - 1] as a
// double first, and a NaN anywhere (a comparison with it is false) leaves the whole image
__device__ __forceinline__ bool face_box(const double A[3], const double B[3], const double C[3], const Cam& cam, Box* b) {
    const double h = cam.near * 0.5;
    if (A[2] < h && B[2] < h && C[2] < h) return false;
    double xlo = 0.0, xhi = (double)(cam.W - 1), ylo = 0.0, yhi = (double)(cam.H - 1);
    if (A[2] >= h && B[2] >= h && C[2] >= h) {
        const double ua = __ddiv_rn(A[0], A[2]) * cam.f + cam.cx, ub = __ddiv_rn(B[0], B[2]) * cam.f + cam.cx, uc = __ddiv_rn(C[0], C[2]) * cam.f + cam.cx;
        const double va = -__ddiv_rn(A[1], A[2]) * cam.f + cam.cy, vb = -__ddiv_rn(B[1], B[2]) * cam.f + cam.cy, vc = -__ddiv_rn(C[1], C[2]) * cam.f + cam.cy;
        if (ua == ua && ub == ub && uc == uc && va == va && vb == vb && vc == vc) {
            xlo = fmax(floor(fmin(fmin(ua, ub), uc)) - 1.0, xlo);
            xhi = fmin(ceil(fmax(fmax(ua, ub), uc)) + 1.0, xhi);
            ylo = fmax(floor(fmin(fmin(va, vb), vc)) - 1.0, ylo);
            yhi = fmin(ceil(fmax(fmax(va, vb), vc)) + 1.0, yhi);
            if (!(xlo <= xhi && ylo <= yhi)) return false;
        }
    }
    b->x0 = (int)xlo; b->x1 = (int)xhi; b->y0 = (int)ylo; b->y1 = (int)yhi;
    return true;
}

// FACE against PIXEL of include/pb3d.h, the one place it is evaluated.  uvwd (or null): U, V, W, det
__device__ __forceinline__ bool ray_face(const double A[3], const double B[3], const double C[3], int u, int v, const Cam& cam, double* t,
                                         double* uvwd) {
    const double sx = __ddiv_rn((double)u - cam.cx, cam.f), sy = -__ddiv_rn((double)v - cam.cy, cam.f);
    const double xa = A[0] - sx * A[2], ya = A[1] - sy * A[2];
    const double xb = B[0] - sx * B[2], yb = B[1] - sy * B[2];
    const double xc = C[0] - sx * C[2], yc = C[1] - sy * C[2];
    const double U = xc * yb - yc * xb, V = xa * yc - ya * xc, W = xb * ya - yb * xa;
    const double det = (U + V) + W;
    const double T = (U * A[2] + V * B[2]) + W * C[2];
    *t = __ddiv_rn(T, det);
    if (uvwd) { uvwd[0] = U; uvwd[1] = V; uvwd[2] = W; uvwd[3] = det; }
    const bool neg = U < 0.0 || V < 0.0 || W < 0.0, pos = U > 0.0 || V > 0.0 || W > 0.0;
    return !(neg && pos) && det != 0.0 && *t >= cam.near;
}

// pixel (u, v) of the image against one face.  PASS 0: the depth minimum; PASS 1: the face minimum among the faces at that depth.
// The plain read in front of the depth atomic only saves atomics: the image never grows, so a t not below it cannot lower it
template <int PASS>
__device__ __forceinline__ void visit(const double A[3], const double B[3], const double C[3], int u, int v, u32 f, const Cam& cam,
                                      u64* depth, u32* win) {
    double t;
    if (!ray_face(A, B, C, u, v, cam, &t, nullptr)) return;
    const i64 pix = (i64)v * cam.W + u;
    const u64 bits = (u64)__double_as_longlong(t);
    if (PASS == 0) {
        if (bits < depth[pix]) atomicMin((unsigned long long*)&depth[pix], (unsigned long long)bits);
    } else {
        if (bits == depth[pix] && f < win[pix]) atomicMin(&win[pix], f);
    }
}

// stats (PASS 0 only): faces pruned, on the small path, on the large path.  jobs[f] (PASS 0 only) = the face's tile jobs, 0 unless large
template <bool I64, int PASS>
__global__ __launch_bounds__(256) void k_render_faces(const double* __restrict__ P, i64 nv, const void* __restrict__ faces, i64 nf, Cam cam,
                                                      u64* __restrict__ depth, u32* __restrict__ win, u32* __restrict__ jobs,
                                                      u64* __restrict__ stats) {
    u64 pruned = 0, small = 0, large = 0;
    for (i64 f = (i64)blockIdx.x * 256 + threadIdx.x; f < nf; f += (i64)gridDim.x * 256) {
        double A[3], B[3], C[3];
        load_face<I64>(P, nv, faces, f, A, B, C);
        Box b;
        u32 njobs = 0;
        if (!face_box(A, B, C, cam, &b)) {
            ++pruned;
        } else if ((i64)(b.x1 - b.x0 + 1) * (b.y1 - b.y0 + 1) <= kLanePixels) {
            ++small;
            for (int v = b.y0; v <= b.y1; ++v)
                for (int u = b.x0; u <= b.x1; ++u) visit<PASS>(A, B, C, u, v, (u32)f, cam, depth, win);
        } else {
            ++large;
            njobs = (u32)((b.x1 >> 3) - (b.x0 >> 3) + 1) * (u32)((b.y1 >> 3) - (b.y0 >> 3) + 1);    // <= Himg * Wimg < 2^31
        }
        if (PASS == 0) jobs[f] = njobs;
    }
    if (PASS == 0) {
        group_add(pruned, &stats[0]);
        group_add(small, &stats[1]);
        group_add(large, &stats[2]);
    }
}

// offsets: nf + 1 job offsets, offsets[nf] = njobs.  Job j belongs to the last face f with offsets[f] <= j (a face without jobs has
// offsets[f] == offsets[f + 1] and is never that one)
template <bool I64, int PASS>
__global__ __launch_bounds__(256) void k_render_tiles(const double* __restrict__ P, i64 nv, const void* __restrict__ faces, i64 nf, Cam cam,
                                                      const i64* __restrict__ offsets, i64 njobs, u64* __restrict__ depth, u32* __restrict__ win) {
    const int lane = threadIdx.x & 63;
    for (i64 j = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); j < njobs; j += (i64)gridDim.x * 4) {
        i64 lo = 0, hi = nf;                        // offsets[lo] <= j < offsets[hi]
        while (hi - lo > 1) {
            const i64 mid = lo + ((hi - lo) >> 1);
            if (offsets[mid] <= j) lo = mid; else hi = mid;
        }
        double A[3], B[3], C[3];
        load_face<I64>(P, nv, faces, lo, A, B, C);
        Box b;
        if (!face_box(A, B, C, cam, &b)) continue;  // never: the face has jobs
        const u32 k = (u32)(j - offsets[lo]), ntx = (u32)((b.x1 >> 3) - (b.x0 >> 3) + 1), ty = k / ntx, tx = k - ty * ntx;
        const int u = (int)(((u32)(b.x0 >> 3) + tx) * 8u) + (lane & 7), v = (int)(((u32)(b.y0 >> 3) + ty) * 8u) + (lane >> 3);
        if (u >= b.x0 && u <= b.x1 && v >= b.y0 && v <= b.y1) visit<PASS>(A, B, C, u, v, (u32)lo, cam, depth, win);
    }
}

template <bool I64>
__global__ __launch_bounds__(256) void k_render_resolve(const double* __restrict__ P, i64 nv, const void* __restrict__ faces, i64 nf, Cam cam,
                                                        const u32* __restrict__ win, double* __restrict__ bary) {
    const i64 npix = (i64)cam.H * cam.W;
    for (i64 pix = (i64)blockIdx.x * 256 + threadIdx.x; pix < npix; pix += (i64)gridDim.x * 256) {
        const u32 f = win[pix];
        double w[3] = {0.0, 0.0, 0.0};
        if ((i64)f < nf) {
            double A[3], B[3], C[3], t, q[4];
            load_face<I64>(P, nv, faces, (i64)f, A, B, C);
            const int v = (int)(pix / cam.W), u = (int)(pix - (i64)v * cam.W);
            ray_face(A, B, C, u, v, cam, &t, q);
            w[0] = __ddiv_rn(q[0], q[3]); w[1] = __ddiv_rn(q[1], q[3]); w[2] = __ddiv_rn(q[2], q[3]);
        }
        bary[3 * pix] = w[0]; bary[3 * pix + 1] = w[1]; bary[3 * pix + 2] = w[2];
    }
}

// a face number outside [0, nf) or a corner index outside [-nv, nv) is never followed: the pixel takes the background
template <bool I64, int CH>
__global__ __launch_bounds__(256) void k_render_shade(const int* __restrict__ face, const double* __restrict__ bary, i64 npix,
                                                      const void* __restrict__ faces, i64 nf, i64 nv, const u8* __restrict__ attr, u32 bg,
                                                      u8* __restrict__ image) {
    for (i64 pix = (i64)blockIdx.x * 256 + threadIdx.x; pix < npix; pix += (i64)gridDim.x * 256) {
        const i64 f = face[pix];
        u32 val = bg;
        if (f >= 0 && f < nf) {
            const double w0 = bary[3 * pix], w1 = bary[3 * pix + 1], w2 = bary[3 * pix + 2];
            int m = 0;
            double best = w0;
            if (w1 > best) { m = 1; best = w1; }
            if (w2 > best) m = 2;
            const i64 idx = load_index<I64>(faces, 3 * f + m);
            if (idx >= -nv && idx < nv) {
                const u8* a = attr + wrap(idx, nv) * CH;
                val = CH == 1 ? a[0] : (u32)a[0] | ((u32)a[1] << 8) | ((u32)a[2] << 16);
            }
        }
#pragma unroll
        for (int c = 0; c < CH; ++c) image[pix * CH + c] = (u8)(val >> (8 * c));
    }
}

__global__ __launch_bounds__(256) void k_render_fill(u64* __restrict__ p, i64 n, u64 value) {
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) p[i] = value;
}

bool finite_all(const double* p, int n) {
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(p[i])) return false;
    return true;
}

}  // namespace

extern "C" {

int pb3d_render_mesh_resident(pb3d_ctx* ctx, const void* d_verts, int verts_f64, int64_t nv, const void* d_faces, int faces_i64, int64_t nf,
                              int frame, double depth, const double R[9], const double cam[3], double f, double cx, double cy, int Himg,
                              int Wimg, double near, double* d_depth, int32_t* d_face, double* d_bary) {
    PB3D_REQUIRE(nv >= 0 && nf >= 0, "pb3d_render_mesh: negative count");
    PB3D_REQUIRE(nv <= kMaxElems && nf <= kMaxElems, "pb3d_render_mesh: at most 2^31 - 1 vertices and faces");
    PB3D_REQUIRE(Himg > 0 && Wimg > 0 && (i64)Himg * Wimg <= kMaxElems, "pb3d_render_mesh: the image must have 1 to 2^31 - 1 pixels (got %d x %d)", Himg,
                 Wimg);
    PB3D_REQUIRE(R != nullptr && cam != nullptr, "pb3d_render_mesh: null argument");
    PB3D_REQUIRE(finite_all(R, 9) && finite_all(cam, 3) && std::isfinite(cx) && std::isfinite(cy), "pb3d_render_mesh: R, cam, cx and cy must be finite");
    PB3D_REQUIRE(std::isfinite(f) && f > 0.0, "pb3d_render_mesh: f must be finite and > 0 (got %g)", f);
    PB3D_REQUIRE(std::isfinite(near) && near > 0.0, "pb3d_render_mesh: near must be finite and > 0 (got %g)", near);
    PB3D_REQUIRE(frame == 0 || frame == 1, "pb3d_render_mesh: frame must be 0 (points) or 1 (meshify), got %d", frame);
    PB3D_REQUIRE(frame == 0 || std::isfinite(depth), "pb3d_render_mesh: depth must be finite");
    PB3D_REQUIRE((nv == 0 || d_verts) && (nf == 0 || d_faces) && d_depth, "pb3d_render_mesh: null buffer");
    PB3D_REQUIRE((uintptr_t)d_depth % 8 == 0 && (uintptr_t)d_face % 4 == 0 && (uintptr_t)d_bary % 8 == 0, "pb3d_render_mesh: misaligned output");
    PB3D_REQUIRE(ctx != nullptr, "pb3d_render_mesh: null context");

    Cam c;
    for (int i = 0; i < 9; ++i) c.R[i] = R[i];
    for (int i = 0; i < 3; ++i) c.c[i] = cam[i];
    c.f = f; c.cx = cx; c.cy = cy; c.near = near; c.depth = frame ? depth : 0.0;
    c.meshify = frame; c.H = Himg; c.W = Wimg;
    const i64 npix = (i64)Himg * Wimg;

    void *cn, *cm = nullptr, *wn = d_face, *jb = nullptr, *of = nullptr;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_RENDER_COUNTS, 4 * sizeof(u64), &cn));
    u64* counts = (u64*)cn;                          // pruned, small, large; then the check's flag
    PB3D_HIP(hipMemsetAsync(cn, 0, 4 * sizeof(u64), ctx->stream));
    if (nv > 0) PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_RENDER_CAMERA, (size_t)nv * 3 * sizeof(double), &cm));
    if (nv > 0 || nf > 0) {
        const unsigned nb = pb3d_stream_blocks(ctx, std::max<i64>(nv, 3 * nf), 256, 8);
        with_mesh_types(verts_f64, faces_i64, [&](auto V, auto I) {
            hipLaunchKernelGGL((k_render_setup<decltype(V)::value, decltype(I)::value>), dim3(nb), dim3(256), 0, ctx->stream, d_verts, (i64)nv,
                               d_faces, (i64)nf, c, (double*)cm, (u32*)(counts + 3));
        });
        PB3D_CHECK_LAUNCH();
        u32 bad;
        PB3D_TRY(pb3d_read_back(ctx, &bad, counts + 3, sizeof(bad)));
        PB3D_TRY(report_mesh_flag("pb3d_render_mesh", bad, nv));
    }

    const bool want_face = d_face != nullptr || d_bary != nullptr;
    if (want_face && !d_face) PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_RENDER_WINNER, (size_t)npix * sizeof(u32), &wn));
    if (nf > 0) {
        PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_RENDER_JOBS, (size_t)nf * sizeof(u32), &jb));
        PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_RENDER_OFFSETS, (size_t)(nf + 1) * sizeof(i64), &of));
        PB3D_TRY(pb3d_scan_reserve(ctx, nf, PB3D_SLOT_RENDER_SCAN_LOCAL, PB3D_SLOT_RENDER_SCAN_SEGS));
    }
    ctx->render_last.valid = false;
    ctx->render_last.timed = false;
    pb3d_stamps<6> st = {ctx->tune_render_timing != 0, 0, {}};       // knob "render_timing"
    u64* dimg = (u64*)d_depth;
    u32* win = (u32*)wn;
    const unsigned pixel_blocks = pb3d_stream_blocks(ctx, npix, 256, 8);
    hipLaunchKernelGGL(k_render_fill, dim3(pixel_blocks), dim3(256), 0, ctx->stream, dimg, npix, kInfBits);
    PB3D_CHECK_LAUNCH();
    if (want_face) PB3D_HIP(hipMemsetAsync(win, 0xff, (size_t)npix * sizeof(u32), ctx->stream));
    PB3D_TRY(st.mark(ctx));

    i64 host[4] = {0, 0, 0, 0};                      // pruned, small, large, tile jobs
    if (nf > 0) {
        const unsigned face_blocks = pb3d_stream_blocks(ctx, nf, 256, 16);
        const double* P = (const double*)cm;
        const i64* offsets = (const i64*)of;
        auto faces_pass = [&](auto pass) {
            if (faces_i64) hipLaunchKernelGGL((k_render_faces<true, decltype(pass)::value>), dim3(face_blocks), dim3(256), 0, ctx->stream, P, (i64)nv,
                                              d_faces, (i64)nf, c, dimg, win, (u32*)jb, counts);
            else hipLaunchKernelGGL((k_render_faces<false, decltype(pass)::value>), dim3(face_blocks), dim3(256), 0, ctx->stream, P, (i64)nv, d_faces,
                                    (i64)nf, c, dimg, win, (u32*)jb, counts);
        };
        auto tiles_pass = [&](auto pass) {
            const unsigned tile_blocks = pb3d_stream_blocks(ctx, host[3], 4, 32);
            if (faces_i64) hipLaunchKernelGGL((k_render_tiles<true, decltype(pass)::value>), dim3(tile_blocks), dim3(256), 0, ctx->stream, P, (i64)nv,
                                              d_faces, (i64)nf, c, offsets, host[3], dimg, win);
            else hipLaunchKernelGGL((k_render_tiles<false, decltype(pass)::value>), dim3(tile_blocks), dim3(256), 0, ctx->stream, P, (i64)nv, d_faces,
                                    (i64)nf, c, offsets, host[3], dimg, win);
        };
        faces_pass(std::integral_constant<int, 0>{});
        PB3D_CHECK_LAUNCH();
        PB3D_TRY(pb3d_scan_counts(ctx, (const u32*)jb, nf, (i64*)of, PB3D_SLOT_RENDER_SCAN_LOCAL, PB3D_SLOT_RENDER_SCAN_SEGS));
        PB3D_HIP(hipMemcpyAsync(counts + 3, offsets + nf, sizeof(i64), hipMemcpyDeviceToDevice, ctx->stream));
        PB3D_TRY(pb3d_read_back(ctx, host, counts, 4 * sizeof(i64)));
        PB3D_TRY(st.mark(ctx));
        if (host[3] > 0) tiles_pass(std::integral_constant<int, 0>{});
        PB3D_CHECK_LAUNCH();
        PB3D_TRY(st.mark(ctx));
        if (want_face) {
            faces_pass(std::integral_constant<int, 1>{});
            PB3D_CHECK_LAUNCH();
            PB3D_TRY(st.mark(ctx));
            if (host[3] > 0) tiles_pass(std::integral_constant<int, 1>{});
            PB3D_CHECK_LAUNCH();
            PB3D_TRY(st.mark(ctx));
        }
    }
    if (d_bary) {
        if (faces_i64) hipLaunchKernelGGL(k_render_resolve<true>, dim3(pixel_blocks), dim3(256), 0, ctx->stream, (const double*)cm, (i64)nv, d_faces,
                                          (i64)nf, c, (const u32*)win, d_bary);
        else hipLaunchKernelGGL(k_render_resolve<false>, dim3(pixel_blocks), dim3(256), 0, ctx->stream, (const double*)cm, (i64)nv, d_faces, (i64)nf, c,
                                (const u32*)win, d_bary);
        PB3D_CHECK_LAUNCH();
    }
    PB3D_TRY(st.mark(ctx));
    for (int i = 0; i < 4; ++i) ctx->render_last.stats[i] = host[i];
    ctx->render_last.valid = true;
    return st.finish(ctx, ctx->render_last.ms, &ctx->render_last.timed);
}

int pb3d_render_shade_resident(pb3d_ctx* ctx, const int32_t* d_face, const double* d_bary, int64_t npix, const void* d_faces, int faces_i64,
                               int64_t nf, int64_t nv, const uint8_t* d_attr, int C, const uint8_t* bg, uint8_t* d_image) {
    PB3D_REQUIRE(npix >= 0 && npix <= kMaxElems, "pb3d_render_shade: 0 to 2^31 - 1 pixels");
    PB3D_REQUIRE(nv >= 0 && nf >= 0 && nv <= kMaxElems && nf <= kMaxElems, "pb3d_render_shade: at most 2^31 - 1 vertices and faces");
    PB3D_REQUIRE(C == 1 || C == 3, "pb3d_render_shade: C must be 1 or 3 (got %d)", C);
    PB3D_REQUIRE(bg != nullptr, "pb3d_render_shade: null argument");
    PB3D_REQUIRE(npix == 0 || (d_face && d_bary && d_image), "pb3d_render_shade: null buffer");
    PB3D_REQUIRE((nf == 0 || d_faces) && (nf == 0 || nv == 0 || d_attr), "pb3d_render_shade: null buffer");
    PB3D_REQUIRE(ctx != nullptr, "pb3d_render_shade: null context");
    if (npix == 0) return PB3D_OK;
    const u32 b = C == 1 ? bg[0] : (u32)bg[0] | ((u32)bg[1] << 8) | ((u32)bg[2] << 16);
    const dim3 grid(pb3d_stream_blocks(ctx, npix, 256, 8));
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, ctx->stream, (const int*)d_face, d_bary, (i64)npix, d_faces, (i64)nf, (i64)nv, d_attr, b, d_image);
    };
    if (faces_i64 && C == 1) go(k_render_shade<true, 1>);
    else if (faces_i64) go(k_render_shade<true, 3>);
    else if (C == 1) go(k_render_shade<false, 1>);
    else go(k_render_shade<false, 3>);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

int pb3d_render_last(const pb3d_ctx* ctx, int64_t stats[4]) {
    PB3D_REQUIRE(ctx != nullptr && stats != nullptr, "pb3d_render_last: null argument");
    PB3D_REQUIRE(ctx->render_last.valid, "pb3d_render_last: no rendering has completed on this context");
    for (int i = 0; i < 4; ++i) stats[i] = ctx->render_last.stats[i];
    return PB3D_OK;
}

int pb3d_render_last_ms(const pb3d_ctx* ctx, double pass_ms[5]) {
    PB3D_REQUIRE(ctx != nullptr && pass_ms != nullptr, "pb3d_render_last_ms: null argument");
    PB3D_REQUIRE(ctx->render_last.valid && ctx->render_last.timed,
                 "pb3d_render_last_ms: the last rendering was not timed (knob render_timing, and a face or bary image asked for)");
    for (int i = 0; i < 5; ++i) pass_ms[i] = ctx->render_last.ms[i];
    return PB3D_OK;
}

}  // extern "C"
