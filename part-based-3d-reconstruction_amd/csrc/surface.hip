// Mesh regularity: the surface block of the inter-method evaluation (reference utils/eval_helpers.py:198-245) -- face normals, vertex
// normals and the three per-vertex quantities of compute_surface_metrics.
//
// Normals are bit for bit NumPy's, in the vertex dtype (float32 or float64; the Makefile passes -ffp-contract=off, every operation
// below is one IEEE operation):  n = cross(v1 - v0, v2 - v0), each component one rounded product minus one rounded product;
// n / (sqrt((x*x + y*y) + z*z) + 1e-8) with 1e-8 rounded to the dtype.  The reference adds face normals into vertices in a double
// loop over (face, corner); floating-point addition is not associative, so no atomics: the vertex -> incident-face lists are
// counted, scanned (csrc/points.hip's scan) and filled -- integer atomics, whose order is then removed by sorting each list -- and
// one lane adds a vertex's face normals in ascending face order, starting from 0.
//
// The per-vertex metrics take the k-neighbour rows of pb3d_knn_dev (csrc/nn.hip) and work in float64.  What cancels is carried as
// an unevaluated sum of two doubles (two_sum / two_prod with an explicit fma): the neighbours' mean, the centred coordinates, the
// n_j . n_i that goes into acos near 1, and the sums.  The smallest covariance eigenvalue has to stay accurate when it is far below the
// largest (a smooth surface): forming the covariance in the input frame would lose it to the rounding of the large entries, so the
// 3 x 3 cyclic Jacobi solve is repeated in its own eigenvector frame -- the centred points are rotated by the vectors found so far
// and the covariance is accumulated again, now nearly diagonal with the small eigenvalue as its own small entry.
#include <cmath>

#include "jacobi3.h"
#include "mesh_index.h"
#include "pb3d_internal.h"

namespace {

constexpr i64 kMaxElems = (1ll << 31) - 1;      // vertices, faces: positions are 32-bit
constexpr int kFrames = 3;                      // covariance solves per vertex: the input frame, then twice its own eigenvector frame

// ---- index check: flag = 1 if any of the n entries is outside [lo, hi) ---------------------------------------------------------------
template <bool I64>
__global__ __launch_bounds__(256) void k_check_indices(const void* __restrict__ idx, i64 n, i64 lo, i64 hi, u32* __restrict__ flag) {
    bool bad = false;
    for (i64 e = (i64)blockIdx.x * 256 + threadIdx.x; e < n; e += (i64)gridDim.x * 256) {
        const i64 v = load_index<I64>(idx, e);
        bad |= v < lo || v >= hi;
    }
    if (bad) atomicOr(flag, 1u);
}

int check_indices(pb3d_ctx* ctx, const void* d_idx, int i64_entries, i64 n, i64 lo, i64 hi, const char* what) {
    if (n == 0) return PB3D_OK;
    void* f;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_SURF_FLAG, sizeof(u32), &f));
    PB3D_HIP(hipMemsetAsync(f, 0, sizeof(u32), ctx->stream));
    const unsigned nb = pb3d_stream_blocks(ctx, n, 256, 8);
    hipLaunchKernelGGL((i64_entries ? k_check_indices<true> : k_check_indices<false>), dim3(nb), dim3(256), 0, ctx->stream, d_idx, n, lo, hi, (u32*)f);
    PB3D_CHECK_LAUNCH();
    u32 bad;
    PB3D_TRY(pb3d_read_back(ctx, &bad, f, sizeof(bad)));
    if (bad) {
        pb3d_set_error("%s: index out of bounds for %lld entries", what, (long long)hi);
        return PB3D_EINDEX;
    }
    return PB3D_OK;
}

// ---- NumPy's arithmetic in the vertex dtype ------------------------------------------------------------------------------------------
// sqrtf is the correctly rounded one (hipcc's default for float sqrt and divide); __fsqrt_rn maps to the approximate native sqrt
__device__ __forceinline__ float np_sqrt(float v) { return sqrtf(v); }
__device__ __forceinline__ double np_sqrt(double v) { return __dsqrt_rn(v); }
__device__ __forceinline__ float np_div(float a, float b) { return __fdiv_rn(a, b); }
__device__ __forceinline__ double np_div(double a, double b) { return __ddiv_rn(a, b); }

// v / (np.linalg.norm(v) + 1e-8)
template <class T>
__device__ __forceinline__ void normalize3(T x, T y, T z, T* out) {
    const T d = np_sqrt((x * x + y * y) + z * z) + (T)1e-8;
    out[0] = np_div(x, d); out[1] = np_div(y, d); out[2] = np_div(z, d);
}

template <class T, bool I64>
__global__ __launch_bounds__(256) void k_triangle_normals(const T* __restrict__ verts, i64 nv, const void* __restrict__ faces, i64 nf,
                                                          T* __restrict__ out) {
    const i64 f = (i64)blockIdx.x * 256 + threadIdx.x;
    if (f >= nf) return;
    const T* v0 = verts + 3 * wrap(load_index<I64>(faces, 3 * f), nv);
    const T* v1 = verts + 3 * wrap(load_index<I64>(faces, 3 * f + 1), nv);
    const T* v2 = verts + 3 * wrap(load_index<I64>(faces, 3 * f + 2), nv);
    const T a0 = v1[0] - v0[0], a1 = v1[1] - v0[1], a2 = v1[2] - v0[2];
    const T b0 = v2[0] - v0[0], b1 = v2[1] - v0[1], b2 = v2[2] - v0[2];
    const T p0 = a1 * b2, m0 = a2 * b1, p1 = a2 * b0, m1 = a0 * b2, p2 = a0 * b1, m2 = a1 * b0;
    normalize3<T>(p0 - m0, p1 - m1, p2 - m2, out + 3 * f);
}

// ---- vertex -> incident faces --------------------------------------------------------------------------------------------------------
template <bool I64>
__global__ __launch_bounds__(256) void k_incident_count(const void* __restrict__ faces, i64 nv, i64 ncorners, u32* __restrict__ counts) {
    for (i64 e = (i64)blockIdx.x * 256 + threadIdx.x; e < ncorners; e += (i64)gridDim.x * 256)
        atomicAdd(&counts[wrap(load_index<I64>(faces, e), nv)], 1u);
}

// cursor: zeroed per-vertex counters; the order within a vertex's list is whatever the atomics give (k_vertex_normals sorts it)
template <bool I64>
__global__ __launch_bounds__(256) void k_incident_fill(const void* __restrict__ faces, i64 nv, i64 ncorners, const i64* __restrict__ start,
                                                       u32* __restrict__ cursor, u32* __restrict__ incident) {
    for (i64 e = (i64)blockIdx.x * 256 + threadIdx.x; e < ncorners; e += (i64)gridDim.x * 256) {
        const i64 v = wrap(load_index<I64>(faces, e), nv);
        incident[start[v] + atomicAdd(&cursor[v], 1u)] = (u32)(e / 3);
    }
}

__device__ __forceinline__ void sift_down(u32* a, i64 root, i64 n) {
    const u32 v = a[root];
    for (;;) {
        i64 c = 2 * root + 1;
        if (c >= n) break;
        u32 cv = a[c];
        if (c + 1 < n) {
            const u32 r = a[c + 1];
            if (r > cv) { cv = r; ++c; }
        }
        if (cv <= v) break;
        a[root] = cv;
        root = c;
    }
    a[root] = v;
}

// ascending heapsort in place: one lane, any length, n log n steps (a fan's list has thousands of entries)
__device__ __forceinline__ void sort_list(u32* a, i64 n) {
    for (i64 i = n / 2 - 1; i >= 0; --i) sift_down(a, i, n);
    for (i64 m = n - 1; m > 0; --m) {
        const u32 t = a[0]; a[0] = a[m]; a[m] = t;
        sift_down(a, 0, m);
    }
}

// one lane per vertex: its incident faces in ascending order, their normals added from 0 in the vertex dtype, then normalised
template <class T>
__global__ __launch_bounds__(256) void k_vertex_normals(i64 nv, const i64* __restrict__ start, u32* __restrict__ incident,
                                                        const T* __restrict__ face_normals, T* __restrict__ out) {
    const i64 v = (i64)blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    const i64 s = start[v], e = start[v + 1];
    sort_list(incident + s, e - s);
    T x = 0, y = 0, z = 0;
    for (i64 p = s; p < e; ++p) {
        const T* n = face_normals + 3 * (i64)incident[p];
        x += n[0]; y += n[1]; z += n[2];
    }
    normalize3<T>(x, y, z, out + 3 * v);
}

// ---- float64 pairs -------------------------------------------------------------------------------------------------------------------
struct dd { double h, l; };     // the value h + l, |l| <= ulp(h) / 2

__device__ __forceinline__ dd two_sum(double a, double b) {
    const double s = a + b, bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}
__device__ __forceinline__ dd two_prod(double a, double b) {
    const double p = a * b;
    return {p, __fma_rn(a, b, -p)};
}
__device__ __forceinline__ dd dd_add(dd a, dd b) {
    const dd s = two_sum(a.h, b.h);
    const double e = s.l + (a.l + b.l);
    const double h = s.h + e;
    return {h, e - (h - s.h)};
}
__device__ __forceinline__ dd dd_add_prod(dd acc, double a, double b) { return dd_add(acc, two_prod(a, b)); }
// (a.h + a.l) / n for a small positive integer n
__device__ __forceinline__ dd dd_div_int(dd a, double n) {
    const double h = a.h / n;
    return {h, (__fma_rn(-h, n, a.h) + a.l) / n};
}
// x - m
__device__ __forceinline__ dd dd_sub_from(double x, dd m) {
    const dd s = two_sum(x, -m.h);
    const double e = s.l - m.l;
    const double h = s.h + e;
    return {h, e - (h - s.h)};
}

// degrees(arccos(clip(a . b, -1, 1))), the dot product rounded once
__device__ __forceinline__ double angle_deg(const double* a, const double* b) {
    dd s = two_prod(a[0], b[0]);
    s = dd_add_prod(s, a[1], b[1]);
    s = dd_add_prod(s, a[2], b[2]);
    const double d = fmin(fmax(s.h + s.l, -1.0), 1.0);
    return acos(d) * (180.0 / 3.14159265358979323846);
}

// one lane per vertex (reference :221-239)
template <bool F64>
__global__ __launch_bounds__(256) void k_surface_metrics(const void* __restrict__ verts, const void* __restrict__ normals, i64 nv,
                                                         const int* __restrict__ idx, int k, double* __restrict__ normal_std,
                                                         double* __restrict__ roughness, double* __restrict__ curvature) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    const int* row = idx + i * k;
    const double kk = (double)k;
    double c[3], cn[3];
    pb3d_load3<F64>(verts, i, c);
    pb3d_load3<F64>(normals, i, cn);

    // neighbour mean and mean angle
    dd sp[3] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}}, sa = {0.0, 0.0};
    for (int j = 0; j < k; ++j) {
        double p[3], n[3];
        pb3d_load3<F64>(verts, row[j], p);
        pb3d_load3<F64>(normals, row[j], n);
#pragma unroll
        for (int a = 0; a < 3; ++a) sp[a] = dd_add(sp[a], {p[a], 0.0});
        sa = dd_add(sa, {angle_deg(n, cn), 0.0});
    }
    dd mean[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) mean[a] = dd_div_int(sp[a], kk);
    const dd mean_a = dd_div_int(sa, kk);

    // np.linalg.norm(nbr_pts.mean(axis=0) - center)
    {
        double d[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) d[a] = (mean[a].h - c[a]) + mean[a].l;
        curvature[i] = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    }

    // np.std(angles): population variance about the mean
    {
        dd var = {0.0, 0.0};
        for (int j = 0; j < k; ++j) {
            double n[3];
            pb3d_load3<F64>(normals, row[j], n);
            const dd dev = dd_sub_from(angle_deg(n, cn), mean_a);
            const double d = dev.h + dev.l;
            var = dd_add_prod(var, d, d);
        }
        normal_std[i] = sqrt((var.h + var.l) / kk);
    }

    // smallest eigenvalue of the neighbours' covariance
    double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    double lam = 0.0;
    for (int frame = 0; frame < kFrames; ++frame) {
        dd C[6] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};    // 00 11 22 01 02 12
        for (int j = 0; j < k; ++j) {
            double p[3];
            pb3d_load3<F64>(verts, row[j], p);
            dd x[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) x[a] = dd_sub_from(p[a], mean[a]);
            double y[3];                    // the centred point in the frame V, rounded once per component
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                dd s = two_prod(x[0].h, V[0][b]);
                s = dd_add_prod(s, x[1].h, V[1][b]);
                s = dd_add_prod(s, x[2].h, V[2][b]);
                y[b] = (s.h + ((x[0].l * V[0][b] + x[1].l * V[1][b]) + x[2].l * V[2][b])) + s.l;
            }
            C[0] = dd_add_prod(C[0], y[0], y[0]);
            C[1] = dd_add_prod(C[1], y[1], y[1]);
            C[2] = dd_add_prod(C[2], y[2], y[2]);
            C[3] = dd_add_prod(C[3], y[0], y[1]);
            C[4] = dd_add_prod(C[4], y[0], y[2]);
            C[5] = dd_add_prod(C[5], y[1], y[2]);
        }
        double A[3][3], R[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
        A[0][0] = C[0].h + C[0].l; A[1][1] = C[1].h + C[1].l; A[2][2] = C[2].h + C[2].l;
        A[0][1] = A[1][0] = C[3].h + C[3].l;
        A[0][2] = A[2][0] = C[4].h + C[4].l;
        A[1][2] = A[2][1] = C[5].h + C[5].l;
        jacobi3(A, R);
        lam = fmin(fmin(A[0][0], A[1][1]), A[2][2]);
        double W[3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) W[a][b] = (V[a][0] * R[0][b] + V[a][1] * R[1][b]) + V[a][2] * R[2][b];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) V[a][b] = W[a][b];
    }
    roughness[i] = fmax(lam, 0.0) / (kk - 1.0);
}

int triangle_normals(pb3d_ctx* ctx, const void* d_verts, int verts_f64, i64 nv, const void* d_faces, int faces_i64, i64 nf, void* d_out) {
    if (nf == 0) return PB3D_OK;
    with_mesh_types(verts_f64, faces_i64, [&](auto V, auto I) {
        using T = std::conditional_t<decltype(V)::value, double, float>;
        hipLaunchKernelGGL((k_triangle_normals<T, decltype(I)::value>), dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, ctx->stream,
                           (const T*)d_verts, nv, d_faces, nf, (T*)d_out);
    });
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

int require_mesh(const char* what, const pb3d_ctx* ctx, const void* d_verts, i64 nv, const void* d_faces, i64 nf, const void* d_out, i64 nout) {
    PB3D_REQUIRE(nv >= 0 && nf >= 0, "%s: negative count", what);
    PB3D_REQUIRE(nv <= kMaxElems && nf <= kMaxElems / 3, "%s: at most 2^31 - 1 vertices and face corners", what);
    PB3D_REQUIRE((nv == 0 || d_verts) && (nf == 0 || d_faces) && (nout == 0 || d_out), "%s: null buffer", what);
    PB3D_REQUIRE(ctx != nullptr, "%s: null context", what);
    return PB3D_OK;
}

}  // namespace

int pb3d_check_index_range(pb3d_ctx* ctx, const void* d_idx, int i64_entries, i64 n, i64 lo, i64 hi, const char* what) {
    return check_indices(ctx, d_idx, i64_entries, n, lo, hi, what);
}

extern "C" {

int pb3d_triangle_normals_dev(pb3d_ctx* ctx, const void* d_verts, int verts_f64, int64_t nv, const void* d_faces, int faces_i64, int64_t nf,
                              void* d_out) {
    PB3D_TRY(require_mesh("pb3d_triangle_normals", ctx, d_verts, nv, d_faces, nf, d_out, nf));
    PB3D_TRY(check_indices(ctx, d_faces, faces_i64, 3 * nf, -nv, nv, "pb3d_triangle_normals"));
    return triangle_normals(ctx, d_verts, verts_f64, nv, d_faces, faces_i64, nf, d_out);
}

int pb3d_vertex_normals_dev(pb3d_ctx* ctx, const void* d_verts, int verts_f64, int64_t nv, const void* d_faces, int faces_i64, int64_t nf,
                            void* d_out) {
    PB3D_TRY(require_mesh("pb3d_vertex_normals", ctx, d_verts, nv, d_faces, nf, d_out, nv));
    PB3D_TRY(check_indices(ctx, d_faces, faces_i64, 3 * nf, -nv, nv, "pb3d_vertex_normals"));
    if (nv == 0) return PB3D_OK;
    const size_t esz = verts_f64 ? sizeof(double) : sizeof(float);
    void *fn, *cnt, *st, *inc;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_SURF_FACE_NORMALS, (size_t)(nf > 0 ? nf : 1) * 3 * esz, &fn));
    PB3D_TRY(triangle_normals(ctx, d_verts, verts_f64, nv, d_faces, faces_i64, nf, fn));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_SURF_VERT_COUNTS, (size_t)nv * sizeof(u32), &cnt));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_SURF_VERT_STARTS, (size_t)(nv + 1) * sizeof(i64), &st));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_SURF_INCIDENT, (size_t)(nf > 0 ? 3 * nf : 1) * sizeof(u32), &inc));
    const i64 nc = 3 * nf;
    const unsigned nb = pb3d_stream_blocks(ctx, nc, 256, 8);
    PB3D_HIP(hipMemsetAsync(cnt, 0, (size_t)nv * sizeof(u32), ctx->stream));
    if (nc > 0) {
        hipLaunchKernelGGL((faces_i64 ? k_incident_count<true> : k_incident_count<false>), dim3(nb), dim3(256), 0, ctx->stream, d_faces, (i64)nv, nc, (u32*)cnt);
        PB3D_CHECK_LAUNCH();
    }
    PB3D_TRY(pb3d_scan_counts(ctx, (const u32*)cnt, nv, (i64*)st, PB3D_SLOT_SURF_SCAN_LOCAL, PB3D_SLOT_SURF_SCAN_SEGS));
    PB3D_HIP(hipMemsetAsync(cnt, 0, (size_t)nv * sizeof(u32), ctx->stream));      // the fill's cursors
    if (nc > 0) {
        hipLaunchKernelGGL((faces_i64 ? k_incident_fill<true> : k_incident_fill<false>), dim3(nb), dim3(256), 0, ctx->stream, d_faces, (i64)nv, nc,
                           (const i64*)st, (u32*)cnt, (u32*)inc);
        PB3D_CHECK_LAUNCH();
    }
    const dim3 grid((unsigned)((nv + 255) / 256));
    if (verts_f64) hipLaunchKernelGGL(k_vertex_normals<double>, grid, dim3(256), 0, ctx->stream, (i64)nv, (const i64*)st, (u32*)inc,
                                      (const double*)fn, (double*)d_out);
    else hipLaunchKernelGGL(k_vertex_normals<float>, grid, dim3(256), 0, ctx->stream, (i64)nv, (const i64*)st, (u32*)inc, (const float*)fn,
                            (float*)d_out);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

int pb3d_surface_metrics_dev(pb3d_ctx* ctx, const void* d_verts, const void* d_normals, int verts_f64, int64_t nv, const int32_t* d_idx, int k,
                             double* d_normal_std, double* d_roughness, double* d_curvature) {
    PB3D_REQUIRE(k >= 2 && k <= PB3D_KNN_MAX_K, "pb3d_surface_metrics: k must be in [2, %d] (got %d)", PB3D_KNN_MAX_K, k);
    PB3D_REQUIRE(nv >= 0 && nv <= kMaxElems, "pb3d_surface_metrics: need 0 <= nv <= 2^31 - 1 vertices");
    if (nv == 0) return PB3D_OK;
    PB3D_REQUIRE(d_verts && d_normals && d_idx && d_normal_std && d_roughness && d_curvature, "pb3d_surface_metrics: null buffer");
    PB3D_REQUIRE(ctx != nullptr, "pb3d_surface_metrics: null context");
    PB3D_TRY(check_indices(ctx, d_idx, 0, (i64)nv * k, 0, nv, "pb3d_surface_metrics"));
    const dim3 grid((unsigned)((nv + 255) / 256));
    if (verts_f64) hipLaunchKernelGGL(k_surface_metrics<true>, grid, dim3(256), 0, ctx->stream, d_verts, d_normals, (i64)nv, d_idx, k,
                                      d_normal_std, d_roughness, d_curvature);
    else hipLaunchKernelGGL(k_surface_metrics<false>, grid, dim3(256), 0, ctx->stream, d_verts, d_normals, (i64)nv, d_idx, k, d_normal_std,
                            d_roughness, d_curvature);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

}  // extern "C"
