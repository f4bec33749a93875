// Unit normals of a point cloud from the k-neighbour rows of pb3d_knn_dev (csrc/nn.hip): what the point-to-plane step of csrc/icp.hip
// needs from a target that carries none (SfM clouds).  include/pb3d.h states the arithmetic to the bit: the neighbours' mean and
// covariance in row order, jacobi3 (csrc/jacobi3.h, shared with the roughness of csrc/surface.hip) on the covariance, the eigenvector
// of the smallest diagonal entry, one division by its length, one sign rule.  Plain float64 after widening -- no FMA (the Makefile
// passes -ffp-contract=off), no double-double: a normal has to be a function of the input that NumPy can restate operation by
// operation, and the direction of the smallest eigenvector is far less sensitive than the smallest eigenvalue the roughness path
// compensates for.
#include <cmath>

#include "jacobi3.h"
#include "pb3d_internal.h"

namespace {

struct View { double v[3]; };

// one lane per point.  VIEW: orient towards vp; else the component of largest magnitude is made positive
template <bool F64, bool VIEW>
__global__ __launch_bounds__(256) void k_point_normals(const void* __restrict__ pts, i64 n, const int* __restrict__ idx, int k, View vp,
                                                       double* __restrict__ out) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int* row = idx + i * k;
    double m[3] = {0.0, 0.0, 0.0};
    for (int j = 0; j < k; ++j) {
        double x[3];
        pb3d_load3<F64>(pts, row[j], x);
#pragma unroll
        for (int a = 0; a < 3; ++a) m[a] = m[a] + x[a];
    }
    const double kk = (double)k;
#pragma unroll
    for (int a = 0; a < 3; ++a) m[a] = m[a] / kk;
    double c00 = 0.0, c01 = 0.0, c02 = 0.0, c11 = 0.0, c12 = 0.0, c22 = 0.0;
    for (int j = 0; j < k; ++j) {
        double x[3];
        pb3d_load3<F64>(pts, row[j], x);
        const double y0 = x[0] - m[0], y1 = x[1] - m[1], y2 = x[2] - m[2];
        c00 = c00 + y0 * y0; c01 = c01 + y0 * y1; c02 = c02 + y0 * y2;
        c11 = c11 + y1 * y1; c12 = c12 + y1 * y2; c22 = c22 + y2 * y2;
    }
    double A[3][3] = {{c00, c01, c02}, {c01, c11, c12}, {c02, c12, c22}};
    double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    jacobi3(A, V);
    // the column of the smallest diagonal entry, the lowest on a tie (selects, not an indexed read: V stays in registers)
    const bool c1 = A[1][1] < A[0][0];
    const double d01 = c1 ? A[1][1] : A[0][0];
    const bool c2 = A[2][2] < d01;
    double nv[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) nv[a] = c2 ? V[a][2] : (c1 ? V[a][1] : V[a][0]);
    const double len = sqrt((nv[0] * nv[0] + nv[1] * nv[1]) + nv[2] * nv[2]);
#pragma unroll
    for (int a = 0; a < 3; ++a) nv[a] = nv[a] / len;
    bool flip;
    if (VIEW) {
        double x[3];
        pb3d_load3<F64>(pts, i, x);
        flip = ((vp.v[0] - x[0]) * nv[0] + (vp.v[1] - x[1]) * nv[1]) + (vp.v[2] - x[2]) * nv[2] < 0.0;
    } else {
        const double a0 = fabs(nv[0]), a1 = fabs(nv[1]), a2 = fabs(nv[2]);
        const bool b1 = a1 > a0;
        const bool b2 = a2 > (b1 ? a1 : a0);
        flip = (b2 ? nv[2] : (b1 ? nv[1] : nv[0])) < 0.0;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) out[3 * i + a] = flip ? -nv[a] : nv[a];
}

template <bool F64, bool VIEW>
void launch(pb3d_ctx* ctx, const void* d_pts, i64 n, const int* d_idx, int k, const View& vp, double* d_out) {
    hipLaunchKernelGGL((k_point_normals<F64, VIEW>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_pts, n, d_idx, k, vp, d_out);
}

}  // namespace

extern "C" {

int pb3d_point_normals_resident(pb3d_ctx* ctx, const void* d_pts, int pts_f64, int64_t n, const int32_t* d_idx, int k, const double* viewpoint,
                                double* d_normals) {
    PB3D_REQUIRE(k >= 3 && k <= PB3D_KNN_MAX_K, "pb3d_point_normals: k must be in [3, %d] (got %d)", PB3D_KNN_MAX_K, k);
    PB3D_REQUIRE(n >= 0 && n <= pb3d_max_points, "pb3d_point_normals: need 0 <= n <= 2^31 - 1 points");
    if (viewpoint)
        for (int a = 0; a < 3; ++a) PB3D_REQUIRE(std::isfinite(viewpoint[a]), "pb3d_point_normals: the viewpoint is not finite");
    if (n == 0) return PB3D_OK;
    PB3D_REQUIRE(n >= k, "pb3d_point_normals: k = %d neighbours of %lld points", k, (long long)n);
    PB3D_REQUIRE(d_pts && d_idx && d_normals, "pb3d_point_normals: null buffer");
    PB3D_REQUIRE(ctx != nullptr, "pb3d_point_normals: null context");
    PB3D_TRY(pb3d_check_index_range(ctx, d_idx, 0, (i64)n * k, 0, n, "pb3d_point_normals"));
    View vp = {{0.0, 0.0, 0.0}};
    if (viewpoint) memcpy(vp.v, viewpoint, sizeof(vp.v));
    if (viewpoint) {
        if (pts_f64) launch<true, true>(ctx, d_pts, n, d_idx, k, vp, d_normals);
        else launch<false, true>(ctx, d_pts, n, d_idx, k, vp, d_normals);
    } else {
        if (pts_f64) launch<true, false>(ctx, d_pts, n, d_idx, k, vp, d_normals);
        else launch<false, false>(ctx, d_pts, n, d_idx, k, vp, d_normals);
    }
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

}  // extern "C"
