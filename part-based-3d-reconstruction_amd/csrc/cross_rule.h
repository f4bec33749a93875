// The crossing rule of csrc/voxelize.hip (rays through the columns of a grid) and csrc/inside.hip (rays through arbitrary query
// points): which faces a ray along the third coordinate crosses, and at what height.  One text for both, so that a query at a lattice
// point gets the bytes of the voxel there.  include/pb3d.h states the rule ("mesh -> grid", FACE steps 1, 3 and 4); the box of step 2
// stays with each user, since one clamps integer columns to a grid and the other compares a query with the corners.
// Every product, sum, difference and quotient is one rounded float64 operation (the Makefile passes -ffp-contract=off).
// Also here: k_check_mesh, the sweep both entries run, and wait for, in front of everything that gathers through the face indices,
// with its host side: check_mesh, and report_mesh_flag for csrc/render.hip, whose set-up kernel raises the same flag.
#pragma once
#include <algorithm>
#include <cmath>

#include "mesh_index.h"
#include "pb3d_internal.h"

namespace {

// bit 0 of the flag = a face index outside [-nv, nv), bit 1 = a vertex coordinate that is not finite
template <bool VF64, bool I64>
__global__ __launch_bounds__(256) void k_check_mesh(const void* __restrict__ verts, i64 nv, const void* __restrict__ faces, i64 nf,
                                                    u32* __restrict__ flag) {
    u32 bad = 0;
    const i64 t0 = (i64)blockIdx.x * 256 + threadIdx.x, step = (i64)gridDim.x * 256;
    for (i64 e = t0; e < 3 * nf; e += step) {
        const i64 v = load_index<I64>(faces, e);
        if (v < -nv || v >= nv) bad |= 1u;
    }
    for (i64 e = t0; e < 3 * nv; e += step) {
        const double x = VF64 ? ((const double*)verts)[e] : (double)((const float*)verts)[e];
        if (!isfinite(x)) bad |= 2u;
    }
    if (bad) atomicOr(flag, bad);
}

// what a raised flag means to the caller of entry `what`: PB3D_EINDEX for bit 0, else PB3D_EINVAL for bit 1
inline int report_mesh_flag(const char* what, u32 bad, i64 nv) {
    if (bad & 1u) {
        pb3d_set_error("%s: index out of bounds for %lld entries", what, (long long)nv);
        return PB3D_EINDEX;
    }
    PB3D_REQUIRE(!(bad & 2u), "%s: a vertex coordinate is not finite", what);
    return PB3D_OK;
}

// the sweep over a mesh with a vertex or a face, the flag cleared first, and its verdict: one host wait.  (A template only so that a
// file which includes this header for the rule alone carries no copy of the four kernels)
template <class = void>
int check_mesh(pb3d_ctx* ctx, const char* what, const void* d_verts, int verts_f64, i64 nv, const void* d_faces, int faces_i64, i64 nf,
                      u32* d_flag) {
    PB3D_HIP(hipMemsetAsync(d_flag, 0, sizeof(u32), ctx->stream));
    const unsigned nb = pb3d_stream_blocks(ctx, 3 * std::max<i64>(nv, nf), 256, 8);
    with_mesh_types(verts_f64, faces_i64, [&](auto V, auto I) {
        hipLaunchKernelGGL((k_check_mesh<decltype(V)::value, decltype(I)::value>), dim3(nb), dim3(256), 0, ctx->stream, d_verts, nv, d_faces, nf,
                           d_flag);
    });
    PB3D_CHECK_LAUNCH();
    u32 bad;
    PB3D_TRY(pb3d_read_back(ctx, &bad, d_flag, sizeof(bad)));
    return report_mesh_flag(what, bad, nv);
}

// what a face needs per ray (x, y): edge e accepts where ex * (y - ly) - ey * (x - lx) is >= 0 (bit e of pos) or < 0
struct CrossFace {
    double ex[3], ey[3], lx[3], ly[3];
    double a0, a1, a2, nx, ny, area;
    u32 pos;
};

// step 1: twice the signed area of the projection; 0: the face contributes nothing
__device__ __forceinline__ double cross_area(const double* A, const double* B, const double* C) {
    return (B[0] - A[0]) * (C[1] - A[1]) - (B[1] - A[1]) * (C[0] - A[0]);
}

__device__ __forceinline__ void set_edge(CrossFace* f, int e, const double* P, const double* Q, bool up) {
    const bool flipped = Q[0] < P[0] || (Q[0] == P[0] && Q[1] < P[1]);
    const double lo0 = flipped ? Q[0] : P[0], lo1 = flipped ? Q[1] : P[1], hi0 = flipped ? P[0] : Q[0], hi1 = flipped ? P[1] : Q[1];
    f->ex[e] = hi0 - lo0;
    f->ey[e] = hi1 - lo1;
    f->lx[e] = lo0;
    f->ly[e] = lo1;
    if (up != flipped) f->pos |= 1u << e;
}

// step 3's set-up, from the first two coordinates of the corners alone; area != 0
__device__ __forceinline__ void cross_edges(const double* A, const double* B, const double* C, double area, CrossFace* f) {
    f->pos = 0;
    const bool up = area > 0.0;
    set_edge(f, 0, A, B, up);
    set_edge(f, 1, B, C, up);
    set_edge(f, 2, C, A, up);
    f->area = area;
}

// step 4's set-up: the plane
__device__ __forceinline__ void cross_plane(const double* A, const double* B, const double* C, CrossFace* f) {
    f->nx = (B[1] - A[1]) * (C[2] - A[2]) - (B[2] - A[2]) * (C[1] - A[1]);
    f->ny = (B[2] - A[2]) * (C[0] - A[0]) - (B[0] - A[0]) * (C[2] - A[2]);
    f->a0 = A[0]; f->a1 = A[1]; f->a2 = A[2];
}

// step 3: all three edges accept the ray through (x, y) (cross_edges has run)
__device__ __forceinline__ bool cross_covers(const CrossFace& f, double x, double y) {
    bool in = true;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const double E = f.ex[e] * (y - f.ly[e]) - f.ey[e] * (x - f.lx[e]);
        in &= ((f.pos >> e) & 1u) ? E >= 0.0 : E < 0.0;
    }
    return in;
}

// step 4: where the ray through (x, y) meets the face's plane (cross_edges and cross_plane have run)
__device__ __forceinline__ double cross_height(const CrossFace& f, double x, double y) {
    return f.a2 - __ddiv_rn(f.nx * (x - f.a0) + f.ny * (y - f.a1), f.area);
}

}  // namespace
