// cast_rays: the first hit (or any hit) of arbitrary rays on a triangle mesh (include/pb3d.h, "rays against a mesh", has the rule to the
// bit and the argument for the margins; DESIGN.md "Rays against a mesh" has the passes and their times).  The face test is
// csrc/render.hip's (Woop, Benthin and Wald 2013, all float64, one rounded operation each) with the pixel's shear replaced by the ray's
// own: with the identity rotation and d = (sx, sy, 1) the operations are that file's, one for one.  What differs is everything around
// the test: the rays are scattered, so nothing is rasterised and the faces need an index.
//
// Index: csrc/face_index.hip's over all three axes, nothing skipped (a face without an area on one axis is hit by rays along another).
//   k_raycast          one lane per ray, in the caller's order.  A SLAB WALK along kz, the axis of the ray's largest |d|: the ray's kz
//                      range, clipped to [t_min, t_max] and to the box of the vertices, gives a run of cell layers; per layer, in the
//                      ray's direction, the ray's kx and ky at the layer's two bounding planes (clipped to the ray's range) give two
//                      intervals, widened by the margin and converted by the index's own cell_of, and every cell of that rectangle
//                      (|Sx|, |Sy| <= 1: usually 1 - 4 cells) has every listed face tested.  A face listed in several visited cells
//                      is tested again; the minimum over (t, face number) is idempotent.  After a layer the walk stops when the
//                      best t is STRICTLY below the t of the layer's far plane -- taken from the unwidened plane -- less
//                      2 tol |Sz| and 1e-12 of itself: a hit beyond that plane cannot be smaller or tie.  In any-hit mode it stops
//                      after the first layer with a hit.  The best (t, face, U, V, W, det) lives in registers and every output is written once.
//                      NO atomics: under knob "raycast_stats" each workgroup leaves five partial counts and k_raycast_totals adds
//                      them, so results and counts are functions of the input alone.
//                      kx, ky, kz are run-time values: the ray's origin and the grid are permuted once with selects and a face's
//                      72-byte corner row is read at computed offsets, so no private array is indexed by them.
//                      first hit 124-126 VGPRs, any hit 108 (116 with the counts); no scratch, no spills, 4 waves per SIMD
//                      (-Rpass-analysis=kernel-resource-usage)
//   k_raycast_totals   one workgroup: the sums of the partial counts
// Host waits per call: the index / finiteness check, the box, one per count of the entries (1 + the number of halvings), one more under
// knob "raycast_stats", one more under knob "raycast_timing".
#include <cmath>

#include "wave.h"
#include "cross_rule.h"
#include "pb3d_internal.h"
#include "ring_walk.h"

namespace {

constexpr i64 kMaxElems = (1ll << 31) - 1;
constexpr int kParts = 5;       // partial counts per workgroup: rays that hit, bad rays, rays missing the box, face tests, cells visited

// (__host__ too: a host program can run the very walk of the kernel, ray by ray, against an index it builds itself)
__host__ __device__ __forceinline__ double sel3(int k, double a0, double a1, double a2) { return k == 0 ? a0 : (k == 1 ? a1 : a2); }
__host__ __device__ __forceinline__ int sel3(int k, int a0, int a1, int a2) { return k == 0 ? a0 : (k == 1 ? a1 : a2); }

// ring_walk.h's cell_of on one (permuted) axis: the same operations, so the same cell
__host__ __device__ __forceinline__ int cell_on(double lo, double inv, int n, double v) {
    return (int)fmin(fmax(floor((v - lo) * inv), 0.0), (double)(n - 1));
}

// a ray ready for the faces: the permuted origin, the shear, the three offsets into a corner row
struct Ray {
    double ox, oy, oz, Sx, Sy, Sz;
    int kx, ky, kz;
};
struct Best {
    double t, U, V, W, det;
    int face;
};
struct Counts { u64 hit, bad, out, tests, cells; };     // kParts of them, in this order

// FACE against RAY of include/pb3d.h, the one place it is evaluated here; r: the face's nine corner values
__host__ __device__ __forceinline__ void try_face(const double* __restrict__ r, int f, const Ray& y, double t_min, double t_max, Best* best) {
    const double Ax = r[y.kx] - y.ox, Ay = r[y.ky] - y.oy, Az = r[y.kz] - y.oz;
    const double Bx = r[3 + y.kx] - y.ox, By = r[3 + y.ky] - y.oy, Bz = r[3 + y.kz] - y.oz;
    const double Cx = r[6 + y.kx] - y.ox, Cy = r[6 + y.ky] - y.oy, Cz = r[6 + y.kz] - y.oz;
    const double ax = Ax - y.Sx * Az, ay = Ay - y.Sy * Az;
    const double bx = Bx - y.Sx * Bz, by = By - y.Sy * Bz;
    const double cx = Cx - y.Sx * Cz, cy = Cy - y.Sy * Cz;
    const double U = cx * by - cy * bx, V = ax * cy - ay * cx, W = bx * ay - by * ax;
    const double det = (U + V) + W;
    const double T = (U * (y.Sz * Az) + V * (y.Sz * Bz)) + W * (y.Sz * Cz);
    const double t = T / det;
    const bool neg = U < 0.0 || V < 0.0 || W < 0.0, pos = U > 0.0 || V > 0.0 || W > 0.0;
    if ((neg && pos) || !(det != 0.0 && t >= t_min && t <= t_max)) return;
    if (best->face < 0 || t < best->t || (t == best->t && f < best->face)) {
        best->t = t; best->U = U; best->V = V; best->W = W; best->det = det; best->face = f;
    }
}

// one ray (o, d) against the index: RAY, the walk and EXIT of include/pb3d.h.  start == null: a mesh without a face
template <bool ANY, bool STATS>
__host__ __device__ __forceinline__ void cast_one(const double (&o)[3], const double (&d)[3], const Grid& g, const i64* __restrict__ start,
                                                  const int* __restrict__ ids, const double* __restrict__ tri, double t_min, double t_max,
                                                  Best* best, Counts* n) {
    const auto fin = [](double v) { return fabs(v) <= 1.7976931348623157e308; };         // finite: false for an infinity and a NaN
    const bool bad = !(fin(o[0]) && fin(o[1]) && fin(o[2]) && fin(d[0]) && fin(d[1]) && fin(d[2])) || (d[0] == 0.0 && d[1] == 0.0 && d[2] == 0.0);
    if (bad) { n->bad = 1; return; }
    if (!start) { n->out = 1; return; }
    Ray y;
    y.kz = 0;
    double big = fabs(d[0]);
    if (fabs(d[1]) > big) { y.kz = 1; big = fabs(d[1]); }
    if (fabs(d[2]) > big) y.kz = 2;
    y.kx = y.kz == 2 ? 0 : y.kz + 1;
    y.ky = y.kx == 2 ? 0 : y.kx + 1;
    y.ox = sel3(y.kx, o[0], o[1], o[2]); y.oy = sel3(y.ky, o[0], o[1], o[2]); y.oz = sel3(y.kz, o[0], o[1], o[2]);
    const double dz = sel3(y.kz, d[0], d[1], d[2]);
    y.Sx = sel3(y.kx, d[0], d[1], d[2]) / dz;
    y.Sy = sel3(y.ky, d[0], d[1], d[2]) / dz;
    y.Sz = 1.0 / dz;
    // the grid as the ray sees it
    const double lox = sel3(y.kx, g.lo[0], g.lo[1], g.lo[2]), hix = sel3(y.kx, g.hi[0], g.hi[1], g.hi[2]);
    const double loy = sel3(y.ky, g.lo[0], g.lo[1], g.lo[2]), hiy = sel3(y.ky, g.hi[0], g.hi[1], g.hi[2]);
    const double loz = sel3(y.kz, g.lo[0], g.lo[1], g.lo[2]), hiz = sel3(y.kz, g.hi[0], g.hi[1], g.hi[2]);
    const double invx = sel3(y.kx, g.inv[0], g.inv[1], g.inv[2]), invy = sel3(y.ky, g.inv[0], g.inv[1], g.inv[2]);
    const double invz = sel3(y.kz, g.inv[0], g.inv[1], g.inv[2]), hz = sel3(y.kz, g.h[0], g.h[1], g.h[2]);
    const int nx = sel3(y.kx, g.n[0], g.n[1], g.n[2]), ny = sel3(y.ky, g.n[0], g.n[1], g.n[2]), nz = sel3(y.kz, g.n[0], g.n[1], g.n[2]);
    const i64 st1 = g.n[2], st0 = (i64)g.n[1] * g.n[2];         // cell_index's strides of axes 1 and 0 (axis 2: 1)
    const i64 stx = y.kx == 0 ? st0 : (y.kx == 1 ? st1 : 1), sty = y.ky == 0 ? st0 : (y.ky == 1 ? st1 : 1),
              stz = y.kz == 0 ? st0 : (y.kz == 1 ? st1 : 1);
    double big_c = fmax(fmax(fabs(o[0]), fabs(o[1])), fabs(o[2]));
#pragma unroll
    for (int a = 0; a < 3; ++a) big_c = fmax(big_c, fmax(fabs(g.lo[a]), fabs(g.hi[a])));
    const double tol = kMargin * big_c, wide = 4.0 * tol;
    // the ray's own kz range, widened, against the box
    const double zs = y.oz + t_min * dz, ze = y.oz + t_max * dz;
    const double rz0 = fmin(zs, ze) - tol, rz1 = fmax(zs, ze) + tol;
    bool walked = false;
    if (rz1 >= loz && rz0 <= hiz) {
        const int c0 = cell_on(loz, invz, nz, rz0), c1 = cell_on(loz, invz, nz, rz1);
        const bool up = dz > 0.0;
        int iz = up ? c0 : c1;
#pragma nounroll
        for (int layer = c0; layer <= c1; ++layer, iz += up ? 1 : -1) {
            const double pa = iz == 0 ? loz : loz + (double)iz * hz;
            const double pb = iz == nz - 1 ? hiz : loz + (double)(iz + 1) * hz;
            const double za = fmax(pa, rz0) - y.oz, zb = fmin(pb, rz1) - y.oz;
            const double xa = y.ox + y.Sx * za, xb = y.ox + y.Sx * zb;
            const double ya = y.oy + y.Sy * za, yb = y.oy + y.Sy * zb;
            const double x0 = fmin(xa, xb) - wide, x1 = fmax(xa, xb) + wide;
            const double y0 = fmin(ya, yb) - wide, y1 = fmax(ya, yb) + wide;
            if (!(x1 < lox || x0 > hix || y1 < loy || y0 > hiy)) {
                walked = true;
                const int ix0 = cell_on(lox, invx, nx, x0), ix1 = cell_on(lox, invx, nx, x1);
                const int iy0 = cell_on(loy, invy, ny, y0), iy1 = cell_on(loy, invy, ny, y1);
                for (int ix = ix0; ix <= ix1; ++ix)
                    for (int iy = iy0; iy <= iy1; ++iy) {
                        const i64 c = ix * stx + iy * sty + iz * stz;
                        const i64 e = start[c + 1];
                        if (STATS) { ++n->cells; n->tests += (u64)(e - start[c]); }
#pragma nounroll
                        for (i64 p = start[c]; p < e; ++p) {
                            const int f = ids[p];
                            try_face(tri + 9 * (i64)f, f, y, t_min, t_max, best);
                        }
                    }
            }
            if (best->face >= 0) {
                if (ANY) break;
                const double t_far = ((up ? pb : pa) - y.oz) * y.Sz;
                if (best->t < t_far - (2.0 * tol * fabs(y.Sz) + 1e-12 * fabs(t_far))) break;
            }
        }
    }
    if (!walked) n->out = 1;
    n->hit = best->face >= 0;
}

// partials (STATS): per workgroup kParts counts
template <bool RF64, bool ANY, bool STATS>
__global__ __launch_bounds__(256) void k_raycast(const void* __restrict__ org, const void* __restrict__ dir, i64 n, Grid g,
                                                 const i64* __restrict__ start, const int* __restrict__ ids, const double* __restrict__ tri,
                                                 double t_min, double t_max, double* __restrict__ out_t, int* __restrict__ out_face,
                                                 double* __restrict__ out_bary, u8* __restrict__ out_hit, u64* __restrict__ partials) {
    const i64 s = (i64)blockIdx.x * 256 + threadIdx.x;
    Counts cnt = {0, 0, 0, 0, 0};
    if (s < n) {
        double o[3], d[3];
        pb3d_load3<RF64>(org, s, o);
        pb3d_load3<RF64>(dir, s, d);
        Best best = {INFINITY, 0.0, 0.0, 0.0, 1.0, -1};
        cast_one<ANY, STATS>(o, d, g, start, ids, tri, t_min, t_max, &best, &cnt);
        if (ANY) {
            out_hit[s] = (u8)(best.face >= 0);
        } else {
            out_t[s] = best.t;
            out_face[s] = best.face;
            if (out_bary) {
                const bool h = best.face >= 0;
                out_bary[3 * s] = h ? best.U / best.det : 0.0;
                out_bary[3 * s + 1] = h ? best.V / best.det : 0.0;
                out_bary[3 * s + 2] = h ? best.W / best.det : 0.0;
            }
        }
    }
    if (STATS) {
        __shared__ u64 w[kParts][4];
        u64* dst = partials + kParts * (i64)blockIdx.x;
        group_total<4>(wave_sum(cnt.hit), w[0], [&](u64 t) { dst[0] = t; });
        group_total<4>(wave_sum(cnt.bad), w[1], [&](u64 t) { dst[1] = t; });
        group_total<4>(wave_sum(cnt.out), w[2], [&](u64 t) { dst[2] = t; });
        group_total<4>(wave_sum(cnt.tests), w[3], [&](u64 t) { dst[3] = t; });
        group_total<4>(wave_sum(cnt.cells), w[4], [&](u64 t) { dst[4] = t; });
    }
}

// one workgroup: stats[k] = the sum of the nb workgroups' partial counts k
__global__ __launch_bounds__(1024) void k_raycast_totals(const u64* __restrict__ partials, i64 nb, u64* __restrict__ stats) {
    __shared__ u64 w[16];
    for (int k = 0; k < kParts; ++k) {
        u64 a = 0;
        for (i64 i = threadIdx.x; i < nb; i += 1024) a += partials[kParts * i + k];
        group_total<16>(wave_sum(a), w, [&](u64 t) { stats[k] = t; });
        __syncthreads();
    }
}

// ix: null for a mesh without a face
template <bool RF64>
void launch_query(pb3d_ctx* ctx, unsigned nb, const void* d_o, const void* d_d, i64 n, const pb3d_face_index* ix, double t_min, double t_max,
                  int any_hit, double* d_t, int* d_face, double* d_bary, u8* d_hit, u64* partials) {
    const Grid g = ix ? ix->g : Grid{};
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(nb), dim3(256), 0, ctx->stream, d_o, d_d, n, g, ix ? ix->starts : nullptr, ix ? ix->ids : nullptr,
                           ix ? ix->tri : nullptr, t_min, t_max, d_t, d_face, d_bary, d_hit, partials);
    };
    if (any_hit && partials) go(k_raycast<RF64, true, true>);
    else if (any_hit) go(k_raycast<RF64, true, false>);
    else if (partials) go(k_raycast<RF64, false, true>);
    else go(k_raycast<RF64, false, false>);
}

}  // namespace

extern "C" {

int pb3d_cast_rays_resident(pb3d_ctx* ctx, const void* d_origins, const void* d_dirs, int rays_f64, int64_t nrays, const void* d_verts,
                            int verts_f64, int64_t nv, const void* d_faces, int faces_i64, int64_t nf, double t_min, double t_max, int any_hit,
                            double* d_t, int32_t* d_face, double* d_bary, uint8_t* d_hit) {
    PB3D_REQUIRE(nrays >= 0 && nv >= 0 && nf >= 0, "pb3d_cast_rays: negative count");
    PB3D_REQUIRE(nrays <= kMaxElems && nv <= kMaxElems && nf <= kMaxElems, "pb3d_cast_rays: at most 2^31 - 1 rays, vertices and faces");
    PB3D_REQUIRE(std::isfinite(t_min) && t_min <= t_max, "pb3d_cast_rays: need t_min finite and t_min <= t_max (got %g, %g)", t_min, t_max);
    if (any_hit) {
        PB3D_REQUIRE(d_t == nullptr && d_face == nullptr && d_bary == nullptr,
                     "pb3d_cast_rays: any-hit mode writes d_hit alone; d_t, d_face and d_bary must be NULL");
        PB3D_REQUIRE(nrays == 0 || d_hit != nullptr, "pb3d_cast_rays: null buffer");
    } else {
        PB3D_REQUIRE(d_hit == nullptr, "pb3d_cast_rays: d_hit belongs to the any-hit mode and must be NULL");
        PB3D_REQUIRE(nrays == 0 || (d_t != nullptr && d_face != nullptr), "pb3d_cast_rays: null buffer");
        PB3D_REQUIRE((uintptr_t)d_t % 8 == 0 && (uintptr_t)d_bary % 8 == 0 && (uintptr_t)d_face % 4 == 0, "pb3d_cast_rays: misaligned output");
    }
    PB3D_REQUIRE((nrays == 0 || (d_origins && d_dirs)) && (nv == 0 || d_verts) && (nf == 0 || d_faces), "pb3d_cast_rays: null buffer");
    PB3D_REQUIRE((uintptr_t)d_origins % (rays_f64 ? 8 : 4) == 0 && (uintptr_t)d_dirs % (rays_f64 ? 8 : 4) == 0, "pb3d_cast_rays: misaligned rays");
    PB3D_REQUIRE(ctx != nullptr, "pb3d_cast_rays: null context");

    void* rb;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_RAYCAST_READBACK, 8 * sizeof(u64), &rb));
    if (nv > 0 || nf > 0) PB3D_TRY(check_mesh(ctx, "pb3d_cast_rays", d_verts, verts_f64, nv, d_faces, faces_i64, nf, (u32*)((u64*)rb + 7)));
    ctx->raycast_last = {false, false, {0.0f, 0.0f}, {0, 0, 0, 0, 0, 0}};
    const bool counted = ctx->tune_raycast_stats != 0;       // knob "raycast_stats"
    if (nrays == 0) {
        ctx->raycast_last.counted = counted;
        return PB3D_OK;
    }

    pb3d_stamps<3> t = {ctx->tune_raycast_timing != 0, 0, {}};       // knob "raycast_timing"
    PB3D_TRY(t.mark(ctx));
    pb3d_face_index ix;
    if (nf > 0) {
        const pb3d_face_index_slots slots = {PB3D_SLOT_RAYCAST_CORNERS, PB3D_SLOT_RAYCAST_READBACK, PB3D_SLOT_RAYCAST_COUNTS,
                                             PB3D_SLOT_RAYCAST_STARTS, PB3D_SLOT_RAYCAST_IDS, PB3D_SLOT_RAYCAST_SCAN_LOCAL,
                                             PB3D_SLOT_RAYCAST_SCAN_SEGS};
        PB3D_TRY(pb3d_face_index_build(ctx, "pb3d_cast_rays", d_verts, verts_f64, nv, d_faces, faces_i64, nf, 3, false, nullptr, slots, &ix));
    }
    PB3D_TRY(t.mark(ctx));
    const unsigned nb = (unsigned)((nrays + 255) / 256);
    void *pt = nullptr, *sv = nullptr;
    if (counted) {
        PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_RAYCAST_PARTIALS, (size_t)nb * kParts * sizeof(u64), &pt));
        PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_RAYCAST_STATS, 6 * sizeof(u64), &sv));
    }
    if (rays_f64) launch_query<true>(ctx, nb, d_origins, d_dirs, nrays, nf > 0 ? &ix : nullptr, t_min, t_max, any_hit, d_t, (int*)d_face, d_bary, d_hit, (u64*)pt);
    else launch_query<false>(ctx, nb, d_origins, d_dirs, nrays, nf > 0 ? &ix : nullptr, t_min, t_max, any_hit, d_t, (int*)d_face, d_bary, d_hit, (u64*)pt);
    PB3D_CHECK_LAUNCH();
    if (counted) {
        hipLaunchKernelGGL(k_raycast_totals, dim3(1), dim3(1024), 0, ctx->stream, (const u64*)pt, (i64)nb, (u64*)sv);
        PB3D_CHECK_LAUNCH();
    }
    PB3D_TRY(t.mark(ctx));
    if (counted) {
        PB3D_TRY(pb3d_read_back(ctx, ctx->raycast_last.stats, sv, kParts * sizeof(i64)));
        ctx->raycast_last.stats[5] = nf > 0 ? ix.entries : 0;
        ctx->raycast_last.counted = true;
    }
    return t.finish(ctx, ctx->raycast_last.ms, &ctx->raycast_last.timed);
}

int pb3d_cast_rays_last(const pb3d_ctx* ctx, int64_t stats[6]) {
    PB3D_REQUIRE(ctx != nullptr && stats != nullptr, "pb3d_cast_rays_last: null argument");
    PB3D_REQUIRE(ctx->raycast_last.counted, "pb3d_cast_rays_last: the last ray cast was not counted (knob raycast_stats)");
    for (int i = 0; i < 6; ++i) stats[i] = ctx->raycast_last.stats[i];
    return PB3D_OK;
}

int pb3d_cast_rays_last_ms(const pb3d_ctx* ctx, double ms[2]) {
    PB3D_REQUIRE(ctx != nullptr && ms != nullptr, "pb3d_cast_rays_last_ms: null argument");
    PB3D_REQUIRE(ctx->raycast_last.timed, "pb3d_cast_rays_last_ms: the last ray cast was not timed (knob raycast_timing)");
    for (int i = 0; i < 2; ++i) ms[i] = ctx->raycast_last.ms[i];
    return PB3D_OK;
}

}  // extern "C"
