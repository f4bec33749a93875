// Binary marching cubes + nearest-filled-voxel colours: meshify_colored_voxel_grid
// (reference utils/voxel_utils.py:53-96).
//
// The reference meshes mask = any(grid[::s,::s,::s] > 0, -1) with skimage's Lewiner marching cubes at
// level 0.5.  With 0/1 corners the triangles of a cube depend only on its 8 corner bits: the case table
// (mc_binary_table.inc) is read off scikit-image by tools/gen_mc_table.py.  Output order is skimage's
// serial order:
//   * an edge vertex belongs to the lowest-scan-order cube (a0, a1, a2) that contains its edge; a cube
//     owns local edge (axis, p, q) iff on each of the two other axes the offset is 1 or the cube sits at
//     index 0; the centre vertex (id 12) is always the cube's own;
//   * a cube creates its owned vertices in the order its triangle list first references them
//     (MC_ORDER); vertices and faces follow cube scan order, faces in table order.
// Normals: skimage adds, for every reference of a vertex by a face, a gradient taken from the 8 corners
// of the referencing cube, and normalises the sum in double at the end.  For binary corners every
// contribution is a small integer vector, so the sum is exact whatever its order: a per-vertex gather
// over the (up to 4) cubes sharing the edge reproduces skimage's float32 normals bit for bit.
//
// Passes: occupancy bitmask of the lattice (rows padded to 64 bits) -> per-block vertex / face counts ->
// exclusive scans (points.hip's scan) -> vertices + per-cube vertex base -> faces -> colours.
//
// The isosurface of a float32 volume (pb3d_iso_*, reference utils/eval_helpers.py:191-195; include/pb3d.h states the rule) runs on
// the same table, ownership and order: the triangles of a cube depend only on which corners are above the level, so only the bits
// pass (k_iso_bits) and the vertex pass (k_iso_verts: interpolated edge vertices, no normals) are its own; counts, scans and faces
// are the kernels above, launched on the LatticeParams half of either parameter block.
#include <cmath>

#include "pb3d_internal.h"
#include "wave.h"

namespace {

#include "mc_binary_table.inc"

// the bit lattice: all the topology passes (counts, vertex base, faces) read
struct LatticeParams {
    i64 n0, n1, n2;      // lattice dims
    i64 m1, m2;          // cubes per axis 1, 2 (n - 1)
    i64 ncubes;
    i64 W;               // 64-bit words per lattice row
};

// ... and the uint8 grid it was taken from (meshify's bits, vertex and colour passes)
struct MeshParams : LatticeParams {
    const u8* grid;
    i64 A1, A2;          // full-resolution dims (axis 1, 2)
    int C, stride;
    float S2;            // full-resolution shape[2]
};

// ... or the float32 volume (the isosurface's bits and vertex passes)
struct IsoParams : LatticeParams {
    const float* vol;    // C-contiguous (n0, n1, n2)
    double level;
    float divisor;
};

__device__ __forceinline__ int lat_bit_row(const u64* __restrict__ row, i64 k) { return (int)((row[k >> 6] >> (k & 63)) & 1ull); }

// case bit a0*4 + a1*2 + a2 = corner (c0+a0, c1+a1, c2+a2) occupied
__device__ __forceinline__ int cube_case(const u64* __restrict__ bits, const LatticeParams& p, i64 c0, i64 c1, i64 c2) {
    int c = 0;
#pragma unroll
    for (int a0 = 0; a0 < 2; ++a0)
#pragma unroll
        for (int a1 = 0; a1 < 2; ++a1) {
            const u64* row = bits + ((c0 + a0) * p.n1 + (c1 + a1)) * p.W;
            c |= lat_bit_row(row, c2) << (a0 * 4 + a1 * 2);
            c |= lat_bit_row(row, c2 + 1) << (a0 * 4 + a1 * 2 + 1);
        }
    return c;
}

// the two axes other than ax, in increasing order
__device__ __forceinline__ void other_axes(int ax, int* oa, int* ob) {
    *oa = ax == 0 ? 1 : 0;
    *ob = ax == 2 ? 1 : 2;
}

// cube (c0,c1,c2) owns local vertex id?  z = bit a of "cube index is 0 on axis a"
__device__ __forceinline__ bool owns(int id, int zbits) {
    if (id == 12) return true;
    int oa, ob;
    other_axes(id >> 2, &oa, &ob);
    return (((id >> 1) & 1) || ((zbits >> oa) & 1)) && ((id & 1) || ((zbits >> ob) & 1));
}

__device__ __forceinline__ int owned_count(int cs, int zbits) {
    int n = 0;
    for (int k = 0; k < 13; ++k) {
        const int id = MC_ORDER[cs][k];
        if (id == 15) break;
        n += owns(id, zbits);
    }
    return n;
}

__device__ __forceinline__ int owned_rank(int cs, int zbits, int id) {
    int r = 0;
    for (int k = 0; k < 13; ++k) {
        const int e = MC_ORDER[cs][k];
        if (e == id) break;
        r += owns(e, zbits);
    }
    return r;
}

__device__ __forceinline__ int zbits_of(i64 c0, i64 c1, i64 c2) { return (c0 == 0) | ((c1 == 0) << 1) | ((c2 == 0) << 2); }

// skimage's per-reference gradient of local vertex id in a cube of case cs, returned in (a0, a1, a2) component order.
// Corner values v_L are taken in Lewiner's corner order L0..L7 = (x,y,z) (0,0,0) (1,0,0) (1,1,0) (0,1,0) (0,0,1) (1,0,1)
// (1,1,1) (0,1,1) with x = a2, y = a1, z = a0, i.e. case bits 0,1,3,2,4,5,7,6; skimage indexes its per-corner gradient
// array (vg below, components x y z) with the binary corner index a0*4 + a1*2 + a2 of the edge's two ends.
struct I3 { int z, y, x; };

__device__ __forceinline__ int vL(int cs, int i) {
    const int lb = (0x67542310 >> (4 * i)) & 0xF;   // Lewiner corner i -> case bit
    return (cs >> lb) & 1;
}

__device__ __forceinline__ I3 vg(int cs, int i) {
    const int v0 = vL(cs, 0), v1 = vL(cs, 1), v2 = vL(cs, 2), v3 = vL(cs, 3), v4 = vL(cs, 4), v5 = vL(cs, 5), v6 = vL(cs, 6),
              v7 = vL(cs, 7);
    switch (i) {
        case 0: return {v0 - v4, v0 - v3, v0 - v1};
        case 1: return {v1 - v5, v1 - v2, v0 - v1};
        case 2: return {v2 - v6, v1 - v2, v3 - v2};
        case 3: return {v3 - v7, v0 - v3, v3 - v2};
        case 4: return {v0 - v4, v4 - v7, v4 - v5};
        case 5: return {v1 - v5, v5 - v6, v4 - v5};
        case 6: return {v2 - v6, v5 - v6, v7 - v6};
        default: return {v3 - v7, v4 - v7, v7 - v6};
    }
}

__device__ __forceinline__ I3 contrib(int cs, int id) {
    if (id == 12) {
        const int v0 = vL(cs, 0), v1 = vL(cs, 1), v2 = vL(cs, 2), v3 = vL(cs, 3), v4 = vL(cs, 4), v5 = vL(cs, 5), v6 = vL(cs, 6),
                  v7 = vL(cs, 7);
        return {0, (v0 + v1 + v4 + v5) - (v2 + v3 + v6 + v7), (v0 + v1 + v2 + v3) - (v4 + v5 + v6 + v7)};
    }
    const int ax = id >> 2, p1 = (id >> 1) & 1, q1 = id & 1;
    // binary index of the edge's low end and the step to its high end
    const int i1 = ax == 0 ? p1 * 2 + q1 : ax == 1 ? p1 * 4 + q1 : p1 * 4 + q1 * 2;
    const int i2 = i1 + (ax == 0 ? 4 : ax == 1 ? 2 : 1);
    const I3 a = vg(cs, i1), b = vg(cs, i2);
    return {a.z + b.z, a.y + b.y, a.x + b.x};
}

__device__ __forceinline__ int refcount(int cs, int id) {
    int n = 0;
    const int e = MC_OFF[cs] + 3 * MC_NTRI[cs];
    for (int k = MC_OFF[cs]; k < e; ++k) n += MC_TRI[k] == id;
    return n;
}

__device__ __forceinline__ void cube_coords(const LatticeParams& p, i64 t, i64* c0, i64* c1, i64* c2) {
    *c2 = t % p.m2;
    const i64 r = t / p.m2;
    *c1 = r % p.m1;
    *c0 = r / p.m1;
}


// occupancy bitmask of the lattice: one wave per 64-bit word, bit k of row (i, j) = any channel of grid[i*s, j*s, k*s] > 0
__global__ __launch_bounds__(256) void k_mesh_bits(MeshParams p, u64* __restrict__ bits) {
    const i64 t = (i64)blockIdx.x * 256 + threadIdx.x;
    const i64 per_row = p.W * 64;
    const i64 row = t / per_row;
    const i64 k = t - row * per_row;
    bool occ = false;
    if (row < p.n0 * p.n1 && k < p.n2) {
        const i64 i = row / p.n1, j = row - i * p.n1;
        const u8* g = p.grid + (((i * p.stride) * p.A1 + j * p.stride) * p.A2 + k * p.stride) * p.C;
        for (int c = 0; c < p.C; ++c) occ |= g[c] != 0;
    }
    const u64 m = __ballot(occ);
    if ((threadIdx.x & 63) == 0 && row < p.n0 * p.n1) bits[row * p.W + (k >> 6)] = m;
}

// inside bitmask of a float32 volume: one wave per lattice row, one lattice point per lane and 64-bit word; bit k of row (i, j) =
// (double)vol[i, j, k] > level.  Rows are padded as k_mesh_bits pads them.  The only full read of the volume
__global__ __launch_bounds__(256) void k_iso_bits(IsoParams p, u64* __restrict__ bits) {
    const int lane = threadIdx.x & 63;
    const i64 rows = p.n0 * p.n1;
    // a capped grid whose waves stride over the rows
    for (i64 row = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (i64)gridDim.x * 4) {
        const float* __restrict__ v = p.vol + row * p.n2;
        u64* __restrict__ out = bits + row * p.W;
        // eight words per round, so that their loads are in flight together
        for (i64 w0 = 0; w0 < p.W; w0 += 8) {
            bool in[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                // k >= n2 in the row's padding and in the words past the row's last: those lanes load the row's last value, so that no
                // load sits behind a branch and all eight are issued before the first is waited for
                const i64 k = (w0 + u) * 64 + lane;
                const float x = v[k < p.n2 ? k : p.n2 - 1];
                in[u] = k < p.n2 && (double)x > p.level;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const u64 m = __ballot(in[u]);
                if (lane == 0 && w0 + u < p.W) out[w0 + u] = m;
            }
        }
    }
}

// per block of 256 cubes: owned vertices and triangles
__global__ __launch_bounds__(256) void k_mesh_count(LatticeParams p, const u64* __restrict__ bits, u32* __restrict__ vcount,
                                                    u32* __restrict__ fcount) {
    __shared__ u32 wsum[4];
    const i64 t = (i64)blockIdx.x * 256 + threadIdx.x;
    u32 nv = 0, nf = 0;
    if (t < p.ncubes) {
        i64 c0, c1, c2;
        cube_coords(p, t, &c0, &c1, &c2);
        const int cs = cube_case(bits, p, c0, c1, c2);
        nf = MC_NTRI[cs];
        if (nf) nv = owned_count(cs, zbits_of(c0, c1, c2));
    }
    u32 tv, tf;
    (void)group_excl_scan<256>(nv, wsum, &tv);
    (void)group_excl_scan<256>(nf, wsum, &tf);
    if (threadIdx.x == 0) { vcount[blockIdx.x] = tv; fcount[blockIdx.x] = tf; }
}

// owned vertices (position, normal) and each cube's first vertex index
__global__ __launch_bounds__(256) void k_mesh_verts(MeshParams p, const u64* __restrict__ bits, const i64* __restrict__ voff,
                                                    int* __restrict__ vbase, float* __restrict__ verts, float* __restrict__ normals) {
    __shared__ u32 wsum[4];
    const i64 t = (i64)blockIdx.x * 256 + threadIdx.x;
    i64 c0 = 0, c1 = 0, c2 = 0;
    int cs = 0, zb = 0;
    u32 nv = 0;
    if (t < p.ncubes) {
        cube_coords(p, t, &c0, &c1, &c2);
        cs = cube_case(bits, p, c0, c1, c2);
        zb = zbits_of(c0, c1, c2);
        if (MC_NTRI[cs]) nv = owned_count(cs, zb);
    }
    u32 tot;
    const u32 before = group_excl_scan<256>(nv, wsum, &tot);
    if (t >= p.ncubes) return;
    const i64 base = voff[blockIdx.x] + before;
    vbase[t] = (int)base;
    if (!nv) return;
    const i64 m0 = p.n0 - 1;
    const float s = (float)p.stride;
    i64 vi = base;
    for (int k = 0; k < 13; ++k) {
        const int id = MC_ORDER[cs][k];
        if (id == 15) break;
        if (!owns(id, zb)) continue;
        float x0, x1, x2;   // skimage's vertex (a0, a1, a2)
        int gz = 0, gy = 0, gx = 0;
        if (id == 12) {
            x0 = (float)c0 + 0.5f; x1 = (float)c1 + 0.5f; x2 = (float)c2 + 0.5f;
            const int r = refcount(cs, 12);
            const I3 g = contrib(cs, 12);
            gz = r * g.z; gy = r * g.y; gx = r * g.x;
        } else {
            const int ax = id >> 2, p1 = (id >> 1) & 1, q1 = id & 1;
            x0 = ax == 0 ? (float)c0 + 0.5f : (float)(c0 + p1);
            x1 = ax == 1 ? (float)c1 + 0.5f : (float)(c1 + (ax == 0 ? p1 : q1));
            x2 = ax == 2 ? (float)c2 + 0.5f : (float)(c2 + q1);
            // every cube that holds the edge adds (references of the edge) x (its gradient)
            for (int dp = 0; dp < 2; ++dp)
                for (int dq = 0; dq < 2; ++dq) {
                    const i64 e0 = ax == 0 ? c0 : c0 + p1 - dp;
                    const i64 e1 = ax == 1 ? c1 : ax == 0 ? c1 + p1 - dp : c1 + q1 - dq;
                    const i64 e2 = ax == 2 ? c2 : c2 + q1 - dq;
                    if (e0 < 0 || e0 >= m0 || e1 < 0 || e1 >= p.m1 || e2 < 0 || e2 >= p.m2) continue;
                    const int cs2 = cube_case(bits, p, e0, e1, e2);
                    const int id2 = 4 * ax + 2 * dp + dq;
                    const int r = refcount(cs2, id2);
                    if (!r) continue;
                    const I3 g = contrib(cs2, id2);
                    gz += r * g.z; gy += r * g.y; gx += r * g.x;
                }
        }
        // reference transform (utils/voxel_utils.py:76-85): (s*a2, s*a1, S2 - s*a0)
        float* v = verts + 3 * vi;
        v[0] = s * x2;
        v[1] = s * x1;
        v[2] = p.S2 - s * x0;
        const double dz = gz, dy = gy, dx = gx;
        const double l2 = (dz * dz + dy * dy) + dx * dx;
        float* nrm = normals + 3 * vi;
        if (l2 > 0.0) {
            const double l = sqrt(l2);
            nrm[0] = (float)(dz / l);
            nrm[1] = (float)(dy / l);
            nrm[2] = (float)(dx / l);
        } else {
            nrm[0] = nrm[1] = nrm[2] = 0.0f;
        }
        ++vi;
    }
}

// the isosurface's owned vertices and each cube's first vertex index: k_mesh_verts' ownership walk.  An edge vertex between lattice
// points a (the lower index on the edge's axis) and b sits at ia + t on that axis, t = (level - va) / (vb - va) in float64 (three
// operations, each rounded once; this file is built without contraction), rounded to float32 once; the centre vertex stays at the
// cube centre.  Every coordinate is then divided by the divisor in float32, correctly rounded (include/pb3d.h states the rule)
__global__ __launch_bounds__(256) void k_iso_verts(IsoParams p, const u64* __restrict__ bits, const i64* __restrict__ voff,
                                                   int* __restrict__ vbase, float* __restrict__ verts) {
    __shared__ u32 wsum[4];
    const i64 t = (i64)blockIdx.x * 256 + threadIdx.x;
    i64 c0 = 0, c1 = 0, c2 = 0;
    int cs = 0, zb = 0;
    u32 nv = 0;
    if (t < p.ncubes) {
        cube_coords(p, t, &c0, &c1, &c2);
        cs = cube_case(bits, p, c0, c1, c2);
        zb = zbits_of(c0, c1, c2);
        if (MC_NTRI[cs]) nv = owned_count(cs, zb);
    }
    u32 tot;
    const u32 before = group_excl_scan<256>(nv, wsum, &tot);
    if (!nv) return;        // the cubes past the last one too
    // k_mesh_faces uses the base of a cube only for a vertex that cube owns (its own, or the owner's of a shared edge): the cubes that own
    // nothing, nearly all of a density volume, write none
    const i64 base = voff[blockIdx.x] + before;
    vbase[t] = (int)base;
    i64 vi = base;
    for (int k = 0; k < 13; ++k) {
        const int id = MC_ORDER[cs][k];
        if (id == 15) break;
        if (!owns(id, zb)) continue;
        float x0, x1, x2;   // (a0, a1, a2) in lattice units
        if (id == 12) {
            x0 = (float)c0 + 0.5f; x1 = (float)c1 + 0.5f; x2 = (float)c2 + 0.5f;
        } else {
            const int ax = id >> 2, p1 = (id >> 1) & 1, q1 = id & 1;
            // the edge's low end; its high end is one step further on axis ax
            const i64 a0 = ax == 0 ? c0 : c0 + p1;
            const i64 a1 = ax == 1 ? c1 : c1 + (ax == 0 ? p1 : q1);
            const i64 a2 = ax == 2 ? c2 : c2 + q1;
            const i64 ia = (a0 * p.n1 + a1) * p.n2 + a2;
            const i64 step = ax == 0 ? p.n1 * p.n2 : ax == 1 ? p.n2 : 1;
            const double va = (double)p.vol[ia], vb = (double)p.vol[ia + step];
            const double num = p.level - va, den = vb - va;
            const double tt = num / den;
            const float along = (float)((double)(ax == 0 ? a0 : ax == 1 ? a1 : a2) + tt);
            x0 = ax == 0 ? along : (float)a0;
            x1 = ax == 1 ? along : (float)a1;
            x2 = ax == 2 ? along : (float)a2;
        }
        float* v = verts + 3 * vi;
        v[0] = __fdiv_rn(x0, p.divisor);
        v[1] = __fdiv_rn(x1, p.divisor);
        v[2] = __fdiv_rn(x2, p.divisor);
        ++vi;
    }
}

// triangles: a reference to a vertex of an earlier cube resolves to that cube's vertex base + the vertex's rank there
__global__ __launch_bounds__(256) void k_mesh_faces(LatticeParams p, const u64* __restrict__ bits, const i64* __restrict__ foff,
                                                    const int* __restrict__ vbase, int* __restrict__ faces) {
    __shared__ u32 wsum[4];
    const i64 t = (i64)blockIdx.x * 256 + threadIdx.x;
    i64 c[3] = {0, 0, 0};
    int cs = 0;
    u32 nf = 0;
    if (t < p.ncubes) {
        cube_coords(p, t, &c[0], &c[1], &c[2]);
        cs = cube_case(bits, p, c[0], c[1], c[2]);
        nf = MC_NTRI[cs];
    }
    u32 tot;
    const u32 before = group_excl_scan<256>(nf, wsum, &tot);
    if (!nf) return;
    const int zb = zbits_of(c[0], c[1], c[2]);
    const int mybase = vbase[t];
    int* f = faces + 3 * (foff[blockIdx.x] + before);
    const int e = MC_OFF[cs] + 3 * (int)nf;
    for (int k = MC_OFF[cs]; k < e; ++k) {
        const int id = MC_TRI[k];
        int vi;
        if (owns(id, zb)) {
            vi = mybase + owned_rank(cs, zb, id);
        } else {
            // owner: one step back on each of the two other axes where the offset is 0 (and the cube is not at 0)
            const int ax = id >> 2, p1 = (id >> 1) & 1, q1 = id & 1;
            // the other two axes (oa, ob) in increasing order: (1,2), (0,2), (0,1)
            const i64 ca = ax == 0 ? c[1] : c[0], cb = ax == 2 ? c[1] : c[2];
            const int sa = !p1 && ca > 0, sb = !q1 && cb > 0;
            const int id2 = id | (sa << 1) | sb;
            const i64 o0 = ax == 0 ? c[0] : c[0] - sa;
            const i64 o1 = ax == 0 ? c[1] - sa : ax == 1 ? c[1] : c[1] - sb;
            const i64 o2 = ax == 2 ? c[2] : c[2] - sb;
            const i64 ot = (o0 * p.m1 + o1) * p.m2 + o2;
            const int ocs = cube_case(bits, p, o0, o1, o2);
            vi = vbase[ot] + owned_rank(ocs, zbits_of(o0, o1, o2), id2);
        }
        f[k - MC_OFF[cs]] = vi;
    }
}

// nearest occupied lattice point of ((S2 - s*a0)/s, a1, a2) (the reference's query verts[:, [2,1,0]] / stride in float32, then
// float64): rows (i, j) in Chebyshev rings around the query's clamped cell, the nearest set bit of each row found word-wise.
// Rows of ring rho >= 1 lie at least (rho - 1/2)^2 + out^2 away (out = the query's distance to the grid box on axis 0; axes 1, 2
// are inside by construction).  Squared distances are exact in float64; ties go to the smallest lattice index.
__global__ __launch_bounds__(256) void k_mesh_colors(MeshParams p, const u64* __restrict__ bits, const float* __restrict__ verts,
                                                     i64 nverts, u8* __restrict__ cols) {
    const i64 v = (i64)blockIdx.x * 256 + threadIdx.x;
    if (v >= nverts) return;
    const float s = (float)p.stride;
    const double q0 = (double)__fdiv_rn(verts[3 * v + 2], s);
    const double q1 = (double)__fdiv_rn(verts[3 * v + 1], s);
    const double q2 = (double)__fdiv_rn(verts[3 * v + 0], s);
    i64 ci = (i64)floor(q0 + 0.5);
    ci = ci < 0 ? 0 : ci > p.n0 - 1 ? p.n0 - 1 : ci;
    i64 cj = (i64)floor(q1 + 0.5);
    cj = cj < 0 ? 0 : cj > p.n1 - 1 ? p.n1 - 1 : cj;
    const double out0 = q0 < 0.0 ? -q0 : q0 > (double)(p.n0 - 1) ? q0 - (double)(p.n0 - 1) : 0.0;
    const double O = out0 * out0;
    const i64 kf = (i64)floor(q2);   // 0 <= q2 <= n2 - 1
    double best = INFINITY;
    i64 bi = 0, bj = 0, bk = 0;
    const i64 rmax = p.n0 > p.n1 ? p.n0 : p.n1;
    for (i64 rho = 0; rho <= rmax; ++rho) {
        if (rho > 0) {
            const double lb = ((double)rho - 0.5) * ((double)rho - 0.5) + O;
            if (lb > best) break;
        }
        for (i64 i = ci - rho; i <= ci + rho; ++i) {
            if (i < 0 || i >= p.n0) continue;
            const bool edge_i = (i == ci - rho) || (i == ci + rho);
            const i64 jstep = edge_i ? 1 : 2 * rho;
            for (i64 j = cj - rho; j <= cj + rho; j += (jstep > 0 ? jstep : 1)) {
                if (j < 0 || j >= p.n1) continue;
                const double di = q0 - (double)i, dj = q1 - (double)j;
                const double rowd = di * di + dj * dj;
                if (rowd > best) continue;
                const u64* row = bits + (i * p.n1 + j) * p.W;
                // how far along the row a point can still tie or win
                const double room = best - rowd;
                const i64 lim = room == INFINITY ? p.n2 : (i64)sqrt(room) + 1;
                // largest set k <= kf
                i64 kL = -1;
                {
                    i64 w = kf >> 6;
                    u64 m = row[w] & (((kf & 63) == 63) ? ~0ull : ((2ull << (kf & 63)) - 1));
                    const i64 wstop = (kf - lim) < 0 ? 0 : ((kf - lim) >> 6);
                    while (true) {
                        if (m) { kL = w * 64 + 63 - __clzll(m); break; }
                        if (w <= wstop) break;
                        --w;
                        m = row[w];
                    }
                }
                // smallest set k > kf
                i64 kR = -1;
                if (kf + 1 < p.n2) {
                    const i64 k1 = kf + 1;
                    i64 w = k1 >> 6;
                    u64 m = row[w] & (~0ull << (k1 & 63));
                    const i64 wlast = p.W - 1;
                    const i64 wstop0 = (k1 + lim) >> 6;
                    const i64 wstop = wstop0 < wlast ? wstop0 : wlast;
                    while (true) {
                        if (m) { kR = w * 64 + __ffsll((long long)m) - 1; break; }
                        if (w >= wstop) break;
                        ++w;
                        m = row[w];
                    }
                    if (kR >= p.n2) kR = -1;
                }
                for (int side = 0; side < 2; ++side) {
                    const i64 k = side ? kR : kL;
                    if (k < 0) continue;
                    const double dk = q2 - (double)k;
                    const double d = rowd + dk * dk;
                    const bool better = d < best || (d == best && ((i * p.n1 + j) * p.n2 + k) < ((bi * p.n1 + bj) * p.n2 + bk));
                    if (better) { best = d; bi = i; bj = j; bk = k; }
                }
            }
        }
    }
    const u8* g = p.grid + (((bi * p.stride) * p.A1 + bj * p.stride) * p.A2 + bk * p.stride) * p.C;
    for (int ch = 0; ch < p.C; ++ch) cols[v * p.C + ch] = g[ch];
}

// cubes and words of a lattice whose n0, n1, n2 are set
void finish_lattice(LatticeParams* p) {
    p->m1 = p->n1 - 1; p->m2 = p->n2 - 1;
    p->ncubes = (p->n0 - 1) * p->m1 * p->m2;
    p->W = (p->n2 + 63) / 64;
}

int make_mesh_params(const u8* d_grid, i64 A0, i64 A1, i64 A2, int C, int stride, MeshParams* p) {
    PB3D_REQUIRE(A0 >= 0 && A1 >= 0 && A2 >= 0 && (C == 1 || C == 3), "pb3d_mesh: bad shape");
    PB3D_REQUIRE(stride >= 1, "pb3d_mesh: stride must be >= 1");
    p->grid = d_grid;
    p->A1 = A1; p->A2 = A2; p->C = C; p->stride = stride;
    p->n0 = (A0 + stride - 1) / stride;
    p->n1 = (A1 + stride - 1) / stride;
    p->n2 = (A2 + stride - 1) / stride;
    PB3D_REQUIRE(p->n0 >= 2 && p->n1 >= 2 && p->n2 >= 2, "pb3d_mesh: Input array must be at least 2x2x2.");
    PB3D_REQUIRE(A2 < (1 << 24), "pb3d_mesh: shape[2] must be < 2^24");
    finish_lattice(p);
    p->S2 = (float)A2;
    PB3D_REQUIRE(d_grid != nullptr, "pb3d_mesh: null grid");
    return PB3D_OK;
}

int make_iso_params(const float* d_vol, i64 n0, i64 n1, i64 n2, double level, float divisor, IsoParams* p) {
    PB3D_REQUIRE(n0 >= 2 && n1 >= 2 && n2 >= 2, "pb3d_iso: Input array must be at least 2x2x2.");
    PB3D_REQUIRE(n0 < (1 << 24) && n1 < (1 << 24) && n2 < (1 << 24), "pb3d_iso: every axis must be < 2^24");
    PB3D_REQUIRE(std::isfinite(level), "pb3d_iso: level must be finite");
    PB3D_REQUIRE(std::isfinite(divisor) && divisor > 0.0f, "pb3d_iso: divisor must be finite and > 0 (got %g)", (double)divisor);
    PB3D_REQUIRE(d_vol != nullptr, "pb3d_iso: null volume");
    p->n0 = n0; p->n1 = n1; p->n2 = n2;
    finish_lattice(p);
    p->vol = d_vol; p->level = level; p->divisor = divisor;
    return PB3D_OK;
}

pb3d_ctx::IsoArgs iso_args(const void* vol, i64 n0, i64 n1, i64 n2, double level, float divisor, i64 nv, i64 nf) {
    u64 lb;
    u32 db;
    memcpy(&lb, &level, sizeof lb);
    memcpy(&db, &divisor, sizeof db);
    return pb3d_ctx::IsoArgs{vol, n0, n1, n2, nv, nf, lb, db};
}

// the passes' time stamps of an isosurface count or fill (knob "iso_timing"): two passes each; each half clears its *_timed flag first
using IsoStamps = pb3d_stamps<3>;

// bitmask of the lattice into PB3D_SLOT_MESH_BITS
int build_bits(pb3d_ctx* ctx, const MeshParams& p, u64** bits) {
    void* b;
    const i64 rows = p.n0 * p.n1;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_MESH_BITS, (size_t)(rows * p.W) * sizeof(u64), &b));
    const i64 threads = rows * p.W * 64;
    hipLaunchKernelGGL(k_mesh_bits, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, ctx->stream, p, (u64*)b);
    PB3D_CHECK_LAUNCH();
    *bits = (u64*)b;
    return PB3D_OK;
}

// The topology of a bit lattice, shared by meshify and the isosurface: per-block vertex and face counts, their two scans into
// PB3D_SLOT_MESH_VERT_OFFSETS / _FACE_OFFSETS, and the two totals after the call's one host wait
int count_lattice(pb3d_ctx* ctx, const LatticeParams& p, const u64* bits, const char* who, i64 tot[2], IsoStamps* stamps = nullptr) {
    const i64 nb = (p.ncubes + 255) / 256;
    void *vc, *fc, *vo, *fo;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_MESH_VERT_COUNTS, (size_t)nb * sizeof(u32), &vc));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_MESH_FACE_COUNTS, (size_t)nb * sizeof(u32), &fc));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_MESH_VERT_OFFSETS, (size_t)(nb + 1) * sizeof(i64), &vo));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_MESH_FACE_OFFSETS, (size_t)(nb + 1) * sizeof(i64), &fo));
    hipLaunchKernelGGL(k_mesh_count, dim3((unsigned)nb), dim3(256), 0, ctx->stream, p, bits, (u32*)vc, (u32*)fc);
    PB3D_CHECK_LAUNCH();
    PB3D_TRY(pb3d_scan_counts(ctx, (const u32*)vc, nb, (i64*)vo, PB3D_SLOT_MESH_VSCAN_LOCAL, PB3D_SLOT_MESH_VSCAN_SEGS));
    PB3D_TRY(pb3d_scan_counts(ctx, (const u32*)fc, nb, (i64*)fo, PB3D_SLOT_MESH_FSCAN_LOCAL, PB3D_SLOT_MESH_FSCAN_SEGS));
    if (stamps) PB3D_TRY(stamps->mark(ctx));
    PB3D_HIP(hipMemcpyAsync(&tot[0], (i64*)vo + nb, sizeof(i64), hipMemcpyDeviceToHost, ctx->stream));
    PB3D_HIP(hipMemcpyAsync(&tot[1], (i64*)fo + nb, sizeof(i64), hipMemcpyDeviceToHost, ctx->stream));
    PB3D_TRY(pb3d_stream_sync(ctx));
    PB3D_REQUIRE(tot[0] < (1ll << 31) && tot[1] < (1ll << 31), "%s: %lld vertices / %lld faces: int32 faces need < 2^31", who,
                 (long long)tot[0], (long long)tot[1]);
    return PB3D_OK;
}

// what a fill reads of its count: the bit lattice and the two offset arrays, still at least as large as this lattice needs
int counted_lattice(const pb3d_ctx* ctx, const LatticeParams& p, const char* fill, const char* count, const u64** bits) {
    const i64 nb = (p.ncubes + 255) / 256;
    const size_t bits_bytes = (size_t)(p.n0 * p.n1 * p.W) * sizeof(u64);
    PB3D_REQUIRE(ctx->scratch[PB3D_SLOT_MESH_BITS] && ctx->scratch_bytes[PB3D_SLOT_MESH_BITS] >= bits_bytes &&
                     ctx->scratch[PB3D_SLOT_MESH_VERT_OFFSETS] && ctx->scratch_bytes[PB3D_SLOT_MESH_VERT_OFFSETS] >= (size_t)(nb + 1) * sizeof(i64) &&
                     ctx->scratch[PB3D_SLOT_MESH_FACE_OFFSETS] && ctx->scratch_bytes[PB3D_SLOT_MESH_FACE_OFFSETS] >= (size_t)(nb + 1) * sizeof(i64),
                 "%s: call %s on the same grid first", fill, count);
    *bits = (const u64*)ctx->scratch[PB3D_SLOT_MESH_BITS];
    return PB3D_OK;
}

// the faces of a counted lattice whose vertex pass has written the per-cube vertex base
int fill_faces(pb3d_ctx* ctx, const LatticeParams& p, const u64* bits, const int* vbase, int32_t* d_faces) {
    hipLaunchKernelGGL(k_mesh_faces, dim3((unsigned)((p.ncubes + 255) / 256)), dim3(256), 0, ctx->stream, p, bits,
                       (const i64*)ctx->scratch[PB3D_SLOT_MESH_FACE_OFFSETS], vbase, (int*)d_faces);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

}  // namespace

extern "C" {

int pb3d_mesh_count_dev(pb3d_ctx* ctx, const uint8_t* d_grid, int64_t A0, int64_t A1, int64_t A2, int C, int stride,
                        int64_t* nverts, int64_t* nfaces) {
    PB3D_REQUIRE(ctx != nullptr && nverts != nullptr && nfaces != nullptr, "pb3d_mesh_count: null argument");
    ctx->mesh_dev.pair.valid = false;
    *nverts = *nfaces = 0;
    MeshParams p;
    PB3D_TRY(make_mesh_params(d_grid, A0, A1, A2, C, stride, &p));
    const i64 nb = (p.ncubes + 255) / 256;
    PB3D_REQUIRE(nb < (1ll << 31) && (p.n0 * p.n1 * p.W * 64 + 255) / 256 < (1ll << 31), "pb3d_mesh_count: grid too large");
    u64* bits;
    PB3D_TRY(build_bits(ctx, p, &bits));
    i64 tot[2];
    PB3D_TRY(count_lattice(ctx, p, bits, "pb3d_mesh_count", tot));
    *nverts = tot[0];
    *nfaces = tot[1];
    ctx->mesh_dev.a = pb3d_ctx::MeshArgs{d_grid, A0, A1, A2, tot[0], tot[1], C, stride};
    pb3d_pair_record(ctx, &ctx->mesh_dev.pair, {PB3D_SLOT_MESH_BITS, PB3D_SLOT_MESH_VERT_OFFSETS, PB3D_SLOT_MESH_FACE_OFFSETS});
    return PB3D_OK;
}

int pb3d_mesh_colors_dev(pb3d_ctx* ctx, const uint8_t* d_grid, int64_t A0, int64_t A1, int64_t A2, int C, int stride,
                         const float* d_verts, int64_t nverts, uint8_t* d_cols) {
    PB3D_REQUIRE(ctx != nullptr && nverts >= 0, "pb3d_mesh_colors: bad argument");
    MeshParams p;
    PB3D_TRY(make_mesh_params(d_grid, A0, A1, A2, C, stride, &p));
    if (nverts == 0) return PB3D_OK;
    PB3D_REQUIRE(d_verts && d_cols, "pb3d_mesh_colors: null buffer");
    PB3D_REQUIRE((nverts + 255) / 256 < (1ll << 31), "pb3d_mesh_colors: too many vertices");
    u64* bits;
    PB3D_TRY(build_bits(ctx, p, &bits));
    hipLaunchKernelGGL(k_mesh_colors, dim3((unsigned)((nverts + 255) / 256)), dim3(256), 0, ctx->stream, p, (const u64*)bits, d_verts,
                       nverts, d_cols);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

int pb3d_mesh_fill_dev(pb3d_ctx* ctx, const uint8_t* d_grid, int64_t A0, int64_t A1, int64_t A2, int C, int stride,
                       int64_t nverts, int64_t nfaces, float* d_verts, int32_t* d_faces, float* d_normals, uint8_t* d_cols) {
    PB3D_REQUIRE(ctx != nullptr, "pb3d_mesh_fill: null context");
    MeshParams p;
    PB3D_TRY(make_mesh_params(d_grid, A0, A1, A2, C, stride, &p));
    if (nverts == 0) return PB3D_OK;
    PB3D_REQUIRE(d_verts && d_faces && d_normals, "pb3d_mesh_fill: null buffer");
    PB3D_TRY(pb3d_pair_check(ctx, ctx->mesh_dev.pair,
                             pb3d_same_args(ctx->mesh_dev.a, pb3d_ctx::MeshArgs{d_grid, A0, A1, A2, nverts, nfaces, C, stride}),
                             "pb3d_mesh_fill", "pb3d_mesh_count"));
    const i64 nb = (p.ncubes + 255) / 256;
    const u64* bits;
    PB3D_TRY(counted_lattice(ctx, p, "pb3d_mesh_fill", "pb3d_mesh_count_dev", &bits));
    void* vb;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_MESH_VERT_BASE, (size_t)p.ncubes * sizeof(int), &vb));
    hipLaunchKernelGGL(k_mesh_verts, dim3((unsigned)nb), dim3(256), 0, ctx->stream, p, bits, (const i64*)ctx->scratch[PB3D_SLOT_MESH_VERT_OFFSETS],
                       (int*)vb, d_verts, d_normals);
    PB3D_CHECK_LAUNCH();
    PB3D_TRY(fill_faces(ctx, p, bits, (const int*)vb, d_faces));
    (void)nfaces;
    if (d_cols) {
        hipLaunchKernelGGL(k_mesh_colors, dim3((unsigned)((nverts + 255) / 256)), dim3(256), 0, ctx->stream, p, bits,
                           (const float*)d_verts, nverts, d_cols);
        PB3D_CHECK_LAUNCH();
    }
    return PB3D_OK;
}

}  // extern "C"

extern "C" {

int pb3d_mesh_count(pb3d_ctx* ctx, const uint8_t* grid, int64_t A0, int64_t A1, int64_t A2, int C, int stride,
                    int64_t* nverts, int64_t* nfaces) {
    PB3D_REQUIRE(ctx != nullptr && nverts != nullptr && nfaces != nullptr, "pb3d_mesh_count: null argument");
    PB3D_REQUIRE(A0 >= 0 && A1 >= 0 && A2 >= 0 && (C == 1 || C == 3) && stride >= 1, "pb3d_mesh_count: bad shape");
    ctx->mesh.pair.valid = false;
    const size_t nb = (size_t)(A0 * A1 * A2 * C);
    PB3D_REQUIRE(grid != nullptr || nb == 0, "pb3d_mesh_count: null grid");
    void* dg = nullptr;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_HOST_IN0, nb ? nb : 1, &dg));
    if (nb) PB3D_HIP(hipMemcpyAsync(dg, grid, nb, hipMemcpyHostToDevice, ctx->stream));
    PB3D_TRY(pb3d_mesh_count_dev(ctx, (const u8*)dg, A0, A1, A2, C, stride, nverts, nfaces));
    ctx->mesh.a = pb3d_ctx::MeshArgs{dg, A0, A1, A2, *nverts, *nfaces, C, stride};
    pb3d_pair_record(ctx, &ctx->mesh.pair, {PB3D_SLOT_HOST_IN0});
    return PB3D_OK;
}

// the device fill checks the device pair that pb3d_mesh_count ran
int pb3d_mesh_fill(pb3d_ctx* ctx, int64_t nverts, int64_t nfaces, float* verts, int32_t* faces, float* normals, uint8_t* cols) {
    PB3D_REQUIRE(ctx != nullptr, "pb3d_mesh_fill: null context");
    const pb3d_ctx::MeshArgs& a = ctx->mesh.a;
    PB3D_TRY(pb3d_pair_check(ctx, ctx->mesh.pair, true, "pb3d_mesh_fill", "pb3d_mesh_count"));
    PB3D_REQUIRE(nverts == a.nv && nfaces == a.nf, "pb3d_mesh_fill: sizes do not match the count");
    ctx->mesh.pair.valid = false;
    if (nverts == 0) return PB3D_OK;
    PB3D_REQUIRE(verts && faces && normals, "pb3d_mesh_fill: null buffer");
    const int C = (int)a.C;
    void *dv, *df, *dn, *dc = nullptr;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_HOST_OUT0, (size_t)nverts * 3 * sizeof(float), &dv));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_HOST_OUT1, (size_t)nfaces * 3 * sizeof(int32_t), &df));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_HOST_OUT2, (size_t)nverts * 3 * sizeof(float), &dn));
    if (cols) PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_MESH_HOST_COLS, (size_t)nverts * C, &dc));
    PB3D_TRY(pb3d_mesh_fill_dev(ctx, (const u8*)a.grid, a.A0, a.A1, a.A2, C, (int)a.stride, nverts, nfaces, (float*)dv, (int32_t*)df, (float*)dn,
                                (u8*)dc));
    PB3D_HIP(hipMemcpyAsync(verts, dv, (size_t)nverts * 3 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    PB3D_HIP(hipMemcpyAsync(faces, df, (size_t)nfaces * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    PB3D_HIP(hipMemcpyAsync(normals, dn, (size_t)nverts * 3 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (cols) PB3D_HIP(hipMemcpyAsync(cols, dc, (size_t)nverts * C, hipMemcpyDeviceToHost, ctx->stream));
    return pb3d_stream_sync(ctx);
}

}  // extern "C"

// ---- isosurface of a float32 volume (include/pb3d.h states the rule): the bits and vertex passes of its own, meshify's topology ----
extern "C" {

int pb3d_iso_count_resident(pb3d_ctx* ctx, const float* d_vol, int64_t n0, int64_t n1, int64_t n2, double level, float divisor,
                       int64_t* nverts, int64_t* nfaces) {
    PB3D_REQUIRE(nverts != nullptr && nfaces != nullptr, "pb3d_iso_count: null argument");
    *nverts = *nfaces = 0;
    IsoParams p;
    PB3D_TRY(make_iso_params(d_vol, n0, n1, n2, level, divisor, &p));
    PB3D_REQUIRE(ctx != nullptr, "pb3d_iso_count: null context");
    ctx->iso_dev.pair.valid = false;
    ctx->iso_last.count_timed = ctx->iso_last.fill_timed = false;
    const i64 nb = (p.ncubes + 255) / 256, rows = p.n0 * p.n1;
    PB3D_REQUIRE(nb < (1ll << 31), "pb3d_iso_count: volume too large");
    void* b;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_MESH_BITS, (size_t)(rows * p.W) * sizeof(u64), &b));
    IsoStamps st = {ctx->tune_iso_timing != 0, 0, {}};
    PB3D_TRY(st.mark(ctx));
    hipLaunchKernelGGL(k_iso_bits, dim3(pb3d_stream_blocks(ctx, rows, 4, 16)), dim3(256), 0, ctx->stream, p, (u64*)b);
    PB3D_CHECK_LAUNCH();
    PB3D_TRY(st.mark(ctx));
    i64 tot[2];
    PB3D_TRY(count_lattice(ctx, p, (const u64*)b, "pb3d_iso_count", tot, &st));
    PB3D_TRY(st.read(&ctx->iso_last.ms[0], &ctx->iso_last.count_timed));
    *nverts = tot[0];
    *nfaces = tot[1];
    ctx->iso_dev.a = iso_args(d_vol, n0, n1, n2, level, divisor, tot[0], tot[1]);
    pb3d_pair_record(ctx, &ctx->iso_dev.pair, {PB3D_SLOT_MESH_BITS, PB3D_SLOT_MESH_VERT_OFFSETS, PB3D_SLOT_MESH_FACE_OFFSETS});
    return PB3D_OK;
}

int pb3d_iso_fill_resident(pb3d_ctx* ctx, const float* d_vol, int64_t n0, int64_t n1, int64_t n2, double level, float divisor,
                      int64_t nverts, int64_t nfaces, float* d_verts, int32_t* d_faces) {
    IsoParams p;
    PB3D_TRY(make_iso_params(d_vol, n0, n1, n2, level, divisor, &p));
    PB3D_REQUIRE(nverts >= 0 && nfaces >= 0, "pb3d_iso_fill: negative size");
    PB3D_REQUIRE(ctx != nullptr, "pb3d_iso_fill: null context");
    PB3D_TRY(pb3d_pair_check(ctx, ctx->iso_dev.pair, pb3d_same_args(ctx->iso_dev.a, iso_args(d_vol, n0, n1, n2, level, divisor, nverts, nfaces)),
                             "pb3d_iso_fill", "pb3d_iso_count"));
    if (nverts == 0) return PB3D_OK;      // a counted mesh without vertices has no faces
    PB3D_REQUIRE(d_verts && d_faces, "pb3d_iso_fill: null buffer");
    const i64 nb = (p.ncubes + 255) / 256;
    const u64* bits;
    PB3D_TRY(counted_lattice(ctx, p, "pb3d_iso_fill", "pb3d_iso_count_resident", &bits));
    void* vb;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_MESH_VERT_BASE, (size_t)p.ncubes * sizeof(int), &vb));
    ctx->iso_last.fill_timed = false;
    IsoStamps st = {ctx->tune_iso_timing != 0, 0, {}};
    PB3D_TRY(st.mark(ctx));
    hipLaunchKernelGGL(k_iso_verts, dim3((unsigned)nb), dim3(256), 0, ctx->stream, p, bits, (const i64*)ctx->scratch[PB3D_SLOT_MESH_VERT_OFFSETS],
                       (int*)vb, d_verts);
    PB3D_CHECK_LAUNCH();
    PB3D_TRY(st.mark(ctx));
    PB3D_TRY(fill_faces(ctx, p, bits, (const int*)vb, d_faces));
    PB3D_TRY(st.mark(ctx));
    return st.finish(ctx, &ctx->iso_last.ms[2], &ctx->iso_last.fill_timed);
}

int pb3d_iso_last(pb3d_ctx* ctx, double pass_ms[4]) {
    PB3D_REQUIRE(ctx != nullptr && pass_ms != nullptr, "pb3d_iso_last: null argument");
    PB3D_REQUIRE(ctx->iso_last.count_timed && ctx->iso_last.fill_timed,
                 "pb3d_iso_last: the last isosurface count and fill were not both timed (knob iso_timing)");
    for (int i = 0; i < 4; ++i) pass_ms[i] = ctx->iso_last.ms[i];
    return PB3D_OK;
}

int pb3d_iso_count(pb3d_ctx* ctx, const float* vol, int64_t n0, int64_t n1, int64_t n2, double level, float divisor, int64_t* nverts,
                   int64_t* nfaces) {
    PB3D_REQUIRE(nverts != nullptr && nfaces != nullptr, "pb3d_iso_count: null argument");
    *nverts = *nfaces = 0;
    IsoParams p;
    PB3D_TRY(make_iso_params(vol, n0, n1, n2, level, divisor, &p));
    PB3D_REQUIRE(ctx != nullptr, "pb3d_iso_count: null context");
    ctx->iso.pair.valid = false;
    const size_t bytes = (size_t)(n0 * n1 * n2) * sizeof(float);
    void* dv = nullptr;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_HOST_IN0, bytes, &dv));
    PB3D_HIP(hipMemcpyAsync(dv, vol, bytes, hipMemcpyHostToDevice, ctx->stream));
    PB3D_TRY(pb3d_iso_count_resident(ctx, (const float*)dv, n0, n1, n2, level, divisor, nverts, nfaces));
    ctx->iso.a = iso_args(dv, n0, n1, n2, level, divisor, *nverts, *nfaces);
    pb3d_pair_record(ctx, &ctx->iso.pair, {PB3D_SLOT_HOST_IN0});
    return PB3D_OK;
}

// the device fill checks the device pair that pb3d_iso_count ran
int pb3d_iso_fill(pb3d_ctx* ctx, int64_t nverts, int64_t nfaces, float* verts, int32_t* faces) {
    PB3D_REQUIRE(ctx != nullptr, "pb3d_iso_fill: null context");
    const pb3d_ctx::IsoArgs& a = ctx->iso.a;
    PB3D_TRY(pb3d_pair_check(ctx, ctx->iso.pair, true, "pb3d_iso_fill", "pb3d_iso_count"));
    PB3D_REQUIRE(nverts == a.nv && nfaces == a.nf, "pb3d_iso_fill: sizes do not match the count");
    ctx->iso.pair.valid = false;
    if (nverts == 0) return PB3D_OK;
    PB3D_REQUIRE(verts && faces, "pb3d_iso_fill: null buffer");
    double level;
    float divisor;
    const u32 db = (u32)a.divisor_bits;
    memcpy(&level, &a.level_bits, sizeof level);
    memcpy(&divisor, &db, sizeof divisor);
    void *dv, *df;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_HOST_OUT0, (size_t)nverts * 3 * sizeof(float), &dv));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_HOST_OUT1, (size_t)nfaces * 3 * sizeof(int32_t), &df));
    PB3D_TRY(pb3d_iso_fill_resident(ctx, (const float*)a.vol, a.n0, a.n1, a.n2, level, divisor, nverts, nfaces, (float*)dv, (int32_t*)df));
    PB3D_HIP(hipMemcpyAsync(verts, dv, (size_t)nverts * 3 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    PB3D_HIP(hipMemcpyAsync(faces, df, (size_t)nfaces * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    return pb3d_stream_sync(ctx);
}

}  // extern "C"
