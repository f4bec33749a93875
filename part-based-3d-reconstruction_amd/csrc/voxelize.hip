// voxelize_mesh: exact solid voxelization of a triangle mesh by crossing parity, and the overlap counts of two resident grids
// (include/pb3d.h has the rules to the bit; DESIGN.md "Mesh to grid" has the passes and their times).
//
// The bit volume holds, per column (i, j) of the grid, W = ceil(n2 / 32) + 1 dwords: bit k of the column is bit k & 31 of dword k >> 5,
// and bit 0 of the last dword is the column's overflow bit (crossings above the grid).
//   k_check_mesh      (csrc/cross_rule.h, with the rule itself: csrc/inside.hip asks the same of arbitrary query points) one sweep
//                     over the face indices and the vertex coordinates: bit 0 of the flag = an index outside [-nv, nv),
//                     bit 1 = a coordinate that is not finite.  The entry's one host wait in front of everything that gathers
//   k_cross_lanes     one lane per face: lattice coordinates, area, column box, the three edge set-ups and the plane, in registers.
//                     A face of at most kLaneCols columns (every marching-cubes face) is walked by its lane; a larger one is listed
//   k_cross_groups    one workgroup per listed face, its threads striding over the face's columns (a CAD wall covers the grid).  The
//                     set-up is computed again from the three vertices -- about sixty float64 operations, once per face and thread,
//                     never per column -- so nothing per face is stored but the list
//                     A crossing is one atomicXor of one bit: integer, commutative, so the bits are a function of the input alone
//   k_scan_expand     per column the prefix XOR: inside a dword by shifts 1, 2, 4, 8, 16, across the column's dwords by a ballot of
//                     the dwords' parities (columns of up to 64 dwords share a wavefront; a longer one takes a wavefront and a carry);
//                     then the bytes along a2: 16 voxels per lane in 16-byte stores where n2 is a multiple of 16 and the output is
//                     16-byte aligned, else 64 consecutive bytes per store instruction whatever the channel count; it counts the
//                     occupied voxels and the open columns on the way
//   k_overlap         the three counts of pb3d_grid_overlap_resident in one sweep
// Counts are integer atomics, one per workgroup of a capped grid.  No floating-point atomics anywhere.
#include <algorithm>
#include <cmath>

#include "wave.h"
#include "cross_rule.h"
#include "mesh_index.h"
#include "pb3d_internal.h"

namespace {

constexpr i64 kMaxElems = (1ll << 31) - 1;
constexpr int kLaneCols = 16;                       // above it a face's columns are walked by a workgroup

struct Vol { u32* bits; i64 n0, n1, n2, W; };
struct Frame { double o[3], vs, depth; int meshify; };

// what a face needs per column: the shared record of csrc/cross_rule.h and the face's columns
struct Face : CrossFace {
    int i0, i1, j0, j1;                             // the column box, inclusive; i1 < i0 or j1 < j0: no column
};

template <bool VF64>
__device__ __forceinline__ void lattice(const void* verts, i64 v, const Frame& fr, double L[3]) {
    double p[3];
    pb3d_load3<VF64>(verts, v, p);
    const double a0 = fr.meshify ? fr.depth - p[2] : p[0], a2 = fr.meshify ? p[0] : p[2];
    L[0] = __ddiv_rn(a0 - fr.o[0], fr.vs);
    L[1] = __ddiv_rn(p[1] - fr.o[1], fr.vs);
    L[2] = __ddiv_rn(a2 - fr.o[2], fr.vs);
}

// false: area == 0, the face contributes nothing
template <bool VF64, bool I64>
__device__ __forceinline__ bool face_setup(const void* verts, i64 nv, const void* faces, i64 f, const Frame& fr, const Vol& v, Face* o) {
    double A[3], B[3], C[3];
    lattice<VF64>(verts, wrap(load_index<I64>(faces, 3 * f), nv), fr, A);
    lattice<VF64>(verts, wrap(load_index<I64>(faces, 3 * f + 1), nv), fr, B);
    lattice<VF64>(verts, wrap(load_index<I64>(faces, 3 * f + 2), nv), fr, C);
    const double area = cross_area(A, B, C);
    if (area == 0.0) return false;
    // clamped in float64 first: the conversions below see values in [0, n - 1] (or an empty range)
    const double ilo = fmax(0.0, ceil(fmin(fmin(A[0], B[0]), C[0]))), ihi = fmin((double)(v.n0 - 1), floor(fmax(fmax(A[0], B[0]), C[0])));
    const double jlo = fmax(0.0, ceil(fmin(fmin(A[1], B[1]), C[1]))), jhi = fmin((double)(v.n1 - 1), floor(fmax(fmax(A[1], B[1]), C[1])));
    const bool some = ilo <= ihi && jlo <= jhi;
    o->i0 = some ? (int)ilo : 0; o->i1 = some ? (int)ihi : -1;
    o->j0 = some ? (int)jlo : 0; o->j1 = some ? (int)jhi : -1;
    cross_edges(A, B, C, area, o);
    cross_plane(A, B, C, o);
    return true;
}

// column (i, j) of the face's box: if the face crosses it, flip the crossing's bit.  i and j are inside the grid (the box is clamped),
// k is clamped below and sent to the overflow bit above: no store leaves the column's W dwords
__device__ __forceinline__ u32 cross_column(const Face& f, int i, int j, const Vol& v) {
    const double x = (double)i, y = (double)j;
    if (!cross_covers(f, x, y)) return 0;
    const double kz = ceil(cross_height(f, x, y));
    u32* col = v.bits + ((i64)i * v.n1 + j) * v.W;
    if (kz <= (double)(v.n2 - 1)) {
        const int k = (int)fmax(kz, 0.0);
        atomicXor(col + (k >> 5), 1u << (k & 31));
    } else {
        atomicXor(col + (v.W - 1), 1u);         // above the grid (or no height at all: a NaN compares false)
    }
    return 1;
}

// stats: crossings, occupied, open columns, flat faces.  large[0] = listed faces (zeroed before), large[1 ...] = their numbers, in
// whatever order the integer atomics give: each is walked on its own
template <bool VF64, bool I64>
__global__ __launch_bounds__(256) void k_cross_lanes(const void* __restrict__ verts, i64 nv, const void* __restrict__ faces, i64 nf, Frame fr, Vol v,
                                                     u32* __restrict__ large, u64* __restrict__ stats) {
    u64 crossings = 0, flat = 0;
    for (i64 f = (i64)blockIdx.x * 256 + threadIdx.x; f < nf; f += (i64)gridDim.x * 256) {
        Face s;
        if (!face_setup<VF64, I64>(verts, nv, faces, f, fr, v, &s)) {
            ++flat;
        } else {
            const i64 ncols = (i64)(s.i1 - s.i0 + 1) * (s.j1 - s.j0 + 1);
            if (ncols > kLaneCols) {
                large[1 + atomicAdd(&large[0], 1u)] = (u32)f;
            } else if (ncols > 0) {
                for (int i = s.i0; i <= s.i1; ++i)
                    for (int j = s.j0; j <= s.j1; ++j) crossings += cross_column(s, i, j, v);
            }
        }
    }
    group_add(crossings, &stats[0]);
    group_add(flat, &stats[3]);
}

template <bool VF64, bool I64>
__global__ __launch_bounds__(256) void k_cross_groups(const void* __restrict__ verts, i64 nv, const void* __restrict__ faces, Frame fr, Vol v,
                                                      const u32* __restrict__ large, u64* __restrict__ stats) {
    const u32 nlarge = large[0];
    u64 crossings = 0;
    for (u32 h = blockIdx.x; h < nlarge; h += gridDim.x) {
        Face s;
        face_setup<VF64, I64>(verts, nv, faces, (i64)large[1 + h], fr, v, &s);      // listed: it has an area
        const u32 nj = (u32)(s.j1 - s.j0 + 1), ncols = (u32)(s.i1 - s.i0 + 1) * nj;    // <= n0 * n1 < 2^31
        for (u32 c = threadIdx.x; c < ncols; c += 256) {
            const u32 q = c / nj;
            crossings += cross_column(s, s.i0 + (int)q, s.j0 + (int)(c - q * nj), v);
        }
    }
    group_add(crossings, &stats[0]);
}

// the bytes of 16 voxels (bit b of bits16 = voxel b is inside) in one, or three, 16-byte stores; p is 16-byte aligned
template <int CH>
__device__ __forceinline__ void store16(u8* p, u32 bits16, u32 value) {
    if (CH == 1) {
        // a nibble's four bits to the low bits of four bytes (the shifted copies never meet), times the byte
        uint4 q;
        q.x = (((bits16 & 15u) * 0x00204081u) & 0x01010101u) * value;
        q.y = ((((bits16 >> 4) & 15u) * 0x00204081u) & 0x01010101u) * value;
        q.z = ((((bits16 >> 8) & 15u) * 0x00204081u) & 0x01010101u) * value;
        q.w = (((bits16 >> 12) * 0x00204081u) & 0x01010101u) * value;
        *(uint4*)p = q;
    } else {
        u32 d[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int m = 0; m < 48; ++m) d[m >> 2] |= ((0u - ((bits16 >> (m / 3)) & 1u)) & ((value >> (8 * (m % 3))) & 0xffu)) << (8 * (m & 3));
        ((uint4*)p)[0] = make_uint4(d[0], d[1], d[2], d[3]);
        ((uint4*)p)[1] = make_uint4(d[4], d[5], d[6], d[7]);
        ((uint4*)p)[2] = make_uint4(d[8], d[9], d[10], d[11]);
    }
}

// A wavefront takes a unit a time: cpw whole columns of span = Wd dwords each (Wd <= 64), or one column 64 dwords a time (Wd > 64,
// cpw = 1), so a column never straddles two wavefronts.  sp = the magic of span.  value: the channels' bytes, channel c in bits 8c ...
// WIDE (n2 a multiple of 16 and out 16-byte aligned: 16 voxels never cross a column's end, and their bytes start on a 16-byte
// boundary): a lane stores 16 voxels a time.  Otherwise 64 consecutive bytes per store instruction, one per lane
struct Scan { const u32* bits; i64 ncol, n2, W; pb3d_magic sp; int cpw; u32 value; u8* out; };

// the columns col0 .. col0 + cpw - 1; every lane of the wavefront calls it with the same col0
template <int CH, bool WIDE>
__device__ __forceinline__ void scan_unit(const Scan& a, i64 col0, u64* occupied, u64* open) {
    const int lane = threadIdx.x & 63, span = (int)a.sp.d;
    const i64 Wd = a.W - 1;
    const int sub = (int)pb3d_div((u32)lane, a.sp), wl = lane - sub * span;
    const u64 mine = ((1ull << lane) - 1) & ~((1ull << (lane - wl)) - 1);     // the lanes below me that hold my column
    const i64 col = col0 + sub;
    const bool lane_on = sub < a.cpw && col < a.ncol;
    u32 carry = 0;
    for (i64 wb = 0; wb < Wd; wb += span) {
        const i64 w = wb + wl;
        const bool on = lane_on && w < Wd;
        const u32 x = on ? a.bits[col * a.W + w] : 0u;
        u32 p = x;
        p ^= p << 1; p ^= p << 2; p ^= p << 4; p ^= p << 8; p ^= p << 16;
        const u64 par = __ballot(p >> 31);
        const u32 c = (u32)(__popcll(par & mine) & 1) ^ carry;
        const u32 full = c ? ~p : p;                // bit b: the parity of the column's crossings at bits 0 .. 32 w + b
        if (Wd > span) carry ^= (u32)(__popcll(par) & 1);
        const i64 left = a.n2 - w * 32;
        const u32 valid = !on ? 0u : left >= 32 ? ~0u : (1u << left) - 1u;
        *occupied += __popc(full & valid);
        if (on && w == Wd - 1) *open += ((full >> 31) ^ a.bits[col * a.W + Wd]) & 1u;
        if (WIDE) {
            // the chunk's 64 dwords are 128 groups of 16 voxels: group g goes to lane g & 63 in round g >> 6
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int g = r * 64 + lane, src = g >> 1, b = (g & 1) * 16;
                const u32 word = __shfl(full, src);
                const int ssub = (int)pb3d_div((u32)src, a.sp);
                const i64 scol = col0 + ssub, sw = wb + (src - ssub * span), k = sw * 32 + b;
                if (ssub < a.cpw && scol < a.ncol && sw < Wd && k < a.n2)
                    store16<CH>(a.out + (scol * a.n2 + k) * CH, (word >> b) & 0xffffu, a.value);
            }
            continue;
        }
        // the chunk's 64 dwords are 2048 voxels = 2048 CH bytes: byte slot s goes to lane s & 63 in round s >> 6
        for (int r = 0; r < 32 * CH; ++r) {
            const int s = r * 64 + lane, vox = s / CH, ch = s - vox * CH, src = vox >> 5, b = vox & 31;
            const u32 word = __shfl(full, src);
            const int ssub = (int)pb3d_div((u32)src, a.sp);
            const i64 scol = col0 + ssub, sw = wb + (src - ssub * span), k = sw * 32 + b;
            if (ssub < a.cpw && scol < a.ncol && sw < Wd && k < a.n2)
                a.out[(scol * a.n2 + k) * CH + ch] = ((word >> b) & 1u) ? (u8)(a.value >> (8 * ch)) : (u8)0;
        }
    }
}

template <int CH, bool WIDE>
__global__ __launch_bounds__(256) void k_scan_expand(Scan a, i64 units, u64* __restrict__ stats) {
    u64 occupied = 0, open = 0;
    for (i64 unit = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); unit < units; unit += (i64)gridDim.x * 4)
        scan_unit<CH, WIDE>(a, unit * a.cpw, &occupied, &open);
    group_add(occupied, &stats[1]);
    group_add(open, &stats[2]);
}

template <int CH>
__device__ __forceinline__ bool occupied_at(const u8* g, i64 v) {
    if (CH == 1) return g[v] != 0;
    const u8* p = g + 3 * v;
    return (p[0] | p[1] | p[2]) != 0;
}

// counts: both, a, b
template <int CA, int CB>
__global__ __launch_bounds__(256) void k_overlap(const u8* __restrict__ a, const u8* __restrict__ b, i64 nvox, u64* __restrict__ counts) {
    u64 both = 0, na = 0, nb = 0;
    for (i64 v = (i64)blockIdx.x * 256 + threadIdx.x; v < nvox; v += (i64)gridDim.x * 256) {
        const bool ia = occupied_at<CA>(a, v), ib = occupied_at<CB>(b, v);
        both += ia && ib; na += ia; nb += ib;
    }
    group_add(both, &counts[0]);
    group_add(na, &counts[1]);
    group_add(nb, &counts[2]);
}

}  // namespace

extern "C" {

int pb3d_voxelize_mesh_resident(pb3d_ctx* ctx, const void* d_verts, int verts_f64, int64_t nv, const void* d_faces, int faces_i64, int64_t nf,
                                int64_t n0, int64_t n1, int64_t n2, const double origin[3], double voxel_size, int frame, double depth,
                                int channels, const uint8_t* value, uint8_t* d_out, int64_t stats[4]) {
    PB3D_REQUIRE(nv >= 0 && nf >= 0, "pb3d_voxelize_mesh: negative count");
    PB3D_REQUIRE(nv <= kMaxElems && nf <= kMaxElems / 3, "pb3d_voxelize_mesh: at most 2^31 - 1 vertices and face corners");
    PB3D_REQUIRE(n0 >= 1 && n1 >= 1 && n2 >= 1, "pb3d_voxelize_mesh: every axis of the grid must be >= 1 (got %lld x %lld x %lld)", (long long)n0,
                 (long long)n1, (long long)n2);
    PB3D_REQUIRE(n0 <= kMaxElems && n1 <= kMaxElems && n2 <= kMaxElems && n0 * n1 <= kMaxElems && n0 * n1 * n2 <= kMaxElems,
                 "pb3d_voxelize_mesh: at most 2^31 - 1 voxels");
    PB3D_REQUIRE(origin != nullptr && value != nullptr, "pb3d_voxelize_mesh: null argument");
    PB3D_REQUIRE(std::isfinite(origin[0]) && std::isfinite(origin[1]) && std::isfinite(origin[2]), "pb3d_voxelize_mesh: origin must be finite");
    PB3D_REQUIRE(std::isfinite(voxel_size) && voxel_size > 0.0, "pb3d_voxelize_mesh: voxel_size must be finite and > 0 (got %g)", voxel_size);
    PB3D_REQUIRE(frame == 0 || frame == 1, "pb3d_voxelize_mesh: frame must be 0 (lattice) or 1 (meshify), got %d", frame);
    PB3D_REQUIRE(frame == 0 || std::isfinite(depth), "pb3d_voxelize_mesh: depth must be finite");
    PB3D_REQUIRE(channels == 1 || channels == 3, "pb3d_voxelize_mesh: channels must be 1 or 3 (got %d)", channels);
    PB3D_REQUIRE((nv == 0 || d_verts) && (nf == 0 || d_faces) && d_out, "pb3d_voxelize_mesh: null buffer");
    PB3D_REQUIRE(ctx != nullptr, "pb3d_voxelize_mesh: null context");

    void *cn, *bt, *lg = nullptr;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_VOXELIZE_COUNTS, 5 * sizeof(u64), &cn));
    u64* counts = (u64*)cn;                          // the four stats, then the check's flag
    PB3D_HIP(hipMemsetAsync(cn, 0, 4 * sizeof(u64), ctx->stream));
    if (nv > 0 || nf > 0) PB3D_TRY(check_mesh(ctx, "pb3d_voxelize_mesh", d_verts, verts_f64, nv, d_faces, faces_i64, nf, (u32*)(counts + 4)));

    const i64 ncol = n0 * n1, Wd = (n2 + 31) / 32, W = Wd + 1;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_VOXELIZE_BITS, (size_t)ncol * W * sizeof(u32), &bt));
    if (nf > 0) PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_VOXELIZE_LARGE, (size_t)(nf + 1) * sizeof(u32), &lg));
    ctx->voxelize_last.valid = true;
    ctx->voxelize_last.timed = false;
    pb3d_stamps<3> t = {ctx->tune_voxelize_timing != 0, 0, {}};      // knob "voxelize_timing"
    PB3D_TRY(t.mark(ctx));
    PB3D_HIP(hipMemsetAsync(bt, 0, (size_t)ncol * W * sizeof(u32), ctx->stream));
    const Vol vol = {(u32*)bt, n0, n1, n2, W};
    if (nf > 0) {
        Frame fr = {{origin[0], origin[1], origin[2]}, voxel_size, frame ? depth : 0.0, frame};
        PB3D_HIP(hipMemsetAsync(lg, 0, sizeof(u32), ctx->stream));
        const unsigned groups = pb3d_stream_blocks(ctx, nf, 1, 8);
        with_mesh_types(verts_f64, faces_i64, [&](auto V, auto I) {
            constexpr bool VF = decltype(V)::value, IF = decltype(I)::value;
            hipLaunchKernelGGL((k_cross_lanes<VF, IF>), dim3(pb3d_stream_blocks(ctx, nf, 256, 16)), dim3(256), 0, ctx->stream, d_verts, (i64)nv, d_faces, (i64)nf,
                               fr, vol, (u32*)lg, counts);
            hipLaunchKernelGGL((k_cross_groups<VF, IF>), dim3(groups), dim3(256), 0, ctx->stream, d_verts, (i64)nv, d_faces, fr, vol, (const u32*)lg,
                               counts);
        });
        PB3D_CHECK_LAUNCH();
    }
    PB3D_TRY(t.mark(ctx));
    const int span = (int)std::min<i64>(Wd, 64), cpw = Wd <= 64 ? 64 / span : 1;
    const i64 units = (ncol + cpw - 1) / cpw;
    const dim3 grid(pb3d_stream_blocks(ctx, units, 4, 16));
    const pb3d_magic sp = pb3d_make_magic((u32)span);
    const u32 val = channels == 1 ? value[0] : (u32)value[0] | ((u32)value[1] << 8) | ((u32)value[2] << 16);
    const Scan sc = {(const u32*)bt, ncol, n2, W, sp, cpw, val, d_out};
    const bool wide = n2 % 16 == 0 && (uintptr_t)d_out % 16 == 0;
    auto scan = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(256), 0, ctx->stream, sc, units, counts); };
    if (channels == 1 && wide) scan(k_scan_expand<1, true>);
    else if (channels == 1) scan(k_scan_expand<1, false>);
    else if (wide) scan(k_scan_expand<3, true>);
    else scan(k_scan_expand<3, false>);
    PB3D_CHECK_LAUNCH();
    PB3D_TRY(t.mark(ctx));
    if (stats) PB3D_TRY(pb3d_read_back(ctx, stats, counts, 4 * sizeof(i64)));
    return t.finish(ctx, ctx->voxelize_last.ms, &ctx->voxelize_last.timed);
}

int pb3d_voxelize_last(pb3d_ctx* ctx, double pass_ms[2]) {
    PB3D_REQUIRE(ctx != nullptr && pass_ms != nullptr, "pb3d_voxelize_last: null argument");
    PB3D_REQUIRE(ctx->voxelize_last.valid, "pb3d_voxelize_last: no voxelization has run on this context");
    PB3D_REQUIRE(ctx->voxelize_last.timed, "pb3d_voxelize_last: the last voxelization was not timed (knob voxelize_timing)");
    for (int i = 0; i < 2; ++i) pass_ms[i] = ctx->voxelize_last.ms[i];
    return PB3D_OK;
}

int pb3d_grid_overlap_resident(pb3d_ctx* ctx, const uint8_t* d_a, int channels_a, const uint8_t* d_b, int channels_b, int64_t nvox, int64_t out[3]) {
    PB3D_REQUIRE(nvox >= 0, "pb3d_grid_overlap: negative count");
    PB3D_REQUIRE((channels_a == 1 || channels_a == 3) && (channels_b == 1 || channels_b == 3), "pb3d_grid_overlap: channels must be 1 or 3 (got %d and %d)",
                 channels_a, channels_b);
    PB3D_REQUIRE(out != nullptr, "pb3d_grid_overlap: null argument");
    PB3D_REQUIRE(nvox == 0 || (d_a && d_b), "pb3d_grid_overlap: null buffer");
    PB3D_REQUIRE(ctx != nullptr, "pb3d_grid_overlap: null context");
    out[0] = out[1] = out[2] = 0;
    if (nvox == 0) return PB3D_OK;
    void* cn;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_OVERLAP_COUNTS, 3 * sizeof(u64), &cn));
    PB3D_HIP(hipMemsetAsync(cn, 0, 3 * sizeof(u64), ctx->stream));
    const dim3 grid(pb3d_stream_blocks(ctx, nvox, 256, 8));
    auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(256), 0, ctx->stream, d_a, d_b, (i64)nvox, (u64*)cn); };
    if (channels_a == 1 && channels_b == 1) go(k_overlap<1, 1>);
    else if (channels_a == 1) go(k_overlap<1, 3>);
    else if (channels_b == 1) go(k_overlap<3, 1>);
    else go(k_overlap<3, 3>);
    PB3D_CHECK_LAUNCH();
    return pb3d_read_back(ctx, out, cn, 3 * sizeof(i64));
}

}  // extern "C"
