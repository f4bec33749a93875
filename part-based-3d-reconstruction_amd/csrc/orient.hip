// mesh_orient: a consistent winding for every orientable patch of a triangle mesh, the patches themselves, their edge counts and their
// ordered signed volumes (include/pb3d.h has the rules to the bit; DESIGN.md "Mesh repair" has the passes and the argument).
//
// The records in (lo, hi) order, their heads, forward bits, scans and edge starts are csrc/meshcomp.hip's (pb3d_mesh_edge_records), the
// forest is csrc/union_find.h's, the sums are mesh_components' (pb3d_mesh_ordered_sums).  What is here:
//   k_pair_unions      one lane per edge; a pair edge (c == 2) with faces a, b and disagreement d unites a ~ b + d nf and
//                      a + nf ~ b + (1 - d) nf in a forest of 2 nf nodes: node j is face j as it came, node nf + j face j flipped
//   pb3d_forest_flatten over the 2 nf entries.  r0 = root[j], r1 = root[nf + j]: the patch's smallest face is min(r0, r1), the patch is
//                      not orientable iff r0 == r1, and the anchor rule flips j iff r0 > r1
//   k_anchors          the "smallest face of its patch" flags and the anchor-rule bits; pb3d_scan_counts numbers the patches
//   k_patch_labels     patch[j]; faces and anchor-rule flips per patch (integer atomics, a few per wavefront); orientable = 0 by a plain
//                      store wherever a face finds r0 == r1
//   k_orient_edges     one lane per edge: pair, disagreeing and boundary edges per patch, and the totals
//   k_orient_records   one lane per record: the records on edges with c > 2, per patch of their face
//   pb3d_mesh_ordered_sums  with vertices: V per patch, S_j negated where the anchor rule flips
//   k_orient_decide    one lane per patch: inverted, the final volume and flip count
//   k_orient_write     one lane per face: flip = anchor bit ^ inverted, and the face row with corners 1 and 2 swapped where it is set
#include <algorithm>

#include "mesh_index.h"
#include "mesh_records.h"
#include "pb3d_internal.h"
#include "union_find.h"

namespace {

constexpr i64 kMaxVertices = (1ll << 31) - 1;
constexpr i64 kMaxFaces = ((1ll << 31) - 1) / 6;    // 2 nf forest nodes and 3 nf records are int32 / u32 with room to spare
constexpr int kCountBlocks = 4;
enum { FACES = 0, PAIRS, DISAGREE, BOUNDARY, NM_RECORDS, FLIPPED, ORIENTABLE, INVERTED, kArrays };
enum { T_PATCHES = 0, T_ORIENTABLE, T_PAIRS, T_DISAGREE, T_FLIPPED, T_INVERTED, T_BOUNDARY, T_NONMANIFOLD };

__global__ __launch_bounds__(256) void k_pair_unions(const u32* __restrict__ val, i64 R, const i64* __restrict__ head_rank, const i64* __restrict__ fwd_rank,
                                                     const u32* __restrict__ pos, int nf, int* parent) {
    const i64 E = head_rank[R];
    for (i64 e = (i64)blockIdx.x * 256 + threadIdx.x; e < E; e += (i64)gridDim.x * 256) {
        const i64 p0 = pos[e], p1 = pos[e + 1];
        if (p1 - p0 != 2) continue;
        const int a = (int)(val[p0] / 3u), b = (int)(val[p0 + 1] / 3u);
        const int d = fwd_rank[p1] - fwd_rank[p0] != 1 ? 1 : 0;
        uf_union(parent, a, b + d * nf);
        uf_union(parent, a + nf, b + (1 - d) * nf);
    }
}

__global__ __launch_bounds__(256) void k_anchors(const int* __restrict__ root, i64 nf, u32* __restrict__ anchor_flag, u32* __restrict__ flip0) {
    const i64 j = (i64)blockIdx.x * 256 + threadIdx.x;
    if (j >= nf) return;
    const int r0 = root[j], r1 = root[nf + j];
    anchor_flag[j] = (r0 < r1 ? r0 : r1) == (int)j ? 1u : 0u;
    flip0[j] = r0 > r1 ? 1u : 0u;
}

// counts[0 .. 8 np) = 0 but orientable = 1; totals: patches
__global__ __launch_bounds__(256) void k_orient_clear(unsigned long long* __restrict__ counts, const i64* __restrict__ np_ptr, unsigned long long* __restrict__ totals) {
    const i64 np = *np_ptr, n = kArrays * np;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) counts[i] = i / np == ORIENTABLE ? 1ull : 0ull;
    if (blockIdx.x == 0 && threadIdx.x == 0) totals[T_PATCHES] = (unsigned long long)np;
}

__global__ __launch_bounds__(256) void k_patch_labels(const int* __restrict__ root, i64 nf, const i64* __restrict__ rank, const u32* __restrict__ flip0,
                                                      int* __restrict__ patch, unsigned long long* counts) {
    const i64 np = rank[nf];
    RunCount faces, flipped;
    for (i64 base = wave_base(); base < nf; base += (i64)gridDim.x * 256) {
        const i64 j = base + lane_id();
        int lab = -1;
        bool fl = false;
        if (j < nf) {
            const int r0 = root[j], r1 = root[nf + j];
            lab = (int)rank[r0 < r1 ? r0 : r1];
            patch[j] = lab;
            fl = flip0[j] != 0u;
            if (r0 == r1) counts[ORIENTABLE * np + lab] = 0ull;         // every writer of the word writes 0
        }
        faces.add(counts + FACES * np, lab, true);
        flipped.add(counts + FLIPPED * np, lab, fl);
    }
    faces.flush(counts + FACES * np);
    flipped.flush(counts + FLIPPED * np);
}

__global__ __launch_bounds__(256) void k_orient_edges(const u32* __restrict__ val, i64 R, const i64* __restrict__ head_rank, const i64* __restrict__ fwd_rank,
                                                      const u32* __restrict__ pos, const int* __restrict__ patch, const i64* __restrict__ np_ptr,
                                                      unsigned long long* counts, unsigned long long* totals) {
    const i64 np = *np_ptr, E = head_rank[R];
    RunCount pairs, disagrees, boundaries;
    WaveTotal tp, td, tb, tn;
    for (i64 base = wave_base(); base < E; base += (i64)gridDim.x * 256) {
        const i64 e = base + lane_id();
        int lab = -1;
        bool pair = false, disagree = false, boundary = false, nonmanifold = false;
        if (e < E) {
            const i64 p0 = pos[e], p1 = pos[e + 1];
            const i64 c = p1 - p0, f = fwd_rank[p1] - fwd_rank[p0];
            pair = c == 2;
            disagree = pair && f != 1;
            boundary = c == 1;
            nonmanifold = c > 2;
            lab = patch[val[p0] / 3u];              // a pair edge's two faces share their patch; a boundary edge has the one face
        }
        pairs.add(counts + PAIRS * np, lab, pair);
        disagrees.add(counts + DISAGREE * np, lab, disagree);
        boundaries.add(counts + BOUNDARY * np, lab, boundary);
        tp.add(pair);
        td.add(disagree);
        tb.add(boundary);
        tn.add(nonmanifold);
    }
    pairs.flush(counts + PAIRS * np);
    disagrees.flush(counts + DISAGREE * np);
    boundaries.flush(counts + BOUNDARY * np);
    tp.flush(&totals[T_PAIRS]);
    td.flush(&totals[T_DISAGREE]);
    tb.flush(&totals[T_BOUNDARY]);
    tn.flush(&totals[T_NONMANIFOLD]);
}

// the record at sorted place p lies on edge head_rank[p] + head[p] - 1; the places from pos[E] on hold the loops
__global__ __launch_bounds__(256) void k_orient_records(const u32* __restrict__ val, i64 R, const u32* __restrict__ head, const i64* __restrict__ head_rank,
                                                        const u32* __restrict__ pos, const int* __restrict__ patch, const i64* __restrict__ np_ptr,
                                                        unsigned long long* counts) {
    const i64 np = *np_ptr, E = head_rank[R], end = pos[E];
    RunCount records;
    for (i64 base = wave_base(); base < end; base += (i64)gridDim.x * 256) {
        const i64 p = base + lane_id();
        int lab = -1;
        bool many = false;
        if (p < end) {
            const i64 e = head_rank[p] + (i64)head[p] - 1;
            many = (i64)pos[e + 1] - (i64)pos[e] > 2;
            lab = patch[val[p] / 3u];
        }
        records.add(counts + NM_RECORDS * np, lab, many);
    }
    records.flush(counts + NM_RECORDS * np);
}

// measures null: no vertices, no volume
__global__ __launch_bounds__(256) void k_orient_decide(const i64* __restrict__ np_ptr, int sign, const double* __restrict__ measures, unsigned long long* counts,
                                                       double* __restrict__ volume, unsigned long long* totals) {
    const i64 np = *np_ptr;
    WaveTotal to, ti;
    for (i64 base = wave_base(); base < np; base += (i64)gridDim.x * 256) {
        const i64 l = base + lane_id();
        bool orientable = false, inverted = false;
        if (l < np) {
            orientable = counts[ORIENTABLE * np + l] != 0ull;
            double V = measures ? measures[np + l] : 0.0;
            inverted = sign != PB3D_ORIENT_KEEP && orientable && counts[BOUNDARY * np + l] == 0ull && (sign == PB3D_ORIENT_POSITIVE ? V < 0.0 : V > 0.0);
            if (inverted) {
                V = -V;
                counts[FLIPPED * np + l] = counts[FACES * np + l] - counts[FLIPPED * np + l];
            }
            counts[INVERTED * np + l] = inverted ? 1ull : 0ull;
            if (volume) volume[l] = V;
        }
        to.add(orientable);
        ti.add(inverted);
    }
    to.flush(&totals[T_ORIENTABLE]);
    ti.flush(&totals[T_INVERTED]);
}

// out null: the bits alone.  The row goes out as it came, negative entries included
template <bool I64>
__global__ __launch_bounds__(256) void k_orient_write(const void* __restrict__ faces, i64 nf, const u32* __restrict__ flip0, const int* __restrict__ patch,
                                                      const i64* __restrict__ np_ptr, const unsigned long long* __restrict__ counts, u8* __restrict__ flip,
                                                      void* __restrict__ out, unsigned long long* totals) {
    const i64 np = *np_ptr;
    WaveTotal flipped;
    for (i64 base = wave_base(); base < nf; base += (i64)gridDim.x * 256) {
        const i64 j = base + lane_id();
        bool fl = false;
        if (j < nf) {
            fl = (flip0[j] != 0u) != (counts[INVERTED * np + patch[j]] != 0ull);
            flip[j] = fl ? 1 : 0;
            if (out) {
                const i64 a = load_index<I64>(faces, 3 * j), b = load_index<I64>(faces, 3 * j + 1), c = load_index<I64>(faces, 3 * j + 2);
                if (I64) { i64* o = (i64*)out + 3 * j; o[0] = a; o[1] = fl ? c : b; o[2] = fl ? b : c; }
                else { int* o = (int*)out + 3 * j; o[0] = (int)a; o[1] = (int)(fl ? c : b); o[2] = (int)(fl ? b : c); }
            }
        }
        flipped.add(fl);
    }
    flipped.flush(&totals[T_FLIPPED]);
}

inline dim3 grid_for(i64 n) { return dim3((unsigned)((n + 255) / 256)); }

struct Args {
    const void* verts; int verts_f64; i64 nv;
    const void* faces; int faces_i64; i64 nf;
    int sign;
    u8* flip;
    int* patch;
    void* out_faces;
    i64* counts;
    double* volume;
};

// nv >= 1, nf >= 1, checked indices.  Everything is enqueued but the read-back of the totals
int run(pb3d_ctx* ctx, const Args& s, int64_t totals[8]) {
    const i64 nf = s.nf, R = 3 * nf;
    void *pa, *fg, *rk, *ms = nullptr, *tt;
    pb3d_edge_records rec;
    PB3D_TRY(pb3d_mesh_edge_records_reserve(ctx, nf, &rec));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_ORIENT_PARENT, (size_t)nf * 2 * sizeof(int), &pa));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_ORIENT_FLAGS, (size_t)nf * 2 * sizeof(u32), &fg));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_ORIENT_RANKS, (size_t)(nf + 1) * sizeof(i64), &rk));
    if (s.verts) {
        PB3D_TRY(pb3d_mesh_ordered_sums_reserve(ctx, nf, true, 0, nullptr));
        PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_ORIENT_MEASURES, (size_t)nf * 2 * sizeof(double), &ms));
    }
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_ORIENT_TOTALS, 8 * sizeof(i64), &tt));
    int* parent = (int*)pa;
    u32 *anchor_flag = (u32*)fg, *flip0 = anchor_flag + nf;
    i64* rank = (i64*)rk;
    const i64* np = rank + nf;
    unsigned long long *tot = (unsigned long long*)tt, *counts = (unsigned long long*)s.counts;
    const unsigned count_blocks = pb3d_stream_blocks(ctx, nf, 256, kCountBlocks), edge_blocks = pb3d_stream_blocks(ctx, R, 256, kCountBlocks);

    PB3D_HIP(hipMemsetAsync(tot, 0, 8 * sizeof(i64), ctx->stream));
    PB3D_TRY(pb3d_forest_init(ctx, parent, 2 * nf));
    PB3D_TRY(pb3d_mesh_edge_records_build(ctx, s.faces, s.faces_i64, nf, s.nv, nullptr, nullptr, &rec));
    // ---- the doubled forest
    hipLaunchKernelGGL(k_pair_unions, dim3(pb3d_stream_blocks(ctx, R, 256, 0)), dim3(256), 0, ctx->stream, rec.val, R, (const i64*)rec.head_rank,
                       (const i64*)rec.fwd_rank, (const u32*)rec.pos, (int)nf, parent);
    PB3D_CHECK_LAUNCH();
    PB3D_TRY(pb3d_forest_flatten(ctx, 2 * nf, parent, nullptr));
    hipLaunchKernelGGL(k_anchors, grid_for(nf), dim3(256), 0, ctx->stream, (const int*)parent, nf, anchor_flag, flip0);
    PB3D_CHECK_LAUNCH();
    PB3D_TRY(pb3d_scan_counts(ctx, anchor_flag, nf, rank, PB3D_SLOT_MESHCOMP_SCAN_LOCAL, PB3D_SLOT_MESHCOMP_SCAN_SEGS));
    // ---- the patches and their counts
    hipLaunchKernelGGL(k_orient_clear, dim3(pb3d_stream_blocks(ctx, kArrays * nf, 256, 8)), dim3(256), 0, ctx->stream, counts, np, tot);
    PB3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_patch_labels, dim3(count_blocks), dim3(256), 0, ctx->stream, (const int*)parent, nf, (const i64*)rank, (const u32*)flip0, s.patch, counts);
    PB3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_orient_edges, dim3(edge_blocks), dim3(256), 0, ctx->stream, rec.val, R, (const i64*)rec.head_rank, (const i64*)rec.fwd_rank,
                       (const u32*)rec.pos, (const int*)s.patch, np, counts, tot);
    PB3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_orient_records, dim3(edge_blocks), dim3(256), 0, ctx->stream, rec.val, R, (const u32*)rec.head, (const i64*)rec.head_rank,
                       (const u32*)rec.pos, (const int*)s.patch, np, counts);
    PB3D_CHECK_LAUNCH();
    // ---- the signed volumes, the sign rule, the faces
    if (s.verts) PB3D_TRY(pb3d_mesh_ordered_sums(ctx, s.verts, s.verts_f64, rec, nf, s.patch, flip0, counts + FACES, np, (double*)ms));
    hipLaunchKernelGGL(k_orient_decide, dim3(count_blocks), dim3(256), 0, ctx->stream, np, s.sign, (const double*)ms, counts, s.volume, tot);
    PB3D_CHECK_LAUNCH();
    hipLaunchKernelGGL((s.faces_i64 ? k_orient_write<true> : k_orient_write<false>), dim3(count_blocks), dim3(256), 0, ctx->stream, s.faces, nf,
                       (const u32*)flip0, (const int*)s.patch, np, (const unsigned long long*)counts, s.flip, s.out_faces, tot);
    PB3D_CHECK_LAUNCH();
    i64 got[8];
    PB3D_TRY(pb3d_read_back(ctx, got, tot, sizeof(got)));
    for (int a = 0; a < 8; ++a) totals[a] = got[a];
    return PB3D_OK;
}

}  // namespace

extern "C" {

int pb3d_mesh_orient_resident(pb3d_ctx* ctx, const void* d_verts, int verts_f64, int64_t nv, const void* d_faces, int faces_i64, int64_t nf,
                              int volume_sign, uint8_t* d_flip, int32_t* d_patch, void* d_out_faces, int64_t* d_counts, double* d_volume,
                              int64_t totals[8]) {
    const char* what = "pb3d_mesh_orient";
    PB3D_REQUIRE(nv >= 0 && nf >= 0, "%s: negative count", what);
    PB3D_REQUIRE(nv <= kMaxVertices && nf <= kMaxFaces, "%s: at most 2^31 - 1 vertices and (2^31 - 1) / 6 faces", what);
    PB3D_REQUIRE(volume_sign == PB3D_ORIENT_KEEP || volume_sign == PB3D_ORIENT_POSITIVE || volume_sign == PB3D_ORIENT_NEGATIVE,
                 "%s: volume_sign must be 0 (keep), 1 (positive) or 2 (negative) (got %d)", what, volume_sign);
    PB3D_REQUIRE(totals != nullptr, "%s: null argument", what);
    PB3D_REQUIRE(volume_sign == PB3D_ORIENT_KEEP || d_verts != nullptr || nv == 0 || nf == 0, "%s: null buffer (the sign rule needs the vertices)", what);
    PB3D_REQUIRE(d_volume == nullptr || d_verts != nullptr || nv == 0 || nf == 0, "%s: null buffer (the volumes need the vertices)", what);
    PB3D_REQUIRE(nf == 0 || (d_faces && d_flip && d_patch && d_counts), "%s: null buffer", what);
    const void* outs[5] = {d_flip, d_patch, d_out_faces, d_counts, d_volume};
    for (const void* o : outs)
        PB3D_REQUIRE(nf == 0 || o == nullptr || (o != d_faces && o != d_verts), "%s: an output may not alias an input", what);
    PB3D_REQUIRE(ctx != nullptr, "%s: null context", what);
    if (nv == 0 && nf > 0) {
        pb3d_set_error("%s: index out of bounds for 0 entries", what);
        return PB3D_EINDEX;
    }
    PB3D_TRY(pb3d_check_index_range(ctx, d_faces, faces_i64, 3 * nf, -nv, nv, what));
    if (nf == 0) {                                             // no face: no patch
        for (int a = 0; a < 8; ++a) totals[a] = 0;
        return PB3D_OK;
    }
    const Args s = {d_verts, verts_f64, nv, d_faces, faces_i64, nf, volume_sign, d_flip, d_patch, d_out_faces, d_counts, d_volume};
    return run(ctx, s, totals);
}

}  // extern "C"
