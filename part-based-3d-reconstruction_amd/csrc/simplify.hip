// simplify_mesh / compact_mesh: vertex-clustering simplification of a triangle mesh, and the face tail of it on its own (include/pb3d.h
// has the rules to the bit; DESIGN.md "Mesh simplification" has the passes and their times).
//
// The clusters are voxel_downsample's voxels of the whole vertex list: pb3d_voxel_downsample_resident (csrc/downsample.hip) is called as
// it stands and leaves rows (centroid or first vertex), first[] and inv[] in this file's slots.  compact_mesh skips that: inv[i] = i.
// The face tail keeps nothing per cluster and nothing per triple, so a cluster in every face is handled like any other:
//   k_face_map        face j -> g = (inv[w0], inv[w1], inv[w2]) of its wrapped corners, in the caller's order (12 bytes a face, read by
//                     every later pass).  KEEP: keep[j] = no two equal, and a kept face marks its clusters.  DROP: the first pair of
//                     the sort, (last rotated cluster, j); a collapsed face gets the key m, which sorts behind every cluster
//   pb3d_sort_pairs   DROP only, three times (csrc/sort_pairs.hip, stable): by the last cluster of the rotated triple, the middle one,
//                     the smallest; k_next_key gathers the next key through the current permutation in between.  The positions start
//                     ascending and every pass is stable, so a run of equal triples ends up in ascending position
//   k_face_repeats    DROP only: the face at sorted place p is kept iff it is no collapsed face and its rotated triple differs from that
//                     of place p - 1 -- the first of a run is its smallest position -- and a kept face marks its clusters
//                     (plain stores of 1: every writer of a word writes the same value)
//   pb3d_scan_counts  twice: the number of kept faces before j, the number of marked clusters before k; both totals go down in the
//                     call's one read-back
//   k_vertex_gather   one lane per input vertex: inverse[i]; the first vertex of a marked cluster also writes the cluster's row, its
//                     index and its colour bytes
//   k_face_gather     a kept face writes the new numbers of its three clusters in the caller's corner order, and its position
#include <algorithm>
#include <cmath>

#include "mesh_index.h"
#include "pb3d_internal.h"

namespace {

constexpr i64 kMaxElems = (1ll << 31) - 1;

struct Tri { u32 g[3]; };

__device__ __forceinline__ Tri load_tri(const u32* __restrict__ G, i64 j) { return Tri{{G[3 * j], G[3 * j + 1], G[3 * j + 2]}}; }
__device__ __forceinline__ bool collapsed(const Tri& t) { return t.g[0] == t.g[1] || t.g[1] == t.g[2] || t.g[0] == t.g[2]; }
// the cyclic rotation that puts the smallest of three distinct clusters first
__device__ __forceinline__ Tri rotated(const Tri& t) {
    if (t.g[0] < t.g[1] && t.g[0] < t.g[2]) return t;
    if (t.g[1] < t.g[2]) return Tri{{t.g[1], t.g[2], t.g[0]}};
    return Tri{{t.g[2], t.g[0], t.g[1]}};
}
__device__ __forceinline__ void mark(u32* __restrict__ used, const Tri& t) { used[t.g[0]] = 1u; used[t.g[1]] = 1u; used[t.g[2]] = 1u; }

// inv null: every vertex its own cluster.  DROP: key / val are the sort's first pairs, keep and used are written by k_face_repeats.
// given (not with DROP): the caller's flags decide what stays, collapsed faces included
template <bool I64, bool DROP>
__global__ __launch_bounds__(256) void k_face_map(const void* __restrict__ faces, i64 nf, i64 nv, const int* __restrict__ inv, u32 m, const u8* __restrict__ given,
                                                  u32* __restrict__ G, u32* __restrict__ keep, u32* __restrict__ used, u32* __restrict__ key,
                                                  u32* __restrict__ val) {
    const i64 j = (i64)blockIdx.x * 256 + threadIdx.x;
    if (j >= nf) return;
    Tri t;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const i64 w = wrap(load_index<I64>(faces, 3 * j + a), nv);
        t.g[a] = inv ? (u32)inv[w] : (u32)w;
        G[3 * j + a] = t.g[a];
    }
    const bool dead = collapsed(t);
    if (DROP) {
        key[j] = dead ? m : rotated(t).g[2];
        val[j] = (u32)j;
    } else {
        const bool stays = given ? given[j] != 0 : !dead;
        keep[j] = stays ? 1u : 0u;
        if (stays) mark(used, t);
    }
}

// key[p] = cluster `which` of the rotated triple of the face at sorted place p
__global__ __launch_bounds__(256) void k_next_key(const u32* __restrict__ G, const u32* __restrict__ val, i64 nf, u32 m, int which, u32* __restrict__ key) {
    const i64 p = (i64)blockIdx.x * 256 + threadIdx.x;
    if (p >= nf) return;
    const Tri t = load_tri(G, (i64)val[p]);
    key[p] = collapsed(t) ? m : rotated(t).g[which];
}

__global__ __launch_bounds__(256) void k_face_repeats(const u32* __restrict__ G, const u32* __restrict__ val, i64 nf, u32* __restrict__ keep,
                                                      u32* __restrict__ used) {
    const i64 p = (i64)blockIdx.x * 256 + threadIdx.x;
    if (p >= nf) return;
    const i64 j = (i64)val[p];
    const Tri t = load_tri(G, j);
    bool stays = !collapsed(t);
    if (stays && p > 0) {
        const Tri q = load_tri(G, (i64)val[p - 1]);         // the collapsed faces are the last of the order: q is none of them
        const Tri a = rotated(t), b = rotated(q);
        stays = a.g[0] != b.g[0] || a.g[1] != b.g[1] || a.g[2] != b.g[2];
    }
    keep[j] = stays ? 1u : 0u;
    if (stays) mark(used, t);
}

__global__ void k_totals(const i64* __restrict__ vertex_total, const i64* __restrict__ face_total, i64* __restrict__ counts) {
    counts[0] = *vertex_total;
    counts[1] = *face_total;
}

// T: the vertex element type; rows are copied element by element, so no list needs more than its element's alignment.  inv / first
// null: every vertex its own cluster and rows = the vertex list.  index, inverse and colors may each be null
template <class T>
__global__ __launch_bounds__(256) void k_vertex_gather(i64 nv, const int* __restrict__ inv, const int* __restrict__ first, const u32* __restrict__ used,
                                                       const i64* __restrict__ vrank, const T* __restrict__ rows, const u8* __restrict__ colors,
                                                       int channels, T* __restrict__ out, int* __restrict__ index, int* __restrict__ inverse,
                                                       u8* __restrict__ out_colors) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    const i64 c = inv ? (i64)inv[i] : i;
    const bool stays = used[c] != 0u;
    const i64 k = vrank[c];
    if (inverse) inverse[i] = stays ? (int)k : -1;
    if (!stays || (first && (i64)first[c] != i)) return;
    for (int a = 0; a < 3; ++a) out[3 * k + a] = rows[3 * c + a];
    if (index) index[k] = (int)i;
    if (colors)
        for (int a = 0; a < channels; ++a) out_colors[channels * k + a] = colors[channels * i + a];
}

template <bool I64>
__global__ __launch_bounds__(256) void k_face_gather(i64 nf, const u32* __restrict__ G, const u32* __restrict__ keep, const i64* __restrict__ frank,
                                                     const i64* __restrict__ vrank, void* __restrict__ out, int* __restrict__ face_index) {
    const i64 j = (i64)blockIdx.x * 256 + threadIdx.x;
    if (j >= nf || !keep[j]) return;
    const i64 t = frank[j];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const i64 k = vrank[G[3 * j + a]];
        if (I64) ((i64*)out)[3 * t + a] = k;
        else ((int*)out)[3 * t + a] = (int)k;
    }
    if (face_index) face_index[t] = (int)j;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
inline dim3 grid_for(i64 n) { return dim3((unsigned)((n + 255) / 256)); }

using Stamps = pb3d_stamps<6>;      // knob "simplify_timing"

// what both entries share
struct Mesh {
    const void* verts; int verts_f64; i64 nv;
    const void* faces; int faces_i64; i64 nf;
    int duplicates;            // PB3D_FACES_DROP or PB3D_FACES_KEEP
    const u8* colors; int channels;
    void *out_verts, *out_faces;
    u8* out_colors;
    int *index, *inverse, *face_index;
    const u8* given;           // pb3d_mesh_select_faces_resident: one flag per face (with PB3D_FACES_KEEP), else null
};

int require_mesh(const char* what, const Mesh& s, const int64_t* counts) {
    PB3D_REQUIRE(s.nv >= 0 && s.nf >= 0, "%s: negative count", what);
    PB3D_REQUIRE(s.nv <= kMaxElems && s.nf <= kMaxElems, "%s: at most 2^31 - 1 vertices and 2^31 - 1 faces", what);
    PB3D_REQUIRE(s.duplicates == PB3D_FACES_DROP || s.duplicates == PB3D_FACES_KEEP, "%s: duplicate_faces must be 0 (drop) or 1 (keep) (got %d)", what, s.duplicates);
    PB3D_REQUIRE(counts != nullptr, "%s: null argument", what);
    PB3D_REQUIRE(s.colors == nullptr || s.channels == 1 || s.channels == 3, "%s: channels must be 1 or 3 (got %d)", what, s.channels);
    PB3D_REQUIRE((s.nv == 0 || s.verts) && (s.nf == 0 || s.faces), "%s: null buffer", what);
    PB3D_REQUIRE(s.nv == 0 || s.nf == 0 || (s.out_verts && s.out_faces && (s.colors == nullptr) == (s.out_colors == nullptr)), "%s: null buffer", what);
    PB3D_REQUIRE(s.nv == 0 || s.nf == 0 || (s.out_verts != s.verts && s.out_faces != s.faces), "%s: an output may not alias an input", what);
    return PB3D_OK;
}

// nv >= 1, nf >= 1, checked indices.  inv / first / rows: the clusters' (null / null / the vertex list: every vertex its own), m their
// number.  Everything is enqueued but the read-back of the two counts
int face_tail(pb3d_ctx* ctx, const Mesh& s, const int* inv, const int* first, const void* rows, i64 m, Stamps& t, int64_t counts[2]) {
    const i64 nf = s.nf, nv = s.nv;
    void *gg, *kp, *us, *fr, *vr, *cn, *kv = nullptr;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_SIMPLIFY_CORNERS, (size_t)nf * 3 * sizeof(u32), &gg));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_SIMPLIFY_KEEP, (size_t)nf * sizeof(u32), &kp));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_SIMPLIFY_USED, (size_t)m * sizeof(u32), &us));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_SIMPLIFY_FACE_RANKS, (size_t)(nf + 1) * sizeof(i64), &fr));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_SIMPLIFY_VERTEX_RANKS, (size_t)(m + 1) * sizeof(i64), &vr));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_SIMPLIFY_COUNTS, 2 * sizeof(i64), &cn));
    if (s.duplicates == PB3D_FACES_DROP) PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_SIMPLIFY_PAIRS, (size_t)nf * 4 * sizeof(u32), &kv));
    // the scans of the call are the sorts' run tables and the two flag arrays': size both scan slots for the largest now, so that none
    // regrows (and waits) midway
    PB3D_TRY(pb3d_scan_reserve(ctx, std::max<i64>(std::max<i64>(nf, m), s.duplicates == PB3D_FACES_DROP ? pb3d_sort_scan_items(nf) : 0),
                               PB3D_SLOT_SIMPLIFY_SCAN_LOCAL, PB3D_SLOT_SIMPLIFY_SCAN_SEGS));
    u32 *G = (u32*)gg, *keep = (u32*)kp, *used = (u32*)us;
    i64 *frank = (i64*)fr, *vrank = (i64*)vr;

    PB3D_HIP(hipMemsetAsync(used, 0, (size_t)m * sizeof(u32), ctx->stream));
    if (s.duplicates == PB3D_FACES_DROP) {
        u32* a = (u32*)kv;
        u32 *key = a, *val = a + nf, *key2 = a + 2 * nf, *val2 = a + 3 * nf;
        hipLaunchKernelGGL((s.faces_i64 ? k_face_map<true, true> : k_face_map<false, true>), grid_for(nf), dim3(256), 0, ctx->stream, s.faces, nf, nv, inv,
                           (u32)m, (const u8*)nullptr, G, keep, used, key, val);
        PB3D_CHECK_LAUNCH();
        PB3D_TRY(t.mark(ctx));
        for (int which = 2; which >= 0; --which) {
            if (which < 2) {
                hipLaunchKernelGGL(k_next_key, grid_for(nf), dim3(256), 0, ctx->stream, (const u32*)G, (const u32*)val, nf, (u32)m, which, key);
                PB3D_CHECK_LAUNCH();
            }
            const u32 *ks, *vs;
            PB3D_TRY(pb3d_sort_pairs(ctx, key, val, key2, val2, nf, m + 1, PB3D_SLOT_SIMPLIFY_SORT_HIST, PB3D_SLOT_SIMPLIFY_SCAN_LOCAL,
                                     PB3D_SLOT_SIMPLIFY_SCAN_SEGS, &ks, &vs));
            if (vs != val) { std::swap(key, key2); std::swap(val, val2); }     // the sorted pair is the next sort's input; its keys are spent
        }
        hipLaunchKernelGGL(k_face_repeats, grid_for(nf), dim3(256), 0, ctx->stream, (const u32*)G, (const u32*)val, nf, keep, used);
        PB3D_CHECK_LAUNCH();
    } else {
        hipLaunchKernelGGL((s.faces_i64 ? k_face_map<true, false> : k_face_map<false, false>), grid_for(nf), dim3(256), 0, ctx->stream, s.faces, nf, nv,
                           inv, (u32)m, s.given, G, keep, used, (u32*)nullptr, (u32*)nullptr);
        PB3D_CHECK_LAUNCH();
        PB3D_TRY(t.mark(ctx));
    }
    PB3D_TRY(t.mark(ctx));
    PB3D_TRY(pb3d_scan_counts(ctx, keep, nf, frank, PB3D_SLOT_SIMPLIFY_SCAN_LOCAL, PB3D_SLOT_SIMPLIFY_SCAN_SEGS));
    PB3D_TRY(pb3d_scan_counts(ctx, used, m, vrank, PB3D_SLOT_SIMPLIFY_SCAN_LOCAL, PB3D_SLOT_SIMPLIFY_SCAN_SEGS));
    hipLaunchKernelGGL(k_totals, dim3(1), dim3(1), 0, ctx->stream, (const i64*)vrank + m, (const i64*)frank + nf, (i64*)cn);
    PB3D_CHECK_LAUNCH();
    PB3D_TRY(t.mark(ctx));
    if (s.verts_f64)
        hipLaunchKernelGGL(k_vertex_gather<double>, grid_for(nv), dim3(256), 0, ctx->stream, nv, inv, first, (const u32*)used, (const i64*)vrank,
                           (const double*)rows, s.colors, s.channels, (double*)s.out_verts, s.index, s.inverse, s.out_colors);
    else
        hipLaunchKernelGGL(k_vertex_gather<float>, grid_for(nv), dim3(256), 0, ctx->stream, nv, inv, first, (const u32*)used, (const i64*)vrank,
                           (const float*)rows, s.colors, s.channels, (float*)s.out_verts, s.index, s.inverse, s.out_colors);
    PB3D_CHECK_LAUNCH();
    hipLaunchKernelGGL((s.faces_i64 ? k_face_gather<true> : k_face_gather<false>), grid_for(nf), dim3(256), 0, ctx->stream, nf, (const u32*)G,
                       (const u32*)keep, (const i64*)frank, (const i64*)vrank, s.out_faces, s.face_index);
    PB3D_CHECK_LAUNCH();
    PB3D_TRY(t.mark(ctx));
    i64 got[2];
    PB3D_TRY(pb3d_read_back(ctx, got, cn, sizeof(got)));
    counts[0] = got[0];
    counts[1] = got[1];
    ctx->simplify_last.counts[1] = got[0];
    ctx->simplify_last.counts[2] = got[1];
    return t.finish(ctx, ctx->simplify_last.ms, &ctx->simplify_last.timed);
}

// the result without a face: nothing stays.  Enqueued
int nothing_stays(pb3d_ctx* ctx, const Mesh& s, int64_t counts[2]) {
    if (s.inverse && s.nv > 0) PB3D_HIP(hipMemsetAsync(s.inverse, 0xff, (size_t)s.nv * sizeof(int), ctx->stream));
    counts[0] = counts[1] = 0;
    return PB3D_OK;
}

int run(pb3d_ctx* ctx, const char* what, const Mesh& s, bool cluster, double voxel_size, const double* origin, int reduce, int64_t counts[2]) {
    if (s.nv == 0 && s.nf > 0) {
        pb3d_set_error("%s: index out of bounds for 0 entries", what);
        return PB3D_EINDEX;
    }
    PB3D_TRY(pb3d_check_index_range(ctx, s.faces, s.faces_i64, 3 * s.nf, -s.nv, s.nv, what));
    if (s.nf == 0) return nothing_stays(ctx, s, counts);
    ctx->simplify_last = {};
    Stamps t = {ctx->tune_simplify_timing != 0, 0, {}};
    PB3D_TRY(t.mark(ctx));
    const int *inv = nullptr, *first = nullptr;
    const void* rows = s.verts;
    i64 m = s.nv;
    if (cluster) {
        void *rw, *fs, *iv;
        PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_SIMPLIFY_CLUSTER_ROWS, (size_t)s.nv * 3 * (s.verts_f64 ? sizeof(double) : sizeof(float)), &rw));
        PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_SIMPLIFY_CLUSTER_FIRST, (size_t)s.nv * sizeof(int), &fs));
        PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_SIMPLIFY_CLUSTER_INVERSE, (size_t)s.nv * sizeof(int), &iv));
        PB3D_TRY(pb3d_voxel_downsample_resident(ctx, s.verts, s.verts_f64, s.nv, voxel_size, origin, reduce, rw, (int*)fs, (int*)iv, nullptr, &m));
        inv = (const int*)iv;
        first = (const int*)fs;
        rows = rw;
    }
    ctx->simplify_last.valid = true;
    ctx->simplify_last.counts[0] = m;
    PB3D_TRY(t.mark(ctx));
    return face_tail(ctx, s, inv, first, rows, m, t, counts);
}

}  // namespace

extern "C" {

int pb3d_mesh_simplify_resident(pb3d_ctx* ctx, const void* d_verts, int verts_f64, int64_t nv, const void* d_faces, int faces_i64, int64_t nf,
                                double voxel_size, const double origin[3], int reduce, int duplicate_faces, const uint8_t* d_colors, int channels,
                                void* d_out_verts, void* d_out_faces, uint8_t* d_out_colors, int32_t* d_index, int32_t* d_inverse,
                                int32_t* d_face_index, int64_t counts[2]) {
    const Mesh s = {d_verts, verts_f64, nv, d_faces, faces_i64, nf, duplicate_faces, d_colors, channels, d_out_verts, d_out_faces, d_out_colors,
                    d_index, d_inverse, d_face_index};
    PB3D_TRY(require_mesh("pb3d_mesh_simplify", s, counts));
    PB3D_REQUIRE(voxel_size > 0.0 && std::isfinite(voxel_size), "pb3d_mesh_simplify: voxel_size must be finite and > 0 (got %g)", voxel_size);
    PB3D_REQUIRE(origin == nullptr || (std::isfinite(origin[0]) && std::isfinite(origin[1]) && std::isfinite(origin[2])),
                 "pb3d_mesh_simplify: origin must be finite");
    PB3D_REQUIRE(reduce == PB3D_DOWNSAMPLE_CENTROID || reduce == PB3D_DOWNSAMPLE_FIRST,
                 "pb3d_mesh_simplify: reduce must be 0 (centroid) or 1 (first) (got %d)", reduce);
    PB3D_REQUIRE(ctx != nullptr, "pb3d_mesh_simplify: null context");
    return run(ctx, "pb3d_mesh_simplify", s, true, voxel_size, origin, reduce, counts);
}

int pb3d_mesh_compact_resident(pb3d_ctx* ctx, const void* d_verts, int verts_f64, int64_t nv, const void* d_faces, int faces_i64, int64_t nf,
                               int duplicate_faces, const uint8_t* d_colors, int channels, void* d_out_verts, void* d_out_faces,
                               uint8_t* d_out_colors, int32_t* d_index, int32_t* d_inverse, int32_t* d_face_index, int64_t counts[2]) {
    const Mesh s = {d_verts, verts_f64, nv, d_faces, faces_i64, nf, duplicate_faces, d_colors, channels, d_out_verts, d_out_faces, d_out_colors,
                    d_index, d_inverse, d_face_index};
    PB3D_TRY(require_mesh("pb3d_mesh_compact", s, counts));
    PB3D_REQUIRE(ctx != nullptr, "pb3d_mesh_compact: null context");
    return run(ctx, "pb3d_mesh_compact", s, false, 0.0, nullptr, 0, counts);
}

int pb3d_mesh_select_faces_resident(pb3d_ctx* ctx, const void* d_verts, int verts_f64, int64_t nv, const void* d_faces, int faces_i64, int64_t nf,
                                    const uint8_t* d_keep, const uint8_t* d_colors, int channels, void* d_out_verts, void* d_out_faces,
                                    uint8_t* d_out_colors, int32_t* d_index, int32_t* d_inverse, int32_t* d_face_index, int64_t counts[2]) {
    const Mesh s = {d_verts, verts_f64, nv, d_faces, faces_i64, nf, PB3D_FACES_KEEP, d_colors, channels, d_out_verts, d_out_faces, d_out_colors,
                    d_index, d_inverse, d_face_index, d_keep};
    PB3D_TRY(require_mesh("pb3d_mesh_select_faces", s, counts));
    PB3D_REQUIRE(nf == 0 || d_keep != nullptr, "pb3d_mesh_select_faces: null buffer");
    PB3D_REQUIRE(nv == 0 || nf == 0 || ((const void*)d_keep != d_out_verts && (const void*)d_keep != d_out_faces),
                 "pb3d_mesh_select_faces: an output may not alias an input");
    PB3D_REQUIRE(ctx != nullptr, "pb3d_mesh_select_faces: null context");
    return run(ctx, "pb3d_mesh_select_faces", s, false, 0.0, nullptr, 0, counts);
}

int pb3d_simplify_last(pb3d_ctx* ctx, int64_t counts[3], double pass_ms[5]) {
    PB3D_REQUIRE(ctx != nullptr && counts != nullptr, "pb3d_simplify_last: null argument");
    PB3D_REQUIRE(ctx->simplify_last.valid, "pb3d_simplify_last: no simplification has run on this context");
    for (int a = 0; a < 3; ++a) counts[a] = ctx->simplify_last.counts[a];
    if (pass_ms) {
        PB3D_REQUIRE(ctx->simplify_last.timed, "pb3d_simplify_last: the last simplification was not timed (knob simplify_timing)");
        for (int i = 0; i < 5; ++i) pass_ms[i] = ctx->simplify_last.ms[i];
    }
    return PB3D_OK;
}

}  // extern "C"
