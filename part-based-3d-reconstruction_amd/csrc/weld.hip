// weld_vertices: the vertices of a mesh (or the points of a cloud) merged by exact coordinate equality, classes numbered by first
// appearance, faces mapped through (include/pb3d.h has the rules to the bit; DESIGN.md "Mesh repair" has the passes).
//
// Nothing is kept per class, nothing is hashed and there is no atomic: a class in which every vertex lies is handled like any other.
//   k_weld_key         one key word per 32 bits of coordinate, the raw bits with -0.0 mapped to +0.0 (for finite values key equality is
//                      IEEE equality), gathered through the current permutation; the first one writes the ascending positions
//   pb3d_sort_pairs    three times for float32, six for float64 (csrc/sort_pairs.hip, stable, m = 2^32): from the low word of the last
//                      coordinate to the high word of the first.  Every pass is stable, so a run of equal rows is in ascending position
//   k_weld_heads       head[p] = the row at sorted place p differs from the one before it (compared as IEEE numbers)
//   pb3d_scan_counts   runs before p.  k_weld_runs: where run r starts, and where the last one ends
//   k_weld_reps        back to input order: each vertex's representative (its run's first record), the "representative" flags and
//                      each representative's class size
//   pb3d_scan_counts   representatives before i = the first-appearance numbers, and their count (the call's read-back)
//   k_weld_gather      one lane per vertex: inverse[i]; a representative also writes its row byte for byte, its position, its class
//                      size and its colour bytes
//   k_weld_faces       every index wrapped and mapped through the representative's number
#include <algorithm>

#include "mesh_index.h"
#include "pb3d_internal.h"

namespace {

constexpr i64 kMaxElems = (1ll << 31) - 1;

// pass k of the sorts: coordinate 2 - k (float32) or 2 - k / 2, low half first (float64)
template <bool F64>
__device__ __forceinline__ u32 key_word(const void* __restrict__ verts, i64 i, int pass) {
    if (F64) {
        const u64 b = ((const u64*)verts)[3 * i + (2 - pass / 2)];
        const u64 z = b == 0x8000000000000000ull ? 0ull : b;
        return (pass & 1) ? (u32)(z >> 32) : (u32)z;
    }
    const u32 b = ((const u32*)verts)[3 * i + (2 - pass)];
    return b == 0x80000000u ? 0u : b;
}

// val_in null: the first pass, place p holds position p
template <bool F64>
__global__ __launch_bounds__(256) void k_weld_key(const void* __restrict__ verts, const u32* __restrict__ val_in, i64 n, int pass, u32* __restrict__ key,
                                                  u32* __restrict__ val_out) {
    const i64 p = (i64)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const i64 i = val_in ? (i64)val_in[p] : p;
    key[p] = key_word<F64>(verts, i, pass);
    if (!val_in) val_out[p] = (u32)p;
}

template <class T>
__global__ __launch_bounds__(256) void k_weld_heads(const T* __restrict__ verts, const u32* __restrict__ val, i64 n, u32* __restrict__ head) {
    const i64 p = (i64)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    bool first = p == 0;
    if (!first) {
        const T *a = verts + 3 * (i64)val[p], *b = verts + 3 * (i64)val[p - 1];
        first = a[0] != b[0] || a[1] != b[1] || a[2] != b[2];
    }
    head[p] = first ? 1u : 0u;
}

// start[r] = the place of run r's first record; start[runs] = n
__global__ __launch_bounds__(256) void k_weld_runs(i64 n, const u32* __restrict__ head, const i64* __restrict__ head_rank, u32* __restrict__ start) {
    const i64 p = (i64)blockIdx.x * 256 + threadIdx.x;
    if (p > n) return;
    if (p == n || head[p]) start[head_rank[p]] = (u32)p;
}

__global__ __launch_bounds__(256) void k_weld_reps(const u32* __restrict__ val, i64 n, const u32* __restrict__ head, const i64* __restrict__ head_rank,
                                                   const u32* __restrict__ start, int* __restrict__ rep, u32* __restrict__ is_rep, u32* __restrict__ size) {
    const i64 p = (i64)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const i64 r = head_rank[p] + (i64)head[p] - 1;
    const i64 i = (i64)val[p];
    rep[i] = (int)val[start[r]];
    is_rep[i] = head[p];
    if (head[p]) size[i] = start[r + 1] - start[r];
}

// T: the vertex element type; rows are copied element by element.  index, inverse, counts and colors may each be null
template <class T>
__global__ __launch_bounds__(256) void k_weld_gather(i64 n, const int* __restrict__ rep, const u32* __restrict__ is_rep, const i64* __restrict__ vrank,
                                                     const u32* __restrict__ size, const T* __restrict__ verts, const u8* __restrict__ colors, int channels,
                                                     T* __restrict__ out, int* __restrict__ index, int* __restrict__ inverse, u32* __restrict__ counts,
                                                     u8* __restrict__ out_colors) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const i64 k = vrank[rep[i]];
    if (inverse) inverse[i] = (int)k;
    if (!is_rep[i]) return;
    for (int a = 0; a < 3; ++a) out[3 * k + a] = verts[3 * i + a];
    if (index) index[k] = (int)i;
    if (counts) counts[k] = size[i];
    if (colors)
        for (int a = 0; a < channels; ++a) out_colors[channels * k + a] = colors[channels * i + a];
}

template <bool I64>
__global__ __launch_bounds__(256) void k_weld_faces(const void* __restrict__ faces, i64 entries, i64 nv, const int* __restrict__ rep, const i64* __restrict__ vrank,
                                                    void* __restrict__ out) {
    const i64 e = (i64)blockIdx.x * 256 + threadIdx.x;
    if (e >= entries) return;
    const i64 k = vrank[rep[wrap(load_index<I64>(faces, e), nv)]];
    if (I64) ((i64*)out)[e] = k;
    else ((int*)out)[e] = (int)k;
}

inline dim3 grid_for(i64 n) { return dim3((unsigned)((n + 255) / 256)); }

struct Args {
    const void* verts; int verts_f64; i64 nv;
    const void* faces; int faces_i64; i64 nf;
    const u8* colors; int channels;
    void *out_verts, *out_faces;
    u8* out_colors;
    int *index, *inverse;
    u32* counts;
};

// nv >= 1, checked indices.  Everything is enqueued but the read-back of the class count
int run(pb3d_ctx* ctx, const Args& s, int64_t* classes) {
    const i64 n = s.nv;
    void *kv, *fl, *rk, *rn;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_WELD_PAIRS, (size_t)n * 4 * sizeof(u32), &kv));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_WELD_FLAGS, (size_t)n * 2 * sizeof(u32), &fl));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_WELD_RANKS, (size_t)(n + 1) * 2 * sizeof(i64), &rk));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_WELD_RUNS, (size_t)(n + 1) * sizeof(u32) + (size_t)n * (sizeof(int) + sizeof(u32)), &rn));
    // the scans of the call are the sorts' run tables and the two flag arrays': size both scan slots for the largest now, so that none
    // regrows (and waits) midway
    PB3D_TRY(pb3d_scan_reserve(ctx, std::max<i64>(n, pb3d_sort_scan_items(n)), PB3D_SLOT_WELD_SCAN_LOCAL, PB3D_SLOT_WELD_SCAN_SEGS));
    u32 *key = (u32*)kv, *val = key + n, *key2 = key + 2 * n, *val2 = key + 3 * n;
    u32 *head = (u32*)fl, *is_rep = head + n;
    i64 *head_rank = (i64*)rk, *vrank = head_rank + (n + 1);
    u32* start = (u32*)rn;
    int* rep = (int*)(start + (n + 1));
    u32* size = (u32*)(rep + n);

    const int passes = s.verts_f64 ? 6 : 3;
    for (int pass = 0; pass < passes; ++pass) {
        const u32* from = pass ? val : nullptr;
        if (s.verts_f64) hipLaunchKernelGGL(k_weld_key<true>, grid_for(n), dim3(256), 0, ctx->stream, s.verts, from, n, pass, key, val);
        else hipLaunchKernelGGL(k_weld_key<false>, grid_for(n), dim3(256), 0, ctx->stream, s.verts, from, n, pass, key, val);
        PB3D_CHECK_LAUNCH();
        const u32 *ks, *vs;
        PB3D_TRY(pb3d_sort_pairs(ctx, key, val, key2, val2, n, 1ll << 32, PB3D_SLOT_WELD_SORT_HIST, PB3D_SLOT_WELD_SCAN_LOCAL, PB3D_SLOT_WELD_SCAN_SEGS,
                                 &ks, &vs));
        if (vs != val) { std::swap(key, key2); std::swap(val, val2); }     // the sorted pair is the next sort's input; its keys are spent
    }
    if (s.verts_f64) hipLaunchKernelGGL(k_weld_heads<double>, grid_for(n), dim3(256), 0, ctx->stream, (const double*)s.verts, (const u32*)val, n, head);
    else hipLaunchKernelGGL(k_weld_heads<float>, grid_for(n), dim3(256), 0, ctx->stream, (const float*)s.verts, (const u32*)val, n, head);
    PB3D_CHECK_LAUNCH();
    PB3D_TRY(pb3d_scan_counts(ctx, head, n, head_rank, PB3D_SLOT_WELD_SCAN_LOCAL, PB3D_SLOT_WELD_SCAN_SEGS));
    hipLaunchKernelGGL(k_weld_runs, grid_for(n + 1), dim3(256), 0, ctx->stream, n, (const u32*)head, (const i64*)head_rank, start);
    PB3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_weld_reps, grid_for(n), dim3(256), 0, ctx->stream, (const u32*)val, n, (const u32*)head, (const i64*)head_rank, (const u32*)start, rep,
                       is_rep, size);
    PB3D_CHECK_LAUNCH();
    PB3D_TRY(pb3d_scan_counts(ctx, is_rep, n, vrank, PB3D_SLOT_WELD_SCAN_LOCAL, PB3D_SLOT_WELD_SCAN_SEGS));
    if (s.verts_f64)
        hipLaunchKernelGGL(k_weld_gather<double>, grid_for(n), dim3(256), 0, ctx->stream, n, (const int*)rep, (const u32*)is_rep, (const i64*)vrank,
                           (const u32*)size, (const double*)s.verts, s.colors, s.channels, (double*)s.out_verts, s.index, s.inverse, s.counts, s.out_colors);
    else
        hipLaunchKernelGGL(k_weld_gather<float>, grid_for(n), dim3(256), 0, ctx->stream, n, (const int*)rep, (const u32*)is_rep, (const i64*)vrank,
                           (const u32*)size, (const float*)s.verts, s.colors, s.channels, (float*)s.out_verts, s.index, s.inverse, s.counts, s.out_colors);
    PB3D_CHECK_LAUNCH();
    if (s.nf > 0) {
        hipLaunchKernelGGL((s.faces_i64 ? k_weld_faces<true> : k_weld_faces<false>), grid_for(3 * s.nf), dim3(256), 0, ctx->stream, s.faces, 3 * s.nf, n,
                           (const int*)rep, (const i64*)vrank, s.out_faces);
        PB3D_CHECK_LAUNCH();
    }
    i64 got;
    PB3D_TRY(pb3d_read_back(ctx, &got, vrank + n, sizeof(got)));
    *classes = got;
    return PB3D_OK;
}

}  // namespace

extern "C" {

int pb3d_weld_vertices_resident(pb3d_ctx* ctx, const void* d_verts, int verts_f64, int64_t nv, const void* d_faces, int faces_i64, int64_t nf,
                                const uint8_t* d_colors, int channels, void* d_out_verts, void* d_out_faces, uint8_t* d_out_colors, int32_t* d_index,
                                int32_t* d_inverse, uint32_t* d_class_counts, int64_t* classes) {
    const char* what = "pb3d_weld_vertices";
    PB3D_REQUIRE(nv >= 0 && nf >= 0, "%s: negative count", what);
    PB3D_REQUIRE(nv <= kMaxElems && nf <= kMaxElems / 3, "%s: at most 2^31 - 1 vertices and (2^31 - 1) / 3 faces", what);
    PB3D_REQUIRE(classes != nullptr, "%s: null argument", what);
    PB3D_REQUIRE(d_colors == nullptr || channels == 1 || channels == 3, "%s: channels must be 1 or 3 (got %d)", what, channels);
    PB3D_REQUIRE((nv == 0 || (d_verts && d_out_verts)) && (nf == 0 || (d_faces && d_out_faces)), "%s: null buffer", what);
    PB3D_REQUIRE(nv == 0 || (d_colors == nullptr) == (d_out_colors == nullptr), "%s: null buffer", what);
    const void* outs[6] = {d_out_verts, d_out_faces, d_out_colors, d_index, d_inverse, d_class_counts};
    for (const void* o : outs)
        PB3D_REQUIRE(o == nullptr || (o != d_verts && o != d_faces && o != (const void*)d_colors), "%s: an output may not alias an input", what);
    PB3D_REQUIRE(ctx != nullptr, "%s: null context", what);
    if (nv == 0 && nf > 0) {
        pb3d_set_error("%s: index out of bounds for 0 entries", what);
        return PB3D_EINDEX;
    }
    if (nf > 0) PB3D_TRY(pb3d_check_index_range(ctx, d_faces, faces_i64, 3 * nf, -nv, nv, what));
    if (nv == 0) {
        *classes = 0;
        return PB3D_OK;
    }
    const Args s = {d_verts, verts_f64, nv, d_faces, faces_i64, nf, d_colors, channels, d_out_verts, d_out_faces, d_out_colors, d_index, d_inverse,
                    d_class_counts};
    return run(ctx, s, classes);
}

}  // extern "C"
