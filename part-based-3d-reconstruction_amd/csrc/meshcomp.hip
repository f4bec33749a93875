// mesh_components: connected components of a triangle mesh, the edge counts of every component and of the whole mesh, and the ordered
// float64 area and signed volume of every component (include/pb3d.h has the rules to the bit; DESIGN.md "Mesh components" has the
// passes and the determinism argument).  pb3d_mesh_select_faces_resident, the tail that turns a face mask into a mesh, is in
// csrc/simplify.hip with the scans and gathers it shares.
//
// Nothing is kept per edge but the position of its first record, and no lane walks along a run, so a fan of thousands of faces round
// one edge is handled like any other:
//   k_records          face j -> its wrapped corners (12 bytes a face, read by every later pass) and the first pairs of the sort,
//                      (hi, 3j + a) for its three directed edges; a loop gets the key nv, which sorts behind every vertex
//   pb3d_sort_pairs    twice (csrc/sort_pairs.hip, stable): by hi, then by lo gathered through the permutation (k_next_key)
//   k_heads            head[p] = record p is the first of its undirected edge, fwd[p] = its source is lo; under "edge" a record that
//                      is no head unites its face with the face of the record before it (csrc/union_find.h, over faces)
//   pb3d_scan_counts   twice: edges before p, forward records before p.  k_head_positions: where edge e starts, and where the last ends
//   k_union_vertices   "vertex" only: every face unites w0 ~ w1 and w1 ~ w2, over vertices
//   k_flatten          every entry of the forest becomes its root.  "edge": the root is the component's smallest face.  "vertex":
//                      an integer atomicMin of the face position per vertex root names it (k_min_face, k_first_faces)
//   pb3d_scan_counts   of the "first face of its component" flags: the component numbers, and their count
//   k_labels           face labels, vertex labels by atomicMin, faces per component (integer atomics, one per run of equal labels
//                      a wavefront meets on its way through the list)
//   k_edges            one lane per edge: c and f are differences at consecutive heads; the four per-component and three total counts
//   measures           A_j and S_j per face, a stable sort of (label, face), segment starts from the face counts, blocks of 256
//                      enumerated by a scan of ceil(faces / 256), one wavefront per block through ordered_sum (csrc/ordered_sum.h),
//                      then one wavefront per component over its block sums.  No floating-point atomics
#include <algorithm>

#include "mesh_index.h"
#include "mesh_records.h"
#include "ordered_sum.h"
#include "pb3d_internal.h"
#include "union_find.h"

namespace {

constexpr i64 kMaxVertices = (1ll << 31) - 1;
constexpr i64 kMaxFaces = ((1ll << 31) - 1) / 6;
constexpr int kUnset = 0x7f7f7f7f;          // hipMemsetAsync(0x7f): above every face position and every label
constexpr int kBlock = 256;                 // faces per block of a component's sum
constexpr int kCountBlocks = 4;             // workgroups per CU of the counting kernels: each wavefront flushes its counts once

template <bool I64>
__global__ __launch_bounds__(256) void k_records(const void* __restrict__ faces, i64 nf, i64 nv, u32* __restrict__ W, u32* __restrict__ key,
                                                 u32* __restrict__ val, int* __restrict__ face_parent, unsigned long long* loops_total) {
    const i64 j = (i64)blockIdx.x * 256 + threadIdx.x;
    if (j >= nf) return;
    u32 w[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        w[a] = (u32)wrap(load_index<I64>(faces, 3 * j + a), nv);
        W[3 * j + a] = w[a];
    }
    int loops = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const Rec e = {w[a], w[(a + 1) % 3]};
        key[3 * j + a] = is_loop(e) ? (u32)nv : hi_of(e);
        val[3 * j + a] = (u32)(3 * j + a);
        loops += is_loop(e) ? 1 : 0;
    }
    if (face_parent) face_parent[j] = (int)j;
    if (loops && loops_total) atomicAdd(loops_total, (unsigned long long)loops);
}

// key[p] = lo of the record at sorted place p
__global__ __launch_bounds__(256) void k_next_key(const u32* __restrict__ W, const u32* __restrict__ val, i64 R, u32 nv, u32* __restrict__ key) {
    const i64 p = (i64)blockIdx.x * 256 + threadIdx.x;
    if (p >= R) return;
    const Rec e = load_rec(W, val[p]);
    key[p] = is_loop(e) ? nv : lo_of(e);
}

// face_parent null: no unions ("vertex")
__global__ __launch_bounds__(256) void k_heads(const u32* __restrict__ W, const u32* __restrict__ val, i64 R, u32* __restrict__ head,
                                               u32* __restrict__ fwd, int* face_parent) {
    const i64 p = (i64)blockIdx.x * 256 + threadIdx.x;
    if (p >= R) return;
    const u32 r = val[p];
    const Rec e = load_rec(W, r);
    bool first = !is_loop(e);
    u32 before = 0;
    if (first && p > 0) {
        before = val[p - 1];
        const Rec q = load_rec(W, before);                  // the loops are the last of the order: q is none of them
        first = lo_of(e) != lo_of(q) || hi_of(e) != hi_of(q);
    }
    head[p] = first ? 1u : 0u;
    fwd[p] = !is_loop(e) && e.src < e.dst ? 1u : 0u;
    if (face_parent && !is_loop(e) && !first) uf_union(face_parent, (int)(r / 3u), (int)(before / 3u));
}

// pos[e] = the place of edge e's first record; pos[E] = the place behind the last record that is no loop
__global__ __launch_bounds__(256) void k_head_positions(const u32* __restrict__ W, const u32* __restrict__ val, i64 R, const u32* __restrict__ head,
                                                        const i64* __restrict__ head_rank, u32* __restrict__ pos) {
    const i64 p = (i64)blockIdx.x * 256 + threadIdx.x;
    if (p > R) return;
    bool writes;
    if (p < R && head[p]) {
        writes = true;
    } else {
        const bool here = p == R || is_loop(load_rec(W, val[p]));
        writes = here && (p == 0 || !is_loop(load_rec(W, val[p - 1])));
    }
    if (writes) pos[head_rank[p]] = (u32)p;
}

__global__ __launch_bounds__(256) void k_iota(int* __restrict__ parent, i64 n) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i < n) parent[i] = (int)i;
}

__global__ __launch_bounds__(256) void k_union_vertices(const u32* __restrict__ W, i64 nf, int* parent) {
    const i64 j = (i64)blockIdx.x * 256 + threadIdx.x;
    if (j >= nf) return;
    const int w0 = (int)W[3 * j], w1 = (int)W[3 * j + 1], w2 = (int)W[3 * j + 2];
    if (w0 != w1) uf_union(parent, w0, w1);
    if (w1 != w2) uf_union(parent, w1, w2);
}

// Every entry of the forest becomes its root.  The stores race with other lanes' searches, but each is an ancestor of its entry and
// the last one is the root, so the result is the same whatever the order.  root_flag null: none written
__global__ __launch_bounds__(256) void k_flatten(i64 n, int* parent, u32* __restrict__ root_flag) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int r = (int)i;
    for (int p = ld(&parent[r]); p != r; p = ld(&parent[r])) r = p;
    st(&parent[i], r);
    if (root_flag) root_flag[i] = r == (int)i ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_min_face(const u32* __restrict__ W, i64 nf, const int* __restrict__ vertex_root, int* min_face) {
    const i64 j = (i64)blockIdx.x * 256 + threadIdx.x;
    const int r = j < nf ? vertex_root[W[3 * j]] : -1;
    // face positions ascend with the lane, so of the lanes that hold the first active lane's root the lowest holds their minimum: one
    // atomic for the run (a wave inside one component), and none where the word is already below (it only ever falls)
    const unsigned long long active = __ballot(r >= 0);
    if (!active) return;
    const int first = __shfl(r, __ffsll(active) - 1);
    const unsigned long long same = __ballot(r == first);
    if (r < 0 || (r == first && (int)(threadIdx.x & 63) != __ffsll(same) - 1)) return;
    if (ld(&min_face[r]) > (int)j) atomicMin(&min_face[r], (int)j);
}

__global__ __launch_bounds__(256) void k_first_faces(const u32* __restrict__ W, i64 nf, const int* __restrict__ vertex_root,
                                                     const int* __restrict__ min_face, u32* __restrict__ root_flag) {
    const i64 j = (i64)blockIdx.x * 256 + threadIdx.x;
    if (j < nf) root_flag[j] = min_face[vertex_root[W[3 * j]]] == (int)j ? 1u : 0u;
}

// counts[0 .. 5 nc) = 0, totals: components, edges, faces
__global__ __launch_bounds__(256) void k_clear_counts(unsigned long long* __restrict__ counts, const i64* __restrict__ nc, const i64* __restrict__ edges,
                                                      i64 nf, unsigned long long* __restrict__ totals) {
    const i64 n = 5 * *nc;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) counts[i] = 0ull;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        totals[0] = (unsigned long long)*nc;
        totals[2] = (unsigned long long)*edges;
        totals[3] = (unsigned long long)nf;
    }
}

// min_face null: "edge", root[] is over faces; else root[] is over vertices
__global__ __launch_bounds__(256) void k_labels(const u32* __restrict__ W, i64 nf, const int* __restrict__ root, const int* __restrict__ min_face,
                                                const i64* __restrict__ rank, int* __restrict__ face_labels, int* vertex_labels,
                                                unsigned long long* counts) {
    RunCount faces;
    for (i64 base = wave_base(); base < nf; base += (i64)gridDim.x * 256) {
        const i64 j = base + lane_id();
        int lab = -1;
        if (j < nf) {
            const int first = min_face ? min_face[root[W[3 * j]]] : root[j];
            lab = (int)rank[first];
            face_labels[j] = lab;
#pragma unroll
            for (int a = 0; a < 3; ++a) atomicMin(&vertex_labels[W[3 * j + a]], lab);
        }
        faces.add(counts, lab, true);
    }
    faces.flush(counts);
}

__global__ __launch_bounds__(256) void k_edges(const u32* __restrict__ val, i64 R, const i64* __restrict__ head_rank, const i64* __restrict__ fwd_rank,
                                               const u32* __restrict__ pos, const int* __restrict__ face_labels, const i64* __restrict__ nc_ptr,
                                               unsigned long long* counts, unsigned long long* totals) {
    const i64 nc = *nc_ptr, E = head_rank[R];
    RunCount edges, boundaries, nonmanifolds, unbalanceds;
    WaveTotal tb, tn, tu;
    for (i64 base = wave_base(); base < E; base += (i64)gridDim.x * 256) {
        const i64 e = base + lane_id();
        int lab = -1;
        bool boundary = false, nonmanifold = false, unbalanced = false;
        if (e < E) {
            const i64 p0 = pos[e], p1 = pos[e + 1];
            const i64 c = p1 - p0, f = fwd_rank[p1] - fwd_rank[p0];
            boundary = c == 1;
            nonmanifold = c > 2;
            unbalanced = 2 * f != c;
            lab = face_labels[val[p0] / 3u];
        }
        edges.add(counts + nc, lab, true);
        boundaries.add(counts + 2 * nc, lab, boundary);
        nonmanifolds.add(counts + 3 * nc, lab, nonmanifold);
        unbalanceds.add(counts + 4 * nc, lab, unbalanced);
        tb.add(boundary);
        tn.add(nonmanifold);
        tu.add(unbalanced);
    }
    edges.flush(counts + nc);
    boundaries.flush(counts + 2 * nc);
    nonmanifolds.flush(counts + 3 * nc);
    unbalanceds.flush(counts + 4 * nc);
    tb.flush(&totals[4]);
    tn.flush(&totals[5]);
    tu.flush(&totals[6]);
}

// out null: the count alone
__global__ __launch_bounds__(256) void k_vertex_labels(const int* __restrict__ labels, i64 nv, int* __restrict__ out, unsigned long long* totals) {
    WaveTotal named;
    for (i64 base = wave_base(); base < nv; base += (i64)gridDim.x * 256) {
        const i64 i = base + lane_id();
        const int l = i < nv ? labels[i] : kUnset;
        if (out && i < nv) out[i] = l != kUnset ? l : -1;
        named.add(l != kUnset);
    }
    named.flush(&totals[1]);
}

// ---- the measures --------------------------------------------------------------------------------------------------------------------
// AS[2j] = A_j, AS[2j + 1] = S_j (-S_j where negate, unless null, is not 0: csrc/orient.hip's flipped faces), every operation one
// rounded float64 operation (-ffp-contract=off); and the first pairs of the (label, face) sort
template <bool F64>
__global__ __launch_bounds__(256) void k_face_measures(const void* __restrict__ verts, const u32* __restrict__ W, i64 nf, const int* __restrict__ face_labels,
                                                       const u32* __restrict__ negate, double* __restrict__ AS, u32* __restrict__ key, u32* __restrict__ val) {
    const i64 j = (i64)blockIdx.x * 256 + threadIdx.x;
    if (j >= nf) return;
    double a[3], b[3], c[3];
    pb3d_load3<F64>(verts, (i64)W[3 * j], a);
    pb3d_load3<F64>(verts, (i64)W[3 * j + 1], b);
    pb3d_load3<F64>(verts, (i64)W[3 * j + 2], c);
    const double e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2];
    const double e2x = c[0] - a[0], e2y = c[1] - a[1], e2z = c[2] - a[2];
    const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    AS[2 * j] = 0.5 * __dsqrt_rn((nx * nx + ny * ny) + nz * nz);
    const double mx = b[1] * c[2] - b[2] * c[1], my = b[2] * c[0] - b[0] * c[2], mz = b[0] * c[1] - b[1] * c[0];
    const double S = (a[0] * mx + a[1] * my) + a[2] * mz;
    AS[2 * j + 1] = negate && negate[j] ? -S : S;
    key[j] = (u32)face_labels[j];
    val[j] = (u32)j;
}

// per component l < nc its faces and its blocks of 256, 0 for l >= nc: the counts of the two scans
__global__ __launch_bounds__(256) void k_segment_counts(const unsigned long long* __restrict__ faces_of, const i64* __restrict__ nc, i64 nf,
                                                        u32* __restrict__ nfaces, u32* __restrict__ nblocks) {
    const i64 l = (i64)blockIdx.x * 256 + threadIdx.x;
    if (l >= nf) return;
    const u32 c = l < *nc ? (u32)faces_of[l] : 0u;
    nfaces[l] = c;
    nblocks[l] = (c + (u32)kBlock - 1u) / (u32)kBlock;
}

// one wavefront per block b: the component is the last l with block_start[l] <= b (every component has a block, so the starts of
// 0 .. nc increase strictly); its faces s .. e of the sorted list are added in order from 0.0
__global__ __launch_bounds__(256) void k_block_sums(const u32* __restrict__ sorted_face, const double* __restrict__ AS, const i64* __restrict__ seg_start,
                                                    const i64* __restrict__ block_start, const i64* __restrict__ nc_ptr, double* __restrict__ block_sum) {
    const i64 nc = *nc_ptr, B = block_start[nc];
    const i64 waves = (i64)gridDim.x * 4;
    for (i64 b = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); b < B; b += waves) {
        i64 lo = 0, hi = nc - 1;
        while (lo < hi) {
            const i64 mid = (lo + hi + 1) >> 1;
            if (block_start[mid] <= b) lo = mid; else hi = mid - 1;
        }
        const i64 s = seg_start[lo] + (b - block_start[lo]) * kBlock;
        const i64 end = seg_start[lo + 1], e = s + kBlock < end ? s + kBlock : end;
        double sum[3];
        ordered_sum(s, e, [&](i64 p, double* v) {
            const i64 j = (i64)sorted_face[p];
            v[0] = AS[2 * j]; v[1] = AS[2 * j + 1]; v[2] = 0.0;
        }, sum);
        if ((threadIdx.x & 63) == 0) { block_sum[2 * b] = sum[0]; block_sum[2 * b + 1] = sum[1]; }
    }
}

// one wavefront per component: its block sums in order from 0.0; area = the sum of A, volume = the sum of S / 6.0
__global__ __launch_bounds__(256) void k_component_sums(const double* __restrict__ block_sum, const i64* __restrict__ block_start,
                                                        const i64* __restrict__ nc_ptr, double* __restrict__ measures) {
    const i64 nc = *nc_ptr;
    const i64 waves = (i64)gridDim.x * 4;
    for (i64 l = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); l < nc; l += waves) {
        double sum[3];
        ordered_sum(block_start[l], block_start[l + 1], [&](i64 b, double* v) { v[0] = block_sum[2 * b]; v[1] = block_sum[2 * b + 1]; v[2] = 0.0; }, sum);
        if ((threadIdx.x & 63) == 0) { measures[l] = sum[0]; measures[nc + l] = __ddiv_rn(sum[1], 6.0); }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
inline dim3 grid_for(i64 n) { return dim3((unsigned)((n + 255) / 256)); }

int scan(pb3d_ctx* ctx, const u32* flags, i64 n, i64* ranks) {
    return pb3d_scan_counts(ctx, flags, n, ranks, PB3D_SLOT_MESHCOMP_SCAN_LOCAL, PB3D_SLOT_MESHCOMP_SCAN_SEGS);
}
int sort(pb3d_ctx* ctx, u32*& key, u32*& val, u32*& key2, u32*& val2, i64 n, i64 m) {
    const u32 *ks, *vs;
    PB3D_TRY(pb3d_sort_pairs(ctx, key, val, key2, val2, n, m, PB3D_SLOT_MESHCOMP_SORT_HIST, PB3D_SLOT_MESHCOMP_SCAN_LOCAL,
                             PB3D_SLOT_MESHCOMP_SCAN_SEGS, &ks, &vs));
    if (vs != val) { std::swap(key, key2); std::swap(val, val2); }
    return PB3D_OK;
}

struct Args {
    const void* verts; int verts_f64; i64 nv;
    const void* faces; int faces_i64; i64 nf;
    bool by_edge;
    int *face_labels, *vertex_labels;
    i64* counts;
    double* measures;
};

// nv >= 1, nf >= 1, checked indices.  Everything is enqueued but the read-back of the totals
int run(pb3d_ctx* ctx, const Args& s, int64_t totals[8]) {
    const i64 nf = s.nf, nv = s.nv, R = 3 * nf;
    const bool measured = s.measures != nullptr;
    void *pa, *mf = nullptr, *rf, *rr, *vl, *own = nullptr, *tt;
    pb3d_edge_records rec;
    PB3D_TRY(pb3d_mesh_edge_records_reserve(ctx, nf, &rec));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_MESHCOMP_PARENT, (size_t)(s.by_edge ? nf : nv) * sizeof(int), &pa));
    if (!s.by_edge) PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_MESHCOMP_MIN_FACE, (size_t)nv * sizeof(int), &mf));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_MESHCOMP_ROOT_FLAGS, (size_t)nf * sizeof(u32), &rf));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_MESHCOMP_ROOT_RANKS, (size_t)(nf + 1) * sizeof(i64), &rr));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_MESHCOMP_VERTEX_LABELS, (size_t)nv * sizeof(int), &vl));
    // the segments' slot: the sums' tables, then the counts nobody asked for
    if (measured || !s.counts) PB3D_TRY(pb3d_mesh_ordered_sums_reserve(ctx, nf, measured, s.counts ? 0 : (size_t)nf * 5 * sizeof(i64), &own));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_MESHCOMP_TOTALS, 8 * sizeof(i64), &tt));
    u32* root_flag = (u32*)rf;
    i64* root_rank = (i64*)rr;
    int *parent = (int*)pa, *min_face = (int*)mf, *vlab = (int*)vl;
    unsigned long long* tot = (unsigned long long*)tt;
    unsigned long long* counts = s.counts ? (unsigned long long*)s.counts : (unsigned long long*)own;
    const i64* nc = root_rank + nf;

    PB3D_HIP(hipMemsetAsync(tot, 0, 8 * sizeof(i64), ctx->stream));
    PB3D_HIP(hipMemsetAsync(vlab, 0x7f, (size_t)nv * sizeof(int), ctx->stream));
    // ---- the records in (lo, hi) order, run heads, forward bits and, under "edge", the unions
    PB3D_TRY(pb3d_mesh_edge_records_build(ctx, s.faces, s.faces_i64, nf, nv, s.by_edge ? parent : (int*)nullptr, &tot[7], &rec));
    const u32 *W = rec.W, *val = rec.val;
    // ---- the components and their numbers
    if (s.by_edge) {
        PB3D_TRY(pb3d_forest_flatten(ctx, nf, parent, root_flag));
    } else {
        PB3D_HIP(hipMemsetAsync(min_face, 0x7f, (size_t)nv * sizeof(int), ctx->stream));
        PB3D_TRY(pb3d_forest_init(ctx, parent, nv));
        hipLaunchKernelGGL(k_union_vertices, grid_for(nf), dim3(256), 0, ctx->stream, W, nf, parent);
        PB3D_CHECK_LAUNCH();
        PB3D_TRY(pb3d_forest_flatten(ctx, nv, parent, nullptr));
        hipLaunchKernelGGL(k_min_face, grid_for(nf), dim3(256), 0, ctx->stream, W, nf, (const int*)parent, min_face);
        PB3D_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_first_faces, grid_for(nf), dim3(256), 0, ctx->stream, W, nf, (const int*)parent, (const int*)min_face, root_flag);
        PB3D_CHECK_LAUNCH();
    }
    PB3D_TRY(scan(ctx, root_flag, nf, root_rank));
    hipLaunchKernelGGL(k_clear_counts, dim3(pb3d_stream_blocks(ctx, 5 * nf, 256, 8)), dim3(256), 0, ctx->stream, counts, nc,
                       (const i64*)rec.head_rank + R, nf, tot);
    PB3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_labels, dim3(pb3d_stream_blocks(ctx, nf, 256, kCountBlocks)), dim3(256), 0, ctx->stream, W, nf, (const int*)parent, (const int*)min_face,
                       (const i64*)root_rank, s.face_labels, vlab, counts);
    PB3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_edges, dim3(pb3d_stream_blocks(ctx, R, 256, kCountBlocks)), dim3(256), 0, ctx->stream, val, R, (const i64*)rec.head_rank, (const i64*)rec.fwd_rank,
                       (const u32*)rec.pos, (const int*)s.face_labels, nc, counts, tot);
    PB3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_vertex_labels, dim3(pb3d_stream_blocks(ctx, nv, 256, kCountBlocks)), dim3(256), 0, ctx->stream, (const int*)vlab, nv, s.vertex_labels, tot);
    PB3D_CHECK_LAUNCH();
    // ---- area and volume
    if (measured) PB3D_TRY(pb3d_mesh_ordered_sums(ctx, s.verts, s.verts_f64, rec, nf, s.face_labels, nullptr, counts, nc, s.measures));
    i64 got[8];
    PB3D_TRY(pb3d_read_back(ctx, got, tot, sizeof(got)));
    for (int a = 0; a < 8; ++a) totals[a] = got[a];
    return PB3D_OK;
}

}  // namespace

// ---- what csrc/orient.hip shares (pb3d_internal.h) ------------------------------------------------------------------------------------------
int pb3d_mesh_edge_records_reserve(pb3d_ctx* ctx, i64 nf, pb3d_edge_records* rec) {
    const i64 R = 3 * nf;
    void *ww, *kv, *fl, *rk, *hp;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_MESHCOMP_CORNERS, (size_t)R * sizeof(u32), &ww));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_MESHCOMP_PAIRS, (size_t)R * 4 * sizeof(u32), &kv));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_MESHCOMP_FLAGS, (size_t)R * 2 * sizeof(u32), &fl));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_MESHCOMP_RANKS, (size_t)(R + 1) * 2 * sizeof(i64), &rk));
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_MESHCOMP_HEADS, (size_t)(R + 1) * sizeof(u32), &hp));
    // the scans of the call are the sorts' run tables and the flag arrays': size both scan slots for the largest now, so that none
    // regrows (and waits) midway
    PB3D_TRY(pb3d_scan_reserve(ctx, std::max<i64>(R, pb3d_sort_scan_items(R)), PB3D_SLOT_MESHCOMP_SCAN_LOCAL, PB3D_SLOT_MESHCOMP_SCAN_SEGS));
    *rec = {(u32*)ww, (u32*)kv, nullptr, (u32*)fl, (u32*)fl + R, (i64*)rk, (i64*)rk + (R + 1), (u32*)hp};
    return PB3D_OK;
}

int pb3d_mesh_edge_records_build(pb3d_ctx* ctx, const void* d_faces, int faces_i64, i64 nf, i64 nv, int* face_parent, unsigned long long* loops,
                                 pb3d_edge_records* rec) {
    const i64 R = 3 * nf;
    u32 *W = rec->W, *key = rec->pairs, *val = key + R, *key2 = key + 2 * R, *val2 = key + 3 * R;
    hipLaunchKernelGGL((faces_i64 ? k_records<true> : k_records<false>), grid_for(nf), dim3(256), 0, ctx->stream, d_faces, nf, nv, W, key, val, face_parent,
                       loops);
    PB3D_CHECK_LAUNCH();
    PB3D_TRY(sort(ctx, key, val, key2, val2, R, nv + 1));
    hipLaunchKernelGGL(k_next_key, grid_for(R), dim3(256), 0, ctx->stream, (const u32*)W, (const u32*)val, R, (u32)nv, key);
    PB3D_CHECK_LAUNCH();
    PB3D_TRY(sort(ctx, key, val, key2, val2, R, nv + 1));
    hipLaunchKernelGGL(k_heads, grid_for(R), dim3(256), 0, ctx->stream, (const u32*)W, (const u32*)val, R, rec->head, rec->fwd, face_parent);
    PB3D_CHECK_LAUNCH();
    PB3D_TRY(scan(ctx, rec->head, R, rec->head_rank));
    PB3D_TRY(scan(ctx, rec->fwd, R, rec->fwd_rank));
    hipLaunchKernelGGL(k_head_positions, grid_for(R + 1), dim3(256), 0, ctx->stream, (const u32*)W, (const u32*)val, R, (const u32*)rec->head,
                       (const i64*)rec->head_rank, rec->pos);
    PB3D_CHECK_LAUNCH();
    rec->val = val;
    return PB3D_OK;
}

int pb3d_forest_init(pb3d_ctx* ctx, int* parent, i64 n) {
    hipLaunchKernelGGL(k_iota, grid_for(n), dim3(256), 0, ctx->stream, parent, n);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

int pb3d_forest_flatten(pb3d_ctx* ctx, i64 n, int* parent, u32* root_flag) {
    hipLaunchKernelGGL(k_flatten, grid_for(n), dim3(256), 0, ctx->stream, n, parent, root_flag);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

// the segments' slot: [face counts | block counts] u32, [segment starts | block starts] int64, then the caller's bytes
static size_t seg_u32_bytes(i64 nf) { return (size_t)nf * 2 * sizeof(u32); }
static size_t seg_i64_bytes(i64 nf) { return (size_t)(nf + 1) * 2 * sizeof(i64); }

int pb3d_mesh_ordered_sums_reserve(pb3d_ctx* ctx, i64 nf, bool sums, size_t extra_bytes, void** extra) {
    void *sg, *ms;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_MESHCOMP_SEGMENTS, seg_u32_bytes(nf) + seg_i64_bytes(nf) + extra_bytes, &sg));
    if (sums) PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_MESHCOMP_MEASURES, (size_t)nf * 4 * sizeof(double), &ms));
    if (extra) *extra = (char*)sg + seg_u32_bytes(nf) + seg_i64_bytes(nf);
    return PB3D_OK;
}

int pb3d_mesh_ordered_sums(pb3d_ctx* ctx, const void* d_verts, int verts_f64, const pb3d_edge_records& rec, i64 nf, const int* face_labels,
                           const u32* negate, const unsigned long long* faces_of, const i64* nc, double* measures) {
    void *sg = ctx->scratch[PB3D_SLOT_MESHCOMP_SEGMENTS], *ms = ctx->scratch[PB3D_SLOT_MESHCOMP_MEASURES];     // _reserve's
    double *AS = (double*)ms, *block_sum = AS + 2 * nf;
    u32 *nfaces = (u32*)sg, *nblocks = nfaces + nf;
    i64 *seg_start = (i64*)((char*)sg + seg_u32_bytes(nf)), *block_start = seg_start + (nf + 1);
    u32 *key = rec.pairs, *val = key + nf, *key2 = key + 2 * nf, *val2 = key + 3 * nf;      // the records are spent
    if (verts_f64)
        hipLaunchKernelGGL(k_face_measures<true>, grid_for(nf), dim3(256), 0, ctx->stream, d_verts, (const u32*)rec.W, nf, face_labels, negate, AS, key, val);
    else
        hipLaunchKernelGGL(k_face_measures<false>, grid_for(nf), dim3(256), 0, ctx->stream, d_verts, (const u32*)rec.W, nf, face_labels, negate, AS, key, val);
    PB3D_CHECK_LAUNCH();
    PB3D_TRY(sort(ctx, key, val, key2, val2, nf, nf));
    hipLaunchKernelGGL(k_segment_counts, grid_for(nf), dim3(256), 0, ctx->stream, faces_of, nc, nf, nfaces, nblocks);
    PB3D_CHECK_LAUNCH();
    PB3D_TRY(scan(ctx, nfaces, nf, seg_start));
    PB3D_TRY(scan(ctx, nblocks, nf, block_start));
    hipLaunchKernelGGL(k_block_sums, dim3(pb3d_stream_blocks(ctx, nf / kBlock + nf / 64 + 1, 4, 32)), dim3(256), 0, ctx->stream, (const u32*)val,
                       (const double*)AS, (const i64*)seg_start, (const i64*)block_start, nc, block_sum);
    PB3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_component_sums, dim3(pb3d_stream_blocks(ctx, nf / 64 + 1, 4, 32)), dim3(256), 0, ctx->stream, (const double*)block_sum,
                       (const i64*)block_start, nc, measures);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

extern "C" {

int pb3d_mesh_components_resident(pb3d_ctx* ctx, const void* d_verts, int verts_f64, int64_t nv, const void* d_faces, int faces_i64, int64_t nf,
                                  int connectivity, int32_t* d_face_labels, int32_t* d_vertex_labels, int64_t* d_counts, double* d_measures,
                                  int64_t totals[8]) {
    const char* what = "pb3d_mesh_components";
    PB3D_REQUIRE(nv >= 0 && nf >= 0, "%s: negative count", what);
    PB3D_REQUIRE(nv <= kMaxVertices && nf <= kMaxFaces, "%s: at most 2^31 - 1 vertices and (2^31 - 1) / 6 faces", what);
    PB3D_REQUIRE(connectivity == PB3D_MESH_CONNECT_EDGE || connectivity == PB3D_MESH_CONNECT_VERTEX,
                 "%s: connectivity must be 0 (edge) or 1 (vertex) (got %d)", what, connectivity);
    PB3D_REQUIRE(totals != nullptr, "%s: null argument", what);
    PB3D_REQUIRE(d_measures == nullptr || d_verts != nullptr || nv == 0 || nf == 0, "%s: null buffer (the measures need the vertices)", what);
    PB3D_REQUIRE(nf == 0 || (d_faces && d_face_labels), "%s: null buffer", what);
    PB3D_REQUIRE(nf == 0 || ((const void*)d_face_labels != d_faces && (const void*)d_vertex_labels != d_faces && (const void*)d_counts != d_faces &&
                             (const void*)d_measures != d_faces && (d_verts == nullptr || ((const void*)d_face_labels != d_verts &&
                             (const void*)d_vertex_labels != d_verts && (const void*)d_counts != d_verts && (const void*)d_measures != d_verts))),
                 "%s: an output may not alias an input", what);
    PB3D_REQUIRE(ctx != nullptr, "%s: null context", what);
    if (nv == 0 && nf > 0) {
        pb3d_set_error("%s: index out of bounds for 0 entries", what);
        return PB3D_EINDEX;
    }
    PB3D_TRY(pb3d_check_index_range(ctx, d_faces, faces_i64, 3 * nf, -nv, nv, what));
    if (nf == 0) {                                             // no face: no component, and no vertex is named.  Enqueued
        if (d_vertex_labels && nv > 0) PB3D_HIP(hipMemsetAsync(d_vertex_labels, 0xff, (size_t)nv * sizeof(int), ctx->stream));
        for (int a = 0; a < 8; ++a) totals[a] = 0;
        return PB3D_OK;
    }
    const Args s = {d_verts, verts_f64, nv, d_faces, faces_i64, nf, connectivity == PB3D_MESH_CONNECT_EDGE, d_face_labels, d_vertex_labels,
                    d_counts, d_measures};
    return run(ctx, s, totals);
}

}  // extern "C"
