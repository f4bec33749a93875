// Members of selected components: the step after a labelling that extract_minaret_voxels_by_label and
// extract_minaret_masks_by_label (reference utils/camera_estimation.py:176-216, :247-325) need -- a few chosen components turned into
// their member coordinates (np.argwhere(labeled == id) order), their extreme-row sums (the keypoints of :329-336) and their 0/1 masks,
// walking each component's bounding box only.  The labelling itself is csrc/ccl.hip; nothing here touches its scratch.
//
// Work layout: the boxes of all selections are laid end to end in one launch, kBlockVox box voxels per workgroup, each workgroup
// inside one selection.  Coordinates are an ordered compaction, as the point extraction does it (csrc/points.hip): per-block member
// counts -> one-workgroup exclusive scan -> fill at the block's offset + in-block rank.  The row sums and the mask are written by the
// count pass, so a call that wants only those is one launch.
#include "pb3d_internal.h"
#include "wave.h"

namespace {

constexpr int kItems = 16;                  // 256-voxel sweeps per block
constexpr int kBlockVox = 256 * kItems;     // box voxels per block

struct MemSel {
    i64 lo0, lo1, lo2;
    u32 n1, n2, nvox;          // box extent along axes 1 and 2; box voxels (< 2^31)
    u32 blk0;                  // first block of the selection in the launch
    pb3d_magic d1, d2;         // exact division by n1, n2
    u32 color;                 // r | g << 8 | b << 16 (channels = 3) or the label value (channels = 1)
    int label;
    i64 out0, cap;             // first coordinate row of the selection and the rows it may fill (its count)
};

struct MemParams {
    i64 A1, A2, nvox_grid;
    int nsel, nblocks;
    MemSel s[PB3D_CCL_MAX_COLORS];
};

__device__ __forceinline__ int sel_of_block(const MemParams& p, u32 b) {
    int k = 0;
    for (int j = 1; j < p.nsel; ++j) k = b >= p.s[j].blk0 ? j : k;
    return k;
}

// box-local linear index -> grid voxel (and the box row b1); false past the end of the box
template <int C>
__device__ __forceinline__ bool member_at(const MemParams& p, const MemSel& s, const u8* __restrict__ grid, const int* __restrict__ labels, u32 li,
                                          i64* vox, u32* b0, u32* b1, u32* b2) {
    if (li >= s.nvox) return false;
    const u32 r = pb3d_div(li, s.d2);
    *b2 = li - r * s.n2;
    *b0 = pb3d_div(r, s.d1);
    *b1 = r - *b0 * s.n1;
    const i64 v = ((s.lo0 + *b0) * p.A1 + (s.lo1 + *b1)) * p.A2 + (s.lo2 + *b2);
    *vox = v;
    const u8* g = grid + v * C;
    const u32 c = C == 3 ? ((u32)g[0] | ((u32)g[1] << 8) | ((u32)g[2] << 16)) : (u32)g[0];
    // the label is read only where the colour matches: a members-only labelling leaves the other entries unspecified
    return c == s.color && labels[v] == s.label;
}

// pass 1: per-block member counts (COUNTS), bottom / top row sums (ROWS), mask bytes (MASK)
template <int C, bool COUNTS, bool ROWS, bool MASK>
__global__ __launch_bounds__(256) void k_members_count(const u8* __restrict__ grid, const int* __restrict__ labels, MemParams p,
                                                       u32* __restrict__ block_counts, unsigned long long* __restrict__ rows, u8* __restrict__ masks) {
    __shared__ u32 wsum[4];
    const int lane = threadIdx.x & 63;
    const int k = sel_of_block(p, blockIdx.x);
    const MemSel& s = p.s[k];
    const u32 base = (blockIdx.x - s.blk0) * (u32)kBlockVox;
    u32 cnt = 0;
    unsigned long long rs[8] = {0, 0, 0, 0, 0, 0, 0, 0};       // bottom {count, sum0, sum1, sum2}, top {...}
    for (int it = 0; it < kItems; ++it) {
        i64 v; u32 b0, b1, b2;
        const bool m = member_at<C>(p, s, grid, labels, base + it * 256 + threadIdx.x, &v, &b0, &b1, &b2);
        if (COUNTS) cnt += (u32)__popcll(__ballot(m));
        if (!m) continue;
        if (MASK) masks[(i64)k * p.nvox_grid + v] = 1;
        if (ROWS) {
            const unsigned long long c0 = (unsigned long long)(s.lo0 + b0), c1 = (unsigned long long)(s.lo1 + b1), c2 = (unsigned long long)(s.lo2 + b2);
            if (b1 == 0) { rs[0] += 1; rs[1] += c0; rs[2] += c1; rs[3] += c2; }
            if (b1 == s.n1 - 1) { rs[4] += 1; rs[5] += c0; rs[6] += c1; rs[7] += c2; }
        }
    }
    if (ROWS && __ballot(rs[0] != 0 || rs[4] != 0)) {
#pragma unroll
        for (int q = 0; q < 8; ++q) rs[q] = wave_sum(rs[q]);
        if (lane == 0)
            for (int q = 0; q < 8; ++q)
                if (rs[q]) atomicAdd(&rows[8 * k + q], rs[q]);
    }
    if (COUNTS) group_total<4>(cnt, wsum, [&](u32 tot) { block_counts[blockIdx.x] = tot; });
}

// exclusive scan of the block counts of the whole launch in one workgroup (a few hundred blocks for minaret boxes; a full 1024^3 box is
// 262144).  offsets[b] - offsets[blk0 of its selection] is the block's first row inside its selection.
__global__ __launch_bounds__(1024) void k_members_scan(const u32* __restrict__ counts, int nb, i64* __restrict__ offsets) {
    __shared__ i64 part[1024];
    group_scan_array(counts, (i64)nb, offsets, (i64*)nullptr, part);
}

// pass 2: coordinates (int64 a0, a1, a2) of the members at their rank inside the selection; never more than its `cap` rows
template <int C>
__global__ __launch_bounds__(256) void k_members_fill(const u8* __restrict__ grid, const int* __restrict__ labels, MemParams p,
                                                      const i64* __restrict__ offsets, i64* __restrict__ coords) {
    __shared__ u32 segoff[kItems * 4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int k = sel_of_block(p, blockIdx.x);
    const MemSel& s = p.s[k];
    const u32 base = (blockIdx.x - s.blk0) * (u32)kBlockVox;
    u64 bal[kItems];
#pragma unroll
    for (int it = 0; it < kItems; ++it) {
        i64 v; u32 b0, b1, b2;
        bal[it] = __ballot(member_at<C>(p, s, grid, labels, base + it * 256 + threadIdx.x, &v, &b0, &b1, &b2));
        if (lane == 0) segoff[it * 4 + w] = (u32)__popcll(bal[it]);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 run = 0;
        for (int i = 0; i < kItems * 4; ++i) { const u32 v = segoff[i]; segoff[i] = run; run += v; }
    }
    __syncthreads();
    const i64 first = offsets[blockIdx.x] - offsets[s.blk0];
    const u64 lt = lane ? (~0ull >> (64 - lane)) : 0ull;
#pragma unroll
    for (int it = 0; it < kItems; ++it) {
        if (!((bal[it] >> lane) & 1)) continue;
        const u32 li = base + it * 256 + threadIdx.x;
        const u32 r = pb3d_div(li, s.d2), b2 = li - r * s.n2, b0 = pb3d_div(r, s.d1), b1 = r - b0 * s.n1;
        const i64 pos = first + segoff[it * 4 + w] + __popcll(bal[it] & lt);
        if (pos >= s.cap) continue;
        i64* o = coords + 3 * (s.out0 + pos);
        o[0] = s.lo0 + b0; o[1] = s.lo1 + b1; o[2] = s.lo2 + b2;
    }
}

template <int C>
int launch_members(pb3d_ctx* ctx, const u8* d_grid, const int* d_labels, const MemParams& p, int outputs, u32* counts, i64* offsets,
                   int64_t* d_coords, int64_t* d_rows, uint8_t* d_masks) {
    const bool want_c = outputs & PB3D_MEMBERS_COORDS, want_r = outputs & PB3D_MEMBERS_ROWS, want_m = outputs & PB3D_MEMBERS_MASK;
    const dim3 g((unsigned)p.nblocks), b(256);
    unsigned long long* rows = (unsigned long long*)d_rows;
#define PB3D_MEMBERS_COUNT(CO, RO, MA) hipLaunchKernelGGL((k_members_count<C, CO, RO, MA>), g, b, 0, ctx->stream, d_grid, d_labels, p, counts, rows, d_masks)
    if (want_c && want_r && want_m) PB3D_MEMBERS_COUNT(true, true, true);
    else if (want_c && want_r) PB3D_MEMBERS_COUNT(true, true, false);
    else if (want_c && want_m) PB3D_MEMBERS_COUNT(true, false, true);
    else if (want_c) PB3D_MEMBERS_COUNT(true, false, false);
    else if (want_r && want_m) PB3D_MEMBERS_COUNT(false, true, true);
    else if (want_r) PB3D_MEMBERS_COUNT(false, true, false);
    else PB3D_MEMBERS_COUNT(false, false, true);
#undef PB3D_MEMBERS_COUNT
    PB3D_CHECK_LAUNCH();
    if (!want_c) return PB3D_OK;
    hipLaunchKernelGGL(k_members_scan, dim3(1), dim3(1024), 0, ctx->stream, (const u32*)counts, p.nblocks, offsets);
    PB3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_members_fill<C>, g, b, 0, ctx->stream, d_grid, d_labels, p, (const i64*)offsets, (i64*)d_coords);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

}  // namespace

extern "C" {

int pb3d_component_members_dev(pb3d_ctx* ctx, const uint8_t* d_grid, int64_t A0, int64_t A1, int64_t A2, int channels, const int32_t* d_labels,
                               int nsel, const uint8_t* colors, const int32_t* labels, const int64_t* bbox_lo_hi, const int64_t* counts, int outputs,
                               int64_t* d_coords, int64_t* d_rows, uint8_t* d_masks) {
    PB3D_REQUIRE(ctx != nullptr, "pb3d_component_members: null context");
    PB3D_REQUIRE(nsel >= 0 && nsel <= PB3D_CCL_MAX_COLORS, "pb3d_component_members: %d selections (at most %d)", nsel, PB3D_CCL_MAX_COLORS);
    PB3D_REQUIRE(channels == 1 || channels == 3, "pb3d_component_members: channels is 1 (labels) or 3 (colours)");
    PB3D_REQUIRE(A0 >= 0 && A1 >= 0 && A2 >= 0, "pb3d_component_members: bad shape");
    const i64 nvox = A0 * A1 * A2;
    PB3D_REQUIRE(nvox < (1ll << 31), "pb3d_component_members: grid too large for 32-bit labels");
    PB3D_REQUIRE(outputs > 0 && (outputs & ~(PB3D_MEMBERS_COORDS | PB3D_MEMBERS_ROWS | PB3D_MEMBERS_MASK)) == 0,
                 "pb3d_component_members: outputs is a non-empty set of PB3D_MEMBERS_COORDS | _ROWS | _MASK");
    if (nsel == 0) return PB3D_OK;
    PB3D_REQUIRE(colors && labels && bbox_lo_hi, "pb3d_component_members: null selection array");
    PB3D_REQUIRE(!(outputs & PB3D_MEMBERS_COORDS) || (d_coords && counts), "pb3d_component_members: coordinates requested with a null buffer");
    PB3D_REQUIRE(!(outputs & PB3D_MEMBERS_ROWS) || d_rows, "pb3d_component_members: row sums requested with a null buffer");
    PB3D_REQUIRE(!(outputs & PB3D_MEMBERS_MASK) || d_masks, "pb3d_component_members: masks requested with a null buffer");
    MemParams p;
    memset(&p, 0, sizeof(p));
    p.A1 = A1; p.A2 = A2; p.nvox_grid = nvox; p.nsel = nsel;
    i64 nb = 0, out0 = 0;
    for (int k = 0; k < nsel; ++k) {
        const int64_t* bb = bbox_lo_hi + 6 * k;
        PB3D_REQUIRE(bb[0] >= 0 && bb[1] >= 0 && bb[2] >= 0 && bb[0] <= bb[3] && bb[1] <= bb[4] && bb[2] <= bb[5] && bb[3] <= A0 && bb[4] <= A1 &&
                         bb[5] <= A2,
                     "pb3d_component_members: box %d [%lld,%lld,%lld)-[%lld,%lld,%lld) outside the grid (%lld,%lld,%lld)", k, (long long)bb[0],
                     (long long)bb[1], (long long)bb[2], (long long)bb[3], (long long)bb[4], (long long)bb[5], (long long)A0, (long long)A1, (long long)A2);
        PB3D_REQUIRE(!(outputs & PB3D_MEMBERS_COORDS) || counts[k] >= 0, "pb3d_component_members: negative count");
        MemSel& s = p.s[k];
        s.lo0 = bb[0]; s.lo1 = bb[1]; s.lo2 = bb[2];
        s.n1 = (u32)(bb[4] - bb[1]); s.n2 = (u32)(bb[5] - bb[2]);
        s.nvox = (u32)((bb[3] - bb[0]) * (i64)s.n1 * s.n2);
        s.d1 = pb3d_make_magic(s.n1 ? s.n1 : 1); s.d2 = pb3d_make_magic(s.n2 ? s.n2 : 1);
        s.color = channels == 3 ? ((u32)colors[3 * k] | ((u32)colors[3 * k + 1] << 8) | ((u32)colors[3 * k + 2] << 16)) : (u32)colors[k];
        s.label = labels[k];
        s.blk0 = (u32)nb;
        s.out0 = out0;
        s.cap = (outputs & PB3D_MEMBERS_COORDS) ? counts[k] : 0;
        out0 += s.cap;
        nb += ((i64)s.nvox + kBlockVox - 1) / kBlockVox;
    }
    // results of empty boxes are the cleared outputs
    if (outputs & PB3D_MEMBERS_ROWS) PB3D_HIP(hipMemsetAsync(d_rows, 0, (size_t)nsel * 8 * sizeof(int64_t), ctx->stream));
    if ((outputs & PB3D_MEMBERS_MASK) && nvox) PB3D_HIP(hipMemsetAsync(d_masks, 0, (size_t)nsel * (size_t)nvox, ctx->stream));
    if (nb == 0) return PB3D_OK;
    PB3D_REQUIRE(d_grid && d_labels, "pb3d_component_members: null grid or labels");
    p.nblocks = (int)nb;
    void *counts_d = nullptr, *offsets_d = nullptr;
    if (outputs & PB3D_MEMBERS_COORDS) {
        PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_MEMBERS_COUNTS, (size_t)nb * sizeof(u32), &counts_d));
        PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_MEMBERS_OFFSETS, (size_t)nb * sizeof(i64), &offsets_d));
    }
    if (channels == 3)
        return launch_members<3>(ctx, d_grid, d_labels, p, outputs, (u32*)counts_d, (i64*)offsets_d, d_coords, d_rows, d_masks);
    return launch_members<1>(ctx, d_grid, d_labels, p, outputs, (u32*)counts_d, (i64*)offsets_d, d_coords, d_rows, d_masks);
}

}  // extern "C"
