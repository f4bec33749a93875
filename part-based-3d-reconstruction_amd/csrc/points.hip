// K6: grid -> points.  Occupancy / colour-select with ORDERED stream compaction.
//
// reference utils/voxel_utils.py:7-21 (get_voxel_points_by_parts) and :35-51 (voxel_grid_to_points):
// both end in numpy.where(mask), i.e. the selected voxels in C order of (a0,a1,a2).  An unordered
// atomic append would break that, so compaction is a three-launch ordered scan: per-block popcounts
// (wave64 ballots) -> exclusive scan of the block counts -> fill at base + in-block rank.
#include "pb3d_internal.h"
#include "wave.h"

namespace {

constexpr int kItems = 16;                 // 256-voxel sweeps per block
constexpr int kBlockVox = 256 * kItems;    // lattice voxels per block

struct SelParams {
    i64 A1, A2;        // grid dims (axis 1, 2)
    i64 L1, L2, nlat;  // lattice dims ([::s]) and total lattice voxels
    int C, ncolors, stride;
    u8 colors[3 * 32];
    u32 colors32[32];   // the same colours packed r | g << 8 | b << 16
    // colour-set membership as ONE perfect-hash probe per voxel (stride-1 kernels): entry = bits 31..24 of
    // mul24(colour, hashK); htab[entry] = colour << 8 for the set's colours, 1 (never equal) elsewhere
    u32 hashK;
    u32 htab[256];
    pb3d_magic d2, d1;  // exact u32 division by A2 and by A1
    int labelsel;      // C == 1 with a label set (row N3: 1-byte label volumes): selected = label in the set (htab[label] == 2)
};

__device__ __forceinline__ i64 lattice_to_voxel(const SelParams& p, i64 li, i64* i0, i64* i1, i64* i2) {
    if (p.stride == 1) {
        *i2 = -1;  // coordinates derived lazily by the caller
        return li;
    }
    const i64 a2 = li % p.L2;
    const i64 r = li / p.L2;
    const i64 a1 = r % p.L1, a0 = r / p.L1;
    *i0 = a0; *i1 = a1; *i2 = a2;
    return ((a0 * p.stride) * p.A1 + a1 * p.stride) * p.A2 + a2 * p.stride;
}

__device__ __forceinline__ bool selected(const SelParams& p, const u8* __restrict__ grid, i64 vox) {
    const u8* g = grid + vox * p.C;
    if (p.labelsel) {
        bool s = false;
        for (int k = 0; k < p.ncolors; ++k) s |= g[0] == p.colors[k];
        return s;
    }
    if (p.ncolors > 0) {
        const u8 r = g[0], gg = g[1], b = g[2];
        bool s = false;
        for (int k = 0; k < p.ncolors; ++k) s |= (r == p.colors[3 * k]) & (gg == p.colors[3 * k + 1]) & (b == p.colors[3 * k + 2]);
        return s;
    }
    bool s = false;
    for (int c = 0; c < p.C; ++c) s |= g[c] != 0;
    return s;
}

__global__ __launch_bounds__(256) void k_points_count(const u8* __restrict__ grid, SelParams p, u32* __restrict__ block_counts) {
    __shared__ u32 wsum[4];
    const i64 base = (i64)blockIdx.x * kBlockVox;
    u32 cnt = 0;
    for (int it = 0; it < kItems; ++it) {
        const i64 li = base + it * 256 + threadIdx.x;
        bool sel = false;
        if (li < p.nlat) {
            i64 i0, i1, i2;
            sel = selected(p, grid, lattice_to_voxel(p, li, &i0, &i1, &i2));
        }
        cnt += (u32)__popcll(__ballot(sel));
    }
    group_total<4>(cnt, wsum, [&](u32 tot) { block_counts[blockIdx.x] = tot; });
}

// Exclusive scan of the nb block counts into 64-bit offsets, three small launches:
//   k_scan_local : 256 threads scan 1024 counts (one 16-byte load per thread) -> in-segment exclusive offsets + segment totals
//   k_scan_totals: one block scans the segment totals into 64-bit segment bases (+ grand total)
//   k_scan_add   : offsets[b] = base[b / 1024] + local[b]
constexpr int kSeg = 1024;

__global__ __launch_bounds__(256) void k_scan_local(const u32* __restrict__ counts, i64 nb, u32* __restrict__ local, u32* __restrict__ seg_total) {
    __shared__ u32 wsum[4];
    const i64 i0 = (i64)blockIdx.x * kSeg + 4 * threadIdx.x;
    u32 c[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = i0 + k < nb ? counts[i0 + k] : 0u;
    u32 before = group_excl_scan<256>(c[0] + c[1] + c[2] + c[3], wsum);
#pragma unroll
    for (int k = 0; k < 4; ++k) { if (i0 + k < nb) local[i0 + k] = before; before += c[k]; }
    if (threadIdx.x == 255) seg_total[blockIdx.x] = before;
}

__global__ __launch_bounds__(1024) void k_scan_totals(const u32* __restrict__ seg_total, i64 nseg, i64* __restrict__ seg_base, i64* __restrict__ total) {
    __shared__ i64 part[1024];
    group_scan_array(seg_total, nseg, seg_base, total, part);
}

__global__ __launch_bounds__(256) void k_scan_add(const u32* __restrict__ local, const i64* __restrict__ seg_base, i64 nb, i64* __restrict__ offsets) {
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < nb; i += (i64)gridDim.x * blockDim.x) offsets[i] = seg_base[i / kSeg] + local[i];
}

__global__ __launch_bounds__(256) void k_points_fill(const u8* __restrict__ grid, SelParams p, const i64* __restrict__ block_off,
                                                     float* __restrict__ pts, u8* __restrict__ cols) {
    __shared__ u32 segoff[kItems * 4 + 1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const i64 base = (i64)blockIdx.x * kBlockVox;
    u64 bal[kItems];
#pragma unroll
    for (int it = 0; it < kItems; ++it) {
        const i64 li = base + it * 256 + threadIdx.x;
        bool sel = false;
        if (li < p.nlat) {
            i64 i0, i1, i2;
            sel = selected(p, grid, lattice_to_voxel(p, li, &i0, &i1, &i2));
        }
        bal[it] = __ballot(sel);
        if (lane == 0) segoff[it * 4 + w] = (u32)__popcll(bal[it]);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 run = 0;
        for (int i = 0; i < kItems * 4; ++i) { const u32 v = segoff[i]; segoff[i] = run; run += v; }
    }
    __syncthreads();
    const i64 out0 = block_off[blockIdx.x];
    const u64 lt = lane ? (~0ull >> (64 - lane)) : 0ull;
#pragma unroll
    for (int it = 0; it < kItems; ++it) {
        if (!((bal[it] >> lane) & 1)) continue;
        const i64 li = base + it * 256 + threadIdx.x;
        const i64 a2 = li % p.L2;
        const i64 r = li / p.L2;
        const i64 a1 = r % p.L1, a0 = r / p.L1;
        const i64 vox = ((a0 * p.stride) * p.A1 + a1 * p.stride) * p.A2 + a2 * p.stride;
        const i64 pos = out0 + segoff[it * 4 + w] + __popcll(bal[it] & lt);
        const float s = (float)p.stride;
        pts[3 * pos + 0] = __fmul_rn((float)a2, s);
        pts[3 * pos + 1] = __fmul_rn((float)a1, s);
        pts[3 * pos + 2] = __fmul_rn((float)a0, s);
        for (int c = 0; c < p.C; ++c) cols[p.C * pos + c] = grid[vox * p.C + c];
    }
}

// ------------------------------------------------------------------------------------------------
// stride == 1, RGB grids: 16 consecutive voxels per thread (48 bytes as three 16-byte loads), so a
// block still covers kBlockVox = 4096 voxels in lattice order and shares the block-count scan with the
// generic kernels.  In-block order = thread order (thread t owns voxels 16t .. 16t+15).
// ------------------------------------------------------------------------------------------------
typedef u32 u32x4v __attribute__((ext_vector_type(4)));

__device__ __forceinline__ u32 select16(const SelParams& p, const u32* htab, const u8* __restrict__ grid, i64 v0, i64 nvox, u32 w[12]) {
    // loads the 48 bytes of voxels v0..v0+15 (bounds-checked at the grid's end) and returns their 16 select bits
    if (v0 + 16 <= nvox) {
        const u32x4v* g = (const u32x4v*)(grid + 3 * v0);
#pragma unroll
        for (int k = 0; k < 3; ++k) { const u32x4v t = g[k]; w[4 * k] = t.x; w[4 * k + 1] = t.y; w[4 * k + 2] = t.z; w[4 * k + 3] = t.w; }
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            u32 t = 0;
            for (int b = 0; b < 4; ++b) { const i64 o = 3 * v0 + 4 * k + b; if (o < 3 * nvox) t |= (u32)grid[o] << (8 * b); }
            w[k] = t;
        }
    }
    u32 bits = 0;
    if (p.ncolors > 0 && p.hashK) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int j = (3 * i) >> 2, sh = (3 * i) & 3;
            const u32 v = __builtin_amdgcn_alignbyte(j + 1 < 12 ? w[j + 1] : 0u, w[j], (u32)sh);   // top byte: the next voxel's red
            const u32 e = (__umul24(v, p.hashK) >> 22) & 0x3fcu;                                  // mul24 ignores the top byte
            bits |= (u32)((v << 8) == *(const u32*)((const u8*)htab + e)) << i;
        }
    } else if (p.ncolors > 0) {                  // no collision-free multiplier found (practically never): compare loop
        u32 vox[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int j = (3 * i) >> 2, sh = (3 * i) & 3;
            vox[i] = __builtin_amdgcn_alignbyte(j + 1 < 12 ? w[j + 1] : 0u, w[j], (u32)sh) & 0x00ffffffu;
        }
        for (int k = 0; k < p.ncolors; ++k) {
            const u32 ck = p.colors32[k];
#pragma unroll
            for (int i = 0; i < 16; ++i) bits |= (u32)(vox[i] == ck) << i;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int j = (3 * i) >> 2, sh = (3 * i) & 3;
            bits |= (u32)((__builtin_amdgcn_alignbyte(j + 1 < 12 ? w[j + 1] : 0u, w[j], (u32)sh) << 8) != 0u) << i;
        }
    }
    const i64 left = nvox - v0;
    if (left < 16) bits &= (1u << left) - 1u;
    return bits;
}

// occupancy grids (C == 1): the 16 voxels are one 16-byte load; selected = byte != 0
__device__ __forceinline__ u32 select16_occ(const u8* __restrict__ grid, i64 v0, i64 nvox, u32 w[4], const u32* htab = nullptr) {
    if (v0 + 16 <= nvox) {
        const u32x4v t = *(const u32x4v*)(grid + v0);
        w[0] = t.x; w[1] = t.y; w[2] = t.z; w[3] = t.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            u32 t = 0;
            for (int b = 0; b < 4; ++b) { const i64 o = v0 + 4 * k + b; if (o < nvox) t |= (u32)grid[o] << (8 * b); }
            w[k] = t;
        }
    }
    u32 bits = 0;
    if (htab) {          // label volumes: one table read per voxel (htab[label] == 2 for the labels of the set)
#pragma unroll
        for (int i = 0; i < 16; ++i) bits |= (u32)(htab[(w[i >> 2] >> (8 * (i & 3))) & 0xffu] == 2u) << i;
        const i64 left = nvox - v0;
        if (left < 16) bits &= (1u << left) - 1u;
        return bits;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) bits |= (u32)(((w[i >> 2] >> (8 * (i & 3))) & 0xffu) != 0u) << i;
    return bits;
}

// masks (one u16 per thread = per 16 voxels, n / 8 bytes in all): the fill pass takes the selection from them instead of recomputing it,
// and loads the grid only where something is selected -- an empty 128-byte line is then read once (here), not twice.
template <int C>
__global__ __launch_bounds__(256) void k_points_count16(const u8* __restrict__ grid, SelParams p, u32* __restrict__ block_counts,
                                                        unsigned short* __restrict__ masks) {
    __shared__ u32 wsum[4];
    __shared__ u32 htab[256];
    htab[threadIdx.x] = p.htab[threadIdx.x];
    __syncthreads();
    const i64 v0 = (i64)blockIdx.x * kBlockVox + 16 * threadIdx.x;
    u32 w[12];
    const u32 sel = v0 < p.nlat ? (C == 3 ? select16(p, htab, grid, v0, p.nlat, w) : select16_occ(grid, v0, p.nlat, w, p.labelsel ? htab : nullptr)) : 0u;
    masks[(i64)blockIdx.x * 256 + threadIdx.x] = (unsigned short)sel;
    group_total<4>(wave_sum((u32)__popc(sel)), wsum, [&](u32 tot) { block_counts[blockIdx.x] = tot; });
}

// ------------------------------------------------------------------------------------------------
// The fill pass of the 16-voxel kernels, WAVE-PRIVATE: a block-wide form (rank -> LDS -> coordinates -> colours behind five block
// barriers, 31 KB of LDS) was bound by that chain and its LDS bank conflicts, not by its bytes.
// Every wavefront is on its own: it owns 1024 consecutive voxels (a quarter of a count-pass block), finds its output offset
// from the block's scanned offset + the popcounts of the earlier waves' masks, and walks its voxels in four rounds of 256 -- lane l
// takes voxels 4 l .. 4 l + 3 of the round, so a round's points are contiguous in the output and every lane takes part in every
// step.  Per round: rank inside the wave (one shuffle scan), coordinates from the lane's first voxel (one pair of exact
// multiply-high divisions per LANE and round, then increments), the points' floats scattered into a wave-private LDS window at the
// phase of the output address, whole 16-byte pieces stored (1 KB contiguous per instruction), the last partial piece carried into
// the next round; the colours likewise as 24-bit records strung into aligned dwords, four records = three dwords at a time.
// No block barrier, 4.2 KB of LDS per wave.  All four rounds' loads (12 bytes per lane where something is selected) are in flight
// before the first is used.
// ------------------------------------------------------------------------------------------------
typedef u32 u32x3v_a4 __attribute__((ext_vector_type(3), aligned(4)));
typedef float f32x4w __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int C>
__global__ __launch_bounds__(256) void k_points_fillw(const u8* __restrict__ grid, SelParams p, const i64* __restrict__ block_off,
                                                      float* __restrict__ pts, u8* __restrict__ cols, const unsigned short* __restrict__ masks) {
    constexpr int FW = 4 + 3 * 256 + 4;                  // floats: <= 3 carried + 768 of a round
    constexpr int RW = 8 + 256 + 8;                      // records: <= 8 waiting + 256 of a round + the over-read of the last group
    __shared__ __attribute__((aligned(16))) float fwin[4][FW];
    __shared__ __attribute__((aligned(16))) u32 rwin[4][RW];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const u32 bid = blockIdx.x;
    const i64 wbase = (i64)bid * kBlockVox + 1024 * wv;
    if (wbase >= p.nlat) return;                          // (whole wave; the kernel has no block barrier)
    const unsigned short* bm = masks + (i64)bid * 256;
    const u32 mymask = bm[64 * wv + lane];                // selection of voxels wbase + 16 lane .. + 15 (bits past the grid's end are zero)
    u32 pre = 0;
    for (int q = 0; q < wv; ++q) pre += (u32)__popc((u32)bm[64 * q + lane]);
    pre = wave_sum(pre);
    const u32 tot = wave_sum((u32)__popc(mymask));
    if (tot == 0) return;
    const i64 out0 = block_off[bid] + pre;
    float* fw = fwin[wv];
    u32* rw = rwin[wv];
    // ---- all loads of the wave
    u32 sel[4];
    u32 w[4][C == 3 ? 3 : 1];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const u32 m = (u32)__shfl((int)mymask, 16 * r + (lane >> 2));
        sel[r] = (m >> (4 * (lane & 3))) & 0xfu;
#pragma unroll
        for (int k = 0; k < (C == 3 ? 3 : 1); ++k) w[r][k] = 0u;
        if (sel[r]) {
            const i64 v = wbase + 256 * r + 4 * lane;
            if (v + 4 <= p.nlat) {
                if (C == 3) { const u32x3v_a4 t = *(const u32x3v_a4*)(grid + 3 * v); w[r][0] = t.x; w[r][1] = t.y; w[r][2] = t.z; }
                else w[r][0] = *(const u32*)(grid + v);
            } else {                                      // the grid's ragged end
                for (int b = 0; b < 4 * (C == 3 ? 3 : 1); ++b)
                    if (C * v + b < C * p.nlat) w[r][b >> 2] |= (u32)grid[C * v + b] << (8 * (b & 3));
            }
        }
    }
    // ---- the wave's first voxel -> (b0, b1, b2): one 64-bit division pair per wave (wbase reaches 2^43)
    const u64 rr = (u64)wbase / (u64)p.A2;
    const u64 b0 = rr / (u64)p.A1;
    const u32 b2 = (u32)((u64)wbase - rr * (u64)p.A2), b1 = (u32)(rr - b0 * (u64)p.A1);
    // ---- output streams
    float* gout = pts + 3 * out0;
    const u32 shift = (u32)(((uintptr_t)gout >> 2) & 3u);           // floats past a 16-byte boundary
    float* gal = gout - shift;                                      // aligned; fw[i] <-> gal[i]
    u32 pend = shift, first_lo = shift;                             // floats [0, first_lo) of the first piece belong to the wave before
    u8* co = cols + (i64)C * out0;
    const u32 nbytes = (u32)C * tot;
    const u32 head = (u32)((4 - ((uintptr_t)co & 3u)) & 3u);
    const u32 hb = head < nbytes ? head : nbytes;                   // bytes up to the first dword boundary of the colour stream
    u32* cw = (u32*)(co + hb);
    // records: record k of the wave sits at window index k + roff until the first compaction; groups start at multiples of 4
    const u32 r00 = C == 3 ? hb / 3 : hb, ph = C == 3 ? hb - 3 * r00 : 0u;      // first record / byte phase of the aligned dwords
    const u32 roff = (4u - r00) & 3u;
    u32 rfill = roff, gidx = r00 ? 4u : 0u, gdone = 0;
    bool head_done = hb == 0;
    auto emit_head = [&]() {
        if ((u32)lane < hb) co[lane] = C == 3 ? (u8)(rw[roff] >> (8 * lane)) : (u8)rw[roff + lane];
        head_done = true;
    };
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const u32 c = (u32)__popc(sel[r]);
        const u32 inc = wave_incl_scan(c);
        const u32 n = (u32)__builtin_amdgcn_readlane((int)inc, 63);
        if (n == 0) continue;
        // ---- scatter: coordinates and colour records of this lane's selected voxels
        {
            const u32 x = b2 + 256u * r + 4u * lane;                 // < A2 + 1024
            const u32 q2 = pb3d_div(x, p.d2);
            u32 a2 = x - q2 * (u32)p.A2;
            const u32 y = b1 + q2;                                   // < A1 + 1024
            const u32 q1 = pb3d_div(y, p.d1);
            u32 a1 = y - q1 * (u32)p.A1;
            u64 a0 = b0 + q1;
            float f0 = (float)a0;                                    // converted once per lane and round: a u64 -> float is eight instructions
            u32 k = inc - c;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if ((sel[r] >> i) & 1u) {
                    float* l = fw + pend + 3 * k;
                    l[0] = (float)a2; l[1] = (float)a1; l[2] = f0;
                    u32 rec;
                    if (C == 3) {
                        const int j = (3 * i) >> 2, sh = (3 * i) & 3;
                        rec = __builtin_amdgcn_alignbyte(j + 1 < 3 ? w[r][j + 1 < 3 ? j + 1 : 0] : 0u, w[r][j], (u32)sh) & 0x00ffffffu;
                    } else rec = (w[r][0] >> (8 * i)) & 0xffu;
                    rw[rfill + k] = rec;
                    ++k;
                }
                if (++a2 == (u32)p.A2) { a2 = 0; if (++a1 == (u32)p.A1) { a1 = 0; f0 = (float)++a0; } }
            }
        }
        wave_sync();
        // ---- points: whole 16-byte pieces leave, the rest is carried
        {
            const u32 nfl = pend + 3 * n, npc = nfl >> 2, left = nfl & 3u;
            for (u32 pz = lane; pz < npc; pz += 64) {
                if (pz == 0 && first_lo) { for (u32 f = first_lo; f < 4; ++f) gal[f] = fw[f]; }
                else *(f32x4w*)(gal + 4 * pz) = *(const f32x4w*)(fw + 4 * pz);      // (nontemporal stores measured slower here: fill 1.47 -> 1.62 ms at 1024^3)
            }
            if (npc) {
                first_lo = 0;
                float t = 0.f;
                if ((u32)lane < left) t = fw[4 * npc + lane];
                wave_sync();
                if ((u32)lane < left) fw[lane] = t;
                gal += 4 * npc; pend = left;
            } else pend = nfl;
        }
        // ---- colours: groups of four records = C dwords whose records (C == 3: and the one behind them) have arrived
        {
            rfill += n;
            const u32 need = C == 3 ? 1u : 0u;
            const u32 ng = rfill >= gidx + need ? (rfill - gidx - need) >> 2 : 0u;
            if (ng) {
                if (!head_done) emit_head();
                for (u32 g = lane; g < ng; g += 64) {
                    const u32x4v va = *(const u32x4v*)(rw + gidx + 4 * g);
                    if (C == 3) {
                        const u32 e4 = rw[gidx + 4 * g + 4];
                        const u32 W0 = va.x | (va.y << 24), W1 = (va.y >> 8) | (va.z << 16), W2 = (va.z >> 16) | (va.w << 8), W3 = e4;
                        u32* d = cw + 3 * (gdone + g);
                        d[0] = __builtin_amdgcn_alignbyte(W1, W0, ph); d[1] = __builtin_amdgcn_alignbyte(W2, W1, ph);
                        d[2] = __builtin_amdgcn_alignbyte(W3, W2, ph);
                    } else cw[gdone + g] = va.x | (va.y << 8) | (va.z << 16) | (va.w << 24);
                }
                const u32 src = gidx + 4 * ng, rem = rfill - src;      // <= 4 records wait for the next round
                u32 t = 0;
                if ((u32)lane < rem) t = rw[src + lane];
                wave_sync();
                if ((u32)lane < rem) rw[lane] = t;
                gdone += ng; gidx = 0; rfill = rem;
            }
        }
        wave_sync();
    }
    // ---- the ends of the two streams
    if ((u32)lane >= first_lo && (u32)lane < pend) gal[lane] = fw[lane];
    if (!head_done) emit_head();
    {
        const u32 q0 = hb + 4 * (u32)C * gdone;               // first stream byte that has not left
        if (q0 < nbytes && (u32)lane < nbytes - q0) {
            if (C == 3) { const u32 bo = ph + lane, rr = (bo * 43691u) >> 17; co[q0 + lane] = (u8)(rw[gidx + rr] >> (8 * (bo - 3 * rr))); }
            else co[q0 + lane] = (u8)rw[gidx + lane];
        }
    }
}

int make_params(i64 A0, i64 A1, i64 A2, int C, const u8* colors, int ncolors, int stride, SelParams* p) {
    PB3D_REQUIRE(A0 >= 0 && A1 >= 0 && A2 >= 0 && (C == 1 || C == 3), "pb3d_points: bad shape (%lld,%lld,%lld,%d)",
                 (long long)A0, (long long)A1, (long long)A2, C);
    PB3D_REQUIRE(stride >= 1, "pb3d_points: stride must be >= 1");
    PB3D_REQUIRE(ncolors >= 0 && ncolors <= 32, "pb3d_points: at most 32 colours");
    PB3D_REQUIRE(ncolors == 0 || colors, "pb3d_points: null colour set");      // C == 1: `colors` holds ncolors 1-byte LABELS
    p->A1 = A1; p->A2 = A2;
    const i64 L0 = (A0 + stride - 1) / stride;
    p->L1 = (A1 + stride - 1) / stride; p->L2 = (A2 + stride - 1) / stride;
    p->nlat = L0 * p->L1 * p->L2;
    p->d2 = pb3d_make_magic((u32)(A2 > 0 ? A2 : 1)); p->d1 = pb3d_make_magic((u32)(A1 > 0 ? A1 : 1));
    p->C = C; p->ncolors = ncolors; p->stride = stride;
    memset(p->colors, 0, sizeof(p->colors));
    p->labelsel = (C == 1 && ncolors > 0) ? 1 : 0;
    if (p->labelsel) {
        memcpy(p->colors, colors, (size_t)ncolors);
        for (int k = 0; k < 32; ++k) p->colors32[k] = 0xffffffffu;
        p->hashK = 0;
        for (int e = 0; e < 256; ++e) p->htab[e] = 1u;
        for (int k = 0; k < ncolors; ++k) p->htab[colors[k]] = 2u;
        return PB3D_OK;
    }
    if (ncolors) memcpy(p->colors, colors, (size_t)3 * ncolors);
    for (int k = 0; k < 32; ++k)
        p->colors32[k] = k < ncolors ? ((u32)colors[3 * k] | ((u32)colors[3 * k + 1] << 8) | ((u32)colors[3 * k + 2] << 16)) : 0xffffffffu;
    // perfect hash of the colour set: first odd 24-bit multiplier of a fixed sequence under which all (distinct)
    // colours fall into different entries of the 256-entry table
    p->hashK = 0;
    for (int e = 0; e < 256; ++e) p->htab[e] = 1u;
    if (ncolors > 0) {
        u32 K = 0x9e3779u;
        for (int attempt = 0; attempt < (1 << 16) && !p->hashK; ++attempt) {
            K = (K * 1664525u + 1013904223u) & 0xffffffu;
            const u32 Ko = K | 1u;
            u32 tab[256];
            for (int e = 0; e < 256; ++e) tab[e] = 1u;
            bool ok = true;
            for (int k = 0; k < ncolors && ok; ++k) {
                const u32 c = p->colors32[k];
                const u32 e = (u32)(((unsigned long long)c * Ko) & 0xffffffffull) >> 24;
                if (tab[e] == 1u) tab[e] = c << 8;
                else if (tab[e] != (c << 8)) ok = false;        // a repeated colour is not a collision
            }
            if (ok) { p->hashK = Ko; memcpy(p->htab, tab, sizeof(tab)); }
        }
    }
    return PB3D_OK;
}

bool aligned16(const u8* d_grid, int stride) { return stride == 1 && (((uintptr_t)d_grid) & 15u) == 0; }

// The count pass and the scan of the block counts; *n = the number of selected voxels.  What the fill pass of the same grid and selection
// reads stays in the context's scratch: the scanned block offsets in slot off_slot and (the 16-voxel kernels) the selection masks in
// slot mask_slot.  Synchronises (returns *n).
int count_pass(pb3d_ctx* ctx, const u8* d_grid, const SelParams& p, bool fast16, pb3d_slot off_slot, pb3d_slot mask_slot, i64* n) {
    const i64 nb = (p.nlat + kBlockVox - 1) / kBlockVox;
    void *counts, *offsets;
    PB3D_TRY(pb3d_scratch(ctx, PB3D_SLOT_BLOCK_COUNTS, (size_t)nb * sizeof(u32), &counts));
    PB3D_TRY(pb3d_scratch(ctx, off_slot, (size_t)(nb + 1) * sizeof(i64), &offsets));
    void* masks = nullptr;
    if (fast16) PB3D_TRY(pb3d_scratch(ctx, mask_slot, (size_t)nb * 256 * sizeof(unsigned short), &masks));
    if (fast16 && p.C == 3) hipLaunchKernelGGL(k_points_count16<3>, dim3((unsigned)nb), dim3(256), 0, ctx->stream, d_grid, p, (u32*)counts, (unsigned short*)masks);
    else if (fast16) hipLaunchKernelGGL(k_points_count16<1>, dim3((unsigned)nb), dim3(256), 0, ctx->stream, d_grid, p, (u32*)counts, (unsigned short*)masks);
    else hipLaunchKernelGGL(k_points_count, dim3((unsigned)nb), dim3(256), 0, ctx->stream, d_grid, p, (u32*)counts);
    PB3D_CHECK_LAUNCH();
    PB3D_TRY(pb3d_scan_counts(ctx, (const u32*)counts, nb, (i64*)offsets, PB3D_SLOT_SCAN_LOCAL, PB3D_SLOT_SCAN_SEGS));
    return pb3d_read_back(ctx, n, (const i64*)offsets + nb, sizeof(i64));
}

// The fill pass after count_pass(off_slot, mask_slot) on the same grid and selection.  d_pts: n*3 floats, d_cols: n*C bytes.
int fill_pass(pb3d_ctx* ctx, const u8* d_grid, const SelParams& p, bool fast16, pb3d_slot off_slot, pb3d_slot mask_slot, float* d_pts, u8* d_cols) {
    const i64 nb = (p.nlat + kBlockVox - 1) / kBlockVox;
    PB3D_REQUIRE(ctx->scratch[off_slot] && ctx->scratch_bytes[off_slot] >= (size_t)(nb + 1) * sizeof(i64),
                 "pb3d_points_fill: call pb3d_points_count first");
    PB3D_REQUIRE(!fast16 || (ctx->scratch[mask_slot] && ctx->scratch_bytes[mask_slot] >= (size_t)nb * 256 * sizeof(unsigned short)),
                 "pb3d_points_fill: call pb3d_points_count first");
    const i64* off = (const i64*)ctx->scratch[off_slot];
    const unsigned short* masks = (const unsigned short*)ctx->scratch[mask_slot];
    if (fast16 && p.C == 1) hipLaunchKernelGGL((k_points_fillw<1>), dim3((unsigned)nb), dim3(256), 0, ctx->stream, d_grid, p, off, d_pts, d_cols, masks);
    else if (fast16) hipLaunchKernelGGL((k_points_fillw<3>), dim3((unsigned)nb), dim3(256), 0, ctx->stream, d_grid, p, off, d_pts, d_cols, masks);
    else hipLaunchKernelGGL(k_points_fill, dim3((unsigned)nb), dim3(256), 0, ctx->stream, d_grid, p, off, d_pts, d_cols);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

}  // namespace

// The exclusive scan of count_pass on any u32 count array (the cell index of csrc/nn.hip): offsets[0..n) and offsets[n] = total.
// Slot local_slot holds n u32 in-segment offsets, slot seg_slot the segment bases (int64) and then the segment totals (u32).
int pb3d_scan_reserve(pb3d_ctx* ctx, i64 n, pb3d_slot local_slot, pb3d_slot seg_slot) {
    void* p;
    PB3D_TRY(pb3d_scratch(ctx, local_slot, (size_t)n * sizeof(u32), &p));
    return pb3d_scratch(ctx, seg_slot, (size_t)((n + kSeg - 1) / kSeg) * (sizeof(u32) + sizeof(i64)), &p);
}

// Enqueue only.
int pb3d_scan_counts(pb3d_ctx* ctx, const u32* d_counts, i64 n, i64* d_offsets, pb3d_slot local_slot, pb3d_slot seg_slot) {
    const i64 nseg = (n + kSeg - 1) / kSeg;
    PB3D_TRY(pb3d_scan_reserve(ctx, n, local_slot, seg_slot));
    void *local = ctx->scratch[local_slot], *segs = ctx->scratch[seg_slot];
    i64* seg_base = (i64*)segs;
    u32* seg_total = (u32*)(seg_base + nseg);
    hipLaunchKernelGGL(k_scan_local, dim3((unsigned)nseg), dim3(256), 0, ctx->stream, d_counts, n, (u32*)local, seg_total);
    PB3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_scan_totals, dim3(1), dim3(1024), 0, ctx->stream, (const u32*)seg_total, nseg, seg_base, d_offsets + n);
    PB3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_scan_add, dim3(pb3d_stream_blocks(ctx, n, 256, 8)), dim3(256), 0, ctx->stream, (const u32*)local,
                       (const i64*)seg_base, n, d_offsets);
    PB3D_CHECK_LAUNCH();
    return PB3D_OK;
}

extern "C" {

int pb3d_points_count_dev(pb3d_ctx* ctx, const uint8_t* d_grid, int64_t A0, int64_t A1, int64_t A2, int C,
                          const uint8_t* colors, int ncolors, int stride, int64_t* n) {
    PB3D_REQUIRE(ctx != nullptr && n != nullptr, "pb3d_points_count: null argument");
    ctx->pts_dev.pair.valid = false;
    SelParams p;
    PB3D_TRY(make_params(A0, A1, A2, C, colors, ncolors, stride, &p));
    *n = 0;
    if (p.nlat == 0) return PB3D_OK;
    PB3D_REQUIRE(d_grid != nullptr, "pb3d_points_count: null grid");
    PB3D_REQUIRE((p.nlat + kBlockVox - 1) / kBlockVox < (1ll << 31), "pb3d_points_count: grid too large");
    PB3D_TRY(count_pass(ctx, d_grid, p, aligned16(d_grid, stride), PB3D_SLOT_POINTS_OFFSETS, PB3D_SLOT_POINTS_MASKS, n));
    ctx->pts_dev.a = pb3d_points_args(d_grid, A0, A1, A2, C, colors, ncolors, stride, *n);
    pb3d_pair_record(ctx, &ctx->pts_dev.pair, {PB3D_SLOT_POINTS_OFFSETS, PB3D_SLOT_POINTS_MASKS});
    return PB3D_OK;
}

// Must follow pb3d_points_count_dev with identical arguments on the same context (the scanned block offsets and the selection masks
// stay in the context's scratch, PB3D_SLOT_POINTS_OFFSETS and PB3D_SLOT_POINTS_MASKS).  d_pts: n*3 floats, d_cols: n*C bytes.
int pb3d_points_fill_dev(pb3d_ctx* ctx, const uint8_t* d_grid, int64_t A0, int64_t A1, int64_t A2, int C,
                         const uint8_t* colors, int ncolors, int stride, int64_t n, float* d_pts, uint8_t* d_cols) {
    PB3D_REQUIRE(ctx != nullptr, "pb3d_points_fill: null context");
    SelParams p;
    PB3D_TRY(make_params(A0, A1, A2, C, colors, ncolors, stride, &p));
    if (p.nlat == 0 || n == 0) return PB3D_OK;
    PB3D_REQUIRE(d_grid && d_pts && d_cols, "pb3d_points_fill: null buffer");
    PB3D_TRY(pb3d_pair_check(ctx, ctx->pts_dev.pair, pb3d_same_args(ctx->pts_dev.a, pb3d_points_args(d_grid, A0, A1, A2, C, colors, ncolors, stride, n)),
                             "pb3d_points_fill", "pb3d_points_count"));
    return fill_pass(ctx, d_grid, p, aligned16(d_grid, stride), PB3D_SLOT_POINTS_OFFSETS, PB3D_SLOT_POINTS_MASKS, d_pts, d_cols);
}

// count + fill in one call.  Its state lives in PB3D_SLOT_EXTRACT_OFFSETS / _MASKS, so a count -> fill pair of the two entries above
// may have this call between its halves.
int pb3d_points_extract_dev(pb3d_ctx* ctx, const uint8_t* d_grid, int64_t A0, int64_t A1, int64_t A2, int C, const uint8_t* colors, int ncolors,
                            int64_t capacity, float* d_pts, uint8_t* d_cols, int64_t* n) {
    PB3D_REQUIRE(ctx != nullptr && n != nullptr && capacity >= 0, "pb3d_points_extract: bad argument");
    *n = 0;
    SelParams p;
    PB3D_TRY(make_params(A0, A1, A2, C, colors, ncolors, 1, &p));
    if (p.nlat == 0) return PB3D_OK;
    PB3D_REQUIRE(d_grid && (capacity == 0 || (d_pts && d_cols)), "pb3d_points_extract: null buffer");
    PB3D_REQUIRE(aligned16(d_grid, 1), "pb3d_points_extract: needs a 16-byte aligned grid");
    PB3D_REQUIRE((p.nlat + kBlockVox - 1) / kBlockVox < (1ll << 31), "pb3d_points_extract: grid too large");
    PB3D_TRY(count_pass(ctx, d_grid, p, true, PB3D_SLOT_EXTRACT_OFFSETS, PB3D_SLOT_EXTRACT_MASKS, n));
    if (*n == 0 || *n > capacity) return PB3D_OK;
    PB3D_TRY(fill_pass(ctx, d_grid, p, true, PB3D_SLOT_EXTRACT_OFFSETS, PB3D_SLOT_EXTRACT_MASKS, d_pts, d_cols));
    return pb3d_stream_sync(ctx);
}

}  // extern "C"
