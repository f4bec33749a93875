// Device pieces shared by the 90-degree kernels of csrc/rotate_tiled.hip.  Every private-array index below is a compile-time constant
// (loops fully unrolled, runtime guards inside): an array indexed at run time is placed in scratch memory.
#pragma once
#include "rot_common.h"
#include "lane48.h"

namespace {

typedef u32 u32_u __attribute__((aligned(1)));

// d[15 - q]: the 4 bytes of the LDS row that holds output byte q, byte i of them for output row i  ->  o[i][w]: bytes 4w .. 4w+3 of
// the 16-byte run of row i
__device__ __forceinline__ void transpose16x4(const u32 d[16], u32 o[4][4]) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        u32 v[4];
        tr4x4(d[15 - 4 * w], d[14 - 4 * w], d[13 - 4 * w], d[12 - 4 * w], v);
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i][w] = v[i];
    }
}

// a thread's four source pieces into local rows lr0 + STEP j of the row-major LDS tile of NB 16-byte blocks per row (the blocks of a
// row XOR-swizzled by its row group, so that transpose16x4's column reads are bank-conflict free); a piece whose bit in `on` is clear
// is stored as zeros
template <int NB, int STEP>
__device__ __forceinline__ void stage4(u8* tile, int lr0, int cb, const u32x4 stg[4], u32 on) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int lr = lr0 + STEP * j;
        *(u32x4*)(tile + lr * 16 * NB + 16 * (cb ^ ((lr >> 4) & (NB - 1)))) = ((on >> j) & 1u) ? stg[j] : (u32x4)(0u);
    }
}

// 16 validity bits of row x for z = zlo .. zlo + 15 from the k_rot_valid table (row stride nw words): zero outside [0, D) -- the
// table is zero past D, and for a negative zlo the bits below z = 0 are shifted in as zeros
__device__ __forceinline__ u32 valid16(const u32* __restrict__ vbits, int nw, i64 x, i64 zlo, i64 D) {
    if (zlo <= -16 || zlo >= D) return 0u;
    const i64 zs = zlo < 0 ? 0 : zlo;
    const u32* vr = vbits + x * nw + (zs >> 5);
    u32 v = (u32)((((u64)vr[1] << 32) | (u64)vr[0]) >> (zs & 31)) & 0xffffu;
    if (zlo < 0) v = (v << (int)(-zlo)) & 0xffffu;
    return v;
}

// an output run with the bytes whose keep bit is clear zeroed (partly kept runs are rare: border cells rejected by the f64 bounds
// test, stream pieces that straddle a plane whose destination mask differs)
__device__ __forceinline__ u32x4 kept_run(const u32 o[4], u32 keep16) {
    u32x4 r = {o[0], o[1], o[2], o[3]};
    if (keep16 != 0xffffu)
#pragma unroll
        for (int w = 0; w < 4; ++w) r[w] &= spread4((keep16 >> (4 * w)) & 0xfu);
    return r;
}

// the 16 source bytes at in + off, byte b being column col + b of a row of D bytes.  A ragged piece (not whole) is still read whole
// while it stays inside the volume's nbytes: the bytes beyond the row belong to the neighbouring row and are dropped by the validity
// bits (their source column is outside [0, D)).  Otherwise it is gathered byte by byte, the bytes outside [0, D) zero.
__device__ __forceinline__ u32x4 load_piece(const u8* in, i64 off, i64 nbytes, bool whole, i64 col, i64 D) {
    if (whole || (off >= 0 && off + 16 <= nbytes)) return __builtin_nontemporal_load((const u32x4_u*)(in + off));
    u32x4 r = (u32x4)(0u);
#pragma unroll
    for (int b = 0; b < 16; ++b)
        if (col + b >= 0 && col + b < D) r[b >> 2] |= (u32)in[off + b] << (8 * (b & 3));
    return r;
}

// the first k (1 .. 15) bytes of r at p, a row end: whole dwords, then bytes
__device__ __forceinline__ void store_head(u8* p, u32x4 r, int k) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (4 * j + 4 <= k) *(u32_u*)(p + 4 * j) = r[j];
#pragma unroll
    for (int b = 0; b < 16; ++b)
        if (b >= (k & ~3) && b < k) p[b] = (u8)(r[b >> 2] >> (8 * (b & 3)));
}

}  // namespace
