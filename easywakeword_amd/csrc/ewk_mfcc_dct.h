// ewk_mfcc_dct.h -- the float32 scorer's DCT stage: one 16-frame log-mel tile to its 20 MFCC
// rows on the matrix cores, optionally with the DCT of the tile's top_db clamp mask.  Reads the
// wave's log-mel tile (W_TILE, the format of ewk_mfcc_tile.h) and the shared DCT operand image
// (L_DCT); writes no LDS.
#pragma once
#include <hip/hip_runtime.h>

#include "ewk_mfcc_layout.h"
#include "ewk_mfcc_tile.h"

namespace ewk {

// DCT of one 16-frame log-mel tile on the matrix cores: C[32 x 16] = D[32 x 128] X[128 x 16]
// with v_mfma_f32_16x16x32_f16 on the f16 hi/lo splits, three products per k-step
// (Dh Xh + Dh Xl + Dl Xh, f32 accumulation; the dropped Dl Xl is ~2^-22 relative).
// Lane l gets C[row = 4h + r][frame col] of row tile 0 (h = l>>4, col = l&15) in c[0..3] and
// row 4h of row tile 1 (coefficient 16 + h) in c[4] -- the layout of the f32 16x16x4 MFMA.  The operands of k-step q
// (6 ds_read_b128) are requested one step ahead of its 6 MFMAs.
#define EWK_DCT_RD(dst, addr, off) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "i"(off) : "memory")
#define EWK_DCT_LOAD(p, q)                                                   \
    do {                                                                     \
        EWK_DCT_RD(Bh[p], bq[q], 0);                                         \
        EWK_DCT_RD(Bl[p], bq[q], 256);                                       \
        EWK_DCT_RD(A0h[p], a0, 2048 * (q));                                  \
        EWK_DCT_RD(A0l[p], a0, 2048 * (q) + 1024);                           \
        EWK_DCT_RD(A1h[p], a1, DCT_RT1_STRIDE * (2 * (q)));                  \
        EWK_DCT_RD(A1l[p], a1, DCT_RT1_STRIDE * (2 * (q) + 1));              \
    } while (0)
#define EWK_DCT_WAIT(p, n)                                                                               \
    asm volatile("s_waitcnt lgkmcnt(" #n ")"                                                             \
                 : "+v"(Bh[p]), "+v"(Bl[p]), "+v"(A0h[p]), "+v"(A0l[p]), "+v"(A1h[p]), "+v"(A1l[p]) \
                 :                                                                                       \
                 : "memory")
#define EWK_MF(a, b, acc) \
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(halfx8, a), __builtin_bit_cast(halfx8, b), acc, 0, 0, 0)
#define EWK_DCT_MFMA(p)                                                                        \
    do {                                                                                       \
        EWK_MF(A0h[p], Bh[p], acc0); EWK_MF(A1h[p], Bh[p], acc1);                              \
        EWK_MF(A0h[p], Bl[p], acc0); EWK_MF(A1h[p], Bl[p], acc1);                              \
        EWK_MF(A0l[p], Bh[p], acc0); EWK_MF(A1l[p], Bh[p], acc1);                              \
        if (MASK) {                                                                            \
            const floatx4 mk = clamp_mask(Bh[p], Bl[p], cp, mnab);                             \
            EWK_MF(A0h[p], mk, am0); EWK_MF(A1h[p], mk, am1);                                  \
            EWK_MF(A0l[p], mk, am0); EWK_MF(A1l[p], mk, am1);                                  \
        }                                                                                      \
    } while (0)

// The split pair of a tile's clamp, as its clamped entries hold it (both halves of each word),
// and its value float(hi) + float(lo).
// float(hi) + float(lo) of the low / high entry of a pair word in one v_fma_mix_f32 (both
// conversions exact, one rounding: the value clamp_store rebuilds)
__device__ __forceinline__ float pair_sum_lo(uint32_t h, uint32_t l) {
    float r;
    asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel_hi:[1,0,1]" : "=v"(r) : "v"(h), "v"(l));
    return r;
}
__device__ __forceinline__ float pair_sum_hi(uint32_t h, uint32_t l) {
    float r;
    asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel:[1,0,1] op_sel_hi:[1,0,1]" : "=v"(r) : "v"(h), "v"(l));
    return r;
}
struct ClampPair {
    uint32_t h2, l2;
    float eff;
};
__device__ __forceinline__ ClampPair clamp_pair(float clampv) {
    ClampPair cp;
    split2(clampv, clampv, cp.h2, cp.l2);
    cp.eff = pair_sum_lo(cp.h2, cp.l2);
    return cp;
}
// One B operand (eight entries of a frame row, hi and lo chunks): the f16 0/1 mask of the
// entries that hold the clamp's pair, and the minimum of all the others into mn (an entry with
// another pair counts as unclamped whatever its value: the record can only flag too often).
// Per pair word: t has a zero half where the entry is the clamp's pair; min(t, 1) - 1 turns
// that half into 0xFFFF and any other into 0 (packed u16); the mask word is 0x3C00 (f16 1.0)
// there, and the hi word gets +inf (0x7C00) there so that the clamped entries drop out of the
// minimum without a compare (inf + lo = inf).
__device__ __forceinline__ floatx4 clamp_mask(floatx4 bh, floatx4 bl, const ClampPair& cp, float& mn) {
    const uint4 h = __builtin_bit_cast(uint4, bh), l = __builtin_bit_cast(uint4, bl);
    const uint32_t hw[4] = {h.x, h.y, h.z, h.w}, lw[4] = {l.x, l.y, l.z, l.w};
    const uint32_t ones = 0x00010001u;
    uint32_t mw[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t t = (hw[k] ^ cp.h2) | (lw[k] ^ cp.l2);
        uint32_t u, zm;
        asm("v_pk_min_u16 %0, %1, %2" : "=v"(u) : "v"(t), "s"(ones));
        asm("v_pk_sub_u16 %0, %1, %2" : "=v"(zm) : "v"(u), "s"(ones));
        mw[k] = zm & 0x3C003C00u;
        const uint32_t hm = (zm & 0x7C007C00u) | (hw[k] & ~zm);
        // (v_min3_f32 written out: fminf on the asm results costs a canonicalising v_max each)
        asm("v_min3_f32 %0, %0, %1, %2" : "+v"(mn) : "v"(pair_sum_lo(hm, lw[k])), "v"(pair_sum_hi(hm, lw[k])));
    }
    return __builtin_bit_cast(floatx4, make_uint4(mw[0], mw[1], mw[2], mw[3]));
}

// MASK: the tile holds entries clamped at `cp`; also returns their mask DCT m = (Dh + Dl) . mask
// (the mask is exact in f16: two products per k-step and row tile) and the lane's minimum of
// the unclamped entries of its frame row chunks (mnab, folded into the caller's value).
template <bool MASK>
__device__ __forceinline__ void tile_dct_m(const float* tile, const float* s_dct, int lane, float (&c)[kSlots],
                                           float (&m)[kSlots], float& mnab, const ClampPair& cp) {
    const int col = lane & 15, g4 = lane >> 4;
    floatx4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    floatx4 am0 = {0.f, 0.f, 0.f, 0.f}, am1 = {0.f, 0.f, 0.f, 0.f};
    // B of k-step q: chunk 4q + g4 of frame row col, at slot (4q + g4) ^ col =
    // 4 (q ^ (col >> 2)) + (g4 ^ (col & 3))
    const uint32_t tb = (uint32_t)(uintptr_t)tile + 512 * col + 16 * (g4 ^ (col & 3));
    uint32_t bq[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) bq[q] = tb + 64 * (q ^ (col >> 2));
    const uint32_t db = (uint32_t)(uintptr_t)s_dct;
    const uint32_t a0 = db + 16 * lane;
    const uint32_t a1 = db + DCT_RT1 + 16 * ((col & 3) == 0 ? 4 * g4 + (col >> 2) : 16);
    floatx4 Bh[2], Bl[2], A0h[2], A0l[2], A1h[2], A1l[2];
    EWK_DCT_LOAD(0, 0);
    EWK_DCT_LOAD(1, 1);
    EWK_DCT_WAIT(0, 6);
    EWK_DCT_MFMA(0);
    EWK_DCT_LOAD(0, 2);
    EWK_DCT_WAIT(1, 6);
    EWK_DCT_MFMA(1);
    EWK_DCT_LOAD(1, 3);
    EWK_DCT_WAIT(0, 6);
    EWK_DCT_MFMA(0);
    EWK_DCT_WAIT(1, 0);
    EWK_DCT_MFMA(1);
    lds_order();
#pragma unroll
    for (int i = 0; i < 4; ++i) c[i] = acc0[i] * (1.0f / kDctScale);
    c[4] = acc1[0] * (1.0f / kDctScale);
    if (MASK) {
#pragma unroll
        for (int i = 0; i < 4; ++i) m[i] = am0[i] * (1.0f / kDctScale);
        m[4] = am1[0] * (1.0f / kDctScale);
    }
}
__device__ __forceinline__ void tile_dct(const float* tile, const float* s_dct, int lane, float (&c)[kSlots]) {
    float m[kSlots], mnab = 0.0f;
    tile_dct_m<false>(tile, s_dct, lane, c, m, mnab, ClampPair{0u, 0u, 0.0f});
}
#undef EWK_DCT_RD
#undef EWK_DCT_LOAD
#undef EWK_DCT_WAIT
#undef EWK_DCT_MFMA
#undef EWK_MF

}  // namespace ewk
