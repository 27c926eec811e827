// ewk_mfcc_tile.h -- the float32 scorer's log-mel tile format (a wave's W_TILE region: 16 frame
// rows x 512 B of f16 hi/lo chunks): the hi/lo split the frame pass (ewk_mfcc_fft.h) writes it
// with, the chunk addressing, and the in-place top_db clamp of a stored tile.  The DCT stage
// (ewk_mfcc_dct.h) reads the same image.
#pragma once
#include <hip/hip_runtime.h>

namespace ewk {

// f16 hi/lo split of a float32: hi = x truncated to f16's 11 significant bits (exact in
// f16 over the dB range), lo = x - hi exactly, stored to f16 with round-to-nearest, so
// float(hi) + float(lo) = x within 2^-22 |x|.
__device__ __forceinline__ float f16_trunc(float x) { return __uint_as_float(__float_as_uint(x) & 0xFFFFE000u); }
typedef _Float16 halfx2 __attribute__((ext_vector_type(2)));
typedef _Float16 halfx8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ uint32_t pk_f16(float a, float b) {   // v_cvt_pk_f16_f32
    halfx2 h;
    h.x = (_Float16)a;
    h.y = (_Float16)b;
    return __builtin_bit_cast(uint32_t, h);
}
__device__ __forceinline__ float f16_lo(uint32_t p) { return (float)__builtin_bit_cast(halfx2, p).x; }
__device__ __forceinline__ float f16_hi(uint32_t p) { return (float)__builtin_bit_cast(halfx2, p).y; }
// eight log-mel values -> their hi chunk and lo chunk (16 B each)
// hi pair = v_cvt_pkrtz_f16_f32 (round toward zero = the 11-bit truncation over the dB
// range), lo = f16(x - float(hi)) by v_fma_mixlo/mixhi_f16 (the subtraction in f32, exact;
// one rounding to f16): 3 VALU per pair instead of 6.
__device__ __forceinline__ void split2(float a, float b, uint32_t& h, uint32_t& l) {
    h = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(a, b));
    uint32_t r;
    asm("v_fma_mixlo_f16 %0, %1, 1.0, -%2 op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %0, %3, 1.0, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
        : "=&v"(r) : "v"(a), "v"(h), "v"(b));
    l = r;
}
__device__ __forceinline__ void split8(const float (&x)[8], uint4& hi, uint4& lo) {
    split2(x[0], x[1], hi.x, lo.x);
    split2(x[2], x[3], hi.y, lo.y);
    split2(x[4], x[5], hi.z, lo.z);
    split2(x[6], x[7], hi.w, lo.w);
}
// Byte offset of k-chunk c of frame row r in the log-mel tile: the row's hi chunks fill its
// first 256 B and the lo chunks the next 256 B, chunk c at slot c ^ r, so the 16 rows of a
// DCT operand read (one chunk per row) and the 16 chunks of a row write both cover all
// 64 banks.
__device__ __forceinline__ int tile_chunk(int r, int c) { return 512 * r + 16 * (c ^ r); }

// top_db clamp of a log-mel tile (its flat 8 KB LDS image): lane l takes the chunk pairs
// p = l + 64 u (frame row p >> 4, slot p & 15), rebuilds each value exactly as
// float(hi) + float(lo), clamps it at theta and writes the re-split pair back in place.
__device__ __forceinline__ void clamp_load(const float4* src, int lane, uint4 (&h)[4], uint4 (&l)[4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int p = lane + 64 * u;
        h[u] = __builtin_bit_cast(uint4, src[32 * (p >> 4) + (p & 15)]);
        l[u] = __builtin_bit_cast(uint4, src[32 * (p >> 4) + 16 + (p & 15)]);
    }
}
__device__ __forceinline__ void clamp_store(float* tile, int lane, const uint4 (&h)[4], const uint4 (&l)[4],
                                            float theta) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const uint32_t hw[4] = {h[u].x, h[u].y, h[u].z, h[u].w}, lw[4] = {l[u].x, l[u].y, l[u].z, l[u].w};
        float x[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            x[2 * k] = fmaxf(f16_lo(hw[k]) + f16_lo(lw[k]), theta);
            x[2 * k + 1] = fmaxf(f16_hi(hw[k]) + f16_hi(lw[k]), theta);
        }
        uint4 hh, ll;
        split8(x, hh, ll);
        const int p = lane + 64 * u;
        uint4* dst = reinterpret_cast<uint4*>(tile) + 32 * (p >> 4) + (p & 15);
        dst[0] = hh;
        dst[16] = ll;
    }
}

}  // namespace ewk
