// ewk_mfcc_dft.h -- register kernels of the float32 scorer's FFT stage (ewk_mfcc_fft.h): the
// radix-4x4 DFT16 with tan-factored W16 twiddles, with and without the window folded in, and
// the batched ds_read_b128 macros that fetch the stage's table rows.  The DFTs touch no LDS;
// the macros read whatever address the caller passes (L_WIN2, L_TW1).
#pragma once
#include <hip/hip_runtime.h>

namespace ewk {

// Eight ds_read_b128 of consecutive 16-B chunks issued together, and their wait.
// Written as asm so the scheduler cannot sink each read next to its first use (at
// 256 VGPRs it does, and every read then costs a full LDS round trip).
#define EWK_LD128(r, a, c) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r[c]) : "v"(a), "i"(16 * (c)) : "memory")
#define EWK_LD128_8(r, addr)                                                                        \
    do {                                                                                           \
        const uint32_t _a = (addr);                                                                \
        EWK_LD128(r, _a, 0); EWK_LD128(r, _a, 1); EWK_LD128(r, _a, 2); EWK_LD128(r, _a, 3);         \
        EWK_LD128(r, _a, 4); EWK_LD128(r, _a, 5); EWK_LD128(r, _a, 6); EWK_LD128(r, _a, 7);         \
    } while (0)
#define EWK_WAIT_8(r)                                                                              \
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), \
                 "+v"(r[5]), "+v"(r[6]), "+v"(r[7]) : : "memory")

__device__ __forceinline__ float2 cmul(float2 a, float2 w) {
    return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x);
}

__device__ __forceinline__ void dft4(float2& a0, float2& a1, float2& a2, float2& a3) {
    const float2 t0 = make_float2(a0.x + a2.x, a0.y + a2.y);
    const float2 t1 = make_float2(a0.x - a2.x, a0.y - a2.y);
    const float2 t2 = make_float2(a1.x + a3.x, a1.y + a3.y);
    const float2 t3 = make_float2(a1.x - a3.x, a1.y - a3.y);
    a0 = make_float2(t0.x + t2.x, t0.y + t2.y);
    a2 = make_float2(t0.x - t2.x, t0.y - t2.y);
    a1 = make_float2(t1.x + t3.y, t1.y - t3.x);   // t1 - i t3
    a3 = make_float2(t1.x - t3.y, t1.y + t3.x);   // t1 + i t3
}

// Second radix-4 stage of the DFT16 with its W16 twiddles folded into FMAs.  Each
// twiddle is written as a real scale times a (1, tan) factor -- W^1 = C1 (1 - iT),
// W^3 = C1 (T - i), W^9 = C1 (-1 + iT), W^2 = R2 (1 - i), W^6 = R2 (-1 - i), T = tan(pi/8)
// -- the two twiddled inputs of a butterfly pair share the scale, and the scale rides
// in the FMAs of the butterfly outputs: 22 / 20 / 22 instructions for rows k1 = 1 / 2 / 3
// instead of 28 / 24 / 28 (three complex multiplies + a radix-4 butterfly).
__device__ __forceinline__ void dft16_stage2(float2 (&x)[16]) {
    constexpr float C1 = 0.92387953251128674f, R2 = 0.70710678118654752f, T = 0.41421356237309505f;
    dft4(x[0], x[1], x[2], x[3]);
    {   // k1 = 1: twiddles W^1, W^2, W^3
        const float2 a0 = x[4], y1 = x[5], y2 = x[6], y3 = x[7];
        const float2 u2 = make_float2(y2.x + y2.y, y2.y - y2.x);                        // Y2 (1 - i)
        const float2 t0 = make_float2(fmaf(R2, u2.x, a0.x), fmaf(R2, u2.y, a0.y));
        const float2 t1 = make_float2(fmaf(-R2, u2.x, a0.x), fmaf(-R2, u2.y, a0.y));
        const float2 u1 = make_float2(fmaf(T, y1.y, y1.x), fmaf(-T, y1.x, y1.y));       // Y1 (1 - iT)
        const float2 u3 = make_float2(fmaf(T, y3.x, y3.y), fmaf(T, y3.y, -y3.x));       // Y3 (T - i)
        const float2 v2 = make_float2(u1.x + u3.x, u1.y + u3.y), v3 = make_float2(u1.x - u3.x, u1.y - u3.y);
        x[4] = make_float2(fmaf(C1, v2.x, t0.x), fmaf(C1, v2.y, t0.y));
        x[6] = make_float2(fmaf(-C1, v2.x, t0.x), fmaf(-C1, v2.y, t0.y));
        x[5] = make_float2(fmaf(C1, v3.y, t1.x), fmaf(-C1, v3.x, t1.y));                // t1 - i C1 v3
        x[7] = make_float2(fmaf(-C1, v3.y, t1.x), fmaf(C1, v3.x, t1.y));                // t1 + i C1 v3
    }
    {   // k1 = 2: twiddles W^2, W^4 = -i, W^6
        const float2 a0 = x[8], y1 = x[9], y2 = x[10], y3 = x[11];
        const float2 t0 = make_float2(a0.x + y2.y, a0.y - y2.x);                        // a0 + (-i Y2)
        const float2 t1 = make_float2(a0.x - y2.y, a0.y + y2.x);
        const float2 u1 = make_float2(y1.x + y1.y, y1.y - y1.x);                        // Y1 (1 - i)
        const float d3 = y3.y - y3.x, n3 = y3.x + y3.y;                                 // Y3 (-1 - i) = (d3, -n3)
        const float2 v2 = make_float2(u1.x + d3, u1.y - n3), v3 = make_float2(u1.x - d3, u1.y + n3);
        x[8] = make_float2(fmaf(R2, v2.x, t0.x), fmaf(R2, v2.y, t0.y));
        x[10] = make_float2(fmaf(-R2, v2.x, t0.x), fmaf(-R2, v2.y, t0.y));
        x[9] = make_float2(fmaf(R2, v3.y, t1.x), fmaf(-R2, v3.x, t1.y));
        x[11] = make_float2(fmaf(-R2, v3.y, t1.x), fmaf(R2, v3.x, t1.y));
    }
    {   // k1 = 3: twiddles W^3, W^6, W^9
        const float2 a0 = x[12], y1 = x[13], y2 = x[14], y3 = x[15];
        const float d2 = y2.y - y2.x, n2 = y2.x + y2.y;                                 // Y2 (-1 - i) = (d2, -n2)
        const float2 t0 = make_float2(fmaf(R2, d2, a0.x), fmaf(-R2, n2, a0.y));
        const float2 t1 = make_float2(fmaf(-R2, d2, a0.x), fmaf(R2, n2, a0.y));
        const float2 u1 = make_float2(fmaf(T, y1.x, y1.y), fmaf(T, y1.y, -y1.x));       // Y1 (T - i)
        const float m3 = fmaf(T, y3.y, y3.x), u3y = fmaf(T, y3.x, -y3.y);               // Y3 (-1 + iT) = (-m3, u3y)
        const float2 v2 = make_float2(u1.x - m3, u1.y + u3y), v3 = make_float2(u1.x + m3, u1.y - u3y);
        x[12] = make_float2(fmaf(C1, v2.x, t0.x), fmaf(C1, v2.y, t0.y));
        x[14] = make_float2(fmaf(-C1, v2.x, t0.x), fmaf(-C1, v2.y, t0.y));
        x[13] = make_float2(fmaf(C1, v3.y, t1.x), fmaf(-C1, v3.x, t1.y));
        x[15] = make_float2(fmaf(-C1, v3.y, t1.x), fmaf(C1, v3.x, t1.y));
    }
}

// In-place radix-4x4 DFT16.  On return x[4*k1 + k2] holds X[k1 + 4*k2].
__device__ __forceinline__ void dft16_perm(float2 (&x)[16]) {
#pragma unroll
    for (int n2 = 0; n2 < 4; ++n2) dft4(x[n2], x[4 + n2], x[8 + n2], x[12 + n2]);
    dft16_stage2(x);
}

// dft16_perm of the windowed input (x[n].x w[n].x, x[n].y w[n].y): the window products
// ride in the first stage's FMAs (t0 = fma(x0, w0, x2 w2), t1 = fma(x0, w0, -x2 w2)).
__device__ __forceinline__ void dft16_perm_win(float2 (&x)[16], const float2 (&w)[16]) {
#pragma unroll
    for (int n2 = 0; n2 < 4; ++n2) {
        const float2 x0 = x[n2], x1 = x[4 + n2], x2 = x[8 + n2], x3 = x[12 + n2];
        const float2 w0 = w[n2], w1 = w[4 + n2], w2 = w[8 + n2], w3 = w[12 + n2];
        const float2 p2 = make_float2(x2.x * w2.x, x2.y * w2.y), p3 = make_float2(x3.x * w3.x, x3.y * w3.y);
        const float2 t0 = make_float2(fmaf(x0.x, w0.x, p2.x), fmaf(x0.y, w0.y, p2.y));
        const float2 t1 = make_float2(fmaf(x0.x, w0.x, -p2.x), fmaf(x0.y, w0.y, -p2.y));
        const float2 t2 = make_float2(fmaf(x1.x, w1.x, p3.x), fmaf(x1.y, w1.y, p3.y));
        const float2 t3 = make_float2(fmaf(x1.x, w1.x, -p3.x), fmaf(x1.y, w1.y, -p3.y));
        x[n2] = make_float2(t0.x + t2.x, t0.y + t2.y);
        x[8 + n2] = make_float2(t0.x - t2.x, t0.y - t2.y);
        x[4 + n2] = make_float2(t1.x + t3.y, t1.y - t3.x);   // t1 - i t3
        x[12 + n2] = make_float2(t1.x - t3.y, t1.y + t3.x);  // t1 + i t3
    }
    dft16_stage2(x);
}

// Natural-order accessor of dft16_perm's output: X[k] lives in slot perm(k).
__device__ __forceinline__ constexpr int dperm(int k) { return 4 * (k & 3) + (k >> 2); }

}  // namespace ewk
