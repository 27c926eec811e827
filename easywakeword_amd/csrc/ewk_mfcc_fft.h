// ewk_mfcc_fft.h -- the float32 scorer's frame pass: staging, window, 256-point four-step FFT,
// real-FFT untangle, mel, log and the tile write, kFPP frames per wave pass (one function,
// frame_pass).  Reads the segment's samples from global memory (SegSrc) and the shared tables
// L_WIN2, L_TW1, L_TW2, L_WPAD; reads and writes the wave's scratch (L_SCR: the sample stage,
// the transpose image, the power spectrum); writes kFPP rows of the wave's log-mel tile (W_TILE).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "ewk_internal.h"
#include "ewk_mfcc_layout.h"
#include "ewk_mfcc_dft.h"
#include "ewk_mfcc_tile.h"

// s_setprio 1 over the frame-pass LDS phases (window, transposes, mel): -0.4 %
#define EWK_SETPRIO(v) __builtin_amdgcn_s_setprio(v)

namespace ewk {

// FFT transpose image of one pass (one real or imaginary plane): row k1 of frame set g
// holds the 64 lanes' values (16 f + j) contiguously, as ds_write_addtid_b32 stores them
// (address = M0 + offset + 4 lane).  Rows are placed so that the untangle's row reads
// -- lane (f, h, j') fetches rows j' and 16 - j' (8 for j' = 0) of frame set h with
// ds_read_b128 -- hit 16 distinct bank quads in every lane group: the row of (r, h)
// starts at quad (j'(r) & 3) + 8 h (mod 16), rows sorted by that shift.
__host__ __device__ constexpr int tr_off(int r, int h) {
    const int jp = r < 8 ? r : (r == 8 ? 0 : 16 - r);
    const int q = (jp >> 2) + (r >= 8 ? 2 : 0);
    return 64 * (16 * h + 4 * (jp & 3) + q) + 4 * ((jp & 3) + 8 * h);   // floats
}

// Segment samples through a buffer descriptor: the hardware range check returns 0
// outside [0, len) (negative offsets wrap to huge unsigned ones), which is exactly
// stft(center=True, pad_mode='constant').  Ring segments wrap at the stream ring.
// RING: 0 linear float32 batch, 1 float32 ring, 2 int16 ring (EWK_RING_I16: the sample
// is x * 32768; the 1/32768 rides in the window table, a power-of-two scale, so the
// windowed products are bit-identical to the float32 ring's).
template <int RING>
struct SegSrc {
    __amdgpu_buffer_rsrc_t rsrc;   // linear: the segment; ring: the whole stream ring
    int32_t len;
    int32_t wrap_at;               // ring: q >= wrap_at -> physical q + start - ring
    int32_t start;                 // ring: physical index of sample 0
    int32_t ring;
};

constexpr int sample_bytes(int ring) { return ring == 2 ? 2 : 4; }

template <int RING>
__device__ __forceinline__ SegSrc<RING> make_src(const void* p, int64_t start, int64_t ring, int32_t len) {
    SegSrc<RING> v;
    const unsigned char* b = static_cast<const unsigned char*>(p) + (RING ? 0 : start * sample_bytes(RING));
    const uint64_t bu = (uint64_t)b;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)bu);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(bu >> 32));
    const void* bb = (const void*)(((uint64_t)hi << 32) | lo);
    const int32_t n = __builtin_amdgcn_readfirstlane(RING ? (int32_t)ring : len);
    v.rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)bb, (short)0, n * sample_bytes(RING), 0x00020000);
    v.len = __builtin_amdgcn_readfirstlane(len);
    v.start = __builtin_amdgcn_readfirstlane((int32_t)start);
    v.ring = __builtin_amdgcn_readfirstlane((int32_t)ring);
    v.wrap_at = v.ring - v.start;
    return v;
}

// Coalesced staging loads: lane l fetches samples q0 + 64*c + l, c < kStageLoads.
template <int RING>
__device__ __forceinline__ void stage_load(const SegSrc<RING>& v, int q0, int lane, float (&r)[kStageLoads]) {
#pragma unroll
    for (int c = 0; c < kStageLoads; ++c) {
        const int q = q0 + 64 * c + lane;
        int off;
        if (RING) {
            const int phys = q >= v.wrap_at ? q - v.wrap_at : q + v.start;
            off = (unsigned)q < (unsigned)v.len ? phys * sample_bytes(RING) : -1;
        } else {
            off = q * 4;
        }
        if (RING == 2)   // buffer_load_sshort + v_cvt_f32_i32: the int16 sample, exactly
            r[c] = (float)(short)__builtin_amdgcn_raw_buffer_load_b16(v.rsrc, off, 0, 0);
        else
            r[c] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(v.rsrc, off, 0, 0));
    }
}

// 13 lane-contiguous rows of 64 floats with ds_write_addtid_b32 (M0 = stage base, saved
// and restored; s_nop 0 for the M0 -> LDS hazard): half the LDS cycles of ds_write_b32
#define EWK_ST13(o)                                                                                            \
    asm volatile("s_mov_b32 %[sv], m0\n\ts_mov_b32 m0, %[base]\n\ts_nop 0\n\t"                              \
                 "ds_write_addtid_b32 %[r0] offset:%[o0]\n\tds_write_addtid_b32 %[r1] offset:%[o1]\n\t"          \
                 "ds_write_addtid_b32 %[r2] offset:%[o2]\n\tds_write_addtid_b32 %[r3] offset:%[o3]\n\t"          \
                 "ds_write_addtid_b32 %[r4] offset:%[o4]\n\tds_write_addtid_b32 %[r5] offset:%[o5]\n\t"          \
                 "ds_write_addtid_b32 %[r6] offset:%[o6]\n\tds_write_addtid_b32 %[r7] offset:%[o7]\n\t"          \
                 "ds_write_addtid_b32 %[r8] offset:%[o8]\n\tds_write_addtid_b32 %[r9] offset:%[o9]\n\t"          \
                 "ds_write_addtid_b32 %[r10] offset:%[o10]\n\tds_write_addtid_b32 %[r11] offset:%[o11]\n\t"      \
                 "ds_write_addtid_b32 %[r12] offset:%[o12]\n\ts_mov_b32 m0, %[sv]"                                 \
                 : [sv] "=&s"(m0save)                                                                          \
                 : [base] "s"(m0base), [r0] "v"(r[o]), [r1] "v"(r[o + 1]), [r2] "v"(r[o + 2]), [r3] "v"(r[o + 3]), \
                   [r4] "v"(r[o + 4]), [r5] "v"(r[o + 5]), [r6] "v"(r[o + 6]), [r7] "v"(r[o + 7]),                \
                   [r8] "v"(r[o + 8]), [r9] "v"(r[o + 9]), [r10] "v"(r[o + 10]), [r11] "v"(r[o + 11]),          \
                   [r12] "v"(r[o + 12]), [o0] "i"(stg_off(o)), [o1] "i"(stg_off(o + 1)), [o2] "i"(stg_off(o + 2)), \
                   [o3] "i"(stg_off(o + 3)), [o4] "i"(stg_off(o + 4)), [o5] "i"(stg_off(o + 5)),                    \
                   [o6] "i"(stg_off(o + 6)), [o7] "i"(stg_off(o + 7)), [o8] "i"(stg_off(o + 8)),                    \
                   [o9] "i"(stg_off(o + 9)), [o10] "i"(stg_off(o + 10)), [o11] "i"(stg_off(o + 11)),                \
                   [o12] "i"(stg_off(o + 12))                                                                     \
                 : "memory")
static_assert(kStageLoads == 26, "stage_store writes two blocks of 13 rows");
__device__ __forceinline__ void stage_store(float* stage, int lane, const float (&r)[kStageLoads]) {
    const uint32_t m0base = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)stage);
    uint32_t m0save;
    EWK_ST13(0);
    EWK_ST13(13);
}

constexpr int kMelW[8] = {2, 2, 2, 3, 4, 6, 9, 12};   // per 16-band group (checked on the host)
constexpr int kMelIt0[8] = {0, 2, 4, 6, 9, 13, 19, 28};    // first weight of group i in Tables::wpad
// Each group's weights start on a b64 (widths 2) or b128 boundary of the LDS row so one
// group is fetched with 1-3 wide reads right before it is used.
constexpr int kMelOff[8] = {0, 2, 4, 8, 12, 16, 24, 36};
constexpr int kMelRow = 48;
static_assert(kMelRow <= WP && WP % 4 == 0, "mel weight rows");

// Column writes of one frame set's transpose image (one plane: real or imaginary), with
// ds_write_addtid_b32 (address = M0 + offset + 4 lane).
template <int G>
__device__ __forceinline__ void xpose_write(const float2 (&ag)[16], int half, uint32_t m0base) {
    constexpr int g = G;
    float w[16];
#pragma unroll
    for (int k1 = 0; k1 < 16; ++k1) w[k1] = half ? ag[dperm(k1)].y : ag[dperm(k1)].x;
    // M0 is compiler-reserved: saved and restored in the same statement; the
    // s_nop covers the M0-write -> LDS-use hazard (without it the stores use the old M0)
    uint32_t m0save;
    asm volatile("s_mov_b32 %[sv], m0\n\ts_mov_b32 m0, %[base]\n\ts_nop 0\n\t"
                 "ds_write_addtid_b32 %[w0] offset:%[o0]\n\tds_write_addtid_b32 %[w1] offset:%[o1]\n\t"
                 "ds_write_addtid_b32 %[w2] offset:%[o2]\n\tds_write_addtid_b32 %[w3] offset:%[o3]\n\t"
                 "ds_write_addtid_b32 %[w4] offset:%[o4]\n\tds_write_addtid_b32 %[w5] offset:%[o5]\n\t"
                 "ds_write_addtid_b32 %[w6] offset:%[o6]\n\tds_write_addtid_b32 %[w7] offset:%[o7]\n\t"
                 "ds_write_addtid_b32 %[w8] offset:%[o8]\n\tds_write_addtid_b32 %[w9] offset:%[o9]\n\t"
                 "ds_write_addtid_b32 %[w10] offset:%[o10]\n\tds_write_addtid_b32 %[w11] offset:%[o11]\n\t"
                 "ds_write_addtid_b32 %[w12] offset:%[o12]\n\tds_write_addtid_b32 %[w13] offset:%[o13]\n\t"
                 "ds_write_addtid_b32 %[w14] offset:%[o14]\n\tds_write_addtid_b32 %[w15] offset:%[o15]\n\t"
                 "s_mov_b32 m0, %[sv]"
                 : [sv] "=&s"(m0save)
                 : [base] "s"(m0base), [w0] "v"(w[0]), [w1] "v"(w[1]), [w2] "v"(w[2]), [w3] "v"(w[3]),
                   [w4] "v"(w[4]), [w5] "v"(w[5]), [w6] "v"(w[6]), [w7] "v"(w[7]), [w8] "v"(w[8]),
                   [w9] "v"(w[9]), [w10] "v"(w[10]), [w11] "v"(w[11]), [w12] "v"(w[12]),
                   [w13] "v"(w[13]), [w14] "v"(w[14]), [w15] "v"(w[15]),
                   [o0] "i"(4 * tr_off(0, g)), [o1] "i"(4 * tr_off(1, g)), [o2] "i"(4 * tr_off(2, g)),
                   [o3] "i"(4 * tr_off(3, g)), [o4] "i"(4 * tr_off(4, g)), [o5] "i"(4 * tr_off(5, g)),
                   [o6] "i"(4 * tr_off(6, g)), [o7] "i"(4 * tr_off(7, g)), [o8] "i"(4 * tr_off(8, g)),
                   [o9] "i"(4 * tr_off(9, g)), [o10] "i"(4 * tr_off(10, g)), [o11] "i"(4 * tr_off(11, g)),
                   [o12] "i"(4 * tr_off(12, g)), [o13] "i"(4 * tr_off(13, g)), [o14] "i"(4 * tr_off(14, g)),
                   [o15] "i"(4 * tr_off(15, g))
                 : "memory");
}

// One kFPP-frame pass: frames t0 .. t0 + kFPP - 1, samples already staged in `scr`.
// Writes rows [row0, row0 + kFPP) of the log-mel tile (clamped at clampv) and returns the
// per-lane max/min of the valid (unclamped) log-mel values.  If next_t0 >= 0, the samples
// of the pass starting at frame next_t0 are fetched meanwhile and staged at the end.
// `lo[i]` = first bin of band j + 16 i (per lane, loaded once per kernel).
template <int RING>
__device__ __forceinline__ void frame_pass(const SegSrc<RING>& v, int t0, int T, int row0, int next_t0,
                                           const unsigned char* smem, float* scr, float* tile,
                                           int lane, const int (&lo)[8], float& vmax, float& vmin, float& nanp,
                                           float clampv EWK_PASS_PARAM) {
    EWK_TS(fp0);
    EWK_SETPRIO(1);
    // lane group f = lane>>4 holds frames fr = 4 g + f (g < kNF) of this pass; the
    // kNF frames of a lane are independent instruction streams (ILP for the wave).
    const int f = lane >> 4, j = lane & 15;
    // after the transpose lane (h, j') = (j >> 3, j & 7) owns bin columns rowA = j' and
    // rowB = 16 - j' (8 for j' = 0) of frame 4h + f (scratch scf)
    const int jp = j & 7;
    const int rowA = jp, rowB = jp ? 16 - jp : 8;
    float* scf = scr + scr_frame_off(4 * (j >> 3) + f);
    bool valid[kNF];
    float* sc[kNF];
#pragma unroll
    for (int g = 0; g < kNF; ++g) {
        valid[g] = t0 + 2 * f + g < T;
        sc[g] = scr + scr_frame_off(4 * g + f);
    }

    // ---- window the staged samples: lane j holds z[16*n1 + j] = x[32*n1+2j] + i x[32*n1+2j+1]
    // (single ds_read_b64s: the compiler would pair them into ds_read2_b64, which
    // costs the LDS twice the cycles per byte)
    float2 a[kNF][16];
    floatx4 t4[8];   // twiddle row W256^(j*k1)
    {
        float2 x[kNF][16];
        {
            const uint32_t sa = (uint32_t)(uintptr_t)(scr + 352 * f + 2 * j);
#define EWK_LD64(g, n) asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(x[g][n]) : "v"(sa), "i"(win_off(g, n)) : "memory")
            EWK_LD64(0, 0); EWK_LD64(0, 1); EWK_LD64(0, 2); EWK_LD64(0, 3); EWK_LD64(0, 4); EWK_LD64(0, 5);
            EWK_LD64(0, 6); EWK_LD64(0, 7); EWK_LD64(0, 8); EWK_LD64(0, 9); EWK_LD64(0, 10); EWK_LD64(0, 11);
            EWK_LD64(0, 12); EWK_LD64(0, 13); EWK_LD64(0, 14); EWK_LD64(0, 15);
            EWK_LD64(1, 11); EWK_LD64(1, 12); EWK_LD64(1, 13); EWK_LD64(1, 14); EWK_LD64(1, 15);
#undef EWK_LD64
        }
        floatx4 w4[8];   // this lane's window pairs, fetched in the same batch
        EWK_LD128_8(w4, (uint32_t)(uintptr_t)(reinterpret_cast<const float4*>(smem + L_WIN2) + j * (TP / 2)));
        EWK_WAIT_8(w4);
        asm volatile("s_waitcnt lgkmcnt(0)"
                     : "+v"(x[0][0]), "+v"(x[0][1]), "+v"(x[0][2]), "+v"(x[0][3]), "+v"(x[0][4]), "+v"(x[0][5]),
                       "+v"(x[0][6]), "+v"(x[0][7]), "+v"(x[0][8]), "+v"(x[0][9]), "+v"(x[0][10]), "+v"(x[0][11]),
                       "+v"(x[0][12]), "+v"(x[0][13]), "+v"(x[0][14]), "+v"(x[0][15])
                     :
                     : "memory");
        asm volatile("s_waitcnt lgkmcnt(0)"
                     : "+v"(x[1][11]), "+v"(x[1][12]), "+v"(x[1][13]), "+v"(x[1][14]), "+v"(x[1][15])
                     :
                     : "memory");
#pragma unroll
        for (int n = 0; n <= 10; ++n) x[1][n] = x[0][n + 5];   // the shared sample pairs
        float2 wv[16];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            wv[2 * c] = make_float2(w4[c].x, w4[c].y);
            wv[2 * c + 1] = make_float2(w4[c].z, w4[c].w);
        }
        EWK_SETPRIO(0);
        // ---- DFT16 over n1 (window folded into its first stage), twiddle W256^(j*k1)
        // (one twiddle row serves every frame of the lane, requested before the DFT16s)
        EWK_LD128_8(t4, (uint32_t)(uintptr_t)(reinterpret_cast<const float4*>(smem + L_TW1) + j * (TP / 2)));
#pragma unroll
        for (int g = 0; g < kNF; ++g) {
#pragma unroll
            for (int n = 0; n < 16; ++n) a[g][n] = x[g][n];
            dft16_perm_win(a[g], wv);
        }
    }
    lds_order();
    EWK_TS(fp1);
    // next pass's samples: issued before the mel stage (registers are free there),
    // stored to the staging area at the end of the pass
    float pf[kStageLoads];
    {
        EWK_WAIT_8(t4);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const floatx4 w = t4[c];   // k1 = 2c+1, 2c+2
#pragma unroll
            for (int g = 0; g < kNF; ++g) {
                a[g][dperm(2 * c + 1)] = cmul(a[g][dperm(2 * c + 1)], make_float2(w.x, w.y));
                if (c < 7) a[g][dperm(2 * c + 2)] = cmul(a[g][dperm(2 * c + 2)], make_float2(w.z, w.w));
            }
        }
    }
    EWK_TS(fp2);
    EWK_SETPRIO(1);
    // ---- transpose through LDS (real, then imaginary half): lane k1 <- A_{n2}[k1].
    // Row r (16 floats) keeps column n in 4-float chunk (n>>2) ^ ((r>>2)&3): the
    // column writes (ds_write_b32, the frames of a 32-lane half 272 floats apart) and
    // the row reads (ds_read_b128) are both bank-conflict free.
    float2 b[kNF][16];
    {
        const uint32_t m0base = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)scr);
        const int offA = tr_off(rowA, j >> 3) + 16 * f, offB = tr_off(rowB, j >> 3) + 16 * f;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
#pragma unroll
            for (int g = 0; g < kNF; ++g) {
                if (g == 0) xpose_write<0>(a[0], half, m0base);
                else xpose_write<1>(a[1], half, m0base);
            }
            lds_order();
            // lane (h, j') = (j >> 3, j & 7) reads two columns of frame 4h + f: c0 = j' and its
            // conjugate partner 16 - j' (column 8 beside column 0 for j' = 0)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const float4* rd = reinterpret_cast<const float4*>(scr + (s2 ? offB : offA));
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float4 q = rd[c];
                    if (half) {
                        b[s2][4 * c].y = q.x; b[s2][4 * c + 1].y = q.y; b[s2][4 * c + 2].y = q.z; b[s2][4 * c + 3].y = q.w;
                    } else {
                        b[s2][4 * c].x = q.x; b[s2][4 * c + 1].x = q.y; b[s2][4 * c + 2].x = q.z; b[s2][4 * c + 3].x = q.w;
                    }
                }
            }
            lds_order();
        }
    }
    EWK_TS(fp3);
    EWK_SETPRIO(0);
    // ---- DFT16 over n2: Z[j + 16*k2] = b[dperm(k2)]
#pragma unroll
    for (int g = 0; g < kNF; ++g) dft16_perm(b[g]);
    EWK_TS(fp4);
    // ---- untangle + power, two conjugate bins per step, no cross-lane traffic.  For
    // k = c0 + 16 it the partner Zp = Z[256 - k] sits in this lane's other column; with
    // A = Z[k] + conj(Zp), B = Z[k] - conj(Zp), C = i W512^k B:
    //   P'[k] = |2 X[k]|^2 = |A - C|^2,  P'[256 - k] = |A + C|^2.
    // Lanes j' = 1..7: it = 0..15 (it = 16 repeats it = 15).  Lane j' = 0 pairs column
    // 0 with itself (it = 0..8: k = 16 it, 256 - k; it = 0 yields bin 256) and column 8
    // with itself (it = 9..16: k = 8 + 16 (it - 9)).
    {
        const bool z0 = jp == 0;
        // the 17 twiddles of this lane class, fetched up front (9 ds_read_b128): read one
        // step ahead they cost an LDS round trip per step behind that step's writes
        float2 tw[18];
        {
            const float4* t4 = reinterpret_cast<const float4*>(smem + L_TW2) + jp * (TP / 2);   // [j'][it], 17 entries
#pragma unroll
            for (int c = 0; c < 9; ++c) {
                const float4 q = t4[c];
                tw[2 * c] = make_float2(q.x, q.y);
                tw[2 * c + 1] = make_float2(q.z, q.w);
            }
        }
        float* pA0 = scf + rowA;                     // P[k]      at pA0[16 it]       (it <= 15)
        float* pA1 = z0 ? scf - 136 : pA0;           //           lane 0, it >= 9
        float* pA2 = z0 ? scf - 136 : pA0 - 16;      //           it = 16
        float* pB0 = scf - rowA;                     // P[256-k]  at pB0[256 - 16 it]
        float* pB1 = z0 ? scf + 136 : pB0;
        float* pB2 = z0 ? scf + 136 : pB0 + 16;
        // two steps per iteration, their stores grouped by base (pa, pa, pb, pb) so that
        // the stores of consecutive steps merge into ds_write2_b32
#pragma unroll
        for (int it0 = 0; it0 < 17; it0 += 2) {
            float py[2], px[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int it = it0 + u;
                if (it >= 17) break;
                const float2 w = tw[it];   // (cos, tan)(2 pi k / 512)
                const float2 ug = b[0][dperm(it < 16 ? it : 15)];
                const float2 vg = b[1][dperm(it < 16 ? 15 - it : 0)];
                float2 uu, vv;
                if (it <= 8) {
                    uu = ug;
                    const float2 vz = b[0][dperm((16 - it) & 15)];
                    vv = z0 ? vz : vg;
                } else {
                    const float2 uz = b[1][dperm(it - 9)], vz = b[1][dperm(24 - it)];
                    uu = z0 ? uz : ug;
                    vv = z0 ? vz : vg;
                }
                const float ar = uu.x + vv.x, ai = uu.y - vv.y;
                const float br = uu.x - vv.x, bi = uu.y + vv.y;
                // w = (c, t = s / c): C = c (t br - bi, t bi + br), its scale in the output FMAs
                const float er = fmaf(w.y, br, -bi), ei = fmaf(w.y, bi, br);
                const float yr = fmaf(-w.x, er, ar), yi = fmaf(-w.x, ei, ai);
                const float xr = fmaf(w.x, er, ar), xi = fmaf(w.x, ei, ai);
                py[u] = yr * yr + yi * yi;
                px[u] = xr * xr + xi * xi;
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int it = it0 + u;
                if (it >= 17) break;
                float* pa = it <= 8 ? pA0 : (it < 16 ? pA1 : pA2);
                pa[16 * it] = py[u];
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int it = it0 + u;
                if (it >= 17) break;
                float* pb = it <= 8 ? pB0 : (it < 16 ? pB1 : pB2);
                pb[256 - 16 * it] = px[u];
            }
        }
        // the zero pad (bins 257..271) the unrolled band loops read past bin 256
        scf[257 + jp] = 0.0f;
        if (jp < 7) scf[265 + jp] = 0.0f;
    }
    lds_order();
    EWK_TS(fp5);
    EWK_SETPRIO(1);
    if (next_t0 >= 0) stage_load(v, next_t0 * HOP - NFFT / 2, lane, pf);
    // ---- mel + log: lane j computes bands m = j + 16*i of its frames (weights shared).
    // The stage's LDS reads go in two batches (band groups 0-5, then 6-7: 19 and 21
    // weights), each followed by its FMAs -- one wait per batch, not one per group.
    float db[kNF][8];
    {
        const float* wrow = reinterpret_cast<const float*>(smem + L_WPAD) + j * WP;
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            const int i0 = hh ? 6 : 0, i1 = hh ? 8 : 6;
            float wv[MEL_ITERS], pv[kNF][MEL_ITERS];
#pragma unroll
            for (int i = i0; i < i1; ++i) {
                if (kMelW[i] <= 2) {
                    const float2 w = *reinterpret_cast<const float2*>(wrow + kMelOff[i]);
                    wv[kMelIt0[i]] = w.x; wv[kMelIt0[i] + 1] = w.y;
                } else {
#pragma unroll
                    for (int c = 0; c < (kMelW[i] + 3) / 4; ++c) {
                        const float4 w = *reinterpret_cast<const float4*>(wrow + kMelOff[i] + 4 * c);
                        const float ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (4 * c + e < kMelW[i]) wv[kMelIt0[i] + 4 * c + e] = ww[e];
                    }
                }
#pragma unroll
                for (int g = 0; g < kNF; ++g) {
                    const float* sp = sc[g] + lo[i];
#pragma unroll
                    for (int q = 0; q < kMelW[i]; ++q) pv[g][kMelIt0[i] + q] = sp[q];
                }
            }
#pragma unroll
            for (int i = i0; i < i1; ++i)
#pragma unroll
                for (int g = 0; g < kNF; ++g) {
                    float acc = 0.0f;
#pragma unroll
                    for (int q = 0; q < kMelW[i]; ++q) acc = fmaf(wv[kMelIt0[i] + q], pv[g][kMelIt0[i] + q], acc);
                    // 10*log10(x) = (10*log10(2)) * log2(x), v_log_f32
                    db[g][i] = 3.0102999566398120f * __log2f(fmaxf(1e-10f, acc));
                    // NaN probe: a NaN sample makes every bin of its frame NaN, which the
                    // amin floor above would hide (fmax returns the number); the reference's
                    // np.maximum propagates it and scores NaN (acc * 0 is NaN for NaN / Inf)
                    if (i == 0) nanp = fmaf(acc, 0.0f, nanp);
                }
        }
    }
    EWK_SETPRIO(0);
    lds_order();
    EWK_TS(fp6);
    // Rows of frames past T keep their (finite: silence gives -100 dB) values: the DCT
    // columns are independent and the statistics skip those frames, so only the frame's
    // max/min needs the validity test, once per frame.  The eight bands of a lane form
    // k-chunk j of its frame row (hi and lo halves, one ds_write_b128 each).
#pragma unroll
    for (int g = 0; g < kNF; ++g) {
        const int r = row0 + 2 * f + g;
        float fmx = db[g][0], fmn = db[g][0], x[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            fmx = fmaxf(fmx, db[g][i]);
            fmn = fminf(fmn, db[g][i]);
            x[i] = fmaxf(db[g][i], clampv);   // top_db recompute path; -inf folds away otherwise
        }
        vmax = fmaxf(vmax, valid[g] ? fmx : -INFINITY);
        vmin = fminf(vmin, valid[g] ? fmn : INFINITY);
        uint4 hi, lo;
        split8(x, hi, lo);
        unsigned char* tb = reinterpret_cast<unsigned char*>(tile) + tile_chunk(r, j);
        *reinterpret_cast<uint4*>(tb) = hi;
        *reinterpret_cast<uint4*>(tb + 256) = lo;
    }
    lds_order();
    if (next_t0 >= 0) stage_store(scr, lane, pf);
    lds_order();
#ifdef EWK_TIMING
    EWK_TS(fp7);
    if (pdbg) {
        pdbg[12] += fp1 - fp0; pdbg[13] += fp2 - fp1; pdbg[14] += fp3 - fp2; pdbg[15] += fp4 - fp3;
        pdbg[16] += fp5 - fp4; pdbg[17] += fp6 - fp5; pdbg[18] += fp7 - fp6; pdbg[19] += 1;
    }
#endif
}

}  // namespace ewk
