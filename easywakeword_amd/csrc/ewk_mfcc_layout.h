// ewk_mfcc_layout.h -- the float32 scorer's (k_score_f32, ewk_mfcc.hip) LDS carve and its debug
// timing macros.  No stage of its own: the byte offsets of every region -- per-wave FFT scratch /
// sample staging (L_SCR), the shared tables the kernel fills (L_WIN2 .. L_DCT), each wave's
// log-mel tile and top_db record (W_TILE, W_SPEC), the ring mode's workgroup words (L_WG) -- that
// the stage headers read and write, and lds_order between their LDS phases.
#pragma once
#include <hip/hip_runtime.h>

#include "ewk_internal.h"

// Per-wave phase timing of the linear-batch scorer (debug builds with -DEWK_TIMING only:
// scripts/mb_score.py prints it; the product build compiles none of it).  dbg[k] sums the
// s_memtime cycles of phase k over the wave's segments; the kernel adds them to g_ewk_dbg.
#ifdef EWK_TIMING
#define EWK_DBG_PARAM , uint64_t(&dbg)[kDbgN]
#define EWK_DBG_ARG , dbg
#define EWK_TS(v) const uint64_t v = __builtin_amdgcn_s_memtime()
#define EWK_TADD(k, a, b) dbg[k] += (b) - (a)
// frame-pass sub-phases (dbg[12..18]) and passes timed (dbg[19]); tile_passes passes nullptr
#define EWK_PASS_PARAM , uint64_t* pdbg
#define EWK_PASS_ARG(x) , x
#else
#define EWK_DBG_PARAM
#define EWK_DBG_ARG
#define EWK_TS(v)
#define EWK_TADD(k, a, b)
#define EWK_PASS_PARAM
#define EWK_PASS_ARG(x)
#endif
#ifdef EWK_TIMING
constexpr int kDbgN = 27;   // [20] masked tiles, [21] cycles of their DCT + mask DCT + sums, [22] [23] cycles and count of the plain tile DCTs,
                            // [24] tiles with clamped entries left without a mask (mask_wanted), [25] [26] those recomputed later: tiles, passes
#endif

namespace ewk {

#ifdef EWK_TIMING
__device__ unsigned long long g_ewk_dbg[kDbgN];
#endif

typedef float floatx4 __attribute__((ext_vector_type(4)));

// LDS carve (bytes, every offset a multiple of 16).  The per-lane table rows are
// transposed to [lane j][index] with a 144-B (36-dword) row pitch so one
// ds_read_b128 fetches 2 float2 entries and a 16-lane group spans all 64 banks.
// Frames per wave pass: kNF per 16-lane group (kNF = 2: two independent FFTs per lane).
constexpr int kFPP = 4 * kNF;
constexpr int kStageLoads = ((kFPP - 1) * HOP + NFFT + 63) / 64;   // dword loads per lane per pass
// frame fr's FFT scratch starts at scr_frame_off(fr) (ewk_internal.h)
constexpr int kScrFrames = kFPP * SCR_FRAME + 8 * (kNF - 1);
// kNF = 2: a lane's two frames are consecutive (slot (g, f) = frame 2f + g of the pass),
// so the second frame's first 11 sample pairs are the first frame's pairs 5..15 (hop 160 =
// 5 x 32) and only 5 more are read.  The stage is skewed -- sample s at s + 32 floor(s / 320)
// -- so the four lane groups' frames (320 samples apart) land 32 banks apart.
__host__ __device__ constexpr int stg_off(int c) { return 256 * c + 128 * (c / 5); }   // bytes of stage row c
__host__ __device__ constexpr int win_off(int g, int n1) {   // bytes: pair n1 of slot g from the lane's base
    return 4 * (160 * g + 32 * n1 + 32 * ((160 * g + 32 * n1) / 320));
}
constexpr int kStageFloats = stg_off(kStageLoads) / 4;
constexpr int kScrFloats = (kScrFrames > kStageFloats) ? kScrFrames : kStageFloats;
// The per-wave FFT scratch (also the sample staging) comes first in LDS: the M0 base of
// ds_write_addtid_b32 is 16 bits wide, so every wave's scratch must start below 64 KB.
constexpr int SCR_BYTES = (kScrFloats * 4 + 15) & ~15;
constexpr int L_SCR = 0;                                  // [wave] kFPP frames x 272 floats
constexpr int L_TAB = L_SCR + WAVES * SCR_BYTES;
static_assert(L_SCR + (WAVES - 1) * SCR_BYTES < 65536, "ds_write_addtid_b32 bases must fit M0[15:0]");

// LDS carve (bytes, every offset a multiple of 16).  The per-lane table rows are
// transposed to [lane j][index] with a 144-B (36-dword) row pitch so one
// ds_read_b128 fetches 2 float2 entries and a 16-lane group spans all 64 banks.
constexpr int TP = 18;                                    // float2 pitch of a [j][16] table row
constexpr int WP = 52;                                    // float pitch of the [j][48] mel weight row (13 chunks: b128/b64 conflict free)
constexpr int L_WIN2 = L_TAB;                             // [j][n1] = win2[16*n1 + j]
constexpr int L_TW1 = L_WIN2 + 16 * TP * 8;               // [j][k1-1] = tw1[16*k1 + j], k1 = 1..15
constexpr int L_TW2 = L_TW1 + 16 * TP * 8;                // [j][k2] = tw2[j + 16*k2]
constexpr int L_WPAD = L_TW2 + 16 * TP * 8;               // [j][kMelOff[i] + q] = wpad[16*(it0_i + q) + j]
constexpr int L_BLO = L_WPAD + 16 * WP * 4;
constexpr int L_DCT = L_BLO + NMEL * 4;
// DCT operand image for v_mfma_f32_16x16x32_f16: D * 2^10 split into f16 hi + lo (the
// products hi*hi + hi*lo + lo*hi carry ~22 bits).  The tile's k order groups each lane's
// eight bands: k-chunk c (k = 8c .. 8c+7) holds bands c + 16 jj, jj = 0..7, so the
// operand of k-step q for lane l is chunk 4q + (l >> 4).  Row tile 0 (coefficients 0..15):
// [q][hi/lo][lane] 16-B chunks; row tile 1 (coefficient 16 + n in row 4n, so that each lane
// group of the output holds one of them): [q][hi/lo][l >> 4][n] for the lanes with
// (l & 15) = 4n, every other lane reads the block's zero chunk.
constexpr float kDctScale = 1024.0f;
constexpr float kTopDbUnits = 80.0f;   // top_db, in the tile's dB units
constexpr int DCT_RT1 = 4 * 2 * 64 * 16;                  // row tile 1: [q][hi/lo] blocks of 17 chunks
constexpr int DCT_RT1_STRIDE = 17 * 16;                   // 16 data chunks [l >> 4][(l & 15) >> 2] + a zero chunk
// coefficient slots per lane: rows 4h .. 4h + 3 of row tile 0, and row 4h of row tile 1, which
// holds coefficient 16 + h (rows 4h + 1 .. 4h + 3 of that tile are zero and are not kept)
constexpr int kSlots = 5;
constexpr int DCT_BYTES = DCT_RT1 + 8 * DCT_RT1_STRIDE;
constexpr int L_SHARED_END = ((L_DCT + DCT_BYTES) + 15) & ~15;
constexpr int W_TILE = 0;                                 // 16 frame rows x 512 B of f16 hi/lo chunks (tile_chunk)
// per-tile record of the speculative top_db clamp (segment_stats): stored log-mel minima per
// pass (above the clamp, for a tile with clamped entries), the clamps and the processing order
// ((passes per tile + 2) x kSpecTiles ints)
constexpr int kSpecTiles = 48;   // tiles of frames 0..767 (7.7 s) are recorded and scout-ordered
constexpr int W_SPEC = W_TILE + 16 * NMEL * 4;
constexpr int kSpecRun = (16 / kFPP) * kSpecTiles;      // spec[kSpecRun + tile]: the tile's clamp
constexpr int kSpecOrder = kSpecRun + kSpecTiles;        // spec[kSpecOrder + k]: k-th tile processed
constexpr int W_BYTES = W_SPEC + (kSpecOrder + kSpecTiles) * 4;
static_assert(W_BYTES % 16 == 0 && kSpecTiles <= 64, "per-wave LDS carve; one bit per recorded tile");
constexpr int L_WG = L_SHARED_END + WAVES * W_BYTES;    // ring mode: segment index + per-wave log-mel max/min
constexpr int LDS_BYTES = L_WG + 16 + 8 * WAVES;
static_assert(LDS_BYTES <= 160 * 1024, "the workgroup must fit a CU's LDS");
static_assert(16 % kFPP == 0, "passes must tile the 16-frame log-mel tile");


__device__ __forceinline__ void lds_order() { asm volatile("" ::: "memory"); }

}  // namespace ewk
