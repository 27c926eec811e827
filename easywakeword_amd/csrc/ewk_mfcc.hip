// ewk_mfcc.hip -- level-2 matcher: fused MFCC + cosine scorer for ragged segment
// batches on gfx950 (CDNA4).
//
// Replaces WordMatcher.extract_mfcc / calculate_similarity / matches
// (reference easywakeword/wakeword.py:544-639), i.e. librosa 0.11.0
// feature.mfcc(n_mfcc=20, n_fft=512, hop=160) + scipy cosine + the score
// scaling, for many segments per launch.
//
// Design.  Linear batches: one wave = one segment; a persistent grid (one 8-wave
// workgroup per CU sharing the LDS tables) pulls segments from an atomic work counter in
// longest-first order.  Ring events of a streaming tick: one segment per workgroup (its
// tiles spread over the 8 waves) for a few hundred events, one per wave for many.
//   frames  : stft(center=True, pad_mode=constant): frame t covers samples
//             [t*160-256, t*160+256) of the segment, zero outside; T = 1+L//160.
//             Samples come through a buffer descriptor whose range check returns 0
//             outside the segment (the padding); ring segments wrap at the stream ring.
//   staging : a wave pass is 8 frames spanning 1,632 contiguous samples, loaded one
//             pass ahead with coalesced dword loads and stored to LDS with
//             ds_write_addtid_b32.
//   FFT     : 16 lanes per frame, two frames per 16-lane group (8 frames per pass: two
//             independent instruction streams per lane).  The 512-point real frame is
//             packed as 256 complex points z[n] = x[2n] + i x[2n+1]; 256 = 16 x 16
//             four-step FFT: a register DFT16 (window folded into its first stage,
//             tan-factored W16 twiddles), a twiddle, an LDS transpose, a second DFT16,
//             then the real-FFT untangle with each bin and its conjugate partner in the
//             same lane (no cross-lane traffic).
//   mel     : Slaney bands from LDS, fully unrolled with compile-time group widths
//             (band m = j + 16 i; widths {2,2,2,3,4,6,9,12}, weights zero-padded), then
//             10*log10(max(1e-10, .)) via v_log_f32; written to a 16-frame log-mel tile
//             as f16 hi/lo pairs (hi = x truncated to 11 bits, lo = x - hi).
//   DCT     : the only dense GEMM on the path: C[32 x 16] = D[32 x 128] . X[128 x 16]
//             per 16-frame tile on the matrix cores, v_mfma_f32_16x16x32_f16 on the hi/lo
//             splits (Dh Xh + Dh Xl + Dl Xh, f32 accumulation), rows 20..31 zero.
//   top_db  : power_to_db clamps at (segment max - 80 dB), a segment-global coupling.
//             Pass 1 clamps each tile speculatively at the running max - 80 dB (exact
//             once the max is known).  When the clamp rises later, a stored tile's clamped
//             entries only have to move up with it: the DCT is linear, so the tile's mask
//             DCT m = D . [entry clamped] shifts its columns by (rise) m inside the shifted
//             sums (ewk_topdb_shift.h), no recompute.  Only a tile holding an unclamped
//             value below the final max - 80 dB (its recorded minimum above the clamp) is
//             recomputed in pass 2 and its contribution swapped in the statistics
//             (nothing is written to global memory but the results).
//   stats   : population mean/std over frames from fp64 shifted sums
//             (d = c - c[frame 0]) -- exact 0 std for identical frames.
//   score   : the reference's own float32 / float64 cosine arithmetic
//             (wakeword.py:611-625 + scipy correlation); NaN kept.  Near-threshold
//             scores are re-scored by k_score_f64 (fp64 path, below).
//
// Source map.  This file: the score finishes and epilogue, the kernel (table fill, work loops),
// the launchers, and the small kernels beside it (k_snapshot, k_bank_mirror, LPT order).  The
// stages, in the order the kernel runs them:
//   ewk_mfcc_layout.h  the LDS carve and the EWK_TIMING macros
//   ewk_mfcc_dft.h     register DFT16s of the FFT
//   ewk_mfcc_tile.h    the log-mel tile's f16 hi/lo format and its top_db clamp
//   ewk_mfcc_fft.h     staging and frame_pass (window, FFT, untangle, mel, log, tile write)
//   ewk_mfcc_dct.h     tile DCT and mask DCT on the matrix cores
//   ewk_mfcc_stats.h   segment_stats / segment_stats_coop, top_db fix-ups, scout, work claiming
//   ewk_rescore.h      the fp64 re-score (included below, after the score finishes)
#include <hip/hip_runtime.h>
#include <math.h>

#include "ewk_internal.h"
#include "ewk_score.h"  // the score arithmetic and listing constants shared with ewk_bank.hip
#include "ewk_db64.h"  // (the fp64 re-score's 10 log10, ewk_rescore.h)
#include "ewk_topdb_shift.h"
#include "ewk_rs_list.h"  // (listing for the fp64 re-score, shared with ewk_bank.hip)
#include "ewk_mfcc_layout.h"
#include "ewk_mfcc_dft.h"
#include "ewk_mfcc_tile.h"
#include "ewk_mfcc_fft.h"
#include "ewk_mfcc_dct.h"
#include "ewk_mfcc_stats.h"

namespace ewk {

// (kRescoreFrames and kTinyStd: ewk_score.h)
// |mean vector| below which the fp64 path decides (round 5: 32, was 64).  Evidence for 32: the
// float32 score error of streaming events is <= 1.2e-5 above |mean| 32 (profiles/r05_v26_mean_err.txt)
// and 600 segments of four other loud recipes with oracle |mean| in [32, 64) score within 8.6e-6
// (round 6, profiles/r06_v1_mean_band_evidence.json); DESIGN.md numerics.
// easywakeword_amd/_lib.py RESCORE_TINY_MEAN mirrors it.
#ifndef EWK_TINY_MEAN
#define EWK_TINY_MEAN 32.0
#endif
constexpr double kTinyMean = EWK_TINY_MEAN;
                                    // (loud audio, c0 cancelling: DESIGN.md numerics)
// A vanishing-mean segment whose float32 similarity percent p = 100 (0.7 sm + 0.3 ss) is below
// -(kNanMarginA / |mean| + kNanMarginB) scores NaN in the reference too (p ** 1.5 of a negative
// p, wakeword.py:621-625): the float32 pass's error in p is far smaller than that (round 6,
// scripts/nan_margin.py: DESIGN.md numerics), so the fp64 re-score cannot change its score or
// decision and the segment is not listed for it.  (Mirrored by _lib.NAN_MARGIN_A / _B.)
#ifndef EWK_NAN_MARGIN_A
#define EWK_NAN_MARGIN_A 0.5
#endif
constexpr double kNanMarginA = EWK_NAN_MARGIN_A;
constexpr double kNanMarginB = 0.05;

// Fast-path finishes (the fp64 re-score keeps the reference's exact pow / sequential dots).
__device__ __forceinline__ double score_f64_finish(double uu_m, double uu_s, double uv_m, double vv_m, double uv_s,
                                                   double vv_s, double& percent) {
#pragma clang fp contract(off)
    const double sm = 1.0 - clip02(1.0 - uv_m / sqrt(uu_m * vv_m));
    const double ss = 1.0 - clip02(1.0 - uv_s / sqrt(uu_s * vv_s));
    percent = (sm * 0.7 + ss * 0.3) * 100.0;
    return percent * sqrt(percent) / 10.0;   // p**1.5 (NaN for p < 0 like pow)
}

__device__ __forceinline__ double score_f32_finish(float uu_m, float uu_s, float uv_m, float vv_m, float uv_s,
                                                   float vv_s) {
#pragma clang fp contract(off)
    const float dm = clip02f(1.0f - uv_m / (float)sqrt((double)(uu_m * vv_m)));
    const float ds = clip02f(1.0f - uv_s / (float)sqrt((double)(uu_s * vv_s)));
    const float combined = (1.0f - dm) * 0.7f + (1.0f - ds) * 0.3f;
    const float percent = combined * 100.0f;
    return (double)(pow15f(percent) / 10.0f);
}

#include "ewk_rescore.h"

// Score one segment from its fp32-rounded mean / std (lane k < 20: coefficient k; one wave):
// wave-parallel dots in a fixed butterfly order, lane 0 finishes the score, writes the
// decision and lists the segment for the fp64 re-score (ewk_rescore.h) when the float32
// pipeline cannot decide it alone.  theta_s: the float32 pass's log-mel max - 80 dB.
template <int RING>
__device__ __forceinline__ void score_epilogue(const ScoreArgs& a, float cmf, float csf, float tmf, float tsf,
                                               int lane, int seg, int len, float theta_s) {
    bool near = a.list_all;
    if (a.has_template) {
        double score, std2, mean2, percent = 0.0;
        if (a.cand_f32) {   // float32 candidates: float products, float-rounded dots (sdot)
            const float uv_m = (float)wave_sum_d((double)(tmf * cmf)), vv_m = (float)wave_sum_d((double)(cmf * cmf));
            const float uv_s = (float)wave_sum_d((double)(tsf * csf)), vv_s = (float)wave_sum_d((double)(csf * csf));
            score = score_f32_finish(a.uu_m32, a.uu_s32, uv_m, vv_m, uv_s, vv_s);
            std2 = vv_s;
            mean2 = vv_m;
        } else {
            const double uv_m = wave_sum_d((double)tmf * (double)cmf), vv_m = wave_sum_d((double)cmf * (double)cmf);
            const double uv_s = wave_sum_d((double)tsf * (double)csf), vv_s = wave_sum_d((double)csf * (double)csf);
            score = score_f64_finish((double)a.uu_m32, (double)a.uu_s32, uv_m, vv_m, uv_s, vv_s, percent);
            std2 = vv_s;
            mean2 = vv_m;
        }
        if (lane == 0) {
            const int match = score >= a.threshold;
            // fp64 re-score: decisions within the margin of the threshold; very short segments
            // (T <= kRescoreFrames) whose 2..16-frame std vectors are too ill-conditioned for the
            // float32 pipeline to meet 1e-4; nearly stationary segments (0 < |std| < kTinyStd:
            // steady noise, or a few bins above the -100 dB floor: std vectors of norm ~1e-2..20
            // whose direction the float32 rounding of the MFCCs (~3e-5 absolute) moves by up to
            // ~3e-4 in the score; scripts/fuzz_err.py over 12 x 200 fuzz segments found 1.3e-4 at
            // |std| = 8); and loud segments whose MFCC mean vector nearly vanishes (|mean| <
            // kTinyMean: c0's positive and negative frames cancel, the float32 log-mel error
            // becomes a direction error, up to 3.6e-4 in the score; DESIGN.md numerics).  An
            // exactly constant segment keeps its NaN (zero std; the reference's own value there
            // is a rounding artefact).
            // (float64 candidates only: a vanishing-mean segment that is NaN beyond the float32 error)
            const bool sure_nan = !a.cand_f32 && percent < -(kNanMarginA / sqrt(mean2) + kNanMarginB);
            near = near || fabs(score - a.threshold) < a.rescore_margin || (1 + len / HOP) <= kRescoreFrames ||
                   (std2 > 0.0 && std2 < kTinyStd * kTinyStd) || (mean2 < kTinyMean * kTinyMean && !sure_nan);
            if (RING) {
                a.events[seg].score = score;
                a.events[seg].match = match;
            } else {
                a.out_score[seg] = score;
                if (a.out_match) a.out_match[seg] = (uint8_t)match;
            }
        }
    }
    if (lane == 0 && near && a.rs_slots) rs_list(a, seg, len, theta_s);   // drained by the re-score launch
}


// Ring modes, statistics for the stream bank (k_bank_events, ewk_bank.hip): the event's float32
// mean / std and the pass's theta_s by event slot (nullptr: none; one wave, lane k < 20:
// coefficient k).
__device__ __forceinline__ void ring_stats_store(const ScoreArgs& a, int seg, int lane, float cmf, float csf,
                                                 float theta_s) {
    if (lane < NMFCC) {
        if (a.out_mean) a.out_mean[(int64_t)seg * NMFCC + lane] = cmf;
        if (a.out_std) a.out_std[(int64_t)seg * NMFCC + lane] = csf;
    }
    if (lane == 0 && a.out_theta) a.out_theta[seg] = theta_s;
}

// MODE 0: linear batch; 1: ring events, one segment per workgroup (cooperative); 2: ring
// events, one segment per wave from the work counter.  S16: int16 rings (EWK_RING_I16).
template <int MODE, int S16>
__global__ __launch_bounds__(64 * WAVES, 1) void k_score_f32(const Tables* __restrict__ tab, ScoreArgs a) {
    constexpr int RING = MODE == 0 ? 0 : (S16 ? 2 : 1);
    const void* ring_base = S16 ? (const void*)a.pcm16 : (const void*)a.pcm;   // ring modes
    constexpr float kWinScale = S16 ? 1.0f / 32768.0f : 1.0f;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // ring mode: the event window and this workgroup's first event, requested before the
    // table fill so their latency overlaps it
    int r_base = 0, r_count = 0;
    ewk_event r_ev = {};
    if (RING) {
        // counters in wrapping count space; slots relative to the bank's epoch base (a watermark
        // left behind an epoch -- no template while its events arrived -- restarts at slot 0)
        r_base = max(0, (int)((uint32_t)*a.ev_base - (uint32_t)a.ev_base0));
        r_count = min((int)((uint32_t)*a.n_events - (uint32_t)a.ev_base0), a.n_seg) - r_base;
        if ((int)blockIdx.x < r_count) r_ev = a.events[r_base + blockIdx.x];
        // one segment per workgroup: a workgroup without one skips the table fill (most of
        // a quiet tick's 256 workgroups)
        if (MODE == 1 && (int)blockIdx.x >= r_count) return;   // (k_rescore_ring ends the tick)
    }
    // ---- cooperative table load (global -> LDS), per-lane rows transposed
    {
        float2* sw2 = reinterpret_cast<float2*>(smem + L_WIN2);
        float2* st1 = reinterpret_cast<float2*>(smem + L_TW1);
        float2* st2 = reinterpret_cast<float2*>(smem + L_TW2);
        for (int i = threadIdx.x; i < 256; i += blockDim.x) {
            const int j = i & 15, n = i >> 4;   // win2[16n + j], tw1[16n + j], tw2[j + 16n]
            sw2[j * TP + n] = make_float2(tab->win2[i].x * kWinScale, tab->win2[i].y * kWinScale);
            if (n > 0) st1[j * TP + n - 1] = tab->tw1[i];
        }
        // [j'][it] = (cos, tan) of tw2[k] for the bin k that lane class j' untangles at step it
        for (int i = threadIdx.x; i < 8 * 17; i += blockDim.x) {
            const int jp = i / 17, it = i % 17;
            const int k = jp ? jp + 16 * (it < 16 ? it : 15) : (it <= 8 ? 16 * it : 8 + 16 * (it - 9));
            const float2 cs = tab->tw2[k];   // (c, t): c = cos is never 0 in float (k = 128: 6.1e-17)
            st2[jp * TP + it] = make_float2(cs.x, cs.y / cs.x);
        }
        int* sb = reinterpret_cast<int*>(smem + L_BLO);
        for (int i = threadIdx.x; i < NMEL; i += blockDim.x) sb[i] = tab->band_lo[i];
        float* sw = reinterpret_cast<float*>(smem + L_WPAD);
        for (int i = threadIdx.x; i < 16 * WP; i += blockDim.x) {
            const int j = i / WP, o = i % WP;
            float w = 0.0f;
#pragma unroll
            for (int g = 0; g < 8; ++g)
                if (o >= kMelOff[g] && o < kMelOff[g] + kMelW[g]) w = tab->wpad[(kMelIt0[g] + o - kMelOff[g]) * 16 + j];
            sw[i] = w;
        }
        // the f16 hi/lo DCT operand chunks (kDctScale keeps the lo parts normal)
        uint4* sd = reinterpret_cast<uint4*>(smem + L_DCT);
        for (int i = threadIdx.x; i < DCT_BYTES / 16; i += blockDim.x) {
            int row = -1, c = 0, hl = 0;
            if (i < DCT_RT1 / 16) {
                const int l = i & 63;
                hl = (i >> 6) & 1;
                row = l & 15;
                c = 4 * (i >> 7) + (l >> 4);
            } else {
                const int k = i - DCT_RT1 / 16, blk = k / 17, slot = k % 17;   // blk = q * 2 + hl
                if (slot < 16) {
                    row = 16 + (slot & 3);
                    c = 4 * (blk >> 1) + (slot >> 2);
                    hl = blk & 1;
                }
            }
            float v[8];
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                const float d = row >= 0 ? tab->dct[row * NMEL + c + 16 * jj] * kDctScale : 0.0f;
                const float h = f16_trunc(d);
                v[jj] = hl ? d - h : h;
            }
            sd[i] = make_uint4(pk_f16(v[0], v[1]), pk_f16(v[2], v[3]), pk_f16(v[4], v[5]), pk_f16(v[6], v[7]));
        }
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int base = 0, count = a.n_seg;
    if (RING) {
        base = r_base;
        count = r_count;
    }
    unsigned char* wbase = smem + L_SHARED_END + wave * W_BYTES;
    float* scr = reinterpret_cast<float*>(smem + L_SCR + wave * SCR_BYTES);
    float* tile = reinterpret_cast<float*>(wbase + W_TILE);
    float* spec = reinterpret_cast<float*>(wbase + W_SPEC);
    int lo[8];   // first bin of this lane's bands j + 16 i
    {
        const int* sb = reinterpret_cast<const int*>(smem + L_BLO);
#pragma unroll
        for (int i = 0; i < 8; ++i) lo[i] = sb[(lane & 15) + 16 * i];
    }
    // persistent waves pull segments from a work counter (ragged lengths balance)
    // the template is loop-invariant: fetched once, off every segment's critical path.
    // (Reserving the next work item ahead was tried: the tail imbalance costs more.)
    const bool act = lane < NMFCC;
    const float tmf = (a.has_template && act) ? a.tmpl[lane] : 0.0f;
    const float tsf = (a.has_template && act) ? a.tmpl[NMFCC + lane] : 0.0f;
    // Ring mode, MODE 1 (a tick of ~10^3-10^4 streams: a few hundred segments, latency
    // bound): one segment per workgroup at a time, its tiles spread over the waves.  MODE 2
    // (10^5-10^6 streams: enough events to keep every wave busy) falls through: the waves
    // take whole segments from the work counter, like a linear batch.
    if (MODE == 1) {
        int* wg_idx = reinterpret_cast<int*>(smem + L_WG);
        float* misc0 = reinterpret_cast<float*>(smem + L_SCR);   // wave 0's FFT scratch (epilogue only)
        // first segment by workgroup index (its event was requested before the table fill),
        // later ones from the work counter (a burst tick's segments balance over the grid)
        for (int idx = blockIdx.x; idx < count;) {
            __syncthreads();   // wave 0's scratch (misc0) and wg_idx are free again
            // the next index is reserved now, its atomic's latency hidden under this segment
            int nxt = 0;
            if (threadIdx.x == 0) nxt = (int)gridDim.x + atomicAdd(a.work, 1);
            const int seg = base + idx;
            const ewk_event ev = idx == (int)blockIdx.x ? r_ev : a.events[seg];
            if (!(ev.flags & EWK_EV_SKIPPED)) {
                const SegSrc<RING> v = make_src<RING>(
                    static_cast<const unsigned char*>(ring_base) + (int64_t)ev.stream * a.ring_len * sample_bytes(RING),
                    ev.ring_start, a.ring_len, ev.length);
                float theta_s;
                segment_stats_coop(v, smem, scr, tile, spec, wave, lane, lo, misc0, theta_s);
                if (wave == 0) ring_stats_store(a, seg, lane, act ? misc0[lane] : 0.0f, act ? misc0[20 + lane] : 0.0f, theta_s);
                if (wave == 0 && (a.has_template || a.list_all))
                    score_epilogue<RING>(a, act ? misc0[lane] : 0.0f, act ? misc0[20 + lane] : 0.0f, tmf, tsf, lane,
                                         seg, v.len, theta_s);
            }
            if (threadIdx.x == 0) wg_idx[0] = nxt;
            __syncthreads();
            idx = wg_idx[0];
        }
        return;   // k_rescore_ring drains the re-score list and ends the tick
    }
#ifdef EWK_TIMING
    uint64_t dbg[kDbgN] = {};
#endif
    const WorkCtx wc = {&a, base, count, true, (int)blockIdx.x * WAVES + wave, (int)gridDim.x * WAVES};
    WorkAhead nx;
    for (;;) {
        EWK_TS(tw0);
        if (nx.state != 3) {   // nothing claimed ahead (first segment, or after a skipped event)
            work_claim<RING>(wc, nx, lane);
            work_order<RING>(wc, nx);
            work_describe<RING>(wc, nx);
        }
        nx.state = 0;
        if (nx.idx >= count) break;
        const int seg = nx.seg;
        int64_t ring = 0;
        const void* p;
        if (RING) {
            if (nx.flags & EWK_EV_SKIPPED) continue;
            p = static_cast<const unsigned char*>(ring_base) + (int64_t)nx.stream * a.ring_len * sample_bytes(RING);
            ring = a.ring_len;
        } else {
            p = a.pcm;
        }
        const SegSrc<RING> v = make_src<RING>(p, nx.start, ring, nx.len);
        EWK_TS(tw1);
        EWK_TADD(0, tw0, tw1);

        double st1[kSlots], st2[kSlots];
        float theta_s;
        segment_stats(v, smem, scr, tile, spec, lane, lo, st1, st2, theta_s, wc, nx EWK_DBG_ARG);
        EWK_TS(tw2);

        // ---- lane k < 20 holds coefficient k's mean / std (fp32-rounded like the reference's)
        const float cmf = act ? (float)st1[0] : 0.0f, csf = act ? (float)st2[0] : 0.0f;
        if (act && !RING) {
            if (a.out_mean) a.out_mean[(int64_t)seg * NMFCC + lane] = cmf;
            if (a.out_std) a.out_std[(int64_t)seg * NMFCC + lane] = csf;
        }
        if (RING) ring_stats_store(a, seg, lane, cmf, csf, theta_s);
        if (a.has_template || a.list_all) score_epilogue<RING>(a, cmf, csf, tmf, tsf, lane, seg, v.len, theta_s);
        lds_order();
        EWK_TS(tw3);
        EWK_TADD(7, tw2, tw3);
#ifdef EWK_TIMING
        dbg[9] += 1;
#endif
    }   // work loop
#ifdef EWK_TIMING
    dbg[8] += 1;
    if (lane == 0)
        for (int k = 0; k < kDbgN; ++k) atomicAdd(&g_ewk_dbg[k], (unsigned long long)dbg[k]);
#endif
    // (the fp64 list is drained by k_rescore_linear / k_rescore_ring, launched after this kernel)
}

#ifdef EWK_RS_TIMING
}  // namespace ewk
extern "C" int ewk_debug_rs(unsigned long long* out) {   // read and reset (debug builds only)
    unsigned long long z[16] = {};
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(ewk::g_rs_dbg), sizeof(z)) != hipSuccess) return -3;
    if (hipMemcpyToSymbol(HIP_SYMBOL(ewk::g_rs_dbg), z, sizeof(z)) != hipSuccess) return -3;
    return 0;
}
extern "C" int ewk_debug_rs_ph(unsigned long long* out) {   // chunk sub-phase cycles (debug builds only)
    unsigned long long z[8] = {};
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(ewk::g_rs_ph), sizeof(z)) != hipSuccess) return -3;
    if (hipMemcpyToSymbol(HIP_SYMBOL(ewk::g_rs_ph), z, sizeof(z)) != hipSuccess) return -3;
    return 0;
}
namespace ewk {
#endif

#ifdef EWK_TIMING
}  // namespace ewk
extern "C" int ewk_debug_timing(unsigned long long* out) {   // read and reset (debug builds only)
    unsigned long long z[kDbgN] = {};
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(ewk::g_ewk_dbg), sizeof(z)) != hipSuccess) return -3;
    if (hipMemcpyToSymbol(HIP_SYMBOL(ewk::g_ewk_dbg), z, sizeof(z)) != hipSuccess) return -3;
    return 0;
}
namespace ewk {
#endif

// Event-count snapshot taken on the gate's stream right after a gate launch: the
// scoring pass that overlaps the next gate scores exactly the events of its own tick.
__global__ void k_snapshot(const int32_t* src, int32_t* dst) { *dst = *src; }

hipError_t launch_snapshot(const int32_t* src, int32_t* dst, hipStream_t s) {
    hipLaunchKernelGGL(k_snapshot, dim3(1), dim3(1), 0, s, src, dst);
    return hipGetLastError();
}

// Poll mirror of an event bank: its four counters and its first min(queued, chunk) events,
// written straight into pinned host memory after the push's last scoring pass (stream-
// ordered, so every score is final).  The host polls it after one event wait instead of
// two D2H copies on a second stream (blit kernels that queue for CU slots behind the next
// gate) and a stream synchronisation.  host: [16 B counters][chunk events], 16-B aligned.
__global__ __launch_bounds__(256) void k_bank_mirror(const int32_t* __restrict__ evc, const ewk_event* __restrict__ ev,
                                                     uint32_t base0, int32_t cap, int32_t chunk,
                                                     unsigned char* __restrict__ host) {
    const uint4 c = *reinterpret_cast<const uint4*>(evc);
    const int32_t n = (int32_t)min(min((uint32_t)(c.x - base0), (uint32_t)cap), (uint32_t)chunk);
    if (threadIdx.x == 0) *reinterpret_cast<uint4*>(host) = c;
    static_assert(sizeof(ewk_event) % 16 == 0, "events copied in 16-B pieces");
    const uint4* src = reinterpret_cast<const uint4*>(ev);
    uint4* dst = reinterpret_cast<uint4*>(host + 16);
    const int nq = n * (int)(sizeof(ewk_event) / 16);
    for (int i = threadIdx.x; i < nq; i += blockDim.x) dst[i] = src[i];
}

hipError_t launch_bank_mirror(const int32_t* evc, const ewk_event* ev, uint32_t base0, int32_t cap, int32_t chunk,
                              unsigned char* host, hipStream_t s) {
    hipLaunchKernelGGL(k_bank_mirror, dim3(1), dim3(256), 0, s, evc, ev, base0, cap, chunk, host);
    return hipGetLastError();
}

// Longest-first work order for a linear batch (LPT: the persistent waves' last
// segments are the shortest, so the grid drains evenly): 64 buckets of the segment's pass
// count, longest first; the order within a bucket is arbitrary (each segment's result
// does not depend on it).
constexpr int kLptBuckets = 64;
__device__ __forceinline__ int lpt_bucket(int32_t len) {   // longest first: bucket 0 = most passes
    const int np = (1 + max(len, 0) / HOP + kFPP - 1) / kFPP;
    return kLptBuckets - 1 - min(np, kLptBuckets - 1);
}

// Grid-parallel LPT order: pass 1 adds each workgroup's bucket histogram of its slice to
// the global totals; pass 2 (every workgroup redoes the 64-bucket exclusive scan) reserves a
// contiguous run per bucket with one atomic on that bucket's cursor and scatters its
// indices.  cnt = order + n: [0, 64) totals, [64, 128) cursors (zeroed before pass 1).
constexpr int kLptBlock = 256;
__global__ __launch_bounds__(kLptBlock) void k_lpt_hist(const int32_t* __restrict__ lengths, int32_t n,
                                                        int32_t* __restrict__ cnt) {
    __shared__ int h[kLptBuckets];
    if (threadIdx.x < kLptBuckets) h[threadIdx.x] = 0;
    __syncthreads();
    for (int i = blockIdx.x * kLptBlock + threadIdx.x; i < n; i += gridDim.x * kLptBlock)
        atomicAdd(&h[lpt_bucket(lengths[i])], 1);
    __syncthreads();
    if (threadIdx.x < kLptBuckets && h[threadIdx.x]) atomicAdd(&cnt[threadIdx.x], h[threadIdx.x]);
}

__global__ __launch_bounds__(kLptBlock) void k_lpt_scatter(const int32_t* __restrict__ lengths, int32_t n,
                                                           int32_t* __restrict__ order, int32_t* __restrict__ cnt,
                                                           int32_t* __restrict__ work, int32_t* __restrict__ rs_ctl) {
    __shared__ int h[kLptBuckets], base[kLptBuckets];
    if (blockIdx.x == 0 && threadIdx.x == 0) {   // the scorer's counters (no fill launches)
        *work = 0;
        for (int i = 0; i < kRsCtl; ++i) rs_ctl[i] = 0;
    }
    if (threadIdx.x < kLptBuckets) h[threadIdx.x] = 0;
    __syncthreads();
    for (int i = blockIdx.x * kLptBlock + threadIdx.x; i < n; i += gridDim.x * kLptBlock)
        atomicAdd(&h[lpt_bucket(lengths[i])], 1);
    __syncthreads();
    if (threadIdx.x < kLptBuckets) {   // one wave: lane = bucket
        const int b = threadIdx.x, tot = cnt[b];
        int incl = tot;
        for (int d = 1; d < kLptBuckets; d <<= 1) {
            const int t = __shfl_up(incl, d, 64);
            if (b >= d) incl += t;
        }
        base[b] = (incl - tot) + (h[b] ? atomicAdd(&cnt[kLptBuckets + b], h[b]) : 0);
        h[b] = 0;
    }
    __syncthreads();
    for (int i = blockIdx.x * kLptBlock + threadIdx.x; i < n; i += gridDim.x * kLptBlock) {
        const int b = lpt_bucket(lengths[i]);
        order[base[b] + atomicAdd(&h[b], 1)] = i;
    }
}

int score_grid(int n_seg, int ring_mode) {
    return ring_mode ? kScoreGridRing : max(1, min((n_seg + WAVES - 1) / WAVES, kScoreGridMax));
}

hipError_t launch_score_f32(const Tables* d_tab, const ScoreArgs& a, int ring_mode, hipStream_t s) {
    if (a.n_seg <= 0) return hipSuccess;
    const int grid = score_grid(a.n_seg, ring_mode);
    if (ring_mode) {   // ring mode: the last workgroup out re-arms the counters after each tick
        if (ring_mode == 2 && a.pcm16) hipLaunchKernelGGL((k_score_f32<2, 1>), dim3(grid), dim3(64 * WAVES), LDS_BYTES, s, d_tab, a);
        else if (ring_mode == 2) hipLaunchKernelGGL((k_score_f32<2, 0>), dim3(grid), dim3(64 * WAVES), LDS_BYTES, s, d_tab, a);
        else if (a.pcm16) hipLaunchKernelGGL((k_score_f32<1, 1>), dim3(grid), dim3(64 * WAVES), LDS_BYTES, s, d_tab, a);
        else hipLaunchKernelGGL((k_score_f32<1, 0>), dim3(grid), dim3(64 * WAVES), LDS_BYTES, s, d_tab, a);
    } else {
        ScoreArgs b = a;
        // the order only matters once the waves queue several segments each
        if (a.order && a.n_seg > 2 * grid * WAVES) {
            int32_t* cnt = a.order + a.n_seg;
            hipError_t e = hipMemsetAsync(cnt, 0, 2 * kLptBuckets * sizeof(int32_t), s);
            if (e != hipSuccess) return e;
            const int g = std::min(256, (a.n_seg + kLptBlock - 1) / kLptBlock);
            hipLaunchKernelGGL(k_lpt_hist, dim3(g), dim3(kLptBlock), 0, s, a.lengths, a.n_seg, cnt);
            hipLaunchKernelGGL(k_lpt_scatter, dim3(g), dim3(kLptBlock), 0, s, a.lengths, a.n_seg, a.order, cnt, a.work,
                               a.rs_ctl);
        } else {
            b.order = nullptr;
            hipError_t e = hipMemsetAsync(a.work, 0, sizeof(int32_t), s);
            if (e == hipSuccess) e = hipMemsetAsync(a.rs_ctl, 0, kRsCtl * sizeof(int32_t), s);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL((k_score_f32<0, 0>), dim3(grid), dim3(64 * WAVES), LDS_BYTES, s, d_tab, b);
    }
    return hipGetLastError();
}

hipError_t launch_rescore_linear(const ScoreArgs& a, hipStream_t s) {
    if (a.n_seg <= 0 || !a.rs_slots) return hipSuccess;
    hipLaunchKernelGGL(k_rescore_linear, dim3(kScoreGridMax), dim3(64 * RS_NW), RS_LDS, s, a);
    return hipGetLastError();
}

// After every ring-mode scorer launch (also without a template: the tick end re-arms the
// counters and advances the watermark).
hipError_t launch_rescore_ring(const ScoreArgs& a, hipStream_t s) {
    if (a.n_seg <= 0) return hipSuccess;
    if (a.pcm16) hipLaunchKernelGGL(k_rescore_ring<2>, dim3(kScoreGridRing), dim3(64 * RS_NW), RS_LDS, s, a);
    else hipLaunchKernelGGL(k_rescore_ring<1>, dim3(kScoreGridRing), dim3(64 * RS_NW), RS_LDS, s, a);
    return hipGetLastError();
}

// The vanishing-mean listing constants above, for the template bank's listing rule.
RescoreCriteria rescore_criteria() { return {kTinyMean, kNanMarginA, kNanMarginB}; }

}  // namespace ewk
