// ewk_mfcc_stats.h -- the float32 scorer's statistics stage: a whole segment, tile by tile, to
// the mean / std of its 20 MFCCs (segment_stats: one wave per segment; segment_stats_coop: one
// workgroup per segment), with the speculative top_db clamp, its shift sums and fix-ups, the
// scout order and the persistent waves' work claiming.  Drives the frame pass and the DCT;
// reads and writes the wave's tile and top_db record (W_TILE, W_SPEC), hands the per-coefficient
// sums over through the waves' scratch (L_SCR) and, in the cooperative mode, meets on L_WG.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "ewk_internal.h"
#include "ewk_topdb_shift.h"
#include "ewk_mfcc_layout.h"
#include "ewk_mfcc_tile.h"
#include "ewk_mfcc_fft.h"
#include "ewk_mfcc_dct.h"

namespace ewk {

// fp64 shifted sums of the frame columns that exist (d = c - cref).
__device__ __forceinline__ void stats_add(const float (&c)[kSlots], const float (&cref)[kSlots], bool ok, double (&s1)[kSlots],
                                          double (&s2)[kSlots]) {
    if (ok) {
#pragma unroll
        for (int i = 0; i < kSlots; ++i) {
            const double d = (double)c[i] - (double)cref[i];
            s1[i] += d;
            s2[i] = fma(d, d, s2[i]);
        }
    }
}

// Swap one tile's contribution: remove the unclamped columns `co`, add the clamped `cn`.
__device__ __forceinline__ void stats_replace(const float (&cn)[kSlots], const float (&co)[kSlots], const float (&cref)[kSlots],
                                              bool ok, double (&s1)[kSlots], double (&s2)[kSlots]) {
    if (ok) {
#pragma unroll
        for (int i = 0; i < kSlots; ++i) {
            const double dn = (double)cn[i] - (double)cref[i], dd = (double)co[i] - (double)cref[i];
            s1[i] += dn - dd;
            s2[i] += fma(dn, dn, -dd * dd);
        }
    }
}

// ---- top_db shift sums (ewk_topdb_shift.h): A, B, C per lane and coefficient slot, in float32
// next to s1 / s2 (the registers of the three row-tile-1 slots that hold no coefficient).
// A masked tile's columns (c at the tile's clamp, m its mask DCT) join the sums.
__device__ __forceinline__ void shift_tile_add(const float (&c)[kSlots], const float (&cref)[kSlots],
                                               const float (&m)[kSlots], bool ok, float (&sA)[kSlots],
                                               float (&sB)[kSlots], float (&sC)[kSlots]) {
    if (ok) {
#pragma unroll
        for (int i = 0; i < kSlots; ++i) shift_add<float, float>(c[i] - cref[i], m[i], sA[i], sB[i], sC[i]);
    }
}
// The clamp of every column in the sums rises by delta.
__device__ __forceinline__ void shift_apply(double delta, const float (&sA)[kSlots], float (&sB)[kSlots],
                                            const float (&sC)[kSlots], double (&s1)[kSlots], double (&s2)[kSlots]) {
#pragma unroll
    for (int i = 0; i < kSlots; ++i) shift_rise<float, float>(delta, sA[i], sB[i], sC[i], s1[i], s2[i]);
}
// Swap one masked tile's contribution: out go its stored columns as shifted to theta.
__device__ __forceinline__ void stats_replace_shift(const float (&cn)[kSlots], const float (&co)[kSlots], const float (&m)[kSlots],
                                                    double delta, const float (&cref)[kSlots], bool ok, double (&s1)[kSlots],
                                                    double (&s2)[kSlots]) {
    if (ok) {
#pragma unroll
        for (int i = 0; i < kSlots; ++i)
            shift_replace((double)cn[i], (double)co[i], (double)m[i], delta, (double)cref[i], s1[i], s2[i]);
    }
}

// Minima of a float over the lanes of each 8-frame pass of a tile (frame column & 8), no LDS.
__device__ __forceinline__ void pass_mins(float x, float (&pm)[2]) {
    x = fminf(x, __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(x), __float_as_int(x), 0x111, 0xf, 0xf, false)));
    x = fminf(x, __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(x), __float_as_int(x), 0x112, 0xf, 0xf, false)));
    x = fminf(x, __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(x), __float_as_int(x), 0x114, 0xf, 0xf, false)));
#pragma unroll
    for (int p = 0; p < 2; ++p) {   // lane 7 of a row: columns 0..7; lane 15: columns 8..15
        const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 7 + 8 * p));
        const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 23 + 8 * p));
        const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 39 + 8 * p));
        const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 55 + 8 * p));
        pm[p] = fminf(fminf(r0, r1), fminf(r2, r3));
    }
}

// Wave minimum / maximum of a float, no LDS: a DPP row scan (row_shr 1, 2, 4, 8: lane 15 of a
// row holds the row's), row_bcast:15 into rows 1 and 3 and row_bcast:31 into rows 2 and 3 (lane
// 63 holds the wave's), one readlane.  Written out: through fminf / fmaxf every DPP step costs a
// copy and a canonicalising v_max_f32 x, x beside the move and the min (ewk_mfcc_dct.h,
// clamp_mask).  The hazard recogniser does not see into the statement, so it carries its own wait
// states: s_nop 1 between a VALU write and a DPP read of the same register (two), s_nop 4 in
// front (five: a VALU write of EXEC before a DPP instruction), s_nop 1 at the end for the
// readlane.  A lane whose source is outside its row, or whose row the row_mask leaves out, keeps
// its value.  A NaN operand yields the other operand (v_min_f32 / v_max_f32, IEEE mode), like
// fminf / fmaxf; the callers' values (pass minima, the running max, scout energies) hold none.
#define EWK_WAVE_RED(op)                                                                       \
    "s_nop 4\n\t" op " %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"                    \
    "s_nop 1\n\t" op " %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"                    \
    "s_nop 1\n\t" op " %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"                    \
    "s_nop 1\n\t" op " %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"                    \
    "s_nop 1\n\t" op " %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"                 \
    "s_nop 1\n\t" op " %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"                 \
    "s_nop 1"
__device__ __forceinline__ float wave_min(float x) {
    asm(EWK_WAVE_RED("v_min_f32_dpp") : "+v"(x));
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 63));
}
__device__ __forceinline__ float wave_max(float x) {
    asm(EWK_WAVE_RED("v_max_f32_dpp") : "+v"(x));
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 63));
}

// Sum over the 16 lanes of each row (DPP row_shr scan, no LDS); the total lands in lane 15 of the row.
// DPP move of a double: two dword moves.  BOUND: lanes without a source read 0 (the bound-control
// form: no `old` register of zeros per half); the permutations below have a source in every lane.
template <int CTRL, bool BOUND>
__device__ __forceinline__ double dpp_d(double x) {
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(x), CTRL, 0xf, 0xf, BOUND);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(x), CTRL, 0xf, 0xf, BOUND);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double row_sum_d(double x) {
    x += dpp_d<0x111, true>(x);   // row_shr:1
    x += dpp_d<0x112, true>(x);   // row_shr:2
    x += dpp_d<0x114, true>(x);   // row_shr:4
    x += dpp_d<0x118, true>(x);   // row_shr:8
    return x;
}

// Sum over the wave (rows via DPP, then the four row totals via readlane); uniform result.
__device__ __forceinline__ double wave_sum_d(double x) {
    x = row_sum_d(x);
    double t = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r)
        t += __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), 16 * r + 15),
                              __builtin_amdgcn_readlane(__double2loint(x), 16 * r + 15));
    return t;
}

// Row scan of a float (row_shr 1, 2, 4, 8; lanes without a source add 0): lane 15 of a row holds
// ((x0 + x1) + (x2 + x3)) + ... over the row's 16 lanes, a balanced tree.
__device__ __forceinline__ float row_sum_f(float x) {
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x111, 0xf, 0xf, false));
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x112, 0xf, 0xf, false));
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x114, 0xf, 0xf, false));
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x118, 0xf, 0xf, false));
    return x;
}

// Sum of a float over the wave (DPP row scans, the row totals via readlane); uniform result.
__device__ __forceinline__ float wave_sum_f(float x) {
    x = row_sum_f(x);
    return (__int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 15)) +
            __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 31))) +
           (__int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 47)) +
            __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 63)));
}

// The per-lane sums s1[0..4], s2[0..4] summed over the 16 frame columns of each row and handed
// over, with cref, to the wave's scratch `pd` ([coefficient][S1, S2, cref] doubles; coefficient
// 4 h + r for slot r < 4 of row h, 16 + h for slot 4).  Every total is the balanced tree of the
// row_shr scan, ((x0 + x1) + (x2 + x3)) + ..., the same pairs added at every level (an addition
// is commutative, so the pairing fixes the bits), but as a narrowing reduction: at each level the
// two lanes of a pair exchange half of what they carry and each adds the other half, so a lane
// carries 10, 5, 3, 2 and at last 1 value instead of 10 at all four levels (12 additions of
// doubles, not 40).  Level by level, a lane's partner and what decides which half it keeps
// (b0..b3: the bits of its column):
//   columns 2i | 2i+1        partner col ^ 1  (quad_perm [1,0,3,2])   k1 = b0 ^ b2: keeps s2, else s1
//   pairs of a quad          partner col ^ 2  (quad_perm [2,3,0,1])   k2 = b1 ^ b2: the odd slot
//   quads of a half row      partner col ^ 7  (row_half_mirror)       k3 = b2 ^ b3: slots 2, 3
//   half rows                partner col ^ 15 (row_mirror)            both lanes add
// A partner at any level holds the same kind of value (k1 is the same in col ^ 2, col ^ 7 and
// col ^ 15, k2 in col ^ 7 and col ^ 15, k3 in col ^ 15).  Slot 4 has no partner slot after the
// first level and is added over the full butterfly.  In the end a lane holds the total of
// (k1 ? s2 : s1)[2 k3 + k2] and of (k1 ? s2 : s1)[4] and stores both; lanes that hold the same
// total store the same bits.
__device__ __forceinline__ void row_sums_to_pd(const float (&cref)[kSlots], const double (&s1)[kSlots],
                                               const double (&s2)[kSlots], int lane, double* pd) {
    // (once per segment: the lane's predicates and addresses are recomputed here, not kept in
    // registers across the work loop and its frame passes)
    asm volatile("" : "+v"(lane));
    const int col = lane & 15, h = lane >> 4;
    const bool k1 = ((col ^ (col >> 2)) & 1) != 0, k2 = (((col >> 1) ^ (col >> 2)) & 1) != 0,
               k3 = (((col >> 2) ^ (col >> 3)) & 1) != 0;
    double v[kSlots];
#pragma unroll
    for (int i = 0; i < kSlots; ++i) {   // columns 2i, 2i + 1
        const double a = s1[i], b = s2[i];
        v[i] = (k1 ? b : a) + dpp_d<0xB1, false>(k1 ? a : b);
    }
    double w[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {        // the two pairs of a quad
        const double a = v[2 * i], b = v[2 * i + 1];
        w[i] = (k2 ? b : a) + dpp_d<0x4E, false>(k2 ? a : b);
    }
    v[4] += dpp_d<0x4E, false>(v[4]);
    const double w0 = w[0], w1 = w[1];
    double z = (k3 ? w1 : w0) + dpp_d<0x141, false>(k3 ? w0 : w1);   // the two quads of a half row
    v[4] += dpp_d<0x141, false>(v[4]);
    z += dpp_d<0x140, false>(z);       // the two half rows
    v[4] += dpp_d<0x140, false>(v[4]);
    // (selects of values: a conditional between the array's elements becomes an indexed read of
    // cref, which puts the array in scratch memory)
    const float r0 = cref[0], r1 = cref[1], r2 = cref[2], r3 = cref[3];
    const float c01 = k2 ? r1 : r0, c23 = k2 ? r3 : r2;
    const float cz = k3 ? c23 : c01;
    const int k = 4 * h + 2 * (int)k3 + (int)k2, kk = 16 + h;
    pd[3 * k + (int)k1] = z;
    pd[3 * k + 2] = (double)cz;
    pd[3 * kk + (int)k1] = v[4];
    pd[3 * kk + 2] = (double)cref[4];
}

// Reduce the per-lane sums over the 16 frame columns (row_sums_to_pd), hand each
// coefficient's (S1, S2, cref) to lane k = coefficient through the
// wave's scratch `pd` (20 x 3 doubles), and finish there: lane k < 20 returns its mean in
// s1[0] and its population std in s2[0] (one fp64 division + sqrt per lane, not eight).
__device__ __forceinline__ void finish_stats(int T, const float (&cref)[kSlots], double (&s1)[kSlots], double (&s2)[kSlots],
                                             int lane, double* pd) {
    row_sums_to_pd(cref, s1, s2, lane, pd);
    lds_order();
    if (lane < NMFCC) {
        const double S1 = pd[3 * lane], S2 = pd[3 * lane + 1], r0 = pd[3 * lane + 2];
        const double Td = (double)T;
        const double mean = r0 + S1 / Td;
        double var = (S2 - S1 * S1 / Td) / Td;
        var = var > 0.0 ? var : 0.0;
        s1[0] = mean;
        s2[0] = sqrt(var);
    }
    lds_order();
}

// Zero the kFPP tile rows of one pass (frames past T).
__device__ __forceinline__ void zero_rows(float* tile, int row0, int lane) {
    for (int m = lane; m < kFPP * NMEL; m += 64) tile[row0 * NMEL + m] = 0.0f;
}

// The tiles of one segment that pass 1 left holding a value below the final max - 80 dB
// are recomputed: the stored tile (clamped at its speculative `run`, rebuilt bit for bit
// by the same frame passes) gives the pass-1 DCT columns to remove, the tile clamped at
// theta in LDS the columns to add.  (Parking every tile in global memory for this pass
// instead wrote 10 KB per 16 frames -- 2.3x the algorithmic traffic -- for the ~16 % of
// bench tiles that need it; recomputing those costs the same time.  Parking only the tiles
// the scout ranks within 3 dB of a later one -- 2.8 per bench segment, 0.47 of them fixed --
// lost 1.5 % too: the parking stores hold up the next pass's vmcnt waits, and a reload
// costs 2/3 of a recompute.  profiles/r03_v2_park_ab.txt.  Rebuilding a self-clamped tile's
// stored image exactly -- its clamp at the run before it, then at its own -- so that the
// columns taken out equal the ones put in to the last bit cost 1.3 %, for score changes of
// ~1e-9: the fix-up recomputes at the tile's final run.  A full-coverage scout (Hann-weighted
// frame energies from every sample, scripts/scout_sim.py H8) cut the recomputes from 0.53 to
// 0.11 tiles per bench segment but its loads cost 4x the time saved: r03_v3_scout_ab.txt.)
// Passes of one tile; `mask` bit p selects pass p (the others' rows are zeroed, like the
// rows of frames past T).
constexpr int kPassesPerTile = 16 / kFPP;
constexpr int kAllPasses = (1 << kPassesPerTile) - 1;
template <int RING>
__device__ __forceinline__ void tile_passes(const SegSrc<RING>& v, int tile_i, int T, const unsigned char* smem,
                                            float* scr, float* tile, int lane, const int (&lo)[8], float& mx,
                                            float& mn, float& nanp, float clampv, int mask = kAllPasses) {
    const int npass = (T + kFPP - 1) / kFPP;
    const int p0 = tile_i * kPassesPerTile;
    mask &= npass - p0 >= kPassesPerTile ? kAllPasses : (1 << max(0, npass - p0)) - 1;
    if (mask) {   // stage the tile's first selected pass
        float r[kStageLoads];
        stage_load(v, (p0 + __builtin_ctz(mask)) * kFPP * HOP - NFFT / 2, lane, r);
        stage_store(scr, lane, r);
        lds_order();
    }
#pragma unroll 1
    for (int p = 0; p < kPassesPerTile; ++p) {
        if ((mask >> p) & 1) {
            const int rest = mask >> (p + 1);   // the next selected pass of this tile is prefetched
            frame_pass(v, (p0 + p) * kFPP, T, p * kFPP, rest ? (p0 + p + 1 + __builtin_ctz(rest)) * kFPP : -1,
                       smem, scr, tile, lane, lo, mx, mn, nanp, clampv EWK_PASS_ARG(nullptr));
        } else {   // frames past T, or a pass left out: zero rows (their columns are not used)
            zero_rows(tile, p * kFPP, lane);
        }
    }
    lds_order();
}

// The passes in `mask` of a tile whose stored values (clamped at `run`) include some below
// the final threshold: recomputed bit for bit, their DCT columns swapped from clamped-at-run
// to clamped-at-theta in the shifted sums.  A pass whose stored minimum is >= theta is
// unchanged and skipped (per-pass records, segment_stats).
template <int RING>
__device__ __forceinline__ void fix_tile(const SegSrc<RING>& v, int tile_i, int T, float run, float theta,
                                         const unsigned char* smem, float* scr, float* tile, int lane,
                                         const int (&lo)[8], const float (&cref)[kSlots], double (&s1)[kSlots],
                                         double (&s2)[kSlots], int mask = kAllPasses, bool shifted = false) {
    const float* s_dct = reinterpret_cast<const float*>(smem + L_DCT);
    float d0 = 0.f, d1 = 0.f, d2 = 0.f;
    tile_passes(v, tile_i, T, smem, scr, tile, lane, lo, d0, d1, d2, run, mask);
    float co[kSlots], cn[kSlots], m[kSlots];
    // shifted: the tile's clamped entries went into the shift sums (segment_stats) and the
    // rises since have moved its stored columns to co + (theta - run) m
    const ClampPair cp = clamp_pair(run), ct = clamp_pair(theta);
    if (shifted) tile_dct_m<true>(tile, s_dct, lane, co, m, d0, cp);
    else tile_dct(tile, s_dct, lane, co);
    {
        uint4 h[4], l[4];
        clamp_load(reinterpret_cast<const float4*>(tile), lane, h, l);
        clamp_store(tile, lane, h, l, theta);
    }
    lds_order();
    tile_dct(tile, s_dct, lane, cn);
    const int col = lane & 15;
    const bool ok = tile_i * 16 + col < T && ((mask >> (col / kFPP)) & 1);
    if (shifted) stats_replace_shift(cn, co, m, (double)ct.eff - (double)cp.eff, cref, ok, s1, s2);
    else stats_replace(cn, co, cref, ok, s1, s2);
}

// Scout of a segment's tiles (tile t: frames 16t .. 16t + 15): the energy of 4 x 64 of its
// samples (one 64-sample row every 640), wave-reduced; lane t returns the estimate for tile
// t (t < ntile <= 64).  Only a processing-order heuristic: the results do not depend on it.
constexpr int kScoutBatch = 8;   // tiles whose scout loads are in flight together
template <int RING, int NB>
__device__ __forceinline__ void scout_batch(const SegSrc<RING>& v, int t0, int lane, float& e) {
    float x[NB][4];
#pragma unroll
    for (int u = 0; u < NB; ++u) {   // tiles t0 + u (past the segment: range-checked zeros)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int qs = (t0 + u) * 16 * HOP + 640 * q + 64 + lane;
            int off;
            if (RING) {
                const int phys = qs >= v.wrap_at ? qs - v.wrap_at : qs + v.start;
                off = (unsigned)qs < (unsigned)v.len ? phys * sample_bytes(RING) : -1;
            } else {
                off = qs * 4;
            }
            if (RING == 2)
                x[u][q] = (float)(short)__builtin_amdgcn_raw_buffer_load_b16(v.rsrc, off, 0, 0);
            else
                x[u][q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(v.rsrc, off, 0, 0));
        }
    }
#pragma unroll
    for (int u = 0; u < NB; ++u) {
        float a = x[u][0] * x[u][0];
#pragma unroll
        for (int q = 1; q < 4; ++q) a = fmaf(x[u][q], x[u][q], a);
        const float tot = wave_sum_f(a);
        if (lane == t0 + u) e = tot;
    }
}

// The same sums for a linear batch, sixteen lanes per tile: lane l of lane row R loads columns
// 4l .. 4l + 3 of each of the four sample rows of tile t0 + 4g + R (one 16-byte load per sample
// row: four loads serve four tiles; the range check zeroes each dword past the segment end on its
// own, scripts/probes/buffer_range_probe.hip, so a row that straddles the end reads what four
// dword loads read).  Each column's square sum is the chain above; (c0 + c1) + (c2 + c3) in the
// lane and the row scan's distances 1 and 2 are the four levels of wave_sum_f's tree over 16
// consecutive columns, its distances 4 and 8 are (r0 + r1) + (r2 + r3): the same pairs at every
// level, so the same bits.  The tile's total lands in lane 15 of its lane row.  (Lanes t0 ..
// t0 + 4G - 1 are set, past ntile to the 0 of samples past the end, where scout_batch leaves
// -1 beyond its batch: such lanes are neither ranked nor near, and never the maximum.)
template <int G>
__device__ __forceinline__ void scout_quads(const SegSrc<0>& v, int t0, int lane, float& e) {
    int ln = lane;   // (the load offsets are recomputed per call, not kept across the work loop)
    asm volatile("" : "+v"(ln));
    const int R = ln >> 4, l = ln & 15;
    floatx4 x[G][4];
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int qs = (t0 + 4 * g + R) * 16 * HOP + 640 * q + 64 + 4 * l;
            x[g][q] = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(v.rsrc, qs * 4, 0, 0));
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        float c[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            c[i] = x[g][0][i] * x[g][0][i];
#pragma unroll
            for (int q = 1; q < 4; ++q) c[i] = fmaf(x[g][q][i], x[g][q][i], c[i]);
        }
        const float tot = row_sum_f((c[0] + c[1]) + (c[2] + c[3]));
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float tr = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(tot), 16 * r + 15));
            if (lane == t0 + 4 * g + r) e = tr;
        }
    }
}

// Scout of a segment's tiles (tile t: frames 16t .. 16t + 15): the energy of 4 x 64 of its
// samples (one 64-sample row every 640), wave-reduced; lane t returns the estimate for tile
// t (t < ntile <= 64).  Only a processing-order heuristic: the results do not depend on it.
// The loads of 8 tiles are in flight together (one memory round trip per 1.3 s of segment).
// Linear batches take scout_quads; the rings (wrap, int16 samples) keep one lane per column.
// (scripts/scout_sim.py replays the order on the oracle's log-mel: this scout leaves ~7 % of
// the bench's tiles to recompute, none with the true tile maxima; max-of-rows variants and
// twice the loads reach 6.1 %.)
template <int RING>
__device__ __forceinline__ float scout_tiles(const SegSrc<RING>& v, int ntile, int lane) {
    float e = -1.0f;
    for (int t0 = 0; t0 < ntile; t0 += kScoutBatch) {
        // the batch sized to the tiles left (a short segment's scout issues 2 or 4 tiles' loads
        // and reductions, not 8)
        const int left = ntile - t0;
        if constexpr (RING == 0) {
            if (left <= 4) scout_quads<1>(v, t0, lane, e);
            else scout_quads<kScoutBatch / 4>(v, t0, lane, e);
        } else if (left <= 2) scout_batch<RING, 2>(v, t0, lane, e);
        else if (left <= 4) scout_batch<RING, 4>(v, t0, lane, e);
        else scout_batch<RING, kScoutBatch>(v, t0, lane, e);
    }
    return e;
}

// The next work item of a persistent wave (linear batches, ring mode 2), claimed ahead:
// its index is requested when the current segment's last tile starts, its work-order entry
// when that tile's passes end and its descriptor before the fix-ups, so neither the atomic
// nor the two dependent loads sit between two segments.  (Claiming at the segment start
// instead holds a reservation for a whole segment and costs more at the batch tail.)
struct WorkAhead {
    int state = 0;      // 0 none, 1 index requested (lane 0), 2 index known, 3 described
    bool first = true;  // the wave's first claim: its own index, no atomic
    int idx = 0;
    int seg = 0;
    int64_t start = 0;
    int32_t len = 0;
    int32_t stream = 0;
    int32_t flags = 0;
};
struct WorkCtx {
    const ScoreArgs* a;
    int base, count;
    bool ahead;         // claim the next item during this segment
    int wid, nw;        // this wave's index in the grid, the grid's waves
};

// The first item of every wave is its own index (work items 0 .. nw - 1), the rest come from
// the counter: one device-scope fetch-add address serves ~1 claim per 11 ns, and a launch's
// first claims all arrive together (2,048 of them: ~23 us for the last;
// scripts/probes/atomic_probe.hip).
template <int RING>
__device__ __forceinline__ void work_claim(const WorkCtx& c, WorkAhead& w, int lane) {
    if (w.first) {
        w.idx = c.wid;
        w.first = false;
    } else if (lane == 0) {
        w.idx = c.nw + atomicAdd(c.a->work, 1);
    }
    w.state = 1;
}
template <int RING>
__device__ __forceinline__ void work_order(const WorkCtx& c, WorkAhead& w) {
    w.idx = __shfl(w.idx, 0, 64);
    w.state = 2;
    if (w.idx < c.count) w.seg = c.base + ((!RING && c.a->order) ? c.a->order[w.idx] : w.idx);
}
template <int RING>
__device__ __forceinline__ void work_describe(const WorkCtx& c, WorkAhead& w) {
    w.state = 3;
    if (w.idx >= c.count) return;
    if (RING) {
        const ewk_event ev = c.a->events[w.seg];
        w.start = ev.ring_start;
        w.len = ev.length;
        w.stream = ev.stream;
        w.flags = ev.flags;
    } else {
        w.start = c.a->offsets[w.seg];
        w.len = c.a->lengths[w.seg];
    }
}

// Whole segment for one wave.  spec: this wave's per-tile record in LDS -- the stored
// log-mel minimum of pass p of tile i (of the values above the clamp, for a tile that holds
// clamped entries) in spec[kPassesPerTile * i + p], the tile's
// speculative clamp in spec[kSpecRun + i] (tiles past kSpecTiles are stored unclamped and
// always recomputed when theta bites), then the processing order (spec[kSpecOrder + k]).
//
// The top_db clamp (max - 80 dB over the whole segment) is applied speculatively at the
// running max, which each tile updates before its DCT; a tile that already holds the
// segment max needs no fix, so the tiles are processed loudest first by a scout estimate
// (bench batch: 16 % of the tiles recomputed in time order, ~5 % in scout order).  When the
// clamp rises, the clamped entries of the earlier tiles move up with it inside the sums
// (ewk_topdb_shift.h); only the passes of a tile that hold an unclamped value below the final
// threshold are recomputed (0.06 per bench segment).  A tile joins those sums (its mask DCT) only
// while the scout still ranks a tile to come near the loudest (mask_wanted: 1.25 of the 2.99
// tiles with clamped entries per bench segment); the others are recomputed if the clamp does rise.
template <int RING>
__device__ void segment_stats(const SegSrc<RING>& v, const unsigned char* smem, float* scr, float* tile,
                              float* spec, int lane, const int (&lo)[8], double (&s1)[kSlots], double (&s2)[kSlots],
                              float& theta_out, const WorkCtx& wc, WorkAhead& nx EWK_DBG_PARAM) {
    EWK_TS(tq0);
    const float* s_dct = reinterpret_cast<const float*>(smem + L_DCT);
    const int T = 1 + v.len / HOP;
    const int ntile = (T + 15) >> 4;
    const int npass = (T + kFPP - 1) / kFPP;
    const int col = lane & 15;
    int* order = reinterpret_cast<int*>(spec + kSpecOrder);
    const bool ordered = ntile > 1 && ntile <= kSpecTiles;
    // the tiles that may get a mask: positions 0 .. near - 2 (mask_wanted); a segment taken in
    // time order keeps every mask, a single tile is its own last
    int near = ntile > 1 ? kSpecTiles + 1 : 1;
    if (ordered) {   // loudest-first order: lane t ranks tile t (ties by index)
        float e = scout_tiles(v, ntile, lane);
        e = e == e ? e : 0.0f;   // NaN samples: a total order (unique ranks) all the same
        // (lanes past ntile hold -1: never the max, never near)
        const float e_max = wave_max(e);
        near = __builtin_popcountll(__ballot(lane < ntile && mask_near(e, e_max)));
        int rank = 0;
        for (int u = 0; u < ntile; ++u) {
            const float eu = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(e), u));
            rank += (eu > e) || (eu == e && u < lane);
        }
        if (lane < ntile) order[rank] = lane;
        lds_order();
    }
    EWK_TS(tq1);
    EWK_TADD(1, tq0, tq1);
    float cref[kSlots];
#pragma unroll
    for (int i = 0; i < kSlots; ++i) { s1[i] = 0.0; s2[i] = 0.0; cref[i] = 0.0f; }
    float vmax = -INFINITY, nanp = 0.0f;
    int tile_i = ordered ? order[0] : 0;
    {   // stage the first pass synchronously
        float r[kStageLoads];
        stage_load(v, tile_i * 16 * HOP - NFFT / 2, lane, r);
        stage_store(scr, lane, r);
        lds_order();
    }
    EWK_TS(tq2);
    EWK_TADD(2, tq1, tq2);
    float run = -INFINITY;   // speculative clamp: running max - 80 dB
    // top_db shift (ewk_topdb_shift.h): srun = the clamp at which the clamped entries of the
    // recorded tiles so far sit in the sums, nshift = some tile has joined the shift sums,
    // shifted = which tiles have, amin = the smallest record (what pass 2 has to look at)
    static_assert(kPassesPerTile == 2, "pass_mins splits a tile in two passes");
    float srun = -INFINITY, amin = INFINITY;
    int nshift = 0;
    float sA[kSlots], sB[kSlots], sC[kSlots];
#pragma unroll
    for (int i = 0; i < kSlots; ++i) { sA[i] = 0.0f; sB[i] = 0.0f; sC[i] = 0.0f; }
    uint64_t shifted = 0;
#ifdef EWK_TIMING
    uint64_t skipped = 0;   // tiles with clamped entries left without a mask
#endif
    for (int k = 0; k < ntile; ++k) {
        EWK_TS(tk0);
        const int next_tile = k + 1 < ntile ? (ordered ? order[k + 1] : k + 1) : -1;
        const bool rec = tile_i < kSpecTiles;
        float tmw = INFINITY;
        if (!rec) run = -INFINITY;
        const bool last = k + 1 == ntile;
        if (last && wc.ahead) work_claim<RING>(wc, nx, lane);
#pragma unroll 1
        for (int p = 0; p < kPassesPerTile; ++p) {
            const int pass = tile_i * kPassesPerTile + p;
            // the next pass to prefetch: this tile's next, else the next tile's first
            const int nxt = p + 1 < kPassesPerTile && pass + 1 < npass ? (pass + 1) * kFPP
                                                                      : (next_tile >= 0 ? next_tile * 16 : -1);
            float tp = INFINITY;
            if (pass < npass)
                frame_pass(v, pass * kFPP, T, p * kFPP, nxt, smem, scr, tile, lane, lo, vmax, tp, nanp, run EWK_PASS_ARG(dbg));
            else   // rows of frames past T: zero (ignored by the statistics)
                zero_rows(tile, p * kFPP, lane);
            const float tpw = wave_min(tp);   // this pass's minimum (its record below)
            tmw = fminf(tmw, tpw);
            if (lane == 0 && rec) spec[kPassesPerTile * tile_i + p] = tpw;
        }
        lds_order();
        EWK_TS(tk1);
        EWK_TADD(3, tk0, tk1);
        if (last && wc.ahead) work_order<RING>(wc, nx);
        // max(max(x, run), final) = max(x, final): a tile stored clamped at the running max
        // (this tile's own values included) is exact unless a later tile raises the max
        const float run2 = rec ? wave_max(vmax) - kTopDbUnits : -INFINITY;
        if (run2 > run && tmw < run2) {   // this tile raised the max over some of its own values
            uint4 h[4], l[4];
            clamp_load(reinterpret_cast<const float4*>(tile), lane, h, l);
            clamp_store(tile, lane, h, l, run2);
            lds_order();
        }
        run = fmaxf(run, run2);
        // the clamp rose: the clamped entries of the tiles before this one move up with it
        if (rec) {
            if (nshift && run > srun) shift_apply((double)clamp_pair(run).eff - (double)clamp_pair(srun).eff, sA, sB, sC, s1, s2);
            srun = run;
        }
        // a tile with clamped entries (only such a tile can be wrong once the max rises again):
        // its mask DCT joins the shift sums and its record is the minimum above the clamp.
        // Only where the clamp can still rise (mask_wanted, ewk_topdb_shift.h: a tile near the
        // loudest by the scout is still to come; never the last tile, whose clamp is theta).
        // Left without a mask the tile is kept like one without clamped entries: records
        // fmaxf(pass min, run) (== run for a pass that holds a clamped entry), amin the same,
        // shifted bit 0, nothing in A / B / C.  If no later tile raises the clamp nothing differs,
        // bit for bit; if one does, those passes have record == run < theta, shift_flags selects
        // them and fix_tile(shifted = false) rebuilds the stored columns at the tile's recorded
        // run (spec[kSpecRun]: for a self-clamped tile the run after its own rise, as for a masked
        // one) and swaps them with stats_replace.  shift_apply only moves tiles that joined the sums.
        const bool clamped = rec && tmw < run;
        const bool masked = clamped && mask_wanted(k, near);
#ifdef EWK_TIMING
        if (clamped && !masked) { dbg[24] += 1; skipped |= 1ull << tile_i; }
#endif
        const bool ok = tile_i * 16 + col < T;
        float c[kSlots], m[kSlots], mnab = INFINITY;
        EWK_TS(tm0);
        if (masked) tile_dct_m<true>(tile, s_dct, lane, c, m, mnab, clamp_pair(run));
        else tile_dct(tile, s_dct, lane, c);
        EWK_TS(tm1);
        if (k == 0) {
#pragma unroll
            for (int i = 0; i < kSlots; ++i) cref[i] = __shfl(c[i], lane & 48, 64);
        }
        stats_add(c, cref, ok, s1, s2);
        float pm[kPassesPerTile] = {INFINITY, INFINITY};
        EWK_TS(tm3);
        if (masked) {
            shift_tile_add(c, cref, m, ok, sA, sB, sC);
            nshift = 1;
            shifted |= 1ull << tile_i;
            pass_mins(ok ? mnab : INFINITY, pm);
            amin = fminf(amin, fminf(pm[0], pm[1]));
#ifdef EWK_TIMING   // the mask phase: a masked tile's DCT with the mask DCT, its sums and minima
            EWK_TS(tm2);
            dbg[20] += 1;
            dbg[21] += (tm1 - tm0) + (tm2 - tm3);
#endif
        } else {
            amin = fminf(amin, fmaxf(tmw, run));
        }
        if (lane == 0 && rec) {   // stored minima: the pass minima as clamped at the tile's run
#pragma unroll
            for (int p = 0; p < kPassesPerTile; ++p)
                spec[kPassesPerTile * tile_i + p] = masked ? pm[p] : fmaxf(spec[kPassesPerTile * tile_i + p], run);
            spec[kSpecRun + tile_i] = run;
        }
        tile_i = next_tile;
        EWK_TS(tk2);
        EWK_TADD(4, tk1, tk2);
#ifdef EWK_TIMING
        if (!masked) { dbg[22] += tm1 - tm0; dbg[23] += 1; }   // the plain DCT the mask phase is set against
#endif
    }
    EWK_TS(tq3);
    if (wc.ahead) work_describe<RING>(wc, nx);
    // wave-wide log-mel max
    vmax = wave_max(vmax);
    const float theta = vmax - kTopDbUnits;
    theta_out = theta;
    // the last rise, to the final threshold: every stored clamped entry now sits at theta
    if (nshift && theta > srun) shift_apply((double)clamp_pair(theta).eff - (double)clamp_pair(srun).eff, sA, sB, sC, s1, s2);
    if (amin < theta) {   // some tile holds an unclamped value below theta
        lds_order();
        for (int cur = 0; cur < ntile; ++cur) {
            const bool rec = cur < kSpecTiles;
            int mask = kAllPasses;
            if (rec) {   // only the passes holding an unclamped stored value below theta change
                mask = 0;
#pragma unroll
                for (int p = 0; p < kPassesPerTile; ++p) mask |= (shift_flags<float>(spec[kPassesPerTile * cur + p], theta) ? 1 : 0) << p;
                if (!mask) continue;
            }
#ifdef EWK_TIMING
            dbg[10] += 1;
            dbg[11] += __builtin_popcount(mask);
            if (rec && ((skipped >> cur) & 1)) { dbg[25] += 1; dbg[26] += __builtin_popcount(mask); }
#endif
            fix_tile(v, cur, T, rec ? spec[kSpecRun + cur] : -INFINITY, theta, smem, scr, tile, lane, lo, cref, s1,
                     s2, mask, rec && ((shifted >> cur) & 1));
        }
    }
    if (__ballot(nanp != nanp)) {   // NaN input: NaN statistics, NaN score (like the reference)
#pragma unroll
        for (int i = 0; i < kSlots; ++i) s1[i] = __builtin_nan("");
    }
    EWK_TS(tq4);
    EWK_TADD(5, tq3, tq4);
    finish_stats(T, cref, s1, s2, lane, reinterpret_cast<double*>(scr));
    EWK_TS(tq5);
    EWK_TADD(6, tq4, tq5);
}


// Ring mode (few segments per tick, latency matters): the workgroup's waves share one
// segment -- wave w takes tiles w, w + WAVES, ... -- and meet twice: for the segment's
// log-mel max (top_db threshold) and to combine their shifted sums.  Wave w's sums are
// shifted by its own first column (cref_w); wave 0 re-centres them on cref_0:
//   S1 = sum_w s1_w + n_w d_w,  S2 = sum_w s2_w + 2 d_w s1_w + n_w d_w^2,  d_w = cref_w - cref_0.
// Leaves mean / std (fp32-rounded) in misc0[0..19], misc0[20..39] (wave 0's scratch).
template <int RING>
__device__ void segment_stats_coop(const SegSrc<RING>& v, unsigned char* smem, float* scr, float* tile,
                                   float* spec, int wave, int lane, const int (&lo)[8], float* misc0,
                                   float& theta_out) {
    const float* s_dct = reinterpret_cast<const float*>(smem + L_DCT);
    float* wg_mm = reinterpret_cast<float*>(smem + L_WG + 16);   // [WAVES][2] max, min
    const int T = 1 + v.len / HOP;
    const int ntile = (T + 15) >> 4;
    const int nloc = ntile > wave ? (ntile - wave + WAVES - 1) / WAVES : 0;
    const int col = lane & 15;
    double s1[kSlots], s2[kSlots];
    float cref[kSlots];
#pragma unroll
    for (int i = 0; i < kSlots; ++i) { s1[i] = 0.0; s2[i] = 0.0; cref[i] = 0.0f; }
    float vmax = -INFINITY, vmin = INFINITY, nanp = 0.0f;
    // the wave's last tile stays in LDS (unclamped) until the segment max is known, so a
    // segment of <= WAVES tiles (T <= 128) is never recomputed; earlier tiles are clamped
    // speculatively at the running max (segment_stats) and recomputed if theta bites
    float run = -INFINITY, last_min = INFINITY;
    for (int lt = 0; lt < nloc; ++lt) {
        const int tile_i = wave + WAVES * lt;
        const bool last = lt + 1 == nloc;
        const bool rec = !last && lt < kSpecTiles;
        if (!rec) run = -INFINITY;
        float tmin = INFINITY;
        tile_passes(v, tile_i, T, smem, scr, tile, lane, lo, vmax, tmin, nanp, run);
        const float tmw = wave_min(tmin);
        vmin = fminf(vmin, tmw);
        if (last) { last_min = tmw; break; }
        const float run2 = rec ? wave_max(vmax) - kTopDbUnits : -INFINITY;
        if (run2 > run && tmw < run2) {   // self-clamp (segment_stats)
            uint4 h[4], l[4];
            clamp_load(reinterpret_cast<const float4*>(tile), lane, h, l);
            clamp_store(tile, lane, h, l, run2);
            lds_order();
        }
        run = fmaxf(run, run2);
        float c[kSlots];
        tile_dct(tile, s_dct, lane, c);
        if (lt == 0) {
#pragma unroll
            for (int i = 0; i < kSlots; ++i) cref[i] = __shfl(c[i], lane & 48, 64);
        }
        stats_add(c, cref, tile_i * 16 + col < T, s1, s2);
        if (lane == 0 && rec) {   // tile-granular records (both passes recomputed when theta bites)
#pragma unroll
            for (int p = 0; p < kPassesPerTile; ++p) spec[kPassesPerTile * lt + p] = fmaxf(tmw, run);
            spec[kSpecRun + lt] = run;
        }
    }
    vmax = wave_max(vmax);
    if (lane == 0) { wg_mm[2 * wave] = vmax; wg_mm[2 * wave + 1] = vmin; }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < WAVES; ++w) { vmax = fmaxf(vmax, wg_mm[2 * w]); vmin = fminf(vmin, wg_mm[2 * w + 1]); }
    const float theta = vmax - kTopDbUnits;
    theta_out = theta;
    if (nloc > 0) {
        const int tile_l = wave + WAVES * (nloc - 1);
        if (last_min < theta) {   // the last tile, still in LDS: clamp at the final threshold
            uint4 h[4], l[4];
            clamp_load(reinterpret_cast<const float4*>(tile), lane, h, l);
            clamp_store(tile, lane, h, l, theta);
            lds_order();
        }
        float c[kSlots];
        tile_dct(tile, s_dct, lane, c);
        if (nloc == 1) {
#pragma unroll
            for (int i = 0; i < kSlots; ++i) cref[i] = __shfl(c[i], lane & 48, 64);
        }
        stats_add(c, cref, tile_l * 16 + col < T, s1, s2);
        if (vmin < theta) {
            lds_order();
            for (int lt = 0; lt + 1 < nloc; ++lt) {
                const bool rec = lt < kSpecTiles;
                if (rec && !(spec[kPassesPerTile * lt] < theta)) continue;
                fix_tile(v, wave + WAVES * lt, T, rec ? spec[kSpecRun + lt] : -INFINITY, theta, smem, scr, tile,
                         lane, lo, cref, s1, s2);
            }
        }
    }
    if (__ballot(nanp != nanp)) {   // NaN input (segment_stats): the combined sums go NaN
#pragma unroll
        for (int i = 0; i < kSlots; ++i) s1[i] = __builtin_nan("");
    }
    // this wave's per-coefficient (s1, s2, cref) -> its scratch, as doubles [coef][3]
    double* pd = reinterpret_cast<double*>(scr);
    row_sums_to_pd(cref, s1, s2, lane, pd);
    __syncthreads();
    if (wave == 0) {
        double mean = 0.0, sd = 0.0;
        if (lane < NMFCC) {
            const double* p0 = reinterpret_cast<const double*>(smem + L_SCR);
            const double r0 = p0[3 * lane + 2];
            double S1 = 0.0, S2 = 0.0;
            for (int w = 0; w < WAVES; ++w) {
                int n = 0;   // valid frames of wave w's tiles
                for (int ti = w; ti < ntile; ti += WAVES) n += min(16, T - 16 * ti);
                if (n == 0) continue;
                const double* pw = reinterpret_cast<const double*>(smem + L_SCR + w * SCR_BYTES);
                const double a1 = pw[3 * lane], a2 = pw[3 * lane + 1], d = pw[3 * lane + 2] - r0;
                S1 += a1 + (double)n * d;
                S2 += a2 + 2.0 * d * a1 + (double)n * d * d;
            }
            const double Td = (double)T;
            mean = r0 + S1 / Td;
            double var = (S2 - S1 * S1 / Td) / Td;
            sd = sqrt(var > 0.0 ? var : 0.0);
        }
        lds_order();
        if (lane < NMFCC) { misc0[lane] = (float)mean; misc0[20 + lane] = (float)sd; }
        lds_order();
    }
}

}  // namespace ewk
