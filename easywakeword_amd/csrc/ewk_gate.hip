// ewk_gate.hip -- level-1 gate for many concurrent streams on gfx950.
//
// One wave per stream, streams independent (no cross-wave sync).  Per tick:
//   a1  ring ingest           SoundBuffer._add_sound_to_buffer  wakeword.py:454-470
//   a2  block RMS + pct25     SoundBuffer._adjust_silence_threshold  :472-486
//   a3  last-0.1 s RMS test   SoundBuffer.is_silent / return_last_n_seconds  :488-513
//   a4  timing FSM            WakeWord._detect_word  :1048-1098
//   a5  segment cut + queue   WakeWord._detect_word  :1100-1118
// All comparisons are float64 and bit-identical to the reference's numpy
// arithmetic: squares of float32 samples are exact in float64, sums follow
// numpy's pairwise order (chunks of 8192, 8-accumulator leaves of <= 128,
// split at n2 = n/2 - (n/2)%8; the tree is flattened once on the host and
// evaluated level by level across the wave), the percentile follows numpy
// 2.2's "linear" method (_compute_virtual_index / _lerp), and the clock is
// tick * tick_seconds.
//
// Incremental state per stream (the reference recomputes everything per tick):
//   * block_rms[b]: RMS of physical block b, refreshed only for the blocks the
//     tick's samples overlap (the other blocks hold the same samples, hence the
//     same value);
//   * sorted_rms: the same multiset kept sorted (one remove + one insert per
//     refreshed block, wave-parallel), so np.percentile(all_rms, 25) is a lookup
//     of the two order statistics it interpolates;
//   * the tick's samples are staged in LDS, so the refreshed block and the last
//     0.1 s window are summed without re-reading the ring; when the window is the
//     refreshed block (aligned ticks, n_last == block) its sum is reused.
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>

#include "ewk_gate.h"

// float64 parity with numpy requires un-fused multiply/add (e.g. the percentile lerp)
#pragma clang fp contract(off)

#include "ewk_gate_pwsum.h"
#include "ewk_gate_rms.h"
#include "ewk_gate_detect.h"

namespace ewk {

int gate_stage_len(int block, int64_t n_last) {
    const int64_t m = std::max<int64_t>(block, n_last);
    if (m > 4096) return 0;              // long callbacks: sum straight from the ring
    return (int)((m + 3) & ~3);
}

// Ring samples are written once per tick and read back only for the few cut segments:
// non-temporal stores keep them from filling the L2 with dirty lines that every launch
// end must write back before the scorer can start.
typedef float f32x4_nt __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void nt_store4(float* p, float4 v) {
    f32x4_nt x = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(x, reinterpret_cast<f32x4_nt*>(p));
}

// the register allocator must allow 4 waves per SIMD (121 VGPRs; 5 spill and run 37 % slower)
#ifndef EWK_GATE_WPE
#define EWK_GATE_WPE 4
#endif
constexpr int kGateWavesPerEU = EWK_GATE_WPE;
// workgroups of 4 waves, one stream per wave up to 524,288 streams, more loop inside the waves.
// (Round 1 capped the grid at one resident wave per slot, 1,024 workgroups, so each wave ran
// its streams in sequence behind the previous stream's final stores; letting the hardware
// refill freed slots with new waves instead took the tick from 11.6 to 9.2 ms at 2 M streams,
// 0.75 to 0.65 ms at 131,072 and 77 to 72 us at 8,192.)
#ifndef EWK_GATE_GRID_MAX
#define EWK_GATE_GRID_MAX 131072
#endif
constexpr int kGateGridMax = EWK_GATE_GRID_MAX;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
constexpr int kIngestLoads = 4;    // tick samples per lane loaded ahead of the ring stores (16: 166 VGPRs, 3 waves/SIMD, 10 % slower)

// RB > 0: the stream's block RMS array and its sorted copy live in registers for the
// whole launch (RB slots per lane, n_blocks <= 64 * RB): loaded once, updated with
// wave shuffles, stored once -- no dependent global round trips per tick.  RB = 0:
// both stay in global memory (any n_blocks).
// PROF (detector profiles): the stream's seven gate timings come from its profile; without it
// they are the launch's (GateArgs) and the kernel holds no profile code.
// LSN (stream listeners, with PROF): lane j, 1 <= j < the stream's listener count, carries
// listener j's _detect_word state in its own registers for the whole launch and steps it after
// listener 0 at every tick, from the tick's wave-uniform is_silent and clock (lsn_step).
template <int RB, int DMA, bool PROF = false, bool LSN = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kGateWavesPerEU, 8))) void k_gate_ticks(GateArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const PwTree* __restrict__ trees = g.trees;   // read-only, cache-resident
    // persistent over streams: wave w takes streams w, w + waves-in-grid, ...; the next
    // stream's first tick is requested (LDS-DMA) as soon as this stream's last tick has
    // issued its stage reads, so its HBM latency overlaps this stream's FSM and stores
    // (readfirstlane: the compiler then knows the stream, hence its state, is wave-uniform --
    // scalar loads into SGPRs instead of a copy of GateStream in every lane's VGPRs)
    // r: the wave's row of the launch (where its samples come from); s: the stream that row
    // feeds (g.ids, subset pushes), which addresses everything else.  Both wave-uniform.
    int r = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + wave);
    const int32_t* __restrict__ ids = g.ids;
    const int wstride = (int)gridDim.x * 4;
    constexpr int kStageEs = DMA == 3 ? 2 : 4;   // int16 stage for the vector int16 path
    const GateLds lds(g.val_len, g.stage, kStageEs, LSN);
    // The trees of the block and last-window sums (lengths < one 8192 chunk) in LDS: every tree
    // level reads its node indices, and from L1/L2 those dependent loads set the block sum's
    // time (~4 us of a ~14 us stream-tick).  (The full-chunk trees, for callbacks > 8192
    // samples, stay in global memory.)
    PwTree* ltree = reinterpret_cast<PwTree*>(smem + lds.trees);
    {
        static_assert(sizeof(PwTree) % 16 == 0, "trees are copied in 16-B pieces");
        constexpr int kPieces = (int)(sizeof(PwTree) / 16);
        const uint4* src0 = reinterpret_cast<const uint4*>(trees + kTreeBlockRem);
        const uint4* src1 = reinterpret_cast<const uint4*>(trees + kTreeLastRem);
        uint4* dst = reinterpret_cast<uint4*>(ltree);
        for (int i = threadIdx.x; i < 2 * kPieces; i += blockDim.x) dst[i] = i < kPieces ? src0[i] : src1[i - kPieces];
        __syncthreads();
    }
    if (r >= g.n_streams) return;
    int s = ids ? __builtin_amdgcn_readfirstlane(ids[r]) : r;
    unsigned char* w = smem + wave * lds.per_wave;
    double* val = reinterpret_cast<double*>(w);
    float* stage = reinterpret_cast<float*>(w + lds.stage);
    int16_t* stage16 = reinterpret_cast<int16_t*>(stage);   // (DMA 3)
    // the staged samples [c0, ...) as a summation source
    auto stage_src = [&](int c0) {
        if constexpr (DMA == 3) return LdsSrc16{stage16 + c0};
        else return LdsSrc{stage + c0};
    };

    const int R = (int)g.ring_len;        // the reference ring: block grid, pointer, fill level
    const int Rs = (int)g.sring_len;      // samples stored per stream (== R unless compact)
    const int fs = g.block;
    const int nb = g.n_blocks;
    const int nl = (int)min<int64_t>(g.n_last, g.ring_len);
    // the first tick's samples are requested before the state: no load waits on another
    float xin[kIngestLoads];
    auto load_chunk = [&](int t, int c0) {
        const int64_t so = (int64_t)r * g.stride + (int64_t)t * g.tick_stride;
#pragma unroll
        for (int m = 0; m < kIngestLoads; ++m) {
            const int i = c0 + lane + 64 * m;
            xin[m] = i < fs ? (g.pcm16 ? (float)__builtin_nontemporal_load(g.pcm16 + so + i) * (1.0f / 32768.0f)
                                       : __builtin_nontemporal_load(g.pcm + so + i)) : 0.0f;
        }
    };
    // DMA == 3 (int16 input, block % 8 == 0, 16-B aligned rows): the tick's samples in 16-B
    // pieces (8 per lane), all in flight at once, widened in registers -- one global round
    // trip per tick like the float32 LDS-DMA path (the 4-sample chunks above take seven)
    u32x4 raw[kPcm16Pieces];
    auto load_vec = [&](int ss, int t) {
        const int16_t* src = g.pcm16 + (int64_t)ss * g.stride + (int64_t)t * g.tick_stride;
        const int ln = lane_here(lane);
#pragma unroll
        for (int c = 0; c < kPcm16Pieces; ++c) {
            const int i0 = 8 * (ln + 64 * c);
            raw[c] = i0 < fs ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src + i0)) : u32x4{0, 0, 0, 0};
        }
    };
    // float32 input with the tick staged in LDS: the tick's samples go global -> LDS by
    // LDS-DMA (global_load_lds), all in flight at once with no VGPRs -- one global round
    // trip per tick instead of one per register chunk
    const bool staged = g.stage >= fs && g.stage >= nl;
    constexpr bool dma = DMA == 1 || DMA == 2;   // launch_gate: float32 input, tick and window fit the stage
    auto dma_tick = [&](int ss, int t) {
        const float* src = g.pcm + (int64_t)ss * g.stride + (int64_t)t * g.tick_stride;
        if (DMA == 2) {   // 16-B pieces (1 KiB per wave-instruction): tick rows 16-B aligned, block % 4 == 0
            for (int c0 = 0; c0 < fs; c0 += 256) {
                if (c0 + 4 * lane < fs)
                    __builtin_amdgcn_global_load_lds(src + c0 + 4 * lane,
                                                     (__attribute__((address_space(3))) void*)(stage + c0), 16, 0, 0);
            }
            return;
        }
        for (int c0 = 0; c0 < fs; c0 += 64) {
            if (c0 + lane < fs)
                __builtin_amdgcn_global_load_lds(src + c0 + lane, (__attribute__((address_space(3))) void*)(stage + c0),
                                                 4, 0, 0);
        }
    };
    if (dma) dma_tick(r, 0);
    else if (DMA == 3) load_vec(r, 0);
    else load_chunk(0, 0);
    for (;;) {
        float* ring = g.ring ? g.ring + (int64_t)s * Rs : nullptr;
        int16_t* ring16 = g.ring16 ? g.ring16 + (int64_t)s * Rs : nullptr;   // PCM16 pushes only (host-checked)
        GateStream st = g.st[s];
        // The stream's detector timings.  PROF: the profile is looked up again for every stream of
        // the loop.  s is wave-uniform (readfirstlane) and both arrays are read through the constant
        // address space -- no kernel writes the table, and the index array only between gate launches
        // (k_scatter_i32) -- so the index and the doubles behind it are s_load instructions into
        // SGPRs.  Index -1 (pf null): the engine's configuration, from the launch arguments.  The
        // re-entry timeout is tested at every tick and kept in registers; the other six are read
        // where the FSM uses them (a state transition, the cut), so they hold no registers across
        // the tick's sums.
        typedef const ewk_detector_profile __attribute__((address_space(4))) * ProfilePtr;
        typedef const int32_t __attribute__((address_space(4))) * IndexPtr;
        ProfilePtr pf = nullptr;
        double reentry_timeout = g.reentry_timeout;
        if constexpr (PROF) {
            const int pi = __builtin_amdgcn_readfirstlane(((IndexPtr)g.stream_profile)[s]);
            if (pi >= 0) {
                pf = (ProfilePtr)g.profiles + pi;
                reentry_timeout = pf->reentry_timeout;
            }
        }
#define EWK_GATE_TIMING(field) ((PROF && pf) ? pf->field : g.field)
        // LSN: the count and the lane's profile index once per stream of the loop, then the lane's
        // 40-byte record (LsnLane: its times go to the lane's LDS words)
        bool lsn_on = false;
        LsnLane ls = {};
        if constexpr (LSN) {
            const int cnt = min(__builtin_amdgcn_readfirstlane(g.lsn_count[s]), (int)EWK_LISTENERS_MAX);
            lsn_on = lane >= 1 && lane < cnt;
            // (lds.lsn, formed from the trees' address as it always was: the kernels' address arithmetic stays)
            ls.base = (LdsTimes)reinterpret_cast<double*>(reinterpret_cast<unsigned char*>(ltree + 2) + wave * kLsnWaveLds);
            ls.lane = lane;
            ls.pi = -1;
            if (lsn_on) {
                ls.pi = g.lsn_tab[(int64_t)s * EWK_LISTENERS_MAX + lane].profile;
                const LsnState in = g.lsn_st[(int64_t)s * kLsnStates + lane - 1];
                ls.silence_start() = in.silence_start;
                ls.sound_start() = in.sound_start;
                ls.sound_end() = in.sound_end;
                ls.start_time() = in.start_time;
                ls.sr = (in.reentries << 2) | (in.state & 3);
                ls.timeout = (ls.pi >= 0 ? g.profiles[ls.pi].reentry_timeout : g.reentry_timeout) > 0.0;
            }
        }
        const int64_t tick0 = g.own_clock ? st.tick : g.tick0;   // the stream's own clock, or the engine's (equal in lockstep)
        double* grms = g.block_rms + (int64_t)s * nb;
        double* sorted2 = g.sorted_rms + (int64_t)s * 2 * nb;
        const PwTree* tbf = trees + kTreeBlockFull;
        const PwTree* tbr = ltree;
        const PwTree* tlf = trees + kTreeLastFull;
        const PwTree* tlr = ltree + 1;
        constexpr int RBn = RB > 0 ? RB : 1;
        double gr[RBn], srt[RBn];
        uint32_t dirty = 0;   // register path: bit j = gr[j] changed, bit RB + j = srt[j] changed (stored back only then)
        if (RB > 0) {   // (this path never double-buffers: sorted_sel stays 0)
#pragma unroll
            for (int j = 0; j < RBn; ++j) {
                const int i = lane + 64 * j;
                gr[j] = i < nb ? grms[i] : 0.0;
                srt[j] = i < nb ? sorted2[i] : 0.0;
            }
        }

        for (int t = 0; t < g.n_ticks; ++t) {
            const int64_t tick = tick0 + t + 1;                      // tick being delivered
            const double t_prev = (double)(tick - 1) * g.tick_seconds;
            // start()-mode re-entry (TimeoutError -> _detect_word again), before the sleep
            if (st.started && reentry_timeout > 0.0 && t_prev - st.start_time > reentry_timeout) {
                st.state = kWaiting;
                st.start_time = t_prev;
                if (st.last_silent) { st.state = kInSilence; st.silence_start = t_prev; }
                st.reentries += 1;
            }
            if constexpr (LSN) {   // the same test per listener, on its own start_time and timeout
                if (lsn_on && ls.timeout && st.started &&
                    t_prev - ls.start_time() > (ls.pi >= 0 ? g.profiles[ls.pi].reentry_timeout : g.reentry_timeout)) {
                    ls.set_state(kWaiting);
                    ls.start_time() = t_prev;
                    if (st.last_silent) { ls.set_state(kInSilence); ls.silence_start() = t_prev; }
                    ls.sr += 4;   // (reentries += 1)
                }
            }
            // ---- a1: ingest `fs` samples at the write pointer (and stage them in LDS)
            const int p0 = st.pointer;
            const int sp0 = st.spos;    // == p0 for the full ring
            // chunks of kIngestLoads loads per lane in flight before any store (the ring may
            // alias the input as far as the compiler knows: a load-store loop serialises them);
            // chunk 0 of this tick was requested before the previous tick's compute
            if (DMA == 2) {   // 16-B ring stores from the stage (ring rows and p0 4-float aligned: no group wraps)
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                wave_sync();
#pragma unroll
                for (int h = 0; h < kDma4Chunks; h += 4) {   // batches of 4 (16 VGPRs)
                    float4 xv[4];
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int i = 256 * (h + c) + 4 * lane;
                        xv[c] = i < fs ? *reinterpret_cast<const float4*>(stage + i) : make_float4(0.f, 0.f, 0.f, 0.f);
                    }
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int i = 256 * (h + c) + 4 * lane;
                        if (i < fs) {
                            int k = sp0 + i;
                            if (k >= Rs) k -= Rs;
                            nt_store4(ring + k, xv[c]);
                        }
                    }
                    if (256 * (h + 4) >= fs) break;
                }
            } else if (dma) {   // this tick's samples landed in the stage: ring stores from LDS
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                wave_sync();
                for (int c0 = 0; c0 < fs; c0 += 64 * kIngestLoads) {
#pragma unroll
                    for (int m = 0; m < kIngestLoads; ++m) {
                        const int i = c0 + lane + 64 * m;
                        xin[m] = i < fs ? stage[i] : 0.0f;
                    }
#pragma unroll
                    for (int m = 0; m < kIngestLoads; ++m) {
                        const int i = c0 + lane + 64 * m;
                        if (i < fs) {   // (float32 input: never an int16 ring)
                            int k = sp0 + i;
                            if (k >= Rs) k -= Rs;
                            ring[k] = xin[m];
                        }
                    }
                }
            }
            if (DMA == 3) {   // int16 pieces: ring (int16 as delivered, or widened) and stage stores
                const int ln = lane_here(lane);
#pragma unroll
                for (int c = 0; c < kPcm16Pieces; ++c) {
                    const int i0 = 8 * (ln + 64 * c);
                    if (i0 < fs) {
                        int k = sp0 + i0;   // 8-sample groups never straddle the wrap (Rs % 8 == 0)
                        if (k >= Rs) k -= Rs;
                        const u32x4 w = raw[c];
                        float v[8];
#pragma unroll
                        for (int h = 0; h < 4; ++h) {
                            v[2 * h] = (float)(short)(w[h] & 0xffffu) * (1.0f / 32768.0f);
                            v[2 * h + 1] = (float)((int)w[h] >> 16) * (1.0f / 32768.0f);
                        }
                        if (ring16) {
                            __builtin_nontemporal_store(w, reinterpret_cast<u32x4*>(ring16 + k));
                        } else {
                            nt_store4(ring + k, make_float4(v[0], v[1], v[2], v[3]));
                            nt_store4(ring + k + 4, make_float4(v[4], v[5], v[6], v[7]));
                        }
                        if (staged) *reinterpret_cast<u32x4*>(stage16 + i0) = w;   // the int16 samples as delivered
                    }
                }
                if (t + 1 < g.n_ticks) load_vec(r, t + 1);   // next tick's samples, in flight during this tick
            }
            for (int c0 = 0; c0 < ((dma || DMA == 3) ? 0 : fs); c0 += 64 * kIngestLoads) {
                if (c0 > 0) load_chunk(t, c0);
#pragma unroll
                for (int m = 0; m < kIngestLoads; ++m) {
                    const int i = c0 + lane + 64 * m;
                    if (i < fs) {
                        int k = sp0 + i;
                        if (k >= Rs) k -= Rs;
                        if (ring16) ring16[k] = (int16_t)(xin[m] * 32768.0f);   // the PCM16 value, exactly
                        else ring[k] = xin[m];
                        if (staged) stage[i] = xin[m];
                    }
                }
            }
            if (t + 1 < g.n_ticks && !dma && DMA != 3) load_chunk(t + 1, 0);   // next tick's samples, in flight during this tick
            __threadfence_block();
            wave_sync();
            const bool wrapped = p0 + fs > R;
            st.pointer = (int32_t)((p0 + fs) % R);
            st.spos = (int32_t)((sp0 + fs) % Rs);
            st.collected = min(st.collected + (int64_t)fs, (int64_t)R);
            const bool full = st.collected >= R;
            // block sum of the window when it coincides with a refreshed block
            double reuse_sum = 0.0;
            bool have_reuse = false;
            // ---- a2: threshold over the physical blocks (only once the ring is full)
            if (full) {
                auto block_sum = [&](int b) -> double {
                    const int a0 = b * fs;
                    if (staged && a0 == p0)   // the block is exactly this tick's samples
                        return pw_sumsq(stage_src, fs, tbf, tbr, lane, val);
                    // reference-ring position a0 + c0 lives at sample-ring position sp0 + (a0 + c0 - p0)
                    // (the identity for the full ring; compact rings only reach this path for
                    // blocks written within the last Rs samples)
                    return pw_sumsq([&](int c0) {
                        int k = (sp0 + (a0 + c0 - p0)) % Rs;
                        if (k < 0) k += Rs;
                        return RingSrc{ring, ring16, k, Rs};
                    }, fs, tbf, tbr, lane, val);
                };
                if (!st.filled && g.compact) {
                    // compact ring: every block RMS was kept as its samples arrived (the blocks
                    // are whole ticks); the last one is this tick's, then the first sort
                    const int b = p0 / fs;
                    const double v = sqrt(block_sum(b) / (double)fs);
                    if (RB > 0) reg_set(gr, b, v, lane, dirty);
                    else if (lane == 0) grms[b] = v;
                    __threadfence_block();
                    wave_sync();
                    if (RB > 0) reg_rank_sort(gr, srt, nb, val, lane, dirty);
                    else rank_sort(grms, sorted2, nb, lane);
                    st.sorted_sel = 0;
                    st.filled = 1;
                } else if (!st.filled) {   // (the same tail, written twice: with one, every kernel's instructions move)
                    for (int b = 0; b < nb; ++b) {
                        const double sum = block_sum(b);
                        if (RB > 0) reg_set(gr, b, sqrt(sum / (double)fs), lane, dirty);
                        else if (lane == 0) grms[b] = sqrt(sum / (double)fs);
                    }
                    __threadfence_block();
                    wave_sync();
                    if (RB > 0) reg_rank_sort(gr, srt, nb, val, lane, dirty);
                    else rank_sort(grms, sorted2, nb, lane);
                    st.sorted_sel = 0;
                    st.filled = 1;
                } else {
                    // refresh the physical blocks overlapping the written range [p0, p0+fs) (mod R)
                    auto refresh = [&](int a0, int a1) {   // [a0, a1) inside [0, R)
                        const int b0 = a0 / fs;
                        const int b1 = (a1 - 1) / fs;
                        for (int b = b0; b <= b1 && b < nb; ++b) {
                            const double sum = block_sum(b);
                            const double v = sqrt(sum / (double)fs);
                            if (nl == fs && b * fs + fs == (int)st.pointer + (st.pointer == 0 ? R : 0)) {
                                reuse_sum = sum;
                                have_reuse = true;
                            }
                            if (RB > 0) {
                                const double vo = reg_get(gr, b);
                                reg_set(gr, b, v, lane, dirty);
                                if (!reg_replace(srt, nb, vo, v, lane, dirty)) reg_rank_sort(gr, srt, nb, val, lane, dirty);
                                continue;
                            }
                            const double vo = grms[b];
                            if (lane == 0) grms[b] = v;
                            const double* cur = sorted2 + (int64_t)st.sorted_sel * nb;
                            double* nxt = sorted2 + (int64_t)(st.sorted_sel ^ 1) * nb;
                            __threadfence_block();
                            wave_sync();
                            if (!sorted_replace(cur, nxt, nb, vo, v, lane)) {
                                __threadfence_block();
                                wave_sync();
                                rank_sort(grms, nxt, nb, lane);
                            }
                            st.sorted_sel ^= 1;
                            __threadfence_block();
                            wave_sync();
                        }
                    };
                    if (!wrapped) refresh(p0, p0 + fs);
                    else { refresh(p0, R); refresh(0, p0 + fs - R); }
                }
                double p25;
                if (RB > 0) {
                    p25 = percentile25([&](int i) { return reg_get(srt, i); }, nb);
                } else {
                    __threadfence_block();
                    wave_sync();
                    const double* cur = sorted2 + (int64_t)st.sorted_sel * nb;
                    p25 = percentile25([&](int i) { return cur[i]; }, nb);
                }
                const double thr = p25 * 1.5;
                // Python max(new, MIN): MIN only if MIN > new
                st.threshold = (g.min_threshold > thr) ? g.min_threshold : thr;
            } else if (g.compact) {
                // filling a compact ring: keep this block's RMS now (its samples will not all
                // be in the sample ring when the reference ring first fills)
                const int b = p0 / fs;
                const double v = sqrt(pw_sumsq(stage_src, fs, tbf, tbr, lane, val) /
                                      (double)fs);
                if (RB > 0) reg_set(gr, b, v, lane, dirty);
                else if (lane == 0) grms[b] = v;
            }
            // ---- a3: is_silent(): RMS of the last n_last samples < threshold
            bool silent = true;
            if (nl > 0) {
                double sum;
                if (have_reuse) {
                    sum = reuse_sum;
                } else if (staged && nl <= fs) {   // the window lies in this tick's samples
                    sum = pw_sumsq([&](int c0) { return stage_src(fs - nl + c0); }, nl, tlf, tlr, lane, val);
                } else {
                    int first = st.spos - nl;
                    if (first < 0) first += Rs;
                    sum = pw_sumsq([&](int c0) {
                        int f = first + c0;
                        if (f >= Rs) f -= Rs;
                        return RingSrc{ring, ring16, f, Rs};
                    }, nl, tlf, tlr, lane, val);
                }
                const double rms = sqrt(sum / (double)nl);
                st.last_rms = rms;
                silent = rms < st.threshold;
            }
            if (dma && t + 1 < g.n_ticks) {   // the stage's last reader (a3) has issued its reads
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                dma_tick(r, t + 1);
            } else if (dma && r + wstride < g.n_streams) {   // last tick: the next row's first
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                dma_tick(r + wstride, 0);
            }
            st.last_silent = silent;
            st.tick = tick;
            const double now = (double)tick * g.tick_seconds;
            // ---- a4/a5: detector
            if (!st.started) {
                if (full) {   // _wait_for_buffer returned: _detect_word entry check
                    st.started = 1;
                    st.state = kWaiting;
                    st.start_time = now;
                    if (silent) { st.state = kInSilence; st.silence_start = now; }
                    if constexpr (LSN) {   // every listener enters at the tick the ring fills
                        if (lsn_on) {
                            ls.set_state(kWaiting);
                            ls.start_time() = now;
                            if (silent) { ls.set_state(kInSilence); ls.silence_start() = now; }
                        }
                    }
                }
                continue;
            }
            {   // wave-uniform FSM (every lane holds the same state): no divergent branch, no broadcast
                switch (st.state) {
                case kWaiting:
                    if (silent) { st.state = kInSilence; st.silence_start = now; }
                    break;
                case kInSilence:
                    if (!silent) {
                        if (now - st.silence_start >= EWK_GATE_TIMING(pre_speech_silence)) { st.state = kInSound; st.sound_start = now; }
                        else st.state = kWaiting;
                    }
                    break;
                case kInSound: {
                    const double d = now - st.sound_start;
                    if (!silent) {
                        if (d > EWK_GATE_TIMING(speech_duration_max)) st.state = kWaiting;
                    } else {
                        if (EWK_GATE_TIMING(speech_duration_min) <= d && d <= EWK_GATE_TIMING(speech_duration_max)) {
                            st.state = kAfterSound;
                            st.sound_end = now;
                        } else st.state = kWaiting;
                    }
                    break;
                }
                case kAfterSound:
                    if (silent) {
                        if (now - st.sound_end >= EWK_GATE_TIMING(post_speech_silence)) {
                            const double xs = st.sound_start - now - EWK_GATE_TIMING(padding);
                            const double xe = st.sound_end - now + EWK_GATE_TIMING(padding);
                            int64_t nreq = (int64_t)(fabs(xs) * (double)g.sample_rate);
                            if (nreq > R) nreq = R;
                            const int64_t e = (int64_t)(fabs(xe) * (double)g.sample_rate);
                            int64_t stop = nreq - e;   // python a[:len-e]
                            if (stop < 0) { stop += nreq; if (stop < 0) stop = 0; }
                            if (stop > nreq) stop = nreq;
                            // (the host sizes a compact ring for the longest possible request)
                            int64_t start = (int64_t)st.spos - nreq;
                            if (start < 0) start += Rs;
                            ewk_event ev;
                            ev.stream = s;
                            ev.length = (int32_t)stop;
                            ev.tick = tick;
                            ev.ring_start = start;
                            ev.time = now;
                            ev.score = __builtin_nan("");
                            ev.match = 0;
                            ev.flags = ((double)stop / (double)g.sample_rate > EWK_GATE_TIMING(max_segment_seconds)) ? EWK_EV_SKIPPED : 0;
                            if (lane == 0) {
                                const uint32_t slot = (uint32_t)atomicAdd(g.ev_count, 1) - (uint32_t)g.ev_base0;
                                if (slot < (uint32_t)g.ev_cap) g.events[slot] = ev;
                                else atomicAdd(g.ev_dropped, 1);
                            }
                            st.state = kWaiting;
                        }
                    } else st.state = kWaiting;
                    break;
                }
            }
            if constexpr (LSN) {
                if (lsn_on) lsn_step(ls, g, silent, now, s, lane, tick, st.spos, R, Rs);
            }
        }
        if (RB > 0 && (st.filled || g.compact)) {   // only the elements this launch changed (one block RMS per tick)
#pragma unroll
            for (int j = 0; j < RBn; ++j) {
                const int i = lane + 64 * j;
                if (i < nb && (dirty & (1u << j))) grms[i] = gr[j];
                if (i < nb && (dirty & (1u << (RB + j)))) sorted2[i] = srt[j];
            }
        }
        if (lane == 0) g.st[s] = st;
        if constexpr (LSN) {
            if (lsn_on) {
                LsnState out;
                out.silence_start = ls.silence_start();
                out.sound_start = ls.sound_start();
                out.sound_end = ls.sound_end();
                out.start_time = ls.start_time();
                out.state = ls.state();
                out.reentries = ls.sr >> 2;
                g.lsn_st[(int64_t)s * kLsnStates + lane - 1] = out;
            }
        }
        r += wstride;
        if (r >= g.n_streams) break;
        s = ids ? __builtin_amdgcn_readfirstlane(ids[r]) : r;
        if (DMA == 3) load_vec(r, 0);
        else if (!dma) load_chunk(0, 0);
    }
#undef EWK_GATE_TIMING
}

}  // namespace ewk

#include "ewk_gate_lifecycle.h"

namespace ewk {

int gate_val_len(const PwTree* trees_host, int n_blocks) {
    int m = 0;
    for (int k = 0; k < kNumTrees; ++k) m = std::max(m, 10 * trees_host[k].n_leaves);
    if (n_blocks <= 64 * kGateRegMax) m = std::max(m, n_blocks);   // register path's rank-sort scratch
    return std::max(2, (m + 1) & ~1);
}

// The instantiations of one (PROF, LSN) pair: RB 2 and kGateRegMax with every DMA, and <0, 0>.
template <bool PROF, bool LSN>
static void launch_gate_family(const GateFamily& f, int grid, size_t lds, hipStream_t s, const GateArgs& g) {
#define EWK_GATE_LAUNCH(RB, DMA) hipLaunchKernelGGL((k_gate_ticks<RB, DMA, PROF, LSN>), dim3(grid), dim3(256), lds, s, g)
    if (f.rb == 2) {
        if (f.dma == 2) EWK_GATE_LAUNCH(2, 2);
        else if (f.dma == 3) EWK_GATE_LAUNCH(2, 3);
        else if (f.dma == 1) EWK_GATE_LAUNCH(2, 1);
        else EWK_GATE_LAUNCH(2, 0);
    } else if (f.rb == kGateRegMax) {
        if (f.dma == 2) EWK_GATE_LAUNCH(kGateRegMax, 2);
        else if (f.dma == 3) EWK_GATE_LAUNCH(kGateRegMax, 3);
        else if (f.dma == 1) EWK_GATE_LAUNCH(kGateRegMax, 1);
        else EWK_GATE_LAUNCH(kGateRegMax, 0);
    } else {
        EWK_GATE_LAUNCH(0, 0);
    }
#undef EWK_GATE_LAUNCH
}

hipError_t launch_gate(const GateArgs& g, hipStream_t s, int grid_cap) {
    if (g.n_streams <= 0 || g.n_ticks <= 0) return hipSuccess;
    // one wave per stream (the hardware refills freed slots), up to kGateGridMax workgroups
    const int grid = std::min((g.n_streams + 3) / 4, grid_cap > 0 ? std::min(grid_cap, kGateGridMax) : kGateGridMax);
    const bool lsn = g.lsn_count != nullptr;
    if (lsn ? (!g.lsn_tab || !g.lsn_st || !g.stream_profile) : (g.profiles == nullptr) != (g.stream_profile == nullptr))
        return hipErrorInvalidValue;
    const GateFamily f = gate_family(g);
    // the DMA 3 instantiations (and only they) stage int16; every other path float
    const size_t lds = GateLds(g.val_len, g.stage, f.dma == 3 ? 2 : 4, lsn).total;
    if (f.lsn) launch_gate_family<true, true>(f, grid, lds, s, g);     // the per-stream timings and the listener lanes
    else if (f.prof) launch_gate_family<true, false>(f, grid, lds, s, g);   // the per-stream timings
    else launch_gate_family<false, false>(f, grid, lds, s, g);
    return hipGetLastError();
}

}  // namespace ewk

