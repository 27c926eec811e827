// ewk_gate.h -- level-1 gate state and launch interface (internal).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ewk.h"
#include "ewk_gate_tree.h"

namespace ewk {

enum { kWaiting = 0, kInSilence = 1, kInSound = 2, kAfterSound = 3 };

// Per-stream state: SoundBuffer fields (wakeword.py:426-433) + _detect_word
// locals (wakeword.py:1048-1052), all float64 times on the virtual clock.
struct GateStream {
    int64_t collected;       // samples_collected (saturates at ring length)
    int64_t tick;            // last tick delivered
    double threshold;        // silence_threshold
    double last_rms;         // RMS of the last 0.1 s at the last tick
    double silence_start;
    double sound_start;
    double sound_end;
    double start_time;       // _detect_word start_time (re-entry timeout)
    int32_t pointer;
    int32_t state;
    int32_t started;
    int32_t last_silent;
    int32_t filled;          // block RMS cache + sorted copy valid
    int32_t reentries;
    int32_t sorted_sel;      // which of the two sorted_rms halves is current
    int32_t spos;            // write position in the sample ring (== pointer when it is the full ring)
};

// Stream listeners (ewk_stream_listeners_set): the _detect_word locals of listener j >= 1 of a
// stream (listener 0's are GateStream's); everything else of GateStream is shared.  40 bytes,
// lsn_st[s * kLsnStates + j - 1].
struct LsnState {
    double silence_start;
    double sound_start;
    double sound_end;
    double start_time;
    int32_t state;
    int32_t reentries;
};
constexpr int kLsnStates = EWK_LISTENERS_MAX - 1;

struct GateArgs {
    const float* pcm;        // stream s, tick t: pcm[s*stride + t*tick_stride + i]
    const int16_t* pcm16;    // or int16 PCM (same indexing), decoded as x / 32768 (exact)
    int64_t stride;
    int64_t tick_stride;
    int32_t n_ticks;
    int32_t n_streams;
    int64_t tick0;           // ticks already delivered
    float* ring;             // [n_streams][sring_len] sample rings (float32) ...
    int16_t* ring16;         // ... or int16 (EWK_RING_I16: PCM16 pushes stored as delivered)
    int64_t ring_len;        // the reference ring (buffer_seconds * sample_rate): blocks, pointer, fill
    int64_t sring_len;       // samples stored per stream (== ring_len, or a compact ring: see ewk_config.ring_samples)
    int32_t compact;         // sring_len < ring_len (block-aligned; block RMSs kept from the first write)
    int32_t pad0;
    double* block_rms;       // [n_streams][n_blocks] RMS of each physical block
    double* sorted_rms;      // [n_streams][2][n_blocks] the same values, ascending (double-buffered)
    GateStream* st;
    const PwTree* trees;     // kNumTrees
    int32_t block;           // callback frame_size
    int32_t n_blocks;        // ring_len // block
    int64_t n_last;          // int(0.1 * sample_rate)
    int32_t sample_rate;
    int32_t stage;           // per-wave LDS sample staging (floats); 0 = read the ring directly
    int32_t val_len;         // per-wave LDS doubles: tree node values (and the register path's sort scratch)
    double tick_seconds;
    double pre_speech_silence, speech_duration_min, speech_duration_max, post_speech_silence;
    double padding, max_segment_seconds, reentry_timeout, min_threshold;
    ewk_event* events;
    int32_t* ev_count;
    int32_t* ev_dropped;
    int32_t ev_cap;
    int32_t ev_base0;         // the bank's epoch base: event slot = count - ev_base0 (wrapping)
    // Subset pushes (ewk_push_streams): row r of pcm is stream ids[r], n_streams counts the rows;
    // nullptr: row r is stream r.  Everything but the samples' source is addressed by the stream.
    const int32_t* ids;
    int32_t own_clock;        // 1: every stream counts from its own GateStream::tick (tick0 unused)
    int32_t pad1;
    // Detector profiles (ewk_detector_profiles_set): stream s is gated with the seven timings of
    // profiles[stream_profile[s]], or with the ones above when the index is -1.  Both nullptr
    // without a table: launch_gate then picks the instantiations without the profile code.
    const ewk_detector_profile* profiles;
    const int32_t* stream_profile;   // [n_streams of the engine], by stream (not by row)
    // Stream listeners: stream s has lsn_count[s] listeners, listener j >= 1 gated with profile
    // lsn_tab[s * EWK_LISTENERS_MAX + j].profile (-1: the timings above) from state
    // lsn_st[s * kLsnStates + j - 1], on lane j.  All nullptr while no stream has more than one
    // listener: launch_gate then picks the instantiations without the listener code.  With them
    // stream_profile is set (listener 0's index), profiles only when a table exists.
    const int32_t* lsn_count;
    const ewk_listener* lsn_tab;
    LsnState* lsn_st;
};

// The dynamic LDS of k_gate_ticks, as byte offsets: four wave areas (one per wave: the tree node
// values / sort scratch, then the stage at `stage`, both rounded to 16 B; `per_wave` each), the
// two sub-chunk trees at `trees`, and with listeners the lanes' times at `lsn` (kLsnWaveLds per
// wave).  stage_es: bytes per staged sample (2 in the DMA 3 instantiations, which stage int16).
constexpr size_t kLsnWaveLds = 4 * EWK_LISTENERS_MAX * sizeof(double);
struct GateLds {
    size_t stage, per_wave, trees, lsn, total;
    __host__ __device__ GateLds(int32_t val_len, int32_t stage_len, int stage_es, bool listeners) {
        stage = ((size_t)val_len * 8 + 15) & ~(size_t)15;
        per_wave = stage + (((size_t)stage_len * stage_es + 15) & ~(size_t)15);
        trees = 4 * per_wave;
        lsn = trees + 2 * sizeof(PwTree);
        total = lsn + (listeners ? 4 * kLsnWaveLds : 0);
    }
};

// grid_cap > 0: at most that many workgroups (ewk_create's EWK_GATE_GRID_MAX), below the
// compile-time maximum; a wave then takes more than one row from 4 * grid_cap rows on.
hipError_t launch_gate(const GateArgs& g, hipStream_t s, int grid_cap = 0);

// register-resident block RMS arrays up to 64 * kGateRegMax blocks (10 s ring: block >= 313 samples)
constexpr int kGateRegMax = 8;
constexpr int kDma4Chunks = 8;     // 16-B DMA path: ticks of up to 8 * 256 samples copied to the ring in one batch
constexpr int kPcm16Pieces = 4;    // int16 path: ticks of up to 4 * 512 samples in 16-B pieces

// The k_gate_ticks<RB, DMA, PROF, LSN> instantiation a launch runs, chosen from its arguments alone
// (ewk_gate_launch_info reports the engine's last one).
//   rb:  2 or kGateRegMax block-RMS slots per lane in registers, 0 = the arrays stay in global memory
//   dma: 0 = the tick through registers (sums from the stage when there is one, else from the ring),
//        1 = LDS-DMA in 4-byte pieces, 2 = LDS-DMA in 16-byte pieces, 3 = int16 input in 16-byte
//        pieces with an int16 stage
//   prof / lsn: the per-stream timings / the listener lanes are compiled in
struct GateFamily {
    int32_t rb, dma, prof, lsn;
};
inline GateFamily gate_family(const GateArgs& g) {
    GateFamily f;
    f.lsn = g.lsn_count != nullptr;
    f.prof = f.lsn || g.profiles != nullptr;
    f.rb = g.n_blocks <= 128 ? 2 : g.n_blocks <= 64 * kGateRegMax ? kGateRegMax : 0;
    // float32 input with the tick and the last window in the stage
    const int64_t nl = g.n_last < g.ring_len ? g.n_last : g.ring_len;
    const bool dma = g.pcm16 == nullptr && g.stage >= g.block && g.stage >= nl;
    // 16-B pieces: every tick row 16-B aligned, whole 4-sample groups that never straddle the ring wrap
    const bool dma4 = dma && g.block % 4 == 0 && g.block <= 256 * kDma4Chunks &&
                      g.stride % 4 == 0 && g.tick_stride % 4 == 0 && g.ring_len % 4 == 0 && g.sring_len % 4 == 0 &&
                      ((uintptr_t)g.pcm & 15) == 0;
    // int16 input in 16-B pieces: rows 16-B aligned, whole 8-sample groups
    const bool vec16 = g.pcm16 != nullptr && g.block % 8 == 0 && g.block <= 512 * kPcm16Pieces &&
                       g.stride % 8 == 0 && g.tick_stride % 8 == 0 && g.sring_len % 8 == 0 &&
                       ((uintptr_t)g.pcm16 & 15) == 0;
    f.dma = f.rb == 0 ? 0 : dma4 ? 2 : vec16 ? 3 : dma ? 1 : 0;
    return f;
}
// ewk_reset_stream_list: streams ids[0..n) back to the state ewk_reset_streams gives every stream,
// in one launch: ring row zeroed with k_ring_zero's agent-scope stores, block RMS row zeroed,
// GateStream = init, and with a resampler its history row zeroed and its fresh flag set.
struct ResetListArgs {
    const int32_t* ids;
    int32_t n;
    unsigned char* ring;     // [n_streams][row_bytes]
    int64_t row_bytes;       // sring_len * sample size (any multiple of the sample size)
    double* block_rms;       // [n_streams][n_blocks]
    int32_t n_blocks;
    GateStream* st;
    double init_threshold;   // ewk_config.initial_threshold
    float* hist;            // nullptr or [n_streams][H]
    int32_t H;
    uint8_t* fresh;          // nullptr or [n_streams]
    LsnState* lsn_st;        // nullptr or [n_streams][kLsnStates]: zeroed (the listener table stays)
};
hipError_t launch_reset_list(const ResetListArgs& a, hipStream_t s);
// dst[ids[i]] = vals[i], i < n (ewk_stream_bank_assign)
hipError_t launch_scatter_i32(int32_t* dst, const int32_t* ids, const int32_t* vals, int32_t n, hipStream_t s);
// lsn_count / lsn_st (both nullptr without listeners): every listener of the stream re-enters
hipError_t launch_reenter(GateStream* st, int32_t first, int32_t n, double tick_seconds, const int32_t* lsn_count,
                          LsnState* lsn_st, hipStream_t s);
// ewk_stream_listeners_set: stream ids[i] gets counts[i] listeners rows[i * EWK_LISTENERS_MAX + j];
// listener 0's entry also goes to stream_profile / stream_word (where not nullptr), a listener at
// or past the stream's old count starts as k_reenter starts listener 0, a dropped one is zeroed.
struct ListenerSetArgs {
    const int32_t* ids;
    const int32_t* counts;
    const ewk_listener* rows;
    int32_t n;
    int32_t pad0;
    int32_t* lsn_count;
    ewk_listener* lsn_tab;
    LsnState* lsn_st;
    const GateStream* st;
    int32_t* stream_profile;
    int32_t* stream_word;
    double tick_seconds;
};
hipError_t launch_listeners_set(const ListenerSetArgs& a, hipStream_t s);
// Zero a ring with agent-scope (sc1) stores: the lines go to memory and are dropped from the
// writing XCD's L2, so no cached copy of the initial zeros outlives the gate's first writes.
hipError_t launch_ring_zero(void* p, size_t bytes, hipStream_t s);
int gate_val_len(const PwTree* trees_host, int n_blocks);
// per-wave sample staging length for a config (0 when the lengths exceed the LDS budget)
int gate_stage_len(int block, int64_t n_last);

}  // namespace ewk
