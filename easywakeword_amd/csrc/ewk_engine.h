// ewk_engine.h -- the engine behind the C ABI (include/ewk.h): its state, and the helpers its
// sources share.  Internal: only ewk_engine.cpp and ewk_engine_{score,resample} (batch side),
// ewk_engine_{stream,chunks,assign,poll}.cpp (streaming side) include it.
#pragma once

#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "ewk_chunk_plan.h"
#include "ewk_g711.h"
#include "ewk_gate.h"
#include "ewk_internal.h"
#include "ewk_snapshot.h"

namespace ewk {

// Sets the calling thread's ewk_last_error string and returns `code`.
int fail(int code, const std::string& msg);

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess)                                                                  \
            return fail(EWK_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e));          \
    } while (0)

// Device memory that grows and is freed with its owner (callers synchronize before a
// temporary goes out of scope).
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;   // elements
    unsigned flags = 0;   // hipExtMallocWithFlags flags (0: hipMalloc)
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    hipError_t reserve(size_t n) {
        if (n <= cap) return hipSuccess;
        release();
        size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
        hipError_t e = flags ? hipExtMallocWithFlags((void**)&p, bytes, flags) : hipMalloc(&p, bytes);
        if (e == hipSuccess) cap = n;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

// Pinned host memory on its way to the device, and the event that says its last DMA has left it:
// reserve(), fill, hipMemcpyAsync on s, sent(s).
struct PinnedStage {
    unsigned char* p = nullptr;
    size_t cap = 0;   // bytes
    hipEvent_t done = nullptr;
    bool recorded = false;
    PinnedStage() = default;
    PinnedStage(const PinnedStage&) = delete;
    PinnedStage& operator=(const PinnedStage&) = delete;
    ~PinnedStage() {
        (void)hipHostFree(p);
        if (done) (void)hipEventDestroy(done);
    }
    hipError_t wait() { return recorded ? hipEventSynchronize(done) : hipSuccess; }
    hipError_t reserve(size_t bytes) {   // at least `bytes`, nothing in flight out of them: the caller's to fill
        hipError_t err = wait();
        if (err == hipSuccess && !done) err = hipEventCreateWithFlags(&done, hipEventDisableTiming);
        if (err != hipSuccess || bytes <= cap) return err;
        (void)hipHostFree(p);
        p = nullptr;
        err = hipHostMalloc((void**)&p, bytes, hipHostMallocDefault);
        cap = err == hipSuccess ? bytes : 0;
        return err;
    }
    hipError_t sent(hipStream_t s) { return recorded = true, hipEventRecord(done, s); }
    template <typename T>
    T* as() const { return reinterpret_cast<T*>(p); }
};

// A chunk push's plan and layout (ewk_chunk_plan.h), kept between pushes for its storage.
struct ChunkPlan {
    std::vector<int32_t> pending, ticks, new_pending, order;   // [n], per listed stream (order: n_ticking used)
    std::vector<int64_t> src_at;                               // [n]: chunk i's first sample in the push's source
    int32_t group_ticks[EWK_CHUNK_MAX_TICKS], group_first[EWK_CHUNK_MAX_TICKS + 1];
    int64_t group_base[EWK_CHUNK_MAX_TICKS];                   // first tick row of group g in chunk_asm
    int32_t in_block = 0, n_ticking = 0, n_groups = 0;
    int64_t asm_total = 0, stage_total = 0;                    // samples: all tick rows; the staged host chunks
};

constexpr int kWorkInts = 32;          // ewk_engine::d_work
constexpr int32_t kPollChunk = 1024;   // events copied speculatively with the counters
constexpr size_t kPollRegion = 16 + (size_t)kPollChunk * sizeof(ewk_event);   // per bank: counters + chunk
constexpr const char* kNoBank = "No reference word set. Call set_bank() first.";

}  // namespace ewk

struct ewk_engine {
    int device = 0;
    hipStream_t stream = nullptr;
    ewk_config cfg{};
    int32_t n_streams = 0;
    int64_t ring_len = 0;           // the reference ring (buffer_seconds * sample_rate)
    int64_t sring_len = 0;          // samples stored per stream (ring_len, or cfg.ring_samples)
    int32_t n_blocks = 0;
    int64_t n_last = 0;

    ewk::Tables* d_tab = nullptr;
    ewk::Tables64* d_tab64 = nullptr;
    float* d_tmpl = nullptr;
    float h_tmpl[2 * ewk::NMFCC];
    float uu_m32 = 0.f, uu_s32 = 0.f;   // numpy float32 dot of the template with itself
    bool has_tmpl = false;

    // fp64 re-score (ewk_rescore.h): slots of listed segments and the chunk part pool, shared
    // by linear and ring launches (which never run concurrently: join_scoring)
    ewk::DevBuf<ewk::RsSlot> rs_slots;
    ewk::DevBuf<int32_t> rs_serial;      // serial slots of a launch
    ewk::DevBuf<ewk::RsPart> rs_parts;   // uncached (ScoreArgs::rs_ctl)
    int32_t rs_cap = 0;             // slots
    int32_t rs_part_cap = 0;        // part records (a slot that finds the pool full runs serially)
    // [0] linear work, [1] ring work, [4..5] event-count snapshots, [16..23] ring re-score
    // counters (ScoreArgs::rs_ctl), [24..31] linear re-score counters
    int32_t* d_work = nullptr;
    int32_t* d_compact = nullptr;   // ewk_compact_positives block counts / offsets
    int32_t compact_cap = 0;        // ... in blocks
    ewk::DevBuf<int32_t> order;     // linear batches: longest-first work order (k_lpt_order)

    // host-API staging
    ewk::DevBuf<float> pcm;
    ewk::DevBuf<int64_t> offsets;
    ewk::DevBuf<int32_t> lengths;
    ewk::DevBuf<float> mean, stdv;
    ewk::DevBuf<double> score;
    ewk::DevBuf<uint8_t> match;
    ewk::DevBuf<double> mean64, std64;

    // template bank (ewk_bank.hip): host copy as set, device copy value-major per word
    std::vector<float> bank_mean, bank_std;   // [K][20]
    std::vector<int32_t> bank_first;          // [n_words + 1]; empty: no bank
    std::vector<double> bank_thr;             // [n_words]
    bool bank_thr_follow = false;             // thresholds follow cfg.similarity_threshold
    int32_t bank_max_word = 0;
    ewk::DevBuf<float> d_bank;                // [K][kBankRow] (BankArgs::bank)
    ewk::DevBuf<int32_t> d_bank_first;
    ewk::DevBuf<double> d_bank_thr;
    ewk::DevBuf<int32_t> bk_cnt, bk_seg, bk_len;   // the fp64 list of a bank scoring call
    ewk::DevBuf<int64_t> bk_off;
    ewk::DevBuf<int32_t> bk_word;             // host-call staging
    ewk::DevBuf<ewk_bank_result> bk_out;
    ewk::DevBuf<double> bk_scores;
    // stream bank (ewk_stream_bank_enable): gated events are scored against the bank.  Per event
    // slot (one set for both event banks: scoring passes are serialised on their stream) the
    // float32 statistics and theta_s of the ring scorer, the fp64 statistics of the re-score, and
    // the list of the events a pass re-scores (BankEvArgs::ev_list); allocated at the first enable.
    bool sbank_on = false;
    bool sbank_words = false;                 // sb_word holds a word per stream (else: word 0)
    ewk::DevBuf<int32_t> sb_word;             // [n_streams]
    ewk::DevBuf<float> sb_mean, sb_std, sb_theta;  // [ev_cap][20], [ev_cap][20], [ev_cap]
    ewk::DevBuf<double> sb_mean64, sb_std64;  // [ev_cap][20]
    ewk::DevBuf<int32_t> sb_list;             // [kEvListHdr + ev_cap]

    // streaming
    void* d_ring = nullptr;         // float32 or int16 samples (cfg.ring_format)
    size_t ring_es = sizeof(float); // bytes per ring sample
    float* ring_f32() const { return ring_es == sizeof(float) ? static_cast<float*>(d_ring) : nullptr; }
    int16_t* ring_i16() const { return ring_es == sizeof(int16_t) ? static_cast<int16_t*>(d_ring) : nullptr; }
    double* d_brms = nullptr;
    double* d_sorted = nullptr;     // [streams][2][n_blocks] sorted block RMS (double-buffered)
    ewk::PwTree* d_trees = nullptr; // numpy pairwise-sum trees for the block and the last 0.1 s
    ewk::GateStream* d_st = nullptr;
    // Two event banks (ev_cap events + 4 counters each: [0] count, [1] dropped,
    // [2] scored watermark): pushes append to `bank`; ewk_poll_lagged drains the
    // other bank while the GPU still works on this one.  The counters only grow (wrapping
    // uint32): a drained bank is re-armed by moving its epoch base to the count the host
    // read -- event i of an epoch is at slot count - base -- so no fill launch per tick.
    ewk_event* d_events = nullptr;   // [2][ev_cap]
    int32_t* d_evc = nullptr;        // [2][4]
    uint32_t ev_base0[2] = {0, 0};   // per bank: count at the start of the current epoch
    uint32_t drop_base0[2] = {0, 0}; // per bank: dropped count at the start of the epoch
    int32_t ev_cap = 0;
    int bank = 0;
    bool bank_used[2] = {false, false};
    hipEvent_t bank_done[2] = {nullptr, nullptr};   // recorded after the last push into a bank
    hipStream_t cstream = nullptr;                  // D2H copies of drained banks
    // Ring-mode scoring of tick t runs on sstream concurrently with the gate of tick t+1
    // on `stream` (the gate only overwrites ring samples older than any scorable segment;
    // see `overlap`).  At most one scoring pass is in flight beside a gate.
    hipStream_t sstream = nullptr;
    hipEvent_t gate_evt[2] = {nullptr, nullptr};
    hipEvent_t score_evt[2] = {nullptr, nullptr};
    bool score_live[2] = {false, false};
    hipEvent_t score_tail = nullptr;                // the latest recorded score_evt
    int64_t push_seq = 0;
    bool overlap = false;
    bool overlap_want = false;                      // EWK_SCORE_OVERLAP=1 at ewk_create (overlap: and the ring has the room)
    int32_t ticks_per_launch = 32;                  // gate launch length (segments must outlive it in the ring)
    ewk_event* ev_bank(int b) { return d_events + (size_t)b * ev_cap; }
    int32_t* evc_bank(int b) { return d_evc + 4 * b; }
    ewk::PinnedStage pcm_stage;       // a push's host samples (ticks or chunks) on the way to push_stage
    ewk::DevBuf<float> push_stage;
    unsigned char* h_poll = nullptr;   // pinned: event counters + the first kPollChunk events
    unsigned char* d_poll = nullptr;   // h_poll's device address (k_bank_mirror writes it)
    // mirror[b]: h_poll's region b holds bank b as of bank_done[b], written by k_bank_mirror
    // after the push's last scoring pass (same stream) -- the poll needs no copies
    bool mirror[2] = {false, false};
    int64_t tick = 0;
    // Stream lifecycle (ewk_push_streams / ewk_reset_stream_list).  A lockstep engine has one clock,
    // `tick`.  The first subset push or list reset desynchronises it: stream s has then had
    // tick + tick_delta[s] ticks (the host mirror of GateStream::tick; full pushes still only
    // advance `tick`) and the gate runs every stream on its own clock.  ewk_reset_streams returns
    // the engine to lockstep.  seen / seen_epoch: the duplicate test of an index list, O(n) per call.
    bool desync = false;
    std::vector<int64_t> tick_delta;   // [n_streams] once desynchronised
    std::vector<uint32_t> seen;        // [n_streams]: the epoch of the call that last listed the stream
    uint32_t seen_epoch = 0;
    ewk::PinnedStage ids_stage;        // [2 * n_streams] int32: an index list (and its values) on the way to d_ids
    ewk::DevBuf<int32_t> d_ids;        // [2 * n_streams]
    int64_t stream_tick(int32_t s) const { return tick + (desync ? tick_delta[s] : 0); }
    // Detector profiles (ewk_detector_profiles_set): the table as set and on the device, and the
    // profile of every stream (-1: cfg) on the device with its host mirror; both per-stream arrays
    // are allocated when a table is first set and empty / all -1 without one.  ticks_per_launch
    // then follows the largest segment request over cfg and the table (set_launch_ticks).
    std::vector<ewk_detector_profile> profiles;
    ewk::DevBuf<ewk_detector_profile> d_profiles;
    ewk::DevBuf<int32_t> d_stream_profile;    // [n_streams]
    std::vector<int32_t> stream_profile;      // [n_streams]
    // Stream listeners (ewk_stream_listeners_set).  Allocated by the first call that gives a stream
    // more than one listener: per stream the count, EWK_LISTENERS_MAX table rows and kLsnStates
    // states on the device, count and rows mirrored on the host (row 0 of the mirror is not read:
    // listener 0 is stream_profile[s] and stream_word[s]).  lsn_multi: streams with more than one
    // listener; the gate runs its listener instantiations only while it is > 0.  lsn_stage:
    // [n_streams * (1 + 2 * EWK_LISTENERS_MAX)] ints, a call's rows and counts on the way to
    // d_lsn_stage (the stream list goes through ids_stage).
    ewk::DevBuf<int32_t> d_lsn_count;          // [n_streams]
    ewk::DevBuf<ewk_listener> d_lsn_tab;       // [n_streams][EWK_LISTENERS_MAX]
    ewk::DevBuf<ewk::LsnState> d_lsn_st;       // [n_streams][kLsnStates]
    std::vector<int32_t> lsn_count;            // [n_streams]; empty: every stream has one listener
    std::vector<ewk_listener> lsn_tab;         // [n_streams][EWK_LISTENERS_MAX]
    int32_t lsn_multi = 0;
    ewk::PinnedStage lsn_stage;
    ewk::DevBuf<int32_t> d_lsn_stage;
    std::vector<int32_t> stream_word;          // host mirror of sb_word (empty: word 0 everywhere)
    bool listeners_on() const { return !lsn_count.empty(); }
    // Packet ingest (ewk_push_chunks*, ewk_chunks.hip); everything is allocated by the first chunk
    // push.  chunk_carry: per stream the samples of its unfinished block, in_block elements of the
    // ring's type ([n_streams][in_block]; regrown when a larger input block is set, which is only
    // possible while nothing is pending).  chunk_pending: its host mirror, samples held per stream
    // (every device read of a carry row is bounded by it, so dropping samples needs no device
    // work); chunk_pending_n: streams holding any.  chunk_asm: the tick rows of one push, grown to
    // the largest push so far.  chunk_stage -> d_chunk: a push's descriptors ([n_streams] ChunkDesc)
    // followed by its ticking streams in plan order ([n_streams] int32, the gate's index lists).
    ewk::DevBuf<unsigned char> chunk_carry, chunk_asm, d_chunk;
    std::vector<int32_t> chunk_pending;        // [n_streams]; empty: no chunk push yet
    int32_t chunk_pending_n = 0;
    ewk::PinnedStage chunk_stage;
    ewk::ChunkPlan chunk_plan;                 // the current push's
    void drop_pending(int32_t s) {
        if (chunk_pending.empty() || chunk_pending[s] == 0) return;
        chunk_pending[s] = 0;
        chunk_pending_n -= 1;
    }
    void drop_all_pending() {
        std::fill(chunk_pending.begin(), chunk_pending.end(), 0);
        chunk_pending_n = 0;
    }
    int32_t gate_grid_cap = 0;     // EWK_GATE_GRID_MAX at ewk_create: workgroups per gate launch (0: the built-in maximum)
    int32_t gate_stage = 0;
    int32_t gate_val_len = 0;       // per-wave LDS doubles of the gate (tree values, sort scratch)
    // ewk_gate_launch_info: the instantiation of the last gate launch (-1 before the first) and
    // how the block and last-window sums are evaluated (pw_tree_kind of the two sub-chunk trees)
    ewk::GateFamily gate_last = {-1, -1, -1, -1};
    int32_t gate_tree_kind[2] = {-1, -1};

    // input-rate resampler (ewk_resample.hip).  rs_in: the filter of ewk_set_input_rate, with the
    // per-stream history ([n_streams][H] float32: the last H input samples) and the resampled
    // ticks the gate reads ([n_streams][n_ticks * block], grown to the longest push so far);
    // rs_one: the filter of the latest ewk_resample call.
    struct RsFilter {
        int32_t rate = 0, up = 1, down = 1, half = 0, J = 0, H = 0, threads = 0, span = 0;
        int64_t c0 = 0;             // ResampleArgs::c0
        ewk::DevBuf<double> taps;   // [J][up]
    };
    RsFilter rs_in, rs_one;
    bool rs_on = false;
    bool rs_fresh = true;   // no push since the history was cleared: the first `delay` outputs are zero
    int32_t rs_in_block = 0, rs_delay = 0;
    ewk::DevBuf<float> rs_hist, rs_out;
    // the same per stream ([n_streams], device), in place of rs_fresh from the first subset push or
    // list reset with a rate set: set where a stream's history was cleared, cleared by its next push
    ewk::DevBuf<uint8_t> rs_flags;

    // Level-3 front end (ewk_whisper_features_*, ewk_engine_whisper.cpp); nothing is allocated
    // before the first call.  wf_y: the segments normalised by k_normalize (float64, packed);
    // wf_raw / wf_fmax: raw log-mel and maximum of every live frame; wf_seg: the per-segment plan;
    // wf_i64 / wf_len / wf_ev: k_normalize's offsets, lengths and events; wf_pcm / wf_out: a host
    // batch on its way in and host-bound features on their way out.  All grow behind the stream.
    ewk::DevBuf<ewk::WhisperTables> wf_tab;
    ewk::DevBuf<double> wf_y;
    ewk::DevBuf<float> wf_raw, wf_fmax, wf_pcm;
    ewk::DevBuf<ewk::WfSeg> wf_seg;
    ewk::DevBuf<int64_t> wf_i64;
    ewk::DevBuf<int32_t> wf_len;
    ewk::DevBuf<ewk_event> wf_ev;
    ewk::DevBuf<unsigned char> wf_out;

    // measurement: (start, stop) event pairs per kernel family
    bool prof = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[6];

    // Stream snapshots (ewk_export_streams / ewk_import_streams, ewk_engine_snapshot.cpp); nothing
    // is allocated before the first call with a host payload.  snap_dev: records between the
    // pack / unpack launch and the DMA, two halves of snap_half bytes; snap_pin: the pinned side
    // of each half (the DMA never touches d_ring).
    ewk::DevBuf<unsigned char> snap_dev;
    ewk::PinnedStage snap_pin[2];
    size_t snap_half = 0;
    std::vector<hipEvent_t> ev_pool;
};

namespace ewk {

hipEvent_t pool_event(ewk_engine* e);   // from ev_pool, or a new one (nullptr: none to be had)

// RAII bracket: records start/stop events around one launch when profiling.
struct ProfScope {
    ewk_engine* e;
    int kind;
    hipStream_t s;
    hipEvent_t a = nullptr, b = nullptr;
    ProfScope(ewk_engine* e_, int kind_, hipStream_t s_) : e(e_), kind(kind_), s(s_) {
        if (!e->prof) return;
        a = pool_event(e);
        b = pool_event(e);
        if (a) (void)hipEventRecord(a, s);
    }
    ~ProfScope() {
        if (!e->prof || !a || !b) return;
        (void)hipEventRecord(b, s);
        e->ev[kind].push_back({a, b});
    }
};

// What a push's samples are: float32, int16 PCM, or G.711 codes with their law (ewk_g711.h).  The
// gate reads the first two; G.711 always goes through the resampler, which hands on float32.
enum SampleType : int32_t { kSampleF32 = 0, kSamplePcm16 = 1, kSampleG711 = 2 };
struct SampleKind {
    SampleType type;
    int32_t law;   // kSampleG711: kG711Ulaw / kG711Alaw (a chunk push with per-chunk laws: unused)
    size_t es() const { return type == kSampleF32 ? sizeof(float) : type == kSamplePcm16 ? sizeof(int16_t) : 1; }
};
constexpr SampleKind kKindF32{kSampleF32, 0}, kKindPcm16{kSamplePcm16, 0};

// Where the tick samples of a push are now: stream (row) r, tick t at p + r * stride + t * tick_stride
// (in samples of `kind`).
struct TickSrc {
    const void* p;
    SampleKind kind;
    int64_t stride, tick_stride;
};

// ewk_engine.cpp
hipError_t join_scoring(ewk_engine* e, hipStream_t s);
hipError_t reserve_rescore(ewk_engine* e, int32_t n_seg);
// the longest segment request of a set of timings, and the gate launch length (with `overlap`) it allows
int64_t segment_need(const ewk_config& c, int64_t ring_len, double speech_duration_max, double post_speech_silence,
                     double padding);
void set_launch_ticks(ewk_engine* e, int64_t seg_need);
// ewk_engine_score.cpp
ScoreArgs base_args(ewk_engine* e);
BankArgs bank_args(ewk_engine* e);
int bank_follow_threshold(ewk_engine* e, hipStream_t s);
enum WordOf { kOfSegment, kOfStream };   // "word index W of {segment|stream} I is outside [0, N)"
int fail_word_index(int32_t word, WordOf of, int32_t i, int32_t n_words);
// polled events about to be read from the rings: EWK_EINVAL for one outside them or from a tick not
// pushed, EWK_EOVERWRITTEN for one whose samples its stream has overwritten since
int check_ring_events(ewk_engine* e, const ewk_event* events, int32_t n);
// ewk_engine_resample.cpp: a push's resample stage -- every tick at *src into rs_out (float32 16 kHz
// blocks, where *src then points), the history saved for the next push; d_list: ResampleArgs::ids
int resample_ticks(ewk_engine* e, TickSrc* src, int32_t rows, int32_t n_ticks, const int32_t* d_list, hipStream_t s);

// A device buffer that launches enqueued on s read grows only once s is idle: an earlier launch
// may still read the old buffer.
template <typename T>
int grow_behind(DevBuf<T>& b, size_t n, hipStream_t s) {
    if (n > b.cap) HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(b.reserve(n));
    return EWK_OK;
}

// ewk_engine_stream.cpp: index lists, and the stages that tick and chunk pushes share
int fail_stream_index(ewk_engine* e, int32_t i, int32_t s);
int check_stream_list(ewk_engine* e, const int32_t* streams, int32_t n);   // of a call that changes streams
int check_query_list(ewk_engine* e, const int32_t* streams, int32_t n);    // of a query (NULL: streams 0..n-1)
int stage_stream_list(ewk_engine* e, const int32_t* streams, const int32_t* vals, int32_t n, hipStream_t s);
int scatter_assign(ewk_engine* e, ewk::DevBuf<int32_t>& dst, std::vector<int32_t>& mirror, const int32_t* streams,
                   const int32_t* vals, int32_t n, hipStream_t s);
int desynchronise(ewk_engine* e, hipStream_t s);
int check_g711(ewk_engine* e, int32_t law, const uint8_t* laws, int32_t n);   // the refusals of a G.711 push
int send_staged(ewk_engine* e, size_t bytes, hipStream_t s);
int gate_ticks(ewk_engine* e, const TickSrc& src, int32_t rows, int32_t n_ticks, const int32_t* d_list,
               const int32_t* streams, hipStream_t s);
int finish_push(ewk_engine* e, hipStream_t s);
// ewk_engine_assign.cpp: the per-stream word and profile index arrays, created on s when first needed
int ensure_stream_words(ewk_engine* e, hipStream_t s);
int ensure_stream_profile(ewk_engine* e, hipStream_t s);
// ewk_engine_poll.cpp
hipError_t ensure_poll_region(ewk_engine* e);

}  // namespace ewk
