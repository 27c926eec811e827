// ewk_engine.cpp -- the C ABI (include/ewk.h): engine lifetime, device memory,
// the level-2 batch scorer entry points and the level-1+2 streaming tick path.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "ewk_gate.h"
#include "ewk_internal.h"

using namespace ewk;

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess)                                                                  \
            return fail(EWK_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e));          \
    } while (0)

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;   // elements
    unsigned flags = 0;   // hipExtMallocWithFlags flags (0: hipMalloc)
    hipError_t reserve(size_t n) {
        if (n <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
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

constexpr int kWorkInts = 32;          // ewk_engine::d_work
constexpr int32_t kPollChunk = 1024;   // events copied speculatively with the counters
constexpr size_t kPollRegion = 16 + (size_t)kPollChunk * sizeof(ewk_event);   // per bank: counters + chunk

// Scoped temporary device buffer (freed on return; callers synchronize before).
template <typename T>
struct TmpBuf : DevBuf<T> {
    ~TmpBuf() { this->release(); }
};

}  // namespace

struct ewk_engine {
    int device = 0;
    hipStream_t stream = nullptr;
    ewk_config cfg{};
    int32_t n_streams = 0;
    int64_t ring_len = 0;           // the reference ring (buffer_seconds * sample_rate)
    int64_t sring_len = 0;          // samples stored per stream (ring_len, or cfg.ring_samples)
    int32_t n_blocks = 0;
    int64_t n_last = 0;

    Tables* d_tab = nullptr;
    Tables64* d_tab64 = nullptr;
    float* d_tmpl = nullptr;
    float h_tmpl[2 * NMFCC];
    float uu_m32 = 0.f, uu_s32 = 0.f;   // numpy float32 dot of the template with itself
    bool has_tmpl = false;

    // fp64 re-score (ewk_rescore.h): slots of listed segments and the chunk part pool, shared
    // by linear and ring launches (which never run concurrently: join_scoring)
    DevBuf<RsSlot> rs_slots;
    DevBuf<int32_t> rs_serial;      // serial slots of a launch
    DevBuf<RsPart> rs_parts;        // uncached (ScoreArgs::rs_ctl)
    int32_t rs_cap = 0;             // slots
    int32_t rs_part_cap = 0;        // part records (a slot that finds the pool full runs serially)
    // [0] linear work, [1] ring work, [4..5] event-count snapshots, [16..23] ring re-score
    // counters (ScoreArgs::rs_ctl), [24..31] linear re-score counters
    int32_t* d_work = nullptr;
    int32_t* d_compact = nullptr;   // ewk_compact_positives block counts / offsets
    int32_t compact_cap = 0;        // ... in blocks
    DevBuf<int32_t> order;          // linear batches: longest-first work order (k_lpt_order)

    // host-API staging
    DevBuf<float> pcm;
    DevBuf<int64_t> offsets;
    DevBuf<int32_t> lengths;
    DevBuf<float> mean, stdv;
    DevBuf<double> score;
    DevBuf<uint8_t> match;
    DevBuf<double> mean64, std64;

    // template bank (ewk_bank.hip): host copy as set, device copy value-major per word
    std::vector<float> bank_mean, bank_std;   // [K][20]
    std::vector<int32_t> bank_first;          // [n_words + 1]; empty: no bank
    std::vector<double> bank_thr;             // [n_words]
    bool bank_thr_follow = false;             // thresholds follow cfg.similarity_threshold
    int32_t bank_max_word = 0;
    DevBuf<float> d_bank;                     // [K][kBankRow] (BankArgs::bank)
    DevBuf<int32_t> d_bank_first;
    DevBuf<double> d_bank_thr;
    DevBuf<int32_t> bk_cnt, bk_seg, bk_len;   // the fp64 list of a bank scoring call
    DevBuf<int64_t> bk_off;
    DevBuf<int32_t> bk_word;                  // host-call staging
    DevBuf<ewk_bank_result> bk_out;
    DevBuf<double> bk_scores;
    // stream bank (ewk_stream_bank_enable): gated events are scored against the bank.  Per event
    // slot (one set for both event banks: scoring passes are serialised on their stream) the
    // float32 statistics and theta_s of the ring scorer, the fp64 statistics of the re-score, and
    // the list of the events a pass re-scores (BankEvArgs::ev_list); allocated at the first enable.
    bool sbank_on = false;
    bool sbank_words = false;                 // sb_word holds a word per stream (else: word 0)
    DevBuf<int32_t> sb_word;                  // [n_streams]
    DevBuf<float> sb_mean, sb_std, sb_theta;  // [ev_cap][20], [ev_cap][20], [ev_cap]
    DevBuf<double> sb_mean64, sb_std64;       // [ev_cap][20]
    DevBuf<int32_t> sb_list;                  // [kEvListHdr + ev_cap]

    // streaming
    void* d_ring = nullptr;         // float32 or int16 samples (cfg.ring_format)
    size_t ring_es = sizeof(float); // bytes per ring sample
    float* ring_f32() const { return ring_es == sizeof(float) ? static_cast<float*>(d_ring) : nullptr; }
    int16_t* ring_i16() const { return ring_es == sizeof(int16_t) ? static_cast<int16_t*>(d_ring) : nullptr; }
    double* d_brms = nullptr;
    double* d_sorted = nullptr;     // [streams][2][n_blocks] sorted block RMS (double-buffered)
    PwTree* d_trees = nullptr;      // numpy pairwise-sum trees for the block and the last 0.1 s
    GateStream* d_st = nullptr;
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
    int32_t ticks_per_launch = 32;                  // gate launch length (segments must outlive it in the ring)
    ewk_event* ev_bank(int b) { return d_events + (size_t)b * ev_cap; }
    int32_t* evc_bank(int b) { return d_evc + 4 * b; }
    DevBuf<float> push_stage;
    float* h_stage = nullptr;       // pinned host staging for ewk_push / ewk_push_many
    unsigned char* h_poll = nullptr;   // pinned: event counters + the first kPollChunk events
    unsigned char* d_poll = nullptr;   // h_poll's device address (k_bank_mirror writes it)
    // mirror[b]: h_poll's region b holds bank b as of bank_done[b], written by k_bank_mirror
    // after the push's last scoring pass (same stream) -- the poll needs no copies
    bool mirror[2] = {false, false};
    size_t h_stage_cap = 0;
    hipEvent_t h_stage_free = nullptr;   // recorded after the last DMA out of h_stage
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
    int32_t* h_ids = nullptr;          // pinned [2 * n_streams]: an index list (and its words) on the way to d_ids
    DevBuf<int32_t> d_ids;             // [2 * n_streams]
    hipEvent_t h_ids_free = nullptr;   // recorded after the last DMA out of h_ids
    int64_t stream_tick(int32_t s) const { return tick + (desync ? tick_delta[s] : 0); }
    int32_t gate_stage = 0;
    int32_t gate_val_len = 0;       // per-wave LDS doubles of the gate (tree values, sort scratch)

    // input-rate resampler (ewk_resample.hip).  rs_in: the filter of ewk_set_input_rate, with the
    // per-stream history ([n_streams][H] float32: the last H input samples) and the resampled
    // ticks the gate reads ([n_streams][n_ticks * block], grown to the longest push so far);
    // rs_one: the filter of the latest ewk_resample call.
    struct RsFilter {
        int32_t rate = 0, up = 1, down = 1, half = 0, J = 0, H = 0, threads = 0, span = 0;
        int64_t c0 = 0;        // ResampleArgs::c0
        DevBuf<double> taps;   // [J][up]
    };
    RsFilter rs_in, rs_one;
    bool rs_on = false;
    bool rs_fresh = true;   // no push since the history was cleared: the first `delay` outputs are zero
    int32_t rs_in_block = 0, rs_delay = 0;
    DevBuf<float> rs_hist, rs_out;
    // the same per stream ([n_streams], device), in place of rs_fresh from the first subset push or
    // list reset with a rate set: set where a stream's history was cleared, cleared by its next push
    DevBuf<uint8_t> rs_flags;

    // measurement: (start, stop) event pairs per kernel family
    bool prof = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[4];
    std::vector<hipEvent_t> ev_pool;
};

static hipEvent_t pool_event(ewk_engine* e) {
    if (!e->ev_pool.empty()) {
        hipEvent_t x = e->ev_pool.back();
        e->ev_pool.pop_back();
        return x;
    }
    hipEvent_t x = nullptr;
    if (hipEventCreate(&x) != hipSuccess) return nullptr;
    return x;
}

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

static void zero_event_state(ewk_engine* e) {
    if (e->d_evc) (void)hipMemsetAsync(e->d_evc, 0, 8 * sizeof(int32_t), e->stream);
    e->ev_base0[0] = e->ev_base0[1] = 0;
    e->drop_base0[0] = e->drop_base0[1] = 0;
    e->bank_used[0] = e->bank_used[1] = false;
    e->mirror[0] = e->mirror[1] = false;
}

static hipError_t ensure_poll_region(ewk_engine* e) {
    if (e->h_poll && e->d_poll) return hipSuccess;
    if (!e->h_poll) {
        hipError_t err = hipHostMalloc((void**)&e->h_poll, 2 * kPollRegion, hipHostMallocDefault);
        if (err != hipSuccess) { e->h_poll = nullptr; return err; }
    }
    hipError_t err = hipHostGetDevicePointer((void**)&e->d_poll, e->h_poll, 0);
    if (err != hipSuccess) {   // never leave a host region without its device alias (the mirror writes through it)
        (void)hipHostFree(e->h_poll);
        e->h_poll = nullptr;
        e->d_poll = nullptr;
    }
    return err;
}

// Order stream s after every ring-mode scoring pass enqueued so far (they run on
// sstream): needed before touching what those passes read or share -- the template,
// the re-score list, the log-mel and fp64 scratch, the event banks.
static hipError_t join_scoring(ewk_engine* e, hipStream_t s) {
    if (!e->overlap || !e->score_tail) return hipSuccess;
    return hipStreamWaitEvent(s, e->score_tail, 0);
}

// The re-score list holds at most one slot per segment of a launch (slots must start zeroed).
static hipError_t reserve_rescore(ewk_engine* e, int32_t n_seg) {
    if (n_seg <= e->rs_cap) return hipSuccess;
    hipError_t err = hipSuccess;
    if (e->stream) err = hipStreamSynchronize(e->stream);
    if (err == hipSuccess && e->sstream) err = hipStreamSynchronize(e->sstream);
    if (err != hipSuccess) return err;
    err = e->rs_slots.reserve((size_t)n_seg);
    if (err == hipSuccess) err = hipMemset(e->rs_slots.p, 0, (size_t)n_seg * sizeof(RsSlot));
    if (err == hipSuccess) err = e->rs_serial.reserve((size_t)n_seg);
    if (err != hipSuccess) return err;
    err = e->order.reserve((size_t)n_seg + kLptScratch);
    if (err != hipSuccess) return err;
    e->rs_cap = n_seg;
    return hipSuccess;
}

// Part records for the chunks of the slots listed in one launch (8 frames each).
static hipError_t reserve_parts(ewk_engine* e, int32_t n) {
    if (n <= e->rs_part_cap) return hipSuccess;
    hipError_t err = hipSuccess;
    if (e->stream) err = hipStreamSynchronize(e->stream);
    if (err == hipSuccess && e->sstream) err = hipStreamSynchronize(e->sstream);
    e->rs_parts.flags = hipDeviceMallocUncached;
    if (err == hipSuccess) err = e->rs_parts.reserve((size_t)n);
    if (err == hipSuccess) e->rs_part_cap = n;
    return err;
}

extern "C" {

void ewk_default_config(ewk_config* c) {
    memset(c, 0, sizeof(*c));
    c->sample_rate = 16000;
    c->buffer_seconds = 10;
    c->block = 1600;
    c->tick_seconds = 0.1;
    c->pre_speech_silence = 0.8;
    c->speech_duration_min = 0.3;
    c->speech_duration_max = 2.0;
    c->post_speech_silence = 0.4;
    c->padding = 0.05;
    c->max_segment_seconds = 3.0;
    c->similarity_threshold = 75.0;
    c->reentry_timeout = 0.0;
    c->min_threshold = 0.005;
    c->initial_threshold = 0.01;
    c->rescore_margin = 1e-3;
}

const char* ewk_last_error(void) { return g_err.c_str(); }
int ewk_abi_version(void) { return EWK_ABI_VERSION; }

int ewk_runtime_info(char* path, int32_t cap, int32_t* hip_version) {
    // the definition hipLaunchKernel resolved to for this library: with RTLD_GLOBAL
    // interposition (e.g. torch's bundled runtime loaded first) it is not the
    // libamdhip64.so.7 libewk.so was linked against
    Dl_info info;
    memset(&info, 0, sizeof(info));
    const void* sym = reinterpret_cast<const void*>(&hipLaunchKernel);
    if (!dladdr(sym, &info) || !info.dli_fname) return fail(EWK_EHIP, "dladdr(hipLaunchKernel) failed");
    if (path && cap > 0) {
        strncpy(path, info.dli_fname, (size_t)cap - 1);
        path[cap - 1] = 0;
    }
    if (hip_version) {
        int v = -1;
        if (hipRuntimeGetVersion(&v) != hipSuccess) v = -1;
        *hip_version = v;
    }
    return EWK_OK;
}

int ewk_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void ewk_destroy(ewk_engine* e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    if (e->sstream) (void)hipStreamSynchronize(e->sstream);
    (void)hipFree(e->d_tab);
    (void)hipFree(e->d_tab64);
    (void)hipFree(e->d_tmpl);
    e->rs_slots.release();
    e->rs_serial.release();
    e->rs_parts.release();
    (void)hipFree(e->d_work);
    (void)hipFree(e->d_compact);
    e->order.release();
    e->pcm.release();
    e->offsets.release();
    e->lengths.release();
    e->mean.release();
    e->stdv.release();
    e->score.release();
    e->match.release();
    e->mean64.release();
    e->std64.release();
    e->d_bank.release();
    e->d_bank_first.release();
    e->d_bank_thr.release();
    e->bk_cnt.release();
    e->bk_seg.release();
    e->bk_len.release();
    e->bk_off.release();
    e->bk_word.release();
    e->bk_out.release();
    e->bk_scores.release();
    e->sb_word.release();
    e->sb_mean.release();
    e->sb_std.release();
    e->sb_theta.release();
    e->sb_mean64.release();
    e->sb_std64.release();
    e->sb_list.release();
    e->push_stage.release();
    e->rs_in.taps.release();
    e->rs_one.taps.release();
    e->rs_hist.release();
    e->rs_out.release();
    e->rs_flags.release();
    e->d_ids.release();
    if (e->h_ids) (void)hipHostFree(e->h_ids);
    if (e->h_ids_free) (void)hipEventDestroy(e->h_ids_free);
    (void)hipFree(e->d_ring);
    (void)hipFree(e->d_brms);
    (void)hipFree(e->d_sorted);
    (void)hipFree(e->d_trees);
    (void)hipFree(e->d_st);
    (void)hipFree(e->d_events);
    (void)hipFree(e->d_evc);
    if (e->h_stage) (void)hipHostFree(e->h_stage);
    if (e->h_poll) (void)hipHostFree(e->h_poll);
    if (e->h_stage_free) (void)hipEventDestroy(e->h_stage_free);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    if (e->cstream) (void)hipStreamDestroy(e->cstream);
    if (e->sstream) (void)hipStreamDestroy(e->sstream);
    for (int b = 0; b < 2; ++b) {
        if (e->bank_done[b]) (void)hipEventDestroy(e->bank_done[b]);
        if (e->gate_evt[b]) (void)hipEventDestroy(e->gate_evt[b]);
        if (e->score_evt[b]) (void)hipEventDestroy(e->score_evt[b]);
    }
    delete e;
}

int ewk_reset_streams(ewk_engine* e);

int ewk_create(ewk_engine** out, int device, int32_t n_streams, const ewk_config* cfg) {
    if (!out) return fail(EWK_EINVAL, "out is NULL");
    *out = nullptr;
    ewk_config c;
    if (cfg) c = *cfg;
    else ewk_default_config(&c);
    if (c.sample_rate != 16000) return fail(EWK_EINVAL, "sample_rate must be 16000 (SoundBuffer.FREQUENCY)");
    if (c.buffer_seconds <= 0) return fail(EWK_EINVAL, "buffer_seconds must be positive");
    if (c.block <= 0 || c.block > 8192) return fail(EWK_EINVAL, "block must be in [1, 8192]");
    if (c.tick_seconds <= 0) return fail(EWK_EINVAL, "tick_seconds must be positive");
    if (c.pre_speech_silence <= 0) return fail(EWK_EINVAL, "pre_speech_silence must be positive");
    if (c.speech_duration_min <= 0) return fail(EWK_EINVAL, "speech_duration_min must be positive");
    if (c.speech_duration_max <= 0) return fail(EWK_EINVAL, "speech_duration_max must be positive");
    if (c.speech_duration_min > c.speech_duration_max)
        return fail(EWK_EINVAL, "speech_duration_min must be <= speech_duration_max");
    if (c.post_speech_silence <= 0) return fail(EWK_EINVAL, "post_speech_silence must be positive");
    if (n_streams < 0) return fail(EWK_EINVAL, "n_streams must be >= 0");
    if (c.ring_format != EWK_RING_F32 && c.ring_format != EWK_RING_I16)
        return fail(EWK_EINVAL, "ring_format must be EWK_RING_F32 or EWK_RING_I16");
    const int64_t ring_len = (int64_t)c.buffer_seconds * c.sample_rate;
    if (ring_len > INT32_MAX / 2) return fail(EWK_EINVAL, "buffer_seconds too large");
    // Longest segment request the cut can make (wakeword.py:1100-1111): nreq =
    // int(|sound_start - now - padding| * sr) with now - sound_start <= max speech +
    // (post silence rounded up to a tick), capped at the ring (return_last_n_seconds).
    const int64_t seg_need = std::min<int64_t>(
        ring_len, (int64_t)((c.speech_duration_max + c.post_speech_silence + c.tick_seconds + c.padding) *
                            (double)c.sample_rate) + 2);
    if (c.ring_samples != 0) {
        if (c.ring_samples < 0 || c.ring_samples > ring_len)
            return fail(EWK_EINVAL, "ring_samples must be in [0, buffer_seconds * sample_rate]");
        if (c.ring_samples < ring_len) {
            if (ring_len % c.block != 0 || c.ring_samples % c.block != 0)
                return fail(EWK_EINVAL, "a compact ring (ring_samples) needs block to divide both rings");
            if (gate_stage_len(c.block, (int64_t)(0.1 * (double)c.sample_rate)) < c.block)
                return fail(EWK_EINVAL, "a compact ring (ring_samples) needs block <= 4096");
            if (c.ring_samples < seg_need + c.block || c.ring_samples < (int64_t)(0.1 * (double)c.sample_rate))
                return fail(EWK_EINVAL, "ring_samples must hold the longest segment request plus one tick (" +
                                            std::to_string(seg_need + c.block) + " samples for this config)");
        }
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(EWK_ENODEV, "no HIP device visible");
    if (device < 0 || device >= ndev) return fail(EWK_ENODEV, "device index out of range");
    HIP_TRY(hipSetDevice(device));

    ewk_engine* e = new ewk_engine();
    e->device = device;
    e->cfg = c;
    e->n_streams = n_streams;
    e->ring_len = ring_len;
    e->sring_len = c.ring_samples > 0 ? (int64_t)c.ring_samples : ring_len;
    e->ring_es = c.ring_format == EWK_RING_I16 ? sizeof(int16_t) : sizeof(float);
    e->n_blocks = (int32_t)(e->ring_len / c.block);
    e->n_last = (int64_t)(0.1 * (double)c.sample_rate);   // int(0.1 * FREQUENCY)
    auto bail = [&](hipError_t err, const char* what) {
        std::string m = std::string(what) + ": " + hipGetErrorString(err);
        ewk_destroy(e);
        return fail(err == hipErrorOutOfMemory ? EWK_ENOMEM : EWK_EHIP, m);
    };
    hipError_t err;
    if ((err = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking)) != hipSuccess) return bail(err, "stream");
    if ((err = hipStreamCreateWithFlags(&e->cstream, hipStreamNonBlocking)) != hipSuccess) return bail(err, "stream");
    if ((err = hipStreamCreateWithFlags(&e->sstream, hipStreamNonBlocking)) != hipSuccess) return bail(err, "stream");
    for (int b = 0; b < 2; ++b) {
        if ((err = hipEventCreateWithFlags(&e->gate_evt[b], hipEventDisableTiming)) != hipSuccess) return bail(err, "event");
        if ((err = hipEventCreateWithFlags(&e->score_evt[b], hipEventDisableTiming)) != hipSuccess) return bail(err, "event");
    }
    for (int b = 0; b < 2; ++b)
        if ((err = hipEventCreateWithFlags(&e->bank_done[b], hipEventDisableTiming)) != hipSuccess)
            return bail(err, "event");
    {
        std::vector<unsigned char> buf(sizeof(Tables));
        Tables* t = reinterpret_cast<Tables*>(buf.data());
        build_tables(t);
        if (!t->ok) {
            ewk_destroy(e);
            return fail(EWK_EHIP, "mel filterbank does not fit the kernel's band layout");
        }
        if ((err = hipMalloc(&e->d_tab, sizeof(Tables))) != hipSuccess) return bail(err, "tables");
        if ((err = hipMemcpy(e->d_tab, t, sizeof(Tables), hipMemcpyHostToDevice)) != hipSuccess) return bail(err, "tables");
        std::vector<unsigned char> buf64(sizeof(Tables64));
        Tables64* t64 = reinterpret_cast<Tables64*>(buf64.data());
        build_tables64(t64);
        for (int m = 0; m < NMEL; ++m)
            if (t64->mel_off[m + 1] - t64->mel_off[m] > (m < NMEL / 2 ? kRsMelWLo : kRsMelW)) {
                ewk_destroy(e);
                return fail(EWK_EHIP, "mel filterbank band wider than the fp64 path's window (kRsMelWLo / kRsMelW)");
            }
        if ((err = hipMalloc(&e->d_tab64, sizeof(Tables64))) != hipSuccess) return bail(err, "tables64");
        if ((err = hipMemcpy(e->d_tab64, t64, sizeof(Tables64), hipMemcpyHostToDevice)) != hipSuccess)
            return bail(err, "tables64");
    }
    if ((err = hipMalloc(&e->d_tmpl, 2 * NMFCC * sizeof(float))) != hipSuccess) return bail(err, "template");
    if ((err = reserve_rescore(e, 4096)) != hipSuccess) return bail(err, "rescore slots");
    if ((err = reserve_parts(e, 16384)) != hipSuccess) return bail(err, "rescore parts");
    if ((err = hipMalloc(&e->d_work, kWorkInts * sizeof(int32_t))) != hipSuccess) return bail(err, "work counter");
    if ((err = hipMemset(e->d_work, 0, kWorkInts * sizeof(int32_t))) != hipSuccess) return bail(err, "work counter");
    if (n_streams > 0) {
        const size_t ring_bytes = (size_t)n_streams * e->sring_len * e->ring_es;
        if ((err = hipMalloc(&e->d_ring, ring_bytes)) != hipSuccess) return bail(err, "ring");
        if ((err = hipMalloc(&e->d_brms, (size_t)n_streams * std::max(1, e->n_blocks) * sizeof(double))) != hipSuccess)
            return bail(err, "block rms");
        if ((err = hipMalloc(&e->d_sorted, (size_t)n_streams * 2 * std::max(1, e->n_blocks) * sizeof(double))) !=
            hipSuccess)
            return bail(err, "sorted block rms");
        if ((err = hipMalloc(&e->d_st, (size_t)n_streams * sizeof(GateStream))) != hipSuccess) return bail(err, "state");
        {
            std::vector<PwTree> tr(kNumTrees);
            const int64_t lens[2] = {c.block, e->n_last};
            for (int k = 0; k < 2; ++k) {
                const int64_t n = std::min<int64_t>(lens[k], e->ring_len);
                build_pw_tree(n > kPwChunk ? kPwChunk : 0, &tr[2 * k]);
                const int64_t r = n % kPwChunk;
                build_pw_tree((int)(n > kPwChunk ? (r ? r : kPwChunk) : n), &tr[2 * k + 1]);
            }
            if ((err = hipMalloc(&e->d_trees, kNumTrees * sizeof(PwTree))) != hipSuccess) return bail(err, "trees");
            if ((err = hipMemcpy(e->d_trees, tr.data(), kNumTrees * sizeof(PwTree), hipMemcpyHostToDevice)) != hipSuccess)
                return bail(err, "trees");
            e->gate_val_len = gate_val_len(tr.data(), e->n_blocks);
        }
        e->ev_cap = std::max(4096, 4 * n_streams);
        if ((err = reserve_rescore(e, e->ev_cap)) != hipSuccess) return bail(err, "rescore list");
        // a tick lists ~4 % of its events (the configs[2] recipe), ~20 chunks each
        if ((err = reserve_parts(e, std::min(262144, std::max(16384, e->ev_cap / 2)))) != hipSuccess)
            return bail(err, "rescore parts");
        if ((err = hipMalloc(&e->d_events, 2 * (size_t)e->ev_cap * sizeof(ewk_event))) != hipSuccess)
            return bail(err, "events");
        if ((err = hipMalloc(&e->d_evc, 8 * sizeof(int32_t))) != hipSuccess) return bail(err, "event counters");
        e->gate_stage = gate_stage_len(c.block, e->n_last);
        {   // A segment is cut at the tick that ends it and scored after its gate launch,
            // so the ticks of one launch after the cut must not reach its first sample:
            // ticks_per_launch <= (ring - longest request) / block (>= 1: a one-tick launch is
            // always safe, the cut never asks for more than the ring).  Overlapping the
            // scoring with the next gate launch doubles the ticks that may pass.
            const int64_t room = (e->sring_len - std::min(seg_need, e->sring_len)) / (int64_t)c.block;
            const int64_t tpl = std::max<int64_t>(1, std::min<int64_t>(32, room));
            const int64_t tpl_ov = std::min<int64_t>(32, room / 2);
            // opt-in (EWK_SCORE_OVERLAP=1): measured on MI355X the extra stream/event calls
            // per tick cost more host time than the concurrency saves (scripts/mb_stream.py)
            const char* env = getenv("EWK_SCORE_OVERLAP");
            e->overlap = tpl_ov >= 1 && env && env[0] == '1';
            e->ticks_per_launch = (int32_t)(e->overlap ? tpl_ov : tpl);
        }
        int rc = ewk_reset_streams(e);
        if (rc != EWK_OK) {
            std::string m = g_err;
            ewk_destroy(e);
            return fail(rc, m);
        }
    }
    if ((err = hipStreamSynchronize(e->stream)) != hipSuccess) return bail(err, "sync");
    *out = e;
    return EWK_OK;
}

int ewk_sync(ewk_engine* e) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipStreamSynchronize(e->sstream));
    return EWK_OK;
}

void* ewk_stream_handle(ewk_engine* e) { return e ? (void*)e->stream : nullptr; }

int ewk_set_template(ewk_engine* e, const float* mean20, const float* std20) {
    if (!e || !mean20 || !std20) return fail(EWK_EINVAL, "NULL argument");
    memcpy(e->h_tmpl, mean20, NMFCC * sizeof(float));
    memcpy(e->h_tmpl + NMFCC, std20, NMFCC * sizeof(float));
    {   // cblas_sdot for n = 20: float products accumulated in double, rounded to float
        double am = 0.0, as = 0.0;
        for (int i = 0; i < NMFCC; ++i) {
            const float pm = mean20[i] * mean20[i], ps = std20[i] * std20[i];
            am += (double)pm;
            as += (double)ps;
        }
        e->uu_m32 = (float)am;
        e->uu_s32 = (float)as;
    }
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(join_scoring(e, e->stream));
    HIP_TRY(hipMemcpyAsync(e->d_tmpl, e->h_tmpl, sizeof(e->h_tmpl), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->has_tmpl = true;
    return EWK_OK;
}

int ewk_set_similarity_threshold(ewk_engine* e, double threshold) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (!(threshold == threshold)) return fail(EWK_EINVAL, "threshold is NaN");
    e->cfg.similarity_threshold = threshold;
    return EWK_OK;
}

int ewk_get_template(ewk_engine* e, float* mean20, float* std20) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (!e->has_tmpl) return fail(EWK_ENOTEMPLATE, "No reference word set. Call set_reference() first.");
    if (mean20) memcpy(mean20, e->h_tmpl, NMFCC * sizeof(float));
    if (std20) memcpy(std20, e->h_tmpl + NMFCC, NMFCC * sizeof(float));
    return EWK_OK;
}

static ScoreArgs base_args(ewk_engine* e) {
    ScoreArgs a;
    memset(&a, 0, sizeof(a));
    a.has_template = e->has_tmpl ? 1 : 0;
    a.tmpl = e->d_tmpl;
    a.uu_m32 = e->uu_m32;
    a.uu_s32 = e->uu_s32;
    a.threshold = e->cfg.similarity_threshold;
    a.rescore_margin = e->cfg.rescore_margin;
    a.rs_ctl = e->d_work + 24;
    a.rs_slots = e->has_tmpl ? e->rs_slots.p : nullptr;
    a.rs_serial = e->rs_serial.p;
    a.rs_cap = e->rs_cap;
    a.rs_parts = e->rs_parts.p;
    a.rs_part_cap = e->rs_part_cap;
    a.tab64 = e->d_tab64;
    a.work = e->d_work;
    a.order = e->order.p;
    return a;
}

// f32 scorer + fp64 rescoring of the near-threshold list, all on `s`.
static int score_linear(ewk_engine* e, const float* d_pcm, const int64_t* d_off, const int32_t* d_len, int32_t n,
                        float* d_mean, float* d_std, double* d_score, uint8_t* d_match, int32_t flags,
                        hipStream_t s) {
    ScoreArgs a = base_args(e);
    a.cand_f32 = (flags & EWK_SCORE_F32_CANDIDATES) ? 1 : 0;
    a.pcm = d_pcm;
    a.offsets = d_off;
    a.lengths = d_len;
    a.n_seg = n;
    a.out_mean = d_mean;
    a.out_std = d_std;
    a.out_score = d_score;
    a.out_match = d_match;
    {   // (launch_score_f32 zeroes the work and re-score counters)
        ProfScope ps(e, 0, s);
        HIP_TRY(launch_score_f32(e->d_tab, a, 0, s));
    }
    {
        ProfScope ps(e, 1, s);
        HIP_TRY(launch_rescore_linear(a, s));
    }
    return EWK_OK;
}

int ewk_score_segments_device(ewk_engine* e, const float* d_pcm, const int64_t* d_offsets, const int32_t* d_lengths,
                              int32_t n_seg, float* d_mean, float* d_std, double* d_score, uint8_t* d_match,
                              int32_t flags, void* stream) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (n_seg < 0) return fail(EWK_EINVAL, "n_seg must be >= 0");
    if (n_seg == 0) return EWK_OK;
    if (!d_pcm || !d_offsets || !d_lengths) return fail(EWK_EINVAL, "NULL device pointer");
    if ((flags & EWK_SCORE_REQUIRE_TEMPLATE) && !e->has_tmpl)
        return fail(EWK_ENOTEMPLATE, "No reference word set. Call set_reference() first.");
    if (e->has_tmpl && !d_score) return fail(EWK_EINVAL, "d_score is required when a template is set");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(reserve_rescore(e, n_seg));
    hipStream_t s = stream ? (hipStream_t)stream : e->stream;
    HIP_TRY(join_scoring(e, s));
    return score_linear(e, d_pcm, d_offsets, d_lengths, n_seg, d_mean, d_std, d_score, d_match, flags, s);
}

static int check_segments(const int64_t* offsets, const int32_t* lengths, int32_t n_seg, int64_t n_pcm,
                          int32_t* max_len) {
    int32_t mx = 0;
    for (int32_t i = 0; i < n_seg; ++i) {
        if (lengths[i] < 0 || offsets[i] < 0 || offsets[i] + lengths[i] > n_pcm)
            return fail(EWK_EINVAL, "segment " + std::to_string(i) + " out of range of pcm");
        mx = std::max(mx, lengths[i]);
    }
    *max_len = mx;
    return EWK_OK;
}

int ewk_score_segments(ewk_engine* e, const float* pcm, int64_t n_pcm, const int64_t* offsets,
                       const int32_t* lengths, int32_t n_seg, float* out_mean, float* out_std, double* out_score,
                       uint8_t* out_match, int32_t flags) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (n_seg < 0 || n_pcm < 0) return fail(EWK_EINVAL, "negative size");
    if ((flags & EWK_SCORE_REQUIRE_TEMPLATE) && !e->has_tmpl)
        return fail(EWK_ENOTEMPLATE, "No reference word set. Call set_reference() first.");
    if (n_seg == 0) return EWK_OK;
    if (!offsets || !lengths || (n_pcm > 0 && !pcm)) return fail(EWK_EINVAL, "NULL argument");
    int32_t max_len = 0;
    int rc = check_segments(offsets, lengths, n_seg, n_pcm, &max_len);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(reserve_rescore(e, n_seg));
    HIP_TRY(e->pcm.reserve(std::max<int64_t>(n_pcm, 1)));
    HIP_TRY(e->offsets.reserve(n_seg));
    HIP_TRY(e->lengths.reserve(n_seg));
    HIP_TRY(e->mean.reserve((size_t)n_seg * NMFCC));
    HIP_TRY(e->stdv.reserve((size_t)n_seg * NMFCC));
    HIP_TRY(e->score.reserve(n_seg));
    HIP_TRY(e->match.reserve(n_seg));
    hipStream_t s = e->stream;
    HIP_TRY(join_scoring(e, s));
    if (n_pcm > 0) HIP_TRY(hipMemcpyAsync(e->pcm.p, pcm, n_pcm * sizeof(float), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(e->offsets.p, offsets, n_seg * sizeof(int64_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(e->lengths.p, lengths, n_seg * sizeof(int32_t), hipMemcpyHostToDevice, s));
    {
        ScoreArgs a = base_args(e);
        a.pcm = e->pcm.p;
        a.offsets = e->offsets.p;
        a.lengths = e->lengths.p;
        a.n_seg = n_seg;
        a.out_mean = e->mean.p;
        a.out_std = e->stdv.p;
        a.out_score = e->score.p;
        a.out_match = e->match.p;
        a.cand_f32 = (flags & EWK_SCORE_F32_CANDIDATES) ? 1 : 0;
        HIP_TRY(launch_score_f32(e->d_tab, a, 0, s));   // (zeroes the work and re-score counters)
        HIP_TRY(launch_rescore_linear(a, s));
    }
    if (out_mean) HIP_TRY(hipMemcpyAsync(out_mean, e->mean.p, (size_t)n_seg * NMFCC * 4, hipMemcpyDeviceToHost, s));
    if (out_std) HIP_TRY(hipMemcpyAsync(out_std, e->stdv.p, (size_t)n_seg * NMFCC * 4, hipMemcpyDeviceToHost, s));
    if (e->has_tmpl) {
        if (out_score) HIP_TRY(hipMemcpyAsync(out_score, e->score.p, n_seg * sizeof(double), hipMemcpyDeviceToHost, s));
        if (out_match) HIP_TRY(hipMemcpyAsync(out_match, e->match.p, n_seg, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    return EWK_OK;
}

int ewk_score_segments_f64(ewk_engine* e, const float* pcm, int64_t n_pcm, const int64_t* offsets,
                           const int32_t* lengths, int32_t n_seg, double* out_mean, double* out_std,
                           double* out_score, int32_t flags) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (n_seg < 0 || n_pcm < 0) return fail(EWK_EINVAL, "negative size");
    if (n_seg == 0) return EWK_OK;
    if (!offsets || !lengths || (n_pcm > 0 && !pcm)) return fail(EWK_EINVAL, "NULL argument");
    int32_t max_len = 0;
    int rc = check_segments(offsets, lengths, n_seg, n_pcm, &max_len);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    HIP_TRY(join_scoring(e, s));
    HIP_TRY(reserve_rescore(e, n_seg));
    HIP_TRY(e->pcm.reserve(std::max<int64_t>(n_pcm, 1)));
    HIP_TRY(e->offsets.reserve(n_seg));
    HIP_TRY(e->lengths.reserve(n_seg));
    HIP_TRY(e->mean64.reserve((size_t)n_seg * NMFCC));
    HIP_TRY(e->std64.reserve((size_t)n_seg * NMFCC));
    HIP_TRY(e->score.reserve(n_seg));
    if (n_pcm > 0) HIP_TRY(hipMemcpyAsync(e->pcm.p, pcm, n_pcm * sizeof(float), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(e->offsets.p, offsets, n_seg * sizeof(int64_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(e->lengths.p, lengths, n_seg * sizeof(int32_t), hipMemcpyHostToDevice, s));
    ScoreArgs a = base_args(e);
    a.pcm = e->pcm.p;
    a.offsets = e->offsets.p;
    a.lengths = e->lengths.p;
    a.n_seg = n_seg;
    a.out_score = e->score.p;
    a.cand_f32 = (flags & EWK_SCORE_F32_CANDIDATES) ? 1 : 0;
    // every segment through the fp64 path: the float32 pass only supplies the speculative
    // top_db clamp of each segment (its own scores are overwritten)
    a.list_all = 1;
    a.rs_slots = e->rs_slots.p;
    a.out_mean64 = e->mean64.p;
    a.out_std64 = e->std64.p;
    HIP_TRY(launch_score_f32(e->d_tab, a, 0, s));
    HIP_TRY(launch_rescore_linear(a, s));
    if (out_mean) HIP_TRY(hipMemcpyAsync(out_mean, e->mean64.p, (size_t)n_seg * NMFCC * 8, hipMemcpyDeviceToHost, s));
    if (out_std) HIP_TRY(hipMemcpyAsync(out_std, e->std64.p, (size_t)n_seg * NMFCC * 8, hipMemcpyDeviceToHost, s));
    if (out_score && e->has_tmpl)
        HIP_TRY(hipMemcpyAsync(out_score, e->score.p, n_seg * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return EWK_OK;
}

int ewk_template_from_pcm(ewk_engine* e, const float* pcm, int64_t n) {
    if (!e || (!pcm && n > 0)) return fail(EWK_EINVAL, "NULL argument");
    if (n <= 0 || n > INT32_MAX) return fail(EWK_EINVAL, "template length must be in [1, 2^31)");
    const int64_t off = 0;
    const int32_t len = (int32_t)n;
    float m[NMFCC], sd[NMFCC];
    const bool had = e->has_tmpl;
    e->has_tmpl = false;   // compute stats only
    int rc = ewk_score_segments(e, pcm, n, &off, &len, 1, m, sd, nullptr, nullptr, EWK_SCORE_F32_CANDIDATES);
    e->has_tmpl = had;
    if (rc) return rc;
    return ewk_set_template(e, m, sd);
}

// ---------------------------------------------------------------- template bank
static_assert(sizeof(ewk_bank_result) == 24, "ewk_bank_result is 24 bytes (include/ewk.h)");
static const char* kNoBank = "No reference word set. Call set_bank() first.";
static const char* kStreamBankOn = "disable the stream bank first";

static int check_bank_layout(int32_t n_words, const int32_t* word_first) {
    if (n_words < 1) return fail(EWK_EINVAL, "a bank needs at least one word");
    if (n_words > EWK_BANK_MAX_TEMPLATES)
        return fail(EWK_EINVAL, "a bank holds at most " + std::to_string(EWK_BANK_MAX_TEMPLATES) + " templates");
    if (!word_first) return fail(EWK_EINVAL, "NULL argument");
    if (word_first[0] != 0) return fail(EWK_EINVAL, "word_first[0] must be 0");
    for (int32_t w = 0; w < n_words; ++w) {
        const int64_t sz = (int64_t)word_first[w + 1] - word_first[w];
        if (sz < 1 || sz > EWK_BANK_MAX_PER_WORD)
            return fail(EWK_EINVAL, "word " + std::to_string(w) + " has " + std::to_string(sz) +
                                        " templates (1.." + std::to_string(EWK_BANK_MAX_PER_WORD) + ")");
        if (word_first[w + 1] > EWK_BANK_MAX_TEMPLATES)
            return fail(EWK_EINVAL, "a bank holds at most " + std::to_string(EWK_BANK_MAX_TEMPLATES) + " templates");
    }
    return EWK_OK;
}

int ewk_bank_set(ewk_engine* e, int32_t n_words, const int32_t* word_first, const float* mean, const float* stdv,
                 const double* thresholds) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (e->sbank_on) return fail(EWK_EINVAL, kStreamBankOn);
    int rc = check_bank_layout(n_words, word_first);
    if (rc) return rc;
    if (!mean || !stdv) return fail(EWK_EINVAL, "NULL argument");
    if (thresholds)
        for (int32_t w = 0; w < n_words; ++w)
            if (!(thresholds[w] == thresholds[w])) return fail(EWK_EINVAL, "threshold is NaN");
    const int32_t K = word_first[n_words];
    std::vector<float> dev((size_t)K * kBankRow);
    int32_t max_word = 0;
    for (int32_t w = 0; w < n_words; ++w) {
        const int32_t f = word_first[w], s = word_first[w + 1] - f;
        max_word = std::max(max_word, s);
        float* base = dev.data() + (size_t)kBankRow * f;
        for (int32_t j = 0; j < s; ++j) {
            const float* m = mean + (size_t)(f + j) * NMFCC;
            const float* sd = stdv + (size_t)(f + j) * NMFCC;
            double am = 0.0, as = 0.0;   // the float32 self-dots, as ewk_set_template computes them
            for (int c = 0; c < NMFCC; ++c) {
                base[c * s + j] = m[c];
                base[(NMFCC + c) * s + j] = sd[c];
                const float pm = m[c] * m[c], ps = sd[c] * sd[c];
                am += (double)pm;
                as += (double)ps;
            }
            base[2 * NMFCC * s + j] = (float)am;
            base[(2 * NMFCC + 1) * s + j] = (float)as;
        }
    }
    std::vector<double> thr(n_words, e->cfg.similarity_threshold);
    if (thresholds) thr.assign(thresholds, thresholds + n_words);
    HIP_TRY(hipSetDevice(e->device));
    // a bank scoring call may still read the old bank (its fp64 pass is asynchronous)
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(e->d_bank.reserve(dev.size()));
    HIP_TRY(e->d_bank_first.reserve((size_t)n_words + 1));
    HIP_TRY(e->d_bank_thr.reserve(n_words));
    HIP_TRY(hipMemcpyAsync(e->d_bank.p, dev.data(), dev.size() * sizeof(float), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->d_bank_first.p, word_first, ((size_t)n_words + 1) * sizeof(int32_t),
                           hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->d_bank_thr.p, thr.data(), n_words * sizeof(double), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->bank_mean.assign(mean, mean + (size_t)K * NMFCC);
    e->bank_std.assign(stdv, stdv + (size_t)K * NMFCC);
    e->bank_first.assign(word_first, word_first + n_words + 1);
    e->bank_thr = thr;
    e->bank_thr_follow = thresholds == nullptr;
    e->bank_max_word = max_word;
    return EWK_OK;
}

int ewk_bank_from_pcm(ewk_engine* e, int32_t n_words, const int32_t* word_first, const float* pcm, int64_t n_pcm,
                      const int64_t* offsets, const int32_t* lengths, const double* thresholds) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (e->sbank_on) return fail(EWK_EINVAL, kStreamBankOn);
    int rc = check_bank_layout(n_words, word_first);
    if (rc) return rc;
    if (!pcm || !offsets || !lengths || n_pcm < 0) return fail(EWK_EINVAL, "NULL argument");
    const int32_t K = word_first[n_words];
    for (int32_t k = 0; k < K; ++k)
        if (lengths[k] < 1) return fail(EWK_EINVAL, "template length must be in [1, 2^31)");
    std::vector<float> m((size_t)K * NMFCC), sd((size_t)K * NMFCC);
    const bool had = e->has_tmpl;
    e->has_tmpl = false;   // compute stats only (as ewk_template_from_pcm)
    rc = ewk_score_segments(e, pcm, n_pcm, offsets, lengths, K, m.data(), sd.data(), nullptr, nullptr,
                            EWK_SCORE_F32_CANDIDATES);
    e->has_tmpl = had;
    if (rc) return rc;
    return ewk_bank_set(e, n_words, word_first, m.data(), sd.data(), thresholds);
}

int ewk_bank_clear(ewk_engine* e) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (e->sbank_on) return fail(EWK_EINVAL, kStreamBankOn);
    e->bank_first.clear();
    e->bank_mean.clear();
    e->bank_std.clear();
    e->bank_thr.clear();
    e->bank_max_word = 0;
    return EWK_OK;
}

int ewk_bank_info(ewk_engine* e, int32_t* n_words, int32_t* n_templates) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    const bool has = !e->bank_first.empty();
    if (n_words) *n_words = has ? (int32_t)e->bank_first.size() - 1 : 0;
    if (n_templates) *n_templates = has ? e->bank_first.back() : 0;
    return EWK_OK;
}

int ewk_bank_get(ewk_engine* e, int32_t tmpl, float* mean20, float* std20) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (e->bank_first.empty()) return fail(EWK_ENOTEMPLATE, kNoBank);
    if (tmpl < 0 || tmpl >= e->bank_first.back()) return fail(EWK_EINVAL, "template index out of range");
    if (mean20) memcpy(mean20, e->bank_mean.data() + (size_t)tmpl * NMFCC, NMFCC * sizeof(float));
    if (std20) memcpy(std20, e->bank_std.data() + (size_t)tmpl * NMFCC, NMFCC * sizeof(float));
    return EWK_OK;
}

// A bank set with NULL thresholds follows the engine's threshold as it stands at each scoring
// call: refresh the device copy on `s` when it moved (the only case that waits for `s`).
static int bank_follow_threshold(ewk_engine* e, hipStream_t s) {
    if (!e->bank_thr_follow || e->bank_thr[0] == e->cfg.similarity_threshold) return EWK_OK;
    std::fill(e->bank_thr.begin(), e->bank_thr.end(), e->cfg.similarity_threshold);
    HIP_TRY(hipMemcpyAsync(e->d_bank_thr.p, e->bank_thr.data(), e->bank_thr.size() * sizeof(double),
                           hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));   // (the copy reads bank_thr)
    return EWK_OK;
}

// What every bank pass takes from the engine's bank.
static BankArgs bank_args(ewk_engine* e) {
    BankArgs b;
    memset(&b, 0, sizeof(b));
    b.bank = e->d_bank.p;
    b.word_first = e->d_bank_first.p;
    b.thresholds = e->d_bank_thr.p;
    b.n_words = (int32_t)e->bank_first.size() - 1;
    b.max_word = e->bank_max_word;
    b.rescore_margin = e->cfg.rescore_margin;
    b.crit = rescore_criteria();
    return b;
}

// The three passes on `s` (device pointers): float32 statistics, bank scores + fp64 list,
// then -- after reading the list count back -- the fp64 statistics of the listed segments and
// their scores again.
static int bank_score(ewk_engine* e, const float* d_pcm, const int64_t* d_off, const int32_t* d_len, int32_t n,
                      const int32_t* d_word, ewk_bank_result* d_out, double* d_scores, int32_t stride, int32_t flags,
                      hipStream_t s) {
    HIP_TRY(reserve_rescore(e, n));
    HIP_TRY(e->mean.reserve((size_t)n * NMFCC));
    HIP_TRY(e->stdv.reserve((size_t)n * NMFCC));
    HIP_TRY(e->bk_cnt.reserve(1));
    HIP_TRY(e->bk_seg.reserve(n));
    HIP_TRY(e->bk_off.reserve(n));
    HIP_TRY(e->bk_len.reserve(n));
    HIP_TRY(join_scoring(e, s));
    {
        int rc = bank_follow_threshold(e, s);
        if (rc) return rc;
    }
    ScoreArgs a = base_args(e);
    a.has_template = 0;   // pass 1: statistics only, nothing listed
    a.rs_slots = nullptr;
    a.pcm = d_pcm;
    a.offsets = d_off;
    a.lengths = d_len;
    a.n_seg = n;
    a.out_mean = e->mean.p;
    a.out_std = e->stdv.p;
    {
        ProfScope ps(e, 0, s);
        HIP_TRY(launch_score_f32(e->d_tab, a, 0, s));
    }
    BankArgs b = bank_args(e);
    b.mean = e->mean.p;
    b.stdv = e->stdv.p;
    b.offsets = d_off;
    b.lengths = d_len;
    b.word = d_word;
    b.n = n;
    b.out = d_out;
    b.out_scores = d_scores;
    b.stride = stride;
    b.cand_f32 = (flags & EWK_SCORE_F32_CANDIDATES) ? 1 : 0;
    b.list_cnt = e->bk_cnt.p;
    b.list_seg = e->bk_seg.p;
    b.list_off = e->bk_off.p;
    b.list_len = e->bk_len.p;
    HIP_TRY(launch_bank_score(b, s));
    int32_t listed = 0;
    HIP_TRY(hipMemcpyAsync(&listed, e->bk_cnt.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (listed <= 0) return EWK_OK;
    if (listed > n) return fail(EWK_EHIP, "bank list count out of range");
    HIP_TRY(e->mean64.reserve((size_t)listed * NMFCC));
    HIP_TRY(e->std64.reserve((size_t)listed * NMFCC));
    // pass 3: the listed segments through the fp64 path (list_all, as ewk_score_segments_f64)
    ScoreArgs f = base_args(e);
    f.has_template = 0;
    f.pcm = d_pcm;
    f.offsets = e->bk_off.p;
    f.lengths = e->bk_len.p;
    f.n_seg = listed;
    f.list_all = 1;
    f.rs_slots = e->rs_slots.p;
    f.out_mean64 = e->mean64.p;
    f.out_std64 = e->std64.p;
    {
        ProfScope ps(e, 1, s);
        HIP_TRY(launch_score_f32(e->d_tab, f, 0, s));
        HIP_TRY(launch_rescore_linear(f, s));
    }
    b.mean = e->mean64.p;
    b.stdv = e->std64.p;
    b.n = listed;
    HIP_TRY(launch_bank_rescore(b, s));
    return EWK_OK;
}

static int check_bank_call(ewk_engine* e, int32_t n_seg, const void* out, const double* out_scores, int32_t stride) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (n_seg < 0) return fail(EWK_EINVAL, "n_seg must be >= 0");
    if (e->bank_first.empty()) return fail(EWK_ENOTEMPLATE, kNoBank);
    if (n_seg > 0 && !out) return fail(EWK_EINVAL, "NULL argument");
    if (out_scores && stride < e->bank_max_word)
        return fail(EWK_EINVAL, "stride " + std::to_string(stride) + " is smaller than the bank's largest word (" +
                                    std::to_string(e->bank_max_word) + ")");
    return EWK_OK;
}

int ewk_score_segments_bank_device(ewk_engine* e, const float* d_pcm, const int64_t* d_offsets,
                                   const int32_t* d_lengths, int32_t n_seg, const int32_t* d_word,
                                   ewk_bank_result* d_out, double* d_out_scores, int32_t stride, int32_t flags,
                                   void* stream) {
    int rc = check_bank_call(e, n_seg, d_out, d_out_scores, stride);
    if (rc) return rc;
    if (n_seg == 0) return EWK_OK;
    if (!d_pcm || !d_offsets || !d_lengths) return fail(EWK_EINVAL, "NULL device pointer");
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = stream ? (hipStream_t)stream : e->stream;
    return bank_score(e, d_pcm, d_offsets, d_lengths, n_seg, d_word, d_out, d_out_scores, stride, flags, s);
}

int ewk_score_segments_bank(ewk_engine* e, const float* pcm, int64_t n_pcm, const int64_t* offsets,
                            const int32_t* lengths, int32_t n_seg, const int32_t* word, ewk_bank_result* out,
                            double* out_scores, int32_t stride, int32_t flags) {
    int rc = check_bank_call(e, n_seg, out, out_scores, stride);
    if (rc) return rc;
    if (n_pcm < 0) return fail(EWK_EINVAL, "negative size");
    if (n_seg == 0) return EWK_OK;
    if (!offsets || !lengths || (n_pcm > 0 && !pcm)) return fail(EWK_EINVAL, "NULL argument");
    int32_t max_len = 0;
    rc = check_segments(offsets, lengths, n_seg, n_pcm, &max_len);
    if (rc) return rc;
    const int32_t n_words = (int32_t)e->bank_first.size() - 1;
    if (word)
        for (int32_t i = 0; i < n_seg; ++i)
            if (word[i] < 0 || word[i] >= n_words)
                return fail(EWK_EINVAL, "word index " + std::to_string(word[i]) + " of segment " + std::to_string(i) +
                                            " is outside [0, " + std::to_string(n_words) + ")");
    HIP_TRY(hipSetDevice(e->device));
    const size_t n_sc = out_scores ? (size_t)n_seg * stride : 0;
    HIP_TRY(e->pcm.reserve(std::max<int64_t>(n_pcm, 1)));
    HIP_TRY(e->offsets.reserve(n_seg));
    HIP_TRY(e->lengths.reserve(n_seg));
    HIP_TRY(e->bk_word.reserve(n_seg));
    HIP_TRY(e->bk_out.reserve(n_seg));
    if (n_sc) HIP_TRY(e->bk_scores.reserve(n_sc));
    hipStream_t s = e->stream;
    HIP_TRY(join_scoring(e, s));
    if (n_pcm > 0) HIP_TRY(hipMemcpyAsync(e->pcm.p, pcm, n_pcm * sizeof(float), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(e->offsets.p, offsets, n_seg * sizeof(int64_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(e->lengths.p, lengths, n_seg * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (word) HIP_TRY(hipMemcpyAsync(e->bk_word.p, word, n_seg * sizeof(int32_t), hipMemcpyHostToDevice, s));
    rc = bank_score(e, e->pcm.p, e->offsets.p, e->lengths.p, n_seg, word ? e->bk_word.p : nullptr, e->bk_out.p,
                    n_sc ? e->bk_scores.p : nullptr, stride, flags, s);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out, e->bk_out.p, n_seg * sizeof(ewk_bank_result), hipMemcpyDeviceToHost, s));
    if (n_sc) HIP_TRY(hipMemcpyAsync(out_scores, e->bk_scores.p, n_sc * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return EWK_OK;
}

// ---------------------------------------------------------------- streaming path
int ewk_reset_streams(ewk_engine* e) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (e->n_streams <= 0) return EWK_OK;
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    HIP_TRY(join_scoring(e, s));
#ifndef EWK_RING_MEMSET
    HIP_TRY(launch_ring_zero(e->d_ring, (size_t)e->n_streams * e->sring_len * e->ring_es, s));
#else   // (the round-6 fill, kept for the A/B of scripts/gpu_miss_prefix.sh)
    HIP_TRY(hipMemsetAsync(e->d_ring, 0, (size_t)e->n_streams * e->sring_len * e->ring_es, s));
#endif
    HIP_TRY(hipMemsetAsync(e->d_brms, 0, (size_t)e->n_streams * std::max(1, e->n_blocks) * sizeof(double), s));
    std::vector<GateStream> st(e->n_streams);
    for (auto& x : st) {
        memset(&x, 0, sizeof(x));
        x.threshold = e->cfg.initial_threshold;
        x.last_silent = 1;
    }
    HIP_TRY(hipMemcpyAsync(e->d_st, st.data(), st.size() * sizeof(GateStream), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(e->d_work, 0, kWorkInts * sizeof(int32_t), s));
    // (a stream bank stays enabled; its list of events to re-score starts empty)
    if (e->sb_list.p) HIP_TRY(hipMemsetAsync(e->sb_list.p, 0, kEvListHdr * sizeof(int32_t), s));
    // (an input rate stays set; the resampler's history starts from silence again)
    if (e->rs_hist.p) HIP_TRY(hipMemsetAsync(e->rs_hist.p, 0, e->rs_hist.cap * sizeof(float), s));
    if (e->rs_flags.p) HIP_TRY(hipMemsetAsync(e->rs_flags.p, 1, e->rs_flags.cap, s));
    e->rs_fresh = true;
    zero_event_state(e);
    HIP_TRY(hipStreamSynchronize(s));
    e->tick = 0;
    e->desync = false;   // one clock again
    std::vector<int64_t>().swap(e->tick_delta);
    return EWK_OK;
}

// ---- stream lifecycle: index lists --------------------------------------------------
// An index list as every call that takes one requires it: 1 <= n <= n_streams, every entry a
// stream, none twice (two waves would run one stream).  Host only; changes nothing but `seen`.
static int check_stream_list(ewk_engine* e, const int32_t* streams, int32_t n) {
    if (!streams) return fail(EWK_EINVAL, "streams is NULL");
    if (n < 1 || n > e->n_streams)
        return fail(EWK_EINVAL, "a stream list holds 1.." + std::to_string(e->n_streams) + " streams, got " +
                                    std::to_string(n));
    if (e->seen.empty()) e->seen.assign((size_t)e->n_streams, 0);
    if (++e->seen_epoch == 0) {   // (wrapped: forget every earlier call)
        std::fill(e->seen.begin(), e->seen.end(), 0);
        e->seen_epoch = 1;
    }
    for (int32_t i = 0; i < n; ++i) {
        const int32_t s = streams[i];
        if (s < 0 || s >= e->n_streams)
            return fail(EWK_EINVAL, "streams[" + std::to_string(i) + "] = " + std::to_string(s) + " is outside [0, " +
                                        std::to_string(e->n_streams) + ")");
        if (e->seen[s] == e->seen_epoch)
            return fail(EWK_EINVAL, "streams[" + std::to_string(i) + "]: stream " + std::to_string(s) +
                                        " is listed twice");
        e->seen[s] = e->seen_epoch;
    }
    return EWK_OK;
}

// The list (and `vals`, one per entry, when given) to the device on s through pinned staging:
// the caller's arrays may die on return.  *d_list / *d_vals: where kernels enqueued on s after
// this call find them, until the next call.
static int stage_stream_list(ewk_engine* e, const int32_t* streams, const int32_t* vals, int32_t n, hipStream_t s,
                             const int32_t** d_list, const int32_t** d_vals) {
    const size_t cap = 2 * (size_t)e->n_streams;
    if (!e->h_ids) {
        HIP_TRY(hipHostMalloc((void**)&e->h_ids, cap * sizeof(int32_t), hipHostMallocDefault));
        HIP_TRY(hipEventCreateWithFlags(&e->h_ids_free, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(e->h_ids_free, s));
    }
    HIP_TRY(e->d_ids.reserve(cap));
    HIP_TRY(hipEventSynchronize(e->h_ids_free));   // the previous list has left the staging
    memcpy(e->h_ids, streams, (size_t)n * sizeof(int32_t));
    if (vals) memcpy(e->h_ids + e->n_streams, vals, (size_t)n * sizeof(int32_t));
    HIP_TRY(hipMemcpyAsync(e->d_ids.p, e->h_ids, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (vals)
        HIP_TRY(hipMemcpyAsync(e->d_ids.p + e->n_streams, e->h_ids + e->n_streams, (size_t)n * sizeof(int32_t),
                               hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(e->h_ids_free, s));
    *d_list = e->d_ids.p;
    if (d_vals) *d_vals = e->d_ids.p + e->n_streams;
    return EWK_OK;
}

// First subset push or list reset: every stream gets a clock of its own.  With a rate set, also
// the per-stream fresh flags, from the engine-wide one.
static int desynchronise(ewk_engine* e, hipStream_t s) {
    if (!e->desync) {
        e->tick_delta.assign((size_t)e->n_streams, 0);
        e->desync = true;
    }
    if (e->rs_on && !e->rs_flags.p) {
        HIP_TRY(e->rs_flags.reserve((size_t)e->n_streams));
        HIP_TRY(hipMemsetAsync(e->rs_flags.p, e->rs_fresh ? 1 : 0, e->rs_flags.cap, s));
    }
    return EWK_OK;
}

// Score the events queued since the last scoring pass (ring mode), then advance the watermark.
// Score the current bank's events [ev_base, *n_events) on stream ss; n_events is the
// live counter (same stream as the gate) or a snapshot of it taken after the gate.
static int score_pending_bank(ewk_engine* e, hipStream_t ss, const int32_t* n_events);

static int score_pending(ewk_engine* e, hipStream_t ss, const int32_t* n_events) {
    if (e->sbank_on) return score_pending_bank(e, ss, n_events);   // (needs no single template)
    if (!e->has_tmpl) return EWK_OK;   // events keep NaN scores until a template exists
    ScoreArgs a = base_args(e);
    a.pcm = e->ring_f32();
    a.pcm16 = e->ring_i16();
    a.ring_len = e->sring_len;
    a.events = e->ev_bank(e->bank);
    a.n_events = n_events;
    a.ev_base = e->evc_bank(e->bank) + 2;
    a.ev_base0 = e->ev_base0[e->bank];
    a.n_seg = e->ev_cap;
    a.work = e->d_work + 1;            // ring-mode counters (zeroed at create, re-armed by the tick end)
    a.rs_ctl = e->d_work + 16;
    // k_rescore_ring (after the scorer) re-scores the listed segments in fp64 and its last
    // workgroup out advances the watermark and writes the poll mirror
    a.adv_ev_base = e->evc_bank(e->bank) + 2;
    HIP_TRY(ensure_poll_region(e));
    a.mirror = e->d_poll + e->bank * kPollRegion;
    a.evc = e->evc_bank(e->bank);
    a.mirror_chunk = std::min<int32_t>(kPollChunk, e->ev_cap);
    {
        ProfScope ps(e, 0, ss);
        HIP_TRY(launch_score_f32(e->d_tab, a, e->n_streams >= kRingWaveStreams ? 2 : 1, ss));
    }
    {
        ProfScope ps(e, 1, ss);
        HIP_TRY(launch_rescore_ring(a, ss));
    }
    return EWK_OK;
}

// Workgroups of the stream bank's event passes: the waves stride over the pending events, so
// the grid follows the engine's size (an empty tick only pays for reading the counters).
static int32_t stream_bank_grid(const ewk_engine* e) {
    return std::min(1024, std::max(8, (e->n_streams + 255) / 256));
}

// The same pass with the stream bank enabled, all on ss, every hand-off a kernel boundary:
//   1 the ring scorer without a template: float32 statistics and theta_s by event slot
//   2 k_bank_events<float>: every pending event against its stream's word; lists the events the
//     float32 statistics cannot decide (re-score slots + sb_list)
//   3 the re-score launch: fp64 statistics of the listed events; ends the tick (counters,
//     watermark) without the poll mirror -- pass 4 still changes events
//   4 k_bank_events<double>: the listed events again from the fp64 statistics
// push_impl writes the poll mirror behind the push's last pass.
static int score_pending_bank(ewk_engine* e, hipStream_t ss, const int32_t* n_events) {
    {
        int rc = bank_follow_threshold(e, ss);
        if (rc) return rc;
    }
    ScoreArgs a = base_args(e);
    a.has_template = 0;
    a.pcm = e->ring_f32();
    a.pcm16 = e->ring_i16();
    a.ring_len = e->sring_len;
    a.events = e->ev_bank(e->bank);
    a.n_events = n_events;
    a.ev_base = e->evc_bank(e->bank) + 2;
    a.ev_base0 = e->ev_base0[e->bank];
    a.n_seg = e->ev_cap;
    a.work = e->d_work + 1;
    a.rs_ctl = e->d_work + 16;
    a.rs_slots = e->rs_slots.p;
    a.adv_ev_base = e->evc_bank(e->bank) + 2;
    a.out_mean = e->sb_mean.p;
    a.out_std = e->sb_std.p;
    a.out_theta = e->sb_theta.p;
    a.out_mean64 = e->sb_mean64.p;
    a.out_std64 = e->sb_std64.p;
    a.evc = e->evc_bank(e->bank);
    BankArgs b = bank_args(e);
    BankEvArgs x;
    x.stream_word = e->sbank_words ? e->sb_word.p : nullptr;
    x.ev_list = e->sb_list.p;
    x.grid = stream_bank_grid(e);
    {
        ProfScope ps(e, 0, ss);
        HIP_TRY(launch_score_f32(e->d_tab, a, e->n_streams >= kRingWaveStreams ? 2 : 1, ss));
    }
    b.mean = e->sb_mean.p;
    b.stdv = e->sb_std.p;
    HIP_TRY(launch_bank_events(b, a, x, ss));
    {
        ProfScope ps(e, 1, ss);
        HIP_TRY(launch_rescore_ring(a, ss));
    }
    b.mean = e->sb_mean64.p;
    b.stdv = e->sb_std64.p;
    HIP_TRY(launch_bank_events_rescore(b, a, x, ss));
    return EWK_OK;
}

int ewk_stream_bank_enable(ewk_engine* e, const int32_t* stream_word) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (e->n_streams <= 0) return fail(EWK_EINVAL, "engine has no streams");
    if (e->bank_first.empty()) return fail(EWK_ENOTEMPLATE, kNoBank);
    const int32_t n_words = (int32_t)e->bank_first.size() - 1;
    if (stream_word)
        for (int32_t s = 0; s < e->n_streams; ++s)
            if (stream_word[s] < 0 || stream_word[s] >= n_words)
                return fail(EWK_EINVAL, "word index " + std::to_string(stream_word[s]) + " of stream " +
                                            std::to_string(s) + " is outside [0, " + std::to_string(n_words) + ")");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));    // the pushes so far keep their scoring
    HIP_TRY(hipStreamSynchronize(e->sstream));
    const size_t cap = (size_t)e->ev_cap;
    const bool fresh = e->sb_list.p == nullptr;
    HIP_TRY(e->sb_mean.reserve(cap * NMFCC));
    HIP_TRY(e->sb_std.reserve(cap * NMFCC));
    HIP_TRY(e->sb_theta.reserve(cap));
    HIP_TRY(e->sb_mean64.reserve(cap * NMFCC));
    HIP_TRY(e->sb_std64.reserve(cap * NMFCC));
    HIP_TRY(e->sb_list.reserve(kEvListHdr + cap));
    if (fresh) HIP_TRY(hipMemset(e->sb_list.p, 0, kEvListHdr * sizeof(int32_t)));
    if (stream_word) {
        HIP_TRY(e->sb_word.reserve((size_t)e->n_streams));
        HIP_TRY(hipMemcpy(e->sb_word.p, stream_word, (size_t)e->n_streams * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    e->sbank_words = stream_word != nullptr;
    e->sbank_on = true;
    return EWK_OK;
}

int ewk_stream_bank_disable(ewk_engine* e) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (!e->sbank_on) return EWK_OK;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipStreamSynchronize(e->sstream));
    e->sbank_on = false;
    return EWK_OK;
}

// streams == nullptr: a tick for every stream (row s of pcm is stream s); else rows 0..n_list-1
// are the ticks of streams[0..n_list) (ewk_push_streams).
static int push_impl(ewk_engine* e, const void* pcm_any, int64_t stride, int64_t tick_stride, int32_t n_ticks,
                     int32_t flags, bool pcm16, const int32_t* streams = nullptr, int32_t n_list = 0) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (e->n_streams <= 0) return fail(EWK_EINVAL, "engine has no streams");
    if (streams || n_list) {   // (validated before anything is enqueued or changed)
        int rc = check_stream_list(e, streams, n_list);
        if (rc) return rc;
    }
    const int32_t rows = streams ? n_list : e->n_streams;
    if (!pcm_any) return fail(EWK_EINVAL, "pcm is NULL");
    if (n_ticks <= 0) return fail(EWK_EINVAL, "n_ticks must be positive");
    if (!pcm16 && e->ring_es == sizeof(int16_t))
        return fail(EWK_EINVAL, "an int16 ring (EWK_RING_I16) takes PCM16 pushes (ewk_push_pcm16)");
    const size_t es = pcm16 ? sizeof(int16_t) : sizeof(float);
    const unsigned char* pcm = static_cast<const unsigned char*>(pcm_any);
    // with an input rate set (ewk_set_input_rate) a tick is in_block samples at that rate
    const int64_t in_block = e->rs_on ? e->rs_in_block : e->cfg.block;
    if (stride < in_block && rows > 1)
        return fail(EWK_EINVAL, e->rs_on ? "stride must be >= the input block (ewk_input_rate_info)" : "stride must be >= block");
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    const void* src = pcm_any;
    int64_t st_stride = stride, tk_stride = tick_stride;
    const int32_t* d_list = nullptr;
    if (streams) {
        int rc = desynchronise(e, s);
        if (rc) return rc;
        rc = stage_stream_list(e, streams, nullptr, n_list, s, &d_list, nullptr);
        if (rc) return rc;
    }
    if (!(flags & EWK_PUSH_DEVICE)) {
        // Gather the caller's (pageable) blocks into pinned staging on the CPU, then
        // DMA asynchronously: the caller's buffer may die as soon as we return.
        const size_t per_stream = (size_t)n_ticks * in_block;
        const size_t total = per_stream * rows;
        if (e->h_stage_free) HIP_TRY(hipEventSynchronize(e->h_stage_free));   // previous DMA done
        if (total > e->h_stage_cap) {
            if (e->h_stage) HIP_TRY(hipHostFree(e->h_stage));
            e->h_stage = nullptr;
            e->h_stage_cap = 0;
            HIP_TRY(hipHostMalloc((void**)&e->h_stage, total * sizeof(float), hipHostMallocDefault));   // >= es bytes each
            e->h_stage_cap = total;
        }
        if (!e->h_stage_free) HIP_TRY(hipEventCreateWithFlags(&e->h_stage_free, hipEventDisableTiming));
        for (int32_t st = 0; st < rows; ++st)
            for (int32_t t = 0; t < n_ticks; ++t)
                memcpy(reinterpret_cast<unsigned char*>(e->h_stage) + ((size_t)st * per_stream + (size_t)t * in_block) * es,
                       pcm + ((size_t)st * stride + (size_t)t * tick_stride) * es, in_block * es);
        HIP_TRY(e->push_stage.reserve(total));
        HIP_TRY(hipMemcpyAsync(e->push_stage.p, e->h_stage, total * es, hipMemcpyHostToDevice, s));
        HIP_TRY(hipEventRecord(e->h_stage_free, s));
        src = e->push_stage.p;
        st_stride = (int64_t)per_stream;
        tk_stride = in_block;
    }
    if (e->rs_on) {
        // resample every tick of the push into rs_out, save the history for the next push, and
        // hand the gate float32 16 kHz blocks
        const ewk_engine::RsFilter& f = e->rs_in;
        const size_t per_stream = (size_t)n_ticks * e->cfg.block;
        if (per_stream * rows > e->rs_out.cap) {
            HIP_TRY(hipStreamSynchronize(s));   // an earlier gate launch may still read the old buffer
            HIP_TRY(e->rs_out.reserve(per_stream * rows));
        }
        ResampleArgs r;
        memset(&r, 0, sizeof(r));
        if (pcm16) r.in16 = static_cast<const int16_t*>(src);
        else r.in = static_cast<const float*>(src);
        r.stride = st_stride;
        r.tick_stride = tk_stride;
        r.in_block = in_block;
        r.n_in = (int64_t)n_ticks * in_block;
        r.hist = e->rs_hist.p;
        r.out = e->rs_out.p;
        r.out_stride = (int64_t)per_stream;
        r.n_out = (int64_t)per_stream;
        r.rows = rows;
        r.ids = d_list;
        r.fresh = e->rs_flags.p;   // per stream once there are flags, else rs_fresh for all
        r.taps = f.taps.p;
        r.up = f.up;
        r.down = f.down;
        r.J = f.J;
        r.H = f.H;
        r.c0 = f.c0;
        r.n_zero = (e->rs_flags.p || e->rs_fresh) ? e->rs_delay : 0;
        r.threads = f.threads;
        r.span = f.span;
        {
            ProfScope ps(e, 3, s);
            HIP_TRY(launch_resample(r, s));
            HIP_TRY(launch_resample_save(r, e->rs_hist.p, e->rs_flags.p, s));
        }
        if (!streams) e->rs_fresh = false;   // (a subset push made the flags: rs_fresh is not read again)
        src = e->rs_out.p;
        st_stride = (int64_t)per_stream;
        tk_stride = e->cfg.block;
        pcm16 = false;
    }
    // Segments must be scored before the ring overwrites them: <= ticks_per_launch ticks per gate launch.
    for (int32_t t0 = 0; t0 < n_ticks; t0 += e->ticks_per_launch) {
        const int32_t nt = std::min<int32_t>(e->ticks_per_launch, n_ticks - t0);
        GateArgs g;
        memset(&g, 0, sizeof(g));
        if (pcm16) g.pcm16 = static_cast<const int16_t*>(src) + (int64_t)t0 * tk_stride;
        else g.pcm = static_cast<const float*>(src) + (int64_t)t0 * tk_stride;
        g.stride = st_stride;
        g.tick_stride = tk_stride;
        g.n_ticks = nt;
        g.n_streams = rows;
        g.ids = d_list;
        g.own_clock = e->desync ? 1 : 0;
        g.tick0 = e->tick;
        g.ring = e->ring_f32();
        g.ring16 = e->ring_i16();
        g.ring_len = e->ring_len;
        g.sring_len = e->sring_len;
        g.compact = e->sring_len < e->ring_len ? 1 : 0;
        g.block_rms = e->d_brms;
        g.sorted_rms = e->d_sorted;
        g.trees = e->d_trees;
        g.st = e->d_st;
        g.block = e->cfg.block;
        g.n_blocks = e->n_blocks;
        g.n_last = e->n_last;
        g.sample_rate = e->cfg.sample_rate;
        g.stage = e->gate_stage;
        g.val_len = e->gate_val_len;
        g.tick_seconds = e->cfg.tick_seconds;
        g.pre_speech_silence = e->cfg.pre_speech_silence;
        g.speech_duration_min = e->cfg.speech_duration_min;
        g.speech_duration_max = e->cfg.speech_duration_max;
        g.post_speech_silence = e->cfg.post_speech_silence;
        g.padding = e->cfg.padding;
        g.max_segment_seconds = e->cfg.max_segment_seconds;
        g.reentry_timeout = e->cfg.reentry_timeout;
        g.min_threshold = e->cfg.min_threshold;
        g.events = e->ev_bank(e->bank);
        g.ev_count = e->evc_bank(e->bank);
        g.ev_dropped = e->evc_bank(e->bank) + 1;
        g.ev_cap = e->ev_cap;
        g.ev_base0 = e->ev_base0[e->bank];
        const int k = (int)(e->push_seq & 1);
        // the scoring pass two launches back must be done: it read snapshot slot k, and
        // at most one pass runs beside a gate
        if (e->overlap && e->score_live[k]) HIP_TRY(hipStreamWaitEvent(s, e->score_evt[k], 0));
        {
            ProfScope ps(e, 2, s);
            HIP_TRY(launch_gate(g, s));
        }
        if (!streams) e->tick += nt;
        else for (int32_t i = 0; i < n_list; ++i) e->tick_delta[streams[i]] += nt;
        if (e->overlap) {
            int32_t* snap = e->d_work + 4 + k;
            HIP_TRY(launch_snapshot(e->evc_bank(e->bank), snap, s));
            HIP_TRY(hipEventRecord(e->gate_evt[k], s));
            HIP_TRY(hipStreamWaitEvent(e->sstream, e->gate_evt[k], 0));
            int rc = score_pending(e, e->sstream, snap);
            if (rc) return rc;
            HIP_TRY(hipEventRecord(e->score_evt[k], e->sstream));
            e->score_live[k] = true;
            e->score_tail = e->score_evt[k];
        } else {
            int rc = score_pending(e, s, e->evc_bank(e->bank));
            if (rc) return rc;
        }
        e->push_seq += 1;
    }
    // the poll mirror of this bank: written by the last scoring pass's tick end, or by
    // k_bank_mirror: behind the gate (no template yet: no scoring pass), or behind the stream
    // bank's last pass (its fp64 pass changes events after the tick end)
    if (e->sbank_on || !e->has_tmpl) {
        hipStream_t ms = e->overlap ? e->sstream : s;
        HIP_TRY(ensure_poll_region(e));
        HIP_TRY(launch_bank_mirror(e->evc_bank(e->bank), e->ev_bank(e->bank), e->ev_base0[e->bank], e->ev_cap,
                                   std::min<int32_t>(kPollChunk, e->ev_cap), e->d_poll + e->bank * kPollRegion, ms));
    }
    e->mirror[e->bank] = true;
    HIP_TRY(hipEventRecord(e->bank_done[e->bank], e->overlap ? e->sstream : s));
    e->bank_used[e->bank] = true;
    return EWK_OK;
}

int ewk_push(ewk_engine* e, const float* pcm, int64_t stride, int32_t flags) {
    return push_impl(e, pcm, stride, 0, 1, flags, false);
}

int ewk_push_many(ewk_engine* e, const float* pcm, int64_t stride, int64_t tick_stride, int32_t n_ticks,
                  int32_t flags) {
    return push_impl(e, pcm, stride, tick_stride, n_ticks, flags, false);
}

int ewk_push_pcm16(ewk_engine* e, const int16_t* pcm, int64_t stride, int32_t flags) {
    return push_impl(e, pcm, stride, 0, 1, flags, true);
}

int ewk_push_many_pcm16(ewk_engine* e, const int16_t* pcm, int64_t stride, int64_t tick_stride, int32_t n_ticks,
                        int32_t flags) {
    return push_impl(e, pcm, stride, tick_stride, n_ticks, flags, true);
}

// ---------------------------------------------------------------- stream lifecycle
int ewk_push_streams(ewk_engine* e, const int32_t* streams, int32_t n, const float* pcm, int64_t stride,
                     int64_t tick_stride, int32_t n_ticks, int32_t flags) {
    if (e && !streams) return fail(EWK_EINVAL, "streams is NULL");
    return push_impl(e, pcm, stride, tick_stride, n_ticks, flags, false, streams, n);
}

int ewk_push_streams_pcm16(ewk_engine* e, const int32_t* streams, int32_t n, const int16_t* pcm, int64_t stride,
                           int64_t tick_stride, int32_t n_ticks, int32_t flags) {
    if (e && !streams) return fail(EWK_EINVAL, "streams is NULL");
    return push_impl(e, pcm, stride, tick_stride, n_ticks, flags, true, streams, n);
}

int ewk_reset_stream_list(ewk_engine* e, const int32_t* streams, int32_t n) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (e->n_streams <= 0) return fail(EWK_EINVAL, "engine has no streams");
    int rc = check_stream_list(e, streams, n);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    HIP_TRY(join_scoring(e, s));   // (overlap mode: the scorer may still read these ring rows)
    rc = desynchronise(e, s);
    if (rc) return rc;
    ResetListArgs a;
    memset(&a, 0, sizeof(a));
    rc = stage_stream_list(e, streams, nullptr, n, s, &a.ids, nullptr);
    if (rc) return rc;
    a.n = n;
    a.ring = static_cast<unsigned char*>(e->d_ring);
    a.row_bytes = e->sring_len * (int64_t)e->ring_es;
    a.block_rms = e->d_brms;
    a.n_blocks = e->n_blocks;
    a.st = e->d_st;
    a.init_threshold = e->cfg.initial_threshold;
    if (e->rs_on) {   // (a rate set earlier and switched off again: set_input_rate clears every row)
        a.hist = e->rs_hist.p;
        a.H = e->rs_in.H;
        a.fresh = e->rs_flags.p;
    }
    HIP_TRY(launch_reset_list(a, s));
    for (int32_t i = 0; i < n; ++i) e->tick_delta[streams[i]] = -e->tick;
    return EWK_OK;
}

int ewk_stream_ticks(ewk_engine* e, const int32_t* streams, int32_t n, int64_t* out) {
    if (!e || !out) return fail(EWK_EINVAL, "NULL argument");
    if (n < 0 || n > e->n_streams)
        return fail(EWK_EINVAL, "n must be in [0, " + std::to_string(e->n_streams) + "]");
    for (int32_t i = 0; i < n; ++i) {
        const int32_t s = streams ? streams[i] : i;
        if (s < 0 || s >= e->n_streams)
            return fail(EWK_EINVAL, "streams[" + std::to_string(i) + "] = " + std::to_string(s) + " is outside [0, " +
                                        std::to_string(e->n_streams) + ")");
    }
    for (int32_t i = 0; i < n; ++i) out[i] = e->stream_tick(streams ? streams[i] : i);
    return EWK_OK;
}

int ewk_stream_bank_assign(ewk_engine* e, const int32_t* streams, int32_t n, const int32_t* words) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (!e->sbank_on) return fail(EWK_EINVAL, "the stream bank is off (ewk_stream_bank_enable)");
    int rc = check_stream_list(e, streams, n);
    if (rc) return rc;
    if (!words) return fail(EWK_EINVAL, "words is NULL");
    const int32_t n_words = (int32_t)e->bank_first.size() - 1;
    for (int32_t i = 0; i < n; ++i)
        if (words[i] < 0 || words[i] >= n_words)
            return fail(EWK_EINVAL, "word index " + std::to_string(words[i]) + " of stream " +
                                        std::to_string(streams[i]) + " is outside [0, " + std::to_string(n_words) + ")");
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    HIP_TRY(join_scoring(e, s));   // (overlap mode: a scoring pass in flight still reads the words)
    if (!e->sbank_words) {   // enabled with word 0 for every stream: the array, all zeros
        HIP_TRY(e->sb_word.reserve((size_t)e->n_streams));
        HIP_TRY(hipMemsetAsync(e->sb_word.p, 0, (size_t)e->n_streams * sizeof(int32_t), s));
        e->sbank_words = true;
    }
    const int32_t *d_list = nullptr, *d_vals = nullptr;
    rc = stage_stream_list(e, streams, words, n, s, &d_list, &d_vals);
    if (rc) return rc;
    HIP_TRY(launch_scatter_i32(e->sb_word.p, d_list, d_vals, n, s));
    return EWK_OK;
}

// ---------------------------------------------------------------- level-3 input / PCM16 decode
static int normalize_impl(ewk_engine* e, const float* d_pcm, const int64_t* offsets, const int32_t* lengths,
                          const ewk_event* events, int32_t n, double* out, int32_t flags) {
    hipStream_t s = e->stream;
    HIP_TRY(join_scoring(e, s));
    std::vector<int64_t> oo(n);
    int64_t total = 0;
    for (int32_t i = 0; i < n; ++i) {
        const int32_t len = events ? events[i].length : lengths[i];
        if (len < 0) return fail(EWK_EINVAL, "negative segment length");
        oo[i] = total;
        total += len;
    }
    TmpBuf<int64_t> d_oo, d_off;
    TmpBuf<int32_t> d_len;
    TmpBuf<ewk_event> d_ev;
    TmpBuf<double> d_out;
    HIP_TRY(d_oo.reserve(std::max<int32_t>(1, n)));
    HIP_TRY(hipMemcpyAsync(d_oo.p, oo.data(), n * sizeof(int64_t), hipMemcpyHostToDevice, s));
    L3Args a;
    memset(&a, 0, sizeof(a));
    a.n = n;
    a.out_offsets = d_oo.p;
    if (events) {
        HIP_TRY(d_ev.reserve(std::max<int32_t>(1, n)));
        HIP_TRY(hipMemcpyAsync(d_ev.p, events, n * sizeof(ewk_event), hipMemcpyHostToDevice, s));
        a.events = d_ev.p;
        a.pcm = e->ring_f32();
        a.pcm16 = e->ring_i16();
        a.ring_len = e->sring_len;
    } else {
        HIP_TRY(d_off.reserve(std::max<int32_t>(1, n)));
        HIP_TRY(d_len.reserve(std::max<int32_t>(1, n)));
        HIP_TRY(hipMemcpyAsync(d_off.p, offsets, n * sizeof(int64_t), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_len.p, lengths, n * sizeof(int32_t), hipMemcpyHostToDevice, s));
        a.pcm = d_pcm;
        a.offsets = d_off.p;
        a.lengths = d_len.p;
    }
    if (flags & EWK_OUT_DEVICE) {
        a.out = out;
    } else {
        HIP_TRY(d_out.reserve(std::max<int64_t>(1, total)));
        a.out = d_out.p;
    }
    HIP_TRY(launch_normalize(a, s));
    if (!(flags & EWK_OUT_DEVICE) && total > 0)
        HIP_TRY(hipMemcpyAsync(out, d_out.p, total * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return EWK_OK;
}

int ewk_normalize_segments(ewk_engine* e, const float* pcm, int64_t n_pcm, const int64_t* offsets,
                           const int32_t* lengths, int32_t n_seg, double* out, int32_t flags) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (n_seg < 0 || n_pcm < 0) return fail(EWK_EINVAL, "negative size");
    if (n_seg == 0) return EWK_OK;
    if (!pcm || !offsets || !lengths || !out) return fail(EWK_EINVAL, "NULL argument");
    for (int32_t i = 0; i < n_seg; ++i)
        if (offsets[i] < 0 || lengths[i] < 0 || offsets[i] + lengths[i] > n_pcm)
            return fail(EWK_EINVAL, "segment " + std::to_string(i) + " outside pcm");
    HIP_TRY(hipSetDevice(e->device));
    const float* d_pcm = pcm;
    TmpBuf<float> tmp;
    if (!(flags & EWK_PCM_DEVICE)) {
        HIP_TRY(tmp.reserve(std::max<int64_t>(1, n_pcm)));
        HIP_TRY(hipMemcpyAsync(tmp.p, pcm, n_pcm * sizeof(float), hipMemcpyHostToDevice, e->stream));
        d_pcm = tmp.p;
    }
    return normalize_impl(e, d_pcm, offsets, lengths, nullptr, n_seg, out, flags);
}

int ewk_normalize_events(ewk_engine* e, const ewk_event* events, int32_t n, double* out, int32_t flags) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (n < 0) return fail(EWK_EINVAL, "negative size");
    if (n == 0) return EWK_OK;
    if (!events || !out) return fail(EWK_EINVAL, "NULL argument");
    if (e->n_streams <= 0) return fail(EWK_EINVAL, "engine has no streams");
    for (int32_t i = 0; i < n; ++i) {
        const ewk_event& ev = events[i];
        if (ev.stream < 0 || ev.stream >= e->n_streams || ev.length < 0 || ev.length > e->sring_len ||
            ev.ring_start < 0 || ev.ring_start >= e->sring_len)
            return fail(EWK_EINVAL, "event " + std::to_string(i) + " outside the rings");
        // The segment is the last nreq >= length samples before the write position of its
        // tick (ewk_gate.hip, the cut), and every later tick of its stream writes one block: it
        // is intact while nreq + (ticks since) * block <= ring.  (The write position after tick k
        // is k * block mod ring for every stream, k counted on the stream's own clock.)
        const int64_t Rs = e->sring_len, blk = e->cfg.block;
        const int64_t now = e->stream_tick(ev.stream);   // its stream's clock (the engine's in lockstep)
        if (ev.tick < 0 || ev.tick > now)
            return fail(EWK_EINVAL, "event " + std::to_string(i) + " is from a tick this engine has not pushed");
        int64_t nreq = ((ev.tick % Rs) * (blk % Rs) % Rs - ev.ring_start) % Rs;
        if (nreq < 0) nreq += Rs;
        if (nreq == 0 && ev.length > 0) nreq = Rs;
        if (nreq + (now - ev.tick) * blk > Rs)
            return fail(EWK_EOVERWRITTEN, "event " + std::to_string(i) + " (tick " + std::to_string(ev.tick) +
                                        "): the ring has overwritten its samples since (now tick " +
                                        std::to_string(now) + "); read positives right after their poll");
    }
    HIP_TRY(hipSetDevice(e->device));
    return normalize_impl(e, nullptr, nullptr, nullptr, events, n, out, flags);
}

int ewk_compact_positives(ewk_engine* e, const double* d_score, const uint8_t* d_match, int32_t n, int64_t first_id,
                          int64_t step, ewk_positive* d_out, int32_t* d_count, int32_t flags, void* stream) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (n < 0) return fail(EWK_EINVAL, "negative size");
    if (!d_count || (n > 0 && (!d_score || !d_match || !d_out))) return fail(EWK_EINVAL, "NULL argument");
    if (flags & ~EWK_COMPACT_APPEND) return fail(EWK_EINVAL, "unknown flags");
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : e->stream;
    const int nb = std::max(1, compact_blocks(n));
    if (nb > e->compact_cap) {   // grown rarely (stream-ordered: the old scratch may be in use)
        HIP_TRY(hipStreamSynchronize(s));
        (void)hipFree(e->d_compact);
        e->d_compact = nullptr;
        e->compact_cap = 0;
        HIP_TRY(hipMalloc(&e->d_compact, 2 * (size_t)nb * sizeof(int32_t)));
        e->compact_cap = nb;
    }
    HIP_TRY(launch_compact_positives(d_score, d_match, n, first_id, step, d_out, d_count, e->d_compact,
                                     (flags & EWK_COMPACT_APPEND) ? 1 : 0, s));
    return EWK_OK;
}

int ewk_decode_pcm16(ewk_engine* e, const int16_t* in, int64_t n, float* out, int32_t flags) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (n < 0) return fail(EWK_EINVAL, "negative size");
    if (n == 0) return EWK_OK;
    if (!in || !out) return fail(EWK_EINVAL, "NULL argument");
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    if (flags & EWK_PCM_DEVICE) {   // both pointers device memory; asynchronous
        HIP_TRY(launch_decode_pcm16(in, out, n, s));
        return EWK_OK;
    }
    TmpBuf<int16_t> d_in;
    TmpBuf<float> d_out;
    HIP_TRY(d_in.reserve(n));
    HIP_TRY(d_out.reserve(n));
    HIP_TRY(hipMemcpyAsync(d_in.p, in, n * sizeof(int16_t), hipMemcpyHostToDevice, s));
    HIP_TRY(launch_decode_pcm16(d_in.p, d_out.p, n, s));
    HIP_TRY(hipMemcpyAsync(out, d_out.p, n * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return EWK_OK;
}

// ---------------------------------------------------------------- input-rate resampler
int ewk_resample_design(int32_t in_rate, int32_t out_rate, double* taps, int32_t cap, int32_t* n_taps, int32_t* up,
                        int32_t* down) {
    if (in_rate <= 0 || out_rate <= 0) return fail(EWK_EINVAL, "sample rates must be positive");
    int32_t u = 1, d = 1;
    resample_ratio(in_rate, out_rate, &u, &d);
    const int64_t n = 20 * (int64_t)std::max(u, d) + 1;
    if (n > 0x7fffffffLL) return fail(EWK_EINVAL, "the filter of this rate pair has more than 2^31 taps");
    if (up) *up = u;
    if (down) *down = d;
    if (n_taps) *n_taps = (int32_t)n;
    if (!taps || cap < n) return fail(EWK_EINVAL, "taps holds fewer than " + std::to_string(n) + " values");
    resample_taps(u, d, taps);
    return EWK_OK;
}

// The filter in_rate -> cfg.sample_rate in the kernel's layout.  Waits for the engine's stream
// before the taps of another rate replace those it may still read.
static int rs_prepare(ewk_engine* e, ewk_engine::RsFilter& f, int32_t in_rate, bool streaming) {
    if (f.rate == in_rate && f.taps.p) return EWK_OK;
    int32_t up = 1, down = 1;
    resample_ratio(in_rate, e->cfg.sample_rate, &up, &down);
    const int64_t half = 10 * (int64_t)std::max(up, down), J = 2 * half / up + 1;
    const int threads = resample_threads(up);
    const int64_t span = threads ? resample_span(up, down, (int32_t)std::min<int64_t>(J, kRsMaxSpan), threads) : 0;
    if (!threads || J + 1 > kRsMaxSpan || span > kRsMaxSpan)
        return fail(EWK_EINVAL, "the filter " + std::to_string(in_rate) + " -> " + std::to_string(e->cfg.sample_rate) +
                                    " Hz (up " + std::to_string(up) + ", down " + std::to_string(down) +
                                    ") is over the size the resampler supports (up <= " + std::to_string(kRsMaxThreads) +
                                    ", " + std::to_string(kRsMaxSpan) + " staged samples per workgroup)");
    // streaming: the whole-signal resample delayed by ceil(half / down) samples
    const int64_t c0 = streaming ? half - (half + down - 1) / down * down : half;
    std::vector<double> h((size_t)(2 * half + 1)), tt((size_t)(J * up), 0.0);
    resample_taps(up, down, h.data());
    for (int64_t j = 0; j < J; ++j)
        for (int64_t p = 0; p < up; ++p)
            if (p + j * up <= 2 * half) tt[(size_t)(j * up + p)] = h[(size_t)(p + j * up)];
    HIP_TRY(hipStreamSynchronize(e->stream));
    f.rate = 0;
    HIP_TRY(f.taps.reserve(tt.size()));
    HIP_TRY(hipMemcpy(f.taps.p, tt.data(), tt.size() * sizeof(double), hipMemcpyHostToDevice));
    f.up = up;
    f.down = down;
    f.half = (int32_t)half;
    f.c0 = c0;
    f.J = (int32_t)J;
    f.H = (int32_t)J + 1;
    f.threads = threads;
    f.span = (int32_t)span;
    f.rate = in_rate;
    return EWK_OK;
}

int ewk_resample(ewk_engine* e, const float* in, int64_t n_in, int32_t in_rate, float* out, int64_t cap,
                 int64_t* n_out, int32_t flags) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (n_out) *n_out = 0;
    if (in_rate <= 0) return fail(EWK_EINVAL, "sample rates must be positive");
    if (n_in < 0 || n_in >= (1LL << 40)) return fail(EWK_EINVAL, "n_in must be in [0, 2^40)");
    int32_t up = 1, down = 1;
    resample_ratio(in_rate, e->cfg.sample_rate, &up, &down);
    const int64_t no = (n_in * up + down - 1) / down;   // ceil(n_in * out / in)
    if (n_out) *n_out = no;
    if (cap < no) return fail(EWK_EINVAL, "out holds fewer than " + std::to_string(no) + " samples");
    if (no == 0) return EWK_OK;
    if (!in || !out) return fail(EWK_EINVAL, "NULL argument");
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    const bool in_dev = (flags & EWK_PCM_DEVICE) != 0, out_dev = (flags & EWK_OUT_DEVICE) != 0;
    if (up == 1 && down == 1) {   // the engine's own rate: a copy (as resample_poly returns it)
        HIP_TRY(hipMemcpyAsync(out, in, (size_t)n_in * sizeof(float), hipMemcpyDefault, s));
        if (!in_dev || !out_dev) HIP_TRY(hipStreamSynchronize(s));
        return EWK_OK;
    }
    int rc = rs_prepare(e, e->rs_one, in_rate, false);
    if (rc) return rc;
    const ewk_engine::RsFilter& f = e->rs_one;
    TmpBuf<float> d_in, d_out;
    if (!in_dev) {
        HIP_TRY(d_in.reserve((size_t)n_in));
        HIP_TRY(hipMemcpyAsync(d_in.p, in, (size_t)n_in * sizeof(float), hipMemcpyHostToDevice, s));
    }
    if (!out_dev) HIP_TRY(d_out.reserve((size_t)no));
    ResampleArgs r;
    memset(&r, 0, sizeof(r));
    r.in = in_dev ? in : d_in.p;
    r.in_block = n_in;
    r.n_in = n_in;
    r.out = out_dev ? out : d_out.p;
    r.out_stride = no;
    r.n_out = no;
    r.rows = 1;
    r.taps = f.taps.p;
    r.up = f.up;
    r.down = f.down;
    r.J = f.J;
    r.H = f.H;
    r.c0 = f.c0;
    r.threads = f.threads;
    r.span = f.span;
    {
        ProfScope ps(e, 3, s);
        HIP_TRY(launch_resample(r, s));
    }
    if (!out_dev) HIP_TRY(hipMemcpyAsync(out, d_out.p, (size_t)no * sizeof(float), hipMemcpyDeviceToHost, s));
    if (!in_dev || !out_dev) HIP_TRY(hipStreamSynchronize(s));   // (the staging buffers die on return)
    return EWK_OK;
}

int ewk_set_input_rate(ewk_engine* e, int32_t in_rate) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (e->n_streams <= 0) return fail(EWK_EINVAL, "engine has no streams");
    if (in_rate < 0) return fail(EWK_EINVAL, "in_rate must be >= 0");
    HIP_TRY(hipSetDevice(e->device));
    if (in_rate == 0 || in_rate == e->cfg.sample_rate) {
        if (!e->rs_on) return EWK_OK;
        HIP_TRY(hipStreamSynchronize(e->stream));
        e->rs_on = false;
        return EWK_OK;
    }
    if (e->ring_es == sizeof(int16_t))
        return fail(EWK_EINVAL, "an int16 ring (EWK_RING_I16) stores PCM16 as delivered: resampled samples are not int16");
    int32_t up = 1, down = 1;
    resample_ratio(in_rate, e->cfg.sample_rate, &up, &down);
    if (((int64_t)e->cfg.block * down) % up)
        return fail(EWK_EINVAL, "a tick of " + std::to_string(e->cfg.block) + " samples at " +
                                    std::to_string(e->cfg.sample_rate) + " Hz is not a whole number of samples at " +
                                    std::to_string(in_rate) + " Hz");
    e->rs_on = false;   // (a failure below leaves the engine at its own rate)
    int rc = rs_prepare(e, e->rs_in, in_rate, true);   // waits for the pushes so far when the rate changes
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    const ewk_engine::RsFilter& f = e->rs_in;
    const size_t nh = (size_t)e->n_streams * f.H;
    if (nh > e->rs_hist.cap) HIP_TRY(e->rs_hist.reserve(nh));
    HIP_TRY(hipMemset(e->rs_hist.p, 0, e->rs_hist.cap * sizeof(float)));
    HIP_TRY(e->rs_out.reserve((size_t)e->n_streams * e->cfg.block));
    if (e->desync || e->rs_flags.p) {   // streams on their own clocks: every one starts fresh
        HIP_TRY(e->rs_flags.reserve((size_t)e->n_streams));
        HIP_TRY(hipMemset(e->rs_flags.p, 1, e->rs_flags.cap));
    }
    e->rs_in_block = (int32_t)((int64_t)e->cfg.block * down / up);
    e->rs_delay = (int32_t)((f.half + down - 1) / down);
    e->rs_fresh = true;
    e->rs_on = true;
    return EWK_OK;
}

int ewk_input_rate_info(ewk_engine* e, int32_t* in_rate, int32_t* in_block, int32_t* delay) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (in_rate) *in_rate = e->rs_on ? e->rs_in.rate : e->cfg.sample_rate;
    if (in_block) *in_block = e->rs_on ? e->rs_in_block : e->cfg.block;
    if (delay) *delay = e->rs_on ? e->rs_delay : 0;
    return EWK_OK;
}

// Event banks are drained in two steps so a failing poll consumes nothing:
// peek_bank waits for the pushes into bank b (copy stream only, no wait on later
// work) and fetches its counters with the first kPollChunk events; take_bank copies
// the rest out and re-arms the bank's counters on the engine stream.
struct BankPeek {
    int32_t n = 0;         // queued events (<= ev_cap)
    int32_t dropped = 0;   // events lost to a full bank
    uint32_t count = 0, dropped_total = 0;   // the raw counters (the next epoch's bases)
    bool used = false;
};

static int peek_bank(ewk_engine* e, int b, BankPeek* pk) {
    *pk = BankPeek();
    if (!e->bank_used[b]) return EWK_OK;
    HIP_TRY(ensure_poll_region(e));
    unsigned char* reg = e->h_poll + b * kPollRegion;
    int32_t* cnt = reinterpret_cast<int32_t*>(reg);
    const int32_t chunk = std::min<int32_t>(kPollChunk, e->ev_cap);
    if (e->mirror[b]) {   // written by k_bank_mirror behind the bank's last push
        HIP_TRY(hipEventSynchronize(e->bank_done[b]));
    } else {
        HIP_TRY(hipStreamWaitEvent(e->cstream, e->bank_done[b], 0));
        HIP_TRY(hipMemcpyAsync(cnt, e->evc_bank(b), 4 * sizeof(int32_t), hipMemcpyDeviceToHost, e->cstream));
        HIP_TRY(hipMemcpyAsync(reg + 16, e->ev_bank(b), (size_t)chunk * sizeof(ewk_event), hipMemcpyDeviceToHost,
                               e->cstream));
        HIP_TRY(hipStreamSynchronize(e->cstream));
    }
    pk->count = (uint32_t)cnt[0];
    pk->dropped_total = (uint32_t)cnt[1];
    pk->n = (int32_t)std::min<uint32_t>(pk->count - e->ev_base0[b], (uint32_t)e->ev_cap);
    pk->dropped = (int32_t)(pk->dropped_total - e->drop_base0[b]);
    pk->used = true;
    return EWK_OK;
}

// Re-arm bank b: its next epoch starts at the counters the host just read (no device work;
// the scorer's watermark is at or behind the new base and is clamped to it).
static int rearm_bank(ewk_engine* e, int b, const BankPeek& pk) {
    e->ev_base0[b] = pk.count;
    e->drop_base0[b] = pk.dropped_total;
    e->bank_used[b] = false;
    e->mirror[b] = false;
    return EWK_OK;
}

static int take_bank(ewk_engine* e, int b, const BankPeek& pk, ewk_event* out) {
    if (!pk.used) return EWK_OK;
    const int32_t chunk = std::min<int32_t>(kPollChunk, e->ev_cap);
    if (pk.n > 0 && out) {
        memcpy(out, e->h_poll + b * kPollRegion + 16, (size_t)std::min(pk.n, chunk) * sizeof(ewk_event));
        if (pk.n > chunk) {
            HIP_TRY(hipMemcpyAsync(out + chunk, e->ev_bank(b) + chunk, (size_t)(pk.n - chunk) * sizeof(ewk_event),
                                   hipMemcpyDeviceToHost, e->cstream));
            HIP_TRY(hipStreamSynchronize(e->cstream));
        }
    }
    return rearm_bank(e, b, pk);
}

// An overflowed bank cannot be delivered whole: re-arm it (its events are lost, the
// engine keeps running) and report how many were dropped.
static int overflow(ewk_engine* e, const BankPeek* pk, const int* banks, int nb) {
    int64_t lost = 0;
    for (int i = 0; i < nb; ++i)
        if (pk[i].used && pk[i].dropped > 0) {
            lost += (int64_t)pk[i].n + pk[i].dropped;
            int rc = rearm_bank(e, banks[i], pk[i]);
            if (rc) return rc;
        }
    return fail(EWK_ENOMEM, "event queue overflow: " + std::to_string(lost) +
                                " events of the overflowed bank(s) dropped; the queue was re-armed");
}

static void sort_events(ewk_event* out, int32_t n) {   // deterministic order: (tick, stream)
    std::sort(out, out + n, [](const ewk_event& x, const ewk_event& y) {
        return x.tick != y.tick ? x.tick < y.tick : x.stream < y.stream;
    });
}

static int poll_banks(ewk_engine* e, const int* banks, int nb, ewk_event* out, int32_t cap, int32_t* n_out) {
    BankPeek pk[2];
    int64_t total = 0;
    bool over = false;
    for (int i = 0; i < nb; ++i) {
        int rc = peek_bank(e, banks[i], &pk[i]);
        if (rc) return rc;
        total += pk[i].n;
        over = over || pk[i].dropped > 0;
    }
    if (over) return overflow(e, pk, banks, nb);
    // validated before either bank is consumed: a short `cap` loses nothing
    if (out && total > std::max(0, cap))
        return fail(EWK_EINVAL, "poll capacity " + std::to_string(cap) + " is smaller than the " +
                                    std::to_string(total) + " queued events (nothing was drained)");
    int32_t n = 0;
    for (int i = 0; i < nb; ++i) {
        int rc = take_bank(e, banks[i], pk[i], out ? out + n : nullptr);
        if (rc) return rc;
        n += pk[i].n;
    }
    if (out) sort_events(out, n);
    *n_out = n;
    return EWK_OK;
}

int ewk_poll(ewk_engine* e, ewk_event* out, int32_t cap, int32_t* n_out) {
    if (!e || !n_out) return fail(EWK_EINVAL, "NULL argument");
    *n_out = 0;
    if (e->n_streams <= 0) return EWK_OK;
    HIP_TRY(hipSetDevice(e->device));
    const int banks[2] = {e->bank ^ 1, e->bank};   // older first
    return poll_banks(e, banks, 2, out, cap, n_out);
}

int ewk_poll_lagged(ewk_engine* e, ewk_event* out, int32_t cap, int32_t* n_out) {
    if (!e || !n_out) return fail(EWK_EINVAL, "NULL argument");
    *n_out = 0;
    if (e->n_streams <= 0) return EWK_OK;
    HIP_TRY(hipSetDevice(e->device));
    const int older = e->bank ^ 1;
    const int banks[1] = {older};
    int rc = poll_banks(e, banks, 1, out, cap, n_out);
    if (rc == EWK_OK || !e->bank_used[older])   // drained (or re-armed after an overflow)
        e->bank = older;   // later pushes append to the drained bank; the newest one drains next time
    return rc;
}

int ewk_reenter(ewk_engine* e, int32_t stream, double reentry_timeout) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (e->n_streams <= 0) return fail(EWK_EINVAL, "engine has no streams");
    if (stream < -1 || stream >= e->n_streams) return fail(EWK_EINVAL, "stream index out of range");
    if (!(reentry_timeout == reentry_timeout)) return fail(EWK_EINVAL, "reentry_timeout is NaN");
    HIP_TRY(hipSetDevice(e->device));
    e->cfg.reentry_timeout = reentry_timeout;   // read by every later gate launch
    const int32_t first = stream < 0 ? 0 : stream;
    const int32_t n = stream < 0 ? e->n_streams : 1;
    HIP_TRY(launch_reenter(e->d_st, first, n, e->cfg.tick_seconds, e->stream));
    return EWK_OK;
}

int ewk_get_stream_state(ewk_engine* e, int32_t stream, ewk_stream_state* out) {
    if (!e || !out) return fail(EWK_EINVAL, "NULL argument");
    if (stream < 0 || stream >= e->n_streams) return fail(EWK_EINVAL, "stream index out of range");
    HIP_TRY(hipSetDevice(e->device));
    GateStream st;
    HIP_TRY(hipMemcpyAsync(&st, e->d_st + stream, sizeof(st), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    out->samples_collected = st.collected;
    out->tick = st.tick;
    out->silence_threshold = st.threshold;
    out->last_rms = st.last_rms;
    out->silence_start_time = st.silence_start;
    out->sound_start_time = st.sound_start;
    out->sound_end_time = st.sound_end;
    out->start_time = st.start_time;
    out->pointer = st.pointer;
    out->state = st.state;
    out->started = st.started;
    out->last_silent = st.last_silent;
    return EWK_OK;
}

int ewk_read_segment(ewk_engine* e, int32_t stream, int64_t ring_start, int32_t length, float* out) {
    if (!e || !out) return fail(EWK_EINVAL, "NULL argument");
    if (stream < 0 || stream >= e->n_streams) return fail(EWK_EINVAL, "stream index out of range");
    if (length < 0 || length > e->sring_len || ring_start < 0 || ring_start >= e->sring_len)
        return fail(EWK_EINVAL, "segment out of range");
    HIP_TRY(hipSetDevice(e->device));
    const size_t es = e->ring_es;
    const unsigned char* base = static_cast<const unsigned char*>(e->d_ring) + (size_t)stream * e->sring_len * es;
    const int64_t first = std::min<int64_t>(length, e->sring_len - ring_start);
    // int16 rings: copied to a host staging buffer, then widened (x / 32768, exact)
    std::vector<int16_t> q(es == sizeof(int16_t) ? (size_t)length : 0);
    unsigned char* dst = es == sizeof(float) ? reinterpret_cast<unsigned char*>(out)
                                             : reinterpret_cast<unsigned char*>(q.data());
    HIP_TRY(hipMemcpyAsync(dst, base + ring_start * es, first * es, hipMemcpyDeviceToHost, e->stream));
    if (length > first)
        HIP_TRY(hipMemcpyAsync(dst + first * es, base, (length - first) * es, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (size_t i = 0; i < q.size(); ++i) out[i] = (float)q[i] * (1.0f / 32768.0f);
    return EWK_OK;
}

int ewk_read_last(ewk_engine* e, int32_t stream, int64_t n_samples, float* out, int64_t* n_out) {
    if (!e || !out || !n_out) return fail(EWK_EINVAL, "NULL argument");
    if (stream < 0 || stream >= e->n_streams) return fail(EWK_EINVAL, "stream index out of range");
    // return_last_n_seconds: at most the reference ring (wakeword.py:500-502)
    int64_t n = std::min<int64_t>(std::max<int64_t>(n_samples, 0), e->ring_len);
    *n_out = 0;
    if (n > e->sring_len)
        return fail(EWK_EINVAL, "the compact ring keeps only the last " + std::to_string(e->sring_len) + " samples");
    HIP_TRY(hipSetDevice(e->device));
    GateStream st;
    HIP_TRY(hipMemcpyAsync(&st, e->d_st + stream, sizeof(st), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    *n_out = n;
    if (n == 0) return EWK_OK;
    int64_t start = st.spos - n;
    if (start < 0) start += e->sring_len;
    return ewk_read_segment(e, stream, start, (int32_t)n, out);
}

int ewk_profile_enable(ewk_engine* e, int32_t on) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    e->prof = on != 0;
    return EWK_OK;
}

int ewk_profile_read(ewk_engine* e, int32_t kind, double* total_ms, int64_t* launches) {
    if (!e || !total_ms || !launches) return fail(EWK_EINVAL, "NULL argument");
    if (kind < 0 || kind > 3) return fail(EWK_EINVAL, "kind must be 0, 1, 2 or 3");
    HIP_TRY(hipSetDevice(e->device));
    double tot = 0.0;
    for (auto& p : e->ev[kind]) {
        HIP_TRY(hipEventSynchronize(p.second));
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, p.first, p.second));
        tot += ms;
        e->ev_pool.push_back(p.first);
        e->ev_pool.push_back(p.second);
    }
    *total_ms = tot;
    *launches = (int64_t)e->ev[kind].size();
    e->ev[kind].clear();
    return EWK_OK;
}

}  // extern "C"
