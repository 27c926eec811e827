// ewk_engine_stream.cpp -- the C ABI's streaming side (levels 1 + 2): pushes and the scoring
// passes behind them, stream index lists and the stream lifecycle, the stream bank, polls and
// ring reads.
#include "ewk_engine.h"

#include "ewk_chunk_plan.h"

using namespace ewk;

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
    // (the listener table stays, as profile and word assignments stay; the states start again)
    if (e->d_lsn_st.p) HIP_TRY(hipMemsetAsync(e->d_lsn_st.p, 0, e->d_lsn_st.cap * sizeof(LsnState), s));
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
    e->drop_all_pending();   // (the carry rows stay as they are: every read of one is bounded by its pending count)
    return EWK_OK;
}

// ---- stream lifecycle: index lists --------------------------------------------------
// An index list as every call that takes one requires it: 1 <= n <= n_streams, every entry a
// stream, none twice (two waves would run one stream).  Host only; changes nothing but `seen`.
static int fail_stream_index(ewk_engine* e, int32_t i, int32_t s) {
    return fail(EWK_EINVAL, "streams[" + std::to_string(i) + "] = " + std::to_string(s) + " is outside [0, " +
                                std::to_string(e->n_streams) + ")");
}

static std::string listener_of(int32_t stream, int32_t j) {
    return "listener " + std::to_string(j) + " of stream " + std::to_string(stream);
}

static int fail_listener_word(int32_t stream, int32_t j, int32_t word, int32_t n_words) {
    return fail(EWK_EINVAL, listener_of(stream, j) + ": word " + std::to_string(word) + " is outside [0, " +
                                std::to_string(n_words) + ")");
}

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
        if (s < 0 || s >= e->n_streams) return fail_stream_index(e, i, s);
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

// ---- scoring passes (ring mode) -----------------------------------------------------
// The current bank's events [ev_base, *n_events) as segments of the rings; n_events is the live
// counter (same stream as the gate) or a snapshot of it taken after the gate.  The re-score
// launch (after the scorer) re-scores the listed segments in fp64 and its last workgroup out
// advances the watermark.
static ScoreArgs ring_args(ewk_engine* e, const int32_t* n_events) {
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
    a.adv_ev_base = e->evc_bank(e->bank) + 2;
    a.evc = e->evc_bank(e->bank);
    return a;
}

// Workgroups of the stream bank's event passes: the waves stride over the pending events, so
// the grid follows the engine's size (an empty tick only pays for reading the counters).
static int32_t stream_bank_grid(const ewk_engine* e) {
    return std::min(1024, std::max(8, (e->n_streams + 255) / 256));
}

// A scoring pass with the stream bank enabled, all on ss, every hand-off a kernel boundary:
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
    ScoreArgs a = ring_args(e, n_events);
    a.has_template = 0;
    a.rs_slots = e->rs_slots.p;
    a.out_mean = e->sb_mean.p;   // statistics by event slot
    a.out_std = e->sb_std.p;
    a.out_theta = e->sb_theta.p;
    a.out_mean64 = e->sb_mean64.p;
    a.out_std64 = e->sb_std64.p;
    BankArgs b = bank_args(e);
    BankEvArgs x;
    x.stream_word = e->sbank_words ? e->sb_word.p : nullptr;
    x.ev_list = e->sb_list.p;
    x.lsn_tab = e->d_lsn_tab.p;
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

// Score the events queued since the last scoring pass on ss, then advance the watermark.
static int score_pending(ewk_engine* e, hipStream_t ss, const int32_t* n_events) {
    if (e->sbank_on) return score_pending_bank(e, ss, n_events);   // (needs no single template)
    if (!e->has_tmpl) return EWK_OK;   // events keep NaN scores until a template exists
    ScoreArgs a = ring_args(e, n_events);
    HIP_TRY(ensure_poll_region(e));    // the re-score launch's last workgroup out writes the poll mirror
    a.mirror = e->d_poll + e->bank * kPollRegion;
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

int ewk_stream_bank_enable(ewk_engine* e, const int32_t* stream_word) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (e->n_streams <= 0) return fail(EWK_EINVAL, "engine has no streams");
    if (e->bank_first.empty()) return fail(EWK_ENOTEMPLATE, kNoBank);
    const int32_t n_words = (int32_t)e->bank_first.size() - 1;
    if (stream_word)
        for (int32_t s = 0; s < e->n_streams; ++s)
            if (stream_word[s] < 0 || stream_word[s] >= n_words)
                return fail_word_index(stream_word[s], kOfStream, s, n_words);
    for (int32_t s = 0; s < (int32_t)e->lsn_count.size(); ++s)
        for (int32_t j = 1; j < e->lsn_count[s]; ++j) {
            const int32_t w = e->lsn_tab[(size_t)s * EWK_LISTENERS_MAX + j].word;
            if (w < 0 || w >= n_words) return fail_listener_word(s, j, w, n_words);
        }
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
    if (stream_word) e->stream_word.assign(stream_word, stream_word + e->n_streams);
    else e->stream_word.clear();
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

// ---- a push, stage by stage ---------------------------------------------------------
// Host samples: gather the caller's (pageable) blocks into pinned staging on the CPU, then DMA
// asynchronously on s -- the caller's buffer may die as soon as we return.
static int stage_host_ticks(ewk_engine* e, TickSrc* src, int32_t rows, int32_t n_ticks, int64_t in_block,
                            hipStream_t s) {
    const size_t es = src->pcm16 ? sizeof(int16_t) : sizeof(float);
    const unsigned char* pcm = static_cast<const unsigned char*>(src->p);
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
                   pcm + ((size_t)st * src->stride + (size_t)t * src->tick_stride) * es, in_block * es);
    HIP_TRY(e->push_stage.reserve(total));
    HIP_TRY(hipMemcpyAsync(e->push_stage.p, e->h_stage, total * es, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(e->h_stage_free, s));
    *src = TickSrc{e->push_stage.p, src->pcm16, (int64_t)per_stream, in_block};
    return EWK_OK;
}

// What every gate launch of one push shares: the engine's configuration and state arrays, and
// the event bank pushes append to.  The launch loop adds the samples, the ticks and the clocks.
static GateArgs gate_args(ewk_engine* e) {
    GateArgs g;
    memset(&g, 0, sizeof(g));
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
    g.reentry_timeout = e->cfg.reentry_timeout;   // (ewk_reenter changes it between pushes)
    g.min_threshold = e->cfg.min_threshold;
    g.events = e->ev_bank(e->bank);
    g.ev_count = e->evc_bank(e->bank);
    g.ev_dropped = e->evc_bank(e->bank) + 1;
    g.ev_cap = e->ev_cap;
    if (!e->profiles.empty()) {   // (else nullptr: the gate without the profile code)
        g.profiles = e->d_profiles.p;
        g.stream_profile = e->d_stream_profile.p;
    }
    if (e->lsn_multi > 0) {   // (else nullptr: the gate without the listener code)
        g.lsn_count = e->d_lsn_count.p;
        g.lsn_tab = e->d_lsn_tab.p;
        g.lsn_st = e->d_lsn_st.p;
        g.stream_profile = e->d_stream_profile.p;   // (all -1 without a table)
    }
    return g;
}

// The scoring pass behind gate launch number push_seq (k = its parity) on s: beside the next gate
// on sstream from a snapshot of the event count (overlap), or next in line on s.
static int score_after_gate(ewk_engine* e, int k, hipStream_t s) {
    if (!e->overlap) return score_pending(e, s, e->evc_bank(e->bank));
    int32_t* snap = e->d_work + 4 + k;
    HIP_TRY(launch_snapshot(e->evc_bank(e->bank), snap, s));
    HIP_TRY(hipEventRecord(e->gate_evt[k], s));
    HIP_TRY(hipStreamWaitEvent(e->sstream, e->gate_evt[k], 0));
    int rc = score_pending(e, e->sstream, snap);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(e->score_evt[k], e->sstream));
    e->score_live[k] = true;
    e->score_tail = e->score_evt[k];
    return EWK_OK;
}

// The poll mirror of this bank: written by the last scoring pass's tick end, or by k_bank_mirror:
// behind the gate (no template yet: no scoring pass), or behind the stream bank's last pass (its
// fp64 pass changes events after the tick end).  Then the bank's done event.
static int finish_push(ewk_engine* e, hipStream_t s) {
    hipStream_t ms = e->overlap ? e->sstream : s;
    if (e->sbank_on || !e->has_tmpl) {
        HIP_TRY(ensure_poll_region(e));
        HIP_TRY(launch_bank_mirror(e->evc_bank(e->bank), e->ev_bank(e->bank), e->ev_base0[e->bank], e->ev_cap,
                                   std::min<int32_t>(kPollChunk, e->ev_cap), e->d_poll + e->bank * kPollRegion, ms));
    }
    e->mirror[e->bank] = true;
    HIP_TRY(hipEventRecord(e->bank_done[e->bank], ms));
    e->bank_used[e->bank] = true;
    return EWK_OK;
}

static int gate_ticks(ewk_engine* e, const TickSrc& src, int32_t rows, int32_t n_ticks, const int32_t* d_list,
                      const int32_t* streams, hipStream_t s);

// A tick push to a stream that holds the samples of an unfinished block (ewk_push_chunks) would
// put its audio out of order.  (Nothing is ever pending on an engine that was never chunk-pushed.)
static int fail_pending(ewk_engine* e, int32_t s) {
    return fail(EWK_EINVAL, "stream " + std::to_string(s) + " holds " + std::to_string(e->chunk_pending[s]) +
                                " pending samples of an unfinished block (ewk_push_chunks): a tick push would put them "
                                "out of order; finish the block with ewk_push_chunks or reset the stream");
}

static int check_nothing_pending(ewk_engine* e, const int32_t* streams, int32_t n_list) {
    if (e->chunk_pending_n == 0) return EWK_OK;
    if (streams) {
        for (int32_t i = 0; i < n_list; ++i)
            if (e->chunk_pending[streams[i]] > 0) return fail_pending(e, streams[i]);
        return EWK_OK;
    }
    for (int32_t s = 0; s < e->n_streams; ++s)
        if (e->chunk_pending[s] > 0) return fail_pending(e, s);
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
    // with an input rate set (ewk_set_input_rate) a tick is in_block samples at that rate
    const int64_t in_block = e->rs_on ? e->rs_in_block : e->cfg.block;
    if (stride < in_block && rows > 1)
        return fail(EWK_EINVAL, e->rs_on ? "stride must be >= the input block (ewk_input_rate_info)" : "stride must be >= block");
    {
        int rc = check_nothing_pending(e, streams, n_list);
        if (rc) return rc;
    }
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    int rc = EWK_OK;
    const int32_t* d_list = nullptr;
    if (streams) {
        rc = desynchronise(e, s);
        if (rc == EWK_OK) rc = stage_stream_list(e, streams, nullptr, n_list, s, &d_list, nullptr);
    }
    TickSrc src{pcm_any, pcm16, stride, tick_stride};
    if (rc == EWK_OK && !(flags & EWK_PUSH_DEVICE)) rc = stage_host_ticks(e, &src, rows, n_ticks, in_block, s);
    if (rc == EWK_OK && e->rs_on) rc = resample_ticks(e, &src, rows, n_ticks, d_list, s);
    if (rc == EWK_OK) rc = gate_ticks(e, src, rows, n_ticks, d_list, streams, s);
    if (rc) return rc;
    return finish_push(e, s);
}

// The gate launches of a push, each with its scoring pass behind it: n_ticks ticks at src for
// `rows` streams -- all of them (d_list and streams nullptr), or those of the index list (on the
// device and on the host).  Updates the tick mirror.
static int gate_ticks(ewk_engine* e, const TickSrc& src, int32_t rows, int32_t n_ticks, const int32_t* d_list,
                      const int32_t* streams, hipStream_t s) {
    GateArgs g = gate_args(e);
    g.stride = src.stride;
    g.tick_stride = src.tick_stride;
    g.n_streams = rows;
    g.ids = d_list;
    // Segments must be scored before the ring overwrites them: <= ticks_per_launch ticks per gate launch.
    for (int32_t t0 = 0; t0 < n_ticks; t0 += e->ticks_per_launch) {
        const int32_t nt = std::min<int32_t>(e->ticks_per_launch, n_ticks - t0);
        if (src.pcm16) g.pcm16 = static_cast<const int16_t*>(src.p) + (int64_t)t0 * src.tick_stride;
        else g.pcm = static_cast<const float*>(src.p) + (int64_t)t0 * src.tick_stride;
        g.n_ticks = nt;
        g.own_clock = e->desync ? 1 : 0;
        g.tick0 = e->tick;
        g.ev_base0 = e->ev_base0[e->bank];
        const int k = (int)(e->push_seq & 1);
        // the scoring pass two launches back must be done: it read snapshot slot k, and
        // at most one pass runs beside a gate
        if (e->overlap && e->score_live[k]) HIP_TRY(hipStreamWaitEvent(s, e->score_evt[k], 0));
        {
            ProfScope ps(e, 2, s);
            HIP_TRY(launch_gate(g, s, e->gate_grid_cap));
        }
        if (!streams) e->tick += nt;
        else for (int32_t i = 0; i < rows; ++i) e->tick_delta[streams[i]] += nt;
        int rc = score_after_gate(e, k, s);
        if (rc) return rc;
        e->push_seq += 1;
    }
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

// ---------------------------------------------------------------- packet ingest
static int fail_chunk_plan(ChunkPlanError err, int32_t bad, int32_t in_block, const int32_t* pending,
                           const int32_t* counts) {
    switch (err) {
        case kChunkPlanPending:
            return fail(EWK_EINVAL, "pending[" + std::to_string(bad) + "] = " + std::to_string(pending[bad]) +
                                        " is outside [0, " + std::to_string(in_block) + ")");
        case kChunkPlanCount:
            return fail(EWK_EINVAL, "counts[" + std::to_string(bad) + "] = " + std::to_string(counts[bad]) +
                                        " is outside [0, " + std::to_string((int64_t)EWK_CHUNK_MAX_TICKS * in_block) +
                                        "] (EWK_CHUNK_MAX_TICKS input blocks of " + std::to_string(in_block) + " samples)");
        case kChunkPlanGroups:
            return fail(EWK_EINVAL, "the plan has " + std::to_string(bad) + " groups, group_cap holds fewer");
        default:
            return fail(EWK_EINVAL, "in_block must be positive, n and group_cap >= 0 and no array NULL");
    }
}

int ewk_chunk_plan(int32_t in_block, int32_t n, const int32_t* pending, const int32_t* counts, int32_t* ticks,
                   int32_t* new_pending, int32_t* order, int32_t* n_ticking, int32_t* group_ticks, int32_t* group_first,
                   int32_t group_cap, int32_t* n_groups) {
    int32_t bad = -1;
    const ChunkPlanError err = chunk_plan(in_block, n, pending, counts, ticks, new_pending, order, n_ticking,
                                          group_ticks, group_first, group_cap, n_groups, &bad);
    return err == kChunkPlanOk ? EWK_OK : fail_chunk_plan(err, bad, in_block, pending, counts);
}

int ewk_stream_pending(ewk_engine* e, const int32_t* streams, int32_t n, int32_t* out) {
    if (!e || !out) return fail(EWK_EINVAL, "NULL argument");
    if (n < 0 || n > e->n_streams)
        return fail(EWK_EINVAL, "n must be in [0, " + std::to_string(e->n_streams) + "]");
    for (int32_t i = 0; i < n; ++i) {
        const int32_t s = streams ? streams[i] : i;
        if (s < 0 || s >= e->n_streams) return fail_stream_index(e, i, s);
    }
    for (int32_t i = 0; i < n; ++i) out[i] = e->chunk_pending.empty() ? 0 : e->chunk_pending[streams ? streams[i] : i];
    return EWK_OK;
}

constexpr int64_t kChunkAlign = 32;   // bytes: a group's first tick row, and a staged chunk's phase (copy_span's widest unit)

// What the first chunk push allocates: the pending mirror, the descriptor staging (pinned and on
// the device, fixed size) and the carry rows -- those again when a larger input block has been set.
static int ensure_chunk_state(ewk_engine* e, int64_t in_block, hipStream_t s) {
    const size_t n = (size_t)e->n_streams;
    const size_t stage_bytes = n * (sizeof(ChunkDesc) + sizeof(int32_t));
    if (!e->h_chunk) {
        HIP_TRY(hipHostMalloc((void**)&e->h_chunk, stage_bytes, hipHostMallocDefault));
        HIP_TRY(hipEventCreateWithFlags(&e->h_chunk_free, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(e->h_chunk_free, s));
    }
    HIP_TRY(e->d_chunk.reserve(stage_bytes));
    const size_t carry_bytes = n * (size_t)in_block * e->ring_es;
    if (carry_bytes > e->chunk_carry.cap) {   // (nothing is pending: a new rate drops it)
        HIP_TRY(hipStreamSynchronize(s));
        HIP_TRY(e->chunk_carry.reserve(carry_bytes));
    }
    if (e->chunk_pending.empty()) e->chunk_pending.assign(n, 0);
    return EWK_OK;
}

// Host chunks, packed into the pinned staging and sent with one copy; chunk i then starts at
// d[i].src of the device staging.  A chunk is placed at the 16-byte phase of the samples it
// follows in its stream's block, so the assembly kernel's loads and stores agree in phase.
static int stage_host_chunks(ewk_engine* e, const void* pcm, bool pcm16, const int64_t* offsets, const int32_t* counts,
                             const int32_t* pending, int32_t n, int64_t* src_at, const void** d_src, hipStream_t s) {
    const size_t es = pcm16 ? sizeof(int16_t) : sizeof(float);
    const int64_t unit = kChunkAlign / (int64_t)es;   // samples
    int64_t total = 0;
    for (int32_t i = 0; i < n; ++i) {
        if (counts[i] == 0) {
            src_at[i] = 0;
            continue;
        }
        src_at[i] = (total + unit - 1) / unit * unit + pending[i] % unit;
        total = src_at[i] + counts[i];
    }
    *d_src = e->push_stage.p;
    if (total == 0) return EWK_OK;
    if (e->h_stage_free) HIP_TRY(hipEventSynchronize(e->h_stage_free));   // previous DMA done
    if ((size_t)total > e->h_stage_cap) {
        if (e->h_stage) HIP_TRY(hipHostFree(e->h_stage));
        e->h_stage = nullptr;
        e->h_stage_cap = 0;
        HIP_TRY(hipHostMalloc((void**)&e->h_stage, (size_t)total * sizeof(float), hipHostMallocDefault));   // >= es bytes each
        e->h_stage_cap = (size_t)total;
    }
    if (!e->h_stage_free) HIP_TRY(hipEventCreateWithFlags(&e->h_stage_free, hipEventDisableTiming));
    unsigned char* h = reinterpret_cast<unsigned char*>(e->h_stage);
    int64_t end = 0;   // (the gaps are copied too: defined bytes)
    for (int32_t i = 0; i < n; ++i) {
        if (counts[i] == 0) continue;
        memset(h + end * es, 0, (size_t)(src_at[i] - end) * es);
        memcpy(h + src_at[i] * es, static_cast<const unsigned char*>(pcm) + offsets[i] * es, (size_t)counts[i] * es);
        end = src_at[i] + counts[i];
    }
    if ((size_t)total > e->push_stage.cap) {
        HIP_TRY(hipStreamSynchronize(s));   // an earlier launch may still read the old buffer
        HIP_TRY(e->push_stage.reserve((size_t)total));
    }
    HIP_TRY(hipMemcpyAsync(e->push_stage.p, e->h_stage, (size_t)total * es, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(e->h_stage_free, s));
    *d_src = e->push_stage.p;
    return EWK_OK;
}

static int push_chunks_impl(ewk_engine* e, const int32_t* streams, int32_t n, const void* pcm, int64_t n_pcm,
                            const int64_t* offsets, const int32_t* counts, int32_t flags, bool pcm16) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (e->n_streams <= 0) return fail(EWK_EINVAL, "engine has no streams");
    int rc = check_stream_list(e, streams, n);   // (everything is validated before anything is enqueued or changed)
    if (rc) return rc;
    if (!offsets || !counts) return fail(EWK_EINVAL, "offsets or counts is NULL");
    if (n_pcm < 0) return fail(EWK_EINVAL, "n_pcm must be >= 0");
    if (!pcm && n_pcm > 0) return fail(EWK_EINVAL, "pcm is NULL");
    if (!pcm16 && e->ring_es == sizeof(int16_t))
        return fail(EWK_EINVAL, "an int16 ring (EWK_RING_I16) takes PCM16 chunks (ewk_push_chunks_pcm16)");
    const int32_t in_block = e->rs_on ? e->rs_in_block : e->cfg.block;
    if (in_block > 0x7fffffff / (EWK_CHUNK_MAX_TICKS + 1))
        return fail(EWK_EINVAL, "the input block is too large for chunk pushes");
    // the plan: pending, ticks, new pending, order and chunk sources, n ints each (src_at: int64)
    e->chunk_plan_buf.resize((size_t)n * 6 + 2);
    int32_t* pend = e->chunk_plan_buf.data();
    int32_t *ticks = pend + n, *new_pend = ticks + n, *order = new_pend + n;
    int64_t* src_at = reinterpret_cast<int64_t*>(order + n + (n & 1));
    for (int32_t i = 0; i < n; ++i) pend[i] = e->chunk_pending.empty() ? 0 : e->chunk_pending[streams[i]];
    int32_t group_ticks[EWK_CHUNK_MAX_TICKS], group_first[EWK_CHUNK_MAX_TICKS + 1], n_ticking = 0, n_groups = 0, bad = -1;
    const ChunkPlanError err = chunk_plan(in_block, n, pend, counts, ticks, new_pend, order, &n_ticking, group_ticks,
                                          group_first, EWK_CHUNK_MAX_TICKS, &n_groups, &bad);
    if (err != kChunkPlanOk) return fail_chunk_plan(err, bad, in_block, pend, counts);
    for (int32_t i = 0; i < n; ++i)
        if (offsets[i] < 0 || offsets[i] > n_pcm - counts[i])
            return fail(EWK_EINVAL, "chunk " + std::to_string(i) + " (offsets[" + std::to_string(i) + "] = " +
                                        std::to_string(offsets[i]) + ", counts[" + std::to_string(i) + "] = " +
                                        std::to_string(counts[i]) + ") is outside pcm[0, " + std::to_string(n_pcm) + ")");
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    rc = desynchronise(e, s);
    if (rc == EWK_OK) rc = ensure_chunk_state(e, in_block, s);
    if (rc) return rc;
    // the tick rows: group g contiguous, row stride ticks_g * in_block, its base aligned
    const int64_t row_unit = kChunkAlign / (int64_t)e->ring_es;
    int64_t group_base[EWK_CHUNK_MAX_TICKS], asm_total = 0;
    for (int32_t g = 0; g < n_groups; ++g) {
        group_base[g] = (asm_total + row_unit - 1) / row_unit * row_unit;
        asm_total = group_base[g] + (int64_t)(group_first[g + 1] - group_first[g]) * group_ticks[g] * in_block;
    }
    if ((size_t)asm_total * e->ring_es > e->chunk_asm.cap) {
        HIP_TRY(hipStreamSynchronize(s));   // an earlier gate launch may still read the old buffer
        HIP_TRY(e->chunk_asm.reserve((size_t)asm_total * e->ring_es));
    }
    const void* d_src = pcm;
    if (flags & EWK_PUSH_DEVICE) {
        for (int32_t i = 0; i < n; ++i) src_at[i] = offsets[i];
    } else {
        rc = stage_host_chunks(e, pcm, pcm16, offsets, counts, pend, n, src_at, &d_src, s);
        if (rc) return rc;
    }
    // descriptors: the ticking chunks in plan order (the gate's index lists follow it), then the
    // appending ones; a chunk without samples needs none
    HIP_TRY(hipEventSynchronize(e->h_chunk_free));   // the previous push's descriptors have left the staging
    ChunkDesc* h_desc = reinterpret_cast<ChunkDesc*>(e->h_chunk);
    int32_t* h_list = reinterpret_cast<int32_t*>(e->h_chunk + (size_t)e->n_streams * sizeof(ChunkDesc));
    int32_t n_desc = 0;
    for (int32_t g = 0; g < n_groups; ++g)
        for (int32_t k = group_first[g]; k < group_first[g + 1]; ++k) {
            const int32_t i = order[k];
            const int64_t row = group_base[g] + (int64_t)(k - group_first[g]) * group_ticks[g] * in_block;
            h_desc[n_desc++] = ChunkDesc{src_at[i], row, streams[i], counts[i], pend[i], 0};
            h_list[k] = streams[i];
        }
    for (int32_t i = 0; i < n; ++i)
        if (ticks[i] == 0 && counts[i] > 0) h_desc[n_desc++] = ChunkDesc{src_at[i], 0, streams[i], counts[i], pend[i], 0};
    if (n_desc == 0) return EWK_OK;   // no samples at all
    unsigned char* d_stage = e->d_chunk.p;
    const int32_t* d_list = reinterpret_cast<const int32_t*>(d_stage + (size_t)e->n_streams * sizeof(ChunkDesc));
    HIP_TRY(hipMemcpyAsync(d_stage, h_desc, (size_t)n_desc * sizeof(ChunkDesc), hipMemcpyHostToDevice, s));
    if (n_ticking)
        HIP_TRY(hipMemcpyAsync(const_cast<int32_t*>(d_list), h_list, (size_t)n_ticking * sizeof(int32_t),
                               hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(e->h_chunk_free, s));
    ChunkArgs a;
    memset(&a, 0, sizeof(a));
    a.src = d_src;
    a.out = e->chunk_asm.p;
    a.carry = e->chunk_carry.p;
    a.desc = reinterpret_cast<const ChunkDesc*>(d_stage);
    a.n = n_desc;
    a.in_block = in_block;
    a.max_ticks = n_groups ? group_ticks[n_groups - 1] : 1;
    a.src16 = pcm16 ? 1 : 0;
    a.out16 = e->ring_es == sizeof(int16_t) ? 1 : 0;
    {
        ProfScope ps(e, 4, s);
        HIP_TRY(launch_chunk_assemble(a, s));
    }
    for (int32_t i = 0; i < n; ++i) {
        int32_t& p = e->chunk_pending[streams[i]];
        e->chunk_pending_n += (new_pend[i] > 0) - (p > 0);
        p = new_pend[i];
    }
    if (n_groups == 0) return EWK_OK;   // nobody ticks: the assembly alone (a poll finds the banks as they were)
    // the plan's ticking streams on the host, for the tick mirror (h_list is the next push's to overwrite)
    for (int32_t k = 0; k < n_ticking; ++k) order[k] = streams[order[k]];
    for (int32_t g = 0; g < n_groups; ++g) {
        const int32_t first = group_first[g], rows = group_first[g + 1] - first, nt = group_ticks[g];
        TickSrc src{e->chunk_asm.p + group_base[g] * e->ring_es, a.out16 != 0, (int64_t)nt * in_block, in_block};
        if (e->rs_on) rc = resample_ticks(e, &src, rows, nt, d_list + first, s);
        if (rc == EWK_OK) rc = gate_ticks(e, src, rows, nt, d_list + first, order + first, s);
        if (rc) return rc;
    }
    return finish_push(e, s);
}

int ewk_push_chunks(ewk_engine* e, const int32_t* streams, int32_t n, const float* pcm, int64_t n_pcm,
                    const int64_t* offsets, const int32_t* counts, int32_t flags) {
    return push_chunks_impl(e, streams, n, pcm, n_pcm, offsets, counts, flags, false);
}

int ewk_push_chunks_pcm16(ewk_engine* e, const int32_t* streams, int32_t n, const int16_t* pcm, int64_t n_pcm,
                          const int64_t* offsets, const int32_t* counts, int32_t flags) {
    return push_chunks_impl(e, streams, n, pcm, n_pcm, offsets, counts, flags, true);
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
    a.lsn_st = e->d_lsn_st.p;
    HIP_TRY(launch_reset_list(a, s));
    for (int32_t i = 0; i < n; ++i) e->tick_delta[streams[i]] = -e->tick;
    for (int32_t i = 0; i < n; ++i) e->drop_pending(streams[i]);
    return EWK_OK;
}

int ewk_stream_ticks(ewk_engine* e, const int32_t* streams, int32_t n, int64_t* out) {
    if (!e || !out) return fail(EWK_EINVAL, "NULL argument");
    if (n < 0 || n > e->n_streams)
        return fail(EWK_EINVAL, "n must be in [0, " + std::to_string(e->n_streams) + "]");
    for (int32_t i = 0; i < n; ++i) {
        const int32_t s = streams ? streams[i] : i;
        if (s < 0 || s >= e->n_streams) return fail_stream_index(e, i, s);
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
        if (words[i] < 0 || words[i] >= n_words) return fail_word_index(words[i], kOfStream, streams[i], n_words);
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
    if (e->stream_word.empty()) e->stream_word.assign((size_t)e->n_streams, 0);
    for (int32_t i = 0; i < n; ++i) e->stream_word[streams[i]] = words[i];
    return EWK_OK;
}

// ---------------------------------------------------------------- detector profiles
static ewk_detector_profile profile_of_config(const ewk_config& c) {
    ewk_detector_profile p;
    p.pre_speech_silence = c.pre_speech_silence;
    p.speech_duration_min = c.speech_duration_min;
    p.speech_duration_max = c.speech_duration_max;
    p.post_speech_silence = c.post_speech_silence;
    p.padding = c.padding;
    p.max_segment_seconds = c.max_segment_seconds;
    p.reentry_timeout = c.reentry_timeout;
    return p;
}

void ewk_default_detector_profile(const ewk_engine* e, ewk_detector_profile* out) {
    if (!out) return;
    if (e) {
        *out = profile_of_config(e->cfg);
        return;
    }
    ewk_config c;
    ewk_default_config(&c);
    *out = profile_of_config(c);
}

// ewk_create's tests of the same fields, written so that a NaN fails them too
static int check_profile(int32_t i, const ewk_detector_profile& p) {
    const std::string who = "profiles[" + std::to_string(i) + "].";
    if (!(p.pre_speech_silence > 0)) return fail(EWK_EINVAL, who + "pre_speech_silence must be positive");
    if (!(p.speech_duration_min > 0)) return fail(EWK_EINVAL, who + "speech_duration_min must be positive");
    if (!(p.speech_duration_max > 0)) return fail(EWK_EINVAL, who + "speech_duration_max must be positive");
    if (!(p.speech_duration_min <= p.speech_duration_max))
        return fail(EWK_EINVAL, who + "speech_duration_min must be <= speech_duration_max");
    if (!(p.post_speech_silence > 0)) return fail(EWK_EINVAL, who + "post_speech_silence must be positive");
    if (!(p.padding >= 0)) return fail(EWK_EINVAL, who + "padding must be >= 0");
    if (!(p.max_segment_seconds > 0)) return fail(EWK_EINVAL, who + "max_segment_seconds must be positive");
    if (!(p.reentry_timeout == p.reentry_timeout)) return fail(EWK_EINVAL, who + "reentry_timeout is NaN");
    return EWK_OK;
}

int ewk_detector_profiles_set(ewk_engine* e, const ewk_detector_profile* profiles, int32_t n) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (e->n_streams <= 0) return fail(EWK_EINVAL, "engine has no streams");
    if (!profiles) n = 0;
    if (n < 0 || n > EWK_PROFILE_MAX)
        return fail(EWK_EINVAL, "a profile table holds 0.." + std::to_string(EWK_PROFILE_MAX) + " profiles, got " +
                                    std::to_string(n));
    const ewk_config& c = e->cfg;
    int64_t need = segment_need(c, e->ring_len, c.speech_duration_max, c.post_speech_silence, c.padding);
    for (int32_t i = 0; i < n; ++i) {
        int rc = check_profile(i, profiles[i]);
        if (rc) return rc;
        const int64_t ni = segment_need(c, e->ring_len, profiles[i].speech_duration_max,
                                        profiles[i].post_speech_silence, profiles[i].padding);
        if (e->sring_len < e->ring_len && e->sring_len < ni + c.block)
            return fail(EWK_EINVAL, "profiles[" + std::to_string(i) + "]: ring_samples must hold the longest segment "
                                    "request plus one tick (" + std::to_string(ni + c.block) +
                                    " samples for this profile, the ring holds " + std::to_string(e->sring_len) + ")");
        need = std::max(need, ni);
    }
    if (n > 0)
        for (int32_t s = 0; s < (int32_t)e->stream_profile.size(); ++s)
            if (e->stream_profile[s] >= n)
                return fail(EWK_EINVAL, "stream " + std::to_string(s) + " points at profile " +
                                            std::to_string(e->stream_profile[s]) + " of a table of " + std::to_string(n) +
                                            ": assign it first (ewk_stream_profile_assign), or clear the table");
    for (int32_t s = 0; s < (int32_t)e->lsn_count.size(); ++s)
        for (int32_t j = 1; j < e->lsn_count[s]; ++j) {
            const int32_t p = e->lsn_tab[(size_t)s * EWK_LISTENERS_MAX + j].profile;
            if (p >= n)
                return fail(EWK_EINVAL, "listener " + std::to_string(j) + " of stream " + std::to_string(s) +
                                            " points at profile " + std::to_string(p) + " of a table of " +
                                            std::to_string(n) + ": set its listeners first (ewk_stream_listeners_set)");
        }
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));    // the pushes so far keep their timings
    HIP_TRY(hipStreamSynchronize(e->sstream));
    if (n == 0) {   // table off: every stream back to the engine's configuration
        if (e->d_stream_profile.p) {
            HIP_TRY(hipMemset(e->d_stream_profile.p, 0xff, (size_t)e->n_streams * sizeof(int32_t)));
            std::fill(e->stream_profile.begin(), e->stream_profile.end(), -1);
        }
        e->profiles.clear();
        set_launch_ticks(e, need);   // (the configuration's own again)
        return EWK_OK;
    }
    HIP_TRY(e->d_profiles.reserve((size_t)n));
    if (!e->d_stream_profile.p) {
        HIP_TRY(e->d_stream_profile.reserve((size_t)e->n_streams));
        HIP_TRY(hipMemset(e->d_stream_profile.p, 0xff, (size_t)e->n_streams * sizeof(int32_t)));
        e->stream_profile.assign((size_t)e->n_streams, -1);
    }
    HIP_TRY(hipMemcpy(e->d_profiles.p, profiles, (size_t)n * sizeof(ewk_detector_profile), hipMemcpyHostToDevice));
    e->profiles.assign(profiles, profiles + n);
    set_launch_ticks(e, need);
    return EWK_OK;
}

int ewk_detector_profiles_info(ewk_engine* e, int32_t* n_profiles) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (n_profiles) *n_profiles = (int32_t)e->profiles.size();
    return EWK_OK;
}

int ewk_detector_profile_get(ewk_engine* e, int32_t profile, ewk_detector_profile* out) {
    if (!e || !out) return fail(EWK_EINVAL, "NULL argument");
    const int32_t n = (int32_t)e->profiles.size();
    if (profile < -1 || profile >= n)
        return fail(EWK_EINVAL, "profile index " + std::to_string(profile) + " is outside [-1, " + std::to_string(n) + ")");
    *out = profile < 0 ? profile_of_config(e->cfg) : e->profiles[profile];
    return EWK_OK;
}

int ewk_stream_profile_assign(ewk_engine* e, const int32_t* streams, int32_t n, const int32_t* profiles) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (e->n_streams <= 0) return fail(EWK_EINVAL, "engine has no streams");
    if (e->profiles.empty()) return fail(EWK_EINVAL, "no profile table is set (ewk_detector_profiles_set)");
    int rc = check_stream_list(e, streams, n);
    if (rc) return rc;
    if (!profiles) return fail(EWK_EINVAL, "profiles is NULL");
    const int32_t n_prof = (int32_t)e->profiles.size();
    for (int32_t i = 0; i < n; ++i)
        if (profiles[i] < -1 || profiles[i] >= n_prof)
            return fail(EWK_EINVAL, "profile index " + std::to_string(profiles[i]) + " of stream " +
                                        std::to_string(streams[i]) + " is outside [-1, " + std::to_string(n_prof) + ")");
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = e->stream;   // (the gate is the only reader, and it runs on s)
    const int32_t *d_list = nullptr, *d_vals = nullptr;
    rc = stage_stream_list(e, streams, profiles, n, s, &d_list, &d_vals);
    if (rc) return rc;
    HIP_TRY(launch_scatter_i32(e->d_stream_profile.p, d_list, d_vals, n, s));
    for (int32_t i = 0; i < n; ++i) e->stream_profile[streams[i]] = profiles[i];
    return EWK_OK;
}

int ewk_stream_profiles(ewk_engine* e, const int32_t* streams, int32_t n, int32_t* out) {
    if (!e || !out) return fail(EWK_EINVAL, "NULL argument");
    if (n < 0 || n > e->n_streams)
        return fail(EWK_EINVAL, "n must be in [0, " + std::to_string(e->n_streams) + "]");
    for (int32_t i = 0; i < n; ++i) {
        const int32_t s = streams ? streams[i] : i;
        if (s < 0 || s >= e->n_streams) return fail_stream_index(e, i, s);
    }
    for (int32_t i = 0; i < n; ++i) {
        const int32_t s = streams ? streams[i] : i;
        out[i] = e->stream_profile.empty() ? -1 : e->stream_profile[s];
    }
    return EWK_OK;
}

// ---------------------------------------------------------------- stream listeners
constexpr size_t kLsnRowInts = 2 * EWK_LISTENERS_MAX;   // a stream's table rows as ints
static_assert(sizeof(ewk_listener) == 8 && sizeof(LsnState) == 40, "listener table layout");

// The per-stream listener arrays, at the first call that gives a stream more than one listener:
// every stream starts with one listener and zeroed states.  Also the per-stream profile index
// when no table ever allocated it (all -1): the listener kernels read listener 0's index there.
static int ensure_listeners(ewk_engine* e, hipStream_t s) {
    if (e->listeners_on()) return EWK_OK;
    const size_t n = (size_t)e->n_streams;
    HIP_TRY(e->d_lsn_count.reserve(n));
    HIP_TRY(e->d_lsn_tab.reserve(n * EWK_LISTENERS_MAX));
    HIP_TRY(e->d_lsn_st.reserve(n * kLsnStates));
    HIP_TRY(e->d_lsn_stage.reserve(n * (kLsnRowInts + 1)));
    if (!e->h_lsn_stage)
        HIP_TRY(hipHostMalloc((void**)&e->h_lsn_stage, n * (kLsnRowInts + 1) * sizeof(int32_t), hipHostMallocDefault));
    if (!e->h_lsn_free) HIP_TRY(hipEventCreateWithFlags(&e->h_lsn_free, hipEventDisableTiming));
    std::fill(e->h_lsn_stage, e->h_lsn_stage + n, 1);
    HIP_TRY(hipMemcpyAsync(e->d_lsn_count.p, e->h_lsn_stage, n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(e->h_lsn_free, s));
    HIP_TRY(hipMemsetAsync(e->d_lsn_tab.p, 0, n * EWK_LISTENERS_MAX * sizeof(ewk_listener), s));
    HIP_TRY(hipMemsetAsync(e->d_lsn_st.p, 0, n * kLsnStates * sizeof(LsnState), s));
    if (!e->d_stream_profile.p) {
        HIP_TRY(e->d_stream_profile.reserve(n));
        HIP_TRY(hipMemsetAsync(e->d_stream_profile.p, 0xff, n * sizeof(int32_t), s));
        e->stream_profile.assign(n, -1);
    }
    e->lsn_tab.assign(n * EWK_LISTENERS_MAX, ewk_listener{-1, 0});
    e->lsn_count.assign(n, 1);
    return EWK_OK;
}

// with the stream bank on: the per-stream word array exists (ewk_stream_bank_assign's rule)
static int ensure_stream_words(ewk_engine* e, hipStream_t s) {
    if (e->sbank_words) return EWK_OK;
    HIP_TRY(e->sb_word.reserve((size_t)e->n_streams));
    HIP_TRY(hipMemsetAsync(e->sb_word.p, 0, (size_t)e->n_streams * sizeof(int32_t), s));
    e->sbank_words = true;
    return EWK_OK;
}

int ewk_stream_listeners_set(ewk_engine* e, const int32_t* streams, int32_t n, const int32_t* count,
                             const ewk_listener* listeners, int32_t stride) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (e->n_streams <= 0) return fail(EWK_EINVAL, "engine has no streams");
    int rc = check_stream_list(e, streams, n);
    if (rc) return rc;
    if (!count) return fail(EWK_EINVAL, "count is NULL");
    if (!listeners) return fail(EWK_EINVAL, "listeners is NULL");
    const int32_t n_prof = (int32_t)e->profiles.size();
    const int32_t n_words = e->sbank_on ? (int32_t)e->bank_first.size() - 1 : 0;
    bool multi = false;
    for (int32_t i = 0; i < n; ++i) {
        if (count[i] < 1 || count[i] > EWK_LISTENERS_MAX)
            return fail(EWK_EINVAL, "stream " + std::to_string(streams[i]) + ": a stream has 1.." +
                                        std::to_string(EWK_LISTENERS_MAX) + " listeners, got count " +
                                        std::to_string(count[i]));
        if (stride < count[i])
            return fail(EWK_EINVAL, "stride " + std::to_string(stride) + " is below the count " + std::to_string(count[i]) +
                                        " of stream " + std::to_string(streams[i]));
        multi = multi || count[i] > 1;
    }
    for (int32_t i = 0; i < n; ++i)
        for (int32_t j = 0; j < count[i]; ++j) {
            const ewk_listener& l = listeners[(size_t)i * stride + j];
            if (l.profile < -1 || l.profile >= n_prof)
                return fail(EWK_EINVAL, listener_of(streams[i], j) + ": profile " + std::to_string(l.profile) +
                                            " is outside [-1, " + std::to_string(n_prof) + ")" +
                                            (n_prof ? "" : " (no profile table is set)"));
            if (e->sbank_on) {
                if (l.word < 0 || l.word >= n_words) return fail_listener_word(streams[i], j, l.word, n_words);
            } else if (l.word != 0) {
                return fail(EWK_EINVAL, listener_of(streams[i], j) + ": word " + std::to_string(l.word) +
                                            " while the stream bank is off (the word must be 0)");
            }
        }
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    HIP_TRY(join_scoring(e, s));   // (overlap mode: a scoring pass in flight still reads the words)
    if (e->sbank_on) {
        rc = ensure_stream_words(e, s);
        if (rc) return rc;
    }
    const int32_t *d_list = nullptr, *d_vals = nullptr;
    if (!e->listeners_on() && !multi) {   // one listener each and no table to keep: the two assign calls
        std::vector<int32_t> v((size_t)n);
        if (n_prof) {
            for (int32_t i = 0; i < n; ++i) v[i] = listeners[(size_t)i * stride].profile;
            rc = stage_stream_list(e, streams, v.data(), n, s, &d_list, &d_vals);
            if (rc) return rc;
            HIP_TRY(launch_scatter_i32(e->d_stream_profile.p, d_list, d_vals, n, s));
            for (int32_t i = 0; i < n; ++i) e->stream_profile[streams[i]] = v[i];
        }
        if (e->sbank_on) {
            for (int32_t i = 0; i < n; ++i) v[i] = listeners[(size_t)i * stride].word;
            rc = stage_stream_list(e, streams, v.data(), n, s, &d_list, &d_vals);
            if (rc) return rc;
            HIP_TRY(launch_scatter_i32(e->sb_word.p, d_list, d_vals, n, s));
            if (e->stream_word.empty()) e->stream_word.assign((size_t)e->n_streams, 0);
            for (int32_t i = 0; i < n; ++i) e->stream_word[streams[i]] = v[i];
        }
        return EWK_OK;
    }
    rc = ensure_listeners(e, s);
    if (rc) return rc;
    rc = stage_stream_list(e, streams, nullptr, n, s, &d_list, nullptr);
    if (rc) return rc;
    // rows (EWK_LISTENERS_MAX per listed stream, whatever the caller's stride), then the counts
    HIP_TRY(hipEventSynchronize(e->h_lsn_free));   // the previous call's rows have left the staging
    ewk_listener* h_rows = reinterpret_cast<ewk_listener*>(e->h_lsn_stage);
    int32_t* h_counts = e->h_lsn_stage + (size_t)n * kLsnRowInts;
    for (int32_t i = 0; i < n; ++i) {
        for (int32_t j = 0; j < EWK_LISTENERS_MAX; ++j)
            h_rows[(size_t)i * EWK_LISTENERS_MAX + j] = j < count[i] ? listeners[(size_t)i * stride + j] : ewk_listener{-1, 0};
        h_counts[i] = count[i];
    }
    HIP_TRY(hipMemcpyAsync(e->d_lsn_stage.p, e->h_lsn_stage, (size_t)n * (kLsnRowInts + 1) * sizeof(int32_t),
                           hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(e->h_lsn_free, s));
    ListenerSetArgs a;
    memset(&a, 0, sizeof(a));
    a.ids = d_list;
    a.rows = reinterpret_cast<const ewk_listener*>(e->d_lsn_stage.p);
    a.counts = e->d_lsn_stage.p + (size_t)n * kLsnRowInts;
    a.n = n;
    a.lsn_count = e->d_lsn_count.p;
    a.lsn_tab = e->d_lsn_tab.p;
    a.lsn_st = e->d_lsn_st.p;
    a.st = e->d_st;
    a.stream_profile = e->d_stream_profile.p;
    a.stream_word = e->sbank_on ? e->sb_word.p : nullptr;
    a.tick_seconds = e->cfg.tick_seconds;
    HIP_TRY(launch_listeners_set(a, s));
    if (e->sbank_on && e->stream_word.empty()) e->stream_word.assign((size_t)e->n_streams, 0);
    for (int32_t i = 0; i < n; ++i) {
        const int32_t st = streams[i];
        e->lsn_multi += (count[i] > 1) - (e->lsn_count[st] > 1);
        e->lsn_count[st] = count[i];
        std::copy(h_rows + (size_t)i * EWK_LISTENERS_MAX, h_rows + (size_t)(i + 1) * EWK_LISTENERS_MAX,
                  e->lsn_tab.begin() + (size_t)st * EWK_LISTENERS_MAX);
        e->stream_profile[st] = listeners[(size_t)i * stride].profile;
        if (e->sbank_on) e->stream_word[st] = listeners[(size_t)i * stride].word;
    }
    return EWK_OK;
}

int ewk_stream_listeners(ewk_engine* e, int32_t stream, ewk_listener* out, int32_t cap, int32_t* n_out) {
    if (!e || !n_out) return fail(EWK_EINVAL, "NULL argument");
    if (stream < 0 || stream >= e->n_streams) return fail(EWK_EINVAL, "stream index out of range");
    const int32_t c = e->listeners_on() ? e->lsn_count[stream] : 1;
    *n_out = c;
    for (int32_t j = 0; out && j < std::min(c, cap); ++j)
        out[j] = j ? e->lsn_tab[(size_t)stream * EWK_LISTENERS_MAX + j]
                   : ewk_listener{e->stream_profile.empty() ? -1 : e->stream_profile[stream],
                                  e->stream_word.empty() ? 0 : e->stream_word[stream]};
    return EWK_OK;
}

int ewk_get_listener_state(ewk_engine* e, int32_t stream, int32_t listener, ewk_stream_state* out) {
    int rc = ewk_get_stream_state(e, stream, out);
    if (rc || listener == 0) return rc;
    const int32_t c = e->listeners_on() ? e->lsn_count[stream] : 1;
    if (listener < 0 || listener >= c)
        return fail(EWK_EINVAL, "stream " + std::to_string(stream) + " has " + std::to_string(c) + " listener(s), asked for " +
                                    std::to_string(listener));
    LsnState ls;
    HIP_TRY(hipMemcpyAsync(&ls, e->d_lsn_st.p + (size_t)stream * kLsnStates + listener - 1, sizeof(ls),
                           hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    out->silence_start_time = ls.silence_start;
    out->sound_start_time = ls.sound_start;
    out->sound_end_time = ls.sound_end;
    out->start_time = ls.start_time;
    out->state = ls.state;
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

static void sort_events(ewk_event* out, int32_t n) {   // deterministic order: (tick, stream, listener)
    std::sort(out, out + n, [](const ewk_event& x, const ewk_event& y) {
        if (x.tick != y.tick) return x.tick < y.tick;
        if (x.stream != y.stream) return x.stream < y.stream;
        return EWK_EV_LISTENER(x.flags) < EWK_EV_LISTENER(y.flags);
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
    HIP_TRY(launch_reenter(e->d_st, first, n, e->cfg.tick_seconds, e->d_lsn_count.p, e->d_lsn_st.p, e->stream));
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
