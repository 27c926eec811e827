// ewk_engine_stream.cpp -- the C ABI's streaming side (levels 1 + 2): the full reset and the
// list reset, stream index lists, the scoring passes and the tick pushes in front of them.  The
// other streaming sources: ewk_engine_chunks.cpp (packet ingest), ewk_engine_assign.cpp (what is
// assigned to streams) and ewk_engine_poll.cpp (polls, state and ring reads).
#include "ewk_engine.h"

using namespace ewk;

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
    if (e->d_evc) (void)hipMemsetAsync(e->d_evc, 0, 8 * sizeof(int32_t), s);   // both event banks: empty, unused
    e->ev_base0[0] = e->ev_base0[1] = 0;
    e->drop_base0[0] = e->drop_base0[1] = 0;
    e->bank_used[0] = e->bank_used[1] = false;
    e->mirror[0] = e->mirror[1] = false;
    HIP_TRY(hipStreamSynchronize(s));
    e->tick = 0;
    e->desync = false;   // one clock again
    std::vector<int64_t>().swap(e->tick_delta);
    e->drop_all_pending();   // (the carry rows stay as they are: every read of one is bounded by its pending count)
    return EWK_OK;
}

// ---- stream lifecycle: index lists --------------------------------------------------
int ewk::fail_stream_index(ewk_engine* e, int32_t i, int32_t s) {
    return fail(EWK_EINVAL, "streams[" + std::to_string(i) + "] = " + std::to_string(s) + " is outside [0, " +
                                std::to_string(e->n_streams) + ")");
}

// An index list as every call that changes streams takes it: 1 <= n <= n_streams, every entry a
// stream, none twice (two waves would run one stream).  Host only; changes nothing but `seen`.
int ewk::check_stream_list(ewk_engine* e, const int32_t* streams, int32_t n) {
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
// the caller's arrays may die on return.  Kernels enqueued on s after this call find them at
// d_ids.p and d_ids.p + n_streams, until the next call.
int ewk::stage_stream_list(ewk_engine* e, const int32_t* streams, const int32_t* vals, int32_t n, hipStream_t s) {
    const size_t cap = 2 * (size_t)e->n_streams;
    HIP_TRY(e->d_ids.reserve(cap));
    HIP_TRY(e->ids_stage.reserve(cap * sizeof(int32_t)));   // (and the previous list has left the staging)
    int32_t* h_list = e->ids_stage.as<int32_t>();
    memcpy(h_list, streams, (size_t)n * sizeof(int32_t));
    if (vals) memcpy(h_list + e->n_streams, vals, (size_t)n * sizeof(int32_t));
    HIP_TRY(hipMemcpyAsync(e->d_ids.p, h_list, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (vals)
        HIP_TRY(hipMemcpyAsync(e->d_ids.p + e->n_streams, h_list + e->n_streams, (size_t)n * sizeof(int32_t),
                               hipMemcpyHostToDevice, s));
    HIP_TRY(e->ids_stage.sent(s));
    return EWK_OK;
}

// dst[streams[i]] = vals[i] on the device, on s, and in dst's host mirror.
int ewk::scatter_assign(ewk_engine* e, DevBuf<int32_t>& dst, std::vector<int32_t>& mirror, const int32_t* streams,
                        const int32_t* vals, int32_t n, hipStream_t s) {
    int rc = stage_stream_list(e, streams, vals, n, s);
    if (rc) return rc;
    HIP_TRY(launch_scatter_i32(dst.p, e->d_ids.p, e->d_ids.p + e->n_streams, n, s));
    for (int32_t i = 0; i < n; ++i) mirror[streams[i]] = vals[i];
    return EWK_OK;
}

// ... and as a query takes it: 0 <= n <= n_streams, streams may be NULL (then: streams 0..n-1).
int ewk::check_query_list(ewk_engine* e, const int32_t* streams, int32_t n) {
    if (n < 0 || n > e->n_streams)
        return fail(EWK_EINVAL, "n must be in [0, " + std::to_string(e->n_streams) + "]");
    for (int32_t i = 0; i < n; ++i) {
        const int32_t s = streams ? streams[i] : i;
        if (s < 0 || s >= e->n_streams) return fail_stream_index(e, i, s);
    }
    return EWK_OK;
}

// First subset push or list reset: every stream gets a clock of its own.  With a rate set, also
// the per-stream fresh flags, from the engine-wide one.
int ewk::desynchronise(ewk_engine* e, hipStream_t s) {
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

// ---- a push, stage by stage ---------------------------------------------------------
// Host samples: gather the caller's (pageable) blocks into pinned staging on the CPU, then DMA
// asynchronously on s -- the caller's buffer may die as soon as we return.
static int stage_host_ticks(ewk_engine* e, TickSrc* src, int32_t rows, int32_t n_ticks, int64_t in_block,
                            hipStream_t s) {
    const size_t es = src->kind.es();
    const unsigned char* pcm = static_cast<const unsigned char*>(src->p);
    const size_t per_stream = (size_t)n_ticks * in_block;
    const size_t bytes = per_stream * rows * es;
    HIP_TRY(e->pcm_stage.reserve(bytes));   // (and the previous DMA is done)
    for (int32_t st = 0; st < rows; ++st)
        for (int32_t t = 0; t < n_ticks; ++t)
            memcpy(e->pcm_stage.p + ((size_t)st * per_stream + (size_t)t * in_block) * es,
                   pcm + ((size_t)st * src->stride + (size_t)t * src->tick_stride) * es, in_block * es);
    int rc = send_staged(e, bytes, s);
    if (rc) return rc;
    *src = TickSrc{e->push_stage.p, src->kind, (int64_t)per_stream, in_block};
    return EWK_OK;
}

int ewk::send_staged(ewk_engine* e, size_t bytes, hipStream_t s) {
    int rc = grow_behind(e->push_stage, (bytes + sizeof(float) - 1) / sizeof(float), s);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(e->push_stage.p, e->pcm_stage.p, bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(e->pcm_stage.sent(s));
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
int ewk::finish_push(ewk_engine* e, hipStream_t s) {
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

// What a G.711 push needs beyond a PCM16 one (host only): a law of ewk.h -- `law`, or every entry of
// `laws` [n] when given -- and an input rate, since the codes are 8 kHz samples and the gate reads
// cfg.sample_rate ones.  (An int16 ring was refused before: it cannot have a rate.)
int ewk::check_g711(ewk_engine* e, int32_t law, const uint8_t* laws, int32_t n) {
    if (!laws && law != EWK_G711_ULAW && law != EWK_G711_ALAW)
        return fail(EWK_EINVAL, "law = " + std::to_string(law) + " is neither EWK_G711_ULAW (0) nor EWK_G711_ALAW (1)");
    for (int32_t i = 0; laws && i < n; ++i)
        if (laws[i] != EWK_G711_ULAW && laws[i] != EWK_G711_ALAW)
            return fail(EWK_EINVAL, "laws[" + std::to_string(i) + "] = " + std::to_string(laws[i]) +
                                        " is neither EWK_G711_ULAW (0) nor EWK_G711_ALAW (1)");
    if (!e->rs_on)
        return fail(EWK_EINVAL, "a G.711 push needs an input rate: the codes are samples at the source's rate "
                                "(8000 Hz for PCMU / PCMA), set it with ewk_set_input_rate first");
    return EWK_OK;
}

// streams == nullptr: a tick for every stream (row s of pcm is stream s); else rows 0..n_list-1
// are the ticks of streams[0..n_list) (ewk_push_streams).
static int push_impl(ewk_engine* e, const void* pcm_any, int64_t stride, int64_t tick_stride, int32_t n_ticks,
                     int32_t flags, SampleKind kind, const int32_t* streams = nullptr, int32_t n_list = 0) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (e->n_streams <= 0) return fail(EWK_EINVAL, "engine has no streams");
    if (streams || n_list) {   // (validated before anything is enqueued or changed)
        int rc = check_stream_list(e, streams, n_list);
        if (rc) return rc;
    }
    const int32_t rows = streams ? n_list : e->n_streams;
    if (!pcm_any) return fail(EWK_EINVAL, "pcm is NULL");
    if (n_ticks <= 0) return fail(EWK_EINVAL, "n_ticks must be positive");
    if (kind.type != kSamplePcm16 && e->ring_es == sizeof(int16_t))
        return fail(EWK_EINVAL, "an int16 ring (EWK_RING_I16) takes PCM16 pushes (ewk_push_pcm16)");
    if (kind.type == kSampleG711) {
        int rc = check_g711(e, kind.law, nullptr, 0);
        if (rc) return rc;
    }
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
    if (streams) {
        rc = desynchronise(e, s);
        if (rc == EWK_OK) rc = stage_stream_list(e, streams, nullptr, n_list, s);
    }
    const int32_t* d_list = streams ? e->d_ids.p : nullptr;
    TickSrc src{pcm_any, kind, stride, tick_stride};
    if (rc == EWK_OK && !(flags & EWK_PUSH_DEVICE)) rc = stage_host_ticks(e, &src, rows, n_ticks, in_block, s);
    if (rc == EWK_OK && e->rs_on) rc = resample_ticks(e, &src, rows, n_ticks, d_list, s);
    if (rc == EWK_OK) rc = gate_ticks(e, src, rows, n_ticks, d_list, streams, s);
    if (rc) return rc;
    return finish_push(e, s);
}

// The gate launches of a push, each with its scoring pass behind it: n_ticks ticks at src for
// `rows` streams -- all of them (d_list and streams nullptr), or those of the index list (on the
// device and on the host).  Updates the tick mirror.
int ewk::gate_ticks(ewk_engine* e, const TickSrc& src, int32_t rows, int32_t n_ticks, const int32_t* d_list,
                    const int32_t* streams, hipStream_t s) {
    GateArgs g = gate_args(e);
    g.stride = src.stride;
    g.tick_stride = src.tick_stride;
    g.n_streams = rows;
    g.ids = d_list;
    // Segments must be scored before the ring overwrites them: <= ticks_per_launch ticks per gate launch.
    for (int32_t t0 = 0; t0 < n_ticks; t0 += e->ticks_per_launch) {
        const int32_t nt = std::min<int32_t>(e->ticks_per_launch, n_ticks - t0);
        if (src.kind.type == kSamplePcm16) g.pcm16 = static_cast<const int16_t*>(src.p) + (int64_t)t0 * src.tick_stride;
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
        e->gate_last = gate_family(g);   // (what launch_gate dispatched on)
        if (!streams) e->tick += nt;
        else for (int32_t i = 0; i < rows; ++i) e->tick_delta[streams[i]] += nt;
        int rc = score_after_gate(e, k, s);
        if (rc) return rc;
        e->push_seq += 1;
    }
    return EWK_OK;
}

int ewk_push(ewk_engine* e, const float* pcm, int64_t stride, int32_t flags) {
    return push_impl(e, pcm, stride, 0, 1, flags, kKindF32);
}

int ewk_push_many(ewk_engine* e, const float* pcm, int64_t stride, int64_t tick_stride, int32_t n_ticks,
                  int32_t flags) {
    return push_impl(e, pcm, stride, tick_stride, n_ticks, flags, kKindF32);
}

int ewk_push_pcm16(ewk_engine* e, const int16_t* pcm, int64_t stride, int32_t flags) {
    return push_impl(e, pcm, stride, 0, 1, flags, kKindPcm16);
}

int ewk_push_many_pcm16(ewk_engine* e, const int16_t* pcm, int64_t stride, int64_t tick_stride, int32_t n_ticks,
                        int32_t flags) {
    return push_impl(e, pcm, stride, tick_stride, n_ticks, flags, kKindPcm16);
}

// ---------------------------------------------------------------- stream lifecycle
int ewk_push_streams(ewk_engine* e, const int32_t* streams, int32_t n, const float* pcm, int64_t stride,
                     int64_t tick_stride, int32_t n_ticks, int32_t flags) {
    if (e && !streams) return fail(EWK_EINVAL, "streams is NULL");
    return push_impl(e, pcm, stride, tick_stride, n_ticks, flags, kKindF32, streams, n);
}

int ewk_push_streams_pcm16(ewk_engine* e, const int32_t* streams, int32_t n, const int16_t* pcm, int64_t stride,
                           int64_t tick_stride, int32_t n_ticks, int32_t flags) {
    if (e && !streams) return fail(EWK_EINVAL, "streams is NULL");
    return push_impl(e, pcm, stride, tick_stride, n_ticks, flags, kKindPcm16, streams, n);
}

int ewk_push_g711(ewk_engine* e, const uint8_t* pcm, int64_t stride, int64_t tick_stride, int32_t n_ticks, int32_t law,
                  int32_t flags) {
    return push_impl(e, pcm, stride, tick_stride, n_ticks, flags, SampleKind{kSampleG711, law});
}

int ewk_push_streams_g711(ewk_engine* e, const int32_t* streams, int32_t n, const uint8_t* pcm, int64_t stride,
                          int64_t tick_stride, int32_t n_ticks, int32_t law, int32_t flags) {
    if (e && !streams) return fail(EWK_EINVAL, "streams is NULL");
    return push_impl(e, pcm, stride, tick_stride, n_ticks, flags, SampleKind{kSampleG711, law}, streams, n);
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
    rc = stage_stream_list(e, streams, nullptr, n, s);
    if (rc) return rc;
    a.ids = e->d_ids.p;
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
    int rc = check_query_list(e, streams, n);
    if (rc) return rc;
    for (int32_t i = 0; i < n; ++i) out[i] = e->stream_tick(streams ? streams[i] : i);
    return EWK_OK;
}
