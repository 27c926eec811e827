// ewk_engine_poll.cpp -- the C ABI's reads of a streaming engine: the event banks and their
// polls, ewk_reenter, stream and listener state, ring reads.
#include "ewk_engine.h"

using namespace ewk;

// The mapped region the poll mirror is written to (k_bank_mirror and the re-score launch's tick
// end, through d_poll) and polls read from (h_poll).
hipError_t ewk::ensure_poll_region(ewk_engine* e) {
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
