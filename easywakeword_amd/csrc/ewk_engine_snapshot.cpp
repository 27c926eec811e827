// ewk_engine_snapshot.cpp -- the C ABI's stream snapshots (ewk_snapshot_plan, ewk_snapshot_info,
// ewk_export_streams, ewk_import_streams): listed streams leave an engine as records
// (ewk_snapshot_plan.h, ewk_snapshot.hip) and continue in any slot of another.
#include "ewk_engine.h"
#include "ewk_snapshot_plan.h"

using namespace ewk;

constexpr size_t kSnapStageBytes = 32u << 20;   // a half of the host-payload staging (or one record)

int ewk_snapshot_plan(const ewk_config* cfg, int32_t in_rate, ewk_snapshot_layout* out) {
    ewk_config c;
    if (cfg) c = *cfg;
    else ewk_default_config(&c);
    const SnapshotPlanError err = snapshot_plan(&c, in_rate, out);
    return err == kSnapPlanOk ? EWK_OK : fail(EWK_EINVAL, snapshot_plan_message(err));
}

// The engine's layout from what it runs with (equal to snapshot_plan of its configuration and rate).
static void engine_layout(const ewk_engine* e, ewk_snapshot_layout* l) {
    memset(l, 0, sizeof(*l));
    l->sample_rate = e->cfg.sample_rate;
    l->block = e->cfg.block;
    l->buffer_seconds = e->cfg.buffer_seconds;
    l->ring_format = e->cfg.ring_format;
    l->n_blocks = e->n_blocks;
    l->in_rate = e->rs_on ? e->rs_in.rate : e->cfg.sample_rate;
    l->in_block = e->rs_on ? e->rs_in_block : e->cfg.block;
    l->hist_len = e->rs_on ? e->rs_in.H : 0;
    l->ring_len = e->ring_len;
    l->sring_len = e->sring_len;
    l->tick_seconds = e->cfg.tick_seconds;
    snapshot_sections(l);
}

int ewk_snapshot_info(ewk_engine* e, ewk_snapshot_layout* out) {
    if (!e || !out) return fail(EWK_EINVAL, "NULL argument");
    if (e->n_streams <= 0) return fail(EWK_EINVAL, "engine has no streams");
    engine_layout(e, out);
    return EWK_OK;
}

static bool carry_holds(const ewk_engine* e, const ewk_snapshot_layout& l) {
    return e->chunk_carry.p && e->chunk_carry.cap >= (size_t)e->n_streams * (size_t)l.in_block * e->ring_es;
}

// Launch arguments but for the list and the records.
static SnapArgs snap_args(ewk_engine* e, const ewk_snapshot_layout& l) {
    SnapArgs a;
    memset(&a, 0, sizeof(a));
    a.n_blocks = e->n_blocks;
    a.record_bytes = l.record_bytes;
    for (int k = 0; k < EWK_SNAP_SECTIONS; ++k) {
        a.off[k] = l.section[k].offset;
        a.sec_bytes[k] = l.section[k].bytes;
    }
    a.ring = static_cast<unsigned char*>(e->d_ring);
    a.row_bytes = e->sring_len * (int64_t)e->ring_es;
    a.st = e->d_st;
    a.block_rms = e->d_brms;
    a.sorted_rms = e->d_sorted;
    a.lsn_st = e->d_lsn_st.p;
    a.lsn_count = e->d_lsn_count.p;
    if (e->rs_on) {
        a.hist = e->rs_hist.p;
        a.H = e->rs_in.H;
        a.fresh = e->rs_flags.p;
        a.fresh_all = e->rs_fresh ? 1 : 0;
    }
    a.compact = e->sring_len < e->ring_len ? 1 : 0;
    a.es = (int32_t)e->ring_es;
    a.carry = carry_holds(e, l) ? e->chunk_carry.p : nullptr;
    a.in_block = l.in_block;
    return a;
}

// The two halves of the host-payload staging, each of `*per` records (at most kSnapStageBytes, or one).
static int reserve_staging(ewk_engine* e, const ewk_snapshot_layout& l, int32_t n, int32_t* per, hipStream_t s) {
    *per = (int32_t)std::max<int64_t>(1, std::min<int64_t>(n, (int64_t)kSnapStageBytes / l.record_bytes));
    const size_t half = (size_t)*per * (size_t)l.record_bytes;
    if (half > e->snap_half) {
        int rc = grow_behind(e->snap_dev, 2 * half, s);
        if (rc) return rc;
        e->snap_half = half;
    }
    for (auto& p : e->snap_pin) HIP_TRY(p.reserve(e->snap_half));
    return EWK_OK;
}

int ewk_export_streams(ewk_engine* e, const int32_t* streams, int32_t n, ewk_stream_meta* meta, void* payload,
                       int64_t cap_bytes, int32_t flags) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (e->n_streams <= 0) return fail(EWK_EINVAL, "engine has no streams");
    int rc = check_stream_list(e, streams, n);
    if (rc) return rc;
    if (!meta || !payload) return fail(EWK_EINVAL, "meta or payload is NULL");
    ewk_snapshot_layout l;
    engine_layout(e, &l);
    if (cap_bytes < (int64_t)n * l.record_bytes)
        return fail(EWK_EINVAL, "payload holds " + std::to_string(cap_bytes) + " bytes, " + std::to_string(n) +
                                    " records of " + std::to_string(l.record_bytes) + " need " +
                                    std::to_string((int64_t)n * l.record_bytes));
    const bool device = (flags & EWK_OUT_DEVICE) != 0;
    if (device && ((uintptr_t)payload & 15)) return fail(EWK_EINVAL, "a device payload must be 16-byte aligned");
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    HIP_TRY(join_scoring(e, s));   // every event of the pushes so far is scored and queued here
    std::vector<int32_t> pend((size_t)n, 0);
    for (int32_t i = 0; i < n; ++i) {
        const int32_t st = streams[i];
        if (!e->chunk_pending.empty()) pend[i] = e->chunk_pending[st];
        ewk_stream_meta& m = meta[i];
        memset(&m, 0, sizeof(m));
        m.magic = l.magic;
        m.version = l.version;
        m.tick = e->stream_tick(st);
        m.record_bytes = l.record_bytes;
        m.fingerprint = l.fingerprint;
        m.pending = pend[i];
        m.profile = e->stream_profile.empty() ? -1 : e->stream_profile[st];
        m.word = e->stream_word.empty() ? 0 : e->stream_word[st];
        m.n_listeners = e->listeners_on() ? e->lsn_count[st] : 1;
        for (int32_t j = 0; j < EWK_LISTENERS_MAX; ++j)
            m.listeners[j] = (j > 0 && j < m.n_listeners) ? e->lsn_tab[(size_t)st * EWK_LISTENERS_MAX + j]
                                                           : ewk_listener{-1, 0};
        m.listeners[0] = ewk_listener{m.profile, m.word};
    }
    rc = stage_stream_list(e, streams, pend.data(), n, s);
    if (rc) return rc;
    SnapArgs a = snap_args(e, l);
    if (device) {
        a.ids = e->d_ids.p;
        a.pending = e->d_ids.p + e->n_streams;
        a.n = n;
        a.rec = static_cast<unsigned char*>(payload);
        ProfScope ps(e, 5, s);
        HIP_TRY(launch_snapshot_pack(a, s));
        return EWK_OK;
    }
    // Host payload: pack a half, copy it to its pinned side, and hand the previous half to the
    // caller while this one is on its way.
    int32_t per = 0;
    rc = reserve_staging(e, l, n, &per, s);
    if (rc) return rc;
    unsigned char* out = static_cast<unsigned char*>(payload);
    int32_t prev_first = 0, prev_n = 0;
    int b = 0;
    for (int32_t first = 0; first < n; first += per, b ^= 1) {
        const int32_t cnt = std::min(per, n - first);
        a.ids = e->d_ids.p + first;
        a.pending = e->d_ids.p + e->n_streams + first;
        a.n = cnt;
        a.rec = e->snap_dev.p + (size_t)b * e->snap_half;
        {
            ProfScope ps(e, 5, s);
            HIP_TRY(launch_snapshot_pack(a, s));
        }
        HIP_TRY(hipMemcpyAsync(e->snap_pin[b].p, a.rec, (size_t)cnt * l.record_bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(e->snap_pin[b].sent(s));
        if (prev_n) {
            HIP_TRY(e->snap_pin[b ^ 1].wait());
            memcpy(out + (size_t)prev_first * l.record_bytes, e->snap_pin[b ^ 1].p, (size_t)prev_n * l.record_bytes);
        }
        prev_first = first;
        prev_n = cnt;
    }
    HIP_TRY(e->snap_pin[b ^ 1].wait());
    memcpy(out + (size_t)prev_first * l.record_bytes, e->snap_pin[b ^ 1].p, (size_t)prev_n * l.record_bytes);
    return EWK_OK;
}

static std::string record_of(int32_t i, int32_t stream) {
    return "record " + std::to_string(i) + " (for stream " + std::to_string(stream) + ")";
}

// Every host check of an import; changes nothing but check_stream_list's `seen`.
static int check_import(ewk_engine* e, const ewk_snapshot_layout& l, const int32_t* streams, int32_t n,
                        const ewk_stream_meta* meta, const void* payload, int64_t bytes, bool device) {
    int rc = check_stream_list(e, streams, n);
    if (rc) return rc;
    if (!meta || !payload) return fail(EWK_EINVAL, "meta or payload is NULL");
    if (bytes != (int64_t)n * l.record_bytes)
        return fail(EWK_EINVAL, "payload of " + std::to_string(bytes) + " bytes: " + std::to_string(n) + " records of " +
                                    std::to_string(l.record_bytes) + " bytes are " +
                                    std::to_string((int64_t)n * l.record_bytes));
    if (device && ((uintptr_t)payload & 15)) return fail(EWK_EINVAL, "a device payload must be 16-byte aligned");
    const int32_t n_prof = (int32_t)e->profiles.size();
    const int32_t n_words = e->sbank_on ? (int32_t)e->bank_first.size() - 1 : 0;
    for (int32_t i = 0; i < n; ++i) {
        const ewk_stream_meta& m = meta[i];
        const std::string who = record_of(i, streams[i]);
        if (m.magic != EWK_SNAPSHOT_MAGIC) return fail(EWK_EINVAL, who + ": not a stream snapshot (magic)");
        if (m.version != EWK_SNAPSHOT_VERSION)
            return fail(EWK_EINVAL, who + ": snapshot version " + std::to_string(m.version) + ", this library reads " +
                                        std::to_string(EWK_SNAPSHOT_VERSION));
        if (m.record_bytes != l.record_bytes || m.fingerprint != l.fingerprint)
            return fail(EWK_EINVAL, who + ": exported with another geometry (record of " + std::to_string(m.record_bytes) +
                                        " bytes, this engine's are " + std::to_string(l.record_bytes) +
                                        "; sample rate, block, rings, ring format, tick and input rate must agree)");
        if (m.tick < 0) return fail(EWK_EINVAL, who + ": negative tick");
        if (m.pending < 0 || m.pending >= l.in_block)
            return fail(EWK_EINVAL, who + ": pending " + std::to_string(m.pending) + " is outside [0, " +
                                        std::to_string(l.in_block) + ")");
        if (m.n_listeners < 1 || m.n_listeners > EWK_LISTENERS_MAX)
            return fail(EWK_EINVAL, who + ": a stream has 1.." + std::to_string(EWK_LISTENERS_MAX) +
                                        " listeners, got " + std::to_string(m.n_listeners));
        for (int32_t j = 0; j < m.n_listeners; ++j) {
            const ewk_listener r = j ? m.listeners[j] : ewk_listener{m.profile, m.word};
            const std::string lj = who + ", listener " + std::to_string(j);
            if (r.profile < -1 || r.profile >= n_prof)
                return fail(EWK_EINVAL, lj + ": profile " + std::to_string(r.profile) + " is outside [-1, " +
                                            std::to_string(n_prof) + ") of this engine's detector-profile table" +
                                            (n_prof ? "" : " (none is set: ewk_detector_profiles_set)"));
            if (e->sbank_on ? (r.word < 0 || r.word >= n_words) : r.word != 0)
                return fail(EWK_EINVAL, lj + ": word " + std::to_string(r.word) +
                                            (e->sbank_on ? " is outside [0, " + std::to_string(n_words) +
                                                               ") of this engine's stream bank"
                                                         : " while this engine's stream bank is off (ewk_stream_bank_enable)"));
        }
    }
    return EWK_OK;
}

int ewk_import_streams(ewk_engine* e, const int32_t* streams, int32_t n, const ewk_stream_meta* meta,
                       const void* payload, int64_t bytes, int32_t flags) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (e->n_streams <= 0) return fail(EWK_EINVAL, "engine has no streams");
    ewk_snapshot_layout l;
    engine_layout(e, &l);
    const bool device = (flags & EWK_PCM_DEVICE) != 0;
    int rc = check_import(e, l, streams, n, meta, payload, bytes, device);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    HIP_TRY(join_scoring(e, s));   // (overlap mode: the scorer may still read these ring rows)
    rc = desynchronise(e, s);
    if (rc) return rc;
    // Profile, word and listeners of every record, device side and mirrors, by the call that sets
    // them (it allocates what its first use allocates; the states it starts are overwritten by the
    // unpack behind it).  Nothing to set on an engine without any table.
    bool multi = false, any_pending = false;
    for (int32_t i = 0; i < n; ++i) {
        multi = multi || meta[i].n_listeners > 1;
        any_pending = any_pending || meta[i].pending > 0;
    }
    if (multi || e->listeners_on() || !e->profiles.empty() || e->sbank_on) {
        std::vector<int32_t> count((size_t)n);
        std::vector<ewk_listener> rows((size_t)n * EWK_LISTENERS_MAX);
        for (int32_t i = 0; i < n; ++i) {
            count[i] = meta[i].n_listeners;
            std::copy(meta[i].listeners, meta[i].listeners + EWK_LISTENERS_MAX, rows.begin() + (size_t)i * EWK_LISTENERS_MAX);
            rows[(size_t)i * EWK_LISTENERS_MAX] = ewk_listener{meta[i].profile, meta[i].word};
        }
        rc = ewk_stream_listeners_set(e, streams, n, count.data(), rows.data(), EWK_LISTENERS_MAX);
        if (rc) return rc;
    }
    // The carry, as a first chunk push allocates it, when a record brings pending samples.
    if (any_pending) {
        const size_t ns = (size_t)e->n_streams;
        HIP_TRY(e->d_chunk.reserve(ns * (sizeof(ChunkDesc) + sizeof(int32_t))));
        rc = grow_behind(e->chunk_carry, ns * (size_t)l.in_block * e->ring_es, s);
        if (rc) return rc;
        if (e->chunk_pending.empty()) e->chunk_pending.assign(ns, 0);
    }
    if (!e->chunk_pending.empty())
        for (int32_t i = 0; i < n; ++i) {
            int32_t& p = e->chunk_pending[streams[i]];
            e->chunk_pending_n += (meta[i].pending > 0) - (p > 0);
            p = meta[i].pending;
        }
    for (int32_t i = 0; i < n; ++i) e->tick_delta[streams[i]] = meta[i].tick - e->tick;
    rc = stage_stream_list(e, streams, nullptr, n, s);
    if (rc) return rc;
    SnapArgs a = snap_args(e, l);
    if (device) {
        a.ids = e->d_ids.p;
        a.n = n;
        a.rec = const_cast<unsigned char*>(static_cast<const unsigned char*>(payload));
        ProfScope ps(e, 5, s);
        HIP_TRY(launch_snapshot_unpack(a, s));
        return EWK_OK;
    }
    // Host payload: through the pinned side of a half into its device side, then the kernel.  The
    // DMA writes staging only, never a ring.
    int32_t per = 0;
    rc = reserve_staging(e, l, n, &per, s);
    if (rc) return rc;
    const unsigned char* in = static_cast<const unsigned char*>(payload);
    int b = 0;
    for (int32_t first = 0; first < n; first += per, b ^= 1) {
        const int32_t cnt = std::min(per, n - first);
        HIP_TRY(e->snap_pin[b].wait());   // the copy out of this half two rounds ago
        memcpy(e->snap_pin[b].p, in + (size_t)first * l.record_bytes, (size_t)cnt * l.record_bytes);
        a.ids = e->d_ids.p + first;
        a.n = cnt;
        a.rec = e->snap_dev.p + (size_t)b * e->snap_half;
        HIP_TRY(hipMemcpyAsync(a.rec, e->snap_pin[b].p, (size_t)cnt * l.record_bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(e->snap_pin[b].sent(s));
        ProfScope ps(e, 5, s);
        HIP_TRY(launch_snapshot_unpack(a, s));
    }
    return EWK_OK;
}
