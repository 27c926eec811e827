// ewk_engine_assign.cpp -- the C ABI's calls that assign something to streams: the stream bank
// and its word per stream, the detector-profile table and its profile per stream, and the
// listeners.  Each keeps a host mirror of what it put on the device; the gate and the scoring
// passes (ewk_engine_stream.cpp) only read the device side.
#include "ewk_engine.h"

using namespace ewk;

static std::string listener_of(int32_t stream, int32_t j) {
    return "listener " + std::to_string(j) + " of stream " + std::to_string(stream);
}

static int fail_listener_word(int32_t stream, int32_t j, int32_t word, int32_t n_words) {
    return fail(EWK_EINVAL, listener_of(stream, j) + ": word " + std::to_string(word) + " is outside [0, " +
                                std::to_string(n_words) + ")");
}

// A stream bank enabled with word 0 for every stream has no array: the array and its mirror, all zeros.
int ewk::ensure_stream_words(ewk_engine* e, hipStream_t s) {
    if (e->sbank_words) return EWK_OK;
    HIP_TRY(e->sb_word.reserve((size_t)e->n_streams));
    HIP_TRY(hipMemsetAsync(e->sb_word.p, 0, (size_t)e->n_streams * sizeof(int32_t), s));
    e->stream_word.assign((size_t)e->n_streams, 0);
    e->sbank_words = true;
    return EWK_OK;
}

// Every stream's profile index -1 (the engine's configuration), on the device (s) and in the mirror.
static int clear_stream_profile(ewk_engine* e, hipStream_t s) {
    HIP_TRY(e->d_stream_profile.reserve((size_t)e->n_streams));
    HIP_TRY(hipMemsetAsync(e->d_stream_profile.p, 0xff, (size_t)e->n_streams * sizeof(int32_t), s));
    e->stream_profile.assign((size_t)e->n_streams, -1);
    return EWK_OK;
}

int ewk::ensure_stream_profile(ewk_engine* e, hipStream_t s) {
    return e->d_stream_profile.p ? EWK_OK : clear_stream_profile(e, s);
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
    rc = ensure_stream_words(e, s);
    return rc ? rc : scatter_assign(e, e->sb_word, e->stream_word, streams, words, n, s);
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
        int rc = e->d_stream_profile.p ? clear_stream_profile(e, e->stream) : EWK_OK;
        if (rc) return rc;
        e->profiles.clear();
        set_launch_ticks(e, need);   // (the configuration's own again)
        return EWK_OK;
    }
    HIP_TRY(e->d_profiles.reserve((size_t)n));
    {   // (both streams are idle: the fill on e->stream is in front of every later gate launch)
        int rc = ensure_stream_profile(e, e->stream);
        if (rc) return rc;
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
    // (the gate is the only reader, and it runs on e->stream)
    return scatter_assign(e, e->d_stream_profile, e->stream_profile, streams, profiles, n, e->stream);
}

int ewk_stream_profiles(ewk_engine* e, const int32_t* streams, int32_t n, int32_t* out) {
    if (!e || !out) return fail(EWK_EINVAL, "NULL argument");
    int rc = check_query_list(e, streams, n);
    if (rc) return rc;
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
    HIP_TRY(e->lsn_stage.reserve(n * (kLsnRowInts + 1) * sizeof(int32_t)));
    int32_t* h_ones = e->lsn_stage.as<int32_t>();
    std::fill(h_ones, h_ones + n, 1);
    HIP_TRY(hipMemcpyAsync(e->d_lsn_count.p, h_ones, n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(e->lsn_stage.sent(s));
    HIP_TRY(hipMemsetAsync(e->d_lsn_tab.p, 0, n * EWK_LISTENERS_MAX * sizeof(ewk_listener), s));
    HIP_TRY(hipMemsetAsync(e->d_lsn_st.p, 0, n * kLsnStates * sizeof(LsnState), s));
    int rc = ensure_stream_profile(e, s);
    if (rc) return rc;
    e->lsn_tab.assign(n * EWK_LISTENERS_MAX, ewk_listener{-1, 0});
    e->lsn_count.assign(n, 1);
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
    if (!e->listeners_on() && !multi) {   // one listener each and no table to keep: the two assign calls
        std::vector<int32_t> v((size_t)n);
        if (n_prof) {
            for (int32_t i = 0; i < n; ++i) v[i] = listeners[(size_t)i * stride].profile;
            rc = scatter_assign(e, e->d_stream_profile, e->stream_profile, streams, v.data(), n, s);
            if (rc) return rc;
        }
        if (e->sbank_on) {
            for (int32_t i = 0; i < n; ++i) v[i] = listeners[(size_t)i * stride].word;
            rc = scatter_assign(e, e->sb_word, e->stream_word, streams, v.data(), n, s);
        }
        return rc;
    }
    rc = ensure_listeners(e, s);
    if (rc) return rc;
    rc = stage_stream_list(e, streams, nullptr, n, s);
    if (rc) return rc;
    // rows (EWK_LISTENERS_MAX per listed stream, whatever the caller's stride), then the counts
    HIP_TRY(e->lsn_stage.wait());   // the previous call's rows have left the staging
    ewk_listener* h_rows = e->lsn_stage.as<ewk_listener>();
    int32_t* h_counts = e->lsn_stage.as<int32_t>() + (size_t)n * kLsnRowInts;
    for (int32_t i = 0; i < n; ++i) {
        for (int32_t j = 0; j < EWK_LISTENERS_MAX; ++j)
            h_rows[(size_t)i * EWK_LISTENERS_MAX + j] = j < count[i] ? listeners[(size_t)i * stride + j] : ewk_listener{-1, 0};
        h_counts[i] = count[i];
    }
    HIP_TRY(hipMemcpyAsync(e->d_lsn_stage.p, h_rows, (size_t)n * (kLsnRowInts + 1) * sizeof(int32_t),
                           hipMemcpyHostToDevice, s));
    HIP_TRY(e->lsn_stage.sent(s));
    ListenerSetArgs a;
    memset(&a, 0, sizeof(a));
    a.ids = e->d_ids.p;
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
