// ewk_engine_score.cpp -- the C ABI's batch side: level-2 scoring of segment batches against the
// template or the template bank, level-3 input, positives compaction, PCM16 decode.
#include "ewk_engine.h"

using namespace ewk;

// What every scorer launch takes from the engine (linear re-score counters; no segments yet).
ScoreArgs ewk::base_args(ewk_engine* e) {
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

// A linear batch (device pointers); the caller adds its outputs.
static ScoreArgs linear_args(ewk_engine* e, const float* d_pcm, const int64_t* d_off, const int32_t* d_len, int32_t n,
                             int32_t flags) {
    ScoreArgs a = base_args(e);
    a.cand_f32 = (flags & EWK_SCORE_F32_CANDIDATES) ? 1 : 0;
    a.pcm = d_pcm;
    a.offsets = d_off;
    a.lengths = d_len;
    a.n_seg = n;
    return a;
}

// Every segment through the fp64 path (statistics into mean64 / std64): the float32 pass only
// supplies the speculative top_db clamp of each segment (its own scores are overwritten).
static void all_through_fp64(ewk_engine* e, ScoreArgs* a) {
    a->list_all = 1;
    a->rs_slots = e->rs_slots.p;
    a->out_mean64 = e->mean64.p;
    a->out_std64 = e->std64.p;
}

// f32 scorer + fp64 rescoring of the near-threshold list, all on `s`.
static int score_linear(ewk_engine* e, const float* d_pcm, const int64_t* d_off, const int32_t* d_len, int32_t n,
                        float* d_mean, float* d_std, double* d_score, uint8_t* d_match, int32_t flags,
                        hipStream_t s) {
    ScoreArgs a = linear_args(e, d_pcm, d_off, d_len, n, flags);
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

static int check_segments(const int64_t* offsets, const int32_t* lengths, int32_t n_seg, int64_t n_pcm) {
    for (int32_t i = 0; i < n_seg; ++i)
        if (lengths[i] < 0 || offsets[i] < 0 || offsets[i] + lengths[i] > n_pcm)
            return fail(EWK_EINVAL, "segment " + std::to_string(i) + " out of range of pcm");
    return EWK_OK;
}

// A host batch into the engine's staging (e->pcm, e->offsets, e->lengths) on s, behind every
// scoring pass in flight.
static int upload_segments(ewk_engine* e, const float* pcm, int64_t n_pcm, const int64_t* offsets,
                           const int32_t* lengths, int32_t n_seg, hipStream_t s) {
    HIP_TRY(e->pcm.reserve(std::max<int64_t>(n_pcm, 1)));
    HIP_TRY(e->offsets.reserve(n_seg));
    HIP_TRY(e->lengths.reserve(n_seg));
    HIP_TRY(join_scoring(e, s));
    if (n_pcm > 0) HIP_TRY(hipMemcpyAsync(e->pcm.p, pcm, n_pcm * sizeof(float), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(e->offsets.p, offsets, n_seg * sizeof(int64_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(e->lengths.p, lengths, n_seg * sizeof(int32_t), hipMemcpyHostToDevice, s));
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
    int rc = check_segments(offsets, lengths, n_seg, n_pcm);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(reserve_rescore(e, n_seg));
    HIP_TRY(e->mean.reserve((size_t)n_seg * NMFCC));
    HIP_TRY(e->stdv.reserve((size_t)n_seg * NMFCC));
    HIP_TRY(e->score.reserve(n_seg));
    HIP_TRY(e->match.reserve(n_seg));
    hipStream_t s = e->stream;
    rc = upload_segments(e, pcm, n_pcm, offsets, lengths, n_seg, s);
    if (rc) return rc;
    ScoreArgs a = linear_args(e, e->pcm.p, e->offsets.p, e->lengths.p, n_seg, flags);
    a.out_mean = e->mean.p;
    a.out_std = e->stdv.p;
    a.out_score = e->score.p;
    a.out_match = e->match.p;
    HIP_TRY(launch_score_f32(e->d_tab, a, 0, s));   // (zeroes the work and re-score counters)
    HIP_TRY(launch_rescore_linear(a, s));
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
    int rc = check_segments(offsets, lengths, n_seg, n_pcm);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    HIP_TRY(reserve_rescore(e, n_seg));
    HIP_TRY(e->mean64.reserve((size_t)n_seg * NMFCC));
    HIP_TRY(e->std64.reserve((size_t)n_seg * NMFCC));
    HIP_TRY(e->score.reserve(n_seg));
    rc = upload_segments(e, pcm, n_pcm, offsets, lengths, n_seg, s);
    if (rc) return rc;
    ScoreArgs a = linear_args(e, e->pcm.p, e->offsets.p, e->lengths.p, n_seg, flags);
    a.out_score = e->score.p;
    all_through_fp64(e, &a);
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
static const char* kStreamBankOn = "disable the stream bank first";

int ewk::fail_word_index(int32_t word, WordOf of, int32_t i, int32_t n_words) {
    return fail(EWK_EINVAL, "word index " + std::to_string(word) + (of == kOfStream ? " of stream " : " of segment ") +
                                std::to_string(i) + " is outside [0, " + std::to_string(n_words) + ")");
}

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
int ewk::bank_follow_threshold(ewk_engine* e, hipStream_t s) {
    if (!e->bank_thr_follow || e->bank_thr[0] == e->cfg.similarity_threshold) return EWK_OK;
    std::fill(e->bank_thr.begin(), e->bank_thr.end(), e->cfg.similarity_threshold);
    HIP_TRY(hipMemcpyAsync(e->d_bank_thr.p, e->bank_thr.data(), e->bank_thr.size() * sizeof(double),
                           hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));   // (the copy reads bank_thr)
    return EWK_OK;
}

// What every bank pass takes from the engine's bank.
BankArgs ewk::bank_args(ewk_engine* e) {
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
    ScoreArgs a = linear_args(e, d_pcm, d_off, d_len, n, 0);
    a.has_template = 0;   // pass 1: statistics only, nothing listed
    a.rs_slots = nullptr;
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
    ScoreArgs f = linear_args(e, d_pcm, e->bk_off.p, e->bk_len.p, listed, 0);
    f.has_template = 0;
    all_through_fp64(e, &f);
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
    rc = check_segments(offsets, lengths, n_seg, n_pcm);
    if (rc) return rc;
    const int32_t n_words = (int32_t)e->bank_first.size() - 1;
    if (word)
        for (int32_t i = 0; i < n_seg; ++i)
            if (word[i] < 0 || word[i] >= n_words) return fail_word_index(word[i], kOfSegment, i, n_words);
    HIP_TRY(hipSetDevice(e->device));
    const size_t n_sc = out_scores ? (size_t)n_seg * stride : 0;
    HIP_TRY(e->bk_word.reserve(n_seg));
    HIP_TRY(e->bk_out.reserve(n_seg));
    if (n_sc) HIP_TRY(e->bk_scores.reserve(n_sc));
    hipStream_t s = e->stream;
    rc = upload_segments(e, pcm, n_pcm, offsets, lengths, n_seg, s);
    if (rc) return rc;
    if (word) HIP_TRY(hipMemcpyAsync(e->bk_word.p, word, n_seg * sizeof(int32_t), hipMemcpyHostToDevice, s));
    rc = bank_score(e, e->pcm.p, e->offsets.p, e->lengths.p, n_seg, word ? e->bk_word.p : nullptr, e->bk_out.p,
                    n_sc ? e->bk_scores.p : nullptr, stride, flags, s);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out, e->bk_out.p, n_seg * sizeof(ewk_bank_result), hipMemcpyDeviceToHost, s));
    if (n_sc) HIP_TRY(hipMemcpyAsync(out_scores, e->bk_scores.p, n_sc * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
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
    DevBuf<int64_t> d_oo, d_off;
    DevBuf<int32_t> d_len;
    DevBuf<ewk_event> d_ev;
    DevBuf<double> d_out;
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
    DevBuf<float> tmp;
    if (!(flags & EWK_PCM_DEVICE)) {
        HIP_TRY(tmp.reserve(std::max<int64_t>(1, n_pcm)));
        HIP_TRY(hipMemcpyAsync(tmp.p, pcm, n_pcm * sizeof(float), hipMemcpyHostToDevice, e->stream));
        d_pcm = tmp.p;
    }
    return normalize_impl(e, d_pcm, offsets, lengths, nullptr, n_seg, out, flags);
}

int ewk::check_ring_events(ewk_engine* e, const ewk_event* events, int32_t n) {
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
    return EWK_OK;
}

int ewk_normalize_events(ewk_engine* e, const ewk_event* events, int32_t n, double* out, int32_t flags) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (n < 0) return fail(EWK_EINVAL, "negative size");
    if (n == 0) return EWK_OK;
    if (!events || !out) return fail(EWK_EINVAL, "NULL argument");
    int rc = check_ring_events(e, events, n);
    if (rc) return rc;
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
    DevBuf<int16_t> d_in;
    DevBuf<float> d_out;
    HIP_TRY(d_in.reserve(n));
    HIP_TRY(d_out.reserve(n));
    HIP_TRY(hipMemcpyAsync(d_in.p, in, n * sizeof(int16_t), hipMemcpyHostToDevice, s));
    HIP_TRY(launch_decode_pcm16(d_in.p, d_out.p, n, s));
    HIP_TRY(hipMemcpyAsync(out, d_out.p, n * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return EWK_OK;
}

int ewk_g711_table(int32_t law, int16_t* out256) {
    if (law != EWK_G711_ULAW && law != EWK_G711_ALAW)
        return fail(EWK_EINVAL, "law = " + std::to_string(law) + " is neither EWK_G711_ULAW (0) nor EWK_G711_ALAW (1)");
    if (!out256) return fail(EWK_EINVAL, "NULL argument");
    for (uint32_t b = 0; b < 256; ++b) out256[b] = (int16_t)g711_decode(b, law);
    return EWK_OK;
}

int ewk_decode_g711(ewk_engine* e, const uint8_t* in, int64_t n, float* out, int32_t law, int32_t flags) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (n < 0) return fail(EWK_EINVAL, "negative size");
    if (law != EWK_G711_ULAW && law != EWK_G711_ALAW)
        return fail(EWK_EINVAL, "law = " + std::to_string(law) + " is neither EWK_G711_ULAW (0) nor EWK_G711_ALAW (1)");
    if (n == 0) return EWK_OK;
    if (!in || !out) return fail(EWK_EINVAL, "NULL argument");
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    if (flags & EWK_PCM_DEVICE) {   // both pointers device memory; asynchronous
        HIP_TRY(launch_decode_g711(in, out, n, law, s));
        return EWK_OK;
    }
    DevBuf<uint8_t> d_in;
    DevBuf<float> d_out;
    HIP_TRY(d_in.reserve(n));
    HIP_TRY(d_out.reserve(n));
    HIP_TRY(hipMemcpyAsync(d_in.p, in, n, hipMemcpyHostToDevice, s));
    HIP_TRY(launch_decode_g711(d_in.p, d_out.p, n, law, s));
    HIP_TRY(hipMemcpyAsync(out, d_out.p, n * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return EWK_OK;
}
