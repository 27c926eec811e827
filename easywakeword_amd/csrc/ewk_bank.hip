// ewk_bank.hip -- template bank: the cosine score of every segment's MFCC statistics against
// the templates of one word (several recordings of it), one lane per template.
//
// A segment's whole MFCC result is its mean[20] / std[20]; the score against one more
// template is a few hundred flops on those 160 bytes.  So the bank is a pass of its own over
// the statistics the fused scorer leaves (k_score_f32 without a template), not a wider
// epilogue inside it:
//   k_bank<float>   every segment from its float32 statistics; lists the segments those
//                   cannot decide (the single-template epilogue's rule, per template)
//   k_bank<double>  the listed segments again from the fp64 statistics of the list_all path
// A segment takes a group of G lanes, G the power of two that holds the bank's largest word
// (64: a whole wave), so a wave scores 64 / G segments per step: lane j of a group keeps
// template word_first[w] + j in registers (40 values and its two self-dots, loaded value-major
// so the group's loads are contiguous) and reloads only when its group's word changes from one
// step to the next.  The segment's 40 statistics and its own self-dots are the same in every
// lane of its group.  The arithmetic is the reference's (ewk_score.h): sequential 20-term dots,
// no contraction, pow(percent, 1.5) / 10 -- for float32 candidates pow15f(percent) / 10, the
// correctly rounded p * sqrt(p) and on purpose not powf (ewk_score.h says why).
//
// The stream bank (k_bank_events) is the same pass over the pending events of a streaming
// tick: bank_pass is the one body, a source policy says where its items come from and where
// the results go (BatchSrc: a linear batch; EventSrc: the event queue of a ring-mode pass).
#include <hip/hip_runtime.h>
#include <math.h>

#include "ewk_internal.h"
#include "ewk_rs_list.h"
#include "ewk_score.h"

namespace ewk {

constexpr int kBankWaves = 4;   // waves per workgroup
constexpr int kBankRun = 16;    // segments per wave and run, at least (one step's 64 / G when that is more)

// ST: the statistics' type.  float: pass over every item (index = item).  double: the re-score
// of the listed items (index = list position).
//
// A source policy SRC (ST-specific) provides
//   item(i, seg, w, len)   item i < n: its segment / event slot, its word (-1: leave it alone)
//                          and its length in samples (read by the float32 pass only)
//   row(i, seg)            row of the item's statistics in BankArgs::mean / stdv
//   scores(seg)            nullptr or the segment's row of per-template scores
//   emit(seg, okw, ...)    lane 0 of the group: the item's result
//   list(seg, len)         lane 0 of the group (float32 pass): the item needs the fp64 statistics
//   kStride                the waves stride over the items (else: the grid covers them, one run each)
//   kF32Cand               BankArgs::cand_f32 may ask for float32 candidates
//
// Wave `run0` of `run_stride` takes runs run0, run0 + run_stride, ... of steps * per items.
// Every lane runs every step (ballots and shuffles span the wave): a lane without an item,
// with a word index outside the bank or past its word's size only carries NaN.
template <typename ST, typename SRC>
__device__ __forceinline__ void bank_pass(const BankArgs& a, const SRC& src, int n, int run0, int run_stride) {
    constexpr bool kRescore = sizeof(ST) == sizeof(double);
    const int lane = threadIdx.x & 63;
    const int G = 1 << a.group_log2;        // lanes per segment
    const int per = 64 >> a.group_log2;     // segments per step
    const int j = lane & (G - 1);           // template within the word
    const int g = lane >> a.group_log2;     // segment within the step
    const unsigned long long gmask = (G == 64 ? ~0ull : (1ull << G) - 1) << (g * G);
    // (a striding source has few items for its grid -- a tick's events: one step per run spreads them)
    const int steps = SRC::kStride ? 1 : max(kBankRun, per) / per;
    const double nan = __builtin_nan("");
    float tm[NMFCC], ts[NMFCC], uu_m = 0.0f, uu_s = 0.0f;
#pragma unroll
    for (int c = 0; c < NMFCC; ++c) tm[c] = ts[c] = 0.0f;
    int cur = -1, first = 0, size = 0;
    double thr = 0.0;
    // (wave-uniform; a source whose grid covers its items -- !kStride -- makes one run per wave)
    const int run_len = steps * per;
    for (int i0 = run0 * run_len; i0 < n; i0 += run_stride * run_len) {
        for (int t = 0; t < steps; ++t) {
            if (i0 + t * per >= n) break;     // (wave-uniform)
            const int i = i0 + t * per + g;
            const bool live = i < n;
            int seg = 0, w = -1, len = 0;
            if (live) src.item(i, seg, w, len);
            // (device batches can carry any index: the host call checks its own)
            const bool okw = live && w >= 0 && w < a.n_words;
            if (okw && w != cur) {
                cur = w;
                first = a.word_first[w];
                size = a.word_first[w + 1] - first;
                thr = a.thresholds[w];
                const float* base = a.bank + (int64_t)kBankRow * first;
                const bool ld = j < size;
#pragma unroll
                for (int c = 0; c < NMFCC; ++c) {
                    tm[c] = ld ? base[c * size + j] : 0.0f;
                    ts[c] = ld ? base[(NMFCC + c) * size + j] : 0.0f;
                }
                uu_m = ld ? base[2 * NMFCC * size + j] : 0.0f;
                uu_s = ld ? base[(2 * NMFCC + 1) * size + j] : 0.0f;
            }
            const bool act = okw && j < size;
            const int64_t row = live ? src.row(i, seg) : 0;
            const ST* pm = static_cast<const ST*>(a.mean) + row * NMFCC;
            const ST* ps = static_cast<const ST*>(a.stdv) + row * NMFCC;
            double score, std2, mean2;
            bool sure_nan = false;
            if (SRC::kF32Cand && a.cand_f32) {   // float32 candidates: float products, float-rounded dots (sdot)
                float cm[NMFCC], cs[NMFCC];
#pragma unroll
                for (int c = 0; c < NMFCC; ++c) {
                    cm[c] = (float)pm[c];
                    cs[c] = (float)ps[c];
                }
                const float vv_m = sdot20(cm, cm), vv_s = sdot20(cs, cs);   // (the same in the whole group)
                score = score_f32cand_dots(uu_m, uu_s, sdot20(tm, cm), vv_m, sdot20(ts, cs), vv_s);
                std2 = vv_s;
                mean2 = vv_m;
            } else {
                double cm[NMFCC], cs[NMFCC];
#pragma unroll
                for (int c = 0; c < NMFCC; ++c) {
                    cm[c] = (double)pm[c];
                    cs[c] = (double)ps[c];
                }
                const double vv_m = ddot20s(cm), vv_s = ddot20s(cs);        // (the same in the whole group)
                double percent;
                score = score_f64cand_dots((double)uu_m, (double)uu_s, ddot20(tm, cm), vv_m, ddot20(ts, cs), vv_s,
                                           percent);
                std2 = vv_s;
                mean2 = vv_m;
                // (a vanishing-mean score that is NaN beyond the float32 error: ewk_mfcc.hip)
                sure_nan = percent < -(a.crit.nan_a / sqrt(mean2) + a.crit.nan_b);
            }
            if (!act) score = nan;
            const bool valid = score == score;
            const unsigned long long hit = (__ballot(valid && score >= thr) & gmask) >> (g * G);
            // best score of the group ignoring NaN, lowest lane on ties (64: no score yet)
            double bs = score;
            int bl = valid ? j : 64;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                if (d < G) {   // (wave-uniform; lane ^ d stays inside the group)
                    const double os = __shfl_xor(bs, d, 64);
                    const int ol = __shfl_xor(bl, d, 64);
                    if (ol < 64 && (bl == 64 || os > bs || (os == bs && ol < bl))) {
                        bs = os;
                        bl = ol;
                    }
                }
            }
            double* srow = live ? src.scores(seg) : nullptr;
            if (srow)
                for (int k = j; k < a.stride; k += G) srow[k] = k < G ? score : nan;
            bool list = false;
            const unsigned long long near_b = __ballot(act && fabs(score - thr) < a.rescore_margin) & gmask;
            const unsigned long long unsure_b = __ballot(act && !sure_nan) & gmask;
            if (!kRescore && okw) {
                // the single-template epilogue's listing rule (score_epilogue), per template
                list = near_b != 0 || (1 + len / HOP) <= kRescoreFrames || (std2 > 0.0 && std2 < kTinyStd * kTinyStd) ||
                       (mean2 < a.crit.tiny_mean * a.crit.tiny_mean && unsure_b != 0);
            }
            if (live && j == 0) {
                src.emit(seg, okw, bl < 64 ? bs : nan, bl < 64 ? bl : -1, first, hit);
                if (list) src.list(seg, len);   // at most once per item, so the list never outgrows the pass
            }
        }
        if (!SRC::kStride) break;
    }
}

// A linear batch: segment i of the batch (float32 pass) / of the list (fp64 pass).
template <typename ST>
struct BatchSrc {
    static constexpr bool kRescore = sizeof(ST) == sizeof(double);
    static constexpr bool kStride = false, kF32Cand = true;
    const BankArgs& a;
    __device__ void item(int i, int& seg, int& w, int& len) const {
        seg = kRescore ? a.list_seg[i] : i;
        w = a.word ? a.word[seg] : 0;
        len = kRescore ? 0 : a.lengths[seg];
    }
    __device__ int64_t row(int i, int) const { return i; }
    __device__ double* scores(int seg) const {
        return a.out_scores ? a.out_scores + (int64_t)seg * a.stride : nullptr;
    }
    __device__ void emit(int seg, bool, double best, int bl, int first, unsigned long long hit) const {
        ewk_bank_result r;
        r.best_score = best;
        r.hit_mask = hit;
        r.best_tmpl = bl >= 0 ? first + bl : -1;
        r.match = hit != 0;
        r.rescored = kRescore ? 1 : 0;
        r.pad = 0;
        a.out[seg] = r;
    }
    __device__ void list(int seg, int len) const {
        const int p = atomicAdd(a.list_cnt, 1);
        a.list_seg[p] = seg;
        a.list_off[p] = a.offsets[seg];
        a.list_len[p] = len;
    }
};

template <typename ST>
__global__ __launch_bounds__(64 * kBankWaves, 2) void k_bank(BankArgs a) {
    const BatchSrc<ST> src{a};
    bank_pass<ST>(a, src, a.n, blockIdx.x * kBankWaves + (threadIdx.x >> 6), gridDim.x * kBankWaves);
}

// The events of a streaming tick: event slot base + i of the pending window (float32 pass) /
// slot ev_list[kEvListHdr + i] (fp64 pass).  Statistics are by event slot in both passes.  An
// event's word is its stream's, or its listener's when listener j >= 1 cut it; a skipped event (EWK_EV_SKIPPED: no level-2 call) is left alone.
template <typename ST>
struct EventSrc {
    static constexpr bool kRescore = sizeof(ST) == sizeof(double);
    static constexpr bool kStride = true, kF32Cand = false;   // (ring segments are float64 candidates)
    const ScoreArgs& s;
    const BankEvArgs& x;
    int base;
    __device__ void item(int i, int& seg, int& w, int& len) const {
        seg = kRescore ? x.ev_list[kEvListHdr + i] : base + i;
        const ewk_event* ev = s.events + seg;
        len = ev->length;
        const int lj = EWK_EV_LISTENER(ev->flags);   // (listener 0's word is the stream's)
        if (ev->flags & EWK_EV_SKIPPED) w = -1;
        else if (lj && x.lsn_tab) w = x.lsn_tab[(int64_t)ev->stream * EWK_LISTENERS_MAX + lj].word;
        else w = x.stream_word ? x.stream_word[ev->stream] : 0;
    }
    __device__ int64_t row(int, int seg) const { return seg; }
    __device__ double* scores(int) const { return nullptr; }
    __device__ void emit(int seg, bool okw, double best, int bl, int, unsigned long long hit) const {
        if (!okw) return;
        ewk_event* ev = s.events + seg;
        ev->score = best;
        ev->match = hit != 0;   // (some template >= the threshold: the best is)
        ev->flags = (ev->flags & ~(63 << EWK_EV_BEST_SHIFT)) | EWK_EV_BANK | (kRescore ? EWK_EV_RESCORED : 0) |
                    (bl >= 0 ? bl << EWK_EV_BEST_SHIFT : 0);
    }
    __device__ void list(int seg, int len) const {
        // (a full re-score list leaves the float32 result standing: no fp64 statistics to read)
        if (rs_list(s, seg, len, s.out_theta[seg])) x.ev_list[kEvListHdr + atomicAdd(&x.ev_list[0], 1)] = seg;
    }
};

template <typename ST>
__global__ __launch_bounds__(64 * kBankWaves, 2) void k_bank_events(BankArgs a, ScoreArgs s, BankEvArgs x) {
    constexpr bool kRescore = sizeof(ST) == sizeof(double);
    int base = 0, n;
    if (kRescore) {
        n = min(x.ev_list[0], s.n_seg);
    } else {   // the pending window, as k_score_f32 reads it (a tick without an event: n <= 0)
        base = max(0, (int)((uint32_t)*s.ev_base - (uint32_t)s.ev_base0));
        n = min((int)((uint32_t)*s.n_events - (uint32_t)s.ev_base0), s.n_seg) - base;
    }
    if (n <= 0) return;
    const EventSrc<ST> src{s, x, base};
    bank_pass<ST>(a, src, n, blockIdx.x * kBankWaves + (threadIdx.x >> 6), gridDim.x * kBankWaves);
    if (kRescore) {
        // every workgroup read the count above; the last one out re-arms the list for the next pass
        __syncthreads();
        if (threadIdx.x == 0 && atomicAdd(&x.ev_list[1], 1) == (int)gridDim.x - 1) {
            x.ev_list[0] = 0;
            x.ev_list[1] = 0;
        }
    }
}

static int group_log2(int max_word) {
    int l = 0;
    while ((1 << l) < max_word) ++l;
    return l;
}

static int bank_grid(const BankArgs& a) {
    const int per_wave = std::max(kBankRun, 64 >> a.group_log2);   // (bank_pass: steps * per)
    const int waves = (a.n + per_wave - 1) / per_wave;
    return (waves + kBankWaves - 1) / kBankWaves;
}

hipError_t launch_bank_score(const BankArgs& a0, hipStream_t s) {
    if (a0.n <= 0) return hipSuccess;
    if (a0.max_word < 1 || a0.max_word > EWK_BANK_MAX_PER_WORD) return hipErrorInvalidValue;
    BankArgs a = a0;
    a.group_log2 = group_log2(a.max_word);
    hipError_t e = hipMemsetAsync(a.list_cnt, 0, sizeof(int32_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_bank<float>, dim3(bank_grid(a)), dim3(64 * kBankWaves), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_bank_rescore(const BankArgs& a0, hipStream_t s) {
    if (a0.n <= 0) return hipSuccess;
    if (a0.max_word < 1 || a0.max_word > EWK_BANK_MAX_PER_WORD) return hipErrorInvalidValue;
    BankArgs a = a0;
    a.group_log2 = group_log2(a.max_word);
    hipLaunchKernelGGL(k_bank<double>, dim3(bank_grid(a)), dim3(64 * kBankWaves), 0, s, a);
    return hipGetLastError();
}

template <typename ST>
static hipError_t launch_events(const BankArgs& b0, const ScoreArgs& a, const BankEvArgs& x, hipStream_t s) {
    if (a.n_seg <= 0 || x.grid <= 0) return hipSuccess;
    if (b0.max_word < 1 || b0.max_word > EWK_BANK_MAX_PER_WORD || !a.events || !x.ev_list) return hipErrorInvalidValue;
    BankArgs b = b0;
    b.group_log2 = group_log2(b.max_word);
    b.cand_f32 = 0;   // ring segments are float64 candidates
    b.out_scores = nullptr;
    hipLaunchKernelGGL(k_bank_events<ST>, dim3(x.grid), dim3(64 * kBankWaves), 0, s, b, a, x);
    return hipGetLastError();
}

hipError_t launch_bank_events(const BankArgs& b, const ScoreArgs& a, const BankEvArgs& x, hipStream_t s) {
    if (!b.mean || !b.stdv || !a.out_theta || !a.rs_slots) return hipErrorInvalidValue;
    return launch_events<float>(b, a, x, s);
}

hipError_t launch_bank_events_rescore(const BankArgs& b, const ScoreArgs& a, const BankEvArgs& x, hipStream_t s) {
    if (!b.mean || !b.stdv) return hipErrorInvalidValue;
    return launch_events<double>(b, a, x, s);
}

}  // namespace ewk
