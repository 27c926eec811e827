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
// no contraction, pow(percent, 1.5) / 10.
#include <hip/hip_runtime.h>
#include <math.h>

#include "ewk_internal.h"
#include "ewk_score.h"

namespace ewk {

constexpr int kBankWaves = 4;   // waves per workgroup
constexpr int kBankRun = 16;    // segments per wave, at least (one step's 64 / G when that is more)

// ST: the statistics' type.  float: pass over every segment (index = segment).  double: the
// re-score of the listed segments (index = list position, segment = list_seg[index]).
// Every lane runs every step (ballots and shuffles span the wave): a lane without a segment,
// with a word index outside the bank or past its word's size only carries NaN.
template <typename ST>
__global__ __launch_bounds__(64 * kBankWaves) void k_bank(BankArgs a) {
    constexpr bool kRescore = sizeof(ST) == sizeof(double);
    const int lane = threadIdx.x & 63;
    const int G = 1 << a.group_log2;        // lanes per segment
    const int per = 64 >> a.group_log2;     // segments per step
    const int j = lane & (G - 1);           // template within the word
    const int g = lane >> a.group_log2;     // segment within the step
    const unsigned long long gmask = (G == 64 ? ~0ull : (1ull << G) - 1) << (g * G);
    const int wave = blockIdx.x * kBankWaves + (threadIdx.x >> 6);
    const int steps = max(kBankRun, per) / per;
    const int i0 = wave * steps * per;
    const double nan = __builtin_nan("");
    float tm[NMFCC], ts[NMFCC], uu_m = 0.0f, uu_s = 0.0f;
#pragma unroll
    for (int c = 0; c < NMFCC; ++c) tm[c] = ts[c] = 0.0f;
    int cur = -1, first = 0, size = 0;
    double thr = 0.0;
    for (int t = 0; t < steps; ++t) {
        if (i0 + t * per >= a.n) break;     // (wave-uniform)
        const int i = i0 + t * per + g;
        const bool live = i < a.n;
        int seg = 0, w = -1;
        if (live) {
            seg = kRescore ? a.list_seg[i] : i;
            w = a.word ? a.word[seg] : 0;
        }
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
        const ST* pm = static_cast<const ST*>(a.mean) + (int64_t)(live ? i : 0) * NMFCC;
        const ST* ps = static_cast<const ST*>(a.stdv) + (int64_t)(live ? i : 0) * NMFCC;
        double score, std2, mean2;
        bool sure_nan = false;
        if (a.cand_f32) {   // float32 candidates: float products, float-rounded dots (sdot)
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
        if (a.out_scores && live) {
            double* row = a.out_scores + (int64_t)seg * a.stride;
            for (int k = j; k < a.stride; k += G) row[k] = k < G ? score : nan;
        }
        bool list = false;
        int len = 0;
        const unsigned long long near_b = __ballot(act && fabs(score - thr) < a.rescore_margin) & gmask;
        const unsigned long long unsure_b = __ballot(act && !sure_nan) & gmask;
        if (!kRescore && okw) {
            // the single-template epilogue's listing rule (score_epilogue), per template
            len = a.lengths[seg];
            list = near_b != 0 || (1 + len / HOP) <= kRescoreFrames || (std2 > 0.0 && std2 < kTinyStd * kTinyStd) ||
                   (mean2 < a.crit.tiny_mean * a.crit.tiny_mean && unsure_b != 0);
        }
        if (live && j == 0) {
            ewk_bank_result r;
            r.best_score = bl < 64 ? bs : nan;
            r.hit_mask = hit;
            r.best_tmpl = bl < 64 ? first + bl : -1;
            r.match = hit != 0;
            r.rescored = kRescore ? 1 : 0;
            r.pad = 0;
            a.out[seg] = r;
            if (list) {   // at most once per segment, so the list never outgrows the batch
                const int p = atomicAdd(a.list_cnt, 1);
                a.list_seg[p] = seg;
                a.list_off[p] = a.offsets[seg];
                a.list_len[p] = len;
            }
        }
    }
}

static int group_log2(int max_word) {
    int l = 0;
    while ((1 << l) < max_word) ++l;
    return l;
}

static int bank_grid(const BankArgs& a) {
    const int per_wave = std::max(kBankRun, 64 >> a.group_log2);   // (k_bank: steps * per)
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

}  // namespace ewk
