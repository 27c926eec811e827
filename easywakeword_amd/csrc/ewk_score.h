// ewk_score.h -- the reference's score arithmetic and the fp64 listing constants, shared by
// the fused scorer (ewk_mfcc.hip, ewk_rescore.h) and the template bank (ewk_bank.hip).
// (kTinyMean and kNanMarginA / kNanMarginB stay in ewk_mfcc.hip, where
// tests/test_rescore_criteria.py reads them; ewk::rescore_criteria() hands them to the bank.)
#pragma once

#include "ewk_internal.h"

namespace ewk {

constexpr int kRescoreFrames = 16;
constexpr double kTinyStd = 20.0;   // |std vector| below which the fp64 path decides (bench batch >= 24.8,
                                    // streaming events >= 32.5: scripts/std_norm_dist.py)

// ---- the score, exactly as WordMatcher.calculate_similarity evaluates it --------
// (wakeword.py:611-625 with scipy 1.15 `correlation`: dist = clip(1 - uv/sqrt(uu*vv), 0, 2)).
// The template u is float32 (librosa.load -> float32 MFCCs).  numpy's dot of two
// float32 vectors is float(sum_double(float(a*b))) (cblas_sdot's scalar path for
// n = 20, verified bit for bit against np.dot); a float32 x float64 or float64 dot
// is a float64 dot.  Two candidate dtypes occur in the reference:
//   float64 (streaming: SoundBuffer slices, wakeword.py:428, 509-513): uu is a
//     float32 dot, uv / vv float64, the rest float64;
//   float32 (WordMatcher on float32 audio): every dot float32 and, under NumPy 2
//     scalar promotion, every following operation float32.
// One operation is not the reference's own: its float32 percent ** 1.5 is libm's powf, which
// no device reproduces bit for bit and which is itself misrounded now and then; the float32
// finishes take pow15f below, the correctly rounded value.  Do not put powf back:
// tests/test_gpu_bank_matrix.py holds the float32 scores to tests/bank_matrix.py's restatement
// of pow15f at less than one float32 ulp.
__device__ __forceinline__ float sdot20(const float* a, const float* b) {
#pragma clang fp contract(off)
    double acc = 0.0;
    for (int i = 0; i < NMFCC; ++i) acc += (double)(a[i] * b[i]);
    return (float)acc;
}

template <typename T>
__device__ __forceinline__ double ddot20(const float* a, const T* b) {
#pragma clang fp contract(off)
    double acc = 0.0;
    for (int i = 0; i < NMFCC; ++i) acc += (double)a[i] * (double)b[i];
    return acc;
}

template <typename T>
__device__ __forceinline__ double ddot20s(const T* a) {
#pragma clang fp contract(off)
    double acc = 0.0;
    for (int i = 0; i < NMFCC; ++i) acc += (double)a[i] * (double)a[i];
    return acc;
}

__device__ __forceinline__ double clip02(double d) {
    if (d < 0.0) return 0.0;
    if (d > 2.0) return 2.0;
    return d;   // NaN passes through (np.clip)
}

__device__ __forceinline__ float clip02f(float d) {
    if (d < 0.0f) return 0.0f;
    if (d > 2.0f) return 2.0f;
    return d;
}

// percent ** 1.5 of a float32 percent (float32 candidates): p * sqrt(p) in double, rounded to
// float32 -- two correctly rounded IEEE operations, so the value is the correctly rounded power
// (a double rounding aside) on any device and host, where powf is whatever each math library
// makes of it: the device's was one float32 ulp off libm's for a fifth of the scores, this is
// for 0.07 % of percents in (0, 100] (libm's own misroundings; DESIGN.md, template bank matrix).
// NaN for p < 0, as powf.
__device__ __forceinline__ float pow15f(float p) {
#pragma clang fp contract(off)
    const double d = (double)p;
    return (float)(d * sqrt(d));
}

// Candidate stats in float64 (the streaming dtype).
__device__ double score_f64cand(const float* tm, const float* ts, const double* cm, const double* cs) {
#pragma clang fp contract(off)
    const double uu_m = (double)sdot20(tm, tm), uu_s = (double)sdot20(ts, ts);
    const double sm = 1.0 - clip02(1.0 - ddot20(tm, cm) / sqrt(uu_m * ddot20s(cm)));
    const double ss = 1.0 - clip02(1.0 - ddot20(ts, cs) / sqrt(uu_s * ddot20s(cs)));
    const double combined = sm * 0.7 + ss * 0.3;
    const double percent = combined * 100.0;
    return pow(percent, 1.5) / 10.0;   // (100**0.5) == 10.0 exactly
}

// Candidate stats in float32 (WordMatcher on float32 audio): float32 arithmetic.
__device__ double score_f32cand(const float* tm, const float* ts, const float* cm, const float* cs) {
#pragma clang fp contract(off)
    float sim[2];
    for (int k = 0; k < 2; ++k) {
        const float* u = k ? ts : tm;
        const float* v = k ? cs : cm;
        const float uu = sdot20(u, u), vv = sdot20(v, v), uv = sdot20(u, v);
        const float prod = uu * vv;                       // float32 * float32
        const float root = (float)sqrt((double)prod);      // math.sqrt, back to float32 (NEP 50)
        const float dist = clip02f(1.0f - uv / root);
        sim[k] = 1.0f - dist;
    }
    const float combined = sim[0] * 0.7f + sim[1] * 0.3f;
    const float percent = combined * 100.0f;
    return (double)(pow15f(percent) / 10.0f);
}

// The same two scores from dot products the caller already holds (the template bank: the
// template's self-dots come from the host, the candidate's are computed once per segment).
// Operation for operation score_f64cand / score_f32cand; percent is the value before the pow.
__device__ __forceinline__ double score_f64cand_dots(double uu_m, double uu_s, double uv_m, double vv_m, double uv_s,
                                                     double vv_s, double& percent) {
#pragma clang fp contract(off)
    const double sm = 1.0 - clip02(1.0 - uv_m / sqrt(uu_m * vv_m));
    const double ss = 1.0 - clip02(1.0 - uv_s / sqrt(uu_s * vv_s));
    const double combined = sm * 0.7 + ss * 0.3;
    percent = combined * 100.0;
    return pow(percent, 1.5) / 10.0;
}

__device__ __forceinline__ double score_f32cand_dots(float uu_m, float uu_s, float uv_m, float vv_m, float uv_s,
                                                     float vv_s) {
#pragma clang fp contract(off)
    const float dm = clip02f(1.0f - uv_m / (float)sqrt((double)(uu_m * vv_m)));
    const float ds = clip02f(1.0f - uv_s / (float)sqrt((double)(uu_s * vv_s)));
    const float combined = (1.0f - dm) * 0.7f + (1.0f - ds) * 0.3f;
    const float percent = combined * 100.0f;
    return (double)(pow15f(percent) / 10.0f);
}

}  // namespace ewk
