// Host model of "top_db masks only where the clamp can still rise" (mask_near / mask_wanted in
// easywakeword_amd/csrc/ewk_topdb_shift.h), in float64 on random tiles in random processing
// orders: for an arbitrary subset of the tiles with clamped entries left without a mask, the
// scorer's bookkeeping -- shift for the masked tiles, per-pass records, recompute of the flagged
// passes (shift_replace for a masked tile, a plain swap for an unmasked one) -- against the sums
// of the tiles clamped at the final threshold directly.  Then the count of near tiles on small
// scout vectors.  Compiled and run by tests/test_topdb_mask_rule.py; prints "key value" lines.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../easywakeword_amd/csrc/ewk_topdb_shift.h"

namespace {
constexpr int NB = 128, NC = 20, NF = 16, NP = 2, FPP = NF / NP;
uint64_t g_state = 0xD1B54A32D192ED03ull;
double uni() {   // [0, 1)
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) / 9007199254740992.0;
}

// The scorer's count: NaN mapped to 0, the tiles with e >= ratio e_max.
int near_count(std::vector<float> e) {
    float emax = 0.0f;
    for (float& x : e) {
        x = x == x ? x : 0.0f;
        emax = std::max(emax, x);
    }
    int n = 0;
    for (float x : e) n += ewk::mask_near(x, emax) ? 1 : 0;
    return n;
}
// Position k of the descending order gets a mask under the count <=> the next tile is near.
long order_mismatch(std::vector<float> e) {
    for (float& x : e) x = x == x ? x : 0.0f;
    std::sort(e.begin(), e.end(), [](float a, float b) { return a > b; });
    const int K = near_count(e);
    long bad = 0;
    for (size_t k = 0; k < e.size(); ++k) {
        const bool next_near = k + 1 < e.size() && ewk::mask_near(e[k + 1], e[0]);
        bad += ewk::mask_wanted((int)k, K) != next_near;
    }
    return bad;
}
}  // namespace

int main() {
    std::vector<double> D(NC * NB);
    for (int k = 0; k < NC; ++k)
        for (int n = 0; n < NB; ++n)
            D[k * NB + n] = std::sqrt((k ? 2.0 : 1.0) / NB) * std::cos(M_PI * (n + 0.5) * k / NB);
    double worst1 = 0.0, worst2 = 0.0;
    long rises = 0, masked_kept = 0, masked_fixed = 0, unmasked_fixed = 0, unmasked_kept = 0, missed = 0;
    long trials_all = 0, trials_none = 0, trials_some = 0;
    for (int trial = 0; trial < 60; ++trial) {
        const int nt = 1 + (int)(uni() * 10);
        const int mode = trial % 3;   // 0: every clamped tile masked, 1: none, 2: a random subset
        (mode == 0 ? trials_all : mode == 1 ? trials_none : trials_some) += 1;
        const bool inject = trial % 2 == 1;
        // tile peaks in processing order: ties, jumps up and steps down
        std::vector<double> peak(nt);
        double p = -20.0 + 10.0 * uni();
        for (int t = 0; t < nt; ++t) {
            const double u = uni();
            p += u < 0.4 ? 1e-3 * uni() : (u < 0.75 ? 6.0 * uni() : -3.0 * uni());
            peak[t] = p;
        }
        const double pmax = *std::max_element(peak.begin(), peak.end());
        const double theta = pmax - 80.0, floor_hi = *std::min_element(peak.begin(), peak.end()) - 81.0;
        std::vector<double> raw((size_t)nt * NF * NB);
        for (int t = 0; t < nt; ++t) {
            const bool loud_only = uni() < 0.2;   // a tile without clamped entries
            for (int i = 0; i < NF * NB; ++i)
                raw[(size_t)t * NF * NB + i] = (loud_only || uni() < 0.6) ? peak[t] - uni() * (peak[t] - (pmax - 60.0))
                                                                          : floor_hi - 20.0 * uni();
            raw[(size_t)t * NF * NB + (int)(uni() * NF * NB)] = peak[t];
        }
        // the speculative pass
        std::vector<double> run_k(nt), rec((size_t)nt * NP);
        std::vector<char> is_masked(nt);
        double run = -INFINITY, srun = -INFINITY;
        double s1[NC] = {}, s2[NC] = {}, A[NC] = {}, B[NC] = {}, C[NC] = {}, cref[NC] = {};
        bool any = false;
        for (int t = 0; t < nt; ++t) {
            run = std::max(run, peak[t] - 80.0);   // the tile's own max included (self-clamp)
            if (inject && run < theta && uni() < 0.5)   // an unclamped value the final clamp will catch
                raw[(size_t)t * NF * NB + 1 + (int)(uni() * (NF * NB - 1))] = run + (theta - run) * (0.05 + 0.9 * uni());
            if (any && run > srun) {
                for (int k = 0; k < NC; ++k) ewk::shift_rise<double, double>(run - srun, A[k], B[k], C[k], s1[k], s2[k]);
                ++rises;
            }
            srun = run;
            run_k[t] = run;
            double tmin = INFINITY;
            for (int i = 0; i < NF * NB; ++i) tmin = std::min(tmin, raw[(size_t)t * NF * NB + i]);
            const bool clamped = tmin < run;
            const bool masked = clamped && (mode == 0 || (mode == 2 && uni() < 0.5));
            is_masked[t] = masked;
            for (int q = 0; q < NP; ++q) {
                double pmin = INFINITY, pmin_above = INFINITY;
                for (int f = q * FPP; f < (q + 1) * FPP; ++f)
                    for (int n = 0; n < NB; ++n) {
                        const double x = raw[((size_t)t * NF + f) * NB + n];
                        pmin = std::min(pmin, x);
                        if (x > run) pmin_above = std::min(pmin_above, x);
                    }
                // a masked tile records the minimum above the clamp, any other the stored minimum
                rec[(size_t)t * NP + q] = masked ? pmin_above : std::max(pmin, run);
            }
            for (int f = 0; f < NF; ++f) {
                const double* x = &raw[((size_t)t * NF + f) * NB];
                for (int k = 0; k < NC; ++k) {
                    double c = 0.0, m = 0.0;
                    for (int n = 0; n < NB; ++n) {
                        c += D[k * NB + n] * std::max(x[n], run);
                        m += D[k * NB + n] * (x[n] <= run ? 1.0 : 0.0);
                    }
                    if (t == 0 && f == 0) cref[k] = c;
                    const double d = c - cref[k];
                    s1[k] += d;
                    s2[k] += d * d;
                    if (masked) {
                        ewk::shift_add<double, double>(d, m, A[k], B[k], C[k]);
                        any = true;
                    }
                }
            }
        }
        if (any && theta > srun)
            for (int k = 0; k < NC; ++k) ewk::shift_rise<double, double>(theta - srun, A[k], B[k], C[k], s1[k], s2[k]);
        // the fix-up: the flagged passes are recomputed and swapped
        for (int t = 0; t < nt; ++t)
            for (int q = 0; q < NP; ++q) {
                bool wrong = false;   // the stored pass differs from the pass clamped at theta
                for (int f = q * FPP; f < (q + 1) * FPP; ++f)
                    for (int n = 0; n < NB; ++n) {
                        const double x = raw[((size_t)t * NF + f) * NB + n];
                        wrong = wrong || (is_masked[t] ? (x > run_k[t] && x < theta) : std::max(x, run_k[t]) < theta);
                    }
                const bool flag = ewk::shift_flags<double>(rec[(size_t)t * NP + q], theta);
                if (wrong && !flag) ++missed;
                if (is_masked[t]) (flag ? masked_fixed : masked_kept) += 1;
                else (flag ? unmasked_fixed : unmasked_kept) += 1;
                if (!flag) continue;
                for (int f = q * FPP; f < (q + 1) * FPP; ++f) {
                    const double* x = &raw[((size_t)t * NF + f) * NB];
                    for (int k = 0; k < NC; ++k) {
                        double co = 0.0, cn = 0.0, m = 0.0;
                        for (int n = 0; n < NB; ++n) {
                            co += D[k * NB + n] * std::max(x[n], run_k[t]);
                            cn += D[k * NB + n] * std::max(x[n], theta);
                            m += D[k * NB + n] * (x[n] <= run_k[t] ? 1.0 : 0.0);
                        }
                        // an unmasked tile never joined A, B, C: its stored columns have not moved
                        if (is_masked[t]) ewk::shift_replace(cn, co, m, theta - run_k[t], cref[k], s1[k], s2[k]);
                        else ewk::shift_replace(cn, co, 0.0, 0.0, cref[k], s1[k], s2[k]);
                    }
                }
            }
        for (int k = 0; k < NC; ++k) {
            double d1 = 0.0, d2 = 0.0, dabs = 0.0;
            for (int t = 0; t < nt; ++t)
                for (int f = 0; f < NF; ++f) {
                    const double* x = &raw[((size_t)t * NF + f) * NB];
                    double c = 0.0;
                    for (int n = 0; n < NB; ++n) c += D[k * NB + n] * std::max(x[n], theta);
                    const double d = c - cref[k];
                    d1 += d;
                    d2 += d * d;
                    dabs += std::fabs(d);
                }
            if (dabs > 0.0) worst1 = std::max(worst1, std::fabs(s1[k] - d1) / dabs);
            if (d2 > 0.0) worst2 = std::max(worst2, std::fabs(s2[k] - d2) / d2);
        }
    }
    std::printf("rel_s1 %.3e\nrel_s2 %.3e\nmissed %ld\nrises %ld\nmasked_kept %ld\nmasked_fixed %ld\n"
                "unmasked_kept %ld\nunmasked_fixed %ld\ntrials_all %ld\ntrials_none %ld\ntrials_some %ld\n",
                worst1, worst2, missed, rises, masked_kept, masked_fixed, unmasked_kept, unmasked_fixed, trials_all,
                trials_none, trials_some);

    // ---- the count of near tiles
    const float r = EWK_MASK_NEAR_RATIO, nanv = std::nanf("");
    std::printf("ratio %.9g\n", (double)r);
    std::printf("k_ties %d\n", near_count({2.5f, 2.5f, 2.5f, 2.5f, 2.5f}));                 // 5: every tile near
    std::printf("k_zero %d\n", near_count({0.0f, 0.0f, 0.0f}));                            // 3: the safe default
    std::printf("k_one %d\n", near_count({7.0f}));                                         // 1
    std::printf("k_one_zero %d\n", near_count({0.0f}));                                    // 1
    std::printf("k_nan %d\n", near_count({nanv, 4.0f, 4.0f * r * 0.5f}));                  // 1: NaN counts as 0
    std::printf("k_all_nan %d\n", near_count({nanv, nanv}));                               // 2: all zero
    std::printf("k_edge %d\n", near_count({8.0f, 8.0f * r, 8.0f * r * 0.999f, 0.0f}));     // 2: e == ratio e_max is near
    std::printf("k_loud_one %d\n", near_count({1.0f, r * 0.5f, r * 0.25f, 0.0f}));         // 1
    long last_masked = 0, single_masked = ewk::mask_wanted(0, 1) ? 1 : 0;
    for (int nt = 1; nt <= 64; ++nt)
        for (int K = 0; K <= nt; ++K) last_masked += ewk::mask_wanted(nt - 1, K) ? 1 : 0;
    std::printf("last_masked %ld\nsingle_masked %ld\n", last_masked, single_masked);
    long bad = 0;
    for (int trial = 0; trial < 2000; ++trial) {
        std::vector<float> e(1 + (int)(uni() * 12));
        for (float& x : e) {
            const double u = uni();
            x = u < 0.1 ? 0.0f : u < 0.15 ? nanv : u < 0.4 ? 1.0f : (float)std::pow(10.0, -3.0 * uni());
        }
        bad += order_mismatch(e);
    }
    std::printf("order_mismatch %ld\n", bad);
    return 0;
}
