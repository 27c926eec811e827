// Host model of the scorer's top_db shift rule (easywakeword_amd/csrc/ewk_topdb_shift.h), in
// float64 on random tiles: the incremental rule (shift_add / shift_rise over a sequence of clamp
// rises, shift_replace for the tiles the rule refuses) against the directly clamped sums.
// Compiled and run by tests/test_topdb_shift_model.py; prints "key value" lines.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../easywakeword_amd/csrc/ewk_topdb_shift.h"

namespace {
constexpr int NB = 128, NC = 20, NF = 16;
uint64_t g_state = 0x9E3779B97F4A7C15ull;
double uni() {   // [0, 1)
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) / 9007199254740992.0;
}
}  // namespace

int main() {
    std::vector<double> D(NC * NB);
    for (int k = 0; k < NC; ++k)
        for (int n = 0; n < NB; ++n)
            D[k * NB + n] = std::sqrt((k ? 2.0 : 1.0) / NB) * std::cos(M_PI * (n + 0.5) * k / NB);
    double worst1 = 0.0, worst2 = 0.0;
    long flag_mismatch = 0, flagged = 0, kept_masked = 0, rises = 0;
    for (int trial = 0; trial < 40; ++trial) {
        const int nt = 2 + (int)(uni() * 12);
        const bool inject = trial % 2 == 1;
        // tile peaks: a random walk that mostly creeps up (ties) and sometimes jumps
        std::vector<double> peak(nt);
        double p = -20.0 + 10.0 * uni();
        for (int t = 0; t < nt; ++t) {
            const double u = uni();
            p += u < 0.5 ? 1e-3 * uni() : (u < 0.8 ? 6.0 * uni() : -3.0 * uni());
            peak[t] = p;
        }
        const double pmax = *std::max_element(peak.begin(), peak.end());
        const double theta = pmax - 80.0, floor_hi = *std::min_element(peak.begin(), peak.end()) - 81.0;
        // raw log-mel: loud entries in [pmax - 60, peak], quiet ones below every clamp
        std::vector<double> raw((size_t)nt * NF * NB);
        for (int t = 0; t < nt; ++t)
            for (int i = 0; i < NF * NB; ++i)
                raw[(size_t)t * NF * NB + i] =
                    uni() < 0.6 ? peak[t] - uni() * (peak[t] - (pmax - 60.0)) : floor_hi - 20.0 * uni();
        for (int t = 0; t < nt; ++t) raw[(size_t)t * NF * NB + (int)(uni() * NF * NB)] = peak[t];
        // the speculative pass
        std::vector<double> run_k(nt), min_above(nt);
        double run = -INFINITY, srun = -INFINITY;
        double s1[NC] = {}, s2[NC] = {}, A[NC] = {}, B[NC] = {}, C[NC] = {}, cref[NC] = {};
        bool any = false;
        for (int t = 0; t < nt; ++t) {
            run = std::max(run, peak[t] - 80.0);
            if (inject && run < theta && uni() < 0.5)   // an unclamped value the final clamp will catch
                raw[(size_t)t * NF * NB + 1 + (int)(uni() * (NF * NB - 1))] = run + (theta - run) * (0.05 + 0.9 * uni());
            if (any && run > srun) {
                for (int k = 0; k < NC; ++k) ewk::shift_rise<double, double>(run - srun, A[k], B[k], C[k], s1[k], s2[k]);
                ++rises;
            }
            srun = run;
            run_k[t] = run;
            min_above[t] = INFINITY;
            for (int f = 0; f < NF; ++f) {
                const double* x = &raw[((size_t)t * NF + f) * NB];
                for (int n = 0; n < NB; ++n)
                    if (x[n] > run) min_above[t] = std::min(min_above[t], x[n]);
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
                    ewk::shift_add<double, double>(d, m, A[k], B[k], C[k]);
                }
            }
            any = true;
        }
        if (theta > srun)
            for (int k = 0; k < NC; ++k) ewk::shift_rise<double, double>(theta - srun, A[k], B[k], C[k], s1[k], s2[k]);
        // the tiles the rule refuses are recomputed; it must refuse exactly the tiles that hold a
        // stored unclamped value in (run_k, theta)
        for (int t = 0; t < nt; ++t) {
            bool window = false;
            for (int i = 0; i < NF * NB; ++i) {
                const double x = raw[(size_t)t * NF * NB + i];
                window = window || (x > run_k[t] && x < theta);
            }
            const bool flag = ewk::shift_flags<double>(min_above[t], theta);
            if (window && !flag) ++flag_mismatch;          // must never be missed
            if (flag) ++flagged; else ++kept_masked;
            if (!flag) continue;
            for (int f = 0; f < NF; ++f) {
                const double* x = &raw[((size_t)t * NF + f) * NB];
                for (int k = 0; k < NC; ++k) {
                    double co = 0.0, cn = 0.0, m = 0.0;
                    for (int n = 0; n < NB; ++n) {
                        co += D[k * NB + n] * std::max(x[n], run_k[t]);
                        cn += D[k * NB + n] * std::max(x[n], theta);
                        m += D[k * NB + n] * (x[n] <= run_k[t] ? 1.0 : 0.0);
                    }
                    ewk::shift_replace(cn, co, m, theta - run_k[t], cref[k], s1[k], s2[k]);
                }
            }
        }
        // the directly clamped sums
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
    std::printf("rel_s1 %.3e\nrel_s2 %.3e\nflag_mismatch %ld\nflagged %ld\nkept %ld\nrises %ld\n", worst1, worst2,
                flag_mismatch, flagged, kept_masked, rises);
    return 0;
}
