// ewk_gate_detect.h -- the listener lanes' _detect_word state and step (included by ewk_gate.hip).
#pragma once

#include "ewk_gate_pwsum.h"

namespace ewk {

// Listener j >= 1 on its lane (LSN kernels).  The kernels without listeners use 104-124 of the 128
// VGPRs that 4 waves per SIMD allow, and ten more per lane for a whole LsnState spilled in every
// family; so a lane keeps in two registers what every tick reads -- state and re-entry count
// (packed), profile index -- with whether it has a re-entry timeout, and its four times in the
// wave's LDS (the lane's own words at stride 16, 512 B per wave; the address is formed from the
// lane index where it is used), read and written on a transition only.
typedef double __attribute__((address_space(3))) LdsDouble;
typedef LdsDouble* LdsTimes;
struct LsnLane {
    LdsTimes base;        // the wave's LDS words (wave-uniform)
    int32_t lane;
    int32_t sr;           // reentries << 2 | state
    int32_t pi;           // profile index (-1: the launch's timings)
    bool timeout;         // the listener's re-entry timeout is positive
    __device__ __forceinline__ int state() const { return sr & 3; }
    __device__ __forceinline__ void set_state(int v) { sr = (sr & ~3) | v; }
    __device__ __forceinline__ LdsTimes t() const { return base + (lane_here(lane) & 15); }
    __device__ __forceinline__ LdsDouble& silence_start() { return t()[0]; }
    __device__ __forceinline__ LdsDouble& sound_start() { return t()[16]; }
    __device__ __forceinline__ LdsDouble& sound_end() { return t()[32]; }
    __device__ __forceinline__ LdsDouble& start_time() { return t()[48]; }
};

// One _detect_word step of listener j >= 1: the FSM and the cut of k_gate_ticks' listener 0,
// operation for operation, on the lane's own state.  The six timings are read from the
// listener's profile where they are compared -- a state transition or the cut -- as per-lane
// loads, rare and divergent; none is live across a tick.
__device__ __forceinline__ void lsn_step(LsnLane& ls, const GateArgs& g, bool silent, double now, int s, int j,
                                         int64_t tick, int spos, int R, int Rs) {
    const ewk_detector_profile* pf = ls.pi >= 0 ? g.profiles + ls.pi : nullptr;
#define EWK_LSN_TIMING(field) (pf ? pf->field : g.field)
    switch (ls.state()) {
    case kWaiting:
        if (silent) { ls.set_state(kInSilence); ls.silence_start() = now; }
        break;
    case kInSilence:
        if (!silent) {
            if (now - ls.silence_start() >= EWK_LSN_TIMING(pre_speech_silence)) { ls.set_state(kInSound); ls.sound_start() = now; }
            else ls.set_state(kWaiting);
        }
        break;
    case kInSound: {
        const double d = now - ls.sound_start();
        if (!silent) {
            if (d > EWK_LSN_TIMING(speech_duration_max)) ls.set_state(kWaiting);
        } else {
            if (EWK_LSN_TIMING(speech_duration_min) <= d && d <= EWK_LSN_TIMING(speech_duration_max)) {
                ls.set_state(kAfterSound);
                ls.sound_end() = now;
            } else ls.set_state(kWaiting);
        }
        break;
    }
    case kAfterSound:
        if (silent) {
            const double sound_end = ls.sound_end();
            if (now - sound_end >= EWK_LSN_TIMING(post_speech_silence)) {
                const double xs = ls.sound_start() - now - EWK_LSN_TIMING(padding);
                const double xe = sound_end - now + EWK_LSN_TIMING(padding);
                int64_t nreq = (int64_t)(fabs(xs) * (double)g.sample_rate);
                if (nreq > R) nreq = R;
                const int64_t e = (int64_t)(fabs(xe) * (double)g.sample_rate);
                int64_t stop = nreq - e;   // python a[:len-e]
                if (stop < 0) { stop += nreq; if (stop < 0) stop = 0; }
                if (stop > nreq) stop = nreq;
                int64_t start = (int64_t)spos - nreq;
                if (start < 0) start += Rs;
                ewk_event ev;
                ev.stream = s;
                ev.length = (int32_t)stop;
                ev.tick = tick;
                ev.ring_start = start;
                ev.time = now;
                ev.score = __builtin_nan("");
                ev.match = 0;
                ev.flags = (((double)stop / (double)g.sample_rate > EWK_LSN_TIMING(max_segment_seconds)) ? EWK_EV_SKIPPED : 0) |
                           (j << EWK_EV_LISTENER_SHIFT);
                // one slot per cutting lane (several listeners may cut at one tick; the poll sorts)
                const uint32_t slot = (uint32_t)atomicAdd(g.ev_count, 1) - (uint32_t)g.ev_base0;
                if (slot < (uint32_t)g.ev_cap) g.events[slot] = ev;
                else atomicAdd(g.ev_dropped, 1);
                ls.set_state(kWaiting);
            }
        } else ls.set_state(kWaiting);
        break;
    }
#undef EWK_LSN_TIMING
}

}  // namespace ewk
