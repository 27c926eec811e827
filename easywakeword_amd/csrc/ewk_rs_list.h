// ewk_rs_list.h -- listing a segment for the fp64 re-score (ewk_rescore.h drains the list).
// One definition for every lister: the fused scorer's epilogue (ewk_mfcc.hip) and the stream
// bank's event pass (ewk_bank.hip).
#pragma once

#include "ewk_internal.h"

namespace ewk {

// List segment `seg` (lane 0 of its scoring wave, after its float32 score is written).  Plain
// stores: the list is read by the re-score launch that follows the lister (stream order).
// False when the list is full (the float32 score stands).
__device__ __forceinline__ bool rs_list(const ScoreArgs& a, int seg, int len, float theta_s) {
    const int s = atomicAdd(&a.rs_ctl[0], 1);
    if (s >= a.rs_cap) return false;   // list full: the float32 score stands
    const int T = 1 + len / HOP;
    const int nch = (T + kRsFrames - 1) / kRsFrames;
    int serial = a.list_all, base = 0;   // list_all (every segment): one wave each, no part records
    bool failed = false;
    if (!serial) {
        base = atomicAdd(&a.rs_ctl[1], nch);
        failed = base < 0 || base > a.rs_part_cap - nch;   // part pool full (or the cursor wrapped)
        if (failed) serial = 1;                             // this slot runs serially
    }
    RsSlot* p = a.rs_slots + s;
    p->seg = seg;
    p->T = T;
    p->base = base;
    p->nclaim = serial ? 1 : nch;
    p->done = 0;
    p->theta_s = theta_s;
    p->serial = serial;
    if (serial) {
        a.rs_serial[atomicAdd(&a.rs_ctl[2], 1)] = s;
        if (failed && base >= 0)   // the reserved records inside the pool: nobody's chunks
            for (int c = base; c < min(base + nch, a.rs_part_cap); ++c) a.rs_parts[c].slot = -1;
    } else {
        for (int c = 0; c < nch; ++c) a.rs_parts[base + c].slot = s;
    }
    return true;
}

}  // namespace ewk
