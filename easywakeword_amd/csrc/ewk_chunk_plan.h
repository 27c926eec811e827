// ewk_chunk_plan.h -- the planning and layout steps of a chunk push (ewk_push_chunks, ewk_chunk_plan).
// Pure host code without HIP: a host compiler builds it alone (tests/test_chunk_plan.py runs it
// under the address and undefined-behaviour sanitizers).
//
// Chunk i delivers counts[i] samples to a stream that holds pending[i] in [0, in_block) samples
// in its carry row.  The push makes ticks[i] = (pending[i] + counts[i]) / in_block gate ticks and
// leaves new_pending[i] = (pending[i] + counts[i]) % in_block samples behind.  The chunks that
// tick are ordered by (ticks, position in the call): the runs of equal ticks are the groups, each
// one gate launch sequence of its own (a gate launch gives every listed stream the same ticks).
#pragma once

#include <stdint.h>

#ifndef EWK_CHUNK_MAX_TICKS
#define EWK_CHUNK_MAX_TICKS 64
#endif

namespace ewk {

enum ChunkPlanError {
    kChunkPlanOk = 0,
    kChunkPlanArgs = 1,      // in_block < 1, n < 0 or a NULL array
    kChunkPlanPending = 2,   // *bad: the entry whose pending is outside [0, in_block)
    kChunkPlanCount = 3,     // *bad: the entry whose count is outside [0, EWK_CHUNK_MAX_TICKS * in_block]
    kChunkPlanGroups = 4,    // more groups than group_cap (*bad: the number of groups)
};

// order [n] (n_ticking entries written), group_ticks [group_cap], group_first [group_cap + 1]
// (n_groups + 1 entries written: group g is order[group_first[g] .. group_first[g + 1])).
// Everything is validated first: a failure writes nothing but *bad.
inline ChunkPlanError chunk_plan(int32_t in_block, int32_t n, const int32_t* pending, const int32_t* counts,
                                 int32_t* ticks, int32_t* new_pending, int32_t* order, int32_t* n_ticking,
                                 int32_t* group_ticks, int32_t* group_first, int32_t group_cap, int32_t* n_groups,
                                 int32_t* bad) {
    if (bad) *bad = -1;
    if (in_block < 1 || n < 0 || group_cap < 0 || !n_ticking || !n_groups || !group_first) return kChunkPlanArgs;
    if (n > 0 && (!pending || !counts || !ticks || !new_pending || !order)) return kChunkPlanArgs;
    if (group_cap > 0 && !group_ticks) return kChunkPlanArgs;
    const int64_t max_count = (int64_t)EWK_CHUNK_MAX_TICKS * in_block;
    int32_t hist[EWK_CHUNK_MAX_TICKS + 1] = {0};   // chunks per tick count (pending < in_block: ticks <= the maximum)
    for (int32_t i = 0; i < n; ++i) {
        if (pending[i] < 0 || pending[i] >= in_block) {
            if (bad) *bad = i;
            return kChunkPlanPending;
        }
        if (counts[i] < 0 || counts[i] > max_count) {
            if (bad) *bad = i;
            return kChunkPlanCount;
        }
        hist[((int64_t)pending[i] + counts[i]) / in_block] += 1;
    }
    int32_t groups = 0;
    for (int32_t t = 1; t <= EWK_CHUNK_MAX_TICKS; ++t) groups += hist[t] > 0;
    if (groups > group_cap) {
        if (bad) *bad = groups;
        return kChunkPlanGroups;
    }
    // a counting sort on ticks, stable in the position
    int32_t first[EWK_CHUNK_MAX_TICKS + 1];
    int32_t g = 0, at = 0;
    for (int32_t t = 1; t <= EWK_CHUNK_MAX_TICKS; ++t) {
        first[t] = at;
        if (hist[t] == 0) continue;
        group_ticks[g] = t;
        group_first[g] = at;
        at += hist[t];
        g += 1;
    }
    group_first[g] = at;
    *n_groups = g;
    *n_ticking = at;
    for (int32_t i = 0; i < n; ++i) {
        const int64_t total = (int64_t)pending[i] + counts[i];
        const int32_t t = (int32_t)(total / in_block);
        ticks[i] = t;
        new_pending[i] = (int32_t)(total - (int64_t)t * in_block);
        if (t > 0) order[first[t]++] = i;
    }
    return kChunkPlanOk;
}

// The layout of a planned push, in samples.  A group's first tick row and a staged chunk's phase
// are aligned to kChunkAlign bytes (copy_span's widest unit): `unit` is that many samples.
constexpr int64_t kChunkAlign = 32;

// Host chunks packed into one staging buffer: src_at[i], where chunk i starts -- each non-empty
// chunk at the next unit-aligned position plus pending[i] % unit, the phase of the samples it
// follows in its stream's block, so the assembly kernel's loads and stores agree in phase (an
// empty chunk: 0).  Returns the samples the buffer holds, the gaps included.
inline int64_t chunk_stage_layout(int64_t unit, int32_t n, const int32_t* pending, const int32_t* counts,
                                  int64_t* src_at) {
    int64_t total = 0;
    for (int32_t i = 0; i < n; ++i) {
        src_at[i] = counts[i] == 0 ? 0 : (total + unit - 1) / unit * unit + pending[i] % unit;
        if (counts[i] > 0) total = src_at[i] + counts[i];
    }
    return total;
}

// The tick rows: group g contiguous from group_base[g], a multiple of row_unit, one row of
// group_ticks[g] * in_block samples per member.  Returns the end of the last group.
inline int64_t chunk_row_layout(int64_t row_unit, int32_t in_block, int32_t n_groups, const int32_t* group_ticks,
                                const int32_t* group_first, int64_t* group_base) {
    int64_t total = 0;
    for (int32_t g = 0; g < n_groups; ++g) {
        group_base[g] = (total + row_unit - 1) / row_unit * row_unit;
        total = group_base[g] + (int64_t)(group_first[g + 1] - group_first[g]) * group_ticks[g] * in_block;
    }
    return total;
}

}  // namespace ewk
