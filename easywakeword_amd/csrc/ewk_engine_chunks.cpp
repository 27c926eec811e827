// ewk_engine_chunks.cpp -- the C ABI's packet ingest (ewk_push_chunks*, ewk_chunk_plan,
// ewk_stream_pending): any number of samples per stream and call, re-blocked into ticks on the
// device; those then go the way of a tick push (ewk_engine_stream.cpp).
#include "ewk_engine.h"

using namespace ewk;

static int fail_chunk_plan(ChunkPlanError err, int32_t bad, int32_t in_block, const int32_t* pending,
                           const int32_t* counts) {
    switch (err) {
        case kChunkPlanPending:
            return fail(EWK_EINVAL, "pending[" + std::to_string(bad) + "] = " + std::to_string(pending[bad]) +
                                        " is outside [0, " + std::to_string(in_block) + ")");
        case kChunkPlanCount:
            return fail(EWK_EINVAL, "counts[" + std::to_string(bad) + "] = " + std::to_string(counts[bad]) +
                                        " is outside [0, " + std::to_string((int64_t)EWK_CHUNK_MAX_TICKS * in_block) +
                                        "] (EWK_CHUNK_MAX_TICKS input blocks of " + std::to_string(in_block) + " samples)");
        case kChunkPlanGroups:
            return fail(EWK_EINVAL, "the plan has " + std::to_string(bad) + " groups, group_cap holds fewer");
        default:
            return fail(EWK_EINVAL, "in_block must be positive, n and group_cap >= 0 and no array NULL");
    }
}

int ewk_chunk_plan(int32_t in_block, int32_t n, const int32_t* pending, const int32_t* counts, int32_t* ticks,
                   int32_t* new_pending, int32_t* order, int32_t* n_ticking, int32_t* group_ticks, int32_t* group_first,
                   int32_t group_cap, int32_t* n_groups) {
    int32_t bad = -1;
    const ChunkPlanError err = chunk_plan(in_block, n, pending, counts, ticks, new_pending, order, n_ticking,
                                          group_ticks, group_first, group_cap, n_groups, &bad);
    return err == kChunkPlanOk ? EWK_OK : fail_chunk_plan(err, bad, in_block, pending, counts);
}

int ewk_stream_pending(ewk_engine* e, const int32_t* streams, int32_t n, int32_t* out) {
    if (!e || !out) return fail(EWK_EINVAL, "NULL argument");
    int rc = check_query_list(e, streams, n);
    if (rc) return rc;
    for (int32_t i = 0; i < n; ++i) out[i] = e->chunk_pending.empty() ? 0 : e->chunk_pending[streams ? streams[i] : i];
    return EWK_OK;
}

// ---- a chunk push, stage by stage ---------------------------------------------------
// Validates the call and plans it into e->chunk_plan, on the host: everything is validated before
// anything is enqueued or changed.
static int plan_chunks(ewk_engine* e, const int32_t* streams, int32_t n, const void* pcm, int64_t n_pcm,
                       const int64_t* offsets, const int32_t* counts, SampleKind kind, const uint8_t* laws) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (e->n_streams <= 0) return fail(EWK_EINVAL, "engine has no streams");
    int rc = check_stream_list(e, streams, n);
    if (rc) return rc;
    if (!offsets || !counts) return fail(EWK_EINVAL, "offsets or counts is NULL");
    if (n_pcm < 0) return fail(EWK_EINVAL, "n_pcm must be >= 0");
    if (!pcm && n_pcm > 0) return fail(EWK_EINVAL, "pcm is NULL");
    if (kind.type != kSamplePcm16 && e->ring_es == sizeof(int16_t))
        return fail(EWK_EINVAL, "an int16 ring (EWK_RING_I16) takes PCM16 chunks (ewk_push_chunks_pcm16)");
    if (kind.type == kSampleG711) {
        rc = check_g711(e, kind.law, laws, n);
        if (rc) return rc;
    }
    ChunkPlan& p = e->chunk_plan;
    p.in_block = e->rs_on ? e->rs_in_block : e->cfg.block;
    if (p.in_block > 0x7fffffff / (EWK_CHUNK_MAX_TICKS + 1))
        return fail(EWK_EINVAL, "the input block is too large for chunk pushes");
    for (auto* v : {&p.pending, &p.ticks, &p.new_pending, &p.order}) v->resize((size_t)n);
    p.src_at.resize((size_t)n);
    for (int32_t i = 0; i < n; ++i) p.pending[i] = e->chunk_pending.empty() ? 0 : e->chunk_pending[streams[i]];
    int32_t bad = -1;
    const ChunkPlanError err = chunk_plan(p.in_block, n, p.pending.data(), counts, p.ticks.data(), p.new_pending.data(),
                                          p.order.data(), &p.n_ticking, p.group_ticks, p.group_first,
                                          EWK_CHUNK_MAX_TICKS, &p.n_groups, &bad);
    if (err != kChunkPlanOk) return fail_chunk_plan(err, bad, p.in_block, p.pending.data(), counts);
    for (int32_t i = 0; i < n; ++i)
        if (offsets[i] < 0 || offsets[i] > n_pcm - counts[i])
            return fail(EWK_EINVAL, "chunk " + std::to_string(i) + " (offsets[" + std::to_string(i) + "] = " +
                                        std::to_string(offsets[i]) + ", counts[" + std::to_string(i) + "] = " +
                                        std::to_string(counts[i]) + ") is outside pcm[0, " + std::to_string(n_pcm) + ")");
    return EWK_OK;
}

// Where everything goes: the tick rows in chunk_asm, and every chunk's first sample -- in the
// caller's device buffer, or in the staging its host chunks are packed into.
static void layout_chunks(ewk_engine* e, int32_t n, const int64_t* offsets, const int32_t* counts, bool device,
                          SampleKind kind) {
    ChunkPlan& p = e->chunk_plan;
    // (a G.711 unit is 16 codes into 64 bytes of float32: its rows start on 64 bytes, so that the
    // staged chunks' phases, taken modulo kChunkAlign codes, agree with their destinations')
    const int64_t row_align = kind.type == kSampleG711 ? 2 * kChunkAlign : kChunkAlign;
    p.asm_total = chunk_row_layout(row_align / (int64_t)e->ring_es, p.in_block, p.n_groups, p.group_ticks,
                                   p.group_first, p.group_base);
    p.stage_total = 0;
    if (device) std::copy(offsets, offsets + n, p.src_at.begin());
    else
        p.stage_total = chunk_stage_layout(kChunkAlign / (int64_t)kind.es(), n,
                                           p.pending.data(), counts, p.src_at.data());
}

// What the first chunk push allocates: the pending mirror, the descriptors' device side and the
// carry rows -- those again when a larger input block has been set (nothing is pending then: a
// new rate drops it); and the tick rows, grown to this push's.
static int ensure_chunk_state(ewk_engine* e, hipStream_t s) {
    const ChunkPlan& p = e->chunk_plan;
    const size_t n = (size_t)e->n_streams;
    HIP_TRY(e->d_chunk.reserve(n * (sizeof(ChunkDesc) + sizeof(int32_t))));
    int rc = grow_behind(e->chunk_carry, n * (size_t)p.in_block * e->ring_es, s);
    if (rc == EWK_OK) rc = grow_behind(e->chunk_asm, (size_t)p.asm_total * e->ring_es, s);
    if (rc == EWK_OK && e->chunk_pending.empty()) e->chunk_pending.assign(n, 0);
    return rc;
}

// Host chunks, packed into the pinned staging as laid out (the gaps zeroed: they are copied too)
// and sent with one copy.
static int stage_host_chunks(ewk_engine* e, const void* pcm, SampleKind kind, const int64_t* offsets, const int32_t* counts,
                             int32_t n, hipStream_t s) {
    const ChunkPlan& p = e->chunk_plan;
    if (p.stage_total == 0) return EWK_OK;
    const size_t es = kind.es();
    HIP_TRY(e->pcm_stage.reserve((size_t)p.stage_total * es));   // (and the previous DMA is done)
    unsigned char* h = e->pcm_stage.p;
    int64_t end = 0;
    for (int32_t i = 0; i < n; ++i) {
        if (counts[i] == 0) continue;
        memset(h + end * es, 0, (size_t)(p.src_at[i] - end) * es);
        memcpy(h + p.src_at[i] * es, static_cast<const unsigned char*>(pcm) + offsets[i] * es, (size_t)counts[i] * es);
        end = p.src_at[i] + counts[i];
    }
    return send_staged(e, (size_t)p.stage_total * es, s);
}

// Descriptors: the ticking chunks in plan order (the gate's index lists follow it, *d_list), then
// the appending ones; a chunk without samples needs none.  *n_desc == 0: nothing was sent.  A G.711
// chunk's descriptor carries its law: laws[i], or the call's.
static int send_descriptors(ewk_engine* e, const int32_t* streams, const int32_t* counts, int32_t n, SampleKind kind,
                            const uint8_t* laws, hipStream_t s, int32_t* n_desc, const int32_t** d_list) {
    auto law_of = [&](int32_t i) -> int32_t { return kind.type != kSampleG711 ? 0 : laws ? laws[i] : kind.law; };
    const ChunkPlan& p = e->chunk_plan;
    const size_t list_at = (size_t)e->n_streams * sizeof(ChunkDesc);
    HIP_TRY(e->chunk_stage.reserve(list_at + (size_t)e->n_streams * sizeof(int32_t)));   // (and the previous push's have left it)
    ChunkDesc* h_desc = e->chunk_stage.as<ChunkDesc>();
    int32_t* h_list = reinterpret_cast<int32_t*>(e->chunk_stage.p + list_at);
    int32_t nd = 0;
    for (int32_t g = 0; g < p.n_groups; ++g)
        for (int32_t k = p.group_first[g]; k < p.group_first[g + 1]; ++k) {
            const int32_t i = p.order[k];
            const int64_t row = p.group_base[g] + (int64_t)(k - p.group_first[g]) * p.group_ticks[g] * p.in_block;
            h_desc[nd++] = ChunkDesc{p.src_at[i], row, streams[i], counts[i], p.pending[i], law_of(i)};
            h_list[k] = streams[i];
        }
    for (int32_t i = 0; i < n; ++i)
        if (p.ticks[i] == 0 && counts[i] > 0)
            h_desc[nd++] = ChunkDesc{p.src_at[i], 0, streams[i], counts[i], p.pending[i], law_of(i)};
    *n_desc = nd;
    if (nd == 0) return EWK_OK;
    int32_t* list = reinterpret_cast<int32_t*>(e->d_chunk.p + list_at);
    HIP_TRY(hipMemcpyAsync(e->d_chunk.p, h_desc, (size_t)nd * sizeof(ChunkDesc), hipMemcpyHostToDevice, s));
    if (p.n_ticking)
        HIP_TRY(hipMemcpyAsync(list, h_list, (size_t)p.n_ticking * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(e->chunk_stage.sent(s));
    *d_list = list;
    return EWK_OK;
}

// The one assembly launch: carry rows and chunks into tick rows, the rest back into the carry rows.
static int assemble_chunks(ewk_engine* e, const void* d_src, int32_t n_desc, SampleKind kind, hipStream_t s) {
    const ChunkPlan& p = e->chunk_plan;
    ChunkArgs a;
    memset(&a, 0, sizeof(a));
    a.src = d_src;
    a.out = e->chunk_asm.p;
    a.carry = e->chunk_carry.p;
    a.desc = reinterpret_cast<const ChunkDesc*>(e->d_chunk.p);
    a.n = n_desc;
    a.in_block = p.in_block;
    a.max_ticks = p.n_groups ? p.group_ticks[p.n_groups - 1] : 1;
    a.src16 = kind.type == kSamplePcm16;
    a.src8 = kind.type == kSampleG711;
    a.out16 = e->ring_es == sizeof(int16_t);
    ProfScope ps(e, 4, s);
    HIP_TRY(launch_chunk_assemble(a, s));
    return EWK_OK;
}

static void update_pending(ewk_engine* e, const int32_t* streams, int32_t n) {
    for (int32_t i = 0; i < n; ++i) {
        int32_t& p = e->chunk_pending[streams[i]];
        e->chunk_pending_n += (e->chunk_plan.new_pending[i] > 0) - (p > 0);
        p = e->chunk_plan.new_pending[i];
    }
}

// Every group's ticks through the resampler and the gate, as a tick push of its streams.
static int gate_groups(ewk_engine* e, const int32_t* streams, const int32_t* d_list, hipStream_t s) {
    ChunkPlan& p = e->chunk_plan;
    // the plan's ticking streams on the host, for the tick mirror (the pinned list is the next push's to overwrite)
    for (int32_t k = 0; k < p.n_ticking; ++k) p.order[k] = streams[p.order[k]];
    for (int32_t g = 0; g < p.n_groups; ++g) {
        const int32_t first = p.group_first[g], rows = p.group_first[g + 1] - first, nt = p.group_ticks[g];
        TickSrc src{e->chunk_asm.p + p.group_base[g] * e->ring_es, e->ring_es == sizeof(int16_t) ? kKindPcm16 : kKindF32,
                    (int64_t)nt * p.in_block, p.in_block};
        int rc = e->rs_on ? resample_ticks(e, &src, rows, nt, d_list + first, s) : EWK_OK;
        if (rc == EWK_OK) rc = gate_ticks(e, src, rows, nt, d_list + first, p.order.data() + first, s);
        if (rc) return rc;
    }
    return finish_push(e, s);
}

static int push_chunks_impl(ewk_engine* e, const int32_t* streams, int32_t n, const void* pcm, int64_t n_pcm,
                            const int64_t* offsets, const int32_t* counts, int32_t flags, SampleKind kind,
                            const uint8_t* laws = nullptr) {
    const bool device = (flags & EWK_PUSH_DEVICE) != 0;
    int rc = plan_chunks(e, streams, n, pcm, n_pcm, offsets, counts, kind, laws);
    if (rc) return rc;
    layout_chunks(e, n, offsets, counts, device, kind);
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    rc = desynchronise(e, s);
    if (rc == EWK_OK) rc = ensure_chunk_state(e, s);
    if (rc == EWK_OK && !device) rc = stage_host_chunks(e, pcm, kind, offsets, counts, n, s);
    int32_t n_desc = 0;
    const int32_t* d_list = nullptr;
    if (rc == EWK_OK) rc = send_descriptors(e, streams, counts, n, kind, laws, s, &n_desc, &d_list);
    if (rc || n_desc == 0) return rc;   // (no samples at all)
    rc = assemble_chunks(e, device ? pcm : e->push_stage.p, n_desc, kind, s);
    if (rc) return rc;
    update_pending(e, streams, n);
    if (e->chunk_plan.n_groups == 0) return EWK_OK;   // nobody ticks: the assembly alone (a poll finds the banks as they were)
    return gate_groups(e, streams, d_list, s);
}

int ewk_push_chunks(ewk_engine* e, const int32_t* streams, int32_t n, const float* pcm, int64_t n_pcm,
                    const int64_t* offsets, const int32_t* counts, int32_t flags) {
    return push_chunks_impl(e, streams, n, pcm, n_pcm, offsets, counts, flags, kKindF32);
}

int ewk_push_chunks_pcm16(ewk_engine* e, const int32_t* streams, int32_t n, const int16_t* pcm, int64_t n_pcm,
                          const int64_t* offsets, const int32_t* counts, int32_t flags) {
    return push_chunks_impl(e, streams, n, pcm, n_pcm, offsets, counts, flags, kKindPcm16);
}

int ewk_push_chunks_g711(ewk_engine* e, const int32_t* streams, int32_t n, const uint8_t* pcm, int64_t n_pcm,
                         const int64_t* offsets, const int32_t* counts, int32_t law, const uint8_t* laws,
                         int32_t flags) {
    return push_chunks_impl(e, streams, n, pcm, n_pcm, offsets, counts, flags, SampleKind{kSampleG711, law}, laws);
}
