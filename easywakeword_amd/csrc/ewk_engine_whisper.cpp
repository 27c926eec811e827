// ewk_engine_whisper.cpp -- the level-3 front end behind ewk_whisper_features_events /
// ewk_whisper_features_segments: k_normalize (ewk_level3.hip) into engine scratch, then the two
// kernels of ewk_whisper.hip, all on the engine's stream.
#include "ewk_engine.h"

using namespace ewk;

// The segments' plan (host): where each one's normalised samples, live frames and frame maxima
// sit in the scratch.  Lengths come from the events or from `lengths`.
struct WfPlan {
    std::vector<WfSeg> seg;
    std::vector<int64_t> y_off;
    int64_t y_total = 0, live_total = 0;
    int32_t max_live = 0;
};

static int plan_segments(const ewk_event* events, const int32_t* lengths, int32_t n, int32_t n_frames, WfPlan* p) {
    p->seg.resize(n);
    p->y_off.resize(n);
    const int64_t window = (int64_t)n_frames * kWfHop;
    for (int32_t i = 0; i < n; ++i) {
        const int32_t len = events ? events[i].length : lengths[i];
        if (len < 0) return fail(EWK_EINVAL, "negative segment length");
        WfSeg& s = p->seg[i];
        s.y_off = p->y_off[i] = p->y_total;
        s.raw_off = p->live_total;
        s.len = (int32_t)std::min<int64_t>(len, window);
        s.n_live = s.len > 0 ? (int32_t)std::min<int64_t>(n_frames, (s.len + 199) / kWfHop + 1) : 0;
        p->y_total += len;
        p->live_total += s.n_live;
        p->max_live = std::max(p->max_live, s.n_live);
    }
    return EWK_OK;
}

static int ensure_whisper_tables(ewk_engine* e, hipStream_t s) {
    if (e->wf_tab.p) return EWK_OK;
    std::vector<unsigned char> buf(sizeof(WhisperTables));
    WhisperTables* t = reinterpret_cast<WhisperTables*>(buf.data());
    build_whisper_tables(t);
    if (!t->ok) return fail(EWK_EHIP, "Whisper mel filterbank does not fit the kernel's packed layout");
    HIP_TRY(e->wf_tab.reserve(1));
    HIP_TRY(hipMemcpyAsync(e->wf_tab.p, t, sizeof(WhisperTables), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));   // `buf` is pageable and leaves scope
    return EWK_OK;
}

// d_pcm / offsets / lengths (linear, offsets and lengths host arrays) or events (ring mode).
static int whisper_impl(ewk_engine* e, const float* d_pcm, const int64_t* offsets, const int32_t* lengths,
                        const ewk_event* events, int32_t n, void* out, int32_t n_frames, int32_t flags) {
    hipStream_t s = e->stream;
    WfPlan p;
    int rc = plan_segments(events, lengths, n, n_frames, &p);
    if (rc) return rc;
    const size_t es = (flags & EWK_FEAT_BF16) ? sizeof(uint16_t) : sizeof(float);
    const size_t out_bytes = (size_t)n * kWfMels * (size_t)n_frames * es;
    HIP_TRY(join_scoring(e, s));
    rc = ensure_whisper_tables(e, s);
    if (rc == EWK_OK) rc = grow_behind(e->wf_y, (size_t)std::max<int64_t>(1, p.y_total), s);
    if (rc == EWK_OK) rc = grow_behind(e->wf_raw, (size_t)std::max<int64_t>(1, p.live_total) * kWfMels, s);
    if (rc == EWK_OK) rc = grow_behind(e->wf_fmax, (size_t)std::max<int64_t>(1, p.live_total), s);
    if (rc == EWK_OK) rc = grow_behind(e->wf_seg, (size_t)n, s);
    if (rc == EWK_OK) rc = grow_behind(e->wf_i64, 2 * (size_t)n, s);
    if (rc == EWK_OK && events) rc = grow_behind(e->wf_ev, (size_t)n, s);
    if (rc == EWK_OK && !events) rc = grow_behind(e->wf_len, (size_t)n, s);
    if (rc == EWK_OK && !(flags & EWK_OUT_DEVICE)) rc = grow_behind(e->wf_out, out_bytes, s);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(e->wf_seg.p, p.seg.data(), n * sizeof(WfSeg), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(e->wf_i64.p, p.y_off.data(), n * sizeof(int64_t), hipMemcpyHostToDevice, s));
    L3Args l3;
    memset(&l3, 0, sizeof(l3));
    l3.n = n;
    l3.out_offsets = e->wf_i64.p;
    l3.out = e->wf_y.p;
    if (events) {
        HIP_TRY(hipMemcpyAsync(e->wf_ev.p, events, n * sizeof(ewk_event), hipMemcpyHostToDevice, s));
        l3.events = e->wf_ev.p;
        l3.pcm = e->ring_f32();
        l3.pcm16 = e->ring_i16();
        l3.ring_len = e->sring_len;
    } else {
        HIP_TRY(hipMemcpyAsync(e->wf_i64.p + n, offsets, n * sizeof(int64_t), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(e->wf_len.p, lengths, n * sizeof(int32_t), hipMemcpyHostToDevice, s));
        l3.pcm = d_pcm;
        l3.offsets = e->wf_i64.p + n;
        l3.lengths = e->wf_len.p;
    }
    HIP_TRY(launch_normalize(l3, s));
    WfArgs a;
    memset(&a, 0, sizeof(a));
    a.y = e->wf_y.p;
    a.seg = e->wf_seg.p;
    a.tab = e->wf_tab.p;
    a.raw = e->wf_raw.p;
    a.fmax = e->wf_fmax.p;
    a.out = (flags & EWK_OUT_DEVICE) ? out : static_cast<void*>(e->wf_out.p);
    a.n_seg = n;
    a.n_frames = n_frames;
    a.bf16 = (flags & EWK_FEAT_BF16) ? 1 : 0;
    a.max_live = p.max_live;
    HIP_TRY(launch_whisper_features(a, s));
    if (!(flags & EWK_OUT_DEVICE)) HIP_TRY(hipMemcpyAsync(out, e->wf_out.p, out_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));   // the plan's host arrays leave scope; the output is complete
    return EWK_OK;
}

static int check_whisper_call(ewk_engine* e, int32_t n, const void* out, int32_t n_frames, int32_t flags,
                              int32_t known_flags) {
    if (!e) return fail(EWK_EINVAL, "engine is NULL");
    if (n < 0) return fail(EWK_EINVAL, "negative size");
    if (n_frames < 1 || n_frames > kWfMaxFrames)
        return fail(EWK_EINVAL, "n_frames = " + std::to_string(n_frames) + " is outside 1.." + std::to_string(kWfMaxFrames));
    if (flags & ~known_flags) return fail(EWK_EINVAL, "unknown flags");
    if (n > 0 && !out) return fail(EWK_EINVAL, "NULL argument");
    return EWK_OK;
}

int ewk_whisper_features_events(ewk_engine* e, const ewk_event* events, int32_t n, void* out, int32_t n_frames,
                                int32_t flags) {
    int rc = check_whisper_call(e, n, out, n_frames, flags, EWK_OUT_DEVICE | EWK_FEAT_BF16);
    if (rc) return rc;
    if (n == 0) return EWK_OK;
    if (!events) return fail(EWK_EINVAL, "NULL argument");
    rc = check_ring_events(e, events, n);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(e->device));
    return whisper_impl(e, nullptr, nullptr, nullptr, events, n, out, n_frames, flags);
}

int ewk_whisper_features_segments(ewk_engine* e, const float* pcm, int64_t n_pcm, const int64_t* offsets,
                                  const int32_t* lengths, int32_t n_seg, void* out, int32_t n_frames, int32_t flags) {
    int rc = check_whisper_call(e, n_seg, out, n_frames, flags, EWK_PCM_DEVICE | EWK_OUT_DEVICE | EWK_FEAT_BF16);
    if (rc) return rc;
    if (n_pcm < 0) return fail(EWK_EINVAL, "negative size");
    if (n_seg == 0) return EWK_OK;
    if (!offsets || !lengths || (n_pcm > 0 && !pcm)) return fail(EWK_EINVAL, "NULL argument");
    for (int32_t i = 0; i < n_seg; ++i)
        if (offsets[i] < 0 || lengths[i] < 0 || offsets[i] + lengths[i] > n_pcm)
            return fail(EWK_EINVAL, "segment " + std::to_string(i) + " outside pcm");
    HIP_TRY(hipSetDevice(e->device));
    const float* d_pcm = pcm;
    if (!(flags & EWK_PCM_DEVICE)) {
        rc = grow_behind(e->wf_pcm, (size_t)std::max<int64_t>(1, n_pcm), e->stream);
        if (rc) return rc;
        if (n_pcm > 0)
            HIP_TRY(hipMemcpyAsync(e->wf_pcm.p, pcm, n_pcm * sizeof(float), hipMemcpyHostToDevice, e->stream));
        d_pcm = e->wf_pcm.p;
    }
    return whisper_impl(e, d_pcm, offsets, lengths, nullptr, n_seg, out, n_frames, flags);
}
