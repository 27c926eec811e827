// ewk_snapshot_plan.h -- the record layout of a stream snapshot (ewk_snapshot_plan,
// ewk_export_streams, ewk_import_streams).  Pure host code without HIP: a host compiler builds it
// alone (tests/test_snapshot_layout.py runs it under the address and undefined-behaviour
// sanitizers).
//
// A record is one stream's device state in fixed sections (EWK_SNAP_*), each starting at a
// multiple of 16 bytes, the record a multiple of 128.  The layout is a function of the geometry
// alone: the configuration's sample rate, block, rings, ring format and tick, and the input rate
// with the input block and history length it implies.  Gate durations and thresholds are not
// geometry.  The fingerprint is FNV-1a over the geometry fields in a fixed order.
#pragma once

#include <stdint.h>
#include <string.h>

#include "../../include/ewk.h"

namespace ewk {

enum SnapshotPlanError {
    kSnapPlanOk = 0,
    kSnapPlanArgs,          // cfg or out NULL
    kSnapPlanSampleRate,    // the tests of ewk_create, in its order
    kSnapPlanBufferSeconds,
    kSnapPlanBlock,
    kSnapPlanTick,
    kSnapPlanPreSilence,
    kSnapPlanSpeechMin,
    kSnapPlanSpeechMax,
    kSnapPlanSpeechOrder,
    kSnapPlanPostSilence,
    kSnapPlanRingFormat,
    kSnapPlanBufferLarge,
    kSnapPlanRingRange,
    kSnapPlanRingDivide,
    kSnapPlanRingBlock,
    kSnapPlanRingNeed,
    kSnapPlanRate,          // the tests of ewk_set_input_rate
    kSnapPlanRateI16,
    kSnapPlanRateBlock,
};

inline const char* snapshot_plan_message(SnapshotPlanError err) {
    switch (err) {
        case kSnapPlanOk: return "";
        case kSnapPlanArgs: return "NULL argument";
        case kSnapPlanSampleRate: return "sample_rate must be 16000 (SoundBuffer.FREQUENCY)";
        case kSnapPlanBufferSeconds: return "buffer_seconds must be positive";
        case kSnapPlanBlock: return "block must be in [1, 8192]";
        case kSnapPlanTick: return "tick_seconds must be positive";
        case kSnapPlanPreSilence: return "pre_speech_silence must be positive";
        case kSnapPlanSpeechMin: return "speech_duration_min must be positive";
        case kSnapPlanSpeechMax: return "speech_duration_max must be positive";
        case kSnapPlanSpeechOrder: return "speech_duration_min must be <= speech_duration_max";
        case kSnapPlanPostSilence: return "post_speech_silence must be positive";
        case kSnapPlanRingFormat: return "ring_format must be EWK_RING_F32 or EWK_RING_I16";
        case kSnapPlanBufferLarge: return "buffer_seconds too large";
        case kSnapPlanRingRange: return "ring_samples must be in [0, buffer_seconds * sample_rate]";
        case kSnapPlanRingDivide: return "a compact ring (ring_samples) needs block to divide both rings";
        case kSnapPlanRingBlock: return "a compact ring (ring_samples) needs block <= 4096";
        case kSnapPlanRingNeed: return "ring_samples must hold the longest segment request plus one tick";
        case kSnapPlanRate: return "in_rate must be >= 0";
        case kSnapPlanRateI16:
            return "an int16 ring (EWK_RING_I16) stores PCM16 as delivered: resampled samples are not int16";
        case kSnapPlanRateBlock: return "a tick is not a whole number of samples at the input rate";
    }
    return "";
}

inline uint64_t snapshot_fnv(uint64_t h, const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001b3ULL;
    return h;
}

// The layout of given geometry (every geometry field of *out set by the caller; hist_len 0 when
// the input rate is the engine's own): sections, record_bytes, fingerprint, magic and version.
inline void snapshot_sections(ewk_snapshot_layout* out) {
    const int64_t es = out->ring_format == EWK_RING_I16 ? 2 : 4;
    int64_t bytes[EWK_SNAP_SECTIONS];
    bytes[EWK_SNAP_GATE] = 96;                                        // sizeof(GateStream)
    bytes[EWK_SNAP_LISTENERS] = (int64_t)(EWK_LISTENERS_MAX - 1) * 40;  // kLsnStates LsnState rows
    bytes[EWK_SNAP_BLOCK_RMS] = (int64_t)out->n_blocks * 8;
    bytes[EWK_SNAP_SORTED] = (int64_t)out->n_blocks * 8;
    bytes[EWK_SNAP_RING] = out->sring_len * es;
    bytes[EWK_SNAP_HISTORY] = (int64_t)out->hist_len * 4;
    bytes[EWK_SNAP_FRESH] = out->hist_len > 0 ? 16 : 0;               // int32 flag, padded
    bytes[EWK_SNAP_CARRY] = (int64_t)out->in_block * es;
    int64_t at = 0;
    for (int k = 0; k < EWK_SNAP_SECTIONS; ++k) {
        out->section[k].offset = at;
        out->section[k].bytes = bytes[k];
        at += (bytes[k] + 15) & ~(int64_t)15;
    }
    out->record_bytes = (at + 127) & ~(int64_t)127;
    out->magic = EWK_SNAPSHOT_MAGIC;
    out->version = EWK_SNAPSHOT_VERSION;
    uint64_t h = 0xcbf29ce484222325ULL;
    const int64_t geo[11] = {out->sample_rate, out->block,    out->buffer_seconds, out->ring_len,
                             out->sring_len,   out->ring_format, out->n_blocks,    out->in_rate,
                             out->in_block,    out->hist_len, 0};
    h = snapshot_fnv(h, geo, sizeof(geo));
    h = snapshot_fnv(h, &out->tick_seconds, sizeof(double));
    out->fingerprint = h;
}

// in_rate 0 or cfg->sample_rate: no resampler.  A failure writes nothing.
inline SnapshotPlanError snapshot_plan(const ewk_config* cfg, int32_t in_rate, ewk_snapshot_layout* out) {
    if (!cfg || !out) return kSnapPlanArgs;
    const ewk_config& c = *cfg;
    if (c.sample_rate != 16000) return kSnapPlanSampleRate;
    if (c.buffer_seconds <= 0) return kSnapPlanBufferSeconds;
    if (c.block <= 0 || c.block > 8192) return kSnapPlanBlock;
    if (!(c.tick_seconds > 0)) return kSnapPlanTick;
    if (!(c.pre_speech_silence > 0)) return kSnapPlanPreSilence;
    if (!(c.speech_duration_min > 0)) return kSnapPlanSpeechMin;
    if (!(c.speech_duration_max > 0)) return kSnapPlanSpeechMax;
    if (!(c.speech_duration_min <= c.speech_duration_max)) return kSnapPlanSpeechOrder;
    if (!(c.post_speech_silence > 0)) return kSnapPlanPostSilence;
    if (c.ring_format != EWK_RING_F32 && c.ring_format != EWK_RING_I16) return kSnapPlanRingFormat;
    const int64_t ring_len = (int64_t)c.buffer_seconds * c.sample_rate;
    if (ring_len > INT32_MAX / 2) return kSnapPlanBufferLarge;
    const int64_t n_last = (int64_t)(0.1 * (double)c.sample_rate);
    if (c.ring_samples != 0) {
        if (c.ring_samples < 0 || c.ring_samples > ring_len) return kSnapPlanRingRange;
        if (c.ring_samples < ring_len) {
            if (ring_len % c.block != 0 || c.ring_samples % c.block != 0) return kSnapPlanRingDivide;
            if ((c.block > n_last ? c.block : n_last) > 4096) return kSnapPlanRingBlock;
            const double need_s =
                (c.speech_duration_max + c.post_speech_silence + c.tick_seconds + c.padding) * (double)c.sample_rate;
            int64_t need = need_s >= (double)ring_len ? ring_len : (int64_t)need_s + 2;
            if (need > ring_len) need = ring_len;
            if (c.ring_samples < need + c.block || c.ring_samples < n_last) return kSnapPlanRingNeed;
        }
    }
    int32_t rate = c.sample_rate, in_block = c.block, hist = 0;
    if (in_rate < 0) return kSnapPlanRate;
    if (in_rate != 0 && in_rate != c.sample_rate) {
        if (c.ring_format == EWK_RING_I16) return kSnapPlanRateI16;
        int64_t a = in_rate, b = c.sample_rate;
        while (b) { const int64_t t = a % b; a = b; b = t; }
        const int64_t up = c.sample_rate / a, down = in_rate / a;
        if (((int64_t)c.block * down) % up) return kSnapPlanRateBlock;
        const int64_t half = 10 * (up > down ? up : down), J = 2 * half / up + 1;
        if ((int64_t)c.block * down / up > INT32_MAX || J + 1 > INT32_MAX) return kSnapPlanRateBlock;
        rate = in_rate;
        in_block = (int32_t)((int64_t)c.block * down / up);
        hist = (int32_t)(J + 1);   // ewk_set_input_rate: the last J + 1 input samples
    }
    ewk_snapshot_layout l;
    memset(&l, 0, sizeof(l));
    l.sample_rate = c.sample_rate;
    l.block = c.block;
    l.buffer_seconds = c.buffer_seconds;
    l.ring_format = c.ring_format;
    l.n_blocks = (int32_t)(ring_len / c.block);
    l.in_rate = rate;
    l.in_block = in_block;
    l.hist_len = hist;
    l.ring_len = ring_len;
    l.sring_len = c.ring_samples > 0 ? (int64_t)c.ring_samples : ring_len;
    l.tick_seconds = c.tick_seconds;
    snapshot_sections(&l);
    *out = l;
    return kSnapPlanOk;
}

}  // namespace ewk
