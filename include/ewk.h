/*
 * ewk.h -- C ABI of the MI355X-native EasyWakeWord hot path (levels 1 + 2).
 *
 * The reference has no FFI; its seams are Python duck types:
 *   - the WordMatcher protocol  (easywakeword/wakeword.py:520-639)
 *   - the SoundBuffer protocol  (easywakeword/wakeword.py:405-517)
 *   - the WakeWord._detect_word tick loop (easywakeword/wakeword.py:1036-1159)
 * Each entry point below names the reference interface it replaces.  The
 * Python facade (easywakeword_amd/wakeword.py) binds these with ctypes; the
 * binding a maintainer would add to the reference is shown in INTEGRATION.md.
 *
 * Conventions
 *   - every int-returning call returns EWK_OK (0) or a negative EWK_E* code;
 *     the message is in the thread-local ewk_last_error().  The facade maps
 *     EWK_EINVAL / EWK_ENOTEMPLATE to ValueError and the rest to RuntimeError.
 *   - the caller owns host arrays; the engine owns its device buffers and its
 *     HIP stream.  One engine per host thread; calls are not re-entrant per
 *     engine.
 *   - *_device entry points take device pointers (e.g. torch tensors'
 *     data_ptr()) and an optional hipStream_t (NULL = the engine's stream).
 */
#ifndef EWK_H
#define EWK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EWK_N_MFCC 20
#define EWK_ABI_VERSION 4

#define EWK_OK 0
#define EWK_EINVAL (-1)       /* bad parameter            -> ValueError            */
#define EWK_ENOTEMPLATE (-2)  /* no reference word set    -> ValueError (wakeword.py:608-609) */
#define EWK_EHIP (-3)         /* HIP runtime failure      -> RuntimeError          */
#define EWK_ENOMEM (-4)       /* allocation failure       -> MemoryError           */
#define EWK_ENODEV (-5)       /* no gfx950 device / bad device index -> RuntimeError */
#define EWK_EOVERWRITTEN (-6) /* ewk_normalize_events: an event's samples were overwritten in its
                                 ring since its tick -> RingOverwrittenError (a ValueError) */

/* event flags */
#define EWK_EV_SKIPPED 1      /* segment longer than max_segment_seconds: no level-2 call (wakeword.py:1113-1118) */
#define EWK_EV_RESCORED 2     /* score and decision from the fp64 path: the fp32 score fell inside
                                 rescore_margin, or the segment is very short (<= 16 frames), nearly
                                 stationary (|std| < 20) or has a vanishing MFCC mean (|mean| < 32,
                                 unless its similarity is negative beyond the fp32 error: NaN either way) */
#define EWK_EV_BANK 4         /* scored against the stream bank (ewk_stream_bank_enable): score = best
                                 score over the templates of the stream's word ignoring NaN (NaN when
                                 all are), match = best >= the word's threshold */
#define EWK_EV_BEST_SHIFT 8   /* with EWK_EV_BANK and a non-NaN score: bits 8..13 of flags hold the best
                                 template's index inside its word (lowest on ties), as
                                 ewk_bank_result.best_tmpl minus word_first[w] */
#define EWK_EV_BEST(flags) (((flags) >> EWK_EV_BEST_SHIFT) & 63)

/* ewk_score_segments* flags */
#define EWK_SCORE_REQUIRE_TEMPLATE 1   /* EWK_ENOTEMPLATE when no template (calculate_similarity) */
#define EWK_SCORE_F32_CANDIDATES 2     /* score with the reference's float32-candidate arithmetic
                                          (WordMatcher fed float32 audio); default: float64
                                          candidates, as SoundBuffer slices are (wakeword.py:428) */

/* ewk_config.ring_format */
#define EWK_RING_F32 0        /* float32 samples (any push)                                  */
#define EWK_RING_I16 1        /* int16 samples: PCM16 pushes only (ewk_push_pcm16 /
                                 ewk_push_many_pcm16), stored as delivered -- exact, half the
                                 HBM per stream; float32 pushes fail with EWK_EINVAL */

/* ewk_push flags */
#define EWK_PUSH_DEVICE 1     /* pcm is a device pointer */
#define EWK_PCM_DEVICE 1      /* input sample pointers are device memory (same bit as EWK_PUSH_DEVICE) */
#define EWK_OUT_DEVICE 4      /* output pointer is device memory (asynchronous where noted) */

typedef struct ewk_engine ewk_engine;

/* Defaults mirror the reference constants (wakeword.py:31-48, 405-431, 1100-1118). */
typedef struct ewk_config {
    int32_t sample_rate;          /* 16000  SoundBuffer.FREQUENCY                  */
    int32_t buffer_seconds;       /* 10     DEFAULT_BUFFER_SECONDS                 */
    int32_t block;                /* 1600   samples per callback == per tick       */
    int32_t ring_samples;         /* 0 = buffer_seconds * sample_rate (the reference ring).
                                     Otherwise samples kept per stream for segment reads: a
                                     compact ring with the same decisions and scores (block
                                     RMSs are kept per block as they arrive), for configs whose
                                     block divides the reference ring; must hold the longest
                                     possible segment request (max speech + post silence + one
                                     tick + padding) plus one tick, else EWK_EINVAL.  Saves HBM
                                     per stream (10 s -> 3 s: 640 KB -> 192 KB); ewk_read_last
                                     fails (EWK_EINVAL) for more than ring_samples. */
    double tick_seconds;          /* 0.1    time.sleep(0.1) in _detect_word        */
    double pre_speech_silence;    /* 0.8    DEFAULT_PRE_SPEECH_SILENCE             */
    double speech_duration_min;   /* 0.3    DEFAULT_SPEECH_DURATION_MIN            */
    double speech_duration_max;   /* 2.0    DEFAULT_SPEECH_DURATION_MAX            */
    double post_speech_silence;   /* 0.4    DEFAULT_POST_SPEECH_SILENCE            */
    double padding;               /* 0.05   wakeword.py:1101                       */
    double max_segment_seconds;   /* 3.0    wakeword.py:1115                       */
    double similarity_threshold;  /* 75.0   WakeWord(similarity_threshold=)        */
    double reentry_timeout;       /* <= 0: continuous; > 0: start()-mode re-entry every timeout s */
    double min_threshold;         /* 0.005  SoundBuffer.MIN_THRESHOLD              */
    double initial_threshold;     /* 0.01   SoundBuffer.silence_threshold init     */
    double rescore_margin;        /* 1e-3   |score - threshold| re-scored in fp64  */
    int32_t ring_format;          /* EWK_RING_F32 (default) or EWK_RING_I16                    */
    int32_t reserved1;
} ewk_config;

/* One level-1 pass (wakeword.py:1097-1124), with its level-2 result. */
typedef struct ewk_event {
    int32_t stream;
    int32_t length;               /* len(word_audio)                               */
    int64_t tick;                 /* virtual tick (time = tick * tick_seconds)     */
    int64_t ring_start;           /* first sample of the segment inside the stream ring */
    double time;
    double score;                 /* scaled similarity (NaN allowed)               */
    int32_t match;                /* score >= similarity_threshold                 */
    int32_t flags;                /* EWK_EV_*                                      */
} ewk_event;

/* Per-stream gate state snapshot (SoundBuffer + _detect_word locals). */
typedef struct ewk_stream_state {
    int64_t samples_collected;
    int64_t tick;
    double silence_threshold;
    double last_rms;
    double silence_start_time;
    double sound_start_time;
    double sound_end_time;
    double start_time;
    int32_t pointer;
    int32_t state;                /* 0 waiting, 1 in_silence, 2 in_sound, 3 after_sound */
    int32_t started;              /* detection running (ring filled once)          */
    int32_t last_silent;
} ewk_stream_state;

void ewk_default_config(ewk_config* cfg);
const char* ewk_last_error(void);
int ewk_abi_version(void);
/* number of visible HIP devices (0 when none); never fails */
int ewk_device_count(void);
/* Which HIP runtime this library's calls bind to: the file that defines the
 * hipLaunchKernel it resolved (dladdr) and hipRuntimeGetVersion (-1 if unavailable).
 * libewk.so links the system ROCm runtime (libamdhip64.so.7); a process that loaded
 * another copy first with RTLD_GLOBAL (PyTorch-ROCm wheels bundle one) binds that
 * copy instead -- then both libraries share ONE runtime and device pointers and
 * hipStream_t values pass between them.  Two runtimes that each own the device are
 * never in use at once. */
int ewk_runtime_info(char* path, int32_t cap, int32_t* hip_version);

/* Engine: device index, number of concurrent streams (0 = scorer only).  Read from the environment
 * at creation: EWK_SCORE_OVERLAP=1 (score tick t beside the gate of tick t + 1) and
 * EWK_GATE_GRID_MAX=<positive integer> (at most that many workgroups per gate launch, below the
 * built-in 131,072: a wave then steps several streams in turn; same results, for tests). */
int ewk_create(ewk_engine** out, int device, int32_t n_streams, const ewk_config* cfg);
void ewk_destroy(ewk_engine* e);
int ewk_sync(ewk_engine* e);
/* the engine's hipStream_t (as void*) */
void* ewk_stream_handle(ewk_engine* e);

/* ---- level 2: the matcher (WordMatcher, wakeword.py:520-639) ---------------- */

/* WordMatcher.set_reference(audio) (wakeword.py:569-578): template = MFCC
 * mean/std of `pcm` computed by the same HIP pipeline as every candidate. */
int ewk_template_from_pcm(ewk_engine* e, const float* pcm, int64_t n);
/* Direct template load (40 floats). */
int ewk_set_template(ewk_engine* e, const float* mean20, const float* std20);
/* Returns EWK_ENOTEMPLATE when none is set. */
int ewk_get_template(ewk_engine* e, float* mean20, float* std20);
/* WordMatcher.matches(audio, threshold) / WakeWord(similarity_threshold=) (wakeword.py:627-639, 676). */
int ewk_set_similarity_threshold(ewk_engine* e, double threshold);

/* WordMatcher.extract_mfcc + calculate_similarity + matches over a ragged
 * batch (wakeword.py:544-639).  Segment i is pcm[offsets[i] : offsets[i] +
 * lengths[i]].  Host buffers; any out_* may be NULL.  Without a template only
 * mean/std are produced (EWK_ENOTEMPLATE if flags has EWK_SCORE_REQUIRE_TEMPLATE). */
int ewk_score_segments(ewk_engine* e, const float* pcm, int64_t n_pcm,
                       const int64_t* offsets, const int32_t* lengths, int32_t n_seg,
                       float* out_mean, float* out_std, double* out_score, uint8_t* out_match,
                       int32_t flags);

/* Device-resident variant: every pointer is device memory; `stream` is a
 * hipStream_t (NULL = the engine stream).  Asynchronous; no host sync. */
int ewk_score_segments_device(ewk_engine* e, const float* d_pcm,
                              const int64_t* d_offsets, const int32_t* d_lengths, int32_t n_seg,
                              float* d_mean, float* d_std, double* d_score, uint8_t* d_match,
                              int32_t flags, void* stream);

/* fp64 reference-precision scorer (the rescoring path) on host buffers. */
int ewk_score_segments_f64(ewk_engine* e, const float* pcm, int64_t n_pcm,
                           const int64_t* offsets, const int32_t* lengths, int32_t n_seg,
                           double* out_mean, double* out_std, double* out_score, int32_t flags);

/* ---- level 2 against many references: the template bank ----------------------- */
/* A bank is a list of words; a word is 1..EWK_BANK_MAX_PER_WORD templates (several
 * recordings of it) stored contiguously, with one threshold.  Each segment of a batch is
 * scored against every template of one word (word[i], or word 0 without an index array):
 * the MFCC statistics are computed once per segment and every further template costs one
 * cosine score on them.  The engine's single template and every entry point above are
 * unaffected by a bank. */
#define EWK_BANK_MAX_PER_WORD 64
#define EWK_BANK_MAX_TEMPLATES 65536
typedef struct ewk_bank_result {   /* 24 bytes */
    double best_score;            /* max over the word's templates ignoring NaN; NaN when all are NaN */
    uint64_t hit_mask;            /* bit j: template word_first[w] + j scored >= the word's threshold */
    int32_t best_tmpl;            /* bank-wide index of best_score's template (lowest on ties), -1 when all NaN */
    uint8_t match;                /* hit_mask != 0 */
    uint8_t rescored;             /* scores of this segment come from the fp64 statistics */
    uint16_t pad;
} ewk_bank_result;

/* Word w is templates word_first[w] .. word_first[w + 1] - 1 of mean / stdv ([K][20] float32,
 * K = word_first[n_words], word_first[0] = 0).  thresholds: one per word, or NULL: every word
 * uses the engine's similarity threshold (ewk_set_similarity_threshold) as it stands at each
 * scoring call.  Replaces any bank already set (waits for the engine's stream first; a bank
 * scoring call still running on a caller's stream must have finished). */
int ewk_bank_set(ewk_engine* e, int32_t n_words, const int32_t* word_first, const float* mean,
                 const float* stdv, const double* thresholds);
/* The same with template k computed from pcm[offsets[k] : offsets[k] + lengths[k]] as
 * ewk_template_from_pcm computes its template. */
int ewk_bank_from_pcm(ewk_engine* e, int32_t n_words, const int32_t* word_first, const float* pcm,
                      int64_t n_pcm, const int64_t* offsets, const int32_t* lengths,
                      const double* thresholds);
int ewk_bank_clear(ewk_engine* e);
/* 0 / 0 without a bank; either pointer may be NULL. */
int ewk_bank_info(ewk_engine* e, int32_t* n_words, int32_t* n_templates);
/* Template `tmpl` (bank-wide index) of the bank; EWK_ENOTEMPLATE without a bank. */
int ewk_bank_get(ewk_engine* e, int32_t tmpl, float* mean20, float* std20);
/* Score segment i against the templates of word[i] (word NULL: word 0).  Host buffers.
 * out_scores (NULL or [n_seg][stride], stride >= the bank's largest word):
 * out_scores[i * stride + j] is the score against template word_first[word[i]] + j, NaN at
 * and past the word's size.  flags: EWK_SCORE_F32_CANDIDATES.  EWK_ENOTEMPLATE without a
 * bank; EWK_EINVAL for a word index outside [0, n_words). */
int ewk_score_segments_bank(ewk_engine* e, const float* pcm, int64_t n_pcm, const int64_t* offsets,
                            const int32_t* lengths, int32_t n_seg, const int32_t* word,
                            ewk_bank_result* out, double* out_scores, int32_t stride, int32_t flags);
/* Device-resident variant: every pointer is device memory, `stream` a hipStream_t (NULL = the
 * engine's stream).  Not fully asynchronous: after the float32 pass the count of segments
 * that need the fp64 statistics is read back (a 4-byte copy and one synchronisation of
 * `stream`); the fp64 pass, when there is one, is then enqueued and the call returns without
 * waiting for it.  A word[i] outside [0, n_words) cannot be checked from the host: that
 * segment gets best_tmpl = -1, a NaN best_score, no hit, and NaN in its out_scores row. */
int ewk_score_segments_bank_device(ewk_engine* e, const float* d_pcm, const int64_t* d_offsets,
                                   const int32_t* d_lengths, int32_t n_seg, const int32_t* d_word,
                                   ewk_bank_result* d_out, double* d_out_scores, int32_t stride,
                                   int32_t flags, void* stream);

/* ---- level 1 + 2: the streaming gate (SoundBuffer + _detect_word) ------------ */

/* One tick for every stream: SoundBuffer._add_sound_to_buffer with a `block`
 * sample callback per stream (wakeword.py:454-486), then is_silent()
 * (wakeword.py:488-513) and one _detect_word FSM step (wakeword.py:1059-1118).
 * Stream s's samples are pcm[s*stride : s*stride + block].  Segments that pass
 * level 1 are scored on the device (level 2) and queued as events. */
int ewk_push(ewk_engine* e, const float* pcm, int64_t stride, int32_t flags);
/* Same for n_ticks consecutive ticks: tick t of stream s is
 * pcm[s*stride + t*tick_stride ...]. One launch sequence, no host sync. */
int ewk_push_many(ewk_engine* e, const float* pcm, int64_t stride, int64_t tick_stride,
                  int32_t n_ticks, int32_t flags);
/* int16 PCM variants (PortAudio / WAV PCM16 as delivered; decoded on the device as
 * x / 32768 -- exactly soundfile's / librosa.load's float32 -- halving ingest bytes). */
int ewk_push_pcm16(ewk_engine* e, const int16_t* pcm, int64_t stride, int32_t flags);
int ewk_push_many_pcm16(ewk_engine* e, const int16_t* pcm, int64_t stride, int64_t tick_stride,
                        int32_t n_ticks, int32_t flags);
/* Drain every queued event (waits for every push so far), sorted by (tick, stream, listener).
 * If more than `cap` are queued nothing is consumed and EWK_EINVAL is returned (poll
 * again with a larger buffer).  If a bank overflowed (more than max(4096, 4 * n_streams)
 * events between polls) its events are dropped, the queue is re-armed so later pushes
 * keep working, and EWK_ENOMEM reports the loss. */
int ewk_poll(ewk_engine* e, ewk_event* out, int32_t cap, int32_t* n_out);
/* Pipelined drain: returns the events of the pushes made before the previous
 * ewk_poll_lagged call, without waiting for the pushes made since -- the GPU
 * keeps working on tick t while the host consumes tick t-1 (one call of latency). */
int ewk_poll_lagged(ewk_engine* e, ewk_event* out, int32_t cap, int32_t* n_out);
int ewk_get_stream_state(ewk_engine* e, int32_t stream, ewk_stream_state* out);
/* A new WakeWord._detect_word call (wakeword.py:1048-1057) on `stream` (-1 = all): for
 * streams whose detection runs, the FSM restarts from the current is_silent() with
 * start_time = now; `reentry_timeout` (<= 0: continuous, > 0: start()-mode re-entry
 * every reentry_timeout s) applies to every later push.  Stream-ordered, asynchronous. */
int ewk_reenter(ewk_engine* e, int32_t stream, double reentry_timeout);
/* SoundBuffer.return_last_n_seconds(n) (wakeword.py:498-513) as float32 (ring values are the float32 input). */
int ewk_read_last(ewk_engine* e, int32_t stream, int64_t n_samples, float* out, int64_t* n_out);
/* Copy the samples of a queued/polled event (ring must not have wrapped over it). */
int ewk_read_segment(ewk_engine* e, int32_t stream, int64_t ring_start, int32_t length, float* out);
/* Reset all stream state (ring, threshold, FSM, event queue).  A stream bank stays enabled. */
int ewk_reset_streams(ewk_engine* e);

/* ---- stream lifecycle: push and reset individual streams ------------------------ */
/* Clients connect and drop, a network source is a packet late, a slot is reused: the calls below
 * deliver ticks to, and reset, a subset of the streams.
 *
 * Own clock.  A stream's tick is the number of ticks delivered to it since creation or its last
 * reset.  Its virtual clock (tick * tick_seconds), its re-entry timeout, ewk_event.tick and
 * ewk_event.time are its own: stream s produces exactly what a one-stream engine produces when fed
 * the same blocks in the same order, whatever the other streams were given in between.  An engine
 * that is only ever pushed with ewk_push* is in lockstep and behaves as before.  The first
 * ewk_push_streams* or ewk_reset_stream_list desynchronises it: from then on ewk_push* (a tick for
 * every stream) also continues each stream's own clock, and ewk_normalize_events tests an event
 * against its stream's tick.  ewk_reset_streams returns the engine to lockstep.  ewk_poll keeps its
 * (tick, stream) order, each tick on its stream's clock.
 *
 * `streams` is always a host array, also with EWK_PUSH_DEVICE (only pcm is device memory then):
 * 4 bytes per stream against 6.4 KB of audio.  It is validated on the host before anything is
 * enqueued or changed: 1 <= n <= n_streams, every index in [0, n_streams), no index twice (two
 * waves would run one stream) -- else EWK_EINVAL, naming the offending entry.  Any order; the
 * array may die when the call returns, as pcm may. */
/* Ticks for a subset of the streams.  Row i of pcm -- pcm[i*stride + t*tick_stride ...], input_block
 * samples, strides in input samples as for ewk_push_many -- is tick t of stream streams[i].  Every
 * listed stream gets the same n_ticks; gate launches are cut and scored as for ewk_push_many
 * (single template, stream bank, EWK_SCORE_OVERLAP=1).  With an input rate set the history carried
 * from push to push is that of streams[i]. */
int ewk_push_streams(ewk_engine* e, const int32_t* streams, int32_t n, const float* pcm,
                     int64_t stride, int64_t tick_stride, int32_t n_ticks, int32_t flags);
int ewk_push_streams_pcm16(ewk_engine* e, const int32_t* streams, int32_t n, const int16_t* pcm,
                           int64_t stride, int64_t tick_stride, int32_t n_ticks, int32_t flags);
/* Streams streams[0..n) back to the state of a new engine; every other stream is untouched.
 * Stream-ordered behind the pushes so far (and behind their scoring), no host synchronisation.
 * After it each listed stream equals a stream of a freshly created engine: ring and block RMSs
 * zero, initial threshold, tick 0, and with an input rate set an empty resampler history whose
 * first `delay` outputs are zero again.  Events of the stream already queued keep their scores,
 * but their samples are gone: ewk_read_segment / ewk_normalize_events on them is the caller's
 * error (ewk_normalize_events reports an event from a tick its stream has not been pushed, or
 * overwritten samples, where its tick test sees it).  Poll, then reset. */
int ewk_reset_stream_list(ewk_engine* e, const int32_t* streams, int32_t n);
/* Ticks delivered to each listed stream since creation or its last reset.  streams NULL: streams 0..n-1.
 * Host bookkeeping only: no device access, no wait.  (The mirror costs nothing per ewk_push* on a
 * lockstep engine -- one engine tick -- and O(n) per subset push or list reset: an engine base
 * tick plus a per-stream delta, 8 bytes per stream, allocated when the engine desynchronises.) */
int ewk_stream_ticks(ewk_engine* e, const int32_t* streams, int32_t n, int64_t* out);

/* ---- packet ingest: any number of samples per stream ---------------------------- */
/* Sources do not deliver whole ticks: an RTP or WebRTC client sends 10, 20, 30 or 60 ms packets, a
 * decoder hands out what it decoded.  The calls below take, for a list of streams, any number of
 * samples each, and re-block them on the device: every stream keeps the samples of its unfinished
 * block (`pending`, in [0, input_block)) in a carry row in device memory, and the gate steps for a
 * stream whenever a whole block has arrived.  Stream s produces exactly what a one-stream engine
 * produces when fed the same samples cut into blocks -- every event field and the score's bits --
 * however the samples were split into chunks.
 *
 * Chunk i is pcm[offsets[i] .. offsets[i] + counts[i]): the next counts[i] input samples of stream
 * streams[i], at the input rate when one is set (ewk_set_input_rate), else at 16 kHz.  streams,
 * offsets and counts are always host arrays (`streams` as for ewk_push_streams); pcm is host
 * memory, or device memory with EWK_PUSH_DEVICE; n_pcm is its length in samples.  counts[i] may be
 * 0, and at most EWK_CHUNK_MAX_TICKS * input_block.  Any sample offset is legal: a float row need
 * not be 16-byte aligned, an int16 offset may be odd (the kernel copies 16 bytes at a time where
 * source and destination agree in phase, as host chunks always do, and narrower at the edges).
 * The push makes (pending + counts[i]) / input_block gate ticks for the stream, taken in order
 * from its carry followed by the chunk, and leaves (pending + counts[i]) % input_block samples in
 * the carry.  Streams that make the same number of ticks share their gate launches, which are cut
 * and scored as for ewk_push_streams; ewk_stream_ticks follows the ticks made.  A push in which no
 * stream completes a block only moves samples.
 *
 * The carry has the ring's sample type.  PCM16 chunks into a float ring are decoded as x / 32768
 * when they are appended (exact: the stream equals one pushed with ewk_push_pcm16); float chunks
 * into an int16 ring are refused, as float pushes are.
 *
 * Everything is validated on the host before anything is enqueued or changed -- the list rules of
 * ewk_push_streams, every count in range, 0 <= offsets[i] and offsets[i] + counts[i] <= n_pcm --
 * else EWK_EINVAL, naming the offending entry.  The first chunk push desynchronises the engine, as
 * a subset push does, and allocates the carry (input_block samples per stream: 6,400 bytes for a
 * float ring at block 1600, 3,200 for an int16 ring), 4 bytes of host mirror per stream and the
 * staging of the descriptors; the buffer of the assembled ticks grows to the largest push.  An
 * engine that is never chunk-pushed allocates none of it.
 *
 * A tick push to a stream with pending samples would put its audio out of order: ewk_push_streams*
 * on such a stream, and ewk_push* while any stream has pending samples, return EWK_EINVAL naming
 * the stream and its pending count.  ewk_reset_streams, ewk_reset_stream_list (for the streams it
 * lists) and ewk_set_input_rate (the unit changes) drop the pending samples. */
#define EWK_CHUNK_MAX_TICKS 64
int ewk_push_chunks(ewk_engine* e, const int32_t* streams, int32_t n, const float* pcm, int64_t n_pcm,
                    const int64_t* offsets, const int32_t* counts, int32_t flags);
int ewk_push_chunks_pcm16(ewk_engine* e, const int32_t* streams, int32_t n, const int16_t* pcm, int64_t n_pcm,
                          const int64_t* offsets, const int32_t* counts, int32_t flags);
/* Samples each listed stream holds in its carry (0 on an engine that was never chunk-pushed).
 * streams NULL: streams 0..n-1.  Reads the host mirror: no device access, no wait. */
int ewk_stream_pending(ewk_engine* e, const int32_t* streams, int32_t n, int32_t* out);
/* The planning step of a chunk push as a pure host function: no engine, no device.  For chunk i of
 * counts[i] samples to a stream holding pending[i] in [0, in_block): ticks[i] = (pending[i] +
 * counts[i]) / in_block and new_pending[i] = (pending[i] + counts[i]) % in_block.  order: the
 * *n_ticking chunks with ticks >= 1, sorted by (ticks, position in the call).  Groups: the runs of
 * equal ticks in order -- group g is order[group_first[g] .. group_first[g + 1]) and makes
 * group_ticks[g] ticks; group_ticks holds group_cap entries, group_first group_cap + 1 (at most
 * EWK_CHUNK_MAX_TICKS groups exist).  EWK_EINVAL, with nothing written, for in_block < 1, a NULL
 * array, a pending or count out of range, or more groups than group_cap. */
int ewk_chunk_plan(int32_t in_block, int32_t n, const int32_t* pending, const int32_t* counts,
                   int32_t* ticks, int32_t* new_pending, int32_t* order, int32_t* n_ticking,
                   int32_t* group_ticks, int32_t* group_first, int32_t group_cap, int32_t* n_groups);

/* ---- level 1 + 2 against many references: the stream bank ---------------------- */
/* From the next push on, every gated event of stream s is scored against the templates of word
 * stream_word[s] of the engine's bank (NULL: word 0 for every stream) instead of the single
 * template, on the device and in the same push: the event carries the best score, the decision
 * (per-word threshold, or the engine's as it stands at each push when the bank was set with
 * NULL thresholds) and, in its flags, EWK_EV_BANK and the best template (EWK_EV_BEST).
 * Candidates are float64, as on the whole ring path.  No single template is needed.  The
 * per-template hit_mask and score row are not delivered per event: a caller who wants them
 * reads the segment back (ewk_read_segment) and scores it with ewk_score_segments_bank.
 * Host array [n_streams], copied.  EWK_ENOTEMPLATE without a bank, EWK_EINVAL for an engine
 * without streams or an index outside [0, n_words).  Waits for the pushes so far.  While
 * enabled, ewk_bank_set / ewk_bank_from_pcm / ewk_bank_clear return EWK_EINVAL ("disable the
 * stream bank first").  The first call allocates the per-event buffers (488 bytes per event
 * slot, 4 slots per stream), freed with the engine. */
int ewk_stream_bank_enable(ewk_engine* e, const int32_t* stream_word);
int ewk_stream_bank_disable(ewk_engine* e);   /* back to the single template; no-op when off */
/* With the stream bank on: stream streams[i] listens for word words[i] from the next push on
 * (a slot reused by a client with another word).  Host arrays, `streams` as for ewk_push_streams.
 * Stream-ordered: the events of the pushes so far keep the word they were scored with, no wait.
 * If the bank was enabled with stream_word NULL the per-stream array is created first, all zeros.
 * EWK_EINVAL when the stream bank is off, for a stream out of range or listed twice, or a word
 * outside [0, n_words); nothing changes then. */
int ewk_stream_bank_assign(ewk_engine* e, const int32_t* streams, int32_t n, const int32_t* words);

/* ---- level 1 per word: detector profiles ------------------------------------------ */
/* In the reference every WakeWord owns its gate timings: the four durations derived from its
 * reference recording (_auto_calculate_speech_durations, wakeword.py:827-943) and its start()-mode
 * re-entry timeout.  A detector profile is those per-WakeWord fields of ewk_config; an engine
 * holds a table of 0..EWK_PROFILE_MAX profiles and every stream points at one of them, the way
 * it points at a word of the stream bank.
 *
 * Profile index.  -1 is the engine's own configuration, exactly as without a table -- including
 * whatever ewk_reenter last stored as its re-entry timeout.  Every stream starts at -1, and a
 * stream on -1 behaves bit for bit as before whether or not a table exists.  Indices 0..n-1 are
 * the table's entries.  The gate re-reads the stream's timings at every launch; nothing else of
 * the stream (block, ring, thresholds, tick_seconds) is per profile.
 *
 * Ring safety.  The longest segment request of a profile is int((speech_duration_max +
 * post_speech_silence + tick_seconds + padding) * sample_rate) + 2 samples (capped at the
 * reference ring).  A compact ring (ewk_config.ring_samples) must hold that plus one block for
 * every profile of the table, and the number of ticks per gate launch (ewk_push_many) follows the
 * largest request over the engine's configuration and the table; it returns to the engine's own
 * when the table is cleared. */
#define EWK_PROFILE_MAX 65536
typedef struct ewk_detector_profile {   /* 56 bytes; the per-WakeWord fields of ewk_config */
    double pre_speech_silence, speech_duration_min, speech_duration_max, post_speech_silence;
    double padding, max_segment_seconds;
    double reentry_timeout;             /* <= 0: continuous; > 0: start()-mode re-entry */
} ewk_detector_profile;
/* The engine's configuration as a profile (what index -1 means; e NULL: the reference defaults
 * of ewk_default_config). */
void ewk_default_detector_profile(const ewk_engine* e_or_null, ewk_detector_profile* out);
/* Replace the table (host array, copied).  n = 0 or profiles NULL: table off, every stream back
 * to -1.  Every entry is validated as ewk_create validates the same fields: the four durations
 * positive, speech_duration_min <= speech_duration_max, padding >= 0, max_segment_seconds > 0,
 * no NaN, n <= EWK_PROFILE_MAX, and with a compact ring the request above plus one block within
 * ring_samples -- else EWK_EINVAL naming the entry and the field (or the samples needed), and
 * nothing changes.  Replacing a table while a stream points at an index >= n is refused
 * (EWK_EINVAL): assign those streams first, or clear the table.  EWK_EINVAL for an engine without
 * streams.  Waits for the pushes so far.  The first table allocates the per-stream index (4 bytes
 * per stream on the device, 4 on the host), freed with the engine. */
int ewk_detector_profiles_set(ewk_engine* e, const ewk_detector_profile* profiles, int32_t n);
/* 0 without a table. */
int ewk_detector_profiles_info(ewk_engine* e, int32_t* n_profiles);
/* Entry `profile` of the table; -1: the engine's configuration (ewk_default_detector_profile). */
int ewk_detector_profile_get(ewk_engine* e, int32_t profile, ewk_detector_profile* out);
/* Stream streams[i] is gated with profile profiles[i] (-1: the engine's configuration) from the
 * next push on.  Host arrays, `streams` as for ewk_push_streams (validated before anything is
 * enqueued, no duplicates); every profile in [-1, n_profiles), else EWK_EINVAL and nothing
 * changes.  Stream-ordered behind the pushes so far, no host wait.  The stream's FSM state and
 * clock are not touched: the next tick steps the same state with the new numbers, as the
 * reference would if the attributes of a live WakeWord were changed between two polls.  A lockstep
 * engine stays in lockstep.  ewk_reset_streams and ewk_reset_stream_list keep the assignments, as
 * they keep word assignments: a reused slot calls this. */
int ewk_stream_profile_assign(ewk_engine* e, const int32_t* streams, int32_t n, const int32_t* profiles);
/* The profile of each listed stream (streams NULL: streams 0..n-1); all -1 without a table.
 * Host mirror: no device access, no wait. */
int ewk_stream_profiles(ewk_engine* e, const int32_t* streams, int32_t n, int32_t* out);

/* ---- level 1 for several words on one microphone: stream listeners ---------------------- */
/* In the reference a room that listens for several words is several WakeWord objects on one
 * device (examples/multi_stage.py): one SoundBuffer, and per WakeWord its own _detect_word call,
 * timings and reference word.  A stream has 1..EWK_LISTENERS_MAX listeners; a listener is a pair
 * (detector profile, word of the stream bank).  All listeners of a stream share its ring, its block
 * RMSs and adaptive threshold, is_silent, its clock and its `started` flag -- one ingest and one
 * threshold pass per tick whatever their number.  Each listener has its own _detect_word state
 * (state, silence_start, sound_start, sound_end, start_time, re-entries), its own timings and its
 * own word: it cuts and queues its own events, each scored against its word, and the events that
 * carry (stream s, listener j) are exactly those of a one-stream engine configured with the
 * listener's profile and word and fed the same blocks -- every field and the score's bits, flags
 * apart from the listener bits.  Listeners multiply a stream's event rate; the event queues keep
 * their capacity (max(4096, 4 * n_streams) events between polls) and their overflow behaviour.
 *
 * Listener 0 is what a stream has without this section: the FSM of ewk_get_stream_state, the
 * profile of ewk_stream_profile_assign, the word of ewk_stream_bank_assign (both calls keep
 * addressing listener 0).  A stream that was never set has that one listener, and an engine
 * without a stream of more than one listener runs the gate kernels it ran before.
 *
 * ewk_reset_streams / ewk_reset_stream_list return every listener's state to the initial state
 * and keep the table, as they keep profile and word assignments.  ewk_reenter re-enters every
 * listener of the stream(s).  ewk_detector_profiles_set refuses to shorten (or clear) a table a
 * listener still points past, and ewk_stream_bank_enable a bank without a listener's word; both
 * name the stream and the listener and change nothing.  ewk_poll / ewk_poll_lagged sort by (tick,
 * stream, listener). */
#define EWK_LISTENERS_MAX 16
#define EWK_EV_LISTENER_SHIFT 16          /* bits 16..19 of ewk_event.flags: the listener that cut the event */
#define EWK_EV_LISTENER(flags) (((flags) >> EWK_EV_LISTENER_SHIFT) & 15)
typedef struct ewk_listener { int32_t profile; int32_t word; } ewk_listener;   /* profile -1: the engine's configuration */

/* Stream streams[i] has count[i] (1..EWK_LISTENERS_MAX) listeners from the next push on:
 * listeners[i * stride + j], j < count[i].  Host arrays, `streams` as for ewk_push_streams.
 * Everything is validated before anything is enqueued or changed: every count in
 * [1, EWK_LISTENERS_MAX], stride >= the largest count, every profile in [-1, n_profiles) (-1 only,
 * without a table), every word in [0, n_words) while the stream bank is on and 0 while it is off
 * -- else EWK_EINVAL naming the stream, the listener and the field.  Stream-ordered behind the
 * pushes so far and their scoring, no host wait; a lockstep engine stays in lockstep.
 *   listener 0      its entry is written through to the stream's profile index and word, as the two
 *                   assign calls would; its FSM state and the stream's clock are untouched.
 *   j >= 1, old     a listener that existed keeps its FSM state and gets the new numbers.
 *   j >= 1, new     starts as a new _detect_word call starts: on a started stream as ewk_reenter
 *                   starts listener 0 (state from the last is_silent, silence_start and start_time =
 *                   the stream's tick * tick_seconds); on a stream whose ring is still filling it
 *                   enters at the tick the ring fills, together with listener 0.
 *   dropped         a listener at or past a smaller count loses its state; re-added later it is new.
 * The first call that gives a stream more than one listener allocates the per-stream table, states
 * and count on the device (16 x 8 + 15 x 40 + 4 = 732 bytes per stream) and the host mirror (132
 * bytes per stream), freed with the engine. */
int ewk_stream_listeners_set(ewk_engine* e, const int32_t* streams, int32_t n, const int32_t* count,
                             const ewk_listener* listeners, int32_t stride);
/* Host mirror, no device access: *n_out listeners of `stream` (1 for a stream never set).  Up to
 * `cap` of them are written to `out` (may be NULL with cap 0). */
int ewk_stream_listeners(ewk_engine* e, int32_t stream, ewk_listener* out, int32_t cap, int32_t* n_out);
/* ewk_get_stream_state with the FSM fields (state and the four times) of listener `listener`
 * (0: the same as ewk_get_stream_state); EWK_EINVAL for a listener the stream does not have. */
int ewk_get_listener_state(ewk_engine* e, int32_t stream, int32_t listener, ewk_stream_state* out);

/* ---- either side of the path --------------------------------------- */
/* Level-3 input: WakeWord._transcribe_audio's normalisation (wakeword.py:1019-1025)
 * y = x - mean(x); y /= max|y| if > 0; y *= 1.5; clip to [-1, 1], float64 and
 * bit-identical to numpy (pairwise mean), on the device.  Outputs are packed:
 * segment i starts at out[sum of the previous lengths].  out is host memory unless
 * flags has EWK_OUT_DEVICE.  Segments of a float32 batch (pcm host memory unless
 * EWK_PCM_DEVICE) ... */
int ewk_normalize_segments(ewk_engine* e, const float* pcm, int64_t n_pcm, const int64_t* offsets,
                           const int32_t* lengths, int32_t n_seg, double* out, int32_t flags);
/* ... or gated segments straight from the stream rings (polled events: stream,
 * ring_start, length), the reference's word_audio of each event. */
int ewk_normalize_events(ewk_engine* e, const ewk_event* events, int32_t n, double* out, int32_t flags);
/* Level-3 front end: the input features of the Whisper model the reference hands each normalised
 * segment to (transcriber.py:122-134), computed on the device in one call.  For a segment and
 * n_frames frames (1..3000; 3000 is the model's 30 s window):
 *   y   the normalisation above (float64), rounded once to float32;
 *   x   n_frames * 160 float32 samples: y cut to that length, zeros behind it;
 *   xp  x reflect-padded by 200 samples at both ends (xp[-j] = x[j], and x[2 n - 2 - j] past the end);
 *   frame t = xp[160 t .. 160 t + 400) times the periodic Hann window 0.5 - 0.5 cos(2 pi i / 400);
 *   P   the squared magnitude of its 201 rfft bins;
 *   L   log10(max(mel @ P, 1e-10)), mel the float32 Slaney filterbank (16 kHz, n_fft 400, 80 bands);
 *   out = (max(L, max of L over the whole [80][n_frames]) - 8) + 4) / 4.
 * So a frame that reads only pad zeros is (max(-10, Lmax - 8) + 4) / 4, a segment that is all zeros
 * after normalisation (or has length 0) is -1.5 everywhere, and a segment with a non-finite sample
 * is NaN in every element.  Only the frames that read a sample of the segment are transformed.
 * Layout: out[i][m][t], i < n, band m < 80, frame t < n_frames contiguous -- n * 80 * n_frames
 * float32, or with EWK_FEAT_BF16 as many bf16 values, each the float32 value rounded to nearest
 * even.  out is host memory unless flags has EWK_OUT_DEVICE.  The work runs on the engine's stream
 * (ewk_stream_handle), behind every push and scoring pass enqueued before it, and the call returns
 * once the features are written.  Normalised samples, raw log-mel frames and staging live in engine
 * scratch that grows with the largest call and is shared by both entry points, so calls on one
 * engine must not overlap.  Errors: EWK_EINVAL for n_frames outside 1..3000, unknown flags and NULL
 * pointers; a refused call writes nothing.
 * ... of gated segments straight from the stream rings (float32, int16 and compact rings, segments
 * across a ring's end included): polled events as for ewk_normalize_events, refused with
 * EWK_EOVERWRITTEN on the same rule. */
#define EWK_FEAT_BF16 8       /* ewk_whisper_features_*: write bf16 instead of float32 */
int ewk_whisper_features_events(ewk_engine* e, const ewk_event* events, int32_t n, void* out, int32_t n_frames,
                                int32_t flags);
/* ... or of segments of a linear float32 batch, shaped like ewk_normalize_segments (pcm host
 * memory unless EWK_PCM_DEVICE; offsets and lengths are host arrays either way). */
int ewk_whisper_features_segments(ewk_engine* e, const float* pcm, int64_t n_pcm, const int64_t* offsets,
                                  const int32_t* lengths, int32_t n_seg, void* out, int32_t n_frames,
                                  int32_t flags);
/* Positives for the level-3 confirm gather (SURVEY.md 8b `ewk_gather_detections`, 8e):
 * the reference confirms every detection (wakeword.py:1120-1130); on N GPUs only the
 * positives cross xGMI.  Compacts the matched segments of a scored batch -- d_score /
 * d_match as ewk_score_segments_device wrote them -- into d_out (device memory,
 * capacity >= n, or >= *d_count + n with EWK_COMPACT_APPEND) in segment order, record
 * i = {first_id + segment index, score, step}, and leaves the count in *d_count (device
 * memory): no host sync, so a C/C++ host can hand d_out / d_count straight to its own
 * RCCL collective.  EWK_COMPACT_APPEND keeps the *d_count
 * records already there (K steps batched into one gather, the batch step of
 * easywakeword_amd.shard.MatchGather); otherwise *d_count is overwritten.
 * Asynchronous on `stream` (NULL = the engine's stream); the engine's scratch is shared,
 * so calls on different streams must be ordered by the caller. */
#define EWK_COMPACT_APPEND 1
typedef struct ewk_positive {
    int64_t id;                   /* first_id + index of the segment in its batch */
    double score;                 /* its scaled similarity (>= threshold) */
    int64_t step;                 /* caller's step tag (e.g. the batch number) */
} ewk_positive;
int ewk_compact_positives(ewk_engine* e, const double* d_score, const uint8_t* d_match, int32_t n,
                          int64_t first_id, int64_t step, ewk_positive* d_out, int32_t* d_count,
                          int32_t flags, void* stream);
/* WAV / PCM16 ingest (librosa.load of a 16 kHz PCM16 file = int16 / 32768 as float32):
 * host arrays unless EWK_PCM_DEVICE (then both are device memory, asynchronous). */
int ewk_decode_pcm16(ewk_engine* e, const int16_t* in, int64_t n, float* out, int32_t flags);

/* ---- G.711 ingest: PCMU / PCMA decoded on the device ------------------------------ */
/* The baseline RTP payloads are G.711 mu-law (PCMU) and A-law (PCMA): one code byte per sample at
 * 8 kHz.  A code is a 16-bit integer v (csrc/ewk_g711.h: branch-free integer arithmetic, equal to
 * CPython's audioop.ulaw2lin / alaw2lin at width 2 on all 256 codes; mu-law -32124..32124 with 0x7F
 * and 0xFF both 0, A-law -32256..32256 with smallest magnitude 8), and the sample is v / 32768,
 * exact in float32 and the expression every PCM16 decode of the engine uses: an engine pushed G.711
 * bytes produces what an engine pushed the decoded PCM16 produces -- every event field, the
 * score's bits, the ring samples and the thresholds.  The codec is memoryless: there is no
 * per-stream state, resets, ewk_set_input_rate and snapshots are unchanged, and a stream may be
 * pushed float32, PCM16 and G.711 in any order, tick by tick. */
#define EWK_G711_ULAW 0
#define EWK_G711_ALAW 1
/* Host only, no engine, no device: the 256 decoded values of a law.  EWK_EINVAL for another law. */
int ewk_g711_table(int32_t law, int16_t* out256);
/* One-shot decode to float32, shaped like ewk_decode_pcm16: host arrays unless EWK_PCM_DEVICE
 * (then both are device memory and the call is asynchronous); `in` at any byte alignment.  Works
 * on an engine without streams. */
int ewk_decode_g711(ewk_engine* e, const uint8_t* in, int64_t n, float* out, int32_t law, int32_t flags);
/* Ticks for every stream: the arguments of ewk_push_many_pcm16, the samples one byte each.
 * Strides, offsets and counts are in samples, which are bytes here; any byte alignment of pcm is
 * legal, for host and device pointers, and a stride or tick_stride need not be a multiple of 4.
 * G.711 is an 8 kHz codec and the gate runs at cfg.sample_rate, so an input rate must be set
 * (ewk_set_input_rate, normally 8000; any rate the resampler accepts works, the bytes are just
 * samples): without one the push returns EWK_EINVAL and says so.  An EWK_RING_I16 ring, which
 * refuses an input rate, refuses G.711 too.  A law outside {0, 1} is EWK_EINVAL.  Everything else
 * is as for PCM16: the list rules of ewk_push_streams, the refusal of a tick push onto pending
 * samples, desynchronisation, ewk_stream_ticks, gate launches cut and scored as for
 * ewk_push_many.  The codes are decoded inside the resampler launch (profile kind 3), read once,
 * straight into its LDS staging; the gate kernels are those of a float32 push with a rate set.
 * Every rule is validated on the host before anything is enqueued or changed. */
int ewk_push_g711(ewk_engine* e, const uint8_t* pcm, int64_t stride, int64_t tick_stride,
                  int32_t n_ticks, int32_t law, int32_t flags);
int ewk_push_streams_g711(ewk_engine* e, const int32_t* streams, int32_t n, const uint8_t* pcm,
                          int64_t stride, int64_t tick_stride, int32_t n_ticks, int32_t law, int32_t flags);
/* Packet ingest (ewk_push_chunks_pcm16's arguments and rules): an RTP client's 160-byte packets
 * as they arrive.  laws: NULL (every chunk is `law`) or a host array [n], one law per chunk -- a
 * fleet mixes PCMU and PCMA in one call; an entry outside {0, 1} is EWK_EINVAL naming it (`law` is
 * not read then).  The codes are decoded by the assembly launch (profile kind 4) into the float32
 * carry and tick rows; ewk_stream_pending counts samples as before. */
int ewk_push_chunks_g711(ewk_engine* e, const int32_t* streams, int32_t n, const uint8_t* pcm, int64_t n_pcm,
                         const int64_t* offsets, const int32_t* counts, int32_t law, const uint8_t* laws,
                         int32_t flags);

/* ---- ingest at the source's own sample rate: the device resampler ------------------ */
/* The reference gets 16 kHz from PortAudio (sd.InputStream(samplerate=16000), wakeword.py:438-444)
 * and from librosa.load(sr=16000); sources without either (network, files, decoders whose output
 * is already in device memory) deliver 8, 44.1, 48 kHz.  The filter is the one of
 * easywakeword_amd.audio.resample = scipy.signal.resample_poly(window=("kaiser", 5.0)):
 * g = gcd(in, out), up = out / g, down = in / g, half = 10 * max(up, down),
 * h = firwin(2 * half + 1, 1 / max(up, down), ("kaiser", 5.0)) * up, zero-phase:
 * y[m] = sum_k h[k] * xu[m * down + half - k] with xu[i * up] = x[i], zeros beyond both ends of x;
 * float64 accumulation over the taps of the output's phase, one rounding to float32. */
/* The filter alone (host, no engine, no device): writes *up, *down and *n_taps = 2 * half + 1,
 * then the taps (float64) when cap >= *n_taps -- else EWK_EINVAL (also for a rate <= 0). */
int ewk_resample_design(int32_t in_rate, int32_t out_rate, double* taps, int32_t cap,
                        int32_t* n_taps, int32_t* up, int32_t* down);
/* A whole signal in_rate -> cfg.sample_rate: *n_out = ceil(n_in * out / in) samples, equal to
 * audio.resample(x, in_rate, 16000) (EWK_EINVAL, with *n_out set, when cap is smaller).  in / out
 * are host memory unless flags has EWK_PCM_DEVICE / EWK_OUT_DEVICE; asynchronous on the engine's
 * stream when both are device memory.  Works on an engine without streams. */
int ewk_resample(ewk_engine* e, const float* in, int64_t n_in, int32_t in_rate,
                 float* out, int64_t cap, int64_t* n_out, int32_t flags);
/* Streaming: from the next push on, every ewk_push / ewk_push_many / ewk_push_pcm16 /
 * ewk_push_many_pcm16 reads in_block = block * down / up samples at in_rate per stream and tick
 * (4800 at 48 kHz, 4410 at 44.1 kHz, 800 at 8 kHz for block 1600; stride and tick_stride count
 * input samples), resamples them on the device with the last J + 1 input samples of each stream
 * carried from push to push (J = floor(2 * half / up) + 1 taps per output) and hands the gate the
 * 16 kHz block.  The zero-phase filter looks ahead, so the 16 kHz stream is the whole-signal
 * resample y delayed by delay = ceil(half / down) samples: its sample n is y[n - delay], zero for
 * n < delay (10 samples = 0.625 ms when downsampling, 20 from 8 kHz).  Events, ring_start, ticks,
 * ewk_read_last / ewk_read_segment, the bank and the stream bank stay in the 16 kHz domain.
 * in_rate 0 or cfg.sample_rate: off.  Waits for the pushes so far and clears the history (as
 * ewk_reset_streams does; the rate stays set across a reset).  The first call allocates the
 * history and one tick of resampled blocks (a longer ewk_push_many grows it), freed with the
 * engine.  EWK_EINVAL: an engine without streams, an EWK_RING_I16 ring (resampled samples are not
 * int16), block * down not a multiple of up (11,025 Hz with block 1600), a filter over the
 * kernel's size (up > 1024, or more than 12,288 staged input samples per workgroup). */
int ewk_set_input_rate(ewk_engine* e, int32_t in_rate);
/* The rate in force with its samples per tick and delay (cfg.sample_rate, block, 0 when off);
 * any pointer may be NULL. */
int ewk_input_rate_info(ewk_engine* e, int32_t* in_rate, int32_t* in_block, int32_t* delay);

/* ---- stream snapshots: export and import listed streams between engines ---------- */
/* A stream leaves the engine it was created in and continues in any slot of another engine of the
 * same geometry -- after a restart, on another GPU, in a rebalanced shard -- as if nothing had
 * happened: exported after k ticks and imported elsewhere, it goes on producing the events the
 * source would have produced, every field (ring_start included) and the score's bits.
 *
 * A snapshot of n streams is (a) ewk_stream_meta meta[n], always host memory: what the engine's
 * host mirrors hold of the stream, and what an importer checks before it touches anything; and
 * (b) a payload of n records of record_bytes each, host or device memory, stream i at payload +
 * i * record_bytes.  A record is the stream's device state in the sections below, each starting
 * at a multiple of 16 bytes, record_bytes a multiple of 128:
 *   EWK_SNAP_GATE       the gate state (SoundBuffer fields and listener 0's _detect_word locals)
 *   EWK_SNAP_LISTENERS  the _detect_word locals of listeners 1..EWK_LISTENERS_MAX-1 (40 bytes each)
 *   EWK_SNAP_BLOCK_RMS  n_blocks float64 block RMSs
 *   EWK_SNAP_SORTED     the same ascending (the current copy behind the adaptive threshold)
 *   EWK_SNAP_RING       the sample ring as stored (sring_len samples of the ring's type, unrotated:
 *                       pointer, and every later event's ring_start, stay valid)
 *   EWK_SNAP_HISTORY    with an input rate set: the resampler's last hist_len input samples (float32)
 *   EWK_SNAP_FRESH      ... and its flag "no push since the history was cleared" (int32)
 *   EWK_SNAP_CARRY      the unfinished block of packet ingest: in_block samples of the ring's type,
 *                       the first `pending` of them meaningful
 * Every byte not covered by live state is zero (padding, listener rows past the count, the carry
 * past `pending`, RMS rows that are not valid yet): two exports of an untouched stream are
 * byte-identical, and a record exported straight after an import equals the imported one.
 *
 * The layout is a function of the geometry alone: sample_rate, block, buffer_seconds / ring_len,
 * sring_len, ring_format, n_blocks, tick_seconds, and the input rate with its in_block and
 * hist_len.  Its fingerprint is a 64-bit hash of exactly those.  Gate durations, thresholds and
 * similarity_threshold are not geometry: a stream may be imported into an engine with other
 * timings, exactly as a profile assignment changes them under a running stream.
 *
 * Queued events are not part of a snapshot: they stay in the source's banks for ewk_poll. */
#define EWK_SNAPSHOT_MAGIC 0x4e534b45u   /* "EKSN" */
#define EWK_SNAPSHOT_VERSION 1
#define EWK_SNAP_GATE 0
#define EWK_SNAP_LISTENERS 1
#define EWK_SNAP_BLOCK_RMS 2
#define EWK_SNAP_SORTED 3
#define EWK_SNAP_RING 4
#define EWK_SNAP_HISTORY 5
#define EWK_SNAP_FRESH 6
#define EWK_SNAP_CARRY 7
#define EWK_SNAP_SECTIONS 8
typedef struct ewk_snapshot_section { int64_t offset; int64_t bytes; } ewk_snapshot_section;
typedef struct ewk_snapshot_layout {   /* 208 bytes */
    uint32_t magic;               /* EWK_SNAPSHOT_MAGIC */
    int32_t version;              /* EWK_SNAPSHOT_VERSION */
    int32_t sample_rate, block, buffer_seconds, ring_format, n_blocks;
    int32_t in_rate;              /* the rate pushes arrive at (sample_rate without a resampler) */
    int32_t in_block;             /* samples per tick at in_rate */
    int32_t hist_len;             /* resampler history samples per stream (0 without a resampler) */
    int64_t ring_len, sring_len;
    double tick_seconds;
    ewk_snapshot_section section[EWK_SNAP_SECTIONS];
    int64_t record_bytes;
    uint64_t fingerprint;
} ewk_snapshot_layout;
typedef struct ewk_stream_meta {       /* 176 bytes */
    uint32_t magic;
    int32_t version;
    int64_t tick;                 /* ticks delivered to the stream (ewk_stream_ticks) */
    int64_t record_bytes;         /* of the layout the record was written with */
    uint64_t fingerprint;         /* ... and its geometry */
    int32_t pending;              /* samples in the carry (ewk_stream_pending) */
    int32_t profile;              /* detector profile of listener 0 (-1: the engine's configuration) */
    int32_t word;                 /* stream-bank word of listener 0 (0 without a stream bank) */
    int32_t n_listeners;          /* 1..EWK_LISTENERS_MAX */
    ewk_listener listeners[EWK_LISTENERS_MAX];   /* rows 0..n_listeners-1 (row 0 = profile, word); the rest {-1, 0} */
} ewk_stream_meta;

/* The layout of a configuration (NULL: the defaults) at an input rate (0 or sample_rate: none).
 * Host only: no engine, no device.  EWK_EINVAL, with nothing written, for a configuration
 * ewk_create would refuse or a rate ewk_set_input_rate would refuse for it. */
int ewk_snapshot_plan(const ewk_config* cfg, int32_t in_rate, ewk_snapshot_layout* out);
/* The engine's own layout, with its current input rate.  EWK_EINVAL for an engine without streams. */
int ewk_snapshot_info(ewk_engine* e, ewk_snapshot_layout* out);
/* Export: meta[i] and record i describe stream streams[i] (`streams` as for ewk_push_streams).
 * payload is host memory, or device memory with EWK_OUT_DEVICE; EWK_EINVAL, with nothing written,
 * when cap_bytes < n * record_bytes.  Waits for nothing but joins the scoring of the pushes so
 * far on the engine's stream first, so their events are scored and queued in this engine.  The
 * exported streams are left as they are: export is a read.  To device memory the call is
 * stream-ordered on the engine's stream, without host synchronisation; to host memory it returns
 * when the payload is in the caller's buffer (copied through bounded pinned staging, two buffers
 * of at most 32 MB or one record).  meta comes from the host mirrors alone. */
int ewk_export_streams(ewk_engine* e, const int32_t* streams, int32_t n, ewk_stream_meta* meta,
                       void* payload, int64_t cap_bytes, int32_t flags);
/* Import: stream streams[i] of e becomes the stream of record i.  payload is host memory, or
 * device memory with EWK_PCM_DEVICE (then no host synchronisation is made; the payload must stay
 * valid until the engine's stream has passed the call).  Everything is checked on the host before
 * anything is enqueued, and a refused import (EWK_EINVAL) changes nothing, on the device or in a
 * host mirror: the list; bytes == n * record_bytes; every meta's magic, version, record_bytes and
 * fingerprint against the engine's own layout (the input rate in force included); pending in [0,
 * in_block); every listener row as ewk_stream_listeners_set checks it -- profile in [-1,
 * n_profiles), word in [0, n_words) with the stream bank on and 0 with it off -- with a message
 * naming the stream and the table.  The caller sets the tables first; it may reassign afterwards
 * with the assign calls, which keep the FSM state and the clock.
 * The import desynchronises the engine (as a subset push does), sets each stream's tick, pending
 * count, profile, word and listeners, allocating what the first such call allocates, and scatters
 * the records on the engine's stream.  The ring row is written with agent-scope stores, as every
 * ring initialisation is.  Events of a slot's previous occupant that are still queued stay
 * queued, as after ewk_reset_stream_list. */
int ewk_import_streams(ewk_engine* e, const int32_t* streams, int32_t n, const ewk_stream_meta* meta,
                       const void* payload, int64_t bytes, int32_t flags);

/* ---- measurement ------------------------------------------------------------ */
/* When enabled, these launches are bracketed by hipEvents on the stream they run on:
 * the scorer and re-score launches of ewk_score_segments_device, of the bank scoring
 * calls (host and device pointers) and of every streaming scoring pass, every gate
 * launch, and the resampler.  The host-copy calls ewk_score_segments and
 * ewk_score_segments_f64 (so ewk_template_from_pcm and ewk_bank_from_pcm too) launch
 * without brackets.  ewk_profile_read resolves them (synchronizing) and returns
 * the summed device time and launch count per kernel family, then clears.
 * kind: 0 = fp32 MFCC scorer (k_score_f32), 1 = fp64 re-scorer, 2 = gate ticks,
 * 3 = resampler launches (ewk_resample, and the resample + history save of a push),
 * 4 = the assembly launch of a chunk push (ewk_push_chunks*),
 * 5 = the pack and unpack launches of ewk_export_streams / ewk_import_streams. */
int ewk_profile_enable(ewk_engine* e, int32_t on);
int ewk_profile_read(ewk_engine* e, int32_t kind, double* total_ms, int64_t* launches);
/* Which gate kernel the engine's last gate launch ran (read-only, host bookkeeping, no wait; any
 * pointer may be NULL).  The gate has one instantiation per family, picked from the geometry, the
 * input's type and alignment, and whether detector profiles or listeners are set:
 *   rb:   block-RMS slots per lane kept in registers, 2 (up to 128 blocks) or 8 (up to 512);
 *         0 = the arrays stay in device memory
 *   dma:  0 = the tick's samples through registers, 1 = float32 input staged by LDS-DMA in 4-byte
 *         pieces, 2 = in 16-byte pieces, 3 = int16 input in 16-byte pieces (int16 stage)
 *   prof, lsn: 1 when the per-stream timings / the listener lanes are compiled in
 * all four -1 before the first launch.  block_tree_kind / last_tree_kind: how the sum over a
 * callback block / over the last 0.1 s follows numpy's pairwise order -- 0 = one leaf of fewer
 * than 8 elements, 1 = one leaf (at most 128), 2 = a balanced tree of at most 16 leaves, 3 = the
 * general tree.  For tests and tuning: a change of the dispatch shows here instead of moving a
 * workload silently onto another kernel.  EWK_EINVAL for an engine without streams. */
int ewk_gate_launch_info(ewk_engine* e, int32_t* rb, int32_t* dma, int32_t* prof, int32_t* lsn,
                         int32_t* block_tree_kind, int32_t* last_tree_kind);

#ifdef __cplusplus
}
#endif
#endif /* EWK_H */
