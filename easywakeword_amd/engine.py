"""Thin Python owners of an ``ewk_engine`` (the C ABI in include/ewk.h).

``Engine``       -- scorer-only engine (level 2): the WordMatcher hot path.
``StreamEngine`` -- N concurrent streams on one GPU (levels 1 + 2): the
                    SoundBuffer + _detect_word hot loop for many microphones.

No CPU fallback exists: construction raises when libewk.so or a GPU is missing.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import asdict, dataclass
from typing import Optional, Tuple

import numpy as np

from . import _lib
from ._lib import N_MFCC, check
from .snapshot import StreamSnapshot, layout_dict

FREQUENCY = 16000


def _f32(audio) -> np.ndarray:
    a = np.asarray(audio)
    if a.ndim != 1:
        a = a.reshape(-1)
    return np.ascontiguousarray(a, dtype=np.float32)


def _law(law) -> int:
    """"ulaw" / "alaw" -> EWK_G711_ULAW / EWK_G711_ALAW."""
    try:
        return _lib.G711_LAWS[law]
    except (KeyError, TypeError):
        raise ValueError(f'law must be "ulaw" or "alaw", got {law!r}') from None


def _pack(segs):
    """Ragged float32 arrays -> (pcm, offsets int64, lengths int32)."""
    n = len(segs)
    lengths = np.array([len(s) for s in segs], dtype=np.int32)
    offsets = np.zeros(n, dtype=np.int64)
    if n:
        offsets[1:] = np.cumsum(lengths[:-1], dtype=np.int64)
    pcm = np.ascontiguousarray(np.concatenate(segs) if n else np.zeros(0, np.float32), dtype=np.float32)
    return pcm, offsets, lengths


@dataclass
class DetectorProfile:
    """The level-1 timings one WakeWord owns (include/ewk.h, ewk_detector_profile): an entry of
    StreamEngine.set_detector_profiles.  A field left None takes the engine's configuration."""
    pre_speech_silence: Optional[float] = None
    speech_duration_min: Optional[float] = None
    speech_duration_max: Optional[float] = None
    post_speech_silence: Optional[float] = None
    padding: Optional[float] = None
    max_segment_seconds: Optional[float] = None
    reentry_timeout: Optional[float] = None    # <= 0: continuous; > 0: start()-mode re-entry


def bank_layout(words, thresholds=None):
    """Layout of a template bank (include/ewk.h): `words` is a list of words, each a sequence of
    1..64 templates (only the lengths are read here).  Returns (word_first int32[n_words + 1],
    thresholds float64[n_words] or None); word w is templates word_first[w] .. word_first[w + 1]
    - 1.  Raises ValueError for an empty bank or word, a word over EWK_BANK_MAX_PER_WORD
    templates, a bank over EWK_BANK_MAX_TEMPLATES or a `thresholds` of another length."""
    sizes = [len(w) for w in words]
    if not sizes:
        raise ValueError("a bank needs at least one word")
    for w, s in enumerate(sizes):
        if s < 1:
            raise ValueError(f"word {w} has no templates")
        if s > _lib.EWK_BANK_MAX_PER_WORD:
            raise ValueError(f"word {w} has {s} templates; at most {_lib.EWK_BANK_MAX_PER_WORD} per word")
    total = int(sum(sizes))
    if total > _lib.EWK_BANK_MAX_TEMPLATES:
        raise ValueError(f"bank has {total} templates; at most {_lib.EWK_BANK_MAX_TEMPLATES}")
    word_first = np.zeros(len(sizes) + 1, dtype=np.int32)
    word_first[1:] = np.cumsum(sizes)
    thr = None
    if thresholds is not None:
        thr = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
        if thr.size != len(sizes):
            raise ValueError(f"{thr.size} thresholds for {len(sizes)} words")
        if np.isnan(thr).any():
            raise ValueError("threshold is NaN")
    return word_first, thr


class Engine:
    """Owns one ewk_engine on `gpu` (scorer-only unless n_streams > 0)."""

    def __init__(self, gpu: int = 0, n_streams: int = 0, config: Optional[_lib.EwkConfig] = None, **cfg):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        if config is None:
            config = _lib.default_config(**cfg)
        self.config = config
        check(self._lib.ewk_create(C.byref(self._h), int(gpu), int(n_streams), C.byref(config)))
        self.gpu = int(gpu)
        self.n_streams = int(n_streams)

    # -- lifetime ------------------------------------------------------------
    def close(self) -> None:
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            self._lib.ewk_destroy(h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def stream_handle(self) -> int:
        return int(self._lib.ewk_stream_handle(self._h) or 0)

    def sync(self) -> None:
        check(self._lib.ewk_sync(self._h))

    # -- measurement ---------------------------------------------------------
    def profile(self, on: bool = True) -> None:
        check(self._lib.ewk_profile_enable(self._h, int(bool(on))))

    def profile_read(self, kind: int = 0):
        """(total_ms, launches) of the kernel family since the last read
        (0 = fp32 scorer, 1 = fp64 re-scorer, 2 = gate, 3 = resampler, 4 = chunk assembly,
        5 = snapshot pack / unpack)."""
        ms = C.c_double(0.0)
        n = C.c_int64(0)
        check(self._lib.ewk_profile_read(self._h, int(kind), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    # -- template ------------------------------------------------------------
    def template_from_pcm(self, audio) -> None:
        a = _f32(audio)
        check(self._lib.ewk_template_from_pcm(self._h, _lib.fptr(a), len(a)))

    def set_template(self, mean, std) -> None:
        m = _f32(mean)
        s = _f32(std)
        if m.size != N_MFCC or s.size != N_MFCC:
            raise ValueError(f"template must be {N_MFCC} means and {N_MFCC} stds")
        check(self._lib.ewk_set_template(self._h, _lib.fptr(m), _lib.fptr(s)))

    def get_template(self) -> Tuple[np.ndarray, np.ndarray]:
        m = np.zeros(N_MFCC, np.float32)
        s = np.zeros(N_MFCC, np.float32)
        check(self._lib.ewk_get_template(self._h, _lib.fptr(m), _lib.fptr(s)))
        return m, s

    def set_threshold(self, threshold: float) -> None:
        check(self._lib.ewk_set_similarity_threshold(self._h, float(threshold)))
        self.config.similarity_threshold = float(threshold)

    # -- level 2 over ragged host batches ------------------------------------
    def score(self, segments, require_template: bool = True, candidate_dtype: str = "auto"):
        """MFCC stats + score of a list of 1-D arrays.  Returns
        (mean[n,20] f32, std[n,20] f32, score[n] f64, match[n] bool).

        candidate_dtype selects the reference arithmetic of the score:
        "float64" (SoundBuffer slices, the streaming path), "float32"
        (WordMatcher fed float32 audio) or "auto" (float32 iff every segment is)."""
        if candidate_dtype == "auto":
            f32 = all(np.asarray(s).dtype == np.float32 for s in segments) and len(segments) > 0
        else:
            f32 = np.dtype(candidate_dtype) == np.float32
        segs = [_f32(s) for s in segments]
        n = len(segs)
        lengths = np.array([len(s) for s in segs], dtype=np.int32)
        offsets = np.zeros(n, dtype=np.int64)
        if n:
            offsets[1:] = np.cumsum(lengths[:-1], dtype=np.int64)
        pcm = np.concatenate(segs) if n else np.zeros(0, np.float32)
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        return self.score_packed(pcm, offsets, lengths, require_template, f32)

    def score_packed(self, pcm: np.ndarray, offsets: np.ndarray, lengths: np.ndarray,
                     require_template: bool = True, f32_candidates: bool = False):
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        lengths = np.ascontiguousarray(lengths, dtype=np.int32)
        n = len(lengths)
        mean = np.zeros((n, N_MFCC), np.float32)
        std = np.zeros((n, N_MFCC), np.float32)
        score = np.full(n, np.nan, np.float64)
        match = np.zeros(n, np.uint8)
        check(self._lib.ewk_score_segments(self._h, _lib.fptr(pcm), len(pcm), _lib.i64ptr(offsets),
                                           _lib.i32ptr(lengths), n, _lib.fptr(mean), _lib.fptr(std),
                                           _lib.dptr(score), _lib.u8ptr(match), self._flags(require_template,
                                                                                            f32_candidates)))
        return mean, std, score, match.astype(bool)

    @staticmethod
    def _flags(require_template: bool, f32: bool) -> int:
        return (_lib.EWK_SCORE_REQUIRE_TEMPLATE if require_template else 0) | \
            (_lib.EWK_SCORE_F32_CANDIDATES if f32 else 0)

    def score_f64(self, segments, candidate_dtype: str = "float64"):
        """Reference-precision (float64) path: (mean[n,20], std[n,20], score[n])."""
        f32 = np.dtype(candidate_dtype) == np.float32
        segs = [_f32(s) for s in segments]
        n = len(segs)
        lengths = np.array([len(s) for s in segs], dtype=np.int32)
        offsets = np.zeros(n, dtype=np.int64)
        if n:
            offsets[1:] = np.cumsum(lengths[:-1], dtype=np.int64)
        pcm = np.ascontiguousarray(np.concatenate(segs) if n else np.zeros(0, np.float32), dtype=np.float32)
        mean = np.zeros((n, N_MFCC), np.float64)
        std = np.zeros((n, N_MFCC), np.float64)
        score = np.full(n, np.nan, np.float64)
        check(self._lib.ewk_score_segments_f64(self._h, _lib.fptr(pcm), len(pcm), _lib.i64ptr(offsets),
                                               _lib.i32ptr(lengths), n, _lib.dptr(mean), _lib.dptr(std),
                                               _lib.dptr(score), self._flags(False, f32)))
        return mean, std, score

    # -- template bank: many references per segment -------------------------------
    @staticmethod
    def _thr_ptr(thr):
        return _lib.dptr(thr) if thr is not None else None

    def set_bank(self, words, thresholds=None) -> None:
        """`words`: a list of words, each a list of (mean[20], std[20]) templates (1..64 per
        word); `thresholds`: one per word, or None for the engine's threshold."""
        word_first, thr = bank_layout(words, thresholds)
        mean = np.zeros((int(word_first[-1]), N_MFCC), np.float32)
        std = np.zeros_like(mean)
        k = 0
        for w in words:
            for m, s in w:
                m, s = _f32(m), _f32(s)
                if m.size != N_MFCC or s.size != N_MFCC:
                    raise ValueError(f"template must be {N_MFCC} means and {N_MFCC} stds")
                mean[k], std[k] = m, s
                k += 1
        check(self._lib.ewk_bank_set(self._h, len(word_first) - 1, _lib.i32ptr(word_first), _lib.fptr(mean),
                                     _lib.fptr(std), self._thr_ptr(thr)))
        self._bank_max_word = int(np.diff(word_first).max())

    def bank_from_pcm(self, words_audio, thresholds=None) -> None:
        """set_bank with every template computed from audio (as template_from_pcm):
        `words_audio` is a list of words, each a list of 1-D arrays."""
        word_first, thr = bank_layout(words_audio, thresholds)
        segs = [_f32(a) for w in words_audio for a in w]
        if any(len(s) == 0 for s in segs):
            raise ValueError("template length must be in [1, 2^31)")
        pcm, offsets, lengths = _pack(segs)
        check(self._lib.ewk_bank_from_pcm(self._h, len(word_first) - 1, _lib.i32ptr(word_first), _lib.fptr(pcm),
                                          len(pcm), _lib.i64ptr(offsets), _lib.i32ptr(lengths), self._thr_ptr(thr)))
        self._bank_max_word = int(np.diff(word_first).max())

    def clear_bank(self) -> None:
        check(self._lib.ewk_bank_clear(self._h))
        self._bank_max_word = 0

    def bank_info(self) -> Tuple[int, int]:
        """(number of words, number of templates); (0, 0) without a bank."""
        nw, nt = C.c_int32(0), C.c_int32(0)
        check(self._lib.ewk_bank_info(self._h, C.byref(nw), C.byref(nt)))
        return int(nw.value), int(nt.value)

    def bank_template(self, tmpl: int) -> Tuple[np.ndarray, np.ndarray]:
        m = np.zeros(N_MFCC, np.float32)
        s = np.zeros(N_MFCC, np.float32)
        check(self._lib.ewk_bank_get(self._h, int(tmpl), _lib.fptr(m), _lib.fptr(s)))
        return m, s

    def score_bank(self, segments, word=None, candidate_dtype: str = "auto", all_scores: bool = False):
        """Score segment i against every template of word[i] (word None: word 0).  Returns a
        structured array (_lib.BANK_RESULT_DTYPE: best_score, hit_mask, best_tmpl, match,
        rescored) and, with all_scores=True, also scores[n, stride] float64: the score against
        template j of the segment's word, NaN past the word's size (stride = the bank's largest word)."""
        if candidate_dtype == "auto":
            f32 = all(np.asarray(s).dtype == np.float32 for s in segments) and len(segments) > 0
        else:
            f32 = np.dtype(candidate_dtype) == np.float32
        pcm, offsets, lengths = _pack([_f32(s) for s in segments])
        n = len(lengths)
        wp = None
        if word is not None:
            word = np.ascontiguousarray(word, dtype=np.int32).reshape(-1)
            if word.size != n:
                raise ValueError(f"{word.size} word indices for {n} segments")
            wp = _lib.i32ptr(word)
        out = np.zeros(n, dtype=_lib.BANK_RESULT_DTYPE)
        stride = getattr(self, "_bank_max_word", 0) or _lib.EWK_BANK_MAX_PER_WORD
        scores = np.full((n, stride), np.nan, np.float64) if all_scores else None
        check(self._lib.ewk_score_segments_bank(self._h, _lib.fptr(pcm), len(pcm), _lib.i64ptr(offsets),
                                                _lib.i32ptr(lengths), n, wp,
                                                out.ctypes.data_as(C.POINTER(_lib.EwkBankResult)),
                                                _lib.dptr(scores) if all_scores else None, stride,
                                                self._flags(False, f32)))
        return (out, scores) if all_scores else out

    def score_bank_device(self, pcm_ptr: int, offsets_ptr: int, lengths_ptr: int, n: int, word_ptr: int,
                          out_ptr: int, scores_ptr: int = 0, stride: int = 0, stream: int = 0,
                          f32_candidates: bool = False) -> None:
        """Device-resident score_bank (e.g. torch tensor data_ptr()s): out_ptr holds n
        ewk_bank_result records (24 bytes each), scores_ptr (0: none) n * stride float64.
        Synchronises `stream` once, after the float32 pass (include/ewk.h)."""
        check(self._lib.ewk_score_segments_bank_device(self._h, C.c_void_p(pcm_ptr), C.c_void_p(offsets_ptr),
                                                       C.c_void_p(lengths_ptr), int(n), C.c_void_p(word_ptr or None),
                                                       C.c_void_p(out_ptr or None), C.c_void_p(scores_ptr or None),
                                                       int(stride), self._flags(False, f32_candidates),
                                                       C.c_void_p(stream or None)))

    def normalize(self, segments) -> list:
        """Level-3 pre-processing of each segment on the GPU (wakeword.py:1019-1025):
        float64, bit-identical to the reference's numpy (see include/ewk.h)."""
        segs = [_f32(s) for s in segments]
        n = len(segs)
        if n == 0:
            return []
        lengths = np.array([len(s) for s in segs], dtype=np.int32)
        offsets = np.zeros(n, dtype=np.int64)
        offsets[1:] = np.cumsum(lengths[:-1], dtype=np.int64)
        pcm = np.ascontiguousarray(np.concatenate(segs), dtype=np.float32)
        out = np.zeros(max(1, int(lengths.sum())), np.float64)
        check(self._lib.ewk_normalize_segments(self._h, pcm.ctypes.data_as(C.c_void_p), len(pcm),
                                               _lib.i64ptr(offsets), _lib.i32ptr(lengths), n,
                                               out.ctypes.data_as(C.c_void_p), 0))
        return [out[o:o + l] for o, l in zip(offsets, lengths)]

    def _feature_out(self, n: int, n_frames: int, dtype: str):
        """The [n, 80, n_frames] output tensor of a whisper_features* call and its flags."""
        import torch
        if dtype not in ("float32", "bfloat16"):
            raise ValueError(f'dtype must be "float32" or "bfloat16", got {dtype!r}')
        if not 1 <= int(n_frames) <= _lib.WHISPER_MAX_FRAMES:
            raise ValueError(f"n_frames = {n_frames} is outside 1..{_lib.WHISPER_MAX_FRAMES}")
        out = torch.empty((n, _lib.WHISPER_MELS, int(n_frames)), device=torch.device("cuda", self.gpu),
                          dtype=torch.bfloat16 if dtype == "bfloat16" else torch.float32)
        return out, _lib.EWK_OUT_DEVICE | (_lib.EWK_FEAT_BF16 if dtype == "bfloat16" else 0)

    def whisper_features(self, segments, n_frames: int = 3000, dtype: str = "float32"):
        """Whisper's log-mel input features of each segment (level-3 normalisation included;
        include/ewk.h, ewk_whisper_features_segments): a [n, 80, n_frames] torch tensor, float32
        or bfloat16, on this engine's device.  `segments`: float32 arrays, or (pcm, offsets,
        lengths) with pcm a float32 torch tensor on this engine's device."""
        pcm_dev = isinstance(segments, tuple) and len(segments) == 3 and hasattr(segments[0], "data_ptr")
        if pcm_dev:
            pcm_t, offsets, lengths = segments
            if str(pcm_t.dtype) != "torch.float32" or not pcm_t.is_contiguous() or pcm_t.device.index != self.gpu:
                raise ValueError("pcm must be a contiguous float32 tensor on this engine's device")
            offsets = np.ascontiguousarray(offsets, dtype=np.int64)
            lengths = np.ascontiguousarray(lengths, dtype=np.int32)
            pcm_ptr, n_pcm, flags_in = C.c_void_p(pcm_t.data_ptr()), pcm_t.numel(), _lib.EWK_PCM_DEVICE
        else:
            pcm, offsets, lengths = _pack([_f32(s) for s in segments])
            pcm_ptr, n_pcm, flags_in = pcm.ctypes.data_as(C.c_void_p), len(pcm), 0
        n = len(lengths)
        out, flags = self._feature_out(n, n_frames, dtype)
        if n:
            check(self._lib.ewk_whisper_features_segments(self._h, pcm_ptr, n_pcm, _lib.i64ptr(offsets),
                                                          _lib.i32ptr(lengths), n, C.c_void_p(out.data_ptr()),
                                                          int(n_frames), flags | flags_in))
        return out

    def decode_pcm16(self, pcm16: np.ndarray) -> np.ndarray:
        """int16 PCM -> float32 (x / 32768, librosa.load's value for 16 kHz PCM16) on the GPU."""
        a = np.ascontiguousarray(pcm16, dtype=np.int16)
        out = np.zeros(a.shape, np.float32)
        if a.size:
            check(self._lib.ewk_decode_pcm16(self._h, a.ctypes.data_as(C.c_void_p), a.size,
                                             out.ctypes.data_as(C.c_void_p), 0))
        return out

    def decode_g711(self, codes: np.ndarray, law: str) -> np.ndarray:
        """G.711 code bytes (`law`: "ulaw" or "alaw") -> float32 (v / 32768, v the code's 16-bit
        value: audio.g711_decode) on the GPU."""
        a = np.ascontiguousarray(codes, dtype=np.uint8)
        out = np.zeros(a.shape, np.float32)
        check(self._lib.ewk_decode_g711(self._h, a.ctypes.data_as(C.c_void_p), a.size,
                                        out.ctypes.data_as(C.c_void_p), _law(law), 0))
        return out

    def resample(self, audio, orig_sr: int) -> np.ndarray:
        """`audio` at orig_sr Hz -> 16 kHz float32 on the GPU: the arithmetic of
        easywakeword_amd.audio.resample (polyphase Kaiser FIR, float64 accumulation),
        ceil(n * 16000 / orig_sr) samples."""
        a = _f32(audio)
        out = np.zeros(-(-len(a) * FREQUENCY // int(orig_sr)) if int(orig_sr) > 0 else 0, np.float32)
        n = C.c_int64(0)
        check(self._lib.ewk_resample(self._h, a.ctypes.data_as(C.c_void_p), len(a), int(orig_sr),
                                     out.ctypes.data_as(C.c_void_p), len(out), C.byref(n), 0))
        return out[: n.value]

    def resample_device(self, in_ptr: int, n_in: int, orig_sr: int, out_ptr: int, cap: int) -> int:
        """Device-resident resample (float32 at in_ptr -> out_ptr, room for `cap` samples);
        asynchronous on the engine's stream.  Returns the number of samples written."""
        n = C.c_int64(0)
        check(self._lib.ewk_resample(self._h, C.c_void_p(in_ptr or None), int(n_in), int(orig_sr),
                                     C.c_void_p(out_ptr or None), int(cap), C.byref(n),
                                     _lib.EWK_PCM_DEVICE | _lib.EWK_OUT_DEVICE))
        return int(n.value)

    def score_device(self, pcm_ptr: int, offsets_ptr: int, lengths_ptr: int, n: int, mean_ptr: int,
                     std_ptr: int, score_ptr: int, match_ptr: int, stream: int = 0,
                     f32_candidates: bool = False) -> None:
        """Device-resident batch (e.g. torch tensor data_ptr()s); asynchronous on `stream`."""
        check(self._lib.ewk_score_segments_device(self._h, C.c_void_p(pcm_ptr), C.c_void_p(offsets_ptr),
                                                  C.c_void_p(lengths_ptr), int(n), C.c_void_p(mean_ptr or None),
                                                  C.c_void_p(std_ptr or None), C.c_void_p(score_ptr or None),
                                                  C.c_void_p(match_ptr or None), self._flags(False, f32_candidates),
                                                  C.c_void_p(stream or None)))


    def compact_positives_device(self, score_ptr: int, match_ptr: int, n: int, first_id: int, out_ptr: int,
                                 count_ptr: int, step: int = 0, append: bool = False, stream: int = 0) -> None:
        """Matched segments of a device batch -> ewk_positive records {id, score, step} at
        out_ptr (device, segment order) and their int32 count at count_ptr (device); with
        append=True after the count already there.  Asynchronous on `stream`, no host sync:
        the buffers go straight to an RCCL gather (include/ewk.h, ewk_compact_positives)."""
        check(self._lib.ewk_compact_positives(self._h, C.c_void_p(score_ptr or None), C.c_void_p(match_ptr or None),
                                              int(n), int(first_id), int(step), C.c_void_p(out_ptr or None),
                                              C.c_void_p(count_ptr or None),
                                              _lib.EWK_COMPACT_APPEND if append else 0, C.c_void_p(stream or None)))


class StreamEngine(Engine):
    """N concurrent 16 kHz streams on one GPU: ring + adaptive threshold + timing
    FSM per stream (level 1) and MFCC matching of every gated segment (level 2)."""

    def __init__(self, n_streams: int, gpu: int = 0, config: Optional[_lib.EwkConfig] = None, **cfg):
        if n_streams <= 0:
            raise ValueError("n_streams must be positive")
        super().__init__(gpu=gpu, n_streams=n_streams, config=config, **cfg)
        self.block = int(self.config.block)
        self.ring_len = int(self.config.buffer_seconds) * FREQUENCY          # the reference ring
        self.sample_ring = int(self.config.ring_samples) or self.ring_len    # samples kept per stream
        # the rate pushes arrive at (set_input_rate), its samples per tick and the delay of the 16 kHz stream
        self.input_rate, self.input_block, self.input_delay = FREQUENCY, self.block, 0

    # -- ingest at the source's own sample rate ---------------------------------
    def set_input_rate(self, hz: int) -> None:
        """From the next push on, blocks arrive at `hz` (e.g. 48000, 44100, 8000): input_block
        samples per stream and tick, resampled to 16 kHz on the device with state carried from
        push to push.  The 16 kHz stream (read_last, events) is audio.resample of the input
        delayed by input_delay samples.  0 or 16000: off.  Clears the resampler's history;
        ValueError for an int16 ring or a rate whose tick is not a whole number of samples."""
        check(self._lib.ewk_set_input_rate(self._h, int(hz)))
        r, b, d = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        check(self._lib.ewk_input_rate_info(self._h, C.byref(r), C.byref(b), C.byref(d)))
        self.input_rate, self.input_block, self.input_delay = int(r.value), int(b.value), int(d.value)

    def push(self, blocks: np.ndarray) -> None:
        """One tick: `blocks` is float32 [n_streams, input_block] (host)."""
        b = np.ascontiguousarray(blocks, dtype=np.float32)
        if b.shape != (self.n_streams, self.input_block):
            raise ValueError(f"expected blocks of shape {(self.n_streams, self.input_block)}, got {b.shape}")
        check(self._lib.ewk_push(self._h, b.ctypes.data_as(C.c_void_p), self.input_block, 0))

    def push_many(self, pcm: np.ndarray) -> None:
        """Several ticks: float32 [n_streams, n_ticks * input_block] (host)."""
        a = np.ascontiguousarray(pcm, dtype=np.float32)
        if a.ndim != 2 or a.shape[0] != self.n_streams or a.shape[1] % self.input_block:
            raise ValueError("pcm must be [n_streams, n_ticks*block]" if self.input_block == self.block else
                             f"pcm must be [n_streams, n_ticks*{self.input_block}] at {self.input_rate} Hz")
        nt = a.shape[1] // self.input_block
        if nt:
            check(self._lib.ewk_push_many(self._h, a.ctypes.data_as(C.c_void_p), a.shape[1], self.input_block, nt, 0))

    def push_pcm16(self, pcm16: np.ndarray) -> None:
        """Ticks of int16 PCM [n_streams, n_ticks * input_block] (host), decoded on the device."""
        a = np.ascontiguousarray(pcm16, dtype=np.int16)
        if a.ndim != 2 or a.shape[0] != self.n_streams or a.shape[1] % self.input_block:
            raise ValueError("pcm16 must be [n_streams, n_ticks*block]" if self.input_block == self.block else
                             f"pcm16 must be [n_streams, n_ticks*{self.input_block}] at {self.input_rate} Hz")
        nt = a.shape[1] // self.input_block
        if nt:
            check(self._lib.ewk_push_many_pcm16(self._h, a.ctypes.data_as(C.c_void_p), a.shape[1], self.input_block,
                                                nt, 0))

    def push_g711(self, codes: np.ndarray, law: str) -> None:
        """Ticks of G.711 code bytes, uint8 [n_streams, n_ticks * input_block] (host), `law` "ulaw"
        (PCMU) or "alaw" (PCMA): decoded inside the device resampler, so an input rate must be set
        (set_input_rate(8000) for telephony).  The engine computes what push_pcm16 of
        audio.g711_decode(codes, law) computes, bit for bit."""
        a = np.ascontiguousarray(codes, dtype=np.uint8)
        if a.ndim != 2 or a.shape[0] != self.n_streams or a.shape[1] % self.input_block:
            raise ValueError("codes must be [n_streams, n_ticks*block]" if self.input_block == self.block else
                             f"codes must be [n_streams, n_ticks*{self.input_block}] at {self.input_rate} Hz")
        nt = a.shape[1] // self.input_block
        if nt:
            check(self._lib.ewk_push_g711(self._h, a.ctypes.data_as(C.c_void_p), a.shape[1], self.input_block,
                                          nt, _law(law), 0))

    def normalize_events(self, events: np.ndarray) -> list:
        """Level-3 pre-processing of polled events straight from the rings (float64 per event)."""
        ev = np.ascontiguousarray(events, dtype=_lib.EVENT_DTYPE)
        n = len(ev)
        if n == 0:
            return []
        lengths = ev["length"].astype(np.int64)
        out = np.zeros(max(1, int(lengths.sum())), np.float64)
        check(self._lib.ewk_normalize_events(self._h, ev.ctypes.data_as(C.POINTER(_lib.EwkEvent)), n,
                                             out.ctypes.data_as(C.c_void_p), 0))
        offs = np.concatenate([[0], np.cumsum(lengths)[:-1]])
        return [out[o:o + l] for o, l in zip(offs, lengths)]

    def normalize_events_device(self, events: np.ndarray) -> list:
        """normalize_events with the float64 output left in GPU memory: a list of torch
        views on this engine's device (level 3 without the host round trip)."""
        import torch
        ev = np.ascontiguousarray(events, dtype=_lib.EVENT_DTYPE)
        n = len(ev)
        if n == 0:
            return []
        lengths = ev["length"].astype(np.int64)
        out = torch.empty(max(1, int(lengths.sum())), dtype=torch.float64, device=torch.device("cuda", self.gpu))
        check(self._lib.ewk_normalize_events(self._h, ev.ctypes.data_as(C.POINTER(_lib.EwkEvent)), n,
                                             C.c_void_p(out.data_ptr()), _lib.EWK_OUT_DEVICE))
        offs = np.concatenate([[0], np.cumsum(lengths)[:-1]])
        return [out[int(o):int(o) + int(l)] for o, l in zip(offs, lengths)]

    def whisper_features_events(self, events: np.ndarray, n_frames: int = 3000, dtype: str = "float32"):
        """Whisper's log-mel input features of polled events, read straight from the rings
        (include/ewk.h, ewk_whisper_features_events): a [n, 80, n_frames] torch tensor, float32 or
        bfloat16, on this engine's device.  RingOverwrittenError as for normalize_events."""
        ev = np.ascontiguousarray(events, dtype=_lib.EVENT_DTYPE)
        out, flags = self._feature_out(len(ev), n_frames, dtype)
        if len(ev):
            check(self._lib.ewk_whisper_features_events(self._h, ev.ctypes.data_as(C.POINTER(_lib.EwkEvent)), len(ev),
                                                        C.c_void_p(out.data_ptr()), int(n_frames), flags))
        return out

    def push_device(self, ptr: int, stride: int, tick_stride: int = 0, n_ticks: int = 1) -> None:
        """Device-resident float32 ticks: stream s, tick t at ptr + 4 * (s * stride + t * tick_stride);
        input_block samples each, strides in input samples (set_input_rate)."""
        check(self._lib.ewk_push_many(self._h, C.c_void_p(ptr), int(stride), int(tick_stride), int(n_ticks),
                                      _lib.EWK_PUSH_DEVICE))

    def push_device_pcm16(self, ptr: int, stride: int, tick_stride: int = 0, n_ticks: int = 1) -> None:
        """Device-resident int16 PCM ticks (indexing as push_device, 2-byte samples)."""
        check(self._lib.ewk_push_many_pcm16(self._h, C.c_void_p(ptr), int(stride), int(tick_stride), int(n_ticks),
                                            _lib.EWK_PUSH_DEVICE))

    def push_device_g711(self, ptr: int, stride: int, tick_stride: int, n_ticks: int, law: str) -> None:
        """Device-resident G.711 ticks (indexing as push_device, 1-byte samples, any alignment)."""
        check(self._lib.ewk_push_g711(self._h, C.c_void_p(ptr), int(stride), int(tick_stride), int(n_ticks),
                                      _law(law), _lib.EWK_PUSH_DEVICE))

    def poll(self, cap: Optional[int] = None, lagged: bool = False) -> np.ndarray:
        """Drain queued events as a structured array (see _lib.EVENT_DTYPE).
        lagged=True: the events of the pushes before the previous lagged poll, without
        waiting for the latest push (pipelined serving; see include/ewk.h)."""
        # a non-lagged poll drains both event banks (each holds up to the engine's queue
        # capacity after a lagged poll), so its default buffer holds two banks
        cap = int(cap or (1 if lagged else 2) * max(4096, 4 * self.n_streams))
        if getattr(self, "_poll_buf", None) is None or len(self._poll_buf) < cap:
            self._poll_buf = np.zeros(cap, dtype=_lib.EVENT_DTYPE)   # reused: polled every tick
            self._poll_n = C.c_int32(0)
        fn = self._lib.ewk_poll_lagged if lagged else self._lib.ewk_poll
        check(fn(self._h, self._poll_buf.ctypes.data_as(C.POINTER(_lib.EwkEvent)), cap, C.byref(self._poll_n)))
        return self._poll_buf[: self._poll_n.value].copy()

    def gate_launch_info(self) -> dict:
        """Which gate kernel the last gate launch ran (include/ewk.h, ewk_gate_launch_info): rb, dma,
        prof, lsn (-1 before the first launch) and block_tree_kind, last_tree_kind (0 = a leaf of
        fewer than 8 elements, 1 = one leaf, 2 = balanced, 3 = general).  Host bookkeeping, no wait."""
        names = ("rb", "dma", "prof", "lsn", "block_tree_kind", "last_tree_kind")
        v = [C.c_int32(-1) for _ in names]
        check(self._lib.ewk_gate_launch_info(self._h, *[C.byref(x) for x in v]))
        return {n: int(x.value) for n, x in zip(names, v)}

    def state(self, stream: int) -> dict:
        st = _lib.EwkStreamState()
        check(self._lib.ewk_get_stream_state(self._h, int(stream), C.byref(st)))
        return {f: getattr(st, f) for f, _ in st._fields_}

    def read_last(self, stream: int, n_samples: int) -> np.ndarray:
        out = np.zeros(max(0, int(n_samples)), np.float32)
        n = C.c_int64(0)
        check(self._lib.ewk_read_last(self._h, int(stream), int(n_samples), _lib.fptr(out), C.byref(n)))
        return out[: n.value]

    def read_segment(self, stream: int, ring_start: int, length: int) -> np.ndarray:
        out = np.zeros(int(length), np.float32)
        check(self._lib.ewk_read_segment(self._h, int(stream), int(ring_start), int(length), _lib.fptr(out)))
        return out

    def reset(self) -> None:
        check(self._lib.ewk_reset_streams(self._h))

    # -- stream lifecycle: push and reset individual streams -----------------------
    def _stream_list(self, streams) -> np.ndarray:
        s = np.ascontiguousarray(streams, dtype=np.int32).reshape(-1)
        if s.size < 1 or s.size > self.n_streams:
            raise ValueError(f"a stream list holds 1..{self.n_streams} streams, got {s.size}")
        return s

    def _push_streams(self, fn, streams, a: np.ndarray, what: str) -> None:
        s = self._stream_list(streams)
        if a.ndim != 2 or a.shape[0] != s.size or a.shape[1] % self.input_block:
            raise ValueError(f"{what} must be [len(streams), n_ticks*block]" if self.input_block == self.block else
                             f"{what} must be [len(streams), n_ticks*{self.input_block}] at {self.input_rate} Hz")
        nt = a.shape[1] // self.input_block
        if nt:
            check(fn(self._h, _lib.i32ptr(s), s.size, a.ctypes.data_as(C.c_void_p), a.shape[1], self.input_block,
                     nt, 0))

    def push_streams(self, streams, pcm: np.ndarray) -> None:
        """Ticks for a subset of the streams: row i of `pcm`, float32 [len(streams), n_ticks *
        input_block] (host), goes to stream streams[i].  Every stream runs on its own clock (ticks
        delivered to it since creation or its last reset): its events are those of a one-stream
        engine fed the same blocks.  ValueError for an empty list, an index out of range or listed
        twice; nothing is delivered then."""
        self._push_streams(self._lib.ewk_push_streams, streams, np.ascontiguousarray(pcm, dtype=np.float32), "pcm")

    def push_streams_pcm16(self, streams, pcm16: np.ndarray) -> None:
        """push_streams with int16 PCM [len(streams), n_ticks * input_block] (host)."""
        self._push_streams(self._lib.ewk_push_streams_pcm16, streams, np.ascontiguousarray(pcm16, dtype=np.int16),
                           "pcm16")

    def push_streams_g711(self, streams, codes: np.ndarray, law: str) -> None:
        """push_streams with G.711 code bytes, uint8 [len(streams), n_ticks * input_block] (host),
        all of `law` ("ulaw" or "alaw"); a fleet that mixes laws makes two calls, or uses
        push_chunks_g711."""
        law = _law(law)
        self._push_streams(lambda *a: self._lib.ewk_push_streams_g711(*a[:-1], law, a[-1]), streams,
                           np.ascontiguousarray(codes, dtype=np.uint8), "codes")

    def push_streams_device(self, streams, ptr: int, stride: int, tick_stride: int = 0, n_ticks: int = 1,
                            pcm16: bool = False, g711: Optional[str] = None) -> None:
        """Device-resident ticks for a subset: row i, tick t at ptr + es * (i * stride + t * tick_stride)
        (es = 4, 2 with pcm16=True, or 1 with g711="ulaw" / "alaw") goes to stream streams[i].
        `streams` stays a host list."""
        s = self._stream_list(streams)
        if g711 is not None:
            if pcm16:
                raise ValueError("pcm16 and g711 exclude each other")
            check(self._lib.ewk_push_streams_g711(self._h, _lib.i32ptr(s), s.size, C.c_void_p(ptr), int(stride),
                                                  int(tick_stride), int(n_ticks), _law(g711), _lib.EWK_PUSH_DEVICE))
            return
        fn = self._lib.ewk_push_streams_pcm16 if pcm16 else self._lib.ewk_push_streams
        check(fn(self._h, _lib.i32ptr(s), s.size, C.c_void_p(ptr), int(stride), int(tick_stride), int(n_ticks),
                 _lib.EWK_PUSH_DEVICE))

    def reset_streams(self, streams) -> None:
        """The listed streams back to the state of a new engine (ring, threshold, FSM, tick 0,
        resampler history); the others are untouched.  Stream-ordered, no wait.  Poll first: events
        of these streams already queued keep their scores but lose their samples."""
        s = self._stream_list(streams)
        check(self._lib.ewk_reset_stream_list(self._h, _lib.i32ptr(s), s.size))

    def stream_ticks(self, streams=None) -> np.ndarray:
        """Ticks delivered to each listed stream (None: all) since creation or its last reset
        (int64; host bookkeeping, no wait)."""
        if streams is None:
            out = np.zeros(self.n_streams, np.int64)
            check(self._lib.ewk_stream_ticks(self._h, None, self.n_streams, _lib.i64ptr(out)))
            return out
        s = np.ascontiguousarray(streams, dtype=np.int32).reshape(-1)
        out = np.zeros(s.size, np.int64)
        if s.size > self.n_streams:
            raise ValueError(f"{s.size} streams listed, the engine has {self.n_streams}")
        check(self._lib.ewk_stream_ticks(self._h, _lib.i32ptr(s), s.size, _lib.i64ptr(out)))
        return out

    # -- packet ingest: any number of samples per stream ---------------------------
    def _push_chunks(self, fn, streams, chunks, dtype) -> None:
        s = self._stream_list(streams)
        parts = [np.ascontiguousarray(c, dtype=dtype).reshape(-1) for c in chunks]
        if len(parts) != s.size:
            raise ValueError(f"{s.size} streams listed, {len(parts)} chunks given")
        counts = np.array([p.size for p in parts], np.int32)
        offsets = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)[:-1]]).astype(np.int64)
        pcm = np.concatenate(parts) if parts else np.zeros(0, dtype)
        check(fn(self._h, _lib.i32ptr(s), s.size, pcm.ctypes.data_as(C.c_void_p), pcm.size, _lib.i64ptr(offsets),
                 _lib.i32ptr(counts), 0))

    def push_chunks(self, streams, chunks) -> None:
        """Any number of samples per stream: chunks[i], a 1-D float32 array (host) of any length up
        to EWK_CHUNK_MAX_TICKS * input_block, holds the next input samples of stream streams[i].
        The engine keeps each stream's unfinished block on the device (stream_pending) and steps
        the gate for a stream whenever a whole block has arrived: its events are those of an engine
        fed the same samples in blocks, however they were cut.  ValueError, with nothing delivered,
        for a bad list or a chunk that is too long."""
        self._push_chunks(self._lib.ewk_push_chunks, streams, chunks, np.float32)

    def push_chunks_pcm16(self, streams, chunks) -> None:
        """push_chunks with int16 PCM chunks (decoded on the device; an int16 ring stores them as they are)."""
        self._push_chunks(self._lib.ewk_push_chunks_pcm16, streams, chunks, np.int16)

    def _chunk_laws(self, law, n: int):
        """(law, laws) of ewk_push_chunks_g711 from one name or a sequence with one name per chunk."""
        if isinstance(law, str):
            return _law(law), None
        laws = np.array([_law(l) for l in law], np.uint8)
        if laws.size != n:
            raise ValueError(f"{n} streams listed, {laws.size} laws given")
        return 0, laws

    def push_chunks_g711(self, streams, chunks, law) -> None:
        """push_chunks with G.711 code bytes (uint8 chunks of any length: an RTP client's 160-byte
        packets as they arrive), decoded on the device.  `law` is "ulaw" or "alaw" for every chunk,
        or a sequence with one name per chunk: a fleet mixes PCMU and PCMA in one call.  Needs an
        input rate (set_input_rate(8000))."""
        s = self._stream_list(streams)
        one, laws = self._chunk_laws(law, s.size)
        lp = laws.ctypes.data_as(C.c_void_p) if laws is not None else None
        self._push_chunks(lambda *a: self._lib.ewk_push_chunks_g711(*a[:-1], one, lp, a[-1]), s, chunks, np.uint8)

    def push_chunks_device(self, streams, ptr: int, n_pcm: int, offsets, counts, pcm16: bool = False,
                           g711=None) -> None:
        """Device-resident chunks: chunk i is the counts[i] samples at ptr + es * offsets[i] (es = 4,
        2 with pcm16=True, or 1 with g711 = a law name or one name per chunk) of a buffer of n_pcm
        samples; any offset, aligned or not.  `streams`, `offsets` and `counts` stay host lists."""
        s = self._stream_list(streams)
        o = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        c = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
        if o.size != s.size or c.size != s.size:
            raise ValueError(f"{s.size} streams listed, {o.size} offsets and {c.size} counts given")
        if g711 is not None:
            if pcm16:
                raise ValueError("pcm16 and g711 exclude each other")
            one, laws = self._chunk_laws(g711, s.size)
            check(self._lib.ewk_push_chunks_g711(self._h, _lib.i32ptr(s), s.size, C.c_void_p(ptr), int(n_pcm),
                                                 _lib.i64ptr(o), _lib.i32ptr(c), one,
                                                 laws.ctypes.data_as(C.c_void_p) if laws is not None else None,
                                                 _lib.EWK_PUSH_DEVICE))
            return
        fn = self._lib.ewk_push_chunks_pcm16 if pcm16 else self._lib.ewk_push_chunks
        check(fn(self._h, _lib.i32ptr(s), s.size, C.c_void_p(ptr), int(n_pcm), _lib.i64ptr(o), _lib.i32ptr(c),
                 _lib.EWK_PUSH_DEVICE))

    def stream_pending(self, streams=None) -> np.ndarray:
        """Samples of an unfinished block each listed stream (None: all) holds on the device
        (int32, in [0, input_block); host bookkeeping, no wait)."""
        if streams is None:
            out = np.zeros(self.n_streams, np.int32)
            check(self._lib.ewk_stream_pending(self._h, None, self.n_streams, _lib.i32ptr(out)))
            return out
        s = np.ascontiguousarray(streams, dtype=np.int32).reshape(-1)
        out = np.zeros(s.size, np.int32)
        if s.size > self.n_streams:
            raise ValueError(f"{s.size} streams listed, the engine has {self.n_streams}")
        check(self._lib.ewk_stream_pending(self._h, _lib.i32ptr(s), s.size, _lib.i32ptr(out)))
        return out

    def assign_stream_words(self, streams, words) -> None:
        """With the stream bank on (set_stream_bank): stream streams[i] listens for word words[i]
        from the next push on; earlier events keep the word they were scored with."""
        s = self._stream_list(streams)
        w = np.ascontiguousarray(words, dtype=np.int32).reshape(-1)
        if w.size != s.size:
            raise ValueError(f"{w.size} word indices for {s.size} streams")
        check(self._lib.ewk_stream_bank_assign(self._h, _lib.i32ptr(s), s.size, _lib.i32ptr(w)))

    # -- detector profiles: per-stream gate timings ---------------------------------
    def _profile_struct(self, i: int, p, base: _lib.EwkDetectorProfile) -> _lib.EwkDetectorProfile:
        d = asdict(p) if isinstance(p, DetectorProfile) else dict(p)
        out = _lib.EwkDetectorProfile()
        for f in _lib.PROFILE_FIELDS:
            v = d.pop(f, None)
            setattr(out, f, float(getattr(base, f) if v is None else v))
        if d:
            raise TypeError(f"profiles[{i}]: unknown field(s) {sorted(d)}")
        return out

    def set_detector_profiles(self, profiles) -> None:
        """The table of detector profiles: a sequence of DetectorProfile instances or dicts of
        their fields (pre_speech_silence, speech_duration_min, speech_duration_max,
        post_speech_silence, padding, max_segment_seconds, reentry_timeout); a missing field takes
        the engine's configuration.  Streams choose an entry with assign_stream_profiles; until
        then, and on index -1, a stream is gated with the engine's configuration as before.
        None or []: table off, every stream back to -1.  Waits for the pushes so far.  ValueError
        (nothing changes) names the entry and field of a bad value, a profile whose longest segment
        does not fit a compact ring, or a stream still pointing past a shorter table."""
        profiles = list(profiles) if profiles is not None else []
        if not profiles:
            check(self._lib.ewk_detector_profiles_set(self._h, None, 0))
            return
        base = _lib.EwkDetectorProfile()
        self._lib.ewk_default_detector_profile(self._h, C.byref(base))
        arr = (_lib.EwkDetectorProfile * len(profiles))(
            *[self._profile_struct(i, p, base) for i, p in enumerate(profiles)])
        check(self._lib.ewk_detector_profiles_set(self._h, arr, len(profiles)))

    def detector_profiles(self) -> list:
        """The table as set: a list of DetectorProfile (empty without a table)."""
        n = C.c_int32(0)
        check(self._lib.ewk_detector_profiles_info(self._h, C.byref(n)))
        out = []
        for i in range(int(n.value)):
            p = _lib.EwkDetectorProfile()
            check(self._lib.ewk_detector_profile_get(self._h, i, C.byref(p)))
            out.append(DetectorProfile(**{f: float(getattr(p, f)) for f in _lib.PROFILE_FIELDS}))
        return out

    def assign_stream_profiles(self, streams, profiles) -> None:
        """Stream streams[i] is gated with entry profiles[i] of the table (-1: the engine's
        configuration) from the next push on.  Its FSM state and clock are kept; stream-ordered,
        no wait.  ValueError (nothing changes) for an index outside [-1, len(table)), a stream out
        of range or listed twice, or without a table."""
        s = self._stream_list(streams)
        p = np.ascontiguousarray(profiles, dtype=np.int32).reshape(-1)
        if p.size != s.size:
            raise ValueError(f"{p.size} profile indices for {s.size} streams")
        check(self._lib.ewk_stream_profile_assign(self._h, _lib.i32ptr(s), s.size, _lib.i32ptr(p)))

    def stream_profiles(self, streams=None) -> np.ndarray:
        """The profile index of each listed stream (None: all), -1 = the engine's configuration
        (int32; host bookkeeping, no wait)."""
        if streams is None:
            out = np.zeros(self.n_streams, np.int32)
            check(self._lib.ewk_stream_profiles(self._h, None, self.n_streams, _lib.i32ptr(out)))
            return out
        s = np.ascontiguousarray(streams, dtype=np.int32).reshape(-1)
        if s.size > self.n_streams:
            raise ValueError(f"{s.size} streams listed, the engine has {self.n_streams}")
        out = np.zeros(s.size, np.int32)
        check(self._lib.ewk_stream_profiles(self._h, _lib.i32ptr(s), s.size, _lib.i32ptr(out)))
        return out

    # -- stream listeners: several (profile, word) pairs on one stream ---------------
    def set_stream_listeners(self, streams, listeners, stride: Optional[int] = None) -> None:
        """Stream streams[i] has the listeners listeners[i] from the next push on: a sequence of
        1.._lib.EWK_LISTENERS_MAX (profile, word) pairs; a bare int is a profile with word 0.  All
        listeners of a stream share its ring, threshold and clock; each runs its own detector with
        its profile's timings (-1: the engine's configuration), and its events -- listener index
        in _lib.event_listener(flags) -- are scored against its word of the stream bank.  Listener
        0 is the stream's own profile and word (assign_stream_profiles / assign_stream_words).
        A listener that existed keeps its state, a new one starts as reenter() starts a stream.
        Stream-ordered, no wait.  ValueError (nothing changes) names the stream, listener and
        field of a bad count, profile or word.  `stride` (default: the longest list) is the row
        length of the table handed to the library."""
        s = self._stream_list(streams)
        rows = [[(int(l), 0) if np.isscalar(l) else (int(l[0]), int(l[1])) for l in row] for row in listeners]
        if len(rows) != s.size:
            raise ValueError(f"{len(rows)} listener lists for {s.size} streams")
        count = np.array([len(r) for r in rows], np.int32)
        stride = max(1, int(count.max())) if stride is None else int(stride)
        tab = (_lib.EwkListener * (max(1, stride) * s.size))()
        for i, row in enumerate(rows):
            for j, (p, w) in enumerate(row[:max(0, stride)]):
                tab[i * stride + j] = _lib.EwkListener(p, w)
        check(self._lib.ewk_stream_listeners_set(self._h, _lib.i32ptr(s), s.size, _lib.i32ptr(count), tab, stride))

    def stream_listeners(self, stream: int) -> list:
        """The listeners of `stream` as (profile, word) pairs (host bookkeeping, no wait): one
        pair, the stream's own profile and word, for a stream never given listeners."""
        out = (_lib.EwkListener * _lib.EWK_LISTENERS_MAX)()
        n = C.c_int32(0)
        check(self._lib.ewk_stream_listeners(self._h, int(stream), out, _lib.EWK_LISTENERS_MAX, C.byref(n)))
        return [(int(out[j].profile), int(out[j].word)) for j in range(int(n.value))]

    def listener_state(self, stream: int, listener: int) -> dict:
        """state(stream) with the detector fields (state and the four times) of `listener`."""
        st = _lib.EwkStreamState()
        check(self._lib.ewk_get_listener_state(self._h, int(stream), int(listener), C.byref(st)))
        return {f: getattr(st, f) for f, _ in st._fields_}

    # -- stream snapshots: listed streams leave this engine and continue in another ---
    def snapshot_layout(self) -> dict:
        """This engine's record layout at its current input rate (snapshot.layout_dict): the
        geometry, "sections" (name -> (offset, bytes)), record_bytes and the fingerprint an
        importer compares."""
        l = _lib.EwkSnapshotLayout()
        check(self._lib.ewk_snapshot_info(self._h, C.byref(l)))
        return layout_dict(l)

    def export_streams(self, streams) -> StreamSnapshot:
        """The listed streams as a StreamSnapshot in host memory: ring, block RMSs and threshold
        history, detector state of every listener, resampler history, pending packet samples, and
        in `meta` the tick, profile, word and listeners.  Joins the scoring of the pushes so far
        (their events stay here, for poll()); the streams themselves are left as they are."""
        s = self._stream_list(streams)
        layout = self.snapshot_layout()
        meta = np.zeros(s.size, dtype=_lib.STREAM_META_DTYPE)
        payload = np.zeros((s.size, layout["record_bytes"]), dtype=np.uint8)
        check(self._lib.ewk_export_streams(self._h, _lib.i32ptr(s), s.size, meta.ctypes.data_as(C.c_void_p),
                                           payload.ctypes.data_as(C.c_void_p), payload.nbytes, 0))
        return StreamSnapshot(meta, payload, layout)

    def import_streams(self, streams, snap: StreamSnapshot) -> None:
        """Stream streams[i] becomes the stream of record i of `snap` and goes on producing the
        events its source would have produced.  This engine must have the snapshot's geometry
        (block, rings, ring format, tick, input rate) and the tables its records point into
        (detector profiles, stream bank) set first; timings and thresholds may differ.  ValueError,
        with nothing changed, names the record and what it does not fit."""
        s = self._stream_list(streams)
        if len(snap) != s.size:
            raise ValueError(f"{len(snap)} records for {s.size} streams")
        meta = np.ascontiguousarray(snap.meta, dtype=_lib.STREAM_META_DTYPE)
        payload = np.ascontiguousarray(snap.payload, dtype=np.uint8)
        check(self._lib.ewk_import_streams(self._h, _lib.i32ptr(s), s.size, meta.ctypes.data_as(C.c_void_p),
                                           payload.ctypes.data_as(C.c_void_p), payload.nbytes, 0))

    def export_streams_device(self, streams, ptr: int, cap: int) -> np.ndarray:
        """export_streams with the records left in device memory at `ptr` (16-byte aligned, room
        for `cap` bytes): stream-ordered on the engine's stream, no wait.  Returns the meta array."""
        s = self._stream_list(streams)
        meta = np.zeros(s.size, dtype=_lib.STREAM_META_DTYPE)
        check(self._lib.ewk_export_streams(self._h, _lib.i32ptr(s), s.size, meta.ctypes.data_as(C.c_void_p),
                                           C.c_void_p(ptr or None), int(cap), _lib.EWK_OUT_DEVICE))
        return meta

    def import_streams_device(self, streams, meta, ptr: int, nbytes: int) -> None:
        """import_streams from records in device memory (on this engine's GPU) at `ptr`: no host
        synchronisation; the records must stay valid until the engine's stream has passed the call."""
        s = self._stream_list(streams)
        m = np.ascontiguousarray(meta, dtype=_lib.STREAM_META_DTYPE).reshape(-1)
        if m.size != s.size:
            raise ValueError(f"{m.size} records for {s.size} streams")
        check(self._lib.ewk_import_streams(self._h, _lib.i32ptr(s), s.size, m.ctypes.data_as(C.c_void_p),
                                           C.c_void_p(ptr or None), int(nbytes), _lib.EWK_PCM_DEVICE))

    def move_streams(self, dst_engine: "StreamEngine", src_streams, dst_streams) -> np.ndarray:
        """Stream src_streams[i] of this engine continues as stream dst_streams[i] of `dst_engine`
        on the same GPU, without a host copy: exported into a device buffer (a torch tensor),
        imported from it behind an event on this engine's stream.  The source streams are left as
        they are (reset_streams frees their slots).  Returns the meta array.  For engines on two
        GPUs copy the records peer to peer between export_streams_device and
        import_streams_device."""
        import torch
        if dst_engine.gpu != self.gpu:
            raise ValueError(f"move_streams works on one GPU (this engine: {self.gpu}, the other: {dst_engine.gpu}); "
                             "across GPUs copy the records peer to peer (INTEGRATION.md)")
        s = self._stream_list(src_streams)
        d = dst_engine._stream_list(dst_streams)
        if d.size != s.size:
            raise ValueError(f"{s.size} source streams for {d.size} destination streams")
        nbytes = int(s.size) * int(self.snapshot_layout()["record_bytes"])
        buf = torch.empty(nbytes, dtype=torch.uint8, device=torch.device("cuda", self.gpu))
        meta = self.export_streams_device(s, buf.data_ptr(), nbytes)
        # the import runs on the other engine's stream: behind this engine's export
        done = torch.cuda.Event()
        src_stream = torch.cuda.ExternalStream(self.stream_handle(), device=torch.device("cuda", self.gpu))
        dst_stream = torch.cuda.ExternalStream(dst_engine.stream_handle(), device=torch.device("cuda", self.gpu))
        done.record(src_stream)
        dst_stream.wait_event(done)
        dst_engine.import_streams_device(d, meta, buf.data_ptr(), nbytes)
        # the buffer goes back to torch's allocator when the import has read it
        buf.record_stream(dst_stream)
        return meta

    # -- stream bank: gated events against many references, per stream ------------
    def set_stream_bank(self, stream_word=None) -> None:
        """From the next push on, every gated event of stream s is scored on the device against
        the templates of word stream_word[s] of this engine's bank (set_bank / bank_from_pcm;
        None: word 0 for every stream) instead of the single template.  Events then carry the
        best score, the decision at the word's threshold and _lib.EWK_EV_BANK with the best
        template in their flags (_lib.event_best_template).  set_bank / bank_from_pcm /
        clear_bank raise ValueError until clear_stream_bank()."""
        wp = None
        if stream_word is not None:
            stream_word = np.ascontiguousarray(stream_word, dtype=np.int32).reshape(-1)
            if stream_word.size != self.n_streams:
                raise ValueError(f"{stream_word.size} word indices for {self.n_streams} streams")
            wp = _lib.i32ptr(stream_word)
        check(self._lib.ewk_stream_bank_enable(self._h, wp))

    def clear_stream_bank(self) -> None:
        """Back to the single template (no-op when the stream bank is off)."""
        check(self._lib.ewk_stream_bank_disable(self._h))

    def reenter(self, stream: int = -1, reentry_timeout: float = 0.0) -> None:
        """A new _detect_word call (wakeword.py:1048-1057) on `stream` (-1 = all) and the
        re-entry timeout for later pushes (0 = continuous, > 0 = start() mode)."""
        check(self._lib.ewk_reenter(self._h, int(stream), float(reentry_timeout)))
        self.config.reentry_timeout = float(reentry_timeout)
