"""The level-3 front end's yardstick, matrix and mutants (tests/test_whisper_frontend.py on the
CPU, tests/test_gpu_whisper_frontend.py on the GPU).

``features_ref`` is a float64 numpy restatement of the semantics in include/ewk.h
(ewk_whisper_features_*): the float32 of the normalised segment, zero-extended or truncated to
n_frames * 160 samples, reflect-padded by 200, 400-point periodic-Hann frames at hop 160, power
of the 201 rfft bins, the float32 Slaney filterbank, log10 clamped at 1e-10, the max - 8 floor and
(L + 4) / 4.  At 3000 frames it is held to transformers' float64
``WhisperFeatureExtractor._np_extract_fbank_features`` (``yardstick``), which does not come from
this project.  Inputs of the matrix are *normalised* segments (float64, as ewk_normalize_* give
them) next to the raw float32 segments they come from.
"""
from __future__ import annotations

import functools

import numpy as np

HOP, N_FFT, N_MELS = 160, 400, 80
YARDSTICK_BOUND = 2e-7     # the yardstick's own float32 output rounding
BAR_CAP = 2.0 ** -10       # a quarter of a bf16 ulp at 0.5..1


def normalize_level3(x):
    """wakeword.py:1019-1025 on the float64 segment (what k_normalize computes bit for bit)."""
    a = np.asarray(x, dtype=np.float64)
    if a.size == 0:
        return a
    a = a - np.mean(a)
    m = np.max(np.abs(a))
    if m > 0:
        a = a / m
    return np.clip(a * 1.5, -1.0, 1.0)


@functools.lru_cache(maxsize=None)
def mel_filters() -> np.ndarray:
    from easywakeword_amd.confirm import _slaney_mel
    return _slaney_mel(16000, N_FFT, N_MELS)


MUTANTS = ("zero_start_pad", "no_end_reflection", "symmetric_hann", "power_next_bin", "mel_row_shift",
           "bands_swapped", "last_live_dropped", "clamp_frame0", "dead_minus_1p5")


def n_live_frames(length: int, n_frames: int) -> int:
    """Frames that read at least one sample of the segment: t with 160 t - 200 < min(length, n)."""
    lc = min(int(length), n_frames * HOP)
    return 0 if lc <= 0 else min(n_frames, (lc + 199) // HOP + 1)


def features_ref(y, n_frames: int = 3000, mutant: str = None) -> np.ndarray:
    """[80, n_frames] float64 features of one normalised segment (`mutant`: a named defect)."""
    assert mutant is None or mutant in MUTANTS
    y32 = np.asarray(y, np.float64).astype(np.float32)
    n = n_frames * HOP
    x = np.zeros(n, np.float32)
    m = min(len(y32), n)
    x[:m] = y32[:m]
    xp = np.pad(x.astype(np.float64), N_FFT // 2, mode="reflect")
    if mutant == "zero_start_pad":
        xp[:N_FFT // 2] = 0.0
    if mutant == "no_end_reflection":
        xp[n + N_FFT // 2:] = 0.0
    i = np.arange(N_FFT)
    win = 0.5 - 0.5 * np.cos(2 * np.pi * i / (N_FFT - 1 if mutant == "symmetric_hann" else N_FFT))
    frames = np.lib.stride_tricks.sliding_window_view(xp, N_FFT)[::HOP][:n_frames]
    power = np.abs(np.fft.rfft(frames * win, axis=1)) ** 2            # [n_frames, 201]
    if mutant == "power_next_bin":
        power = np.roll(power, 1, axis=1)
    mel = mel_filters().astype(np.float64)
    if mutant == "mel_row_shift":
        mel = np.roll(mel, 1, axis=1)
    L = np.log10(np.maximum(mel @ power.T, 1e-10))                    # [80, n_frames]
    if mutant == "bands_swapped":
        L = L[np.arange(N_MELS) ^ 1]
    live = n_live_frames(len(y32), n_frames)
    if mutant == "last_live_dropped" and live > 0:
        L[:, live - 1] = -10.0
    top = L[:, 0].max() if mutant == "clamp_frame0" else L.max()
    out = (np.maximum(L, top - 8.0) + 4.0) / 4.0
    if mutant == "dead_minus_1p5":
        out[:, live:] = -1.5
    return out


@functools.lru_cache(maxsize=None)
def _extractor():
    from transformers import WhisperFeatureExtractor
    return WhisperFeatureExtractor()


def yardstick(y) -> np.ndarray:
    """transformers' numpy front end on the float32 of a normalised segment: [80, 3000] float64."""
    y32 = np.asarray(y, np.float64).astype(np.float32)
    x = np.zeros(3000 * HOP, np.float32)
    m = min(len(y32), len(x))
    x[:m] = y32[:m]
    return np.asarray(_extractor()._np_extract_fbank_features(x[None], "cpu")[0], np.float64)


def torch_front_end(ys, n_frames: int = 3000) -> np.ndarray:
    """The parent's float32 front end (WhisperConfirm.log_mel's arithmetic, on the CPU) at
    n_frames frames: [len(ys), 80, n_frames] float64.  Its worst error against features_ref over
    the matrix is E of the bar."""
    import torch
    n = n_frames * HOP
    x = torch.zeros((len(ys), n), dtype=torch.float32)
    for i, a in enumerate(ys):
        a = torch.as_tensor(np.asarray(a, np.float64).astype(np.float32)[:n])
        x[i, :a.numel()] = a
    spec = torch.stft(x, N_FFT, HOP, window=torch.hann_window(N_FFT), return_complex=True)
    power = spec[..., :-1].abs() ** 2
    log_spec = torch.clamp(torch.from_numpy(mel_filters()) @ power, min=1e-10).log10()
    log_spec = torch.maximum(log_spec, log_spec.amax(dim=(1, 2), keepdim=True) - 8.0)
    return ((log_spec + 4.0) / 4.0).double().numpy()


# ---------------------------------------------------------------- the matrix
class Case:
    def __init__(self, family: str, name: str, raw: np.ndarray, n_frames: int):
        self.family, self.name, self.n_frames = family, name, n_frames
        self.raw = np.ascontiguousarray(raw, np.float32)       # what the engine is given
        self.y = normalize_level3(self.raw)                    # what the front end sees

    def __repr__(self):
        return f"{self.family}:{self.name}"


def tone_case(k: int) -> np.ndarray:
    """(A) bin k: sin(2 pi k i / 400 + 0.3) over 800 samples, 6 dB down every 160, + 1e-3 noise."""
    rng = np.random.default_rng(1)
    i = np.arange(800)
    x = np.sin(2 * np.pi * k * i / 400 + 0.3) * 0.5 ** (i // 160) + 1e-3 * rng.standard_normal(800)
    return x.astype(np.float32)


NOISE_LENGTHS = (2, 120, 121, 159, 160, 161, 199, 200, 201, 399, 400, 401, 1079, 1080, 1081, 1280, 2000)


def noise_case(n: int) -> np.ndarray:
    rng = np.random.default_rng(1000 + n)
    return (0.1 * rng.standard_normal(n)).astype(np.float32)


def quiet_then_loud() -> np.ndarray:
    """(B, added) 920 samples, quiet but for a burst in the last 40: frame 6, the last live one,
    windows the burst at 0.65-0.90 and frame 5 at 0.65-0.35, so the maximum log-mel is in frame 6."""
    rng = np.random.default_rng(77)
    x = 1e-3 * rng.standard_normal(920)
    x[880:] += 0.5 * np.sin(2 * np.pi * 37 * np.arange(40) / 400)
    return x.astype(np.float32)


def long_case(n: int) -> np.ndarray:
    rng = np.random.default_rng(2000 + n)
    i = np.arange(n)
    x = 0.2 * np.sin(2 * np.pi * 440 * i / 16000) * (1 + 0.5 * np.sin(2 * np.pi * 3 * i / 16000))
    return (x + 0.02 * rng.standard_normal(n)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def matrix():
    cases = [Case("A", f"tone{k}", tone_case(k), 8) for k in range(201)]
    cases += [Case("B", f"noise{n}", noise_case(n), 8) for n in NOISE_LENGTHS]
    cases.append(Case("B", "quiet_then_loud", quiet_then_loud(), 8))
    cases += [Case("C", f"len{n}", long_case(n), 3000) for n in (1, 6400, 48800)]
    cases.append(Case("C", "zeros", np.zeros(3200, np.float32), 3000))
    nan = long_case(4000)
    nan[1234] = np.nan
    cases.append(Case("C", "nan", nan, 3000))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def references():
    """features_ref of every case of the matrix, computed once and shared (read-only)."""
    out = []
    for c in matrix():
        r = features_ref(c.y, c.n_frames)
        r.setflags(write=False)
        out.append(r)
    return tuple(out)


def max_err(got, want) -> float:
    """Worst absolute difference; NaN must sit exactly where the reference has it (else inf)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return float("inf")
    d = np.abs(got - want)
    d = d[~np.isnan(d)]
    return float(d.max()) if d.size else 0.0


@functools.lru_cache(maxsize=None)
def parent_error():
    """E of the bar, per family and overall: the worst error of the parent's float32 front end
    (torch_front_end) over the matrix against features_ref."""
    per = {}
    cases, refs = matrix(), references()
    for fam, nf in (("A", 8), ("B", 8), ("C", 3000)):
        idx = [i for i, c in enumerate(cases) if c.family == fam]
        got = torch_front_end([cases[i].y for i in idx], nf)
        per[fam] = max(max_err(got[j], refs[i]) for j, i in enumerate(idx))
    per["all"] = max(per.values())
    return per


def bar() -> float:
    """Every float32 element within min(4 E, 2^-10) of the yardstick."""
    return min(4.0 * parent_error()["all"], BAR_CAP)


def bf16_round(a: np.ndarray) -> np.ndarray:
    """float32 -> bf16 bits (uint16), round to nearest even; NaN -> 0x7FC0."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    r[np.isnan(a)] = 0x7FC0
    return r
