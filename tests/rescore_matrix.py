"""Shared by the re-score matrix tests (tests/test_rescore_matrix.py on the CPU,
tests/test_gpu_rescore_matrix.py on the GPU): the inputs that drive the fp64 re-score
(csrc/ewk_rescore.h) through every chunk shape and drain path, the facts a numpy replay
(scripts/f64_chunk_model.py) shows of each, and the oracle's float64 statistics and scores.

Every input is deterministic float32.  A case names the path it is meant for (`path`) and carries
a `check` that asserts, from the oracle and the replay alone, that the input reaches it:

  a  chunk grid     T = 1, 2, 3, 7, 8, 9, 15, 16, 17, 18: a single chunk of n = 1, one partial chunk
                    that is also the merge's reference frame, a last chunk of n = 1, 2, 3, 7, 8
  b  dummy frame    odd last n: the frame past the segment's end rides through rs_frames with
                    valid[j] = false, and here it is the loudest frame of all
  c  64-chunk rounds  64, 65 and 129 chunks; the max, or the only ambiguous chunk, in a late round
                    of rs_finish's `c0 += 64` loop
  d  clamp structure  no clamped value (need_b false), chunks clamped entirely (chunk 0 among
                    them: rA0 = 0), digital silence, a partly clamped chunk 0, all zeros
  e  redo_all       theta_s (float32, overflowed) is not within kRsWindow of theta
  f  non-finite     a NaN / Inf sample on the fp64 path itself

The carrier is non-stationary (a chirp under a ~7 Hz envelope plus 30 % noise), so the std vectors
of short segments are well conditioned.
"""
import os
import sys

import numpy as np

import synth
from oracle import mfcc_ref

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "scripts"))
import f64_chunk_model as fm  # noqa: E402

SR = 16000
W = 2e-4                 # kRsWindow (ewk_rescore.h)
THETA_S_OFFSET = 1e-5    # the replay's theta_s - theta: the float32 pass's measured error is <= 2e-5 dB
GRID_L = (1, 2, 159, 160, 161, 319, 320, 1119, 1120, 1121, 1279, 1280, 1281, 2399, 2400, 2559, 2560, 2561, 2719, 2720)
DUMMY_K = (0, 2, 24, 26, 28, 30)
FLAG_DELTAS = (0.0, 3e-6, -3e-6, 1.5e-4)
LONG = 163840
# the only cases whose oracle score is NaN: T = 1 (zero std) and e (negative similarity)
NAN_SCORE = ("a_L1", "a_L2", "a_L159", "b_k0", "e_huge")


def carrier(L, seed, amp=0.2):
    rng = np.random.default_rng(seed)
    t = np.arange(L) / SR
    env = 0.15 + np.abs(np.sin(2 * np.pi * 7.3 * t + seed))
    return amp * env * (np.sin(2 * np.pi * (300 + 40 * seed) * t + 900 * t * t) + 0.3 * rng.standard_normal(L))


def _tone(L, f, a, s0, s1):
    y = np.zeros(L)
    t = np.arange(s1 - s0) / SR
    y[s0:s1] = a * np.sin(2 * np.pi * f * t) * np.hanning(s1 - s0)
    return y


def raw_log_mel(y):
    """oracle float64 log-mel [128, T] before the top_db clamp."""
    mel_basis, _ = mfcc_ref._tables()
    S = mfcc_ref.power_spectrogram(np.asarray(y, np.float64))
    return 10.0 * np.log10(np.maximum(mfcc_ref.AMIN, np.einsum("ft,mf->mt", S, mel_basis)))


class Case:
    def __init__(self, name, family, path, x, check, oracle=True, expect=None):
        self.name, self.family, self.path = name, family, path
        self.x = np.ascontiguousarray(x, dtype=np.float32)
        self.check = check
        self.oracle = oracle      # compared with oracle/mfcc_ref.py (False: d-v and f)
        self.expect = expect      # "zero_std" (d-v) or "nan" (f) where it is not
        self.T = 1 + len(self.x) // 160
        self.n_chunks = -(-self.T // 8)
        self.last_n = self.T % 8 or 8


# ---- what the oracle and the replay show of a case (computed once) ----------------------------
_facts = {}


def template():
    """The word's oracle template, float32 (as Engine.set_template keeps it)."""
    if "template" not in _facts:
        tm, ts = mfcc_ref.extract_mfcc(synth.load_word().astype(np.float32))
        _facts["template"] = (tm.astype(np.float32), ts.astype(np.float32))
    return _facts["template"]


def oracle(case):
    """(mean, std, score) of the reference's float64 path."""
    key = ("oracle", case.name)
    if key not in _facts:
        tm, ts = template()
        with np.errstate(all="ignore"):
            cm, cs = mfcc_ref.extract_mfcc(case.x.astype(np.float64))
            s = float(mfcc_ref.similarity_from_stats(tm, ts, cm, cs))
        for a in (cm, cs):
            a.setflags(write=False)
        _facts[key] = (cm, cs, s)
    return _facts[key]


def replay(case, theta_s=None):
    """model_stats of a case at theta_s (default: the exact theta + THETA_S_OFFSET)."""
    key = ("replay", case.name, theta_s)
    if key not in _facts:
        x = case.x.astype(np.float64)
        th = theta_s
        if th is None:
            th = float(raw_log_mel(x).max()) - 80.0 + THETA_S_OFFSET
        _facts[key] = fm.model_stats(x, th, W=W)
    return _facts[key]


def replay_error(case):
    """(|dmean| / scale, |dstd| / scale, |dscore|) of the replay against the oracle."""
    cm, cs, s = oracle(case)
    m, sd, _, _ = replay(case)
    tm, ts = template()
    with np.errstate(all="ignore"):
        s2 = float(mfcc_ref.similarity_from_stats(tm, ts, m, sd))
    scale = max(1.0, float(np.abs(cm).max()))
    ds = 0.0 if (np.isnan(s) and np.isnan(s2)) else abs(s - s2)
    return float(np.abs(m - cm).max()) / scale, float(np.abs(sd - cs).max()) / scale, ds


# ---- the checks ------------------------------------------------------------------------------
def _check_grid(T, last_n):
    def check(c):
        assert (c.T, c.last_n, c.n_chunks) == (T, last_n, -(-T // 8))
        _, cs, s = oracle(c)
        if T > 1:
            assert np.linalg.norm(cs) > 1.0 and np.isfinite(s)    # a conditioned std vector
    return check


def _check_dummy(c):
    melw, win = mfcc_ref._tables()
    x = c.x.astype(np.float64)
    assert c.T % 2 == 1 and c.last_n in (1, 3, 5, 7)
    valid = fm.frame_logmel(x, np.arange(c.T), win, melw)
    dummy = fm.frame_logmel(x, c.T, win, melw)        # the frame past the end
    assert dummy.max() > valid.max() + 1.0, (dummy.max(), valid.max())
    if c.T >= 25:
        # entries a theta taken from the dummy would move: after the clamp at the valid theta they
        # lie between the two thetas
        moved = int((valid < dummy.max() - 80.0).sum())
        assert moved >= 20, moved


def _check_rounds(n_chunks):
    def check(c):
        assert c.n_chunks == n_chunks
        info = replay(c)[3]
        assert len(info["clamp_frac"]) == n_chunks
    return check


def _check_late_max(c):
    info = replay(c)[3]
    assert info["max_chunk"] >= 64, info["max_chunk"]
    lm, th = info["lm"], info["theta"]
    assert int(((lm > th - 25.0) & (lm < th)).sum()) >= 1000
    # the loudest value of the first 64 chunks (one round of the maxima loop) is far under theta + 80
    assert lm[:512].max() < th


def _check_late_flag(c):
    info = replay(c)[3]
    assert len(info["ambiguous"]) == 1 and 64 <= info["ambiguous"][0] < 128, info["ambiguous"]
    assert info["recomputed"] == info["ambiguous"] and info["max_chunk"] >= 64


def _check_no_clamp(c):
    info = replay(c)[3]
    assert info["lm"].min() > info["theta"] + W + THETA_S_OFFSET
    assert not info["clamp_frac"].any()


def _check_clamped_chunks(c):
    f = replay(c)[3]["clamp_frac"]
    assert int((f == 1.0).sum()) >= 10 and f[0] == 1.0 and int((f == 0.0).sum()) >= 1, f


def _check_lead_silence(c):
    info = replay(c)[3]
    assert 0.0 < info["clamp_frac"][0] < 1.0
    assert (info["lm"][0] < info["theta"]).all()       # chunk 0's first frame (the merge's reference): all clamped


def _check_zeros(c):
    assert not c.x.any() and not c.oracle
    assert np.ptp(mfcc_ref.log_mel(c.x.astype(np.float64))) == 0.0


def _check_redo_all(c):
    cm, cs, s = oracle(c)
    assert np.isfinite(cm).all() and np.isfinite(cs).all() and np.isnan(s)
    with np.errstate(all="ignore"):
        X = np.abs(np.fft.rfft(mfcc_ref.frames(c.x.astype(np.float64)) * mfcc_ref.hann_window(), axis=-1))
        assert np.float32(X.max()) ** 2 == np.inf      # the float32 power overflows: theta_s is not finite
    # the replay of redo_all itself: theta_s = inf recomputes every chunk and lands on the oracle
    m, sd, rc, info = replay(c, float("inf"))
    assert info["redo_all"] and rc == c.n_chunks
    scale = max(1.0, float(np.abs(cm).max()))
    assert np.abs(m - cm).max() <= 1e-11 * scale and np.abs(sd - cs).max() <= 1e-11 * scale


def _check_non_finite(c):
    bad = np.flatnonzero(~np.isfinite(c.x))
    assert len(bad) == 1 and not c.oracle
    chunk = int(bad[0]) // 160 // 8
    assert 0 < chunk < c.n_chunks - 1                  # a middle chunk


# ---- the inputs ------------------------------------------------------------------------------
def _dummy_input(k):
    L = 160 * k + 159
    rng = np.random.default_rng(k)
    t = np.arange(L) / SR
    y = 0.05 * (0.2 + np.abs(np.sin(2 * np.pi * 5 * t))) * np.sin(2 * np.pi * 700 * t + 400 * t * t)
    y += 1e-3 * rng.standard_normal(L)
    y[-80:] += 0.8 * np.sin(2 * np.pi * 1500 * np.arange(80) / SR)
    return y


def _late_max_input():
    """A loud burst in chunks >= 100 only; before and after it noise whose level wanders by
    +-5 dB around 102 dB below the burst's loudest band (the median entry; a band's spread from
    frame to frame puts the loudest about 85 dB below it): every entry under theta, most of them
    above theta - 25 dB."""
    rng = np.random.default_rng(64)
    L = LONG
    burst = np.zeros(L)
    burst[132000:150000] = carrier(18000, 3, 0.5)
    M = raw_log_mel(burst).max()
    t = np.arange(L) / SR
    noise = rng.standard_normal(L) * 10 ** (0.25 * np.sin(2 * np.pi * 0.9 * t))        # +-5 dB
    noise[131000:151000] = 0.0
    n0 = np.median(raw_log_mel(noise[:60000]))
    return burst + noise * 10 ** ((M - 102.0 - n0) / 20.0)


def _late_flag_input(delta):
    """test_gpu_rescore_window.py's recipe at 129 chunks: the quiet tone's peak band at
    M - 80 + delta in chunk 70, the loud tone in chunk 100, exact zeros elsewhere."""
    L = LONG
    loud = _tone(L, 900.0, 0.6, 128060, 129060)
    quiet1 = _tone(L, 3300.0, 1.0, 89560, 90760)
    M = raw_log_mel(loud).max()
    b0 = raw_log_mel(quiet1).max()
    return loud + quiet1 * 10 ** ((M - 80.0 + delta - b0) / 20.0)


def _build():
    cases = []

    def add(*a, **k):
        cases.append(Case(*a, **k))

    for L in GRID_L:
        T = 1 + L // 160
        add(f"a_L{L}", "a", f"T={T}, last n={T % 8 or 8}", carrier(L, L % 7), _check_grid(T, T % 8 or 8))
    for k in DUMMY_K:
        add(f"b_k{k}", "b", "the loudest frame is the dummy past the end", _dummy_input(k), _check_dummy)
    add("c_T512", "c", "64 chunks: one round", carrier(81919, 1), _check_rounds(64))
    add("c_T513", "c", "65 chunks: a second round of one", carrier(81920, 2), _check_rounds(65))
    add("c_T1025", "c", "129 chunks: three rounds", carrier(LONG, 3), _check_rounds(129))
    add("c_late_max", "c", "the max in round 2 or 3 only", _late_max_input(), _check_late_max)
    for i, d in enumerate(FLAG_DELTAS):
        add(f"c_late_flag{i}", "c", f"the only ambiguous chunk in round 2 (delta {d:g} dB)", _late_flag_input(d),
            _check_late_flag)
    rng = np.random.default_rng(1)
    L = 20000
    noclamp = carrier(L, 4) + 2e-3 * rng.standard_normal(L)
    add("d_no_clamp", "d", "need_b false in every chunk", noclamp, _check_no_clamp)
    y = 1e-7 * rng.standard_normal(L)
    y[9000:12000] += carrier(3000, 5, 0.5)
    add("d_noise_burst", "d", "chunks clamped entirely (chunk 0: rA0 = 0) and chunks not at all", y, _check_clamped_chunks)
    y = np.zeros(L)
    y[9000:12000] += carrier(3000, 6, 0.5)
    add("d_zeros_burst", "d", "the same over digital silence", y, _check_clamped_chunks)
    y = carrier(L, 7, 0.5)
    y[:600] = 0.0
    add("d_lead_silence", "d", "chunk 0 partly clamped from its first frame", y, _check_lead_silence)
    for n in (1600, 20000):
        add(f"d_zeros_L{n}", "d", "constant log-mel", np.zeros(n), _check_zeros, oracle=False, expect="zero_std")
    add("e_huge", "e", "redo_all", carrier(16000, 8, 1e18), _check_redo_all)
    for name, val in (("f_nan", np.nan), ("f_inf", np.inf)):
        y = noclamp.copy()
        y[10000] = val
        add(name, "f", "fl & 2", y, _check_non_finite, oracle=False, expect="nan")
    assert len({c.name for c in cases}) == len(cases)
    return cases


_cases = []


def cases():
    if not _cases:
        _cases.extend(_build())
    return _cases


def by_family(*families):
    return [c for c in cases() if c.family in families]


# the shaped cases: the ones whose result a wrong wave-to-chunk hand-off would move most
def shaped():
    return [c for c in cases() if c.family == "b" or c.name.startswith(("c_late", "d_noise_burst")) or c.family == "e"]


# ---- ring sources ----------------------------------------------------------------------------
RING_STREAMS = 10
RING_SEED = 4100               # tests/test_gpu_int16_ring.py's ten PCM16 streams
COMPACT_RING = 43200


def pcm16_streams():
    """[10, L] int16, a whole number of 1,600-sample ticks."""
    if "pcm16" not in _facts:
        rows = []
        for i in range(RING_STREAMS):
            rng = np.random.default_rng(RING_SEED + i)
            p, _ = synth.make_stream(seed=RING_SEED + 500 + i, n_words=4, sigma=float(rng.uniform(2e-4, 4e-3)),
                                     gain=float(rng.uniform(0.3, 2.5)), distractors=bool(i % 2))
            rows.append(p)
        L = min(len(p) for p in rows) // 1600 * 1600
        x = np.stack([p[:L] for p in rows])
        _facts["pcm16"] = np.clip(np.round(x.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)
    return _facts["pcm16"]


def ring_oracle_events():
    """Per stream, the oracle's events (default gate) of the PCM16 streams' float32 values."""
    if "ring_events" not in _facts:
        from oracle.gate_ref import GateConfig, run_stream
        x = pcm16_streams().astype(np.float32) / np.float32(32768.0)
        _facts["ring_events"] = [run_stream(x[i], GateConfig()).events for i in range(RING_STREAMS)]
    return _facts["ring_events"]


def straddles(tick, n_request, length, ring=COMPACT_RING, block=1600):
    """Does the segment cut at `tick` cross the physical end of a ring of `ring` samples?"""
    start = (tick * block - n_request) % ring
    return start + length > ring


# ---- pooled slots past the float32 pass's NaN --------------------------------------------------
# A segment whose float32 statistics are not finite is listed for the re-score only by its length
# (T <= 16 frames), and with the word's template a huge segment's score is NaN (negative
# similarity).  So that the part pool's redo_all and NaN-flag branches show in a score: segments of
# T = 15 and 16 (two chunks), scored against the statistics of another huge segment.
def huge_template():
    """Oracle statistics of a carrier at amplitude 1e18, float32: a template huge segments match."""
    if "huge_template" not in _facts:
        with np.errstate(all="ignore"):
            tm, ts = mfcc_ref.extract_mfcc(carrier(16000, 9, 1e18).astype(np.float32).astype(np.float64))
        _facts["huge_template"] = (tm.astype(np.float32), ts.astype(np.float32))
    return _facts["huge_template"]


def huge_score(case):
    """The oracle's float64 score of a case against huge_template()."""
    cm, cs, _ = oracle(case)
    with np.errstate(all="ignore"):
        return float(mfcc_ref.similarity_from_stats(*huge_template(), cm, cs))


def _check_short_redo_all(c):
    assert c.T <= 16 and c.n_chunks == 2
    _check_redo_all(c)
    assert np.isfinite(huge_score(c))


def _check_short_non_finite(c):
    bad = np.flatnonzero(~np.isfinite(c.x))
    assert c.T <= 16 and c.n_chunks == 2 and len(bad) == 1 and bad[0] // 160 // 8 == 1    # in chunk 1 only
    assert bad[0] >= 7 * 160 + 256             # past frame 7's last sample: no frame of chunk 0 sees it


_short = []


def short_cases():
    if not _short:
        for L in (2399, 2400):
            _short.append(Case(f"e_huge_L{L}", "e", "redo_all in the finishing wave of a pooled slot",
                               carrier(L, 8, 1e18), _check_short_redo_all))
        y = carrier(2400, 4)
        y[2300] = np.nan
        _short.append(Case("f_nan_L2400", "f", "fl & 2 from a part record", y, _check_short_non_finite,
                           oracle=False, expect="nan"))
    return _short
