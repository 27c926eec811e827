"""Shared by the float32 scorer matrix tests (tests/test_scorer_matrix.py on the CPU,
tests/test_gpu_scorer_matrix.py on the GPU): inputs that reach the index maps of k_score_f32
(csrc/ewk_mfcc.hip) one at a time, their oracle statistics (computed once), the yardsticks, a
staged replay of the oracle and the mutants -- small wrong versions of one stage each -- that the
CPU test runs to show the inputs would notice the mistakes they are built for.  Nothing here touches
a GPU or imports the product.

Every segment is float32, seeded with PCG64 by its case, and short: L = (T - 1) * 160 + rem samples
give T = 1 + L // 160 frames.

  tone probe (k, T, rem, amp)   amp * g[n // 160] * cos(2 pi k n / 512 + 0.3) + N(0, 1e-4 * amp / 0.5):
                    all the energy in FFT bin k; g is a per-hop gain drawn from [-30, 0] dB, so the
                    frames differ (a large std, well-conditioned statistics) and the noise floor lies
                    under max - 80 dB in most bands (the top_db clamp and its shift are active)
  click probe (T, rem)   N(0, 1e-4) plus one click per 160-sample hop, amplitude 0.05 ... 0.9 of either
                    sign at a random place in the hop: a flat spectrum whose level per frame depends
                    on where the Hann window meets the clicks -- a frame read from the wrong samples
                    changes it

  A  spectral sweep   tone probes k = 0 ... 256 at T = 17, rem = 37: the FFT's index maps, both untangle
                      lane classes, every mel band's weights and read window, every tile chunk slot
  B  frame grid       tone probes k = 5, 128, 250 and click probes at T = 1 ... 40, 47, 48, 49 with
                      rem = 0, 1, 159, and tone probes k = 128 at T = 767 ... 770: every remainder of the
                      8-frame pass and the 16-frame tile, a lane's unpaired second frame, one / two /
                      three tiles, the 48-tile record edge, the right pad at every alignment
  C  amplitude        tone probes k = 5, 128, 250 at T = 17, amp = 5e-4, 0.5, 15: the f16 hi / lo split of
                      the log-mel tile over its value range
  D  pad and placement   24 cases of B (T = 1, 2, 9, 17, tone k = 128 and clicks, every rem) inside a loud
                      filler at chosen base alignments, and windows of one buffer that overlap by 300
                      samples: the buffer descriptor's range check on both ends
  E  batch position   A + B + C in one batch, 32 of them alone and again behind 2,100 short segments:
                      first claim by grid index against counter claims, batch independence

Ring modes (MODE 1 and MODE 2) are out of scope: they expose no statistics read-back, and adding one
would change the ABI.  They share frame_pass with MODE 0, so families A to C cover their transform;
their own parts -- the wrap in stage_load, int16 loads, segment_stats_coop -- stay with the
streaming tests.

Frame permutations are deliberately absent from the mutants: mean and std cannot see them, and a
kernel that permutes frames is not wrong.
"""
import functools

import numpy as np
import scipy.fft

import synth
import template_cases as tc
from oracle import mfcc_ref

HOP = mfcc_ref.HOP
N_FFT = mfcc_ref.N_FFT
BAR = tc.BAR                  # 1e-4: a score, or what an error in the statistics moves one by
SPREAD_CAP = tc.SPREAD_CAP    # 1e-5: what the oracle's own float32 arithmetic may leave open
THRESHOLD = tc.THRESHOLD
RTOL, ATOL = 1e-4, 2e-3       # the suite's per-coefficient bar on float32 mean / std
MIN_STD, MIN_MEAN = 20.0, 32.0   # below either the fp64 re-score decides
SHORT_T = 16                  # T <= 16: re-scored whatever the statistics
CAUGHT = 10.0                 # a mutant is caught where it leaves the bar by this factor

A_T, A_REM = 17, 37
B_K = (5, 128, 250)
B_T = tuple(range(1, 41)) + (47, 48, 49)
B_REM = (0, 1, 159)
LONG_T = (767, 768, 769, 770)      # kSpecTiles = 48 tiles of 16 frames: the record's edge
LONG_K, LONG_REM = 128, 37
C_AMP = (5e-4, 0.5, 15.0)
D_T = (1, 2, 9, 17)
D_K = 128
D_GAP = 700
D_MOD64 = (0, 1, 2, 3, 31, 63, 5, 17, 33, 47, 59, 21)   # base offsets mod 64, cycled over the 24 cases
D_OVERLAP = 300
D_SHORT_STEP = 37          # an odd step for the windows too short to overlap by D_OVERLAP
E_SAMPLE = 32
E_PAD_N, E_PAD_LEN = 2100, 161


def _rng(*key):
    return np.random.Generator(np.random.PCG64([int(k) for k in key]))


def seg_len(T, rem):
    return (T - 1) * HOP + rem


def tone_probe(k, T, rem, amp=0.5, seed=()):
    L = seg_len(T, rem)
    rng = _rng(1, k, T, rem, *seed)
    g = 10.0 ** (rng.uniform(-30.0, 0.0, T + 1) / 20.0)
    n = np.arange(L)
    x = amp * g[n // HOP] * np.cos(2.0 * np.pi * k * n / N_FFT + 0.3)
    x += rng.normal(0.0, 1e-4 * amp / 0.5, L)
    return x.astype(np.float32)


def click_probe(T, rem, seed=()):
    L = seg_len(T, rem)
    rng = _rng(2, T, rem, *seed)
    x = rng.normal(0.0, 1e-4, L)
    hops = T + 1
    pos = np.arange(hops) * HOP + rng.integers(0, HOP, hops)
    a = rng.uniform(0.05, 0.9, hops) * rng.choice([-1.0, 1.0], hops)
    keep = pos < L
    x[pos[keep]] += a[keep]
    return x.astype(np.float32)


class Case:
    def __init__(self, name, family, kind, T, rem, x, k=None, amp=None):
        self.name, self.family, self.kind, self.T, self.rem, self.k, self.amp = name, family, kind, T, rem, k, amp
        self.x = np.ascontiguousarray(x, dtype=np.float32)
        self.x.setflags(write=False)

    def __repr__(self):
        return self.name


def _build():
    out = []
    for k in range(257):
        out.append(Case(f"A_k{k}", "A", "tone", A_T, A_REM, tone_probe(k, A_T, A_REM, seed=(10,)), k=k, amp=0.5))
    for T in B_T:
        for rem in B_REM:
            for k in B_K:
                out.append(Case(f"B_tone{k}_T{T}_r{rem}", "B", "tone", T, rem, tone_probe(k, T, rem), k=k, amp=0.5))
            out.append(Case(f"B_click_T{T}_r{rem}", "B", "click", T, rem, click_probe(T, rem)))
    for T in LONG_T:
        out.append(Case(f"B_long_T{T}", "B", "tone", T, LONG_REM, tone_probe(LONG_K, T, LONG_REM), k=LONG_K, amp=0.5))
    for k in B_K:
        for i, amp in enumerate(C_AMP):
            out.append(Case(f"C_k{k}_a{amp:g}", "C", "tone", A_T, A_REM, tone_probe(k, A_T, A_REM, amp, seed=(30, i)),
                            k=k, amp=amp))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def cases():
    """Families A, B and C: every case once, in a fixed order."""
    return _build()


def by_family(*families):
    return [c for c in cases() if c.family in families]


def case(name):
    return _by_name()[name]


@functools.lru_cache(maxsize=None)
def _by_name():
    return {c.name: c for c in cases()}


# ---- the oracle, once ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def template():
    """The word's oracle template, float32 (as Engine.set_template keeps it)."""
    tm, ts = mfcc_ref.extract_mfcc(synth.load_word().astype(np.float32))
    return tm.astype(np.float32), ts.astype(np.float32)


def stats_of(x, dtype=np.float64):
    """Oracle (mean, std) of float32 samples in `dtype` arithmetic, read-only."""
    with np.errstate(all="ignore"):
        m, s = mfcc_ref.extract_mfcc(np.asarray(x, np.float32).astype(dtype))
    m, s = np.asarray(m), np.asarray(s)
    m.setflags(write=False)
    s.setflags(write=False)
    return m, s


_stats = {}


def oracle(c, dtype="float64"):
    """Oracle (mean, std) of a case (computed once, shared, read-only)."""
    key = (c.name, dtype)
    if key not in _stats:
        _stats[key] = stats_of(c.x, np.dtype(dtype))
    return _stats[key]


def score_of(stats, tmpl=None):
    """The reference's score of (mean, std) against a template (default: the word's)."""
    tm, ts = tmpl or template()
    with np.errstate(all="ignore"):
        return float(mfcc_ref.similarity_from_stats(tm, ts, stats[0], stats[1]))


def oracle_score(c):
    key = (c.name, "score")
    if key not in _stats:
        _stats[key] = score_of(oracle(c))
    return _stats[key]


# ---- yardsticks --------------------------------------------------------------------------------
def drift(a, b):
    """template_cases.template_drift over candidate_stats(): how far the difference between two
    (mean, std) pairs moves a score when they serve as templates."""
    with np.errstate(all="ignore"):
        return tc.template_drift(a, b, tc.candidate_stats())


def coeff_excess(got, ref):
    """max over the 40 coefficients of |got - ref| / (ATOL + RTOL |ref|): <= 1 inside the suite's
    per-coefficient bar.  A NaN counts as infinitely far."""
    worst = 0.0
    for g, r in zip(got, ref):
        with np.errstate(all="ignore"):
            e = np.abs(np.asarray(g, np.float64) - r) / (ATOL + RTOL * np.abs(r))
        worst = max(worst, float(np.where(np.isnan(e), np.inf, e).max()))
    return worst


def excess(got, ref, T):
    """How many times over the bars that apply at T frames `got` is from `ref`: the per-coefficient
    bar at any T, and above SHORT_T frames also the drift in units of BAR (the larger of the two: the
    GPU test asserts both)."""
    e = coeff_excess(got, ref)
    if T > SHORT_T:
        e = max(e, drift(got, ref) / BAR)
    return e


def n_frames(x):
    return mfcc_ref.n_frames(len(x))


def norms(stats):
    return float(np.linalg.norm(stats[0])), float(np.linalg.norm(stats[1]))


# ---- the oracle in stages, and the mutants ------------------------------------------------------
def replay(x, dtype=np.float64, frames=None, power=None, weights=None, peak=None, bands=None):
    """mfcc_ref.extract_mfcc stage by stage: frames -> windowed rfft power -> mel -> dB + top_db ->
    DCT -> mean / std.  Each keyword replaces or edits one stage's result (a mutant)."""
    y = np.asarray(x, np.float32).astype(dtype)
    melw, win = mfcc_ref._tables()
    fr = mfcc_ref.frames(y)                                    # [T, 512]
    if frames is not None:
        fr = frames(fr.copy())
    spec = np.fft.rfft(win[None, :] * fr, axis=-1)
    cdt = np.complex64 if y.dtype == np.float32 else np.complex128
    P = np.abs(spec.astype(cdt).T) ** 2.0                      # [257, T]
    if power is not None:
        P = power(P.copy())
    W = melw if weights is None else weights(melw.copy())
    with np.errstate(all="ignore"):
        mel = np.einsum("...ft,mf->...mt", P, W, optimize=True)
        db = 10.0 * np.log10(np.maximum(mfcc_ref.AMIN, mel))
        db -= 10.0 * np.log10(np.maximum(mfcc_ref.AMIN, 1.0))
        top = db.max() if peak is None else peak(db)
        db = np.maximum(db, top - mfcc_ref.TOP_DB)
        if bands is not None:
            db = bands(db.copy())
        c = scipy.fft.dct(db, axis=-2, type=2, norm="ortho")[..., :mfcc_ref.N_MFCC, :]
        return np.mean(c, axis=1), np.std(c, axis=1)


def mut_bin_to_next(k):
    """Power of bin k lands in bin k + 1 (past bin 256: nowhere)."""
    def power(P):
        if k + 1 < P.shape[0]:
            P[k + 1] += P[k]
        P[k] = 0.0
        return P
    return dict(power=power)


def mut_band_row_shifted(m, by=1):
    """Band m's weight row one bin up (by = 1) or down (by = -1)."""
    def weights(W):
        W[m] = np.roll(W[m], by)
        return W
    return dict(weights=weights)


def mut_bands_swapped(m):
    """Bands m and m ^ 1 change places in the DCT's input."""
    def bands(db):
        db[[m, m ^ 1]] = db[[m ^ 1, m]]
        return db
    return dict(bands=bands)


def mut_last_frame_dropped():
    return dict(frames=lambda fr: fr[:-1])


def mut_last_frame_repeats():
    """Frame T - 1 computed as a copy of frame T - 2."""
    def frames(fr):
        fr[-1] = fr[-2]
        return fr
    return dict(frames=frames)


def mut_frame_rotated(f, by):
    """Frame f's 512 samples rotated by `by`."""
    def frames(fr):
        fr[f] = np.roll(fr[f], by)
        return fr
    return dict(frames=frames)


def mut_first_tile_peak():
    """The top_db clamp taken from the first tile's max, not the segment's."""
    return dict(peak=lambda db: db[:, :16].max())


def mut_pad_from_buffer(buf, off, n, side):
    """The zero padding of frame 0 (side "left") or of the last frame (side "right") of the segment
    buf[off:off + n] read from the buffer it lies in: what a missing range check would load."""
    def frames(fr):
        f = 0 if side == "left" else fr.shape[0] - 1
        j = f * HOP + np.arange(N_FFT) - N_FFT // 2     # frame f's sample indices inside the segment
        out = j < 0 if side == "left" else j >= n
        fr[f, out] = buf[off + j[out]]
        return fr
    return dict(frames=frames)


def zero_weight_bins():
    """FFT bins no mel band weighs, from the oracle's filterbank."""
    W = mfcc_ref.mel_filterbank()
    return [k for k in range(W.shape[1]) if not W[:, k].any()]


def bins_without_leverage():
    """Bins whose move to k + 1 changes no band: column k of the oracle's filterbank equals column
    k + 1 (the column past 256 counting as zero).  A zero column next to a weighted one is not
    among them: bin 0's power arriving in bin 1 is seen by band 0."""
    W = mfcc_ref.mel_filterbank()
    W = np.concatenate([W, np.zeros((W.shape[0], 1), W.dtype)], axis=1)
    return [k for k in range(W.shape[1] - 1) if np.array_equal(W[:, k], W[:, k + 1])]


def band_peak_bins():
    W = mfcc_ref.mel_filterbank()
    return [int(np.argmax(W[m])) for m in range(W.shape[0])]


def band_support(m):
    """The bins band m weighs, and one more on either side (where a shifted row has weight)."""
    k = np.flatnonzero(mfcc_ref.mel_filterbank()[m])
    return list(range(max(int(k[0]) - 1, 0), min(int(k[-1]) + 1, N_FFT // 2) + 1))


# ---- family D: placement --------------------------------------------------------------------------
def d_cases():
    """The 24 cases of family B that family D places."""
    out = []
    for T in D_T:
        for rem in B_REM:
            out.append(case(f"B_tone{D_K}_T{T}_r{rem}"))
            out.append(case(f"B_click_T{T}_r{rem}"))
    return out


def filler(n, seed=40):
    """A 0.9-amplitude sine plus noise: what a read past a segment's ends would find."""
    rng = _rng(seed)
    t = np.arange(n)
    return (0.9 * np.sin(2.0 * np.pi * 0.0371 * t + 1.0) + rng.normal(0.0, 0.02, n)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def d_spaced_layout():
    """(buffer, offsets, lengths): the D cases with at least D_GAP samples of filler between and
    around them, segment i starting at an offset congruent to D_MOD64[i % 12] mod 64."""
    cs = d_cases()
    offs, pos = [], 0
    for i, c in enumerate(cs):
        o = pos + D_GAP
        o += (D_MOD64[i % len(D_MOD64)] - o) % 64
        offs.append(o)
        pos = o + len(c.x)
    buf = filler(pos + D_GAP + 64)
    for o, c in zip(offs, cs):
        buf[o:o + len(c.x)] = c.x
    buf.setflags(write=False)
    return buf, np.array(offs, np.int64), np.array([len(c.x) for c in cs], np.int32)


@functools.lru_cache(maxsize=None)
def d_overlap_layout():
    """(buffer, offsets, lengths): windows of the D cases' lengths over one buffer, the longest
    first.  The cases are written in order, each D_OVERLAP samples before the previous one ends, or
    D_SHORT_STEP samples after its start where it is no longer than that (T <= 2): a window keeps
    the head of its own case and ends in the heads of the cases that follow.  The T = 9 and T = 17
    windows share exactly D_OVERLAP samples with the next one, a T = 2 window all but D_SHORT_STEP,
    and the T = 1 windows (0, 1 and 159 samples) lie D_SHORT_STEP apart; but for the two empty ones,
    no two windows hold the same samples."""
    cs = sorted(d_cases(), key=lambda c: -c.T)
    offs, pos = [], D_GAP + 1
    for c in cs:
        offs.append(pos)
        pos += max(len(c.x) - D_OVERLAP, D_SHORT_STEP)
    buf = filler(max(o + len(c.x) for o, c in zip(offs, cs)) + D_GAP, seed=41)
    for o, c in zip(offs, cs):
        buf[o:o + len(c.x)] = c.x
    buf.setflags(write=False)
    return buf, np.array(offs, np.int64), np.array([len(c.x) for c in cs], np.int32)


def windows(layout):
    buf, offs, lens = layout
    return [buf[o:o + n] for o, n in zip(offs.tolist(), lens.tolist())]


# ---- family E: batch position ---------------------------------------------------------------------
def e_sample():
    """Indices into cases() of the 32 segments scored again alone and behind the padding: the four
    long ones, and a seeded draw of the rest."""
    cs = cases()
    long_ = [i for i, c in enumerate(cs) if c.name.startswith("B_long")]
    rest = [i for i in range(len(cs)) if i not in long_]
    pick = _rng(50).choice(rest, E_SAMPLE - len(long_), replace=False)
    return sorted(long_ + [int(i) for i in pick])


def e_pad_segment():
    return click_probe(2, 1, seed=(51,))
