"""The template-bank matrix (tests/test_bank_matrix.py, tests/test_gpu_bank_matrix.py): a numpy
restatement of the bank pass (csrc/ewk_bank.hip over csrc/ewk_score.h), the banks, batches and
word patterns that put it on every launch geometry, and the named defects the matrix must see.

Geometry of the pass: a segment takes G = 2^ceil(log2(largest word)) lanes, a wave scores
per = 64 / G segments per step and run = max(16, per) items per launch, lanes reload their
template only when their group's word changes, the best template comes from an xor-shuffle
reduction over the steps d < G (ties to the lowest lane), hit_mask is a ballot masked and
shifted per group.

Everything here is computed on the CPU from the oracle (oracle.mfcc_ref) alone:

  pool        the 68 distinct float32 templates of bank_cases.oracle_templates() and one more
              whose std vector is all zero (uu_s = 0: NaN against anything)
  segments    N_SEG ragged segments of 3200..8000 samples (>= 21 frames: the float32 pass can
              decide them) with two of at most 16 frames at SHORT_AT (always re-scored); they
              are the first of a seeded candidate list that are unambiguous against every word
              of every plain bank: top two scores at least MARGIN apart, so an argmax cannot
              depend on the 1e-4 by which the engine's statistics move a score (the special
              banks and the short segments are not selected for; test_bank_matrix.py asserts
              the same of every batch of the matrix, the tied lanes of a tie word aside)
  banks       one per largest-word size in SIZES (every G, at the power of two and one past the
              previous one): four words, one of a single template, word_first unaligned, and
              one special bank per G: tie words (one template at two or three lanes), NaN words
              (the zero-std template at lane 0, at the last lane, at the lane that would have
              been best, at every lane) and, at G = 64, the two hit-bit-63 words
  thresholds  per word, the midpoint of the widest gap between adjacent oracle scores in the
              middle half of the word's scores: both hit values occur, no score lies within
              MARGIN of it
"""
import functools
import math

import numpy as np

import bank_cases
import synth
from oracle import mfcc_ref

SIZES = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64)
EVENT_SIZES = (2, 5, 16, 32)
PATTERNS = ("constant", "cycle", "blocks", "random")
TIE_PAIRS = ((0, 1), (0, 2), (2, 3), (5, 13), (0, 32), (31, 32), (62, 63))
MARGIN = 1e-3
SEED = 4100
N_CAND = 900            # candidates the N_SEG segments are the first unambiguous ones of
N_SEG = 8 * 64 + 3      # the largest batch (G = 1: run = 64)
SHORT_AT = (1, 4)       # <= 16 frames: fp64 whatever the margin
GATE = dict(pre_speech_silence=0.8, speech_duration_min=0.3, speech_duration_max=2.0, post_speech_silence=0.4)
EVENT_STREAM_SEED = 4003
NAN_TMPL = 68           # pool index of the zero-std template
KTINY_STD = 20.0        # csrc/ewk_score.h kTinyStd
RESCORE_FRAMES = 16     # csrc/ewk_score.h kRescoreFrames


def geometry(max_word):
    """(G, per, run) of a bank whose largest word has max_word templates."""
    g = 1
    while g < max_word:
        g *= 2
    per = 64 // g
    return g, per, max(16, per)


def batch_sizes(max_word):
    """The batch sizes on every step, run and workgroup edge of the bank's geometry."""
    _, per, run = geometry(max_word)
    ns = [1, per - 1, per, per + 1, run - 1, run, run + 1, 4 * run - 1, 4 * run, 4 * run + 1, 8 * run + 3]
    return sorted({n for n in ns if n > 0})


# ---------------------------------------------------------------- the reference
def _seq_dot(a, b):
    """sum_c a[..., c] * b[..., c], accumulated in the order c = 0..19 (ddot20 / sdot20)."""
    acc = np.zeros(np.broadcast_shapes(a.shape, b.shape)[:-1], np.result_type(a, b))
    for c in range(a.shape[-1]):
        acc = acc + a[..., c] * b[..., c]
    return acc


def _sdot(a, b):
    """sdot20: float32 products accumulated in double, rounded to float32."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    acc = np.zeros(np.broadcast_shapes(a.shape, b.shape)[:-1], np.float64)
    for c in range(a.shape[-1]):
        acc = acc + (a[..., c] * b[..., c]).astype(np.float64)
    return acc.astype(np.float32)


def _pow15_f64(x):
    return math.pow(x, 1.5) if x >= 0.0 else math.nan     # (NaN and negatives: NaN, as pow)


def _pow15(p):
    """percent ** 1.5 as ewk_score.h takes it.  float32 (pow15f): p * sqrt(p) in double, rounded
    to float32 -- IEEE operations, the same bits on the device and here.  float64: pow(p, 1.5),
    one element at a time through libm's scalar pow (numpy's array loop may take a vector
    library's)."""
    if p.dtype == np.float32:
        d = p.astype(np.float64)
        return (d * np.sqrt(d)).astype(np.float32)
    return np.array([_pow15_f64(x) for x in p.ravel()], p.dtype).reshape(p.shape)


def bank_ref(tm, ts, cm, cs, cand="float64", mutant=None):
    """The score of every segment (cm, cs: [n, 20]) against every template (tm, ts: [k, 20]
    float32), operation for operation as csrc/ewk_score.h:

      cand="float64"  score_f64cand_dots: the templates' self-dots are sdot20 (float32 products,
                      double accumulator, rounded to float32), uv and vv are double dots of the
                      statistics as given (float32 statistics widen exactly), then
                      1 - clip(1 - uv / sqrt(uu * vv), 0, 2), * 0.7 + * 0.3, * 100, pow(p, 1.5) / 10
      cand="float32"  score_f32cand_dots: the statistics rounded to float32, every dot an sdot20,
                      the rest in float32 (the square root in double, rounded; the power
                      pow15f: p * sqrt(p) in double, rounded)

    Returns (score[n, k] float64, percent[n, k], mean2[n], std2[n]): mean2 / std2 are the
    segment's self-dots vv_m / vv_s, which the listing rule reads."""
    tm, ts = np.asarray(tm, np.float32), np.asarray(ts, np.float32)
    if mutant == "std_mean_swapped":
        tm, ts = ts, tm
    uu_m, uu_s = _sdot(tm, tm), _sdot(ts, ts)
    with np.errstate(all="ignore"):
        if cand == "float64":
            cm, cs = np.asarray(cm, np.float64), np.asarray(cs, np.float64)
            vv_m, vv_s = _seq_dot(cm, cm), _seq_dot(cs, cs)
            uv_m = _seq_dot(tm.astype(np.float64)[None], cm[:, None])
            uv_s = _seq_dot(ts.astype(np.float64)[None], cs[:, None])
            wm, ws = vv_m, vv_s
            if mutant == "vv_neighbour":
                wm, ws = np.roll(vv_m, -1), np.roll(vv_s, -1)
            sm = 1.0 - np.clip(1.0 - uv_m / np.sqrt(uu_m.astype(np.float64)[None] * wm[:, None]), 0.0, 2.0)
            ss = 1.0 - np.clip(1.0 - uv_s / np.sqrt(uu_s.astype(np.float64)[None] * ws[:, None]), 0.0, 2.0)
            percent = (sm * 0.7 + ss * 0.3) * 100.0
            score = _pow15(percent) / 10.0
        elif cand == "float32":
            cm, cs = np.asarray(cm).astype(np.float32), np.asarray(cs).astype(np.float32)
            vv_m, vv_s = _sdot(cm, cm), _sdot(cs, cs)
            uv_m, uv_s = _sdot(tm[None], cm[:, None]), _sdot(ts[None], cs[:, None])
            wm, ws = vv_m, vv_s
            if mutant == "vv_neighbour":
                wm, ws = np.roll(vv_m, -1), np.roll(vv_s, -1)
            one = np.float32(1.0)
            rm = np.sqrt((uu_m[None] * wm[:, None]).astype(np.float64)).astype(np.float32)
            rs = np.sqrt((uu_s[None] * ws[:, None]).astype(np.float64)).astype(np.float32)
            dm = np.clip(one - uv_m / rm, np.float32(0.0), np.float32(2.0))
            ds = np.clip(one - uv_s / rs, np.float32(0.0), np.float32(2.0))
            percent = ((one - dm) * np.float32(0.7) + (one - ds) * np.float32(0.3)) * np.float32(100.0)
            score = (_pow15(percent) / np.float32(10.0)).astype(np.float64)
        else:
            raise ValueError(cand)
    return score, percent.astype(np.float64), vv_m.astype(np.float64), vv_s.astype(np.float64)


def summarise(scores, thr, mutant=None):
    """What the pass makes of a row of scores (scores[n, s], NaN past the word's size; thr[n]):
    hit_mask (bit j: scores[:, j] >= thr), match, best_score ignoring NaN, best_tmpl (the lowest
    index among equal bests, -1 when the row is all NaN)."""
    scores = np.asarray(scores, np.float64)
    n, s = scores.shape
    thr = np.broadcast_to(np.asarray(thr, np.float64), (n,))
    with np.errstate(invalid="ignore"):
        hit = scores >= thr[:, None]
    weights = np.uint64(1) << np.arange(s, dtype=np.uint64)
    hit_mask = (hit * weights[None]).sum(axis=1, dtype=np.uint64)
    valid = ~np.isnan(scores)
    if mutant == "nan_as_number":          # NaN as -inf in the hit test (no change), as 0 in the best
        valid = np.ones_like(valid)
        scores = np.where(np.isnan(scores), 0.0, scores)
    filled = np.where(valid, scores, -np.inf)
    best = filled.max(axis=1) if s else np.full(n, -np.inf)
    is_best = valid & (filled == best[:, None])
    if mutant == "tie_high":
        tmpl = s - 1 - np.argmax(is_best[:, ::-1], axis=1)
    else:
        tmpl = np.argmax(is_best, axis=1)
    none = ~valid.any(axis=1)
    return dict(hit_mask=hit_mask, match=hit_mask != 0, best_score=np.where(none, np.nan, best),
                best_tmpl=np.where(none, -1, tmpl).astype(np.int32))


MUTANTS = (
    "tmpl_plus_1",        # lane j scores template j + 1 of the bank
    "no_reload",          # the previous item's word: its templates and size (a cache never reloaded)
    "prev_threshold",     # the previous item's word's threshold
    "tie_high",           # equal bests go to the highest index
    "hit_next_group",     # hit_mask taken from the next group of the step
    "nan_as_number",      # NaN as -inf in the hit test and as 0 in the best
    "std_mean_swapped",   # the std templates against the mean statistics and the reverse
    "vv_neighbour",       # the candidate self-dots of the neighbouring segment
)


# ---------------------------------------------------------------- the pool and the segments
@functools.lru_cache(maxsize=None)
def pool():
    """(mean[69, 20], std[69, 20]) float32: bank_cases.oracle_templates() and the NaN template."""
    tm, ts = bank_cases.oracle_templates()
    assert tm.shape == (68, 20) and len({m.tobytes() + s.tobytes() for m, s in zip(tm, ts)}) == 68
    return (np.concatenate([tm, tm[:1]]).astype(np.float32),
            np.concatenate([ts, np.zeros((1, 20), np.float32)]).astype(np.float32))


def oracle_stats(segs, dtype):
    st = [mfcc_ref.extract_mfcc(np.asarray(x).astype(dtype)) for x in segs]
    return np.array([m for m, _ in st], dtype), np.array([s for _, s in st], dtype)


CANDS = ("float64", "float32")


def pool_scores(segs):
    """({cand: scores[n, 69]}, {cand: (mean, std)}): the segments' oracle statistics in either
    candidate dtype and their scores against the pool."""
    tm, ts = pool()
    stats = {c: oracle_stats(segs, np.dtype(c)) for c in CANDS}
    return {c: bank_ref(tm, ts, *stats[c], cand=c)[0] for c in CANDS}, stats


@functools.lru_cache(maxsize=None)
def event_stream():
    """(pcm, events): one synthetic stream of three words and the gate oracle's events on it."""
    from oracle.gate_ref import GateConfig, run_stream
    pcm, _ = synth.make_stream(seed=EVENT_STREAM_SEED, n_words=3, sigma=1e-3)
    pcm = synth.pcm16_roundtrip(pcm)
    return pcm, [e for e in run_stream(pcm, GateConfig(**GATE)).events if not e.skipped]


class Bank:
    """sizes / first: the words; tmpl[K]: pool index of every template; ties[w]: the lanes of
    word w that hold one template (or None); thr[n_words] once thresholds() has run."""

    def __init__(self, name, words, ties=None):
        self.name = name
        self.words = [list(w) for w in words]
        self.sizes = [len(w) for w in words]
        self.first = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.tmpl = np.array([k for w in words for k in w], np.int64)
        self.max_word = max(self.sizes)
        self.G, self.per, self.run = geometry(self.max_word)
        self.n_words = len(words)
        self.ties = ties or [None] * self.n_words
        self.thr = None

    def templates(self):
        """The words as Engine.set_bank takes them."""
        tm, ts = pool()
        return [[(tm[k], ts[k]) for k in w] for w in self.words]

    def n_max(self):
        return 8 * self.run + 3

    def pattern(self, kind, n):
        """word[n] of a batch: constant (the largest word), cycling per item (a reload every
        step), blocks of `per` (the word changes exactly between steps) or seeded random."""
        i = np.arange(n)
        if isinstance(kind, int):               # (that word throughout)
            w = np.full(n, kind)
        elif kind == "constant":
            w = np.full(n, int(np.argmax(self.sizes)))
        elif kind == "cycle":
            w = i % self.n_words
        elif kind == "blocks":
            w = (i // self.per) % self.n_words
        elif kind == "random":
            w = np.random.Generator(np.random.PCG64(SEED + self.max_word)).integers(0, self.n_words, self.n_max())[:n]
        else:
            raise ValueError(kind)
        return w.astype(np.int32)

    def rows(self, all_scores, word, mutant=None):
        """scores[n, max_word] of segment i against the templates of word[i], from all_scores[n, 69]
        by pool index (NaN past the word's size), and thr[n]."""
        word = np.asarray(word, np.int64)
        n = len(word)
        tw = word.copy()
        if mutant == "no_reload" and n > 1:
            tw[1:] = word[:-1]
        hw = word.copy()
        if mutant == "prev_threshold" and n > 1:
            hw[1:] = word[:-1]
        out = np.full((n, self.max_word), np.nan)
        K = len(self.tmpl)
        for w in range(self.n_words):
            sel = np.nonzero(tw == w)[0]
            if not len(sel):
                continue
            k = np.arange(self.first[w], self.first[w + 1])
            if mutant == "tmpl_plus_1":
                k = (k + 1) % K
            out[np.ix_(sel, np.arange(self.sizes[w]))] = all_scores[np.ix_(sel, self.tmpl[k])]
        return out, self.thr[hw]

    def expect(self, all_scores, word, mutant=None):
        """(rows, summary) the pass must give for a batch; best_tmpl is the bank's template index."""
        rows, thr = self.rows(all_scores, word, mutant)
        s = summarise(rows, thr, mutant)
        if mutant == "hit_next_group":
            i = np.arange(len(word))
            ok = (i % self.per != self.per - 1) & (i + 1 < len(word))      # (the step's last group: no bits)
            nxt = np.where(ok, np.roll(s["hit_mask"], -1), np.uint64(0))
            s["hit_mask"], s["match"] = nxt, nxt != 0
        fw = self.first[np.asarray(word, np.int64)]
        if mutant == "no_reload" and len(word) > 1:
            fw = np.concatenate([fw[:1], fw[:-1]])
        s["best_tmpl"] = np.where(s["best_tmpl"] >= 0, s["best_tmpl"] + fw, -1).astype(np.int32)
        return rows, s


def _perm(seed, k):
    return [int(x) for x in np.random.Generator(np.random.PCG64(seed)).permutation(68)[:k]]


def _plain_words(L):
    small = min(3, L)
    return [_perm(SEED + 10 * L, small), _perm(SEED + 10 * L + 1, 1), _perm(SEED + 10 * L + 2, L),
            _perm(SEED + 10 * L + 3, max(1, L // 2 + 1) if L > 1 else 1)]


def _popular_best(scores, members):
    """The member of a word that is most often the best template over the rows of scores[n, 69]."""
    sub = scores[:, members]
    best = np.array(members)[np.nanargmax(sub, axis=1)]
    vals, cnt = np.unique(best, return_counts=True)
    return int(vals[np.argmax(cnt)])


def _special_words(G, scores):
    """The special bank of a G: (words, ties).  Word w's base is a seeded draw of G pool
    templates; T is the one most often best over the segments that cycle onto word w.  Tie words
    hold T at two (three) lanes, NaN words the zero-std template."""
    words, ties = [], []
    pairs = [p for p in TIE_PAIRS if p[1] < G]
    if G >= 4:
        pairs.append((1, G // 2, G - 1))
    kinds = [("tie", p) for p in pairs] + [("nan", "first"), ("nan", "last"), ("nan", "best"), ("nan", "all")]
    kinds.insert(1, ("single", None))          # a one-template word: word_first unaligned
    nw = len(kinds)
    for w, (kind, arg) in enumerate(kinds):
        base = _perm(SEED + 1000 * G + w, G)
        mine = scores[w::nw]                    # (the cycle pattern puts these segments on word w)
        tie = None
        if kind == "single":
            base = base[:1]
        elif kind == "tie":
            t = _popular_best(mine, base)
            rest = [k for k in base if k != t]
            word = []
            for lane in range(G):
                word.append(t if lane in arg else rest.pop())
            base, tie = word, tuple(arg)
        elif arg == "first":
            base[0] = NAN_TMPL
        elif arg == "last":
            base[-1] = NAN_TMPL
        elif arg == "best":
            base[base.index(_popular_best(mine, base))] = NAN_TMPL
        else:
            base = [NAN_TMPL] * G
        words.append(base)
        ties.append(tie)
    return words, ties


BIT63_N = 17            # the hit-bit-63 batch: run + 1 segments


def _bit63_words(scores, seg):
    """Two 64-template words for segment `seg`: its best template at lane 63 (the threshold
    between its best and its second best: bit 63 alone), and its worst at lane 63 (between
    the worst and the next: every bit but 63).  Returns (words, the two thresholds)."""
    base = [k for k in _perm(SEED + 6300, 65) if np.isfinite(scores[seg, k])][:64]
    order = sorted(base, key=lambda k: scores[seg, k])        # ascending
    up = order[:]                                             # best last, second best at lane 62
    down = order[2:] + order[1::-1]                           # worst last, the next worst at lane 62
    s = scores[seg]
    return [up, _perm(SEED + 6301, 1), down], ((s[up[63]] + s[up[62]]) / 2, (s[down[63]] + s[down[62]]) / 2)


def _bit63_bank(scores):
    """The hit-bit-63 bank on the segment of the batch that leaves every score of the batch
    farthest from the two thresholds."""
    best = None
    for seg in range(BIT63_N):
        words, thr = _bit63_words(scores["float64"], seg)
        d = min(np.nanmin(np.abs(scores[c][:BIT63_N][:, words[w]] - t))
                for c in scores for w, t in ((0, thr[0]), (2, thr[1])))
        if best is None or d > best[0]:
            best = (d, seg, words, thr)
    return best[1:]


def _threshold(vals, lo=0.25, hi=0.75):
    """The midpoint of the widest gap between adjacent values in the middle half of `vals`."""
    v = np.sort(vals[np.isfinite(vals)])
    if v.size < 2:
        return 50.0
    a, b = int(v.size * lo), max(int(v.size * lo) + 2, int(math.ceil(v.size * hi)))
    mid = v[a:b]
    i = int(np.argmax(np.diff(mid)))
    return float((mid[i] + mid[i + 1]) / 2)


def _word_gap_ok(scores, members, tie):
    """Per row of scores[n, 69]: the word's two best scores are at least MARGIN apart in every
    candidate dtype -- or, in a tie word, the tied lanes' one score stands for them all."""
    cols = list(dict.fromkeys(members)) if tie else list(members)
    sub = np.sort(np.where(np.isnan(scores[:, cols]), -np.inf, scores[:, cols]), axis=1)
    if sub.shape[1] < 2:
        return np.ones(len(scores), bool)
    with np.errstate(invalid="ignore"):
        return ~(sub[:, -1] - sub[:, -2] < MARGIN)           # (-inf - -inf: NaN: one or no score)


class Matrix:
    """The segments, the banks and their thresholds: see the module's docstring."""

    def __init__(self):
        cand = synth.ragged_segments(SEED, N_CAND, 3200, 8000)
        short = synth.ragged_segments(SEED + 1, len(SHORT_AT), 1600, 2559)
        assert all(1 + len(s) // 160 <= RESCORE_FRAMES for s in short)
        plain = {L: _plain_words(L) for L in SIZES}
        # the oracle runs once per candidate and dtype, and only as far down the list as it takes
        keep, parts, lo = [], [], 0
        while len(keep) < N_SEG:
            assert lo < N_CAND, len(keep)
            hi = min(N_CAND, lo + max(16, N_SEG - len(keep) + 8))
            sc, st = pool_scores(cand[lo:hi])
            ok = np.ones(hi - lo, bool)
            for c in CANDS:
                for L in SIZES:
                    for w in plain[L]:
                        ok &= _word_gap_ok(sc[c], w, None)
            parts.append((lo, sc, st))
            keep.extend(int(lo + i) for i in np.nonzero(ok)[0])
            lo = hi
        keep = keep[:N_SEG]
        self.n_candidates_dropped = keep[-1] + 1 - N_SEG
        self.segs = [cand[i] for i in keep]

        def rows(table):        # the kept candidates' rows of the per-part tables
            where = {lo + i: (k, i) for k, (lo, sc, _) in enumerate(parts) for i in range(len(sc["float64"]))}
            return np.array([table(parts[where[g][0]])[where[g][1]] for g in keep])

        self.scores = {c: rows(lambda p, c=c: p[1][c]) for c in CANDS}     # oracle statistics: conditions, thresholds
        self.stats = {c: tuple(rows(lambda p, c=c, j=j: p[2][c][j]) for j in (0, 1)) for c in CANDS}
        sc, st = pool_scores(short)
        for k, at in enumerate(SHORT_AT):
            self.segs[at] = short[k]
            for c in CANDS:
                self.scores[c][at] = sc[c][k]
                self.stats[c][0][at], self.stats[c][1][at] = st[c][0][k], st[c][1][k]
        self.events = [np.asarray(e.audio, np.float64) for e in event_stream()[1]]
        self.event_scores = pool_scores(self.events)[0]
        self.banks = {L: Bank(f"L{L}", plain[L]) for L in SIZES}
        self.special = {}
        for G in (1, 2, 4, 8, 16, 32, 64):
            words, ties = _special_words(G, self.scores["float64"][:8 * geometry(G)[2] + 3])
            self.special[G] = Bank(f"special{G}", words, ties)
        self.bit63_seg, words, thr63 = _bit63_bank(self.scores)
        self.bit63 = Bank("bit63", words)
        for b in self.all_banks():
            self._thresholds(b)
        self.bit63.thr[0], self.bit63.thr[2] = thr63       # around that segment's extreme scores

    def all_banks(self):
        return list(self.banks.values()) + list(self.special.values()) + [self.bit63]

    def _thresholds(self, b):
        thr = []
        for w in range(b.n_words):
            k = b.tmpl[b.first[w]:b.first[w + 1]]
            vals = np.concatenate([self.scores[c][:, k].ravel() for c in self.scores] +
                                  [self.event_scores[c][:, k].ravel() for c in self.event_scores])
            thr.append(_threshold(vals))
        # distinct per word (an all-NaN or repeated word falls back to 50: nudge it)
        for w in range(len(thr)):
            while thr[w] in thr[:w]:
                thr[w] += 0.25
        b.thr = np.array(thr, np.float64)

    def cases(self, b):
        """(kind, n) of every batch of bank b in the matrix: a batch is the first n segments."""
        if b is self.bit63:
            return [(0, BIT63_N), (2, BIT63_N)]
        if b.ties.count(None) < b.n_words or NAN_TMPL in b.tmpl:          # a special bank
            return [("cycle", b.n_max()), ("random", b.n_max()), ("cycle", b.run + 1)]
        return [(kind, n) for kind in PATTERNS for n in batch_sizes(b.max_word)]

    def family(self, G):
        """The banks whose segments take G lanes."""
        return [b for b in self.all_banks() if b.G == G]

    @functools.lru_cache(maxsize=None)
    def mutant_scores(self, mutant, cand="float64"):
        """scores[N_SEG, 69] of the oracle statistics by bank_ref with a defect in its arithmetic."""
        tm, ts = pool()
        return bank_ref(tm, ts, *self.stats[cand], cand=cand, mutant=mutant)[0]

    def conditions(self, b, scores, word):
        """(top-2 gap, threshold distance) minima of a batch from scores[n, 69]: the two best
        scores of a row apart (exact ties of a tie word's lanes aside) and every score away
        from its word's threshold."""
        rows, thr = b.rows(scores, word)
        gap = np.inf
        for i, w in enumerate(np.asarray(word)):
            r = rows[i, :b.sizes[w]]
            if b.ties[w]:
                r = np.delete(r, b.ties[w][1:])
            f = np.sort(r[np.isfinite(r)])
            if f.size >= 2:
                gap = min(gap, f[-1] - f[-2])
        with np.errstate(invalid="ignore"):
            d = np.abs(rows - thr[:, None])
        return float(gap), float(np.nanmin(d)) if np.isfinite(d).any() else np.inf


@functools.lru_cache(maxsize=None)
def matrix():
    return Matrix()


def listed(b, word, lengths, rows, percent_rows, mean2, std2, margin, cand, tiny_mean, nan_a, nan_b):
    """The float32 pass's listing rule (ewk_bank.hip, the single-template epilogue's per
    template): rescored[n] for a batch whose rows / percent_rows[n, max_word] and mean2 / std2
    come from bank_ref on the float32 statistics."""
    thr = b.thr[np.asarray(word, np.int64)]
    act = np.arange(b.max_word)[None] < np.array(b.sizes)[np.asarray(word, np.int64)][:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        near = (act & (np.abs(rows - thr[:, None]) < margin)).any(axis=1)
        sure = percent_rows < -(nan_a / np.sqrt(mean2) + nan_b)[:, None]
        if cand == "float32":
            sure = np.zeros_like(sure)
        unsure = (act & ~sure).any(axis=1)
        short = 1 + np.asarray(lengths) // 160 <= RESCORE_FRAMES
        return near | short | ((std2 > 0.0) & (std2 < KTINY_STD * KTINY_STD)) | \
            ((mean2 < tiny_mean * tiny_mean) & unsure)


def ulps(got, ref, dtype=np.float64):
    """|got - ref| in units of ref's spacing in `dtype` (0 where both are NaN, inf where one is)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    with np.errstate(invalid="ignore"):
        d = np.abs(got - ref) / np.spacing(np.abs(ref).astype(dtype)).astype(np.float64)
    d = np.where(np.isnan(got) & np.isnan(ref), 0.0, d)
    return np.where(np.isnan(got) != np.isnan(ref), np.inf, d)
