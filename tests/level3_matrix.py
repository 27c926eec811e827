"""Shared by the level-3 matrix tests (tests/test_level3_matrix.py on the CPU,
tests/test_gpu_level3_matrix.py on the GPU): the split rule of numpy's pairwise summation as plain
Python, a float64 model of the whole reduction, the reference, the bit comparison and the seeded
case builders.  Nothing here touches a GPU.

k_normalize (csrc/ewk_level3.hip) evaluates np.mean's pairwise tree lane-parallel, once per
8192-sample chunk: split top-down (a node of m > 128 samples splits at n2 = m/2 - (m/2) % 8),
leaves numbered by ballot, nodes combined bottom-up, all LDS state reused for the next chunk.  The
cases below reach every chunk length, every class of tree, the chunk-to-chunk reuse, every place a
ring can wrap inside a segment, and the values numpy treats specially.

The GPU tests compare with normalize_ref -- the reference's numpy expression -- and never with the
model; the model is held to numpy on the CPU, so that a numpy that sums differently fails there.
"""
import numpy as np

from oracle.gate_ref import normalize_level3

CHUNK = 8192          # np.add.reduce walks a contiguous array in buffers of 8192 elements
LEAF = 128            # a node of at most 128 elements is summed, not split
BLOCK = 1600
RING_COMPACT = 43200  # the smallest compact ring the default configuration accepts
RING_DEFAULT = 160000
N_STREAMS = 4


# ---- the split rule -----------------------------------------------------------------------------
def levels(cn):
    """The nodes of a chunk of cn samples, depth by depth: levels(cn)[d] is the list of
    (start, length) at depth d, in order.  A node of more than 128 samples has two children."""
    out = [[(0, cn)]]
    while True:
        nxt = []
        for st, m in out[-1]:
            if m > LEAF:
                n2 = m // 2
                n2 -= n2 % 8
                nxt += [(st, n2), (st + n2, m - n2)]
        if not nxt:
            return out
        out.append(nxt)


def tree(cn):
    """(leaves, cls): the leaves of a chunk of cn samples as (start, length, depth), in sample
    order, and the deepest depth at which a node still splits (-1: the chunk is one leaf)."""
    lv = levels(cn)
    leaves = sorted((st, m, d) for d, nodes in enumerate(lv) for st, m in nodes if m <= LEAF)
    return leaves, len(lv) - 2


def mixed_depths(cn):
    """The depths at which a leaf stands beside a node that splits again."""
    return [d for d, nodes in enumerate(levels(cn))
            if any(m <= LEAF for _, m in nodes) and any(m > LEAF for _, m in nodes)]


# ---- numpy's reduction, in plain Python -----------------------------------------------------------
def _leaf_sum(x, s, n):
    if n < 8:
        r = 0.0
        for i in range(s, s + n):
            r += x[i]
        return r
    r0, r1, r2, r3, r4, r5, r6, r7 = x[s:s + 8]
    lim = s + n - n % 8
    for i in range(s + 8, lim, 8):
        r0 += x[i]
        r1 += x[i + 1]
        r2 += x[i + 2]
        r3 += x[i + 3]
        r4 += x[i + 4]
        r5 += x[i + 5]
        r6 += x[i + 6]
        r7 += x[i + 7]
    r = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7))
    for i in range(lim, s + n):
        r += x[i]
    return r


def _pairwise(x, s, n):
    if n <= LEAF:
        return _leaf_sum(x, s, n)
    n2 = n // 2
    n2 -= n2 % 8
    return _pairwise(x, s, n2) + _pairwise(x, s + n2, n - n2)


def pairwise_sum(x, chunk=CHUNK):
    """np.add.reduce of a contiguous float64 array as Python float arithmetic: chunks of 8192
    accumulated from 0.0, each chunk summed by the pairwise recursion.  chunk=None: one recursion
    over the whole array (what numpy does not do -- test_level3_matrix.py keeps that a fact)."""
    x = np.asarray(x, np.float64).tolist()
    n = len(x)
    if chunk is None:
        return _pairwise(x, 0, n)
    acc = 0.0
    for c0 in range(0, n, chunk):
        acc += _pairwise(x, c0, min(chunk, n - c0))
    return acc


# ---- the reference and the comparison -------------------------------------------------------------
def normalize_ref(x):
    """The reference's level-3 normalisation (oracle.gate_ref.normalize_level3: its numpy
    expression) of one segment.  Non-finite samples make numpy warn; they are meant."""
    with np.errstate(all="ignore"):
        return normalize_level3(np.asarray(x))


def bits_equal(got, want):
    """float64 arrays of one shape with NaN in the same places and the same bits everywhere else
    (so +0.0 and -0.0 differ)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float64 and want.dtype == np.float64, (got.dtype, want.dtype)
    assert got.shape == want.shape, (got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    if not np.array_equal(gn, wn):
        return False
    return np.array_equal(np.ascontiguousarray(got).view(np.int64)[~gn], np.ascontiguousarray(want).view(np.int64)[~wn])


def first_diff(got, want):
    """Where and how two arrays bits_equal rejects differ (for a failure message)."""
    got, want = np.asarray(got), np.asarray(want)
    gn, wn = np.isnan(got), np.isnan(want)
    bad = np.flatnonzero((gn != wn) | (~gn & ~wn & (got.view(np.int64) != want.view(np.int64))))
    i = int(bad[0])
    return dict(n_diff=len(bad), first=i, got=float(got[i]).hex(), want=float(want[i]).hex())


# ---- linear cases ---------------------------------------------------------------------------------
def gauss(rng, n):
    """Gaussian of a random scale 1e-4..1 plus a DC offset, float32."""
    return (rng.standard_normal(n) * 10 ** rng.uniform(-4, 0) + rng.uniform(-0.1, 0.1)).astype(np.float32)


def wide(rng, n):
    """Gaussian samples scaled sample by sample over forty binades, float32.  The float64 sum of
    gauss() data is nearly always exact, whatever the order of the additions; these sums round at
    most additions, so they tell one summation order from another."""
    return (rng.standard_normal(n) * 2.0 ** rng.integers(-40, 1, n)).astype(np.float32)


RECIPES = {"gauss": gauss, "wide": wide}
CALL_SAMPLES = 8 * 1024 * 1024     # 64 MB of float64 output a call


def chunk_length_calls(seed=20):
    """Every length 1..8192 once, in a seeded order, cut into calls of at most CALL_SAMPLES."""
    order = np.random.default_rng(seed).permutation(np.arange(1, CHUNK + 1))
    calls, cur, tot = [], [], 0
    for n in order.tolist():
        if tot + n > CALL_SAMPLES:
            calls.append(cur)
            cur, tot = [], 0
        cur.append(n)
        tot += n
    calls.append(cur)
    return calls


N_CALLS = 5


def chunk_length_segments(call, recipe="gauss", seed=21):
    rng = np.random.default_rng(seed + call + 100 * list(RECIPES).index(recipe))
    return [RECIPES[recipe](rng, n) for n in chunk_length_calls()[call]]


# tails r of a segment of 8192 * k + r samples: the LDS tree state of a full chunk (64 leaves of
# 128, split depth 5) is reused for a chunk of r
TAILS = [1, 7, 8, 128, 129, 249, 256, 257, 489, 512, 519, 969, 1031, 1929, 2055, 3849, 4103, 7688, 7689, 8191]
LONG = [160000, 320000]


def tail_lengths():
    """8192 * k + r for k in 1, 2 and r in TAILS (8192 + 1 and 2 * 8192 + 249 among them: the
    shortest tail, and the shortest tail with a leaf beside a split node, after full chunks), and
    the long segments."""
    out = [CHUNK * k + r for k in (1, 2) for r in TAILS] + LONG
    assert CHUNK + 1 in out and 2 * CHUNK + 249 in out
    return out


def tail_segments(recipe="gauss", seed=22):
    rng = np.random.default_rng(seed + 100 * list(RECIPES).index(recipe))
    return [RECIPES[recipe](rng, n) for n in tail_lengths()]


VALUE_LENGTHS = [300, 8193, 20000]
NONFINITE = ("nan", "pos_inf", "neg_inf", "both_inf")


def value_cases(n, seed=23):
    """name -> float32 segment of n samples with the values numpy treats specially."""
    rng = np.random.default_rng(seed + n)
    base = gauss(rng, n)
    out = {}
    x = base.copy()
    x[[n // 3, n - 2]] = np.nan
    out["nan"] = x
    x = base.copy()
    x[[5, n - 1]] = np.inf            # mean +inf: -1.0 at the finite samples, NaN at these two
    out["pos_inf"] = x
    x = base.copy()
    x[[0, n // 2]] = -np.inf
    out["neg_inf"] = x
    x = base.copy()
    x[7], x[n - 9] = np.inf, -np.inf  # mean NaN: all NaN
    out["both_inf"] = x
    x = np.full(n, 3e38, np.float32)
    x[1::2] = -3e38
    out["huge"] = x
    x = (rng.integers(1, 1 << 23, n) * np.float64(2.0 ** -149)).astype(np.float32)   # float32 denormals
    x[rng.random(n) < 0.5] = 0.0
    x[::5] *= -1                      # (negative denormals and negative zeros among them)
    out["denormal"] = x
    if n > CHUNK:
        out["constant"] = np.full(n, 0.25, np.float32)   # max |y| == 0: unscaled zeros
    out["neg_zero"] = np.full(n, -0.0, np.float32)       # numpy sums these to +0.0: y = -0.0 - 0.0
    out["one_ulp"] = (1.0 + rng.integers(0, 16, n) * 2.0 ** -23).astype(np.float32)
    return out


def value_batch():
    """(names, segments): every value case with a clean Gaussian neighbour on either side."""
    rng = np.random.default_rng(24)
    names, segs = ["clean"], [gauss(rng, 517)]
    for n in VALUE_LENGTHS:
        for name, x in value_cases(n).items():
            names += [f"{name}_{n}", "clean"]
            segs += [x, gauss(rng, int(rng.integers(130, 9000)))]
    return names, segs


def device_form_segments(seed=25):
    """The batch of the device-form test: a zero-length segment, one chunk, tails, a mixed tree."""
    rng = np.random.default_rng(seed)
    return [gauss(rng, n) for n in (249, 0, 8193, 1, 7689, 16391, 129)]


# ---- ring cases -----------------------------------------------------------------------------------
RING_LENGTHS = [1, 7, 129, 249, 8191, 8192, 8193, 16391, 43200]
WRAPS = ("none", "first_chunk", "chunk_end", "second_chunk", "last_sample", "whole_ring")
RING_TICKS = {RING_COMPACT: 30, RING_DEFAULT: 110}     # pushed before the events: each ring has wrapped


def ring_signal(fmt, ring, seed=26):
    """(src, data): what is pushed into the N_STREAMS rings -- float32 noise of sigma 1e-3, distinct
    per stream, or its int16 quantisation for an int16 ring (fmt 1) -- and the float32 values the
    ring then holds (int16 k decodes to k / 32768)."""
    n = RING_TICKS[ring] * BLOCK
    rng = np.random.default_rng(seed + 7 * fmt + ring)
    x = (rng.standard_normal((N_STREAMS, n)) * 1e-3 + rng.uniform(-2e-4, 2e-4, (N_STREAMS, 1))).astype(np.float32)
    if fmt == 0:
        return x, x
    k = np.round(x.astype(np.float64) * 32768.0).astype(np.int16)
    return k, k.astype(np.float32) / np.float32(32768.0)


def nreq_of(ring, now, ring_start):
    """The host rule of ewk_normalize_events for an event of tick `now`: the samples between its
    ring_start and the write position, 0 meaning the whole ring."""
    n = (now * BLOCK - ring_start) % ring
    return n if n else ring


def _wrap_at(kind, length, ring, w_pos):
    """Samples of the segment before the physical wrap (None: no wrap), or False if this kind
    cannot be placed for this length with w_pos samples written since the ring's start."""
    lo_fit = max(1, length - w_pos)       # length <= nreq = w_pos + w
    if kind == "first_chunk":
        lo, hi = lo_fit, min(length, CHUNK) - 1
    elif kind == "chunk_end":
        lo, hi = max(lo_fit, CHUNK), CHUNK if length > CHUNK else 0
    elif kind == "second_chunk":
        lo, hi = max(lo_fit, CHUNK + 1), min(length, 2 * CHUNK) - 1
    elif kind == "last_sample":
        lo, hi = max(lo_fit, length - 1), length - 1
    else:
        raise ValueError(kind)
    hi = min(hi, ring - w_pos)            # (past that, ring_start would lie below the write position)
    if lo > hi or hi < 1:
        return False
    return (lo + hi + 1) // 2


def ring_events(ring):
    """The crafted events of one ring size, tick = now: dicts of stream, ring_start, length and the
    wrap kind, every listed length at every wrap position the host rule admits, streams in a
    shuffled order."""
    now = RING_TICKS[ring]
    w_pos = now * BLOCK % ring
    assert 0 < w_pos and now * BLOCK > ring
    out = []
    for length in RING_LENGTHS:
        if length > ring:
            continue
        if length <= ring - w_pos:      # ends on the ring's last sample: k never reaches ring
            out.append(dict(ring_start=ring - length, length=length, wrap="none"))
        if length <= w_pos:             # the newest samples, below the write position
            out.append(dict(ring_start=w_pos - length, length=length, wrap="none"))
        for kind in WRAPS[1:5]:
            w = _wrap_at(kind, length, ring, w_pos)
            if w:
                out.append(dict(ring_start=ring - w, length=length, wrap=kind))
    out.append(dict(ring_start=w_pos, length=ring, wrap="whole_ring"))
    rng = np.random.default_rng(27 + ring)
    for i, e in enumerate(out):
        e["stream"] = i % N_STREAMS
    return [out[i] for i in rng.permutation(len(out))]


def event_array(events, now):
    from easywakeword_amd import _lib
    ev = np.zeros(len(events), _lib.EVENT_DTYPE)
    for r, e in zip(ev, events):
        r["stream"], r["length"], r["tick"], r["ring_start"] = e["stream"], e["length"], now, e["ring_start"]
    return ev


def ring_image(data, ring):
    """The ring after `data` (one stream's float32 values) was pushed: global sample j lives at
    j mod ring."""
    n = len(data)
    img = np.zeros(ring, np.float32)
    j = np.arange(max(0, n - ring), n)
    img[j % ring] = data[j]
    return img


def ring_segment(data, ring, ring_start, length):
    """An event's samples from the pushed samples."""
    return ring_image(data, ring)[(ring_start + np.arange(length)) % ring]
