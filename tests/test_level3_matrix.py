"""The level-3 matrix's reference side, held to numpy (CPU): the plain-Python model of
np.add.reduce agrees with numpy at every chunk length, the facts about the pairwise tree that
k_normalize's LDS arrays rely on, and the conditions a case list must meet before a kernel is
looked at -- so a numpy that sums differently, or a case list that shrank, fails here."""
import collections

import numpy as np
import pytest

import level3_matrix as lm

_rng = np.random.default_rng(1)
# float32-valued float64 data with a DC offset
_DATA = (_rng.standard_normal(170000) * 0.05 + 0.03).astype(np.float32).astype(np.float64)


# the same over forty binades: these sums round, so the order of the additions shows
_WIDE = lm.wide(np.random.default_rng(2), 170000).astype(np.float64)
_SETS = {"gauss": _DATA, "wide": _WIDE}


@pytest.mark.parametrize("data", list(_SETS))
def test_model_equals_numpy_at_every_chunk_length(data):
    bad = []
    for n in range(1, lm.CHUNK + 1):
        x = _SETS[data][3 * n:4 * n]
        if lm.pairwise_sum(x) != np.add.reduce(x):
            bad.append(n)
    assert not bad, bad[:20]


@pytest.mark.parametrize("data", list(_SETS))
@pytest.mark.parametrize("n", [8193, 16384, 16385, 24576 + 129, 65536 + 7689, 160000])
def test_model_equals_numpy_past_one_chunk(n, data):
    x = _SETS[data][5:5 + n]
    assert lm.pairwise_sum(x) == np.add.reduce(x)
    assert lm.pairwise_sum(x) / n == np.mean(x)


def test_numpy_sums_in_chunks_of_8192():
    """One pairwise recursion over 48000 samples is not what numpy computes; the chunked one is.
    (If this fails numpy has changed its buffering, and k_normalize's chunking is wrong with it.)"""
    x = _WIDE[:48000]
    assert lm.pairwise_sum(x) == np.add.reduce(x)
    assert lm.pairwise_sum(x, chunk=None) != np.add.reduce(x)


def test_only_the_wide_data_tells_summation_orders_apart():
    """float32 Gaussians of one scale sum exactly in float64 in any order -- a tree evaluated in
    the wrong order still gives numpy's mean on them; the wide recipe's sums round.  In-order
    summation against numpy at 218 lengths above one leaf."""
    differ = {k: sum(sum(v[n:2 * n].tolist()) != np.add.reduce(v[n:2 * n]) for n in range(129, lm.CHUNK + 1, 37))
              for k, v in _SETS.items()}
    assert differ["gauss"] == 0 and differ["wide"] >= 190, differ


def test_model_on_zeros_of_either_sign():
    """numpy accumulates from +0.0: negative zeros alone sum to +0.0, as in the model."""
    for n in (1, 7, 8, 300, 8193):
        x = np.full(n, -0.0)
        s = np.add.reduce(x)
        assert s == 0.0 and not np.signbit(s) and not np.signbit(lm.pairwise_sum(x))


def test_tree_facts():
    """What the kernel's arrays (128 nodes a depth, 9 depths, 128 leaves) rely on, and the class
    populations of the issue's table."""
    pop = collections.Counter()
    max_leaves = max_nodes = max_depth = 0
    for cn in range(1, lm.CHUNK + 1):
        lv = lm.levels(cn)
        leaves, cls = lm.tree(cn)
        pop[cls] += 1
        max_leaves = max(max_leaves, len(leaves))
        max_nodes = max(max_nodes, max(len(nodes) for nodes in lv))
        max_depth = max(max_depth, cls)
        # the leaves tile the chunk in order, none above 128 samples
        pos = 0
        for st, m, d in leaves:
            assert st == pos and 0 < m <= lm.LEAF and d <= cls + 1
            pos += m
        assert pos == cn
    assert (max_leaves, max_nodes, max_depth) == (65, 64, 6)
    assert [pop[c] for c in range(-1, 7)] == [128, 121, 242, 484, 968, 1936, 3872, 441]
    assert lm.tree(128) == ([(0, 128, 0)], -1)
    assert lm.tree(249) == ([(0, 120, 1), (120, 64, 2), (184, 65, 2)], 1)
    assert lm.mixed_depths(249) == [1] and lm.mixed_depths(248) == [] and lm.mixed_depths(8192) == []
    assert min(cn for cn in range(1, lm.CHUNK + 1) if lm.mixed_depths(cn)) == 249
    assert sum(len(set(m for _, m, _ in lm.tree(cn)[0])) > 2 for cn in range(1, lm.CHUNK + 1)) == 6553
    assert lm.tree(8192)[1] == 5 and len(lm.tree(8192)[0]) == 64


def test_tail_list_covers_every_class():
    classes = {lm.tree(r)[1] for r in lm.TAILS}
    assert classes == set(range(-1, 7))
    mixed = {lm.tree(r)[1] for r in lm.TAILS if lm.mixed_depths(r)}
    assert mixed >= set(range(1, 7)), mixed
    want = {1, 7, 8, 128, 129, 249, 256, 257, 489, 512, 519, 969, 1031, 1929, 2055, 3849, 4103, 7688, 7689, 8191}
    assert want <= set(lm.TAILS)
    lengths = lm.tail_lengths()
    for k in (1, 2):
        assert {lm.CHUNK * k + r for r in want} <= set(lengths)
    assert lengths.count(160000) == 1 and lengths.count(320000) == 1


def test_chunk_length_calls_cover_every_length_once():
    calls = lm.chunk_length_calls()
    assert len(calls) == lm.N_CALLS
    assert sorted(n for c in calls for n in c) == list(range(1, lm.CHUNK + 1))
    assert max(sum(c) for c in calls) * 8 <= 64 << 20
    segs = lm.chunk_length_segments(0)
    assert [len(s) for s in segs] == calls[0] and segs[0].dtype == np.float32


def test_linear_cases_are_what_they_claim():
    for x in lm.tail_segments() + lm.tail_segments("wide") + lm.chunk_length_segments(1)[:50] + \
            lm.chunk_length_segments(1, "wide")[:50] + [s for s in lm.device_form_segments() if len(s)]:
        assert np.isfinite(x).all() and (len(x) == 1 or x.min() < x.max())
    names, segs = lm.value_batch()
    assert len(names) == len(segs)
    for i, (name, x) in enumerate(zip(names, segs)):
        assert x.dtype == np.float32
        if name.rsplit("_", 1)[0] in lm.NONFINITE:
            assert not np.isfinite(x).all()
            assert names[i - 1] == "clean" and names[i + 1] == "clean"
        else:
            assert np.isfinite(x).all(), name
    for n in lm.VALUE_LENGTHS:
        v = lm.value_cases(n)
        assert ("constant" in v) == (n > lm.CHUNK)
        ref = {k: lm.normalize_ref(x) for k, x in v.items()}
        assert np.isnan(ref["nan"]).all() and np.isnan(ref["both_inf"]).all()
        inf = np.isinf(v["pos_inf"])
        assert np.isnan(ref["pos_inf"][inf]).all() and (ref["pos_inf"][~inf] == -1.0).all()
        inf = np.isinf(v["neg_inf"])
        assert np.isnan(ref["neg_inf"][inf]).all() and (ref["neg_inf"][~inf] == 1.0).all()
        assert (np.abs(ref["huge"]) == 1.0).all()
        d = v["denormal"]
        assert (np.abs(d[d != 0]) < np.finfo(np.float32).tiny).all() and (d == 0).any() and (d != 0).any()
        assert np.signbit(d[d == 0]).any() and not np.signbit(d[d == 0]).all()
        assert np.signbit(ref["neg_zero"]).all() and (ref["neg_zero"] == 0).all()
        if "constant" in v:
            assert (ref["constant"] == 0).all() and not np.signbit(ref["constant"]).any()
        # one ulp of the mean moves most output bits: the outputs are not on a coarse grid
        assert len(np.unique(ref["one_ulp"])) >= 8


def test_bits_equal():
    a = np.array([0.0, 1.0, np.nan, -2.5])
    assert lm.bits_equal(a, a.copy())
    assert not lm.bits_equal(a, np.array([-0.0, 1.0, np.nan, -2.5]))          # the sign of zero
    assert not lm.bits_equal(a, np.array([0.0, 1.0, 3.0, -2.5]))              # NaN in another place
    assert not lm.bits_equal(a, np.array([0.0, np.nextafter(1.0, 2.0), np.nan, -2.5]))
    assert lm.first_diff(a, np.array([-0.0, 1.0, np.nan, -2.5]))["first"] == 0
    with pytest.raises(AssertionError):
        lm.bits_equal(a, a[:3])
    with pytest.raises(AssertionError):
        lm.bits_equal(a.astype(np.float32), a)


@pytest.mark.parametrize("ring", [lm.RING_COMPACT, lm.RING_DEFAULT])
def test_ring_events_obey_the_host_rule(ring):
    """Every crafted event is one ewk_normalize_events accepts at tick = now (length <= nreq <=
    ring), the wrap falls where its kind says, and no kind or length has dropped out."""
    now = lm.RING_TICKS[ring]
    assert now * lm.BLOCK > ring                       # the ring has wrapped
    events = lm.ring_events(ring)
    seen = collections.defaultdict(set)
    for e in events:
        L, st = e["length"], e["ring_start"]
        assert 0 <= st < ring and 0 < L <= ring and 0 <= e["stream"] < lm.N_STREAMS
        nreq = lm.nreq_of(ring, now, st)
        assert L <= nreq <= ring, e
        w = ring - st                                  # samples before the physical wrap
        kind = e["wrap"]
        if kind == "none":
            assert w >= L
        elif kind == "first_chunk":
            assert 0 < w < min(L, lm.CHUNK)
        elif kind == "chunk_end":
            assert w == lm.CHUNK < L and st + lm.CHUNK == ring
        elif kind == "second_chunk":
            assert lm.CHUNK < w < min(L, 2 * lm.CHUNK)
        elif kind == "last_sample":
            assert w == L - 1
        else:
            assert kind == "whole_ring" and L == ring == nreq
        seen[kind].add(L)
    assert set(seen) == set(lm.WRAPS)
    assert set().union(*seen.values()) == {n for n in lm.RING_LENGTHS if n <= ring} | {ring}
    assert seen["none"] >= {1, 7, 129, 249, 8191, 8192, 8193, 16391}
    assert seen["first_chunk"] >= {7, 129, 249, 8191, 8192, 8193}
    assert seen["last_sample"] >= {7, 129, 249, 8191, 8192, 8193, 16391}
    assert 8193 in seen["chunk_end"] and 16391 in seen["second_chunk"]
    if ring == lm.RING_DEFAULT:                        # room behind the write position for the long ones
        assert 16391 in seen["first_chunk"] and 16391 in seen["chunk_end"] and 43200 in seen["last_sample"]
    assert {e["stream"] for e in events} == set(range(lm.N_STREAMS))
    assert [e["stream"] for e in events] != sorted(e["stream"] for e in events)


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("ring", [lm.RING_COMPACT, lm.RING_DEFAULT])
def test_ring_segments_are_finite_and_not_constant(ring, fmt):
    src, data = lm.ring_signal(fmt, ring)
    assert src.shape == data.shape == (lm.N_STREAMS, lm.RING_TICKS[ring] * lm.BLOCK)
    assert data.dtype == np.float32 and src.dtype == (np.int16 if fmt else np.float32)
    if fmt:
        assert np.array_equal(data.astype(np.float64) * 32768.0, src.astype(np.float64))
    assert len({data[s].tobytes() for s in range(lm.N_STREAMS)}) == lm.N_STREAMS
    for e in lm.ring_events(ring):
        seg = lm.ring_segment(data[e["stream"]], ring, e["ring_start"], e["length"])
        assert len(seg) == e["length"] and np.isfinite(seg).all()
        assert e["length"] == 1 or seg.min() < seg.max()     # (one sample is all there is to be constant)
    # the image is the last `ring` samples, global sample j at j mod ring
    img = lm.ring_image(data[0], ring)
    n = data.shape[1]
    assert img[(n - 1) % ring] == data[0, n - 1] and img[n % ring] == data[0, n - ring]


def test_event_array():
    ev = lm.event_array(lm.ring_events(lm.RING_COMPACT)[:3], 30)
    assert ev["tick"].tolist() == [30, 30, 30] and (ev["length"] > 0).all()
