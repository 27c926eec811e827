"""Shared by the stream-listener tests: the recipes, the CPU oracle's event lists per (stream,
profile) -- oracle/gate_ref.py through profile_cases.run, one run per pair -- the properties of
those lists that make the recipes tell listeners apart, and the per-listener comparisons.

A listener is a pair (detector profile, word).  The profiles are profile_cases.PROFILES; the five
listeners of the main recipe are the engine's configuration (-1) and the table's four entries.
"""
import numpy as np

import lifecycle_util as lu
import profile_cases as pc
from golden_io import score_close
from oracle import mfcc_ref
from oracle.gate_ref import DetectorRef

BLOCK = pc.BLOCK
LISTENERS = (-1, 0, 1, 2, 3)          # main recipe: every stream has these five
GEOMETRY_LISTENERS = (-1, 0, 1, 3)
LISTENER_MASK = 15 << 16              # EWK_EV_LISTENER bits of ewk_event.flags
FILL = 100                            # ticks until the 10 s ring is full (block 1600)

GEOMETRIES = {
    # name: (block, seed, PCM16 pushes, engine config, oracle events, skipped, ticks)
    "b1600_i16_compact": (1600, 8900, True,
                          dict(ring_format=1, ring_samples=lu.min_ring(1600, 2.4, 0.5, 0.1)), 31, 4, 232),
    "b400_regs8": (400, 8700, False, {}, 30, 8, 978),
    "b250_memory": (250, 8802, False, {}, 29, 8, 1470),
}

_cache = {}


def oracle_lists(data, streams, profiles, block=BLOCK, keep_audio=True):
    """{(stream, profile): the oracle's events}, one run per pair."""
    return {(s, p): pc.run(data[s], pc.gate_config(p, block), keep_audio=keep_audio)
            for s in streams for p in profiles}


def run_entered(pcm, cfg, enter_at):
    """The oracle with a new _detect_word call made after `enter_at` ticks (what reenter(stream)
    does, and how a listener added to a running stream starts): the entry check on the buffer as
    it stands, the events before it dropped."""
    det = DetectorRef(cfg, keep_audio=False)
    det.buf = pc.MemoBuffer(cfg.buffer_seconds)
    for k in range(len(pcm) // cfg.block):
        if k == enter_at and det.started:
            det._enter()
        det.push_tick(pcm[k * cfg.block:(k + 1) * cfg.block])
    return [e for e in det.events if e.tick > enter_at]


def main_case():
    """Streams 0..3 of the 12-stream recipe with the five listeners: data (all 12 streams),
    n_ticks, ref[(stream, profile)]."""
    if "main" not in _cache:
        data = pc.main_case()["data"]
        _cache["main"] = dict(data=data, n_ticks=data.shape[1] // BLOCK,
                              ref=oracle_lists(data, range(4), LISTENERS))
    return _cache["main"]


def same_tick_cuts(ref, stream, profiles):
    """Ticks at which every listed profile cuts an event on `stream`."""
    ticks = [set(e.tick for e in ref[(stream, p)]) for p in profiles]
    return sorted(set.intersection(*ticks))


def assert_main_recipe(case):
    """What the oracle's lists must show before an engine is looked at: no test on them passes
    with listeners ignored (all lists of a stream equal) or with one listener per stream."""
    ref = case["ref"]
    assert case["n_ticks"] == 231
    assert sum(len(r) for r in ref.values()) == 49
    skipped = {k: sum(e.skipped for e in r) for k, r in ref.items()}
    assert sum(skipped.values()) == 7
    assert all(v == 0 for (s, p), v in skipped.items() if p != 1)   # profile 1: max_segment_seconds 0.8
    assert [skipped[(s, 1)] for s in range(4)] == [0, 4, 1, 2]
    counts = [[len(ref[(s, p)]) for p in LISTENERS] for s in range(4)]
    assert counts == [[3, 3, 3, 2, 3], [4, 4, 4, 2, 4], [1, 1, 1, 1, 1], [3, 3, 3, 0, 3]], counts
    for s in range(4):
        keys = [tuple(pc.key(ref[(s, p)])) for p in LISTENERS]
        assert len(set(keys)) >= 4, s
    assert 161 in same_tick_cuts(ref, 0, (-1, 1, 2)) and 191 in same_tick_cuts(ref, 0, (-1, 1, 2))
    assert 161 in same_tick_cuts(ref, 2, (-1, 1, 2))


def geometry_case(name):
    """Two streams with the listeners (-1, 0, 1, 3) at another block size / ring format: src (what
    is pushed), data (the float32 values it decodes to), ref[(stream, profile)]."""
    if name not in _cache:
        block, seed, pcm16, cfg, n_events, n_skipped, n_ticks = GEOMETRIES[name]
        data = lu.streams(2, block, seed)
        src = data
        if pcm16:
            src, data = lu.to_pcm16(data)
        ref = oracle_lists(data, range(2), GEOMETRY_LISTENERS, block)
        assert data.shape[1] // block == n_ticks
        assert sum(len(r) for r in ref.values()) == n_events
        assert sum(e.skipped for r in ref.values() for e in r) == n_skipped
        for s in range(2):
            keys = [tuple(pc.key(ref[(s, p)])) for p in GEOMETRY_LISTENERS]
            assert len(set(keys)) == 4, (name, s)
        if name == "b1600_i16_compact":
            both = [sum(1 for t, c in _tick_counts(ref, s).items() if c > 1) for s in range(2)]
            assert both == [5, 6], both
        _cache[name] = dict(block=block, pcm16=pcm16, cfg=cfg, src=src, data=data, ref=ref, n_ticks=n_ticks)
    return _cache[name]


def _tick_counts(ref, stream):
    out = {}
    for (s, p), r in ref.items():
        if s == stream:
            for e in r:
                out[e.tick] = out.get(e.tick, 0) + 1
    return out


def rows(profiles, words=None):
    """A stream's listener list: (profile, word) pairs."""
    return [(int(p), int(words[j]) if words is not None else 0) for j, p in enumerate(profiles)]


def listener_of(ev):
    return (ev["flags"] >> 16) & 15


def by_listener(ev, streams, n_listeners):
    """{(stream, j): its events in tick order}."""
    lj = listener_of(ev)
    out = {}
    for s in streams:
        for j in range(n_listeners):
            m = ev[(ev["stream"] == s) & (lj == j)]
            out[(s, j)] = m[np.argsort(m["tick"], kind="stable")]
    return out


def as_streams(ev, width):
    """Events of (stream s, listener j) as events of stream width * s + j without listener bits:
    what an engine with one stream per listener produces."""
    out = ev.copy()
    out["stream"] = width * ev["stream"] + listener_of(ev)
    out["flags"] = ev["flags"] & ~LISTENER_MASK
    return out


def check_oracle(mine, ref, template, budget):
    """One listener's events against the oracle's list: (tick, length, skipped) and time equal;
    while budget[0] > 0 the scored events within 1e-4 of oracle/mfcc_ref (the project's bar) with
    equal decisions.  Returns (events, scores compared)."""
    tm, ts = template
    assert pc.engine_key(mine) == pc.key(ref), (pc.engine_key(mine), pc.key(ref))
    np.testing.assert_array_equal(mine["time"], np.array([e.time for e in ref], np.float64))
    n_sc = 0
    for m, e in zip(mine, ref):
        if e.skipped or e.audio is None or budget[0] <= 0:
            continue
        cm, cs = mfcc_ref.extract_mfcc(e.audio)
        s = float(mfcc_ref.similarity_from_stats(tm, ts, cm, cs))
        assert score_close(float(m["score"]), s, 1e-4), (e.tick, float(m["score"]), s)
        assert bool(m["match"]) == (s >= 75.0), e.tick
        budget[0] -= 1
        n_sc += 1
    return len(ref), n_sc
