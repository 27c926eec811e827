"""Stream snapshots, the continuation test (the scheme is in snapshot_util.py): six streams
exported from engine B after k ticks and imported into slots [7, 2, 5, 0, 8, 3] of a nine-stream
engine C, which is on another clock, go on producing exactly what engine A, which got everything,
produces -- through a host payload, through tobytes / frombytes and through move_streams.

Cut ticks (block 1600): k = 191, where the CPU oracle has the six streams in InSound, InSound,
InSilence, AfterSound, InSilence, InSound and an event of stream 3 at tick 192; k = 40, rings not
full, detection not started; k = 100, the tick at which the ring fills and the pointer wraps.
Rings at k = 191: float32 full, float32 compact, int16 compact (PCM16 pushes), block 512 (312
blocks, rows of the full ring not a multiple of the block) and block 311: 514 blocks, the largest
block with more than the 512 the gate keeps in registers, so the sorted copy is the
memory-resident one with its two halves (the smallest block the engine accepts, 1, would make
376,000 ticks of this data)."""
import pytest

import lifecycle_util as lu
import snapshot_util as su

pytestmark = pytest.mark.gpu

RINGS = {
    # name: (block, engine config, PCM16 pushes)
    "f32_full": (1600, {}, False),
    "f32_compact": (1600, dict(ring_samples=lu.min_ring(1600)), False),
    "i16_compact": (1600, dict(ring_samples=lu.min_ring(1600), ring_format=1), True),
    "b512_full": (512, {}, False),
    "b311_memory_sorted": (311, {}, False),
    "i16_b500_odd_rows": (500, None, True),     # snapshot_util.odd_rows_case: rows 8 bytes off a 16-byte boundary
}


def case_of(ring):
    block, cfg, pcm16 = RINGS[ring]
    if cfg is None:
        return su.odd_rows_case()
    return su.make_case(ring, block=block, cfg=cfg, pcm16=pcm16)


def run(ring, k, via, **kw):
    case = case_of(ring)
    r = su.run_bc(case, k, via, **kw)
    try:
        states = [s["state"] for s in r["cut"]]
        print(f"{ring} k={k} {via}: states at the cut {states}, events B {len(r['ev_b'])} C {len(r['ev_c'])}, "
              f"C's ticks {sorted(set(r['ev_c']['tick'].tolist()))}")
        after = su.assert_continues(case, r, k)
        return case, r, after
    finally:
        r["b"].close()
        r["c"].close()


@pytest.mark.parametrize("via", su.VIAS)
def test_cut_in_the_middle_of_words(via):
    """k = 191: streams in the middle of a word, one a tick before its event, one that never
    produces an event and carries only its threshold history."""
    case, r, after = run("f32_full", 191, via)
    assert case["n_ticks"] == 235
    states = [s["state"] for s in r["cut"]]
    assert su.AFTER_SOUND in states and su.IN_SOUND in states
    assert after >= 5
    assert all(s["started"] == 1 for s in r["cut"])


@pytest.mark.parametrize("via", su.VIAS)
def test_cut_before_the_ring_is_full(via):
    """k = 40: started == 0 and 64,000 samples collected; the imported streams enter at A's tick."""
    case, r, _ = run("f32_full", 40, via)
    assert all(s["started"] == 0 and s["samples_collected"] == 64000 for s in r["cut"])
    a = su.run_a(case)
    assert min(int(t) for t in a["ev"]["tick"]) > 100


@pytest.mark.parametrize("via", su.VIAS)
def test_cut_at_the_tick_the_ring_fills(via):
    """k = 100: the ring has just filled and the pointer has wrapped to 0."""
    case, r, _ = run("f32_full", 100, via)
    assert all(s["samples_collected"] == 160000 and s["pointer"] == 0 for s in r["cut"])


@pytest.mark.parametrize("ring", [r for r in RINGS if r != "f32_full"])
@pytest.mark.parametrize("via", ["host", "move"])
def test_other_rings(ring, via):
    """k = 191 (the same second of audio at other blocks) for every ring kind."""
    block = RINGS[ring][0]
    k = round(191 * 1600 / block)
    case, r, after = run(ring, k, via)
    assert all(s["started"] == 1 for s in r["cut"])
    if block == 1600:
        states = [s["state"] for s in r["cut"]]
        assert su.AFTER_SOUND in states and su.IN_SOUND in states
        assert after >= 5
    else:
        assert after >= 1   # (another block is another gate: the oracle's states at the cut were checked at block 1600 only)
    if ring == "b311_memory_sorted":
        assert r["at_end"]["n_blocks"] == 514


def test_desynchronised_source_and_a_subset():
    """B on its own clocks (fed through push_streams), and only streams 4 and 1 moved, into slots
    0 and 8 of C: they continue, B's other streams and C's other slots are untouched."""
    case = case_of("f32_full")
    a = su.run_a(case)
    k = 191
    b, c = su.engine(case, su.N), su.engine(case, su.NC)
    try:
        ev_b = su.push_listed(b, case, list(range(su.N))[::-1], case["src"][::-1], 0, k)
        su.push_lockstep(c, case, case["other"], 0, su.C_PRE)
        su.transfer(b, c, "host", [4, 1], [0, 8])
        ev_c = su.map_back(su.push_listed(c, case, [0, 8], case["src"][[4, 1]], k, case["n_ticks"]), [0, 8])
        want = a["ev"][(a["ev"]["stream"] == 4) | (a["ev"]["stream"] == 1)].copy()
        want["stream"] = [0 if s == 4 else 1 for s in want["stream"]]
        got_b = ev_b[(ev_b["stream"] == 4) | (ev_b["stream"] == 1)].copy()
        got_b["stream"] = [0 if s == 4 else 1 for s in got_b["stream"]]
        import numpy as np
        assert lu.assert_events_equal(want, np.concatenate([got_b, ev_c]), 2) == len(want) > 0
        assert c.state(0) == a["state"][4] and c.state(8) == a["state"][1]
        assert b.stream_ticks().tolist() == [k] * su.N                     # export is a read
        rest = su.push_listed(b, case, list(range(su.N)), case["src"], k, case["n_ticks"])
        lu.assert_events_equal(a["ev"], np.concatenate([ev_b, rest]), su.N)
    finally:
        b.close()
        c.close()
