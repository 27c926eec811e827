"""Shared by the stream-snapshot GPU tests: the A / B / C scheme.

Data: lifecycle_util.streams(6, block, 4100) (235 ticks at block 1600).  Engine A takes all of it
in lockstep: its events and final states are the expectation (the existing tests tie A to the
oracle).  Engine B takes the first k ticks and is polled, then exported.  Engine C has 9 streams
and has been pushed C_PRE lockstep ticks of other audio (so its clock differs from the records'
and tick_delta is exercised); it imports the six records into slots SLOTS and gets the remaining
ticks through push_streams.  With C's slots mapped back, B's events followed by C's must equal
A's under lifecycle_util.assert_events_equal (every field, ring_start included, and the score's
bits), and every stream's final state() must equal A's.
"""
import numpy as np

import lifecycle_util as lu
from golden_io import matcher_fixture, template_arrays

N, NC = 6, 9
SLOTS = [7, 2, 5, 0, 8, 3]
SEED = 4100
C_PRE = 13
VIAS = ("host", "bytes", "move")
IN_SILENCE, IN_SOUND, AFTER_SOUND = 1, 2, 3

_template = []
_cache = {}


def template():
    if not _template:
        fx, _ = matcher_fixture()
        _template.append(template_arrays(fx))
    return _template[0]


def make_case(name, block=1600, cfg=None, pcm16=False, setup=None, rate=None, own_template=True):
    """A geometry and what is pushed into it, computed once per name.  src / other: the samples as
    pushed (int16 for PCM16 pushes, at `rate` when one is set) of the six streams and of C's
    earlier audio; setup(engine): tables, rate and whatever else an engine of the case needs."""
    if name in _cache:
        return _cache[name]
    data = lu.streams(N, block, SEED)
    other = lu.streams(NC, block, SEED + 5200)[:, :C_PRE * block]
    in_block = block
    if pcm16:
        data, other = lu.to_pcm16(data)[0], lu.to_pcm16(other)[0]
    if rate:
        import resample_gpu_util as ru
        in_block = ru.in_block_of(rate, block)
        assert in_block % block == 0
        data, other = (np.repeat(x, in_block // block, axis=1) for x in (data, other))   # zero-order hold
    case = dict(name=name, block=block, in_block=in_block, cfg=dict(cfg or {}), pcm16=pcm16, setup=setup, rate=rate,
                src=np.ascontiguousarray(data), other=np.ascontiguousarray(other), n_ticks=data.shape[1] // in_block,
                own_template=own_template)
    _cache[name] = case
    return case


def odd_rows_case():
    """An int16 compact ring whose rows are not a multiple of 16 bytes: block 500, 81 blocks, 81,000
    bytes a row -- every other row starts 8 bytes past a 16-byte boundary, so its copy has a head
    and a tail of 2-byte pieces and 16-byte stores fed from 8-byte-aligned loads.  (Rows at the
    2- and 4-byte phases need an odd number of samples a row, which the engine's ring
    initialisation takes only for stream counts that are a multiple of 4 or 2.)"""
    ring = lu.min_ring(500)
    assert ring == 40500 and (2 * ring) % 16 == 8
    return make_case("i16_b500_odd_rows", block=500, cfg=dict(ring_samples=ring, ring_format=1), pcm16=True)


def engine(case, n):
    from easywakeword_amd import StreamEngine
    eng = StreamEngine(n, block=case["block"], tick_seconds=case["block"] / 16000, **case["cfg"])
    if case["own_template"]:
        eng.set_template(*template())
    if case["rate"]:
        eng.set_input_rate(case["rate"])
    if case["setup"]:
        case["setup"](eng)
    return eng


def step_of(case):
    return 7 * max(1, 1600 // case["block"])   # ticks per push


def push_lockstep(eng, case, src, t0, t1):
    """Ticks [t0, t1) of every stream, a tick for all of them at a time; returns the events."""
    ib, out = case["in_block"], []
    for t in range(t0, t1, step_of(case)):
        rows = src[:, t * ib:min(t + step_of(case), t1) * ib]
        (eng.push_pcm16 if case["pcm16"] else eng.push_many)(rows)
        out.append(eng.poll())
    return np.concatenate(out) if out else eng.poll()


def push_listed(eng, case, streams, src, t0, t1):
    """The same through push_streams: row i goes to streams[i]."""
    ib, out = case["in_block"], []
    for t in range(t0, t1, step_of(case)):
        rows = src[:, t * ib:min(t + step_of(case), t1) * ib]
        (eng.push_streams_pcm16 if case["pcm16"] else eng.push_streams)(streams, rows)
        out.append(eng.poll())
    return np.concatenate(out) if out else eng.poll()


def push_packets(eng, case, streams, src, s0, s1, packet=320):
    """Samples [s0, s1) of every row in packets of `packet` samples through push_chunks."""
    fn = eng.push_chunks_pcm16 if case["pcm16"] else eng.push_chunks
    out = []
    for at in range(s0, s1, 16 * packet):
        for p in range(at, min(at + 16 * packet, s1), packet):
            fn(streams, [r[p:min(p + packet, s1)] for r in src])
        out.append(eng.poll())
    return np.concatenate(out) if out else eng.poll()


def run_a(case):
    """Engine A, once per case: its events and the final state of every stream."""
    if "a" not in case:
        a = engine(case, N)
        ev = push_lockstep(a, case, case["src"], 0, case["n_ticks"])
        case["a"] = dict(ev=ev, state=[a.state(i) for i in range(N)],
                         lsn_state=[[a.listener_state(i, j) for j in range(len(a.stream_listeners(i)))] for i in range(N)])
        a.close()
    return case["a"]


def transfer(b, c, via, src_streams=None, slots=SLOTS):
    """The records of B's streams into C's slots, by one of the three ways; returns the meta array."""
    from easywakeword_amd import StreamSnapshot
    src_streams = list(range(N)) if src_streams is None else src_streams
    if via == "move":
        return b.move_streams(c, src_streams, slots)
    snap = b.export_streams(src_streams)
    if via == "bytes":
        snap = StreamSnapshot.frombytes(snap.tobytes())
    c.import_streams(slots, snap)
    return snap.meta


def map_back(ev, slots=SLOTS):
    """C's events as events of the streams the slots hold; an event of another slot fails."""
    out = ev.copy()
    inv = {s: i for i, s in enumerate(slots)}
    assert set(ev["stream"].tolist()) <= set(inv), sorted(set(ev["stream"].tolist()))
    out["stream"] = [inv[int(s)] for s in ev["stream"]]
    return out


def run_bc(case, k, via, b_desync=False, packets=False, extra=0):
    """Engines B and C of the scheme.  packets: B and C are fed 320-sample packets, and B is
    exported with `extra` samples of tick k + 1 pending.  Returns everything a test asserts on;
    the caller closes b and c."""
    src, ib, T = case["src"], case["in_block"], case["n_ticks"]
    b = engine(case, N)
    if packets:
        ev_b = push_packets(b, case, list(range(N)), src, 0, k * ib + extra)
    elif b_desync:
        ev_b = push_listed(b, case, list(range(N))[::-1], src[::-1], 0, k)
    else:
        ev_b = push_lockstep(b, case, src, 0, k)
    cut = [b.state(i) for i in range(N)]
    c = engine(case, NC)
    push_lockstep(c, case, case["other"], 0, C_PRE)
    meta = transfer(b, c, via)
    at_import = dict(ticks=c.stream_ticks(SLOTS).tolist(), pending=c.stream_pending(SLOTS).tolist(),
                     profiles=c.stream_profiles(SLOTS).tolist(), listeners=[c.stream_listeners(s) for s in SLOTS],
                     state=[c.state(s) for s in SLOTS], others=c.stream_ticks([1, 4, 6]).tolist())
    if packets:
        ev_c = push_packets(c, case, SLOTS, src, k * ib + extra, T * ib)
    else:
        ev_c = push_listed(c, case, SLOTS, src, k, T)
    at_end = dict(other_profiles=c.stream_profiles([1, 4, 6]).tolist(),
                  other_listeners=[c.stream_listeners(s) for s in (1, 4, 6)], n_blocks=c.snapshot_layout()["n_blocks"])
    return dict(b=b, c=c, ev_b=ev_b, ev_c=map_back(ev_c), cut=cut, meta=meta, at_import=at_import, at_end=at_end)


def assert_continues(case, r, k):
    """B's events followed by C's equal A's; every final state equals A's.  Returns the number of
    streams with an event after the cut."""
    a = run_a(case)
    assert (r["ev_b"]["tick"] <= k).all() and (r["ev_c"]["tick"] > k).all()
    total = lu.assert_events_equal(a["ev"], np.concatenate([r["ev_b"], r["ev_c"]]), N)
    assert total == len(a["ev"]) and total > 0
    c = r["c"]
    for i, s in enumerate(SLOTS):
        assert c.state(s) == a["state"][i], (i, s, c.state(s), a["state"][i])
        for j, want in enumerate(a["lsn_state"][i]):
            assert c.listener_state(s, j) == want, (i, s, j)
    assert c.stream_ticks(SLOTS).tolist() == [case["n_ticks"]] * N
    assert c.stream_ticks([1, 4, 6]).tolist() == [C_PRE] * 3          # the other slots: untouched
    assert r["at_import"]["ticks"] == [k] * N and r["at_import"]["others"] == [C_PRE] * 3
    assert r["at_import"]["state"] == r["cut"]
    return len(set(r["ev_c"]["stream"].tolist()))
