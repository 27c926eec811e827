"""Stream snapshots carry every per-stream feature: the A / B / C scheme of snapshot_util.py at
k = 191 with an input rate (resampler history and fresh flag, B in lockstep and desynchronised),
packet ingest (B exported with a partial block pending), a stream bank with a word per stream, a
detector-profile table with a profile per stream, and three listeners per stream.  C has the same
tables set before the import; the imported profiles, words and listeners equal B's."""
import numpy as np
import pytest

import bank_cases as bc
import listener_cases as lc
import profile_cases as pc
import snapshot_util as su

pytestmark = pytest.mark.gpu

K = 191
WORDS = [2, 0, 1, 1, 2, 0]                    # stream i listens for word WORDS[i] of the 3-word bank
PROFILES = [1, -1, 0, 2, 1, 0]                # ... and is gated with profile PROFILES[i] of the first three
LISTENERS = [lc.rows((-1, 0, 1), (0, 1, 2)), lc.rows((2, 1, 0), (1, 1, 0)), lc.rows((0, -1, 2), (2, 0, 1)),
             lc.rows((1, 2, -1), (0, 2, 2)), lc.rows((-1, 1, 0), (1, 0, 0)), lc.rows((0, 2, 1), (2, 1, 0))]
THRESHOLDS = (96.0, 92.0, 86.0)


def finish(case, r, k=K):
    try:
        print(f"{case['name']}: events B {len(r['ev_b'])} C {len(r['ev_c'])}")
        after = su.assert_continues(case, r, k)
        assert after >= 1
        return r
    finally:
        r["b"].close()
        r["c"].close()


def per_slot(values):
    """What every slot of C holds after the import: B's value of the stream moved there."""
    return [values[i] for i in range(su.N)]


@pytest.mark.parametrize("b_desync", [False, True], ids=["lockstep", "desynchronised"])
def test_input_rate(b_desync):
    """48 kHz pushes: the record carries the resampler's history row and the fresh flag -- from
    rs_fresh while B is in lockstep, from its per-stream flags once it is desynchronised."""
    case = su.make_case("rate48k", rate=48000)
    assert case["in_block"] == 4800
    r = finish(case, su.run_bc(case, K, "host", b_desync=b_desync))
    assert (r["meta"]["record_bytes"] == r["meta"]["record_bytes"][0]).all()


def test_input_rate_fresh_flag_before_the_first_push():
    """Streams exported before their first push are fresh: the first `delay` outputs of the
    importer are zero again, as A's were."""
    case = su.make_case("rate48k", rate=48000)
    a = su.run_a(case)
    b, c = su.engine(case, su.N), su.engine(case, su.NC)
    try:
        su.push_lockstep(c, case, case["other"], 0, su.C_PRE)       # C's own flags are cleared by its pushes
        su.transfer(b, c, "host")
        ev_c = su.map_back(su.push_listed(c, case, su.SLOTS, case["src"], 0, case["n_ticks"]))
        import lifecycle_util as lu
        assert lu.assert_events_equal(a["ev"], ev_c, su.N) == len(a["ev"]) > 0
    finally:
        b.close()
        c.close()


@pytest.mark.parametrize("via", ["host", "move"])
def test_packet_ingest_with_a_partial_block_pending(via):
    """B is fed 320-sample packets and exported 640 samples into tick 192; C continues with packets."""
    case = su.make_case("f32_full")
    r = su.run_bc(case, K, via, packets=True, extra=640)
    assert r["b"].stream_pending().tolist() == [640] * su.N
    assert r["at_import"]["pending"] == [640] * su.N and r["meta"]["pending"].tolist() == [640] * su.N
    assert r["c"].stream_pending([1, 4, 6]).tolist() == [0, 0, 0]
    finish(case, r)
    assert r["at_import"]["ticks"] == [K] * su.N


def test_packet_ingest_int16_ring():
    case = su.make_case("i16_compact", cfg=dict(ring_samples=su.lu.min_ring(1600), ring_format=1), pcm16=True)
    r = su.run_bc(case, K, "host", packets=True, extra=37)
    assert r["at_import"]["pending"] == [37] * su.N
    finish(case, r)


def bank_setup(eng):
    eng.bank_from_pcm(bc.bank_audio(), thresholds=THRESHOLDS)
    eng.set_stream_bank(None)


def test_stream_bank_word_per_stream():
    """B's streams listen for WORDS; C's bank is enabled with word 0 everywhere: the import
    assigns the words, and the events carry the bank's scores and best templates."""
    def with_words(eng):
        bank_setup(eng)
        if eng.n_streams == su.N:
            eng.assign_stream_words(list(range(su.N)), WORDS)
    case = su.make_case("bank", setup=with_words, own_template=False)
    r = finish(case, su.run_bc(case, K, "host"))
    assert r["meta"]["word"].tolist() == WORDS
    assert [l[0][1] for l in r["at_import"]["listeners"]] == per_slot(WORDS)
    from easywakeword_amd import _lib
    assert (r["ev_c"]["flags"] & _lib.EWK_EV_BANK).any()


def profile_setup(eng):
    eng.set_detector_profiles(pc.PROFILES[:3])
    if eng.n_streams == su.N:
        eng.assign_stream_profiles(list(range(su.N)), PROFILES)


def test_detector_profile_per_stream():
    case = su.make_case("profiles", setup=profile_setup)
    r = finish(case, su.run_bc(case, K, "host"))
    assert r["meta"]["profile"].tolist() == PROFILES
    assert r["at_import"]["profiles"] == per_slot(PROFILES)
    assert r["at_end"]["other_profiles"] == [-1, -1, -1]


def listener_setup(eng):
    eng.bank_from_pcm(bc.bank_audio(), thresholds=THRESHOLDS)
    eng.set_stream_bank(None)
    eng.set_detector_profiles(pc.PROFILES[:3])
    if eng.n_streams == su.N:
        eng.set_stream_listeners(list(range(su.N)), LISTENERS)


@pytest.mark.parametrize("via", ["host", "move"])
def test_three_listeners_per_stream(via):
    """Every stream has three (profile, word) listeners; C has the tables but no listeners yet:
    the import allocates them, and every listener's detector continues where it was."""
    case = su.make_case("listeners", setup=listener_setup, own_template=False)
    r = finish(case, su.run_bc(case, K, via))
    assert r["meta"]["n_listeners"].tolist() == [3] * su.N
    assert r["at_import"]["listeners"] == per_slot(LISTENERS)
    assert r["at_end"]["other_listeners"] == [[(-1, 0)]] * 3
    seen = set(lc.listener_of(np.concatenate([r["ev_b"], r["ev_c"]])).tolist())
    assert seen == {0, 1, 2}, seen


def test_import_without_the_tables_is_refused_and_changes_nothing():
    """A record pointing into a table the destination does not have: ValueError naming the record
    and the table, and C exports what it exported before."""
    case = su.make_case("listeners", setup=listener_setup, own_template=False)
    plain = su.make_case("f32_full")
    b, c = su.engine(case, su.N), su.engine(plain, su.NC)
    try:
        su.push_lockstep(b, case, case["src"], 0, 14)
        su.push_lockstep(c, plain, plain["other"], 0, su.C_PRE)
        snap = b.export_streams(list(range(su.N)))
        before = c.export_streams(list(range(su.NC)))
        with pytest.raises(ValueError, match=r"record 0 \(for stream 7\), listener 1: profile 0 .*detector-profile table"):
            c.import_streams(su.SLOTS, snap)
        c.set_detector_profiles(pc.PROFILES[:3])
        with pytest.raises(ValueError, match=r"record 0 \(for stream 7\), listener 1: word 1 .*stream bank is off"):
            c.import_streams(su.SLOTS, snap)
        after = c.export_streams(list(range(su.NC)))
        assert before.meta.tobytes() == after.meta.tobytes() and before.payload.tobytes() == after.payload.tobytes()
        assert c.stream_ticks().tolist() == [su.C_PRE] * su.NC
        assert [c.stream_listeners(s) for s in range(su.NC)] == [[(-1, 0)]] * su.NC
    finally:
        b.close()
        c.close()
