"""Stream bank on the GPU (ewk_stream_bank_enable, k_bank_events in csrc/ewk_bank.hip): the
streaming engine scores every gated event against all templates of its stream's word, on the
device and in the same push.

Bar: the oracle's events (tick, length, skipped); the best score within 1e-4 of the oracle's
maximum over the word's templates (NaN == NaN), 1e-9 when every event goes through fp64; the
decision at the word's threshold and the best template exact (a best template within
bank_cases.TIE of the oracle's best is the 1e-4 bar's own ambiguity).

Inputs (all tests but the last): the three-word bank of tests/bank_cases.py (1, 3 and 64
templates), thresholds 90 / 93 / 99.5, and 12 synthetic PCM16 streams listening for word
i % 3.  With the CPU oracle alone they give 26 events on 10 of the streams: word 0 has 6 (best
85.27..99.90, nearest to its threshold 90.62), word 1 has 10 (83.53..93.41, nearest 93.048),
word 2 has 10 (98.74..99.97, nearest 99.718; each with one NaN template score: the NaN skip);
no best score within 1e-3 of its threshold, every top-2 gap at least 8e-4.  The streams, the
oracle's events and their scores are computed once and shared.
"""
import numpy as np
import pytest

import bank_cases as bc
import synth
from golden_io import score_close
from oracle import mfcc_ref
from oracle.gate_ref import GateConfig, run_stream

pytestmark = pytest.mark.gpu

THRESHOLDS = (90.0, 93.0, 99.5)
GATE = dict(pre_speech_silence=0.8, speech_duration_min=0.3, speech_duration_max=2.0, post_speech_silence=0.4)
N = 12
FIRST = np.concatenate([[0], np.cumsum(bc.SIZES)])
N_EVENTS = 26


def make_streams():
    """float32 [12, L] PCM16-exact streams, their int16 samples and stream_word."""
    pcms = []
    for i in range(N):
        rng = np.random.default_rng(900 + i)
        p, _ = synth.make_stream(seed=4000 + i, n_words=3, sigma=float(rng.uniform(1e-4, 3e-3)),
                                 gain=float(rng.uniform(0.3, 2.0)), distractors=bool(i % 2))
        pcms.append(synth.pcm16_roundtrip(p))
    L = max(len(p) for p in pcms)            # whole streams (196..211 ticks), the shorter ones zero-padded:
    assert L % 1600 == 0                     # every stream's own events, and no others
    data = np.zeros((N, L), np.float32)
    for i, p in enumerate(pcms):
        data[i, :len(p)] = p
    q = np.round(data.astype(np.float64) * 32768.0).astype(np.int16)
    assert np.array_equal(q.astype(np.float32) / np.float32(32768.0), data)
    return data, q, np.arange(N, dtype=np.int32) % 3


def oracle_events(data, word, tm, ts):
    """Per stream: the oracle's events, each with its scores[64] against its word's templates."""
    out = []
    for i in range(len(data)):
        evs = run_stream(data[i], GateConfig(**GATE)).events
        w = int(word[i])
        rows = []
        for e in evs:
            sc = np.full(64, np.nan)
            if not e.skipped:
                cm, cs = mfcc_ref.extract_mfcc(e.audio)
                for j in range(bc.SIZES[w]):
                    k = FIRST[w] + j
                    sc[j] = float(mfcc_ref.similarity_from_stats(tm[k], ts[k], cm, cs))
            rows.append(sc)
        out.append((evs, rows))
    return out


@pytest.fixture(scope="module")
def scorer():
    """A scorer engine holding the bank: its templates are every engine's (same pipeline)."""
    from easywakeword_amd import Engine
    e = Engine()
    e.bank_from_pcm(bc.bank_audio(), thresholds=THRESHOLDS)
    yield e
    e.close()


@pytest.fixture(scope="module")
def case(scorer):
    data, q, word = make_streams()
    tpl = [scorer.bank_template(k) for k in range(68)]
    tm, ts = np.array([m for m, _ in tpl]), np.array([s for _, s in tpl])
    return dict(data=data, q=q, word=word, tm=tm, ts=ts, ref=oracle_events(data, word, tm, ts))


def _engine(ring, **extra):
    from easywakeword_amd import StreamEngine
    kw = dict(GATE)
    if ring == "i16":
        kw.update(ring_format=1, ring_samples=48000)
    kw.update(extra)
    return StreamEngine(N, **kw)


def _run(eng, case, ring, segments=False):
    """Push 8 ticks at a time and poll; with segments=True every event's samples are read back
    right after its poll (the ring still holds them)."""
    src = case["q"] if ring == "i16" else case["data"]
    got, segs = [], []
    for c in range(0, src.shape[1], 8 * 1600):
        if ring == "i16":
            eng.push_pcm16(src[:, c:c + 8 * 1600])
        else:
            eng.push_many(src[:, c:c + 8 * 1600])
        ev = eng.poll()
        got.append(ev)
        if segments:
            segs.extend(eng.read_segment(int(e["stream"]), int(e["ring_start"]), int(e["length"])) for e in ev)
    return np.concatenate(got), segs


def _bank_engine(case, ring, **extra):
    eng = _engine(ring, **extra)
    eng.bank_from_pcm(bc.bank_audio(), thresholds=THRESHOLDS)
    eng.set_stream_bank(case["word"])
    return eng


@pytest.fixture(scope="module")
def f32_run(case):
    """The float32-ring run of test 1, with every event's segment read back."""
    eng = _bank_engine(case, "f32")
    ev, segs = _run(eng, case, "f32", segments=True)
    eng.close()
    return ev, segs


def _check(ev, case, tol, exact_best, need_rescored=False):
    from easywakeword_amd import _lib
    n_ev, worst, bad = 0, 0.0, []
    for i, (ref, rows) in enumerate(case["ref"]):
        mine = ev[ev["stream"] == i]
        mine = mine[np.argsort(mine["tick"], kind="stable")]
        assert [(int(m["tick"]), int(m["length"]), bool(m["flags"] & 1)) for m in mine] == \
               [(e.tick, e.length, e.skipped) for e in ref], i
        w = int(case["word"][i])
        for m, e, sc in zip(mine, ref, rows):
            n_ev += 1
            if e.skipped:
                assert not (int(m["flags"]) & _lib.EWK_EV_BANK), (i, m)
                continue
            flags, score = int(m["flags"]), float(m["score"])
            assert flags & _lib.EWK_EV_BANK, (i, m)
            if need_rescored:
                assert flags & _lib.EWK_EV_RESCORED or np.isnan(score), (i, m)
            if np.all(np.isnan(sc)):
                assert np.isnan(score) and not m["match"], (i, m)
                continue
            best = float(np.nanmax(sc))
            print(f"stream {i} tick {int(m['tick'])}: score {score!r} oracle {best!r} diff {abs(score - best):.3g} "
                  f"best {_lib.event_best_template(flags)} oracle {int(np.nanargmax(sc))} flags {flags:#x}")
            if not score_close(score, best, tol):
                bad.append((i, int(m["tick"]), score, best))
                continue
            worst = max(worst, abs(score - best))
            assert bool(m["match"]) == (best >= THRESHOLDS[w]), (i, m, best)
            got = int(_lib.event_best_template(flags))
            assert got < bc.SIZES[w], (i, m)
            if exact_best:
                assert got == int(np.nanargmax(sc)), (i, m, sc[:bc.SIZES[w]])
            else:
                assert sc[got] >= best - bc.TIE, (i, m, got, sc[got], best)
    print(f"{n_ev} events, max |score - oracle| = {worst:.3g}")
    assert not bad, bad
    assert n_ev == N_EVENTS
    return n_ev


@pytest.mark.parametrize("ring", ["f32", "i16"])
def test_stream_bank_vs_oracle(case, f32_run, ring):
    if ring == "f32":
        ev = f32_run[0]
    else:
        eng = _bank_engine(case, ring)
        ev, _ = _run(eng, case, ring)
        eng.close()
    assert len(ev) == N_EVENTS
    _check(ev, case, 1e-4, exact_best=False)


def test_stream_bank_rescore_all(case):
    """rescore_margin = 1e9: every event is listed, gets its fp64 statistics from the re-score
    launch and its score again from k_bank_events<double>."""
    eng = _bank_engine(case, "f32", rescore_margin=1e9)
    ev, _ = _run(eng, case, "f32")
    eng.close()
    _check(ev, case, 1e-9, exact_best=True, need_rescored=True)


def test_stream_bank_matches_batch_bank(case, f32_run, scorer):
    """Every event of test 1 against the batch bank on its own segment, read back from the ring."""
    from easywakeword_amd import _lib
    ev, segs = f32_run
    assert len(ev) == len(segs) == N_EVENTS
    for m, seg in zip(ev, segs):
        w = int(case["word"][int(m["stream"])])
        res = scorer.score_bank([seg.astype(np.float64)], word=[w])
        print(f"stream {int(m['stream'])} tick {int(m['tick'])}: stream {float(m['score'])!r} "
              f"batch {float(res['best_score'][0])!r}")
        assert score_close(float(m["score"]), float(res["best_score"][0]), 2e-4), (m, res)
        assert bool(m["match"]) == bool(res["match"][0]), (m, res)
        if not np.isnan(m["score"]):
            assert int(_lib.event_best_template(int(m["flags"]))) == int(res["best_tmpl"][0]) - int(FIRST[w]), (m, res)


def test_enable_disable_and_errors(case):
    from easywakeword_amd import Engine, _lib
    word = synth.load_word()
    eng = _engine("f32")
    with pytest.raises(ValueError, match="No reference word set"):      # EWK_ENOTEMPLATE
        eng.set_stream_bank()
    eng.bank_from_pcm(bc.bank_audio(), thresholds=THRESHOLDS)
    with pytest.raises(ValueError, match="outside"):
        eng.set_stream_bank(np.full(N, 3, np.int32))
    with pytest.raises(ValueError):
        eng.set_stream_bank(np.zeros(N + 1, np.int32))
    scorer_only = Engine()
    scorer_only.bank_from_pcm(bc.bank_audio())
    with pytest.raises(ValueError, match="no streams"):
        check = _lib.check
        check(scorer_only._lib.ewk_stream_bank_enable(scorer_only._h, None))
    scorer_only.close()
    eng.set_stream_bank(case["word"])                 # no single template set: works
    eng.set_stream_bank(case["word"])                 # (again: replaces the words)
    for call in (lambda: eng.set_bank([[eng.bank_template(0)]]), lambda: eng.bank_from_pcm([[word]]), eng.clear_bank):
        with pytest.raises(ValueError, match="disable the stream bank first"):
            call()
    assert eng.bank_info() == (3, 68)
    half = case["data"][:, : 160 * 1600]              # some pushes with the bank on, then a reset
    eng.push_many(half)
    ev = eng.poll()
    assert len(ev) and all(int(f) & _lib.EWK_EV_BANK for f in ev["flags"] if not f & 1)
    eng.reset()                                       # (keeps the enable state)
    with pytest.raises(ValueError, match="disable the stream bank first"):
        eng.clear_bank()
    eng.clear_stream_bank()
    eng.clear_stream_bank()                           # no-op when off
    eng.template_from_pcm(word)
    plain = _engine("f32")
    plain.template_from_pcm(word)
    a, _ = _run(eng, case, "f32")
    b, _ = _run(plain, case, "f32")
    assert len(a) == len(b) == N_EVENTS
    assert not np.any(a["flags"] & _lib.EWK_EV_BANK)
    assert a.tobytes() == b.tobytes()                 # field for field, score bits included
    eng.clear_bank()                                  # allowed again
    assert eng.bank_info() == (0, 0)
    eng.close()
    plain.close()


# ---------------------------------------------------------------- one segment per wave
N_WAVE = 65536        # kRingWaveStreams: the smallest count that selects ring mode 2
TICKS = 250


def _run_wave(sig, setup):
    from easywakeword_amd import StreamEngine
    se = StreamEngine(N_WAVE, ring_samples=48000)
    aux = setup(se)
    got = []
    for t in range(TICKS):
        se.push_device(sig.data_ptr() + t * 1600 * 4, 1600, 1600, 1)
        got.append(se.poll(lagged=True))
    got.append(se.poll())
    se.close()
    ev = np.concatenate(got)
    return ev[np.lexsort((ev["stream"], ev["tick"]))], aux


def test_stream_bank_one_segment_per_wave():
    import torch
    import bench
    from easywakeword_amd import _lib
    dev = torch.device("cuda", 0)
    word = bench.load_word()
    sig = bench.make_shifted_signal(torch, dev, N_WAVE, TICKS, 4321, word)
    sword = np.arange(N_WAVE, dtype=np.int32) % 3

    def bank3(se):
        se.bank_from_pcm(bc.bank_audio(), thresholds=THRESHOLDS)
        se.set_stream_bank(sword)
        tpl = [se.bank_template(k) for k in range(68)]
        return np.array([m for m, _ in tpl]), np.array([s for _, s in tpl])

    ev, (tm, ts) = _run_wave(sig, bank3)
    rng = np.random.default_rng(11)
    sample = sorted(set([0, 1, 2, 32767, 32768, N_WAVE - 2, N_WAVE - 1] + rng.choice(N_WAVE, 9, replace=False).tolist()))
    n_events = n_scored = 0
    for sid in sample:
        audio = sig[sid * 1600:(sid + TICKS) * 1600].cpu().numpy()
        ref = run_stream(audio, GateConfig()).events
        mine = ev[ev["stream"] == sid]
        assert [(int(m["tick"]), int(m["length"]), bool(m["flags"] & 1)) for m in mine] == \
               [(e.tick, e.length, e.skipped) for e in ref], sid
        n_events += len(ref)
        w = int(sword[sid])
        for m, e in zip(mine, ref):
            if e.skipped:
                continue
            cm, cs = mfcc_ref.extract_mfcc(e.audio)
            sc = np.array([float(mfcc_ref.similarity_from_stats(tm[FIRST[w] + j], ts[FIRST[w] + j], cm, cs))
                           for j in range(bc.SIZES[w])])
            flags, score = int(m["flags"]), float(m["score"])
            assert flags & _lib.EWK_EV_BANK, (sid, m)
            n_scored += 1
            if np.all(np.isnan(sc)):
                assert np.isnan(score) and not m["match"], (sid, m)
                continue
            best = float(np.nanmax(sc))
            print(f"stream {sid} tick {int(m['tick'])}: score {score!r} oracle {best!r}")
            assert score_close(score, best, 1e-4), (sid, int(m["tick"]), score, best)
            assert bool(m["match"]) == (best >= THRESHOLDS[w]), (sid, m, best)
            got = int(_lib.event_best_template(flags))
            assert got < bc.SIZES[w] and sc[got] >= best - bc.TIE, (sid, m, got, best)
    assert n_events >= 16 and n_scored >= 10

    def bank1(se):       # a 1 x 1 bank of the engine's own template, the engine's threshold
        se.template_from_pcm(word)
        se.set_bank([[se.get_template()]])
        se.set_stream_bank()

    one, _ = _run_wave(sig, bank1)
    single, _ = _run_wave(sig, lambda se: se.template_from_pcm(word))
    del sig
    torch.cuda.empty_cache()
    assert len(one) == len(single) > N_WAVE // 4
    for f in ("stream", "tick", "length", "match"):
        np.testing.assert_array_equal(one[f], single[f], err_msg=f)
    np.testing.assert_array_equal(one["flags"] & 1, single["flags"] & 1)
    scored = (single["flags"] & 1) == 0
    assert np.all(one["flags"][scored] & _lib.EWK_EV_BANK) and not np.any(single["flags"] & _lib.EWK_EV_BANK)
    a, b = one["score"], single["score"]
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(a)
    print("max |1x1 bank - single| =", float(np.max(np.abs(a[ok] - b[ok]))))
    assert float(np.max(np.abs(a[ok] - b[ok]))) <= 2e-4
