"""k_score_f32 (csrc/ewk_mfcc.hip) on the inputs of tests/scorer_matrix.py, through
Engine.score_device on linear batches (MODE 0), against oracle/mfcc_ref.py's float64 statistics of
the same float32 samples.  The template is reference_word.wav's, the threshold 75.

Bars, all the project's own:
  T > 16    template_drift(gpu statistics, oracle float64 statistics, candidate_stats()) <= 1e-4
            (template_cases.BAR: the statistics' error as what it moves a score by), every
            coefficient of mean and std within rtol 1e-4 / atol 2e-3, the score within 1e-4, the
            decision the oracle's
  T <= 16   the float32 mean / std -- what Engine.score, extract_mfcc and the bank pass hand on,
            although the fp64 re-score decides the score -- within rtol 1e-4 / atol 2e-3 of the
            float64 oracle; the final score within 1e-4, the decision identical; T = 1: std exactly
            0 and a NaN score
  D         the same bits as from a tightly packed buffer, whatever surrounds a segment
  E         the same bits alone, inside the batch and behind 2,100 other segments

tests/test_scorer_matrix.py shows on the CPU that the inputs meet the conditions under which these
bars are claimed, and that a wrong bin, band, frame, pad or clamp leaves them by a factor of 10.
Ring modes are out of scope (see tests/scorer_matrix.py).  Every test prints the worst figures per
family next to the oracle's own float32-against-float64 figures, and dumps the records of failing
cases (tests/evidence.py) before it asserts.
"""
import math

import numpy as np
import pytest

import evidence
import scorer_matrix as sm
import synth
from golden_io import score_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    import easywakeword_amd as ewa
    dev = torch.device("cuda", 0)
    eng = ewa.Engine()
    eng.template_from_pcm(synth.load_word())
    yield torch, dev, eng
    eng.close()


def score_layout(env, buf, offsets, lengths):
    """Engine.score_device on segments buf[offsets[i]:offsets[i] + lengths[i]] of one device buffer."""
    torch, dev, eng = env
    n = len(lengths)
    pcm = torch.from_numpy(np.array(buf, dtype=np.float32)).to(dev)      # (a copy: the layouts are read-only)
    off = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.int64)).to(dev)
    ln = torch.from_numpy(np.ascontiguousarray(lengths, dtype=np.int32)).to(dev)
    mean = torch.empty((n, 20), device=dev)
    std = torch.empty((n, 20), device=dev)
    score = torch.empty(n, device=dev, dtype=torch.float64)
    match = torch.empty(n, device=dev, dtype=torch.uint8)
    s = torch.cuda.current_stream(dev)
    eng.score_device(pcm.data_ptr(), off.data_ptr(), ln.data_ptr(), n, mean.data_ptr(), std.data_ptr(),
                     score.data_ptr(), match.data_ptr(), s.cuda_stream)
    torch.cuda.synchronize()
    return mean.cpu().numpy(), std.cpu().numpy(), score.cpu().numpy(), match.cpu().numpy().astype(bool)


def score_packed(env, segs):
    lengths = np.array([len(x) for x in segs], np.int32)
    offsets = np.zeros(len(segs), np.int64)
    offsets[1:] = np.cumsum(lengths[:-1], dtype=np.int64)
    buf = np.concatenate(segs) if lengths.sum() else np.zeros(1, np.float32)
    return score_layout(env, buf, offsets, lengths)


@pytest.fixture(scope="module")
def batch(env):
    """Families A, B and C in one batch."""
    return score_packed(env, [c.x for c in sm.cases()])


def _dscore(a, b):
    return 0.0 if math.isnan(a) and math.isnan(b) else abs(a - b)


def record(env, name, T, x_stats64, x_stats32, got):
    """One case against the oracle: the figures, and the bars it misses."""
    tmpl = env[2].get_template()
    mean, std, score, match = got
    cm, cs = x_stats64
    ref = sm.score_of(x_stats64, tmpl)
    r = dict(name=name, T=T, score=float(score), oracle_score=ref, match=bool(match),
             dmean=float(np.abs(mean - cm).max()), dstd=float(np.abs(std - cs).max()),
             dscore=_dscore(float(score), ref), coeff=sm.coeff_excess((mean, std), x_stats64),
             drift=sm.drift((mean, std), x_stats64) if T > 1 else 0.0,
             o_dmean=float(np.abs(x_stats32[0] - cm).max()), o_dstd=float(np.abs(x_stats32[1] - cs).max()),
             o_drift=sm.drift(x_stats32, x_stats64) if T > 1 else 0.0,
             o_dscore=_dscore(sm.score_of(x_stats32, tmpl), ref))
    miss = []
    if r["coeff"] > 1.0:
        miss.append("coefficients")
    if T > sm.SHORT_T and not r["drift"] <= sm.BAR:
        miss.append("drift")
    if not score_close(score, ref, sm.BAR):
        miss.append("score")
    if bool(match) != bool(ref >= sm.THRESHOLD):
        miss.append("decision")
    if T == 1 and (std.any() or not math.isnan(score)):
        miss.append("one frame: std 0, NaN score")
    r["miss"] = miss
    if miss:
        r.update(mean=mean, std=std, oracle_mean=cm, oracle_std=cs)
    return r


def report(what, records):
    """Print the worst figures of `records` (the GPU's, then the oracle's own float32 against its
    float64), dump the failing ones, assert that there are none."""
    for label, rows in (("T > 16", [r for r in records if r["T"] > sm.SHORT_T]),
                        ("T <= 16", [r for r in records if r["T"] <= sm.SHORT_T])):
        if rows:
            w = {k: max(r[k] for r in rows) for k in ("dmean", "dstd", "drift", "dscore", "coeff",
                                                      "o_dmean", "o_dstd", "o_drift", "o_dscore")}
            print(f"{what}, {label} ({len(rows)} cases): worst |dmean| {w['dmean']:.2e} |dstd| {w['dstd']:.2e} "
                  f"drift {w['drift']:.2e} |dscore| {w['dscore']:.2e} coefficient bar x {w['coeff']:.3f}; "
                  f"oracle float32 vs float64: |dmean| {w['o_dmean']:.2e} |dstd| {w['o_dstd']:.2e} "
                  f"drift {w['o_drift']:.2e} |dscore| {w['o_dscore']:.2e}")
    bad = [r for r in records if r["miss"]]
    if bad:
        path = evidence.dump("scorer_matrix", dict(what=what, failing=bad))
        print(f"{what}: {len(bad)} failing cases, records in {path}")
    assert not bad, [(r["name"], r["miss"], r["drift"], r["coeff"], r["dscore"]) for r in bad[:20]]


def family_records(env, batch, family):
    cs = sm.cases()
    return [record(env, c.name, c.T, sm.oracle(c), sm.oracle(c, "float32"), [a[i] for a in batch])
            for i, c in enumerate(cs) if c.family == family]


def test_a_spectral_sweep(env, batch):
    """One tone probe per FFT bin: the FFT's transpose and untangle pairs, every mel band's weights
    and read window, every chunk slot of the tile."""
    recs = family_records(env, batch, "A")
    assert [r["name"] for r in recs] == [f"A_k{k}" for k in range(257)]
    report("A spectral sweep", recs)


def test_b_frame_grid(env, batch):
    """T = 1 ... 40, 47, 48, 49 at rem 0, 1, 159, tones and clicks, and T = 767 ... 770."""
    recs = family_records(env, batch, "B")
    assert len(recs) == 4 * 43 * 3 + 4
    report("B frame grid, tone probes", [r for r in recs if "tone" in r["name"] or "long" in r["name"]])
    report("B frame grid, click probes", [r for r in recs if "click" in r["name"]])


def test_c_amplitude(env, batch):
    report("C amplitude", family_records(env, batch, "C"))


def _same_bits(a, b, what):
    for x, y, f in zip(a, b, ("mean", "std", "score", "match")):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        if x.dtype == np.float32:
            x, y = x.view(np.int32), y.view(np.int32)
        elif x.dtype == np.float64:
            x, y = x.view(np.int64), y.view(np.int64)
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: {f}")


def test_d_loud_filler_around_every_segment(env):
    """700 samples of a 0.9-amplitude filler before and after each segment, bases at 0, 1, 2, 3, 31,
    63 and odd offsets mod 64: only the range check keeps the filler out of the 256-sample pads."""
    cs = sm.d_cases()
    buf, offs, lens = sm.d_spaced_layout()
    spaced = score_layout(env, buf, offs, lens)
    packed = score_packed(env, [c.x for c in cs])
    recs = [record(env, c.name, c.T, sm.oracle(c), sm.oracle(c, "float32"), [a[i] for a in spaced])
            for i, c in enumerate(cs)]
    diff = [c.name for i, c in enumerate(cs)
            if not (np.array_equal(spaced[0][i].view(np.int32), packed[0][i].view(np.int32))
                    and np.array_equal(spaced[1][i].view(np.int32), packed[1][i].view(np.int32)))]
    print(f"D spaced: {len(cs)} segments, base offsets mod 64 {sorted(set((offs % 64).tolist()))}; "
          f"statistics that differ from the packed buffer's: {diff}")
    if diff:
        evidence.dump("scorer_matrix", dict(what="D spaced vs packed", differ=diff, offsets=offs, lengths=lens,
                                            spaced_mean=spaced[0], packed_mean=packed[0],
                                            spaced_std=spaced[1], packed_std=packed[1]))
    report("D pad and placement, spaced", recs)
    _same_bits(spaced, packed, "spaced vs packed")


def test_d_overlapping_segments(env):
    """Windows of one buffer, each starting 300 samples before the previous one ends (37 after its
    start where it is too short for that).  They are segments of their own, held to the conditions
    by tests/test_scorer_matrix.py and here to every bar, the drift above 16 frames included."""
    layout = sm.d_overlap_layout()
    wins = sm.windows(layout)
    over = score_layout(env, *layout)
    packed = score_packed(env, wins)
    recs = [record(env, f"window{i}_L{len(x)}", 1 + len(x) // 160, sm.stats_of(x), sm.stats_of(x, np.float32),
                   [a[i] for a in over]) for i, x in enumerate(wins)]
    report("D pad and placement, overlapping", recs)
    _same_bits(over, packed, "overlapping vs packed")


def test_e_batch_position(env, batch):
    """32 segments inside the A + B + C batch (786 segments on 792 waves: each wave's first claim, by
    grid index), each alone (wave 0), and at the end of a batch of 2,132 (the grid stops at 2,048
    waves: indices from 2,048 on are claimed from the work counter): the same bits."""
    cs = sm.cases()
    idx = sm.e_sample()
    sample = [cs[i].x for i in idx]
    inside = [a[idx] for a in batch]
    alone = [score_packed(env, [x]) for x in sample]
    alone = [np.concatenate([r[k] for r in alone]) for k in range(4)]
    pad = sm.e_pad_segment()
    behind = score_packed(env, [pad] * sm.E_PAD_N + sample)
    pads = [a[:sm.E_PAD_N] for a in behind]
    behind = [a[sm.E_PAD_N:] for a in behind]
    worst = max(_dscore(float(a), float(b)) for a, b in zip(inside[2], alone[2]))
    print(f"E: {[cs[i].name for i in idx]}; worst |score inside - alone| {worst:.3e}; "
          f"finite scores {int(np.isfinite(inside[2]).sum())} of {len(idx)}")
    _same_bits(alone, inside, "alone vs inside the batch")
    _same_bits(behind, inside, "behind 2,100 segments vs inside the batch")
    _same_bits([a[1:] for a in pads], [a[:-1] for a in pads], "the 2,100 copies among themselves")
