"""The gate's persistent row loop under an index list: past kGateGridMax * 4 = 524,288 rows a
wave takes a second row, requests its first tick early (the next-row prefetch) and looks its
stream up again.  One engine of 524,288 + 64 streams with the smallest compact ring, pushed as one
subset push per tick with a fixed permutation of all streams; 256 sampled streams -- the last 64
rows' among them -- against the oracle: event ticks, lengths, and scores to 1e-4.
"""
import numpy as np
import pytest

import lifecycle_util as lu
import synth
from golden_io import matcher_fixture, score_close, template_arrays
from oracle import mfcc_ref
from oracle.gate_ref import GateConfig, run_stream

pytestmark = pytest.mark.gpu

N = 524288 + 64
BLOCK, TICKS, BUFFER = 1600, 90, 4


@pytest.mark.parametrize("pcm16", [True, False], ids=["i16_ring_load_vec", "f32_ring_dma_prefetch"])
def test_permuted_rows_past_the_grid(pcm16):
    """int16 compact ring: launch_gate <2, 3>, the load_vec path; float32 compact ring: <2, 2>, the
    dma_tick prefetch of the next row.  Took 3.5 s (int16) and 2.5 s (float32) on an MI355X, the
    oracle of the 256 streams included."""
    import torch
    import bench
    from easywakeword_amd import StreamEngine
    dev = torch.device("cuda", 0)
    tm, ts = template_arrays(matcher_fixture()[0])
    sig = bench.make_shifted_signal(torch, dev, N, TICKS, 4242, synth.load_word(), pcm16=pcm16)
    es = 2 if pcm16 else 4
    cfg = dict(buffer_seconds=BUFFER, ring_samples=lu.min_ring(BLOCK))
    if pcm16:
        cfg["ring_format"] = 1
    eng = StreamEngine(N, **cfg)
    eng.set_template(tm, ts)
    perm = np.random.default_rng(77).permutation(N).astype(np.int32)      # row i is stream perm[i]
    for t in range(TICKS):
        eng.push_streams_device(perm, sig.data_ptr() + t * BLOCK * es, BLOCK, BLOCK, 1, pcm16=pcm16)
    np.testing.assert_array_equal(eng.stream_ticks(perm[-3:]), [TICKS] * 3)
    ev = eng.poll()
    rows = np.unique(np.concatenate([np.arange(N - 64, N), np.arange(64),
                                     np.random.default_rng(78).integers(64, N - 64, 128)]))
    assert len(rows) >= 250
    ev = ev[np.isin(ev["stream"], perm[rows])]
    n_ev = n_sc = n_tail = 0
    for r in rows:
        x = sig[r * BLOCK:(r + TICKS) * BLOCK].cpu().numpy()
        if pcm16:
            x = x.astype(np.float32) / np.float32(32768.0)
        ref = run_stream(x, GateConfig(buffer_seconds=BUFFER)).events
        mine = ev[ev["stream"] == perm[r]]
        mine = mine[np.argsort(mine["tick"], kind="stable")]
        assert [(int(m["tick"]), int(m["length"]), bool(m["flags"] & 1)) for m in mine] == \
               [(e.tick, e.length, e.skipped) for e in ref], (r, perm[r])
        n_ev += len(ref)
        n_tail += len(ref) if r >= N - 64 else 0
        for m, e in zip(mine, ref):
            if e.skipped or (n_sc >= 24 and r < N - 64) or n_sc >= 40:
                continue
            cm, cs = mfcc_ref.extract_mfcc(e.audio)
            s = float(mfcc_ref.similarity_from_stats(tm, ts, cm, cs))
            assert score_close(float(m["score"]), s, 1e-4), (r, int(m["tick"]), float(m["score"]), s)
            n_sc += 1
    eng.close()
    print(f"{n_ev} events on {len(rows)} streams ({n_tail} on the last 64 rows), {n_sc} scores checked")
    assert n_ev >= 100 and n_tail >= 10 and n_sc >= 10
