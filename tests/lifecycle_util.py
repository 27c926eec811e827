"""Shared by the stream-lifecycle GPU tests (push_streams / reset_streams): the stream recipe of
test_gpu_compact_ring.py, the seeded subset schedule, and the per-stream event comparison."""
import numpy as np

import synth

EVENT_FIELDS = ("tick", "length", "ring_start", "time", "flags", "match")


def streams(n, block, seed0, n_words=4):
    """test_gpu_compact_ring._streams: n float32 streams, cut to a whole number of blocks."""
    pcms = []
    for i in range(n):
        rng = np.random.default_rng(seed0 + i)
        p, _ = synth.make_stream(seed=seed0 + 1000 + i, n_words=n_words, sigma=float(rng.uniform(1e-4, 4e-3)),
                                 gain=float(rng.uniform(0.3, 2.5)), distractors=bool(i % 2), block=block)
        pcms.append(p)
    L = min(len(p) for p in pcms)
    L -= L % block
    return np.stack([p[:L] for p in pcms]).astype(np.float32)


def min_ring(block, max_speech=2.0, post=0.4, pad=0.05):
    """test_gpu_compact_ring._min_ring: the smallest compact ring of a config."""
    need = int((max_speech + post + block / 16000 + pad) * 16000) + 2 + block
    return -(-need // block) * block


def to_pcm16(data):
    """(int16 samples, the float32 values they decode to)."""
    q = np.clip(np.round(data.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)
    return q, q.astype(np.float32) / np.float32(32768.0)


def schedule(n, n_ticks, seed, sizes=None, max_ticks=7, done=None):
    """A seeded random delivery of n_ticks ticks to each of n streams: a list of (subset, nt,
    first) -- the streams of one push in shuffled order, its 1..max_ticks ticks, and the tick each
    listed stream is at.  Subset sizes are drawn from {1, n/2, n - 1, n} (capped by the streams that
    still have ticks to get); every stream's blocks go in order until all have had all of them."""
    rng = np.random.default_rng(seed)
    sizes = sizes or sorted({1, max(1, n // 2), max(1, n - 1), n})
    done = np.zeros(n, np.int64) if done is None else np.array(done, np.int64)
    out = []
    while (done < n_ticks).any():
        cand = np.flatnonzero(done < n_ticks)
        k = min(int(rng.choice(sizes)), len(cand))
        sub = rng.permutation(cand)[:k].astype(np.int32)
        nt = int(min(int(rng.integers(1, max_ticks + 1)), (n_ticks - done[sub]).min()))
        out.append((sub, nt, done[sub].copy()))
        done[sub] += nt
    return out


def rows_of(data, sub, first, nt, block):
    """[len(sub), nt * block]: ticks first[i] .. first[i] + nt of stream sub[i]."""
    return np.stack([data[s, f * block:(f + nt) * block] for s, f in zip(sub, first)])


def by_stream(ev, n):
    """Events per stream, in tick order."""
    out = []
    for i in range(n):
        m = ev[ev["stream"] == i]
        out.append(m[np.argsort(m["tick"], kind="stable")])
    return out


def assert_events_equal(a, b, n, fields=EVENT_FIELDS):
    """Per stream: every field equal and the score's bits equal.  Returns the events compared."""
    total = 0
    for i, (x, y) in enumerate(zip(by_stream(a, n), by_stream(b, n))):
        assert len(x) == len(y), (i, x["tick"], y["tick"])
        for f in fields:
            np.testing.assert_array_equal(x[f], y[f], err_msg=f"stream {i} {f}")
        np.testing.assert_array_equal(x["score"].view(np.int64), y["score"].view(np.int64), err_msg=f"stream {i} score")
        total += len(x)
    return total
