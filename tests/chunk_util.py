"""Shared by the packet-ingest GPU tests (push_chunks): the seeded chunk schedule and the runner
that delivers it from host or device memory and checks ticks and pending after every push."""
import numpy as np


def sizes(block):
    return [0, 1, 160, 320, 480, block - 1, block, block + 1, 2 * block + 7, 5 * block]


def schedule(n, length, block, seed, size_set=None, first_push=None, prologue=True):
    """A seeded delivery of `length` samples to each of n streams, every stream's samples in order:
    a list of pushes, each a list of (stream, start, count).  Per push a random subset of the
    streams that still have samples (1, n/2, n - 1 or n of them, shuffled); per stream a size drawn
    from size_set (default sizes(block): mean at least half a block), cut at the stream's end.
    With `prologue` every stream starts with [block - 1, block, block, 1]: the second chunk finds
    pending = block - 1, makes one tick and leaves block - 1 again -- old and new carry overlap in
    all but one sample.  first_push: {stream: count}, delivered before anything else."""
    rng = np.random.default_rng(seed)
    size_set = list(size_set or sizes(block))
    assert np.mean(size_set) >= block / 2
    pro = [block - 1, block, block, 1] if prologue else []
    done = np.zeros(n, np.int64)
    step = np.zeros(n, np.int64)
    out = []
    if first_push:
        out.append([(s, 0, c) for s, c in first_push.items()])
        for s, c in first_push.items():
            done[s] += c
    subset_sizes = sorted({1, max(1, n // 2), max(1, n - 1), n})
    while (done < length).any():
        cand = np.flatnonzero(done < length)
        k = min(int(rng.choice(subset_sizes)), len(cand))
        push = []
        for s in rng.permutation(cand)[:k]:
            want = pro[step[s]] if step[s] < len(pro) else int(rng.choice(size_set))
            c = int(min(want, length - done[s]))
            push.append((int(s), int(done[s]), c))
            done[s] += c
            step[s] += 1
        out.append(push)
    return out


def device_buffer(src, push, phases, fill=9):
    """The chunks of one push in one device buffer, chunk k starting at a sample offset congruent to
    phases[k % len(phases)] modulo 16 (gaps hold a value no stream holds, so a read from a gap shows
    in the ring).  Returns (torch tensor, offsets, counts)."""
    import torch
    offs, at = [], 0
    for k, (_, _, c) in enumerate(push):
        at = (at + 15) // 16 * 16 + phases[k % len(phases)]
        offs.append(at)
        at += c
    buf = np.full(at + 16, fill, src.dtype)
    for (s, a, c), o in zip(push, offs):
        buf[o:o + c] = src[s, a:a + c]
    return torch.from_numpy(buf).to(torch.device("cuda", 0)), offs, [c for _, _, c in push]


def run(eng, src, block, sched, where="host", pcm16=False, phases=(0,), poll_every=16):
    """Deliver a schedule to `eng` through push_chunks / push_chunks_pcm16 (where="host") or
    push_chunks_device; after every push stream_ticks() and stream_pending() are the delivered
    samples divided by, and modulo, `block` (the input block).  Returns the polled events."""
    n = eng.n_streams
    delivered = np.zeros(n, np.int64)
    got, keep = [], []
    for k, push in enumerate(sched):
        streams = [s for s, _, _ in push]
        if where == "host":
            chunks = [src[s, a:a + c] for s, a, c in push]
            (eng.push_chunks_pcm16 if pcm16 else eng.push_chunks)(streams, chunks)
        else:
            buf, offs, counts = device_buffer(src, push, phases)
            eng.push_chunks_device(streams, buf.data_ptr(), buf.numel(), offs, counts, pcm16=pcm16)
            keep.append(buf)
        for s, _, c in push:
            delivered[s] += c
        np.testing.assert_array_equal(eng.stream_ticks(), delivered // block, err_msg=f"push {k}")
        np.testing.assert_array_equal(eng.stream_pending(), delivered % block, err_msg=f"push {k}")
        if k % poll_every == poll_every - 1:
            got.append(eng.poll())
            eng.sync()          # the device buffers of the pushes so far have been read
            keep.clear()
    got.append(eng.poll())
    eng.sync()
    return np.concatenate(got), delivered
