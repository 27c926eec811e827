#!/usr/bin/env python3
"""Cost of the stream bank per streaming tick: 8,192 resident streams of
bench.make_shifted_signal, one tick per push (the real-time cadence, lagged polls), HIP events
on the engine's stream around every push, four cases alternated round by round in one process:

  a  the single template
  b  a stream bank of 1 word x 1 template
  c  a stream bank of 1 word x 64 templates
  d  a stream bank of 1,024 words x 8 templates, a random word per stream

Every engine hears the same ticks.  After the rounds every engine is fed silence until its
events stop, and the same alternation times empty ticks: what the bank's extra launches cost
when there is nothing to score.  Prints one JSON line.

    python scripts/bench_stream_bank.py [--streams 8192] [--rounds 5] [--ticks 40] [--cases abcd] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=8192)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=40, help="timed ticks per case and round")
    ap.add_argument("--empty-ticks", type=int, default=40, help="timed empty ticks per case and round")
    ap.add_argument("--cases", default="abcd", help="the cases to run (a alone needs no stream bank)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    import bench
    import easywakeword_amd as ewa

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    word = bench.load_word()
    n = args.streams
    keys = [k for k in "abcd" if k in args.cases]
    warm = 10                                       # untimed ticks after the prefill
    total = 100 + warm + args.rounds * args.ticks
    sig = bench.make_shifted_signal(torch, dev, n, total, args.seed, word)
    silence = torch.zeros(n * 1600, device=dev, dtype=torch.float32)

    probe = ewa.Engine()
    probe.template_from_pcm(word)
    tm, ts = probe.get_template()
    probe.close()

    def variants(k):   # the word and perturbed copies of it (scripts/bench_bank.py)
        r = np.random.Generator(np.random.PCG64(args.seed + k))
        return [(tm, ts)] + [((tm + r.normal(0, 2.0, 20)).astype(np.float32),
                              np.abs(ts + r.normal(0, 1.0, 20)).astype(np.float32)) for _ in range(k - 1)]

    v = variants(64)
    banks = {"b": [variants(1)], "c": [v], "d": [[v[(w + j) % 64] for j in range(8)] for w in range(1024)]}
    rng = np.random.Generator(np.random.PCG64(args.seed))
    stream_word = rng.integers(0, 1024, n).astype(np.int32)

    engines, streams = {}, {}
    for k in keys:
        se = ewa.StreamEngine(n)
        if k == "a":
            se.set_template(tm, ts)
        else:
            se.set_bank(banks[k])
            se.set_stream_bank(stream_word if k == "d" else None)
        engines[k] = se
        streams[k] = torch.cuda.ExternalStream(se.stream_handle(), device=dev)

    n_events = {k: 0 for k in keys}

    def ticks(k, src, t0, nt, per_call=1, timed=None, stride=1600):
        se, es = engines[k], streams[k]
        t = t0
        while t < t0 + nt:
            m = min(per_call, t0 + nt - t)
            if timed is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(es)
            se.push_device(src.data_ptr() + (t * 1600 * 4 if src is sig else 0), stride, 1600 if src is sig else 0, m)
            if timed is not None:
                e1.record(es)
                timed.append((e0, e1))
            n_events[k] += len(se.poll(lagged=True))
            t += m

    for k in keys:                                   # prefill (ring fill + detection start), then warm-up
        ticks(k, sig, 0, 100, 32)
        ticks(k, sig, 100, warm)
        engines[k].sync()
    torch.cuda.synchronize()

    def rounds(src, t0, nt):
        ms = {k: [] for k in keys}
        for r in range(args.rounds):
            for k in keys:
                ev = []
                ticks(k, src, t0 + r * nt if src is sig else 0, nt, timed=ev)
                engines[k].sync()
                ms[k].append([a.elapsed_time(b) for a, b in ev])
        return ms

    for k in keys:
        n_events[k] = 0
    busy = rounds(sig, 100 + warm, args.ticks)
    scored = dict(n_events)
    for k in keys:                                   # silence until the last segments are cut and scored
        ticks(k, silence, 0, 40)
        engines[k].sync()
        n_events[k] = 0
    empty = rounds(silence, 0, args.empty_ticks)
    stray = dict(n_events)                           # (0 everywhere: the empty ticks were empty)

    def summary(ms):
        out = {}
        for k, runs in ms.items():
            med = [float(np.median(r)) for r in runs]
            out[k] = {"tick_ms_median": float(np.median(np.concatenate(runs))), "round_medians": [round(x, 5) for x in med],
                      "round_spread": float(max(med) - min(med))}
        return out

    res = {"streams": n, "rounds": args.rounds, "ticks_per_round": args.ticks, "cases": keys,
           "events_per_tick": {k: scored[k] / (args.rounds * args.ticks) for k in keys},
           "events_in_empty_ticks": stray, "busy": summary(busy), "empty": summary(empty)}
    if "a" in keys:
        a_busy, a_empty = res["busy"]["a"]["tick_ms_median"], res["empty"]["a"]["tick_ms_median"]
        for k in keys:
            if k == "a":
                continue
            res[f"{k}_minus_a_ms"] = res["busy"][k]["tick_ms_median"] - a_busy
            res[f"{k}_over_a"] = res["busy"][k]["tick_ms_median"] / a_busy
            e = res["empty"][k]["tick_ms_median"]
            res[f"{k}_empty_extra_ms"] = e - a_empty
            res[f"{k}_empty_extra_share"] = (e - a_empty) / e
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    for e in engines.values():
        e.close()


if __name__ == "__main__":
    main()
