#!/usr/bin/env python3
"""Cost of subset pushes per streaming tick: 8,192 resident streams of bench.make_shifted_signal,
one tick per push (the real-time cadence, lagged polls), HIP events on the engine's stream around
every push, the cases alternated round by round in one process, an engine each:

  a  ewk_push_many: every stream, lockstep
  b  ewk_push_streams with the identity list
  c  ewk_push_streams with all streams in a random permutation
  d  ewk_push_streams with a random half of the streams
  e  ewk_push_streams with a random sixteenth

Row i of a push hears the signal from tick i on, whatever stream it feeds, so every case reads
the same memory per row.  After the timed rounds the same ticks run once more with the engine's
profiling on, for the gate's share of a tick (ewk_profile_read kind 2).  Prints one JSON line.

    python scripts/bench_push_streams.py [--streams 8192] [--rounds 5] [--ticks 40] [--cases abcde] [--out FILE]

(--cases a runs on a build without the stream-lifecycle calls: the parent-commit comparison.)
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
    ap.add_argument("--cases", default="abcde")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    import bench
    import easywakeword_amd as ewa

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    word = bench.load_word()
    n = args.streams
    keys = [k for k in "abcde" if k in args.cases]
    warm = 10                                       # untimed ticks after the prefill
    total = 100 + warm + (args.rounds + 1) * args.ticks
    sig = bench.make_shifted_signal(torch, dev, n, total, args.seed, word)

    probe = ewa.Engine()
    probe.template_from_pcm(word)
    tm, ts = probe.get_template()
    probe.close()

    rng = np.random.Generator(np.random.PCG64(args.seed))
    perm = rng.permutation(n).astype(np.int32)
    lists = {"a": None, "b": np.arange(n, dtype=np.int32), "c": perm,
             "d": rng.permutation(n)[: n // 2].astype(np.int32), "e": rng.permutation(n)[: n // 16].astype(np.int32)}

    engines, streams = {}, {}
    for k in keys:
        se = ewa.StreamEngine(n)
        se.set_template(tm, ts)
        engines[k] = se
        streams[k] = torch.cuda.ExternalStream(se.stream_handle(), device=dev)

    n_events = {k: 0 for k in keys}

    def ticks(k, t0, nt, per_call=1, timed=None):
        se, es = engines[k], streams[k]
        t = t0
        while t < t0 + nt:
            m = min(per_call, t0 + nt - t)
            if timed is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(es)
            if lists[k] is None:
                se.push_device(sig.data_ptr() + t * 1600 * 4, 1600, 1600, m)
            else:
                se.push_streams_device(lists[k], sig.data_ptr() + t * 1600 * 4, 1600, 1600, m)
            if timed is not None:
                e1.record(es)
                timed.append((e0, e1))
            n_events[k] += len(se.poll(lagged=True))
            t += m

    for k in keys:                                   # prefill (ring fill + detection start), then warm-up
        ticks(k, 0, 100, 32)
        ticks(k, 100, warm)
        engines[k].sync()
        n_events[k] = 0
    torch.cuda.synchronize()

    ms = {k: [] for k in keys}
    for r in range(args.rounds):
        for k in keys:
            ev = []
            ticks(k, 100 + warm + r * args.ticks, args.ticks, timed=ev)
            engines[k].sync()
            ms[k].append([a.elapsed_time(b) for a, b in ev])
    scored = dict(n_events)

    gate = {}
    for k in keys:                                   # one more round with the kernel families bracketed
        engines[k].profile(True)
        ticks(k, 100 + warm + args.rounds * args.ticks, args.ticks)
        engines[k].sync()
        g_ms, g_n = engines[k].profile_read(2)
        engines[k].profile(False)
        gate[k] = g_ms / max(1, g_n)

    res = {"streams": n, "rounds": args.rounds, "ticks_per_round": args.ticks, "cases": keys,
           "rows": {k: int(n if lists[k] is None else len(lists[k])) for k in keys},
           "events_per_tick": {k: scored[k] / (args.rounds * args.ticks) for k in keys}, "tick": {}}
    for k in keys:
        med = [float(np.median(r)) for r in ms[k]]
        tick = float(np.median(np.concatenate(ms[k])))
        res["tick"][k] = {"tick_ms_median": tick, "round_medians": [round(x, 5) for x in med],
                          "round_min": min(med), "round_max": max(med),
                          "gate_ms_per_launch": gate[k], "gate_share": gate[k] / tick}
    if "a" in keys:
        for k in keys:
            if k != "a":
                res[f"{k}_minus_a_ms"] = res["tick"][k]["tick_ms_median"] - res["tick"]["a"]["tick_ms_median"]
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
