#!/usr/bin/env python3
"""Cost of detector profiles per streaming tick: 8,192 resident streams of bench.make_shifted_signal
(the configs[2] recipe), one lockstep tick per push (the real-time cadence, lagged polls), the cases
alternated round by round in one process, an engine each:

  a  no profile table (the gate without the profile code)
  b  a table of one profile equal to the engine's configuration, assigned to every stream
  c  a table of 16 profiles, assigned at random

The profiles of c differ from the configuration by 1..16 ms of speech_duration_max and are
otherwise equal to it, so all three cases gate (nearly) the same events and the difference is the
mechanism: the index and timing loads per stream-tick.  A round of a case is `--ticks` ticks timed
with HIP events on the engine's stream around every push (the tick), then as many with the
engine's profiling on for the gate launch alone (ewk_profile_read kind 2).  Prints one JSON line:
per case the median over all ticks, the per-round medians and their min..max.

    python scripts/bench_gate_profiles.py [--streams 8192] [--rounds 5] [--ticks 40] [--out FILE]
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
    ap.add_argument("--ticks", type=int, default=40, help="ticks per case, round and kind of timing")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    import bench
    import easywakeword_amd as ewa

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    word = bench.load_word()
    n = args.streams
    keys = ["a", "b", "c"]
    warm = 10                                       # untimed ticks after the prefill
    total = 100 + warm + args.rounds * 2 * args.ticks
    sig = bench.make_shifted_signal(torch, dev, n, total, args.seed, word)

    probe = ewa.Engine()
    probe.template_from_pcm(word)
    tm, ts = probe.get_template()
    probe.close()

    rng = np.random.Generator(np.random.PCG64(args.seed))
    tables = {"a": None, "b": [{}],
              "c": [dict(speech_duration_max=2.0 + 0.001 * (j + 1)) for j in range(16)]}
    assign = {"b": np.zeros(n, np.int32), "c": rng.integers(0, 16, n).astype(np.int32)}

    engines, streams = {}, {}
    for k in keys:
        se = ewa.StreamEngine(n)
        se.set_template(tm, ts)
        if tables[k] is not None:
            se.set_detector_profiles(tables[k])
            se.assign_stream_profiles(np.arange(n, dtype=np.int32), assign[k])
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
            se.push_device(sig.data_ptr() + t * 1600 * 4, 1600, 1600, m)
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

    tick_ms = {k: [] for k in keys}
    gate_ms = {k: [] for k in keys}
    for r in range(args.rounds):
        t0 = 100 + warm + r * 2 * args.ticks
        for k in keys:
            ev = []
            ticks(k, t0, args.ticks, timed=ev)
            engines[k].sync()
            tick_ms[k].append([a.elapsed_time(b) for a, b in ev])
        for k in keys:                               # the same cases with the gate launches bracketed
            engines[k].profile(True)
            ticks(k, t0 + args.ticks, args.ticks)
            engines[k].sync()
            g_ms, g_n = engines[k].profile_read(2)
            engines[k].profile(False)
            gate_ms[k].append(g_ms / max(1, g_n))

    res = {"streams": n, "rounds": args.rounds, "ticks_per_round": args.ticks,
           "cases": {"a": "no table", "b": "one profile, every stream", "c": "16 profiles, assigned at random"},
           "events_per_tick": {k: n_events[k] / (args.rounds * 2 * args.ticks) for k in keys}, "tick": {}, "gate": {}}
    for k in keys:
        med = [float(np.median(r)) for r in tick_ms[k]]
        res["tick"][k] = {"ms_median": float(np.median(np.concatenate(tick_ms[k]))),
                          "round_medians": [round(x, 5) for x in med], "round_min": min(med), "round_max": max(med)}
        g = gate_ms[k]
        res["gate"][k] = {"ms_per_launch_median": float(np.median(g)), "rounds": [round(x, 6) for x in g],
                          "round_min": min(g), "round_max": max(g)}
    for k in "bc":
        res[f"tick_{k}_minus_a_ms"] = res["tick"][k]["ms_median"] - res["tick"]["a"]["ms_median"]
        res[f"gate_{k}_minus_a_ms"] = res["gate"][k]["ms_per_launch_median"] - res["gate"]["a"]["ms_per_launch_median"]
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
