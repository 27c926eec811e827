#!/usr/bin/env python3
"""Cost of stream listeners per streaming tick, beside the alternative without them.

Streams hear bench.make_shifted_signal (the configs[2] recipe), one lockstep tick per push (the
real-time cadence, lagged polls), the cases alternated round by round in one process, an engine each:

  a    8,192 streams, no listeners (the gate without the listener code)
  l4   8,192 streams, 4 listeners each
  l16  8,192 streams, 16 listeners each
  s4   32,768 streams fed 4 copies of the audio, stream 4 r + j on profile j: what 4 words per
       microphone cost without listeners

Listener j (and profile j of s4) differs from the configuration by j ms of speech_duration_max and
is otherwise equal to it, so every listener gates (nearly) the events of case a and the cases
differ by the mechanism and by the number of events scored.  A round of a case is `--ticks` ticks
timed with HIP events on the engine's stream around every push (the tick), then as many with the
engine's profiling on for the gate launch alone (ewk_profile_read kind 2).  Device memory is the
drop of free memory (hipMemGetInfo) over the creation and configuration of the case's engine.
Prints one JSON line: per case the median over all ticks, the per-round medians, their min..max.

    python scripts/bench_listeners.py [--streams 8192] [--rounds 5] [--ticks 20] [--warm 40] [--cases a,l4,l16,s4] [--out FILE]

The comparison with the parent commit (case a and bench.py's value) is scripts/bench_vs_parent.py.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"a": "8192 streams, no listeners", "l4": "4 listeners per stream", "l16": "16 listeners per stream",
         "s4": "4x the streams, 4 copies of the audio, a profile each"}


def measure(args):
    import torch
    import bench
    import easywakeword_amd as ewa

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    word = bench.load_word()
    n = args.streams
    keys = [k for k in args.cases.split(",") if k]
    warm = args.warm                                # untimed ticks after the prefill
    total = 100 + warm + args.rounds * 2 * args.ticks
    sig = bench.make_shifted_signal(torch, dev, n, total, args.seed, word)
    copies = None
    if "s4" in keys:   # row 4 r + j = stream r's audio, materialised: [4 n, total * 1600]
        rows = torch.as_strided(sig, (n, total * 1600), (1600, 1))
        copies = rows.repeat_interleave(4, dim=0).contiguous()

    probe = ewa.Engine()
    probe.template_from_pcm(word)
    tm, ts = probe.get_template()
    probe.close()

    table = [dict(speech_duration_max=2.0 + 0.001 * (j + 1)) for j in range(16)]
    engines, streams, mem = {}, {}, {}
    for k in keys:
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info(0)[0]
        m = 4 * n if k == "s4" else n
        se = ewa.StreamEngine(m)
        se.set_template(tm, ts)
        if k != "a":
            se.set_detector_profiles(table)
        if k == "s4":
            se.assign_stream_profiles(np.arange(m, dtype=np.int32), (np.arange(m) % 4 - 1).astype(np.int32))
        elif k != "a":
            c = int(k[1:])
            se.set_stream_listeners(np.arange(m, dtype=np.int32), [[j - 1 for j in range(c)]] * m)
        se.sync()
        mem[k] = free0 - torch.cuda.mem_get_info(0)[0]
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
            if k == "s4":
                se.push_device(copies.data_ptr() + t * 1600 * 4, copies.shape[1], 1600, m)
            else:
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

    res = {"streams": n, "rounds": args.rounds, "ticks_per_round": args.ticks, "warm_ticks": warm, "cases": {k: CASES[k] for k in keys},
           "events_per_tick": {k: n_events[k] / (args.rounds * 2 * args.ticks) for k in keys},
           "device_bytes": mem, "tick": {}, "gate": {}}
    for k in keys:
        med = [float(np.median(r)) for r in tick_ms[k]]
        res["tick"][k] = {"ms_median": float(np.median(np.concatenate(tick_ms[k]))),
                          "round_medians": [round(x, 5) for x in med], "round_min": min(med), "round_max": max(med)}
        g = gate_ms[k]
        res["gate"][k] = {"ms_per_launch_median": float(np.median(g)), "rounds": [round(x, 6) for x in g],
                          "round_min": min(g), "round_max": max(g)}
    for e in engines.values():
        e.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=8192)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=20, help="ticks per case, round and kind of timing")
    ap.add_argument("--warm", type=int, default=40,
                    help="untimed ticks after the 100 of the prefill: the first segments are cut ~20 ticks after the ring fills")
    ap.add_argument("--cases", default="a,l4,l16,s4")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    res = measure(args)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
