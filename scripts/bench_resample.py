#!/usr/bin/env python3
"""Cost of the input-rate resampler per streaming tick: 8,192 resident streams, one tick per
device push (the real-time cadence, lagged polls), HIP events on the engine's stream around
every push, four cases alternated round by round in one process:

  a  16 kHz float32 (no input rate set: the push as it always was)
  b  48 kHz float32
  c  44.1 kHz float32
  d  48 kHz PCM16

Every engine hears the same signal: bench.make_shifted_signal at 16 kHz for a, linearly
interpolated to the case's rate for b, c, d (the words stay words, so the scoring load is
comparable; the events per tick are recorded).  After the timed rounds one more round runs with
the engine's profiler on: the resampler's own device time (ewk_profile_read kind 3, the
resample launch and the history save) and the bytes it moves, (input + output) / time, next to
the 8 TB/s HBM figure.  Prints one JSON line.

    python scripts/bench_resample.py [--streams 8192] [--rounds 5] [--ticks 40] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"a": (16000, False), "b": (48000, False), "c": (44100, False), "d": (48000, True)}
HBM_BYTES_PER_S = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=8192)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=40, help="timed ticks per case and round")
    ap.add_argument("--cases", default="abcd")
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
    warm = 10
    total = 100 + warm + (args.rounds + 1) * args.ticks
    sig16 = bench.make_shifted_signal(torch, dev, n, total, args.seed, word)

    def at_rate(rate, pcm16):
        if rate == 16000:
            x = sig16
        else:
            m = sig16.numel() // 1600 * (rate // 10)
            x = torch.nn.functional.interpolate(sig16.view(1, 1, -1), size=m, mode="linear",
                                                align_corners=False).view(-1).contiguous()
        if pcm16:
            x = torch.round(x * 32768.0).clamp_(-32768, 32767).to(torch.int16)
        return x

    probe = ewa.Engine()
    probe.template_from_pcm(word)
    tm, ts = probe.get_template()
    probe.close()

    engines, streams, sigs, blocks = {}, {}, {}, {}
    for k in keys:
        rate, pcm16 = CASES[k]
        se = ewa.StreamEngine(n)
        se.set_template(tm, ts)
        se.set_input_rate(rate)
        engines[k], sigs[k], blocks[k] = se, at_rate(rate, pcm16), se.input_block
        streams[k] = torch.cuda.ExternalStream(se.stream_handle(), device=dev)
    torch.cuda.synchronize()

    n_events = {k: 0 for k in keys}

    def ticks(k, t0, nt, per_call=1, timed=None):
        se, es, ib = engines[k], streams[k], blocks[k]
        push = se.push_device_pcm16 if CASES[k][1] else se.push_device
        esz = sigs[k].element_size()
        t = t0
        while t < t0 + nt:
            m = min(per_call, t0 + nt - t)
            if timed is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(es)
            push(sigs[k].data_ptr() + t * ib * esz, ib, ib, m)
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

    prof = {}
    for k in keys:                                   # one more round under the engine's profiler
        se = engines[k]
        se.profile(True)
        ticks(k, 100 + warm + args.rounds * args.ticks, args.ticks)
        se.sync()
        gate_ms, gate_n = se.profile_read(2)
        rs_ms, rs_n = se.profile_read(3)
        se.profile(False)
        prof[k] = {"gate_ms_per_tick": gate_ms / max(1, gate_n), "resample_launches": int(rs_n)}
        if rs_n:
            per = rs_ms / rs_n
            moved = n * (blocks[k] * sigs[k].element_size() + 1600 * 4)
            prof[k].update({"resample_ms_per_tick": per, "resample_bytes_per_tick": int(moved),
                            "resample_bytes_per_s": moved / (per * 1e-3),
                            "resample_share_of_hbm_peak": moved / (per * 1e-3) / HBM_BYTES_PER_S})

    res = {"streams": n, "rounds": args.rounds, "ticks_per_round": args.ticks, "cases": keys,
           "case_rates": {k: {"rate": CASES[k][0], "pcm16": CASES[k][1], "input_block": blocks[k]} for k in keys},
           "hbm_peak_bytes_per_s": HBM_BYTES_PER_S,
           "events_per_tick": {k: scored[k] / (args.rounds * args.ticks) for k in keys}, "tick": {}, "profile": prof}
    for k, runs in ms.items():
        med = [float(np.median(r)) for r in runs]
        res["tick"][k] = {"tick_ms_median": float(np.median(np.concatenate(runs))),
                          "round_medians": [round(x, 5) for x in med], "round_spread": float(max(med) - min(med))}
    if "a" in keys:
        a = res["tick"]["a"]["tick_ms_median"]
        for k in keys:
            if k != "a":
                res[f"{k}_minus_a_ms"] = res["tick"][k]["tick_ms_median"] - a
                res[f"{k}_over_a"] = res["tick"][k]["tick_ms_median"] / a
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
