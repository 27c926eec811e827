#!/usr/bin/env python3
"""Cost of packet ingest (ewk_push_chunks) per streaming tick: 8,192 resident streams of
bench.make_shifted_signal in device memory, lagged polls, HIP events on the engine's stream around
every tick's pushes, the cases alternated round by round in one process, an engine each:

  a  ewk_push_many: every stream, lockstep
  b  ewk_push_streams with the identity list
  c  ewk_push_chunks, exactly one block per stream, nothing pending
  d  ewk_push_chunks, five 320-sample packets per stream and tick: four pushes that only append
     and one that ticks; the sum of the five
  e  ewk_push_chunks, seeded random sizes from 160 to 4800 samples per stream, one push per
     100 ms (on average 1.55 ticks per stream and push); reported per push and per tick made

Stream i hears the signal from tick i on, in every case.  After the timed rounds the same pushes
run once more with the engine's profiling on: the gate's launches (ewk_profile_read kind 2) and
the assembly launch (kind 4) with its bytes -- per chunk pending + count samples read and as many
written, from the shapes -- over its time, against the 6.3 TB/s of a float4 copy.  One JSON line.

    python scripts/bench_push_chunks.py [--streams 8192] [--rounds 5] [--ticks 40] [--cases abcde] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BLOCK = 1600
COPY_TBS = 6.3      # float4 copy on the MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=8192)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=40, help="timed ticks (100 ms steps) per case and round")
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
    steps = (args.rounds + 1) * args.ticks
    total = 100 + 3 * (warm + steps) + 4            # (case e moves up to 3 ticks a step)
    sig = bench.make_shifted_signal(torch, dev, n, total, args.seed, word)
    n_pcm = int(sig.numel())

    probe = ewa.Engine()
    probe.template_from_pcm(word)
    tm, ts = probe.get_template()
    probe.close()

    ident = np.arange(n, dtype=np.int32)
    base = ident.astype(np.int64) * BLOCK           # stream i starts at tick i of the signal
    engines, streams, pos, rngs = {}, {}, {}, {}
    for k in keys:
        se = ewa.StreamEngine(n)
        se.set_template(tm, ts)
        engines[k] = se
        streams[k] = torch.cuda.ExternalStream(se.stream_handle(), device=dev)
        pos[k] = np.zeros(n, np.int64)              # samples delivered per stream
        rngs[k] = np.random.Generator(np.random.PCG64(args.seed + 1))

    n_events = {k: 0 for k in keys}
    moved = {k: 0 for k in keys}                    # samples through the assembly kernel (read; as many written)
    made = {k: 0 for k in keys}                     # ticks made, summed over the streams

    def chunk_push(k, counts):
        se = engines[k]
        pend = pos[k] % BLOCK
        se.push_chunks_device(ident, sig.data_ptr(), n_pcm, base + pos[k], counts)
        moved[k] += int((pend + counts).sum())
        made[k] += int(((pend + counts) // BLOCK).sum())
        pos[k] += counts

    def step(k):
        """100 ms of audio for every stream (case e: a random 10..300 ms)."""
        se = engines[k]
        t = int(pos[k][0] // BLOCK)
        if k == "a":
            se.push_device(sig.data_ptr() + t * BLOCK * 4, BLOCK, BLOCK, 1)
        elif k == "b":
            se.push_streams_device(ident, sig.data_ptr() + t * BLOCK * 4, BLOCK, BLOCK, 1)
        elif k == "c":
            chunk_push(k, np.full(n, BLOCK, np.int32))
        elif k == "d":
            for _ in range(5):
                chunk_push(k, np.full(n, 320, np.int32))
        else:
            chunk_push(k, rngs[k].integers(160, 4801, n).astype(np.int32))
        if k in "ab":
            pos[k] += BLOCK
            made[k] += n

    def run(k, nt, timed=None):
        se, es = engines[k], streams[k]
        for _ in range(nt):
            if timed is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(es)
            step(k)
            if timed is not None:
                e1.record(es)
                timed.append((e0, e1))
            n_events[k] += len(se.poll(lagged=True))

    for k in keys:                                   # prefill (ring fill + detection start) in lockstep, then warm-up
        for t in range(0, 100, 25):
            engines[k].push_device(sig.data_ptr() + t * BLOCK * 4, BLOCK, BLOCK, 25)
            engines[k].poll(lagged=True)
        pos[k] += 100 * BLOCK
        run(k, warm)
        engines[k].sync()
        n_events[k] = moved[k] = made[k] = 0
    torch.cuda.synchronize()

    ms = {k: [] for k in keys}
    for r in range(args.rounds):
        for k in keys:
            ev = []
            run(k, args.ticks, timed=ev)
            engines[k].sync()
            ms[k].append([a.elapsed_time(b) for a, b in ev])
    scored, ticks_made = dict(n_events), dict(made)

    prof = {}
    for k in keys:                                   # one more round with the kernel families bracketed
        engines[k].profile(True)
        moved[k] = 0
        run(k, args.ticks)
        engines[k].sync()
        g_ms, g_n = engines[k].profile_read(2)
        a_ms, a_n = engines[k].profile_read(4)
        engines[k].profile(False)
        prof[k] = dict(gate_ms=g_ms / args.ticks, gate_launches=g_n / args.ticks, asm_ms=a_ms / args.ticks,
                       asm_launches=a_n / args.ticks, asm_bytes=2 * 4 * moved[k] / args.ticks)

    n_steps = args.rounds * args.ticks
    res = {"streams": n, "rounds": args.rounds, "steps_per_round": args.ticks, "cases": keys,
           "events_per_step": {k: scored[k] / n_steps for k in keys},
           "ticks_per_stream_and_step": {k: ticks_made[k] / (n_steps * n) for k in keys}, "step": {}}
    for k in keys:
        med = [float(np.median(r)) for r in ms[k]]
        step_ms = float(np.median(np.concatenate(ms[k])))
        p = prof[k]
        row = {"step_ms_median": step_ms, "round_medians": [round(x, 5) for x in med], "round_min": min(med),
               "round_max": max(med), "ms_per_tick_made": step_ms / (ticks_made[k] / (n_steps * n)),
               "gate_ms_per_step": p["gate_ms"], "gate_launches_per_step": p["gate_launches"]}
        if p["asm_launches"]:
            tbs = p["asm_bytes"] / (p["asm_ms"] * 1e-3) / 1e12
            row.update({"assembly_ms_per_step": p["asm_ms"], "assembly_launches_per_step": p["asm_launches"],
                        "assembly_bytes_per_step": p["asm_bytes"], "assembly_tb_per_s": tbs,
                        "assembly_share_of_copy_rate": tbs / COPY_TBS})
        res["step"][k] = row
    for ref in ("a", "b"):
        if ref in keys:
            for k in keys:
                if k > ref:
                    res[f"{k}_over_{ref}"] = res["step"][k]["ms_per_tick_made"] / res["step"][ref]["ms_per_tick_made"]
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
