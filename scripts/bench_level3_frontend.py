#!/usr/bin/env python3
"""Cost of the level-3 front end: polled positives of the 8,192-stream recipe (bench.make_streams,
160 ticks, the newest matches -- still in the rings) to Whisper's [n, 80, 3000] input features,
three ways, alternated round by round in one process on one engine:

  torch        WhisperConfirm.log_mel(StreamEngine.normalize_events_device(events)): float32, the
               path the kernels can replace (30 s zero-filled buffers, 3,001-frame STFT)
  kernel_f32   StreamEngine.whisper_features_events(events)                    (csrc/ewk_whisper.hip)
  kernel_bf16  StreamEngine.whisper_features_events(events, dtype="bfloat16")  (what the model reads)

for 1, 64 and 512 positives.  Each timing is a host clock around one call that ends in a device
synchronise (the kernel path synchronises its stream before it returns), median / min / max over
the rounds after warm-up.  Peak extra device memory: for torch the allocator's peak above what was
allocated before the call (the output included); for the kernel paths the engine's scratch after
the call (the drop in free device memory not explained by torch's allocator; it only ever grows,
so sizes run in ascending order on a fresh engine per path) plus the output tensor.  The largest
difference between the kernel's float32 features and torch's is recorded beside the timings.
Prints one JSON line.

    python scripts/bench_level3_frontend.py [--streams 8192] [--rounds 7] [--sizes 1,64,512] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def positives(torch, bench, ewa, dev, n_streams, seed, word):
    """A fresh engine that has heard 160 ticks, and its matched events, newest first."""
    period, pcm = bench.make_streams(torch, dev, n_streams, seed, word)
    se = ewa.StreamEngine(n_streams)
    se.template_from_pcm(word)
    evs = []
    for t in range(0, 160, 32):
        se.push_device(pcm.data_ptr() + t * 1600 * 4, period * 1600, 1600, 32)
        evs.append(se.poll())
    ev = np.concatenate(evs)
    pos = ev[(ev["match"] != 0) & ((ev["flags"] & 1) == 0)]
    return se, pcm, pos[np.argsort(-pos["tick"], kind="stable")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=8192)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", default="1,64,512")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    import bench
    import easywakeword_amd as ewa
    from easywakeword_amd.confirm import WhisperConfirm

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    word = bench.load_word()
    sizes = sorted(int(s) for s in args.sizes.split(","))
    wc = WhisperConfirm(device=dev, max_new_tokens=2)

    def used():   # device memory in use that torch's allocator does not hold
        free, total = torch.cuda.mem_get_info()
        return total - free - torch.cuda.memory_reserved()

    # ---- memory: a fresh engine per kernel path, sizes ascending
    mem = {}
    for path, dtype in (("kernel_f32", "float32"), ("kernel_bf16", "bfloat16")):
        se, pcm, pos = positives(torch, bench, ewa, dev, args.streams, args.seed, word)
        assert len(pos) >= sizes[-1], (len(pos), sizes)
        torch.cuda.synchronize()
        base = used()
        for n in sizes:
            out = se.whisper_features_events(pos[:n], dtype=dtype)
            scratch = used() - base
            mem[f"{path}_{n}"] = {"engine_scratch_bytes": int(scratch), "output_bytes": out.numel() * out.element_size(),
                                  "peak_extra_bytes": int(scratch) + out.numel() * out.element_size()}
            del out
        se.close()
        del pcm
    se, pcm, pos = positives(torch, bench, ewa, dev, args.streams, args.seed, word)
    live = {n: int(np.minimum(3000, (np.minimum(pos[:n]["length"], 480000) + 199) // 160 + 1).sum()) for n in sizes}
    for n in sizes:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = wc.log_mel(se.normalize_events_device(pos[:n]))
        torch.cuda.synchronize()
        mem[f"torch_{n}"] = {"peak_extra_bytes": int(torch.cuda.max_memory_allocated() - base),
                             "output_bytes": out.numel() * out.element_size()}
        del out

    # ---- time: the three paths alternated, one engine
    paths = {
        "torch": lambda ev: wc.log_mel(se.normalize_events_device(ev)),
        "kernel_f32": lambda ev: se.whisper_features_events(ev),
        "kernel_bf16": lambda ev: se.whisper_features_events(ev, dtype="bfloat16"),
    }
    res = {"streams": args.streams, "rounds": args.rounds, "sizes": sizes, "live_frames": live, "memory": mem, "ms": {},
           "max_abs_kernel_minus_torch": {}}
    for n in sizes:
        ev = pos[:n]
        with torch.no_grad():
            a = paths["torch"](ev)
            b = paths["kernel_f32"](ev)
            res["max_abs_kernel_minus_torch"][str(n)] = float((a - b).abs().max())
            del a, b
            times = {k: [] for k in paths}
            for r in range(args.rounds + 2):
                for k, fn in paths.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = fn(ev)
                    torch.cuda.synchronize()
                    dt = (time.perf_counter() - t0) * 1e3
                    del out
                    if r >= 2:   # two warm-up rounds
                        times[k].append(dt)
        for k, xs in times.items():
            res["ms"][f"{k}_{n}"] = {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs))}
    se.close()
    res["what"] = ("level-3 front end, events of the 8,192-stream recipe to [n, 80, 3000] features: host-clock ms per "
                   "call ending in a device synchronise, paths alternated round by round in one process; torch = "
                   "WhisperConfirm.log_mel(normalize_events_device(events)) float32; kernel_* = "
                   "StreamEngine.whisper_features_events; memory: peak extra device bytes per call (see the script)")
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
