#!/usr/bin/env python3
"""Cost of the template bank on bench.py's seeded 65,536-segment ragged batch (device-resident,
HIP events after warm-up, one process, the cases alternated round by round):

  a  ewk_score_segments_device, the single template
  b  ewk_score_segments_bank_device, 1 word x 1 template
  c  1 word x 64 templates
  d  1,024 words x 8 templates, a random word per segment

and the fraction of segments each bank case lists for the fp64 pass (a has no such read-out; with
one template the rule of b is a's).  Prints one JSON line.

    python scripts/bench_bank.py [--segments 65536] [--rounds 7] [--warmup 2] [--rescore-margin M]
                                 [--f32-candidates] [--out FILE]

--f32-candidates scores every case with float32 candidates (EWK_SCORE_F32_CANDIDATES: the float32
finishes of ewk_score.h / ewk_mfcc.hip); the default is the streaming arithmetic, float64 candidates.
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
    ap.add_argument("--segments", type=int, default=65536)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rescore-margin", type=float, default=None,
                    help="rescore_margin of the bank engines (0: no near-threshold listing, which shows "
                         "what the fp64 pass costs)")
    ap.add_argument("--f32-candidates", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    import bench
    import easywakeword_amd as ewa
    from easywakeword_amd import _lib

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    word = bench.load_word()
    n = args.segments
    pcm, d_off, d_len, frames, lengths, offsets = bench.make_segments(torch, dev, n, args.seed, word)
    mean = torch.empty((n, 20), device=dev)
    std = torch.empty((n, 20), device=dev)
    score = torch.empty(n, device=dev, dtype=torch.float64)
    match = torch.empty(n, device=dev, dtype=torch.uint8)
    out = torch.zeros(n * 24, device=dev, dtype=torch.uint8)
    rng = np.random.Generator(np.random.PCG64(args.seed))
    d_word = torch.from_numpy(rng.integers(0, 1024, n).astype(np.int32)).to(dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    sh = stream.cuda_stream

    # templates: the word and perturbed copies of it (scores spread around the threshold)
    single = ewa.Engine()
    single.template_from_pcm(word)
    tm, ts = single.get_template()

    def variants(k):
        r = np.random.Generator(np.random.PCG64(args.seed + k))
        return [(tm, ts)] + [((tm + r.normal(0, 2.0, 20)).astype(np.float32),
                              np.abs(ts + r.normal(0, 1.0, 20)).astype(np.float32)) for _ in range(k - 1)]

    banks = {"b": [variants(1)], "c": [variants(64)]}
    v = variants(64)
    banks["d"] = [[v[(w + j) % 64] for j in range(8)] for w in range(1024)]
    engines = {"a": single}
    for key, words in banks.items():
        e = ewa.Engine() if args.rescore_margin is None else ewa.Engine(rescore_margin=args.rescore_margin)
        e.set_bank(words)
        engines[key] = e

    def run(key):
        e = engines[key]
        if key == "a":
            e.score_device(pcm.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n, mean.data_ptr(), std.data_ptr(),
                           score.data_ptr(), match.data_ptr(), sh, f32_candidates=args.f32_candidates)
        else:
            e.score_bank_device(pcm.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n,
                                d_word.data_ptr() if key == "d" else 0, out.data_ptr(), 0, 0, sh,
                                f32_candidates=args.f32_candidates)

    keys = ["a", "b", "c", "d"]
    for _ in range(args.warmup):
        for k in keys:
            run(k)
    torch.cuda.synchronize()
    ms = {k: [] for k in keys}
    for _ in range(args.rounds):
        for k in keys:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            run(k)
            e1.record(stream)
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))

    listed = {}
    for k in ("b", "c", "d"):
        run(k)
        torch.cuda.synchronize()
        listed[k] = float(out.cpu().numpy().view(_lib.BANK_RESULT_DTYPE)["rescored"].mean())
    res = {"segments": n, "frames": frames, "rounds": args.rounds, "rescore_margin": args.rescore_margin,
           "f32_candidates": bool(args.f32_candidates),
           "ms_median": {k: float(np.median(v_)) for k, v_ in ms.items()},
           "ms_min": {k: float(np.min(v_)) for k, v_ in ms.items()},
           "ms_all": {k: [round(x, 4) for x in v_] for k, v_ in ms.items()},
           "listed_fraction": listed}
    med = res["ms_median"]
    res["b_minus_a_ms"] = med["b"] - med["a"]
    res["c_minus_b_ms"] = med["c"] - med["b"]
    res["d_minus_b_ms"] = med["d"] - med["b"]
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
