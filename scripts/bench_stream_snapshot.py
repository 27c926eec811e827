#!/usr/bin/env python3
"""Cost of moving streams between engines (ewk_export_streams / ewk_import_streams) on one MI355X:
two engines of 8,192 resident streams each, for the default configuration and for 3 s int16 rings.

  move   src.move_streams(dst, first n, first n) for n = 1, 64, 1,024, 8,192: records packed into a
         device buffer and unpacked from it, no host copy.  The pack and unpack launch times come
         from ewk_profile_read kind 5 of the source and of the destination engine.
  copy   the yardstick, timed in the same process with HIP events: a float4-vectorised copy kernel
         (torch.mul(x, 1, out=y) on float32) over the same number of bytes.
  host   one export_streams and one import_streams of 1,024 streams through the bounded pinned
         staging (wall clock, the import with its synchronisation), against a pinned host-to-device
         copy of the same bytes (torch, non_blocking from a pinned tensor).

The cases are alternated round by round; every figure is reported with its round-to-round spread.
Rates count the bytes read plus the bytes written (2 x n x record_bytes), for the launches and for
the copy alike, so the fraction is the launches' share of what the copy kernel reaches.  One JSON line.

    python scripts/bench_stream_snapshot.py [--streams 8192] [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {
    "default_f32_10s": (dict(), False),
    "i16_3s": (dict(ring_samples=48000, ring_format=1), True),
}


def spread(xs):
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs)), "rounds": [round(float(x), 5) for x in xs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=8192)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-streams", type=int, default=1024)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    import easywakeword_amd as ewa

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    n = args.streams
    sizes = [s for s in (1, 64, 1024, 8192) if s <= n]
    res = {"streams": n, "rounds": args.rounds, "sizes": sizes, "config": {}}

    for name, (cfg, pcm16) in CONFIGS.items():
        src, dst = ewa.StreamEngine(n, **cfg), ewa.StreamEngine(n, **cfg)
        lay = src.snapshot_layout()
        rb = lay["record_bytes"]
        gen = torch.Generator(device=dev).manual_seed(7)
        for eng in (src, dst):                      # three ticks of noise: rings and states that are not all zero
            if pcm16:
                pcm = torch.randint(-3000, 3000, (n, 3 * 1600), generator=gen, device=dev, dtype=torch.int16)
                eng.push_device_pcm16(pcm.data_ptr(), 3 * 1600, 1600, 3)
            else:
                pcm = 0.05 * torch.randn((n, 3 * 1600), generator=gen, device=dev)
                eng.push_device(pcm.data_ptr(), 3 * 1600, 1600, 3)
            eng.sync()
            eng.poll()
            eng.profile(True)
        big = max(sizes) * rb
        x = torch.zeros(big // 4, dtype=torch.float32, device=dev)
        y = torch.empty_like(x)

        def copy_ms(nbytes):
            a, b = x[: nbytes // 4], y[: nbytes // 4]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.mul(a, 1.0, out=b)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)

        def move_ms(k):
            ids = np.arange(k, dtype=np.int32)
            src.move_streams(dst, ids, ids)
            src.sync()
            dst.sync()
            (p_ms, p_n), (u_ms, u_n) = src.profile_read(5), dst.profile_read(5)
            assert p_n == 1 and u_n == 1, (p_n, u_n)
            return p_ms, u_ms

        for k in sizes:                              # warm-up: allocations, first launches
            move_ms(k)
            copy_ms(k * rb)
        pack = {k: [] for k in sizes}
        unpack = {k: [] for k in sizes}
        copy = {k: [] for k in sizes}
        for _ in range(args.rounds):
            for k in sizes:
                p, u = move_ms(k)
                pack[k].append(p)
                unpack[k].append(u)
                copy[k].append(copy_ms(k * rb))
        rows = {}
        for k in sizes:
            moved = 2.0 * k * rb
            gbs = lambda ms: moved / (ms * 1e-3) / 1e9
            pm, um, cm = (float(np.median(v[k])) for v in (pack, unpack, copy))
            rows[str(k)] = {"bytes": k * rb, "pack_ms": spread(pack[k]), "unpack_ms": spread(unpack[k]),
                            "copy_ms": spread(copy[k]), "pack_gb_per_s": gbs(pm), "unpack_gb_per_s": gbs(um),
                            "copy_gb_per_s": gbs(cm), "pack_share_of_copy": cm / pm, "unpack_share_of_copy": cm / um}
        del x, y

        hn = min(args.host_streams, n)
        ids = np.arange(hn, dtype=np.int32)
        exp, imp, h2d = [], [], []
        pinned = torch.empty(hn * rb, dtype=torch.uint8).pin_memory()
        on_dev = torch.empty(hn * rb, dtype=torch.uint8, device=dev)
        snap = src.export_streams(ids)               # warm-up: the staging is allocated here
        dst.import_streams(ids, snap)
        dst.sync()
        for _ in range(max(2, args.rounds // 2 + 1)):
            t0 = time.perf_counter()
            snap = src.export_streams(ids)
            t1 = time.perf_counter()
            dst.import_streams(ids, snap)
            dst.sync()
            t2 = time.perf_counter()
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            on_dev.copy_(pinned, non_blocking=True)
            torch.cuda.synchronize()
            t4 = time.perf_counter()
            exp.append((t1 - t0) * 1e3)
            imp.append((t2 - t1) * 1e3)
            h2d.append((t4 - t3) * 1e3)
        hb = hn * rb
        host = {"streams": hn, "bytes": hb, "export_ms": spread(exp), "import_ms": spread(imp), "pinned_h2d_ms": spread(h2d),
                "export_gb_per_s": hb / (np.median(exp) * 1e-3) / 1e9, "import_gb_per_s": hb / (np.median(imp) * 1e-3) / 1e9,
                "pinned_h2d_gb_per_s": hb / (np.median(h2d) * 1e-3) / 1e9}
        res["config"][name] = {"record_bytes": rb, "ring_bytes": lay["sections"]["ring"][1], "move": rows, "host": host}
        del pinned, on_dev, snap
        src.close()
        dst.close()
        torch.cuda.empty_cache()

    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
