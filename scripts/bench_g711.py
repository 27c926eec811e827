#!/usr/bin/env python3
"""Cost of G.711 ingest per streaming tick: 8,192 resident streams at input rate 8000, one tick per
push (the real-time cadence, lagged polls), HIP events on the engine's stream around every push,
the input kinds alternated round by round in one process, an engine each:

  f32    8 kHz float32      (3,200 bytes per stream-tick)
  pcm16  8 kHz PCM16        (1,600)
  ulaw   8 kHz G.711 mu-law (800)
  alaw   8 kHz G.711 A-law  (800)

in two modes: `device` (the ticks are in device memory already: the resampler launch reads them in
place) and `host` (the ticks are in pinned host memory: the engine gathers the rows into its
staging and copies them over PCIe, so the timed span holds the gather, the H2D copy, the resampler,
the gate and the scoring).  And a chunk step of five 160-sample packets per stream and tick,
device-resident, PCM16 against mu-law.  Every engine hears the same 8 kHz signal
(bench.make_shifted_signal, linearly interpolated to 8 kHz, quantised to PCM16; the G.711 kinds
its encoding).  After the timed rounds one more round runs with the engine's profiler on: the
resample stage (ewk_profile_read kind 3), the gate (kind 2) and the assembly launch (kind 4).  The
H2D rate is measured in the same process (a pinned 32 MB copy, median of 9) and the copy-alone
time of each host row follows from its bytes.  The yardstick of the G.711 rows is the PCM16 row.
Prints one JSON line.

    python scripts/bench_g711.py [--streams 8192] [--rounds 5] [--ticks 30] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KINDS = ("f32", "pcm16", "ulaw", "alaw")
BYTES = {"f32": 4, "pcm16": 2, "ulaw": 1, "alaw": 1}
IB, BLOCK, RATE = 800, 1600, 8000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=8192)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=30, help="timed ticks per kind, mode and round")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    import bench
    import easywakeword_amd as ewa
    from easywakeword_amd import _lib, audio

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    word = bench.load_word()
    n = args.streams
    warm = 10
    per_engine = 2 * (args.rounds + 1) * args.ticks           # device and host ticks of a tick engine
    total = 100 + warm + max(per_engine, (args.rounds + 1) * args.ticks)
    sig16 = bench.make_shifted_signal(torch, dev, n, total, args.seed, word)
    m = sig16.numel() // BLOCK * IB
    x8 = torch.nn.functional.interpolate(sig16.view(1, 1, -1), size=m, mode="linear", align_corners=False).view(-1)
    q = torch.round(x8 * 32768.0).clamp_(-32768, 32767).to(torch.int16).contiguous()
    q_host = q.cpu().numpy()
    host = {"f32": x8.contiguous().cpu(), "pcm16": torch.from_numpy(q_host),
            "ulaw": torch.from_numpy(audio.g711_encode(q_host, "ulaw")),
            "alaw": torch.from_numpy(audio.g711_encode(q_host, "alaw"))}
    host = {k: v.pin_memory() for k, v in host.items()}
    sigs = {k: v.to(dev) for k, v in host.items()}
    del sig16, x8, q

    probe = ewa.Engine()
    probe.template_from_pcm(word)
    tm, ts = probe.get_template()
    probe.close()

    def engine():
        se = ewa.StreamEngine(n)
        se.set_template(tm, ts)
        se.set_input_rate(RATE)
        return se, torch.cuda.ExternalStream(se.stream_handle(), device=dev)

    tick_eng = {k: engine() for k in KINDS}
    chunk_eng = {k: engine() for k in ("pcm16", "ulaw")}
    at = {k: 0 for k in KINDS}                     # ticks delivered per tick engine
    n_events = {}

    def push(k, mode, nt=1):
        se = tick_eng[k][0]
        base = (sigs[k].data_ptr() if mode == "device" else host[k].data_ptr()) + at[k] * IB * BYTES[k]
        flags = _lib.EWK_PUSH_DEVICE if mode == "device" else 0
        if k == "f32":
            rc = se._lib.ewk_push_many(se.handle, C.c_void_p(base), IB, IB, nt, flags)
        elif k == "pcm16":
            rc = se._lib.ewk_push_many_pcm16(se.handle, C.c_void_p(base), IB, IB, nt, flags)
        else:
            rc = se._lib.ewk_push_g711(se.handle, C.c_void_p(base), IB, IB, nt, _lib.G711_LAWS[k], flags)
        _lib.check(rc)
        at[k] += nt

    def run(k, mode, nt, timed=None):
        se, es = tick_eng[k]
        for _ in range(nt):
            if timed is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(es)
            push(k, mode)
            if timed is not None:
                e1.record(es)
                timed.append((e0, e1))
            n_events[(k, mode)] = n_events.get((k, mode), 0) + len(se.poll(lagged=True))

    ident = np.arange(n, dtype=np.int32)
    c_at = {k: 0 for k in chunk_eng}               # samples delivered per stream of a chunk engine
    counts = np.full(n, 160, np.int32)

    def chunk_step(k, timed=None):
        se, es = chunk_eng[k]
        if timed is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(es)
        for _ in range(5):
            offs = ident.astype(np.int64) * IB + c_at[k]
            se.push_chunks_device(ident, sigs[k].data_ptr(), int(sigs[k].numel()), offs, counts,
                                  pcm16=(k == "pcm16"), g711=(k if k != "pcm16" else None))
            c_at[k] += 160
        if timed is not None:
            e1.record(es)
            timed.append((e0, e1))
        se.poll(lagged=True)

    for k in KINDS:                                 # prefill (ring fill + detection start), then warm-up
        for t in range(0, 100, 25):
            push(k, "device", 25)
            tick_eng[k][0].poll(lagged=True)
        run(k, "device", warm // 2)
        run(k, "host", warm // 2)
        tick_eng[k][0].sync()
    for k in chunk_eng:
        se = chunk_eng[k][0]
        for t in range(0, 100, 25):
            ptr = sigs[k].data_ptr() + t * IB * BYTES[k]
            if k == "pcm16":
                se.push_device_pcm16(ptr, IB, IB, 25)
            else:
                se.push_device_g711(ptr, IB, IB, 25, k)
            se.poll(lagged=True)
        c_at[k] = 100 * IB
        for _ in range(warm):
            chunk_step(k)
        se.sync()
    torch.cuda.synchronize()
    n_events.clear()

    ms = {(k, mode): [] for k in KINDS for mode in ("device", "host")}
    cms = {k: [] for k in chunk_eng}
    for r in range(args.rounds):
        for mode in ("device", "host"):
            for k in KINDS:
                ev = []
                run(k, mode, args.ticks, timed=ev)
                tick_eng[k][0].sync()
                ms[(k, mode)].append([a.elapsed_time(b) for a, b in ev])
        for k in chunk_eng:
            ev = []
            for _ in range(args.ticks):
                chunk_step(k, timed=ev)
            chunk_eng[k][0].sync()
            cms[k].append([a.elapsed_time(b) for a, b in ev])
    scored = dict(n_events)

    prof = {}
    for mode in ("device", "host"):                 # one more round under the engine's profiler
        for k in KINDS:
            se = tick_eng[k][0]
            se.profile(True)
            run(k, mode, args.ticks)
            se.sync()
            g_ms, g_n = se.profile_read(2)
            r_ms, r_n = se.profile_read(3)
            se.profile(False)
            prof[(k, mode)] = {"gate_ms_per_tick": g_ms / max(1, g_n), "resample_ms_per_tick": r_ms / max(1, r_n),
                               "resample_launches": int(r_n)}
    cprof = {}
    for k in chunk_eng:
        se = chunk_eng[k][0]
        se.profile(True)
        for _ in range(args.ticks):
            chunk_step(k)
        se.sync()
        a_ms, a_n = se.profile_read(4)
        r_ms, r_n = se.profile_read(3)
        g_ms, g_n = se.profile_read(2)
        se.profile(False)
        cprof[k] = {"assembly_ms_per_step": a_ms / args.ticks, "assembly_launches_per_step": a_n / args.ticks,
                    "resample_ms_per_step": r_ms / args.ticks, "gate_ms_per_step": g_ms / args.ticks}

    # the H2D rate of this session: a pinned 32 MB copy on a stream of its own
    src = torch.empty(32 << 20, dtype=torch.uint8).pin_memory()
    dst = torch.empty(32 << 20, dtype=torch.uint8, device=dev)
    rates = []
    for _ in range(10):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src, non_blocking=True)
        e1.record()
        torch.cuda.synchronize()
        rates.append(src.numel() / (e0.elapsed_time(e1) * 1e-3))
    h2d = float(np.median(rates[1:]))

    def row(runs):
        med = [float(np.median(r)) for r in runs]
        return {"ms_median": float(np.median(np.concatenate(runs))), "round_medians": [round(x, 5) for x in med],
                "round_min": min(med), "round_max": max(med)}

    n_ticks = args.rounds * args.ticks
    res = {"streams": n, "input_rate": RATE, "rounds": args.rounds, "ticks_per_round": args.ticks,
           "h2d_bytes_per_s": h2d, "tick": {"device": {}, "host": {}}, "chunk_step_5x160": {}}
    for (k, mode), runs in ms.items():
        d = row(runs)
        d.update(prof[(k, mode)])
        d["events_per_tick"] = scored.get((k, mode), 0) / n_ticks
        d["bytes_per_stream_tick"] = IB * BYTES[k]
        if mode == "host":
            d["pcie_bytes_per_tick"] = n * IB * BYTES[k]
            d["copy_alone_ms_at_h2d_rate"] = n * IB * BYTES[k] / h2d * 1e3
        res["tick"][mode][k] = d
    for k, runs in cms.items():
        d = row(runs)
        d.update(cprof[k])
        res["chunk_step_5x160"][k] = d
    for mode in ("device", "host"):                 # the G.711 rows against the PCM16 rounds' own range
        y = res["tick"][mode]["pcm16"]
        for k in ("ulaw", "alaw"):
            x = res["tick"][mode][k]
            x["tick_median_inside_pcm16_rounds"] = bool(y["round_min"] <= x["ms_median"] <= y["round_max"])
            x["tick_median_above_pcm16_rounds"] = bool(x["ms_median"] > y["round_max"])
            x["resample_over_pcm16"] = x["resample_ms_per_tick"] / y["resample_ms_per_tick"]
    y, x = res["chunk_step_5x160"]["pcm16"], res["chunk_step_5x160"]["ulaw"]
    x["step_median_above_pcm16_rounds"] = bool(x["ms_median"] > y["round_max"])
    x["assembly_over_pcm16"] = x["assembly_ms_per_step"] / y["assembly_ms_per_step"]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    for se, _ in list(tick_eng.values()) + list(chunk_eng.values()):
        se.close()


if __name__ == "__main__":
    main()
