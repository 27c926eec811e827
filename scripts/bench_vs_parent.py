#!/usr/bin/env python3
"""This checkout against a built checkout of its parent commit, alternated on one GPU:

  tick   scripts/bench_push_streams.py --cases a (the lockstep tick of 8,192 streams without any
         table or list: tick_ms_median and gate_ms_per_launch), and
  bench  bench.py --gpus 1 --steps 20 --warmup 5 (`value`), and
  chunks scripts/bench_push_chunks.py --cases cd (packet ingest at 8,192 streams: step_ms_median of
         case c, one block per stream and push, and of case d, five 320-sample packets per tick), and
  resample scripts/bench_resample.py --cases bcd --rounds 3 --ticks 30 (the tick with an input rate
         set, 48 kHz float32, 44.1 kHz float32 and 48 kHz PCM16: tick_ms_median and the resample stage
         from ewk_profile_read kind 3),

each in a fresh process per tree and round, the order of the two trees swapped every round.
Acceptance as profiles/engine_split_vs_parent.json: this checkout's median inside the min..max of
the parent's rounds.  A step that fails or runs past its time limit ends the script at once.

    python scripts/bench_vs_parent.py --parent DIR [--what tick,bench,chunks,resample] [--rounds 5] --out FILE

DIR holds the parent commit with its own libewk.so built in place (git worktree + python -m
easywakeword_amd.build there).  An existing FILE is extended: `tick`, `bench`, `chunks` and
`resample` may come from separate calls.  FILE is rewritten after every round.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_json(tree, argv, limit):
    """The last JSON line a script of `tree` prints."""
    env = dict(os.environ)
    env.pop("EWK_LIB", None)
    p = subprocess.run([sys.executable] + argv, cwd=tree, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=limit)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        raise SystemExit(f"{argv[0]} in {tree} ended with {p.returncode}")
    for line in reversed(p.stdout.strip().splitlines()):
        if line.startswith("{"):
            return json.loads(line)
    raise SystemExit(f"{argv[0]} in {tree} printed no JSON line")


def stats(name, xs):
    return {f"{name}_median": float(np.median(xs)), f"{name}_min": float(min(xs)), f"{name}_max": float(max(xs))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--what", default="tick,bench")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    trees = {"parent": os.path.abspath(args.parent), "new": ROOT}
    res = {"parent": {}, "new": {}}
    if os.path.exists(args.out):
        with open(args.out) as f:
            res = json.load(f)
    what = args.what.split(",")
    if "tick" in what:
        for t in trees:
            res[t]["tick_ms"], res[t]["gate_ms"] = [], []
    if "bench" in what:
        for t in trees:
            res[t]["bench_value"] = []
    if "chunks" in what:
        for t in trees:
            res[t]["chunk_c_ms"], res[t]["chunk_d_ms"] = [], []
    rs_rows = {"b": "rs48_f32", "c": "rs441_f32", "d": "rs48_pcm16"}
    if "resample" in what:
        for t in trees:
            for v in rs_rows.values():
                res[t][v + "_tick_ms"], res[t][v + "_stage_ms"] = [], []
    names = ("tick_ms", "gate_ms", "bench_value", "chunk_c_ms", "chunk_d_ms") + tuple(
        v + s for v in rs_rows.values() for s in ("_tick_ms", "_stage_ms"))
    for r in range(args.rounds):
        order = ["parent", "new"] if r % 2 == 0 else ["new", "parent"]
        for t in order:
            if "tick" in what:
                d = run_json(trees[t], ["scripts/bench_push_streams.py", "--cases", "a"], 240)
                res[t]["tick_ms"].append(d["tick"]["a"]["tick_ms_median"])
                res[t]["gate_ms"].append(d["tick"]["a"]["gate_ms_per_launch"])
            if "bench" in what:
                d = run_json(trees[t], ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], 400)
                res[t]["bench_value"].append(d["value"])
            if "chunks" in what:
                d = run_json(trees[t], ["scripts/bench_push_chunks.py", "--cases", "cd"], 240)
                res[t]["chunk_c_ms"].append(d["step"]["c"]["step_ms_median"])
                res[t]["chunk_d_ms"].append(d["step"]["d"]["step_ms_median"])
            if "resample" in what:
                d = run_json(trees[t], ["scripts/bench_resample.py", "--cases", "bcd", "--rounds", "3", "--ticks", "30"],
                             300)
                for k, v in rs_rows.items():
                    res[t][v + "_tick_ms"].append(d["tick"][k]["tick_ms_median"])
                    res[t][v + "_stage_ms"].append(d["profile"][k]["resample_ms_per_tick"])
            print(f"round {r} {t} done", flush=True)
        summarise(res, trees, names)
        res["rounds_done"] = r + 1
        write(args.out, res)
    print(json.dumps(res))


def summarise(res, trees, names):
    for t in trees:
        for name in names:
            if res[t].get(name):
                res[t].update(stats(name, res[t][name]))
    for name in names:
        if res["new"].get(name) and res["parent"].get(name):
            res[f"{name}_new_median_inside_parent_range"] = bool(
                res["parent"][f"{name}_min"] <= res["new"][f"{name}_median"] <= res["parent"][f"{name}_max"])
    res["what"] = ("lockstep streaming tick (scripts/bench_push_streams.py --cases a, 8,192 streams, no profile table, "
                   "HIP-event ms per tick, median of 5 rounds x 40 ticks; gate_ms: its gate launch from "
                   "ewk_profile_read kind 2), bench.py --gpus 1 --steps 20 --warmup 5 `value` and packet ingest "
                   "(scripts/bench_push_chunks.py --cases cd, step_ms_median of cases c and d): the parent "
                   "commit's build against this one, a fresh process per tree and round, the order swapped every "
                   "round (scripts/bench_vs_parent.py); acceptance: the new build's median inside the min..max of "
                   "the parent's rounds; rs*_tick_ms / rs*_stage_ms: the tick and the resample stage (kind 3) of "
                   "scripts/bench_resample.py --cases bcd --rounds 3 --ticks 30 at 48 kHz float32, 44.1 kHz float32 "
                   "and 48 kHz PCM16")


def write(out, res):
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
