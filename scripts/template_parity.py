#!/usr/bin/env python3
"""Measure template parity per reference recording (tests/template_cases.py) on the GPU and write
the raw figures as JSON: the numbers behind DESIGN.md section 4, "Template derivation".

    python scripts/template_parity.py [--label float32_derivation] [--out profiles/template_parity.json]

Per recording: |mean|, |std|, frames and reference_spread (oracle alone), the drift of the
template template_from_pcm derives, the worst |score - reference| over the candidate batch
(float64 and float32 candidates), and the drift of the mean / std Engine.score returns for it
(with a template set and with none).  Nothing is asserted here; tests/test_gpu_template_parity.py
holds the bounds.  An existing --out file keeps its other labels.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import template_cases as tc  # noqa: E402


def measure():
    from easywakeword_amd import Engine
    eng, bare = Engine(), Engine()
    cands = list(tc.candidates())
    recs = [x for _, x in tc.recordings()]
    eng.template_from_pcm(tc.recording("word"))
    set_m, set_s, _, _ = eng.score(recs, candidate_dtype="float64")
    no_m, no_s, _, _ = bare.score(recs, require_template=False)
    rows = {}
    for k, name in enumerate(tc.NAMES):
        eng.template_from_pcm(recs[k])
        row = dict(tc.describe(name))
        row["template_drift"] = tc.template_drift(eng.get_template(), tc.oracle_template(name), tc.candidate_stats())
        for dt in ("float64", "float32"):
            _, _, score, _ = eng.score(cands, candidate_dtype=dt)
            ref = tc.oracle_scores(name, dt)
            ok = np.isfinite(ref) & np.isfinite(score)
            row[f"end_to_end_{dt}"] = float(np.max(np.abs(score[ok] - ref[ok]))) if ok.any() else 0.0
            row[f"nan_mismatch_{dt}"] = int(np.sum(np.isnan(ref) != np.isnan(score)))
        row["returned_drift_template_set"] = tc.template_drift((set_m[k], set_s[k]), tc.oracle_template(name),
                                                               tc.candidate_stats())
        row["returned_drift_no_template"] = tc.template_drift((no_m[k], no_s[k]), tc.oracle_template(name),
                                                              tc.candidate_stats())
        rows[name] = row
        print(name, json.dumps(row))
    eng.close()
    bare.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="float32_derivation")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "template_parity.json"))
    a = ap.parse_args()
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    doc[a.label] = measure()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
