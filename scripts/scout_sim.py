"""Offline model of k_score_f32's loudest-first tile order (CPU, oracle log-mel).

For segments of the bench's ragged recipe (bench.make_segments on the CPU) it computes each
16-frame tile's exact max / min log-mel (before top_db), orders the tiles by a scout
heuristic, replays the speculative clamp (running max - 80 dB, self-clamp included) and
counts the tiles and 8-frame passes the kernel would recompute.  Usage:
    python scripts/scout_sim.py [n_segments] [fixed_len]

The "shift rule" lines replay the kernel's rule (csrc/ewk_topdb_shift.h) on the current scout
order: a tile's clamped entries move up with the clamp inside the statistics, so a tile is
recomputed only if one of its unclamped stored values lies between its own clamp and the final
threshold.  They also give the share of tiles that hold a clamped entry (the tiles that pay for
the mask DCT) and break the counts down per segment kind of the bench recipe.

    python scripts/scout_sim.py mask [n]
replays "masks only where the clamp can still rise" (mask_near / mask_wanted in
csrc/ewk_topdb_shift.h) on the ragged batch (4n/3 segments), L = 16,000 and L = 6,400 (n each):
per window X the masks built, the clamped tiles left without a mask that a later rise recomputes,
and the recomputed passes (profiles/r08_v1_scout_sim_mask_rule.txt).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HOP = 160


def log_mel_raw(y):
    from oracle import mfcc_ref
    mel_basis, _ = mfcc_ref._tables()
    S = mfcc_ref.power_spectrogram(y.astype(np.float64))
    mel = np.einsum("ft,mf->mt", S, mel_basis)
    return 10.0 * np.log10(np.maximum(1e-10, mel))          # [128, T]


def sample_rows(y, t, rows, width, stride, first):
    base = t * 16 * HOP
    out = []
    for q in range(rows):
        s0 = base + first + stride * q
        seg = y[max(0, s0):max(0, s0 + width)]
        out.append(seg if len(seg) == width else np.concatenate([seg, np.zeros(width - len(seg))]))
    return np.stack(out)


def heuristics(y, ntile):
    h = {}
    r4 = [sample_rows(y, t, 4, 64, 640, 64) for t in range(ntile)]
    h["H0 sum 4x64 (current)"] = np.array([float((r.astype(np.float32) ** 2).sum()) for r in r4])
    r8 = [sample_rows(y, t, 8, 32, 320, 64) for t in range(ntile)]
    h["H1 max 8x32"] = np.array([float((r ** 2).sum(axis=1).max()) for r in r8])
    h["H1b max 4x64"] = np.array([float((r ** 2).sum(axis=1).max()) for r in r4])
    r16 = [sample_rows(y, t, 16, 16, 160, 64) for t in range(ntile)]
    h["H2 max 16x16"] = np.array([float((r ** 2).sum(axis=1).max()) for r in r16])
    r8b = [sample_rows(y, t, 8, 64, 320, 64) for t in range(ntile)]   # 2x the loads
    h["H3 max 8x64 (2x loads)"] = np.array([float((r ** 2).sum(axis=1).max()) for r in r8b])
    # full coverage: the max over the tile's 16 frames of the frame energy (512-sample
    # windows, Hann-weighted or flat), and of 160-sample hop chunks
    yp = np.concatenate([np.zeros(256), y.astype(np.float64), np.zeros(256 + 16 * HOP * ntile)])
    win = np.hanning(514)[1:-1]
    fe = np.array([[float(((yp[(16 * t + f) * HOP:(16 * t + f) * HOP + 512] * win) ** 2).sum()) for f in range(16)]
                   for t in range(ntile)])
    h["H4 max frame energy (hann)"] = fe.max(axis=1)
    fe2 = np.array([[float((yp[(16 * t + f) * HOP:(16 * t + f) * HOP + 512] ** 2).sum()) for f in range(16)]
                    for t in range(ntile)])
    h["H5 max frame energy (flat)"] = fe2.max(axis=1)
    ch = np.array([[float((yp[256 + (16 * t + f) * HOP:256 + (16 * t + f + 1) * HOP] ** 2).sum()) for f in range(16)]
                   for t in range(ntile)])
    h["H6 max hop-chunk energy"] = ch.max(axis=1)
    w2 = win ** 2
    for fs, ss in ((2, 1), (4, 1), (8, 1), (4, 2), (4, 4), (8, 2), (16, 1)):
        e = np.array([[float((yp[(16 * t + f) * HOP:(16 * t + f) * HOP + 512:ss] ** 2 * w2[::ss]).sum())
                       for f in range(0, 16, fs)] for t in range(ntile)])
        h[f"H7 hann frames/{fs} samples/{ss}"] = e.max(axis=1)
    # chunked: energy of C-sample chunks, frame energy = sum of chunk energies x mean w^2
    for C in (16, 32, 64):
        wc = w2.reshape(512 // C, C).mean(axis=1)
        u = yp[:len(yp) // C * C].reshape(-1, C)
        ce = (u ** 2).sum(axis=1)
        e = np.array([[float((ce[(16 * t + f) * HOP // C:(16 * t + f) * HOP // C + 512 // C] * wc).sum())
                       for f in range(16)] for t in range(ntile)])
        h[f"H8 chunk {C} hann-weighted"] = e.max(axis=1)
    return h


KINDS = {0: "word", 1: "word", 2: "tone 880 Hz", 3: "noise burst"}


def bench_kinds(n, seed=1234):
    """The segment kinds bench.make_segments draws (same generator, same draws)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    rng.integers(6400, 33600 + 1, n)
    rng.uniform(1e-4, 5e-3, n)
    rng.uniform(0.2, 3.0, n)
    return rng.integers(0, 4, n)


def scout_order(y, ntile):
    """The kernel's processing order: loudest first by the 4 x 64-sample scout, ties by index."""
    e = [float((sample_rows(y, t, 4, 64, 640, 64).astype(np.float32) ** 2).sum()) for t in range(ntile)]
    return sorted(range(ntile), key=lambda t: (-e[t], t))


def replay_rules(L, order):
    """Replay the speculative clamp over the raw log-mel L [128, T] in tile order `order`.
    Returns the counts of both rules: tiles / passes whose stored minimum is below the final
    threshold (old), tiles / passes holding an unclamped stored value in (run_k, theta) (shift
    rule), the tiles holding a clamped entry (masked) and the tiles after the first that raise
    the max over their own stored values (late_self_clamps: they are re-clamped in place and
    every earlier tile shifts), and the largest rise theta - run_k over the passes that hold a
    clamped entry and are not recomputed (max_kept_rise: what the shift alone has to get right)."""
    T = L.shape[1]
    theta = L.max() - 80.0
    run = -np.inf
    out = {"old_tiles": 0, "old_passes": 0, "new_tiles": 0, "new_passes": 0, "masked": 0, "tiles": len(order),
           "late_self_clamps": 0, "max_kept_rise": 0.0, "kept_partial": 0}
    for t in order:
        X = L[:, 16 * t:min(T, 16 * t + 16)]
        out["late_self_clamps"] += bool(np.isfinite(run) and X.max() - 80.0 > run and X.min() < X.max() - 80.0)
        run = max(run, X.max() - 80.0)
        out["masked"] += bool(X.min() < run)
        old = new = 0
        for p in (0, 8):
            P = X[:, p:p + 8]
            if P.size == 0:
                continue
            old += bool(max(P.min(), run) < theta)
            free = P[P > run]                      # the unclamped stored values
            flag = bool(free.size and free.min() < theta)
            new += flag
            if not flag and P.min() < run:         # shifted, never recomputed
                out["max_kept_rise"] = max(out["max_kept_rise"], float(theta - run))
                out["kept_partial"] += bool(free.size and theta - run >= 1.0)   # mask neither empty nor full
        out["old_tiles"] += old > 0
        out["old_passes"] += old
        out["new_tiles"] += new > 0
        out["new_passes"] += new
    return out


def scout_energy(y, ntile):
    return np.array([float((sample_rows(y, t, 4, 64, 640, 64).astype(np.float32) ** 2).sum()) for t in range(ntile)])


def replay_mask_rule(L, order, e, X):
    """Replay "masks only where the clamp can still rise" (mask_near / mask_wanted in
    csrc/ewk_topdb_shift.h) over the raw log-mel L [128, T] in scout order `order` (scout
    energies e).  X: the window in dB; None = every tile with a clamped entry is masked (the rule
    before), inf = all but the last.  Returns masks built, clamped tiles left without one, those
    of them recomputed later (tiles, passes), and all recomputed passes."""
    T = L.shape[1]
    theta = L.max() - 80.0
    if X is None:
        near = len(order) + 1
    else:
        emax = max(float(e.max()), 0.0)
        near = int(sum(1 for t in order if e[t] >= 10.0 ** (-X / 10.0) * emax)) if np.isfinite(X) else len(order)
    out = {"masks": 0, "skipped": 0, "skipped_fixed_tiles": 0, "skipped_fixed_passes": 0, "passes": 0,
           "near": min(near, len(order)), "kept_shifted_passes": 0, "first_skipped_fixed": 0, "rises": 0}
    run = -np.inf
    for k, t in enumerate(order):
        X16 = L[:, 16 * t:min(T, 16 * t + 16)]
        out["rises"] += bool(k and X16.max() - 80.0 > run)
        run = max(run, X16.max() - 80.0)
        clamped = bool(X16.min() < run)
        masked = clamped and k + 1 < near
        out["masks"] += masked
        out["skipped"] += clamped and not masked
        fixed = 0
        for p in (0, 8):
            P = X16[:, p:p + 8]
            if P.size == 0:
                continue
            if masked:      # record: the minimum above the clamp
                free = P[P > run]
                flag = bool(free.size and free.min() < theta)
                # shifted by a decibel or more with a mask neither empty nor full, never recomputed
                out["kept_shifted_passes"] += bool(not flag and P.min() < run and free.size and theta - run >= 1.0)
                fixed += flag
            else:           # record: max(pass minimum, run)
                fixed += bool(max(P.min(), run) < theta)
        out["passes"] += fixed
        if clamped and not masked and fixed:
            out["skipped_fixed_tiles"] += 1
            out["skipped_fixed_passes"] += fixed
            out["first_skipped_fixed"] += k == 0
    return out


MASK_CYCLES = 3292      # a masked tile beyond a plain DCT (profiles/r07_v3_phase_timing.txt: 5,085 - 1,793)
PASS_CYCLES = 9500      # a recomputed pass with its share of fix_tile's two DCTs (assumed, not measured)


def mask_rule_table(n, fixed):
    """The table of the mask rule for one bench batch: per window X the masks built, the clamped
    tiles left without one that a later rise recomputes, and the recomputed passes, per segment."""
    import torch
    import bench
    word = bench.load_word()
    pcm, off, ln, frames, lengths, offsets = bench.make_segments(torch, torch.device("cpu"), n, 1234, word,
                                                                   fixed_len=fixed)
    pcm = pcm.numpy()
    rows = [("always (before)", None), ("X =  3 dB", 3.0), ("X =  6 dB", 6.0), ("X = 10 dB", 10.0),
            ("X = 20 dB", 20.0), ("all but the last", np.inf)]
    tot = {name: None for name, _ in rows}
    followed = 0
    for i in range(n):
        y = pcm[offsets[i]:offsets[i] + lengths[i]].astype(np.float32)
        L = log_mel_raw(y)
        ntile = (L.shape[1] + 15) // 16
        e = scout_energy(y, ntile)
        order = sorted(range(ntile), key=lambda t: (-e[t], t))
        for name, X in rows:
            r = replay_mask_rule(L, order, e, X)
            tot[name] = r if tot[name] is None else {k: tot[name][k] + r[k] for k in r}
        # masked tiles (rule before) with any rise of the clamp after them
        run, runs = -np.inf, []
        for t in order:
            X16 = L[:, 16 * t:16 * t + 16]
            run = max(run, X16.max() - 80.0)
            runs.append((run, bool(X16.min() < run)))
        followed += sum(1 for r, c in runs if c and r < runs[-1][0])
    base = tot["always (before)"]
    print(f"mask rule, {n} segments, fixed_len={fixed or 'ragged'}: masked tiles/segment {base['masks'] / n:.3f}, "
          f"of them followed by any rise {followed / n:.3f}")
    print("  rule               masks/seg  skipped/seg  skipped recomputed: tiles/seg passes/seg  all passes/seg  "
          "extra passes/seg  modelled cycles/seg")
    for name, _ in rows:
        r = tot[name]
        extra = (r["passes"] - base["passes"]) / n
        print(f"  {name:18s} {r['masks'] / n:9.3f} {r['skipped'] / n:12.3f} {r['skipped_fixed_tiles'] / n:29.4f} "
              f"{r['skipped_fixed_passes'] / n:10.4f} {r['passes'] / n:15.4f} {extra:17.4f} "
              f"{(r['masks'] * MASK_CYCLES + (r['passes'] - base['passes']) * PASS_CYCLES) / n:20,.0f}")


POS = {}
PARK = {}


def simulate(order, tmax, tmin, pmin, name=""):
    run = -np.inf
    stored, stored_p = {}, {}
    for t in order:
        run = max(run, tmax[t] - 80.0)
        stored[t] = max(tmin[t], run)
        stored_p[t] = [max(m, run) for m in pmin[t]]
    theta = tmax.max() - 80.0
    tiles = sum(1 for t in order if stored[t] < theta)
    passes = sum(sum(1 for m in stored_p[t] if m < theta) for t in order)
    pos = POS.setdefault(name, {})
    for k, t in enumerate(order):   # processing position of the recomputed tiles
        if stored[t] < theta:
            pos[k] = pos.get(k, 0) + 1
    return tiles, passes


def main():
    import torch
    import bench
    if len(sys.argv) > 1 and sys.argv[1] == "mask":   # the mask rule's table for the three bench batches
        n = int(sys.argv[2]) if len(sys.argv) > 2 else 300
        for fixed in (0, 16000, 6400):
            mask_rule_table(n + n // 3 if fixed == 0 else n, fixed)
        return
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1500
    fixed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    word = bench.load_word()
    pcm, off, ln, frames, lengths, offsets = bench.make_segments(torch, torch.device("cpu"), n, 1234, word,
                                                                   fixed_len=fixed)
    pcm = pcm.numpy()
    tot = {}
    n_tiles = 0
    kinds = bench_kinds(n)
    rules = {}
    for i in range(n):
        y = pcm[offsets[i]:offsets[i] + lengths[i]].astype(np.float32)
        L = log_mel_raw(y)
        T = L.shape[1]
        ntile = (T + 15) // 16
        n_tiles += ntile
        tmax = np.array([L[:, 16 * t:min(T, 16 * t + 16)].max() for t in range(ntile)])
        tmin = np.array([L[:, 16 * t:min(T, 16 * t + 16)].min() for t in range(ntile)])
        pmin = [[L[:, p:min(T, p + 8)].min() if p < T else np.inf for p in (16 * t, 16 * t + 8)] for t in range(ntile)]
        hs = heuristics(y, ntile)
        r = replay_rules(L, scout_order(y, ntile) if ntile > 1 else [0])
        for key in ("all", KINDS[int(kinds[i])]):
            acc = rules.setdefault(key, dict.fromkeys(r, 0) | {"segments": 0})
            for name, val in r.items():
                acc[name] = max(acc[name], val) if name == "max_kept_rise" else acc[name] + int(val)
            acc["segments"] += 1
        hs["oracle (true tile max)"] = tmax
        hs["time order"] = -np.arange(ntile, dtype=float)
        # hybrid: the current scout's order, its top K re-ranked by the chunked Hann energy
        h0, h8 = hs["H0 sum 4x64 (current)"], hs["H8 chunk 32 hann-weighted"]
        for K in (2, 3, 4, 6):
            o0 = sorted(range(ntile), key=lambda t: (-h0[t], t))
            top = sorted(o0[:K], key=lambda t: (-h8[t], t))
            hs[f"H9 hybrid top {K}"] = {t: -k for k, t in enumerate(top + o0[K:])}
        for name, sc in hs.items():
            order = sorted(range(ntile), key=lambda t: (-sc[t], t))
            a, b = simulate(order, tmax, tmin, pmin, name)
            ta, tb = tot.get(name, (0, 0))
            tot[name] = (ta + a, tb + b)
        # parking policy on the current scout: park tile k if an unprocessed tile's scout energy
        # is within X dB of the best processed so far (a later tile might raise the max)
        sc = hs["H0 sum 4x64 (current)"]
        order = sorted(range(ntile), key=lambda t: (-sc[t], t))
        db = 10 * np.log10(np.maximum(sc, 1e-30))
        run = -np.inf
        stored = {}
        for k, t in enumerate(order):
            run = max(run, tmax[t] - 80.0)
            stored[t] = max(tmin[t], run)
        theta = tmax.max() - 80.0
        for X in (0, 3, 6, 10, 20):
            parked = fixed_parked = fixed_rec = 0
            best = -np.inf
            for k, t in enumerate(order):
                best = max(best, db[t])
                rest = max((db[u] for u in order[k + 1:]), default=-np.inf)
                park = rest > best - X
                need = stored[t] < theta
                parked += park
                fixed_parked += need and park
                fixed_rec += need and not park
            key = f"park X={X:2d} dB"
            pa, fp, fr = PARK.get(key, (0, 0, 0))
            PARK[key] = (pa + parked, fp + fixed_parked, fr + fixed_rec)
    print(f"{n} segments, {n_tiles} tiles (fixed_len={fixed or 'ragged'})")
    for name, (a, b) in tot.items():
        print(f"  {name:28s} recomputed tiles/segment {a / n:6.3f} ({100.0 * a / n_tiles:5.1f} % of tiles)  "
              f"passes/segment {b / n:6.3f}  positions {dict(sorted(POS.get(name, {}).items())[:6])}")
    for key, acc in rules.items():
        ns = max(1, acc["segments"])
        print(f"  shift rule, {key:12s} ({acc['segments']} segments): stored min < theta "
              f"{acc['old_tiles'] / ns:6.3f} tiles {acc['old_passes'] / ns:6.3f} passes/segment; "
              f"unclamped value in (run_k, theta) {acc['new_tiles'] / ns:6.3f} tiles "
              f"{acc['new_passes'] / ns:6.3f} passes/segment; "
              f"tiles with a clamped entry {100.0 * acc['masked'] / max(1, acc['tiles']):5.1f} %")
    for key, (pa, fp, fr) in PARK.items():
        print(f"  {key}: parked tiles/segment {pa / n:6.3f}, fixes from parked {fp / n:6.3f}, "
              f"recomputed {fr / n:6.3f}")


if __name__ == "__main__":
    main()
