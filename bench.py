#!/usr/bin/env python3
"""bench.py -- MFCC frames/s of the level-2 scorer (+ streaming level-1 gate)
on MI355X, next to the CPU oracle on the host cores.

Contract (see the task's bench section): ``python bench.py --gpus N --steps K
--warmup W``; for N>1 it is launched under torch.distributed.run, one rank per
GPU (RCCL).  Rank 0 prints ONE JSON line.

A plain run does only what the headline figure needs: it builds the batch, runs W warm-up
and K timed steps, writes the last timed step's results if ``--dump-outputs DIR`` is given
(mean, std, score and match of every segment as ``DIR/<name>.npy``; the batch is seeded, so
two runs with the same arguments score identical inputs) and prints the line (``value``,
``ms_per_step`` = wall milliseconds per timed step, ``roofline`` from the timed steps' own
kernel times).  ``--full`` adds every other leg described under "Extra fields" below.

Workload (BASELINE.json configs[1], "1024 concurrent synthetic 16 kHz streams,
MFCC+cosine match, 1xMI355X"): per GPU, 1024 streams x 64 gated segments =
65536 ragged segments with L ~ U{6400..33600} samples, resident
in HBM as one fp32 buffer.  Half the segments carry the reference word (gain
U(0.2,3), noise sigma U(1e-4,5e-3)), a quarter an 880 Hz burst, a quarter a
high-passed noise burst (scores ~70, below the default 75), so both decisions
occur.  A step = one scorer pass over the
whole batch: MFCC (stft+mel+log+top_db+DCT), mean/std, cosine score, match,
and the fp64 re-score of near-threshold segments.  For N>1 the step also
gathers the matched segments' (id, score) records to rank 0 over RCCL -- the
positives that feed the optional Whisper confirm: device-side
compaction, an all_gather of the counts, point-to-point records.  Streams shard
across ranks (weak scaling).

Extra fields: ``roofline`` (dominant kernel k_score_f32, 640 algorithmic bytes
per MFCC frame, HIP-event timed); with ``--full`` also ``fixed_length`` / ``short_length``
(the scorer on segments of one length), ``pcie_inclusive``, ``cpu_baseline`` (oracle/mfcc_ref.py, the
librosa-0.11 restatement, on rank 0 at N=1 only, time-bounded sample),
``streaming`` (configs[2]: 8192 streams through the full level-1 + level-2
engine, one tick per push), ``streaming_f32_max`` (as many resident streams as HBM holds
with the reference's 10 s float32 rings) and ``streaming_max`` (as many resident streams as
HBM holds with compact 3 s int16 rings fed int16 PCM -- what a PCM16
microphone delivers, stored exactly): measured per tick, never extrapolated --
every timed tick's GPU time is recorded (a HIP event pair on the engine stream around
the tick's launches; host-ingest legs add that tick's own H2D copy), and
``streams_realtime`` is the resident count when the MAX over the timed ticks is within
the 100 ms tick budget (else 0): ticks arriving every 100 ms then never queue.
"""
from __future__ import annotations

import argparse
import json
import itertools
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

METRIC = "real-time 16 kHz streams sustained + MFCC frames/sec at 1/2/4/8 GPUs"
HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec (MI355X_MICROARCH.md)
# VALU issue peak: 256 CUs x 4 SIMD-32 x one wave64 instruction per 2 cycles at the 2.4 GHz
# spec clock (= the 157.3 TF FP32 vector peak counted in FMAs; MI355X_MICROARCH.md)
VALU_PEAK_WAVE_INSTR_S = 256 * 4 * 2.4e9 / 2
BYTES_PER_FRAME = 640          # 160 new fp32 samples per MFCC frame
HOP = 160
SR = 16000


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--streams", type=int, default=1024, help="streams per GPU (config 2)")
    ap.add_argument("--segments-per-stream", type=int, default=64)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed (mean, std, score, "
                         "match of every segment) as DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="after the headline measurement also run every other leg (fixed-length and short "
                         "segments, the PCIe-inclusive pass, the CPU baselines, the streaming legs with level 3 "
                         "and host ingest); the options below select among those legs and need --full")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=10.0)
    ap.add_argument("--no-streaming", action="store_true")
    ap.add_argument("--stream-count", type=int, default=8192, help="config 3 streams per GPU")
    ap.add_argument("--stream-ticks", type=int, default=600, help="ticks after the 10 s prefill")
    ap.add_argument("--big-streams", type=int, default=1 << 23,
                    help="streams resident with the reference's full 10 s float32 rings, capped by free HBM "
                         "(0 = skip)")
    ap.add_argument("--max-streams", type=int, default=1 << 23,
                    help="streams resident with compact int16 sample rings, capped by free HBM (0 = skip)")
    ap.add_argument("--max-ring", type=int, default=48000, help="compact ring samples per stream (3 s)")
    ap.add_argument("--max-float32", action="store_true",
                    help="streaming_max with float32 input and rings instead of int16 PCM")
    ap.add_argument("--big-ticks", type=int, default=300, help="ticks after the prefill for the big runs")
    ap.add_argument("--fixed-len", type=int, default=16000,
                    help="also time the scorer on segments of this one length (0 = skip)")
    ap.add_argument("--short-len", type=int, default=6400,
                    help="also time the scorer on segments of this length (short_length; 0 = skip)")
    ap.add_argument("--confirm-batch", type=int, default=64, help="config 5: Whisper-tiny batch (0 = skip)")
    ap.add_argument("--no-pcie", dest="pcie", action="store_false",
                    help="skip the host-buffer (PCIe-inclusive) pass over the batch")
    ap.add_argument("--no-host-ingest", dest="host_ingest", action="store_false",
                    help="skip the pinned-host ingest legs (streaming_host_ingest)")
    ap.add_argument("--host-streams-f32", type=int, default=131072)
    ap.add_argument("--host-streams-i16", type=int, default=1048576)
    ap.add_argument("--host-ticks", type=int, default=200, help="timed ticks of the host-ingest legs")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


def load_word() -> np.ndarray:
    import wave
    with wave.open(os.path.join(ROOT, "tests", "golden", "reference_word.wav"), "rb") as w:
        raw = w.readframes(w.getnframes())
    return np.frombuffer(raw, dtype="<i2").astype(np.float32) / np.float32(32768.0)


def make_segments(torch, dev, n_seg, seed, word, fixed_len=0):
    """Synthetic ragged batch on the GPU (deterministic per seed); fixed_len > 0: every
    segment that many samples (SURVEY.md 8d config 2's L = 16000 / T = 101 variant)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    lengths = rng.integers(6400, 33600 + 1, n_seg).astype(np.int32)
    if fixed_len > 0:
        lengths[:] = fixed_len
    offsets = np.zeros(n_seg, np.int64)
    offsets[1:] = np.cumsum(lengths[:-1], dtype=np.int64)
    total = int(lengths.sum())
    sigma = rng.uniform(1e-4, 5e-3, n_seg)
    gain = rng.uniform(0.2, 3.0, n_seg)
    kind = rng.integers(0, 4, n_seg)             # 0,1 word; 2 tone 880 Hz; 3 high-passed noise burst
    start = (rng.random(n_seg) * np.maximum(1, lengths - len(word))).astype(np.int64)
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    pcm = torch.randn(total, generator=g, device=dev, dtype=torch.float32)
    seg_id = torch.repeat_interleave(torch.arange(n_seg, device=dev), torch.from_numpy(lengths.astype(np.int64)).to(dev))
    pcm.mul_(torch.from_numpy(sigma.astype(np.float32)).to(dev)[seg_id])
    del seg_id
    wl = len(word)
    wv = torch.from_numpy(word).to(dev)
    tone = torch.from_numpy((0.3 * np.sin(2 * np.pi * 880 * np.arange(wl) / 16000)).astype(np.float32)).to(dev)
    ar = torch.arange(wl, device=dev)
    hp = torch.randn(wl + 1, generator=g, device=dev, dtype=torch.float32)
    hp = (hp[1:] - hp[:-1]) * 0.1                 # differenced white noise: scores ~70 < 75
    for c0 in range(0, n_seg, 2048):
        c1 = min(n_seg, c0 + 2048)
        L = torch.from_numpy(lengths[c0:c1].astype(np.int64)).to(dev)
        base = torch.from_numpy(offsets[c0:c1] + start[c0:c1]).to(dev)
        room = L - torch.from_numpy(start[c0:c1]).to(dev)
        k = torch.from_numpy(kind[c0:c1]).to(dev)
        gn = torch.from_numpy(gain[c0:c1].astype(np.float32)).to(dev)
        src = torch.where((k <= 1)[:, None], wv[None, :],
                          torch.where((k == 2)[:, None], tone[None, :], hp[None, :]))
        val = src * gn[:, None]
        mask = ar[None, :] < room[:, None]
        idx = base[:, None] + ar[None, :]
        pcm.index_put_((idx[mask],), val[mask], accumulate=True)
    frames = int((1 + lengths.astype(np.int64) // HOP).sum())
    return (pcm, torch.from_numpy(offsets).to(dev), torch.from_numpy(lengths).to(dev), frames,
            lengths, offsets)


DUMP_BYTES_MAX = 64 * 10**6    # --dump-outputs writes at most this much in all


def dump_outputs(out_dir, seed, rank, world, arrays):
    """Write the scorer's per-segment results (device tensors, first axis = segment) as
    <out_dir>/<name>.npy (<name>_rank<r>.npy for N > 1): float32 stays float32, everything else
    becomes float64 (match: 0.0 / 1.0).  A batch whose results exceed DUMP_BYTES_MAX is written
    as a fixed sample of its segments, drawn from `seed`, with the sampled segments' ids in
    segment_index.npy."""
    os.makedirs(out_dir, exist_ok=True)
    host = {}
    for name, t in arrays.items():
        a = t.detach().cpu().numpy()
        host[name] = a if a.dtype == np.float32 else a.astype(np.float64)
    n = len(next(iter(host.values())))
    row = sum(a.itemsize * int(np.prod(a.shape[1:], dtype=np.int64)) for a in host.values()) + 8
    keep = DUMP_BYTES_MAX // (row * max(1, world)) - 16      # the .npy headers fit in the slack
    if n > keep:
        idx = np.sort(np.random.Generator(np.random.PCG64(seed)).choice(n, keep, replace=False))
        host = {name: np.ascontiguousarray(a[idx]) for name, a in host.items()}
        host["segment_index"] = idx.astype(np.float64)
    sfx = f"_rank{rank}" if world > 1 else ""
    for name, a in host.items():
        np.save(os.path.join(out_dir, f"{name}{sfx}.npy"), a)


# --------------------------------------------------------------------------- CPU baseline
def _pin(cpu):
    """Pin this worker process to one host CPU (None: leave it floating)."""
    if cpu is not None:
        try:
            os.sched_setaffinity(0, {int(cpu)})
        except (AttributeError, OSError):
            pass


def worker_cpus(procs):
    """One distinct CPU per worker, spread over this process's affinity mask (a GPU box may
    list 256 host CPUs for a 16-core quota: unpinned workers migrate and time-share, which
    made round 3's per-process rates spread 231 %)."""
    try:
        cpus = sorted(os.sched_getaffinity(0))
    except AttributeError:
        return [None] * procs
    if len(cpus) < procs:
        return [None] * procs
    step = len(cpus) // procs
    return [cpus[i * step] for i in range(procs)]


def _cpu_worker(args):
    seg_list, seconds, cpu = args
    _pin(cpu)
    os.environ["OMP_NUM_THREADS"] = "1"
    from oracle import mfcc_ref
    tm, ts = mfcc_ref.extract_mfcc(load_word())
    t0 = time.perf_counter()
    c0 = time.process_time()
    frames = 0
    n = 0
    # the worker's share of the batch, repeated until the round's time is up (single-threaded
    # workers get through it in well under a second)
    for x in itertools.cycle(seg_list):
        cm, cs = mfcc_ref.extract_mfcc(x.astype(np.float64))   # float64 candidate path (wakeword.py:1105-1121)
        mfcc_ref.similarity_from_stats(tm, ts, cm, cs)
        frames += 1 + len(x) // HOP
        n += 1
        if time.perf_counter() - t0 > seconds:
            break
    return frames, n, time.perf_counter() - t0, time.process_time() - c0


def host_cores():
    """(processes to use, CPUs in this process's affinity mask, cgroup CPU quota in cores or None).
    One process per usable core: the affinity count, capped by the cgroup CPU quota when one is
    set (a GPU box's job may list 256 host CPUs but own 16 of them; more processes than the
    quota would only time-share the same cores)."""
    try:
        aff = len(os.sched_getaffinity(0))
    except AttributeError:
        aff = os.cpu_count() or 1
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, period = f.read().split()[:2]
        if q != "max":
            quota = max(1, int(int(q) // int(period)))
    except (OSError, ValueError):
        pass
    return max(1, min(aff, quota) if quota else aff), aff, quota


def _rates_summary(res):
    frames = sum(r[0] for r in res)
    wall = max(r[2] for r in res)
    rates = np.array([r[0] / r[2] for r in res if r[2] > 0])   # each worker process's own rate
    return frames, wall, rates


def cpu_baseline(host_pcm, lengths, offsets, seconds, rounds=3):
    """The oracle port on `procs` pinned worker processes, `rounds` back-to-back rounds of
    seconds / rounds each in one pool after a short warm-up round.  Every round is reported;
    `value` is the best round's aggregate (the box's other tenants only ever slow a round down:
    two rounds on one box differed by 35 % in round 4) and `round_agreement_pct` how far the
    rounds' median-per-process x cores figures are apart (reproducibility)."""
    import multiprocessing as mp
    procs, aff, quota = host_cores()
    per = max(1, len(lengths) // procs)
    cpus = worker_cpus(procs)
    jobs = []
    for p in range(procs):
        idx = range(p * per, min(len(lengths), (p + 1) * per))
        jobs.append(([host_pcm[offsets[i] - offsets[0]: offsets[i] - offsets[0] + lengths[i]] for i in idx],
                     seconds / rounds, cpus[p]))
    ctx = mp.get_context("spawn")
    out_rounds = []
    with _OneThreadEnv(), ctx.Pool(procs, initializer=_pool_init) as pool:
        # an unreported ~1 s warm-up round first (imports, first-call and page-fault costs,
        # clock ramp: a first timed round ran 25 % below the second on one box)
        pool.map(_cpu_worker, [(j[0], 1.0, j[2]) for j in jobs], chunksize=1)
        for _ in range(rounds):
            res = pool.map(_cpu_worker, jobs, chunksize=1)
            frames, wall, rates = _rates_summary(res)
            # frames per second of the process's own CPU time: what a core does while the process
            # runs on it (wall time also counts cgroup throttling and other tenants' time slices)
            cpu_rates = np.array([r[0] / r[3] for r in res if r[3] > 0])
            out_rounds.append({"value": frames / wall, "median_x_cores": float(np.median(rates) * procs),
                               "cpu_time_x_cores": float(np.median(cpu_rates) * procs),
                               "segments": sum(r[1] for r in res), "frames": frames, "rates": rates})
    last = max(out_rounds, key=lambda r: r["value"])   # the best round
    rates = last["rates"]
    mx = [r["median_x_cores"] for r in out_rounds]
    cx = [r["cpu_time_x_cores"] for r in out_rounds]
    return {"value": last["value"], "unit": "frames/s", "cores": procs, "host_cores_affinity": aff,
            "cpu_quota_cores": quota, "kind": "port", "pinned": cpus[0] is not None,
            "statistic": f"best of {rounds} rounds",
            # robust to one slow or one unusually idle core: the median process rate x cores
            "median_x_cores": last["median_x_cores"],
            "rounds": [{"value": r["value"], "median_x_cores": r["median_x_cores"],
                        "cpu_time_x_cores": r["cpu_time_x_cores"]} for r in out_rounds],
            "round_agreement_pct": float(100.0 * (max(mx) - min(mx)) / max(1e-9, float(np.mean(mx)))),
            # the same per-process medians over CPU time instead of wall time: the reproducible
            # figure on a shared host (it leaves out the time the process was not running)
            "cpu_time_x_cores": float(np.median(cx)),
            "cpu_time_agreement_pct": float(100.0 * (max(cx) - min(cx)) / max(1e-9, float(np.mean(cx)))),
            # per-core rate and its spread over the worker processes: the aggregate depends on
            # how many cores the box's cgroup grants and how busy its other tenants keep them
            "per_core": {"median": float(np.median(rates)), "min": float(rates.min()), "max": float(rates.max()),
                         "spread_pct": float(100.0 * (rates.max() - rates.min()) / np.median(rates)),
                         "unit": "frames/s per process"},
            "sample": f"{last['segments']} segment scorings ({last['frames']} MFCC frames; each process cycles over its "
                      f"{per} segments of the same ragged batch) per round, "
                      f"float64 candidate path, oracle/mfcc_ref.py (numpy/scipy restatement of librosa 0.11.0 mfcc + "
                      f"scipy cosine), {procs} pinned processes x {rounds} rounds x ~{seconds / rounds:.0f} s, "
                      f"OMP_NUM_THREADS=1"}


def event_sources(word, rng):
    """[5, len(word)] float32 event sources of the streaming recipe:
    the word, then distractors -- an 880 Hz tone burst and the time-reversed word (both
    score above 75 against the word, false positives of the reference's matcher: MFCC
    mean/std are time-symmetric and dominated by c0), a high-passed noise burst (scores
    ~50-80) and a loud white-noise burst (negative similarity -> NaN score, no match)."""
    wl = len(word)
    tt = np.arange(wl, dtype=np.float64) / SR
    peak = float(np.abs(word).max())
    return np.stack([word, peak * 0.5 * np.sin(2 * np.pi * 880.0 * tt), word[::-1],
                     np.diff(rng.standard_normal(wl + 1)) * 0.5,
                     rng.standard_normal(wl) * 1.5]).astype(np.float32)


def event_kind(rng, n):
    """Per-event source index: the word with probability 1/2, else one of the four distractors."""
    return np.where(rng.random(n) < 0.5, 0, rng.integers(1, 5, n))


def _cpu_stream_worker(args):
    """Faithful CPU level 1 + level 2 (oracle/gate_ref.py DetectorRef + mfcc_ref scoring of every
    emitted segment) on one synthetic stream of the streaming bench's recipe, ~`seconds` of work."""
    seed, seconds, cpu = args
    _pin(cpu)
    os.environ["OMP_NUM_THREADS"] = "1"
    from oracle import gate_ref, mfcc_ref
    word = load_word()
    tm, ts = mfcc_ref.extract_mfcc(word)
    rng = np.random.Generator(np.random.PCG64(seed))
    P = 160 * 1600
    pcm = (rng.standard_normal(P) * rng.uniform(1e-4, 3e-3)).astype(np.float32)
    table = event_sources(word, rng)
    for e in range(5):
        pos = e * P // 5 + int(rng.integers(0, 8000))
        src = table[int(event_kind(rng, 1)[0])]
        pcm[pos:pos + len(word)] += (src * rng.uniform(0.3, 2.0)).astype(np.float32)
    det = gate_ref.DetectorRef(gate_ref.GateConfig(), keep_audio=True)
    t0 = time.perf_counter()
    ticks = 0
    while time.perf_counter() - t0 < seconds:
        k = ticks % 160
        ev = det.push_tick(pcm[k * 1600:(k + 1) * 1600])
        if ev is not None and not ev.skipped:
            cm, cs = mfcc_ref.extract_mfcc(ev.audio)
            mfcc_ref.similarity_from_stats(tm, ts, cm, cs)
        ticks += 1
    wall = time.perf_counter() - t0
    return ticks, wall


def cpu_stream_baseline(seconds, procs):
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    with _OneThreadEnv(), ctx.Pool(procs, initializer=_pool_init) as pool:
        cpus = worker_cpus(procs)
        res = pool.map(_cpu_stream_worker, [(9000 + p, seconds, cpus[p]) for p in range(procs)], chunksize=1)
    rtf = sum(t * 0.1 / w for t, w in res)       # seconds of audio per second, summed over processes
    per = np.array([t * 0.1 / w for t, w in res])
    return {"value": rtf, "unit": "streams sustained in real time", "cores": procs, "kind": "port",
            "pinned": cpus[0] is not None, "median_x_cores": float(np.median(per) * procs),
            "per_core": {"median": float(np.median(per)), "min": float(per.min()), "max": float(per.max()),
                         "spread_pct": float(100.0 * (per.max() - per.min()) / np.median(per)),
                         "unit": "real-time streams per process"},
            "sample": f"{procs} processes x ~{seconds:.0f} s, each one synthetic stream of the streaming recipe "
                      f"through oracle/gate_ref.py DetectorRef (ring, block RMS, pct25, FSM, cut) + "
                      f"oracle/mfcc_ref.py level 2 per emitted segment, OMP_NUM_THREADS=1"}


_ONE_THREAD = {"OMP_NUM_THREADS": "1", "OPENBLAS_NUM_THREADS": "1", "MKL_NUM_THREADS": "1"}


def _pool_init():
    os.environ.update(_ONE_THREAD)
    sys.path.insert(0, ROOT)
    try:   # a spawned worker imported numpy (bench.py) before this ran: cap the BLAS pool now
        from threadpoolctl import threadpool_limits
        threadpool_limits(1)
    except ImportError:
        pass


class _OneThreadEnv:
    """The worker pool's processes start with one BLAS / OpenMP thread each (the variables are
    read when numpy loads, before any initializer runs): `cores` counts the threads used."""

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in _ONE_THREAD}
        os.environ.update(_ONE_THREAD)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# --------------------------------------------------------------------------- streaming (config 3)
def confirm_bench(se, ev, final_tick, batch, dev):
    """Level 3: GPU normalisation of gathered positives straight from the
    rings (bit-exact wakeword.py:1019-1025), then one batched Whisper-tiny decode."""
    import torch
    from easywakeword_amd.confirm import WhisperConfirm
    pos = ev[(ev["match"] != 0) & ((ev["flags"] & 1) == 0) & (ev["tick"] > final_tick - 80)]
    pos = pos[np.argsort(-pos["tick"], kind="stable")][:batch]
    if len(pos) == 0:
        return {"segments": 0}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    audio = se.normalize_events_device(pos)          # float64, stays on the GPU
    t1 = time.perf_counter()
    wc = WhisperConfirm(device=dev)
    wc.transcribe(audio)                            # warm-up at the timed shape (kernels, allocator)
    torch.cuda.synchronize()
    reps = 3
    t2 = time.perf_counter()
    for _ in range(reps):
        wc.transcribe(audio)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    whisper_s = (t3 - t2) / reps
    return {"segments": int(len(pos)), "normalize_ms": (t1 - t0) * 1e3, "whisper_batch_ms": whisper_s * 1e3,
            "segments_per_s": len(pos) / (whisper_s + t1 - t0), "max_new_tokens": wc.max_new_tokens,
            "model": "whisper-tiny dims (transformers WhisperConfig default), random init: no weights offline "
                     "(timing only, parity unpinned)"}


def fixed_length_bench(torch, dev, ewa, eng, word, n_seg, seed, sh, fixed_len=16000, reps=5):
    """Scorer kernel on n_seg segments of one fixed length (default L = 16000, T = 101 frames each)."""
    pcm, d_off, d_len, frames, _, _ = make_segments(torch, dev, n_seg, seed + 17, word, fixed_len=fixed_len)
    mean = torch.empty((n_seg, 20), device=dev, dtype=torch.float32)
    std = torch.empty((n_seg, 20), device=dev, dtype=torch.float32)
    score = torch.empty(n_seg, device=dev, dtype=torch.float64)
    match = torch.empty(n_seg, device=dev, dtype=torch.uint8)

    def step():
        eng.score_device(pcm.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n_seg, mean.data_ptr(),
                         std.data_ptr(), score.data_ptr(), match.data_ptr(), sh)

    step()
    torch.cuda.synchronize()
    eng.profile(True)
    for _ in range(reps):
        step()
    torch.cuda.synchronize()
    k_ms, k_n = eng.profile_read(0)
    eng.profile(False)
    ms = k_ms / max(1, k_n)
    out = {"segment_samples": fixed_len, "segments": n_seg, "frames_per_launch": frames, "kernel_ms": ms,
           "frames_per_s": frames / (ms / 1e3), "roofline_frac": frames * BYTES_PER_FRAME / (ms / 1e3) / (HBM_PEAK_GBS * 1e9),
           "matches": int(match.sum().item())}
    del pcm
    return out


def pcie_inclusive_bench(torch, eng, pcm, lengths, offsets, frames, reps=3):
    """The same batch through the host-buffer boundary (ewk_score_segments: the caller's PCM in
    PINNED host memory, copied to HBM, scored, results copied back, one call per batch): the
    PCIe-inclusive rate, bounded by the H2D copy of 640 B per frame.  Never the bench `value`."""
    host = torch.empty(pcm.numel(), dtype=torch.float32, pin_memory=True)
    host.copy_(pcm)
    torch.cuda.synchronize()
    h = host.numpy()
    off = np.ascontiguousarray(offsets - offsets[0], dtype=np.int64)
    ln = np.ascontiguousarray(lengths, dtype=np.int32)
    eng.score_packed(h, off, ln)                # warm-up (device buffers sized)
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        eng.score_packed(h, off, ln)
        times.append(time.perf_counter() - t0)
    t = float(np.median(times))
    del host, h
    return {"boundary": "ewk_score_segments, PCM from pinned host memory, one call per batch (copy in, "
                        "score, results out; synchronous)", "segments": int(len(ln)), "frames": int(frames),
            "call_ms_median": t * 1e3, "frames_per_s": frames / t, "h2d_bytes": int(pcm.numel() * 4),
            "h2d_gbs_effective": pcm.numel() * 4 / t / 1e9}


def make_streams(torch, dev, n_streams, seed, word):
    """The streaming recipe on the GPU: per stream a 16 s loop (160 ticks) of N(0, sigma)
    noise with five events at jittered positions (half words, half distractors).
    Returns (period_ticks, pcm[n_streams, period_ticks * 1600] float32)."""
    period_ticks = 160                       # 16 s loop per stream, distinct per stream
    P = period_ticks * 1600
    g = torch.Generator(device=dev)
    g.manual_seed(seed + 7)
    rng = np.random.Generator(np.random.PCG64(seed + 11))
    sig = torch.from_numpy(rng.uniform(1e-4, 3e-3, n_streams).astype(np.float32)).to(dev)
    pcm = torch.randn((n_streams, P), generator=g, device=dev, dtype=torch.float32) * sig[:, None]
    wl = len(word)
    table = torch.from_numpy(event_sources(word, rng)).to(dev)
    for e in range(5):
        pos = (e * P // 5 + rng.integers(0, 8000, n_streams)).astype(np.int64)
        gain = torch.from_numpy(rng.uniform(0.3, 2.0, n_streams).astype(np.float32)).to(dev)
        kind = event_kind(rng, n_streams)
        src = table[torch.from_numpy(kind).to(dev)] * gain[:, None]
        idx = torch.from_numpy(pos).to(dev)[:, None] + torch.arange(wl, device=dev)[None, :]
        pcm.scatter_add_(1, idx, src)
    torch.cuda.synchronize()
    return period_ticks, pcm


def make_shifted_signal(torch, dev, n_streams, n_ticks, seed, word, pcm16=False):
    """Input for very many streams in bounded memory: one long synthetic signal of
    n_streams + n_ticks ticks (N(0, sigma) noise, sigma redrawn every 16 s, an event every
    U(2.4, 4.0) s: half words, half distractors, gain U(0.3, 2)); stream s hears it from
    tick s on, i.e. stream s's tick t is signal[(s + t) * 1600 :][:1600] (push stride =
    tick stride = 1600).  Every tick reads n_streams distinct rows (no cache reuse
    within a tick); 6.4 KB per stream instead of a private 16 s loop (1 MB)."""
    total = (n_streams + n_ticks) * 1600
    rng = np.random.Generator(np.random.PCG64(seed + 13))
    g = torch.Generator(device=dev)
    g.manual_seed(seed + 5)
    piece = 16 * SR
    n_piece = -(-total // piece)
    sig = torch.empty((n_piece, piece), device=dev, dtype=torch.float32)
    sig.normal_(generator=g)
    sig.mul_(torch.from_numpy(rng.uniform(1e-4, 3e-3, n_piece).astype(np.float32)).to(dev)[:, None])
    sig = sig.view(-1)
    total = sig.numel()
    wl = len(word)
    gaps = rng.uniform(2.4, 4.0, int(total / SR / 2.4) + 2)
    pos = (np.cumsum(gaps) * SR).astype(np.int64)
    pos = pos[pos + wl < total]
    table = torch.from_numpy(event_sources(word, rng)).to(dev)
    kind = torch.from_numpy(event_kind(rng, len(pos))).to(dev)
    gain = torch.from_numpy(rng.uniform(0.3, 2.0, len(pos)).astype(np.float32)).to(dev)
    ar = torch.arange(wl, device=dev)
    for c0 in range(0, len(pos), 4096):
        c1 = min(len(pos), c0 + 4096)
        idx = torch.from_numpy(pos[c0:c1]).to(dev)[:, None] + ar[None, :]
        sig.index_put_((idx.reshape(-1),), (table[kind[c0:c1]] * gain[c0:c1, None]).reshape(-1), accumulate=True)
    if pcm16:   # what a PCM16 microphone delivers: round(x * 32768), saturated (the float copy is freed)
        q = torch.empty(sig.numel(), device=dev, dtype=torch.int16)
        for i0 in range(0, sig.numel(), 1 << 28):
            i1 = min(sig.numel(), i0 + (1 << 28))
            q[i0:i1] = torch.round(sig[i0:i1] * 32768.0).clamp_(-32768, 32767).to(torch.int16)
        del sig
        torch.cuda.empty_cache()
        sig = q
    torch.cuda.synchronize()
    return sig


def tick_stats(ms) -> dict:
    """Per-tick latency summary (ms) and the real-time verdict: every tick within 100 ms."""
    a = np.asarray(ms, dtype=np.float64)
    if not len(a):
        return {"tick_ms_max": None, "tick_ms_p999": None, "tick_ms_p50": None, "ticks_over_100ms": None}
    return {"tick_ms_max": float(a.max()), "tick_ms_p999": float(np.percentile(a, 99.9)),
            "tick_ms_p99": float(np.percentile(a, 99.0)), "tick_ms_p50": float(np.median(a)),
            "tick_ms_mean": float(a.mean()), "ticks_timed": int(len(a)),
            "ticks_over_100ms": int((a > 100.0).sum())}


def fit_streams(torch, dev, ring_samples, signal_ticks, reserve=8 << 30, sample_bytes=4):
    """Largest multiple of 65,536 streams whose engine + shared input signal fit in the
    free HBM (ring, block-RMS arrays, state, two event banks, one tick of signal each;
    an int16 signal's float32 staging is freed before the engine is built)."""
    free, _ = torch.cuda.mem_get_info(dev)
    per = ring_samples * sample_bytes + 3 * (10 * SR // 1600) * 8 + 96 + 2 * 4 * 48 + 1600 * sample_bytes
    n = int((free - reserve - signal_ticks * 1600 * sample_bytes) // per)
    return max(65536, n // 65536 * 65536)


def streaming_bench(torch, dev, eng_mod, n_streams, n_ticks, seed, word, world=1, first_stream=0, cdev=None,
                    confirm_batch=0, ring_samples=0, shifted=False, prof_ticks=200, pcm16=False):
    """Full level-1 + level-2 engine on `n_streams` RESIDENT synthetic streams: 10 s
    prefill, then `n_ticks` ticks launched one at a time (the real-time cadence).
    shifted=False: a private 16 s loop per stream (make_streams); True: the shared
    long signal of make_shifted_signal (for 10^5-10^6 streams).  ring_samples > 0:
    compact sample rings (ewk_config.ring_samples; same events and scores).  pcm16: int16
    PCM input (shifted signal only) into int16 rings (EWK_RING_I16, exact; half the bytes).
    With world > 1 every tick also gathers the ranks' positive detections
    {stream, tick, length, score} to rank 0 over RCCL (easywakeword_amd.shard.gather_positives)."""
    prof_ticks = min(prof_ticks, n_ticks)
    if shifted:
        pcm = make_shifted_signal(torch, dev, n_streams, 100 + n_ticks + prof_ticks, seed, word, pcm16=pcm16)
        period_ticks, stride = None, 1600
    else:
        period_ticks, pcm = make_streams(torch, dev, n_streams, seed, word)
        stride = period_ticks * 1600
    se = eng_mod.StreamEngine(n_streams, gpu=dev.index if dev.index is not None else 0,
                              ring_samples=int(ring_samples), ring_format=1 if pcm16 else 0)
    push = se.push_device_pcm16 if pcm16 else se.push_device
    es = 2 if pcm16 else 4
    se.template_from_pcm(word)
    base = pcm.data_ptr()

    events = []
    es_ = torch.cuda.ExternalStream(se.stream_handle(), device=dev)
    tick_ev = []    # (start, end) event pair per timed tick, on the engine stream
    col = None
    if world > 1:   # level-3 feed: positives to rank 0 every second, PCM of the newest 64 per rank
        from easywakeword_amd.shard import PositiveCollector
        col = PositiveCollector(first_stream, cdev, every=10, audio_cap=64,
                                audio_fn=(se.normalize_events_device if cdev.type == "cuda" else
                                          lambda e: [a.cpu() for a in se.normalize_events_device(e)]))

    def run(t0, nt, per_call, lagged=False, timed=False):
        t = t0
        while t < t0 + nt:
            if period_ticks is None:
                k, n = t, min(per_call, nt - (t - t0))
            else:
                k = t % period_ticks
                n = min(per_call, nt - (t - t0), period_ticks - k)
            if timed:   # the stream reaches e0 when the previous tick's last kernel is done
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(es_)
            push(base + k * 1600 * es, stride, 1600, n)
            if timed:
                e1.record(es_)
                tick_ev.append((e0, e1))
            # the host consumes detections every call; lagged: tick t-1's events while the GPU runs tick t
            ev = se.poll(lagged=lagged)
            events.append(ev)
            if col is not None:             # positives of every rank -> rank 0 (level-3 input)
                col.add(ev)
                col.tick(n)
            t += n
        return t

    t = run(0, 100, 32)                      # prefill (ring fill + detection start)
    se.sync()
    events.clear()
    torch.cuda.synchronize()
    w0 = time.perf_counter()
    t = run(t, n_ticks, 1, lagged=True, timed=True)   # one tick per call: the real-time cadence, pipelined
    events.append(se.poll())                 # the last tick's events
    se.sync()
    wall = time.perf_counter() - w0
    torch.cuda.synchronize()
    lat = tick_stats([a.elapsed_time(b) for a, b in tick_ev])
    ev = np.concatenate(events) if events else np.zeros(0, dtype=se.poll().dtype)
    # per-kernel times from a separate instrumented pass (event records stay out of the timed wall)
    events.clear()
    se.profile(True)
    t = run(t, prof_ticks, 1, lagged=True)
    events.append(se.poll())
    se.sync()
    gate_ms, gate_n = se.profile_read(2)
    sc_ms, sc_n = se.profile_read(0)
    r_ms, r_n = se.profile_read(1)
    se.profile(False)
    ev_latest = np.concatenate(events) if events else ev
    per_tick = wall / n_ticks
    real = ev[(ev["flags"] & 1) == 0]
    gate_ms_tick = gate_ms / max(1, gate_n)
    ring = int(ring_samples) if ring_samples else 10 * SR
    out = {"streams": n_streams, "resident": True, "ticks": n_ticks, "audio_seconds_per_stream": n_ticks * 0.1,
           "input": ("shared long signal, stream s from tick s (make_shifted_signal)" if shifted
                     else "private 16 s loop per stream (make_streams)") + (", int16 PCM" if pcm16 else ", float32"),
           "ring_samples_per_stream": ring, "ring_format": "int16" if pcm16 else "float32",
           "ring_bytes_total": ring * es * n_streams,
           "wall_s": wall, "ms_per_tick": per_tick * 1e3, **lat,
           "realtime": lat["tick_ms_max"] is not None and lat["tick_ms_max"] <= 100.0,
           "realtime_headroom": 100.0 / lat["tick_ms_max"] if lat["tick_ms_max"] else None,
           # measured, never extrapolated: the resident count if the slowest of the timed ticks
           # (its GPU time, tick start -> tick end on the engine stream) fit the 100 ms tick
           # budget, else 0
           "streams_realtime": float(n_streams) if lat["tick_ms_max"] is not None and lat["tick_ms_max"] <= 100.0
                               else 0.0,
           "realtime_criterion": "max over timed ticks of the tick's GPU time <= 100 ms",
           "gate_kernel_ms_per_tick": gate_ms_tick,
           # the gate's algorithmic bytes: 1600 samples read + written to the ring per stream-tick
           "gate_bytes_per_stream_tick": 2 * 1600 * es,
           "gate_hbm_frac": n_streams * 2 * 1600 * es / (gate_ms_tick / 1e3) / (HBM_PEAK_GBS * 1e9)
                            if gate_ms_tick else None,
           "scorer_kernel_ms_per_tick": sc_ms / max(1, sc_n),
           "rescore_kernel_ms_per_tick": r_ms / max(1, r_n),
           "kernel_times": f"separate instrumented pass of {prof_ticks} ticks",
           "events": int(len(real)), "matches": int(real["match"].sum()) if len(real) else 0,
           "mfcc_frames": int((1 + real["length"].astype(np.int64) // HOP).sum()) if len(real) else 0}
    out["mfcc_frames_per_s"] = out["mfcc_frames"] / wall   # gated segments scored, over the timed ticks
    if col is not None:
        col.flush()
        out["positives_gathered_to_rank0"] = col.gathered
        out["positive_pcm_gathered_to_rank0"] = col.gathered_audio
        out["gather"] = "every 10 ticks: counts all_gather + point-to-point records and normalised PCM to rank 0"
    if confirm_batch > 0:   # config 5: level 3 on the latest positives still in the rings
        out["confirm"] = confirm_bench(se, ev_latest, t, confirm_batch, dev)
    se.close()
    del pcm
    return out


def streaming_host_bench(torch, dev, eng_mod, n_streams, n_ticks, seed, word, ring_samples=0, pcm16=False,
                         prefill=100):
    """End-to-end ingest: every tick's PCM of all `n_streams` streams starts in PINNED HOST
    memory (what a capture server holds after its sockets / sound cards deliver a block per
    stream), is DMA'd to the GPU over PCIe on a copy stream (double-buffered device staging,
    tick t+1's copy overlapping tick t's gate and scorer), then pushed (the reference's
    callback ingest, wakeword.py:438-444, 454-470).  Input: make_shifted_signal, so tick t of
    all streams is ONE contiguous host slice of n_streams x 1600 samples and every tick moves
    n_streams x 6.4 KB (3.2 KB int16) over PCIe -- the real per-tick volume."""
    sig = make_shifted_signal(torch, dev, n_streams, prefill + n_ticks + 1, seed, word, pcm16=pcm16)
    host = torch.empty(sig.numel(), dtype=sig.dtype, pin_memory=True)
    host.copy_(sig)
    del sig
    torch.cuda.empty_cache()
    es = 2 if pcm16 else 4
    se = eng_mod.StreamEngine(n_streams, gpu=dev.index if dev.index is not None else 0,
                              ring_samples=int(ring_samples), ring_format=1 if pcm16 else 0)
    push = se.push_device_pcm16 if pcm16 else se.push_device
    se.template_from_pcm(word)
    per = n_streams * 1600
    stage = [torch.empty(per, dtype=host.dtype, device=dev) for _ in range(2)]
    cs = torch.cuda.Stream(dev)
    es_ = torch.cuda.ExternalStream(se.stream_handle(), device=dev)
    free = [torch.cuda.Event() for _ in range(2)]
    free_used = [False, False]
    cev = {}        # tick -> (start, end) events of its own H2D copy on the copy stream
    comp = {}       # tick -> (start, end) events of its kernels on the engine stream

    def copy(t):
        b = t % 2
        with torch.cuda.stream(cs):
            if free_used[b]:
                cs.wait_event(free[b])          # the gate of tick t-2 has read this staging buffer
            c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            c0.record(cs)
            stage[b].copy_(host[t * 1600: t * 1600 + per], non_blocking=True)
            c1.record(cs)
            cev[t] = (c0, c1)

    events = []

    def run(t0, nt, timed):
        copy(t0)
        for t in range(t0, t0 + nt):
            b = t % 2
            if t + 1 < t0 + nt:
                copy(t + 1)                     # the next tick's DMA, ahead of this tick's kernels
            es_.wait_event(cev[t][1])
            if timed:   # the engine stream starts the tick once its copy and the previous tick are done
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(es_)
            push(stage[b].data_ptr(), 1600, 0, 1)
            if timed:
                e1.record(es_)
                comp[t] = (e0, e1)
            free[b].record(es_)
            free_used[b] = True
            events.append(se.poll(lagged=True))
        events.append(se.poll())

    run(0, prefill, False)
    se.sync()
    torch.cuda.synchronize()
    events.clear()
    w0 = time.perf_counter()
    run(prefill, n_ticks, True)
    se.sync()
    torch.cuda.synchronize()
    wall = time.perf_counter() - w0
    ev = np.concatenate(events)
    real = ev[(ev["flags"] & 1) == 0]
    per_tick = wall / n_ticks
    # a tick's latency from its PCM in host memory to its detections: its own H2D copy, then
    # its kernels (in real time the copy starts when the block arrives and nothing queues);
    # both from that tick's own event pairs (one shared pair per staging buffer was
    # re-recorded by the next copy before it was read)
    ticks = range(prefill, prefill + n_ticks)
    copy_ms = [cev[t][0].elapsed_time(cev[t][1]) for t in ticks]
    comp_ms = [comp[t][0].elapsed_time(comp[t][1]) for t in ticks]
    h2d = float(np.median(copy_ms)) if copy_ms else None
    lat = tick_stats([c + k for c, k in zip(copy_ms, comp_ms)])
    lat["compute_ms_max"] = float(max(comp_ms)) if comp_ms else None
    out = {"streams": n_streams, "resident": False, "ingest": "pinned host -> HBM DMA every tick (copy stream, "
                                                            "double-buffered), then push",
           "ticks": n_ticks, "ring_format": "int16" if pcm16 else "float32",
           "ring_samples_per_stream": int(ring_samples) or 10 * SR,
           "h2d_bytes_per_tick": per * es, "h2d_ms_per_tick_median": h2d,
           "h2d_gbs": per * es / (h2d / 1e3) / 1e9 if h2d else None,
           "wall_s": wall, "ms_per_tick": per_tick * 1e3, **lat,
           "realtime": lat["tick_ms_max"] is not None and lat["tick_ms_max"] <= 100.0,
           "realtime_headroom": 100.0 / lat["tick_ms_max"] if lat["tick_ms_max"] else None,
           "streams_realtime": float(n_streams) if lat["tick_ms_max"] is not None and lat["tick_ms_max"] <= 100.0
                               else 0.0,
           "realtime_criterion": "max over timed ticks of (the tick's H2D copy + its GPU time) <= 100 ms",
           "events": int(len(real)), "matches": int(real["match"].sum()) if len(real) else 0}
    se.close()
    del host, stage
    torch.cuda.empty_cache()
    return out


def _rccl_version(torch):
    try:
        v = torch.cuda.nccl.version()
        return ".".join(str(x) for x in v) if isinstance(v, tuple) else str(v)
    except Exception as exc:   # noqa: BLE001 - reported, not fatal
        return f"unavailable ({type(exc).__name__})"


# --------------------------------------------------------------------------- main
def main():
    args = parse()
    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and rank == 0:
        print(f"warning: --gpus {args.gpus} but WORLD_SIZE {world}", file=sys.stderr)
    # EWK_BENCH_BACKEND=gloo rehearses the N>1 path with several ranks on one GPU
    # (collectives on CPU copies); the real multi-GPU run uses RCCL ("nccl").
    backend = os.environ.get("EWK_BENCH_BACKEND", "nccl")
    local = local % max(1, torch.cuda.device_count())
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    cdev = dev if backend == "nccl" else torch.device("cpu")   # where collective buffers live
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    import easywakeword_amd as ewa
    word = load_word()
    n_seg = args.streams * args.segments_per_stream
    pcm, d_off, d_len, frames, lengths, offsets = make_segments(torch, dev, n_seg, args.seed + 1000 * rank, word)
    mean = torch.empty((n_seg, 20), device=dev, dtype=torch.float32)
    std = torch.empty((n_seg, 20), device=dev, dtype=torch.float32)
    score = torch.empty(n_seg, device=dev, dtype=torch.float64)
    match = torch.empty(n_seg, device=dev, dtype=torch.uint8)
    eng = ewa.Engine(gpu=local)
    eng.template_from_pcm(word)
    stream = torch.cuda.Stream(dev)          # a real (non-null) stream shared by the kernel, RCCL and events
    torch.cuda.set_stream(stream)
    sh = stream.cuda_stream
    assert sh != 0
    if world > 1:   # positives only: device compaction, counts all_gather, P2P records (tests/test_dist_gloo.py)
        from easywakeword_amd.shard import MatchGather
        # the matched segments' (id, score, step) records stay on the device across the
        # steps of a loop and go to rank 0 (the confirm stage's input) in ONE gather per
        # loop: no host sync inside the loop
        gather = MatchGather(n_seg, rank * n_seg, cdev, steps=max(args.steps, args.warmup, 1))
    gathered = [0]

    def step():
        eng.score_device(pcm.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n_seg, mean.data_ptr(),
                         std.data_ptr(), score.data_ptr(), match.data_ptr(), sh)
        if world > 1:
            gather.add(score.to(cdev), match.to(cdev))

    def flush():
        if world > 1:
            rec = gather.flush()
            gathered[0] = 0 if rec is None else int(rec.shape[0])

    torch.cuda.synchronize()
    for _ in range(args.warmup):
        step()
    flush()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    eng.profile(True)
    ev0 = torch.cuda.Event(enable_timing=True)
    ev1 = torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    ev0.record(stream)
    for _ in range(args.steps):
        step()
    flush()   # the K steps' positives -> rank 0, inside the timed region
    ev1.record(stream)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    k_ms, k_n = eng.profile_read(0)
    r_ms, r_n = eng.profile_read(1)
    eng.profile(False)
    step_ms = ev0.elapsed_time(ev1) / args.steps
    t_rank = torch.tensor([wall], dtype=torch.float64, device=cdev)
    if world > 1:
        dist.all_reduce(t_rank, op=dist.ReduceOp.MAX)
    t_max = float(t_rank.item())
    frames_all = torch.tensor([frames], dtype=torch.float64, device=cdev)   # ranks' ragged batches differ
    if world > 1:
        dist.all_reduce(frames_all)
    value = float(frames_all.item()) * args.steps / t_max
    n_match = int(match.sum().item())
    n_nan = int(torch.isnan(score).sum().item())
    if args.dump_outputs:   # the last timed step's results, before any other leg runs
        dump_outputs(args.dump_outputs, args.seed, rank, world,
                     {"mean": mean, "std": std, "score": score, "match": match})

    full = args.full
    fixed = fixed_length_bench(torch, dev, ewa, eng, word, n_seg, args.seed + 1000 * rank, sh) \
        if full and args.fixed_len > 0 and world == 1 else None
    # the reference's shortest gated segment (0.4 s: speech_duration_min 0.3 s + padding), where
    # the per-segment fixed cost weighs most
    short = fixed_length_bench(torch, dev, ewa, eng, word, n_seg, args.seed + 1000 * rank, sh,
                               fixed_len=args.short_len) if full and args.short_len > 0 and world == 1 else None
    pcie = pcie_inclusive_bench(torch, eng, pcm, lengths, offsets, frames) \
        if full and args.pcie and world == 1 else None
    kernel_s = (k_ms / max(1, k_n)) / 1e3
    achieved = frames * BYTES_PER_FRAME / kernel_s / 1e9
    traffic, traffic_src, compute = None, None, None
    tf = os.path.join(ROOT, "profiles", "traffic_k_score_f32.json")
    if os.path.exists(tf):   # PMC-measured HBM bytes/frame of this kernel (scripts/gpu_round.sh pmc)
        with open(tf) as fh:
            t = json.load(fh)
        traffic = t["traffic_bytes_per_frame"] * frames / 1e9
        traffic_src = f"profiles/traffic_k_score_f32.json ({t['segments']} segments, {t['method']})"
        if t.get("valu_instr_per_frame"):
            # the bound that actually binds k_score_f32: VALU issue
            ach = t["valu_instr_per_frame"] * frames / kernel_s
            compute = {"bound": "valu-issue", "achieved": ach / 1e12, "peak": VALU_PEAK_WAVE_INSTR_S / 1e12,
                       "unit": "T wave64-instr/s", "frac": ach / VALU_PEAK_WAVE_INSTR_S,
                       "valu_instr_per_frame": t["valu_instr_per_frame"],
                       "frames_per_s_at_valu_peak": VALU_PEAK_WAVE_INSTR_S / t["valu_instr_per_frame"],
                       "source": "SQ_INSTS_VALU per frame from profiles/traffic_k_score_f32.json x frames / "
                                 "HIP-event kernel time; peak at the 2.4 GHz spec clock"}

    out = {
        "metric": METRIC,
        "value": value,
        "unit": "frames/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "full": full,
        "ms_per_step": t_max / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "fp32",
        "data": "synthetic (ragged segments built from tests/golden/reference_word.wav + Gaussian noise, seeded)",
        "config": {
            "workload": f"configs[1]: {args.streams} streams x {args.segments_per_stream} gated segments per GPU "
                        f"(L~U{{6400..33600}}), MFCC(20,512,160)+cosine match per segment",
            "segments_per_gpu": n_seg,
            "frames_per_step_per_gpu": frames,
            "frames_per_step_all_gpus": int(frames_all.item()),
            "global_batch": n_seg * world,
            "parallelism": f"dp{world} (stream shards, RCCL gather of positive records to rank 0)" if world > 1
                           else "dp1",
        },
        "roofline": {
            "bound": "hbm",
            "kernel": "k_score_f32",
            "achieved": achieved,
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": achieved / HBM_PEAK_GBS,
            "traffic": traffic,
            "traffic_unit": "GB per launch",
            "traffic_source": traffic_src,
            "kernel_ms": kernel_s * 1e3,
            "launches": k_n,
            "algorithmic_bytes_per_launch": frames * BYTES_PER_FRAME,
        },
        "compute_roofline": compute,
        "step_event_ms": step_ms,
        "rescore_kernel_ms": r_ms / max(1, r_n),
        "matches_per_step": n_match,
        "nan_scores": n_nan,
    }
    if fixed is not None:
        out["fixed_length"] = fixed
    if short is not None:
        out["short_length"] = short
    if pcie is not None:
        out["pcie_inclusive"] = pcie
    if world > 1:   # what the collectives actually ran on (a SCALE run can check RCCL saw N ranks)
        out["distributed"] = {"world_size_seen": dist.get_world_size(), "backend": str(dist.get_backend()),
                              "rccl_version": _rccl_version(torch), "positives_gathered_to_rank0": gathered[0],
                              "gather": "positives held on the device over the timed loop, one counts all_gather + "
                                        "point-to-point records to rank 0 after its last step (inside the timing)"}

    streaming = full and not args.no_streaming
    if full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        sample = min(n_seg, max(16, host_cores()[0]) * 400)
        host = pcm[: int(offsets[sample - 1] + lengths[sample - 1])].cpu().numpy()
        out["cpu_baseline"] = cpu_baseline(host, lengths[:sample], offsets[:sample], args.cpu_seconds)
        if streaming:
            out["cpu_baseline"]["streaming"] = cpu_stream_baseline(min(args.cpu_seconds, 10.0),
                                                                   out["cpu_baseline"]["cores"])
    if streaming:
        del pcm
        torch.cuda.empty_cache()
        st = streaming_bench(torch, dev, ewa, args.stream_count, args.stream_ticks, args.seed + rank, word,
                             world=world, first_stream=rank * args.stream_count, cdev=cdev,
                             confirm_batch=args.confirm_batch if rank == 0 else 0)
        out["streaming"] = st
        best = st["streams_realtime"]
        for key, n_req, ring, p16 in (("streaming_f32_max", args.big_streams, 0, False),
                                      ("streaming_max", args.max_streams, args.max_ring, not args.max_float32)):
            if n_req <= 0:
                continue
            torch.cuda.empty_cache()
            n = min(n_req, fit_streams(torch, dev, ring or 10 * SR, 100 + 2 * args.big_ticks,
                                       sample_bytes=2 if p16 else 4))
            r = streaming_bench(torch, dev, ewa, n, args.big_ticks, args.seed + 31 * rank, word, world=world,
                                first_stream=rank * n, cdev=cdev, ring_samples=ring, shifted=True, prof_ticks=50,
                                pcm16=p16)
            r["requested_streams"] = n_req
            out[key] = r
            best = max(best, r["streams_realtime"])
        if args.host_ingest and world == 1:
            # end-to-end ingest from pinned host memory (the resident legs above start with the
            # audio already in HBM): the reference's 10 s float32 rings, and 3 s int16 rings
            hi = {}
            for key, n_req, ring, p16 in (("f32_131072", args.host_streams_f32, 0, False),
                                          ("i16_1048576", args.host_streams_i16, args.max_ring, True)):
                if n_req <= 0:
                    continue
                torch.cuda.empty_cache()
                n = min(n_req, fit_streams(torch, dev, ring or 10 * SR, 0, sample_bytes=2 if p16 else 4))
                hi[key] = streaming_host_bench(torch, dev, ewa, n, args.host_ticks, args.seed + 47, word,
                                               ring_samples=ring, pcm16=p16)
                hi[key]["requested_streams"] = n_req
            out["streaming_host_ingest"] = hi
            out["streams_realtime_host_ingest"] = max([r["streams_realtime"] for r in hi.values()] or [0.0])
        tot = torch.tensor([best], dtype=torch.float64, device=cdev)
        if world > 1:
            dist.all_reduce(tot)
        out["streams_realtime_total"] = float(tot.item())
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
