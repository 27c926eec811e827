"""bench.dump_outputs (--dump-outputs DIR): the last timed step's per-segment results as
float32 / float64 .npy files, whole when they fit the byte cap, else a fixed seeded sample."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


@pytest.fixture(scope="module")
def results():
    torch = pytest.importorskip("torch")
    g = torch.Generator().manual_seed(5)
    n = 1000
    score = torch.randn(n, generator=g, dtype=torch.float64)
    score[7] = float("nan")
    return {"mean": torch.randn(n, 20, generator=g), "std": torch.randn(n, 20, generator=g), "score": score,
            "match": (torch.rand(n, generator=g) > 0.5).to(torch.uint8)}


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_whole_batch(results, tmp_path):
    bench.dump_outputs(str(tmp_path / "o"), 1234, 0, 1, results)
    got = _load(tmp_path / "o")
    assert sorted(got) == ["match", "mean", "score", "std"]
    assert got["mean"].dtype == np.float32 and got["std"].dtype == np.float32
    assert got["score"].dtype == np.float64 and got["match"].dtype == np.float64
    for k, a in got.items():
        assert np.array_equal(a, results[k].numpy().astype(a.dtype), equal_nan=True), k
    assert set(np.unique(got["match"])) <= {0.0, 1.0}


def test_dump_sample_is_fixed_and_within_the_cap(results, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 50000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), 1234, 0, 1, results)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 50000
    idx = a["segment_index"].astype(np.int64)
    assert 0 < len(idx) < 1000 and np.all(np.diff(idx) > 0)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
        if k != "segment_index":
            assert np.array_equal(a[k], results[k].numpy()[idx].astype(a[k].dtype), equal_nan=True), k


def test_plain_run_is_not_full(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    args = bench.parse()
    assert args.full is False and args.dump_outputs is None and args.steps == 3
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    args = bench.parse()
    assert args.full is True and args.dump_outputs == "d"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()
