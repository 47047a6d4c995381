"""``bench.py``: the plain run (exactly ``--steps`` timed steps, the headline fields only) and ``--dump-outputs`` (what
the last timed step left to its caller, float32 / float64, at most 64 MB, identical inputs from run to run)."""

from __future__ import annotations

import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import bench

ROOT = Path(__file__).resolve().parents[1]


class TestWriteOutputs:
    def test_small_outputs_are_written_whole(self, tmp_path):
        arrays = {"w": np.arange(12, dtype=np.float32).reshape(3, 4), "loss": np.array(0.5),
                  "counts": np.arange(5, dtype=np.int64)}
        bench.write_outputs(tmp_path, arrays)
        assert sorted(p.name for p in tmp_path.iterdir()) == ["counts.npy", "loss.npy", "w.npy"]
        w, loss, counts = (np.load(tmp_path / f"{n}.npy") for n in ("w", "loss", "counts"))
        assert w.dtype == np.float32 and np.array_equal(w, arrays["w"])
        assert loss.dtype == np.float64 and loss.shape == () and float(loss) == 0.5
        assert counts.dtype == np.float64 and np.array_equal(counts, np.arange(5))

    def test_large_outputs_are_sampled_under_the_limit(self, tmp_path):
        limit = 40_000
        arrays = {"big": np.arange(20_000, dtype=np.float32), "bigger": np.arange(30_000, dtype=np.float64),
                  "tiny": np.ones(3, np.float32)}
        shapes = bench.write_outputs(tmp_path / "a", arrays, limit=limit)
        bench.write_outputs(tmp_path / "b", arrays, limit=limit)
        assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) <= limit
        assert shapes["tiny"] == ((3,), (3,)) and shapes["big"][1] == (20_000,) and shapes["big"][0][0] < 20_000
        for name, a in arrays.items():
            s = np.load(tmp_path / "a" / f"{name}.npy")
            assert s.dtype == a.dtype
            assert np.array_equal(s, np.load(tmp_path / "b" / f"{name}.npy"))  # the same sample every time
            assert np.isin(s, a).all()
        for name in ("big", "bigger"):  # distinct elements of the arange, in storage order
            assert np.all(np.diff(np.load(tmp_path / "a" / f"{name}.npy")) > 0)


def test_step_outputs_name_the_state_and_the_metrics():
    from whisper_sae.sae.model import TopKSAE
    from whisper_sae.sae.training import TrainingMetrics
    m = TopKSAE(16, 64, k=4)
    met = TrainingMetrics(loss=1.5, reconstruction_loss=1.5, sparsity_loss=0.0, l0=4.0, dead_feature_ratio=0.25,
                          learning_rate=1e-4, step=7)
    out = bench.step_outputs(m, met)
    for k, v in m.state_dict().items():
        assert out[k].shape == tuple(v.shape)
        assert out[k].dtype == (np.float32 if v.is_floating_point() else np.float64)
    assert out["metrics.loss"] == 1.5 and out["metrics.step"] == 7.0 and out["metrics.dead_feature_ratio"] == 0.25
    assert "metrics.grad_norm" not in out  # not a field of a host-side record


def _plain_run(cwd: Path, dump: Path) -> dict:
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--batch", "2048",
           "--ring-rows", "65536", "--dump-outputs", str(dump)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=cwd)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-1000:]
    return json.loads(lines[0])


def _tree() -> set:
    return {p for p in ROOT.rglob("*") if not {"__pycache__", ".pytest_cache", ".git"} & set(p.relative_to(ROOT).parts)}


@pytest.mark.gpu
def test_plain_run_times_steps_and_dumps_the_same_outputs_twice(tmp_path):
    before = _tree()
    runs = [_plain_run(tmp_path, tmp_path / f"out{i}") for i in range(2)]
    assert _tree() == before  # nothing written into the checkout, which may be read-only
    for j in runs:
        assert j["steps"] == 3 and len(j["windows_ms_per_step"]) == 1 and j["ms_per_step"] > 0
        assert j["unit"] == "activations/s" and j["higher_is_better"] is True and j["dtype"] == "bf16"
        assert j["value"] == pytest.approx(2048 * 1e3 / j["ms_per_step"])
        assert not {"cpu_baseline", "roofline", "probe_kernel_us", "strip_predict"} & set(j)
    names = sorted(p.name for p in (tmp_path / "out0").iterdir())
    assert names == sorted(p.name for p in (tmp_path / "out1").iterdir())
    assert {"encoder.weight.npy", "decoder.weight.npy", "b_pre.npy", "metrics.loss.npy", "metrics.grad_norm.npy"} <= set(names)
    assert sum((tmp_path / "out0" / n).stat().st_size for n in names) <= 64 * 10**6
    for n in names:
        a, b = np.load(tmp_path / "out0" / n), np.load(tmp_path / "out1" / n)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), n
        assert np.array_equal(a, b), n  # same arguments, same inputs: the path is bit-reproducible run to run
    assert float(np.load(tmp_path / "out0" / "metrics.loss.npy")) == pytest.approx(runs[0]["final_loss"], rel=1e-6)
    w = torch.from_numpy(np.load(tmp_path / "out0" / "decoder.weight.npy"))
    assert torch.allclose(w.norm(dim=0), torch.ones(w.shape[1]), atol=1e-5)  # the step renormalised the columns
