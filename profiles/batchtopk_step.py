#!/usr/bin/env python3
"""Step time of the BatchTopK SAE next to the TopK SAE, same box, same run.

    python profiles/batchtopk_step.py [--batch 16384] [--steps 50] [--windows 7] [--only topk|batchtopk]

384 -> 3072, k = 32, BatchTopK cap 64, bf16 (use_amp), one ``SAETrainer.train_step`` per step on a batch resident on the
device.  The two trainers alternate window by window (median of the windows reported), so clock and thermal drift hit
both alike.  ``--only`` runs one of them (for a ``rocprofv3 --kernel-trace --stats`` run of that step alone).  Prints
one JSON line.
"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for _p in (str(ROOT), str(ROOT / "whisper-sae_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

D, H, K, KMAX = 384, 3072, 32, 64


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only", choices=("topk", "batchtopk"), default=None)
    a = ap.parse_args()

    import torch

    from whisper_sae.config import TrainingConfig
    from whisper_sae.sae import BatchTopKSAE, SAETrainer, TopKSAE

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    x = torch.randn(a.batch, D, device=dev).to(torch.bfloat16)
    cfg = TrainingConfig(batch_size=a.batch, learning_rate=1e-4, warmup_steps=0, use_amp=True, num_workers=0)
    tmp = tempfile.TemporaryDirectory(prefix="btk_step_")
    runs = {}
    for name in ("topk", "batchtopk"):
        if a.only and a.only != name:
            continue
        torch.manual_seed(1)
        m = TopKSAE(D, H, k=K) if name == "topk" else BatchTopKSAE(D, H, k=K, max_k_per_row=KMAX)
        runs[name] = SAETrainer(m.to(dev), cfg, device="cuda:0", run_dir=tmp.name)
    for tr in runs.values():
        for _ in range(a.warmup):
            tr.train_step(x)
    torch.cuda.synchronize()
    times = {n: [] for n in runs}
    for _ in range(a.windows):
        for n, tr in runs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.steps):
                tr.train_step(x)
            t1.record()
            t1.synchronize()
            times[n].append(t0.elapsed_time(t1) * 1e3 / a.steps)
    out = {"config": {"D": D, "H": H, "k": K, "max_k_per_row": KMAX, "batch": a.batch, "precision": "bf16",
                      "steps_per_window": a.steps, "windows": a.windows},
           "step_us_median": {n: round(statistics.median(v), 2) for n, v in times.items()},
           "step_us_windows": {n: [round(t, 2) for t in v] for n, v in times.items()}}
    if len(runs) == 2:
        out["ratio_batchtopk_over_topk"] = round(out["step_us_median"]["batchtopk"] / out["step_us_median"]["topk"], 4)
    if "batchtopk" in runs:
        sel = runs["batchtopk"].model.last_selection()
        out["last_selection"] = {"t": sel.threshold, "saturated_rows": sel.saturated_rows, "kept": sel.kept,
                                 "kept_per_row": sel.kept / a.batch}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
