"""How the first-order feature table compares with exact ablations (profiles/attribution_note.md).

Seeded random-init tiny Whisper (the recipe of the causal tests), an fp32 TopK SAE 64 -> 512, k = 8, on encoder layer 1.
``attribution_effects`` gives the estimate for every feature from one forward and one backward; the 32 features with the
largest ``|attribution|`` are then ablated one at a time with ``WhisperIntervention`` and the same metric (batch mean of
the first decoder step's log-probability of the clean argmax token) is measured exactly.  Reported: sign agreement,
Spearman rank correlation and the relative size of the gap.  A finding for the note, not a test.

    python profiles/attribution_vs_ablation.py [--out outputs/attribution_vs_ablation.json]
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "whisper-sae_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from whisper_sae.causal import FeatureEdit, SAEIntervention, WhisperIntervention, attribution_effects  # noqa: E402
from whisper_sae.causal.hooks import _first_step  # noqa: E402
from whisper_sae.sae.model import TopKSAE  # noqa: E402


def ranks(x: np.ndarray) -> np.ndarray:
    order = np.argsort(x, kind="stable")
    r = np.empty(len(x))
    r[order] = np.arange(len(x))
    return r


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--top", type=int, default=32)
    ap.add_argument("--out", default="outputs/attribution_vs_ablation.json")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    from transformers import WhisperConfig, WhisperForConditionalGeneration
    dev = "cuda:0"
    cfg = WhisperConfig(vocab_size=200, num_mel_bins=80, encoder_layers=2, decoder_layers=2, encoder_attention_heads=2,
                        decoder_attention_heads=2, encoder_ffn_dim=128, decoder_ffn_dim=128, d_model=64,
                        max_source_positions=50, max_target_positions=16, decoder_start_token_id=1, pad_token_id=0,
                        bos_token_id=1, eos_token_id=2)
    torch.manual_seed(0)
    model = WhisperForConditionalGeneration(cfg).eval().to(dev)
    mel = torch.from_numpy(np.random.default_rng(5).standard_normal((4, 80, 100)).astype(np.float32)).to(dev)
    torch.manual_seed(50)
    sae = TopKSAE(64, 512, k=8, precision="fp32")
    with torch.no_grad():
        sae.decoder.weight.mul_(10.0)
        sae.b_pre.normal_(0.0, 0.1)
    sae = sae.to(dev).eval()
    tap = ("encoder", 1)

    table = attribution_effects(model, mel, sae, tap, top_n=args.top)
    with torch.no_grad():
        _, logp0 = _first_step(model, mel, None)
        token = logp0.argmax(dim=-1, keepdim=True)
        m0 = float(logp0.gather(1, token).mean())
        rows = []
        for f, entry in table["features"].items():
            with WhisperIntervention(model, {tap: SAEIntervention(sae, FeatureEdit.ablate([int(f)]))}):
                _, logp1 = _first_step(model, mel, None)
            exact = float(logp1.gather(1, token).mean()) - m0
            rows.append({"feature": int(f), "attribution": entry["attribution"], "exact_ablation": exact,
                         "rows_active": entry["rows_active"]})
    est = np.array([r["attribution"] for r in rows])
    exact = np.array([r["exact_ablation"] for r in rows])
    moved = exact != 0
    result = {"tap": list(tap), "metric": table["metric"], "metric_value": m0, "n_features": len(rows),
              "sign_agreement": float(np.mean(np.sign(est[moved]) == np.sign(exact[moved]))) if moved.any() else None,
              "spearman": float(np.corrcoef(ranks(est), ranks(exact))[0, 1]),
              "spearman_of_magnitudes": float(np.corrcoef(ranks(np.abs(est)), ranks(np.abs(exact)))[0, 1]),
              "median_relative_gap": float(np.median(np.abs(est[moved] - exact[moved]) / np.abs(exact[moved]))) if moved.any() else None,
              "features": rows, "device": torch.cuda.get_device_name(0)}
    out_path = Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
