"""Time one feature intervention two ways (profiles/intervention_note.md):

(a) ``SAEIntervention.apply``: wsae_layernorm_rows -> wsae_encode_topk -> wsae_intervene, per launch and in total;
(b) what the public API allowed before it: torch LayerNorm -> ``sae.encode`` (dense [rows, H]) -> scale one column of a
    copy -> ``sae.decode`` of the edited and of the unedited code -> inverse norm in torch.

384 -> 3072, k = 32, fp32 hidden states, 16384 rows, bf16 ctx, one ablated feature, keep_error.  The two are timed in
alternation with device events after a warm-up, and their outputs are compared before anything is timed.

    python profiles/intervention_timing.py [--rows 16384] [--iters 200] [--out outputs/intervention_timing.json]
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

from whisper_sae import _native as N  # noqa: E402
from whisper_sae.causal import FeatureEdit, SAEIntervention  # noqa: E402
from whisper_sae.sae.model import TopKSAE  # noqa: E402


def timed(fn, iters: int) -> list:
    """Device time of each of ``iters`` calls, in microseconds."""
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for start, end in pairs:
        start.record()
        fn()
        end.record()
    torch.cuda.synchronize()
    return [start.elapsed_time(end) * 1e3 for start, end in pairs]


def summary(samples: list) -> dict:
    a = np.asarray(samples)
    return {"median_us": float(np.median(a)), "p10_us": float(np.percentile(a, 10)), "p90_us": float(np.percentile(a, 90)),
            "n": int(a.size)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default="outputs/intervention_timing.json")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    D, H, K, rows = 384, 3072, 32, args.rows

    torch.manual_seed(0)
    sae = TopKSAE(D, H, k=K, precision="bf16")
    with torch.no_grad():
        sae.decoder.weight.mul_(10.0)
        sae.b_pre.normal_(0.0, 0.1)
    sae = sae.to(dev).eval()
    norm = torch.nn.LayerNorm(D).to(dev)
    with torch.no_grad():
        norm.weight.uniform_(0.5, 1.5)
        norm.bias.normal_(0.0, 0.3)
    h = (torch.randn(rows, D, device=dev) * 2.0 + 0.5).contiguous()

    # the batch's most frequent feature is the one ablated
    probe = SAEIntervention(sae, FeatureEdit(), layer_norm=norm)
    probe.apply(h)
    vals, idx = probe.last_code
    counts = torch.bincount(idx[vals > 0].long().flatten(), minlength=H)
    feature = int(counts.argmax())
    iv = SAEIntervention(sae, FeatureEdit.ablate([feature]), layer_norm=norm)

    def new_path():
        return iv.apply(h)

    def old_path():
        a = torch.nn.functional.layer_norm(h, (D,), norm.weight, norm.bias, norm.eps)
        code = sae.encode(a)
        edited = code.clone()
        edited[:, feature] *= 0.0
        a2 = a + (sae.decode(edited) - sae.decode(code))
        mu = h.mean(dim=-1, keepdim=True)
        sigma = torch.sqrt(h.var(dim=-1, unbiased=False, keepdim=True) + norm.eps)
        return mu + sigma * (a2 - norm.bias) / norm.weight

    with torch.no_grad():
        out_new, out_old = new_path(), old_path()
        torch.cuda.synchronize()
        gap = float((out_new - out_old).abs().max())
        scale = float(out_new.abs().max())
        changed = iv.last_changed_rows
        assert gap <= 1e-3 * scale, f"the two paths disagree: {gap} at scale {scale}"

        # (a) per launch: the three stages of apply() on their own
        eng = sae.bind()
        st = eng.stream()
        gamma, beta, eps = iv._norm_tensors(norm, eng.device)
        a_buf = torch.empty(rows, D, dtype=torch.float32, device=dev)
        scale_t, fidx, fval, n_force = iv.edit.tables(H, dev)
        out = torch.empty_like(h)
        cnt = torch.zeros(1, dtype=torch.int32, device=dev)
        state = {}

        def stage_ln():
            N.check(eng.lib.wsae_layernorm_rows(h.data_ptr(), N.DT_F32, rows, D, gamma.data_ptr(), beta.data_ptr(), eps,
                                                a_buf.data_ptr(), N.DT_F32, st), "wsae_layernorm_rows")

        def stage_code():
            _, state["handle"], _, state["vals"], state["idx"] = sae._code(a_buf, training=False)

        def stage_intervene():
            N.check(eng.lib.wsae_intervene(state["handle"], eng.pack.data_ptr(), h.data_ptr(), N.DT_F32, rows,
                                           state["vals"].data_ptr(), state["idx"].data_ptr(), gamma.data_ptr(),
                                           beta.data_ptr(), eps, scale_t.data_ptr(), fidx.data_ptr(), fval.data_ptr(),
                                           n_force, 0, N.IV_KEEP_ERROR, out.data_ptr(), N.DT_F32, cnt.data_ptr(), st),
                    "wsae_intervene")

        stage_ln(), stage_code(), stage_intervene()
        for fn in (new_path, old_path, stage_ln, stage_code, stage_intervene):
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        t_new, t_old = [], []
        for _ in range(4):  # alternate the two, in blocks
            t_new += timed(new_path, args.iters // 4)
            t_old += timed(old_path, args.iters // 4)
        stages = {"wsae_layernorm_rows": summary(timed(stage_ln, args.iters)),
                  "encode (wsae_prepare + wsae_encode_topk launches, SAE._code)": summary(timed(stage_code, args.iters)),
                  "wsae_intervene": summary(timed(stage_intervene, args.iters))}

    result = {"shape": {"D": D, "H": H, "k": K, "rows": rows, "hidden_dtype": "fp32", "ctx": "bf16", "mode": "keep_error"},
              "ablated_feature": feature, "rows_changed": changed, "max_abs_gap_new_vs_old": gap, "output_scale": scale,
              "new_apply": summary(t_new), "old_composition": summary(t_old), "new_stages": stages,
              "device": torch.cuda.get_device_name(0), "torch": torch.__version__}
    result["ratio_old_over_new"] = result["old_composition"]["median_us"] / result["new_apply"]["median_us"]
    out_path = Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
