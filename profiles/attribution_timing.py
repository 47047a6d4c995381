"""Time one feature attribution two ways (profiles/attribution_note.md):

(a) ``SAEAttribution.attribute``: wsae_layernorm_rows -> wsae_encode_topk -> wsae_attribute, per stage and in total;
(b) what the public API allowed before it: torch LayerNorm -> ``sae.encode`` (dense [rows, H]) -> dense
    ``(sigma G / gamma) @ W_d`` -> multiply by the dense code -> column sums.

384 -> 3072, k = 32, fp32 hidden states and gradient, 16384 rows, bf16 ctx, every feature ablated.  The two are timed in
alternating blocks with device events after a warm-up, and their per-feature sums are compared before anything is timed.
``--trace`` runs only a few calls of (a), for a kernel trace taken from outside:

    python profiles/attribution_timing.py [--rows 16384] [--dims D H K] [--iters 200] [--out outputs/attribution_timing.json]
    rocprofv3 --kernel-trace --stats -d outputs/attribution_trace -- python profiles/attribution_timing.py --trace
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
from whisper_sae.causal import SAEAttribution  # noqa: E402
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
    ap.add_argument("--dims", type=int, nargs=3, default=[384, 3072, 32], metavar=("D", "H", "K"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--trace", action="store_true", help="a few calls of the new path only (for rocprofv3)")
    ap.add_argument("--out", default="outputs/attribution_timing.json")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    (D, H, K), rows = args.dims, args.rows

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
    grad = (torch.randn(rows, D, device=dev) * 1e-2).contiguous()
    at = SAEAttribution(sae, layer_norm=norm)

    def new_path():
        return at.attribute(h, grad)

    def old_path():
        a = torch.nn.functional.layer_norm(h, (D,), norm.weight, norm.bias, norm.eps)
        code = sae.encode(a)
        sigma = torch.sqrt(h.var(dim=-1, unbiased=False, keepdim=True) + norm.eps)
        s = (sigma * grad / norm.weight) @ sae.decoder.weight  # [rows, H]: every feature's direction against every row
        per_entry = -code * s
        return per_entry.sum(dim=0), per_entry.abs().sum(dim=0)

    with torch.no_grad():
        if args.trace:
            for _ in range(10):
                new_path()
            torch.cuda.synchronize()
            print("trace run done")
            return
        res = new_path()
        old_sum, old_abs = old_path()
        torch.cuda.synchronize()
        gap = float((res.feat_sum - old_sum).abs().max())
        scale = float(res.feat_abs.max())
        # (sae.decoder.weight is fp32, the kernel reads the bf16 shadow the ctx's decode reads: agreement to bf16 precision)
        assert gap <= 2e-2 * scale, f"the two paths disagree: {gap} at scale {scale}"
        active = int((res.vals > 0).sum())

        # (a) per stage: the three stages of attribute() on their own
        eng = sae.bind()
        st = eng.stream()
        gamma, beta, eps = at._ops.norm_tensors(norm, eng.device)
        a_buf = torch.empty(rows, D, dtype=torch.float32, device=dev)
        attr = torch.empty(rows, K, dtype=torch.float32, device=dev)
        fsum, fabs = torch.empty(H, device=dev), torch.empty(H, device=dev)
        frows = torch.empty(H, dtype=torch.int32, device=dev)
        ws_bytes = int(eng.lib.wsae_attribute_workspace_bytes(H))
        ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev)
        state = {}

        def stage_ln():
            N.check(eng.lib.wsae_layernorm_rows(h.data_ptr(), N.DT_F32, rows, D, gamma.data_ptr(), beta.data_ptr(), eps,
                                                a_buf.data_ptr(), N.DT_F32, st), "wsae_layernorm_rows")

        def stage_code():
            _, state["handle"], _, state["vals"], state["idx"] = sae._code(a_buf, training=False)

        def stage_attribute(per_feature=True):
            N.check(eng.lib.wsae_attribute(state["handle"], eng.pack.data_ptr(), h.data_ptr(), N.DT_F32, grad.data_ptr(),
                                           N.DT_F32, rows, state["vals"].data_ptr(), state["idx"].data_ptr(),
                                           gamma.data_ptr(), eps, 0, 0, attr.data_ptr(),
                                           fsum.data_ptr() if per_feature else 0, fabs.data_ptr() if per_feature else 0,
                                           frows.data_ptr() if per_feature else 0, ws.data_ptr(), ws.numel() * 8, st),
                    "wsae_attribute")

        def stage_attr_only():
            stage_attribute(per_feature=False)

        stage_ln(), stage_code(), stage_attribute()
        for fn in (new_path, old_path, stage_ln, stage_code, stage_attribute, stage_attr_only):
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        t_new, t_old = [], []
        for _ in range(4):  # alternate the two, in blocks
            t_new += timed(new_path, args.iters // 4)
            t_old += timed(old_path, args.iters // 4)
        stages = {"wsae_layernorm_rows": summary(timed(stage_ln, args.iters)),
                  "encode (wsae_prepare + wsae_encode_topk launches, SAE._code)": summary(timed(stage_code, args.iters)),
                  "wsae_attribute (memset + 3 kernels)": summary(timed(stage_attribute, args.iters)),
                  "wsae_attribute, attr only (1 kernel)": summary(timed(stage_attr_only, args.iters))}

    result = {"shape": {"D": D, "H": H, "k": K, "rows": rows, "hidden_dtype": "fp32", "grad_dtype": "fp32", "ctx": "bf16",
                        "edit": "ablate all"},
              "entries_with_nonzero_weight": active, "max_abs_gap_feat_sum_new_vs_old": gap, "feat_abs_scale": scale,
              "new_attribute": summary(t_new), "old_composition": summary(t_old), "new_stages": stages,
              "device": torch.cuda.get_device_name(0), "torch": torch.__version__}
    result["ratio_old_over_new"] = result["old_composition"]["median_us"] / result["new_attribute"]["median_us"]
    out_path = Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
