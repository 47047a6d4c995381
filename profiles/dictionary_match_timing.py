"""Time the nearest-feature search two ways (profiles/dictionary_match_note.md):

(a) ``nearest_features`` = ``wsae_match_rows``: stage (normalise / convert) -> GEMM with the selection as its epilogue ->
    merge of the column splits; the similarity matrix is never written;
(b) what the public API allowed before it: ``F.normalize`` both -> ``A @ B.T`` -> ``.topk(n)``, chunked over rows of A
    where the dense matrix would exceed 2 GiB (the chunk is reported).  bf16 mode of (b): the normalised operands are cast
    to bf16, the product is a bf16 matrix, the top-k runs on it.

Shapes 3072^2 x 384, 12288^2 x 768, 40960^2 x 1280, n = 4, both modes, random unit-scale rows, B != A.  One process,
alternating windows of (a) and (b), device events, median and p10-p90.  Before anything is timed the two are compared:
the fraction of rows whose best match agrees (near-ties may resolve differently in bf16) and the largest gap between
the best-match values.  ``--trace`` runs only a few calls of (a) at 12288^2 x 768, for a kernel trace from outside:

    python profiles/dictionary_match_timing.py [--out outputs/dictionary_match_timing.json]
    rocprofv3 --kernel-trace --stats -d outputs/match_trace -- python profiles/dictionary_match_timing.py --trace
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "whisper-sae_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from whisper_sae import _native as N  # noqa: E402
from whisper_sae.analysis import nearest_features  # noqa: E402

BF16_DENSE_PEAK_TFLOPS = 2500.0             # as bench.py
FP32_MFMA_PEAK_TFLOPS = 2500.0 / 16.0       # v_mfma_f32_32x32x2_f32 runs at 1/16 of the bf16 rate
SHAPES = [(3072, 384, 40), (12288, 768, 10), (40960, 1280, 3)]  # (H, D, calls per window)
DENSE_LIMIT = 2 << 30


def timed(fn, iters: int) -> list:
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


def torch_composition(a, b, n, precision, chunk):
    an, bn = F.normalize(a, dim=1), F.normalize(b, dim=1)
    if precision == "bf16":
        an, bn = an.bfloat16(), bn.bfloat16()
    vals, idx = [], []
    for r0 in range(0, a.shape[0], chunk):
        v, i = (an[r0:r0 + chunk] @ bn.T).topk(n, dim=1)
        vals.append(v)
        idx.append(i)
    return torch.cat(vals).float(), torch.cat(idx)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--trace", action="store_true", help="a few calls of the new path only (for rocprofv3)")
    ap.add_argument("--out", default="outputs/dictionary_match_timing.json")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)

    if args.trace:
        a = torch.randn(12288, 768, device=dev, generator=gen)
        b = torch.randn(12288, 768, device=dev, generator=gen)
        for precision in ("fp32", "bf16"):
            for _ in range(5):
                nearest_features(a, b, n=args.n, precision=precision)
        torch.cuda.synchronize()
        print("trace run done")
        return

    results = []
    for H, D, iters in SHAPES:
        a = torch.randn(H, D, device=dev, generator=gen)
        b = torch.randn(H, D, device=dev, generator=gen)
        chunk = H if H * H * 4 <= DENSE_LIMIT else 8192
        flop = 2.0 * H * H * D
        for precision in ("fp32", "bf16"):
            def new_path():
                return nearest_features(a, b, n=args.n, precision=precision)

            def old_path():
                return torch_composition(a, b, args.n, precision, chunk)

            nv, ni = new_path()
            ov, oi = old_path()
            torch.cuda.synchronize()
            agree = float((ni[:, 0].long() == oi[:, 0]).float().mean())
            gap = float((nv[:, 0] - ov[:, 0]).abs().max())
            del nv, ni, ov, oi
            for fn in (new_path, old_path):
                for _ in range(2):
                    fn()
            torch.cuda.synchronize()
            t_new, t_old = [], []
            for _ in range(args.windows):
                t_new += timed(new_path, iters)
                t_old += timed(old_path, iters)
            peak = BF16_DENSE_PEAK_TFLOPS if precision == "bf16" else FP32_MFMA_PEAK_TFLOPS
            sn, so = summary(t_new), summary(t_old)
            ws = int(N.lib().wsae_match_workspace_bytes(H, H, D, args.n, N.PREC_BF16 if precision == "bf16" else N.PREC_FP32))
            row = {"rows_a": H, "rows_b": H, "dim": D, "n": args.n, "precision": precision, "torch_row_chunk": chunk,
                   "torch_dense_bytes_per_chunk": chunk * H * (2 if precision == "bf16" else 4), "workspace_bytes": ws,
                   "best_match_agreement": agree, "best_value_max_gap": gap, "wsae_match_rows": sn, "torch_composition": so,
                   "ratio_torch_over_new": so["median_us"] / sn["median_us"],
                   "whole_call_tflops": flop / sn["median_us"] / 1e6, "mfma_peak_tflops": peak,
                   "whole_call_fraction_of_peak": flop / sn["median_us"] / 1e6 / peak}
            print(json.dumps(row), flush=True)
            results.append(row)
        del a, b
        torch.cuda.empty_cache()
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "windows": args.windows, "results": results}
    out_path = Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
