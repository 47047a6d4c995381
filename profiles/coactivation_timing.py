"""Time the co-firing count two ways (profiles/coactivation_note.md):

(a) ``wsae_coact_update``: one integer atomic per (active entry of A in the window, active entry of B) of every row,
    straight from the two compact codes;
(b) what the public API allowed before it: ``wsae_densify`` of both codes to ``[B, H]``, then
    ``(a > 0).to(bf16).T @ (b > 0).to(bf16)`` (the window's columns of a) added into an fp32 table.  The product is asked
    for in fp32 (``out_dtype``) where torch offers it, since a bf16 result cannot hold a count above 256 exactly; which
    form ran, and whether its table equals (a)'s, is reported.

Shapes 3072^2, 12288^2 and a 4096-row window of 40960^2; k = 32; B = 16384; distinct indices per row, drawn uniformly
and with Zipf-like feature frequencies (weight 1 / (1 + f): hot features contend for their cells).  One process,
alternating windows of (a) and (b), device events, median and p10-p90.  ``wsae_coact_top`` (n = 4) is timed alone on
the table the updates left.  ``--trace`` runs a few calls of (a) and of the selection only, for a kernel trace:

    python profiles/coactivation_timing.py [--out outputs/coactivation_timing.json]
    rocprofv3 --kernel-trace --stats -d outputs/coact_trace -- python profiles/coactivation_timing.py --trace
"""

from __future__ import annotations

import argparse
import ctypes as C
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

K, B = 32, 16384
SHAPES = [(3072, 0, 3072, 20), (12288, 0, 12288, 10), (40960, 8192, 4096, 5)]  # (H, a_lo, a_rows, calls per window)
METRICS = {"jaccard": N.COACT_JACCARD, "phi": N.COACT_PHI}


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


def draw_code(H: int, gen, skewed: bool):
    """[B, K] code with distinct indices per row (Gumbel top-k: sampling without replacement by feature weight) and
    about a fifth of the values <= 0."""
    idx = torch.empty(B, K, dtype=torch.int32, device="cuda:0")
    logw = -torch.log1p(torch.arange(H, device="cuda:0", dtype=torch.float32)) if skewed else None
    for r0 in range(0, B, 2048):
        g = -torch.log(-torch.log(torch.rand(2048, H, device="cuda:0", generator=gen).clamp_(1e-20, 1.0 - 1e-7)))
        if skewed:
            g += logw
        idx[r0:r0 + 2048] = g.topk(K, dim=1).indices.int()
    vals = torch.randn(B, K, device="cuda:0", generator=gen) + 0.85
    return vals.contiguous(), idx.contiguous()


class Ctx:
    """A bare ctx of the C ABI, for ``wsae_densify`` alone."""

    def __init__(self, H: int):
        self.handle = C.c_void_p()
        cfg = N.Config(32, H, K, B, N.PREC_FP32, 0)
        N.check(N.lib().wsae_ctx_create(C.byref(cfg), C.byref(self.handle)), "wsae_ctx_create")

    def densify(self, code, out):
        N.check(N.lib().wsae_densify(self.handle, code[0].data_ptr(), code[1].data_ptr(), B, out.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream), "wsae_densify")

    def close(self):
        N.check(N.lib().wsae_ctx_destroy(self.handle), "wsae_ctx_destroy")


def mm_fp32(x, y):
    """bf16 x bf16 -> fp32 where this torch can; else the bf16 product widened (inexact above 256)."""
    try:
        return torch.mm(x, y, out_dtype=torch.float32), "fp32_out"
    except (TypeError, RuntimeError):
        return torch.mm(x, y).float(), "bf16_out"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--trace", action="store_true", help="a few calls of the new kernels only (for rocprofv3)")
    ap.add_argument("--out", default="outputs/coactivation_timing.json")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    lib = N.lib()
    stream = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    results = []
    for H, a_lo, a_rows, iters in SHAPES:
        counts = torch.zeros(a_rows, H, dtype=torch.int32, device=dev)
        fire_a = torch.zeros(H, dtype=torch.int32, device=dev)
        fire_b = torch.zeros(H, dtype=torch.int32, device=dev)
        total = torch.zeros(1, dtype=torch.int64, device=dev)
        out_v = torch.empty(a_rows, 4, dtype=torch.float32, device=dev)
        out_i = torch.empty(a_rows, 4, dtype=torch.int32, device=dev)
        out_c = torch.empty(a_rows, 4, dtype=torch.int32, device=dev)

        def clear():
            for t in (counts, fire_a, fire_b, total):
                t.zero_()

        def top(metric):
            N.check(lib.wsae_coact_top(counts.data_ptr(), H, a_lo, a_rows, H, fire_a.data_ptr(), fire_b.data_ptr(),
                                       total.data_ptr(), METRICS[metric], 1, 0, 4, out_v.data_ptr(), out_i.data_ptr(),
                                       out_c.data_ptr(), None, 0, stream()), "wsae_coact_top")

        for skewed in (False, True):
            ca, cb = draw_code(H, gen, skewed), draw_code(H, gen, skewed)

            def new_path():
                N.check(lib.wsae_coact_update(ca[0].data_ptr(), ca[1].data_ptr(), K, H, cb[0].data_ptr(), cb[1].data_ptr(), K,
                                              H, B, None, a_lo, a_rows, counts.data_ptr(), H, fire_a.data_ptr(),
                                              fire_b.data_ptr(), total.data_ptr(), None, 0, stream()), "wsae_coact_update")

            if args.trace:
                for _ in range(3):
                    new_path()
                for metric in METRICS:
                    for _ in range(3):
                        top(metric)
                torch.cuda.synchronize()
                continue

            ctx = Ctx(H)
            da = torch.empty(B, H, dtype=torch.float32, device=dev)
            db = torch.empty(B, H, dtype=torch.float32, device=dev)
            table = torch.zeros(a_rows, H, dtype=torch.float32, device=dev)
            form = []

            def old_path():
                ctx.densify(ca, da)
                ctx.densify(cb, db)
                prod, how = mm_fp32((da[:, a_lo:a_lo + a_rows] > 0).to(torch.bfloat16).t(), (db > 0).to(torch.bfloat16))
                form.append(how)
                table.add_(prod)

            clear()
            new_path()
            old_path()
            torch.cuda.synchronize()
            equal = bool(torch.equal(counts.float(), table))
            pairs = int(counts.sum(dtype=torch.int64))
            hottest = int(counts.max())
            for fn in (new_path, old_path):
                for _ in range(2):
                    fn()
            torch.cuda.synchronize()
            t_new, t_old = [], []
            for _ in range(args.windows):
                t_new += timed(new_path, iters)
                t_old += timed(old_path, iters)
            t_top = {m: [] for m in METRICS}
            for metric in METRICS:
                top(metric)
            torch.cuda.synchronize()
            for _ in range(args.windows):
                for metric in METRICS:
                    t_top[metric] += timed(lambda: top(metric), iters)
            sn, so = summary(t_new), summary(t_old)
            row = {"hidden_a": H, "hidden_b": H, "a_lo": a_lo, "a_rows": a_rows, "k": K, "rows_per_call": B,
                   "feature_frequencies": "zipf" if skewed else "uniform", "pairs_per_call": pairs,
                   "hottest_cell_per_call": hottest, "torch_product": form[-1], "tables_equal_after_one_call": equal,
                   "wsae_coact_update": sn, "torch_composition": so,
                   "ratio_torch_over_new": so["median_us"] / sn["median_us"],
                   "atomics_per_us": pairs / sn["median_us"],
                   "dense_operand_bytes": 2 * B * H * 4, "table_bytes": a_rows * H * 4,
                   "wsae_coact_top_n4": {m: summary(t) for m, t in t_top.items()},
                   "top_table_gbytes_per_s": {m: a_rows * H * 4 / summary(t)["median_us"] / 1e3 for m, t in t_top.items()}}
            print(json.dumps(row), flush=True)
            results.append(row)
            ctx.close()
            del da, db, table, ctx
            torch.cuda.empty_cache()
        del counts
        torch.cuda.empty_cache()
    if args.trace:
        print("trace run done")
        return
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "windows": args.windows, "results": results}
    out_path = Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
