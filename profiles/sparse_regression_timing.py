"""Time the sparse ridge regression statistics against the torch formulations a user would otherwise write
(profiles/sparse_regression_note.md).

kernel   ``wsae_probe_plan`` once (timed by profiles/sparse_probe_timing.py); ``wsae_gram_update`` over all rows of G;
         the moments (one ``wsae_probe_backward`` on the targets with a column of ones, lde = C + 1);
         ``wsae_regress_forward`` with targets (pred and the five sums); one whole ``SparseRegression.update``.
         The longest list: the same code with feature 0 forced onto every row, and ``wsae_gram_update`` on the row window
         of that one column alone - how long one workgroup holds up the launch.
torch A  ``torch.sparse`` CSR in float64: ``X^T @ X`` (sparse x sparse) and ``X^T @ Y`` (sparse x dense), the CSR of the
         code and of its transpose built once, outside the timed window.  The sparse x sparse product is first run on an
         eighth of the utterances; the full one is run once only if that predicts less than ``--csr-budget`` seconds.
         Recorded as unsupported if this build of torch refuses a product.
torch B  windowed dense float64: per window of ``--window`` rows the dense [window, P] code by ``scatter_``, then
         ``G += Xw^T @ Xw`` and ``M += Xw^T @ Yw`` by ``matmul``.

The code is ``persistent_code`` of tests/runs_oracle.py (distinct indices per row, all values positive - the torch paths
rely on that): 2048 utterances of 1500 frames, k = 32, 8 targets; H = 3072 with all features, and H = 40960 with 4096
scattered features (every tenth).  One shape per process, device events, median and p10-p90; every process adds its row to
the output file.

    python profiles/sparse_regression_timing.py --shape 0 [--out outputs/sparse_regression_timing.json]
"""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "whisper-sae_amd"), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import runs_oracle as RO  # noqa: E402
from whisper_sae import _native as N  # noqa: E402
from whisper_sae.analysis import SparseRegression  # noqa: E402

K, T, UTT, TARGETS = 32, 1500, 2048, 8
SHAPES = [(3072, 1), (40960, 10)]  # (H, stride of the regression's features)


def timed(fn, iters: int, warm: bool = True) -> dict:
    """Device-event samples of ``fn`` (microseconds) after one warm-up call."""
    if warm:
        fn()
    torch.cuda.synchronize()
    ev = []
    for _ in range(iters):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        ev.append((start, end))
    torch.cuda.synchronize()
    a = np.asarray([s.elapsed_time(e) * 1e3 for s, e in ev])
    return {"median_us": float(np.median(a)), "p10_us": float(np.percentile(a, 10)), "p90_us": float(np.percentile(a, 90)),
            "n": int(a.size)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, required=True, choices=range(len(SHAPES)))
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--utterances", type=int, default=UTT)
    ap.add_argument("--window", type=int, default=65536)
    ap.add_argument("--csr-budget", type=float, default=20.0)
    ap.add_argument("--out", default="outputs/sparse_regression_timing.json")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    lib = N.lib()
    stream = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    H, stride = SHAPES[args.shape]
    C, rows = TARGETS, args.utterances * T
    rng = np.random.default_rng(H)
    code = RO.persistent_code(rng, rows, K, H)
    vals, idx = torch.from_numpy(code[0]).to(dev), torch.from_numpy(code[1]).to(dev)
    del code
    Y = torch.randn(rows, C, generator=torch.Generator().manual_seed(2)).to(dev)
    seg = torch.arange(args.utterances, dtype=torch.int32, device=dev)[:, None].expand(args.utterances, T).reshape(-1).contiguous()
    features = None if stride == 1 else torch.arange(0, H, stride)
    reg = SparseRegression(H, C, features=features, device=dev)
    reg._ensure_device()
    P, col_of = reg.n_cols, reg._col_of
    print(json.dumps({"stage": "data", "rows": rows, "P": P}), flush=True)

    # ---- the kernels, through the C ABI -----------------------------------------------------------------------------------
    cap = rows * K
    col_ptr = torch.empty(P + 1, dtype=torch.int64, device=dev)
    t_row = torch.empty(cap, dtype=torch.int32, device=dev)
    t_val = torch.empty(cap, dtype=torch.float32, device=dev)
    nnz_d = torch.zeros(1, dtype=torch.int64, device=dev)
    E = torch.cat([Y, torch.ones(rows, 1, device=dev)], 1).contiguous()
    plan_bytes = lib.wsae_probe_plan_workspace_bytes(rows, K, H, P)
    bwd_bytes = lib.wsae_probe_backward_workspace_bytes(rows, P, C + 1, cap)
    fwd_bytes = lib.wsae_regress_forward_workspace_bytes(rows, K, H, P, C, 0)
    gram_bytes = lib.wsae_gram_workspace_bytes(rows, K, H, P, P, cap)
    ws = torch.empty(max(plan_bytes, bwd_bytes, fwd_bytes, gram_bytes, 1), dtype=torch.uint8, device=dev)
    G = torch.zeros(P, P, dtype=torch.float64, device=dev)
    MX = torch.zeros(P, C + 1, dtype=torch.float64, device=dev)
    sums = torch.zeros(C + 1, dtype=torch.float64, device=dev)
    W = (0.1 * torch.randn(P, C, dtype=torch.float64, generator=torch.Generator().manual_seed(3))).to(dev)
    bias = torch.zeros(C, dtype=torch.float64, device=dev)
    pred = torch.empty(rows, C, dtype=torch.float32, device=dev)
    n_used = torch.zeros(1, dtype=torch.int64, device=dev)
    stats = torch.zeros(5, C, dtype=torch.float64, device=dev)

    def plan():
        N.check(lib.wsae_probe_plan(vals.data_ptr(), idx.data_ptr(), K, H, seg.data_ptr(), rows, N.ptr(col_of), P, col_ptr.data_ptr(),
                                    t_row.data_ptr(), t_val.data_ptr(), cap, nnz_d.data_ptr(), ws.data_ptr(), plan_bytes, stream()),
                "wsae_probe_plan")

    def gram(p_lo=0, p_rows=P):
        N.check(lib.wsae_gram_update(vals.data_ptr(), idx.data_ptr(), K, H, seg.data_ptr(), rows, N.ptr(col_of), P,
                                     col_ptr.data_ptr(), t_row.data_ptr(), t_val.data_ptr(), cap, p_lo, p_rows,
                                     G[p_lo:].data_ptr(), P, ws.data_ptr(), gram_bytes, stream()), "wsae_gram_update")

    def moments():
        N.check(lib.wsae_probe_backward(col_ptr.data_ptr(), t_row.data_ptr(), t_val.data_ptr(), cap, P, E.data_ptr(), C + 1, C + 1,
                                        rows, MX.data_ptr(), sums.data_ptr(), ws.data_ptr(), bwd_bytes, stream()),
                "wsae_probe_backward")

    def forward():
        N.check(lib.wsae_regress_forward(vals.data_ptr(), idx.data_ptr(), K, H, seg.data_ptr(), Y.data_ptr(), C, rows, 0, C,
                                         N.ptr(col_of), P, W.data_ptr(), C, bias.data_ptr(), pred.data_ptr(), C, n_used.data_ptr(),
                                         stats.data_ptr(), ws.data_ptr(), fwd_bytes, stream()), "wsae_regress_forward")

    plan()
    torch.cuda.synchronize()
    nnz = int(nnz_d)
    lens = (col_ptr[1:] - col_ptr[:-1]).cpu().numpy()
    G.zero_()
    gram()
    torch.cuda.synchronize()
    first = G.clone()
    G.zero_()
    gram()
    torch.cuda.synchronize()
    gram_bits = int((first.view(torch.int64) != G.view(torch.int64)).sum())
    times = {"wsae_gram_update": timed(gram, args.iters), "moments_wsae_probe_backward": timed(moments, args.iters),
             "wsae_regress_forward": timed(forward, args.iters)}
    print(json.dumps({"stage": "kernels", "times": times}), flush=True)

    # ---- torch B: windowed dense float64 ----------------------------------------------------------------------------------
    cols = idx.long() if col_of is None else col_of.long()[idx.long()]
    has = cols >= 0
    Gd = torch.zeros(P, P, dtype=torch.float64, device=dev)
    Md = torch.zeros(P, C, dtype=torch.float64, device=dev)
    Yd = Y.double()

    def dense_windows(with_gram=True, with_moment=True):
        Gd.zero_()
        Md.zero_()
        for a in range(0, rows, args.window):
            e = min(a + args.window, rows)
            Xw = torch.zeros(e - a, P + 1, dtype=torch.float64, device=dev)  # (column P takes the entries without a column)
            Xw.scatter_(1, torch.where(has[a:e], cols[a:e], torch.full_like(cols[a:e], P)), vals[a:e].double())
            Xw = Xw[:, :P]
            if with_gram:
                Gd.addmm_(Xw.T, Xw)
            if with_moment:
                Md.addmm_(Xw.T, Yd[a:e])

    dense_windows()
    torch.cuda.synchronize()
    upper = torch.triu(first)
    gram_dev = float((upper - torch.triu(Gd)).abs().max() / Gd.abs().max())
    moment_dev = float((MX[:, :C] / (args.iters + 1) - Md).abs().max() / Md.abs().max())  # (MX accumulated iters + 1 calls)
    times["torch_dense_windows_gram"] = timed(lambda: dense_windows(True, False), max(args.iters // 2, 2))
    times["torch_dense_windows_moment"] = timed(lambda: dense_windows(False, True), max(args.iters // 2, 2))
    print(json.dumps({"stage": "dense", "gram_dev": gram_dev, "moment_dev": moment_dev}), flush=True)
    del Gd

    # ---- torch A: CSR products in float64 ---------------------------------------------------------------------------------
    def csr_of(n_rows):
        per_row = has[:n_rows].sum(1)
        crow = torch.zeros(n_rows + 1, dtype=torch.int64, device=dev)
        crow[1:] = per_row.cumsum(0)
        order = torch.argsort(torch.where(has[:n_rows], cols[:n_rows], torch.full_like(cols[:n_rows], P)), dim=1, stable=True)
        c_sorted, v_sorted = cols[:n_rows].gather(1, order), vals[:n_rows].gather(1, order).double()
        keep = c_sorted >= 0
        X = torch.sparse_csr_tensor(crow, c_sorted[keep], v_sorted[keep], size=(n_rows, P))
        return X, X.to_sparse_coo().t().coalesce().to_sparse_csr()

    csr = {"supported": True}
    try:
        small_rows = max(args.utterances // 8, 1) * T
        Xs, Xst = csr_of(small_rows)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        Gs = torch.sparse.mm(Xst, Xs)
        torch.cuda.synchronize()
        small_s = time.perf_counter() - t0
        csr["gram_eighth_rows"] = small_rows
        csr["gram_eighth_first_call_s"] = small_s
        csr["gram_eighth"] = timed(lambda: torch.sparse.mm(Xst, Xs), 2)
        del Gs, Xs, Xst
        X, Xt = csr_of(rows)
        times["torch_csr_moment"] = timed(lambda: torch.sparse.mm(Xt, Yd), args.iters)
        Mc = torch.sparse.mm(Xt, Yd)
        csr["moment_deviation_from_dense"] = float((Mc - Md).abs().max() / Md.abs().max())
        if csr["gram_eighth"]["median_us"] * 8e-6 * 2 < args.csr_budget:
            t0 = time.perf_counter()
            Gc = torch.sparse.mm(Xt, X)
            torch.cuda.synchronize()
            csr["gram_full_first_call_s"] = time.perf_counter() - t0
            times["torch_csr_gram"] = timed(lambda: torch.sparse.mm(Xt, X), 1, warm=False)
            csr["gram_deviation_from_kernel"] = float((torch.triu(Gc.to_dense()) - upper).abs().max() / upper.abs().max())
            del Gc
        else:
            csr["gram_full"] = "not run: the eighth predicts more than the budget"
        del X, Xt
    except Exception as exc:  # noqa: BLE001 - recorded, not hidden
        csr.update(supported=False, error=f"{type(exc).__name__}: {exc}"[:300])
    print(json.dumps({"stage": "csr", "csr": csr}), flush=True)

    # ---- one whole update through the Python layer, and the solve ---------------------------------------------------------
    del t_row, t_val, first, upper
    reg.update((vals, idx), Y, segments=seg)
    times["SparseRegression_update"] = timed(lambda: reg.update((vals, idx), Y, segments=seg), max(args.iters // 2, 2))
    t0 = time.perf_counter()
    fit = reg.fit(1e-3, torch.arange(min(P, 64)))
    fit_64_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    fit = reg.fit(1e-3)
    fit_all_s = time.perf_counter() - t0

    # ---- the longest list: feature 0 (column 0 in both shapes) on every row ---------------------------------------------------
    idx[:, 0] = 0
    t_row = torch.empty(cap, dtype=torch.int32, device=dev)
    t_val = torch.empty(cap, dtype=torch.float32, device=dev)
    plan()
    torch.cuda.synchronize()
    longest = int((col_ptr[1] - col_ptr[0]))
    times["wsae_gram_update_longest_list_alone"] = timed(lambda: gram(0, 1), 3)
    times["wsae_gram_update_with_longest_list"] = timed(gram, 3)

    g = times["wsae_gram_update"]["median_us"]
    pair_terms = float((G.triu() != 0).sum())  # (cells; the terms are counted from the lists below)
    row = {"hidden": H, "columns": P, "k": K, "targets": C, "utterances": args.utterances, "frames_per_utterance": T, "rows": rows,
           "nnz": nnz, "list_len_mean": float(lens.mean()), "list_len_max": int(lens.max()), "chunk": N.PROBE_CHUNK,
           "gram_bits_differ_run_to_run": gram_bits, "gram_max_rel_deviation_kernel_vs_dense": gram_dev,
           "moment_max_rel_deviation_kernel_vs_dense": moment_dev, "gram_nonzero_upper_cells": pair_terms, "csr": csr,
           "times": times, "fit_64_columns_s": fit_64_s, "fit_all_columns_s": fit_all_s, "r2_train": fit.r2_train.tolist(),
           "longest_list_entries": longest, "gram_rows_per_us": nnz / g,
           "ratio_dense_windows_gram_over_kernel": times["torch_dense_windows_gram"]["median_us"] / g,
           "ratio_dense_windows_moment_over_kernel": times["torch_dense_windows_moment"]["median_us"]
           / times["moments_wsae_probe_backward"]["median_us"]}
    print(json.dumps(row), flush=True)
    out_path = Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    res = json.loads(out_path.read_text()) if out_path.exists() else {"results": []}
    res.update(device=torch.cuda.get_device_name(0), torch=torch.__version__, iters=args.iters)
    res["results"] = [r for r in res["results"] if r["hidden"] != H] + [row]
    out_path.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
