"""Time the sparse linear probe against the torch formulations a user would otherwise write
(profiles/sparse_probe_note.md).

kernel   ``wsae_probe_plan`` once; ``wsae_probe_forward`` (lde = 64) and ``wsae_probe_backward`` per evaluation; one whole
         evaluation of the objective through ``SparseProbe.loss_and_grad`` (what one L-BFGS closure costs).
torch A  gathered-row logits ``bias + sum_j v_j W[col_j]``, ``log_softmax``, the gradient by ``index_add_`` of the
         value-weighted error rows, in slabs of 256 utterances (the [rows, k, C] intermediate of all rows at once is 16 GB).
torch B  the same two products as ``torch.sparse`` CSR matrix products (the CSR of the code and of its transpose built
         once, outside the timed window); recorded as unsupported if this build of torch refuses one of them.
Both torch gradients are float32 sums in an order the hardware chooses: the script runs each twice and counts the
elements whose bits differ, next to the same count for the kernel.

The code is ``persistent_code`` of tests/runs_oracle.py, the code of the other notes (distinct indices per row, all values
positive - the torch paths rely on that): 2048 utterances of 1500 frames, k = 32, C = 41; H = 3072 with all features, and
H = 40960 with a probe on 4096 scattered features (every tenth).  Labels piecewise constant (mean 6 frames), 5 % of the
stretches unlabelled.  One shape per process, device events, kernel and torch taking turns call by call, median and
p10-p90; every process adds its row to the output file.

    python profiles/sparse_probe_timing.py --shape 0 [--out outputs/sparse_probe_timing.json]
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "whisper-sae_amd"), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import label_oracle as LO  # noqa: E402
import runs_oracle as RO  # noqa: E402
from whisper_sae import _native as N  # noqa: E402
from whisper_sae.analysis import SparseProbe  # noqa: E402

K, T, UTT, CLASSES, LDE = 32, 1500, 2048, 41, 64
SHAPES = [(3072, 1), (40960, 10)]  # (H, stride of the probe's features)
SLAB = 256  # utterances per slab of torch A


def alternating(fns, iters: int) -> list:
    """One sample list (microseconds) per function; the functions take turns call by call."""
    events = [[] for _ in fns]
    for _ in range(iters):
        for n, fn in enumerate(fns):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            end.record()
            events[n].append((start, end))
    torch.cuda.synchronize()
    return [[s.elapsed_time(e) * 1e3 for s, e in ev] for ev in events]


def summary(samples: list) -> dict:
    a = np.asarray(samples)
    return {"median_us": float(np.median(a)), "p10_us": float(np.percentile(a, 10)), "p90_us": float(np.percentile(a, 90)),
            "n": int(a.size)}


def bits_differ(a: torch.Tensor, b: torch.Tensor) -> int:
    view = torch.int64 if a.dtype == torch.float64 else torch.int32
    return int((a.contiguous().view(view) != b.contiguous().view(view)).sum())


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, required=True, choices=range(len(SHAPES)))
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--utterances", type=int, default=UTT)
    ap.add_argument("--out", default="outputs/sparse_probe_timing.json")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    lib = N.lib()
    stream = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    H, stride = SHAPES[args.shape]
    C, rows = CLASSES, args.utterances * T
    rng = np.random.default_rng(H)
    code = RO.persistent_code(rng, rows, K, H)
    vals, idx = torch.from_numpy(code[0]).to(dev), torch.from_numpy(code[1]).to(dev)
    del code
    labels = torch.from_numpy(LO.piecewise_labels(rng, rows, C, hold=6.0, unlabelled=0.05)).to(dev)
    seg = torch.arange(args.utterances, dtype=torch.int32, device=dev)[:, None].expand(args.utterances, T).reshape(-1).contiguous()
    features = None if stride == 1 else torch.arange(0, H, stride)
    probe = SparseProbe(H, C, features=features, l2=1e-4, device=dev)
    probe._ensure_device()
    P, col_of = probe.n_cols, probe._col_of
    gen = torch.Generator(device="cpu").manual_seed(1)
    W = (0.1 * torch.randn(P, C, generator=gen)).to(dev)
    bias = (0.1 * torch.randn(C, generator=gen)).to(dev)

    # ---- the kernels, through the C ABI -----------------------------------------------------------------------------------
    cap = rows * K
    col_ptr = torch.empty(P + 1, dtype=torch.int64, device=dev)
    t_row = torch.empty(cap, dtype=torch.int32, device=dev)
    t_val = torch.empty(cap, dtype=torch.float32, device=dev)
    nnz_d = torch.zeros(1, dtype=torch.int64, device=dev)
    plan_bytes = lib.wsae_probe_plan_workspace_bytes(rows, K, H, P)
    bwd_bytes = lib.wsae_probe_backward_workspace_bytes(rows, P, C, cap)
    ws = torch.empty(max(plan_bytes, bwd_bytes, 1), dtype=torch.uint8, device=dev)
    err = torch.empty(rows, LDE, dtype=torch.float32, device=dev)
    counters = torch.zeros(3, dtype=torch.int64, device=dev)
    gW = torch.zeros(P, C, dtype=torch.float64, device=dev)
    gb = torch.zeros(C, dtype=torch.float64, device=dev)

    def plan():
        N.check(lib.wsae_probe_plan(vals.data_ptr(), idx.data_ptr(), K, H, seg.data_ptr(), rows, N.ptr(col_of), P, col_ptr.data_ptr(),
                                    t_row.data_ptr(), t_val.data_ptr(), cap, nnz_d.data_ptr(), ws.data_ptr(), plan_bytes, stream()),
                "wsae_probe_plan")

    def forward():
        N.check(lib.wsae_probe_forward(vals.data_ptr(), idx.data_ptr(), K, H, seg.data_ptr(), labels.data_ptr(), rows, 0, C,
                                       N.ptr(col_of), P, W.data_ptr(), C, bias.data_ptr(), None, err.data_ptr(), LDE, None,
                                       counters[0:].data_ptr(), counters[1:].data_ptr(), counters[2:].data_ptr(), None, None, 0,
                                       stream()), "wsae_probe_forward")

    def backward():
        gW.zero_()
        gb.zero_()
        N.check(lib.wsae_probe_backward(col_ptr.data_ptr(), t_row.data_ptr(), t_val.data_ptr(), cap, P, err.data_ptr(), LDE, C, rows,
                                        gW.data_ptr(), gb.data_ptr(), ws.data_ptr(), bwd_bytes, stream()), "wsae_probe_backward")

    plan()
    forward()
    backward()
    torch.cuda.synchronize()
    nnz, n_used = int(nnz_d), int(counters[0])
    first = gW.clone()
    backward()
    kernel_bits = bits_differ(first, gW)

    # ---- torch A: gather, log_softmax, index_add_ -------------------------------------------------------------------------
    cols = idx.long() if col_of is None else col_of.long()[idx.long()]
    has = cols >= 0
    cols_c, v_eff = cols.clamp(min=0), vals * has
    valid = (labels >= 0) & (labels < C)
    lab_c = labels.clamp(0, C - 1).long()
    slab = SLAB * T

    def torch_forward(out_err):
        total = torch.zeros((), dtype=torch.float32, device=dev)
        for a in range(0, rows, slab):
            e = min(a + slab, rows)
            logits = bias + (v_eff[a:e, :, None] * W[cols_c[a:e]]).sum(1)
            logp = torch.log_softmax(logits, dim=1)
            ok = valid[a:e]
            total += -(logp.gather(1, lab_c[a:e, None])[:, 0] * ok).sum()
            p = logp.exp()
            p.scatter_add_(1, lab_c[a:e, None], -torch.ones(e - a, 1, device=dev))
            out_err[a:e] = p * ok[:, None]
        return total

    t_err = torch.empty(rows, C, dtype=torch.float32, device=dev)
    t_gW = torch.zeros(P, C, dtype=torch.float32, device=dev)

    def torch_backward():
        t_gW.zero_()
        for a in range(0, rows, slab):
            e = min(a + slab, rows)
            t_gW.index_add_(0, cols_c[a:e].reshape(-1), (v_eff[a:e, :, None] * t_err[a:e, None, :]).reshape(-1, C))
        return t_err.sum(0)

    torch_forward(t_err)
    torch_backward()
    torch.cuda.synchronize()
    err_dev = float((t_err - err[:, :C]).abs().max())
    grad_dev = float((t_gW.double() - first).abs().max())
    grad_scale = float(first.abs().max())
    t_first = t_gW.clone()
    torch_backward()
    torch.cuda.synchronize()
    index_add_bits = bits_differ(t_first, t_gW)
    index_add_maxdiff = float((t_first - t_gW).abs().max())

    # ---- torch B: CSR products --------------------------------------------------------------------------------------------
    csr = {"supported": True}
    try:
        per_row = has.sum(1)
        crow = torch.zeros(rows + 1, dtype=torch.int64, device=dev)
        crow[1:] = per_row.cumsum(0)
        X = torch.sparse_csr_tensor(crow, cols[has], vals[has], size=(rows, P))
        Xt = X.to_sparse_coo().t().coalesce().to_sparse_csr()
        s_gW = torch.sparse.mm(Xt, t_err)
        s_logits = torch.sparse.mm(X, W)
        torch.cuda.synchronize()
        s_again = torch.sparse.mm(Xt, t_err)
        csr.update(bits_differ=bits_differ(s_gW, s_again), max_diff=float((s_gW - s_again).abs().max()),
                   grad_deviation_from_kernel=float((s_gW.double() - first).abs().max()))
        del s_logits, s_again
    except Exception as exc:  # noqa: BLE001 - recorded, not hidden
        csr = {"supported": False, "error": f"{type(exc).__name__}: {exc}"[:300]}

    # ---- one whole evaluation through the Python layer ----------------------------------------------------------------------
    del t_row, t_val, col_ptr  # (the probe keeps a plan of its own)
    probe.add_data((vals, idx), labels, segments=seg)
    probe.weight.copy_(W.double())
    probe.bias.copy_(bias.double())
    loss_a, gW_a, _ = probe.loss_and_grad()
    loss_b, gW_b, _ = probe.loss_and_grad()
    torch.cuda.synchronize()
    iteration_bits = bits_differ(gW_a, gW_b) + int(loss_a.item() != loss_b.item())
    sh = probe._shards[0]
    col_ptr, t_row, t_val, cap = sh["col_ptr"], sh["t_row"], sh["t_val"], sh["nnz"]
    bwd_bytes = lib.wsae_probe_backward_workspace_bytes(rows, P, C, cap)

    # ---- timings: kernel and torch take turns ---------------------------------------------------------------------------------
    fns = [forward, lambda: torch_forward(t_err), backward, torch_backward, lambda: probe.loss_and_grad()]
    names = ["wsae_probe_forward", "torch_gather_log_softmax", "wsae_probe_backward", "torch_index_add", "loss_and_grad"]
    if csr["supported"]:
        fns += [lambda: torch.sparse.mm(X, W), lambda: torch.sparse.mm(Xt, t_err)]
        names += ["torch_csr_forward_product", "torch_csr_backward_product"]
    alternating(fns, 1)  # warm-up of every shape
    times = dict(zip(names, (summary(s) for s in alternating(fns, args.iters))))
    # the plan last: it writes a plan of full capacity again
    t_row = torch.empty(rows * K, dtype=torch.int32, device=dev)
    t_val = torch.empty(rows * K, dtype=torch.float32, device=dev)
    col_ptr, cap = torch.empty(P + 1, dtype=torch.int64, device=dev), rows * K
    plan()
    times["wsae_probe_plan"] = summary(alternating([plan], args.iters)[0])

    fwd, bwd = times["wsae_probe_forward"]["median_us"], times["wsae_probe_backward"]["median_us"]
    row = {"hidden": H, "probe_columns": P, "k": K, "classes": C, "lde": LDE, "utterances": args.utterances,
           "frames_per_utterance": T, "rows": rows, "nnz": nnz, "rows_used": n_used, "chunk": N.PROBE_CHUNK,
           "err_max_deviation_torch_vs_kernel": err_dev, "grad_max_deviation_torch_vs_kernel": grad_dev,
           "grad_max_abs": grad_scale, "kernel_grad_bits_differ_run_to_run": kernel_bits,
           "loss_and_grad_bits_differ_run_to_run": iteration_bits,
           "index_add_grad_bits_differ_run_to_run": index_add_bits, "index_add_grad_max_diff_run_to_run": index_add_maxdiff,
           "index_add_grad_elements": P * C, "csr": csr, "times": times,
           "backward_gather_bytes": nnz * C * 4, "backward_effective_GBps": nnz * C * 4 / bwd * 1e-3,
           "forward_over_backward": fwd / bwd,
           "ratio_torch_gather_over_forward": times["torch_gather_log_softmax"]["median_us"] / fwd,
           "ratio_torch_index_add_over_backward": times["torch_index_add"]["median_us"] / bwd}
    print(json.dumps(row), flush=True)
    out_path = Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    res = json.loads(out_path.read_text()) if out_path.exists() else {"results": []}
    res.update(device=torch.cuda.get_device_name(0), torch=torch.__version__, iters=args.iters)
    res["results"] = [r for r in res["results"] if r["hidden"] != H] + [row]
    out_path.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
