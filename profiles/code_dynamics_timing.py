"""Time ``wsae_dyn_update`` and ``wsae_boundary_score`` against the torch paths a user would otherwise write
(profiles/code_dynamics_note.md):

similarity   one call over the whole code, cosine, lags (1,) and (1, 2, 3, 5, 8, 13, 21, 34): with the ``sim`` matrix and
             no state, and with the state and no matrix.  torch, the better of
             sorted        one sort of the composite keys ``row H + feature`` of all entries, then per lag a
                           ``searchsorted`` of the keys of row r + lag moved back by ``lag H`` and a row sum of the matched
                           products;
             dense         (H = 3072 only) windows of 16384 rows scattered into a dense fp32 matrix, per lag the row sums
                           of the product of the matrix with itself ``lag`` rows on.
             Both give the cosine in fp32 with another order of additions: the script checks them against the kernel to
             1e-5 before it times anything.
sweep        the boundary counts of the novelty curve 1 - cosine(lag 1) at 64 thresholds, tolerance 1, against references
             at the label changes.  torch: the oracle's two-pointer loop with one pointer pair per (utterance, threshold),
             all of them advanced together, over per-threshold prediction lists made by one sort.  It yields the same
             integers, which the script checks first.

The code is ``persistent_code`` of tests/runs_oracle.py, the code the other notes use (distinct indices per row, all
values positive - the torch paths rely on that): 2048 utterances of 1500 frames, k = 32, H = 3072 and H = 40960.  One shape
per process (``--shape``), device events, warm-up calls, median and p10-p90; every process adds its rows to the output file.

    python profiles/code_dynamics_timing.py --shape 0 [--out outputs/code_dynamics_timing.json]
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
for p in (str(ROOT), str(ROOT / "whisper-sae_amd"), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import label_oracle as LO  # noqa: E402
import runs_oracle as RO  # noqa: E402
from whisper_sae import _native as N  # noqa: E402

K, T, UTT = 32, 1500, 2048
SHAPES = [3072, 40960]
LAG_SETS = [(1,), (1, 2, 3, 5, 8, 13, 21, 34)]
N_THR, TOL, WINDOW = 64, 1, 16384


def timed(fn, iters: int, warmup: int = 2) -> list:
    for _ in range(warmup):
        fn()
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


def torch_sorted(vals, idx, H: int, lags) -> torch.Tensor:
    """Cosine ``[rows, L]`` by sorted keys and ``searchsorted``; utterances are ``T`` rows each, no padding."""
    rows, k = vals.shape
    r = torch.arange(rows, device=vals.device)
    keys = (r[:, None] * H + idx.long()).reshape(-1)
    keys, order = torch.sort(keys)
    v = vals.reshape(-1)[order]
    norm = torch.sqrt((vals * vals).sum(1))
    out = torch.full((rows, len(lags)), float("nan"), device=vals.device)
    for li, lag in enumerate(lags):
        want = keys + lag * H  # the same feature, lag rows on
        pos = torch.searchsorted(keys, want).clamp_(max=keys.numel() - 1)
        hit = keys[pos] == want
        dot = torch.zeros(rows, device=vals.device).index_add_(0, keys // H, torch.where(hit, v * v[pos], torch.zeros_like(v)))
        q = r + lag
        ok = (q < rows) & (q // T == r // T)
        qc = q.clamp(max=rows - 1)
        out[:, li] = torch.where(ok, (dot / (norm * norm[qc])).clamp(max=1.0), out[:, li])
    return out


def torch_dense(vals, idx, H: int, lags) -> torch.Tensor:
    """Cosine ``[rows, L]`` by dense windows (for an H where a window fits)."""
    rows, k = vals.shape
    reach = max(lags)
    out = torch.full((rows, len(lags)), float("nan"), device=vals.device)
    r_all = torch.arange(rows, device=vals.device)
    for a in range(0, rows, WINDOW):
        b, e = min(a + WINDOW, rows), min(a + WINDOW + reach, rows)
        dense = torch.zeros(e - a, H, device=vals.device)
        dense.scatter_(1, idx[a:e].long(), vals[a:e])
        norm = torch.sqrt((dense * dense).sum(1))
        for li, lag in enumerate(lags):
            n = min(b, e - lag) - a
            if n <= 0:
                continue
            dot = (dense[:n] * dense[lag:lag + n]).sum(1)
            r = r_all[a:a + n]
            ok = (r + lag) // T == r // T
            cos = (dot / (norm[:n] * norm[lag:lag + n])).clamp(max=1.0)
            out[a:a + n, li] = torch.where(ok, cos, out[a:a + n, li])
    return out


def torch_sweep(nov, ref, thr, tol: int):
    """``(n_pred, n_hit, n_ref, n_peaks)`` of ``nov [U, T]`` (NaN = undefined) and ``ref [U, T]``: the two-pointer walk with
    one pointer pair per (utterance, threshold)."""
    U, Tn = nov.shape
    dev = nov.device
    ninf = torch.full_like(nov, float("-inf"))
    x = torch.where(torch.isnan(nov), ninf, nov)
    left = torch.cat([ninf[:, :1], x[:, :-1]], 1)
    right = torch.cat([x[:, 1:], ninf[:, :1]], 1)
    peak = ~torch.isnan(nov) & (nov > left) & (nov >= right)
    pos = torch.arange(Tn, device=dev, dtype=torch.int32)
    big = torch.tensor(1 << 20, device=dev, dtype=torch.int32)
    max_p, max_r = int(peak.sum(1).max()), int((ref != 0).sum(1).max())
    # per (utterance, threshold): the rows of the predictions, ascending, padded with `big`
    is_pred = peak[:, None, :] & (nov[:, None, :] >= thr[None, :, None])
    n_pred = is_pred.sum((0, 2))
    plist = torch.sort(torch.where(is_pred, pos, big), dim=2).values[:, :, :max_p + 1].contiguous()
    rlist = torch.sort(torch.where(ref != 0, pos, big), dim=1).values[:, :max_r + 1].contiguous()
    rlist = rlist[:, None, :].expand(U, thr.numel(), max_r + 1)
    i = torch.zeros(U, thr.numel(), dtype=torch.int64, device=dev)
    j = torch.zeros_like(i)
    hits = torch.zeros_like(i)
    for _ in range(max_p + max_r):
        p = plist.gather(2, i[:, :, None])[:, :, 0]
        q = rlist.gather(2, j[:, :, None])[:, :, 0]
        live = (p < big) & (q < big)
        hit = live & ((p - q).abs() <= tol)
        hits += hit
        i += hit | (live & ~hit & (p < q))
        j += hit | (live & ~hit & (p >= q))
    return n_pred, hits.sum(0), int((ref != 0).sum()), int(peak.sum())


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, required=True, choices=range(len(SHAPES)))
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--utterances", type=int, default=UTT)
    ap.add_argument("--out", default="outputs/code_dynamics_timing.json")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    lib = N.lib()
    stream = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    H, U = SHAPES[args.shape], args.utterances
    rows = U * T
    rng = np.random.default_rng(H)
    code = RO.persistent_code(rng, rows, K, H)
    vals, idx = torch.from_numpy(code[0]).to(dev), torch.from_numpy(code[1]).to(dev)
    del code
    labels = torch.from_numpy(LO.piecewise_labels(rng, rows, 41, hold=6.0, unlabelled=0.05)).to(dev)
    seg = torch.arange(U, dtype=torch.int32, device=dev)[:, None].expand(U, T).reshape(-1).contiguous()
    z = lambda *shape, dtype=torch.int64: torch.zeros(*shape, dtype=dtype, device=dev)  # noqa: E731
    out_rows = []

    for lags in LAG_SETS:
        L = len(lags)
        need = lib.wsae_dyn_workspace_bytes(rows, K, H, L)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        sim = torch.empty(rows, L, device=dev)
        state = [z(L, 3), z(L, 3), z(L, 3), z(L, 3, N.DYN_BINS), z(1)]
        c_lags = (C.c_int32 * L)(*lags)

        def call(sim_out, st):
            rc = lib.wsae_dyn_update(vals.data_ptr(), idx.data_ptr(), K, H, seg.data_ptr(), None, labels.data_ptr(), rows, c_lags, L,
                                     N.DYN_COSINE, N.ptr(sim_out), *[N.ptr(t) for t in st], ws.data_ptr(), need, stream())
            assert rc == 0, N.last_error()

        none = [None] * 5
        call(sim, none)
        ref_sorted = torch_sorted(vals, idx, H, lags)
        torch.cuda.synchronize()
        same_nan = bool(torch.equal(torch.isnan(sim), torch.isnan(ref_sorted)))
        gap_sorted = float((sim - ref_sorted).nan_to_num().abs().max())
        del ref_sorted
        row = {"what": "similarity", "hidden": H, "k": K, "utterances": U, "frames_per_utterance": T, "rows": rows,
               "lags": list(lags), "metric": "cosine", "workspace_bytes": int(need), "same_nan_mask_as_torch": same_nan,
               "max_gap_to_torch_sorted": gap_sorted,
               "wsae_dyn_update_sim": summary(timed(lambda: call(sim, none), args.iters)),
               "wsae_dyn_update_state": summary(timed(lambda: call(None, state), args.iters)),
               "torch_sorted_searchsorted": summary(timed(lambda: torch_sorted(vals, idx, H, lags), max(3, args.iters // 3), 1))}
        best = row["torch_sorted_searchsorted"]["median_us"]
        row["better_torch"] = "sorted_searchsorted"
        if H <= 4096:
            ref_dense = torch_dense(vals, idx, H, lags)
            torch.cuda.synchronize()
            row["max_gap_to_torch_dense"] = float((sim - ref_dense).nan_to_num().abs().max())
            del ref_dense
            row["torch_dense_windows"] = summary(timed(lambda: torch_dense(vals, idx, H, lags), max(3, args.iters // 3), 1))
            if row["torch_dense_windows"]["median_us"] < best:
                best, row["better_torch"] = row["torch_dense_windows"]["median_us"], "dense_windows"
        else:
            row["torch_dense_windows"] = None  # a [window, 40960] fp32 matrix per 16384 rows: not a formulation anyone would run
        row["ratio_better_torch_over_kernel_sim"] = best / row["wsae_dyn_update_sim"]["median_us"]
        row["ratio_better_torch_over_kernel_state"] = best / row["wsae_dyn_update_state"]["median_us"]
        pairs = int((~torch.isnan(sim)).sum())
        row["pairs"] = pairs
        row["pairs_per_us_sim"] = pairs / row["wsae_dyn_update_sim"]["median_us"]
        print(json.dumps(row), flush=True)
        out_rows.append(row)
        if lags == (1,):
            nov = (1.0 - sim[:, 0]).contiguous()
        del ws, sim, state

    # the sweep
    ref = torch.zeros(rows, dtype=torch.uint8, device=dev)
    lab2 = labels.reshape(U, T)
    ref.reshape(U, T)[:, :-1] = ((lab2[:, 1:] != lab2[:, :-1]) & (lab2[:, 1:] >= 0) & (lab2[:, :-1] >= 0)).to(torch.uint8)
    thr = torch.linspace(0.0, 1.0, N_THR, device=dev)
    need = lib.wsae_boundary_workspace_bytes(rows, N_THR, TOL)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    counts = [z(N_THR), z(N_THR), z(1), z(1)]

    def sweep():
        rc = lib.wsae_boundary_score(nov.data_ptr(), seg.data_ptr(), ref.data_ptr(), rows, thr.data_ptr(), N_THR, TOL,
                                     *[t.data_ptr() for t in counts], None, ws.data_ptr(), need, stream())
        assert rc == 0, N.last_error()

    sweep()
    t_pred, t_hit, t_ref, t_peaks = torch_sweep(nov.reshape(U, T), ref.reshape(U, T), thr, TOL)
    torch.cuda.synchronize()
    same = (torch.equal(counts[0], t_pred) and torch.equal(counts[1], t_hit) and int(counts[2]) == t_ref and int(counts[3]) == t_peaks)
    row = {"what": "boundary_sweep", "hidden": H, "utterances": U, "frames_per_utterance": T, "rows": rows, "thresholds": N_THR,
           "tolerance": TOL, "references": t_ref, "peaks": t_peaks, "same_integers_as_torch": bool(same),
           "wsae_boundary_score": summary(timed(sweep, args.iters)),
           "torch_two_pointer_vectorised": summary(timed(lambda: torch_sweep(nov.reshape(U, T), ref.reshape(U, T), thr, TOL), 3, 1))}
    row["ratio_torch_over_kernel"] = row["torch_two_pointer_vectorised"]["median_us"] / row["wsae_boundary_score"]["median_us"]
    print(json.dumps(row), flush=True)
    out_rows.append(row)

    out_path = Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    res = json.loads(out_path.read_text()) if out_path.exists() else {"results": []}
    res.update(device=torch.cuda.get_device_name(0), torch=torch.__version__, iters=args.iters)
    res["results"] = [r for r in res["results"] if r["hidden"] != H] + out_rows
    out_path.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
