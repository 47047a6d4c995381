"""Time ``wsae_cluster_assign`` and ``wsae_cluster_accumulate`` against the torch paths a user would otherwise write
(profiles/code_clustering_note.md):

assign       one call over the whole code with every output and the state, cosine (normalize = 1), 100 and 500 clusters.
             torch:
             csr           the ``torch.sparse`` CSR matrix of the code (built once, outside the timing) times ``Ct``, then
                           ``topk(2)`` over the clusters - the ``[frames, n_clusters]`` product exists;
             dense         (H = 3072 only) windows of 16384 rows scattered into a dense fp32 matrix, ``matmul`` with ``Ct``,
                           ``topk(2)``.
             Both give the scores in fp32 with another order of additions: the script reports the share of frames whose
             winner agrees with the kernel's and the largest gap of the best score.
accumulate   one call over the plan with the inverse norms as row weights.  torch: ``index_add_`` of the weighted entries
             into a float32 ``[n_clusters, n_cols]`` matrix by ``assign * n_cols + column`` - float atomics; the script runs
             it twice and reports the share of elements whose bits differ.
plan         ``wsae_probe_plan`` (once per fit of in-memory data).
iteration    assign, accumulate and the update of the centroids from the integers (torch, float64) together.

The code is ``persistent_code`` of tests/runs_oracle.py, the code the other notes use: 2048 utterances of 1500 frames,
k = 32; shape 0 is all features of H = 3072, shape 1 is 4096 scattered features of H = 40960.  One shape per process
(``--shape``), device events, warm-up calls, median and p10-p90; every process adds its rows to the output file.

    python profiles/code_clustering_timing.py --shape 0 [--out outputs/code_clustering_timing.json]
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

import runs_oracle as RO  # noqa: E402
from whisper_sae import _native as N  # noqa: E402

K, T, UTT = 32, 1500, 2048
SHAPES = [(3072, None), (40960, 4096)]
CLUSTERS = [100, 500]
WINDOW, N_CLASSES = 16384, 41


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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, required=True)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--utterances", type=int, default=UTT)
    ap.add_argument("--out", default=str(ROOT / "outputs" / "code_clustering_timing.json"))
    args = ap.parse_args()
    H, n_feat = SHAPES[args.shape]
    U = args.utterances
    rows = U * T
    dev = torch.device("cuda", 0)
    lib = N.lib()
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream  # noqa: E731
    rng = np.random.default_rng(2400 + args.shape)
    code = RO.persistent_code(rng, rows, K, H)
    vals, idx = torch.from_numpy(code[0]).to(dev), torch.from_numpy(code[1]).to(dev)
    del code
    if n_feat is None:
        col_of, P = None, H
        col = idx.long()
    else:
        feats = torch.from_numpy(np.sort(rng.choice(H, n_feat, replace=False))).to(dev)
        col_of = torch.full((H,), -1, dtype=torch.int32, device=dev)
        col_of[feats] = torch.arange(n_feat, dtype=torch.int32, device=dev)
        P = n_feat
        col = col_of[idx.long()].long()
    seg = torch.arange(U, dtype=torch.int32, device=dev)[:, None].expand(U, T).reshape(-1).contiguous()
    labels = torch.from_numpy(rng.integers(0, N_CLASSES, rows).astype(np.int32)).to(dev)
    z = lambda *shape, dtype=torch.int64: torch.zeros(*shape, dtype=dtype, device=dev)  # noqa: E731

    # the plan
    col_ptr, nnz = z(P + 1), z(1)
    cap = rows * K if n_feat is None else int((col >= 0).sum())
    t_row, t_val = z(cap, dtype=torch.int32), z(cap, dtype=torch.float32)
    need = lib.wsae_probe_plan_workspace_bytes(rows, K, H, P)
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)

    def plan():
        rc = lib.wsae_probe_plan(vals.data_ptr(), idx.data_ptr(), K, H, seg.data_ptr(), rows, N.ptr(col_of), P, col_ptr.data_ptr(),
                                 t_row.data_ptr(), t_val.data_ptr(), cap, nnz.data_ptr(), ws.data_ptr(), need, stream())
        assert rc == 0, N.last_error()

    plan()
    assert int(nnz) == cap
    base = {"hidden": H, "n_cols": P, "k": K, "utterances": U, "frames_per_utterance": T, "rows": rows, "entries": cap}
    out_rows = [dict(base, what="plan", wsae_probe_plan=summary(timed(plan, args.iters)))]
    print(json.dumps(out_rows[-1]), flush=True)

    # the torch CSR matrix of the code (outside the timing)
    has = col >= 0
    crow = torch.zeros(rows + 1, dtype=torch.int64, device=dev)
    crow[1:] = torch.cumsum(has.sum(1), 0)
    csr = torch.sparse_csr_tensor(crow, col[has], vals[has], size=(rows, P))
    flat_col, flat_val, flat_row = col[has], vals[has], torch.arange(rows, device=dev)[:, None].expand(rows, K)[has]

    for C in CLUSTERS:
        gen = torch.Generator(device="cpu").manual_seed(C)
        Ct = torch.rand(P, C, generator=gen).pow(8).to(dev)  # sparse-ish positive centroids, as k-means of such codes has
        Ct = (Ct / Ct.norm(dim=0, keepdim=True)).contiguous()
        a_out = z(rows, dtype=torch.int32)
        best, second, inv = (z(rows, dtype=torch.float32) for _ in range(3))
        state = [z(C), z(C), z(C, N_CLASSES), z(3)]
        S_q = z(P, C)

        def assign():
            rc = lib.wsae_cluster_assign(vals.data_ptr(), idx.data_ptr(), K, H, seg.data_ptr(), rows, N.ptr(col_of), P, Ct.data_ptr(), C,
                                         None, C, 1, labels.data_ptr(), N_CLASSES, a_out.data_ptr(), best.data_ptr(), second.data_ptr(),
                                         inv.data_ptr(), *[t.data_ptr() for t in state], None, 0, stream())
            assert rc == 0, N.last_error()

        def accumulate():
            rc = lib.wsae_cluster_accumulate(col_ptr.data_ptr(), t_row.data_ptr(), t_val.data_ptr(), cap, P, a_out.data_ptr(),
                                             inv.data_ptr(), rows, C, S_q.data_ptr(), C, None, 0, stream())
            assert rc == 0, N.last_error()

        def update():
            cnt = state[0].clamp(min=1).double() * float(2 ** 20)
            c64 = S_q.double() / cnt[None, :]
            c64 = c64 / (c64 * c64).sum(0).sqrt().clamp(min=1e-300)
            return c64.float()

        def iteration():
            for t in state:
                t.zero_()
            S_q.zero_()
            assign()
            accumulate()
            return update()

        def torch_csr():
            return (csr @ Ct).topk(min(2, C), dim=1)

        def torch_dense():
            out_v, out_i = [], []
            for lo in range(0, rows, WINDOW):
                hi = min(lo + WINDOW, rows)
                dense = torch.zeros(hi - lo, P, device=dev)
                dense.scatter_(1, idx[lo:hi].long(), vals[lo:hi])
                v2, i2 = (dense @ Ct).topk(min(2, C), dim=1)
                out_v.append(v2), out_i.append(i2)
            return torch.cat(out_v), torch.cat(out_i)

        def torch_index_add():
            w = flat_val * inv[flat_row]
            return torch.zeros(C * P, device=dev).index_add_(0, a_out.long()[flat_row] * P + flat_col, w)

        assign()
        ref_v, ref_i = torch_csr()
        torch.cuda.synchronize()
        ok = a_out >= 0
        row = dict(base, what="assign", n_clusters=C, assigned=int(ok.sum()),
                   same_winner_as_torch_csr=float((ref_i[:, 0][ok] == a_out[ok]).double().mean()),
                   max_gap_best_to_torch_csr=float((ref_v[:, 0][ok] - best[ok]).abs().max()),
                   gathered_bytes=int(cap) * C * 4)
        del ref_v, ref_i
        row["wsae_cluster_assign"] = summary(timed(assign, args.iters))
        row["torch_sparse_csr_topk2"] = summary(timed(torch_csr, max(3, args.iters // 2), 1))
        better = row["torch_sparse_csr_topk2"]["median_us"]
        row["better_torch"] = "sparse_csr"
        if n_feat is None and H <= 4096:
            row["torch_dense_windows_topk2"] = summary(timed(torch_dense, 3, 1))
            if row["torch_dense_windows_topk2"]["median_us"] < better:
                better, row["better_torch"] = row["torch_dense_windows_topk2"]["median_us"], "dense_windows"
        else:
            row["torch_dense_windows_topk2"] = None
        row["ratio_better_torch_over_kernel"] = better / row["wsae_cluster_assign"]["median_us"]
        row["gathered_GB_per_s"] = row["gathered_bytes"] / row["wsae_cluster_assign"]["median_us"] / 1e3
        print(json.dumps(row), flush=True)
        out_rows.append(row)

        S_q.zero_()
        accumulate()
        one, two = torch_index_add(), torch_index_add()
        torch.cuda.synchronize()
        ref = (S_q.double() / float(2 ** 20)).t().reshape(-1)
        row = dict(base, what="accumulate", n_clusters=C,
                   max_gap_to_torch_index_add=float((ref - one.double()).abs().max()),
                   torch_share_of_elements_whose_bits_differ_between_two_runs=float(
                       (one.view(torch.int32) != two.view(torch.int32)).double().mean()),
                   torch_share_among_nonzero_elements=float(
                       ((one.view(torch.int32) != two.view(torch.int32)) & (one != 0)).double().sum() / max(int((one != 0).sum()), 1)))
        del one, two, ref
        row["wsae_cluster_accumulate"] = summary(timed(accumulate, args.iters))
        row["torch_index_add"] = summary(timed(torch_index_add, max(3, args.iters // 2), 1))
        row["ratio_torch_over_kernel"] = row["torch_index_add"]["median_us"] / row["wsae_cluster_accumulate"]["median_us"]
        print(json.dumps(row), flush=True)
        out_rows.append(row)

        row = dict(base, what="iteration", n_clusters=C, wsae_iteration=summary(timed(iteration, args.iters)))
        print(json.dumps(row), flush=True)
        out_rows.append(row)
        del Ct, a_out, best, second, inv, state, S_q

    out_path = Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    res = json.loads(out_path.read_text()) if out_path.exists() else {"results": []}
    res.update(device=torch.cuda.get_device_name(0), torch=torch.__version__, iters=args.iters)
    res["results"] = [r for r in res["results"] if (r["hidden"], r["n_cols"]) != (H, P)] + out_rows
    out_path.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
