"""Time ``wsae_dtw_matrix`` and ``wsae_abx_count`` against the torch formulation a user would otherwise write
(profiles/abx_note.md):

distances    one X window of ``--window`` items against all items, cosine, normalised.  torch: the frames of the items
             scattered into dense ``[items, Lmax, H]`` windows and normalised, ``matmul`` of the X frames against the
             frames of a block of items for the cosine costs, and the dynamic program over all pairs of the block at once
             by anti-diagonals on padded ``[x, items, Lmax + 1, Lmax + 1]`` tensors (float64 totals with the path length
             carried along and the tie-break of the contract).
counts       the triples of that window.  torch: per category pair (c, c') one broadcast comparison
             ``d[x, a, None] < d[x, None, b]`` over the X and A items of c and the B items of c'.
score        one whole ``AbxItems.score()`` (all windows; the kernels only - the torch path is the sum of the above).

Before anything is timed the two are compared: distances to 1e-5 (the number of cells beyond it is recorded and must stay
below 1e-4 of them: a path flips where two totals lie within a rounding error), counts up to the triples whose two
distances lie within 1e-5 of each other (that number is printed).

The code is ``persistent_code`` of tests/runs_oracle.py (2048 utterances of 1500 frames, k = 32, H = 3072 and H = 40960),
the items the runs of a piecewise-constant label track of 41 classes, subsampled to ``--items``.  One shape per process,
device events, warm-up calls, median and p10-p90; every process adds its rows to the output file.

    python profiles/abx_timing.py --shape 0 --items 4096 [--out outputs/abx_timing.json]
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
from whisper_sae.analysis import AbxItems  # noqa: E402

K, T, UTT, CLASSES = 32, 1500, 2048, 41
SHAPES = [3072, 40960]


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


def dense_items(store: AbxItems, H: int, lo: int, hi: int):
    """``[hi - lo, Lmax, H]`` float32 unit rows (zero rows behind an item's end) of the items lo .. hi - 1."""
    st, ln = store.starts[lo:hi].long(), store.lengths[lo:hi].long()
    Lm = int(store.lengths.max())
    c = store._flat()
    pos = torch.arange(Lm, device=st.device)
    rows = (st[:, None] + pos[None, :]).clamp(max=c["vals"].shape[0] - 1)
    live = pos[None, :] < ln[:, None]
    dense = torch.zeros(hi - lo, Lm, H, device=st.device)
    dense.scatter_(2, c["idx"][rows].long(), c["vals"][rows] * live[:, :, None])
    return dense / dense.norm(dim=2, keepdim=True).clamp_min(1e-30), ln


def torch_distances(store: AbxItems, H: int, x_lo: int, x_hi: int, block: int) -> torch.Tensor:
    """``[x_hi - x_lo, n_items]`` float32 normalised DTW distances, a block of ``block`` items at a time."""
    n = store.n_items
    dev = store.starts.device
    X, x_len = dense_items(store, H, x_lo, x_hi)
    nx, Lm = X.shape[0], X.shape[1]
    out = torch.empty(nx, n, device=dev)
    inf = float("inf")
    ar = torch.arange(Lm, device=dev)
    for b_lo in range(0, n, block):
        b_hi = min(b_lo + block, n)
        B, b_len = dense_items(store, H, b_lo, b_hi)
        nb = B.shape[0]
        cost = 1.0 - torch.clamp(torch.matmul(X.reshape(nx * Lm, H), B.reshape(nb * Lm, H).t()), max=1.0)
        cost = cost.reshape(nx, Lm, nb, Lm).permute(0, 2, 1, 3).double()  # [x, b, i, j]
        D = torch.full((nx, nb, Lm + 1, Lm + 1), inf, dtype=torch.float64, device=dev)
        L = torch.zeros((nx, nb, Lm + 1, Lm + 1), dtype=torch.int32, device=dev)
        D[:, :, 0, 0] = 0.0
        for d in range(2 * Lm - 1):  # the anti-diagonal i + j = d
            i = ar[max(0, d - Lm + 1):min(d, Lm - 1) + 1]
            j = d - i
            best, steps = D[:, :, i, j], L[:, :, i, j]  # the diagonal predecessor (padded coordinates)
            for pi, pj in ((i, j + 1), (i + 1, j)):      # above, left: strictly smaller wins
                cand = D[:, :, pi, pj]
                take = cand < best
                best, steps = torch.where(take, cand, best), torch.where(take, L[:, :, pi, pj], steps)
            D[:, :, i + 1, j + 1] = cost[:, :, i, j] + best
            L[:, :, i + 1, j + 1] = steps + 1
        ei = x_len[:, None].expand(nx, nb)
        ej = b_len[None, :].expand(nx, nb)
        xi = torch.arange(nx, device=dev)[:, None].expand(nx, nb)
        bi = torch.arange(nb, device=dev)[None, :].expand(nx, nb)
        out[:, b_lo:b_hi] = (D[xi, bi, ei, ej] / L[xi, bi, ei, ej].double()).float()
    return out


def torch_counts(dist: torch.Tensor, x_lo: int, cat: torch.Tensor, n_cats: int, margin: float = 0.0):
    """``(wins2, total, near)`` int64 of the window ``dist [n_x, n_items]``: per category pair one broadcast comparison;
    ``near``: the triples whose two distances lie within ``margin`` of each other."""
    dev = dist.device
    n_x = dist.shape[0]
    wins2 = torch.zeros(n_cats, n_cats, dtype=torch.int64, device=dev)
    total = torch.zeros_like(wins2)
    near = torch.zeros((), dtype=torch.int64, device=dev)
    x_cat = cat[x_lo:x_lo + n_x]
    members = [torch.nonzero(cat == c).reshape(-1) for c in range(n_cats)]
    for c in range(n_cats):
        xs = torch.nonzero(x_cat == c).reshape(-1)
        if not xs.numel() or members[c].numel() < 2:
            continue
        da = dist[xs][:, members[c]]                              # [x, a]
        not_self = members[c][None, :] != (xs + x_lo)[:, None]   # a != x
        for c2 in range(n_cats):
            if c2 == c or not members[c2].numel():
                continue
            db = dist[xs][:, members[c2]]                         # [x, b]
            lt = (da[:, :, None] < db[:, None, :]) & not_self[:, :, None]
            eq = (da[:, :, None] == db[:, None, :]) & not_self[:, :, None]
            wins2[c, c2] = 2 * lt.sum() + eq.sum()
            total[c, c2] = not_self.sum() * members[c2].numel()
            if margin:
                near += (((da[:, :, None] - db[:, None, :]).abs() <= margin) & not_self[:, :, None]).sum()
    return wins2, total, near


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, required=True, choices=range(len(SHAPES)))
    ap.add_argument("--items", type=int, default=4096)
    ap.add_argument("--window", type=int, default=1024)
    ap.add_argument("--torch-window", type=int, default=64, help="the X items of the torch distance pass (scaled to --window)")
    ap.add_argument("--torch-block", type=int, default=512)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--utterances", type=int, default=UTT)
    ap.add_argument("--out", default="outputs/abx_timing.json")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    lib = N.lib()
    H, U = SHAPES[args.shape], args.utterances
    rng = np.random.default_rng(H)
    code = RO.persistent_code(rng, U * T, K, H)
    labels = torch.from_numpy(LO.piecewise_labels(rng, U * T, CLASSES, hold=6.0, unlabelled=0.05)).to(dev).reshape(U, T)
    vals, idx = torch.from_numpy(code[0]).to(dev).reshape(U, T, K), torch.from_numpy(code[1]).to(dev).reshape(U, T, K)
    del code
    full = AbxItems(H, device=dev)
    full.add((vals, idx), labels=labels, n_classes=CLASSES)
    del vals, idx
    store = full.subsample(args.items, seed=0)
    n, n_x = store.n_items, min(args.window, store.n_items)
    frames = int(store.lengths.sum())
    cat = store.category
    row = {"hidden": H, "k": K, "utterances": U, "frames_per_utterance": T, "items_in_dataset": full.n_items, "items": n,
           "frames_of_items": frames, "mean_length": frames / n, "max_length": int(store.lengths.max()), "window": n_x,
           "metric": "cosine", "normalize": True, "mode": "any", "categories": CLASSES}
    del full

    # the kernels
    dist = torch.empty(n_x, n, device=dev)
    need = lib.wsae_abx_workspace_bytes(n, n_x, CLASSES)
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    tables = [torch.zeros(CLASSES, CLASSES, dtype=torch.int64, device=dev) for _ in range(2)] + [torch.zeros(1, dtype=torch.int64, device=dev)]

    def count():
        rc = lib.wsae_abx_count(dist.data_ptr(), n, 0, n_x, n, cat.data_ptr(), None, None, CLASSES, N.ABX_ANY, tables[0].data_ptr(),
                                tables[1].data_ptr(), tables[2].data_ptr(), ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, N.last_error()

    store.distances((0, n_x), out=dist)
    count()
    torch.cuda.synchronize()
    k_wins2, k_total = tables[0].clone(), tables[1].clone()

    # agreement before any timing
    tw = min(args.torch_window, n_x)
    ref = torch_distances(store, H, 0, tw, args.torch_block)
    gap = (ref - dist[:tw]).abs()
    beyond = int((gap > 1e-5).sum())
    row.update(max_gap_to_torch=float(gap.max()), cells_compared=int(gap.numel()), cells_beyond_1e_5=beyond)
    print(json.dumps({"agreement": "distances", "max_gap": row["max_gap_to_torch"], "beyond_1e-5": beyond, "cells": gap.numel()}), flush=True)
    assert beyond <= 1e-4 * gap.numel(), "torch and kernel distances disagree"
    t_wins2, t_total, near = torch_counts(dist, 0, cat, CLASSES, margin=1e-5)
    torch.cuda.synchronize()
    same_total = bool(torch.equal(t_total, k_total))
    wins_gap = int((t_wins2 - k_wins2).abs().sum())
    row.update(count_totals_equal=same_total, count_wins2_difference=wins_gap, triples=int(k_total.sum()), triples_within_1e_5=int(near))
    print(json.dumps({"agreement": "counts", "totals_equal": same_total, "wins2_difference": wins_gap, "triples_within_1e-5": int(near)}),
          flush=True)
    assert same_total and wins_gap <= 2 * int(near), "torch and kernel counts disagree"

    # the timings
    pairs = int(store.lengths[:n_x].sum()) * frames
    row["frame_pairs_of_the_window"] = pairs
    row["wsae_dtw_matrix_window"] = summary(timed(lambda: store.distances((0, n_x), out=dist), args.iters))
    row["frame_pairs_per_us"] = pairs / row["wsae_dtw_matrix_window"]["median_us"]
    row["wsae_abx_count_window"] = summary(timed(count, args.iters))
    row["triples_per_us"] = row["triples"] / row["wsae_abx_count_window"]["median_us"]
    row["score_all_windows"] = summary(timed(lambda: store.score("any", row_block=n_x, with_context=False, n_cats=CLASSES),
                                             max(3, args.iters // 3), 1))
    t = summary(timed(lambda: torch_distances(store, H, 0, tw, args.torch_block), 3, 1))
    row["torch_distances_x_items"] = tw
    row["torch_distances"] = t
    row["torch_distances_scaled_to_window_us"] = t["median_us"] * n_x / tw
    row["ratio_torch_over_kernel_distances"] = row["torch_distances_scaled_to_window_us"] / row["wsae_dtw_matrix_window"]["median_us"]
    row["torch_counts_window"] = summary(timed(lambda: torch_counts(dist, 0, cat, CLASSES), 3, 1))
    row["ratio_torch_over_kernel_counts"] = row["torch_counts_window"]["median_us"] / row["wsae_abx_count_window"]["median_us"]
    print(json.dumps(row), flush=True)

    out_path = Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    res = json.loads(out_path.read_text()) if out_path.exists() else {"results": []}
    res.update(device=torch.cuda.get_device_name(0), torch=torch.__version__, iters=args.iters)
    res["results"] = [r for r in res["results"] if (r["hidden"], r["items"]) != (H, n)] + [row]
    out_path.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
