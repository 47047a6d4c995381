"""Time ``wsae_pair_update`` and both directions of ``wsae_pair_top`` against the torch formulation a user would otherwise
write (profiles/token_association_note.md).

The data: 2048 utterances of 1500 frames, k = 32, ``persistent_code`` of tests/runs_oracle.py (the code of
profiles/temporal_note.md) and tokens in runs of 5 to 25 frames drawn from a Zipf law over the 51 865 tokens of Whisper's
vocabulary (``zipf_tokens`` of tests/token_oracle.py); shape 0 is H = 3072, shape 1 is H = 40 960.

update   the stream as ``TokenAssociation`` feeds it: calls of ``--batch`` utterances into one table.  A first pass through
         the tracker (capacity 2^20, growing by itself) gives the number of distinct pairs, the final capacity and the
         time of the pass with its growth steps (host clock, once); the timed passes then fill a fresh table of the final
         capacity with the same calls (device events around the whole pass, the reset of the table outside them).
top      ``wsae_pair_top`` per feature (lift) and per token (precision), n = 10, min_count = 5, on the final table.
torch    composite int64 keys ``feature << 32 | token`` of every entry that forms a pair, ``torch.unique(return_inverse,
         return_counts)`` and an ``index_add_`` of the fixed-point values for the sums - one call over all rows, which
         spares it the merge of batches; then per direction the float64 scores, a stable ``sort`` by score, a stable sort by
         group and the first n of every group.
Both must yield the same integers: the script asserts that the export of the table equals the unique keys with their
counts and sums, and that ids, counts and scores (bit for bit) of both selections agree.

One shape per process (``--shape``), warm-up calls, median and p10-p90; every process adds its rows to the output file.

    python profiles/token_association_timing.py --shape 0 [--out outputs/token_association_timing.json]
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
import token_oracle as TO  # noqa: E402
from whisper_sae import _native as N  # noqa: E402
from whisper_sae.analysis import TokenAssociation  # noqa: E402

K, T, UTT, VOCAB = 32, 1500, 2048, 51865
SHAPES = [3072, 40960]
TOP_N, MIN_COUNT = 10, 5


def timed(fn, iters: int, warmup: int = 1, prepare=None) -> list:
    pairs = []
    for it in range(warmup + iters):
        if prepare is not None:
            prepare()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        if it >= warmup:
            pairs.append((start, end))
    torch.cuda.synchronize()
    return [start.elapsed_time(end) * 1e3 for start, end in pairs]


def summary(samples: list) -> dict:
    a = np.asarray(samples)
    return {"median_us": float(np.median(a)), "p10_us": float(np.percentile(a, 10)), "p90_us": float(np.percentile(a, 90)),
            "n": int(a.size)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, required=True)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--utterances", type=int, default=UTT)
    ap.add_argument("--batch", type=int, default=64, help="utterances per call of wsae_pair_update")
    ap.add_argument("--out", default=str(ROOT / "outputs" / "token_association_timing.json"))
    args = ap.parse_args()
    H, U = SHAPES[args.shape], args.utterances
    rows = U * T
    dev = torch.device("cuda", 0)
    lib = N.lib()
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream  # noqa: E731
    rng = np.random.default_rng(2700 + args.shape)
    code = RO.persistent_code(rng, rows, K, H)
    vals, idx = torch.from_numpy(code[0]).to(dev), torch.from_numpy(code[1]).to(dev)
    del code
    tokens = torch.from_numpy(TO.zipf_tokens(rng, rows, VOCAB)).to(dev)
    seg = torch.arange(U, dtype=torch.int32, device=dev)[:, None].expand(U, T).reshape(-1).contiguous()
    calls = [(u * T, min(u + args.batch, U) * T) for u in range(0, U, args.batch)]
    base = {"hidden": H, "n_tokens": VOCAB, "k": K, "utterances": U, "frames_per_utterance": T, "rows": rows,
            "entries": rows * K, "utterances_per_call": args.batch}

    # ---- the pass through the tracker: distinct pairs, final capacity, the time with growth ----------------------------------
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tracker = TokenAssociation(H, VOCAB, device=dev)
    for a, b in calls:
        tracker.update((vals[a:b], idx[a:b]), tokens[a:b], segments=seg[a:b])
    n_pairs = tracker.n_pairs
    torch.cuda.synchronize()
    tracker_s = time.perf_counter() - t0
    cap = tracker.capacity
    base.update(distinct_pairs=n_pairs, final_capacity=cap, table_bytes=20 * cap, load_factor=n_pairs / cap,
                growth_steps=tracker.grown, tracker_pass_with_growth_ms=tracker_s * 1e3)
    print(json.dumps(base), flush=True)

    # ---- wsae_pair_update into a fresh table of the final capacity ------------------------------------------------------------
    keys = torch.empty(cap, dtype=torch.int64, device=dev)
    cnt = torch.empty(cap, dtype=torch.int32, device=dev)
    sum_q = torch.empty(cap, dtype=torch.int64, device=dev)
    status = torch.empty(2, dtype=torch.int64, device=dev)
    feat_rows, tok_rows, pair_rows = (torch.empty(n, dtype=torch.int64, device=dev) for n in (H, VOCAB, 1))

    def reset():
        keys.fill_(-1)
        for t in (cnt, sum_q, status, feat_rows, tok_rows, pair_rows):
            t.zero_()

    def update():
        for a, b in calls:
            rc = lib.wsae_pair_update(vals[a:b].data_ptr(), idx[a:b].data_ptr(), K, H, seg[a:b].data_ptr(), tokens[a:b].data_ptr(),
                                      b - a, VOCAB, 0, keys.data_ptr(), cnt.data_ptr(), sum_q.data_ptr(), cap, status.data_ptr(),
                                      feat_rows.data_ptr(), tok_rows.data_ptr(), pair_rows.data_ptr(), stream())
            assert rc == 0, N.last_error()

    out_rows = []
    row = dict(base, what="update", wsae_pair_update=summary(timed(update, args.iters, prepare=reset)))
    assert status.tolist() == [n_pairs, 0]
    row["entries_per_us"] = rows * K / row["wsae_pair_update"]["median_us"]

    # ---- the torch formulation ------------------------------------------------------------------------------------------------
    def torch_table():
        key = (idx.long() << 32 | tokens.long()[:, None]).reshape(-1)  # (every entry is active and every frame a pair here)
        q = torch.round(vals.clamp(max=4096.0) * 1048576.0).long().reshape(-1)
        uk, inv, c = torch.unique(key, return_inverse=True, return_counts=True)
        return uk, c, torch.zeros(uk.numel(), dtype=torch.int64, device=dev).index_add_(0, inv, q)

    uk, uc, us = torch_table()
    used = torch.nonzero(keys >= 0)[:, 0]
    sk, order = torch.sort(keys[used])
    used = used[order]
    assert torch.equal(sk, uk) and torch.equal(cnt[used].long(), uc) and torch.equal(sum_q[used], us)
    assert torch.equal(pair_rows, torch.tensor([rows], device=dev)) and torch.equal(tok_rows, torch.bincount(tokens.long(), minlength=VOCAB))
    assert torch.equal(feat_rows, torch.bincount(idx.reshape(-1).long(), minlength=H))
    del used, sk, order
    row["torch_unique_index_add"] = summary(timed(torch_table, max(3, args.iters // 2), 1))
    row["ratio_torch_over_kernel"] = row["torch_unique_index_add"]["median_us"] / row["wsae_pair_update"]["median_us"]
    print(json.dumps(row), flush=True)
    out_rows.append(row)

    for by, score, groups in ((N.PAIR_BY_FEATURE, "lift", H), (N.PAIR_BY_TOKEN, "precision", VOCAB)):
        need = lib.wsae_pair_top_workspace_bytes(cap, groups)
        ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev)
        ids, counts = (torch.empty(groups, TOP_N, dtype=torch.int32, device=dev) for _ in range(2))
        scores = torch.empty(groups, TOP_N, dtype=torch.float64, device=dev)
        sums = torch.empty(groups, TOP_N, dtype=torch.int64, device=dev)

        def top():
            rc = lib.wsae_pair_top(keys.data_ptr(), cnt.data_ptr(), sum_q.data_ptr(), cap, feat_rows.data_ptr(), tok_rows.data_ptr(),
                                   pair_rows.data_ptr(), H, VOCAB, by, groups, N.PAIR_SCORES.index(score), MIN_COUNT, TOP_N,
                                   ids.data_ptr(), scores.data_ptr(), counts.data_ptr(), sums.data_ptr(), ws.data_ptr(), need, stream())
            assert rc == 0, N.last_error()

        def torch_top():
            keep = uc >= MIN_COUNT
            k2, c2 = uk[keep], uc[keep]
            f, t = k2 >> 32, k2 & 0xFFFFFFFF
            c, a, b = c2.double(), feat_rows[f].double(), tok_rows[t].double()
            s = (c * pair_rows.double()) / (a * b) if score == "lift" else c / a
            grp, ident = (f, t) if by == N.PAIR_BY_FEATURE else (t, f)
            o1 = torch.argsort(s, descending=True, stable=True)  # (keys ascend: equal scores keep the lower id first)
            o2 = o1[torch.argsort(grp[o1], stable=True)]
            g_sorted = grp[o2]
            start = torch.zeros(groups + 1, dtype=torch.int64, device=dev)
            start[1:] = torch.cumsum(torch.bincount(g_sorted, minlength=groups), 0)
            rank = torch.arange(g_sorted.numel(), device=dev) - start[g_sorted]
            head = rank < TOP_N
            out_i = torch.full((groups, TOP_N), -1, dtype=torch.int64, device=dev)
            out_s = torch.full((groups, TOP_N), float("-inf"), dtype=torch.float64, device=dev)
            out_c = torch.zeros(groups, TOP_N, dtype=torch.int64, device=dev)
            at = (g_sorted[head], rank[head])
            out_i[at], out_s[at], out_c[at] = ident[o2][head], s[o2][head], c2[o2][head]
            return out_i, out_s, out_c

        top()
        ti, ts, tc = torch_top()
        assert torch.equal(ids.long(), ti) and torch.equal(counts.long(), tc)
        assert torch.equal(scores.view(torch.int64), ts.view(torch.int64))
        row = dict(base, what="top", by="feature" if by == N.PAIR_BY_FEATURE else "token", score=score, n=TOP_N,
                   min_count=MIN_COUNT, listed=int((ti >= 0).sum()), workspace_bytes=need)
        del ti, ts, tc
        row["wsae_pair_top"] = summary(timed(top, args.iters))
        row["torch_sort_segmented_head"] = summary(timed(torch_top, max(3, args.iters // 2), 1))
        row["ratio_torch_over_kernel"] = row["torch_sort_segmented_head"]["median_us"] / row["wsae_pair_top"]["median_us"]
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
