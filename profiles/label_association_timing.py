"""Time ``wsae_label_update`` against the torch path a user would otherwise write (profiles/label_association_note.md):

kernel   one call over the whole code: S = 8 strata (the profile's quantile edges), C = 41 classes, L = 1 (lag 0) and
         L = 5 (lags -2 .. 2).
torch    the strata by comparison against the gathered edges, then per lag one ``bincount`` of the composite key
         ``((feature L + lag) C + class) S + stratum`` over the entries whose pair holds, and one ``bincount`` of the
         classes for ``pair_rows``.  It yields the same integers, which the script checks before it times anything.
A/B      with ``--experiment-lib``: the form that combines equal cells in LDS first (profiles/experiments/
         wsae_labels_combine.hip) against the shipped form, in this process, alternating call by call, after a check that
         both give the same integers.

The code is ``persistent_code`` of tests/runs_oracle.py, the code the other notes use (distinct indices per row, all
values positive - the torch path relies on that): 2048 utterances of 1500 frames, k = 32, H = 3072 whole width and
H = 40960 through a window of 4096 features.  The labels are piecewise constant with a geometric holding time of mean 6
frames, 5 % of the stretches unlabelled.  One shape per process (``--shape``), device events, median and p10-p90; every
process adds its rows to the output file.

    python profiles/label_association_timing.py --shape 0 [--out outputs/label_association_timing.json]
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
from whisper_sae.analysis.profile import histogram_quantile  # noqa: E402

K, T, UTT = 32, 1500, 2048
SHAPES = [(3072, 0, 3072), (40960, 8192, 4096)]  # (H, f_lo, f_cols)
CLASSES, STRATA = 41, 8
LAG_SETS = [(0, 0), (-2, 2)]


def timed(fn, iters: int) -> list:
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for start, end in pairs:
        start.record()
        fn()
        end.record()
    torch.cuda.synchronize()
    return [start.elapsed_time(end) * 1e3 for start, end in pairs]


def alternating(fns, iters: int) -> list:
    """One sample list per function; the functions take turns call by call."""
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


def torch_labels(vals, idx, labels, f_lo: int, f_cols: int, edges, n_classes: int, lags, cnt, pair_rows) -> None:
    """The plain-torch formulation, added into ``cnt [f_cols, L, C, S]`` int32 and ``pair_rows [L, C]`` int64.  Utterances
    are ``T`` rows each, no padding; indices are distinct within a row and values positive."""
    dev = vals.device
    n_rows = vals.shape[0]
    S, L = edges.shape[1] + 1, lags[1] - lags[0] + 1
    i = idx.long() - f_lo
    inside = (vals > 0) & (i >= 0) & (i < f_cols)
    rows = torch.arange(n_rows, device=dev)[:, None].expand_as(idx)[inside]
    c, v = i[inside], vals[inside]
    stratum = torch.zeros_like(c)
    for j in range(S - 1):
        stratum += edges[:, j][c] <= v
    all_rows = torch.arange(n_rows, device=dev)
    for li in range(L):
        q = all_rows + (lags[0] + li)
        lab = labels[q.clamp(0, n_rows - 1)].long()
        cls = torch.where((q >= 0) & (q < n_rows) & (q // T == all_rows // T) & (lab >= 0) & (lab < n_classes), lab,
                          torch.full_like(lab, -1))
        pair_rows[li] += torch.bincount(cls[cls >= 0], minlength=n_classes)
        mine = cls[rows]
        ok = mine >= 0
        key = ((c[ok] * L + li) * n_classes + mine[ok]) * S + stratum[ok]
        cnt += torch.bincount(key, minlength=cnt.numel()).view(cnt.shape).int()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, required=True, choices=range(len(SHAPES)))
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--utterances", type=int, default=UTT)
    ap.add_argument("--experiment-lib", default="", help="libwsae_labels_combine.so: A/B the LDS-combining form")
    ap.add_argument("--out", default="outputs/label_association_timing.json")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    lib = N.lib()
    stream = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    H, f_lo, f_cols = SHAPES[args.shape]
    rows = args.utterances * T
    rng = np.random.default_rng(H)
    code = RO.persistent_code(rng, rows, K, H)
    vals, idx = torch.from_numpy(code[0]).to(dev), torch.from_numpy(code[1]).to(dev)
    del code
    labels = torch.from_numpy(LO.piecewise_labels(rng, rows, CLASSES, hold=6.0, unlabelled=0.05)).to(dev)
    seg = torch.arange(args.utterances, dtype=torch.int32, device=dev)[:, None].expand(args.utterances, T).reshape(-1).contiguous()

    # the edges: the quantiles of a profile of the same code
    z = lambda *shape, dtype=torch.int32: torch.zeros(*shape, dtype=dtype, device=dev)  # noqa: E731
    prof = {"fires": z(f_cols), "hist": z(f_cols, N.PROFILE_BINS), "max_bits": z(f_cols),
            "min_bits": torch.full((f_cols,), 0x7F800000, dtype=torch.int32, device=dev), "over": z(f_cols),
            "sum_q": z(f_cols, dtype=torch.int64), "total_rows": z(1, dtype=torch.int64)}
    N.check(lib.wsae_profile_update(vals.data_ptr(), idx.data_ptr(), K, H, None, rows, f_lo, f_cols, prof["fires"].data_ptr(),
                                    prof["hist"].data_ptr(), prof["max_bits"].data_ptr(), prof["min_bits"].data_ptr(),
                                    prof["over"].data_ptr(), prof["sum_q"].data_ptr(), prof["total_rows"].data_ptr(), None, 0, stream()),
            "wsae_profile_update")
    edges = torch.stack([histogram_quantile(prof["hist"], prof["fires"], prof["min_bits"], prof["max_bits"], j / STRATA)
                         for j in range(1, STRATA)], dim=1).float().contiguous()
    active = int(prof["fires"].sum())
    del prof

    combine = None
    if args.experiment_lib:
        combine = C.CDLL(args.experiment_lib).wsae_label_update_combine
        combine.restype, combine.argtypes = N.SIGNATURES["wsae_label_update"]

    out_rows = []
    for lags in LAG_SETS:
        L = lags[1] - lags[0] + 1
        state = lambda: (z(f_cols, L, CLASSES, STRATA), z(L, CLASSES, dtype=torch.int64))  # noqa: E731
        cnt, pair_rows = state()

        def call(fn, cnt=cnt, pair_rows=pair_rows, lags=lags):
            rc = fn(vals.data_ptr(), idx.data_ptr(), K, H, seg.data_ptr(), labels.data_ptr(), rows, CLASSES, lags[0], lags[1],
                    f_lo, f_cols, edges.data_ptr(), STRATA, cnt.data_ptr(), pair_rows.data_ptr(), None, 0, stream())
            assert rc == 0, rc

        call(lib.wsae_label_update)
        t_cnt, t_pairs = state()
        torch_labels(vals, idx, labels, f_lo, f_cols, edges, CLASSES, lags, t_cnt, t_pairs)
        torch.cuda.synchronize()
        same = torch.equal(cnt, t_cnt) and torch.equal(pair_rows, t_pairs)
        pairs, increments, distinct = int(pair_rows.sum()), int(cnt.long().sum()), int((cnt > 0).sum())
        t_kernel = timed(lambda: call(lib.wsae_label_update), args.iters)
        t_torch = timed(lambda: torch_labels(vals, idx, labels, f_lo, f_cols, edges, CLASSES, lags, t_cnt, t_pairs),
                        max(2, args.iters // 3))
        sk, stt = summary(t_kernel), summary(t_torch)
        row = {"hidden": H, "f_lo": f_lo, "f_cols": f_cols, "k": K, "utterances": args.utterances, "frames_per_utterance": T,
               "rows": rows, "classes": CLASSES, "strata": STRATA, "lags": list(lags), "active_entries_in_window": active,
               "pairs": pairs, "cnt_increments": increments, "cnt_cells_touched": distinct,
               "same_integers_as_torch": bool(same), "wsae_label_update": sk, "torch_compare_bincount": stt,
               "ratio_torch_over_kernel": stt["median_us"] / sk["median_us"],
               "cnt_increments_per_us": increments / sk["median_us"]}
        if combine is not None:
            c_cnt, c_pairs = state()
            call(combine, c_cnt, c_pairs)
            torch.cuda.synchronize()
            ref_cnt, ref_pairs = state()
            call(lib.wsae_label_update, ref_cnt, ref_pairs)
            torch.cuda.synchronize()
            row["combine_same_integers"] = bool(torch.equal(c_cnt, ref_cnt) and torch.equal(c_pairs, ref_pairs))
            t_a, t_b = alternating([lambda: call(lib.wsae_label_update), lambda: call(combine, c_cnt, c_pairs)], args.iters)
            sa, sb = summary(t_a), summary(t_b)
            row.update(ab_direct=sa, ab_combine=sb, ab_ratio_combine_over_direct=sb["median_us"] / sa["median_us"])
        print(json.dumps(row), flush=True)
        out_rows.append(row)
        del cnt, pair_rows, t_cnt, t_pairs

    out_path = Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    res = json.loads(out_path.read_text()) if out_path.exists() else {"results": []}
    res.update(device=torch.cuda.get_device_name(0), torch=torch.__version__, iters=args.iters)
    res["results"] = [r for r in res["results"] if r["hidden"] != H] + out_rows
    out_path.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
