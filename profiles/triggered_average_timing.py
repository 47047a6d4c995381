"""Time ``wsae_sta_update`` against the torch path a user would otherwise write (profiles/triggered_average_note.md):

kernel  one call over all rows: the transposition of the code to per-feature trigger lists (count, scan, offsets,
        scatter) and the feature-owning accumulation.
torch   per chunk of rows the active entries of the code (``nonzero``), then per lag one ``index_add_`` of
        ``w * y[r + lag]`` in float64 into ``acc [f_cols * L, C]`` (and of ``w`` and 1 into ``wsum`` and ``cnt``).  The
        dense code ``[rows, H]`` a matrix product would need is 37 GB here and is never built.  ``index_add_`` adds with
        atomics in no fixed order, so its sums agree with the kernel's only to rounding: the script checks every cell
        against the first-order bound ``(n - 1) 2^-53 sum |terms|`` (``sum |terms|`` from a kernel pass over ``|y|``),
        and that the counts are equal, before it times anything.

The code has persistence (``persistent_code`` of tests/runs_oracle.py).  Shape of DESIGN.md section 15: 2048 utterances
of 1500 frames, k = 32, a signal of 160 channels, lags -8 .. 8; H = 3072 whole width and H = 40960 through a window of
4096 features.  One process, alternating windows of the paths, device events, median and p10-p90.

    python profiles/triggered_average_timing.py [--out outputs/triggered_average_timing.json] [--note outputs/note.md]

The split of a call into its launches comes from a kernel trace of ``--trace`` (a few calls of the kernel only: whole
window, then the window of the single feature with the longest list, whose accumulation launch is that feature's chain):

    rocprofv3 --kernel-trace --output-format csv -d outputs/sta_trace -- python profiles/triggered_average_timing.py --trace
    python profiles/triggered_average_timing.py --kernel-trace outputs/sta_trace/.../*_kernel_trace.csv
"""

from __future__ import annotations

import argparse
import csv
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

K, T, S, C = 32, 1500, 2048, 160
LAGS = (-8, 8)
L = LAGS[1] - LAGS[0] + 1
SHAPES = [(3072, 0, 3072), (40960, 8192, 4096)]  # (H, f_lo, f_cols)
TRACE_WARM, TRACE_CALLS = 2, 3
LAUNCHES = 5  # count, scan, offsets, scatter, accumulate


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


def new_state(f_cols: int, dev) -> dict:
    return {"acc": torch.zeros(f_cols, L, C, dtype=torch.float64, device=dev),
            "wsum": torch.zeros(f_cols, L, dtype=torch.float64, device=dev),
            "cnt": torch.zeros(f_cols, L, dtype=torch.int64, device=dev)}


def torch_sta(vals, idx, seg, y, f_lo: int, f_cols: int, st: dict, chunk_rows: int) -> None:
    """The plain-torch formulation, added into ``st``.  The code has distinct indices per row and no padding frames."""
    rows = vals.shape[0]
    acc, wsum, cnt = st["acc"].view(f_cols * L, C), st["wsum"].view(-1), st["cnt"].view(-1)
    for r0 in range(0, rows, chunk_rows):
        v, i = vals[r0:r0 + chunk_rows], idx[r0:r0 + chunk_rows].long() - f_lo
        inside = (v > 0) & (i >= 0) & (i < f_cols)
        rr, ee = inside.nonzero(as_tuple=True)
        f, w, r = i[rr, ee] * L, v[rr, ee].double(), rr + r0
        sr = seg[r]
        for j in range(L):
            t = r + (LAGS[0] + j)
            tc = t.clamp(0, rows - 1)
            ok = (t == tc) & (seg[tc] == sr)
            fo, wo = f[ok] + j, w[ok]
            acc.index_add_(0, fo, wo[:, None] * y[tc[ok]].double())
            wsum.index_add_(0, fo, wo)
            cnt.index_add_(0, fo, torch.ones_like(fo))


def read_trace(path: Path) -> list:
    """Per shape the median durations (us) of the launches of the traced calls: whole window, then single feature."""
    with open(path, newline="") as fh:
        rows = [r for r in csv.DictReader(fh) if "sta_" in r.get("Kernel_Name", "")]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    dur = [(r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3) for r in rows]
    per_shape = (TRACE_WARM + 2 * TRACE_CALLS) * LAUNCHES
    if len(dur) != per_shape * len(SHAPES):
        raise SystemExit(f"{path}: {len(dur)} sta_ dispatches, expected {per_shape * len(SHAPES)}")
    out = []
    for s in range(len(SHAPES)):
        calls = [dur[s * per_shape + c * LAUNCHES:s * per_shape + (c + 1) * LAUNCHES] for c in range(TRACE_WARM + 2 * TRACE_CALLS)]
        assert all("accum" in c[4][0] and "walk" in c[0][0] and "walk" in c[3][0] for c in calls), calls[0]
        med = lambda cs, k: float(np.median([c[k][1] for c in cs]))  # noqa: E731
        whole, single = calls[TRACE_WARM:TRACE_WARM + TRACE_CALLS], calls[TRACE_WARM + TRACE_CALLS:]
        out.append({"count_us": med(whole, 0), "scan_us": med(whole, 1), "offsets_us": med(whole, 2), "scatter_us": med(whole, 3),
                    "transposition_us": sum(med(whole, k) for k in range(4)), "accumulation_us": med(whole, 4),
                    "longest_chain_us": med(single, 4)})
    return out


def write_note(path: Path, res: dict) -> None:
    r = res["results"]
    cell = lambda fn: " | ".join(fn(x) for x in r)  # noqa: E731
    us = lambda v: f"{v:.0f} µs"  # noqa: E731
    lines = [
        "# Feature-triggered averages (`wsae_sta_update`): what was measured", "",
        f"Written by `python profiles/triggered_average_timing.py` on an {res['device']} (torch {res['torch']}), together with",
        f"`profiles/triggered_average_timing.json`.  One process, {res['windows']} alternating windows of "
        f"{res['iters_per_window']} kernel calls and one torch pass each, device events, medians; p10 and p90 are in the JSON.", "",
        "## The workload", "",
        f"`persistent_code` of `tests/runs_oracle.py`: {r[0]['utterances']} utterances of {r[0]['frames_per_utterance']} frames "
        f"({r[0]['rows']} rows), k = {K}, a float32 signal of {C} channels, lags {LAGS[0]} .. {LAGS[1]} (L = {L}), every "
        "active frame a trigger weighted by its value.", "",
        "| | " + cell(lambda x: f"H = {x['hidden']}, window [{x['f_lo']}, {x['f_lo'] + x['f_cols']})") + " |",
        "|---|" + "---|" * len(r),
        "| triggers in the window | " + cell(lambda x: str(x["triggers_in_window"])) + " |",
        "| fp64 multiply-adds | " + cell(lambda x: f"{x['fma']:.3g}") + " |",
        "| longest list (triggers of one feature) | " + cell(lambda x: f"{x['longest_list']} (mean {x['mean_list']:.0f})") + " |", "",
        "## Correctness", "",
        "The kernel's `acc`, `wsum` and `cnt` equal the numpy oracle bit for bit on every shape of",
        "`tests/test_gpu_triggered_average.py`.  Here the torch path's counts are compared with the kernel's, and its float64",
        "sums, added with atomics in no fixed order, with the first-order bound `(n - 1) 2^-53 sum |terms|` of every cell" +
        (" - they stay inside it:" if all(x["inside_first_order_bound"] for x in r) else " - NOT all of them stay inside it:"), "",
        "| | " + cell(lambda x: f"H = {x['hidden']}") + " |", "|---|" + "---|" * len(r),
        "| counts equal | " + cell(lambda x: str(x["same_counts_as_torch"])) + " |",
        "| largest `|torch - kernel|` / bound, `acc` | " + cell(lambda x: f"{x['max_acc_error_over_bound']:.3f}") + " |",
        "| largest `|torch - kernel|` / bound, `wsum` | " + cell(lambda x: f"{x['max_wsum_error_over_bound']:.3f}") + " |", "",
        "## Speed", "",
        "| | " + cell(lambda x: f"H = {x['hidden']}") + " |", "|---|" + "---|" * len(r),
        "| `wsae_sta_update`, one call | " + cell(lambda x: us(x["wsae_sta_update"]["median_us"])) + " |",
        "| torch: `nonzero` + per-lag `index_add_` in float64 | " + cell(lambda x: us(x["torch_index_add"]["median_us"])) + " |",
        "| torch / kernel | " + cell(lambda x: f"{x['ratio_torch_over_kernel']:.1f}") + " |",
        "| fp64 multiply-adds per second (kernel) | " + cell(lambda x: f"{x['fma'] / x['wsae_sta_update']['median_us'] / 1e6:.2f} T") + " |"]
    if all("trace" in x for x in r):
        tr = lambda k: cell(lambda x: us(x["trace"][k]))  # noqa: E731
        lines += ["| transposition: count / scan / offsets / scatter (kernel trace) | " +
                  cell(lambda x: " / ".join(f"{x['trace'][k]:.0f}" for k in ("count_us", "scan_us", "offsets_us", "scatter_us")) + " µs") + " |",
                  "| transposition, the four launches | " + tr("transposition_us") + " |",
                  "| accumulation launch | " + tr("accumulation_us") + " |",
                  "| the longest feature's chain alone (accumulation launch of a window of that feature) | " + tr("longest_chain_us") + " |",
                  "| its share of the accumulation launch | " +
                  cell(lambda x: f"{100 * x['trace']['longest_chain_us'] / x['trace']['accumulation_us']:.0f} %") + " |"]
    slower = [x for x in r if x["ratio_torch_over_kernel"] < 1]
    lines += ["", "## What the figures say", ""]
    if slower:
        lines += ["The kernel is NOT faster than the torch formulation at " + ", ".join(f"H = {x['hidden']}" for x in slower) +
                  ": a finding, stated in the README as well.  What torch cannot give at any speed is these bits: its sums", "depend on the order the atomics arrive in.", ""]
    else:
        lines += ["The kernel is ahead of the torch formulation on both shapes, and unlike it gives the same bits every time: the",
                  "torch sums depend on the order the atomics arrive in.", ""]
    lines += ["A feature's chain is sequential by definition, and only the channel tiles (three waves at 160 channels) share it:",
              "the accumulation launch cannot end before the longest list has been walked, whatever the rest of the chip does.",
              "Long lists are scheduled first so that the short ones fill in behind them.", "",
              "Not measured: bf16 signals, k = 128, other lag counts and channel counts, the onset trigger (far fewer, isolated",
              "triggers: the walk over signal rows then looks up L lags per row for one term), codes with other list-length",
              "distributions.", ""]
    path.write_text("\n".join(lines))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--utterances", type=int, default=S)
    ap.add_argument("--frames", type=int, default=T)
    ap.add_argument("--chunk-rows", type=int, default=16384, help="rows per chunk of the torch path")
    ap.add_argument("--trace", action="store_true", help="a few calls of the kernel only (for rocprofv3 --kernel-trace)")
    ap.add_argument("--kernel-trace", default=None, help="the kernel trace CSV of a --trace run: adds the split by launch")
    ap.add_argument("--out", default="outputs/triggered_average_timing.json")
    ap.add_argument("--note", default=None, help="also write the note (markdown) here")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    lib = N.lib()
    stream = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    n_seg, frames = args.utterances, args.frames
    rows = n_seg * frames
    seg = torch.arange(n_seg, dtype=torch.int32, device=dev).repeat_interleave(frames).contiguous()
    y = torch.randn(rows, C, dtype=torch.float32, device=dev, generator=torch.Generator(device=dev).manual_seed(17))
    y_abs = None
    trace = read_trace(Path(args.kernel_trace)) if args.kernel_trace else None
    results = []
    for n_shape, (H, f_lo, f_cols) in enumerate(SHAPES):
        code = RO.persistent_code(np.random.default_rng(H), rows, K, H)
        vals, idx = torch.from_numpy(code[0]).to(dev), torch.from_numpy(code[1]).to(dev)
        del code
        print(f"H = {H}: code on the device", flush=True)

        def call(state, signal, lo=f_lo, cols=f_cols):
            need = lib.wsae_sta_workspace_bytes(rows, K, H, lo, cols)
            nonlocal_ws = call.ws
            if nonlocal_ws is None or nonlocal_ws.numel() < need:
                call.ws = nonlocal_ws = torch.empty(need, dtype=torch.uint8, device=dev)
            N.check(lib.wsae_sta_update(vals.data_ptr(), idx.data_ptr(), K, H, seg.data_ptr(), rows, signal.data_ptr(), N.DT_F32,
                                        C, C, LAGS[0], LAGS[1], lo, cols, N.STA_TRIGGER_ALL, N.STA_WEIGHT_VALUE,
                                        state["acc"].data_ptr(), state["wsum"].data_ptr(), state["cnt"].data_ptr(),
                                        nonlocal_ws.data_ptr(), nonlocal_ws.numel(), stream()), "wsae_sta_update")

        call.ws = None
        st = new_state(f_cols, dev)
        call(st, y)
        torch.cuda.synchronize()
        lists = st["cnt"][:, -LAGS[0]].clone()  # every trigger has its lag-0 term
        longest = int(lists.argmax())
        if args.trace:
            one = new_state(1, dev)
            for _ in range(TRACE_WARM - 1 + TRACE_CALLS):
                call(st, y)
            for _ in range(TRACE_CALLS):
                call(one, y, f_lo + longest, 1)
            torch.cuda.synchronize()
            print(f"H = {H}: traced, longest list {int(lists.max())} (feature {f_lo + longest})", flush=True)
            del vals, idx, st, one
            torch.cuda.empty_cache()
            continue
        # one pass of each path on zeroed state, and the kernel over |y| for the bound
        st_abs, st_torch = new_state(f_cols, dev), new_state(f_cols, dev)
        if y_abs is None:
            y_abs = y.abs()
        call(st_abs, y_abs)
        torch_sta(vals, idx, seg, y, f_lo, f_cols, st_torch, args.chunk_rows)
        torch.cuda.synchronize()
        print(f"H = {H}: torch pass done", flush=True)
        same_counts = bool(torch.equal(st["cnt"], st_torch["cnt"]))
        u = 2.0 ** -53
        n1 = (st["cnt"] - 1).clamp(min=0).double()
        bound_acc = n1[..., None] * u * st_abs["acc"]
        bound_w = n1 * u * st["wsum"]
        err_acc, err_w = (st["acc"] - st_torch["acc"]).abs(), (st["wsum"] - st_torch["wsum"]).abs()
        over = lambda err, bound: float(torch.where(err > 0, err / bound, torch.zeros_like(err)).max())  # noqa: E731 (x / 0 = inf)
        ratio_acc, ratio_w = over(err_acc, bound_acc), over(err_w, bound_w)
        n_trig, terms = int(lists.sum()), int(st["cnt"].sum())
        del st_abs, bound_acc, err_acc
        torch.cuda.empty_cache()

        def kernel_path():
            call(st, y)

        def torch_path():
            torch_sta(vals, idx, seg, y, f_lo, f_cols, st_torch, args.chunk_rows)

        kernel_path()
        torch.cuda.synchronize()
        t_kernel, t_torch = [], []
        for _ in range(args.windows):
            t_kernel += timed(kernel_path, args.iters)
            t_torch += timed(torch_path, 1)
            print(f"H = {H}: window done", flush=True)
        sk, so = summary(t_kernel), summary(t_torch)
        row = {"hidden": H, "f_lo": f_lo, "f_cols": f_cols, "k": K, "utterances": n_seg, "frames_per_utterance": frames,
               "rows": rows, "channels": C, "lags": list(LAGS), "triggers_in_window": n_trig, "terms": terms, "fma": terms * C,
               "longest_list": int(lists.max()), "longest_feature": f_lo + longest, "mean_list": n_trig / f_cols,
               "same_counts_as_torch": same_counts, "max_acc_error_over_bound": ratio_acc,
               "max_wsum_error_over_bound": ratio_w, "inside_first_order_bound": bool(ratio_acc <= 1.0 and ratio_w <= 1.0),
               "wsae_sta_update": sk, "torch_index_add": so, "torch_chunk_rows": args.chunk_rows,
               "ratio_torch_over_kernel": so["median_us"] / sk["median_us"]}
        if trace is not None:
            row["trace"] = trace[n_shape]
        print(json.dumps(row), flush=True)
        results.append(row)
        del vals, idx, st, st_torch
        torch.cuda.empty_cache()
    if args.trace:
        return
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "windows": args.windows,
           "iters_per_window": args.iters, "results": results}
    out_path = Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(res, indent=1) + "\n")
    if args.note:
        write_note(Path(args.note), res)


if __name__ == "__main__":
    main()
