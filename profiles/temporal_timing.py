"""Time ``wsae_runs_update`` against the torch path a user would otherwise write (profiles/temporal_note.md):

kernel  (a) the statistics alone (run counts, lengths, the two histograms), straight from the compact code;
        (b) the same with the event list (every run, ``min_event_len`` = 1; the cursor is reset before each call).
torch   per chunk of utterances a dense boolean ``[utterances, features, frames]`` tensor scattered from the code, run
        starts and ends as differences along time, ``nonzero`` (which lists them in (utterance, feature, frame) order,
        so the i-th start pairs with the i-th end), then ``bincount`` / ``scatter_reduce`` per feature.  It yields the
        same integers, which the script checks before it times anything.

The code has persistence (``persistent_code`` of tests/runs_oracle.py: per code column an on/off Markov chain with mean
holding times from 1 to 256 frames); an i.i.d. code has almost no run longer than a frame and would time the wrong
thing.  Shape of DESIGN.md section 15: 2048 utterances of 1500 frames, k = 32, H = 3072 whole width and H = 40960
through a window of 4096 features.  One process, alternating windows of the paths, device events, median and p10-p90.

    python profiles/temporal_timing.py [--out outputs/temporal_timing.json]
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

K, T, S = 32, 1500, 2048
SHAPES = [(3072, 0, 3072), (40960, 8192, 4096)]  # (H, f_lo, f_cols)
BINS = N.RUNS_BINS
FIELDS = ("frames", "runs", "dur_max", "dur_sq", "dur_hist", "gap_hist")


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
    z = lambda *shape, dtype=torch.int32: torch.zeros(*shape, dtype=dtype, device=dev)  # noqa: E731
    return {"frames": z(f_cols), "runs": z(f_cols), "dur_max": z(f_cols), "dur_sq": z(f_cols, dtype=torch.int64),
            "dur_hist": z(f_cols, BINS), "gap_hist": z(f_cols, BINS), "total_rows": z(1, dtype=torch.int64)}


def bin_of(x: torch.Tensor, edges: torch.Tensor) -> torch.Tensor:
    """The histogram bin of lengths ``x >= 1`` (include/wsae.h): ``edges`` = 64, 128, ..., 2^20."""
    return torch.where(x <= 32, x - 1, 32 + torch.bucketize(x - 1, edges, right=True))


def torch_runs(vals, idx, n_utt: int, frames: int, f_lo: int, f_cols: int, st: dict, chunk: int) -> None:
    """The plain-torch formulation, added into ``st``.  The code has distinct indices per row and no padding frames."""
    dev = vals.device
    edges = 2 ** torch.arange(6, 21, device=dev)
    v3, i3 = vals.view(n_utt, frames, -1), idx.view(n_utt, frames, -1)
    for u0 in range(0, n_utt, chunk):
        v, i = v3[u0:u0 + chunk], i3[u0:u0 + chunk].long() - f_lo
        U = v.shape[0]
        inside = (v > 0) & (i >= 0) & (i < f_cols)
        on = torch.zeros(U, frames, f_cols + 1, dtype=torch.bool, device=dev)
        on.scatter_(2, torch.where(inside, i, torch.full_like(i, f_cols)), inside)
        on = on[:, :, :f_cols].transpose(1, 2).contiguous()  # [U, F, T]: nonzero then lists (utterance, feature, frame)
        first = on.clone()
        first[:, :, 1:] &= ~on[:, :, :-1]
        last = on.clone()
        last[:, :, :-1] &= ~on[:, :, 1:]
        a, b = first.nonzero(), last.nonzero()
        f, d = a[:, 1], b[:, 2] - a[:, 2] + 1
        st["runs"] += torch.bincount(f, minlength=f_cols).int()
        st["frames"] += on.sum((0, 2)).int()
        st["dur_sq"] += torch.zeros(f_cols, dtype=torch.int64, device=dev).index_add_(0, f, d * d)
        st["dur_max"].copy_(torch.maximum(st["dur_max"], torch.zeros(f_cols, dtype=torch.int64, device=dev)
                                          .scatter_reduce_(0, f, d, "amax").int()))
        st["dur_hist"] += torch.bincount(f * BINS + bin_of(d, edges), minlength=f_cols * BINS).view(f_cols, BINS).int()
        follows = (a[1:, 0] == a[:-1, 0]) & (a[1:, 1] == a[:-1, 1])  # the next run of the same (utterance, feature)
        g = (a[1:, 2] - b[:-1, 2] - 1)[follows]
        st["gap_hist"] += torch.bincount(f[1:][follows] * BINS + bin_of(g, edges), minlength=f_cols * BINS).view(f_cols, BINS).int()
        st["total_rows"] += U * frames


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--utterances", type=int, default=S)
    ap.add_argument("--frames", type=int, default=T)
    ap.add_argument("--chunk", type=int, default=64, help="utterances per dense chunk of the torch path")
    ap.add_argument("--out", default="outputs/temporal_timing.json")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    lib = N.lib()
    stream = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    n_seg, frames = args.utterances, args.frames
    rows = n_seg * frames
    seg = torch.arange(n_seg, dtype=torch.int32, device=dev).repeat_interleave(frames).contiguous()
    results = []
    for H, f_lo, f_cols in SHAPES:
        code = RO.persistent_code(np.random.default_rng(H), rows, K, H)
        vals, idx = torch.from_numpy(code[0]).to(dev), torch.from_numpy(code[1]).to(dev)
        del code
        ws = torch.empty(lib.wsae_runs_workspace_bytes(rows, K, H, n_seg, f_lo, f_cols), dtype=torch.uint8, device=dev)
        st, st_ev, st_torch = (new_state(f_cols, dev) for _ in range(3))
        cursor = torch.zeros(1, dtype=torch.int64, device=dev)

        def call(state, ev_int=None, ev_flt=None, cap=0, count=None):
            N.check(lib.wsae_runs_update(vals.data_ptr(), idx.data_ptr(), K, H, seg.data_ptr(), rows, n_seg, 0, f_lo, f_cols,
                                         state["frames"].data_ptr(), state["runs"].data_ptr(), state["dur_max"].data_ptr(),
                                         state["dur_sq"].data_ptr(), state["dur_hist"].data_ptr(), state["gap_hist"].data_ptr(),
                                         state["total_rows"].data_ptr(), N.ptr(ev_int), N.ptr(ev_flt), cap, 1, N.ptr(count),
                                         ws.data_ptr(), ws.numel(), stream()), "wsae_runs_update")

        # one pass of each path on zeroed state: the same integers, and the size of the event list
        call(st)
        call(st_ev, count=cursor)  # (capacity 0: the call only counts)
        n_events = int(cursor.item())
        ev_int = torch.zeros(n_events, 4, dtype=torch.int32, device=dev)
        ev_flt = torch.zeros(n_events, 2, dtype=torch.float32, device=dev)
        torch_runs(vals, idx, n_seg, frames, f_lo, f_cols, st_torch, args.chunk)
        torch.cuda.synchronize()
        equal = all(torch.equal(st[f], st_torch[f]) and torch.equal(st[f], st_ev[f]) for f in FIELDS + ("total_rows",))
        n_runs, n_frames = int(st["runs"].sum()), int(st["frames"].sum())
        assert n_events == n_runs, (n_events, n_runs)
        hist = st["dur_hist"].sum(0).cpu().numpy()

        def stats_only():
            call(st)

        def with_events():
            cursor.zero_()
            call(st_ev, ev_int, ev_flt, n_events, cursor)

        def torch_path():
            torch_runs(vals, idx, n_seg, frames, f_lo, f_cols, st_torch, args.chunk)

        for fn in (stats_only, with_events):
            fn()
        torch.cuda.synchronize()
        t_stats, t_events, t_torch = [], [], []
        for _ in range(args.windows):
            t_stats += timed(stats_only, args.iters)
            t_events += timed(with_events, args.iters)
            t_torch += timed(torch_path, max(1, args.iters // 2))
        ss, se, so = summary(t_stats), summary(t_events), summary(t_torch)
        row = {"hidden": H, "f_lo": f_lo, "f_cols": f_cols, "k": K, "utterances": n_seg, "frames_per_utterance": frames,
               "rows": rows, "active_frames_in_window": n_frames, "runs_in_window": n_runs,
               "mean_run_length": n_frames / max(n_runs, 1), "longest_run": int(st["dur_max"].max()),
               "runs_of_one_frame": int(hist[0]), "runs_longer_than_32": int(hist[32:].sum()),
               "same_integers_as_torch": bool(equal),
               "wsae_runs_update": ss, "wsae_runs_update_with_events": se, "torch_dense_diff_bincount": so,
               "torch_chunk_utterances": args.chunk,
               "ratio_torch_over_kernel": so["median_us"] / ss["median_us"],
               "ratio_torch_over_kernel_with_events": so["median_us"] / se["median_us"],
               "code_gbytes_per_s": rows * K * 8 / ss["median_us"] / 1e3,
               "runs_per_us": n_runs / ss["median_us"]}
        print(json.dumps(row), flush=True)
        results.append(row)
        del vals, idx, st, st_ev, st_torch, ev_int, ev_flt
        torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "windows": args.windows,
           "iters_per_window": args.iters, "results": results}
    out_path = Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
