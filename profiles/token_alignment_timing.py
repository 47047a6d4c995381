"""Time ``wsae_align_cost`` and ``wsae_align_dtw`` against what a user would otherwise run (profiles/token_alignment_note.md).

The data: ``--utterances`` (16) utterances of softmaxed random logits with a diagonal ridge, 1500 frames; shape 0 is 10
heads x 448 tokens (a full decoder context on the alignment heads of a large checkpoint), shape 1 is 6 heads x 64 tokens
(a short transcript on those of a small one); float32 and float16 weights.

cost     ``wsae_align_cost`` (width 7) against the formulation of ``transformers`` on the same device, in the dtype of the
         weights: ``torch.std_mean(unbiased=False)`` over the token axis, ``_median_filter`` (reflect pad, unfold, sort),
         the negative mean over the heads.  The largest difference between the two costs is recorded (the float32
         formulation rounds more often than the kernel does; the float16 one computes in float16).
dtw      ``wsae_align_dtw`` on the kernel's cost, all utterances in one call, against (a) ``_dynamic_time_warping`` of
         ``transformers`` on the CPU - what users run today; one utterance, host clock, times the number of utterances -
         and (b) an anti-diagonal DTW written in torch on the device, all utterances in one batch: one gather / compare /
         scatter round per anti-diagonal.  (b) performs the same float32 addition per cell, so the script asserts that
         its final costs equal ``path_cost`` bit for bit; (a)'s path of utterance 0 must equal the kernel's.

Device events around every call, warm-up calls, median and p10-p90; one shape per process (``--shape``); every process
adds its rows to the output file.

    python profiles/token_alignment_timing.py --shape 0 [--out outputs/token_alignment_timing.json]
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

from whisper_sae import _native as N  # noqa: E402

FRAMES, WIDTH = 1500, 7
SHAPES = [(10, 448), (6, 64)]  # (heads, tokens)


def timed(fn, iters: int, warmup: int = 2) -> list:
    pairs = []
    for it in range(warmup + iters):
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


def ridge_weights(n_utt: int, n_heads: int, n_tok: int, frames: int, dev, seed: int) -> torch.Tensor:
    """Softmaxed random logits with a diagonal ridge, float32 ``[n_utt, n_heads, n_tok, frames]`` (tests/align_oracle.py's
    ``attention``, generated on the device)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    logits = torch.randn(n_utt, n_heads, n_tok, frames, generator=g, device=dev)
    centre = (torch.arange(n_tok, device=dev)[:, None] + 0.5) * frames / n_tok
    logits += 4.0 * torch.exp(-0.5 * ((torch.arange(frames, device=dev)[None, :] - centre) / max(frames / n_tok, 1.0)) ** 2)
    return torch.softmax(logits, dim=-1)


def library_cost(w: torch.Tensor, median_filter) -> torch.Tensor:
    std, mean = torch.std_mean(w, dim=-2, keepdim=True, unbiased=False)
    return -median_filter((w - mean) / std, WIDTH).mean(dim=1)


def wavefront_plan(n: int, k: int, dev):
    """Per anti-diagonal the row and column indices of its cells in the (n + 1) x (k + 1) table."""
    plan = []
    for d in range(2, n + k + 1):
        i = torch.arange(max(1, d - k), min(n, d - 1) + 1, device=dev)
        plan.append((i, d - i))
    return plan


def wavefront_dtw(cost: torch.Tensor, plan) -> torch.Tensor:
    """``D [n_utt, n + 1, k + 1]`` float32 of ``cost [n_utt, n, k]``: the recurrence of the library, an anti-diagonal at a
    time, every utterance at once."""
    n_utt, n, k = cost.shape
    D = torch.full((n_utt, n + 1, k + 1), float("inf"), dtype=torch.float32, device=cost.device)
    D[:, 0, 0] = 0.0
    for i, j in plan:
        c0, c1, c2 = D[:, i - 1, j - 1], D[:, i - 1, j], D[:, i, j - 1]
        diag = (c0 < c1) & (c0 < c2)
        up = ~diag & (c1 < c0) & (c1 < c2)
        D[:, i, j] = cost[:, i - 1, j - 1] + torch.where(diag, c0, torch.where(up, c1, c2))
    return D


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, required=True)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--utterances", type=int, default=16)
    ap.add_argument("--frames", type=int, default=FRAMES)
    ap.add_argument("--out", default=str(ROOT / "outputs" / "token_alignment_timing.json"))
    args = ap.parse_args()
    import transformers.models.whisper.generation_whisper as G
    n_heads, n_tok = SHAPES[args.shape]
    U, F = args.utterances, args.frames
    dev = torch.device("cuda", 0)
    lib = N.lib()
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream  # noqa: E731
    w32 = ridge_weights(U, n_heads, n_tok, F, dev, 2800 + args.shape)
    nt = torch.full((U,), n_tok, dtype=torch.int32, device=dev)
    nf = torch.full((U,), F, dtype=torch.int32, device=dev)
    first = torch.zeros(U, dtype=torch.int32, device=dev)
    cost = torch.empty(U, n_tok, F, dtype=torch.float32, device=dev)
    n_bad = torch.empty(U, dtype=torch.int32, device=dev)
    status = torch.zeros(2, dtype=torch.int64, device=dev)
    frame_pos = torch.empty(U, F, dtype=torch.int32, device=dev)
    tok_start, tok_end = (torch.empty(U, n_tok, dtype=torch.int32, device=dev) for _ in range(2))
    path_cost = torch.empty(U, dtype=torch.float32, device=dev)
    path_len = torch.empty(U, dtype=torch.int32, device=dev)
    need = lib.wsae_align_workspace_bytes(U, n_tok, F)
    ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev)
    base = {"utterances": U, "heads": n_heads, "tokens": n_tok, "frames": F, "width": WIDTH}
    out_rows = []

    for dtype, code in ((torch.float16, N.DT_F16), (torch.float32, N.DT_F32)):  # (float32 last: its cost feeds the DTW)
        w = w32.to(dtype)

        def kernel_cost():
            rc = lib.wsae_align_cost(w.data_ptr(), code, U, n_heads, n_tok, F, nt.data_ptr(), nf.data_ptr(), WIDTH, cost.data_ptr(),
                                     n_bad.data_ptr(), status.data_ptr(), stream())
            assert rc == 0, N.last_error()

        kernel_cost()
        want = library_cost(w, G._median_filter)
        assert status.tolist() == [0, 0]
        row = dict(base, what="cost", dtype=str(dtype).replace("torch.", ""), weight_bytes=w.numel() * w.element_size(),
                   max_abs_difference=float((cost - want.float()).abs().max()))
        del want
        row["wsae_align_cost"] = summary(timed(kernel_cost, args.iters))
        row["torch_std_mean_median_filter"] = summary(timed(lambda: library_cost(w, G._median_filter), max(3, args.iters // 4), 1))
        row["ratio_torch_over_kernel"] = row["torch_std_mean_median_filter"]["median_us"] / row["wsae_align_cost"]["median_us"]
        row["weight_gb_per_s"] = row["weight_bytes"] / row["wsae_align_cost"]["median_us"] * 1e-3
        print(json.dumps(row), flush=True)
        out_rows.append(row)
    del w, w32

    def kernel_dtw():
        rc = lib.wsae_align_dtw(cost.data_ptr(), U, n_tok, F, first.data_ptr(), nt.data_ptr(), nf.data_ptr(), n_bad.data_ptr(),
                                frame_pos.data_ptr(), tok_start.data_ptr(), tok_end.data_ptr(), path_cost.data_ptr(),
                                path_len.data_ptr(), status.data_ptr(), ws.data_ptr(), need, stream())
        assert rc == 0, N.last_error()

    kernel_dtw()
    torch.cuda.synchronize()
    assert status.tolist() == [0, 0] and bool((path_len > 0).all())
    row = dict(base, what="dtw", cells=U * n_tok * F, workspace_bytes=need)
    row["wsae_align_dtw"] = summary(timed(kernel_dtw, args.iters))
    # (a) the library on the CPU: utterance 0
    m = cost[0].cpu().numpy()
    t0 = time.perf_counter()
    text, time_idx = G._dynamic_time_warping(m)
    cpu_s = time.perf_counter() - t0
    jumps = np.pad(np.diff(text), (1, 0), constant_values=1).astype(bool)
    assert np.array_equal(time_idx[jumps], tok_start[0].cpu().numpy()) and len(text) == int(path_len[0])
    row["library_cpu_one_utterance_ms"] = cpu_s * 1e3
    row["library_cpu_all_utterances_ms"] = cpu_s * 1e3 * U
    row["ratio_library_cpu_over_kernel"] = cpu_s * 1e6 * U / row["wsae_align_dtw"]["median_us"]
    # (b) the anti-diagonal formulation on the device
    plan = wavefront_plan(n_tok, F, dev)
    D = wavefront_dtw(cost, plan)
    assert torch.equal(D[:, n_tok, F].view(torch.int32), path_cost.view(torch.int32))
    del D
    row["torch_antidiagonal"] = summary(timed(lambda: wavefront_dtw(cost, plan), 3, 1))
    row["ratio_torch_over_kernel"] = row["torch_antidiagonal"]["median_us"] / row["wsae_align_dtw"]["median_us"]
    row["cells_per_us"] = row["cells"] / row["wsae_align_dtw"]["median_us"]
    print(json.dumps(row), flush=True)
    out_rows.append(row)

    out_path = Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    res = json.loads(out_path.read_text()) if out_path.exists() else {"results": []}
    res.update(device=torch.cuda.get_device_name(0), torch=torch.__version__, iters=args.iters)
    res["results"] = [r for r in res["results"] if (r["heads"], r["tokens"]) != (n_heads, n_tok)] + out_rows
    out_path.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
