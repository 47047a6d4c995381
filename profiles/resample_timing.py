"""Time ``wsae_resample`` against the same algorithm in torch on the same device (profiles/resample_note.md).

The data: 64 utterances of 30 s at the source rate (seeded noise plus two tones, lengths varied between 15 and 30 s),
resident on the device.  Cells: 48 kHz stereo int16 -> float32, 48 kHz mono float32 -> float32, 44.1 kHz stereo int16 ->
int16, 8 kHz mono int16 -> float32, all to 16 kHz.  Per cell, on the same data:

kernel    ``Resampler.__call__`` into a preallocated output (one kernel; the tap table is resident).
torch     what torchaudio's ``Resample`` does, written here from the formula of ``sinc_resample_kernel``: conversion to
          float32, channel mean, ``F.pad``, ``F.conv1d(x[:, None], kernel[:, None], stride=orig)``, transpose, crop (and
          ``round(y * 32768)``, clamp, ``to(int16)`` where the cell asks for int16).  The dense kernel is resident.

The two are timed in ALTERNATING windows (``--rounds`` x [``--calls`` kernel calls, ``--calls`` / 5 torch calls]), device
events around every window, after a warm-up of both; the median window and the spread are kept.  "Bytes needed" counts every
valid input element read once and every output cell written once; the rate is set against the 6.3 TB/s that
profiles/audio_clips_note.md takes as achievable.  The largest difference between the two results is recorded: the orders
of summation differ, so it is not zero.

    python profiles/resample_timing.py [--out outputs/resample_timing.json]
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "whisper-sae_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from whisper_sae.data import Resampler, sinc_resample_kernel  # noqa: E402

SECONDS, NEW_FREQ = 30, 16000
HBM_ACHIEVABLE = 6.3e12
CELLS = (("48k stereo int16 -> float32", 48000, 2, torch.int16, torch.float32),
         ("48k mono float32 -> float32", 48000, 1, torch.float32, torch.float32),
         ("44.1k stereo int16 -> int16", 44100, 2, torch.int16, torch.int16),
         ("8k mono int16 -> float32", 8000, 1, torch.int16, torch.float32))


def waveforms(n: int, rate: int, channels: int, dtype, seed: int):
    """``(x [n, S, channels] or [n, S], lengths)`` on the host; the channels differ by a gain."""
    g = torch.Generator().manual_seed(seed)
    S = SECONDS * rate
    t = torch.arange(S, dtype=torch.float32) / rate
    hz = 100.0 + 3000.0 * torch.rand(n, 2, generator=g)
    wave = 0.05 * torch.randn(n, S, generator=g)
    wave += 0.3 * torch.sin(2 * torch.pi * hz[:, :1] * t) + 0.2 * torch.sin(2 * torch.pi * hz[:, 1:] * t)
    if channels > 1:
        wave = torch.stack([wave * (1.0 - 0.1 * c) for c in range(channels)], dim=2)
    if dtype == torch.int16:
        wave = (wave * 32768).round().clamp(-32768, 32767).to(torch.int16)
    lengths = torch.randint(S // 2, S + 1, (n,), generator=g)
    lengths[0] = S
    return wave.contiguous(), lengths.to(torch.int32)


def torch_resample(x, lengths, dense, width: int, orig: int, new: int, out_dtype):
    """torchaudio's ``_apply_sinc_resample_kernel`` on a batch, samples beyond a length zeroed first."""
    f = x.to(torch.float32) * (2.0 ** -15) if x.dtype == torch.int16 else x
    if f.dim() == 3:
        f = f.mean(dim=2)
    S = f.shape[1]
    f = f * (torch.arange(S, device=f.device)[None, :] < lengths[:, None])
    y = F.conv1d(F.pad(f, (width, width + orig))[:, None], dense[:, None], stride=orig)
    y = y.transpose(1, 2).reshape(f.shape[0], -1)[:, :-(-new * S // orig)]
    if out_dtype == torch.int16:
        y = (y * 32768).round().clamp(-32768, 32767).to(torch.int16)
    return y


def window_ms(fn, calls: int) -> float:
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / calls


def summary(samples: list) -> dict:
    a = np.asarray(samples)
    return {"median_ms": float(np.median(a)), "min_ms": float(a.min()), "max_ms": float(a.max()), "windows": int(a.size)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--utterances", type=int, default=64)
    ap.add_argument("--out", default=str(ROOT / "outputs" / "resample_timing.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    U = args.utterances
    rows = []
    for name, rate, channels, x_dtype, out_dtype in CELLS:
        host, lengths = waveforms(U, rate, channels, x_dtype, 3100 + rate // 100 + channels)
        x, lengths = host.to(dev), lengths.to(dev)
        rs = Resampler(rate, NEW_FREQ, dev)
        kernel64, width = sinc_resample_kernel(rate, NEW_FREQ)
        dense = torch.from_numpy(kernel64).to(dev, torch.float32)
        S = x.shape[1]
        out = torch.empty(U, rs.out_cols(S), dtype=out_dtype, device=dev)
        kernel = lambda: rs(x, lengths, out=out)  # noqa: E731
        baseline = lambda: torch_resample(x, lengths, dense, width, rs.orig, rs.new, out_dtype)  # noqa: E731
        _, out_len = kernel()
        want = baseline()
        valid = torch.arange(out.shape[1], device=dev)[None, :] < out_len[:, None]
        diff = (out.to(torch.float32) - want.to(torch.float32)).abs() * valid
        row = {"cell": name, "utterances": U, "orig_freq": rate, "channels": channels, "frames": S, "out_cols": int(out.shape[1]),
               "orig": rs.orig, "new": rs.new, "n_taps": rs.n_taps, "halo": rs.halo,
               "max_abs_difference_to_torch": float(diff.max()), "cells_that_differ": int((diff > 0).sum()),
               "cells_compared": int(valid.sum())}
        del want, diff, valid
        for _ in range(2):  # warm-up of both
            window_ms(kernel, args.calls)
            window_ms(baseline, max(1, args.calls // 5))
        k_ms, t_ms = [], []
        for _ in range(args.rounds):
            k_ms.append(window_ms(kernel, args.calls))
            t_ms.append(window_ms(baseline, max(1, args.calls // 5)))
        row["wsae_resample"] = summary(k_ms)
        row["torch_on_device"] = summary(t_ms)
        row["ratio_torch_over_kernel"] = row["torch_on_device"]["median_ms"] / row["wsae_resample"]["median_ms"]
        needed = int(lengths.sum()) * channels * x.element_size() + out.numel() * out.element_size()
        row["needed_bytes"] = needed
        row["needed_bytes_per_s"] = needed / (row["wsae_resample"]["median_ms"] * 1e-3)
        row["share_of_achievable_hbm"] = row["needed_bytes_per_s"] / HBM_ACHIEVABLE
        row["needed_fma"] = int(out_len.sum()) * rs.n_taps
        row["fma_per_s"] = row["needed_fma"] / (row["wsae_resample"]["median_ms"] * 1e-3)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del x, out, dense, rs
        torch.cuda.empty_cache()
    out_path = Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps({"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "rounds": args.rounds,
                                    "calls_per_window": args.calls, "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE,
                                    "results": rows}, indent=1) + "\n")


if __name__ == "__main__":
    main()
