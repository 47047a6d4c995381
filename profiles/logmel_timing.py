"""Time ``wsae_logmel`` against what a user would otherwise run (profiles/logmel_note.md).

The data: ``U`` utterances of 30 s (480000 samples, float32: seeded noise plus two tones, lengths varied), ``U`` in 16, 64;
``n_mels`` in 80, 128.  Per cell, on the same data:

kernel    ``LogMel.__call__`` into a preallocated output (both kernels; the tables and the workspace are resident).
torch     baseline 2: the arithmetic of ``WhisperFeatureExtractor._torch_extract_fbank_features`` on the device - Hann
          window, ``torch.stft``, ``|.|^2`` without the last frame, ``filters.T @``, clamp, ``log10``, the per-utterance maximum,
          ``(v + 4) / 4`` - the waveforms already on the device, the result left there.
cpu       baseline 1: the installed extractor's default call on the host (what the reference pays per batch), host clock,
          on ``--cpu-utterances`` (16) utterances; for 64 the figure is scaled and says so.

The kernel and the torch baseline are timed in ALTERNATING windows (``--rounds`` x [``--calls`` kernel calls, ``--calls`` / 5
torch calls]), device events around every window, after a warm-up of both; the median window and the spread are kept.
Achieved FLOP/s counts the operations the algorithm needs (``2 * 400 * 402`` for the DFT and ``2 * 201 * n_mels`` for the mel
contraction per frame) against the 155 TFLOP/s measured for the f32-input MFMA; the executed (zero-padded) count is also
given.  The largest difference between the kernel's and the torch baseline's features is recorded.

    python profiles/logmel_timing.py [--out outputs/logmel_timing.json]
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

from whisper_sae.data import LogMel, mel_filter_bank  # noqa: E402

P, HOP, N_FFT = 480000, 160, 400
F32_MFMA_PEAK = 155e12


def waveforms(n: int, seed: int):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(P, dtype=torch.float32) / 16000.0
    hz = 100.0 + 3000.0 * torch.rand(n, 2, generator=g)
    wave = 0.05 * torch.randn(n, P, generator=g)
    wave += 0.3 * torch.sin(2 * torch.pi * hz[:, :1] * t) + 0.2 * torch.sin(2 * torch.pi * hz[:, 1:] * t)
    lengths = torch.randint(P // 2, P + 1, (n,), generator=g)
    lengths[0] = P
    wave[torch.arange(P)[None, :] >= lengths[:, None]] = 0.0
    return wave, lengths.to(torch.int32)


def torch_features(wave: torch.Tensor, window: torch.Tensor, filters_t: torch.Tensor) -> torch.Tensor:
    stft = torch.stft(wave, N_FFT, HOP, window=window, return_complex=True)
    magnitudes = (stft[..., :-1].abs() ** 2).contiguous()
    log_spec = torch.clamp(filters_t @ magnitudes, min=1e-10).log10()
    max_val = log_spec.max(dim=2, keepdim=True)[0].max(dim=1, keepdim=True)[0]
    return (torch.maximum(log_spec, max_val - 8.0) + 4.0) / 4.0


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
    ap.add_argument("--cpu-utterances", type=int, default=16)
    ap.add_argument("--utterances", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--out", default=str(ROOT / "outputs" / "logmel_timing.json"))
    args = ap.parse_args()
    from transformers import WhisperFeatureExtractor
    dev = torch.device("cuda", 0)
    rows = []
    for U in args.utterances:
        host_wave, lengths = waveforms(U, 2900 + U)
        wave = host_wave.to(dev)
        for n_mels in (80, 128):
            frontend = LogMel(n_mels, dev)
            out = torch.empty(U, n_mels, P // HOP, device=dev)
            window = torch.hann_window(N_FFT, device=dev)
            filters_t = torch.from_numpy(mel_filter_bank(n_mels)).to(dev, torch.float32).T.contiguous()
            kernel = lambda: frontend(wave, lengths_dev, out=out)  # noqa: E731
            lengths_dev = lengths.to(dev)
            baseline = lambda: torch_features(wave, window, filters_t)  # noqa: E731
            kernel()
            want = baseline()
            row = {"utterances": U, "n_mels": n_mels, "n_samples": P, "frames": P // HOP,
                   "max_abs_difference_to_torch": float((out - want).abs().max())}
            del want
            for _ in range(2):  # warm-up of both
                window_ms(kernel, args.calls)
                window_ms(baseline, max(1, args.calls // 5))
            k_ms, t_ms = [], []
            for _ in range(args.rounds):
                k_ms.append(window_ms(kernel, args.calls))
                t_ms.append(window_ms(baseline, max(1, args.calls // 5)))
            row["wsae_logmel"] = summary(k_ms)
            row["torch_on_device"] = summary(t_ms)
            row["ratio_torch_over_kernel"] = row["torch_on_device"]["median_ms"] / row["wsae_logmel"]["median_ms"]
            frames = U * (P // HOP)
            needed = frames * (2 * 400 * 402 + 2 * 201 * n_mels)
            executed = frames * (2 * 400 * 416 + 2 * 208 * n_mels)
            row["needed_gflop"], row["executed_gflop"] = needed * 1e-9, executed * 1e-9
            row["achieved_tflops_needed"] = needed / (row["wsae_logmel"]["median_ms"] * 1e-3) * 1e-12
            row["share_of_f32_mfma_peak"] = needed / (row["wsae_logmel"]["median_ms"] * 1e-3) / F32_MFMA_PEAK
            # baseline 1: the extractor's default call on the host
            n_cpu = min(U, args.cpu_utterances)
            extractor = WhisperFeatureExtractor(feature_size=n_mels)
            clips = [host_wave[i, :int(lengths[i])].numpy() for i in range(n_cpu)]
            extractor(clips[:1], sampling_rate=16000, return_tensors="np")
            cpu = []
            for _ in range(2):
                t0 = time.perf_counter()
                extractor(clips, sampling_rate=16000, return_tensors="np")
                cpu.append((time.perf_counter() - t0) * 1e3)
            row["extractor_cpu_ms"] = min(cpu) * U / n_cpu
            row["extractor_cpu_measured_on_utterances"] = n_cpu
            row["extractor_cpu_scaled"] = n_cpu != U
            row["ratio_cpu_over_kernel"] = row["extractor_cpu_ms"] / row["wsae_logmel"]["median_ms"]
            print(json.dumps(row), flush=True)
            rows.append(row)
            del frontend, out
    out_path = Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps({"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "rounds": args.rounds,
                                    "calls_per_window": args.calls, "results": rows}, indent=1) + "\n")


if __name__ == "__main__":
    main()
