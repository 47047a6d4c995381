"""Time ``wsae_clip_extract`` against what a user would otherwise run (profiles/audio_clips_note.md).

Cells, waveforms of 30 s (480000 samples) resident on the device:
  pcm     61440 clips (3072 features x 20) of 16000 samples from an int16 bank of 2048 utterances to int16 output,
          peak gain 0.95, no fade, the padded rows layout.
  float   the same from a float32 bank of 512 utterances to float32 output.
  events  the runs that ``RunTracker`` lists on the persistent synthetic code of tests/runs_oracle.py (128 utterances of 1500
          encoder frames, k = 32, H = 3072: about 10^6 events), each cut to 320 .. 16000 samples, int16 bank to int16
          output, clips packed end to end (the montage layout: a padded layout would be 30 GB).

Per cell, on the same tables:
  kernel  one ``wsae_clip_extract`` call into a preallocated output (both kernels; tables and workspace resident).
  torch   the torch formulation on the device, in chunks of ``--chunk`` clips: a padded advanced-index gather, ``abs().amax``,
          divide, multiply, round, clamp - the result left on the device in the padded layout.  Where its values can be
          compared (every cell a clip owns) the number of differing cells is recorded.
The two are timed in ALTERNATING windows (``--rounds`` x [``--calls`` kernel calls, one torch pass]), device events around
every window, after a warm-up of both.  Achieved bytes/s counts the bytes the task needs - every sample of a clip read once
and written once - against the 6.3 TB/s achievable HBM rate of MI355X_MICROARCH.md; the kernel itself reads the samples twice
(the second time from L2 / Infinity Cache where they stay), which the note says next to the figure.
  cpu     for ``--cpu-features`` (256) features of the pcm cell: the reference's per-clip arithmetic in torch on the host
          (slice, ``abs().max()``, divide, multiply; the float32 waveform of an utterance loaded once per feature that cites
          it - here: converted from the int16 bank's host copy), host clock.  Writing the files (``write_wav`` per clip) is
          timed separately on ``--files`` clips.

    python profiles/audio_clips_timing.py [--out outputs/audio_clips_timing.json]
"""

from __future__ import annotations

import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "whisper-sae_amd"), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import runs_oracle as RO  # noqa: E402
from whisper_sae import _native as N  # noqa: E402
from whisper_sae.analysis import RunTracker, clip_table_for_events, write_wav  # noqa: E402

S, HBM = 480000, 6.3e12
TARGET = 0.95


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


def torch_clips(bank, lengths, utt, start, count, max_count, pcm_out):
    """The torch formulation for one chunk -> (padded [c, max_count] output, n [c])."""
    ar = torch.arange(max_count, device=bank.device)
    first = start.clamp(min=0)
    n = torch.minimum(count.long().clamp(max=max_count), (lengths[utt.long()].long() - first).clamp(min=0))
    own = ar[None, :] < n[:, None]
    x = bank[utt.long()[:, None], (first[:, None] + ar[None, :]).clamp(max=bank.shape[1] - 1)]
    x = x.float() * 2.0 ** -15 if bank.dtype == torch.int16 else x
    x = torch.where(own, x, torch.zeros_like(x))
    m = x.abs().amax(1, keepdim=True)
    y = torch.where(m > 0, x / m * TARGET, x)
    if pcm_out:
        y = (y * 32767.0).round().clamp(-32768, 32767).to(torch.int16)
    return y, n


def run_cell(name, bank, lengths, utt, start, count, max_count, off, out_elems, pcm_out, args, padded_rows):
    dev = bank.device
    lib = N.lib()
    n_clips = utt.numel()
    out = torch.zeros(out_elems, dtype=torch.int16 if pcm_out else torch.float32, device=dev)
    out_len = torch.zeros(n_clips, dtype=torch.int32, device=dev)
    peak = torch.zeros(n_clips, dtype=torch.float32, device=dev)
    ws = torch.empty(lib.wsae_clip_workspace_bytes(n_clips, max_count), dtype=torch.uint8, device=dev)
    codes = {torch.float32: N.DT_F32, torch.int16: N.DT_I16}
    stream = torch.cuda.current_stream().cuda_stream

    def kernel():
        N.check(lib.wsae_clip_extract(bank.data_ptr(), codes[bank.dtype], bank.shape[0], bank.stride(0), lengths.data_ptr(), S, n_clips,
                                      utt.data_ptr(), start.data_ptr(), count.data_ptr(), max_count, off.data_ptr(), N.CLIP_GAIN_PEAK,
                                      TARGET, 0, out.data_ptr(), codes[out.dtype], out_elems, out_len.data_ptr(), peak.data_ptr(),
                                      ws.data_ptr(), ws.numel(), stream), "wsae_clip_extract")

    def baseline(keep=None):
        for c0 in range(0, n_clips, args.chunk):
            sl = slice(c0, min(c0 + args.chunk, n_clips))
            y, n = torch_clips(bank, lengths, utt[sl], start[sl], count[sl], max_count, pcm_out)
            if keep is not None:
                keep(c0, y, n)

    kernel()
    torch.cuda.synchronize()
    samples = int(out_len.clamp(min=0).sum().item())
    differing = [0, 0]

    def compare(c0, y, n):  # every cell a clip owns, against the kernel's output
        ar = torch.arange(max_count, device=dev)
        own = ar[None, :] < n[:, None]
        at = (off[c0:c0 + y.shape[0], None] + ar[None, :])[own]
        differing[0] += int((out[at] != y[own]).sum().item())
        differing[1] += int(own.sum().item())

    baseline(compare)
    row = {"cell": name, "clips": n_clips, "samples": samples, "bank": f"{bank.shape[0]} x {bank.shape[1]} {bank.dtype}",
           "output": str(out.dtype), "layout": "rows" if padded_rows else "packed",
           "cells_differing_from_torch": differing[0], "cells_compared": differing[1]}
    for _ in range(2):
        window_ms(kernel, args.calls)
        window_ms(baseline, 1)
    k_ms, t_ms = [], []
    for _ in range(args.rounds):
        k_ms.append(window_ms(kernel, args.calls))
        t_ms.append(window_ms(baseline, 1))
    row["wsae_clip_extract"], row["torch_on_device"] = summary(k_ms), summary(t_ms)
    row["ratio_torch_over_kernel"] = row["torch_on_device"]["median_ms"] / row["wsae_clip_extract"]["median_ms"]
    needed = samples * (bank.element_size() + out.element_size())
    seconds = row["wsae_clip_extract"]["median_ms"] * 1e-3
    row["needed_gb"] = needed * 1e-9
    row["achieved_tb_per_s_needed"] = needed / seconds * 1e-12
    row["share_of_achievable_hbm"] = needed / seconds / HBM
    row["moved_gb_with_second_read"] = (needed + samples * bank.element_size()) * 1e-9
    print(json.dumps(row), flush=True)
    return row, out, out_len


def fixed_table(n_utt, n_clips, seed, dev):
    g = torch.Generator().manual_seed(seed)
    lengths = torch.randint(S // 2, S + 1, (n_utt,), generator=g).to(torch.int32)
    utt = torch.randint(0, n_utt, (n_clips,), generator=g).to(torch.int32)
    position = (torch.rand(n_clips, generator=g) * (lengths[utt.long()] // 320)).long()  # an encoder frame of the utterance
    start = position * 320 - 8000  # half a second before it: negative near the start, cut near the end
    count = torch.full((n_clips,), 16000, dtype=torch.int32)
    off = torch.arange(n_clips, dtype=torch.int64) * 16000
    return [t.to(dev) for t in (lengths, utt, start, count, off)]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--chunk", type=int, default=4096)
    ap.add_argument("--features", type=int, default=3072)
    ap.add_argument("--event-utterances", type=int, default=128)
    ap.add_argument("--cpu-features", type=int, default=256)
    ap.add_argument("--files", type=int, default=512)
    ap.add_argument("--out", default=str(ROOT / "outputs" / "audio_clips_timing.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda", 0)
    n_clips = args.features * 20
    rows = []

    # ---- pcm ----
    bank = torch.randint(-32768, 32768, (2048, S), dtype=torch.int16, device=dev)
    lengths, utt, start, count, off = fixed_table(2048, n_clips, 1, dev)
    row, out, out_len = run_cell("pcm", bank, lengths, utt, start, count, 16000, off, n_clips * 16000, True, args, True)
    # the reference's arithmetic on the host for a subset of the features, and the files
    sub = min(args.cpu_features, args.features) * 20
    h_bank, h_len = bank.cpu(), lengths.cpu()
    h_utt, h_start = utt[:sub].cpu().tolist(), start[:sub].cpu().tolist()
    t0 = time.perf_counter()
    clips = []
    for f0 in range(0, sub, 20):
        cache = {}
        for c in range(f0, f0 + 20):
            u = h_utt[c]
            if u not in cache:  # the reference loads an utterance once per feature that cites it
                cache[u] = h_bank[u, :int(h_len[u])].float() * 2.0 ** -15
            audio = cache[u]
            lo = max(0, h_start[c])
            clip = audio[lo:min(len(audio), lo + 16000)]
            if clip.abs().max() > 0:
                clip = clip / clip.abs().max() * 0.95
            clips.append(clip)
    row["reference_arithmetic_cpu_ms"] = (time.perf_counter() - t0) * 1e3
    row["reference_arithmetic_cpu_clips"] = sub
    row["reference_arithmetic_cpu_ms_scaled_to_all"] = row["reference_arithmetic_cpu_ms"] * n_clips / sub
    host = out.view(n_clips, 16000)[:args.files].cpu().numpy()
    host_len = out_len[:args.files].cpu().numpy()
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        for c in range(len(host)):
            write_wav(Path(tmp) / f"{c}.wav", host[c, :host_len[c]], 16000)
        row["write_wav_ms_per_clip"] = (time.perf_counter() - t0) * 1e3 / len(host)
    t0 = time.perf_counter()
    out.cpu()
    row["copy_to_host_ms"] = (time.perf_counter() - t0) * 1e3
    kernel_pcm = np.stack([np.clip(np.rint(c.numpy() * np.float32(32767)), -32768, 32767).astype(np.int16)
                           for c in clips[:args.files] if len(c) == 16000])
    mine = np.stack([host[c] for c in range(min(args.files, sub)) if host_len[c] == 16000])
    row["cells_differing_from_reference_arithmetic"] = int((kernel_pcm != mine).sum())
    rows.append(row)
    del bank, out, h_bank, clips

    # ---- float ----
    bank = torch.rand(512, S, device=dev) * 2 - 1
    lengths, utt, start, count, off = fixed_table(512, n_clips, 2, dev)
    rows.append(run_cell("float", bank, lengths, utt, start, count, 16000, off, n_clips * 16000, False, args, True)[0])
    del bank

    # ---- events ----
    U, FR, K, H = args.event_utterances, 1500, 32, 3072
    code = RO.persistent_code(np.random.default_rng(H), U * FR, K, H)
    runs = RunTracker(H, max_events=12 * U * FR, device=dev)
    runs.update((torch.from_numpy(code[0]).to(dev).view(U, FR, K), torch.from_numpy(code[1]).to(dev).view(U, FR, K)))
    utt, start, count = clip_table_for_events(runs.events(), stride=2, max_samples=16000)
    del runs, code
    bank = torch.randint(-32768, 32768, (U, S), dtype=torch.int16, device=dev)
    lengths = torch.full((U,), S, dtype=torch.int32, device=dev)
    ends = torch.cumsum(count.long(), 0)
    off = (ends - count.long()).contiguous()
    row = run_cell("events", bank, lengths, utt.contiguous(), start.contiguous(), count.contiguous(), 16000, off, int(ends[-1].item()),
                   True, args, False)[0]
    row["count_min"], row["count_max"], row["count_mean"] = int(count.min()), int(count.max()), float(count.float().mean())
    rows.append(row)

    out_path = Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps({"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "rounds": args.rounds,
                                    "calls_per_window": args.calls, "torch_chunk": args.chunk, "results": rows}, indent=1) + "\n")


if __name__ == "__main__":
    main()
