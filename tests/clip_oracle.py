"""numpy restatement of the audio clip export (include/wsae.h, ``wsae_clip_extract``): float32
operations in the stated order, ``np.rint`` (round half to even) for the PCM conversion.

Bounds of clip c: u = clip_utt[c]; L = min(max(length[u], 0), max_length); s0 = max(clip_start[c], 0); count =
min(max(clip_count[c], 0), max_count); e = min(s0 + count, L); n = max(e - s0, 0).
Peak m = max |x_j| (0 for an empty clip).  GAIN_PEAK and m > 0: y = fl(fl(x / m) * target), else y = x.  fade F >= 1:
y = fl(y * fl(float(min(min(j, n - 1 - j) + 1, F)) / float(F))).  float32 output: y; int16 output: clamp(rint(fl(y * 32767)),
-32768, 32767), except that GAIN_NONE, F = 0, int16 in and int16 out copies the samples.
A clip with u outside [0, n_utt), clip_off < 0 or clip_off + n > out_elems writes nothing: out_len = -1, out_peak = 0.
"""

from __future__ import annotations

import numpy as np

from oracle import synth

GAIN_NONE, GAIN_PEAK = 0, 1
F32 = np.float32


def as_float(x: np.ndarray) -> np.ndarray:
    """int16 samples scaled by 2^-15 (exact), float32 as they are."""
    if x.dtype == np.int16:
        return x.astype(F32) * F32(2.0 ** -15)
    assert x.dtype == np.float32
    return x


def bounds(start: int, count: int, length: int, max_length: int, max_count: int):
    """(s0, n)."""
    L = min(max(int(length), 0), int(max_length))
    s0 = max(int(start), 0)
    cnt = min(max(int(count), 0), int(max_count))
    return s0, max(min(s0 + cnt, L) - s0, 0)


def fade_ramp(n: int, fade: int) -> np.ndarray:
    j = np.arange(n, dtype=np.int64)
    d = np.minimum(np.minimum(j, n - 1 - j) + 1, fade)
    return d.astype(F32) / F32(fade)


def clip_values(x: np.ndarray, gain_mode: int, target: float, fade: int, out_int16: bool):
    """``x``: the clip's n samples as stored (float32 or int16) -> (output values, peak)."""
    xf = as_float(x)
    m = F32(np.abs(xf).max()) if xf.size else F32(0)
    if out_int16 and x.dtype == np.int16 and gain_mode == GAIN_NONE and fade == 0:
        return x.copy(), m
    y = xf
    if gain_mode == GAIN_PEAK and m > 0:
        y = (xf / m).astype(F32) * F32(target)
    if fade >= 1:
        y = (y * fade_ramp(len(y), fade)).astype(F32)
    y = y.astype(F32)
    if out_int16:
        y = np.clip(np.rint((y * F32(32767)).astype(F32)), -32768, 32767).astype(np.int16)
    return y, m


def extract(x: np.ndarray, lengths, max_length: int, utt, start, count, max_count: int, off, gain_mode: int, target: float,
            fade: int, out: np.ndarray):
    """``x [n_utt, >= max_length]``; ``out``: the 1-D output buffer as it is before the call (its dtype is the output
    type).  Returns (out after the call, out_len int32, out_peak float32)."""
    out = out.copy()
    n_clips = len(utt)
    out_len = np.zeros(n_clips, np.int32)
    peak = np.zeros(n_clips, F32)
    for c in range(n_clips):
        u = int(utt[c])
        if not 0 <= u < x.shape[0]:
            out_len[c] = -1
            continue
        s0, n = bounds(start[c], count[c], lengths[u], max_length, max_count)
        o = int(off[c])
        if o < 0 or o + n > out.size:
            out_len[c] = -1
            continue
        y, m = clip_values(x[u, s0:s0 + n], gain_mode, target, fade, out.dtype == np.int16)
        out[o:o + n] = y
        out_len[c], peak[c] = n, m
    return out, out_len, peak


# ---- the waveforms behind tests/golden/g20_* (the generator and the tests build them from here; only outputs are stored) ----
GOLDEN_LENGTHS = (4000, 3000, 2500)
GOLDEN_SILENCE = (1, 800, 2400)  # utterance 1 is zero on [800, 2400)


def golden_waveform(u: int) -> np.ndarray:
    """Utterance ``u`` of the G20 goldens: 16-bit values from the counter generator, as float32 in [-1, 1)."""
    pcm = (synth.counter_u64(GOLDEN_LENGTHS[u], 20, u) >> np.uint64(48)).astype(np.int64) - 32768
    wave = pcm.astype(np.int16).astype(F32) * F32(2.0 ** -15)
    if u == GOLDEN_SILENCE[0]:
        wave[GOLDEN_SILENCE[1]:GOLDEN_SILENCE[2]] = 0
    return wave
