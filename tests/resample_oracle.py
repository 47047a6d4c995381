"""numpy oracles of the resampler (include/wsae.h, ``wsae_resample``).

``fma32`` is a correctly rounded float32 fused multiply-add; ``resample_exact`` is the contract, operation by operation, and
reproduces the kernel's bits; ``resample_ideal`` is the dense float64 formulation that torchaudio computes."""

from __future__ import annotations

import math

import numpy as np

from whisper_sae.data import sinc_resample_kernel


def fma32(a, b, c) -> np.ndarray:
    """``fl32(a * b + c)`` with one rounding, elementwise on float32 arrays.

    The product of two float32 is exact in float64.  TwoSum gives the rounding error of the float64 sum; where it is nonzero
    and the sum's last bit is even, the sum moves one ulp towards the error: that is the sum rounded to odd, and rounding an
    odd-rounded float64 to float32 is the same as rounding the exact value once (it takes two extra bits; there are 29)."""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (np.asarray(s).view(np.int64) & 1) == 0
    odd = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
    return np.where((err != 0) & even, odd, s).astype(np.float32)


def downmix(x: np.ndarray, channels: int) -> np.ndarray:
    """Interleaved frames ``[L * channels]`` (float32, or int16 scaled by 2^-15) -> mono float32 ``[L]``: the channels
    summed in their order, one IEEE division."""
    x = np.asarray(x)
    f = x.astype(np.float32) * np.float32(2.0 ** -15) if x.dtype == np.int16 else x.astype(np.float32)
    f = f.reshape(-1, channels)
    s = f[:, 0].copy()
    if channels == 1:
        return s
    for c in range(1, channels):
        s = s + f[:, c]
    return s / np.float32(channels)


def resample_exact(x, channels: int, length: int, orig: int, new: int, taps32: np.ndarray, first: np.ndarray, out_dtype):
    """One utterance by the contract: ``x`` holds at least ``length * channels`` interleaved elements.  Returns ``y`` of
    ``out_len = ceil(new * length / orig)`` cells, float32 or (``out_dtype = np.int16``) ``clamp(rint(y * 32768))``."""
    taps32 = np.asarray(taps32, dtype=np.float32)
    first = np.asarray(first, dtype=np.int64)
    L = max(int(length), 0)
    mono = downmix(np.asarray(x).reshape(-1)[:L * channels], channels)
    out_len = -((-new * L) // orig)
    j = np.arange(out_len, dtype=np.int64)
    i, p = j // new, j % new
    acc = np.zeros(out_len, dtype=np.float32)
    base = i * orig + first[p]
    for w in range(taps32.shape[1]):
        m = base + w
        inside = (m >= 0) & (m < L)
        xz = np.where(inside, mono[np.clip(m, 0, max(L - 1, 0))] if L else np.float32(0), np.float32(0)).astype(np.float32)
        acc = fma32(xz, taps32[p, w], acc)
    if np.dtype(out_dtype) == np.int16:
        return np.clip(np.rint(acc * np.float32(32768)), -32768, 32767).astype(np.int16)
    return acc


def dense_apply(kernel: np.ndarray, width: int, x: np.ndarray, orig: int, new: int) -> np.ndarray:
    """``y[i new + p] = sum_n kernel[p][n] xpad[i orig + n]``, ``xpad[m] = x[m - width]``, in float64, ``ceil(new len(x) /
    orig)`` cells."""
    kernel = np.asarray(kernel, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    K = kernel.shape[1]
    n_out = -((-new * x.size) // orig)
    blocks = -(-n_out // new)
    xpad = np.concatenate((np.zeros(width), x, np.zeros(blocks * orig + K)))
    idx = (np.arange(blocks) * orig)[:, None] + np.arange(K)[None, :]
    return (xpad[idx] @ kernel.T).reshape(-1)[:n_out]


def resample_ideal(x, orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99) -> np.ndarray:
    """Mono ``x`` through the dense float64 kernel: what ``torchaudio.transforms.Resample(orig_freq, new_freq)`` computes."""
    g = math.gcd(int(orig_freq), int(new_freq))
    kernel, width = sinc_resample_kernel(orig_freq, new_freq, lowpass_filter_width, rolloff)
    return dense_apply(kernel, width, x, int(orig_freq) // g, int(new_freq) // g)
