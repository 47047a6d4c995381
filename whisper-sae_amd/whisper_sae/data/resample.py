"""Resampling on the device: waveforms at any rate and channel count in, mono at 16 kHz out.

``Resampler`` holds the polyphase tap table of ``wsae_resample`` and turns a batch of interleaved waveforms (float32 or 16-bit
PCM) into mono waveforms at the new rate.  The filter is torchaudio's default (``sinc_interp_hann``, ``lowpass_filter_width
= 6``, ``rolloff = 0.99``), the one the reference's ``LibriSpeechDataset`` runs; nothing of torchaudio is imported.  The
arithmetic is fixed operation by operation in ``include/wsae.h``; ``tests/resample_oracle.py`` restates it in numpy.
``AudioFrontEnd`` is the composition ``LogMel()(*Resampler(rate)(x, lengths))``.  There is no CPU path.
"""

from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from .. import _native as N
from .._device import gpu_device
from .audio import N_SAMPLES, SAMPLE_RATE, LogMel
from .waveforms import _DTYPES, head, head_device, pack_waveforms


def _reduced(orig_freq, new_freq) -> Tuple[int, int]:
    if int(orig_freq) != orig_freq or int(new_freq) != new_freq or orig_freq < 1 or new_freq < 1:
        raise ValueError(f"the rates must be positive integers, got {orig_freq} and {new_freq}")
    g = math.gcd(int(orig_freq), int(new_freq))
    return int(orig_freq) // g, int(new_freq) // g


def sinc_resample_kernel(orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99
                         ) -> Tuple[np.ndarray, int]:
    """``(kernel float64 [new, 2 width + orig], width)`` with ``orig``, ``new`` the rates divided by their gcd: torchaudio's
    ``_get_sinc_resample_kernel`` for the Hann window, in numpy float64.  Output ``i new + p`` of the resampler is
    ``sum_n kernel[p][n] xpad[i orig + n]`` with ``xpad[m] = x[m - width]``."""
    orig, new = _reduced(orig_freq, new_freq)
    if lowpass_filter_width < 1:
        raise ValueError(f"lowpass_filter_width must be positive, got {lowpass_filter_width}")
    if not 0.0 < rolloff <= 1.0:
        raise ValueError(f"rolloff must lie in (0, 1], got {rolloff}")
    base = min(orig, new) * float(rolloff)
    width = int(math.ceil(lowpass_filter_width * orig / base))
    idx = np.arange(-width, width + orig, dtype=np.float64) / orig
    t = (np.arange(0, -new, -1, dtype=np.float64)[:, None] / new + idx[None, :]) * base
    t = np.clip(t, -lowpass_filter_width, lowpass_filter_width)
    window = np.cos(t * np.pi / lowpass_filter_width / 2) ** 2
    t = t * np.pi
    with np.errstate(invalid="ignore", divide="ignore"):
        kernel = np.where(t == 0, 1.0, np.sin(t) / t)
    kernel *= window * (base / orig)
    return kernel, width


def compact_taps(kernel: np.ndarray, width: int) -> Tuple[np.ndarray, np.ndarray, int]:
    """``(taps float32 [new, W], first int32 [new], halo)``: the kernel rounded to float32 once, each phase cut to the span
    from its first to its last nonzero tap; ``W`` is the longest span, a shorter one slides so that it stays inside the kernel
    and keeps the zeros that are there.  ``first[p] = lo[p] - width`` is the input frame, relative to ``i orig``, that tap 0
    of phase ``p`` multiplies; ``halo = width`` bounds ``-first[p]`` and ``first[p] + W - orig``."""
    k32 = np.asarray(kernel).astype(np.float32)
    new, K = k32.shape
    lo, hi = np.zeros(new, np.int64), np.zeros(new, np.int64)
    for p in range(new):
        nz = np.flatnonzero(k32[p])
        if nz.size:
            lo[p], hi[p] = nz[0], nz[-1]
    W = int((hi - lo).max()) + 1
    lo = np.minimum(lo, K - W)
    taps = np.stack([k32[p, lo[p]:lo[p] + W] for p in range(new)])
    return np.ascontiguousarray(taps), (lo - int(width)).astype(np.int32), int(width)


def resampled_length(n: int, orig_freq: int, new_freq: int = SAMPLE_RATE) -> int:
    """``ceil(new n / orig)``: the samples ``n`` input frames become (torchaudio's ``target_length``)."""
    orig, new = _reduced(orig_freq, new_freq)
    if n < 0:
        raise ValueError(f"n must not be negative, got {n}")
    return -((-new * int(n)) // orig)


class Resampler:
    """``Resampler(orig_freq)(waveforms, lengths) -> (y [n_utt, out_cols], out_lengths int32 [n_utt])`` on ``device``.

    The tables go to the device once.  Equal rates give the identity table and still run the kernel, for the downmix and the
    dtype conversion."""

    def __init__(self, orig_freq: int, new_freq: int = SAMPLE_RATE, device="cuda", lowpass_filter_width: int = 6,
                 rolloff: float = 0.99):
        self.orig, self.new = _reduced(orig_freq, new_freq)
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        if max(self.orig, self.new) > N.RESAMPLE_MAX_RATE:
            raise ValueError(f"{orig_freq} -> {new_freq} reduces to {self.orig} / {self.new}: both must be at most {N.RESAMPLE_MAX_RATE}")
        if self.orig == self.new:
            taps, first, halo = np.ones((1, 1), np.float32), np.zeros(1, np.int32), 0
        else:
            taps, first, halo = compact_taps(*sinc_resample_kernel(self.orig, self.new, lowpass_filter_width, rolloff))
        if taps.shape[1] > N.RESAMPLE_MAX_TAPS or halo > N.RESAMPLE_MAX_HALO:
            raise ValueError(f"{orig_freq} -> {new_freq} needs {taps.shape[1]} taps per phase and a halo of {halo}: at most "
                             f"{N.RESAMPLE_MAX_TAPS} and {N.RESAMPLE_MAX_HALO} are served")
        self.device = gpu_device("Resampler", device)
        self.n_taps, self.halo = int(taps.shape[1]), int(halo)
        self.taps = torch.from_numpy(taps).to(self.device).contiguous()
        self.first = torch.from_numpy(first).to(self.device).contiguous()

    def out_cols(self, samples: int) -> int:
        return -((-self.new * int(samples)) // self.orig)

    def __call__(self, waveforms: Union[Tensor, Sequence[Tensor]], lengths=None, *, out: Optional[Tensor] = None,
                 out_dtype: Optional[torch.dtype] = None) -> Tuple[Tensor, Tensor]:
        """``waveforms``: ``[n_utt, S]`` (mono), ``[n_utt, S, C]`` (interleaved channels) or a list of 1-D / ``[S_i, C]``
        tensors, float32 or int16 (scaled by 2^-15), on the device.  ``lengths [n_utt]``: the valid frames (default ``S``;
        values above ``S`` are clamped to it).  ``out``: a float32 or int16 ``[n_utt, ceil(new S / orig)]`` tensor (or view
        with unit stride along the samples) to write into; ``out_dtype`` (default float32) where there is none.  The result
        is ``(y, out_lengths)``: ``y`` is zero from ``out_lengths[u]`` on; int16 is ``rint(y * 32768)``, saturated."""
        x, lengths, n_utt, s, c = pack_waveforms("Resampler", waveforms, lengths, self.device, channels=True, keep_empty=True)
        shape = (n_utt, self.out_cols(s))
        if out is None:
            out_dtype = torch.float32 if out_dtype is None else out_dtype
            if out_dtype not in _DTYPES:
                raise ValueError(f"out_dtype must be float32 or int16, got {out_dtype}")
            out = torch.empty(shape, dtype=out_dtype, device=self.device)
        else:
            if not isinstance(out, Tensor):
                raise ValueError("out must be a tensor")
            if tuple(out.shape) != shape or out.dtype not in _DTYPES or out_dtype not in (None, out.dtype):
                raise ValueError(f"out must be {'float32 or int16' if out_dtype is None else out_dtype} {list(shape)}, got "
                                 f"{out.dtype} {list(out.shape)}")
            if out.device != self.device:
                raise ValueError(f"out is on {out.device}, this Resampler on {self.device}")
            if shape[1] > 1 and out.stride(1) != 1 or (n_utt > 1 and out.stride(0) < shape[1]):
                raise ValueError(f"out needs unit stride along the samples and rows that do not overlap, got strides {out.stride()}")
        if n_utt == 0 or shape[1] == 0:
            return out, torch.zeros(n_utt, dtype=torch.int32, device=self.device)
        out_len = torch.empty(n_utt, dtype=torch.int32, device=self.device)
        ld_x = x.stride(0) if n_utt > 1 else max(x.stride(0), s * c)
        ld_y = out.stride(0) if n_utt > 1 else max(out.stride(0), shape[1])
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            N.check(N.lib().wsae_resample(x.data_ptr(), _DTYPES[x.dtype], n_utt, ld_x, c, lengths.data_ptr(), s, self.orig, self.new,
                                          self.taps.data_ptr(), self.first.data_ptr(), self.n_taps, self.halo, out.data_ptr(),
                                          _DTYPES[out.dtype], ld_y, shape[1], out_len.data_ptr(), stream), "wsae_resample")
        return out, out_len


def resample(waveforms, orig_freq: int, new_freq: int = SAMPLE_RATE, lengths=None, *, device=None, lowpass_filter_width: int = 6,
             rolloff: float = 0.99, **kw):
    """One-shot ``Resampler(orig_freq, new_freq, device, ...)(waveforms, lengths, **kw)``; ``device`` defaults to that of the
    waveforms.  Build a ``Resampler`` once where more than one batch is converted: it keeps the tables on the device."""
    return Resampler(orig_freq, new_freq, head_device(waveforms) if device is None else device, lowpass_filter_width, rolloff)(waveforms, lengths, **kw)


class AudioFrontEnd:
    """``AudioFrontEnd(sample_rate)(waveforms, lengths)`` = ``LogMel(n_mels)(*Resampler(sample_rate)(waveforms, lengths))``:
    waveforms at ``sample_rate`` with any channel count in, Whisper's ``input_features`` out.  Mono input at 16 kHz goes to the
    ``LogMel`` directly.  It has ``LogMel``'s call signature and is accepted wherever ``frontend=`` is; a 3-D tensor is a
    batch of interleaved waveforms ``[n_utt, S, C]`` when its last axis has at most 8 entries (``is_waveform``)."""

    def __init__(self, sample_rate: int, n_mels: int = 80, device="cuda", n_samples: int = N_SAMPLES, filters=None, basis=None,
                 lowpass_filter_width: int = 6, rolloff: float = 0.99):
        self.logmel = LogMel(n_mels, device, n_samples, filters, basis)
        self.resampler = Resampler(sample_rate, SAMPLE_RATE, self.logmel.device, lowpass_filter_width, rolloff)
        self.sample_rate, self.device = int(sample_rate), self.logmel.device
        self.n_mels, self.n_samples, self.frames = self.logmel.n_mels, self.logmel.n_samples, self.logmel.frames

    @staticmethod
    def is_waveform(t) -> bool:
        return isinstance(t, Tensor) and (t.dim() == 2 or (t.dim() == 3 and t.shape[2] <= N.RESAMPLE_MAX_CHANNELS))

    def __call__(self, waveforms, lengths=None, *, out: Optional[Tensor] = None, return_power: bool = False):
        first = head(waveforms)
        mono = isinstance(first, Tensor) and first.dim() == (1 if isinstance(waveforms, (list, tuple)) else 2)
        if not (mono and self.resampler.orig == self.resampler.new):
            waveforms, lengths = self.resampler(waveforms, lengths)
        return self.logmel(waveforms, lengths, out=out, return_power=return_power)


__all__ = ["AudioFrontEnd", "Resampler", "compact_taps", "resample", "resampled_length", "sinc_resample_kernel"]
