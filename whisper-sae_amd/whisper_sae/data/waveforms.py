"""The bank of waveforms the audio kernels read (``LogMel``, ``Resampler``, ``WaveformBank``): ragged rows or a padded tensor
in, one zero-padded tensor with unit-stride rows and its int32 lengths on the device out."""

from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from .. import _native as N
from .._device import gpu_device, need_gpu

_DTYPES = {torch.float32: N.DT_F32, torch.int16: N.DT_I16}


def head(waveforms):
    """The first row of a list of waveforms, else ``waveforms`` itself."""
    return waveforms[0] if isinstance(waveforms, (list, tuple)) and waveforms else waveforms


def head_device(waveforms):
    """The device of the first waveform; ``"cuda"`` where there is no tensor to ask."""
    first = head(waveforms)
    return first.device if isinstance(first, Tensor) else "cuda"


def _shape(t) -> str:
    return str(tuple(t.shape)) if isinstance(t, Tensor) else type(t).__name__


def pack_waveforms(what: str, waveforms, lengths, device, *, channels: bool = False, host: bool = False,
                   keep_empty: bool = False, contiguous: bool = False, max_samples: Optional[int] = None
                   ) -> Tuple[Tensor, Tensor, int, int, int]:
    """``(bank, lengths int32 [n_utt] on the device, n_utt, S, C)`` of ``[n_utt, S]`` waveforms or a list of 1-D rows, for
    the object ``what`` names in the messages.

    ``channels``: ``[n_utt, S, C]`` and rows ``[S_i, C]`` of interleaved frames are taken too, ``1 <= C <=
    RESAMPLE_MAX_CHANNELS``.  ``host``: CPU tensors are moved to ``device``, and shape, dtype and the number of lengths are
    checked before a GPU is asked for; without it every tensor must be on the GPU (``WsaeError``) and on ``device``, a
    resolved one.  ``keep_empty``: ``S == 0`` stays; otherwise it becomes one column of zeros with all lengths 0 (nothing
    else gives the kernel an address).  ``contiguous``: the bank is made contiguous; otherwise it is copied only where its
    frames are not interleaved at unit stride or its rows overlap.  ``max_samples``: the largest ``S``."""
    ranks = (1, 2) if channels else (1,)
    listed = isinstance(waveforms, (list, tuple))
    if listed:
        if lengths is not None:
            raise ValueError("lengths come from the waveforms themselves when a list is given")
        if not waveforms:
            raise ValueError("the list of waveforms is empty")
        for i, w in enumerate(waveforms):
            if not isinstance(w, Tensor) or w.dim() not in ranks:
                raise ValueError(f"waveform {i} must be a {'1-D or [samples, channels]' if channels else '1-D'} tensor, got {_shape(w)}")
            if w.dtype != waveforms[0].dtype:
                raise ValueError(f"waveform {i} is {w.dtype}, waveform 0 is {waveforms[0].dtype}")
            if w.shape[1:] != waveforms[0].shape[1:]:
                raise ValueError(f"waveform {i} is {tuple(w.shape)}, waveform 0 is {tuple(waveforms[0].shape)}: the channels differ")
            if not host:
                need_gpu(what, w.device)
    elif not isinstance(waveforms, Tensor) or waveforms.dim() - 1 not in ranks:
        forms = ("[n_utt, samples], [n_utt, samples, channels] or a list of such rows" if channels
                 else "[n_utt, samples] or a list of 1-D tensors")
        raise ValueError(f"waveforms must be {forms}, got {_shape(waveforms)}")
    dtype = head(waveforms).dtype
    if host:
        if dtype not in _DTYPES:
            raise ValueError(f"waveforms must be float32 or int16, got {dtype}")
        if not listed and lengths is not None and torch.as_tensor(lengths).numel() != waveforms.shape[0]:
            raise ValueError(f"lengths has {torch.as_tensor(lengths).numel()} entries for {waveforms.shape[0]} utterances")
        device = gpu_device(what, device)
    if listed:
        sizes = [int(w.shape[0]) for w in waveforms]
        packed = torch.zeros((len(sizes), max(max(sizes), 0 if keep_empty else 1)) + tuple(waveforms[0].shape[1:]), dtype=dtype,
                             device=device)
        for i, w in enumerate(waveforms):
            packed[i, :sizes[i]] = w
        waveforms, lengths = packed, torch.tensor(sizes, dtype=torch.int32)
    if host:
        waveforms = waveforms.to(device)
    else:
        need_gpu(what, waveforms.device)
        if waveforms.device != device:
            raise ValueError(f"waveforms are on {waveforms.device}, this {what} on {device}")
        if dtype not in _DTYPES:
            raise ValueError(f"waveforms must be float32 or int16, got {dtype}")
    n_utt, s = waveforms.shape[:2]
    c = waveforms.shape[2] if waveforms.dim() == 3 else 1
    if not 1 <= c <= N.RESAMPLE_MAX_CHANNELS:
        raise ValueError(f"waveforms have {c} channels, 1 to {N.RESAMPLE_MAX_CHANNELS} are served")
    if s == 0 and not keep_empty:
        waveforms, lengths, s = waveforms.new_zeros((n_utt, 1) + tuple(waveforms.shape[2:])), torch.zeros(n_utt, dtype=torch.int32), 1
    if max_samples is not None and s > max_samples:
        raise ValueError(f"waveforms have {s} samples, this {what} takes at most n_samples = {max_samples}")
    if lengths is None:
        lengths = torch.full((n_utt,), s, dtype=torch.int32, device=device)
    else:
        lengths = torch.as_tensor(lengths).reshape(-1)
        if lengths.numel() != n_utt:
            raise ValueError(f"lengths has {lengths.numel()} entries for {n_utt} utterances")
        lengths = lengths.to(device=device, dtype=torch.int32).contiguous()
    x = waveforms if waveforms.dim() == 3 else waveforms.unsqueeze(2)
    if contiguous or not ((c == 1 or x.stride(2) == 1) and (s <= 1 or x.stride(1) == c) and (n_utt <= 1 or x.stride(0) >= s * c)):
        waveforms = waveforms.contiguous()  # (frames interleaved, rows that do not overlap)
    return waveforms, lengths, int(n_utt), int(s), int(c)
