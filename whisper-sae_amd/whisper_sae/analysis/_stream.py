"""What the analysis trackers share: the checks on a compact ``(values, indices)`` code, the
segment id of every frame, the feature window, the workspace, the eval-mode scaffold of the ``collect_*`` functions and
the ranking of the ``top_*_features`` functions.  Plain functions; every tracker keeps its own state and numbering."""

from __future__ import annotations

from contextlib import contextmanager
from typing import Optional, Tuple

import torch
from torch import Tensor

from .. import _native as N
from ..sae.engine import require_device_tensor


def need_gpu(what: str, dev: Optional[torch.device]) -> torch.device:
    if dev is None:
        if not torch.cuda.is_available():
            raise N.WsaeError(f"{what} needs a GPU: its kernels run on the device and there is no CPU implementation")
        dev = torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise N.WsaeError(f"{what} cannot run on '{dev}': its kernels run on the GPU only")
    N.lib()  # fail loudly when the HIP library is not built
    return dev


def feature_window(window, hidden: int, name: str = "f_window") -> Tuple[int, int]:
    """``(lo, cols)`` of ``window`` (None: all ``hidden`` features); ``ValueError`` unless it lies inside them."""
    lo, cols = (0, hidden) if window is None else (int(window[0]), int(window[1]))
    if lo < 0 or cols < 1 or lo + cols > hidden:
        raise ValueError(f"{name} {window} is outside [0, {hidden})")
    return lo, cols


def compact_code(code, what: str, max_k: int, dims: Optional[Tuple[int, ...]] = (2, 3), also=()):
    """``(values, indices, k)`` of a code after the checks that need no tracker state, in this order: a pair
    (``TypeError``), device tensors (``WsaeError``; ``also``: further ``(tensor, name)`` to check with them), one shape of
    ``dims`` dimensions (None: any leading shape) and ``1 <= k <= max_k`` (``ValueError``)."""
    if not (isinstance(code, (tuple, list)) and len(code) == 2):
        raise TypeError(f"{what} must be a (values, indices) pair")
    vals, idx = code
    require_device_tensor(vals, f"{what} values")
    require_device_tensor(idx, f"{what} indices")
    for t, name in also:
        require_device_tensor(t, name)
    if vals.shape != idx.shape or (vals.dim() < 1 if dims is None else vals.dim() not in dims):
        want = "differ in shape" if dims is None else "must share a [n_utt, T, k] or [rows, k] shape"
        raise ValueError(f"{what}: values {tuple(vals.shape)} and indices {tuple(idx.shape)} {want}")
    k = vals.shape[-1]
    if not 1 <= k <= max_k:
        raise ValueError(f"{what}: k must be in 1..{max_k}, got {k}")
    return vals, idx, k


def flat_code(vals: Tensor, idx: Tensor, k: int) -> Tuple[Tensor, Tensor]:
    """Contiguous ``[rows, k]`` float32 / int32."""
    return (vals.detach().reshape(-1, k).to(torch.float32).contiguous(),
            idx.detach().reshape(-1, k).to(torch.int32).contiguous())


def frame_segments(vals: Tensor, segments: Optional[Tensor], frame_mask: Optional[Tensor], dev, first: int = 0):
    """The segment id of every frame, int32 ``[rows]``, and the utterances of a ``[n_utt, T, k]`` code, which are
    numbered ``first, first + 1, ...`` (None for a flat ``[rows, k]`` code, whose ids are ``segments``).  A frame with
    ``frame_mask == 0`` gets -1."""
    if vals.dim() == 3:
        if segments is not None:
            raise ValueError("a [n_utt, T, k] code numbers its utterances itself: pass segments only with a flat code")
        n_utt, T = vals.shape[0], vals.shape[1]
        seg = torch.arange(first, first + n_utt, dtype=torch.int32, device=dev)[:, None].expand(n_utt, T).reshape(-1)
    else:
        if segments is None:
            raise ValueError("a flat [rows, k] code needs segments [rows]")
        require_device_tensor(segments, "segments")
        if segments.numel() != vals.shape[0]:
            raise ValueError(f"segments has {segments.numel()} ids for {vals.shape[0]} rows")
        n_utt, seg = None, segments.detach().reshape(-1).to(device=dev, dtype=torch.int32)
    if frame_mask is not None:
        require_device_tensor(frame_mask, "frame_mask")
        if frame_mask.numel() != seg.shape[0]:
            raise ValueError(f"frame_mask has {frame_mask.numel()} flags for {seg.shape[0]} frames")
        seg = torch.where(frame_mask.detach().reshape(-1).to(dev) != 0, seg, torch.full_like(seg, -1))
    return seg.contiguous(), n_utt


def take_form(tracker, vals: Tensor, why: str = "") -> str:
    """"numbered" for a ``[n_utt, T, k]`` code, "flat" otherwise; ``ValueError`` when ``tracker._form`` is the other."""
    form = "numbered" if vals.dim() == 3 else "flat"
    if tracker._form not in (None, form):
        raise ValueError(f"this tracker has taken {tracker._form} updates: [n_utt, T, k] codes and flat codes with segments "
                         f"{why}cannot be mixed")
    return form


def grow(tracker, elems: int, dtype, dev) -> Tensor:
    """``tracker._ws`` with at least ``elems`` elements of ``dtype``."""
    if tracker._ws is None or tracker._ws.numel() < elems:
        tracker._ws = None  # (release before the larger one is taken)
        tracker._ws = torch.empty(elems, dtype=dtype, device=dev)
    return tracker._ws


@contextmanager
def encoding(*models, hint: str):
    """The scaffold of a ``collect_*`` function: every module must offer ``encode_compact`` (``TypeError`` with the
    caller's ``hint``) and runs in eval mode under ``no_grad``; its previous mode is restored."""
    for m in models:
        if not hasattr(m, "encode_compact"):
            raise TypeError(f"{type(m).__name__} has no compact code (encode_compact): {hint}")
    modes = [m.training for m in models]
    for m in models:
        m.eval()
    try:
        with torch.no_grad():
            yield
    finally:
        for m, mode in zip(models, modes):
            m.train(mode)


def utterance_code(model, x: Tensor, device) -> Tuple[Tensor, Tensor]:
    """The compact code of ``x [n_utt, T, D]`` as ``[n_utt, T, k]``."""
    vals, idx = model.encode_compact(x.to(device))
    shape = (x.shape[0], x.shape[1], vals.shape[-1])
    return vals.reshape(shape), idx.reshape(shape)


def rank_features(score: Tensor, ok: Tensor, n: int) -> Tensor:
    """The indices of the ``n`` largest ``score`` among the candidates ``ok``, descending, ties to the lower index;
    fewer than ``n`` when fewer candidates exist."""
    key = torch.where(ok, score, torch.full_like(score, float("-inf")))
    order = torch.argsort(key, descending=True, stable=True)[:max(int(n), 0)]
    return order[ok[order]]
