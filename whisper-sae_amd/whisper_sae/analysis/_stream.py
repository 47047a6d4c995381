"""What the analysis trackers share: the checks on a compact ``(values, indices)`` code, the
segment id of every frame, the feature window, the column map of a feature subset, the labels and the lag of a frame, the
row bound of an int32 state, the workspace, the transposed plan, the ``_state``-dict lifecycle, the batch iterators and the
eval-mode scaffold of the ``collect_*`` functions, and the rankings of the ``top_*`` functions and the curves.  Plain
functions; every tracker keeps its own state and numbering."""

from __future__ import annotations

from contextlib import contextmanager
from typing import Optional, Tuple

import torch
from torch import Tensor

from .. import _native as N
from .._device import grow, need_gpu, workspace  # noqa: F401  (the trackers take them from here)
from ..sae.engine import require_device_tensor

MAX_ROWS = 2 ** 31 - 1  # the int32 range: the rows of one call, and the frames an int32 state counts in all


def feature_window(window, hidden: int, name: str = "f_window") -> Tuple[int, int]:
    """``(lo, cols)`` of ``window`` (None: all ``hidden`` features); ``ValueError`` unless it lies inside them."""
    lo, cols = (0, hidden) if window is None else (int(window[0]), int(window[1]))
    if lo < 0 or cols < 1 or lo + cols > hidden:
        raise ValueError(f"{name} {window} is outside [0, {hidden})")
    return lo, cols


def check_lag(lag) -> None:
    if not -1024 <= int(lag) <= 1024:
        raise ValueError(f"lag must be in -1024..1024, got {lag}")


def check_index(c, count: int, what: str) -> int:
    """``int(c)`` of a class or target number; ``ValueError`` outside ``[0, count)``."""
    if not 0 <= int(c) < count:
        raise ValueError(f"{what} {c} is outside [0, {count})")
    return int(c)


def column_table(feats: Tensor, hidden: int) -> Tensor:
    """int32 ``[hidden]`` on the CPU: the position of every feature in ``feats`` (int64, in range), -1 elsewhere."""
    col_of = torch.full((hidden,), -1, dtype=torch.int32)
    col_of[feats] = torch.arange(feats.numel(), dtype=torch.int32)
    return col_of


def column_map(features, hidden: int) -> Tuple[Tensor, Optional[Tensor]]:
    """``(feature_index int64, col_of int32 or None)`` on the CPU after the checks on ``features`` (None: all ``hidden``
    features, which need no table)."""
    if features is None:
        return torch.arange(hidden, dtype=torch.int64), None
    feats = torch.as_tensor(features)
    if feats.dim() != 1 or feats.numel() < 1 or feats.is_floating_point() or feats.dtype == torch.bool:
        raise ValueError(f"features must be a 1-D tensor of at least one index, got {tuple(feats.shape)} {feats.dtype}")
    feats = feats.detach().cpu().to(torch.int64)
    if int(feats.min()) < 0 or int(feats.max()) >= hidden:
        raise ValueError(f"features must lie in [0, {hidden})")
    if torch.unique(feats).numel() != feats.numel():
        raise ValueError("features holds an index twice")
    return feats, column_table(feats, hidden)


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


def check_frame_labels(vals: Tensor, labels: Tensor) -> None:
    if labels.shape != vals.shape[:-1] or labels.is_floating_point() or labels.dtype == torch.bool:
        raise ValueError(f"labels must hold one integer per frame, in the shape {tuple(vals.shape[:-1])} of the code's "
                         f"frames: got {tuple(labels.shape)} {labels.dtype}")


def frame_labels(vals: Tensor, labels: Tensor, n_classes: int) -> Tensor:
    """int32 ``[rows]``: the label of every frame of the code, -1 where it lies outside ``[0, n_classes)``."""
    check_frame_labels(vals, labels)
    lab = labels.detach().reshape(-1).to(torch.int64)  # (labels beyond int32 are outside every [0, n_classes))
    return torch.where((lab >= 0) & (lab < n_classes), lab, torch.full_like(lab, -1)).to(torch.int32).contiguous()


def check_row_bound(tracker, more: int, merging: bool = False) -> None:
    """``WsaeError`` when ``tracker._submitted + more`` frames leave the int32 range of the tracker's counts; the message
    of ``update``, or (``merging``) of ``merge``."""
    if tracker._submitted + more > MAX_ROWS:
        name, tail = (".merge", "") if merging else ("", ", the range of the int32 state")
        raise N.WsaeError(f"{type(tracker).__name__}{name}: {tracker._submitted} + {more} frames exceed {MAX_ROWS}{tail}")


def take_form(tracker, vals: Tensor, why: str = "") -> str:
    """"numbered" for a ``[n_utt, T, k]`` code, "flat" otherwise; ``ValueError`` when ``tracker._form`` is the other."""
    form = "numbered" if vals.dim() == 3 else "flat"
    if tracker._form not in (None, form):
        raise ValueError(f"this tracker has taken {tracker._form} updates: [n_utt, T, k] codes and flat codes with segments "
                         f"{why}cannot be mixed")
    return form


def transposed_plan(tracker, v: Tensor, i: Tensor, k: int, seg: Tensor, rows: int):
    """``(col_ptr int64 [n_cols + 1], t_row int32, t_val float32, nnz)``: the flat code transposed by ``wsae_probe_plan``
    over the tracker's columns (``hidden``, ``n_cols``, ``_col_of``) - per column the rows on which it fires and its
    values there.  The lists hold ``nnz`` entries at least: their size is a guess first, and where the plan counts more
    entries than that, it is transposed once more at the true count.  One read of ``nnz`` from the device per pass."""
    dev, lib, P = v.device, N.lib(), tracker.n_cols
    col_ptr = torch.empty(P + 1, dtype=torch.int64, device=dev)
    nnz = torch.zeros(1, dtype=torch.int64, device=dev)
    need = lib.wsae_probe_plan_workspace_bytes(rows, k, tracker.hidden, P)
    if need < 0:
        raise N.WsaeError(f"wsae_probe_plan_workspace_bytes rejects rows={rows} k={k} hidden={tracker.hidden} cols={P}")
    # first guess: every entry of the code for the full dictionary, the subset's share of them (with room) otherwise
    cap = rows * k if tracker._col_of is None else min(rows * k, 1024 + 2 * rows * k * P // tracker.hidden)
    with torch.cuda.device(dev):
        for _ in range(2):
            t_row = torch.empty(cap, dtype=torch.int32, device=dev)
            t_val = torch.empty(cap, dtype=torch.float32, device=dev)
            ws = workspace(tracker, need, dev)
            N.check(lib.wsae_probe_plan(v.data_ptr(), i.data_ptr(), k, tracker.hidden, seg.data_ptr(), rows, N.ptr(tracker._col_of),
                                        P, col_ptr.data_ptr(), N.ptr(t_row), N.ptr(t_val), cap, nnz.data_ptr(), ws.data_ptr(), need,
                                        torch.cuda.current_stream(dev).cuda_stream), "wsae_probe_plan")
            n = int(nnz.item())
            if n <= cap:
                break
            del t_row, t_val
            cap = n  # (the plan names the true count: grow once and transpose again)
    return col_ptr, t_row, t_val, n


# ---- the lifecycle of a tracker that keeps its tensors in a ``_state`` dict (some of them None) ---------------------------
def state_field(tracker, name: str) -> Tensor:
    tracker._ensure_device()
    return tracker._state[name]


def state_property(name: str, doc: str) -> property:
    return property(lambda tracker: state_field(tracker, name), doc=doc)


def state_to_cpu(tracker) -> dict:
    """The ``"state"`` entry of a saved tracker."""
    tracker._ensure_device()
    return {name: None if t is None else t.cpu() for name, t in tracker._state.items()}


def state_from_saved(tracker, saved: dict) -> None:
    tracker._ensure_device()
    for name, t in saved.items():
        if t is not None:
            tracker._state[name].copy_(t)


def batches(utterances):
    """``(x [n_utt, T, D], frame_mask or None)`` of every item: a tensor, or a pair ``(x, frame_mask)``."""
    for batch in utterances:
        x, mask = (batch[0], batch[1]) if isinstance(batch, (tuple, list)) else (batch, None)
        if x.dim() != 3:
            raise ValueError(f"an utterance batch must be [n_utt, T, D], got {tuple(x.shape)}")
        yield x, mask


def labelled_batches(utterances):
    """``(x, labels or targets, frame_mask or None)`` of every item ``(x, labels)`` or ``(x, labels, frame_mask)``."""
    for batch in utterances:
        if not isinstance(batch, (tuple, list)) or len(batch) not in (2, 3):
            raise ValueError("an item must be (x [n_utt, T, D], labels [n_utt, T]) or (x, labels, frame_mask)")
        x, labels, mask = batch[0], batch[1], batch[2] if len(batch) == 3 else None
        if x.dim() != 3:
            raise ValueError(f"an utterance batch must be [n_utt, T, D], got {tuple(x.shape)}")
        yield x, labels, mask


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


def top_weights(w: Tensor, features: Tensor, n: int) -> Tuple[Tensor, Tensor]:
    """``(features, weights)`` at the ``n`` largest of the weights ``w``, descending, ties to the lower position."""
    order = rank_features(w, torch.ones_like(w, dtype=torch.bool), n)
    return features[order], w[order]


def curve_arguments(ranking, sizes) -> Tuple[Tensor, Tuple[int, ...]]:
    """``(ranking int64 [n] on the CPU, sizes)`` of a k-sparse curve; ``ValueError`` unless the sizes are prefixes of it."""
    ranking = torch.as_tensor(ranking).detach().reshape(-1).cpu().to(torch.int64)
    sizes = tuple(int(s) for s in sizes)
    if not sizes or min(sizes) < 1 or max(sizes) > ranking.numel():
        raise ValueError(f"sizes must lie in 1..{ranking.numel()}, the length of the ranking: got {sizes}")
    return ranking, sizes
