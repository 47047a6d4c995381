"""Feature-triggered averages: what is in the input when a feature fires?

The average of a dense per-frame signal - log-mel frames, another layer's residual, frame energy, a one-hot phone
alignment - around the frames on which a feature is active, over ALL of its firing frames: the spike-triggered average.
``TriggeredAverageTracker`` accumulates, per feature and lag, the weighted sum of the signal, the sum of the weights and
the number of terms straight from the compact ``(values, indices)`` code (``wsae_sta_update`` - the dense ``[frames, H]``
matrix never exists).  Every cell is one chain of float64 additions in frame order, so the state does not depend on the
launch geometry, on the window a feature is read through or on how whole utterances are grouped into batches, as long as
they arrive in the same order.  Lags never cross an utterance: pass whole utterances.  The averages, the per-channel
baseline and the contrast are plain torch in float64.

Out of scope: triggers other than "active" and "onset", per-lag weights, second moments per feature (the contrast is
against the signal's own per-channel spread), significance tests, plots and audio IO.
"""

from __future__ import annotations

from pathlib import Path
from typing import Optional, Tuple

import torch
from torch import Tensor

from .. import _native as N
from . import _stream

TRIGGERS = {"all": N.STA_TRIGGER_ALL, "onset": N.STA_TRIGGER_ONSET}
WEIGHTS = {"value": N.STA_WEIGHT_VALUE, "one": N.STA_WEIGHT_ONE}
_STAT_ROWS = 1 << 16  # rows per step of the baseline sums (bounds the float64 copy of the signal)


def mel_frames(mel: Tensor, stride: int = 2) -> Tensor:
    """``[n_utt, n_mels, stride * T] -> [n_utt, T, stride * n_mels]``, sub-frame major: channel ``s * n_mels + m`` of
    frame ``t`` is mel bin ``m`` of column ``stride * t + s``.  Whisper's encoder position ``t`` sees the mel columns
    ``2 t`` and ``2 t + 1`` (its second convolution has stride 2)."""
    stride = int(stride)
    if mel.dim() != 3 or stride < 1 or mel.shape[2] % stride:
        raise ValueError(f"mel must be [n_utt, n_mels, stride * T] with stride >= 1, got {tuple(mel.shape)} and stride {stride}")
    n_utt, n_mels, cols = mel.shape
    return mel.reshape(n_utt, n_mels, cols // stride, stride).permute(0, 2, 3, 1).reshape(n_utt, cols // stride, stride * n_mels)


def as_spectrogram(template: Tensor, n_mels: int, stride: int = 2) -> Tensor:
    """The inverse of ``mel_frames`` on the last two dimensions: ``[..., L, stride * n_mels] -> [..., n_mels, L * stride]``,
    a template over ``L`` lags as a patch of ``L * stride`` mel columns."""
    n_mels, stride = int(n_mels), int(stride)
    if template.dim() < 2 or n_mels < 1 or stride < 1 or template.shape[-1] != stride * n_mels:
        raise ValueError(f"template must be [..., L, {stride} * {n_mels}], got {tuple(template.shape)}")
    lead, L = template.shape[:-2], template.shape[-2]
    t = template.reshape(*lead, L, stride, n_mels)
    return t.movedim(-1, -3).reshape(*lead, n_mels, L * stride)


def triggered_average(sums: Tensor, weights: Tensor) -> Tensor:
    """``sums [F, L, C] / weights [F, L]``, float64, NaN where the weight is 0 (no term at that lag)."""
    w = weights.double()[..., None]
    return torch.where(w != 0, sums.double() / w, torch.full_like(sums.double(), float("nan")))


def signal_baseline(sig_sum: Tensor, sig_sq: Tensor, total_rows) -> Tuple[Tensor, Tensor]:
    """Per-channel mean and (population) standard deviation of the signal over the non-padding rows, float64; NaN
    without rows."""
    n = torch.as_tensor(total_rows).double().reshape(-1)[0]
    mean = sig_sum.double() / n
    std = (sig_sq.double() / n - mean * mean).clamp(min=0).sqrt()
    return mean, std


def template_contrast(average: Tensor, mean: Tensor, std: Tensor) -> Tensor:
    """``(average - mean_c) / std_c``: the template in units of the channel's own spread; NaN where ``std_c == 0``."""
    z = (average - mean) / std
    return torch.where(std > 0, z, torch.full_like(z, float("nan")))


class TriggeredAverageTracker:
    """Feature-triggered sums of a per-frame signal over a stream of whole utterances.

    ``lags=(lo, hi)``: the lags ``lo .. hi`` (at most 64, within +-1024; 0 need not be among them).  ``trigger="all"``:
    every frame on which a feature is active; ``"onset"``: only the first frame of each run.  ``weight="value"``: a
    trigger weighs its activation; ``"one"``: 1.  ``f_window=(f_lo, f_cols)``: keep only those features.  The state lives
    on the device of the first update (or ``device``)."""

    def __init__(self, hidden: int, channels: int, *, lags: Tuple[int, int] = (-8, 8), trigger: str = "all",
                 weight: str = "value", f_window: Optional[Tuple[int, int]] = None, device=None):
        self.hidden, self.channels = int(hidden), int(channels)
        if self.hidden < 1:
            raise ValueError(f"hidden must be positive, got {hidden}")
        if not 1 <= self.channels <= N.STA_MAX_CH:
            raise ValueError(f"channels must be in 1..{N.STA_MAX_CH}, got {channels}")
        self.lag_lo, self.lag_hi = int(lags[0]), int(lags[1])
        if not (-1024 <= self.lag_lo <= self.lag_hi <= 1024) or self.lag_hi - self.lag_lo + 1 > N.STA_MAX_LAGS:
            raise ValueError(f"lags must be (lo, hi) with -1024 <= lo <= hi <= 1024 and at most {N.STA_MAX_LAGS} lags, got {lags}")
        if trigger not in TRIGGERS or weight not in WEIGHTS:
            raise ValueError(f"trigger must be one of {tuple(TRIGGERS)} and weight one of {tuple(WEIGHTS)}, got {trigger!r}, "
                             f"{weight!r}")
        self.trigger, self.weight = trigger, weight
        self.f_lo, self.f_cols = _stream.feature_window(f_window, self.hidden)
        self.device = torch.device(device) if device is not None else None
        self._state: Optional[dict] = None
        self._ws: Optional[Tensor] = None
        self._form: Optional[str] = None  # "numbered" ([n_utt, T, k] updates) or "flat" (rows with segments)

    n_lags = property(lambda self: self.lag_hi - self.lag_lo + 1, doc="The number of lags L.")

    # ---- state ----------------------------------------------------------------------------------
    def _ensure_device(self, like: Optional[Tensor] = None) -> torch.device:
        if self._state is not None:
            return self._state["acc"].device
        dev = _stream.need_gpu("TriggeredAverageTracker", self.device or (like.device if like is not None else None))
        z = lambda *shape, dtype=torch.float64: torch.zeros(*shape, dtype=dtype, device=dev)  # noqa: E731
        self._state = {"acc": z(self.f_cols, self.n_lags, self.channels), "wsum": z(self.f_cols, self.n_lags),
                       "cnt": z(self.f_cols, self.n_lags, dtype=torch.int64), "sig_sum": z(self.channels),
                       "sig_sq": z(self.channels), "total_rows": z(1, dtype=torch.int64)}
        self.device = self._state["acc"].device
        return self.device

    sums = _stream.state_property("acc", "``[f_cols, L, C]`` float64: the weighted sums of the signal.")
    weights = _stream.state_property("wsum", "``[f_cols, L]`` float64: the sums of the weights.")
    counts = _stream.state_property("cnt", "``[f_cols, L]`` int64: the number of terms.")
    sig_sum = _stream.state_property("sig_sum", "``[C]`` float64: the signal summed over the non-padding frames.")
    sig_sq = _stream.state_property("sig_sq", "``[C]`` float64: ... and its squares.")
    total_rows = _stream.state_property("total_rows", "``[1]`` int64: the non-padding frames seen.")

    # ---- accumulation ---------------------------------------------------------------------------
    def update(self, code, signal: Tensor, segments: Optional[Tensor] = None, frame_mask: Optional[Tensor] = None) -> None:
        """One batch of whole utterances.  ``code = (values, indices)``: either ``[n_utt, T, k]`` with ``signal
        [n_utt, T, C]`` (``segments`` must be None), or flat ``[rows, k]`` in time order with ``signal [rows, C]`` and
        ``segments [rows]``, the utterance number of each row (negative: padding).  ``signal`` is float32 or bfloat16
        (anything else is converted to float32).  A tracker takes one of the two forms, not both.  Frames with
        ``frame_mask == 0`` are padding: they trigger nothing, end a run, and their signal is never read."""
        vals, idx, k = _stream.compact_code(code, "code", N.STA_MAX_K, also=((signal, "signal"),))
        if signal.shape != vals.shape[:-1] + (self.channels,):
            raise ValueError(f"signal must be {tuple(vals.shape[:-1]) + (self.channels,)} for this code, got {tuple(signal.shape)}")
        dev = self._ensure_device(vals)
        if vals.device != dev or signal.device != dev:
            raise N.WsaeError(f"the code is on {vals.device} and the signal on {signal.device}, the tracker on {dev}")
        form = _stream.take_form(self, vals)
        seg, _ = _stream.frame_segments(vals, segments, frame_mask, dev)
        rows = seg.shape[0]
        if rows > _stream.MAX_ROWS:
            raise N.WsaeError(f"TriggeredAverageTracker: {rows} frames in one update exceed {_stream.MAX_ROWS}")
        self._form = form
        if rows == 0:
            return
        v, i = _stream.flat_code(vals, idx, k)
        y = signal.detach()
        if y.dtype not in (torch.float32, torch.bfloat16):
            y = y.to(torch.float32)
        if not (y.dim() == 2 and y.stride(1) == 1 and y.stride(0) >= self.channels):
            y = y.reshape(-1, self.channels).contiguous()
        ldy = y.stride(0) if rows > 1 else max(y.stride(0), self.channels)
        st = self._state
        with torch.cuda.device(dev):
            need = int(N.lib().wsae_sta_workspace_bytes(rows, k, self.hidden, self.f_lo, self.f_cols))
            if need < 0:
                raise N.WsaeError(f"wsae_sta_workspace_bytes rejected rows = {rows}, k = {k}")
            _stream.grow(self, (need + 7) // 8, torch.int64, dev)
            N.check(N.lib().wsae_sta_update(
                v.data_ptr(), i.data_ptr(), k, self.hidden, seg.data_ptr(), rows, y.data_ptr(),
                N.DT_BF16 if y.dtype == torch.bfloat16 else N.DT_F32, self.channels, ldy, self.lag_lo, self.lag_hi, self.f_lo,
                self.f_cols, TRIGGERS[self.trigger], WEIGHTS[self.weight], st["acc"].data_ptr(), st["wsum"].data_ptr(),
                st["cnt"].data_ptr(), self._ws.data_ptr(), self._ws.numel() * 8,
                torch.cuda.current_stream(dev).cuda_stream), "wsae_sta_update")
        live = seg >= 0
        st["total_rows"] += live.sum()
        zero = torch.zeros((), dtype=torch.float64, device=dev)
        for lo in range(0, rows, _STAT_ROWS):  # the baseline: plain torch, float64, padding rows replaced by 0
            y64 = torch.where(live[lo:lo + _STAT_ROWS, None], y[lo:lo + _STAT_ROWS].double(), zero)
            st["sig_sum"] += y64.sum(0)
            st["sig_sq"] += (y64 * y64).sum(0)

    def _same_kind(self, other: "TriggeredAverageTracker") -> bool:
        key = lambda t: (t.hidden, t.channels, t.lag_lo, t.lag_hi, t.trigger, t.weight, t.f_lo, t.f_cols)  # noqa: E731
        return key(self) == key(other)

    def merge(self, other: "TriggeredAverageTracker") -> None:
        """Add the state of a tracker of the same kind (another shard of the dataset): one float64 add per cell."""
        if not self._same_kind(other):
            raise ValueError("merge needs two trackers of the same sizes, lags, trigger, weight and window")
        if other._state is None:
            return
        dev = self._ensure_device(other._state["acc"])
        for name, t in other._state.items():
            self._state[name] += t.to(dev)
        self._form = self._form or other._form

    # ---- reading --------------------------------------------------------------------------------
    def averages(self) -> Tensor:
        """``[f_cols, L, C]`` float64: ``sums / weights``, NaN where a feature has no term at a lag."""
        return triggered_average(self.sums, self.weights)

    def baseline(self) -> Tuple[Tensor, Tensor]:
        """``(mean, std)``, ``[C]`` float64 each: the signal over all non-padding frames."""
        return signal_baseline(self.sig_sum, self.sig_sq, self.total_rows)

    def contrast(self) -> Tensor:
        """``[f_cols, L, C]`` float64: ``(average - mean_c) / std_c``."""
        mean, std = self.baseline()
        return template_contrast(self.averages(), mean, std)

    # ---- persistence ----------------------------------------------------------------------------
    def save(self, path) -> None:
        torch.save({"hidden": self.hidden, "channels": self.channels, "lags": [self.lag_lo, self.lag_hi],
                    "trigger": self.trigger, "weight": self.weight, "f_window": [self.f_lo, self.f_cols], "form": self._form,
                    "state": _stream.state_to_cpu(self)}, Path(path))

    @classmethod
    def load(cls, path, device=None) -> "TriggeredAverageTracker":
        data = torch.load(Path(path), map_location="cpu", weights_only=True)
        t = cls(data["hidden"], data["channels"], lags=tuple(data["lags"]), trigger=data["trigger"], weight=data["weight"],
                f_window=tuple(data["f_window"]), device=device)
        _stream.state_from_saved(t, data["state"])
        t._form = data["form"]
        return t


def top_template_features(tracker, by: str = "contrast_peak", n: int = 20, min_count: int = 1, counts: Optional[Tensor] = None):
    """The ``n`` features with the most distinct template as ``(indices, scores)``.  ``tracker``: a
    ``TriggeredAverageTracker``, or a contrast tensor ``[F, L, C]`` together with ``counts [F, L]``.
    ``by="contrast_peak"``: the largest ``|contrast|`` over lags and channels; ``"contrast_energy"``: the mean of
    ``contrast^2`` over them (NaN cells are left out of both).  Only features whose largest per-lag count reaches
    ``min_count`` and whose score is not NaN are candidates (fewer than ``n`` may remain).  Ties go to the lower index."""
    if by not in ("contrast_peak", "contrast_energy"):
        raise ValueError(f"by must be 'contrast_peak' or 'contrast_energy', got {by!r}")
    if isinstance(tracker, Tensor):
        if counts is None:
            raise ValueError("a contrast tensor needs counts [F, L]")
        z = tracker.double()
    else:
        z, counts = tracker.contrast(), tracker.counts
    flat = z.reshape(z.shape[0], -1)
    ok_cell = ~torch.isnan(flat)
    clean = torch.where(ok_cell, flat, torch.zeros_like(flat))
    cells = ok_cell.sum(1)
    nan = torch.full((z.shape[0],), float("nan"), dtype=torch.float64, device=z.device)
    if by == "contrast_peak":
        score = torch.where(cells > 0, clean.abs().amax(1), nan)
    else:
        score = torch.where(cells > 0, (clean * clean).sum(1) / cells.clamp(min=1), nan)
    ok = (counts.reshape(z.shape[0], -1).amax(1) >= int(min_count)) & ~torch.isnan(score)
    order = _stream.rank_features(score, ok, n)
    return order, score[order]


def collect_triggered_averages(model, utterances, *, device="cuda", **tracker_kw) -> TriggeredAverageTracker:
    """Triggered averages over a dataset.  Every item of ``utterances`` is ``(x [n_utt, T, D], signal [n_utt, T, C])`` or
    ``(x, signal, frame_mask [n_utt, T])``.  ``tracker_kw`` goes to ``TriggeredAverageTracker`` (the number of channels is
    read off the first signal).  The module must offer ``encode_compact`` (TopK and BatchTopK SAEs; a ReLU SAE's code is
    dense: ``TypeError``) and is run in eval mode; its previous mode is restored."""
    tracker = None
    with _stream.encoding(model, hint="triggered averages are for TopK-family codes"):
        for batch in utterances:
            if not isinstance(batch, (tuple, list)) or len(batch) not in (2, 3):
                raise TypeError("an item must be (x, signal) or (x, signal, frame_mask)")
            x, signal = batch[0], batch[1]
            mask = batch[2] if len(batch) == 3 else None
            if x.dim() != 3 or signal.dim() != 3:
                raise ValueError(f"x and signal must be [n_utt, T, .], got {tuple(x.shape)} and {tuple(signal.shape)}")
            if tracker is None:
                tracker = TriggeredAverageTracker(model.hidden_dim, signal.shape[-1], device=device, **tracker_kw)
            tracker.update(_stream.utterance_code(model, x, device), signal.to(device),
                           frame_mask=None if mask is None else mask.to(device))
    if tracker is None:
        raise ValueError("collect_triggered_averages: no utterances")
    return tracker
