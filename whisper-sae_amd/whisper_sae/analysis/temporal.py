"""Temporal run statistics: does a feature blink on for a frame or two, as a burst or an onset
does, or does it hold for a phone, a syllable or the whole utterance, as speaker, channel and language do - and where in
the utterance are its activations?

The unit between the frame and the utterance is the run: a maximal stretch of consecutive frames of one utterance on
which a feature is active.  ``RunTracker`` counts runs, their lengths and the gaps between them straight from the compact
``(values, indices)`` code (``wsae_runs_update`` - the dense ``[frames, H]`` matrix never exists), and optionally lists
every run as an event ``(feature, utterance, start, length, total, peak)``, the bounds a clip extractor needs instead of
a fixed window around one top frame.  The state is integer, so it does not depend on the order of the batches, on how
whole utterances are grouped into batches or on the launch geometry.  Runs end with the call: pass whole utterances.
The summary over ``[f_cols]`` vectors is plain torch in float64.

Out of scope: lagged co-firing between different features (``CoactivationTracker`` on a shifted code gives it), runs
continued across calls, dense / ReLU codes, magnitude envelopes beyond ``total`` and ``peak``, merging the trackers of
data-parallel ranks beyond ``merge``, plots and audio IO.
"""

from __future__ import annotations

from pathlib import Path
from typing import NamedTuple, Optional, Tuple

import torch
from torch import Tensor

from .. import _native as N
from . import _stream

RUNS_BINS = N.RUNS_BINS


class RunSummary(NamedTuple):
    """Per feature of the window.  ``runs``, ``frames``: int64 counts.  Float64: ``max_duration``, ``mean_duration``
    (frames / runs), ``std_duration`` (population standard deviation of the run lengths), ``median_duration`` and
    ``median_gap`` (read off the histograms: the lower length of the smallest bin whose cumulative count reaches half
    the total; exact up to 32 frames), all in frames, or in milliseconds when ``frame_ms`` was given;
    ``persistence`` = 1 - runs / frames, which is P(active at t + 1 | active at t, same utterance) up to the runs that
    end with their utterance; ``duty`` = frames / total rows; ``event_rate`` = runs / total rows.  Where a feature has no
    run every ratio is NaN (``max_duration`` is 0); ``median_gap`` is NaN where it has no gap."""

    runs: Tensor
    frames: Tensor
    max_duration: Tensor
    mean_duration: Tensor
    std_duration: Tensor
    median_duration: Tensor
    persistence: Tensor
    duty: Tensor
    event_rate: Tensor
    median_gap: Tensor


class FeatureEvents(NamedTuple):
    """One element per run, ordered by (feature, utterance, start): ``feature``, ``utterance``, ``start`` (the frame
    offset inside the utterance), ``length`` int32; ``total`` (the float32 sum of the run's values in frame order) and
    ``peak`` float32."""

    feature: Tensor
    utterance: Tensor
    start: Tensor
    length: Tensor
    total: Tensor
    peak: Tensor

    def sample_bounds(self, samples_per_frame: int, context_frames: int = 0) -> Tuple[Tensor, Tensor]:
        """``(start_sample, end_sample)`` int64 per event, ``end`` exclusive: the run widened by ``context_frames`` on
        either side (not below sample 0; the caller clips the end to the utterance's length)."""
        spf, ctx = int(samples_per_frame), int(context_frames)
        if spf < 1 or ctx < 0:
            raise ValueError(f"samples_per_frame must be positive and context_frames not negative, got {spf}, {ctx}")
        start = self.start.to(torch.int64)
        lo = (start - ctx).clamp(min=0) * spf
        hi = (start + self.length.to(torch.int64) + ctx) * spf
        return lo, hi


def bin_lower_length(bins: Tensor) -> Tensor:
    """The smallest length of each histogram bin: ``b + 1`` up to bin 31, ``2^(b - 27) + 1`` from bin 32 on."""
    b = bins.to(torch.int64)
    return torch.where(b < 32, b + 1, torch.bitwise_left_shift(torch.ones_like(b), (b - 27).clamp(min=0)) + 1)


def histogram_quantile(hist: Tensor, q: float) -> Tensor:
    """Per row of ``hist [F, 48]``: the lower length of the smallest bin whose cumulative count reaches ``q`` times the
    row's total, float64 (NaN for an empty row)."""
    q = float(q)
    if not 0.0 < q <= 1.0:
        raise ValueError(f"q must lie in (0, 1], got {q}")
    cum = hist.to(torch.int64).cumsum(1)
    total = cum[:, -1]
    reached = cum.double() >= q * total.double()[:, None]
    first = reached.to(torch.int8).argmax(1)
    out = bin_lower_length(first).double()
    return torch.where(total > 0, out, torch.full_like(out, float("nan")))


def summarize_runs(frames: Tensor, runs: Tensor, dur_max: Tensor, dur_sq: Tensor, dur_hist: Tensor,
                   gap_hist: Optional[Tensor], total_rows: Tensor, frame_ms: Optional[float] = None) -> RunSummary:
    """The summary of an integer state (the fields of ``wsae_runs_update``, on any device), float64, plain torch."""
    unit = 1.0 if frame_ms is None else float(frame_ms)
    n, fr = runs.double(), frames.double()
    rows = total_rows.double().reshape(-1)[0]
    nan = torch.full_like(n, float("nan"))
    some = runs > 0
    mean = torch.where(some, fr / n, nan)
    std = torch.where(some, (dur_sq.double() / n - mean * mean).clamp(min=0).sqrt(), nan)
    gap = nan if gap_hist is None else histogram_quantile(gap_hist, 0.5)
    return RunSummary(runs=runs.to(torch.int64), frames=frames.to(torch.int64), max_duration=dur_max.double() * unit,
                      mean_duration=mean * unit, std_duration=std * unit,
                      median_duration=histogram_quantile(dur_hist, 0.5) * unit,
                      persistence=torch.where(some, 1.0 - n / fr, nan), duty=torch.where(some, fr / rows, nan),
                      event_rate=torch.where(some, n / rows, nan), median_gap=gap * unit)


class RunTracker:
    """Run statistics of a compact code over a stream of whole utterances.

    ``f_window=(f_lo, f_cols)``: keep only the features ``f_lo .. f_lo + f_cols - 1``.  ``gaps=False`` drops the gap
    histogram.  ``max_events > 0`` keeps an event list of that capacity; only runs of at least ``min_event_len`` frames
    are listed.  The state lives on the device of the first update (or ``device``)."""

    def __init__(self, hidden: int, *, f_window: Optional[Tuple[int, int]] = None, gaps: bool = True, max_events: int = 0,
                 min_event_len: int = 1, device=None):
        self.hidden = int(hidden)
        if self.hidden < 1:
            raise ValueError(f"hidden must be positive, got {hidden}")
        self.f_lo, self.f_cols = _stream.feature_window(f_window, self.hidden)
        self.with_gaps = bool(gaps)
        self.max_events, self.min_event_len = int(max_events), int(min_event_len)
        if self.max_events < 0 or self.min_event_len < 1:
            raise ValueError(f"max_events must not be negative and min_event_len at least 1, got {max_events}, {min_event_len}")
        self.device = torch.device(device) if device is not None else None
        self._state: Optional[dict] = None
        self._ws: Optional[Tensor] = None
        self._next = 0       # the utterance number a 3-D code's first utterance gets
        self._form: Optional[str] = None  # "numbered" ([n_utt, T, k] updates) or "flat" (the caller's numbers)
        self._submitted = 0  # rows handed to update so far, padding included (host-side bound of the int32 state)

    # ---- state ----------------------------------------------------------------------------------
    def _ensure_device(self, like: Optional[Tensor] = None) -> torch.device:
        if self._state is not None:
            return self._state["frames"].device
        dev = _stream.need_gpu("RunTracker", self.device or (like.device if like is not None else None))
        z = lambda *shape, dtype=torch.int32: torch.zeros(*shape, dtype=dtype, device=dev)  # noqa: E731
        st = {"frames": z(self.f_cols), "runs": z(self.f_cols), "dur_max": z(self.f_cols),
              "dur_sq": z(self.f_cols, dtype=torch.int64), "dur_hist": z(self.f_cols, RUNS_BINS),
              "gap_hist": z(self.f_cols, RUNS_BINS) if self.with_gaps else None, "total_rows": z(1, dtype=torch.int64),
              "ev_int": None, "ev_flt": None, "ev_count": None}
        if self.max_events:
            st.update(ev_int=z(self.max_events, 4), ev_flt=z(self.max_events, 2, dtype=torch.float32),
                      ev_count=z(1, dtype=torch.int64))
        self._state = st
        self.device = st["frames"].device
        return self.device

    frames = _stream.state_property("frames", "``[f_cols]`` int32: the frames on which the feature was active.")
    runs = _stream.state_property("runs", "``[f_cols]`` int32: the number of runs.")
    max_run = _stream.state_property("dur_max", "``[f_cols]`` int32: the longest run, in frames.")
    sum_squares = _stream.state_property("dur_sq", "``[f_cols]`` int64: the sum of the squared run lengths.")
    duration_hist = _stream.state_property("dur_hist", "``[f_cols, 48]`` int32: the run-length histogram.")
    total_rows = _stream.state_property("total_rows", "``[1]`` int64: the non-padding frames seen.")

    @property
    def gap_hist(self) -> Tensor:
        if not self.with_gaps:
            raise ValueError("this tracker keeps no gap histogram: build it with gaps=True")
        return _stream.state_field(self, "gap_hist")

    @property
    def event_count(self) -> int:
        """Runs that qualified as events so far, dropped ones included (synchronises the device)."""
        return 0 if self._state is None or self._state["ev_count"] is None else int(self._state["ev_count"].item())

    # ---- accumulation ---------------------------------------------------------------------------
    def update(self, code, segments: Optional[Tensor] = None, frame_mask: Optional[Tensor] = None) -> None:
        """One batch of whole utterances.  ``code = (values, indices)``: either ``[n_utt, T, k]``, whose utterances are
        numbered from a running base (``segments`` must be None), or flat ``[rows, k]`` in time order with ``segments
        [rows]``, the caller's utterance number of each row (negative: padding).  The numbers may be global ones: the
        call works on ``number - smallest number of the call`` (this form reads the smallest and the largest number back
        from the device), its workspace and job count grow with the span of the numbers of one call, and the events carry
        the caller's numbers.  A tracker takes one of the two forms, not both.  Frames with ``frame_mask == 0`` are
        padding: they end a run and count for nothing."""
        vals, idx, k = _stream.compact_code(code, "code", N.RUNS_MAX_K)
        dev = self._ensure_device(vals)
        if vals.device != dev:
            raise N.WsaeError(f"the code is on {vals.device}, the tracker on {dev}")
        form = _stream.take_form(self, vals, "number their utterances differently and ")
        seg, n_utt = _stream.frame_segments(vals, segments, frame_mask, dev)
        used, rows = n_utt or 0, seg.shape[0]
        base, n_seg = self._next, used  # (a flat code: read back below)
        _stream.check_row_bound(self, rows)  # (frames, runs and the histogram cells are int32)
        if rows and n_utt is None:
            base, live = 0, seg >= 0
            hi = int(seg.max().item())
            if hi >= 0:  # (else padding only: n_seg stays below 1)
                base = int(torch.where(live, seg, torch.full_like(seg, hi)).min().item())
                seg = torch.where(live, seg - base, seg)
                n_seg = hi - base + 1
        if rows == 0 or n_seg < 1:  # nothing, or padding only
            self._next += used
            self._submitted += rows
            self._form = form
            return
        v, i = _stream.flat_code(vals, idx, k)
        st = self._state
        with torch.cuda.device(dev):
            _stream.grow(self, 2 * n_seg, torch.int32, dev)
            N.check(N.lib().wsae_runs_update(
                v.data_ptr(), i.data_ptr(), k, self.hidden, seg.data_ptr(), rows, n_seg, base, self.f_lo, self.f_cols,
                st["frames"].data_ptr(), st["runs"].data_ptr(), st["dur_max"].data_ptr(), st["dur_sq"].data_ptr(),
                st["dur_hist"].data_ptr(), N.ptr(st["gap_hist"]), st["total_rows"].data_ptr(), N.ptr(st["ev_int"]),
                N.ptr(st["ev_flt"]), self.max_events, self.min_event_len, N.ptr(st["ev_count"]), self._ws.data_ptr(),
                self._ws.numel() * 4, torch.cuda.current_stream(dev).cuda_stream), "wsae_runs_update")
        self._next += used  # (only now: a failed call has counted nothing and leaves the numbering where it was)
        self._submitted += rows
        self._form = form

    def _same_kind(self, other: "RunTracker") -> bool:
        return (self.hidden, self.f_lo, self.f_cols, self.with_gaps, self.max_events > 0, self.min_event_len) == \
               (other.hidden, other.f_lo, other.f_cols, other.with_gaps, other.max_events > 0, other.min_event_len)

    def merge(self, other: "RunTracker") -> None:
        """Add the state of a tracker of the same kind (another shard of the dataset): integer adds, a maximum, and the
        other's events appended (the capacity grows to hold both lists).  Trackers fed ``[n_utt, T, k]`` codes number
        their utterances from 0 each: the other's utterance numbers are moved behind this tracker's running base.
        Trackers fed flat codes carry the caller's own numbers, which are kept as they are - keeping them distinct
        across shards is the caller's business.  The two forms do not merge."""
        if not self._same_kind(other):
            raise ValueError("merge needs two trackers of the same size, window, gap and event settings")
        if None not in (self._form, other._form) and self._form != other._form:
            raise ValueError(f"merge: a tracker of {self._form} updates and one of {other._form} updates number their "
                             f"utterances differently")
        _stream.check_row_bound(self, other._submitted, merging=True)
        if other._state is None:
            return
        dev = self._ensure_device(other._state["frames"])
        a, b = self._state, other._state
        for name in ("frames", "runs", "dur_sq", "dur_hist", "total_rows") + (("gap_hist",) if self.with_gaps else ()):
            a[name] += b[name].to(dev)
        torch.maximum(a["dur_max"], b["dur_max"].to(dev), out=a["dur_max"])
        if self.max_events:
            na, nb = int(a["ev_count"].item()), int(b["ev_count"].item())
            ka, kb = min(na, self.max_events), min(nb, other.max_events)
            # records that either tracker had already dropped stay lost: then the list is cut to what is held, so that
            # the cursor (the sum of the two) stays past the capacity and events() goes on saying so
            cap = max(self.max_events, ka + kb) if na + nb == ka + kb else ka + kb
            ev_int = torch.zeros(cap, 4, dtype=torch.int32, device=dev)
            ev_flt = torch.zeros(cap, 2, dtype=torch.float32, device=dev)
            ev_int[:ka], ev_flt[:ka] = a["ev_int"][:ka], a["ev_flt"][:ka]
            ev_int[ka:ka + kb], ev_flt[ka:ka + kb] = b["ev_int"][:kb].to(dev), b["ev_flt"][:kb].to(dev)
            if other._form == "numbered":
                ev_int[ka:ka + kb, 1] += self._next
            a["ev_int"], a["ev_flt"], self.max_events = ev_int, ev_flt, cap
            a["ev_count"].fill_(na + nb)
        self._next += other._next
        self._submitted += other._submitted
        self._form = self._form or other._form

    # ---- reading --------------------------------------------------------------------------------
    def duration_quantile(self, q: float, frame_ms: Optional[float] = None) -> Tensor:
        """``[f_cols]`` float64: the ``q`` quantile of the run lengths read off the histogram (the lower length of the
        smallest bin whose cumulative count reaches ``q * runs``; exact up to 32 frames), in frames or milliseconds."""
        out = histogram_quantile(self.duration_hist, q)
        return out if frame_ms is None else out * float(frame_ms)

    def summary(self, frame_ms: Optional[float] = None) -> RunSummary:
        """The per-feature summary, float64 from the integers; durations in frames, or in milliseconds with
        ``frame_ms`` (20 for Whisper's encoder)."""
        self._ensure_device()
        st = self._state
        return summarize_runs(st["frames"], st["runs"], st["dur_max"], st["dur_sq"], st["dur_hist"], st["gap_hist"],
                              st["total_rows"], frame_ms=frame_ms)

    def events(self, feature: Optional[int] = None) -> FeatureEvents:
        """The listed runs in the canonical order (feature, utterance, start); ``feature=f``: those of feature f alone.
        Raises ``WsaeError`` when more runs qualified than the list holds."""
        if not self.max_events:
            raise ValueError("this tracker keeps no events: build it with max_events > 0")
        self._ensure_device()
        n = self.event_count
        if n > self.max_events:
            raise N.WsaeError(f"RunTracker.events: {n} runs qualified as events but the list holds {self.max_events}; build "
                              f"the tracker with max_events >= {n} (or a larger min_event_len) and run again")
        ev_int, ev_flt = self._state["ev_int"][:n], self._state["ev_flt"][:n]
        order = torch.argsort(ev_int[:, 2], stable=True)
        order = order[torch.argsort(ev_int[order, 1], stable=True)]
        order = order[torch.argsort(ev_int[order, 0], stable=True)]
        if feature is not None:
            order = order[ev_int[order, 0] == int(feature)]
        ev_int, ev_flt = ev_int[order], ev_flt[order]
        return FeatureEvents(feature=ev_int[:, 0].contiguous(), utterance=ev_int[:, 1].contiguous(),
                             start=ev_int[:, 2].contiguous(), length=ev_int[:, 3].contiguous(),
                             total=ev_flt[:, 0].contiguous(), peak=ev_flt[:, 1].contiguous())

    # ---- persistence ----------------------------------------------------------------------------
    def save(self, path) -> None:
        torch.save({"hidden": self.hidden, "f_window": [self.f_lo, self.f_cols], "gaps": self.with_gaps,
                    "max_events": self.max_events, "min_event_len": self.min_event_len, "next": self._next, "form": self._form,
                    "submitted": self._submitted, "state": _stream.state_to_cpu(self)}, Path(path))

    @classmethod
    def load(cls, path, device=None) -> "RunTracker":
        data = torch.load(Path(path), map_location="cpu", weights_only=True)
        t = cls(data["hidden"], f_window=tuple(data["f_window"]), gaps=data["gaps"], max_events=data["max_events"],
                min_event_len=data["min_event_len"], device=device)
        _stream.state_from_saved(t, data["state"])
        t._next, t._submitted, t._form = int(data["next"]), int(data["submitted"]), data["form"]
        return t


def top_temporal_features(summary: RunSummary, by: str = "mean_duration", n: int = 20, min_runs: int = 1,
                          largest: bool = True):
    """The ``n`` features with the largest (``largest=False``: smallest) value of the summary field ``by`` as
    ``(indices, values)``; only features with at least ``min_runs`` runs and a value that is not NaN are candidates
    (fewer than ``n`` may remain).  Ties go to the lower index."""
    if by not in RunSummary._fields:
        raise ValueError(f"by must be one of {RunSummary._fields}, got {by!r}")
    value = getattr(summary, by).double()
    ok = (summary.runs >= int(min_runs)) & ~torch.isnan(value)
    order = _stream.rank_features(value if largest else -value, ok, n)
    return order, getattr(summary, by)[order]


def collect_runs(model, utterances, *, device="cuda", **tracker_kw) -> RunTracker:
    """Run statistics over a dataset of utterances.  Every item of ``utterances`` is a tensor ``[n_utt, T, D]`` or a pair
    ``(x, frame_mask [n_utt, T])``; utterances are numbered in the order they arrive.  ``tracker_kw`` goes to
    ``RunTracker``.  The module must offer ``encode_compact`` (TopK and BatchTopK SAEs; a ReLU SAE's code is dense:
    ``TypeError``) and is run in eval mode; its previous mode is restored."""
    with _stream.encoding(model, hint="run statistics are for TopK-family codes"):
        tracker = RunTracker(model.hidden_dim, device=device, **tracker_kw)
        for x, mask in _stream.batches(utterances):
            tracker.update(_stream.utterance_code(model, x, device), frame_mask=None if mask is None else mask.to(device))
    return tracker
