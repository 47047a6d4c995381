"""Code dynamics: how the code of a frame as a whole moves through time.

``frame_similarity`` gives the similarity (cosine, dot, Jaccard) of the codes of frames t and t + lag straight from the
compact ``(values, indices)`` code (``wsae_dyn_update`` - the dense ``[frames, H]`` matrix never exists), never across an
utterance.  ``CodeDynamics`` streams the same call over a dataset and keeps integer statistics per lag and per label
class of the pair (within one label, across two labels, unlabelled): ``summary`` reads means, deviations, quantiles, the
within / across separation and the time scale of the representation off them in float64.  ``boundary_curve`` scores the
local maxima of a per-frame curve (``novelty``) against reference boundaries at every threshold at once
(``wsae_boundary_score``): precision, recall, F1, over-segmentation and R-value at a tolerance in frames.  Every state is
a set of integer sums: it does not depend on the order of the batches, on the grouping of whole utterances into batches
or on the launch geometry, and the states of two shards add.

Out of scope: similarity between two different codes or layers, self-similarity matrices, smoothing of the curve,
segment-level labels from the boundaries, dense / ReLU codes.
"""

from __future__ import annotations

import math
from pathlib import Path
from typing import NamedTuple, Optional, Sequence, Tuple

import torch
from torch import Tensor

from .. import _native as N
from ..sae.engine import require_device_tensor
from . import _stream

METRICS = {"cosine": N.DYN_COSINE, "dot": N.DYN_DOT, "jaccard": N.DYN_JACCARD}
GROUPS = ("all", "within", "across")  # all pairs; both frames labelled and equal; both labelled and different
_GROUP_CLASSES = {"all": (0, 1, 2), "within": (0,), "across": (1,)}
_SCALE = 2.0 ** -30


def _check_lags(lags) -> Tuple[int, ...]:
    lags = tuple(int(l) for l in lags)
    if not 1 <= len(lags) <= N.DYN_MAX_LAGS:
        raise ValueError(f"lags must hold 1..{N.DYN_MAX_LAGS} lags, got {len(lags)}")
    if any(not 1 <= l <= N.DYN_MAX_LAG for l in lags) or any(b <= a for a, b in zip(lags, lags[1:])):
        raise ValueError(f"lags must ascend within 1..{N.DYN_MAX_LAG}, got {lags}")
    return lags


def _check_metric(metric: str) -> int:
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {tuple(METRICS)}, got {metric!r}")
    return METRICS[metric]


def _check_weights(weights, hidden: Optional[int]) -> Optional[Tensor]:
    if weights is None:
        return None
    if not isinstance(weights, Tensor) or weights.dim() != 1 or (hidden is not None and weights.numel() != hidden):
        want = "hidden" if hidden is None else str(hidden)
        raise ValueError(f"weights must be a [{want}] tensor, got "
                         f"{tuple(weights.shape) if isinstance(weights, Tensor) else type(weights).__name__}")
    return weights.detach().to(torch.float32).contiguous()


def _dyn_call(vals, idx, k, hidden, seg, weight, label, lags, metric, sim, state, holder):
    """``wsae_dyn_update`` on a flat code; ``holder._ws`` keeps the workspace."""
    rows, dev, lib = vals.shape[0], vals.device, N.lib()
    need = lib.wsae_dyn_workspace_bytes(rows, k, hidden, len(lags))
    if need < 0:
        raise N.WsaeError(f"wsae_dyn_workspace_bytes rejects rows={rows} k={k} hidden={hidden} lags={len(lags)}")
    ws = _stream.workspace(holder, need, dev)
    c_lags = (N._i32 * len(lags))(*lags)
    st = state or {}
    with torch.cuda.device(dev):
        N.check(lib.wsae_dyn_update(
            vals.data_ptr(), idx.data_ptr(), k, hidden, N.ptr(seg), N.ptr(weight), N.ptr(label), rows, c_lags, len(lags), metric,
            N.ptr(sim), N.ptr(st.get("pairs")), N.ptr(st.get("sim_q")), N.ptr(st.get("sq_q")), N.ptr(st.get("hist")),
            N.ptr(st.get("total_rows")), ws.data_ptr(), need, torch.cuda.current_stream(dev).cuda_stream), "wsae_dyn_update")


class _Workspace:
    _ws = None


def _segments_of(vals: Tensor, segments, frame_mask, dev) -> Optional[Tensor]:
    """The segment ids of a code of any leading shape: a ``[..., T, k]`` code numbers its ``[...]`` utterances itself, a
    ``[rows, k]`` code without ``segments`` is one utterance."""
    if vals.dim() == 2 and segments is None and frame_mask is None:
        return None
    if vals.dim() == 2 and segments is None:
        segments = torch.zeros(vals.shape[0], dtype=torch.int32, device=dev)
    if vals.dim() > 3:
        if segments is not None:
            raise ValueError("a [..., T, k] code numbers its utterances itself: pass segments only with a flat code")
        vals = vals.reshape(-1, vals.shape[-2], vals.shape[-1])
    return _stream.frame_segments(vals, segments, frame_mask, dev)[0]


def frame_similarity(code, lags: Sequence[int] = (1,), metric: str = "cosine", weights: Optional[Tensor] = None,
                     segments: Optional[Tensor] = None, frame_mask: Optional[Tensor] = None,
                     hidden: Optional[int] = None) -> Tensor:
    """``[..., n_lags]`` float32: the similarity of the code of every frame to the code ``lag`` frames later, NaN where
    that frame lies in another utterance, behind the end, or either of them is padding (``frame_mask == 0`` or
    ``segments < 0``).  ``code = (values, indices)`` ``[..., T, k]`` (every leading index an utterance) or flat
    ``[rows, k]`` with ``segments [rows]`` (None: one utterance).  ``metric``: ``"cosine"`` (clamped to 1), ``"dot"`` or
    ``"jaccard"`` of the sets of active features.  ``weights [hidden]`` scale every feature's value; a weight <= 0 or NaN
    removes the feature (a subset, idf weights).  ``hidden`` defaults to the length of ``weights`` or, without them, to
    "every index >= 0 is a feature"."""
    vals, idx, k = _stream.compact_code(code, "code", N.DYN_MAX_K, dims=None)
    if vals.dim() < 2:
        raise ValueError(f"code: values {tuple(vals.shape)} must be [..., T, k] or [rows, k]")
    lags, m = _check_lags(lags), _check_metric(metric)
    weight = _check_weights(weights, hidden)
    dev = _stream.need_gpu("frame_similarity", vals.device)
    if weight is not None:
        require_device_tensor(weight, "weights")
    hidden = int(hidden) if hidden is not None else (weight.numel() if weight is not None else 2 ** 31 - 1)
    seg = _segments_of(vals, segments, frame_mask, dev)
    v, i = _stream.flat_code(vals, idx, k)
    sim = torch.empty(v.shape[0], len(lags), dtype=torch.float32, device=dev)
    if v.shape[0]:
        _dyn_call(v, i, k, hidden, seg, weight, None, lags, m, sim, None, _Workspace())
    return sim.reshape(*vals.shape[:-1], len(lags))


def novelty(similarity: Tensor, lag_index: int = 0) -> Tensor:
    """``1 - similarity[..., lag_index]``: the curve whose peaks are candidate boundaries; entry t describes the step from
    frame t to t + lag.  NaN stays NaN."""
    return 1.0 - similarity[..., int(lag_index)]


# ---- the streaming tracker ----------------------------------------------------------------------------------------------------
class LagStats(NamedTuple):
    """Per lag, ``[n_lags]``: ``pairs`` int64; ``mean``, ``std``, ``median``, ``q10``, ``q90`` float64 (NaN without pairs)."""

    pairs: Tensor
    mean: Tensor
    std: Tensor
    median: Tensor
    q10: Tensor
    q90: Tensor


def hist_quantile(hist: Tensor, p: float) -> Tensor:
    """The ``p`` quantile of histograms ``[..., 64]`` of equal bins over [0, 1], float64: with n the total and t = p n,
    bin j is the first occupied bin whose cumulative count reaches t, and the result j / 64 + (t - cum[j - 1]) / hist[j] /
    64 - accurate to one bin.  NaN for an empty histogram."""
    h = hist.to(torch.int64)
    cum = h.cumsum(-1)
    n = cum[..., -1]
    t = float(p) * n.double()
    reached = (cum.double() >= t[..., None]) & (h > 0)
    j = reached.to(torch.int8).argmax(-1)
    before = (cum - h).gather(-1, j[..., None])[..., 0].double()
    inside = h.gather(-1, j[..., None])[..., 0].double()
    q = j.double() / N.DYN_BINS + (t - before) / torch.where(inside > 0, inside, torch.ones_like(inside)) / N.DYN_BINS
    return torch.where(n > 0, q, torch.full_like(q, float("nan")))


class DynamicsSummary:
    """What ``CodeDynamics.summary`` returns, on the host.  ``lags`` the lags; ``all``, ``within``, ``across``: ``LagStats``
    of all pairs, of the pairs inside one label and of the pairs across two labels; ``separation [n_lags]`` float64:
    (mean_within - mean_across) / sqrt((var_within + var_across) / 2); ``total_rows`` the frames seen."""

    def __init__(self, lags, groups, total_rows: int):
        self.lags, self.total_rows = tuple(lags), int(total_rows)
        self.all, self.within, self.across = groups["all"], groups["within"], groups["across"]
        pooled = torch.sqrt((self.within.std ** 2 + self.across.std ** 2) / 2)
        ok = pooled > 0
        self.separation = torch.where(ok, (self.within.mean - self.across.mean) / torch.where(ok, pooled, torch.ones_like(pooled)),
                                      torch.full_like(pooled, float("nan")))

    def timescale(self, group: str = "all") -> float:
        """The lag at which the mean similarity, linear between the requested lags, falls below 1/e of its value at the
        smallest lag; ``inf`` if it never does, NaN without pairs at the smallest lag."""
        if group not in GROUPS:
            raise ValueError(f"group must be one of {GROUPS}, got {group!r}")
        means = getattr(self, group).mean.tolist()
        if math.isnan(means[0]):
            return math.nan
        level = means[0] / math.e
        for i in range(1, len(means)):
            if means[i] < level:
                step = (means[i - 1] - level) / (means[i - 1] - means[i])
                return self.lags[i - 1] + step * (self.lags[i] - self.lags[i - 1])
        return math.inf


def summarize_state(lags, state: dict) -> DynamicsSummary:
    """``DynamicsSummary`` from integer state (any device): with n the pairs of a group, mean = sim_q / n / 2^30, the
    second moment sq_q / n / 2^30 (its terms are (x >> 15)^2), std = sqrt(max(second - mean^2, 0))."""
    st = {name: t.detach().cpu() for name, t in state.items()}
    groups = {}
    for g, classes in _GROUP_CLASSES.items():
        cls = list(classes)
        n = st["pairs"][:, cls].sum(1)
        nd = torch.where(n > 0, n, torch.ones_like(n)).double()
        nan = torch.full((n.numel(),), float("nan"), dtype=torch.float64)
        mean = st["sim_q"][:, cls].sum(1).double() / nd * _SCALE
        second = st["sq_q"][:, cls].sum(1).double() / nd * _SCALE
        std = torch.sqrt(torch.clamp(second - mean * mean, min=0.0))
        hist = st["hist"][:, cls].sum(1)
        groups[g] = LagStats(n, torch.where(n > 0, mean, nan), torch.where(n > 0, std, nan), hist_quantile(hist, 0.5),
                             hist_quantile(hist, 0.1), hist_quantile(hist, 0.9))
    return DynamicsSummary(lags, groups, int(st["total_rows"][0]))


class CodeDynamics:
    """Similarity statistics of a compact code against itself ``lag`` frames later, over a stream of utterances.

    ``lags``: ascending, distinct, 1..1024, at most 16.  ``metric``: ``"cosine"`` or ``"jaccard"`` (``"dot"`` is not
    bounded and has no statistics: use ``frame_similarity``).  ``weights [hidden]`` and ``hidden`` as in
    ``frame_similarity``.  The state lives on the device of the first update (or ``device``)."""

    def __init__(self, lags: Sequence[int] = (1,), metric: str = "cosine", weights: Optional[Tensor] = None, device=None,
                 hidden: Optional[int] = None):
        self.lags, self.metric = _check_lags(lags), metric
        if _check_metric(metric) == N.DYN_DOT:
            raise ValueError("CodeDynamics keeps statistics of similarities in [0, 1]: metric must be 'cosine' or 'jaccard'")
        if hidden is not None and int(hidden) < 1:
            raise ValueError(f"hidden must be positive, got {hidden}")
        self.weights = _check_weights(weights, None if hidden is None else int(hidden))
        self.hidden = int(hidden) if hidden is not None else (self.weights.numel() if self.weights is not None else 2 ** 31 - 1)
        self.device = torch.device(device) if device is not None else None
        self._state: Optional[dict] = None
        self._form: Optional[str] = None
        self._submitted = 0
        self._ws = None

    n_lags = property(lambda self: len(self.lags), doc="The number of lags.")

    def _ensure_device(self, like: Optional[Tensor] = None) -> torch.device:
        if self._state is not None:
            return self._state["pairs"].device
        dev = _stream.need_gpu("CodeDynamics", self.device or (like.device if like is not None else None))
        L = self.n_lags
        self._state = {"pairs": torch.zeros(L, 3, dtype=torch.int64, device=dev),
                       "sim_q": torch.zeros(L, 3, dtype=torch.int64, device=dev),
                       "sq_q": torch.zeros(L, 3, dtype=torch.int64, device=dev),
                       "hist": torch.zeros(L, 3, N.DYN_BINS, dtype=torch.int64, device=dev),
                       "total_rows": torch.zeros(1, dtype=torch.int64, device=dev)}
        self.device = self._state["pairs"].device  # (with its index: "cuda" names the current device)
        if self.weights is not None:
            self.weights = self.weights.to(self.device)
        return self.device

    pairs = _stream.state_property("pairs", "``[n_lags, 3]`` int64: the pairs within a label, across labels, otherwise.")
    sim_q = _stream.state_property("sim_q", "``[n_lags, 3]`` int64: the sum of llrint(similarity 2^30).")
    sq_q = _stream.state_property("sq_q", "``[n_lags, 3]`` int64: the sum of (llrint(similarity 2^30) >> 15)^2.")
    hist = _stream.state_property("hist", "``[n_lags, 3, 64]`` int64: the pairs by similarity, 64 equal bins over [0, 1].")
    total_rows = _stream.state_property("total_rows", "``[1]`` int64: the frames seen, padding excluded.")

    def update(self, code, labels: Optional[Tensor] = None, segments: Optional[Tensor] = None,
               frame_mask: Optional[Tensor] = None, return_similarity: bool = False) -> Optional[Tensor]:
        """One batch of whole utterances.  ``code = (values, indices)`` ``[n_utt, T, k]`` (with ``labels [n_utt, T]``), or
        flat ``[rows, k]`` with ``segments [rows]`` (and ``labels [rows]``).  ``labels``: an integer per frame, < 0 for
        "unlabelled"; None: every pair counts as unlabelled.  With ``return_similarity`` the ``[..., n_lags]`` matrix of
        the batch is returned as well; without it, it is never written."""
        also = () if labels is None else ((labels, "labels"),)
        vals, idx, k = _stream.compact_code(code, "code", N.DYN_MAX_K, also=also)
        dev = self._ensure_device(vals)
        if vals.device != dev or (labels is not None and labels.device != dev):
            raise N.WsaeError(f"the code is on {vals.device}" + ("" if labels is None else f" and the labels on {labels.device}")
                              + f", the tracker on {dev}")
        form = _stream.take_form(self, vals)
        seg, _ = _stream.frame_segments(vals, segments, frame_mask, dev)
        rows = seg.shape[0]
        lab = None
        if labels is not None:
            _stream.check_frame_labels(vals, labels)
            lab = torch.clamp(labels.detach().reshape(-1).to(torch.int64), min=-1, max=2 ** 31 - 1).to(torch.int32).contiguous()
        _stream.check_row_bound(self, rows)
        self._form = form
        sim = torch.empty(rows, self.n_lags, dtype=torch.float32, device=dev) if return_similarity else None
        if rows:
            v, i = _stream.flat_code(vals, idx, k)
            _dyn_call(v, i, k, self.hidden, seg, self.weights, lab, self.lags, METRICS[self.metric], sim, self._state, self)
        self._submitted += rows
        return None if sim is None else sim.reshape(*vals.shape[:-1], self.n_lags)

    def _same_kind(self, other: "CodeDynamics") -> bool:
        if (self.hidden, self.lags, self.metric) != (other.hidden, other.lags, other.metric):
            return False
        if (self.weights is None) != (other.weights is None):
            return False
        return self.weights is None or torch.equal(self.weights.cpu().view(torch.int32), other.weights.cpu().view(torch.int32))

    def merge(self, other: "CodeDynamics") -> None:
        """Add the state of a tracker of the same kind (size, lags, metric, weights bit for bit) over other utterances."""
        if not self._same_kind(other):
            raise ValueError("merge needs two trackers with the same size, lags, metric and weights")
        _stream.check_row_bound(self, other._submitted, merging=True)
        if other._state is not None:
            dev = self._ensure_device(other._state["pairs"])
            for name, t in other._state.items():
                self._state[name] += t.to(dev)
        self._form = self._form or other._form
        self._submitted += other._submitted

    def summary(self) -> DynamicsSummary:
        """The per-lag summary, float64 from the integers (``summarize_state``)."""
        self._ensure_device()
        return summarize_state(self.lags, self._state)

    def save(self, path) -> None:
        torch.save({"hidden": self.hidden, "lags": list(self.lags), "metric": self.metric,
                    "weights": None if self.weights is None else self.weights.cpu(), "form": self._form,
                    "submitted": self._submitted, "state": _stream.state_to_cpu(self)}, Path(path))

    @classmethod
    def load(cls, path, device=None) -> "CodeDynamics":
        data = torch.load(Path(path), map_location="cpu", weights_only=True)
        d = cls(tuple(data["lags"]), data["metric"], data["weights"], device=device, hidden=data["hidden"])
        _stream.state_from_saved(d, data["state"])
        d._form, d._submitted = data["form"], int(data["submitted"])
        return d


def collect_code_dynamics(model, utterances, lags: Sequence[int] = (1,), metric: str = "cosine",
                          weights: Optional[Tensor] = None, device="cuda") -> CodeDynamics:
    """The code dynamics over a dataset of utterances.  Every item is ``x [n_utt, T, D]``, ``(x, frame_mask)``,
    ``(x, labels)`` or ``(x, labels, frame_mask)``; in a pair, an integer tensor is ``labels`` and a bool or floating one
    the mask.  The module must offer ``encode_compact`` (TopK and BatchTopK SAEs; a ReLU SAE's code is dense:
    ``TypeError``) and is run in eval mode; its previous mode is restored."""
    with _stream.encoding(model, hint="code dynamics are for TopK-family codes"):
        dyn = CodeDynamics(lags, metric, weights, device=device, hidden=model.hidden_dim)
        for item in utterances:
            labels = mask = None
            if isinstance(item, (tuple, list)):
                if len(item) == 3:
                    x, labels, mask = item
                elif len(item) == 2:
                    x, second = item
                    if second is not None and (second.is_floating_point() or second.dtype == torch.bool):
                        mask = second
                    else:
                        labels = second
                else:
                    raise ValueError("an item must be x [n_utt, T, D], (x, frame_mask), (x, labels) or (x, labels, frame_mask)")
            else:
                x = item
            if x.dim() != 3:
                raise ValueError(f"an utterance batch must be [n_utt, T, D], got {tuple(x.shape)}")
            dyn.update(_stream.utterance_code(model, x, device), None if labels is None else labels.to(device),
                       frame_mask=None if mask is None else mask.to(device))
    return dyn


# ---- boundaries ---------------------------------------------------------------------------------------------------------------
def boundaries_from_labels(labels: Tensor, segments: Optional[Tensor] = None, frame_mask: Optional[Tensor] = None) -> Tensor:
    """uint8 flags in the shape of ``labels`` (``[..., T]``, every leading index an utterance, or ``[rows]`` with
    ``segments``): 1 at t where the label changes between t and t + 1, both frames are labelled (>= 0) and both lie in the
    same stretch (same utterance, neither masked)."""
    if labels.is_floating_point() or labels.dtype == torch.bool or labels.dim() < 1:
        raise ValueError(f"labels must hold one integer per frame, got {tuple(labels.shape)} {labels.dtype}")
    lab = labels.detach().to(torch.int64)
    ok = lab >= 0
    if frame_mask is not None:
        if frame_mask.shape != labels.shape:
            raise ValueError(f"frame_mask {tuple(frame_mask.shape)} must have the shape {tuple(labels.shape)} of the labels")
        ok = ok & (frame_mask.to(lab.device) != 0)
    if segments is not None:
        if labels.dim() != 1 or segments.shape != labels.shape:
            raise ValueError("segments go with flat labels [rows] of the same length")
        seg = segments.to(lab.device)
        ok = ok & (seg >= 0)
    out = torch.zeros(lab.shape, dtype=torch.uint8, device=lab.device)
    change = (lab[..., 1:] != lab[..., :-1]) & ok[..., 1:] & ok[..., :-1]
    if segments is not None:
        change = change & (seg[1:] == seg[:-1])
    out[..., :-1] = change.to(torch.uint8)
    return out


class BoundaryCurve:
    """The score of a boundary curve at every threshold, on the host.  ``thresholds`` float32 ``[n]`` as given;
    ``n_pred``, ``n_hit`` int64 ``[n]``, ``n_ref``, ``n_peaks`` ints; ``precision`` hit / pred, ``recall`` hit / ref, ``f1``
    2 hit / (pred + ref), ``over_segmentation`` pred / ref - 1 (= R / P - 1), ``r_value`` 1 - (|r1| + |r2|) / 2 with
    r1 = sqrt((1 - R)^2 + OS^2) and r2 = (-OS + R - 1) / sqrt(2): float64 ``[n]``, NaN where a denominator is 0."""

    def __init__(self, thresholds: Tensor, n_pred: Tensor, n_hit: Tensor, n_ref: int, n_peaks: int, tolerance: int):
        self.thresholds, self.tolerance = thresholds.detach().cpu().to(torch.float32), int(tolerance)
        self.n_pred, self.n_hit = n_pred.detach().cpu().to(torch.int64), n_hit.detach().cpu().to(torch.int64)
        self.n_ref, self.n_peaks = int(n_ref), int(n_peaks)
        pred, hit, ref = self.n_pred.double(), self.n_hit.double(), float(self.n_ref)
        nan = torch.full_like(pred, float("nan"))
        self.precision = torch.where(pred > 0, hit / torch.where(pred > 0, pred, torch.ones_like(pred)), nan)
        self.recall = hit / ref if ref > 0 else nan.clone()
        self.f1 = torch.where(pred + ref > 0, 2 * hit / torch.clamp(pred + ref, min=1.0), nan)
        self.over_segmentation = pred / ref - 1 if ref > 0 else nan.clone()
        r1 = torch.sqrt((1 - self.recall) ** 2 + self.over_segmentation ** 2)
        r2 = (-self.over_segmentation + self.recall - 1) / math.sqrt(2)
        self.r_value = 1 - (r1.abs() + r2.abs()) / 2

    def best(self, by: str = "f1") -> dict:
        """The threshold with the largest ``by`` (``"f1"`` or ``"r_value"``; the first of equals, NaN never wins) as
        ``{"index", "threshold", "precision", "recall", "f1", "over_segmentation", "r_value", "n_pred", "n_hit"}``."""
        if by not in ("f1", "r_value"):
            raise ValueError(f"by must be 'f1' or 'r_value', got {by!r}")
        score = getattr(self, by)
        if bool(torch.isnan(score).all()):
            raise ValueError(f"no threshold has a {by}: the curve has no references or no predictions")
        i = int(torch.where(torch.isnan(score), torch.full_like(score, float("-inf")), score).argmax())
        out = {"index": i, "threshold": float(self.thresholds[i]), "n_pred": int(self.n_pred[i]), "n_hit": int(self.n_hit[i])}
        for name in ("precision", "recall", "f1", "over_segmentation", "r_value"):
            out[name] = float(getattr(self, name)[i])
        return out


def _flat_rows(t: Tensor, name: str, shape) -> Tensor:
    require_device_tensor(t, name)
    if t.shape != shape:
        raise ValueError(f"{name} {tuple(t.shape)} must have the shape {tuple(shape)} of the novelty curve")
    return t.detach().reshape(-1)


class BoundaryScorer:
    """``boundary_curve`` over a dataset in pieces: ``update`` adds the counts of a batch of whole utterances, ``curve``
    reads them.  ``thresholds``: 1..256 values in any order; ``tolerance``: 0..64 frames."""

    def __init__(self, thresholds, tolerance: int = 1, device=None):
        thr = torch.as_tensor(thresholds, dtype=torch.float32).detach().reshape(-1)
        if not 1 <= thr.numel() <= N.BOUNDARY_MAX_THR:
            raise ValueError(f"thresholds must hold 1..{N.BOUNDARY_MAX_THR} values, got {thr.numel()}")
        if not 0 <= int(tolerance) <= N.BOUNDARY_MAX_TOL:
            raise ValueError(f"tolerance must be in 0..{N.BOUNDARY_MAX_TOL} frames, got {tolerance}")
        self.thresholds, self.tolerance = thr.cpu().contiguous(), int(tolerance)
        self.device = torch.device(device) if device is not None else None
        self._state: Optional[dict] = None
        self._thr = None
        self._ws = None

    def _ensure_device(self, like: Optional[Tensor] = None) -> torch.device:
        if self._state is not None:
            return self._state["n_pred"].device
        dev = _stream.need_gpu("BoundaryScorer", self.device or (like.device if like is not None else None))
        n = self.thresholds.numel()
        self._state = {"n_pred": torch.zeros(n, dtype=torch.int64, device=dev), "n_hit": torch.zeros(n, dtype=torch.int64, device=dev),
                       "n_ref": torch.zeros(1, dtype=torch.int64, device=dev), "n_peaks": torch.zeros(1, dtype=torch.int64, device=dev)}
        self.device = self._state["n_pred"].device
        self._thr = self.thresholds.to(self.device)
        return self.device

    n_pred = _stream.state_property("n_pred", "``[n_thr]`` int64: the predictions at every threshold.")
    n_hit = _stream.state_property("n_hit", "``[n_thr]`` int64: the hits at every threshold.")
    n_ref = _stream.state_property("n_ref", "``[1]`` int64: the reference boundaries.")
    n_peaks = _stream.state_property("n_peaks", "``[1]`` int64: the local maxima of the curve.")

    def update(self, novelty: Tensor, reference: Optional[Tensor] = None, segments: Optional[Tensor] = None,
               frame_mask: Optional[Tensor] = None, return_peaks: bool = False) -> Optional[Tensor]:
        """One batch of whole utterances: ``novelty`` float ``[..., T]`` (every leading index an utterance) or ``[rows]``
        with ``segments`` (None: one utterance), NaN = undefined; ``reference`` flags of the same shape (nonzero = a
        boundary between t and t + 1; None: none).  With ``return_peaks`` the uint8 mask of the local maxima."""
        require_device_tensor(novelty, "novelty")
        if novelty.dim() < 1 or not novelty.is_floating_point():
            raise ValueError(f"novelty must be a floating [..., T] or [rows] tensor, got {tuple(novelty.shape)} {novelty.dtype}")
        dev = self._ensure_device(novelty)
        if novelty.device != dev:
            raise N.WsaeError(f"the novelty curve is on {novelty.device}, the scorer on {dev}")
        nov = novelty.detach().reshape(-1).to(torch.float32).contiguous()
        rows = nov.shape[0]
        ref = None
        if reference is not None:
            ref = (_flat_rows(reference, "reference", novelty.shape).to(dev) != 0).to(torch.uint8).contiguous()
        as_code = novelty.reshape(-1, novelty.shape[-1], 1) if novelty.dim() > 1 else novelty.reshape(-1, 1)
        if novelty.dim() == 1 and segments is None and frame_mask is None:
            seg = None
        else:
            if novelty.dim() == 1 and segments is None:
                segments = torch.zeros(rows, dtype=torch.int32, device=dev)
            seg = _stream.frame_segments(as_code, segments, frame_mask, dev)[0]
        peaks = torch.empty(rows, dtype=torch.uint8, device=dev) if return_peaks else None
        if rows:
            if rows > _stream.MAX_ROWS:
                raise N.WsaeError(f"BoundaryScorer: {rows} frames in one call exceed {_stream.MAX_ROWS}")
            lib, st = N.lib(), self._state
            need = lib.wsae_boundary_workspace_bytes(rows, self._thr.numel(), self.tolerance)
            ws = _stream.workspace(self, need, dev)
            with torch.cuda.device(dev):
                N.check(lib.wsae_boundary_score(nov.data_ptr(), N.ptr(seg), N.ptr(ref), rows, self._thr.data_ptr(), self._thr.numel(),
                                                self.tolerance, st["n_pred"].data_ptr(), st["n_hit"].data_ptr(),
                                                st["n_ref"].data_ptr(), st["n_peaks"].data_ptr(), N.ptr(peaks), ws.data_ptr(), need,
                                                torch.cuda.current_stream(dev).cuda_stream), "wsae_boundary_score")
        return None if peaks is None else peaks.reshape(novelty.shape)

    def merge(self, other: "BoundaryScorer") -> None:
        """Add the counts of a scorer with the same thresholds (bit for bit) and tolerance."""
        if self.tolerance != other.tolerance or not torch.equal(self.thresholds.view(torch.int32), other.thresholds.view(torch.int32)):
            raise ValueError("merge needs two scorers with the same thresholds and tolerance")
        if other._state is not None:
            dev = self._ensure_device(other._state["n_pred"])
            for name, t in other._state.items():
                self._state[name] += t.to(dev)

    def curve(self) -> BoundaryCurve:
        self._ensure_device()
        st = self._state
        return BoundaryCurve(self.thresholds, st["n_pred"], st["n_hit"], int(st["n_ref"].item()), int(st["n_peaks"].item()),
                             self.tolerance)


def boundary_curve(novelty: Tensor, reference: Tensor, thresholds, tolerance: int = 1, segments: Optional[Tensor] = None,
                   frame_mask: Optional[Tensor] = None) -> BoundaryCurve:
    """Precision, recall, F1, over-segmentation and R-value of the peaks of ``novelty`` against the ``reference`` flags at
    every threshold (``BoundaryScorer`` in one call): a peak is a frame whose value exceeds its left neighbour and is no
    less than its right one, a prediction a peak at or above the threshold, and predictions and references of an
    utterance are matched greedily one to one in time order within ``tolerance`` frames."""
    scorer = BoundaryScorer(thresholds, tolerance)
    scorer.update(novelty, reference, segments=segments, frame_mask=frame_mask)
    return scorer.curve()


def detect_boundaries(novelty: Tensor, threshold: float, segments: Optional[Tensor] = None,
                      frame_mask: Optional[Tensor] = None) -> Tensor:
    """bool mask in the shape of ``novelty``: the peaks of the curve (``boundary_curve``) at or above ``threshold``."""
    scorer = BoundaryScorer([float(threshold)], 0)
    peaks = scorer.update(novelty, None, segments=segments, frame_mask=frame_mask, return_peaks=True)
    return (peaks != 0) & (novelty.detach() >= float(threshold))
