"""Label association: which feature detects which class of a per-frame label - phoneme, word
position, speaker, language token - how well, at which activation threshold and how many frames early or late?

``LabelAssociation`` keeps integer counts ``cnt [feature, lag, class, value stratum]`` and ``pair_rows [lag, class]``,
taken in one pass from the compact ``(values, indices)`` code and an integer label per frame (``wsae_label_update`` - the
dense ``[frames, H]`` matrix never exists).  The value strata come from per-feature edges fixed at construction
(``ActivationProfile.quantile_edges``), so the single-feature probe "feature >= threshold" can be read at every edge:
``scores`` gives precision, recall, F1, Jaccard, phi, mutual information and AUROC per (feature, class), each at the best
threshold and the best lag, in float64 from the integers.  The state does not depend on the order of the batches, on the
grouping of whole utterances into batches or on the launch geometry, and the states of two shards add.

Out of scope: several label tiers per tracker (use one tracker each), soft or multi-label frames, significance or
permutation nulls, probes over more than one feature, plots, dense / ReLU codes.
"""

from __future__ import annotations

import math
from pathlib import Path
from typing import Dict, NamedTuple, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor

from .. import _native as N
from . import _stream
from .profile import ActivationProfile

METRICS = ("precision", "recall", "f1", "jaccard", "phi", "mi", "auroc")


class LabelScores(NamedTuple):
    """Per (feature of the window, class), ``[f_cols, C]``.  ``score`` float64: the metric at the best threshold (and the
    best lag for ``lag="best"``), NaN where no cell qualifies; ``threshold_index`` int64 (0: "active", t >= 1: value >=
    edge t - 1); ``threshold`` float32 (0 for t = 0, else the edge); ``lag`` int64; ``tp``, ``fires``, ``positives`` int64:
    the frames on which the feature was at or above the threshold and the class present, the feature at or above the
    threshold, the class present - all at the winning (threshold, lag)."""

    score: Tensor
    threshold_index: Tensor
    threshold: Tensor
    lag: Tensor
    tp: Tensor
    fires: Tensor
    positives: Tensor


class BestLabels(NamedTuple):
    """Per feature of the window, ``[f_cols]``: ``label`` int64, the class with the best score (-1 where no class
    qualifies; ties go to the lower class), and that cell of ``LabelScores``."""

    label: Tensor
    score: Tensor
    threshold_index: Tensor
    threshold: Tensor
    lag: Tensor
    tp: Tensor
    fires: Tensor
    positives: Tensor


def _ratio(num: Tensor, den: Tensor) -> Tensor:
    """num / den in float64, NaN where den == 0."""
    num, den = num.double(), den.double()
    return torch.where(den != 0, num / torch.where(den != 0, den, torch.ones_like(den)), torch.full_like(den, float("nan")))


def _plogp(n: Tensor, row: Tensor, col: Tensor, total: Tensor) -> Tensor:
    """n / N log2(n N / (row col)) of one cell of a 2 x 2 table, 0 where n == 0."""
    n, row, col = n.double(), row.double(), col.double()
    ok = n > 0
    one = torch.ones_like(n)
    arg = torch.where(ok, n * total / (torch.where(ok, row, one) * torch.where(ok, col, one)), one)
    return torch.where(ok, n / total * torch.log2(arg), torch.zeros_like(n))


def threshold_counts(cnt_l: Tensor, pair_l: Tensor):
    """``(TP [F, C, S], A [F, 1, S], P [1, C, 1], N)`` as int64 from the counts of one lag, ``cnt_l [F, C, S]`` and
    ``pair_l [C]``: TP[f, c, t] = sum over s >= t of cnt, A = sum over c of TP, P = pair_l, N = sum of P."""
    c = cnt_l.to(torch.int64)
    tp = c.flip(2).cumsum(2).flip(2)
    p = pair_l.to(torch.int64)
    return tp, tp.sum(1, keepdim=True), p[None, :, None], p.sum()


def metric_table(cnt_l: Tensor, pair_l: Tensor, metric: str) -> Tensor:
    """``[F, C, S]`` float64: ``metric`` (not "auroc") of the detector "feature f at threshold t" for class c at one lag,
    from integer state (any device).  NaN where a denominator is 0."""
    tp, a, p, n = threshold_counts(cnt_l, pair_l)
    if metric == "precision":
        return _ratio(tp, a.expand_as(tp))
    if metric == "recall":
        return _ratio(tp, p.expand_as(tp))
    if metric == "f1":
        return _ratio(2 * tp, a + p)
    if metric == "jaccard":
        return _ratio(tp, a + p - tp)
    fp, fn = a - tp, p - tp
    tn = n - a - fn
    if metric == "phi":
        den = torch.sqrt((a * (n - a)).double() * (p * (n - p)).double())
        return _ratio(tp * tn - fp * fn, den)
    if metric == "mi":
        total = n.double()
        mi = (_plogp(tp, a, p, total) + _plogp(fp, a, n - p, total) + _plogp(fn, n - a, p, total)
              + _plogp(tn, n - a, n - p, total))
        return torch.where(n > 0, mi, torch.full_like(mi, float("nan")))
    raise ValueError(f"metric must be one of {METRICS}, got {metric!r}")


def auroc_table(cnt_l: Tensor, pair_l: Tensor) -> Tensor:
    """``[F, C]`` float64: the area under the ROC curve of feature f's activation as a score for class c at one lag.  The
    ordered levels are inactive < stratum 0 < ... < stratum S - 1; per level pos = cnt[f, c, s] and neg = the other
    classes' counts, the inactive level holds the remainders of P and N - P; the area is the sum over levels of
    pos (neg_below + neg / 2) over P (N - P): ties count half.  NaN where P (N - P) == 0."""
    pos = cnt_l.to(torch.int64)
    neg = pos.sum(1, keepdim=True) - pos
    p = pair_l.to(torch.int64)[None, :]
    n = p.sum()
    pos0, neg0 = p - pos.sum(2), (n - p) - neg.sum(2)
    below = neg0[:, :, None] + neg.cumsum(2) - neg  # the negatives on lower levels
    twice = pos0 * neg0 + (pos * (2 * below + neg)).sum(2)  # twice the numerator: an integer
    return _ratio(twice, 2 * (p * (n - p)).expand_as(twice))


class LabelAssociation:
    """Feature-by-class counts of a compact code against an integer label per frame, over a stream of utterances.

    ``edges [f_cols, S - 1]`` float32, ascending per feature (None: one stratum), fixed at construction: an activation
    ``v`` of feature f falls into the stratum numbered by the count of f's edges that are ``<= v``.  ``lags=(lo, hi)``:
    the label is read ``lo .. hi`` frames after the activation (-1024 <= lo <= hi <= 1024, at most 16 lags), never across
    an utterance.  ``f_window=(f_lo, f_cols)``: keep only the features ``f_lo .. f_lo + f_cols - 1``.  A label outside
    ``[0, n_classes)`` (-1 for "unlabelled") drops that frame as a label and nothing else.  The state lives on the device
    of the first update (or ``device``); ``ValueError`` when it would exceed ``max_state_bytes``."""

    def __init__(self, hidden: int, n_classes: int, edges: Optional[Tensor] = None, *, lags: Tuple[int, int] = (0, 0),
                 f_window: Optional[Tuple[int, int]] = None, device=None, max_state_bytes: int = 2 ** 31):
        self.hidden, self.n_classes = int(hidden), int(n_classes)
        if self.hidden < 1:
            raise ValueError(f"hidden must be positive, got {hidden}")
        if not 1 <= self.n_classes <= N.LABEL_MAX_CLASSES:
            raise ValueError(f"n_classes must be in 1..{N.LABEL_MAX_CLASSES}, got {n_classes}")
        self.f_lo, self.f_cols = _stream.feature_window(f_window, self.hidden)
        self.lag_lo, self.lag_hi = int(lags[0]), int(lags[1])
        if not (-1024 <= self.lag_lo <= self.lag_hi <= 1024 and self.lag_hi - self.lag_lo + 1 <= N.LABEL_MAX_LAGS):
            raise ValueError(f"lags must satisfy -1024 <= lo <= hi <= 1024 with at most {N.LABEL_MAX_LAGS} lags, got {lags}")
        if edges is not None:
            if not isinstance(edges, Tensor) or edges.dim() != 2 or edges.shape[0] != self.f_cols:
                raise ValueError(f"edges must be a [{self.f_cols}, n_strata - 1] tensor, got "
                                 f"{tuple(edges.shape) if isinstance(edges, Tensor) else type(edges).__name__}")
            if not 1 <= edges.shape[1] + 1 <= N.LABEL_MAX_STRATA:
                raise ValueError(f"n_strata must be in 1..{N.LABEL_MAX_STRATA}, got {edges.shape[1] + 1}")
            edges = edges.detach().to(torch.float32).contiguous()
            if edges.shape[1] == 0:
                edges = None
        self.n_strata = 1 if edges is None else edges.shape[1] + 1
        self.edges = edges
        need = 4 * self.f_cols * self.n_lags * self.n_classes * self.n_strata + 8 * self.n_lags * self.n_classes
        if need > int(max_state_bytes):
            raise ValueError(f"the state [{self.f_cols}, {self.n_lags}, {self.n_classes}, {self.n_strata}] int32 takes {need} "
                             f"bytes, more than max_state_bytes = {max_state_bytes}: narrow the window, the lags or the strata")
        self.device = torch.device(device) if device is not None else None
        self._state: Optional[dict] = None
        self._form: Optional[str] = None  # "numbered" ([n_utt, T, k] updates) or "flat" (rows with segments)
        self._submitted = 0  # rows handed to update so far, padding included (host-side bound of the int32 state)

    n_lags = property(lambda self: self.lag_hi - self.lag_lo + 1, doc="The number of lags L.")

    # ---- state ----------------------------------------------------------------------------------
    def _ensure_device(self, like: Optional[Tensor] = None) -> torch.device:
        if self._state is not None:
            return self._state["cnt"].device
        dev = _stream.need_gpu("LabelAssociation", self.device or (like.device if like is not None else None))
        self._state = {"cnt": torch.zeros(self.f_cols, self.n_lags, self.n_classes, self.n_strata, dtype=torch.int32, device=dev),
                       "pair_rows": torch.zeros(self.n_lags, self.n_classes, dtype=torch.int64, device=dev)}
        if self.edges is not None:
            self.edges = self.edges.to(dev)
        self.device = self._state["cnt"].device
        return self.device

    cnt = _stream.state_property(
        "cnt", "``[f_cols, L, C, S]`` int32: frames on which the feature fired in the stratum, by the label `lag` later.")
    pair_rows = _stream.state_property("pair_rows", "``[L, C]`` int64: the labelled frame pairs of each lag.")

    # ---- accumulation ---------------------------------------------------------------------------
    def update(self, code, labels: Tensor, frame_mask: Optional[Tensor] = None, segments: Optional[Tensor] = None) -> None:
        """One batch of whole utterances.  ``code = (values, indices)`` ``[n_utt, T, k]`` with ``labels [n_utt, T]``, or
        flat ``[rows, k]`` with ``labels [rows]`` and ``segments [rows]`` (the utterance of every row; < 0: padding).
        Frames with ``frame_mask == 0`` are padding: they fire nothing and label nothing."""
        vals, idx, k = _stream.compact_code(code, "code", N.LABEL_MAX_K, also=((labels, "labels"),))
        dev = self._ensure_device(vals)
        if vals.device != dev or labels.device != dev:
            raise N.WsaeError(f"the code is on {vals.device} and the labels on {labels.device}, the tracker on {dev}")
        form = _stream.take_form(self, vals)
        seg, _ = _stream.frame_segments(vals, segments, frame_mask, dev)
        rows = seg.shape[0]
        _stream.check_frame_labels(vals, labels)
        _stream.check_row_bound(self, rows)  # (a cell of cnt is int32 and takes at most one count per frame)
        self._form = form
        if rows == 0:
            return
        v, i = _stream.flat_code(vals, idx, k)
        lab = _stream.frame_labels(vals, labels, self.n_classes)
        st = self._state
        with torch.cuda.device(dev):
            N.check(N.lib().wsae_label_update(
                v.data_ptr(), i.data_ptr(), k, self.hidden, seg.data_ptr(), lab.data_ptr(), rows, self.n_classes, self.lag_lo,
                self.lag_hi, self.f_lo, self.f_cols, N.ptr(self.edges), self.n_strata, st["cnt"].data_ptr(),
                st["pair_rows"].data_ptr(), None, 0, torch.cuda.current_stream(dev).cuda_stream), "wsae_label_update")
        self._submitted += rows

    def _same_kind(self, other: "LabelAssociation") -> bool:
        mine = (self.hidden, self.f_lo, self.f_cols, self.n_classes, self.lag_lo, self.lag_hi, self.n_strata)
        if mine != (other.hidden, other.f_lo, other.f_cols, other.n_classes, other.lag_lo, other.lag_hi, other.n_strata):
            return False
        if self.edges is None:
            return True
        # bit for bit, so that the NaN edges of a silent feature compare equal
        return torch.equal(self.edges.cpu().view(torch.int32), other.edges.cpu().view(torch.int32))

    def merge(self, other: "LabelAssociation") -> None:
        """Add the state of a tracker of the same kind (size, window, classes, lags, edges bit for bit) over other
        utterances: an integer add."""
        if not self._same_kind(other):
            raise ValueError("merge needs two trackers with the same size, window, classes, lags and edges")
        _stream.check_row_bound(self, other._submitted, merging=True)
        if other._state is not None:
            dev = self._ensure_device(other._state["cnt"])
            for name, t in other._state.items():
                self._state[name] += t.to(dev)
        self._form = self._form or other._form
        self._submitted += other._submitted

    # ---- reading --------------------------------------------------------------------------------
    def _lag_order(self, lag) -> list:
        """The lag indices to search, in the order of preference among equal scores: nearer 0 first, then the lower."""
        if isinstance(lag, str):
            if lag != "best":
                raise ValueError(f"lag must be an int or 'best', got {lag!r}")
            return sorted(range(self.n_lags), key=lambda li: (abs(self.lag_lo + li), self.lag_lo + li))
        if not self.lag_lo <= int(lag) <= self.lag_hi:
            raise ValueError(f"lag {lag} is not among the lags {self.lag_lo} .. {self.lag_hi} of this tracker")
        return [int(lag) - self.lag_lo]

    def scores(self, metric: str = "f1", lag: Union[int, str] = 0, min_count: int = 1) -> LabelScores:
        """The ``metric`` of every (feature, class) at its best threshold, at ``lag`` or (``"best"``) the best lag.

        At one lag and threshold index t (t = 0: "active", t >= 1: value >= edge t - 1): TP[f, c, t] = the sum over s >= t
        of cnt, A[f, t] = the sum over c of TP, P[c] = pair_rows, N = the sum of P, FP = A - TP, FN = P - TP,
        TN = N - A - FN.  ``precision`` TP / A, ``recall`` TP / P, ``f1`` 2 TP / (A + P), ``jaccard`` TP / (A + P - TP),
        ``phi`` (TP TN - FP FN) / sqrt(A (N - A) P (N - P)), ``mi`` the mutual information of the 2 x 2 table in bits
        (0 log 0 = 0), ``auroc`` (no threshold: index 0) as ``auroc_table``.  NaN where a denominator is 0.  A cell with
        TP < ``min_count`` scores NaN and never wins; ties go to the lower threshold, then the lag nearer 0, then the
        lower lag."""
        if metric not in METRICS:
            raise ValueError(f"metric must be one of {METRICS}, got {metric!r}")
        order = self._lag_order(lag)
        dev = self._ensure_device()
        cnt, pair_rows = self._state["cnt"], self._state["pair_rows"]
        best = None
        for li in order:
            tp, a, p, _ = threshold_counts(cnt[:, li], pair_rows[li])
            if metric == "auroc":
                table = auroc_table(cnt[:, li], pair_rows[li])[:, :, None]
                tp, a = tp[:, :, :1], a[:, :, :1]
            else:
                table = metric_table(cnt[:, li], pair_rows[li], metric)
            table = torch.where(tp >= int(min_count), table, torch.full_like(table, float("nan")))
            key = torch.where(torch.isnan(table), torch.full_like(table, float("-inf")), table)
            t = key.argmax(2, keepdim=True)  # (the first of equal maxima: the lower threshold)
            here = (table.gather(2, t)[:, :, 0], key.gather(2, t)[:, :, 0], t[:, :, 0],
                    torch.full_like(t[:, :, 0], self.lag_lo + li), tp.gather(2, t)[:, :, 0],
                    a.expand_as(tp).gather(2, t)[:, :, 0], p.expand_as(tp)[:, :, 0])
            if best is None:
                best = here
            else:  # (a better score, or an equal one at a lower threshold; otherwise the earlier lag of the order stays)
                better = (here[1] > best[1]) | ((here[1] == best[1]) & (here[2] < best[2]))
                best = tuple(torch.where(better, h, b) for h, b in zip(here, best))
        score, _, t, lag_of, tp, fires, positives = best
        if self.edges is None:
            thr = torch.zeros(t.shape, dtype=torch.float32, device=dev)
        else:
            padded = torch.cat([torch.zeros(self.f_cols, 1, dtype=torch.float32, device=dev), self.edges], dim=1)
            thr = padded.gather(1, t)
        return LabelScores(score=score, threshold_index=t, threshold=thr, lag=lag_of, tp=tp, fires=fires, positives=positives)

    # ---- persistence ----------------------------------------------------------------------------
    def save(self, path) -> None:
        torch.save({"hidden": self.hidden, "n_classes": self.n_classes, "lags": [self.lag_lo, self.lag_hi],
                    "f_window": [self.f_lo, self.f_cols], "edges": None if self.edges is None else self.edges.cpu(),
                    "form": self._form, "submitted": self._submitted, "state": _stream.state_to_cpu(self)}, Path(path))

    @classmethod
    def load(cls, path, device=None) -> "LabelAssociation":
        data = torch.load(Path(path), map_location="cpu", weights_only=True)
        a = cls(data["hidden"], data["n_classes"], data["edges"], lags=tuple(data["lags"]), f_window=tuple(data["f_window"]),
                device=device, max_state_bytes=2 ** 62)
        _stream.state_from_saved(a, data["state"])
        a._form, a._submitted = data["form"], int(data["submitted"])
        return a


def top_label_features(assoc: LabelAssociation, n: int = 20, metric: str = "f1", lag: Union[int, str] = 0,
                       min_count: int = 1) -> Tuple[Tensor, Tensor]:
    """Per class the ``n`` features with the best score (``LabelAssociation.scores``) as ``(features [C, n] int64,
    scores [C, n] float64)``, descending, ties to the lower index; features are indices in ``[0, hidden)``.  Only cells
    whose score is not NaN are candidates: where a class has fewer, the row ends in -1 / NaN."""
    sc = assoc.scores(metric, lag, min_count).score
    n = max(int(n), 0)
    feats = torch.full((assoc.n_classes, n), -1, dtype=torch.int64, device=sc.device)
    vals = torch.full((assoc.n_classes, n), float("nan"), dtype=torch.float64, device=sc.device)
    for c in range(assoc.n_classes):
        col = sc[:, c]
        order = _stream.rank_features(col, ~torch.isnan(col), n)
        feats[c, :order.numel()] = order + assoc.f_lo
        vals[c, :order.numel()] = col[order]
    return feats, vals


def best_labels(assoc: LabelAssociation, metric: str = "f1", lag: Union[int, str] = "best", min_count: int = 1) -> BestLabels:
    """Per feature of the window the class it detects best (``LabelAssociation.scores``; ties to the lower class)."""
    sc = assoc.scores(metric, lag, min_count)
    key = torch.where(torch.isnan(sc.score), torch.full_like(sc.score, float("-inf")), sc.score)
    c = key.argmax(1, keepdim=True)
    any_ok = ~torch.isnan(sc.score.gather(1, c)[:, 0])
    label = torch.where(any_ok, c[:, 0], torch.full_like(c[:, 0], -1))
    return BestLabels(label, *(field.gather(1, c)[:, 0] for field in sc))


def automated_labels(assoc: LabelAssociation, class_names: Sequence[str], metric: str = "f1", lag: Union[int, str] = "best",
                     min_count: int = 1, min_score: Optional[float] = None) -> Dict[int, dict]:
    """``{feature: {"label", "metric", "score", "threshold", "lag", "precision", "recall"}}`` for every feature of the
    window that has a best class (``best_labels``; with ``min_score``: a score of at least that): the shape of the
    reference's ``FeatureInterpretation.automated_labels``.  ``precision`` and ``recall`` are those of the winning
    (threshold, lag)."""
    if len(class_names) != assoc.n_classes:
        raise ValueError(f"class_names has {len(class_names)} names for {assoc.n_classes} classes")
    best = BestLabels(*(field.cpu() for field in best_labels(assoc, metric, lag, min_count)))
    out = {}
    for col in torch.nonzero(best.label >= 0)[:, 0].tolist():
        score = float(best.score[col])
        if min_score is not None and not score >= float(min_score):
            continue
        tp, fires, pos = int(best.tp[col]), int(best.fires[col]), int(best.positives[col])
        out[assoc.f_lo + col] = {"label": class_names[int(best.label[col])], "metric": metric, "score": score,
                                 "threshold": float(best.threshold[col]), "lag": int(best.lag[col]),
                                 "precision": tp / fires if fires else math.nan, "recall": tp / pos if pos else math.nan}
    return out


def collect_label_association(model, utterances, n_classes: int, profile_or_edges: Union[ActivationProfile, Tensor, None] = None,
                              *, n_strata: int = 8, lags: Tuple[int, int] = (0, 0), f_window: Optional[Tuple[int, int]] = None,
                              device="cuda", max_state_bytes: int = 2 ** 31) -> LabelAssociation:
    """The label association over a dataset of utterances.  Every item of ``utterances`` is ``(x [n_utt, T, D],
    labels [n_utt, T])`` or ``(x, labels, frame_mask [n_utt, T])``.  ``profile_or_edges`` is the profile of an earlier pass
    (``collect_activation_profile``), whose ``quantile_edges(n_strata)`` and window are taken, or a tensor of edges
    ``[f_cols, n_strata - 1]`` that goes with ``f_window`` (None: one stratum).  The module must offer ``encode_compact``
    (TopK and BatchTopK SAEs; a ReLU SAE's code is dense: ``TypeError``) and is run in eval mode; its previous mode is
    restored."""
    with _stream.encoding(model, hint="label association is for TopK-family codes"):
        if isinstance(profile_or_edges, ActivationProfile):
            if profile_or_edges.hidden != model.hidden_dim:
                raise ValueError(f"the profile has {profile_or_edges.hidden} features, the module {model.hidden_dim}")
            edges = profile_or_edges.quantile_edges(n_strata)
            f_window = (profile_or_edges.f_lo, profile_or_edges.f_cols)
        else:
            edges = profile_or_edges
        assoc = LabelAssociation(model.hidden_dim, n_classes, edges, lags=lags, f_window=f_window, device=device,
                                 max_state_bytes=max_state_bytes)
        for x, labels, mask in _stream.labelled_batches(utterances):
            assoc.update(_stream.utterance_code(model, x, device), labels.to(device),
                         frame_mask=None if mask is None else mask.to(device))
    return assoc
