"""Code clustering: do the frames fall into a few hundred discrete units, do the units line up
with phones, and which features define a unit?

``CodeKMeans`` runs Lloyd's k-means over the compact ``(values, indices)`` code.  Neither the dense ``[frames, H]`` code
nor a ``[frames, n_clusters]`` product exists: ``wsae_cluster_assign`` scores a frame against every centroid from the k
gathered rows of the transposed centroid matrix and keeps the winner, the runner-up and integer statistics, and
``wsae_cluster_accumulate`` adds every entry of the transposed plan (``wsae_probe_plan``) into the integer centroid sums
of its frame's cluster.  The sums are integers, so two fits of the same data agree bit for bit whatever the batching, and
the sums of two shards add (``merge_sums``).  ``metric="cosine"`` is spherical k-means (unit centroids, frames weighted by
the inverse of their norm), ``"euclidean"`` the plain one (the score is ``x . c - |c|^2 / 2``).

``ClusterScores`` turns a cluster-by-class contingency table into cluster purity, class (phone) purity, mutual
information, PNMI, NMI, V-measure and the adjusted Rand index; ``unit_sequences`` collapses the frame units of an
utterance into a unit string.

Out of scope: k-means++ and restarts, soft assignments, several GPUs beyond ``merge_sums``, label lags (the caller
shifts the labels), HMM or duration models on the unit strings.
"""

from __future__ import annotations

import math
from pathlib import Path
from typing import List, NamedTuple, Optional, Tuple

import torch
from torch import Tensor

from .. import _native as N
from . import _stream

Q_SCALE = float(2 ** 20)  # S_q and best_q count 2^-20
METRICS = ("cosine", "euclidean")


class IterationStats(NamedTuple):
    """``objective``: the mean quality of the assigned frames under the centroids they were assigned with (the cosine
    to the own centroid, or ``x . c - |c|^2 / 2``; larger is better); ``counts`` int64 ``[n_clusters]``; ``n_empty``:
    the clusters without a frame (re-seeded); ``n_changed``: the frames whose unit differs from the previous iteration
    (None where the batches of the two iterations do not line up)."""

    objective: float
    counts: Tensor
    n_empty: int
    n_changed: Optional[int]


class ClusterScores(NamedTuple):
    """The scores of a contingency table ``[clusters, classes]`` in float64.  ``cluster_purity``: the share of frames in
    the majority class of their cluster (the many-to-one accuracy, ``many_to_one``, is the same number); ``class_purity``
    (phone purity): the share of frames in the majority cluster of their class; ``mutual_information`` in nats;
    ``pnmi = I / H(class)``; ``nmi = 2 I / (H(cluster) + H(class))``; ``v_measure``: the harmonic mean of homogeneity and
    completeness; ``ari``: the adjusted Rand index; ``best_class`` int64 ``[clusters]``: the majority class of every
    cluster (the lowest at a tie); ``n_frames``: the table's total."""

    cluster_purity: float
    class_purity: float
    many_to_one: float
    mutual_information: float
    pnmi: float
    nmi: float
    v_measure: float
    ari: float
    best_class: Tensor
    n_frames: int


def cluster_scores(table) -> ClusterScores:
    """``ClusterScores`` of an integer table ``[clusters, classes]`` (``ValueError`` unless 2-D, non-negative and not
    all zero)."""
    t = torch.as_tensor(table).detach().cpu()
    if t.dim() != 2 or t.is_floating_point() or bool((t < 0).any()) or int(t.sum()) == 0:
        raise ValueError(f"a contingency table must be a non-negative integer [clusters, classes] tensor with a frame in it, "
                         f"got {tuple(t.shape)} {t.dtype}")
    t = t.to(torch.float64)
    n = t.sum()
    rows, cols = t.sum(1), t.sum(0)

    def entropy(m: Tensor) -> float:
        p = m[m > 0] / n
        return float(-(p * p.log()).sum())

    h_k, h_c = entropy(rows), entropy(cols)
    nz = t > 0
    mi = float((t[nz] / n * (t[nz] * n / torch.outer(rows, cols)[nz]).log()).sum())
    hom = 1.0 if h_c == 0 else mi / h_c
    com = 1.0 if h_k == 0 else mi / h_k
    comb2 = lambda x: x * (x - 1.0) / 2.0
    s_ij, s_a, s_b = float(comb2(t).sum()), float(comb2(rows).sum()), float(comb2(cols).sum())
    expected, max_index = s_a * s_b / float(comb2(n)) if float(n) > 1 else 0.0, 0.5 * (s_a + s_b)
    purity = float(t.max(1).values.sum() / n)
    return ClusterScores(cluster_purity=purity, class_purity=float(t.max(0).values.sum() / n), many_to_one=purity,
                         mutual_information=mi, pnmi=mi / h_c if h_c > 0 else math.nan,
                         nmi=2.0 * mi / (h_k + h_c) if h_k + h_c > 0 else math.nan,
                         v_measure=2.0 * hom * com / (hom + com) if hom + com > 0 else 0.0,
                         ari=(s_ij - expected) / (max_index - expected) if max_index != expected else 1.0,
                         best_class=t.argmax(1), n_frames=int(n))


def unit_sequences(assign: Tensor, segments: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """``(units, lengths, utterances)`` int64: the runs of consecutive equal units inside an utterance.  ``assign`` is
    ``[n_utt, T]`` (every row an utterance) or ``[rows]`` with ``segments [rows]``; frames with unit -1 (or a segment
    < 0) are dropped and end a run."""
    a = torch.as_tensor(assign).detach()
    if a.is_floating_point() or a.dtype == torch.bool or a.dim() not in (1, 2):
        raise ValueError(f"assign must hold one integer per frame as [n_utt, T] or [rows], got {tuple(a.shape)} {a.dtype}")
    if a.dim() == 2:
        if segments is not None:
            raise ValueError("an [n_utt, T] assignment numbers its utterances itself: pass segments only with a flat one")
        seg = torch.arange(a.shape[0], device=a.device)[:, None].expand_as(a).reshape(-1)
    else:
        if segments is None:
            raise ValueError("a flat [rows] assignment needs segments [rows]")
        seg = torch.as_tensor(segments).detach().reshape(-1).to(a.device)
        if seg.numel() != a.numel():
            raise ValueError(f"segments has {seg.numel()} ids for {a.numel()} rows")
    a, seg = a.reshape(-1).to(torch.int64), seg.to(torch.int64)
    valid = (a >= 0) & (seg >= 0)
    prev_ok = torch.zeros_like(valid)
    prev_ok[1:] = valid[:-1] & (a[1:] == a[:-1]) & (seg[1:] == seg[:-1])
    start = valid & ~prev_ok
    run = torch.cumsum(start.to(torch.int64), 0) - 1
    lengths = torch.bincount(run[valid], minlength=int(start.sum()))
    return a[start], lengths, seg[start]


class CodeKMeans:
    """k-means with ``n_clusters`` (1 .. 1024) centroids over the features ``features`` (a 1-D index tensor without
    duplicates; None: all ``hidden``) of a compact code.  ``n_classes > 0`` keeps the cluster-by-class contingency table
    of the frames that ``accumulate`` is given labels for."""

    def __init__(self, n_clusters: int, hidden: int, features: Optional[Tensor] = None, metric: str = "cosine", device=None,
                 seed: int = 0, n_classes: int = 0):
        self.n_clusters, self.hidden, self.seed, self.n_classes = int(n_clusters), int(hidden), int(seed), int(n_classes)
        if self.hidden < 1:
            raise ValueError(f"hidden must be positive, got {hidden}")
        if not 1 <= self.n_clusters <= N.CLUSTER_MAX:
            raise ValueError(f"n_clusters must be in 1..{N.CLUSTER_MAX}, got {n_clusters}")
        if not 0 <= self.n_classes <= N.CLUSTER_MAX:
            raise ValueError(f"n_classes must be in 0..{N.CLUSTER_MAX}, got {n_classes}")
        if metric not in METRICS:
            raise ValueError(f"metric must be one of {METRICS}, got {metric!r}")
        self.metric = metric
        self.feature_index, self._col_of = _stream.column_map(features, self.hidden)
        self._col_of_cpu = self._col_of
        self.n_cols = self.feature_index.numel()
        self.device = torch.device(device) if device is not None else None
        self._state: Optional[dict] = None
        self._ws: Optional[Tensor] = None
        self._seeded = False
        self._last = None            # (values, indices, assign, quality) of the last batch: the frames a re-seed draws from
        self._assigns: List[Tensor] = []  # the assignments of this iteration's batches, and of the previous one
        self._prev_assigns: Optional[List[Tensor]] = None
        self.last_contingency: Optional[Tensor] = None

    # ---- state ----------------------------------------------------------------------------------
    def _ensure_device(self, like: Optional[Tensor] = None) -> torch.device:
        if self._state is not None:
            return self.device
        dev = _stream.need_gpu("CodeKMeans", self.device or (like.device if like is not None else None))
        C, P = self.n_clusters, self.n_cols
        z = lambda *shape: torch.zeros(*shape, dtype=torch.int64, device=dev)
        self._state = {"Ct": torch.zeros(P, C, dtype=torch.float32, device=dev),
                       "bias": torch.zeros(C, dtype=torch.float32, device=dev), "S_q": z(P, C), "count": z(C), "best_q": z(C),
                       "contingency": z(C, self.n_classes) if self.n_classes else None, "totals": z(3)}
        dev = self._state["Ct"].device  # ("cuda" has become "cuda:0")
        self.feature_index = self.feature_index.to(dev)
        if self._col_of is not None:
            self._col_of = self._col_of.to(dev)
        self.device = dev
        return dev

    counts = _stream.state_property("count", "int64 [n_clusters]: the frames assigned to every cluster since the last step.")
    sums = _stream.state_property("S_q", "int64 [n_cols, n_clusters]: the centroid sums since the last step, in 2^-20.")
    contingency = _stream.state_property("contingency", "int64 [n_clusters, n_classes] since the last step (None without classes).")
    totals = _stream.state_property("totals", "int64 [3]: assigned frames, empty frames, labelled assigned frames.")

    @property
    def centroids(self) -> Tensor:
        """float32 ``[n_clusters, n_cols]``: column p belongs to feature ``feature_index[p]``."""
        return _stream.state_field(self, "Ct").t().contiguous()

    def _prepare(self, code, segments, frame_mask, labels):
        also = () if labels is None else ((labels, "labels"),)
        vals, idx, k = _stream.compact_code(code, "code", N.CLUSTER_MAX_K, also=also)
        dev = self._ensure_device(vals)
        if vals.device != dev:
            raise N.WsaeError(f"the code is on {vals.device}, the clustering on {dev}")
        seg, _ = _stream.frame_segments(vals, segments, frame_mask, dev)
        if seg.shape[0] > _stream.MAX_ROWS:
            raise N.WsaeError(f"CodeKMeans: {seg.shape[0]} frames in one batch exceed {_stream.MAX_ROWS}")
        lab = None
        if labels is not None:
            if not self.n_classes:
                raise ValueError("labels need a clustering made with n_classes > 0")
            lab = _stream.frame_labels(vals, labels, self.n_classes).to(dev)
        v, i = _stream.flat_code(vals, idx, k)
        return v, i, k, seg, lab

    def _assign(self, v, i, k, seg, lab, Ct, bias, normalize, with_state: bool):
        """One ``wsae_cluster_assign`` call -> ``(assign, best, second, inv_norm)``."""
        dev, rows, st = v.device, seg.shape[0], self._state
        out_i = torch.empty(rows, dtype=torch.int32, device=dev)
        best, second, inv = (torch.empty(rows, dtype=torch.float32, device=dev) for _ in range(3))
        C = Ct.shape[1]
        state = [st["count"], st["best_q"], st["contingency"] if lab is not None else None, st["totals"]] if with_state else [None] * 4
        with torch.cuda.device(dev):
            N.check(N.lib().wsae_cluster_assign(
                v.data_ptr(), i.data_ptr(), k, self.hidden, seg.data_ptr(), rows, N.ptr(self._col_of), self.n_cols, Ct.data_ptr(), C,
                N.ptr(bias), C, int(normalize), N.ptr(lab), self.n_classes if lab is not None else 0, out_i.data_ptr(),
                best.data_ptr(), second.data_ptr(), inv.data_ptr(), *(N.ptr(t) for t in state), None, 0,
                torch.cuda.current_stream(dev).cuda_stream), "wsae_cluster_assign")
        return out_i, best, second, inv

    def _row_centroid(self, v_row: Tensor, i_row: Tensor) -> Tensor:
        """float64 ``[n_cols]`` on the CPU: the frame as a dense row over the columns (first active entries only)."""
        x = torch.zeros(self.n_cols, dtype=torch.float64)
        seen = set()
        for val, f in zip(v_row.tolist(), i_row.tolist()):
            if not val > 0 or f in seen:
                continue
            seen.add(f)
            if 0 <= f < self.hidden:
                col = f if self._col_of_cpu is None else int(self._col_of_cpu[f])
                if col >= 0:
                    x[col] = val
        return x

    def _finish(self, c64: Tensor) -> Tensor:
        """float32 centroids from float64 ones ``[n_cols, m]``: unit columns for cosine (a zero column stays), one rounding."""
        if self.metric == "cosine":
            norm = (c64 * c64).sum(0).sqrt()
            c64 = c64 / torch.where(norm > 0, norm, torch.ones_like(norm))
        return c64.to(torch.float32)

    def _set_bias(self) -> None:
        st = self._state
        if self.metric == "euclidean":
            c = st["Ct"].double()
            st["bias"].copy_((-0.5 * (c * c).sum(0)).to(torch.float32))

    # ---- the centroids --------------------------------------------------------------------------
    def init_centroids(self, code=None, init="sample", segments: Optional[Tensor] = None,
                       frame_mask: Optional[Tensor] = None) -> None:
        """Seed the centroids.  ``init="sample"``: ``n_clusters`` distinct non-empty frames of ``code`` (the head of a
        permutation of the non-empty frames drawn with a generator seeded by ``seed``, in ascending frame order).
        ``init`` a tensor ``[n_clusters, n_cols]``: these centroids (for cosine they are divided by their norm).  The sums
        are cleared."""
        if isinstance(init, str):
            if init != "sample":
                raise ValueError(f"init must be \"sample\" or a [n_clusters, n_cols] tensor, got {init!r}")
            if code is None:
                raise ValueError("init=\"sample\" draws frames: pass a code")
            v, i, k, seg, _ = self._prepare(code, segments, frame_mask, None)
            dev = v.device
            probe = torch.zeros(self.n_cols, 1, dtype=torch.float32, device=dev)
            a, _, _, _ = self._assign(v, i, k, seg, None, probe, None, False, False) if seg.shape[0] else (seg, None, None, None)
            ok = torch.nonzero(a >= 0).reshape(-1).cpu()
            if ok.numel() < self.n_clusters:
                raise ValueError(f"the code holds {ok.numel()} non-empty frames for {self.n_clusters} clusters")
            perm = torch.randperm(ok.numel(), generator=torch.Generator().manual_seed(self.seed))[:self.n_clusters]
            rows = torch.sort(ok[perm]).values.to(dev)
            vr, ir = v[rows].cpu(), i[rows].cpu()
            c64 = torch.stack([self._row_centroid(vr[j], ir[j]) for j in range(self.n_clusters)], 1)
        else:
            c = torch.as_tensor(init).detach()
            if c.shape != (self.n_clusters, self.n_cols) or not c.is_floating_point() or not bool(torch.isfinite(c).all()):
                raise ValueError(f"centroids must be a finite floating [{self.n_clusters}, {self.n_cols}] tensor, got "
                                 f"{tuple(c.shape)} {c.dtype}")
            self._ensure_device(c if c.is_cuda else None)
            c64 = c.to(torch.float64).t().cpu()
        self._state["Ct"].copy_(self._finish(c64))
        self._set_bias()
        self._clear()
        self._prev_assigns = None
        self._seeded = True

    def _clear(self) -> None:
        for name in ("S_q", "count", "best_q", "contingency", "totals"):
            if self._state[name] is not None:
                self._state[name].zero_()
        self._assigns = []

    def accumulate(self, code, segments: Optional[Tensor] = None, frame_mask: Optional[Tensor] = None,
                   labels: Optional[Tensor] = None, _plan=None) -> Tensor:
        """Assign the frames of one batch of whole utterances under the current centroids and add them to the sums.
        ``code = (values, indices)`` ``[n_utt, T, k]``, or flat ``[rows, k]`` with ``segments [rows]``; frames with
        ``frame_mask == 0`` are padding; ``labels`` (one integer per frame) feed the contingency table.  Returns
        ``assign`` int32 ``[rows]``: the unit of every frame, -1 for padding and for frames without an active feature."""
        if not self._seeded:
            raise ValueError("CodeKMeans has no centroids: call init_centroids first")
        v, i, k, seg, lab = self._prepare(code, segments, frame_mask, labels)
        rows, dev, st = seg.shape[0], v.device, self._state
        if rows == 0:
            return torch.empty(0, dtype=torch.int32, device=dev)
        cosine = self.metric == "cosine"
        a, best, _, inv = self._assign(v, i, k, seg, lab, st["Ct"], None if cosine else st["bias"], cosine, True)
        col_ptr, t_row, t_val, n = _plan if _plan is not None else _stream.transposed_plan(self, v, i, k, seg, rows)
        with torch.cuda.device(dev):
            N.check(N.lib().wsae_cluster_accumulate(
                col_ptr.data_ptr(), N.ptr(t_row), N.ptr(t_val), min(n, t_row.numel()), self.n_cols, a.data_ptr(),
                inv.data_ptr() if cosine else None, rows, self.n_clusters, st["S_q"].data_ptr(), self.n_clusters, None, 0,
                torch.cuda.current_stream(dev).cuda_stream), "wsae_cluster_accumulate")
        quality = best * inv if cosine else best
        self._last = (v, i, a, torch.where(a >= 0, quality, torch.full_like(quality, float("inf"))))
        self._assigns.append(a)
        return a

    def step(self) -> IterationStats:
        """The new centroids from the integer sums: ``double(S_q) / (double(count) 2^20)``, for cosine divided by its
        float64 norm, rounded to float32 once; the Euclidean bias follows.  A cluster without a frame is re-seeded from
        the assigned frame of the last batch with the smallest quality (ties to the lowest row; the next smallest for
        the next empty cluster).  The sums are cleared (``last_contingency`` keeps the table of the iteration)."""
        self._ensure_device()
        st = self._state
        count, total = st["count"].clone(), int(st["totals"][0])
        if total == 0:
            raise ValueError("CodeKMeans.step: no frame was assigned since the last step")
        objective = int(st["best_q"].sum()) / Q_SCALE / total
        full = count > 0
        c64 = st["S_q"].double() / (torch.where(full, count, torch.ones_like(count)).double() * Q_SCALE)[None, :]
        st["Ct"].copy_(torch.where(full[None, :], self._finish(c64), st["Ct"]))
        empty = torch.nonzero(~full).reshape(-1).tolist()
        if empty:
            v, i, a, quality = self._last
            order = torch.argsort(quality, stable=True)[:len(empty)]
            order = order[(a[order] >= 0)].cpu()
            vr, ir = v[order.to(v.device)].cpu(), i[order.to(v.device)].cpu()
            for j, c in enumerate(empty[:order.numel()]):
                st["Ct"][:, c] = self._finish(self._row_centroid(vr[j], ir[j])[:, None])[:, 0].to(st["Ct"].device)
        self._set_bias()
        n_changed = None
        if self._prev_assigns is not None and len(self._prev_assigns) == len(self._assigns) and all(
                p.shape == q.shape for p, q in zip(self._prev_assigns, self._assigns)):
            n_changed = sum(int((p != q).sum()) for p, q in zip(self._prev_assigns, self._assigns))
        self._prev_assigns = self._assigns
        self.last_contingency = None if st["contingency"] is None else st["contingency"].clone()
        self._clear()
        return IterationStats(objective, count, len(empty), n_changed)

    def fit(self, code, segments: Optional[Tensor] = None, frame_mask: Optional[Tensor] = None, labels: Optional[Tensor] = None,
            max_iter: int = 50, tol: float = 1e-6, init="sample") -> List[IterationStats]:
        """Fit data that are in memory: one plan, then ``accumulate`` and ``step`` until no assignment changes, the
        relative gain of the objective falls below ``tol`` or ``max_iter`` iterations.  Centroids that were set before
        are kept (``init`` seeds them otherwise).  Returns the statistics of every iteration."""
        if not self._seeded:
            self.init_centroids(code, init, segments, frame_mask)
        v, i, k, seg, _ = self._prepare(code, segments, frame_mask, None)
        plan = _stream.transposed_plan(self, v, i, k, seg, seg.shape[0]) if seg.shape[0] else None
        history: List[IterationStats] = []
        for _ in range(int(max_iter)):
            self.accumulate(code, segments, frame_mask, labels, _plan=plan)
            history.append(self.step())
            if history[-1].n_changed == 0:
                break
            if len(history) > 1:
                prev, cur = history[-2].objective, history[-1].objective
                if abs(cur - prev) <= float(tol) * abs(prev):
                    break
        return history

    def predict(self, code, segments: Optional[Tensor] = None, frame_mask: Optional[Tensor] = None):
        """``(assign int32, score, margin float32)`` per frame under the current centroids; nothing is added to the sums.
        ``score``: the cosine to the winning centroid, or ``x . c - |c|^2 / 2`` for Euclidean; ``margin``: the winner's
        raw score minus the runner-up's (inf with one cluster); both 0 where ``assign`` is -1."""
        if not self._seeded:
            raise ValueError("CodeKMeans has no centroids: call init_centroids first")
        v, i, k, seg, _ = self._prepare(code, segments, frame_mask, None)
        if seg.shape[0] == 0:
            e = torch.empty(0, dtype=torch.float32, device=v.device)
            return torch.empty(0, dtype=torch.int32, device=v.device), e, e.clone()
        cosine = self.metric == "cosine"
        st = self._state
        a, best, second, inv = self._assign(v, i, k, seg, None, st["Ct"], None if cosine else st["bias"], cosine, False)
        return a, best * inv if cosine else best, best - second

    def score(self, code, labels: Tensor, segments: Optional[Tensor] = None, frame_mask: Optional[Tensor] = None) -> ClusterScores:
        """``ClusterScores`` of the units of ``code`` against ``labels`` under the current centroids (nothing is kept)."""
        a, _, _ = self.predict(code, segments, frame_mask)
        n_classes = self.n_classes or max(int(labels.max()) + 1, 1)  # (without n_classes: what the labels name)
        lab = _stream.frame_labels(code[0], labels, n_classes).to(a.device)
        ok = (a >= 0) & (lab >= 0)
        table = torch.bincount(a[ok].long() * n_classes + lab[ok].long(), minlength=self.n_clusters * n_classes)
        return cluster_scores(table.reshape(self.n_clusters, n_classes))

    def top_features(self, n: int = 10) -> Tuple[Tensor, Tensor]:
        """``(features int64, weights float32)`` ``[n_clusters, min(n, n_cols)]``: the heaviest features of every unit,
        descending, ties to the lower column."""
        Ct = _stream.state_field(self, "Ct")
        pairs = [_stream.top_weights(Ct[:, c], self.feature_index, n) for c in range(self.n_clusters)]
        return torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])

    def merge_sums(self, other: "CodeKMeans") -> None:
        """Add the sums another clustering gathered under the same centroids (another shard of the iteration)."""
        if not isinstance(other, CodeKMeans):
            raise TypeError(f"merge_sums needs a CodeKMeans, got {type(other).__name__}")
        mine = (self.n_clusters, self.hidden, self.metric, self.n_classes, self.n_cols)
        theirs = (other.n_clusters, other.hidden, other.metric, other.n_classes, other.n_cols)
        if mine != theirs or not torch.equal(self.feature_index.cpu(), other.feature_index.cpu()):
            raise ValueError(f"merge_sums: the clusterings differ: {mine} and {theirs}")
        self._ensure_device()
        other._ensure_device()
        if not torch.equal(self._state["Ct"].cpu(), other._state["Ct"].cpu()):
            raise ValueError("merge_sums: the sums were gathered under different centroids")
        for name in ("S_q", "count", "best_q", "contingency", "totals"):
            if self._state[name] is not None:
                self._state[name] += other._state[name].to(self.device)
        if other._last is not None:
            self._last = tuple(t.to(self.device) for t in other._last)
        self._assigns = self._assigns + [t.to(self.device) for t in other._assigns]

    # ---- persistence ----------------------------------------------------------------------------
    def save(self, path) -> None:
        """The centroids and the sums, without the data."""
        torch.save({"n_clusters": self.n_clusters, "hidden": self.hidden, "metric": self.metric, "seed": self.seed,
                    "n_classes": self.n_classes, "seeded": self._seeded,
                    "features": None if self._col_of is None else self.feature_index.cpu(),
                    "state": _stream.state_to_cpu(self)}, Path(path))

    @classmethod
    def load(cls, path, device=None) -> "CodeKMeans":
        data = torch.load(Path(path), map_location="cpu", weights_only=True)
        km = cls(data["n_clusters"], data["hidden"], features=data["features"], metric=data["metric"], device=device,
                 seed=data["seed"], n_classes=data["n_classes"])
        _stream.state_from_saved(km, data["state"])
        km._seeded = bool(data["seeded"])
        return km


def collect_code_clusters(model, utterances, n_clusters: int, metric: str = "cosine", features: Optional[Tensor] = None,
                          n_classes: int = 0, max_iter: int = 20, tol: float = 1e-6, seed: int = 0, device="cuda"):
    """Cluster the codes of a dataset of utterances: ``(CodeKMeans, [IterationStats])``.  Every item is ``x [n_utt, T,
    D]``, ``(x, frame_mask)``, ``(x, labels)`` or ``(x, labels, frame_mask)``; in a pair, an integer tensor is ``labels`` and
    a bool or floating one the mask.  ``utterances`` is walked once per iteration, so it must be re-iterable (a list, a
    dataset - not a generator: ``TypeError``).  The centroids are seeded from the frames of the first item.  The module
    must offer ``encode_compact`` (TopK and BatchTopK SAEs; a ReLU SAE's code is dense: ``TypeError``) and is run in eval
    mode; its previous mode is restored."""
    if iter(utterances) is utterances:
        raise TypeError("utterances is walked once per iteration: pass a re-iterable (a list or a dataset), not an iterator")

    def items():
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
            yield (_stream.utterance_code(model, x, device), None if labels is None else labels.to(device),
                   None if mask is None else mask.to(device))

    history: List[IterationStats] = []
    with _stream.encoding(model, hint="code clustering is for TopK-family codes"):
        km = CodeKMeans(n_clusters, model.hidden_dim, features, metric, device=device, seed=seed, n_classes=n_classes)
        for _ in range(int(max_iter)):
            seen = False
            for code, labels, mask in items():
                if not km._seeded:
                    km.init_centroids(code, "sample", frame_mask=mask)
                km.accumulate(code, frame_mask=mask, labels=labels if n_classes else None)
                seen = True
            if not seen:
                raise ValueError("collect_code_clusters: no utterances")
            history.append(km.step())
            if history[-1].n_changed == 0:
                break
            if len(history) > 1 and abs(history[-1].objective - history[-2].objective) <= float(tol) * abs(history[-2].objective):
                break
    return km, history
