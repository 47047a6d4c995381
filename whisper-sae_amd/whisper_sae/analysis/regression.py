"""Sparse ridge regression: does a feature, or a small set of features, track a CONTINUOUS per-frame
quantity - F0, energy, a formant, position in the utterance, a coordinate of another layer - and how much of its variance
do they explain?

``SparseRegression`` accumulates the sufficient statistics of a linear regression of ``n_targets`` float targets per frame
on the compact ``(values, indices)`` code in ONE streaming pass: the Gram matrix of the code ``G = X^T X``
(``wsae_gram_update``), the cross moment ``M = X^T Y``, the column sums, the target sums and the frame count (one
``wsae_probe_backward`` call on the lag-shifted targets with a column of ones appended).  The dense ``[frames, H]`` code
never exists, nothing of the data is kept and no float is added with an atomic.  Afterwards every ridge penalty, every
feature subset and the whole k-sparse regression curve are host-side Cholesky solves of sub-blocks (``fit``,
``regression_curve``); ``evaluate`` / ``predict`` apply a fitted map to other data through ``wsae_regress_forward``.

Out of scope: L1 / elastic-net penalties, per-frame weights, targets in float64 (they are read as float32), several GPUs.
"""

from __future__ import annotations

from pathlib import Path
from typing import NamedTuple, Optional, Sequence, Tuple

import torch
from torch import Tensor

from .. import _native as N
from . import _stream


class RegressionFit(NamedTuple):
    """``weight`` float64 ``[n, C]`` and ``bias`` ``[C]`` on the CPU; ``columns`` int64 ``[n]``: the tracker's columns the
    rows of ``weight`` belong to, ``features`` their feature indices; ``l2``; ``objective``: ``1/(2n) sum |y - b - W^T x|^2 +
    l2 / 2 |W|^2`` at the solution; ``r2_train`` float64 ``[C]`` (NaN where a target has no variance)."""

    weight: Tensor
    bias: Tensor
    columns: Tensor
    features: Tensor
    l2: float
    objective: float
    r2_train: Tensor


class RegressionReport(NamedTuple):
    """Per target, float64 ``[C]`` on the CPU: the mean squared error, ``r2 = 1 - sum (y - yhat)^2 / sum (y - ybar)^2`` and
    the Pearson correlation of target and prediction (NaN where a variance is 0); ``n_frames``: the frames used."""

    mse: Tensor
    r2: Tensor
    pearson: Tensor
    n_frames: int


class RegressionCurve(NamedTuple):
    """Per size n of ``sizes``: the ridge fit on the first n features of the ranking.  ``train_r2`` / ``test_r2`` float64
    ``[len(sizes), C]``; ``features`` the ranking that was used (int64)."""

    sizes: Tuple[int, ...]
    train_r2: Tensor
    test_r2: Tensor
    features: Tensor


def ridge_from_statistics(gram: Tensor, moment: Tensor, col_sum: Tensor, target_sum: Tensor, target_sq: Tensor, n: float,
                          l2: float):
    """``(W [P, C], b [C], objective, r2 [C])`` in float64 from the FULL symmetric ``gram [P, P]``, ``moment [P, C]``, the
    sums ``col_sum [P]``, ``target_sum [C]``, ``target_sq [C]`` and the frame count: the minimiser of ``1/(2n) sum |y - b -
    W^T x|^2 + l2 / 2 |W|^2`` (the intercept is not penalised), by a Cholesky solve of ``(Gc / n + l2 I) W = Mc / n`` on the
    centred statistics, then ``b = ybar - W^T xbar``.  Runs on the tensors' device; no data are read."""
    n = float(n)
    if not n > 0:
        raise ValueError("the statistics hold no frame")
    if not float(l2) >= 0:
        raise ValueError(f"l2 must not be negative, got {l2}")
    G, M = gram.to(torch.float64), moment.to(torch.float64)
    xbar, ybar = col_sum.to(torch.float64) / n, target_sum.to(torch.float64) / n
    Gc = G / n - torch.outer(xbar, xbar)
    B = M / n - torch.outer(xbar, ybar)
    A = Gc + float(l2) * torch.eye(G.shape[0], dtype=torch.float64, device=G.device)
    L, info = torch.linalg.cholesky_ex(A)
    if int(info) != 0:
        raise ValueError("the ridge system is not positive definite: raise l2 (a feature that never fires, or two features "
                         "that fire together with proportional values, make the Gram matrix singular)")
    W = torch.cholesky_solve(B, L)
    b = ybar - W.T @ xbar
    var_y = target_sq.to(torch.float64) / n - ybar * ybar
    mse = var_y - 2 * (W * B).sum(0) + (W * (Gc @ W)).sum(0)
    objective = float(0.5 * mse.sum() + 0.5 * float(l2) * (W * W).sum())
    r2 = torch.where(var_y > 0, 1 - mse / torch.where(var_y > 0, var_y, torch.ones_like(var_y)), torch.full_like(var_y, float("nan")))
    return W, b, objective, r2


def _pearson(cov: Tensor, var_a: Tensor, var_b: Tensor) -> Tensor:
    ok = (var_a[:, None] > 0) & (var_b[None, :] > 0)
    den = torch.sqrt(torch.where(ok, var_a[:, None] * var_b[None, :], torch.ones_like(cov)))
    return torch.where(ok, cov / den, torch.zeros_like(cov))


class SparseRegression:
    """The statistics of a linear regression of ``n_targets`` (1 .. 1023) float targets per frame on the features
    ``features`` (a 1-D index tensor without duplicates, at most 8192 of them; None: all ``hidden``) of a compact code.  The
    target of a frame is read ``lag`` frames later (-1024 .. 1024), never across an utterance; a frame whose target row holds
    a non-finite value is dropped.  The state is float64 on the device: ``G`` (upper triangle) ``[n_cols, n_cols]``, the
    moments ``[n_cols, C + 1]`` (``X^T Y``, then the column sums), the sums ``[C + 1]`` (``sum Y``, then the frames) and
    ``sum Y^2 [C]``."""

    def __init__(self, hidden: int, n_targets: int, *, features: Optional[Tensor] = None, lag: int = 0, device=None):
        self.hidden, self.n_targets, self.lag = int(hidden), int(n_targets), int(lag)
        if self.hidden < 1:
            raise ValueError(f"hidden must be positive, got {hidden}")
        if not 1 <= self.n_targets <= N.PROBE_MAX_CLASSES - 1:  # (the column of ones is one more)
            raise ValueError(f"n_targets must be in 1..{N.PROBE_MAX_CLASSES - 1}, got {n_targets}")
        _stream.check_lag(lag)
        self.feature_index, self._col_of = _stream.column_map(features, self.hidden)
        self.n_cols = self.feature_index.numel()
        if self.n_cols > N.GRAM_MAX_COLS:
            raise ValueError(f"{self.n_cols} features exceed the {N.GRAM_MAX_COLS} columns of a Gram matrix: pass a subset")
        self.device = torch.device(device) if device is not None else None
        self._G: Optional[Tensor] = None
        self._MX: Optional[Tensor] = None
        self._sums: Optional[Tensor] = None
        self._syy: Optional[Tensor] = None
        self._form: Optional[str] = None
        self._ws: Optional[Tensor] = None

    # ---- state ----------------------------------------------------------------------------------
    def _ensure_device(self, like: Optional[Tensor] = None) -> torch.device:
        if self._G is not None:
            return self._G.device
        dev = _stream.need_gpu("SparseRegression", self.device or (like.device if like is not None else None))
        P, C = self.n_cols, self.n_targets
        self._G = torch.zeros(P, P, dtype=torch.float64, device=dev)
        self._MX = torch.zeros(P, C + 1, dtype=torch.float64, device=dev)
        self._sums = torch.zeros(C + 1, dtype=torch.float64, device=dev)
        self._syy = torch.zeros(C, dtype=torch.float64, device=dev)
        self.feature_index = self.feature_index.to(dev)
        if self._col_of is not None:
            self._col_of = self._col_of.to(dev)
        self.device = dev
        return dev

    @property
    def n_frames(self) -> int:
        """The frames used so far (a float64 sum of ones: exact below 2^53)."""
        return 0 if self._sums is None else int(round(float(self._sums[-1])))

    def _prepare(self, code, targets, frame_mask, segments, n_targets: int, check_form: bool, need_segments: bool = True):
        also = () if targets is None else ((targets, "targets"),)
        vals, idx, k = _stream.compact_code(code, "code", N.PROBE_MAX_K, also=also)
        dev = self._ensure_device(vals)
        if vals.device != dev or (targets is not None and targets.device != dev):
            raise N.WsaeError(f"the code is on {vals.device}" + ("" if targets is None else f" and the targets on {targets.device}")
                              + f", the regression on {dev}")
        form = _stream.take_form(self, vals) if check_form else None
        if vals.dim() == 2 and segments is None and not need_segments:
            seg = None
            if frame_mask is not None:
                raise ValueError("a flat [rows, k] code takes a frame_mask only with segments")
        else:
            seg, _ = _stream.frame_segments(vals, segments, frame_mask, dev)
        rows = vals.numel() // k
        if rows > _stream.MAX_ROWS:
            raise N.WsaeError(f"SparseRegression: {rows} frames in one call exceed {_stream.MAX_ROWS}")
        Y = None
        if targets is not None:
            if targets.shape != vals.shape[:-1] + (n_targets,) or not targets.is_floating_point():
                raise ValueError(f"targets must be floating, {tuple(vals.shape[:-1]) + (n_targets,)}: one row of {n_targets} per "
                                 f"frame of the code; got {tuple(targets.shape)} {targets.dtype}")
            Y = targets.detach().reshape(rows, n_targets).to(torch.float32).contiguous()
        v, i = _stream.flat_code(vals, idx, k)
        return v, i, k, seg, Y, rows, form

    def _shifted(self, seg: Tensor, Y: Tensor, rows: int):
        """``(E float32 [rows, C + 1], seg_used)``: the rule of ``wsae_regress_forward`` folded into the segment ids, and the
        targets ``Y[r + lag]`` of the used rows with a column of ones; exact zeros on the other rows."""
        dev = seg.device
        q = torch.arange(rows, device=dev) + self.lag
        inside = (q >= 0) & (q < rows)
        qc = q.clamp(0, max(rows - 1, 0))
        used = (seg >= 0) & inside & (seg[qc] == seg) & torch.isfinite(Y[qc]).all(1)
        E = torch.zeros(rows, self.n_targets + 1, dtype=torch.float32, device=dev)
        E[:, :-1] = torch.where(used[:, None], Y[qc], torch.zeros_like(Y))
        E[:, -1] = used.to(torch.float32)
        return E, torch.where(used, seg, torch.full_like(seg, -1)).contiguous()

    # ---- accumulation ---------------------------------------------------------------------------
    def update(self, code, targets: Tensor, frame_mask: Optional[Tensor] = None, segments: Optional[Tensor] = None) -> None:
        """Add whole utterances.  ``code = (values, indices)`` ``[n_utt, T, k]`` with ``targets [n_utt, T, C]``, or flat
        ``[rows, k]`` with ``targets [rows, C]`` and ``segments [rows]`` (the utterance of every row; < 0: padding).  Frames
        with ``frame_mask == 0`` are padding.  Nothing of the data is kept."""
        v, i, k, seg, Y, rows, form = self._prepare(code, targets, frame_mask, segments, self.n_targets, True)
        self._form = form
        if rows == 0:
            return
        dev = v.device
        lib = N.lib()
        P, C = self.n_cols, self.n_targets
        E, seg = self._shifted(seg, Y, rows)
        col_ptr, t_row, t_val, n = _stream.transposed_plan(self, v, i, k, seg, rows)
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            need = max(lib.wsae_gram_workspace_bytes(rows, k, self.hidden, P, P, n),
                       lib.wsae_probe_backward_workspace_bytes(rows, P, C + 1, n))
            ws = _stream.workspace(self, need, dev)
            N.check(lib.wsae_gram_update(v.data_ptr(), i.data_ptr(), k, self.hidden, seg.data_ptr(), rows, N.ptr(self._col_of), P,
                                         col_ptr.data_ptr(), N.ptr(t_row), N.ptr(t_val), n, 0, P, self._G.data_ptr(), P,
                                         ws.data_ptr(), need, st), "wsae_gram_update")
            N.check(lib.wsae_probe_backward(col_ptr.data_ptr(), N.ptr(t_row), N.ptr(t_val), n, P, E.data_ptr(), C + 1, C + 1, rows,
                                            self._MX.data_ptr(), self._sums.data_ptr(), ws.data_ptr(), need, st),
                    "wsae_probe_backward")
            Yd = E[:, :-1].to(torch.float64)
            self._syy += (Yd * Yd).sum(0)

    def merge(self, other: "SparseRegression") -> None:
        """Add the state of another shard (same dictionary, targets, features and lag)."""
        if (other.hidden, other.n_targets, other.lag, other.n_cols) != (self.hidden, self.n_targets, self.lag, self.n_cols) or \
                not torch.equal(other.feature_index.cpu(), self.feature_index.cpu()):
            raise ValueError("merge needs two trackers over the same features, targets and lag")
        if other._G is None:
            return
        dev = self._ensure_device(other._G)
        for name in ("_G", "_MX", "_sums", "_syy"):
            getattr(self, name).add_(getattr(other, name).to(dev))

    # ---- the statistics -------------------------------------------------------------------------
    def gram(self) -> Tensor:
        """float64 ``[n_cols, n_cols]``: the full symmetric matrix (the kernel keeps its upper triangle)."""
        self._ensure_device()
        return torch.triu(self._G) + torch.triu(self._G, 1).T

    moment = property(lambda self: self._view("_MX")[:, :-1], doc="float64 [n_cols, C]: X^T Y.")
    col_sum = property(lambda self: self._view("_MX")[:, -1], doc="float64 [n_cols]: the sum of every feature's activation.")
    target_sum = property(lambda self: self._view("_sums")[:-1], doc="float64 [C]: the sum of every target.")
    target_sq = property(lambda self: self._view("_syy"), doc="float64 [C]: the sum of every target's square.")

    def _view(self, name: str) -> Tensor:
        self._ensure_device()
        return getattr(self, name)

    def _need_frames(self) -> float:
        n = self.n_frames
        if n < 1:
            raise ValueError("SparseRegression holds no frame: call update first")
        return float(n)

    def _variances(self):
        n = self._need_frames()
        xbar, ybar = self.col_sum / n, self.target_sum / n
        var_x = torch.diagonal(self._G) / n - xbar * xbar
        var_y = self.target_sq / n - ybar * ybar
        return n, xbar, ybar, var_x, var_y

    def correlations(self) -> Tensor:
        """float64 ``[n_cols, C]``: the Pearson r of every feature's activation (0 where it does not fire) with every
        target over the used frames, from the statistics; 0 where either variance is 0."""
        n, xbar, ybar, var_x, var_y = self._variances()
        return _pearson(self.moment / n - torch.outer(xbar, ybar), var_x, var_y)

    def feature_correlations(self) -> Tensor:
        """float64 ``[n_cols, n_cols]``: the same between the features themselves."""
        n, xbar, _, var_x, _ = self._variances()
        return _pearson(self.gram() / n - torch.outer(xbar, xbar), var_x, var_x)

    # ---- the solve ------------------------------------------------------------------------------
    def fit(self, l2: float = 1e-3, columns: Optional[Tensor] = None) -> RegressionFit:
        """The ridge fit on the columns ``columns`` of the tracker (positions in ``feature_index``, without duplicates; None:
        all): a float64 Cholesky solve of that sub-block of the statistics on the host (``ridge_from_statistics``).  No data
        are read again."""
        n = self._need_frames()
        if columns is None:
            cols = torch.arange(self.n_cols, dtype=torch.int64)
        else:
            cols = torch.as_tensor(columns).detach().reshape(-1).cpu()
            if cols.numel() < 1 or cols.is_floating_point() or cols.dtype == torch.bool:
                raise ValueError("columns must hold at least one integer position")
            cols = cols.to(torch.int64)
            if int(cols.min()) < 0 or int(cols.max()) >= self.n_cols or torch.unique(cols).numel() != cols.numel():
                raise ValueError(f"columns must be distinct positions in [0, {self.n_cols})")
        at = cols.to(self._G.device)
        lo, hi = torch.minimum(at[:, None], at[None, :]), torch.maximum(at[:, None], at[None, :])
        G = self._G[lo, hi].cpu()  # (the upper triangle holds the cell of every pair)
        W, b, objective, r2 = ridge_from_statistics(G, self.moment[at].cpu(), self.col_sum[at].cpu(), self.target_sum.cpu(),
                                                    self.target_sq.cpu(), n, l2)
        return RegressionFit(W, b, cols, self.feature_index[at].cpu(), float(l2), objective, r2)

    def _fit_map(self, fit: RegressionFit, dev):
        """``(col_of int32 [hidden], W float64 [n, C], bias)`` of a fit on the device."""
        if fit.weight.shape != (fit.features.numel(), self.n_targets) or fit.bias.numel() != self.n_targets:
            raise ValueError(f"the fit holds weights {tuple(fit.weight.shape)} for {fit.features.numel()} features and "
                             f"{self.n_targets} targets")
        feats = fit.features.to(torch.int64)
        if int(feats.min()) < 0 or int(feats.max()) >= self.hidden:
            raise ValueError(f"the fit's features must lie in [0, {self.hidden})")
        return (_stream.column_table(feats, self.hidden).to(dev), fit.weight.to(dev, torch.float64).contiguous(), fit.bias.to(dev, torch.float64).contiguous())

    def _forward(self, fit, v, i, k, seg, Y, rows, pred, n_used, stats):
        dev = v.device
        lib = N.lib()
        col_of, W, b = self._fit_map(fit, dev)
        C = self.n_targets
        need = lib.wsae_regress_forward_workspace_bytes(rows, k, self.hidden, W.shape[0], C, self.lag) if Y is not None else 0
        if need < 0:
            raise N.WsaeError(f"wsae_regress_forward_workspace_bytes rejects rows={rows} k={k} hidden={self.hidden}")
        with torch.cuda.device(dev):
            ws = _stream.workspace(self, need, dev)
            N.check(lib.wsae_regress_forward(v.data_ptr(), i.data_ptr(), k, self.hidden, N.ptr(seg), N.ptr(Y), C, rows, self.lag, C,
                                             col_of.data_ptr(), W.shape[0], W.data_ptr(), C, b.data_ptr(), N.ptr(pred), C,
                                             N.ptr(n_used), N.ptr(stats), ws.data_ptr(), need,
                                             torch.cuda.current_stream(dev).cuda_stream), "wsae_regress_forward")

    def evaluate(self, fit: RegressionFit, code, targets: Tensor, frame_mask: Optional[Tensor] = None,
                 segments: Optional[Tensor] = None) -> RegressionReport:
        """A fit on other data (the forward product only; nothing is kept): per target the mean squared error, R^2 and
        the Pearson r of target and prediction over the frames the tracker's rule uses, from the forward's five sums."""
        v, i, k, seg, Y, rows, _ = self._prepare(code, targets, frame_mask, segments, self.n_targets, False)
        dev = v.device
        C = self.n_targets
        n_used = torch.zeros(1, dtype=torch.int64, device=dev)
        stats = torch.zeros(5, C, dtype=torch.float64, device=dev)
        if rows:
            self._forward(fit, v, i, k, seg, Y, rows, None, n_used, stats)
        n = int(n_used.item())
        nan = torch.full((C,), float("nan"), dtype=torch.float64)
        if n == 0:
            return RegressionReport(nan, nan.clone(), nan.clone(), 0)
        sy, syy, sp, spp, see = stats.cpu()
        var_y, var_p = syy / n - (sy / n) ** 2, spp / n - (sp / n) ** 2
        cov = (syy + spp - see) / (2 * n) - sy * sp / (n * n)  # sum y yhat = (sum y^2 + sum yhat^2 - sum (y - yhat)^2) / 2
        one = torch.ones_like(var_y)
        r2 = torch.where(var_y > 0, 1 - see / n / torch.where(var_y > 0, var_y, one), nan)
        ok = (var_y > 0) & (var_p > 0)
        pearson = torch.where(ok, cov / torch.sqrt(torch.where(ok, var_y * var_p, one)), nan)
        return RegressionReport(see / n, r2, pearson, n)

    def predict(self, fit: RegressionFit, code, frame_mask: Optional[Tensor] = None, segments: Optional[Tensor] = None) -> Tensor:
        """float32 ``[n_utt, T, C]`` / ``[rows, C]``: the fit's prediction on every frame, exact zeros on padding.  A flat
        code may come without ``segments`` (no padding then)."""
        v, i, k, seg, _, rows, _ = self._prepare(code, None, frame_mask, segments, self.n_targets, False, need_segments=False)
        pred = torch.zeros(rows, self.n_targets, dtype=torch.float32, device=v.device)
        if rows:
            self._forward(fit, v, i, k, seg, None, rows, pred, None, None)
        return pred.reshape(tuple(code[0].shape[:-1]) + (self.n_targets,))

    def top_weights(self, fit: RegressionFit, c: int, n: int = 10) -> Tuple[Tensor, Tensor]:
        """``(features int64, weights float64)``: the ``n`` features with the largest weight for target ``c``, descending,
        ties to the lower column."""
        c = _stream.check_index(c, self.n_targets, "target")
        return _stream.top_weights(fit.weight[:, c], fit.features, n)

    # ---- persistence ----------------------------------------------------------------------------
    def save(self, path) -> None:
        """The statistics, not the data."""
        self._ensure_device()
        torch.save({"hidden": self.hidden, "n_targets": self.n_targets, "lag": self.lag,
                    "features": None if self._col_of is None else self.feature_index.cpu(), "G": self._G.cpu(),
                    "MX": self._MX.cpu(), "sums": self._sums.cpu(), "syy": self._syy.cpu()}, Path(path))

    @classmethod
    def load(cls, path, device=None) -> "SparseRegression":
        data = torch.load(Path(path), map_location="cpu", weights_only=True)
        s = cls(data["hidden"], data["n_targets"], features=data["features"], lag=data["lag"], device=device)
        s._ensure_device()
        for name, key in (("_G", "G"), ("_MX", "MX"), ("_sums", "sums"), ("_syy", "syy")):
            getattr(s, name).copy_(data[key])
        return s


def regression_curve(stats: SparseRegression, test, ranking: Tensor, sizes: Sequence[int] = (1, 2, 4, 8, 16, 32, 64),
                     l2: float = 1e-3) -> RegressionCurve:
    """The k-sparse regression curve from ONE accumulated state: per size n the ridge fit on the first n features of
    ``ranking`` (an ordered feature index, all of them among the tracker's features) - a solve of a sub-block - with its
    training R^2 and the R^2 of ``evaluate`` on ``test``, the argument tuple ``(code, targets[, frame_mask[, segments]])``."""
    ranking, sizes = _stream.curve_arguments(ranking, sizes)
    where = torch.full((stats.hidden,), -1, dtype=torch.int64)
    where[stats.feature_index.cpu()] = torch.arange(stats.n_cols, dtype=torch.int64)
    if ranking.numel() and (int(ranking.min()) < 0 or int(ranking.max()) >= stats.hidden or bool((where[ranking] < 0).any())):
        raise ValueError("the ranking names a feature the statistics do not cover")
    columns = where[ranking]
    train = torch.zeros(len(sizes), stats.n_targets, dtype=torch.float64)
    held = torch.zeros_like(train)
    for j, n in enumerate(sizes):
        fit = stats.fit(l2, columns[:n])
        train[j], held[j] = fit.r2_train, stats.evaluate(fit, *test).r2
    return RegressionCurve(sizes, train, held, ranking)


def top_correlated_features(stats: SparseRegression, c: int, n: int = 10) -> Tuple[Tensor, Tensor]:
    """``(features int64, r float64)``: the ``n`` features whose activation correlates most strongly (by ``|r|``) with target
    ``c``, descending, ties to the lower column; features without variance are no candidates."""
    c = _stream.check_index(c, stats.n_targets, "target")
    r = stats.correlations()[:, c]
    _, _, _, var_x, _ = stats._variances()
    order = _stream.rank_features(r.abs(), var_x > 0, n)
    return stats.feature_index[order], r[order]


def collect_regression(model, utterances, n_targets: int, *, features: Optional[Tensor] = None, lag: int = 0,
                       device=None) -> SparseRegression:
    """The regression statistics over a dataset.  Every item of ``utterances`` is ``(x [n_utt, T, D], targets [n_utt, T, C])``
    or ``(x, targets, frame_mask [n_utt, T])``; T may differ between items.  The module must offer ``encode_compact`` (TopK
    and BatchTopK SAEs; a ReLU SAE's code is dense: ``TypeError``) and is run in eval mode; its previous mode is
    restored."""
    with _stream.encoding(model, hint="sparse regression is for TopK-family codes"):
        dev = _stream.need_gpu("collect_regression", torch.device(device) if device is not None else None)
        stats = SparseRegression(model.hidden_dim, n_targets, features=features, lag=lag, device=dev)
        for x, targets, mask in _stream.labelled_batches(utterances):
            v, i = _stream.utterance_code(model, x, dev)
            stats.update((v, i), targets.to(dev), None if mask is None else mask.to(dev))
    return stats
