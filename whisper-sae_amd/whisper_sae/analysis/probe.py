"""Sparse linear probes: how well does a SET of features predict a per-frame label - and how small
can the set be?

``SparseProbe`` fits a softmax regression of an integer label per frame on the compact ``(values, indices)`` code.  The
dense ``[frames, H]`` code never exists: the data stay on the device in compact form, ``wsae_probe_plan`` transposes them
once per shard, and one evaluation of the objective is ``wsae_probe_forward`` (row-wise: logits from the k gathered weight
rows, softmax, loss, the error rows) and ``wsae_probe_backward`` (column-wise: a feature's gradient is the value-weighted
sum of the error rows on which it fires) per shard.  Neither adds floats with atomics: the loss is an integer sum of
quantised row losses and the gradient a fixed order of float64 additions, so two fits of the same data agree bit for bit,
whatever the batching.  ``features`` restricts the probe to a subset of the dictionary - ``sparse_probe_curve`` fits one
probe per prefix of a ranking (``top_label_features``), the k-sparse probing plot.

Out of scope: dense probes on raw activations, L1 / proximal sparsity (the subset probes cover the sparse case),
minibatch or SGD fitting, several GPUs.
"""

from __future__ import annotations

import math
from pathlib import Path
from typing import NamedTuple, Optional, Sequence, Tuple

import torch
from torch import Tensor

from .. import _native as N
from . import _stream

LOSS_SCALE = float(2 ** 20)  # loss_q counts 2^-20


class ProbeFit(NamedTuple):
    """``loss``: the objective at the fitted parameters (mean row loss + l2 / 2 |W|^2); ``grad_norm``: the 2-norm of its
    gradient there; ``iterations`` / ``evaluations`` of L-BFGS; ``converged``: ``grad_norm <= tolerance_grad``."""

    loss: float
    grad_norm: float
    iterations: int
    evaluations: int
    converged: bool


class ProbeReport(NamedTuple):
    """``loss``: the mean (class-weighted) row loss, without the penalty; ``accuracy``; ``n_frames``: the frames that carry
    a label; ``confusion`` int64 ``[C, C]`` (label, prediction); ``precision``, ``recall``, ``f1`` float64 ``[C]`` from it
    (NaN where a denominator is 0)."""

    loss: float
    accuracy: float
    n_frames: int
    confusion: Tensor
    precision: Tensor
    recall: Tensor
    f1: Tensor


class ProbeCurve(NamedTuple):
    """Per size n of ``sizes``: the probe on the first n features of the ranking.  ``train_loss`` is the fitted objective,
    ``test_loss`` / ``test_accuracy`` those of ``evaluate``; ``features`` the ranking that was used (int64)."""

    sizes: Tuple[int, ...]
    train_loss: Tensor
    test_loss: Tensor
    test_accuracy: Tensor
    features: Tensor


class ProbeData(NamedTuple):
    """A dataset in flat form on the device: ``code = (values, indices) [rows, k]``, ``labels [rows]``, ``segments [rows]``
    (the number of the frame's utterance, -1 for padding), ``n_utt`` utterances."""

    code: Tuple[Tensor, Tensor]
    labels: Tensor
    segments: Tensor
    n_utt: int

    def subset(self, utterance_mask: Tensor):
        """``(code, labels, frame_mask, segments)`` - the arguments of ``add_data`` / ``evaluate`` - with the frames of the
        utterances whose ``utterance_mask`` is False masked out."""
        if utterance_mask.numel() != self.n_utt:
            raise ValueError(f"utterance_mask has {utterance_mask.numel()} flags for {self.n_utt} utterances")
        keep = utterance_mask.to(self.segments.device, torch.bool)[self.segments.clamp(min=0).long()] & (self.segments >= 0)
        return self.code, self.labels, keep, self.segments


class SparseProbe:
    """Softmax regression of ``n_classes`` labels on the features ``features`` (a 1-D index tensor without duplicates;
    None: all ``hidden``) of a compact code.  The label of a frame is read ``lag`` frames later (-1024 .. 1024), never
    across an utterance; a label outside ``[0, n_classes)`` drops the frame.  Objective: the mean over the used frames of
    ``class_weight[y]`` times the cross-entropy, plus ``l2 / 2`` times the squared norm of the weights (the bias is not
    penalised); with ``l2 > 0`` it is strictly convex.  The parameters are float64 on the device and are cast to float32
    for the kernels."""

    def __init__(self, hidden: int, n_classes: int, *, features: Optional[Tensor] = None, lag: int = 0, l2: float = 1e-4,
                 class_weight: Optional[Tensor] = None, device=None):
        self.hidden, self.n_classes, self.lag, self.l2 = int(hidden), int(n_classes), int(lag), float(l2)
        if self.hidden < 1:
            raise ValueError(f"hidden must be positive, got {hidden}")
        if not 1 <= self.n_classes <= N.PROBE_MAX_CLASSES:
            raise ValueError(f"n_classes must be in 1..{N.PROBE_MAX_CLASSES}, got {n_classes}")
        _stream.check_lag(lag)
        if not self.l2 >= 0:
            raise ValueError(f"l2 must not be negative, got {l2}")
        self.feature_index, self._col_of = _stream.column_map(features, self.hidden)
        self.n_cols = self.feature_index.numel()
        if class_weight is not None:
            cw = torch.as_tensor(class_weight).detach().to(torch.float32).reshape(-1).cpu()
            if cw.numel() != self.n_classes or not bool(torch.isfinite(cw).all()) or bool((cw < 0).any()):
                raise ValueError(f"class_weight must hold {self.n_classes} finite weights >= 0")
            class_weight = cw.contiguous()
        self.class_weight = class_weight
        self.device = torch.device(device) if device is not None else None
        self._theta: Optional[Tensor] = None  # float64 [P * C + C]: the weights [P, C], then the bias
        self._shards: list = []
        self._form: Optional[str] = None
        self._err: Optional[Tensor] = None
        self._ws: Optional[Tensor] = None

    # ---- state ----------------------------------------------------------------------------------
    def _ensure_device(self, like: Optional[Tensor] = None) -> torch.device:
        if self._theta is not None:
            return self._theta.device
        dev = _stream.need_gpu("SparseProbe", self.device or (like.device if like is not None else None))
        self._theta = torch.zeros(self.n_cols * self.n_classes + self.n_classes, dtype=torch.float64, device=dev)
        self.feature_index = self.feature_index.to(dev)
        if self._col_of is not None:
            self._col_of = self._col_of.to(dev)
        if self.class_weight is not None:
            self.class_weight = self.class_weight.to(dev)
        self.device = self._theta.device
        return self.device

    @property
    def weight(self) -> Tensor:
        """float64 ``[n_cols, C]``: row p belongs to feature ``feature_index[p]`` (a view of the parameters)."""
        self._ensure_device()
        return self._theta[:self.n_cols * self.n_classes].view(self.n_cols, self.n_classes)

    @property
    def bias(self) -> Tensor:
        """float64 ``[C]`` (a view of the parameters)."""
        self._ensure_device()
        return self._theta[self.n_cols * self.n_classes:]

    def _prepare(self, code, labels, frame_mask, segments, check_form: bool):
        vals, idx, k = _stream.compact_code(code, "code", N.PROBE_MAX_K, also=((labels, "labels"),))
        dev = self._ensure_device(vals)
        if vals.device != dev or labels.device != dev:
            raise N.WsaeError(f"the code is on {vals.device} and the labels on {labels.device}, the probe on {dev}")
        form = _stream.take_form(self, vals) if check_form else None
        seg, _ = _stream.frame_segments(vals, segments, frame_mask, dev)
        lab = _stream.frame_labels(vals, labels, self.n_classes)
        if seg.shape[0] > _stream.MAX_ROWS:
            raise N.WsaeError(f"SparseProbe: {seg.shape[0]} frames in one shard exceed {_stream.MAX_ROWS}")
        v, i = _stream.flat_code(vals, idx, k)
        return v, i, k, seg, lab, form

    # ---- data -----------------------------------------------------------------------------------
    def add_data(self, code, labels: Tensor, frame_mask: Optional[Tensor] = None, segments: Optional[Tensor] = None) -> None:
        """One shard of whole utterances, kept on the device with its plan.  ``code = (values, indices)`` ``[n_utt, T, k]``
        with ``labels [n_utt, T]``, or flat ``[rows, k]`` with ``labels [rows]`` and ``segments [rows]`` (the utterance of
        every row; < 0: padding).  Frames with ``frame_mask == 0`` are padding."""
        v, i, k, seg, lab, form = self._prepare(code, labels, frame_mask, segments, True)
        self._form = form
        rows = seg.shape[0]
        if rows == 0:
            return
        col_ptr, t_row, t_val, n = _stream.transposed_plan(self, v, i, k, seg, rows)
        if n < t_row.numel():  # (the shard keeps its plan: cut it to size)
            t_row, t_val = t_row[:n].clone(), t_val[:n].clone()
        self._shards.append({"v": v, "i": i, "k": k, "seg": seg, "lab": lab, "rows": rows, "col_ptr": col_ptr, "t_row": t_row,
                             "t_val": t_val, "nnz": n})
        if self._err is None or self._err.numel() < rows * self.n_classes:
            self._err = None
            self._err = torch.empty(rows * self.n_classes, dtype=torch.float32, device=v.device)

    n_shards = property(lambda self: len(self._shards), doc="The shards added so far.")

    def _forward(self, sh, W32, b32, err, counters, confusion):
        dev = W32.device
        C = self.n_classes
        N.check(N.lib().wsae_probe_forward(
            sh["v"].data_ptr(), sh["i"].data_ptr(), sh["k"], self.hidden, sh["seg"].data_ptr(), sh["lab"].data_ptr(), sh["rows"],
            self.lag, C, N.ptr(self._col_of), self.n_cols, W32.data_ptr(), C, b32.data_ptr(), N.ptr(self.class_weight),
            N.ptr(err), C, None, counters[0:].data_ptr(), counters[1:].data_ptr(), counters[2:].data_ptr(), N.ptr(confusion),
            None, 0, torch.cuda.current_stream(dev).cuda_stream), "wsae_probe_forward")

    def _params32(self):
        return self.weight.to(torch.float32).contiguous(), self.bias.to(torch.float32).contiguous()

    def loss_and_grad(self) -> Tuple[Tensor, Tensor, Tensor]:
        """``(loss, gW [n_cols, C], gb [C])`` in float64 at the current parameters, over all shards: the mean row loss
        over the used frames plus ``l2 / 2 |W|^2``, and its gradient (the sums divided by the used frames, ``l2 W`` added
        in float64)."""
        if not self._shards:
            raise ValueError("SparseProbe has no data: call add_data first")
        dev = self._ensure_device()
        C, P = self.n_classes, self.n_cols
        W32, b32 = self._params32()
        counters = torch.zeros(3, dtype=torch.int64, device=dev)  # n_used, n_correct, loss_q
        gW = torch.zeros(P, C, dtype=torch.float64, device=dev)
        gb = torch.zeros(C, dtype=torch.float64, device=dev)
        lib = N.lib()
        with torch.cuda.device(dev):
            for sh in self._shards:
                self._forward(sh, W32, b32, self._err, counters, None)
                need = lib.wsae_probe_backward_workspace_bytes(sh["rows"], P, C, sh["nnz"])
                ws = _stream.workspace(self, need, dev)
                N.check(lib.wsae_probe_backward(sh["col_ptr"].data_ptr(), N.ptr(sh["t_row"]), N.ptr(sh["t_val"]), sh["nnz"], P,
                                                self._err.data_ptr(), C, C, sh["rows"], gW.data_ptr(), gb.data_ptr(),
                                                ws.data_ptr(), need, torch.cuda.current_stream(dev).cuda_stream),
                        "wsae_probe_backward")
        n = counters[0].double()
        W = self.weight
        loss = counters[2].double() / LOSS_SCALE / n + 0.5 * self.l2 * (W * W).sum()
        return loss, gW / n + self.l2 * W, gb / n

    def fit(self, max_iter: int = 200, tolerance_grad: float = 1e-5, history: int = 10) -> ProbeFit:
        """Minimise the objective from the current parameters with ``torch.optim.LBFGS`` on the float64 parameters until
        the 2-norm of the gradient is at most ``tolerance_grad``, or ``max_iter`` iterations; every evaluation is one
        forward and one backward per shard (``minimize_lbfgs``).  The parameters are left at the evaluated point with
        the smallest gradient."""
        if not self._shards:
            raise ValueError("SparseProbe has no data: call add_data first")
        self._ensure_device()

        def objective():
            loss, gW, gb = self.loss_and_grad()
            return loss, torch.cat([gW.reshape(-1), gb])

        return minimize_lbfgs(self._theta, objective, max_iter, tolerance_grad, history)

    def evaluate(self, code, labels: Tensor, frame_mask: Optional[Tensor] = None, segments: Optional[Tensor] = None) -> ProbeReport:
        """The probe on other data (the forward product only; nothing is kept)."""
        v, i, k, seg, lab, _ = self._prepare(code, labels, frame_mask, segments, False)
        dev = v.device
        C = self.n_classes
        counters = torch.zeros(3, dtype=torch.int64, device=dev)
        confusion = torch.zeros(C, C, dtype=torch.int64, device=dev)
        if seg.shape[0]:
            W32, b32 = self._params32()
            with torch.cuda.device(dev):
                self._forward({"v": v, "i": i, "k": k, "seg": seg, "lab": lab, "rows": seg.shape[0]}, W32, b32, None, counters,
                              confusion)
        n_used, n_correct, loss_q = (int(x) for x in counters.tolist())
        cm = confusion.double()
        tp, pred, true = cm.diagonal(), cm.sum(0), cm.sum(1)
        nan = torch.full_like(tp, float("nan"))
        one = torch.ones_like(tp)
        ratio = lambda a, b: torch.where(b != 0, a / torch.where(b != 0, b, one), nan)
        return ProbeReport(loss=loss_q / LOSS_SCALE / n_used if n_used else math.nan,
                           accuracy=n_correct / n_used if n_used else math.nan, n_frames=n_used, confusion=confusion,
                           precision=ratio(tp, pred), recall=ratio(tp, true), f1=ratio(2 * tp, pred + true))

    def top_weights(self, c: int, n: int = 10) -> Tuple[Tensor, Tensor]:
        """``(features int64, weights float64)``: the ``n`` features with the largest weight for class ``c``, descending,
        ties to the lower column."""
        c = _stream.check_index(c, self.n_classes, "class")
        return _stream.top_weights(self.weight[:, c], self.feature_index, n)

    # ---- persistence ----------------------------------------------------------------------------
    def save(self, path) -> None:
        """The probe without its data."""
        self._ensure_device()
        torch.save({"hidden": self.hidden, "n_classes": self.n_classes, "lag": self.lag, "l2": self.l2,
                    "features": None if self._col_of is None else self.feature_index.cpu(),
                    "class_weight": None if self.class_weight is None else self.class_weight.cpu(),
                    "theta": self._theta.cpu()}, Path(path))

    @classmethod
    def load(cls, path, device=None) -> "SparseProbe":
        data = torch.load(Path(path), map_location="cpu", weights_only=True)
        p = cls(data["hidden"], data["n_classes"], features=data["features"], lag=data["lag"], l2=data["l2"],
                class_weight=data["class_weight"], device=device)
        p._ensure_device()
        p._theta.copy_(data["theta"])
        return p


class _Converged(Exception):
    pass


def minimize_lbfgs(theta: Tensor, objective, max_iter: int = 200, tolerance_grad: float = 1e-5, history: int = 10) -> ProbeFit:
    """Minimise a smooth convex ``objective() -> (loss, flat gradient)`` of the float64 tensor ``theta`` in place.

    Two runs of ``torch.optim.LBFGS`` share the iteration budget.  The first uses the strong Wolfe line search.  Its
    sufficient-decrease test compares losses, and a loss whose rows are computed in float32 resolves differences of about
    1e-8 of its value - near the optimum a step gains less than that (gradient^2 / curvature), the test fails on noise
    and the run stalls at a gradient some times ``tolerance_grad``.  The gradient itself is far more accurate, so a second
    run without line search (unit quasi-Newton steps, judged by the gradient alone) finishes from there.  Every
    evaluation checks the 2-norm of its gradient and ends the fit at that point when it is at most ``tolerance_grad``;
    otherwise ``theta`` ends at the evaluated point with the smallest gradient.  Deterministic given a deterministic
    objective."""
    max_iter, tol = int(max_iter), float(tolerance_grad)
    best = {"norm": math.inf, "loss": math.nan, "theta": theta.clone()}
    evaluations = 0

    def closure():
        nonlocal evaluations
        evaluations += 1
        loss, grad = objective()
        norm = float(torch.linalg.vector_norm(grad))
        if not math.isfinite(float(loss)) or not math.isfinite(norm):
            raise N.WsaeError("the probe's objective is not finite: no frame carries a label, or the code or the parameters "
                              "hold inf")
        if norm < best["norm"]:
            best["norm"], best["loss"] = norm, float(loss)
            best["theta"].copy_(theta)
        if norm <= tol:
            raise _Converged
        theta.grad = grad
        return loss

    iterations = 0
    try:
        for search in ("strong_wolfe", None):
            if max_iter - iterations < 1:
                break
            opt = torch.optim.LBFGS([theta], lr=1.0, max_iter=max_iter - iterations, tolerance_grad=0.0, tolerance_change=0.0,
                                    history_size=int(history), line_search_fn=search)
            try:
                opt.step(closure)
            finally:
                iterations += int(opt.state[theta].get("n_iter", 0))
    except _Converged:
        pass
    theta.grad = None
    theta.copy_(best["theta"])
    return ProbeFit(best["loss"], best["norm"], iterations, evaluations, best["norm"] <= tol)


def utterance_split(n_utt: int, holdout: float = 0.2, seed: int = 0) -> Tuple[Tensor, Tensor]:
    """``(train, test)``: two bool masks ``[n_utt]`` that partition the utterances, ``round(holdout n_utt)`` of them (one
    at least, one fewer than all at most) held out, drawn with ``seed``.  Expand them through ``frame_mask``
    (``mask[:, None] & frame_mask``, or ``ProbeData.subset``): frames of one utterance never sit on both sides."""
    n_utt = int(n_utt)
    if n_utt < 2:
        raise ValueError(f"a split needs at least two utterances, got {n_utt}")
    if not 0.0 < float(holdout) < 1.0:
        raise ValueError(f"holdout must lie in (0, 1), got {holdout}")
    n_test = min(max(int(round(float(holdout) * n_utt)), 1), n_utt - 1)
    perm = torch.randperm(n_utt, generator=torch.Generator().manual_seed(int(seed)))
    test = torch.zeros(n_utt, dtype=torch.bool)
    test[perm[:n_test]] = True
    return ~test, test


def sparse_probe_curve(train, test, ranking: Tensor, sizes: Sequence[int] = (1, 2, 4, 8, 16, 32, 64), *, hidden: int,
                       n_classes: int, max_iter: int = 200, tolerance_grad: float = 1e-5, **probe_kwargs) -> ProbeCurve:
    """The k-sparse probing curve: one probe per size n on the first n features of ``ranking`` (an ordered feature index,
    for example a row of ``top_label_features``).  ``train`` and ``test`` are the argument tuples of ``add_data`` /
    ``evaluate``: ``(code, labels[, frame_mask[, segments]])``.  ``probe_kwargs`` go to ``SparseProbe``."""
    ranking, sizes = _stream.curve_arguments(ranking, sizes)
    if "features" in probe_kwargs:
        raise ValueError("sparse_probe_curve chooses the features itself: pass the ranking")
    out = {name: torch.zeros(len(sizes), dtype=torch.float64) for name in ("train_loss", "test_loss", "test_accuracy")}
    for j, n in enumerate(sizes):
        probe = SparseProbe(hidden, n_classes, features=ranking[:n], **probe_kwargs)
        probe.add_data(*train)
        out["train_loss"][j] = probe.fit(max_iter=max_iter, tolerance_grad=tolerance_grad).loss
        report = probe.evaluate(*test)
        out["test_loss"][j], out["test_accuracy"][j] = report.loss, report.accuracy
    return ProbeCurve(sizes, out["train_loss"], out["test_loss"], out["test_accuracy"], ranking)


def collect_probe_data(model, utterances, device=None) -> ProbeData:
    """Encode a labelled dataset for a probe.  Every item of ``utterances`` is ``(x [n_utt, T, D], labels [n_utt, T])`` or
    ``(x, labels, frame_mask [n_utt, T])``; T may differ between items.  The module must offer ``encode_compact`` (TopK
    and BatchTopK SAEs; a ReLU SAE's code is dense: ``TypeError``) and is run in eval mode; its previous mode is
    restored."""
    vals, idxs, labs, segs = [], [], [], []
    n_utt = 0
    with _stream.encoding(model, hint="sparse probes are for TopK-family codes"):
        dev = _stream.need_gpu("collect_probe_data", torch.device(device) if device is not None else None)
        for x, labels, mask in _stream.labelled_batches(utterances):
            v, i = _stream.utterance_code(model, x, dev)
            if labels.shape != x.shape[:2]:
                raise ValueError(f"labels {tuple(labels.shape)} do not match the frames {tuple(x.shape[:2])}")
            seg, _ = _stream.frame_segments(v, None, None if mask is None else mask.to(dev), dev, first=n_utt)
            vals.append(v.reshape(-1, v.shape[-1]))
            idxs.append(i.reshape(-1, i.shape[-1]))
            labs.append(labels.to(dev).reshape(-1))
            segs.append(seg)
            n_utt += x.shape[0]
    if not vals:
        raise ValueError("collect_probe_data: no utterances")
    return ProbeData((torch.cat(vals), torch.cat(idxs)), torch.cat(labs), torch.cat(segs), n_utt)
