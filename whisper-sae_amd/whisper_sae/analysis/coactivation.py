"""Co-activation statistics: which features fire together, which feature of SAE B fires on the
same frames as feature f of SAE A, which features are redundant in use although their directions differ.

All of it is one computation over a stream of activation rows: for every pair (feature i of code A, feature j of code B)
the number of rows on which both fire (``wsae_coact_update``, straight from the compact ``(values, indices)`` code - the
dense ``[B, H]`` matrices never exist), then per feature the strongest partners under a normalised score
(``wsae_coact_top`` - the score matrix never exists either).  The state is integer, so a table does not depend on the
order of the batches, on how they were split or on the launch geometry.  The reductions over ``[H]`` vectors are plain
torch.

Out of scope: magnitude-weighted (Pearson on the values) correlation, dense / ReLU codes (the dense GEMM is the right
tool there), data-parallel reduction of the tables beyond ``merge``, optimal one-to-one (Hungarian) assignment, plots.
"""

from __future__ import annotations

from pathlib import Path
from typing import NamedTuple, Optional, Tuple

import torch
from torch import Tensor

from .. import _native as N
from ..sae.engine import require_device_tensor
from . import _stream

_METRICS = {"count": N.COACT_COUNT, "cond": N.COACT_COND, "jaccard": N.COACT_JACCARD, "phi": N.COACT_PHI}
MAX_ROWS = _stream.MAX_ROWS  # the marginals and the table cells are int32 ("rows", not "frames": its own two messages)


class CoactivationNeighbors(NamedTuple):
    """``values [rows, n]`` float32, ``indices [rows, n]`` int32 and ``counts [rows, n]`` int32 (the raw co-firing count
    of each pair), per row sorted by value descending, then index ascending; where fewer than ``n`` candidates exist the
    tail is ``(-inf, -1, 0)``."""

    values: Tensor
    indices: Tensor
    counts: Tensor


def _code(code, what: str) -> Tuple[Tensor, Tensor]:
    """``(values, indices)`` of any leading shape -> contiguous ``[rows, k]`` float32 / int32 device tensors."""
    return _stream.flat_code(*_stream.compact_code(code, what, N.COACT_MAX_K, dims=None))


class CoactivationTracker:
    """Co-firing counts of two compact codes over a stream of rows.

    ``hidden_b=None``: one code against itself (the table is symmetric, its diagonal the firing counts).
    ``a_window=(a_lo, a_rows)``: keep only the table rows of features ``a_lo .. a_lo + a_rows - 1`` of A, so that a large
    pair of dictionaries is processed in passes (40960 x 40960 int32 is 6.7 GB); the firing counts always cover every
    feature.  The state lives on the device of the first update (or ``device``)."""

    def __init__(self, hidden_a: int, hidden_b: Optional[int] = None, *, a_window: Optional[Tuple[int, int]] = None,
                 device=None):
        self.hidden_a = int(hidden_a)
        self.is_self = hidden_b is None
        self.hidden_b = self.hidden_a if hidden_b is None else int(hidden_b)
        if self.hidden_a < 1 or self.hidden_b < 1:
            raise ValueError(f"hidden sizes must be positive, got {hidden_a}, {hidden_b}")
        self.a_lo, self.a_rows = _stream.feature_window(a_window, self.hidden_a, "a_window")
        self.device = torch.device(device) if device is not None else None
        self._ldc = (self.hidden_b + 3) // 4 * 4  # 16-byte rows: wsae_coact_top then loads 16 bytes per lane
        self._counts: Optional[Tensor] = None
        self._fire_a: Optional[Tensor] = None
        self._fire_b: Optional[Tensor] = None
        self._total: Optional[Tensor] = None
        self._submitted = 0  # rows handed to update so far, masked ones included (host-side bound of the int32 state)

    # ---- state ----------------------------------------------------------------------------------
    @property
    def full_window(self) -> bool:
        return self.a_lo == 0 and self.a_rows == self.hidden_a

    def _ensure_device(self, like: Optional[Tensor] = None) -> torch.device:
        if self._counts is not None:
            return self._counts.device
        dev = _stream.need_gpu("CoactivationTracker", self.device or (like.device if like is not None else None))
        self._counts = torch.zeros(self.a_rows, self._ldc, dtype=torch.int32, device=dev)
        self._fire_a = torch.zeros(self.hidden_a, dtype=torch.int32, device=dev)
        self._fire_b = None if self.is_self else torch.zeros(self.hidden_b, dtype=torch.int32, device=dev)
        self._total = torch.zeros(1, dtype=torch.int64, device=dev)
        self.device = self._counts.device  # (with its index: "cuda" has become "cuda:0")
        return self.device

    @property
    def counts(self) -> Tensor:
        """``[a_rows, hidden_b]`` int32 view of the table: ``counts[i - a_lo, j]`` rows on which i and j both fired."""
        self._ensure_device()
        return self._counts[:, :self.hidden_b]

    @property
    def fire_a(self) -> Tensor:
        self._ensure_device()
        return self._fire_a

    @property
    def fire_b(self) -> Tensor:
        self._ensure_device()
        return self._fire_a if self.is_self else self._fire_b

    @property
    def rows(self) -> int:
        """Rows that contributed so far (synchronises the device)."""
        return 0 if self._total is None else int(self._total.item())

    # ---- accumulation ---------------------------------------------------------------------------
    def update(self, code_a, code_b=None, row_mask: Optional[Tensor] = None) -> None:
        """One batch: ``code = (values, indices)`` of any leading shape, as ``encode_compact`` returns it; an entry is
        active iff its value is positive.  ``code_b=None``: the code against itself (self-trackers only).  ``row_mask``:
        one flag per row, rows with a zero flag contribute nothing."""
        va, ia = _code(code_a, "code_a")
        if code_b is None:
            if not self.is_self:
                raise ValueError("this tracker compares two codes: update needs code_b")
            vb, ib = va, ia
        else:
            if self.is_self:
                raise ValueError("this tracker compares a code with itself: build it with hidden_b= to pass code_b")
            vb, ib = _code(code_b, "code_b")
            if vb.shape[0] != va.shape[0]:
                raise ValueError(f"code_a has {va.shape[0]} rows and code_b {vb.shape[0]}")
            if vb.device != va.device:
                raise N.WsaeError(f"the codes are on different devices: {va.device} and {vb.device}")
        rows = va.shape[0]
        dev = self._ensure_device(va)
        if va.device != dev:
            raise N.WsaeError(f"the code is on {va.device}, the tracker on {dev}")
        mask = None
        if row_mask is not None:
            require_device_tensor(row_mask, "row_mask")
            if row_mask.numel() != rows:
                raise ValueError(f"row_mask has {row_mask.numel()} flags for {rows} rows")
            mask = (row_mask.detach().reshape(-1) != 0).to(device=dev, dtype=torch.uint8).contiguous()
        if self._submitted + rows > MAX_ROWS:
            raise N.WsaeError(f"CoactivationTracker: {self._submitted} + {rows} rows exceed {MAX_ROWS}, the range of the int32 "
                              f"counts; merge the tables of shorter runs in a wider type instead")
        if rows == 0:
            return
        with torch.cuda.device(dev):
            N.check(N.lib().wsae_coact_update(
                va.data_ptr(), ia.data_ptr(), va.shape[1], self.hidden_a, vb.data_ptr(), ib.data_ptr(), vb.shape[1],
                self.hidden_b, rows, N.ptr(mask), self.a_lo, self.a_rows, self._counts.data_ptr(), self._ldc,
                self._fire_a.data_ptr(), N.ptr(self._fire_b), self._total.data_ptr(), None, 0,
                torch.cuda.current_stream(dev).cuda_stream), "wsae_coact_update")
        self._submitted += rows

    def merge(self, other: "CoactivationTracker") -> None:
        """Add the tables of a tracker of the same shape (another shard of the dataset)."""
        same = (self.hidden_a, self.hidden_b, self.is_self, self.a_lo, self.a_rows) == \
               (other.hidden_a, other.hidden_b, other.is_self, other.a_lo, other.a_rows)
        if not same:
            raise ValueError("merge needs two trackers of the same sizes, window and kind")
        if self._submitted + other._submitted > MAX_ROWS:
            raise N.WsaeError(f"CoactivationTracker.merge: {self._submitted} + {other._submitted} rows exceed {MAX_ROWS}")
        if other._counts is None:
            return
        dev = self._ensure_device(other._counts)
        self._counts += other._counts.to(dev)
        self._fire_a += other._fire_a.to(dev)
        if not self.is_self:
            self._fire_b += other._fire_b.to(dev)
        self._total += other._total.to(dev)
        self._submitted += other._submitted

    # ---- reading --------------------------------------------------------------------------------
    def neighbors(self, n: int = 4, metric: str = "jaccard", min_count: int = 1, exclude_self: Optional[bool] = None,
                  side: str = "a") -> CoactivationNeighbors:
        """Per feature its ``n`` strongest partners.  ``metric``: ``"count"`` (c), ``"cond"`` (c / n_i), ``"jaccard"``
        (c / (n_i + m_j - c)) or ``"phi"`` (the correlation of the two firing indicators), each computed in fp64 from the
        integers and rounded once to float32.  Pairs with fewer than ``min_count`` common rows are no candidates.
        ``side="a"``: the partners in B of the window's features of A; ``side="b"``: the partners in A of every feature
        of B (full window only).  ``exclude_self`` defaults to true for a self-tracker."""
        if metric not in _METRICS:
            raise ValueError(f"metric must be one of {sorted(_METRICS)}, got {metric!r}")
        if not 1 <= int(n) <= N.MATCH_MAX_N:
            raise ValueError(f"n must be in 1..{N.MATCH_MAX_N}, got {n}")
        if int(min_count) < 0:
            raise ValueError(f"min_count must not be negative, got {min_count}")
        if side not in ("a", "b"):
            raise ValueError(f"side must be 'a' or 'b', got {side!r}")
        if exclude_self is None:
            exclude_self = self.is_self
        dev = self._ensure_device()
        n = int(n)
        if side == "a":
            table, ldc, lo, rows, width = self._counts, self._ldc, self.a_lo, self.a_rows, self.hidden_b
            f_row, f_col = self._fire_a, self.fire_b
        else:
            if not self.full_window:
                raise ValueError("side='b' needs the whole table: this tracker keeps only a window of A's features")
            table = self.counts.t().contiguous()
            ldc, lo, rows, width = self.hidden_a, 0, self.hidden_b, self.hidden_a
            f_row, f_col = self.fire_b, self._fire_a
        with torch.cuda.device(dev):
            values = torch.empty(rows, n, dtype=torch.float32, device=dev)
            indices = torch.empty(rows, n, dtype=torch.int32, device=dev)
            counts = torch.empty(rows, n, dtype=torch.int32, device=dev)
            N.check(N.lib().wsae_coact_top(table.data_ptr(), ldc, lo, rows, width, f_row.data_ptr(), f_col.data_ptr(),
                                           self._total.data_ptr(), _METRICS[metric], int(min_count), 1 if exclude_self else 0,
                                           n, values.data_ptr(), indices.data_ptr(), counts.data_ptr(), None, 0,
                                           torch.cuda.current_stream(dev).cuda_stream), "wsae_coact_top")
        return CoactivationNeighbors(values, indices, counts)

    # ---- persistence ----------------------------------------------------------------------------
    def save(self, path) -> None:
        self._ensure_device()
        torch.save({"hidden_a": self.hidden_a, "hidden_b": None if self.is_self else self.hidden_b,
                    "a_window": [self.a_lo, self.a_rows], "submitted": self._submitted, "counts": self.counts.cpu(),
                    "fire_a": self._fire_a.cpu(), "fire_b": None if self.is_self else self._fire_b.cpu(),
                    "total_rows": self._total.cpu()}, Path(path))

    @classmethod
    def load(cls, path, device=None) -> "CoactivationTracker":
        data = torch.load(Path(path), map_location="cpu", weights_only=True)
        t = cls(data["hidden_a"], data["hidden_b"], a_window=tuple(data["a_window"]), device=device)
        dev = t._ensure_device()
        t._counts[:, :t.hidden_b] = data["counts"].to(dev)
        t._fire_a.copy_(data["fire_a"])
        if not t.is_self:
            t._fire_b.copy_(data["fire_b"])
        t._total.copy_(data["total_rows"])
        t._submitted = int(data["submitted"])
        return t


def collect_coactivation(model_a, model_b=None, dataloader=None, *, a_window: Optional[Tuple[int, int]] = None,
                         device="cuda") -> CoactivationTracker:
    """Co-activation tables over a dataset.  ``model_b=None``: ``model_a``'s features with each other.  Every module
    must offer ``encode_compact`` (TopK and BatchTopK SAEs; a ReLU SAE's code is dense: ``TypeError``) and is run in
    eval mode; its previous mode is restored.  A batch is one tensor for both modules, or a pair ``(x_a, x_b)`` with
    equal leading shape for two layers (with one module, a pair's first element is the input, as in
    ``collect_top_activations``)."""
    if dataloader is None:
        raise TypeError("collect_coactivation needs a dataloader")
    models = [model_a] if model_b is None else [model_a, model_b]
    with _stream.encoding(*models, hint="co-activation statistics are for TopK-family codes; use a dense matrix product for a "
                                  "ReLU SAE"):
        tracker = CoactivationTracker(model_a.hidden_dim, None if model_b is None else model_b.hidden_dim,
                                      a_window=a_window, device=device)
        for batch in dataloader:
            if isinstance(batch, (tuple, list)):
                xs = [batch[0], batch[1] if model_b is not None and len(batch) > 1 and isinstance(batch[1], Tensor)
                      else batch[0]]
            else:
                xs = [batch, batch]
            if xs[0].shape[:-1] != xs[1].shape[:-1]:
                raise ValueError(f"the two inputs of a batch differ in leading shape: {tuple(xs[0].shape)} and "
                                 f"{tuple(xs[1].shape)}")
            codes = [m.encode_compact(x.to(device)) for m, x in zip(models, xs)]
            tracker.update(codes[0], codes[1] if model_b is not None else None)
    return tracker


def _side(best: Tensor, thresholds) -> dict:
    return {"mean_best_phi": float(best.mean()),
            "fraction_at_least": {str(float(t)): float((best >= float(t)).float().mean()) for t in thresholds},
            "histogram": {"lo": -1.0, "hi": 1.0,
                          "counts": [int(c) for c in torch.histc(best.clamp(-1.0, 1.0), bins=20, min=-1.0, max=1.0).cpu()]}}


def compare_activations(tracker: CoactivationTracker, thresholds=(0.5, 0.7, 0.9)) -> dict:
    """Summary of how two dictionaries overlap in use, as plain JSON shaped like ``compare_dictionaries``: the mean over
    each side's features of the best partner's phi, per threshold the fraction of each side's features whose best
    partner reaches it, the mutual best partners (``[i, j]``) and a 20-bin histogram over ``[-1, 1]`` of the best phi of
    each side.  A feature without a partner (it never fired with anything) counts as phi 0.  Needs a full window."""
    if not tracker.full_window:
        raise ValueError("compare_activations needs the whole table: this tracker keeps only a window of A's features")
    ab = tracker.neighbors(n=1, metric="phi", min_count=1, side="a")
    ba = tracker.neighbors(n=1, metric="phi", min_count=1, side="b")
    ia, ib = ab.indices[:, 0].long(), ba.indices[:, 0].long()
    va = torch.where(ia >= 0, ab.values[:, 0], torch.zeros_like(ab.values[:, 0]))
    vb = torch.where(ib >= 0, ba.values[:, 0], torch.zeros_like(ba.values[:, 0]))
    back = torch.where(ia >= 0, ib[ia.clamp(min=0)], torch.full_like(ia, -1))
    mi = torch.nonzero(back == torch.arange(ia.shape[0], device=ia.device)).flatten()
    sa, sb = _side(va, thresholds), _side(vb, thresholds)
    return {"rows": tracker.rows, "features_a": int(va.shape[0]), "features_b": int(vb.shape[0]),
            "mean_best_phi_a_to_b": sa["mean_best_phi"], "mean_best_phi_b_to_a": sb["mean_best_phi"],
            "fraction_at_least": {"a": sa["fraction_at_least"], "b": sb["fraction_at_least"]},
            "mutual_best": int(mi.numel()),
            "mutual_pairs": [[int(i), int(j)] for i, j in zip(mi.cpu().tolist(), ia[mi].cpu().tolist())],
            "histogram": {"a": sa["histogram"], "b": sb["histogram"]}}
