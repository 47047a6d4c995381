"""ABX phone discrimination: does the code keep phonetic identity, with no classifier and no
clustering in between?

Given three tokens A, B and X - A and X instances of one phone, B of another - X should lie closer to A than to B, where
"closer" is the DTW-aligned frame distance between the tokens.  ``segment_distances`` gives the DTW distance between any
two row ranges of a compact ``(values, indices)`` code (``wsae_dtw_matrix``: cosine or Jaccard frame costs straight from
the code, path-length normalised), which is also query-by-example search.  ``items_from_labels`` cuts a label track into
items.  ``AbxItems`` keeps only the rows of the items of a dataset and ``score`` walks windows of X rows: the distances
of a window against all items, then the integer triple count (``wsae_abx_count``), so the items x items matrix never
exists at once.  ``AbxScores`` are integers: shards add, whatever the order.

Out of scope: the angular (arccos) frame distance, items longer than 64 frames, Sakoe-Chiba bands, the ZeroSpeech
mean-over-contexts-then-speakers hierarchy (a cell pools its triples over contexts and speakers), several GPUs beyond
adding shards.
"""

from __future__ import annotations

from pathlib import Path
from typing import List, Optional, Tuple

import torch
from torch import Tensor

from .. import _native as N
from ..sae.engine import require_device_tensor
from . import _stream
from .dynamics import _check_weights, _segments_of

METRICS = {"cosine": N.DTW_COSINE, "jaccard": N.DTW_JACCARD}
MODES = {"any": N.ABX_ANY, "within": N.ABX_WITHIN, "across": N.ABX_ACROSS}
_CONTEXT_BASE = 1 << 15  # the context id of a store without n_classes: labels below 2^15 - 1


def _check_metric(metric: str) -> int:
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {tuple(METRICS)}, got {metric!r}")
    return METRICS[metric]


def _check_mode(mode: str) -> int:
    if mode not in MODES:
        raise ValueError(f"mode must be one of {tuple(MODES)}, got {mode!r}")
    return MODES[mode]


def _item_pair(starts, lengths, what: str, dev) -> Tuple[Tensor, Tensor]:
    """int32 ``[n]`` starts and lengths on ``dev``."""
    st, ln = torch.as_tensor(starts), torch.as_tensor(lengths)
    if st.dim() != 1 or st.shape != ln.shape or st.is_floating_point() or ln.is_floating_point():
        raise ValueError(f"{what}: starts {tuple(st.shape)} and lengths {tuple(ln.shape)} must be integer tensors of one [n] shape")
    return (st.detach().to(device=dev, dtype=torch.int32).contiguous(), ln.detach().to(device=dev, dtype=torch.int32).contiguous())


def _dtw_call(v, i, k, hidden, seg, weight, a, b, metric, normalize, dist, steps, holder) -> None:
    """``wsae_dtw_matrix`` on a flat code into ``dist [n_a, ldd]`` (and ``steps``); ``holder._ws`` keeps the workspace."""
    rows, dev, lib = v.shape[0], v.device, N.lib()
    n_a, n_b = a[0].numel(), b[0].numel()
    need = lib.wsae_dtw_workspace_bytes(rows, k, hidden, n_a, n_b)
    if need < 0:
        raise N.WsaeError(f"wsae_dtw_workspace_bytes rejects rows={rows} k={k} hidden={hidden} n_a={n_a} n_b={n_b}")
    ws = _stream.workspace(holder, need, dev)
    with torch.cuda.device(dev):
        N.check(lib.wsae_dtw_matrix(v.data_ptr(), i.data_ptr(), k, hidden, N.ptr(seg), N.ptr(weight), rows, a[0].data_ptr(),
                                    a[1].data_ptr(), n_a, b[0].data_ptr(), b[1].data_ptr(), n_b, metric, int(bool(normalize)),
                                    dist.data_ptr(), N.ptr(steps), dist.stride(0), ws.data_ptr(), need,
                                    torch.cuda.current_stream(dev).cuda_stream), "wsae_dtw_matrix")


class _Workspace:
    _ws = None


def segment_distances(code, starts, lengths, other=None, hidden: Optional[int] = None, metric: str = "cosine",
                      normalize: bool = True, weights: Optional[Tensor] = None, segments: Optional[Tensor] = None,
                      frame_mask: Optional[Tensor] = None, return_steps: bool = False):
    """``[n_a, n_b]`` float32: the DTW distance between the items ``[starts, starts + lengths)`` (rows of the flattened
    code) and the items ``other = (starts_b, lengths_b)`` (None: the a-items against themselves).  ``code = (values,
    indices)`` ``[..., T, k]`` or flat ``[rows, k]``.  The frame cost is 1 - cosine (``metric="cosine"``) or 1 - Jaccard of
    the sets of active features (``"jaccard"``); with ``normalize`` the cost of the best path is divided by its length.
    An item with a length outside 1..64 or rows outside the code gives NaN.  ``weights [hidden]`` scale every feature's
    value, a weight <= 0 removes it; frames with ``frame_mask == 0`` or ``segments < 0`` hold no active feature.  With
    ``return_steps`` also the int32 path lengths."""
    vals, idx, k = _stream.compact_code(code, "code", N.DTW_MAX_K, dims=None)
    if vals.dim() < 2:
        raise ValueError(f"code: values {tuple(vals.shape)} must be [..., T, k] or [rows, k]")
    m = _check_metric(metric)
    weight = _check_weights(weights, hidden)
    if other is not None and not (isinstance(other, (tuple, list)) and len(other) == 2):
        raise TypeError("other must be a (starts, lengths) pair")
    dev = _stream.need_gpu("segment_distances", vals.device)
    if weight is not None:
        require_device_tensor(weight, "weights")
    hidden = int(hidden) if hidden is not None else (weight.numel() if weight is not None else 2 ** 31 - 1)
    a = _item_pair(starts, lengths, "items", dev)
    b = a if other is None else _item_pair(other[0], other[1], "other", dev)
    seg = _segments_of(vals, segments, frame_mask, dev)
    v, i = _stream.flat_code(vals, idx, k)
    n_a, n_b = a[0].numel(), b[0].numel()
    dist = torch.full((n_a, n_b), float("nan"), dtype=torch.float32, device=dev)
    steps = torch.zeros((n_a, n_b), dtype=torch.int32, device=dev) if return_steps else None
    if n_a and n_b and v.shape[0]:
        _dtw_call(v, i, k, hidden, seg, weight, a, b, m, normalize, dist, steps, _Workspace())
    return (dist, steps) if return_steps else dist


# ---- items ---------------------------------------------------------------------------------------------------------------------
class LabelItems(tuple):
    """``(starts, lengths, category[, context])`` int32 tensors of ``items_from_labels``; ``dropped_short`` and
    ``dropped_long``: the labelled runs left out for their length."""

    dropped_short = 0
    dropped_long = 0


def items_from_labels(labels: Tensor, segments: Optional[Tensor] = None, frame_mask: Optional[Tensor] = None, min_len: int = 1,
                      max_len: int = N.DTW_MAX_LEN, with_context: bool = False, n_classes: Optional[int] = None) -> LabelItems:
    """The items of a label track: ``labels`` ``[..., T]`` (every leading index an utterance) or flat ``[rows]`` with
    ``segments``; an item is a maximal run of one label >= 0 inside one utterance (frames with ``frame_mask == 0`` or
    ``segments < 0`` end a run) whose length lies in ``min_len..max_len``.  Starts are rows of the flattened track.  With
    ``with_context`` the context id (previous label + 1) (n_classes + 1) + (next label + 1) of the runs next to it in the
    utterance, "none" (-1) at the edges and next to unlabelled frames; ``n_classes`` defaults to the largest label + 1.
    Plain torch, on the device of ``labels`` (CPU tensors work)."""
    if labels.is_floating_point() or labels.dtype == torch.bool or labels.dim() < 1:
        raise ValueError(f"labels must hold one integer per frame, got {tuple(labels.shape)} {labels.dtype}")
    if not 1 <= int(min_len) <= int(max_len) <= N.DTW_MAX_LEN:
        raise ValueError(f"need 1 <= min_len <= max_len <= {N.DTW_MAX_LEN}, got {min_len} and {max_len}")
    dev = labels.device
    lab = labels.detach().reshape(-1).to(torch.int64)
    rows = lab.numel()
    if segments is not None:
        if labels.dim() != 1 or segments.shape != labels.shape:
            raise ValueError("segments go with flat labels [rows] of the same length")
        seg = segments.detach().to(device=dev, dtype=torch.int64)
    elif labels.dim() > 1:
        seg = torch.arange(rows // labels.shape[-1], device=dev).repeat_interleave(labels.shape[-1])
    else:
        seg = torch.zeros(rows, dtype=torch.int64, device=dev)
    if frame_mask is not None:
        if frame_mask.shape != labels.shape:
            raise ValueError(f"frame_mask {tuple(frame_mask.shape)} must have the shape {tuple(labels.shape)} of the labels")
        seg = torch.where(frame_mask.detach().reshape(-1).to(dev) != 0, seg, torch.full_like(seg, -1))
    lab = torch.where(seg >= 0, torch.clamp(lab, min=-1), torch.full_like(lab, -1))
    if n_classes is None:
        n_classes = int(lab.max()) + 1 if rows and int(lab.max()) >= 0 else 1
    head = torch.ones(rows, dtype=torch.bool, device=dev)
    if rows > 1:
        head[1:] = (lab[1:] != lab[:-1]) | (seg[1:] != seg[:-1])
    first = torch.nonzero(head).reshape(-1)
    length = torch.diff(first, append=torch.tensor([rows], device=dev))
    run_lab, run_seg = lab[first], seg[first]
    none = torch.full((1,), -1, dtype=torch.int64, device=dev)
    prev = torch.where(torch.cat([none, run_seg[:-1]]) == run_seg, torch.cat([none, run_lab[:-1]]), none)
    nxt = torch.where(torch.cat([run_seg[1:], none]) == run_seg, torch.cat([run_lab[1:], none]), none)
    labelled = run_lab >= 0
    keep = labelled & (length >= int(min_len)) & (length <= int(max_len))
    parts: List[Tensor] = [first[keep].to(torch.int32), length[keep].to(torch.int32), run_lab[keep].to(torch.int32)]
    if with_context:
        parts.append(((prev[keep] + 1) * (int(n_classes) + 1) + nxt[keep] + 1).to(torch.int32))
    out = LabelItems(parts)
    out.dropped_short = int((labelled & (length < int(min_len))).sum())
    out.dropped_long = int((labelled & (length > int(max_len))).sum())
    return out


# ---- scores --------------------------------------------------------------------------------------------------------------------
class AbxScores:
    """The counts of ``AbxItems.score``, on the host.  ``wins2``, ``total`` int64 ``[n_cats, n_cats]`` (cell [c, c']: X and
    A of category c, B of c'; ``wins2`` counts 2 per triple with X closer to A and 1 per tie), ``skipped`` the admissible
    triples with a NaN distance.  ``score = wins2 / (2 total)`` float64, NaN where ``total == 0``; ``error`` = 1 - the mean
    of ``score`` over the cells with triples.  Two scores add (shards, X windows)."""

    def __init__(self, wins2: Tensor, total: Tensor, skipped: int, mode: str = "any"):
        self.wins2, self.total = wins2.detach().cpu().to(torch.int64), total.detach().cpu().to(torch.int64)
        self.skipped, self.mode = int(skipped), mode

    @property
    def score(self) -> Tensor:
        t = self.total.double()
        return torch.where(self.total > 0, self.wins2.double() / (2.0 * torch.clamp(t, min=1.0)), torch.full_like(t, float("nan")))

    @property
    def n_triples(self) -> int:
        return int(self.total.sum())

    @property
    def error(self) -> float:
        ok = self.total > 0
        return 1.0 - float(self.score[ok].mean()) if bool(ok.any()) else float("nan")

    @property
    def by_category(self) -> Tensor:
        """float64 ``[n_cats]``: the mean score of category c (as X and A) over the categories it met as B; NaN without."""
        ok = self.total > 0
        s = torch.where(ok, self.score, torch.zeros_like(self.score)).sum(1)
        n = ok.sum(1)
        return torch.where(n > 0, s / torch.clamp(n, min=1).double(), torch.full_like(s, float("nan")))

    def confusable(self, n: int = 10) -> List[Tuple[int, int, float]]:
        """The ``n`` cells ``(c, c', score)`` with the lowest score, ascending; ties to the lower cell."""
        score, ok = self.score.reshape(-1), (self.total > 0).reshape(-1)
        order = _stream.rank_features(-torch.where(ok, score, torch.zeros_like(score)), ok, n)
        C = self.total.shape[1]
        return [(int(c) // C, int(c) % C, float(score[c])) for c in order]

    def __add__(self, other: "AbxScores") -> "AbxScores":
        if self.total.shape != other.total.shape or self.mode != other.mode:
            raise ValueError("scores add only with the same categories and mode")
        return AbxScores(self.wins2 + other.wins2, self.total + other.total, self.skipped + other.skipped, self.mode)


# ---- the item store ------------------------------------------------------------------------------------------------------------
def _gather_rows(starts: Tensor, lengths: Tensor) -> Tensor:
    """int64: the rows of the items, item after item."""
    ln = lengths.to(torch.int64)
    off = torch.cumsum(ln, 0) - ln
    total = int(ln.sum())
    return torch.arange(total, device=ln.device) - off.repeat_interleave(ln) + starts.to(torch.int64).repeat_interleave(ln)


class AbxItems:
    """The items of a dataset for ABX scoring: only the rows of the items are kept (the speech of thousands of utterances
    shrinks to the frames of its phone tokens), with the category, context and speaker of every item.  ``hidden``: the
    dictionary size; ``metric``, ``normalize``, ``weights`` as in ``segment_distances``."""

    def __init__(self, hidden: int, metric: str = "cosine", normalize: bool = True, weights: Optional[Tensor] = None, device=None):
        if int(hidden) < 1:
            raise ValueError(f"hidden must be positive, got {hidden}")
        _check_metric(metric)
        self.hidden, self.metric, self.normalize = int(hidden), metric, bool(normalize)
        self.weights = _check_weights(weights, self.hidden)
        self.device = torch.device(device) if device is not None else None
        self.k: Optional[int] = None
        self._chunks: List[dict] = []
        self._has_context, self._has_speaker = True, True
        self._ws = None

    def _ensure_device(self, like: Optional[Tensor] = None) -> torch.device:
        dev = _stream.need_gpu("AbxItems", self.device or (like.device if like is not None else None))
        if self.device is None or self.device.index is None:
            self.device = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        if self.weights is not None:
            self.weights = self.weights.to(self.device)
        return self.device

    def _flat(self) -> dict:
        """The store as one chunk (the chunks are concatenated once and the starts re-based)."""
        if len(self._chunks) > 1:
            out, base = {}, 0
            starts = []
            for c in self._chunks:
                starts.append(c["starts"] + base)
                base += c["vals"].shape[0]
            for name in ("vals", "idx", "seg", "lengths", "category", "context", "speaker"):
                out[name] = torch.cat([c[name] for c in self._chunks])
            out["starts"] = torch.cat(starts)
            self._chunks = [out]
        return self._chunks[0] if self._chunks else None

    n_items = property(lambda self: sum(c["starts"].numel() for c in self._chunks), doc="The items kept.")
    n_rows = property(lambda self: sum(c["vals"].shape[0] for c in self._chunks), doc="The rows kept.")
    starts = property(lambda self: self._flat()["starts"], doc="int32 ``[n_items]``: the first row of every item in the store.")
    lengths = property(lambda self: self._flat()["lengths"], doc="int32 ``[n_items]``.")
    category = property(lambda self: self._flat()["category"], doc="int32 ``[n_items]``.")
    context = property(lambda self: self._flat()["context"], doc="int32 ``[n_items]`` (0 where none was given).")
    speaker = property(lambda self: self._flat()["speaker"], doc="int32 ``[n_items]`` (-1 where none was given).")

    def _append(self, v, i, seg, lengths, category, context, speaker) -> None:
        if self.k is not None and v.shape[1] != self.k:
            raise ValueError(f"this store holds codes of k = {self.k}, got k = {v.shape[1]}")
        self.k = v.shape[1]
        ln = lengths.to(torch.int64)
        self._chunks.append({"vals": v, "idx": i, "seg": seg, "starts": (torch.cumsum(ln, 0) - ln).to(torch.int32),
                             "lengths": lengths, "category": category, "context": context, "speaker": speaker})

    def add(self, code, labels: Optional[Tensor] = None, items=None, speakers=None, frame_mask: Optional[Tensor] = None,
            segments: Optional[Tensor] = None, min_len: int = 1, max_len: int = N.DTW_MAX_LEN,
            n_classes: Optional[int] = None) -> int:
        """The items of one batch: ``code = (values, indices)`` ``[n_utt, T, k]`` or flat ``[rows, k]``; either ``labels``
        (one integer per frame: ``items_from_labels`` with contexts, ``n_classes`` fixing the context ids across batches)
        or ``items = (starts, lengths, category[, context])`` in rows of the flattened code.  ``speakers``: an int, or one id per
        utterance of a ``[n_utt, T, k]`` code with ``labels``, one per item with ``items``.  Returns the number of items added."""
        also = () if labels is None else ((labels, "labels"),)
        vals, idx, k = _stream.compact_code(code, "code", N.DTW_MAX_K, also=also)
        dev = self._ensure_device(vals)
        if vals.device != dev:
            raise N.WsaeError(f"the code is on {vals.device}, the store on {dev}")
        if (labels is None) == (items is None):
            raise ValueError("add needs labels or items (one of them)")
        v, i = _stream.flat_code(vals, idx, k)
        rows = v.shape[0]
        if labels is not None:
            _stream.check_frame_labels(vals, labels)
            base = _CONTEXT_BASE if n_classes is None else int(n_classes)
            items = items_from_labels(labels.to(dev), segments, frame_mask, min_len, max_len, with_context=True, n_classes=base)
        elif not (isinstance(items, (tuple, list)) and len(items) in (3, 4)):
            raise TypeError("items must be (starts, lengths, category) or (starts, lengths, category, context)")
        st, ln = _item_pair(items[0], items[1], "items", dev)
        cat = torch.as_tensor(items[2]).detach().to(device=dev, dtype=torch.int32).reshape(-1)
        if cat.numel() != st.numel():
            raise ValueError(f"items: {cat.numel()} categories for {st.numel()} items")
        if st.numel() and bool(((ln < 1) | (ln > N.DTW_MAX_LEN) | (st < 0) | (st.to(torch.int64) + ln > rows)).any()):
            raise ValueError(f"items: every item needs 1 <= length <= {N.DTW_MAX_LEN} and rows inside the {rows} rows of the code")
        if len(items) == 4:
            ctx = torch.as_tensor(items[3]).detach().to(device=dev, dtype=torch.int32).reshape(-1)
            if ctx.numel() != st.numel():
                raise ValueError(f"items: {ctx.numel()} contexts for {st.numel()} items")
        else:
            ctx, self._has_context = torch.zeros_like(cat), False
        if speakers is None:
            spk, self._has_speaker = torch.full_like(cat, -1), False
        else:
            spk = torch.as_tensor(speakers).detach().to(device=dev, dtype=torch.int32).reshape(-1)
            per_utt = labels is not None and vals.dim() == 3  # (with labels: one id per utterance; with items: per item)
            if spk.numel() == 1:
                spk = spk.expand(st.numel())
            elif per_utt and spk.numel() == vals.shape[0]:
                spk = spk[(st // vals.shape[1]).to(torch.int64)]
            elif per_utt or spk.numel() != st.numel():
                raise ValueError(f"speakers: {spk.numel()} ids for " +
                                 (f"{vals.shape[0]} utterances" if per_utt else f"{st.numel()} items"))
        seg = torch.zeros(rows, dtype=torch.int32, device=dev)
        if vals.dim() == 2 and segments is not None or frame_mask is not None:
            flat_seg = segments if vals.dim() == 2 and segments is not None else None
            if vals.dim() == 2 and flat_seg is None:
                flat_seg = torch.zeros(rows, dtype=torch.int32, device=dev)
            seg = torch.clamp(_stream.frame_segments(vals, flat_seg, frame_mask, dev)[0], max=0)
        take = _gather_rows(st, ln)
        self._append(v[take], i[take], seg[take].contiguous(), ln, cat.contiguous(), ctx.contiguous(), spk.contiguous())
        return st.numel()

    def _same_kind(self, other: "AbxItems") -> bool:
        if (self.hidden, self.metric, self.normalize) != (other.hidden, other.metric, other.normalize):
            return False
        if self.k is not None and other.k is not None and self.k != other.k:
            return False
        if (self.weights is None) != (other.weights is None):
            return False
        return self.weights is None or torch.equal(self.weights.cpu().view(torch.int32), other.weights.cpu().view(torch.int32))

    def merge(self, other: "AbxItems") -> None:
        """Add the items of a store of the same kind (size, k, metric, normalisation, weights bit for bit)."""
        if not self._same_kind(other):
            raise ValueError("merge needs two stores with the same size, k, metric, normalisation and weights")
        if other.n_items:
            dev = self._ensure_device(other._flat()["vals"])
            c = other._flat()
            self._append(*(c[name].to(dev) for name in ("vals", "idx", "seg", "lengths", "category", "context", "speaker")))
        self._has_context, self._has_speaker = self._has_context and other._has_context, self._has_speaker and other._has_speaker

    def _like(self) -> "AbxItems":
        out = AbxItems(self.hidden, self.metric, self.normalize, self.weights, self.device)
        out._has_context, out._has_speaker = self._has_context, self._has_speaker
        return out

    def subsample(self, max_items: int, seed: int = 0) -> "AbxItems":
        """A store of at most ``max_items`` items drawn uniformly without replacement (in their order); the same for
        the same ``seed``."""
        out = self._like()
        if not self.n_items:
            return out
        c = self._flat()
        n = c["starts"].numel()
        pick = torch.arange(n)
        if int(max_items) < n:
            pick = torch.sort(torch.randperm(n, generator=torch.Generator().manual_seed(int(seed)))[:max(int(max_items), 0)])[0]
        pick = pick.to(c["starts"].device)
        take = _gather_rows(c["starts"][pick], c["lengths"][pick])
        out._append(c["vals"][take], c["idx"][take], c["seg"][take], c["lengths"][pick], c["category"][pick], c["context"][pick],
                    c["speaker"][pick])
        return out

    def distances(self, rows: Optional[Tuple[int, int]] = None, out: Optional[Tensor] = None) -> Tensor:
        """float32 ``[n, n_items]``: the distances of the items ``rows = (lo, hi)`` (None: all) against all items."""
        n = self.n_items
        lo, hi = (0, n) if rows is None else (int(rows[0]), int(rows[1]))
        if not 0 <= lo <= hi <= n:
            raise ValueError(f"rows {rows} are outside the {n} items")
        dev = self._ensure_device()
        dist = out[:hi - lo] if out is not None else torch.empty(hi - lo, n, dtype=torch.float32, device=dev)
        if hi > lo:
            c = self._flat()
            _dtw_call(c["vals"], c["idx"], self.k, self.hidden, c["seg"], self.weights, (c["starts"][lo:hi], c["lengths"][lo:hi]),
                      (c["starts"], c["lengths"]), METRICS[self.metric], self.normalize, dist, None, self)
        return dist

    def score(self, mode: str = "any", row_block: int = 1024, with_context: Optional[bool] = None,
              n_cats: Optional[int] = None) -> AbxScores:
        """The ABX counts over all triples of the store.  ``mode``: ``"any"`` (speakers ignored), ``"within"`` (A, B and X
        of one speaker) or ``"across"`` (A and B of one speaker, X of another).  A, B and X share a context where the
        items carry one (``with_context``: None = where every item has one).  X is walked in windows of ``row_block``
        items: their distances against all items, then the count."""
        m = _check_mode(mode)
        if int(row_block) < 1:
            raise ValueError(f"row_block must be positive, got {row_block}")
        if m != N.ABX_ANY and not self._has_speaker:
            raise ValueError(f"mode {mode!r} needs speakers on every item of the store")
        use_ctx = self._has_context if with_context is None else bool(with_context)
        if use_ctx and not self._has_context:
            raise ValueError("with_context needs a context on every item of the store")
        dev = self._ensure_device()
        n = self.n_items
        c = self._flat()
        top = int(c["category"].max()) + 1 if n else 1
        n_cats = max(top, 1) if n_cats is None else int(n_cats)
        if not 1 <= n_cats <= N.ABX_MAX_CATS:
            raise ValueError(f"the categories must lie below {N.ABX_MAX_CATS}, got {n_cats}")
        wins2 = torch.zeros(n_cats, n_cats, dtype=torch.int64, device=dev)
        total, skipped = torch.zeros_like(wins2), torch.zeros(1, dtype=torch.int64, device=dev)
        if n:
            lib, block = N.lib(), min(int(row_block), n)
            dist = torch.empty(block, n, dtype=torch.float32, device=dev)
            need = lib.wsae_abx_workspace_bytes(n, block, n_cats)
            count_ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
            for lo in range(0, n, block):
                hi = min(lo + block, n)
                self.distances((lo, hi), out=dist)
                with torch.cuda.device(dev):
                    N.check(lib.wsae_abx_count(dist.data_ptr(), dist.stride(0), lo, hi - lo, n, c["category"].data_ptr(),
                                               c["context"].data_ptr() if use_ctx else 0, c["speaker"].data_ptr(), n_cats, m,
                                               wins2.data_ptr(), total.data_ptr(), skipped.data_ptr(), count_ws.data_ptr(), need,
                                               torch.cuda.current_stream(dev).cuda_stream), "wsae_abx_count")
        return AbxScores(wins2, total, int(skipped.item()), mode)

    def save(self, path) -> None:
        c = self._flat()
        torch.save({"hidden": self.hidden, "metric": self.metric, "normalize": self.normalize, "k": self.k,
                    "weights": None if self.weights is None else self.weights.cpu(), "has_context": self._has_context,
                    "has_speaker": self._has_speaker, "store": None if c is None else {name: t.cpu() for name, t in c.items()}},
                   Path(path))

    @classmethod
    def load(cls, path, device=None) -> "AbxItems":
        data = torch.load(Path(path), map_location="cpu", weights_only=True)
        s = cls(data["hidden"], data["metric"], data["normalize"], data["weights"], device=device)
        s._has_context, s._has_speaker = bool(data["has_context"]), bool(data["has_speaker"])
        if data["store"] is not None:
            dev = s._ensure_device()
            s.k = int(data["k"])
            s._chunks = [{name: t.to(dev) for name, t in data["store"].items()}]
        return s


# ---- over a dataset --------------------------------------------------------------------------------------------------------------
class _DenseCode:
    """A module with a dense ReLU code seen as one with a compact code: all ``hidden <= 128`` entries of a frame, or the
    128 largest where no frame has more active ones."""

    def __init__(self, module):
        self.module, self.hidden_dim = module, module.hidden_dim

    training = property(lambda self: self.module.training)

    def eval(self):
        self.module.eval()

    def train(self, mode: bool = True):
        self.module.train(mode)

    def encode_compact(self, x: Tensor):
        h = self.module(x.reshape(-1, x.shape[-1])).hidden
        h = h.reshape(-1, h.shape[-1]).float()
        if h.shape[1] > N.DTW_MAX_K and int((h > 0).sum(1).max()) > N.DTW_MAX_K:
            raise N.WsaeError(f"a frame of this dense code has more than {N.DTW_MAX_K} active features: no compact code holds it")
        vals, idx = torch.topk(h, min(h.shape[1], N.DTW_MAX_K), dim=1)
        return vals, idx.to(torch.int32)


def compact_module(model):
    """``model`` itself where it offers ``encode_compact`` (TopK, BatchTopK), a view with one for a ReLU SAE."""
    return _DenseCode(model) if not hasattr(model, "encode_compact") and getattr(model, "is_relu", False) else model


def collect_abx(model, utterances, mode: str = "any", max_len: int = N.DTW_MAX_LEN, with_context: bool = False, speakers=None,
                max_items: Optional[int] = None, seed: int = 0, metric: str = "cosine", normalize: bool = True,
                weights: Optional[Tensor] = None, min_len: int = 1, n_classes: Optional[int] = None, row_block: int = 1024,
                device="cuda", return_items: bool = False):
    """The ABX scores of a module over a dataset.  Every item of ``utterances`` is ``(x [n_utt, T, D], labels [n_utt, T])``
    or ``(x, labels, frame_mask)``; the phone tokens are the runs of one label (``items_from_labels``, ``min_len`` ..
    ``max_len`` frames).  ``speakers``: one id per utterance of the whole dataset, in order (needed by ``"within"`` and
    ``"across"``).  ``max_items``: score a uniform subsample of that many items (``seed``).  The module must offer
    ``encode_compact`` (TopK and BatchTopK SAEs) or be a ReLU SAE, and is run in eval mode; its previous mode is
    restored.  With ``return_items`` also the ``AbxItems`` store."""
    _check_mode(mode), _check_metric(metric)
    model = compact_module(model)
    with _stream.encoding(model, hint="ABX scores need a compact code or a ReLU SAE"):
        store = AbxItems(model.hidden_dim, metric, normalize, weights, device=device)
        seen = 0
        for x, labels, mask in _stream.labelled_batches(utterances):
            spk = None
            if speakers is not None:
                spk = torch.as_tensor(speakers).reshape(-1)[seen:seen + x.shape[0]]
                if spk.numel() != x.shape[0]:
                    raise ValueError(f"speakers holds {torch.as_tensor(speakers).numel()} ids, the dataset more utterances")
            store.add(_stream.utterance_code(model, x, device), labels=labels.to(device), speakers=spk,
                      frame_mask=None if mask is None else mask.to(device), min_len=min_len, max_len=max_len, n_classes=n_classes)
            seen += x.shape[0]
    if max_items is not None:
        store = store.subsample(max_items, seed)
    scores = store.score(mode, row_block, with_context=with_context, n_cats=n_classes)
    return (scores, store) if return_items else scores
