"""Group effect sizes: which features separate two groups of utterances (speaker gender, accent,
language, read vs. spontaneous speech), and how sure are we?

The statistical unit is the utterance, not the frame: ``SegmentPooler`` sums a compact ``(values, indices)`` code over the
frames of each utterance (``wsae_pool_update`` - the dense ``[frames, H]`` matrix never exists, and the fp32 sums are in
row order, so they do not depend on how the frames were batched), and ``group_effect_sizes`` compares two groups of
utterances per feature: Cohen's d and Hedges' g with stratified-bootstrap percentile intervals (``wsae_group_effect``,
fp64 throughout - the ``[replicates, H]`` matrix never exists either).  The draws of ``bootstrap_weights`` come from a CPU
generator, so an analysis is the same on every machine.

Out of scope: permutation tests and p-values, power analysis, more than two groups at once (one-vs-rest is a loop),
frame-level resampling, max pooling, data-parallel merging of poolers, plots.
"""

from __future__ import annotations

from pathlib import Path
from typing import NamedTuple, Optional, Tuple

import torch
from torch import Tensor

from .. import _native as N
from ..sae.engine import require_device_tensor
from . import _stream


class GroupEffects(NamedTuple):
    """Per feature of the window, float64: Cohen's ``d`` (group a minus group b over the pooled standard deviation),
    Hedges' ``g``, the group means, the bootstrap percentile interval ``ci_lo .. ci_hi`` of d and its bootstrap standard
    error ``se`` (NaN without replicates); ``n_a``, ``n_b``: the utterances compared, ``n_boot``: the replicates kept."""

    d: Tensor
    g: Tensor
    mean_a: Tensor
    mean_b: Tensor
    ci_lo: Tensor
    ci_hi: Tensor
    se: Tensor
    n_a: int
    n_b: int
    n_boot: int


class SegmentPooler:
    """Per-utterance sums of a compact code.

    ``f_window=(f_lo, f_cols)``: keep only the features ``f_lo .. f_lo + f_cols - 1`` (a 40960-wide dictionary over many
    utterances is processed in passes).  ``counts=True`` also keeps, per utterance and feature, the number of frames on
    which the feature fired.  The state lives on the device of the first update (or ``device``)."""

    def __init__(self, hidden: int, n_segments: int, *, f_window: Optional[Tuple[int, int]] = None, counts: bool = False,
                 device=None):
        self.hidden, self.n_segments = int(hidden), int(n_segments)
        if self.hidden < 1 or self.n_segments < 1:
            raise ValueError(f"hidden and n_segments must be positive, got {hidden}, {n_segments}")
        self.f_lo, self.f_cols = _stream.feature_window(f_window, self.hidden)
        self.with_counts = bool(counts)
        self.device = torch.device(device) if device is not None else None
        self._ld = (self.f_cols + 3) // 4 * 4
        self._sum: Optional[Tensor] = None
        self._cnt: Optional[Tensor] = None
        self._rows: Optional[Tensor] = None
        self._ws: Optional[Tensor] = None
        self._next = 0       # the segment a 3-D code's first utterance gets
        self._submitted = 0  # frames handed to update so far (host-side bound of the int32 state)

    # ---- state ----------------------------------------------------------------------------------
    def _ensure_device(self, like: Optional[Tensor] = None) -> torch.device:
        if self._sum is not None:
            return self._sum.device
        dev = _stream.need_gpu("SegmentPooler", self.device or (like.device if like is not None else None))
        self._sum = torch.zeros(self.n_segments, self._ld, dtype=torch.float32, device=dev)
        self._cnt = torch.zeros(self.n_segments, self._ld, dtype=torch.int32, device=dev) if self.with_counts else None
        self._rows = torch.zeros(self.n_segments, dtype=torch.int32, device=dev)
        self._ws = torch.empty(2 * self.n_segments, dtype=torch.int32, device=dev)
        self.device = self._sum.device
        return self.device

    @property
    def sums(self) -> Tensor:
        """``[n_segments, f_cols]`` float32 view: the sum of each feature's active values over the utterance's frames."""
        self._ensure_device()
        return self._sum[:, :self.f_cols]

    @property
    def counts(self) -> Tensor:
        if not self.with_counts:
            raise ValueError("this pooler keeps no firing counts: build it with counts=True")
        self._ensure_device()
        return self._cnt[:, :self.f_cols]

    @property
    def frames(self) -> Tensor:
        """``[n_segments]`` int32: the frames that contributed to each utterance."""
        self._ensure_device()
        return self._rows

    def means(self) -> Tensor:
        """``[n_segments, f_cols]`` float64: sum / frames (NaN for an utterance without frames)."""
        return self.sums.double() / self.frames.double()[:, None]

    def rates(self) -> Tensor:
        """``[n_segments, f_cols]`` float64: the fraction of the utterance's frames on which the feature fired."""
        return self.counts.double() / self.frames.double()[:, None]

    # ---- accumulation ---------------------------------------------------------------------------
    def update(self, code, segments: Optional[Tensor] = None, frame_mask: Optional[Tensor] = None) -> None:
        """One batch.  ``code = (values, indices)``: either ``[n_utt, T, k]``, whose utterances are numbered from a running
        base (``segments`` must be None), or flat ``[rows, k]`` with ``segments [rows]`` (ids outside
        ``0 .. n_segments - 1`` mark padding; the frames of an utterance should arrive together).  Frames with
        ``frame_mask == 0`` contribute nothing."""
        vals, idx, k = _stream.compact_code(code, "code", N.POOL_MAX_K)
        dev = self._ensure_device(vals)
        if vals.device != dev:
            raise N.WsaeError(f"the code is on {vals.device}, the pooler on {dev}")
        seg, n_utt = _stream.frame_segments(vals, segments, frame_mask, dev, first=self._next)
        used, rows = n_utt or 0, seg.shape[0]
        if self._next + used > self.n_segments:
            raise ValueError(f"{self._next} + {used} utterances exceed n_segments = {self.n_segments}")
        _stream.check_row_bound(self, rows)  # (seg_rows and the counts are int32)
        if rows == 0:
            self._next += used
            return
        v, i = _stream.flat_code(vals, idx, k)
        with torch.cuda.device(dev):
            N.check(N.lib().wsae_pool_update(
                v.data_ptr(), i.data_ptr(), k, self.hidden, seg.data_ptr(), rows, self.n_segments, self.f_lo, self.f_cols,
                self._sum.data_ptr(), N.ptr(self._cnt), self._ld, self._rows.data_ptr(), self._ws.data_ptr(),
                self._ws.numel() * 4, torch.cuda.current_stream(dev).cuda_stream), "wsae_pool_update")
        self._next += used  # (only now: a failed call has pooled nothing and leaves the numbering where it was)
        self._submitted += rows

    # ---- persistence ----------------------------------------------------------------------------
    def save(self, path) -> None:
        self._ensure_device()
        torch.save({"hidden": self.hidden, "n_segments": self.n_segments, "f_window": [self.f_lo, self.f_cols],
                    "next": self._next, "submitted": self._submitted, "sums": self.sums.cpu(),
                    "counts": self.counts.cpu() if self.with_counts else None, "frames": self._rows.cpu()}, Path(path))

    @classmethod
    def load(cls, path, device=None) -> "SegmentPooler":
        data = torch.load(Path(path), map_location="cpu", weights_only=True)
        p = cls(data["hidden"], data["n_segments"], f_window=tuple(data["f_window"]), counts=data["counts"] is not None,
                device=device)
        dev = p._ensure_device()
        p._sum[:, :p.f_cols] = data["sums"].to(dev)
        if p.with_counts:
            p._cnt[:, :p.f_cols] = data["counts"].to(dev)
        p._rows.copy_(data["frames"])
        p._next, p._submitted = int(data["next"]), int(data["submitted"])
        return p


def bootstrap_weights(labels, n_boot: int, *, group_a=0, group_b=1, seed: int = 0, balanced: bool = False,
                      device=None) -> Tensor:
    """Stratified resampling weights, int16 ``[n_boot, S]``: replicate r draws ``n_g`` members of each of the two groups
    with replacement (``balanced=True``: ``min(n_a, n_b)`` from each, the balanced sampling of the reference's design
    notes); ``w[r, s]`` is how often utterance s was drawn, 0 outside the two groups.  Drawn with a CPU generator (the same
    on every machine), then moved to ``device``."""
    lab = torch.as_tensor(labels).detach().reshape(-1).cpu()
    n_boot = int(n_boot)
    if n_boot < 1:
        raise ValueError(f"n_boot must be positive, got {n_boot}")
    S = lab.shape[0]
    members = [torch.nonzero(lab == g).flatten() for g in (group_a, group_b)]
    if any(m.numel() == 0 for m in members):
        raise ValueError(f"labels hold no member of group {group_a!r} or of group {group_b!r}")
    draws = [min(m.numel() for m in members)] * 2 if balanced else [m.numel() for m in members]
    if max(draws) > 32767:
        raise ValueError(f"a group of {max(draws)} members cannot be drawn into int16 weights")
    gen = torch.Generator().manual_seed(int(seed))
    w = torch.zeros(n_boot, S, dtype=torch.int32)
    for m, n in zip(members, draws):
        pick = m[torch.randint(m.numel(), (n_boot, n), generator=gen)]
        w.scatter_add_(1, pick, torch.ones_like(pick, dtype=torch.int32))
    w = w.to(torch.int16)
    return w if device is None else w.to(device)


def _effect_call(X: Tensor, ld: int, f_cols: int, div: Optional[Tensor], group: Tensor, boot: Optional[Tensor],
                 alpha: float) -> GroupEffects:
    dev, S = X.device, group.shape[0]
    R = 0 if boot is None else boot.shape[0]
    lib = N.lib()
    need = lib.wsae_group_effect_workspace_bytes(S, f_cols, R)
    if need < 0:
        raise ValueError(f"group effect sizes: {S} utterances, {f_cols} features, {R} replicates are out of range "
                         f"(replicates: 0 or 2..{N.BOOT_MAX_R})")
    with torch.cuda.device(dev):
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        out = torch.empty(7, f_cols, dtype=torch.float64, device=dev)
        rec = torch.zeros(3, dtype=torch.int32, device=dev)
        o = [out[i].data_ptr() for i in range(7)]
        N.check(lib.wsae_group_effect(X.data_ptr(), ld, N.ptr(div), group.data_ptr(), S, f_cols, N.ptr(boot), R, float(alpha),
                                      o[0], o[1], o[2], o[3], o[4], o[5], o[6], rec.data_ptr(), ws.data_ptr(), ws.numel(),
                                      torch.cuda.current_stream(dev).cuda_stream), "wsae_group_effect")
        n_a, n_b, kept = (int(v) for v in rec.cpu())
    return GroupEffects(d=out[2], g=out[3], mean_a=out[0], mean_b=out[1], ci_lo=out[4], ci_hi=out[5], se=out[6], n_a=n_a,
                        n_b=n_b, n_boot=kept)


def group_effect_sizes(pooled_or_matrix, labels, *, group_a=0, group_b=1, n_boot: int = 1000, alpha: float = 0.05,
                       seed: int = 0, balanced: bool = False, use: str = "mean") -> GroupEffects:
    """Effect sizes of group_a against group_b per feature.  ``pooled_or_matrix``: a ``SegmentPooler`` (``use="mean"``:
    the per-utterance mean activation, sum / frames; ``"sum"``: the sums; ``"rate"``: the firing rate, which needs
    ``counts=True``; an utterance without frames is left out) or a plain ``[S, H]`` float32 device tensor - the route for
    ReLU SAEs and any other per-utterance matrix.  ``labels [S]`` may hold more than two classes; the two named ones are
    compared.  ``n_boot=0``: point statistics only."""
    if use not in ("mean", "sum", "rate"):
        raise ValueError(f"use must be 'mean', 'sum' or 'rate', got {use!r}")
    if not 0.0 < float(alpha) < 1.0:
        raise ValueError(f"alpha must lie in (0, 1), got {alpha}")
    n_boot = int(n_boot)
    if n_boot != 0 and not 2 <= n_boot <= N.BOOT_MAX_R:
        raise ValueError(f"n_boot must be 0 or in 2..{N.BOOT_MAX_R}, got {n_boot}")
    div = None
    if isinstance(pooled_or_matrix, SegmentPooler):
        p = pooled_or_matrix
        dev = p._ensure_device()
        ld, f_cols, S = p._ld, p.f_cols, p.n_segments
        if use == "rate":
            X = torch.zeros_like(p._sum)
            X[:, :f_cols] = p.counts.float()  # (exact below 2^24 frames per utterance)
        else:
            X = p._sum
        if use != "sum":
            div = p._rows
    elif isinstance(pooled_or_matrix, Tensor):
        X = pooled_or_matrix
        require_device_tensor(X, "the per-utterance matrix")
        if X.dim() != 2 or X.dtype != torch.float32:
            raise ValueError(f"the per-utterance matrix must be [S, H] float32, got {tuple(X.shape)} {X.dtype}")
        X = X.detach().contiguous()
        dev = _stream.need_gpu("group_effect_sizes", X.device)
        S, f_cols = X.shape
        ld = f_cols
    else:
        raise TypeError("group_effect_sizes takes a SegmentPooler or a [S, H] float32 device tensor")
    lab = torch.as_tensor(labels).detach().reshape(-1).cpu()
    if lab.shape[0] != S:
        raise ValueError(f"labels has {lab.shape[0]} entries for {S} utterances")
    group = torch.full((S,), -1, dtype=torch.int32)
    group[lab == group_a] = 0
    group[lab == group_b] = 1
    boot = None
    if n_boot:
        boot = bootstrap_weights(lab, n_boot, group_a=group_a, group_b=group_b, seed=seed, balanced=balanced,
                                 device=dev).contiguous()
    return _effect_call(X, ld, f_cols, div, group.to(dev), boot, alpha)


def top_group_features(effects: GroupEffects, n: int = 20, require_ci_excludes_zero: bool = True):
    """The ``n`` features with the largest ``|g|`` as ``(indices, g)``; with ``require_ci_excludes_zero`` only features
    whose interval lies on one side of zero are candidates (fewer than ``n`` may remain)."""
    score = effects.g.abs()
    ok = torch.isfinite(score)
    if require_ci_excludes_zero:
        ok &= (effects.ci_lo > 0) | (effects.ci_hi < 0)
    order = _stream.rank_features(score, ok, n)
    return order, effects.g[order]


def collect_pooled(model, utterances, *, n_segments: Optional[int] = None, f_window: Optional[Tuple[int, int]] = None,
                   counts: bool = False, device="cuda") -> SegmentPooler:
    """Pool a dataset of utterances.  Every item of ``utterances`` is a tensor ``[n_utt, T, D]`` or a pair
    ``(x, frame_mask [n_utt, T])``; utterances are numbered in the order they arrive.  ``n_segments`` defaults to the total
    of a list.  The module must offer ``encode_compact`` (TopK and BatchTopK SAEs; for a ReLU SAE pool the dense code in
    torch and pass the matrix to ``group_effect_sizes``: ``TypeError``) and is run in eval mode; its previous mode is
    restored."""
    with _stream.encoding(model, hint="pool its dense code in torch and pass the [S, H] matrix to group_effect_sizes"):
        if n_segments is None:
            utterances = list(utterances)
            n_segments = sum((b[0] if isinstance(b, (tuple, list)) else b).shape[0] for b in utterances)
        pooler = SegmentPooler(model.hidden_dim, n_segments, f_window=f_window, counts=counts, device=device)
        for x, mask in _stream.batches(utterances):
            pooler.update(_stream.utterance_code(model, x, device), frame_mask=None if mask is None else mask.to(device))
    return pooler
