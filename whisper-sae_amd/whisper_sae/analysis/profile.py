"""Activation profiles: what does the distribution of a feature's activations look like - its
firing density, its mean when active, its median and tails - and what does the feature do when it is not at its maximum?

``ActivationProfile`` keeps, per feature, a histogram of its active values over 192 bins read off the float's bits (eight
per octave over ``[2^-12, 2^12)``), the count, the minimum and maximum and a fixed-point sum, straight from the compact
``(values, indices)`` code (``wsae_profile_update`` - the dense ``[frames, H]`` matrix never exists).  ``ActivationSampler``
keeps, per feature and value stratum, a uniform sample without replacement of the activations that fell into the stratum
(``wsae_sample_update``): a bottom-m sketch under a hash of (frame ordinal, feature, seed), so top-activating examples
can be read next to examples from every quantile band.  Both states are integer: they do not depend on the order of the
batches, on the batching or on the launch geometry, and the states of two shards merge exactly.  The readers over
``[f_cols]`` vectors are plain torch in float64.

Out of scope: dense / ReLU codes, weighted samples, plots, fetching the audio behind an ordinal.
"""

from __future__ import annotations

import math
from pathlib import Path
from typing import List, NamedTuple, Optional, Tuple, Union

import torch
from torch import Tensor

from .. import _native as N
from ..sae.engine import require_device_tensor
from . import _stream

MAX_ORDINALS = 2 ** 31           # a key keeps its ordinal in 31 bits
PROFILE_BINS = N.PROFILE_BINS
MIN_INIT = 0x7F800000            # min_bits before anything fired: the bits of +inf
EMPTY_KEY = -1                   # 2^64 - 1 in the int64 tensors that hold the uint64 keys
_SIGN = -2 ** 63                 # key ^ _SIGN orders as int64 the way key orders as uint64


class ProfileSummary(NamedTuple):
    """Per feature of the window.  ``fires``, ``over`` (values >= 4096): int64 counts.  Float64: ``density`` = fires /
    total rows; ``mean`` = sum_q 2^-20 / fires (values above 4096 enter as 4096); ``max`` and ``min``, exact; ``median``,
    ``q10``, ``q90``, ``q99`` read off the histogram (``ActivationProfile.quantile``: accurate to one bin, at most 12.5 %
    relative).  Where a feature never fired every value field is NaN (``density`` is 0)."""

    fires: Tensor
    density: Tensor
    mean: Tensor
    max: Tensor
    min: Tensor
    median: Tensor
    q10: Tensor
    q90: Tensor
    q99: Tensor
    over: Tensor


class DensityHistogram(NamedTuple):
    """``counts`` int64 ``[bins]``: features per bin of log10(density); ``edges`` float64 ``[bins + 1]``; ``dead``: the
    features that never fired (they have no logarithm and are in no bin)."""

    counts: Tensor
    edges: Tensor
    dead: int


class SampledActivations(NamedTuple):
    """The sampled activations of one feature, sorted by stratum and then key: ``stratum`` int64, ``value`` float32,
    ``ordinal`` int64 (the frame's number in the stream), ``utterance`` / ``frame`` int64 (-1 where the frame came with a
    flat code); ``seen`` int64 ``[n_strata]``: every activation of the stratum, sampled or not."""

    stratum: Tensor
    value: Tensor
    ordinal: Tensor
    utterance: Tensor
    frame: Tensor
    seen: Tensor


def bin_lower_edge(bins: Tensor) -> Tensor:
    """The lower edge of bin ``j`` as float64, ``2^(j // 8 - 12) (1 + (j % 8) / 8)``, read back from the bit pattern
    ``(j + 920) << 20``; ``j = 192`` gives 4096."""
    return ((bins.to(torch.int64) + 920) << 20).to(torch.int32).view(torch.float32).double()


def _bits_value(bits: Tensor, fires: Tensor) -> Tensor:
    v = bits.contiguous().view(torch.float32).double()
    return torch.where(fires > 0, v, torch.full_like(v, float("nan")))


def histogram_quantile(hist: Tensor, fires: Tensor, min_bits: Tensor, max_bits: Tensor, q: float) -> Tensor:
    """``ActivationProfile.quantile`` on raw integer state (any device)."""
    q = float(q)
    if not 0.0 <= q <= 1.0:
        raise ValueError(f"q must lie in [0, 1], got {q}")
    h = hist.to(torch.int64)
    cum = h.cumsum(1)
    t = q * fires.double()
    reached = (cum.double() >= t[:, None]) & (h > 0)
    j = reached.to(torch.int8).argmax(1)
    inf = torch.full_like(t, float("inf"))
    lo = torch.where(j == 0, torch.zeros_like(t), bin_lower_edge(j))
    hi = torch.where(j == PROFILE_BINS - 1, inf, bin_lower_edge(j + 1))
    lo = torch.maximum(lo, _bits_value(min_bits, fires))
    hi = torch.minimum(hi, _bits_value(max_bits, fires))
    h_j, cum_j = h.gather(1, j[:, None])[:, 0], cum.gather(1, j[:, None])[:, 0]
    frac = (t - (cum_j - h_j).double()) / h_j.double()
    out = torch.where(frac == 0, lo, lo + frac * (hi - lo))
    return torch.where(fires > 0, out, torch.full_like(out, float("nan")))


def _mask_segments(frame_mask: Optional[Tensor], rows: int, dev) -> Optional[Tensor]:
    """int32 ``[rows]``: 0 for a frame, -1 where ``frame_mask == 0``; None without a mask."""
    if frame_mask is None:
        return None
    require_device_tensor(frame_mask, "frame_mask")
    if frame_mask.numel() != rows:
        raise ValueError(f"frame_mask has {frame_mask.numel()} flags for {rows} frames")
    return ((frame_mask.detach().reshape(-1).to(dev) != 0).to(torch.int32) - 1).contiguous()


class ActivationProfile:
    """Value histograms and moments of a compact code over a stream of frames.

    ``f_window=(f_lo, f_cols)``: keep only the features ``f_lo .. f_lo + f_cols - 1``.  The state lives on the device of
    the first update (or ``device``)."""

    def __init__(self, hidden: int, *, f_window: Optional[Tuple[int, int]] = None, device=None):
        self.hidden = int(hidden)
        if self.hidden < 1:
            raise ValueError(f"hidden must be positive, got {hidden}")
        self.f_lo, self.f_cols = _stream.feature_window(f_window, self.hidden)
        self.device = torch.device(device) if device is not None else None
        self._state: Optional[dict] = None
        self._submitted = 0  # rows handed to update so far, padding included (host-side bound of the int32 state)

    # ---- state ----------------------------------------------------------------------------------
    def _ensure_device(self, like: Optional[Tensor] = None) -> torch.device:
        if self._state is not None:
            return self._state["fires"].device
        dev = _stream.need_gpu("ActivationProfile", self.device or (like.device if like is not None else None))
        z = lambda *shape, dtype=torch.int32: torch.zeros(*shape, dtype=dtype, device=dev)  # noqa: E731
        self._state = {"fires": z(self.f_cols), "hist": z(self.f_cols, PROFILE_BINS), "max_bits": z(self.f_cols),
                       "min_bits": torch.full((self.f_cols,), MIN_INIT, dtype=torch.int32, device=dev),
                       "over": z(self.f_cols), "sum_q": z(self.f_cols, dtype=torch.int64),
                       "total_rows": z(1, dtype=torch.int64)}
        self.device = self._state["fires"].device
        return self.device

    fires = _stream.state_property("fires", "``[f_cols]`` int32: the rows on which the feature was active.")
    hist = _stream.state_property("hist", "``[f_cols, 192]`` int32: the value histogram.")
    max_bits = _stream.state_property("max_bits", "``[f_cols]`` int32: the bits of the largest value.")
    min_bits = _stream.state_property("min_bits", "``[f_cols]`` int32: the bits of the smallest value.")
    over = _stream.state_property("over", "``[f_cols]`` int32: the values >= 4096.")
    sum_q = _stream.state_property("sum_q", "``[f_cols]`` int64: the sum of rint(min(v, 4096) 2^20).")
    total_rows = _stream.state_property("total_rows", "``[1]`` int64: the non-padding frames seen.")

    # ---- accumulation ---------------------------------------------------------------------------
    def update(self, code, frame_mask: Optional[Tensor] = None) -> None:
        """One batch.  ``code = (values, indices)``, ``[n_utt, T, k]`` or flat ``[rows, k]``.  Frames with
        ``frame_mask == 0`` are padding and count for nothing."""
        vals, idx, k = _stream.compact_code(code, "code", N.PROFILE_MAX_K)
        dev = self._ensure_device(vals)
        if vals.device != dev:
            raise N.WsaeError(f"the code is on {vals.device}, the profile on {dev}")
        v, i = _stream.flat_code(vals, idx, k)
        rows = v.shape[0]
        seg = _mask_segments(frame_mask, rows, dev)
        # (fires and the histogram cells are int32, and sum_q holds 2^31 - 1 terms of at most 2^32)
        _stream.check_row_bound(self, rows)
        if rows == 0:
            return
        st = self._state
        with torch.cuda.device(dev):
            N.check(N.lib().wsae_profile_update(
                v.data_ptr(), i.data_ptr(), k, self.hidden, N.ptr(seg), rows, self.f_lo, self.f_cols, st["fires"].data_ptr(),
                st["hist"].data_ptr(), st["max_bits"].data_ptr(), st["min_bits"].data_ptr(), st["over"].data_ptr(),
                st["sum_q"].data_ptr(), st["total_rows"].data_ptr(), None, 0, torch.cuda.current_stream(dev).cuda_stream),
                "wsae_profile_update")
        self._submitted += rows

    def merge(self, other: "ActivationProfile") -> None:
        """Add the state of a profile of the same size and window (another shard of the dataset): integer adds, a
        minimum and a maximum."""
        if (self.hidden, self.f_lo, self.f_cols) != (other.hidden, other.f_lo, other.f_cols):
            raise ValueError("merge needs two profiles of the same size and window")
        _stream.check_row_bound(self, other._submitted, merging=True)
        if other._state is None:
            return
        dev = self._ensure_device(other._state["fires"])
        a, b = self._state, other._state
        for name in ("fires", "hist", "over", "sum_q", "total_rows"):
            a[name] += b[name].to(dev)
        torch.maximum(a["max_bits"], b["max_bits"].to(dev), out=a["max_bits"])
        torch.minimum(a["min_bits"], b["min_bits"].to(dev), out=a["min_bits"])
        self._submitted += other._submitted

    # ---- reading --------------------------------------------------------------------------------
    def quantile(self, q: float) -> Tensor:
        """``[f_cols]`` float64: the ``q`` quantile (0 <= q <= 1) of every feature's active values, read off the
        histogram.  With N = fires and t = q N: bin j is the first bin with hist[j] > 0 whose cumulative count reaches t;
        lo / hi are its edges (0 below bin 0, +inf above bin 191) clipped to [min, max], which moves the lower edge of the
        first occupied bin and the upper edge of the last; the result is lo + (t - cum[j - 1]) / hist[j] * (hi - lo), and
        lo where that fraction is 0.  The true quantile lies in the same bin, so the result is accurate to one bin: at
        most 12.5 % relative inside [2^-12, 2^12).  NaN where the feature never fired."""
        self._ensure_device()
        st = self._state
        return histogram_quantile(st["hist"], st["fires"], st["min_bits"], st["max_bits"], q)

    def summary(self) -> ProfileSummary:
        """The per-feature summary, float64 from the integers."""
        self._ensure_device()
        st = self._state
        fires = st["fires"]
        n = fires.double()
        nan = torch.full_like(n, float("nan"))
        mean = torch.where(fires > 0, st["sum_q"].double() * 2.0 ** -20 / n, nan)
        return ProfileSummary(fires=fires.to(torch.int64), density=n / st["total_rows"].double()[0], mean=mean,
                              max=_bits_value(st["max_bits"], fires), min=_bits_value(st["min_bits"], fires),
                              median=self.quantile(0.5), q10=self.quantile(0.1), q90=self.quantile(0.9),
                              q99=self.quantile(0.99), over=st["over"].to(torch.int64))

    def quantile_edges(self, n_strata: int) -> Tensor:
        """``[f_cols, n_strata - 1]`` float32: the quantiles j / n_strata, the edges of ``n_strata`` bands of equal
        probability for ``ActivationSampler`` (NaN where a feature never fired: all it does later is stratum 0)."""
        n = _check_strata(n_strata)
        cols = [self.quantile(j / n) for j in range(1, n)]
        if not cols:
            return torch.zeros(self.f_cols, 0, dtype=torch.float32, device=self._ensure_device())
        return torch.stack(cols, dim=1).to(torch.float32)

    def fraction_of_max_edges(self, n_strata: int) -> Tensor:
        """``[f_cols, n_strata - 1]`` float32: edges at j / n_strata of every feature's maximum (NaN where it never fired)."""
        n = _check_strata(n_strata)
        self._ensure_device()
        top = _bits_value(self._state["max_bits"], self._state["fires"])
        frac = torch.arange(1, n, dtype=torch.float64, device=top.device) / n
        return (top[:, None] * frac[None, :]).to(torch.float32)

    def density_histogram(self, bins: int = 40, lowest: Optional[float] = None) -> DensityHistogram:
        """The histogram over features of log10(density), the standard health check of a dictionary (dead features,
        ultra-dense ones, the two humps): ``bins`` equal bins over ``[lowest, 0]``; ``lowest`` defaults to
        floor(log10(1 / total rows)), below which no feature that fired can lie.  Features that never fired are counted
        in ``dead``."""
        bins = int(bins)
        if bins < 1:
            raise ValueError(f"bins must be positive, got {bins}")
        self._ensure_device()
        fires, rows = self._state["fires"], self._state["total_rows"].double()[0]
        alive = fires > 0
        if lowest is None:
            lowest = -math.ceil(math.log10(max(float(rows.item()), 10.0)))
        lowest = float(lowest)
        if not lowest < 0.0:
            raise ValueError(f"lowest must be negative, got {lowest}")
        logd = torch.log10(fires[alive].double() / rows)
        cell = ((logd - lowest) / (0.0 - lowest) * bins).floor().clamp(0, bins - 1).to(torch.int64)
        counts = torch.bincount(cell, minlength=bins)
        edges = torch.linspace(lowest, 0.0, bins + 1, dtype=torch.float64, device=fires.device)
        return DensityHistogram(counts=counts, edges=edges, dead=int((~alive).sum().item()))

    # ---- persistence ----------------------------------------------------------------------------
    def save(self, path) -> None:
        torch.save({"hidden": self.hidden, "f_window": [self.f_lo, self.f_cols], "submitted": self._submitted,
                    "state": _stream.state_to_cpu(self)}, Path(path))

    @classmethod
    def load(cls, path, device=None) -> "ActivationProfile":
        data = torch.load(Path(path), map_location="cpu", weights_only=True)
        p = cls(data["hidden"], f_window=tuple(data["f_window"]), device=device)
        _stream.state_from_saved(p, data["state"])
        p._submitted = int(data["submitted"])
        return p


def _check_strata(n_strata) -> int:
    n = int(n_strata)
    if not 1 <= n <= N.SAMPLE_MAX_STRATA:
        raise ValueError(f"n_strata must be in 1..{N.SAMPLE_MAX_STRATA}, got {n_strata}")
    return n


def top_profile_features(summary: ProfileSummary, by: str = "density", n: int = 20, min_fires: int = 1, largest: bool = True):
    """The ``n`` features with the largest (``largest=False``: smallest) value of the summary field ``by`` as
    ``(indices, values)``; only features with at least ``min_fires`` activations and a value that is not NaN are
    candidates (fewer than ``n`` may remain).  Ties go to the lower index."""
    if by not in ProfileSummary._fields:
        raise ValueError(f"by must be one of {ProfileSummary._fields}, got {by!r}")
    value = getattr(summary, by).double()
    ok = (summary.fires >= int(min_fires)) & ~torch.isnan(value)
    order = _stream.rank_features(value if largest else -value, ok, n)
    return order, getattr(summary, by)[order]


class ActivationSampler:
    """Uniform samples of a feature's activations per value stratum, over a stream of frames.

    ``edges [f_cols, n_strata - 1]`` float32, ascending per feature (None: one stratum): an activation ``v`` of feature f
    falls into the stratum numbered by the count of f's edges that are ``<= v``.  Per (feature, stratum) the ``keep``
    activations with the smallest key are held, the key being a hash of (frame ordinal, feature, ``seed``) above the
    ordinal: which frames are sampled depends on the data and the seed alone.  Frames are numbered from
    ``ordinal_base`` in the order they arrive, padding included; give the samplers of different shards disjoint ranges
    and ``merge`` is exact."""

    def __init__(self, hidden: int, edges: Optional[Tensor] = None, *, keep: int = 8, seed: int = 0,
                 f_window: Optional[Tuple[int, int]] = None, ordinal_base: int = 0, device=None):
        self.hidden = int(hidden)
        if self.hidden < 1:
            raise ValueError(f"hidden must be positive, got {hidden}")
        self.f_lo, self.f_cols = _stream.feature_window(f_window, self.hidden)
        self.keep, self.seed, self.ordinal_base = int(keep), int(seed), int(ordinal_base)
        if not 1 <= self.keep <= N.SAMPLE_MAX_KEEP:
            raise ValueError(f"keep must be in 1..{N.SAMPLE_MAX_KEEP}, got {keep}")
        if not 0 <= self.seed < 2 ** 32:
            raise ValueError(f"seed must be in 0..2^32 - 1, got {seed}")
        if not 0 <= self.ordinal_base < MAX_ORDINALS:
            raise ValueError(f"ordinal_base must be in 0..2^31 - 1, got {ordinal_base}")
        if edges is not None:
            if not isinstance(edges, Tensor) or edges.dim() != 2 or edges.shape[0] != self.f_cols:
                raise ValueError(f"edges must be a [{self.f_cols}, n_strata - 1] tensor, got "
                                 f"{tuple(edges.shape) if isinstance(edges, Tensor) else type(edges).__name__}")
            _check_strata(edges.shape[1] + 1)
            edges = edges.detach().to(torch.float32).contiguous()
            if edges.shape[1] == 0:
                edges = None
        self.n_strata = 1 if edges is None else edges.shape[1] + 1
        self.edges = edges
        self.device = torch.device(device) if device is not None else None
        self._state: Optional[dict] = None
        self._ws: Optional[Tensor] = None
        self._next = self.ordinal_base            # the ordinal of the next frame
        self._records: List[Tuple[int, int, int]] = []  # (first ordinal, n_utt, T) of every [n_utt, T, k] update

    # ---- state ----------------------------------------------------------------------------------
    def _ensure_device(self, like: Optional[Tensor] = None) -> torch.device:
        if self._state is not None:
            return self._state["keys"].device
        dev = _stream.need_gpu("ActivationSampler", self.device or (like.device if like is not None else None))
        shape = (self.f_cols, self.n_strata, self.keep)
        self._state = {"keys": torch.full(shape, EMPTY_KEY, dtype=torch.int64, device=dev),
                       "svals": torch.zeros(shape, dtype=torch.float32, device=dev),
                       "seen": torch.zeros(shape[:2], dtype=torch.int32, device=dev)}
        if self.edges is not None:
            self.edges = self.edges.to(dev)
        self.device = self._state["keys"].device
        return self.device

    keys = _stream.state_property("keys",
                                  "``[f_cols, n_strata, keep]`` int64 holding the uint64 keys, ascending; -1 (2^64 - 1) = unused.")
    values = _stream.state_property("svals", "``[f_cols, n_strata, keep]`` float32: the values beside the keys.")
    seen = _stream.state_property("seen", "``[f_cols, n_strata]`` int32: the activations of each stratum.")

    # ---- accumulation ---------------------------------------------------------------------------
    def update(self, code, frame_mask: Optional[Tensor] = None) -> None:
        """One batch.  ``code = (values, indices)``, ``[n_utt, T, k]`` or flat ``[rows, k]``; its frames take the next
        ordinals, those with ``frame_mask == 0`` (padding, never sampled) too."""
        vals, idx, k = _stream.compact_code(code, "code", N.PROFILE_MAX_K)
        dev = self._ensure_device(vals)
        if vals.device != dev:
            raise N.WsaeError(f"the code is on {vals.device}, the sampler on {dev}")
        v, i = _stream.flat_code(vals, idx, k)
        rows = v.shape[0]
        seg = _mask_segments(frame_mask, rows, dev)
        if self._next + rows > MAX_ORDINALS:
            raise N.WsaeError(f"ActivationSampler: the ordinals {self._next} + {rows} leave [0, 2^31)")
        st = self._state
        if rows:
            lib = N.lib()
            need = lib.wsae_sample_workspace_bytes(rows, k, self.hidden, self.f_lo, self.f_cols, self.n_strata, self.keep)
            if need < 0:
                raise N.WsaeError(f"ActivationSampler: {rows} frames of k = {k} are more than one call takes (2^31 - 1 "
                                  f"entries): feed smaller batches")
            with torch.cuda.device(dev):
                ws = _stream.grow(self, (need + 7) // 8, torch.int64, dev)
                N.check(lib.wsae_sample_update(
                    v.data_ptr(), i.data_ptr(), k, self.hidden, N.ptr(seg), rows, self._next, self.f_lo, self.f_cols,
                    N.ptr(self.edges), self.n_strata, self.keep, self.seed, st["keys"].data_ptr(), st["svals"].data_ptr(),
                    st["seen"].data_ptr(), ws.data_ptr(), ws.numel() * 8, torch.cuda.current_stream(dev).cuda_stream),
                    "wsae_sample_update")
        if vals.dim() == 3 and rows:
            self._records.append((self._next, vals.shape[0], vals.shape[1]))
        self._next += rows

    def _same_kind(self, other: "ActivationSampler") -> bool:
        if (self.hidden, self.f_lo, self.f_cols, self.keep, self.seed, self.n_strata) != \
                (other.hidden, other.f_lo, other.f_cols, other.keep, other.seed, other.n_strata):
            return False
        if self.edges is None:
            return True
        # bit for bit, so that the NaN edges of a silent feature compare equal
        return torch.equal(self.edges.cpu().view(torch.int32), other.edges.cpu().view(torch.int32))

    def merge(self, other: "ActivationSampler") -> None:
        """Take in the state of a sampler of the same kind (``edges``, ``seed``, ``keep``, window) over other frames: per
        list the union of the two samples cut to the ``keep`` smallest keys, which is the sample one sampler fed both
        streams would hold.  The two ranges of ordinals must not overlap (``ordinal_base``): ``ValueError`` otherwise."""
        if not self._same_kind(other):
            raise ValueError("merge needs two samplers with the same edges, seed, keep and window")
        a, b = (self.ordinal_base, self._next), (other.ordinal_base, other._next)
        if a[0] < b[1] and b[0] < a[1]:
            raise ValueError(f"merge: the ordinals [{a[0]}, {a[1]}) and [{b[0]}, {b[1]}) overlap; give the shards disjoint "
                             f"ranges with ordinal_base")
        if other._state is not None:
            dev = self._ensure_device(other._state["keys"])
            st, ot = self._state, other._state
            keys = torch.cat([st["keys"], ot["keys"].to(dev)], dim=2)
            vals = torch.cat([st["svals"], ot["svals"].to(dev)], dim=2)
            order = torch.argsort(keys ^ _SIGN, dim=2, stable=True)[:, :, :self.keep]  # (unsigned order)
            st["keys"], st["svals"] = keys.gather(2, order).contiguous(), vals.gather(2, order).contiguous()
            st["seen"] += ot["seen"].to(dev)
        self._records = sorted(self._records + other._records)
        if a[0] == a[1]:
            self.ordinal_base, self._next = b
        elif b[0] != b[1]:  # the merged sampler covers both ranges and goes on behind them
            self.ordinal_base, self._next = min(a[0], b[0]), max(a[1], b[1])

    # ---- reading --------------------------------------------------------------------------------
    def _locate(self, ordinal: Tensor) -> Tuple[Tensor, Tensor]:
        """(utterance, frame) of ordinals from the update records; -1 where an ordinal came with a flat code."""
        utt = torch.full_like(ordinal, -1)
        frame = torch.full_like(ordinal, -1)
        first = 0  # utterances are numbered in the order of their ordinals
        for base, n_utt, T in sorted(self._records):
            off = ordinal - base
            here = (off >= 0) & (off < n_utt * T)
            utt = torch.where(here, first + off // T, utt)
            frame = torch.where(here, off % T, frame)
            first += n_utt
        return utt, frame

    def examples(self, feature: int) -> SampledActivations:
        """The sampled activations of ``feature`` (its index in ``[0, hidden)``; it must lie in the window)."""
        c = int(feature) - self.f_lo
        if not 0 <= c < self.f_cols:
            raise ValueError(f"feature {feature} is outside the window [{self.f_lo}, {self.f_lo + self.f_cols})")
        self._ensure_device()
        keys, vals = self._state["keys"][c].cpu(), self._state["svals"][c].cpu()
        held = keys != EMPTY_KEY
        stratum = torch.arange(self.n_strata)[:, None].expand_as(keys)[held]
        ordinal = keys[held] & 0xFFFFFFFF
        utt, frame = self._locate(ordinal)
        return SampledActivations(stratum=stratum, value=vals[held], ordinal=ordinal, utterance=utt, frame=frame,
                                  seen=self._state["seen"][c].cpu().to(torch.int64))

    # ---- persistence ----------------------------------------------------------------------------
    def save(self, path) -> None:
        torch.save({"hidden": self.hidden, "f_window": [self.f_lo, self.f_cols], "keep": self.keep, "seed": self.seed,
                    "ordinal_base": self.ordinal_base, "next": self._next, "records": [list(r) for r in self._records],
                    "edges": None if self.edges is None else self.edges.cpu(), "state": _stream.state_to_cpu(self)}, Path(path))

    @classmethod
    def load(cls, path, device=None) -> "ActivationSampler":
        data = torch.load(Path(path), map_location="cpu", weights_only=True)
        s = cls(data["hidden"], data["edges"], keep=data["keep"], seed=data["seed"], f_window=tuple(data["f_window"]),
                ordinal_base=data["ordinal_base"], device=device)
        _stream.state_from_saved(s, data["state"])
        s._next, s._records = int(data["next"]), [tuple(r) for r in data["records"]]
        return s


def collect_activation_profile(model, utterances, *, device="cuda", **profile_kw) -> ActivationProfile:
    """The activation profile over a dataset of utterances.  Every item of ``utterances`` is a tensor ``[n_utt, T, D]``
    or a pair ``(x, frame_mask [n_utt, T])``.  ``profile_kw`` goes to ``ActivationProfile``.  The module must offer
    ``encode_compact`` (TopK and BatchTopK SAEs; a ReLU SAE's code is dense: ``TypeError``) and is run in eval mode; its
    previous mode is restored."""
    with _stream.encoding(model, hint="activation profiles are for TopK-family codes"):
        profile = ActivationProfile(model.hidden_dim, device=device, **profile_kw)
        for x, mask in _stream.batches(utterances):
            profile.update(_stream.utterance_code(model, x, device), frame_mask=None if mask is None else mask.to(device))
    return profile


def collect_activation_samples(model, utterances, profile_or_edges: Union[ActivationProfile, Tensor, None], *,
                               n_strata: int = 10, keep: int = 8, seed: int = 0, f_window: Optional[Tuple[int, int]] = None,
                               ordinal_base: int = 0, device="cuda") -> ActivationSampler:
    """A second pass over the dataset of ``collect_activation_profile``: samples per quantile band.  ``profile_or_edges``
    is the profile of the first pass, whose ``quantile_edges(n_strata)`` and window are taken, or a tensor of edges
    ``[f_cols, n_strata - 1]`` (``fraction_of_max_edges`` for instance; None: one stratum), which goes with ``f_window``."""
    with _stream.encoding(model, hint="activation samples are for TopK-family codes"):
        if isinstance(profile_or_edges, ActivationProfile):
            if profile_or_edges.hidden != model.hidden_dim:
                raise ValueError(f"the profile has {profile_or_edges.hidden} features, the module {model.hidden_dim}")
            edges = profile_or_edges.quantile_edges(n_strata)
            f_window = (profile_or_edges.f_lo, profile_or_edges.f_cols)
        else:
            edges = profile_or_edges
        sampler = ActivationSampler(model.hidden_dim, edges, keep=keep, seed=seed, f_window=f_window,
                                    ordinal_base=ordinal_base, device=device)
        for x, mask in _stream.batches(utterances):
            sampler.update(_stream.utterance_code(model, x, device), frame_mask=None if mask is None else mask.to(device))
    return sampler
