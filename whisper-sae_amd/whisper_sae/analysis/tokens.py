"""Token association: which tokens - of the decoder's vocabulary, or word types of a forced
alignment - does a feature fire on, and which features announce a token?

``TokenAssociation`` is the sparse counterpart of ``LabelAssociation`` for label sets of 10^4 to 10^7 classes: exact
integer statistics ``(count, fixed-point activation sum)`` of every (feature, token) pair that actually occurs, kept in an
open-addressing hash table in device memory that ``wsae_pair_update`` fills straight from the compact ``(values, indices)``
code, in memory proportional to the number of distinct pairs - no ``[hidden, n_tokens]`` array exists at any point.  Both
directions are ranked on the device (``wsae_pair_top``): ``top_tokens`` of every feature, ``top_features`` of every token,
by count, precision, recall, F1, Jaccard, lift, PMI or mean activation.  The set of (pair, count, sum) triples and the
marginals do not depend on batching, call order or launch geometry, and two shards merge exactly; the slot a pair lands in
may vary from run to run, and nothing reads it: ``pairs()``, ``save`` and every comparison go through the sorted export.

Out of scope: several lags or value strata per tracker (use one tracker each), NPMI, a feature window, approximate
heavy-hitter sketches, several GPUs beyond ``merge``.
"""

from __future__ import annotations

from pathlib import Path
from typing import Dict, List, NamedTuple, Optional, Sequence

import torch
from torch import Tensor

from .. import _native as N
from . import _stream

SCORES = N.PAIR_SCORES + ("pmi",)  # pmi = log(lift), taken here on the selected entries
MIN_CAPACITY, MAX_CAPACITY = 1 << 10, 1 << 31
Q_SCALE = 2.0 ** -20  # sum_q is the sum of rint(min(v, 4096) 2^20)


class TopPairs(NamedTuple):
    """Per group (feature or token), ``[n_groups, n]``: ``ids`` int64, the tokens of a feature or the features of a token,
    best score first, ties to the lower id, -1 behind the end of a short list; ``scores`` float64 (-inf there); ``counts``
    int64, the frames on which the pair occurred; ``mean_activation`` float64, the feature's mean value on them (NaN behind
    the end)."""

    ids: Tensor
    scores: Tensor
    counts: Tensor
    mean_activation: Tensor


class PairExport(NamedTuple):
    """Every pair of the table on the CPU, keys ascending (by feature, then token): ``feature``, ``token``, ``count``,
    ``sum_q`` int64 ``[n_pairs]``."""

    feature: Tensor
    token: Tensor
    count: Tensor
    sum_q: Tensor


def _pow2_at_least(n: int) -> int:
    return 1 << max(int(n) - 1, 0).bit_length()


class TokenAssociation:
    """Feature-by-token counts of a compact code against an integer token per frame, over a stream of utterances.

    The token of a frame is read ``lag`` frames after the activation (-1024..1024; +1 on a decoder layer: the next token),
    never across an utterance; a token outside ``[0, n_tokens)`` (-1 for "no token") drops that frame as a token and nothing
    else.  ``capacity`` slots (a power of two, at least 1024) are allocated on the first update; the table grows by itself,
    so that it is never more than half full.  The state lives on the device of the first update (or ``device``)."""

    def __init__(self, hidden: int, n_tokens: int, lag: int = 0, capacity: int = 1 << 20, device=None):
        self.hidden, self.n_tokens, self.lag = int(hidden), int(n_tokens), int(lag)
        if self.hidden < 1:
            raise ValueError(f"hidden must be positive, got {hidden}")
        if not 1 <= self.n_tokens <= N.PAIR_MAX_TOKENS:
            raise ValueError(f"n_tokens must be in 1..{N.PAIR_MAX_TOKENS}, got {n_tokens}")
        _stream.check_lag(self.lag)
        capacity = int(capacity)
        if not MIN_CAPACITY <= capacity <= MAX_CAPACITY or capacity & (capacity - 1):
            raise ValueError(f"capacity must be a power of two in {MIN_CAPACITY}..{MAX_CAPACITY}, got {capacity}")
        self._initial_capacity = capacity
        self.device = torch.device(device) if device is not None else None
        self._state: Optional[dict] = None
        self._form: Optional[str] = None  # "numbered" ([n_utt, T, k] updates) or "flat" (rows with segments)
        self._submitted = 0  # rows handed to update so far, padding included (host-side bound of the int32 counts)
        self._bound = 0      # host-side upper bound of the occupied slots
        self.grown = 0       # how often the table was replaced by a larger one
        self._ws = None

    # ---- state ----------------------------------------------------------------------------------
    @staticmethod
    def _empty_table(cap: int, dev) -> dict:
        return {"keys": torch.full((cap,), -1, dtype=torch.int64, device=dev),  # (2^64 - 1 = empty)
                "cnt": torch.zeros(cap, dtype=torch.int32, device=dev),
                "sum_q": torch.zeros(cap, dtype=torch.int64, device=dev),
                "status": torch.zeros(2, dtype=torch.int64, device=dev)}

    def _ensure_device(self, like: Optional[Tensor] = None) -> torch.device:
        if self._state is not None:
            return self._state["keys"].device
        dev = _stream.need_gpu("TokenAssociation", self.device or (like.device if like is not None else None))
        self._state = self._empty_table(self._initial_capacity, dev)
        self._state.update(feat_rows=torch.zeros(self.hidden, dtype=torch.int64, device=dev),
                           tok_rows=torch.zeros(self.n_tokens, dtype=torch.int64, device=dev),
                           pair_rows=torch.zeros(1, dtype=torch.int64, device=dev))
        self.device = self._state["keys"].device
        return self.device

    feat_rows = _stream.state_property("feat_rows", "``[hidden]`` int64: the paired frames on which the feature was active.")
    tok_rows = _stream.state_property("tok_rows", "``[n_tokens]`` int64: the paired frames that carry the token.")
    pair_rows = _stream.state_property("pair_rows", "``[1]`` int64: the frames that form a pair.")

    @property
    def capacity(self) -> int:
        return self._initial_capacity if self._state is None else self._state["keys"].numel()

    def _read_status(self) -> int:
        """The occupied slots, read from the device (one synchronisation); ``WsaeError`` if anything was ever dropped."""
        occupied, dropped = self._state["status"].tolist()
        if dropped:
            raise N.WsaeError(f"TokenAssociation: {dropped} contributions found no slot in a table of {self.capacity} slots "
                              f"({occupied} occupied): the counts are incomplete")
        self._bound = occupied
        return occupied

    @property
    def n_pairs(self) -> int:
        """The distinct (feature, token) pairs seen so far."""
        self._ensure_device()
        return self._read_status()

    def _stream_ptr(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _insert(self, keys: Tensor, cnt: Tensor, sum_q: Tensor) -> None:
        """``wsae_pair_merge`` of a source table or list on this device into the table."""
        st = self._state
        with torch.cuda.device(self.device):
            N.check(N.lib().wsae_pair_merge(keys.data_ptr(), cnt.data_ptr(), sum_q.data_ptr(), keys.numel(), st["keys"].data_ptr(),
                                            st["cnt"].data_ptr(), st["sum_q"].data_ptr(), st["keys"].numel(),
                                            st["status"].data_ptr(), self._stream_ptr()), "wsae_pair_merge")

    def _reserve(self, more: int) -> None:
        """Room for ``more`` further slots under the rule occupied + more <= capacity / 2: by the host-side bound where it
        allows, else by one read of the true count, else by moving the contents into a larger table."""
        if self._bound + more > self.capacity // 2:
            occupied = self._read_status()
            if occupied + more > self.capacity // 2:
                cap = _pow2_at_least(2 * (occupied + more))
                if cap > MAX_CAPACITY:
                    raise N.WsaeError(f"TokenAssociation: {occupied} + {more} pairs need more than {MAX_CAPACITY} slots")
                old = {name: self._state[name] for name in ("keys", "cnt", "sum_q")}
                self._state.update(self._empty_table(cap, self.device))
                self._insert(old["keys"], old["cnt"], old["sum_q"])
                self.grown += 1
        self._bound += more

    # ---- accumulation ---------------------------------------------------------------------------
    def update(self, code, tokens: Tensor, segments: Optional[Tensor] = None, frame_mask: Optional[Tensor] = None) -> None:
        """One batch of whole utterances.  ``code = (values, indices)`` ``[n_utt, T, k]`` with ``tokens [n_utt, T]``, or
        flat ``[rows, k]`` with ``tokens [rows]`` and ``segments [rows]`` (the utterance of every row; < 0: padding).
        Frames with ``frame_mask == 0`` are padding: they fire nothing and carry no token."""
        vals, idx, k = _stream.compact_code(code, "code", N.PAIR_MAX_K, also=((tokens, "tokens"),))
        dev = self._ensure_device(vals)
        if vals.device != dev or tokens.device != dev:
            raise N.WsaeError(f"the code is on {vals.device} and the tokens on {tokens.device}, the tracker on {dev}")
        form = _stream.take_form(self, vals)
        seg, _ = _stream.frame_segments(vals, segments, frame_mask, dev)
        rows = seg.shape[0]
        _stream.check_frame_labels(vals, tokens)
        _stream.check_row_bound(self, rows)  # (a count is int32 and takes at most one per frame)
        self._form = form
        if rows == 0:
            return
        v, i = _stream.flat_code(vals, idx, k)
        tok = _stream.frame_labels(vals, tokens, self.n_tokens)
        self._reserve(rows * k)
        st = self._state
        with torch.cuda.device(dev):
            N.check(N.lib().wsae_pair_update(
                v.data_ptr(), i.data_ptr(), k, self.hidden, seg.data_ptr(), tok.data_ptr(), rows, self.n_tokens, self.lag,
                st["keys"].data_ptr(), st["cnt"].data_ptr(), st["sum_q"].data_ptr(), st["keys"].numel(), st["status"].data_ptr(),
                st["feat_rows"].data_ptr(), st["tok_rows"].data_ptr(), st["pair_rows"].data_ptr(), self._stream_ptr()),
                "wsae_pair_update")
        self._submitted += rows

    def merge(self, other: "TokenAssociation") -> None:
        """Add the state of a tracker of the same kind (size, vocabulary, lag) over other utterances: the other table's
        pairs are inserted into this one (which grows first where it must), the marginals add."""
        if (self.hidden, self.n_tokens, self.lag) != (other.hidden, other.n_tokens, other.lag):
            raise ValueError("merge needs two trackers with the same size, vocabulary and lag")
        _stream.check_row_bound(self, other._submitted, merging=True)
        if other._state is not None:
            dev = self._ensure_device(other._state["keys"])
            self._reserve(other._read_status())
            src = {name: t.to(dev) for name, t in other._state.items()}
            self._insert(src["keys"], src["cnt"], src["sum_q"])
            for name in ("feat_rows", "tok_rows", "pair_rows"):
                self._state[name] += src[name]
        self._form = self._form or other._form
        self._submitted += other._submitted

    # ---- reading --------------------------------------------------------------------------------
    def pairs(self) -> PairExport:
        """The canonical export: every pair on the CPU, keys ascending.  It does not depend on the slot layout."""
        self._ensure_device()
        self._read_status()
        st = self._state
        used = torch.nonzero(st["keys"] >= 0)[:, 0]
        keys, order = torch.sort(st["keys"][used])
        used = used[order]
        return PairExport((keys >> 32).cpu(), (keys & 0xFFFFFFFF).cpu(), st["cnt"][used].to(torch.int64).cpu(),
                          st["sum_q"][used].cpu())

    def _top(self, by: int, n: int, score: str, min_count: int) -> TopPairs:
        if score not in SCORES:
            raise ValueError(f"score must be one of {SCORES}, got {score!r}")
        if not 1 <= int(n) <= N.PAIR_MAX_N:
            raise ValueError(f"n must be in 1..{N.PAIR_MAX_N}, got {n}")
        n, min_count = int(n), max(int(min_count), 1)
        dev = self._ensure_device()
        self._read_status()
        st, lib = self._state, N.lib()
        groups = self.hidden if by == N.PAIR_BY_FEATURE else self.n_tokens
        cap = st["keys"].numel()
        need = lib.wsae_pair_top_workspace_bytes(cap, groups)
        if need < 0:
            raise N.WsaeError(f"wsae_pair_top_workspace_bytes rejects cap={cap} n_groups={groups}")
        ids = torch.empty(groups, n, dtype=torch.int32, device=dev)
        scores = torch.empty(groups, n, dtype=torch.float64, device=dev)
        counts = torch.empty(groups, n, dtype=torch.int32, device=dev)
        sums = torch.empty(groups, n, dtype=torch.int64, device=dev)
        ws = _stream.grow(self, (need + 7) // 8, torch.int64, dev)  # (8-byte aligned)
        with torch.cuda.device(dev):
            N.check(lib.wsae_pair_top(st["keys"].data_ptr(), st["cnt"].data_ptr(), st["sum_q"].data_ptr(), cap,
                                      st["feat_rows"].data_ptr(), st["tok_rows"].data_ptr(), st["pair_rows"].data_ptr(),
                                      self.hidden, self.n_tokens, by, groups, N.PAIR_SCORES.index("lift" if score == "pmi" else score),
                                      min_count, n, ids.data_ptr(), scores.data_ptr(), counts.data_ptr(), sums.data_ptr(),
                                      ws.data_ptr(), need, self._stream_ptr()), "wsae_pair_top")
        if score == "pmi":
            scores = torch.log(scores)  # (log of -inf behind the end of a list is NaN: put the marker back)
            scores = torch.where(ids >= 0, scores, torch.full_like(scores, float("-inf")))
        c = counts.double()
        mean = torch.where(counts > 0, sums.double() * Q_SCALE / torch.where(counts > 0, c, torch.ones_like(c)),
                           torch.full_like(c, float("nan")))
        return TopPairs(ids.to(torch.int64), scores, counts.to(torch.int64), mean)

    def top_tokens(self, n: int = 10, score: str = "lift", min_count: int = 5) -> TopPairs:
        """Per feature its ``n`` best tokens, ``[hidden, n]``.  With c the pair's count, a = ``feat_rows``, b =
        ``tok_rows`` and N = ``pair_rows``: ``count`` c, ``precision`` c / a, ``recall`` c / b, ``f1`` 2 c / (a + b),
        ``jaccard`` c / (a + b - c), ``lift`` c N / (a b), ``pmi`` log(lift), ``mean`` the mean activation.  Pairs with
        fewer than ``min_count`` frames are skipped."""
        return self._top(N.PAIR_BY_FEATURE, n, score, min_count)

    def top_features(self, n: int = 10, score: str = "precision", min_count: int = 5) -> TopPairs:
        """Per token its ``n`` best features, ``[n_tokens, n]``; the scores of ``top_tokens``."""
        return self._top(N.PAIR_BY_TOKEN, n, score, min_count)

    def describe(self, feature: int, vocab: Optional[Sequence[str]] = None, n: int = 10, score: str = "lift",
                 min_count: int = 5) -> List[Dict]:
        """The ``n`` best tokens of one feature as a list of dicts for a report: ``token``, ``text`` (``vocab[token]``, or
        the number), ``count``, ``score``, ``precision``, ``recall``, ``mean_activation``."""
        feature = _stream.check_index(feature, self.hidden, "feature")
        if vocab is not None and len(vocab) != self.n_tokens:
            raise ValueError(f"vocab has {len(vocab)} entries for {self.n_tokens} tokens")
        top = self.top_tokens(n, score, min_count)
        row = [field[feature].cpu() for field in top]
        a, tok_rows = int(self.feat_rows[feature]), self.tok_rows
        out = []
        for t, s, c, m in zip(*(field.tolist() for field in row)):
            if t < 0:
                break
            out.append({"token": t, "text": str(t) if vocab is None else vocab[t], "count": c, "score": s, "precision": c / a,
                        "recall": c / int(tok_rows[t]), "mean_activation": m})
        return out

    # ---- persistence ----------------------------------------------------------------------------
    def save(self, path) -> None:
        """The canonical export and the marginals - not the slot layout."""
        export = self.pairs()
        torch.save({"hidden": self.hidden, "n_tokens": self.n_tokens, "lag": self.lag, "capacity": self.capacity,
                    "form": self._form, "submitted": self._submitted, "pairs": dict(export._asdict()),
                    "marginals": {name: self._state[name].cpu() for name in ("feat_rows", "tok_rows", "pair_rows")}}, Path(path))

    @classmethod
    def load(cls, path, device=None) -> "TokenAssociation":
        data = torch.load(Path(path), map_location="cpu", weights_only=True)
        a = cls(data["hidden"], data["n_tokens"], data["lag"], data["capacity"], device=device)
        dev = a._ensure_device()
        p = data["pairs"]
        if p["count"].numel():
            a._reserve(p["count"].numel())
            a._insert(((p["feature"] << 32) | p["token"]).to(dev), p["count"].to(dev, torch.int32), p["sum_q"].to(dev))
        for name, t in data["marginals"].items():
            a._state[name].copy_(t)
        a._form, a._submitted = data["form"], int(data["submitted"])
        return a


def collect_token_association(model, utterances, n_tokens: int, *, lag: int = 0, capacity: int = 1 << 20,
                              device="cuda") -> TokenAssociation:
    """The token association over a dataset of utterances.  Every item of ``utterances`` is ``(x [n_utt, T, D],
    tokens [n_utt, T])`` or ``(x, tokens, frame_mask [n_utt, T])``.  The module must offer ``encode_compact`` (TopK and
    BatchTopK SAEs; a ReLU SAE's code is dense: ``TypeError``) and is run in eval mode; its previous mode is restored."""
    with _stream.encoding(model, hint="token association is for TopK-family codes"):
        assoc = TokenAssociation(model.hidden_dim, n_tokens, lag=lag, capacity=capacity, device=device)
        for x, tokens, mask in _stream.labelled_batches(utterances):
            assoc.update(_stream.utterance_code(model, x, device), tokens.to(device),
                         frame_mask=None if mask is None else mask.to(device))
    return assoc
