"""Token association on the MI355X: the table of ``wsae_pair_update`` / ``wsae_pair_merge`` (through its canonical export),
the marginals and ``status`` exactly against the dict oracle of tests/token_oracle.py - lags, both forms of ``seg``, rows
that straddle the blocks, the largest vocabulary, exact counts under contention, colliding keys that wrap around, a table
too small for its pairs (the probe loop is bounded), growth, batching and call order, merging - ``wsae_pair_top`` bit for
bit in both directions for every score, and the Python layer on real modules.  The inputs and the conditions that keep
them from being degenerate are checked on the CPU in tests/test_token_association.py."""

from __future__ import annotations

import tempfile

import numpy as np
import pytest
import torch

import token_oracle as TO
from whisper_sae import _native as N
from whisper_sae.analysis import PairExport, TokenAssociation, TopPairs, collect_token_association
from whisper_sae.sae.model import BatchTopKSAE, ReLUSAE, TopKSAE

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
JUNK = 0x5a5a5a5
TAIL = 3  # junk elements behind every state array


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class PairState:
    """Device state of the three entry points: every array has three more elements than its size, filled with junk that
    must survive; the workspace of ``wsae_pair_top`` holds 0xAB on entry and keeps it behind the size the query names."""

    def __init__(self, hidden, n_tokens, cap):
        self.hidden, self.n_tokens, self.cap = hidden, n_tokens, cap
        self.keys = torch.full((cap + TAIL,), -1, dtype=torch.int64, device=DEV)
        self.cnt = torch.zeros(cap + TAIL, dtype=torch.int32, device=DEV)
        self.sum_q = torch.zeros(cap + TAIL, dtype=torch.int64, device=DEV)
        self.status = torch.zeros(2 + TAIL, dtype=torch.int64, device=DEV)
        self.feat_rows = torch.zeros(hidden + TAIL, dtype=torch.int64, device=DEV)
        self.tok_rows = torch.zeros(n_tokens + TAIL, dtype=torch.int64, device=DEV)
        self.pair_rows = torch.zeros(1 + TAIL, dtype=torch.int64, device=DEV)
        for t, n in self._sized():
            t[n:] = JUNK

    def _sized(self):
        return ((self.keys, self.cap), (self.cnt, self.cap), (self.sum_q, self.cap), (self.status, 2),
                (self.feat_rows, self.hidden), (self.tok_rows, self.n_tokens), (self.pair_rows, 1))

    def update(self, code, seg, tokens, lag=0, n_rows=None, n_tokens=None):
        v, i = dev(np.asarray(code[0], np.float32)), dev(np.asarray(code[1], np.int32))
        s = None if seg is None else dev(np.asarray(seg, np.int32))
        tok = dev(np.asarray(tokens, np.int32))
        rc = N.lib().wsae_pair_update(v.data_ptr(), i.data_ptr(), v.shape[1], self.hidden, N.ptr(s), tok.data_ptr(),
                                      v.shape[0] if n_rows is None else n_rows, self.n_tokens if n_tokens is None else n_tokens,
                                      lag, self.keys.data_ptr(), self.cnt.data_ptr(), self.sum_q.data_ptr(), self.cap,
                                      self.status.data_ptr(), self.feat_rows.data_ptr(), self.tok_rows.data_ptr(),
                                      self.pair_rows.data_ptr(), torch.cuda.current_stream().cuda_stream)
        N.check(rc, "wsae_pair_update")
        torch.cuda.synchronize()
        return self

    def merge_from(self, src):
        N.check(N.lib().wsae_pair_merge(src.keys.data_ptr(), src.cnt.data_ptr(), src.sum_q.data_ptr(), src.cap, self.keys.data_ptr(),
                                        self.cnt.data_ptr(), self.sum_q.data_ptr(), self.cap, self.status.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream), "wsae_pair_merge")
        for name in ("feat_rows", "tok_rows", "pair_rows"):
            getattr(self, name)[:-TAIL] += getattr(src, name)[:-TAIL]
        torch.cuda.synchronize()
        return self

    def intact(self):
        return all(bool((t[n:] == JUNK).all()) for t, n in self._sized())

    def export(self):
        assert self.intact()
        keys = self.keys[:self.cap]
        used = torch.nonzero(keys >= 0)[:, 0]
        k, order = torch.sort(keys[used])
        used = used[order]
        assert int(self.status[0]) == used.numel()  # the occupied slots
        return {"feature": (k >> 32).cpu().numpy(), "token": (k & 0xFFFFFFFF).cpu().numpy(),
                "count": self.cnt[used].cpu().numpy().astype(np.int64), "sum_q": self.sum_q[used].cpu().numpy()}

    def marginals(self):
        return {"feat_rows": self.feat_rows[:self.hidden].cpu().numpy(), "tok_rows": self.tok_rows[:self.n_tokens].cpu().numpy(),
                "pair_rows": self.pair_rows[:1].cpu().numpy()}

    def equals(self, want, dropped=0):
        TO.same_export(self.export(), TO.export(want))
        TO.same_marginals(self.marginals(), want)
        assert self.status[:2].tolist() == [len(want["table"]), dropped]

    def top(self, by, score, min_count, n):
        groups = self.hidden if by == TO.BY_FEATURE else self.n_tokens
        lib = N.lib()
        need = lib.wsae_pair_top_workspace_bytes(self.cap, groups)
        assert need >= 0
        ws = torch.full((need + 64,), 0xAB, dtype=torch.uint8, device=DEV)  # (arbitrary contents on entry)
        out = {"ids": torch.full((groups * n + TAIL,), JUNK, dtype=torch.int32, device=DEV),
               "scores": torch.full((groups * n + TAIL,), 7.5, dtype=torch.float64, device=DEV),
               "counts": torch.full((groups * n + TAIL,), JUNK, dtype=torch.int32, device=DEV),
               "sums": torch.full((groups * n + TAIL,), JUNK, dtype=torch.int64, device=DEV)}
        N.check(lib.wsae_pair_top(self.keys.data_ptr(), self.cnt.data_ptr(), self.sum_q.data_ptr(), self.cap,
                                  self.feat_rows.data_ptr(), self.tok_rows.data_ptr(), self.pair_rows.data_ptr(), self.hidden,
                                  self.n_tokens, by, groups, TO.SCORES.index(score), min_count, n, out["ids"].data_ptr(),
                                  out["scores"].data_ptr(), out["counts"].data_ptr(), out["sums"].data_ptr(), ws.data_ptr(), need,
                                  torch.cuda.current_stream().cuda_stream), "wsae_pair_top")
        torch.cuda.synchronize()
        assert bool((ws[need:] == 0xAB).all()) and self.intact()
        for name, junk in (("ids", JUNK), ("scores", 7.5), ("counts", JUNK), ("sums", JUNK)):
            assert bool((out[name][groups * n:] == junk).all()), name
        return {name: t[:groups * n].reshape(groups, n).cpu().numpy() for name, t in out.items()}


@pytest.fixture(scope="module")
def general():
    return TO.general_case()


@pytest.fixture(scope="module")
def general_state(general):
    """The general case at lag 0 on the device and in the oracle, shared by the tests that only read it."""
    code, seg, tokens = general
    return (PairState(TO.HIDDEN, TO.TOKENS, 1 << 18).update(code, seg, tokens, 0),
            TO.update(code, seg, tokens, TO.HIDDEN, TO.TOKENS, 0))


# ---- 1: the general case ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lag", TO.LAGS)
def test_state_equals_the_oracle(general, lag):
    code, seg, tokens = general
    for s in (seg, None):
        got = PairState(TO.HIDDEN, TO.TOKENS, 1 << 18).update(code, s, tokens, lag)
        got.equals(TO.update(code, s, tokens, TO.HIDDEN, TO.TOKENS, lag))


def test_wide_dictionary_takes_the_global_feature_counts():
    """More features than a block counts in LDS: ``feat_rows`` goes to memory directly."""
    rng = np.random.default_rng(2730)
    rows, k, hidden, n_tokens = 700, 32, 9000, 600
    code = TO.RO.spoil(rng, TO.RO.persistent_code(rng, rows, k, hidden), hidden)
    seg = (np.arange(rows) // 90).astype(np.int32)
    tokens = TO.zipf_tokens(rng, rows, n_tokens)
    want = TO.update(code, seg, tokens, hidden, n_tokens, 1)
    assert (want["feat_rows"][8192:] > 0).any()
    PairState(hidden, n_tokens, 1 << 16).update(code, seg, tokens, 1).equals(want)


# ---- 2: rows that straddle the 256-entry blocks -------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 31, 32, 33, 128])
def test_width_edges(k):
    code, seg, tokens = TO.wide_case(k)
    for lag in (0, 1):
        PairState(300, 40, 1 << 16).update(code, seg, tokens, lag).equals(TO.update(code, seg, tokens, 300, 40, lag))


# ---- 3: the largest vocabulary ------------------------------------------------------------------------------------------------
def test_vocabulary_edge():
    n_tokens = 1 << 24
    rng = np.random.default_rng(2740)
    rows, k, hidden = 300, 8, 64
    code = TO.RO.persistent_code(rng, rows, k, hidden)
    tokens = np.repeat(rng.choice(np.array([0, n_tokens - 1, n_tokens - 2, 1, 12345678, n_tokens, -1], np.int64), rows // 5), 5)
    tokens[:5], tokens[5:10] = 0, n_tokens - 1
    tokens = tokens.astype(np.int32)
    want = TO.update(code, None, tokens, hidden, n_tokens, -1)
    assert want["tok_rows"][0] > 0 and want["tok_rows"][n_tokens - 1] > 0 and want["pair_rows"][0] < rows - 1
    st = PairState(hidden, n_tokens, 1 << 13).update(code, None, tokens, -1)
    st.equals(want)
    TO.same_top(st.top(TO.BY_FEATURE, "lift", 1, 4), TO.top(want, TO.BY_FEATURE, "lift", 1, 4))
    got, ref = st.top(TO.BY_TOKEN, "precision", 1, 1), TO.top(want, TO.BY_TOKEN, "precision", 1, 1)
    TO.same_top(got, ref)
    assert ref["ids"][0, 0] >= 0 and ref["ids"][n_tokens - 1, 0] >= 0 and (ref["ids"] >= 0).sum() == 5
    rc = N.lib().wsae_pair_update(4096, 4096, k, hidden, None, 4096, rows, n_tokens + 1, 0, 4096, 4096, 4096, 1024, 4096, 4096, 4096,
                                  4096, None)
    assert rc == -1 and "n_tokens" in N.last_error()  # rejected on the host: the made-up pointers were never read


# ---- 4: exact counts under contention -----------------------------------------------------------------------------------------
def test_counts_exactly_under_contention():
    rows = 20_000
    vals = np.tile(np.array([[1.5, 0.25]], np.float32), (rows, 1))
    idx = np.tile(np.array([[3, 5]], np.int32), (rows, 1))
    tokens = ((np.arange(rows) // 10) % 2 * 7).astype(np.int32)  # tokens 0 and 7 in runs of ten frames
    want = TO.update((vals, idx), None, tokens, 16, 8)
    assert want["table"] == {TO.key_of(3, 0): [rows // 2, rows // 2 * 3 * 2 ** 19], TO.key_of(3, 7): [rows // 2, rows // 2 * 3 * 2 ** 19],
                             TO.key_of(5, 0): [rows // 2, rows // 2 * 2 ** 18], TO.key_of(5, 7): [rows // 2, rows // 2 * 2 ** 18]}
    PairState(16, 8, 1 << 17).update((vals, idx), None, tokens).equals(want)


# ---- 5: colliding keys and wrap-around ----------------------------------------------------------------------------------------
def test_collisions_and_wrap_around():
    code, tokens, keys = TO.collision_case()
    want = TO.update(code, None, tokens, 64, 4096)
    st = PairState(64, 4096, 1024).update(code, None, tokens)
    st.equals(want)  # every key is found, with its exact count
    # the keys that start in the last two slots wrapped around: the first slots of the table hold them
    late = {k for k in keys if TO.home_slot(k, 1024) >= 1022}
    held = st.keys[:1024].cpu().numpy()
    assert len(late) >= 16 and sum(int(k) in late for k in held[:64]) >= 14
    # a table of twice the size, by wsae_pair_merge: the same export
    PairState(64, 4096, 2048).merge_from(st).equals(want)


# ---- 6: a table too small for its pairs ---------------------------------------------------------------------------------------
def test_overfull_table_drops_and_counts_what_it_cannot_hold():
    n = 2000
    counts = 1 + np.arange(n) % 3
    f, t = np.repeat(np.arange(n) % 50, counts), np.repeat(np.arange(n), counts)
    order = np.random.default_rng(2750).permutation(f.size)
    code = (np.ones((f.size, 1), np.float32), f[order].reshape(-1, 1).astype(np.int32))
    tokens = t[order].astype(np.int32)
    want = TO.update(code, None, tokens, 50, n)
    assert len(want["table"]) == n
    st = PairState(50, n, 1024).update(code, None, tokens)  # returns WSAE_OK, and returns at all: the probe loop is bounded
    assert st.intact()
    occupied, dropped = st.status[:2].tolist()
    ex = st.export()
    landed = {TO.key_of(a, b): c for a, b, c in zip(ex["feature"].tolist(), ex["token"].tolist(), ex["count"].tolist())}
    missing = set(want["table"]) - set(landed)
    assert occupied <= 1024 and occupied == len(landed) and occupied + len(missing) == n
    assert dropped > 0 and dropped == sum(want["table"][k][0] for k in missing)
    assert all(want["table"][k][0] == c for k, c in landed.items())  # what landed carries exact counts
    TO.same_marginals(st.marginals(), want)  # the marginals count every pair
    # the Python layer, its bookkeeping bypassed
    tracker = TokenAssociation(50, n, capacity=1024, device=DEV)
    tracker._reserve = lambda more: None
    tracker.update((dev(code[0]), dev(code[1])), dev(tokens), segments=torch.zeros(f.size, dtype=torch.int32, device=DEV))
    with pytest.raises(N.WsaeError, match="found no slot"):
        tracker.n_pairs
    with pytest.raises(N.WsaeError):
        tracker.pairs()
    with pytest.raises(N.WsaeError):
        tracker.top_tokens()


# ---- 7 and 8: growth, batching and call order ---------------------------------------------------------------------------------
def utterance_chunks(seg):
    """Row ranges that hold whole utterances each: cut where a new utterance begins (padding goes with the one before)."""
    starts = [int(np.nonzero(seg == u)[0][0]) for u in np.unique(seg[seg >= 0])]
    starts[0] = 0
    return list(zip(starts, starts[1:] + [seg.size]))


def tracker_state(t):
    return {"feat_rows": t.feat_rows.cpu().numpy(), "tok_rows": t.tok_rows.cpu().numpy(), "pair_rows": t.pair_rows.cpu().numpy()}


def feed(tracker, general, chunks):
    code, seg, tokens = general
    for a, b in chunks:
        tracker.update((dev(code[0][a:b]), dev(code[1][a:b])), dev(tokens[a:b]), segments=dev(seg[a:b]))
    return tracker


def test_growth(general, general_state):
    want = general_state[1]
    chunks = utterance_chunks(general[1])
    small = feed(TokenAssociation(TO.HIDDEN, TO.TOKENS, capacity=1024, device=DEV), general, chunks)
    large = feed(TokenAssociation(TO.HIDDEN, TO.TOKENS, capacity=1 << 20, device=DEV), general, chunks)
    assert small.grown >= 2 and large.grown == 0 and large.capacity == 1 << 20
    assert small.n_pairs == large.n_pairs == len(want["table"]) <= small.capacity // 2
    for t in (small, large):
        assert isinstance(t.pairs(), PairExport)
        TO.same_export({k: v.numpy() for k, v in t.pairs()._asdict().items()}, TO.export(want))
        TO.same_marginals(tracker_state(t), want)


def test_batching_and_call_order_do_not_matter(general):
    code, seg, tokens = general
    chunks = utterance_chunks(seg)
    assert len(chunks) == TO.UTTS
    for lag in (-2, 3):
        want = TO.update(code, seg, tokens, TO.HIDDEN, TO.TOKENS, lag)
        for order in (chunks, chunks[::-1]):
            st = PairState(TO.HIDDEN, TO.TOKENS, 1 << 18)
            for a, b in order:
                st.update((code[0][a:b], code[1][a:b]), seg[a:b], tokens[a:b], lag)
            st.equals(want)
    st = PairState(TO.HIDDEN, TO.TOKENS, 1 << 18).update(code, seg, tokens, 3)
    st.update(code, seg, tokens, 3, n_rows=0)  # no rows: nothing is touched
    st.equals(TO.update(code, seg, tokens, TO.HIDDEN, TO.TOKENS, 3))


# ---- 9: merging ---------------------------------------------------------------------------------------------------------------
def test_merge(general, general_state):
    want = general_state[1]
    chunks = utterance_chunks(general[1])
    a = feed(TokenAssociation(TO.HIDDEN, TO.TOKENS, capacity=1 << 17, device=DEV), general, chunks[:5])
    b = feed(TokenAssociation(TO.HIDDEN, TO.TOKENS, capacity=1 << 17, device=DEV), general, chunks[5:])
    tiny = TokenAssociation(TO.HIDDEN, TO.TOKENS, capacity=1024, device=DEV)
    tiny.merge(a)  # into a smaller table, which must grow first
    assert tiny.grown == 1 and tiny.n_pairs == a.n_pairs
    tiny.merge(b)
    b.merge(a)
    for t in (b, tiny):
        TO.same_export({k: v.numpy() for k, v in t.pairs()._asdict().items()}, TO.export(want))
        TO.same_marginals(tracker_state(t), want)
        assert t._submitted == TO.ROWS


# ---- 10: the selections -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("score", TO.SCORES)
@pytest.mark.parametrize("by", [TO.BY_FEATURE, TO.BY_TOKEN], ids=["per_feature", "per_token"])
def test_top_equals_the_oracle(general_state, by, score):
    st, want = general_state
    for n in (1, 10, 32):
        for min_count in (1, 3):
            ref = TO.top(want, by, score, min_count, n)
            TO.same_top(st.top(by, score, min_count, n), ref, (by, score, n, min_count))
    assert (ref["ids"][:, 0] < 0).any() and ((ref["ids"][:, 0] >= 0) & (ref["ids"][:, -1] < 0)).any()  # empty and short lists


# ---- 11: the Python layer -----------------------------------------------------------------------------------------------------
D, H, K, UTT, T, VOCAB = 64, 256, 8, 6, 50, 500


def utterances(seed):
    """6 utterances of 50 frames in three batches, with tokens in runs and a frame mask.  A frame repeats for a stretch
    of about three frames, so a feature fires often."""
    gen = torch.Generator().manual_seed(seed)
    proto = torch.randn(UTT, 14, D, generator=gen)
    hold = (torch.rand(UTT, T, generator=gen) < 0.3).cumsum(1) % 14
    x = torch.gather(proto, 1, hold[:, :, None].expand(UTT, T, D)) * torch.exp(torch.randn(UTT, T, 1, generator=gen))
    mask = torch.ones(UTT, T)
    for u in range(UTT):
        mask[u, 38 + (u % 4) * 3:] = 0
    mask[3, 10] = 0
    rng = np.random.default_rng(seed)
    tokens = torch.from_numpy(TO.zipf_tokens(rng, UTT * T, VOCAB, 3, 9).astype(np.int64).reshape(UTT, T))
    tokens[2, 5:9], tokens[4, 20] = -1, VOCAB
    return [(x[:3], tokens[:3], mask[:3]), (x[3:4], tokens[3:4], mask[3:4]), (x[4:], tokens[4:], mask[4:])], mask, tokens


@pytest.mark.parametrize("kind", ["topk", "batch_topk"])
def test_python_layer_on_real_modules(kind):
    torch.manual_seed(1 if kind == "topk" else 2)
    sae = (TopKSAE(D, H, k=K) if kind == "topk" else BatchTopKSAE(D, H, k=K, max_k_per_row=16)).to(DEV)
    batches, mask, tokens = utterances(5)
    sae.train()
    assoc = collect_token_association(sae, batches, VOCAB, lag=1, capacity=1024)
    assert sae.training and assoc.lag == 1
    sae.eval()
    codes = [sae.encode_compact(x.to(DEV)) for x, _, _ in batches]
    vals, idx = (np.concatenate([c[i].reshape(-1, c[i].shape[-1]).cpu().numpy() for c in codes]) for i in (0, 1))
    seg = np.where(mask.reshape(-1).numpy() != 0, np.repeat(np.arange(UTT), T), -1).astype(np.int32)
    flat_tokens = tokens.reshape(-1).numpy()
    want = TO.update((vals, idx), seg, flat_tokens, H, VOCAB, 1)
    assert want["pair_rows"][0] > 150 and len(want["table"]) > 500

    def same(tracker, ref):
        TO.same_export({k: v.numpy() for k, v in tracker.pairs()._asdict().items()}, TO.export(ref))
        TO.same_marginals(tracker_state(tracker), ref)
        assert tracker.n_pairs == len(ref["table"])

    same(assoc, want)
    for by, call in ((TO.BY_FEATURE, assoc.top_tokens), (TO.BY_TOKEN, assoc.top_features)):
        for score in ("lift", "precision", "mean"):
            got, ref = call(n=5, score=score, min_count=2), TO.top(want, by, score, 2, 5)
            assert isinstance(got, TopPairs) and got.ids.dtype == torch.int64 and got.scores.dtype == torch.float64
            TO.same_top({"ids": got.ids.cpu().numpy(), "scores": got.scores.cpu().numpy(), "counts": got.counts.cpu().numpy(),
                         "sums": ref["sums"]}, ref, (by, score))
            mean = np.where(ref["counts"] > 0, ref["sums"] * 2.0 ** -20 / np.maximum(ref["counts"], 1), np.nan)
            assert np.array_equal(got.mean_activation.cpu().numpy(), mean, equal_nan=True)
    pmi, lift = assoc.top_tokens(n=5, score="pmi", min_count=2), TO.top(want, TO.BY_FEATURE, "lift", 2, 5)
    assert np.array_equal(pmi.ids.cpu().numpy(), lift["ids"])
    listed = lift["ids"] >= 0  # (behind the end of a list the score stays -inf)
    assert np.array_equal(pmi.scores.cpu().numpy()[~listed], lift["scores"][~listed]) and listed.sum() > 100
    np.testing.assert_allclose(pmi.scores.cpu().numpy()[listed], np.log(lift["scores"][listed]), rtol=1e-14, atol=1e-15)
    busy = int(np.argmax(want["feat_rows"]))
    lines = assoc.describe(busy, vocab=[f"tok{t}" for t in range(VOCAB)], n=5, min_count=2)
    assert [e["token"] for e in lines] == [t for t in lift["ids"][busy].tolist() if t >= 0] and lines
    assert all(e["text"] == f"tok{e['token']}" and e["count"] >= 2 and 0 < e["precision"] <= 1 and 0 < e["recall"] <= 1 for e in lines)
    # flat codes with segments; forms do not mix; two shards; save / load, and a loaded tracker goes on counting
    flat = TokenAssociation(H, VOCAB, lag=1, capacity=1 << 14, device=DEV)
    flat.update((dev(vals), dev(idx)), dev(flat_tokens), segments=dev(seg))
    same(flat, want)
    with pytest.raises(ValueError):
        flat.update((dev(vals).reshape(UTT, T, -1), dev(idx).reshape(UTT, T, -1)), dev(flat_tokens).reshape(UTT, T))
    a = collect_token_association(sae, batches[:1], VOCAB, lag=1, capacity=1024)
    b = collect_token_association(sae, batches[1:], VOCAB, lag=1, capacity=1024)
    b.merge(a)
    same(b, want)
    with tempfile.TemporaryDirectory(prefix="wsae_tokens_") as d:
        assoc.save(f"{d}/a.pt")
        back = TokenAssociation.load(f"{d}/a.pt", device=DEV)
    same(back, want)
    assert back._submitted == UTT * T and back.lag == 1 and back.capacity == assoc.capacity
    x0, t0, m0 = batches[1]
    c0 = sae.encode_compact(x0.to(DEV))
    back.update((c0[0].reshape(1, T, -1), c0[1].reshape(1, T, -1)), t0.to(DEV), frame_mask=m0.to(DEV))
    again = (c0[0].reshape(T, -1).cpu().numpy(), c0[1].reshape(T, -1).cpu().numpy())
    same(back, TO.update(again, np.where(m0.reshape(-1).numpy() != 0, 0, -1), t0.reshape(-1).numpy(), H, VOCAB, 1, state=want))
    # errors that need the device
    with pytest.raises(N.WsaeError):
        assoc.update((torch.from_numpy(vals), torch.from_numpy(idx)), torch.from_numpy(flat_tokens), segments=torch.from_numpy(seg))
    with pytest.raises(ValueError):
        assoc.update((dev(vals).reshape(UTT, T, -1), dev(idx).reshape(UTT, T, -1)), dev(flat_tokens)[:7])
    with pytest.raises(ValueError):
        assoc.update((dev(vals).reshape(UTT, T, -1), dev(idx).reshape(UTT, T, -1)), dev(flat_tokens).reshape(UTT, T).float())
    with pytest.raises(ValueError):
        assoc.describe(H)
    with pytest.raises(TypeError):
        collect_token_association(ReLUSAE(D, H).to(DEV), batches, VOCAB)
