"""Label association on the MI355X: the state of ``wsae_label_update`` bit for bit against the numpy oracle of
tests/label_oracle.py - every lag set, stratum count, window and both forms of ``seg``, rows that straddle the blocks,
exact counts under contention, the grid-stride loop, both forms of the ``pair_rows`` sum - the properties that make the
state independent of batching and call order, and the Python layer on real modules.  The inputs and the conditions that
keep them from being degenerate are checked on the CPU in tests/test_label_association.py."""

from __future__ import annotations

import re
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch

import label_oracle as LO
import runs_oracle as RO
from whisper_sae import _native as N
from whisper_sae.analysis import (BestLabels, LabelAssociation, LabelScores, automated_labels, best_labels,
                                  collect_activation_profile, collect_label_association, top_label_features)
from whisper_sae.sae.model import BatchTopKSAE, ReLUSAE, TopKSAE

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
JUNK = 0x5a5a5a5
TAIL = 3  # junk rows behind every state array
SOURCE = Path(__file__).resolve().parents[1] / "whisper-sae_amd" / "csrc" / "wsae_labels.hip"


def kernel_constant(name):
    return int(re.search(r"constexpr int " + name + r" = (\d+);", SOURCE.read_text()).group(1))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class LabelState:
    """Device state of ``wsae_label_update``: ``cnt`` has three more feature rows than the window and ``pair_rows`` three
    more rows than lags, filled with junk that must survive; the workspace holds 0xAB on entry and keeps it behind the
    size the query names."""

    def __init__(self, hidden, C, lags, edges=None, window=None):
        self.hidden, self.C, self.lags = hidden, C, lags
        self.f_lo, self.f_cols = (0, hidden) if window is None else window
        self.L = lags[1] - lags[0] + 1
        self.S = 1 if edges is None else edges.shape[1] + 1
        self.edges = None if edges is None else dev(np.asarray(edges, np.float32))
        self.cnt = torch.zeros(self.f_cols + TAIL, self.L, C, self.S, dtype=torch.int32, device=DEV)
        self.pair_rows = torch.zeros(self.L + TAIL, C, dtype=torch.int64, device=DEV)
        self.cnt[self.f_cols:], self.pair_rows[self.L:] = JUNK, JUNK

    def update(self, code, seg, labels, n_rows=None):
        v, i = dev(code[0]), dev(code[1])
        s = None if seg is None else dev(np.asarray(seg, np.int32))
        lab = dev(np.asarray(labels, np.int32))
        n_rows = v.shape[0] if n_rows is None else n_rows
        lib = N.lib()
        need = lib.wsae_label_workspace_bytes(n_rows, v.shape[1], self.hidden, self.f_lo, self.f_cols, self.C, self.lags[0],
                                              self.lags[1], self.S)
        assert need >= 0
        ws = torch.full((need + 64,), 0xAB, dtype=torch.uint8, device=DEV)  # (arbitrary contents on entry)
        N.check(lib.wsae_label_update(v.data_ptr(), i.data_ptr(), v.shape[1], self.hidden, N.ptr(s), lab.data_ptr(), n_rows,
                                      self.C, self.lags[0], self.lags[1], self.f_lo, self.f_cols, N.ptr(self.edges), self.S,
                                      self.cnt.data_ptr(), self.pair_rows.data_ptr(), ws.data_ptr(), need,
                                      torch.cuda.current_stream().cuda_stream), "wsae_label_update")
        torch.cuda.synchronize()
        assert bool((ws[need:] == 0xAB).all())
        return self

    def arrays(self):
        assert bool((self.cnt[self.f_cols:] == JUNK).all()) and bool((self.pair_rows[self.L:] == JUNK).all())
        return {"cnt": self.cnt[:self.f_cols].cpu().numpy(), "pair_rows": self.pair_rows[:self.L].cpu().numpy()}


@pytest.fixture(scope="module")
def general():
    return LO.general_case()


# ---- 1: the general case ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [None, LO.WINDOW], ids=["all", "window"])
@pytest.mark.parametrize("lags", LO.LAGS, ids=lambda l: f"lags{l[0]}_{l[1]}")
@pytest.mark.parametrize("S", LO.STRATA, ids=lambda s: f"S{s}")
def test_state_equals_the_oracle(general, S, lags, window):
    code, seg, labels = general
    edges = LO.general_edges(S, window)
    got = LabelState(LO.HIDDEN, LO.CLASSES, lags, edges, window).update(code, seg, labels).arrays()
    LO.same(got, LO.update(code, seg, labels, LO.HIDDEN, LO.CLASSES, lags, edges, window))
    # without seg: one segment, nothing is padding
    got = LabelState(LO.HIDDEN, LO.CLASSES, lags, edges, window).update(code, None, labels).arrays()
    LO.same(got, LO.update(code, None, labels, LO.HIDDEN, LO.CLASSES, lags, edges, window))


# ---- 2: rows that straddle the 256-entry blocks -------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 31, 32, 33, 128])
def test_width_edges(k):
    code, seg, labels = LO.wide_case(k)
    edges = np.sort(np.random.default_rng(k).uniform(0.02, 40.0, (300, 3)).astype(np.float32), axis=1)
    for window in (None, (250, 50)):
        e = edges if window is None else edges[250:300]
        got = LabelState(300, 5, (-1, 1), e, window).update(code, seg, labels).arrays()
        LO.same(got, LO.update(code, seg, labels, 300, 5, (-1, 1), e, window))


# ---- 3: exact counts under contention -----------------------------------------------------------------------------------------
def test_counts_exactly_under_contention():
    rows = 20_000
    vals = np.ones((rows, 2), np.float32)
    idx = np.tile(np.array([[3, 5]], np.int32), (rows, 1))
    labels = np.zeros(rows, np.int32)
    want = LO.update((vals, idx), None, labels, 16, 1, (-1, 1))
    assert want["cnt"][3].reshape(-1).tolist() == [rows - 1, rows, rows - 1] == want["cnt"][5].reshape(-1).tolist()
    assert want["pair_rows"].reshape(-1).tolist() == [rows - 1, rows, rows - 1] and want["cnt"].sum() == 2 * (3 * rows - 2)
    LO.same(LabelState(16, 1, (-1, 1)).update((vals, idx), None, labels).arrays(), want)


# ---- 4: more entries than one pass of the grid --------------------------------------------------------------------------------
def test_more_entries_than_one_pass_of_the_grid():
    block, grid = kernel_constant("LB_BLOCK"), kernel_constant("LB_MAX_BLOCKS")
    k, hidden, C = 32, 512, 5
    rows = block * grid // k + 301  # the grid-stride loop runs a second, partial time
    assert rows * k > block * grid and (rows * k) % block
    rng = np.random.default_rng(2300)
    code = RO.persistent_code(rng, rows, k, hidden)
    seg = (np.arange(rows) // 1500).astype(np.int32)
    labels = LO.piecewise_labels(rng, rows, C)
    window = (100, 64)
    edges = np.full((64, 1), 0.7, np.float32)
    want = LO.update(code, seg, labels, hidden, C, (-1, 1), edges, window)
    assert want["cnt"].min() >= 0 and (want["cnt"].sum((0, 1, 2)) > 1000).all()
    LO.same(LabelState(hidden, C, (-1, 1), edges, window).update(code, seg, labels).arrays(), want)


# ---- 5: both forms of the pair_rows sum ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [256, 257, 1024])
def test_both_pair_rows_forms(C):
    cells = kernel_constant("LB_LDS_CELLS")
    lags = (-7, 8)  # L = 16
    assert (16 * C <= cells) == (C == 256) and 16 * 256 == cells  # at the bound, just over it, the largest table
    rng = np.random.default_rng(2400 + C)
    rows, k, hidden, window = 3000, 4, 64, (8, 8)
    code = RO.spoil(rng, RO.persistent_code(rng, rows, k, hidden), hidden)
    seg = (np.arange(rows) // 700).astype(np.int32)
    seg[rng.random(rows) < 0.05] = -1
    labels = rng.integers(-1, C + 1, rows).astype(np.int32)
    labels[:C] = np.arange(C)
    want = LO.update(code, seg, labels, hidden, C, lags, None, window)
    assert (want["pair_rows"] > 0).mean() > 0.8 and want["pair_rows"][:, C - 1].sum() > 0 and want["cnt"].sum() > 1000
    LO.same(LabelState(hidden, C, lags, None, window).update(code, seg, labels).arrays(), want)


# ---- 6: batching and call order -----------------------------------------------------------------------------------------------
def utterance_cuts(seg, at):
    """Rows near ``at`` where an utterance ends: both neighbours live, in different utterances."""
    out = []
    for a in at:
        r = next(i for i in range(a, seg.size) if seg[i - 1] >= 0 and seg[i] >= 0 and seg[i - 1] != seg[i])
        out.append(r)
    return out


def test_batching_and_call_order_do_not_matter(general):
    code, seg, labels = general
    lags, S = (-2, 3), 4
    edges = LO.general_edges(S)
    want = LO.update(code, seg, labels, LO.HIDDEN, LO.CLASSES, lags, edges)
    c1, c2 = utterance_cuts(seg, (130, 420))
    cuts = [(0, c1), (c1, c2), (c2, LO.ROWS)]
    for order in (cuts, cuts[::-1]):
        st = LabelState(LO.HIDDEN, LO.CLASSES, lags, edges)
        for a, b in order:
            st.update((code[0][a:b], code[1][a:b]), seg[a:b], labels[a:b])
        LO.same(st.arrays(), want)
    # two shards merged equal one stream
    shards = []
    for a, b in ((0, c2), (c2, LO.ROWS)):
        t = LabelAssociation(LO.HIDDEN, LO.CLASSES, torch.from_numpy(edges), lags=lags, device=DEV)
        t.update((dev(code[0][a:b]), dev(code[1][a:b])), dev(labels[a:b]), segments=dev(seg[a:b]))
        shards.append(t)
    shards[1].merge(shards[0])
    LO.same({"cnt": shards[1].cnt.cpu().numpy(), "pair_rows": shards[1].pair_rows.cpu().numpy()}, want)


# ---- 7: no rows ---------------------------------------------------------------------------------------------------------------
def test_no_rows_leave_the_state_untouched(general):
    code, seg, labels = general
    edges = LO.general_edges(4)
    st = LabelState(LO.HIDDEN, LO.CLASSES, (-2, 3), edges).update(code, seg, labels)
    st.update(code, seg, labels, n_rows=0)
    st.update(code, None, labels, n_rows=0)
    LO.same(st.arrays(), LO.update(code, seg, labels, LO.HIDDEN, LO.CLASSES, (-2, 3), edges))


# ---- 8: the Python layer ------------------------------------------------------------------------------------------------------
D, H, K, UTT, T, C = LO.D, LO.H, LO.SAE_K, LO.UTT, LO.T, LO.PY_CLASSES


def utterances(seed):
    """12 utterances of 40 frames in three batches, with labels and a frame mask.  A frame repeats for a stretch of about
    three frames at a loudness that varies over a few octaves, so a feature fires often and over a range of values."""
    gen = torch.Generator().manual_seed(seed)
    proto = torch.randn(UTT, 14, D, generator=gen)
    hold = (torch.rand(UTT, T, generator=gen) < 0.3).cumsum(1) % 14
    x = torch.gather(proto, 1, hold[:, :, None].expand(UTT, T, D)) * torch.exp(torch.randn(UTT, T, 1, generator=gen))
    mask = torch.ones(UTT, T)
    for u in range(UTT):
        mask[u, 24 + (u % 5) * 3:] = 0
    mask[3, 10] = 0
    labels = torch.from_numpy(LO.python_layer_labels())
    return [(x[:5], labels[:5], mask[:5]), (x[5:6], labels[5:6], mask[5:6]), (x[6:], labels[6:], mask[6:])], mask, labels


def make_sae(cls, seed, **kw):
    torch.manual_seed(seed)
    return cls(D, H, k=K, **kw).to(DEV)


def state_of(assoc):
    return {"cnt": assoc.cnt.cpu().numpy(), "pair_rows": assoc.pair_rows.cpu().numpy()}


@pytest.mark.parametrize("kind", ["topk", "batch_topk"])
def test_python_layer_on_real_modules(kind):
    sae = make_sae(TopKSAE, 1) if kind == "topk" else make_sae(BatchTopKSAE, 2, max_k_per_row=16)
    batches, mask, labels = utterances(5)
    lags, S = (-2, 2), 5
    sae.train()
    prof = collect_activation_profile(sae, [(x, m) for x, _, m in batches])
    assoc = collect_label_association(sae, batches, C, prof, n_strata=S, lags=lags)
    assert sae.training and assoc.n_strata == S and (assoc.f_lo, assoc.f_cols) == (0, H)
    sae.eval()
    codes = [sae.encode_compact(x.to(DEV)) for x, _, _ in batches]
    vals, idx = (np.concatenate([c[i].reshape(-1, c[i].shape[-1]).cpu().numpy() for c in codes]) for i in (0, 1))
    seg = np.where(mask.reshape(-1).numpy() != 0, np.repeat(np.arange(UTT), T), -1).astype(np.int32)
    flat_labels = labels.reshape(-1).numpy()
    edges = prof.quantile_edges(S).cpu().numpy()
    want = LO.update((vals, idx), seg, flat_labels, H, C, lags, edges)
    assert want["pair_rows"].min() > 0 and (want["cnt"].sum((1, 2, 3)) >= 10).sum() >= 10 and (want["cnt"].sum((0, 1, 2)) > 0).all()
    LO.same(state_of(assoc), want)
    # the readers: ratios of exact integers after a handful of float64 operations
    compared = 0
    for metric in LO.METRICS:
        for lag in (0, "best"):
            got, ref = assoc.scores(metric, lag, 3), LO.scores(want, lags, edges, metric, lag, 3)
            assert isinstance(got, LabelScores)
            np.testing.assert_allclose(got.score.cpu().numpy(), ref["score"], rtol=1e-12, atol=1e-12, equal_nan=True,
                                       err_msg=f"{metric} {lag}")
            for name in ("threshold_index", "lag", "tp", "fires", "positives"):
                assert np.array_equal(getattr(got, name).cpu().numpy(), ref[name]), (metric, lag, name)
            assert np.array_equal(got.threshold.cpu().numpy(), ref["threshold"], equal_nan=True)
        # the lists of a real module's small dataset hold equal scores (ratios of small integers), so they are compared
        # where the oracle's scores differ by more than 1e-9: the classes whose first n + 1 scores do, the features whose
        # best two classes do.  test_selection_on_inputs_with_distinct_scores compares every list.
        ref = LO.scores(want, lags, edges, metric, "best", 3)
        clear_c, clear_f = LO.selection_gaps_hold(ref["score"], 5), LO.best_label_gaps_hold(ref["score"])
        feats, top = top_label_features(assoc, n=5, metric=metric, lag="best", min_count=3)
        wf, wv = LO.top_label_features(ref["score"], 5)
        assert np.array_equal(feats.cpu().numpy()[clear_c], wf[clear_c]), metric
        np.testing.assert_allclose(top.cpu().numpy(), wv, rtol=1e-12, atol=1e-12, equal_nan=True)
        bl, wb = best_labels(assoc, metric, "best", 3), LO.best_labels(ref)
        assert isinstance(bl, BestLabels)
        for name in ("label", "threshold_index", "lag", "tp", "fires", "positives"):
            assert np.array_equal(getattr(bl, name).cpu().numpy()[clear_f], wb[name][clear_f]), (metric, name)
        compared += int(clear_c.sum()) + int(clear_f.sum())
    assert compared > 7 * H // 4  # (the restriction leaves most of the 7 (C + H) cells)
    auto = automated_labels(assoc, [f"ph{c}" for c in range(C)], "f1", "best", 3)
    ref = LO.scores(want, lags, edges, "f1", "best", 3)
    wb, clear_f = LO.best_labels(ref), LO.best_label_gaps_hold(ref["score"])
    assert sorted(auto) == np.nonzero(wb["label"] >= 0)[0].tolist() and len(auto) >= 10
    assert all(e["label"] == f"ph{wb['label'][f]}" and e["lag"] == wb["lag"][f] for f, e in auto.items() if clear_f[f])
    # flat codes with segments and a window; save / load; a loaded tracker goes on counting; merge of two shards
    flat = LabelAssociation(H, C, torch.from_numpy(edges[64:164]), lags=lags, f_window=(64, 100), device=DEV)
    flat.update((dev(vals), dev(idx)), dev(flat_labels), segments=dev(seg))
    LO.same(state_of(flat), LO.update((vals, idx), seg, flat_labels, H, C, lags, edges[64:164], (64, 100)))
    with pytest.raises(ValueError):
        flat.update((dev(vals).reshape(UTT, T, -1), dev(idx).reshape(UTT, T, -1)), dev(flat_labels).reshape(UTT, T))  # forms mix
    a = collect_label_association(sae, batches[:1], C, prof, n_strata=S, lags=lags)
    b = collect_label_association(sae, batches[1:], C, prof, n_strata=S, lags=lags)
    b.merge(a)
    LO.same(state_of(b), want)
    with tempfile.TemporaryDirectory(prefix="wsae_labels_") as d:
        assoc.save(f"{d}/a.pt")
        back = LabelAssociation.load(f"{d}/a.pt", device=DEV)
    LO.same(state_of(back), want)
    assert torch.equal(back.edges.view(torch.int32), assoc.edges.view(torch.int32)) and back._submitted == UTT * T
    x0, l0, m0 = batches[1]
    c0 = sae.encode_compact(x0.to(DEV))
    back.update((c0[0].reshape(1, T, -1), c0[1].reshape(1, T, -1)), l0.to(DEV), frame_mask=m0.to(DEV))
    again = (c0[0].reshape(T, -1).cpu().numpy(), c0[1].reshape(T, -1).cpu().numpy())
    seg0 = np.where(m0.reshape(-1).numpy() != 0, 0, -1)
    LO.same(state_of(back), LO.update(again, seg0, l0.reshape(-1).numpy(), H, C, lags, edges, state=want))
    # errors that need the device
    with pytest.raises(N.WsaeError):
        assoc.update((torch.from_numpy(vals), torch.from_numpy(idx)), torch.from_numpy(flat_labels), segments=torch.from_numpy(seg))
    with pytest.raises(ValueError):
        assoc.update((dev(vals).reshape(UTT, T, -1), dev(idx).reshape(UTT, T, -1)), dev(flat_labels)[:7])
    with pytest.raises(ValueError):
        assoc.update((dev(vals).reshape(UTT, T, -1), dev(idx).reshape(UTT, T, -1)), dev(flat_labels).reshape(UTT, T).float())
    with pytest.raises(ValueError):  # [T, n_utt] labels have the right number of elements and the wrong shape
        assoc.update((dev(vals).reshape(UTT, T, -1), dev(idx).reshape(UTT, T, -1)), dev(flat_labels).reshape(T, UTT))
    with pytest.raises(TypeError):
        collect_label_association(ReLUSAE(D, H).to(DEV), batches, C)


def test_selection_on_inputs_with_distinct_scores():
    """Every top list and every best label, through the Python layer on the kernel's state, on the inputs whose compared
    scores the CPU tests show to differ by more than 1e-9 (``selection_case``)."""
    code, seg, labels, edges = LO.selection_case()
    S, lags, n, min_count = LO.SELECTION
    want = LO.update(code, seg, labels, LO.SEL_HIDDEN, LO.SEL_CLASSES, lags, edges)
    assoc = LabelAssociation(LO.SEL_HIDDEN, LO.SEL_CLASSES, torch.from_numpy(edges), lags=lags, device=DEV)
    assoc.update((dev(code[0]), dev(code[1])), dev(labels), segments=dev(seg))
    LO.same(state_of(assoc), want)
    for metric in LO.METRICS:
        for lag in (0, "best"):
            ref = LO.scores(want, lags, edges, metric, lag, min_count)
            got = assoc.scores(metric, lag, min_count)
            np.testing.assert_allclose(got.score.cpu().numpy(), ref["score"], rtol=1e-12, atol=1e-12, equal_nan=True)
            assert np.array_equal(got.threshold_index.cpu().numpy(), ref["threshold_index"]), (metric, lag)
            assert np.array_equal(got.lag.cpu().numpy(), ref["lag"]), (metric, lag)
            feats, top = top_label_features(assoc, n=n, metric=metric, lag=lag, min_count=min_count)
            wf, wv = LO.top_label_features(ref["score"], n)
            assert np.array_equal(feats.cpu().numpy(), wf), (metric, lag)
            np.testing.assert_allclose(top.cpu().numpy(), wv, rtol=1e-12, atol=1e-12)
            bl, wb = best_labels(assoc, metric, lag, min_count), LO.best_labels(ref)
            for name in ("label", "threshold_index", "lag", "tp", "fires", "positives"):
                assert np.array_equal(getattr(bl, name).cpu().numpy(), wb[name]), (metric, lag, name)


# ---- 9: why the strata and the lags exist -------------------------------------------------------------------------------------
def test_planted_detector():
    code, labels, edges, f = LO.planted_case()
    assoc = LabelAssociation(16, 5, torch.from_numpy(edges), lags=(-1, 3), device=DEV)
    assoc.update((dev(code[0])[None], dev(code[1])[None]), dev(labels.astype(np.int64))[None])
    LO.same(state_of(assoc), LO.update(code, None, labels, 16, 5, (-1, 3), edges))
    bl = best_labels(assoc, "f1", "best")
    assert int(bl.label[f]) == 3 and int(bl.lag[f]) == 2 and int(bl.threshold_index[f]) > 0 and float(bl.score[f]) == 1.0
    assert float(bl.threshold[f]) == 1.0 and int(bl.tp[f]) == int(bl.fires[f]) == int(bl.positives[f]) > 20
    at_zero = assoc.scores("f1", 0).score[f, 3]
    active_only = LabelAssociation(16, 5, None, lags=(2, 2), device=DEV)
    active_only.update((dev(code[0])[None], dev(code[1])[None]), dev(labels.astype(np.int64))[None])
    assert float(at_zero) < 0.9 and float(active_only.scores("f1", 2).score[f, 3]) < 0.9  # no lag, or no threshold: no detector
