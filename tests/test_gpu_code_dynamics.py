"""Code dynamics on the MI355X: ``wsae_dyn_update`` and ``wsae_boundary_score`` bit for bit against the sequential numpy
oracle of tests/dynamics_oracle.py - the ``uint32`` view of every similarity that is not NaN, the NaN masks, every
integer of the state and of the counts - the properties that make the results independent of the other lags of a call,
of the grouping of whole utterances into calls and of the ``sim`` output, and the Python layer on real modules.  The
inputs and the conditions that keep them from being degenerate are checked on the CPU in tests/test_code_dynamics.py."""

from __future__ import annotations

import ctypes as C
import tempfile

import numpy as np
import pytest
import torch

import dynamics_oracle as DO
from whisper_sae import _native as N
from whisper_sae.analysis import (BoundaryCurve, BoundaryScorer, CodeDynamics, DynamicsSummary, boundaries_from_labels,
                                  boundary_curve, collect_code_dynamics, detect_boundaries, frame_similarity, novelty)
from whisper_sae.sae.model import BatchTopKSAE, ReLUSAE, TopKSAE

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
JUNK = 0x5a5a5a5
JUNK_F = 123.25
TAIL = 3  # junk rows behind every output


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class DynState:
    """Device state of ``wsae_dyn_update`` with three junk rows of lags behind every array, which must survive; the
    workspace holds 0xAB on entry and keeps it behind the size the query names."""

    def __init__(self, n_lags):
        self.L = n_lags
        self.t = {"pairs": torch.zeros(n_lags + TAIL, 3, dtype=torch.int64, device=DEV),
                  "sim_q": torch.zeros(n_lags + TAIL, 3, dtype=torch.int64, device=DEV),
                  "sq_q": torch.zeros(n_lags + TAIL, 3, dtype=torch.int64, device=DEV),
                  "hist": torch.zeros(n_lags + TAIL, 3, DO.BINS, dtype=torch.int64, device=DEV),
                  "total_rows": torch.zeros(1 + TAIL, dtype=torch.int64, device=DEV)}
        for name, t in self.t.items():
            t[(1 if name == "total_rows" else n_lags):] = JUNK

    def arrays(self):
        out = {}
        for name, t in self.t.items():
            n = 1 if name == "total_rows" else self.L
            assert bool((t[n:] == JUNK).all()), name
            out[name] = t[:n].cpu().numpy()
        return out


def dyn_call(code, hidden, lags, metric, seg=None, weight=None, label=None, state=None, want_sim=True, rows=None, expect=0):
    """One call -> ``sim [rows, n_lags]`` as numpy (None without ``want_sim``); ``state``: a ``DynState`` to add to."""
    v, i = dev(code[0]), dev(code[1])
    s = None if seg is None else dev(np.asarray(seg, np.int32))
    w = None if weight is None else dev(np.asarray(weight, np.float32))
    lab = None if label is None else dev(np.asarray(label, np.int32))
    n_rows, k, L = (v.shape[0] if rows is None else rows), v.shape[1], len(lags)
    lib = N.lib()
    need = lib.wsae_dyn_workspace_bytes(n_rows, k, hidden, L)
    assert need >= 0
    ws = torch.full((need + 64,), 0xAB, dtype=torch.uint8, device=DEV)
    sim = torch.full((v.shape[0] + TAIL, L), JUNK_F, dtype=torch.float32, device=DEV) if want_sim else None
    st = state.t if state is not None else {}
    rc = lib.wsae_dyn_update(v.data_ptr(), i.data_ptr(), k, hidden, N.ptr(s), N.ptr(w), N.ptr(lab), n_rows, (C.c_int32 * L)(*lags), L,
                             metric, N.ptr(sim), N.ptr(st.get("pairs")), N.ptr(st.get("sim_q")), N.ptr(st.get("sq_q")),
                             N.ptr(st.get("hist")), N.ptr(st.get("total_rows")), ws.data_ptr(), need,
                             torch.cuda.current_stream().cuda_stream)
    assert rc == expect, N.last_error()
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xAB).all())
    if sim is None:
        return None
    assert bool((sim[n_rows:] == JUNK_F).all())
    return sim[:n_rows].cpu().numpy()


def case_of(n):
    return DO.planted_case() if n == "planted" else DO.similarity_case(n)


CASES = list(range(len(DO.SHAPES))) + ["planted"]
# (metric, weighted, labelled): all three metrics, with and without weights and labels
COMBOS = ((DO.COSINE, False, False), (DO.COSINE, True, True), (DO.JACCARD, True, False), (DO.JACCARD, False, True),
          (DO.DOT, False, False), (DO.DOT, True, False))


# ---- 1: every case, lag set and metric ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", CASES, ids=[str(c) if isinstance(c, str) else "x".join(map(str, DO.SHAPES[c])) for c in CASES])
def test_similarity_and_state_equal_the_oracle(n):
    case = case_of(n)
    for lags in DO.LAG_SETS:
        for metric, weighted, labelled in COMBOS:
            what = (n, lags, metric, weighted, labelled)
            weight = case["weight"] if weighted else None
            label = case["label"] if labelled else None
            want_sim, want_st = DO.case_update(n, lags, metric, weighted, labelled)
            st = DynState(len(lags)) if metric != DO.DOT else None
            got = dyn_call(case["code"], case["hidden"], lags, metric, case["seg"], weight, label, st)
            DO.same_bits(got, want_sim, what)
            if st is not None:
                DO.same_state(st.arrays(), want_st, what)
            if lags[-1] == 1024:  # longer than every segment
                assert np.isnan(got[:, -1]).all() and (st is None or st.arrays()["pairs"][-1].sum() == 0)


def test_without_segments_the_call_is_one_utterance():
    case = DO.similarity_case(1)
    lags = (1, 2, 3, 5, 8)
    for metric in (DO.COSINE, DO.JACCARD):
        want_sim, want_st = DO.update(case["code"], case["hidden"], lags, metric, None, case["weight"], case["label"])
        st = DynState(len(lags))
        DO.same_bits(dyn_call(case["code"], case["hidden"], lags, metric, None, case["weight"], case["label"], st), want_sim)
        DO.same_state(st.arrays(), want_st)
        assert want_st["total_rows"][0] == 257 and not np.isnan(want_sim[:-8]).any()


# ---- 2: the properties --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 4, "planted"])
def test_a_lag_alone_or_among_others(n):
    case = case_of(n)
    lags = (1, 2, 3, 5, 8)
    for metric in (DO.COSINE, DO.JACCARD):
        st_all = DynState(len(lags))
        sim_all = dyn_call(case["code"], case["hidden"], lags, metric, case["seg"], case["weight"], case["label"], st_all)
        all_arrays = st_all.arrays()
        for li, lag in enumerate(lags):
            st = DynState(1)
            sim = dyn_call(case["code"], case["hidden"], (lag,), metric, case["seg"], case["weight"], case["label"], st)
            DO.same_bits(sim[:, 0], sim_all[:, li], (n, lag))
            alone = st.arrays()
            for name in ("pairs", "sim_q", "sq_q", "hist"):
                assert np.array_equal(alone[name][0], all_arrays[name][li]), (n, lag, name)
            assert alone["total_rows"][0] == all_arrays["total_rows"][0]


def utterance_cuts(seg, at):
    """Rows near ``at`` where an utterance ends: the last live row before and the row itself lie in different utterances."""
    out = []
    for a in at:
        r = a
        while True:
            before = seg[:r][seg[:r] >= 0]
            if seg[r] >= 0 and before.size and before[-1] != seg[r]:
                break
            r += 1
        out.append(r)
    return out


@pytest.mark.parametrize("n", [2, "planted"])
def test_state_does_not_depend_on_batching_call_order_or_the_sim_output(n):
    case = case_of(n)
    rows = case["seg"].size
    lags = (1, 2, 3, 5, 8)
    want_sim, want = DO.case_update(n, lags, DO.COSINE, True, True)
    c1, c2 = utterance_cuts(case["seg"], (rows // 3, 2 * rows // 3))
    cuts = [(0, c1), (c1, c2), (c2, rows)]
    assert c1 < c2 < rows
    for order in (cuts, cuts[::-1], [cuts[1], cuts[0], cuts[2]]):
        st = DynState(len(lags))
        for a, b in order:
            sim = dyn_call((case["code"][0][a:b], case["code"][1][a:b]), case["hidden"], lags, DO.COSINE, case["seg"][a:b],
                           case["weight"], case["label"][a:b], st)
            DO.same_bits(sim, want_sim[a:b], (n, a, b))
        DO.same_state(st.arrays(), want, (n, order))
    st = DynState(len(lags))
    assert dyn_call(case["code"], case["hidden"], lags, DO.COSINE, case["seg"], case["weight"], case["label"], st, want_sim=False) is None
    DO.same_state(st.arrays(), want, "sim == NULL")


def test_no_rows_and_rejected_calls_touch_nothing():
    case = DO.similarity_case(1)
    lags = (1, 2)
    st = DynState(2)
    dyn_call(case["code"], case["hidden"], lags, DO.COSINE, case["seg"], None, case["label"], st)
    before = st.arrays()
    dyn_call(case["code"], case["hidden"], lags, DO.COSINE, case["seg"], None, case["label"], st, rows=0)
    dyn_call(case["code"], case["hidden"], lags, DO.DOT, case["seg"], None, case["label"], st, expect=-1)  # DOT with a state
    assert "WSAE_DYN_DOT" in N.last_error()
    DO.same_state(st.arrays(), before)


def test_pairs_count_exactly_under_contention():
    """Every pair of 20000 identical rows lands in one cell of the state: the LDS sums and the flush lose nothing."""
    rows = 20_000
    code = (np.ones((rows, 2), np.float32), np.tile(np.array([[3, 5]], np.int32), (rows, 1)))
    st = DynState(2)
    sim = dyn_call(code, 16, (1, 7), DO.COSINE, None, None, np.zeros(rows, np.int32), st)
    got = st.arrays()
    assert got["pairs"].tolist() == [[rows - 1, 0, 0], [rows - 7, 0, 0]] and got["total_rows"][0] == rows
    assert got["sim_q"][:, 0].tolist() == [(rows - 1) << 30, (rows - 7) << 30] and got["hist"][0, 0, 63] == rows - 1
    assert got["sq_q"][:, 0].tolist() == [(rows - 1) << 30, (rows - 7) << 30]
    assert (sim[:-1, 0] == 1.0).all() and np.isnan(sim[-1, 0]) and np.isnan(sim[-7:, 1]).all()


# ---- 3: boundaries ------------------------------------------------------------------------------------------------------------
class Counts:
    """Device counts of ``wsae_boundary_score`` with junk behind every array."""

    def __init__(self, n_thr):
        self.n = n_thr
        self.t = {"n_pred": torch.zeros(n_thr + TAIL, dtype=torch.int64, device=DEV),
                  "n_hit": torch.zeros(n_thr + TAIL, dtype=torch.int64, device=DEV),
                  "n_ref": torch.zeros(1 + TAIL, dtype=torch.int64, device=DEV),
                  "n_peaks": torch.zeros(1 + TAIL, dtype=torch.int64, device=DEV)}
        for name, t in self.t.items():
            t[(n_thr if name in ("n_pred", "n_hit") else 1):] = JUNK

    def arrays(self):
        out = {}
        for name, t in self.t.items():
            n = self.n if name in ("n_pred", "n_hit") else 1
            assert bool((t[n:] == JUNK).all()), name
            out[name] = t[:n].cpu().numpy()
        return out


def score_call(nov, thr, tol, seg=None, ref=None, counts=None, want_peaks=True, rows=None):
    """One call -> ``(the Counts, peaks uint8 [rows] as numpy or None)``."""
    x, t = dev(np.asarray(nov, np.float32)), dev(np.asarray(thr, np.float32))
    s = None if seg is None else dev(np.asarray(seg, np.int32))
    r = None if ref is None else dev(np.asarray(ref, np.uint8))
    n_rows = x.shape[0] if rows is None else rows
    counts = Counts(t.shape[0]) if counts is None else counts
    lib = N.lib()
    need = lib.wsae_boundary_workspace_bytes(n_rows, t.shape[0], tol)
    assert need >= 0
    ws = torch.full((need + 64,), 0xAB, dtype=torch.uint8, device=DEV)
    peaks = torch.full((x.shape[0] + TAIL,), 0x5a, dtype=torch.uint8, device=DEV) if want_peaks else None
    c = counts.t
    N.check(lib.wsae_boundary_score(x.data_ptr(), N.ptr(s), N.ptr(r), n_rows, t.data_ptr(), t.shape[0], tol, c["n_pred"].data_ptr(),
                                    c["n_hit"].data_ptr(), c["n_ref"].data_ptr(), c["n_peaks"].data_ptr(), N.ptr(peaks),
                                    ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream), "wsae_boundary_score")
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xAB).all())
    if peaks is None:
        return counts, None
    assert bool((peaks[n_rows:] == 0x5a).all())
    return counts, peaks[:n_rows].cpu().numpy()


def thresholds(n_thr):
    """``n_thr`` thresholds over [0, 1] in a shuffled order, with equal values and both infinities where there is room."""
    rng = np.random.default_rng(n_thr)
    thr = rng.permutation(np.linspace(0.0, 1.0, n_thr)).astype(np.float32)
    if n_thr >= 8:
        thr[1], thr[5] = thr[0], thr[4]
        thr[2], thr[n_thr - 1] = -np.inf, np.inf
    return thr


@pytest.mark.parametrize("n_thr", [1, 64, 65, 256])
@pytest.mark.parametrize("tol", [0, 1, 3])
def test_planted_boundaries_equal_the_oracle(tol, n_thr):
    case, nov = DO.planted_case(), DO.planted_novelty()
    thr = thresholds(n_thr) if n_thr > 1 else np.array([0.7], np.float32)
    want, want_peaks = DO.boundary_score(nov, thr, tol, case["seg"], case["ref"])
    counts, peaks = score_call(nov, thr, tol, case["seg"], case["ref"])
    got = counts.arrays()
    DO.same_counts(got, want, (tol, n_thr))
    assert np.array_equal(peaks, want_peaks) and want["n_hit"].max() > 100
    if n_thr >= 8:
        assert got["n_pred"][2] == got["n_peaks"][0] > 0 and got["n_pred"][n_thr - 1] == 0 == got["n_hit"][n_thr - 1]
        assert got["n_pred"][1] == got["n_pred"][0] and got["n_hit"][5] == got["n_hit"][4]


def test_boundaries_without_references_without_segments_and_with_a_large_tolerance():
    case, nov = DO.planted_case(), DO.planted_novelty()
    thr = thresholds(64)
    for seg, ref, tol in ((case["seg"], None, 1), (None, case["ref"], 1), (None, None, 0), (case["seg"], case["ref"], 64),
                          (None, case["ref"], 37)):
        want, want_peaks = DO.boundary_score(nov, thr, tol, seg, ref)
        counts, peaks = score_call(nov, thr, tol, seg, ref)
        DO.same_counts(counts.arrays(), want, (seg is None, ref is None, tol))
        assert np.array_equal(peaks, want_peaks)
        assert (want["n_ref"][0] == 0) == (ref is None) and (want["n_hit"].sum() == 0) == (ref is None)
    # the peaks output is optional
    counts, peaks = score_call(nov, thr, 1, case["seg"], case["ref"], want_peaks=False)
    DO.same_counts(counts.arrays(), DO.boundary_score(nov, thr, 1, case["seg"], case["ref"])[0])
    assert peaks is None


def test_dense_references_and_many_short_stretches():
    """References on most rows (the waiting list of the match fills up to the tolerance) and stretches of 1 .. 9 rows, more
    of them than one pass of the walking waves takes."""
    rng = np.random.default_rng(77)
    rows = 24_000
    nov = rng.random(rows).astype(np.float32)
    nov[rng.random(rows) < 0.05] = np.nan
    ref = (rng.random(rows) < 0.6).astype(np.uint8)
    seg = np.cumsum(rng.random(rows) < 0.25).astype(np.int32)
    seg[rng.random(rows) < 0.05] = -1
    thr = np.array([0.2, 0.5, 0.8, -np.inf], np.float32)
    assert len(DO.stretches(rows, seg)) > 2048
    for tol in (0, 2, 64):
        want, want_peaks = DO.boundary_score(nov, thr, tol, seg, ref)
        counts, peaks = score_call(nov, thr, tol, seg, ref)
        DO.same_counts(counts.arrays(), want, tol)
        assert np.array_equal(peaks, want_peaks)
    long_seg = (np.arange(rows) // 9000).astype(np.int32)
    for tol in (1, 5):
        want, _ = DO.boundary_score(nov, thr, tol, long_seg, ref)
        DO.same_counts(score_call(nov, thr, tol, long_seg, ref)[0].arrays(), want, tol)
        assert want["n_hit"][3] > 5000


@pytest.mark.parametrize("n", range(len(DO.HAND_SEQUENCES)))
def test_hand_worked_sequences(n):
    nov, ref, seg, thr, tol, want = DO.hand_sequence(n)
    counts, peaks = score_call(nov, thr, tol, seg, ref)
    got = counts.arrays()
    assert (int(got["n_pred"][0]), int(got["n_hit"][0]), int(got["n_ref"][0]), int(got["n_peaks"][0])) == tuple(want)
    assert np.array_equal(peaks, DO.find_peaks(nov, seg))


def test_two_boundary_calls_add_up_to_one():
    case, nov = DO.planted_case(), DO.planted_novelty()
    thr = thresholds(65)
    rows = nov.size
    cut = utterance_cuts(case["seg"], (rows // 2,))[0]
    want, want_peaks = DO.boundary_score(nov, thr, 1, case["seg"], case["ref"])
    counts = Counts(65)
    _, p1 = score_call(nov[cut:], thr, 1, case["seg"][cut:], case["ref"][cut:], counts)
    _, p0 = score_call(nov[:cut], thr, 1, case["seg"][:cut], case["ref"][:cut], counts)
    DO.same_counts(counts.arrays(), want)
    assert np.array_equal(np.concatenate([p0, p1]), want_peaks)
    score_call(nov, thr, 1, case["seg"], case["ref"], counts, rows=0)  # no rows: nothing moves
    DO.same_counts(counts.arrays(), want)


# ---- 4: the Python layer on real modules --------------------------------------------------------------------------------------
D, H, K, UTT, T = 64, 256, 8, 12, 40


def utterances(seed):
    """12 utterances of 40 frames in three batches with labels and a frame mask.  A frame repeats for a stretch of about
    three frames at a varying loudness, and the label of a frame is its stretch: codes persist inside a label."""
    gen = torch.Generator().manual_seed(seed)
    proto = torch.randn(UTT, 14, D, generator=gen)
    hold = (torch.rand(UTT, T, generator=gen) < 0.3).cumsum(1) % 14
    x = torch.gather(proto, 1, hold[:, :, None].expand(UTT, T, D)) * torch.exp(0.3 * torch.randn(UTT, T, 1, generator=gen))
    x = x + 0.3 * torch.randn(UTT, T, D, generator=gen)
    mask = torch.ones(UTT, T)
    for u in range(UTT):
        mask[u, 24 + (u % 5) * 3:] = 0
    mask[3, 10] = 0
    labels = hold.clone()
    labels[torch.rand(UTT, T, generator=gen) < 0.1] = -1
    return [(x[:5], labels[:5], mask[:5]), (x[5:6], labels[5:6], mask[5:6]), (x[6:], labels[6:], mask[6:])], mask, labels


def make_sae(cls, seed, **kw):
    torch.manual_seed(seed)
    return cls(D, H, k=K, **kw).to(DEV)


def state_of(dyn):
    return {name: getattr(dyn, name).cpu().numpy() for name in DO.STATE_FIELDS}


@pytest.mark.parametrize("kind", ["topk", "batch_topk"])
def test_python_layer_on_real_modules(kind):
    sae = make_sae(TopKSAE, 1) if kind == "topk" else make_sae(BatchTopKSAE, 2, max_k_per_row=16)
    batches, mask, labels = utterances(5)
    lags = (1, 2, 3, 5)
    sae.train()
    dyn = collect_code_dynamics(sae, batches, lags)
    assert sae.training and dyn.hidden == H and dyn.lags == lags
    sae.eval()
    codes = [sae.encode_compact(x.to(DEV)) for x, _, _ in batches]
    vals, idx = (np.concatenate([c[i].reshape(-1, c[i].shape[-1]).cpu().numpy() for c in codes]) for i in (0, 1))
    k = vals.shape[1]
    seg = np.where(mask.reshape(-1).numpy() != 0, np.repeat(np.arange(UTT), T), -1).astype(np.int32)
    flat_labels = labels.reshape(-1).numpy().astype(np.int32)
    want_sim, want = DO.update((vals, idx), H, lags, DO.COSINE, seg, None, flat_labels)
    assert (want["pairs"][0] > 20).all() and want["total_rows"][0] == int(mask.sum())
    DO.same_state(state_of(dyn), want)
    # the summary: float64 from the integers
    s = dyn.summary()
    assert isinstance(s, DynamicsSummary) and s.total_rows == int(mask.sum())
    for g, classes in (("all", (0, 1, 2)), ("within", (0,)), ("across", (1,))):
        for li in range(len(lags)):
            ref = DO.group_stats(want, li, classes)
            got = getattr(s, g)
            assert int(got.pairs[li]) == ref[0]
            np.testing.assert_allclose([float(t[li]) for t in got[1:]], ref[1:], rtol=1e-13, equal_nan=True)
        np.testing.assert_allclose(s.timescale(g), DO.timescale(lags, getattr(s, g).mean.tolist()), rtol=1e-13)
    assert float(s.within.mean[0]) > float(s.across.mean[0])
    # frame_similarity: numbered and flat forms agree with the oracle and with each other, the mask is respected
    v3, i3 = dev(vals).reshape(UTT, T, k), dev(idx).reshape(UTT, T, k)
    numbered = frame_similarity((v3, i3), lags, frame_mask=mask.to(DEV), hidden=H)
    assert numbered.shape == (UTT, T, len(lags))
    DO.same_bits(numbered.reshape(-1, len(lags)).cpu().numpy(), want_sim)
    flat = frame_similarity((dev(vals), dev(idx)), lags, segments=dev(seg), hidden=H)
    DO.same_bits(flat.cpu().numpy(), want_sim)
    assert bool(torch.isnan(numbered[3, 10]).all()) and bool(torch.isnan(numbered[3, 9, 0])) and not bool(torch.isnan(numbered[3, 9, 1]))
    for metric, code in (("dot", DO.DOT), ("jaccard", DO.JACCARD)):
        got = frame_similarity((v3, i3), (1, 4), metric, frame_mask=mask.to(DEV))
        DO.same_bits(got.reshape(-1, 2).cpu().numpy(), DO.update((vals, idx), 2 ** 31 - 1, (1, 4), code, seg)[0], metric)
    w = torch.rand(H, generator=torch.Generator().manual_seed(3))
    w[::7] = 0
    got = frame_similarity((dev(vals), dev(idx)), (1,), weights=w.to(DEV), segments=dev(seg))
    DO.same_bits(got.cpu().numpy(), DO.update((vals, idx), H, (1,), DO.COSINE, seg, w.numpy())[0], "weights")
    one = frame_similarity((dev(vals[:T]), dev(idx[:T])), (1,))  # a flat code without segments: one utterance
    DO.same_bits(one.cpu().numpy(), DO.update((vals[:T], idx[:T]), 2 ** 31 - 1, (1,), DO.COSINE)[0])
    # update: the flat form, the returned similarity, forms do not mix
    flat_dyn = CodeDynamics(lags, hidden=H, device=DEV)
    back_sim = flat_dyn.update((dev(vals), dev(idx)), dev(flat_labels), segments=dev(seg), return_similarity=True)
    DO.same_bits(back_sim.cpu().numpy(), want_sim)
    DO.same_state(state_of(flat_dyn), want)
    with pytest.raises(ValueError):
        flat_dyn.update((v3, i3), dev(flat_labels).reshape(UTT, T))
    with pytest.raises(ValueError):
        dyn.update((v3, i3), dev(flat_labels)[:7])
    with pytest.raises(N.WsaeError):
        dyn.update((torch.from_numpy(vals).reshape(UTT, T, k), torch.from_numpy(idx).reshape(UTT, T, k)))
    # items without labels and without a mask; merge of two shards; save / load; a loaded tracker goes on counting
    plain = collect_code_dynamics(sae, [x for x, _, _ in batches], lags, metric="jaccard")
    DO.same_state(state_of(plain), DO.update((vals, idx), H, lags, DO.JACCARD, np.repeat(np.arange(UTT), T).astype(np.int32))[1])
    masked = collect_code_dynamics(sae, [(x, m) for x, _, m in batches], lags)
    DO.same_state(state_of(masked), DO.update((vals, idx), H, lags, DO.COSINE, seg)[1])
    a, b = collect_code_dynamics(sae, batches[:1], lags), collect_code_dynamics(sae, batches[1:], lags)
    b.merge(a)
    DO.same_state(state_of(b), want)
    with tempfile.TemporaryDirectory(prefix="wsae_dynamics_") as d:
        dyn.save(f"{d}/a.pt")
        back = CodeDynamics.load(f"{d}/a.pt", device=DEV)
    DO.same_state(state_of(back), want)
    assert back.lags == lags and back.hidden == H and back.metric == "cosine" and back._submitted == UTT * T
    x0, l0, m0 = batches[1]
    c0 = sae.encode_compact(x0.to(DEV))
    back.update((c0[0].reshape(1, T, -1), c0[1].reshape(1, T, -1)), l0.to(DEV), frame_mask=m0.to(DEV))
    again = (c0[0].reshape(T, -1).cpu().numpy(), c0[1].reshape(T, -1).cpu().numpy())
    seg0 = np.where(m0.reshape(-1).numpy() != 0, 0, -1).astype(np.int32)
    DO.same_state(state_of(back), DO.update(again, H, lags, DO.COSINE, seg0, None, l0.reshape(-1).numpy(), state=want)[1])
    with pytest.raises(TypeError):
        collect_code_dynamics(ReLUSAE(D, H).to(DEV), [x for x, _, _ in batches], lags)
    # boundaries on the module's own code: the curve equals the oracle's, whichever way the dataset is cut
    nov = novelty(numbered)
    ref = boundaries_from_labels(labels.to(DEV), frame_mask=mask.to(DEV))
    assert np.array_equal(ref.reshape(-1).cpu().numpy(), DO.reference_flags(flat_labels, seg))
    thr = np.linspace(0, 1, 33).astype(np.float32)
    curve = boundary_curve(nov, ref, thr, tolerance=1, frame_mask=mask.to(DEV))
    counts, peaks = DO.boundary_score(1 - want_sim[:, 0], thr, 1, seg, ref.reshape(-1).cpu().numpy())
    assert isinstance(curve, BoundaryCurve) and curve.n_ref == counts["n_ref"][0] > 20 and curve.n_peaks == counts["n_peaks"][0]
    assert np.array_equal(curve.n_pred.numpy(), counts["n_pred"]) and np.array_equal(curve.n_hit.numpy(), counts["n_hit"])
    scorer = BoundaryScorer(thr, 1, device=DEV)
    scorer.update(nov[:5], ref[:5], frame_mask=mask[:5].to(DEV))
    scorer.update(nov[5:].reshape(-1), ref[5:].reshape(-1), segments=dev(seg[5 * T:]))
    pieces = scorer.curve()
    assert torch.equal(pieces.n_pred, curve.n_pred) and torch.equal(pieces.n_hit, curve.n_hit) and pieces.n_ref == curve.n_ref
    found = detect_boundaries(nov, 0.5, frame_mask=mask.to(DEV))
    assert found.dtype == torch.bool and found.shape == nov.shape
    assert np.array_equal(found.reshape(-1).cpu().numpy(), (peaks != 0) & (1 - want_sim[:, 0] >= 0.5))


def test_best_threshold_of_the_planted_case():
    case = DO.planted_case()
    vals, idx = dev(case["code"][0]), dev(case["code"][1])
    seg = dev(case["seg"])
    sim = frame_similarity((vals, idx), (1,), segments=seg, hidden=case["hidden"])
    nov = novelty(sim)
    assert np.array_equal(nov.cpu().numpy().view(np.uint32), DO.planted_novelty().view(np.uint32))
    ref = boundaries_from_labels(dev(case["label"]), segments=seg)
    thr = DO.planted_thresholds()
    for tol in (0, 1):
        curve = boundary_curve(nov, ref, thr, tolerance=tol, segments=seg)
        counts, _ = DO.boundary_score(DO.planted_novelty(), thr, tol, case["seg"], ref.cpu().numpy())
        want = DO.curve(counts)
        for by in ("f1", "r_value"):
            best = curve.best(by)
            i = DO.best_index(want[by])
            assert best["index"] == i and best["threshold"] == float(thr[i]) and best[by] == pytest.approx(want[by][i], rel=1e-13)
        assert curve.best()["f1"] >= 0.9  # (the references of boundaries_from_labels miss the few unlabelled frames)
        np.testing.assert_allclose(curve.r_value.numpy(), want["r_value"], rtol=1e-13, equal_nan=True)
