"""Code dynamics without a GPU: the oracle of tests/dynamics_oracle.py on hand-worked rows and
sequences, the conditions that keep the inputs of tests/test_gpu_code_dynamics.py from being degenerate, the summary and
curve formulas on hand-made integer states, host argument errors, the workspace queries, and the agreement of the header,
``_native.SIGNATURES`` and the exports."""

from __future__ import annotations

import math
import re
from pathlib import Path

import numpy as np
import pytest

import dynamics_oracle as DO

HEADER = Path(__file__).resolve().parents[1] / "include" / "wsae.h"
NAMES = ("wsae_dyn_workspace_bytes", "wsae_dyn_update", "wsae_boundary_workspace_bytes", "wsae_boundary_score")
NAN = np.nan


# ---- 1: the similarity rules on hand-worked rows ------------------------------------------------------------------------------
def hand_rows():
    """hidden = 8, k = 4.  Rows: 0 plain; 1 a duplicate index (the first active entry wins, also over a larger later one);
    2 v <= 0 and a NaN value; 3 indices -1 and hidden; 4 empty; 5 = row 0 again; 6 disjoint from row 0; 7 a duplicate whose
    first entry is not active (v <= 0), so the second one counts."""
    vals = np.array([[1.0, 2.0, 2.0, 4.0],
                     [3.0, 5.0, 1.0, 1.0],
                     [-1.0, NAN, 0.0, 2.0],
                     [1.0, 1.0, 3.0, 1.0],
                     [0.0, -2.0, NAN, 0.0],
                     [1.0, 2.0, 2.0, 4.0],
                     [1.0, 1.0, 1.0, 1.0],
                     [-3.0, 2.0, 1.0, 1.0]], np.float32)
    idx = np.array([[0, 1, 2, 3],
                    [1, 1, 2, 6],
                    [0, 1, 2, 3],
                    [-1, 8, 2, 3],
                    [0, 1, 2, 3],
                    [0, 1, 2, 3],
                    [4, 5, 6, 7],
                    [1, 1, 2, 3]], np.int32)
    return vals, idx


def test_canonical_rows_by_hand():
    canon = DO.canonical(hand_rows(), 8)
    assert canon[0] == ([(0, 1.0), (1, 2.0), (2, 2.0), (3, 4.0)], 25.0, 4)
    assert canon[1] == ([(1, 3.0), (2, 1.0), (6, 1.0)], 11.0, 3)  # the duplicate of 1 counts once, with 3 and not 5
    assert canon[2] == ([(3, 2.0)], 4.0, 1)
    assert canon[3] == ([(2, 3.0), (3, 1.0)], 10.0, 2)
    assert canon[4] == ([], 0.0, 0)
    assert canon[7] == ([(1, 2.0), (2, 1.0), (3, 1.0)], 6.0, 3)  # the first entry of 1 is not active: the second is the first active
    # weights: 0, NaN and negative remove a feature; the value is one float32 product
    w = np.array([1.0, 0.5, 0.0, NAN, 1.0, -1.0, 3.0, 1.0], np.float32)
    cw = DO.canonical(hand_rows(), 8, weight=w)
    assert cw[0] == ([(0, 1.0), (1, 1.0)], 2.0, 2)
    assert cw[1] == ([(1, 1.5), (6, 3.0)], 11.25, 2)
    assert cw[6] == ([(4, 1.0), (6, 3.0), (7, 1.0)], 11.0, 3)
    third = np.float32(1.0) / np.float32(3.0)
    one = DO.canonical((np.array([[3.0]], np.float32), np.array([[0]], np.int32)), 1, weight=np.array([third], np.float32))
    assert one[0][0] == [(0, float(np.float32(np.float32(3.0) * third)))]
    # padding: nothing is active
    assert DO.canonical(hand_rows(), 8, seg=np.array([0, -1, 0, 0, 0, 0, 0, 0]))[1] == ([], 0.0, 0)


def test_similarity_by_hand():
    code = hand_rows()
    lags = (1, 5)
    cos, st = DO.update(code, 8, lags, DO.COSINE)
    dot, st_dot = DO.update(code, 8, lags, DO.DOT)
    jac, _ = DO.update(code, 8, lags, DO.JACCARD)
    f32 = np.float32
    # (0, 1): common 1, 2 -> s = 2 * 3 + 2 * 1 = 8
    assert dot[0, 0] == 8.0 and cos[0, 0] == f32(8 / math.sqrt(25 * 11)) and jac[0, 0] == f32(2 / 5)
    # (0, 5): identical rows
    assert dot[0, 1] == 25.0 and cos[0, 1] == 1.0 and jac[0, 1] == 1.0
    # (1, 6): common 6; (1, 2): disjoint -> exact zeros; (3, 4) and (4, 5): an empty row
    assert dot[1, 1] == 1.0 and jac[1, 1] == f32(1 / 6)
    assert dot[1, 0] == 0.0 and cos[1, 0] == 0.0 and jac[1, 0] == 0.0
    assert cos[3, 0] == 0.0 and jac[3, 0] == 0.0 and cos[4, 0] == 0.0 and jac[4, 0] == 0.0
    # (5, 6): disjoint; (2, 7): common 3 -> 2 * 1
    assert cos[5, 0] == 0.0 and dot[2, 1] == 2.0 and cos[2, 1] == f32(2 / math.sqrt(4 * 6))
    # beyond the end: NaN
    assert np.isnan(cos[7, 0]) and np.isnan(cos[3:, 1]).all() and not np.isnan(cos[:3, 1]).any()
    # the state: no labels -> class 2; DOT keeps none
    assert st["pairs"].tolist() == [[0, 0, 7], [0, 0, 3]] and st["total_rows"][0] == 8 and st_dot["pairs"].sum() == 0
    x = [round(float(c) * 2 ** 30) for c in cos[:7, 0]]
    assert st["sim_q"][0, 2] == sum(x) and st["sq_q"][0, 2] == sum((v >> 15) ** 2 for v in x)
    assert st["hist"][0, 2, 63] == 0 and st["hist"][1, 2, 63] == 1 and st["hist"][0, 2, 0] == 5  # 1.0 lands in the last bin
    # both rows empty: Jaccard 0 / 0 is 0
    empty = (np.zeros((2, 2), np.float32), np.zeros((2, 2), np.int32))
    assert DO.update(empty, 4, (1,), DO.JACCARD)[0][0, 0] == 0.0 and DO.update(empty, 4, (1,), DO.COSINE)[0][0, 0] == 0.0
    # segments, padding, labels: (0, 1) within, (1, 2) across, (2, 3) unlabelled, (3, 4) crosses, 5 is padding, (4, 6) spans it
    seg = np.array([0, 0, 0, 0, 1, -1, 1, 1], np.int32)
    label = np.array([2, 2, 3, -1, 1, 1, 1, 1], np.int32)
    sim, st = DO.update(code, 8, (1, 2), DO.COSINE, seg=seg, label=label)
    assert np.isnan(sim[:, 0]).tolist() == [False, False, False, True, True, True, False, True]
    assert np.isnan(sim[:, 1]).tolist() == [False, False, True, True, False, True, True, True]
    assert st["pairs"].tolist() == [[2, 1, 1], [1, 1, 1]] and st["total_rows"][0] == 7
    # the cosine never exceeds 1: rounding can push s / sqrt(n n) past it
    v = np.array([[0.1, 0.7, 0.3]], np.float32)
    twice = (np.repeat(v, 2, 0), np.tile(np.arange(3, dtype=np.int32), (2, 1)))
    assert DO.update(twice, 3, (1,), DO.COSINE)[0][0, 0] == 1.0


# ---- 2: the match on hand-worked sequences ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", range(len(DO.HAND_SEQUENCES)))
def test_match_by_hand(n):
    nov, ref, seg, thr, tol, want = DO.hand_sequence(n)
    st, peaks = DO.boundary_score(nov, thr, tol, seg, ref)
    assert (int(st["n_pred"][0]), int(st["n_hit"][0]), int(st["n_ref"][0]), int(st["n_peaks"][0])) == tuple(want)
    assert int(peaks.sum()) == want[3]


def test_match_and_peak_rules():
    assert DO.match([10], [9, 11], 1) == 1 and DO.match([11], [10, 11], 1) == 1 and DO.match([10], [9, 11], 0) == 0
    assert DO.match([], [1, 2], 3) == 0 and DO.match([1, 2], [], 3) == 0 and DO.match([1, 5, 9], [2, 4, 10], 1) == 3
    assert DO.match([1, 2, 3], [3], 1) == 1  # 1 is too early and is dropped, 2 takes the reference, 3 finds none
    plateau = np.array([0, .8, .8, .8, 0], np.float32)
    assert DO.find_peaks(plateau).tolist() == [0, 1, 0, 0, 0]
    assert DO.find_peaks(np.array([.3], np.float32)).tolist() == [1]  # a stretch of length 1
    assert DO.find_peaks(np.array([-np.inf, NAN, -np.inf], np.float32)).tolist() == [0, 0, 0]
    assert DO.find_peaks(np.array([.3, .2, .5, .5], np.float32), np.array([0, 0, 1, -1])).tolist() == [1, 0, 1, 0]
    # thresholds: -inf keeps every peak, +inf none, NaN none
    nov = np.array([.1, .9, .1, .5, .2], np.float32)
    st, _ = DO.boundary_score(nov, np.array([-np.inf, np.inf, NAN, .5, .6], np.float32), 0, None, np.array([0, 1, 0, 0, 0]))
    assert st["n_pred"].tolist() == [2, 0, 0, 2, 1] and st["n_hit"].tolist() == [1, 0, 0, 1, 1] and st["n_peaks"][0] == 2
    assert DO.reference_flags(np.array([1, 1, 2, -1, 3, 4, 4, 5]), np.array([0, 0, 0, 0, 0, 1, 1, -1])).tolist() == [0, 1, 0, 0, 0, 0, 0, 0]


# ---- 3: the inputs of the GPU tests are not degenerate ------------------------------------------------------------------------
@pytest.mark.parametrize("n", range(len(DO.SHAPES)))
def test_conditions_on_the_similarity_cases(n):
    rows, k, hidden, n_seg = DO.SHAPES[n]
    case = DO.similarity_case(n)
    assert case["code"][0].shape == (rows, k) and case["hidden"] == hidden
    assert len(set(case["seg"][case["seg"] >= 0].tolist())) == n_seg
    if rows == 1:  # one row has no pair: the whole output is NaN, which is what the case is for
        sim, st = DO.case_update(n, DO.ALL_LAGS, DO.COSINE)
        assert np.isnan(sim).all() and st["pairs"].sum() == 0 and st["total_rows"][0] == 1
        return
    vals, idx = case["code"]
    assert (case["seg"] < 0).any() and np.isnan(vals).any() and (vals <= 0).any() and (idx == -1).any() and (idx == hidden).any()
    assert any(len(set(row.tolist())) < k for row in idx) and (case["weight"] == 0).any() and np.isnan(case["weight"]).any()
    for lags in DO.LAG_SETS:
        for metric in (DO.COSINE, DO.DOT, DO.JACCARD):
            for weighted in (False, True):
                sim, st = DO.case_update(n, lags, metric, weighted, labelled=True)
                v = sim[~np.isnan(sim)]
                assert np.isnan(sim).any() and (v == 0).any(), (lags, metric, weighted)
                inside = (v > 0) & (v < 1) if metric != DO.DOT else v > 0
                assert inside.mean() >= 0.5, (lags, metric, weighted, inside.mean())
                if lags[-1] == 1024:  # longer than every segment: an all-NaN column that counts nothing
                    assert np.isnan(sim[:, -1]).all() and st["pairs"][-1].sum() == 0
                if metric != DO.DOT:
                    assert (st["pairs"][0] > 0).all()  # within, across and unlabelled pairs all occur at the first lag


def test_conditions_on_the_planted_case():
    case = DO.planted_case()
    rows = case["seg"].size
    assert 1100 <= rows <= 1250 and len(set(case["seg"][case["seg"] >= 0].tolist())) == 12 and case["code"][0].shape[1] == 16
    sim, st = DO.case_update("planted", (1, 2, 3, 5, 8), DO.COSINE, labelled=True)
    _, within, *_ = DO.group_stats(st, 0, (0,))
    _, across, *_ = DO.group_stats(st, 0, (1,))
    assert within > 0.4 and across < 0.1 and DO.separation(st, 0) > 3
    v = sim[~np.isnan(sim)]
    assert ((v > 0) & (v < 1)).mean() >= 0.5 and (v == 0).any() and np.isnan(sim).any()
    nov = DO.planted_novelty()
    counts, _ = DO.boundary_score(nov, DO.planted_thresholds(), 0, case["seg"], case["ref"])
    f1 = DO.curve(counts)["f1"]
    assert counts["n_ref"][0] > 100 and counts["n_peaks"][0] > 2 * counts["n_ref"][0]
    assert f1[DO.best_index(f1)] >= 0.95
    assert np.nanmin(f1) < 0.7  # and the threshold matters


# ---- 4: the readers on hand-made integer states -------------------------------------------------------------------------------
def hand_state():
    st = DO.empty_state(3)
    half, quarter = 2 ** 29, 2 ** 28
    # lag 0: within 4 pairs at 0.5, across 4 pairs at 0.25 and 0.0 (two each); lag 1: everything at 0.25; lag 2: at 0.0625
    for li, cls, x, n in ((0, 0, half, 4), (0, 1, quarter, 2), (0, 1, 0, 2), (1, 0, quarter, 4), (1, 1, quarter, 4),
                          (2, 2, 2 ** 26, 8)):
        st["pairs"][li, cls] += n
        st["sim_q"][li, cls] += n * x
        st["sq_q"][li, cls] += n * (x >> 15) ** 2
        st["hist"][li, cls, min(x >> 24, 63)] += n
    st["total_rows"][0] = 9
    return st


def test_summary_formulas_on_a_hand_made_state():
    import torch

    from whisper_sae.analysis.dynamics import hist_quantile, summarize_state
    st = hand_state()
    lags = (1, 2, 4)
    s = summarize_state(lags, {k: torch.from_numpy(v) for k, v in st.items()})
    assert s.total_rows == 9 and s.lags == lags
    assert s.all.pairs.tolist() == [8, 8, 8] and s.within.pairs.tolist() == [4, 4, 0] and s.across.pairs.tolist() == [4, 4, 0]
    assert s.within.mean[0] == 0.5 and s.within.std[0] == 0.0 and s.across.mean[0] == 0.125 and s.across.std[0] == 0.125
    assert s.all.mean.tolist() == [0.3125, 0.25, 0.0625] and math.isnan(s.within.mean[2]) and math.isnan(s.across.std[2])
    # separation: (0.5 - 0.125) / sqrt((0 + 0.125^2) / 2); equal groups: 0 / 0 -> NaN
    assert s.separation[0] == pytest.approx(0.375 / math.sqrt(0.125 ** 2 / 2), rel=1e-15) and math.isnan(s.separation[1])
    # quantiles: lag 0 "all": bins 0 (2), 16 (2), 32 (4); the median is reached in bin 16 at its upper end
    assert s.all.median[0] == pytest.approx(16 / 64 + (4 - 2) / 2 / 64) and s.all.q10[0] == pytest.approx(0.8 / 2 / 64)
    assert s.all.q90[0] == pytest.approx(32 / 64 + (7.2 - 4) / 4 / 64) and math.isnan(s.within.median[2])
    # the time scale: means 0.3125, 0.25, 0.0625 at lags 1, 2, 4; 1/e of 0.3125 is crossed between 2 and 4
    level = 0.3125 / math.e
    assert s.timescale() == pytest.approx(2 + (0.25 - level) / (0.25 - 0.0625) * 2, rel=1e-15)
    assert s.timescale("within") == math.inf and s.timescale() == pytest.approx(DO.timescale(lags, s.all.mean.tolist()))
    with pytest.raises(ValueError):
        s.timescale("nope")
    # against the oracle's formulas, every group and lag
    for g, classes in (("all", (0, 1, 2)), ("within", (0,)), ("across", (1,))):
        for li in range(3):
            want = DO.group_stats(st, li, classes)
            got = getattr(s, g)
            assert int(got.pairs[li]) == want[0]
            np.testing.assert_allclose([float(t[li]) for t in got[1:]], want[1:], rtol=1e-14, atol=0, equal_nan=True)
    for li in range(3):
        np.testing.assert_allclose(float(s.separation[li]), DO.separation(st, li), rtol=1e-14, equal_nan=True)
    h = torch.zeros(2, 64, dtype=torch.int64)
    h[0, 5] = 10
    q = hist_quantile(h, 0.5)
    assert float(q[0]) == pytest.approx(5 / 64 + 0.5 / 64) and math.isnan(float(q[1]))
    assert DO.hist_quantile(h[0].numpy(), 0.5) == pytest.approx(float(q[0]))


def test_curve_formulas_on_hand_made_counts():
    import torch

    from whisper_sae.analysis.dynamics import BoundaryCurve
    thr = torch.tensor([0.9, 0.5, 0.1, 2.0])
    pred, hit = torch.tensor([5, 10, 20, 0]), torch.tensor([5, 8, 10, 0])
    c = BoundaryCurve(thr, pred, hit, 10, 25, 1)
    assert c.precision[:3].tolist() == [1.0, 0.8, 0.5] and math.isnan(c.precision[3])
    assert c.recall.tolist() == [0.5, 0.8, 1.0, 0.0] and c.over_segmentation.tolist() == [-0.5, 0.0, 1.0, -1.0]
    assert c.f1.tolist() == pytest.approx([10 / 15, 0.8, 20 / 30, 0.0])
    # R-value by hand at threshold 0.5: OS = 0, R = 0.8 -> r1 = 0.2, r2 = -0.2 / sqrt(2)
    assert float(c.r_value[1]) == pytest.approx(1 - (0.2 + 0.2 / math.sqrt(2)) / 2, rel=1e-12)
    assert float(c.r_value[2]) == pytest.approx(1 - (1.0 + 1.0 / math.sqrt(2)) / 2, rel=1e-12)
    best = c.best()
    assert best["index"] == 1 and best["threshold"] == 0.5 and best["n_pred"] == 10 and best["n_hit"] == 8
    assert c.best("r_value")["index"] == 1
    with pytest.raises(ValueError):
        c.best("precision")
    want = DO.curve({"n_pred": pred.numpy(), "n_hit": hit.numpy(), "n_ref": np.array([10])})
    for name, w in want.items():
        np.testing.assert_allclose(getattr(c, name).numpy(), w, rtol=1e-14, equal_nan=True, err_msg=name)
    # no references: recall and F1 of nothing
    none = BoundaryCurve(thr, pred, torch.zeros(4, dtype=torch.int64), 0, 25, 1)
    assert torch.isnan(none.recall).all() and torch.isnan(none.r_value).all() and float(none.f1[0]) == 0.0 and math.isnan(none.f1[3])
    with pytest.raises(ValueError):
        none.best("r_value")
    # ties go to the first threshold
    tie = BoundaryCurve(torch.tensor([0.3, 0.2]), torch.tensor([4, 4]), torch.tensor([2, 2]), 4, 9, 0)
    assert tie.best()["index"] == 0


# ---- 5: host argument errors: made-up (aligned, never dereferenced) pointers ---------------------------------------------------
def _dyn(N, k=32, hidden=64, n_rows=16, lags=(1, 2), metric=0, vals=4096, idx=4096, seg=4096, weight=4096, label=4096, sim=4096,
         pairs=4096, sim_q=4096, sq_q=4096, hist=4096, total_rows=4096, ws=4096, ws_bytes=2 ** 40, null_lags=False):
    import ctypes as C
    arr = None if null_lags else (C.c_int32 * max(len(lags), 1))(*lags)
    return N.lib().wsae_dyn_update(vals, idx, k, hidden, seg, weight, label, n_rows, arr, len(lags), metric, sim, pairs, sim_q, sq_q,
                                   hist, total_rows, ws, ws_bytes, None)


DYN_ERRORS = {"k0": dict(k=0), "k129": dict(k=129), "hidden0": dict(hidden=0), "n_rows_2p31": dict(n_rows=2 ** 31),
              "n_rows_negative": dict(n_rows=-1), "null_vals": dict(vals=None), "null_idx": dict(idx=None),
              "null_lags": dict(null_lags=True), "no_lags": dict(lags=()), "lags17": dict(lags=tuple(range(1, 18))),
              "lag0": dict(lags=(0, 1)), "lag1025": dict(lags=(1, 1025)), "lags_descend": dict(lags=(2, 1)),
              "lags_equal": dict(lags=(3, 3)), "metric3": dict(metric=3), "metric_negative": dict(metric=-1),
              "dot_with_state": dict(metric=1), "half_a_state": dict(hist=None), "only_total_rows": dict(
                  pairs=None, sim_q=None, sq_q=None, hist=None),
              "nothing_to_write": dict(sim=None, pairs=None, sim_q=None, sq_q=None, hist=None, total_rows=None),
              "workspace_small": dict(ws_bytes=1000), "workspace_null": dict(ws=None), "workspace_negative": dict(ws_bytes=-1),
              "workspace_unaligned": dict(ws=4100)}


@pytest.mark.parametrize("kw", list(DYN_ERRORS.values()), ids=list(DYN_ERRORS))
def test_dyn_argument_errors_do_not_need_a_gpu(kw):
    from whisper_sae import _native as N
    assert _dyn(N, **kw) == -1
    assert "wsae_dyn_update" in N.last_error()


def _bd(N, n_rows=16, n_thr=8, tol=1, nov=4096, seg=4096, ref=4096, thr=4096, n_pred=4096, n_hit=4096, n_ref=4096, n_peaks=4096,
        peaks=4096, ws=4096, ws_bytes=2 ** 40):
    return N.lib().wsae_boundary_score(nov, seg, ref, n_rows, thr, n_thr, tol, n_pred, n_hit, n_ref, n_peaks, peaks, ws, ws_bytes,
                                       None)


BD_ERRORS = {"null_nov": dict(nov=None), "null_thr": dict(thr=None), "null_n_pred": dict(n_pred=None), "null_n_hit": dict(n_hit=None),
             "null_n_ref": dict(n_ref=None), "null_n_peaks": dict(n_peaks=None), "n_rows_2p31": dict(n_rows=2 ** 31),
             "n_rows_negative": dict(n_rows=-1), "thr0": dict(n_thr=0), "thr257": dict(n_thr=257), "tol_negative": dict(tol=-1),
             "tol65": dict(tol=65), "workspace_small": dict(ws_bytes=100), "workspace_null": dict(ws=None),
             "workspace_negative": dict(ws_bytes=-1), "workspace_unaligned": dict(ws=4100)}


@pytest.mark.parametrize("kw", list(BD_ERRORS.values()), ids=list(BD_ERRORS))
def test_boundary_argument_errors_do_not_need_a_gpu(kw):
    from whisper_sae import _native as N
    assert _bd(N, **kw) == -1
    assert "wsae_boundary_score" in N.last_error()


def test_empty_calls_and_the_workspace_queries():
    from whisper_sae import _native as N
    assert _dyn(N, n_rows=0) == 0 and _dyn(N, n_rows=0, ws=None, ws_bytes=0) == 0 and _dyn(N, n_rows=0, seg=None, label=None) == 0
    assert _dyn(N, n_rows=0, metric=1, pairs=None, sim_q=None, sq_q=None, hist=None, total_rows=None) == 0
    assert _dyn(N, n_rows=0, sim=None, k=128, lags=tuple(range(1009, 1025)), metric=2) == 0
    assert _bd(N, n_rows=0) == 0 and _bd(N, n_rows=0, ws=None, ws_bytes=0) == 0 and _bd(N, n_rows=0, seg=None, ref=None, peaks=None) == 0
    assert _bd(N, n_rows=0, n_thr=256, tol=64) == 0 and _bd(N, n_rows=0, n_thr=1, tol=0) == 0
    q = N.lib().wsae_dyn_workspace_bytes
    assert q(0, 1, 1, 1) == 0 and q(16, 128, 64, 16) > 0
    rows, k = 2048 * 1500, 32
    assert 8 * rows * k + 12 * rows <= q(rows, k, 40960, 8) <= 8 * rows * k + 12 * rows + 4 * 256
    assert q(2 ** 31 - 1, 128, 2 ** 31 - 1, 16) >= 8 * 128 * (2 ** 31 - 1)  # (64-bit sizes)
    for bad in ((16, 0, 64, 1), (16, 129, 64, 1), (-1, 32, 64, 1), (2 ** 31, 32, 64, 1), (16, 32, 0, 1), (16, 32, 64, 0),
                (16, 32, 64, 17)):
        assert q(*bad) == -1, bad
    b = N.lib().wsae_boundary_workspace_bytes
    assert b(0, 1, 0) == 0 and 5 * rows <= b(rows, 64, 1) <= 5 * rows + 3 * 256
    for bad in ((-1, 8, 1), (2 ** 31, 8, 1), (16, 0, 1), (16, 257, 1), (16, 8, -1), (16, 8, 65)):
        assert b(*bad) == -1, bad


# ---- 6: header, SIGNATURES and exports ----------------------------------------------------------------------------------------
def test_header_signatures_and_exports_agree():
    import whisper_sae.analysis as A
    from whisper_sae import _native as N
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    lib = N.lib()
    for name in NAMES:
        proto = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert proto, name
        assert len(proto.group(1).split(",")) == len(N.SIGNATURES[name][1]), name
        assert getattr(lib, name) is not None
    defines = {k: int(v) for k, v in re.findall(r"#define (WSAE_(?:DYN|BOUNDARY)_[A-Z_]+) (\d+)", text)}
    assert defines == {"WSAE_DYN_COSINE": N.DYN_COSINE, "WSAE_DYN_DOT": N.DYN_DOT, "WSAE_DYN_JACCARD": N.DYN_JACCARD,
                       "WSAE_DYN_MAX_K": N.DYN_MAX_K, "WSAE_DYN_MAX_LAGS": N.DYN_MAX_LAGS, "WSAE_DYN_MAX_LAG": N.DYN_MAX_LAG,
                       "WSAE_DYN_BINS": N.DYN_BINS, "WSAE_BOUNDARY_MAX_THR": N.BOUNDARY_MAX_THR,
                       "WSAE_BOUNDARY_MAX_TOL": N.BOUNDARY_MAX_TOL}
    assert (N.DYN_MAX_K, N.DYN_MAX_LAGS, N.DYN_MAX_LAG, N.DYN_BINS, N.BOUNDARY_MAX_THR, N.BOUNDARY_MAX_TOL) == (128, 16, 1024, 64, 256, 64)
    assert (DO.COSINE, DO.DOT, DO.JACCARD, DO.BINS) == (N.DYN_COSINE, N.DYN_DOT, N.DYN_JACCARD, N.DYN_BINS)
    for name in ("frame_similarity", "CodeDynamics", "DynamicsSummary", "novelty", "boundaries_from_labels", "boundary_curve",
                 "BoundaryCurve", "BoundaryScorer", "detect_boundaries", "collect_code_dynamics"):
        assert name in A.__all__ and hasattr(A, name)


# ---- 7: the Python layer ------------------------------------------------------------------------------------------------------
def test_python_layer_argument_errors():
    import torch

    from whisper_sae import _native as N
    from whisper_sae.analysis import (BoundaryScorer, CodeDynamics, boundaries_from_labels, boundary_curve, collect_code_dynamics,
                                      detect_boundaries, frame_similarity, novelty)
    from whisper_sae.sae.model import ReLUSAE
    code = (torch.ones(2, 3, 2), torch.zeros(2, 3, 2, dtype=torch.int32))
    with pytest.raises(N.WsaeError):
        frame_similarity(code)  # CPU tensors
    with pytest.raises(N.WsaeError):
        CodeDynamics((1,)).update(code)
    with pytest.raises(TypeError):
        frame_similarity(torch.ones(2, 3, 2))
    with pytest.raises(TypeError):
        CodeDynamics((1,)).update(torch.ones(2, 3, 2))
    with pytest.raises(N.WsaeError):
        CodeDynamics((1,), device="cpu").summary()
    for kw in (dict(lags=()), dict(lags=tuple(range(1, 18))), dict(lags=(0,)), dict(lags=(1025,)), dict(lags=(2, 1)),
               dict(lags=(2, 2)), dict(metric="dot"), dict(metric="nope"), dict(weights=torch.ones(2, 2)), dict(weights=[1.0]),
               dict(weights=torch.ones(7), hidden=8), dict(hidden=0)):
        with pytest.raises(ValueError):
            CodeDynamics(**{"lags": (1,), **kw})
    assert CodeDynamics((1, 2), weights=torch.ones(9)).hidden == 9 and CodeDynamics((1, 2), hidden=5).hidden == 5
    for other in (CodeDynamics((1, 3)), CodeDynamics((1, 2), "jaccard"), CodeDynamics((1, 2), hidden=8),
                  CodeDynamics((1, 2), weights=torch.ones(4))):
        with pytest.raises(ValueError):
            CodeDynamics((1, 2)).merge(other)
    w = torch.tensor([1.0, float("nan")])
    a, b = CodeDynamics((1, 2), weights=w), CodeDynamics((1, 2), weights=w.clone())
    a._submitted, b._submitted = 10, 20
    a.merge(b)  # NaN weights are equal bit for bit; neither has state: only the bookkeeping moves
    assert a._submitted == 30
    b._submitted = 2 ** 31 - 20
    with pytest.raises(N.WsaeError):
        a.merge(b)
    for kw in (dict(thresholds=[]), dict(thresholds=[0.0] * 257), dict(thresholds=[0.5], tolerance=-1),
               dict(thresholds=[0.5], tolerance=65)):
        with pytest.raises(ValueError):
            BoundaryScorer(**kw)
    with pytest.raises(ValueError):
        BoundaryScorer([0.5]).merge(BoundaryScorer([0.6]))
    with pytest.raises(ValueError):
        BoundaryScorer([0.5]).merge(BoundaryScorer([0.5], tolerance=2))
    with pytest.raises(N.WsaeError):
        boundary_curve(torch.zeros(2, 5), torch.zeros(2, 5), [0.5])  # CPU tensors
    with pytest.raises(N.WsaeError):
        detect_boundaries(torch.zeros(5), 0.5)
    with pytest.raises(TypeError):
        collect_code_dynamics(ReLUSAE(16, 32), [torch.zeros(2, 4, 16)], (1,))
    # the two helpers that are plain tensor code
    sim = torch.tensor([[0.25, 0.5], [float("nan"), 1.0]])
    assert novelty(sim)[0] == 0.75 and torch.isnan(novelty(sim)[1]) and novelty(sim, 1).tolist() == [0.5, 0.0]
    labels = torch.tensor([[1, 1, 2, -1, 3, 4], [5, 6, 6, 6, 7, 7]])
    mask = torch.tensor([[1, 1, 1, 1, 1, 1], [1, 1, 1, 1, 0, 1]])
    assert boundaries_from_labels(labels).tolist() == [[0, 1, 0, 0, 1, 0], [1, 0, 0, 1, 0, 0]]
    assert boundaries_from_labels(labels, frame_mask=mask).tolist() == [[0, 1, 0, 0, 1, 0], [1, 0, 0, 0, 0, 0]]
    flat, seg = torch.tensor([1, 1, 2, -1, 3, 4, 4, 5]), torch.tensor([0, 0, 0, 0, 0, 1, 1, -1])
    assert boundaries_from_labels(flat, segments=seg).tolist() == DO.reference_flags(flat.numpy(), seg.numpy()).tolist()
    for bad in (dict(labels=labels.float()), dict(labels=labels, frame_mask=mask[:1]), dict(labels=labels, segments=seg)):
        with pytest.raises(ValueError):
            boundaries_from_labels(**bad)
