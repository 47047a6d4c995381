"""Label association without a GPU: the numpy oracle of tests/label_oracle.py against hand-worked rows (one per reason a
pair is dropped, the stratum rule at an edge, at equal edges and at NaN edges) and against a triple Python loop, the AUROC
formula against brute-force counting of frame pairs, F1 / phi / MI against hand-computed 2 x 2 tables, the conditions that
keep the GPU test inputs from being degenerate, every argument error of ``wsae_label_update`` (raised before any HIP
call), the workspace query, the header / ``SIGNATURES`` / exports, the Python layer's errors and its float64 readers on the
oracle's integer state."""

from __future__ import annotations

import math
import re
from pathlib import Path

import numpy as np
import pytest

import label_oracle as LO
import profile_oracle as PO

HEADER = Path(__file__).resolve().parents[1] / "include" / "wsae.h"
NAMES = ("wsae_label_workspace_bytes", "wsae_label_update")


def code_of(rows, k=2):
    """rows: per row a list of (index, value) -> (vals, idx) padded with (0, 0.0) entries."""
    vals, idx = np.zeros((len(rows), k), np.float32), np.zeros((len(rows), k), np.int32)
    for r, entries in enumerate(rows):
        for e, (i, v) in enumerate(entries):
            idx[r, e], vals[r, e] = i, v
    return vals, idx


# ---- the oracle against hand-worked cases -----------------------------------------------------------------------------------
def test_pair_rule_one_row_per_drop_reason():
    # feature 1 fires on every row; lag +1; C = 3
    code = code_of([[(1, 1.0)]] * 8)
    #         r:  0   1   2   3   4   5   6   7
    seg = [0, 0, -1, 0, 1, 1, 1, 1]
    labels = [2, 1, 0, 0, 1, -1, 3, 2]
    # (0,1): label 1, kept.  (1,1): neighbour 2 is padding, i.e. another segment id (-1 != 0).  (2,1): row 2 is padding.
    # (3,1): neighbour 4 is in segment 1.  (4,1): label -1.  (5,1): label 3 >= C.  (6,1): label 2, kept.  (7,1): 8 is outside.
    st = LO.update(code, seg, labels, 4, 3, (1, 1))
    assert st["pair_rows"].tolist() == [[0, 1, 1]]
    assert st["cnt"][1, 0].reshape(-1).tolist() == [0, 1, 1] and st["cnt"].sum() == 2
    assert LO.pair_classes(seg, labels, 8, 3, 1).tolist() == [1, -1, -1, -1, -1, -1, 2, -1]
    # lag -1 from row 0 is outside the call too; lag 0 on a padding row; without seg one segment and nothing is padding
    assert LO.pair_classes(seg, labels, 8, 3, -1).tolist() == [-1, 2, -1, -1, -1, 1, -1, -1]
    assert LO.pair_classes(seg, labels, 8, 3, 0).tolist() == [2, 1, -1, 0, 1, -1, -1, 2]
    assert LO.pair_classes(None, labels, 8, 3, 1).tolist() == [1, 0, 0, 1, -1, -1, 2, -1]
    # pair_rows counts a pair whatever the features do: no feature fires here
    quiet = LO.update(code_of([[(1, -1.0)]] * 8), seg, labels, 4, 3, (0, 1))
    assert quiet["pair_rows"].tolist() == [[1, 2, 2], [0, 1, 1]] and quiet["cnt"].sum() == 0
    # a feature outside the window counts nothing in cnt, the pairs stay
    win = LO.update(code, seg, labels, 4, 3, (1, 1), window=(2, 2))
    assert win["cnt"].shape == (2, 1, 3, 1) and win["cnt"].sum() == 0 and win["pair_rows"].tolist() == [[0, 1, 1]]


def test_stratum_rule_at_an_edge_at_equal_edges_and_at_nan_edges():
    nan = np.nan
    edges = np.array([[0.5, 1.0, 2.0],      # feature 0
                      [1.0, 1.0, 1.0],      # feature 1: equal edges - strata 1 and 2 stay empty
                      [nan, nan, nan]], np.float32)  # feature 2: never fired in the profile - all it does is stratum 0
    rows = [[(0, 0.25), (1, 0.99)], [(0, 0.5), (1, 1.0)], [(0, 1.5), (2, 7.0)], [(0, 2.0), (2, np.inf)],
            [(0, np.nextafter(np.float32(0.5), np.float32(0))), (1, 5.0)]]
    st = LO.update(code_of(rows), None, [0] * 5, 3, 1, (0, 0), edges)
    assert st["cnt"][0, 0, 0].tolist() == [2, 1, 1, 1]   # 0.25 and just below 0.5 | 0.5 (an edge counts: <=) | 1.5 | 2.0
    assert st["cnt"][1, 0, 0].tolist() == [1, 0, 0, 2]
    assert st["cnt"][2, 0, 0].tolist() == [2, 0, 0, 0]
    # the activity rule is the profile's: the first ACTIVE entry of a repeated index gives the value; NaN is not active
    st = LO.update(code_of([[(0, -3.0), (0, 1.0)], [(0, nan), (0, 0.25)], [(0, 2.5), (0, 0.25)]]), None, [0] * 3, 3, 1, (0, 0), edges)
    assert st["cnt"][0, 0, 0].tolist() == [1, 0, 1, 1]


def test_vectorised_oracle_equals_the_triple_loop():
    rng = np.random.default_rng(5)
    rows, k, hidden, C = 90, 4, 12, 4
    vals = rng.uniform(-0.3, 2.0, (rows, k)).astype(np.float32)
    idx = rng.integers(-1, hidden + 1, (rows, k)).astype(np.int32)
    seg = (np.arange(rows) // 13).astype(np.int32)
    seg[rng.random(rows) < 0.15] = -1
    labels = rng.integers(-1, C + 1, rows).astype(np.int32)
    edges = np.sort(rng.uniform(0, 2, (hidden, 3)).astype(np.float32), axis=1)
    edges[3] = np.nan
    for lags in ((0, 0), (-3, 2), (2, 4), (-15, 0)):
        for s, e, w in ((seg, edges, None), (None, None, None), (seg, edges[2:9], (2, 7))):
            LO.same(LO.update((vals, idx), s, labels, hidden, C, lags, e, w), LO.update_loop((vals, idx), s, labels, hidden, C, lags, e, w))
    # two calls over whole utterances, in either order, and the merge of two shards equal one call
    cut = 52  # rows 52 .. begin segment 4
    assert seg[cut - 1] != seg[cut] or seg[cut] < 0
    whole = LO.update((vals, idx), seg, labels, hidden, C, (-3, 2), edges)
    a = LO.update((vals[:cut], idx[:cut]), seg[:cut], labels[:cut], hidden, C, (-3, 2), edges)
    b = LO.update((vals[cut:], idx[cut:]), seg[cut:], labels[cut:], hidden, C, (-3, 2), edges)
    ab = LO.update((vals[cut:], idx[cut:]), seg[cut:], labels[cut:], hidden, C, (-3, 2), edges, state=a)
    for st in (ab, LO.merge(a, b), LO.merge(b, a)):
        LO.same(st, whole)


def test_auroc_formula_against_counting_frame_pairs():
    code, seg, labels = LO.general_case()
    for S, lags in ((4, (-2, 3)), (1, (0, 0)), (16, (5, 6))):
        edges = LO.general_edges(S)
        st = LO.update(code, seg, labels, LO.HIDDEN, LO.CLASSES, lags, edges)
        for li in (0, lags[1] - lags[0]):
            table = LO.auroc_table(st["cnt"][:, li], st["pair_rows"][li])
            busy = np.argsort(-st["cnt"][:, li].sum((1, 2)), kind="stable")[:4]
            for f in list(busy) + [LO.NAN_EDGES, LO.TIED, 0]:
                for c in (0, 3, LO.CLASSES - 1):
                    want = LO.auroc_brute(code, seg, labels, LO.HIDDEN, LO.CLASSES, lags[0] + li, edges, f, c)
                    assert abs(table[f, c] - want) <= 1e-12, (S, lags, f, c, table[f, c], want)
    # hand-worked: levels inactive, s0, s1; class 0 on levels (inactive, s1, s1), class 1 on (inactive, s0, s1)
    cnt = np.zeros((1, 2, 2), np.int32)
    cnt[0, 0] = [0, 2]
    cnt[0, 1] = [1, 1]
    pairs = np.array([3, 3])
    # positives of class 0 at levels [-1, 1, 1], negatives at [-1, 0, 1]: wins = (0.5) + (2 + 0.5) + (2 + 0.5) = 5.5 of 9
    assert LO.auroc_table(cnt, pairs)[0, 0] == 5.5 / 9 and LO.auroc_table(cnt, pairs)[0, 1] == 3.5 / 9
    assert np.isnan(LO.auroc_table(cnt, np.array([3, 0]))).all()  # no negatives, or no positives


def test_f1_phi_and_mi_against_hand_computed_tables():
    # one feature, two classes, two strata: class 0 on (s0: 1, s1: 6), class 1 on (s0: 3, s1: 2); P = (10, 10)
    cnt = np.array([[[1, 6], [3, 2]]], np.int32)
    pairs = np.array([10, 10])
    # t = 0: TP = 7, A = 12, P = 10, N = 20: FP = 5, FN = 3, TN = 5.  t = 1: TP = 6, A = 8: FP = 2, FN = 4, TN = 8.
    tp, a, p, n = LO.threshold_counts(cnt, pairs)
    assert tp[0].tolist() == [[7, 6], [5, 2]] and a[0, 0].tolist() == [12, 8] and n == 20
    assert np.array_equal(LO.metric_table(cnt, pairs, "precision")[0, 0], [7 / 12, 6 / 8])
    assert np.array_equal(LO.metric_table(cnt, pairs, "recall")[0, 0], [7 / 10, 6 / 10])
    assert np.array_equal(LO.metric_table(cnt, pairs, "f1")[0, 0], [14 / 22, 12 / 18])
    assert np.array_equal(LO.metric_table(cnt, pairs, "jaccard")[0, 0], [7 / 15, 6 / 12])
    phi = LO.metric_table(cnt, pairs, "phi")[0, 0]
    assert abs(phi[0] - (7 * 5 - 5 * 3) / math.sqrt(12 * 8 * 10 * 10)) < 1e-15
    assert abs(phi[1] - (6 * 8 - 2 * 4) / math.sqrt(8 * 12 * 10 * 10)) < 1e-15

    def mi_of(tp, fp, fn, tn):
        tot = tp + fp + fn + tn
        out = 0.0
        for x, row, col in ((tp, tp + fp, tp + fn), (fp, tp + fp, fp + tn), (fn, fn + tn, tp + fn), (tn, fn + tn, fp + tn)):
            if x:
                out += x / tot * math.log2(x * tot / (row * col))
        return out

    mi = LO.metric_table(cnt, pairs, "mi")[0, 0]
    assert abs(mi[0] - mi_of(7, 5, 3, 5)) < 1e-15 and abs(mi[1] - mi_of(6, 2, 4, 8)) < 1e-15
    # a perfect detector: 1 bit at P = N / 2, phi 1, f1 1; an empty cell contributes 0 (0 log 0 = 0)
    perfect = np.array([[[0, 10], [0, 0]]], np.int32)
    assert LO.metric_table(perfect, pairs, "mi")[0, 0, 1] == 1.0 and LO.metric_table(perfect, pairs, "phi")[0, 0, 1] == 1.0
    assert LO.metric_table(perfect, pairs, "f1")[0, 0, 1] == 1.0
    # denominators of 0 give NaN: a feature that never fires has no precision and no phi, but recall 0
    silent = np.zeros((1, 2, 2), np.int32)
    assert np.isnan(LO.metric_table(silent, pairs, "precision")).all() and np.isnan(LO.metric_table(silent, pairs, "phi")).all()
    assert (LO.metric_table(silent, pairs, "recall") == 0).all() and (LO.metric_table(silent, pairs, "mi") == 0).all()
    # the selection: the best threshold, ties to the lower one; min_count hides cells with few true positives
    st = {"cnt": cnt[:, None], "pair_rows": pairs[None]}
    edges = np.array([[1.5]], np.float32)
    sc = LO.scores(st, (0, 0), edges, "f1")
    assert sc["threshold_index"].tolist() == [[1, 0]] and sc["score"][0, 0] == 12 / 18 and sc["threshold"].tolist() == [[1.5, 0.0]]
    assert sc["tp"].tolist() == [[6, 5]] and sc["fires"].tolist() == [[8, 12]] and sc["positives"].tolist() == [[10, 10]]
    assert np.isnan(LO.scores(st, (0, 0), edges, "f1", min_count=7)["score"][0, 1])
    assert LO.scores(st, (0, 0), edges, "f1", min_count=7)["threshold_index"].tolist() == [[0, 0]]
    tie = {"cnt": np.array([[[[0, 4]]], [[[2, 2]]]], np.int32), "pair_rows": np.array([[4]])}  # recall 1 at both thresholds / t = 0
    assert LO.scores(tie, (0, 0), np.array([[1.0], [1.0]], np.float32), "recall")["threshold_index"].tolist() == [[0], [0]]
    # lags: equal scores at lags -1, 1 and 2 -> the nearer to 0, then the lower
    lagged = {"cnt": np.array([[[[3]], [[1]], [[3]], [[3]]]], np.int32), "pair_rows": np.array([[4], [4], [4], [4]])}
    assert LO.scores(lagged, (-1, 2), None, "recall", lag="best")["lag"].tolist() == [[-1]]
    assert LO.scores(lagged, (-1, 2), None, "recall", lag=0)["score"].tolist() == [[0.25]]
    assert LO.lag_order((-2, 3), "best") == [2, 1, 3, 0, 4, 5]
    # two lags tie at different thresholds: the lower threshold wins before the lag nearer 0 is asked.  One feature, two
    # classes, two strata, lags 0 and 1, precision of class 0:
    #   lag 0: class 0 on (s0: 0, s1: 2), class 1 on (s0: 1, s1: 0) -> t = 0: 2 / 3, t = 1: 2 / 2 = 1
    #   lag 1: class 0 on (s0: 1, s1: 1), class 1 on nothing         -> t = 0: 2 / 2 = 1, t = 1: 1 / 1 = 1
    # the best score 1 is reached at (t = 1, lag 0), (t = 0, lag 1) and (t = 1, lag 1): the rule picks t = 0, hence lag 1,
    # with tp = 2, fires = 2 and positives = pair_rows[lag 1][class 0] = 2.  Class 1 has true positives at (t = 0, lag 0)
    # only: 1 / 3.
    cross = {"cnt": np.array([[[[0, 2], [1, 0]], [[1, 1], [0, 0]]]], np.int32), "pair_rows": np.array([[3, 1], [2, 1]])}
    cross_edges = np.array([[1.5]], np.float32)
    for sc in (LO.scores(cross, (0, 1), cross_edges, "precision", "best"), _module_scores(cross, (0, 1), cross_edges, "precision", "best")):
        assert sc["score"].tolist() == [[1.0, 1 / 3]] and sc["threshold_index"].tolist() == [[0, 0]] and sc["lag"].tolist() == [[1, 0]]
        assert sc["tp"].tolist() == [[2, 1]] and sc["fires"].tolist() == [[2, 3]] and sc["positives"].tolist() == [[2, 1]]
        assert sc["threshold"].tolist() == [[0.0, 0.0]]
    # ... and with the lags the other way round (-1 and 0, the same tables): lag 0 now holds the t = 0 maximum
    for sc in (LO.scores(cross, (-1, 0), cross_edges, "precision", "best"), _module_scores(cross, (-1, 0), cross_edges, "precision", "best")):
        assert sc["threshold_index"].tolist() == [[0, 0]] and sc["lag"].tolist() == [[0, -1]]
    # at one lag alone the threshold is that lag's own
    for sc in (LO.scores(cross, (0, 1), cross_edges, "precision", 0), _module_scores(cross, (0, 1), cross_edges, "precision", 0)):
        assert sc["score"].tolist() == [[1.0, 1 / 3]] and sc["threshold_index"].tolist() == [[1, 0]] and sc["threshold"].tolist() == [[1.5, 0.0]]


def _module_scores(st, lags, edges, metric, lag, min_count=1):
    """``LabelAssociation.scores`` on hand-made integer state (CPU tensors: the readers need no kernel), as a dict."""
    import torch

    from whisper_sae.analysis import LabelAssociation
    F, _, C, _ = st["cnt"].shape
    a = LabelAssociation(F, C, None if edges is None else torch.from_numpy(edges), lags=lags)
    a._state = {"cnt": torch.from_numpy(st["cnt"]), "pair_rows": torch.from_numpy(st["pair_rows"].astype(np.int64))}
    return {k: v.numpy() for k, v in a.scores(metric, lag, min_count)._asdict().items()}


# ---- the GPU test inputs are not degenerate -----------------------------------------------------------------------------------
def test_conditions_on_the_gpu_test_inputs():
    code, seg, labels = LO.general_case()
    vals, idx = code
    assert vals.shape == (LO.ROWS, LO.K) and LO.ROWS % 64 and LO.ROWS * LO.K > 256
    lo, cols = LO.WINDOW
    # every drop reason occurs, for some lag of the tested sets
    n = LO.ROWS
    live = seg >= 0
    assert (~live).any()                                                               # padding rows
    for lag in (-2, 3, 5):
        q = np.arange(n) + lag
        inside = (q >= 0) & (q < n)
        qc = np.clip(q, 0, n - 1)
        assert (live & ~inside).any()                                                  # the neighbour is outside the call
        assert (live & inside & (seg[qc] >= 0) & (seg[qc] != seg)).any()               # ... in another utterance
        assert (live & inside & (seg[qc] < 0)).any()                                   # ... padding
        assert (live & inside & (seg[qc] == seg) & (labels[qc] < 0)).any()             # label < 0
        assert (live & inside & (seg[qc] == seg) & (labels[qc] >= LO.CLASSES)).any()   # label >= C
    assert (np.bincount(seg[live]) == 1).any()                                         # a one-row utterance
    # the spoiled code: values <= 0, NaN, +inf, indices outside, a repeat whose first ACTIVE entry is not its first entry
    assert np.isnan(vals).any() and np.isinf(vals).any() and (vals < 0).any() and (vals == 0).any()
    assert ((idx < 0) | (idx >= LO.HIDDEN)).any()
    late = [(r, e) for r in np.nonzero(live)[0] for e in range(1, LO.K)
            if vals[r, e] > 0 and lo <= idx[r, e] < lo + cols and (idx[r, :e] == idx[r, e]).any()
            and not ((idx[r, :e] == idx[r, e]) & (vals[r, :e] > 0)).any()]
    assert len(late) >= 2
    r_act, f_act, v_act, _ = PO.first_active(code, seg, LO.HIDDEN)
    assert ((f_act < lo) & (f_act >= lo - 2)).any() and ((f_act >= lo + cols) & (f_act < lo + cols + 2)).any()  # next to the window
    for S in LO.STRATA:
        edges = LO.general_edges(S)
        for lags in LO.LAGS:
            st = LO.update(code, seg, labels, LO.HIDDEN, LO.CLASSES, lags, edges)
            assert (st["pair_rows"] > 0).all() and (st["cnt"].sum((0, 3)) > 0).all()   # every class at every lag
            assert (st["cnt"].sum((0, 1, 2)) > 0).all()                                # every stratum index
            assert st["cnt"][LO.NAN_EDGES].sum() > 0 and st["cnt"][LO.NAN_EDGES][:, :, 1:].sum() == 0  # NaN edges: stratum 0
            assert st["cnt"][:lo].sum() > 0 and st["cnt"][lo + cols:].sum() > 0        # firing features outside the window
            win = LO.update(code, seg, labels, LO.HIDDEN, LO.CLASSES, lags, LO.general_edges(S, LO.WINDOW), LO.WINDOW)
            assert np.array_equal(win["cnt"], st["cnt"][lo:lo + cols]) and np.array_equal(win["pair_rows"], st["pair_rows"])
            if S > 2:
                assert st["cnt"][LO.TIED].sum() > 0 and st["cnt"][LO.TIED][:, :, 1:S - 1].sum() == 0  # equal edges: empty strata
        if S > 1:
            on_edge = (f_act == 25) & (v_act == edges[25, 0])
            assert on_edge.any() and PO.stratum_of(edges[f_act[on_edge]], v_act[on_edge]).min() >= 1  # a value equal to an edge
    for k in (1, 31, 32, 33, 128):
        wcode, wseg, wlab = LO.wide_case(k)
        wide = LO.update(wcode, wseg, wlab, 300, 5, (-1, 1), None)
        assert wide["cnt"].sum() > 0 and (wide["pair_rows"].sum(1) > 0).all() and (wseg < 0).any()
    selection_inputs_are_unambiguous()


def selection_inputs_are_unambiguous():
    """For the checks of the top lists and of the best labels (``selection_case`` and ``SELECTION`` of
    tests/label_oracle.py): per class the oracle's n-th and (n + 1)-th scores differ by more than 1e-9 - and so do all
    neighbours above them - so the expected index lists are unambiguous; likewise every feature's best and second-best
    class."""
    code, seg, labels, edges = LO.selection_case()
    S, lags, n, min_count = LO.SELECTION
    assert edges.shape == (LO.SEL_HIDDEN, S - 1)
    st = LO.update(code, seg, labels, LO.SEL_HIDDEN, LO.SEL_CLASSES, lags, edges)
    for metric in LO.METRICS:
        for lag in (0, "best"):
            score = LO.scores(st, lags, edges, metric, lag, min_count)["score"]
            for c in range(LO.SEL_CLASSES):
                col = np.sort(score[:, c][~np.isnan(score[:, c])])[::-1]
                assert col.size > n and col[n - 1] - col[n] > 1e-9, (metric, lag, c)
            assert LO.selection_gaps_hold(score, n).all() and LO.best_label_gaps_hold(score).all(), (metric, lag)
            assert (~np.isnan(score)).any(1).sum() >= 20


# ---- argument errors: made-up (aligned, never dereferenced) pointers, every case fails its checks first -----------------
def _label(N, k=32, hidden=64, n_rows=16, C=8, lag_lo=-1, lag_hi=1, f_lo=0, f_cols=64, edges=4096, S=4, vals=4096, idx=4096,
           seg=4096, labels=4096, cnt=4096, pair_rows=4096, ws=None, ws_bytes=0):
    return N.lib().wsae_label_update(vals, idx, k, hidden, seg, labels, n_rows, C, lag_lo, lag_hi, f_lo, f_cols, edges, S, cnt,
                                     pair_rows, ws, ws_bytes, None)


LABEL_ERRORS = {"k0": dict(k=0), "k129": dict(k=129), "window_past_end": dict(f_lo=40, f_cols=25),
                "window_negative": dict(f_lo=-1), "window_empty": dict(f_cols=0), "n_rows_2p31": dict(n_rows=2 ** 31),
                "n_rows_negative": dict(n_rows=-1), "hidden0": dict(hidden=0), "null_vals": dict(vals=None),
                "null_idx": dict(idx=None), "null_labels": dict(labels=None), "null_cnt": dict(cnt=None),
                "null_pair_rows": dict(pair_rows=None), "classes0": dict(C=0), "classes1025": dict(C=1025),
                "lag_lo_below": dict(lag_lo=-1025, lag_hi=-1020), "lag_hi_above": dict(lag_lo=1020, lag_hi=1025),
                "lags_reversed": dict(lag_lo=2, lag_hi=1), "lags17": dict(lag_lo=-8, lag_hi=8),
                "lags_wrap": dict(lag_lo=-2 ** 31, lag_hi=2 ** 31 - 1), "strata0": dict(S=0), "strata17": dict(S=17),
                "edges_missing": dict(edges=None, S=2), "workspace_negative": dict(ws_bytes=-1)}


@pytest.mark.parametrize("kw", list(LABEL_ERRORS.values()), ids=list(LABEL_ERRORS))
def test_label_argument_errors_do_not_need_a_gpu(kw):
    from whisper_sae import _native as N
    assert _label(N, **kw) == -1
    assert "wsae_label_update" in N.last_error()


def test_empty_calls_and_the_workspace_query():
    from whisper_sae import _native as N
    assert _label(N, n_rows=0) == 0 and _label(N, n_rows=0, seg=None) == 0 and _label(N, n_rows=0, ws=4096, ws_bytes=64) == 0
    assert _label(N, n_rows=0, S=1, edges=None) == 0 and _label(N, n_rows=0, lag_lo=-1024, lag_hi=-1009) == 0
    assert _label(N, n_rows=0, lag_lo=1009, lag_hi=1024, C=1024, S=16, k=128) == 0
    q = N.lib().wsae_label_workspace_bytes
    need = q(3_072_000, 32, 40960, 8192, 4096, 41, -2, 2, 8)
    assert need >= 0 and q(0, 1, 1, 0, 1, 1, 0, 0, 1) >= 0 and q(16, 128, 64, 0, 64, 1024, 1009, 1024, 16) >= 0
    for bad in ((16, 0, 64, 0, 64, 8, 0, 0, 4), (16, 129, 64, 0, 64, 8, 0, 0, 4), (-1, 32, 64, 0, 64, 8, 0, 0, 4),
                (2 ** 31, 32, 64, 0, 64, 8, 0, 0, 4), (16, 32, 64, 60, 5, 8, 0, 0, 4), (16, 32, 0, 0, 64, 8, 0, 0, 4),
                (16, 32, 64, 0, 64, 0, 0, 0, 4), (16, 32, 64, 0, 64, 1025, 0, 0, 4), (16, 32, 64, 0, 64, 8, 1, 0, 4),
                (16, 32, 64, 0, 64, 8, -1025, -1020, 4), (16, 32, 64, 0, 64, 8, 1020, 1025, 4), (16, 32, 64, 0, 64, 8, 0, 16, 4),
                (16, 32, 64, 0, 64, 8, -2 ** 31, 2 ** 31 - 1, 4), (16, 32, 64, 0, 64, 8, 0, 0, 0), (16, 32, 64, 0, 64, 8, 0, 0, 17)):
        assert q(*bad) == -1, bad


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
    defines = {k: int(v) for k, v in re.findall(r"#define (WSAE_LABEL_[A-Z_]+) (\d+)", text)}
    assert defines == {"WSAE_LABEL_MAX_K": N.LABEL_MAX_K, "WSAE_LABEL_MAX_CLASSES": N.LABEL_MAX_CLASSES,
                       "WSAE_LABEL_MAX_LAGS": N.LABEL_MAX_LAGS, "WSAE_LABEL_MAX_STRATA": N.LABEL_MAX_STRATA}
    assert defines == {"WSAE_LABEL_MAX_K": 128, "WSAE_LABEL_MAX_CLASSES": 1024, "WSAE_LABEL_MAX_LAGS": 16,
                       "WSAE_LABEL_MAX_STRATA": 16}
    for name in ("LabelAssociation", "LabelScores", "BestLabels", "top_label_features", "best_labels", "automated_labels",
                 "collect_label_association"):
        assert name in A.__all__ and hasattr(A, name)


# ---- the Python layer ---------------------------------------------------------------------------------------------------------
def test_python_layer_argument_errors():
    import torch

    from whisper_sae import _native as N
    from whisper_sae.analysis import LabelAssociation, collect_label_association
    from whisper_sae.sae.model import ReLUSAE
    code = (torch.ones(2, 3, 2), torch.zeros(2, 3, 2, dtype=torch.int32))
    labels = torch.zeros(2, 3, dtype=torch.int64)
    with pytest.raises(N.WsaeError):
        LabelAssociation(8, 3).update(code, labels)  # CPU tensors
    with pytest.raises(TypeError):
        LabelAssociation(8, 3).update(torch.ones(2, 3, 2), labels)
    with pytest.raises(N.WsaeError):
        LabelAssociation(8, 3, device="cpu").scores()
    for kw in (dict(hidden=0), dict(n_classes=0), dict(n_classes=1025), dict(f_window=(4, 5)), dict(lags=(1, 0)),
               dict(lags=(-1025, -1020)), dict(lags=(1020, 1025)), dict(lags=(0, 16)), dict(edges=torch.zeros(7, 2)),
               dict(edges=torch.zeros(8, 16)), dict(edges=torch.zeros(8)), dict(edges=[0.5])):
        with pytest.raises(ValueError):
            LabelAssociation(**{"hidden": 8, "n_classes": 3, **kw})
    # the state bound: [40960, 5, 41, 8] int32 is 269 MB
    LabelAssociation(40960, 41, torch.zeros(40960, 7), lags=(-2, 2))
    with pytest.raises(ValueError, match="narrow the window, the lags or the strata"):
        LabelAssociation(40960, 41, torch.zeros(40960, 7), lags=(-2, 2), max_state_bytes=2 ** 28)
    with pytest.raises(ValueError, match="narrow the window, the lags or the strata"):
        LabelAssociation(40960, 1024, torch.zeros(40960, 15), lags=(0, 15))
    assert LabelAssociation(40960, 1024, torch.zeros(4096, 7), lags=(0, 7), f_window=(100, 4096), max_state_bytes=2 ** 31).n_lags == 8
    edges = torch.tensor([[0.5, 1.0]] * 8)
    nan_edges = torch.full((8, 2), float("nan"))
    for other in (LabelAssociation(9, 3, torch.tensor([[0.5, 1.0]] * 9)), LabelAssociation(8, 4, edges), LabelAssociation(8, 3),
                  LabelAssociation(8, 3, edges + 1), LabelAssociation(8, 3, edges, lags=(0, 1)), LabelAssociation(8, 3, nan_edges),
                  LabelAssociation(8, 3, edges[:4], f_window=(0, 4))):
        with pytest.raises(ValueError):
            LabelAssociation(8, 3, edges).merge(other)
    a, b = LabelAssociation(8, 3, nan_edges), LabelAssociation(8, 3, nan_edges.clone())
    a._submitted, b._submitted = 10, 20
    a.merge(b)  # NaN edges are equal bit for bit; neither has state: only the bookkeeping moves
    assert a._submitted == 30
    b._submitted = 2 ** 31 - 20
    with pytest.raises(N.WsaeError):
        a.merge(b)
    for bad in (dict(metric="nope"), dict(lag=1), dict(lag="nearest")):
        with pytest.raises(ValueError):
            LabelAssociation(8, 3).scores(**bad)
    with pytest.raises(TypeError):
        collect_label_association(ReLUSAE(16, 32), [(torch.zeros(2, 4, 16), torch.zeros(2, 4, dtype=torch.int64))], 3)


class _OracleBacked:
    """A ``LabelAssociation`` whose state is the oracle's integers on the CPU: the readers need no kernel."""

    def __new__(cls, st, hidden, C, lags, edges, window=None):
        import torch

        from whisper_sae.analysis import LabelAssociation
        a = LabelAssociation(hidden, C, None if edges is None else torch.from_numpy(edges), lags=lags, f_window=window)
        a._state = {k: torch.from_numpy(v) for k, v in st.items()}
        return a


def test_readers_on_the_oracles_integer_state():
    import torch

    from whisper_sae.analysis import BestLabels, LabelScores, automated_labels, best_labels, top_label_features
    from whisper_sae.analysis.labels import auroc_table, metric_table
    code, seg, labels = LO.general_case()
    lags = (-2, 3)
    for S, window in ((4, None), (1, LO.WINDOW), (16, LO.WINDOW)):
        edges = LO.general_edges(S, window)
        st = LO.update(code, seg, labels, LO.HIDDEN, LO.CLASSES, lags, edges, window)
        assoc = _OracleBacked(st, LO.HIDDEN, LO.CLASSES, lags, edges, window)
        cnt, pairs = torch.from_numpy(st["cnt"]), torch.from_numpy(st["pair_rows"])
        for li in (0, 2, 5):
            for metric in LO.METRICS[:-1]:
                np.testing.assert_allclose(metric_table(cnt[:, li], pairs[li], metric).numpy(),
                                           LO.metric_table(st["cnt"][:, li], st["pair_rows"][li], metric), rtol=1e-12, atol=1e-12,
                                           equal_nan=True, err_msg=metric)
            np.testing.assert_allclose(auroc_table(cnt[:, li], pairs[li]).numpy(), LO.auroc_table(st["cnt"][:, li], st["pair_rows"][li]),
                                       rtol=1e-12, atol=1e-12, equal_nan=True)
        for metric in LO.METRICS:
            for lag in (0, -2, "best"):
                for min_count in (1, 3):
                    got, want = assoc.scores(metric, lag, min_count), LO.scores(st, lags, edges, metric, lag, min_count)
                    assert isinstance(got, LabelScores)
                    np.testing.assert_allclose(got.score.numpy(), want["score"], rtol=1e-12, atol=1e-12, equal_nan=True)
                    for name in ("threshold_index", "lag", "tp", "fires", "positives"):
                        g = getattr(got, name)
                        assert g.dtype == torch.int64 and np.array_equal(g.numpy(), want[name]), (metric, lag, name)
                    assert got.threshold.dtype == torch.float32 and np.array_equal(got.threshold.numpy(), want["threshold"], equal_nan=True)
                    assert got.score.dtype == torch.float64 and got.score.shape == (assoc.f_cols, LO.CLASSES)
    # the top lists, the best labels and the dict of labels, on the inputs whose scores are shown to differ
    code, seg, labels, edges = LO.selection_case()
    S, lags, n, min_count = LO.SELECTION
    window = (8, 32)
    for win, e in ((None, edges), (window, edges[8:40])):
        st = LO.update(code, seg, labels, LO.SEL_HIDDEN, LO.SEL_CLASSES, lags, e, win)
        assoc = _OracleBacked(st, LO.SEL_HIDDEN, LO.SEL_CLASSES, lags, e, win)
        for metric in LO.METRICS:
            for lag in (0, "best"):
                want = LO.scores(st, lags, e, metric, lag, min_count)
                if win is not None:  # (the gaps were asserted for the whole width; a window has a subset of the scores)
                    assert LO.selection_gaps_hold(want["score"], n).all() and LO.best_label_gaps_hold(want["score"]).all()
                feats, vals = top_label_features(assoc, n=n, metric=metric, lag=lag, min_count=min_count)
                wf, wv = LO.top_label_features(want["score"], n, assoc.f_lo)
                assert np.array_equal(feats.numpy(), wf) and np.allclose(vals.numpy(), wv, rtol=1e-12, atol=1e-12, equal_nan=True)
                bl, wb = best_labels(assoc, metric, lag, min_count), LO.best_labels(want)
                assert isinstance(bl, BestLabels)
                for name in ("label", "threshold_index", "lag", "tp", "fires", "positives"):
                    assert np.array_equal(getattr(bl, name).numpy(), wb[name]), (metric, name)
        names = [f"c{c}" for c in range(LO.SEL_CLASSES)]
        auto = automated_labels(assoc, names, "f1", "best", min_count)
        bl = LO.best_labels(LO.scores(st, lags, e, "f1", "best", min_count))
        assert sorted(auto) == [assoc.f_lo + int(c) for c in np.nonzero(bl["label"] >= 0)[0]] and len(auto) > 10
        for f, entry in auto.items():
            c = f - assoc.f_lo
            assert set(entry) == {"label", "metric", "score", "threshold", "lag", "precision", "recall"}
            assert entry["label"] == names[bl["label"][c]] and entry["metric"] == "f1" and entry["lag"] == bl["lag"][c]
            assert entry["precision"] == bl["tp"][c] / bl["fires"][c] and entry["recall"] == bl["tp"][c] / bl["positives"][c]
            assert abs(entry["score"] - 2 / (1 / entry["precision"] + 1 / entry["recall"])) < 1e-12
        assert len(automated_labels(assoc, names, "f1", "best", min_count, min_score=0.3)) < len(auto)
        with pytest.raises(ValueError):
            automated_labels(assoc, names[:-1])
    # fewer candidates than n: the lists end in -1 / NaN
    few = _OracleBacked(LO.update(code_of([[(1, 1.0)], [(2, 1.0)]], 1), None, [0, 1], 4, 2, (0, 0)), 4, 2, (0, 0), None)
    feats, vals = top_label_features(few, n=3, metric="f1")
    assert feats.tolist() == [[1, -1, -1], [2, -1, -1]] and vals[:, 0].tolist() == [1.0, 1.0] and bool(torch.isnan(vals[:, 1:]).all())
    assert best_labels(few, "f1", 0).label.tolist() == [-1, 0, 1, -1]


def test_planted_detector_in_the_oracle():
    code, labels, edges, f = LO.planted_case()
    st = LO.update(code, None, labels, 16, 5, (-1, 3), edges)
    sc = LO.scores(st, (-1, 3), edges, "f1", "best")
    bl = LO.best_labels(sc)
    assert bl["label"][f] == 3 and bl["lag"][f] == 2 and bl["threshold_index"][f] == 1 and bl["score"][f] == 1.0
    assert LO.metric_table(st["cnt"][:, 3], st["pair_rows"][3], "f1")[f, 3, 0] < 0.9
    assert LO.scores(st, (-1, 3), edges, "f1", 0)["score"][f, 3] < 0.9
