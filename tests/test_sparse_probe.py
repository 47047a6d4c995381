"""Sparse linear probes without a GPU: the numpy oracle of tests/probe_oracle.py against itself (its gradient against
central finite differences, its plan against a dense transposition, its chunked backward against a matrix product, its
float32 mirror against float64), the conditions that keep the shared inputs from being degenerate, and the argument
errors the Python layer raises before it needs a device.  The kernels are compared with this oracle in
tests/test_gpu_sparse_probe.py."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import probe_oracle as PB
from whisper_sae import _native as N
from whisper_sae.analysis import SparseProbe, sparse_probe_curve, utterance_split


@pytest.fixture(scope="module")
def general():
    return PB.general_case()


def fit_problem(features=None, class_weight=False):
    code, seg, labels = PB.fit_case()
    col_of, P = None, PB.FIT_HIDDEN
    if features is not None:
        col_of = np.full(PB.FIT_HIDDEN, -1, np.int32)
        col_of[list(features)] = np.arange(len(features))
        P = len(features)
    ent = PB.entries(code, seg, PB.FIT_HIDDEN, col_of)
    y = PB.row_labels(seg, labels, PB.FIT_ROWS, PB.FIT_C, 0)
    cw = np.array([0.5, 1.0, 2.0], np.float32) if class_weight else None
    return code, ent, y, P, cw


# ---- 1: the oracle's gradient -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("features", [None, PB.FIT_FEATURES], ids=["all", "subset"])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "class_weight"])
def test_gradient_agrees_with_central_differences(features, weighted):
    _, ent, y, P, cw = fit_problem(features, weighted)
    X = PB.dense_design(ent, PB.FIT_ROWS, P)
    rng = np.random.default_rng(1)
    theta = 0.3 * rng.standard_normal(P * PB.FIT_C + PB.FIT_C)
    loss, grad = PB.objective64(X, y, theta, PB.FIT_C, PB.FIT_L2, cw)
    h = 1e-6
    for j in rng.choice(theta.size, min(25, theta.size), replace=False):
        step = np.zeros(theta.size)
        step[j] = h
        num = (PB.objective64(X, y, theta + step, PB.FIT_C, PB.FIT_L2, cw)[0]
               - PB.objective64(X, y, theta - step, PB.FIT_C, PB.FIT_L2, cw)[0]) / (2 * h)
        assert abs(num - grad[j]) <= 1e-8 + 1e-6 * abs(grad[j]), (j, num, grad[j])
    # the same gradient from the pieces the kernels compute: the forward's error rows through the chunked backward
    W, b = theta[:P * PB.FIT_C].reshape(P, PB.FIT_C), theta[P * PB.FIT_C:]
    fw = PB.forward64(ent, y, W, b, PB.FIT_C, cw)
    n = int(fw["used"].sum())
    gW, gb = PB.backward(PB.plan(ent, P), fw["err"].astype(np.float32), PB.FIT_C)
    np.testing.assert_allclose(np.concatenate([(gW / n + PB.FIT_L2 * W).reshape(-1), gb / n]), grad, rtol=0, atol=1e-7)
    assert abs(fw["row_loss"].sum() / n + 0.5 * PB.FIT_L2 * (W * W).sum() - loss) < 1e-12


def test_reference_fit_reaches_its_tolerance():
    _, ent, y, P, cw = fit_problem(PB.FIT_FEATURES, True)
    X = PB.dense_design(ent, PB.FIT_ROWS, P)
    theta = PB.fit64(X, y, PB.FIT_C, PB.FIT_L2, cw)
    assert np.linalg.norm(PB.objective64(X, y, theta, PB.FIT_C, PB.FIT_L2, cw)[1]) < 1e-10
    assert abs(theta[P * PB.FIT_C:].sum()) < 1e-9  # the biases keep their sum


# ---- 2: the plan --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("columns", PB.COLUMNS)
def test_plan_equals_a_dense_transposition(general, columns):
    code, seg = general
    col_of, P = PB.col_map(columns)
    for s in (seg, None):
        got = PB.plan(PB.entries(code, s, PB.HIDDEN, col_of), P)
        want = PB.plan_dense(code, s, PB.HIDDEN, col_of, P)
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and np.array_equal(a, b)
        col_ptr, t_row, _ = got
        assert col_ptr[-1] == t_row.size > 100
        for p in range(P):
            assert np.all(np.diff(t_row[col_ptr[p]:col_ptr[p + 1]]) > 0)  # ascending row, a row once


def test_chunked_backward_is_a_matrix_product(general):
    code, seg = general
    ent = PB.entries(code, seg, PB.HIDDEN)
    err = np.random.default_rng(3).standard_normal((PB.ROWS, 7)).astype(np.float32)
    gW, gb = PB.backward(PB.plan(ent, PB.HIDDEN), err, 5)
    X = PB.dense_design(ent, PB.ROWS, PB.HIDDEN)
    np.testing.assert_allclose(gW, X.T @ err[:, :5].astype(np.float64), rtol=0, atol=1e-10)
    np.testing.assert_allclose(gb, err[:, :5].astype(np.float64).sum(0), rtol=0, atol=1e-10)
    code, seg, _, _ = PB.chunk_case()
    col_ptr = PB.plan(PB.entries(code, seg, PB.HIDDEN), PB.HIDDEN)[0]
    lens = np.diff(col_ptr)
    assert lens[0] == 2 * PB.CHUNK + 100 and lens[1] == (2 * PB.CHUNK + 100 + 2) // 3 and 0 < lens[2:].max() <= PB.CHUNK  # three chunks, one


# ---- 3: the inputs are not degenerate -----------------------------------------------------------------------------------------
def test_general_inputs_hit_every_rule(general):
    (vals, idx), seg = general
    assert 680 <= PB.ROWS <= 720 and np.unique(seg[seg >= 0]).size == 5 and len(set(np.bincount(seg[seg >= 0]))) == 5
    assert (seg < 0).sum() > 20 and (vals == 0).any() and (vals < 0).any() and np.isnan(vals).any() and not np.isinf(vals).any()
    assert (idx < 0).any() and (idx >= PB.HIDDEN).any()
    rep = (idx[:, 1:] == idx[:, :-1]) & (vals[:, 1:] > 0) & (vals[:, :-1] > 0) & (seg >= 0)[:, None]
    assert rep.sum() > 10  # an index repeated within a row, both entries active
    r, pos, col, v = PB.entries((vals, idx), seg, PB.HIDDEN)
    assert v[(r == 20) & (col == 25)].tolist() == [0.625] and v[(r == 21) & (col == 26)].tolist() == [1.5]
    assert v[(r == 22) & (col == 27)].tolist() == [0.75]
    assert np.unique(r * PB.HIDDEN + col).size == r.size and (v > 0).all() and (seg[r] >= 0).all()
    for columns in ("window", "subset"):
        col_of, P = PB.col_map(columns)
        sub = PB.entries((vals, idx), seg, PB.HIDDEN, col_of)
        assert 50 < sub[0].size < r.size and sub[2].max() < P and np.unique(sub[2]).size > P // 2
    assert np.unique(PB.entries((vals, idx), seg, PB.HIDDEN, PB.col_map("window")[0])[2]).size < PB.WINDOW[1]  # columns without entries
    assert sorted(PB.col_map("subset")[0][PB.col_map("subset")[0] >= 0].tolist()) == list(range(11))
    assert np.any(np.diff(np.nonzero(PB.col_map("subset")[0] >= 0)[0]) > 1)  # scattered ...
    sub_cols = PB.col_map("subset")[0]
    assert np.any(np.diff(sub_cols[sub_cols >= 0]) < 0)  # ... and not in ascending order of the features


@pytest.mark.parametrize("C", PB.CLASSES)
def test_labels_hit_every_rule(general, C):
    _, seg = general
    labels = PB.labels_for(C)
    assert (labels == -1).any() and (labels >= C).any()
    y0 = PB.row_labels(seg, labels, PB.ROWS, C, 0)
    assert np.unique(y0[y0 >= 0]).size == C  # every class occurs
    assert ((y0 < 0) & (seg >= 0)).any() and (y0[seg < 0] < 0).all()
    for lag in PB.LAGS[1:]:
        y = PB.row_labels(seg, labels, PB.ROWS, C, lag)
        q = np.arange(PB.ROWS) + lag
        inside = (q >= 0) & (q < PB.ROWS)
        qc = np.clip(q, 0, PB.ROWS - 1)
        ok_label = (labels[qc] >= 0) & (labels[qc] < C)
        assert (y[~inside] < 0).all() and (~inside & (seg >= 0)).any()  # the lag leaves the call
        crosses = inside & (seg >= 0) & (seg[qc] >= 0) & (seg[qc] != seg) & ok_label
        assert crosses.any() and (y[crosses] < 0).all()  # ... or the utterance
        to_padding = inside & (seg >= 0) & (seg[qc] < 0) & ok_label
        assert to_padding.any() and (y[to_padding] < 0).all()
        assert (y >= 0).sum() > 400 and not np.array_equal(y, y0)


@pytest.mark.parametrize("columns", PB.COLUMNS)
@pytest.mark.parametrize("C", PB.CLASSES)
def test_accuracy_inputs_exclude_no_row(general, C, columns):
    """No used row has a float64 margin between its two largest logits below 8 d (d: the largest deviation of the float32
    mirror from float64 on these inputs), so argmax and confusion can be compared exactly on every row."""
    code, seg = general
    col_of, P = PB.col_map(columns)
    ent = PB.entries(code, seg, PB.HIDDEN, col_of)
    y = PB.row_labels(seg, PB.labels_for(C), PB.ROWS, C, 0)
    W, b, cw = PB.parameters(P, C, C)
    ref = PB.forward64(ent, y, W, b, C, cw)
    mir = PB.mirror32(code, ent, y, W, b, C, cw)
    d = max(np.abs(mir["err"] - ref["err"]).max(), np.abs(mir["row_loss"] - ref["row_loss"]).max())
    assert 0 < d < 2e-5 or C == 1
    assert ref["margin"][ref["used"]].min() >= 8 * d
    assert (ref["err"][~ref["used"]] == 0).all() and ref["used"].sum() > 500
    if C > 1:
        assert np.unique(ref["argmax"][ref["used"]]).size > 1
        np.testing.assert_allclose(ref["err"].sum(1), 0, atol=1e-12)
    assert PB.confusion(y, ref["argmax"], C).sum() == ref["used"].sum()
    assert PB.loss_q(mir["row_loss"]) > 0 or C == 1


def test_loss_q_is_exact_in_float32():
    loss = np.array([0.0, 1.0, 0.3, 1023.99994, 5000.0, 2.0 ** -21, 3 * 2.0 ** -21], np.float32)
    want = [0, 2 ** 20, int(np.rint(float(np.float32(0.3)) * 2 ** 20)), int(np.rint(float(np.float32(1023.99994)) * 2 ** 20)),
            1024 * 2 ** 20, 0, 2]  # ties to even
    assert PB.loss_q(loss) == sum(want)


# ---- 4: the Python layer before it needs a device -----------------------------------------------------------------------------
def test_argument_errors_need_no_device():
    with pytest.raises(ValueError, match="hidden"):
        SparseProbe(0, 3)
    for C in (0, N.PROBE_MAX_CLASSES + 1):
        with pytest.raises(ValueError, match="n_classes"):
            SparseProbe(16, C)
    with pytest.raises(ValueError, match="lag"):
        SparseProbe(16, 3, lag=1025)
    with pytest.raises(ValueError, match="l2"):
        SparseProbe(16, 3, l2=-1.0)
    with pytest.raises(ValueError, match="twice"):
        SparseProbe(16, 3, features=torch.tensor([1, 5, 1]))
    for bad in ([16], [-1, 2]):
        with pytest.raises(ValueError, match=r"\[0, 16\)"):
            SparseProbe(16, 3, features=torch.tensor(bad))
    for bad in (torch.zeros(2, 2, dtype=torch.int64), torch.tensor([0.5, 1.0]), torch.zeros(0, dtype=torch.int64)):
        with pytest.raises(ValueError, match="1-D"):
            SparseProbe(16, 3, features=bad)
    for bad in (torch.ones(2), torch.tensor([1.0, -1.0, 1.0]), torch.tensor([1.0, float("nan"), 1.0])):
        with pytest.raises(ValueError, match="class_weight"):
            SparseProbe(16, 3, class_weight=bad)
    p = SparseProbe(16, 3, features=torch.tensor([7, 2, 9]), lag=-2, class_weight=[1.0, 2.0, 0.5])
    assert p.n_cols == 3 and p.feature_index.tolist() == [7, 2, 9] and p._col_of.tolist().count(-1) == 13
    assert [int(p._col_of[f]) for f in (7, 2, 9)] == [0, 1, 2] and SparseProbe(16, 3).n_cols == 16
    with pytest.raises(ValueError, match="no data"):
        p.loss_and_grad()
    with pytest.raises(ValueError, match="no data"):
        p.fit()
    with pytest.raises(TypeError):
        p.add_data(torch.zeros(4, 2), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(N.WsaeError):  # host tensors
        p.add_data((torch.zeros(4, 2), torch.zeros(4, 2, dtype=torch.int32)), torch.zeros(4, dtype=torch.int64),
                   segments=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="ranking"):
        sparse_probe_curve((), (), torch.arange(4), sizes=(1, 8), hidden=16, n_classes=3)
    with pytest.raises(ValueError, match="ranking"):
        sparse_probe_curve((), (), torch.arange(4), sizes=(1, 2), hidden=16, n_classes=3, features=torch.arange(2))


def test_utterance_split():
    train, test = utterance_split(20, 0.2, seed=3)
    assert train.dtype == torch.bool and bool((train ^ test).all()) and int(test.sum()) == 4
    again = utterance_split(20, 0.2, seed=3)
    assert torch.equal(again[1], test) and not torch.equal(utterance_split(20, 0.2, seed=4)[1], test)
    assert int(utterance_split(2, 0.01)[1].sum()) == 1 and int(utterance_split(3, 0.99)[1].sum()) == 2
    for bad in ((1, 0.2), (10, 0.0), (10, 1.0)):
        with pytest.raises(ValueError):
            utterance_split(*bad)
