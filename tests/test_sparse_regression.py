"""Sparse ridge regression without a GPU: the numpy oracle of tests/regress_oracle.py against dense float64 algebra (its
chunked Gram matrix and moments against ``X^T X`` / ``X^T Y`` of the densified code, its forward product and five sums
against a matrix product), the argument errors the library finds on the host, the ridge algebra of
``ridge_from_statistics`` on hand-made statistics, and the errors the Python layer raises before it needs a device.  The
kernels are compared with this oracle in tests/test_gpu_sparse_regression.py."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import probe_oracle as PB
import regress_oracle as RG
from whisper_sae import _native as N
from whisper_sae.analysis import (RegressionCurve, RegressionFit, RegressionReport, SparseRegression, regression_curve,
                                  ridge_from_statistics, top_correlated_features)


# ---- 1: the oracle against dense float64 --------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden,k,columns,lag", [(96, 5, "identity", 0), (96, 32, "permuted", -3), (300, 33, "subset", 1),
                                                  (96, 128, "identity", 0)])
def test_oracle_statistics_equal_dense_products(hidden, k, columns, lag):
    code, seg = RG.general_case(hidden, k, rows=600)
    col_of, P = RG.col_map(columns, hidden)
    Y = RG.targets(np.random.default_rng(k), 600, 3)
    s = RG.statistics(code, seg, Y, lag, hidden, col_of, P)
    X, T = s["X"], s["T"]
    assert X.shape[0] == int(s["used"].sum()) > 300 and (X != 0).sum() > 600
    want = RG.gram_dense(X)
    scale = np.abs(want).max()
    np.testing.assert_allclose(np.triu(s["G"]), np.triu(want), rtol=1e-12, atol=1e-12 * scale)
    assert not np.tril(s["G"], -1).any()  # the oracle leaves the cells with c < p alone
    np.testing.assert_allclose(RG.mirror_upper(s["G"]), want, rtol=1e-12, atol=1e-12 * scale)
    np.testing.assert_allclose(s["MX"][:, :-1], X.T @ T, rtol=1e-12, atol=1e-12 * np.abs(X.T @ T).max())
    np.testing.assert_allclose(s["MX"][:, -1], X.sum(0), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(s["gb"][:-1], T.sum(0), rtol=1e-12, atol=1e-12)
    assert s["gb"][-1] == X.shape[0]  # the frames, an exact sum of ones
    # the rule folded into the segments: the plan holds the used rows only
    assert set(np.unique(s["pl"][1])) <= set(np.nonzero(s["used"])[0])


def test_oracle_windows_and_calls_compose():
    code, seg = RG.general_case(96, 5, rows=500)
    ent = PB.entries(code, seg, 96)
    pl = PB.plan(ent, 96)
    whole = RG.gram(pl, ent, 500, 96)
    parts = np.concatenate([RG.gram(pl, ent, 500, 96, p_lo=a, p_rows=b) for a, b in ((0, 1), (1, 40), (41, 55))])
    assert np.array_equal(parts, whole)
    twice = RG.gram(pl, ent, 500, 96, G=whole)
    np.testing.assert_allclose(twice, 2 * whole, rtol=1e-15)


def test_oracle_long_lists_span_chunks():
    code, seg, hidden = RG.long_case()
    rows = seg.size
    ent = PB.entries(code, seg, hidden)
    pl = PB.plan(ent, hidden)
    n3 = int(pl[0][4] - pl[0][3])
    assert 2 * RG.CHUNK < n3 < 3 * RG.CHUNK and n3 % RG.CHUNK  # three chunks, the last one ragged
    X = PB.dense_design(ent, rows, hidden)
    want = RG.gram_dense(X)
    np.testing.assert_allclose(np.triu(RG.gram(pl, ent, rows, hidden)), np.triu(want), rtol=1e-12)


@pytest.mark.parametrize("lag", [0, 2, -1])
def test_oracle_forward_equals_a_dense_product(lag):
    hidden, k, rows, C = 96, 8, 2 * RG.CHUNK + 37, 3
    code, seg = RG.general_case(hidden, k, rows=rows)
    col_of, P = RG.col_map("permuted", hidden)
    rng = np.random.default_rng(5)
    Y = RG.targets(rng, rows, C)
    W, b = rng.standard_normal((P, C)), rng.standard_normal(C)
    ent = PB.entries(code, seg, hidden, col_of)
    pred, n_used, stats = RG.forward(code, ent, seg, Y, lag, W, b, C)
    X = PB.dense_design(ent, rows, P)
    z = X @ W + b
    live = seg >= 0
    np.testing.assert_allclose(pred[live], z[live].astype(np.float32), rtol=2e-7, atol=1e-7)
    assert not pred[~live].any()
    used = RG.used_rows(seg, Y, rows, lag)
    assert n_used == int(used.sum()) and 0 < n_used < int(live.sum())
    y = Y[np.clip(np.arange(rows) + lag, 0, rows - 1)][used].astype(np.float64)
    want = np.stack([y.sum(0), (y * y).sum(0), z[used].sum(0), (z[used] ** 2).sum(0), ((y - z[used]) ** 2).sum(0)])
    np.testing.assert_allclose(stats, want, rtol=1e-11, atol=1e-9)
    only, none, nothing = RG.forward(code, ent, seg, None, lag, W, b, C)
    assert np.array_equal(only, pred) and none == 0 and nothing is None


# ---- 2: argument errors are found on the host ----------------------------------------------------------------------------------
def test_workspace_bytes_reject_invalid_arguments():
    lib = N.lib()
    entry_bytes = 8 * 100 * 8  # the column and the value of every entry of the code
    for p_rows, cap in ((96, 800), (1, 0)):
        assert entry_bytes <= lib.wsae_gram_workspace_bytes(100, 8, 96, 96, p_rows, cap) <= entry_bytes + 512
    for bad in ((-1, 8, 96, 96, 96, 800), (100, 0, 96, 96, 96, 800), (100, N.PROBE_MAX_K + 1, 96, 96, 96, 800),
                (100, 8, 0, 1, 1, 800), (100, 8, 96, 97, 1, 800), (100, 8, 96, 0, 1, 800), (100, 8, 96, 96, 0, 800),
                (100, 8, 96, 96, 97, 800), (100, 8, 96, 96, 96, -1), (2 ** 31, 8, 96, 96, 96, 800),
                (100, 8, 20000, N.GRAM_MAX_COLS + 1, 1, 800)):
        assert lib.wsae_gram_workspace_bytes(*bad) == -1, bad
    assert lib.wsae_gram_workspace_bytes(100, 8, 20000, N.GRAM_MAX_COLS, 1, 800) >= entry_bytes
    chunks = -(-5000 // N.PROBE_CHUNK)
    need = lib.wsae_regress_forward_workspace_bytes(5000, 8, 96, 96, 7, 0)
    assert 8 * chunks * 5 * 7 <= need <= 8 * chunks * 5 * 7 + 256
    for bad in ((-1, 8, 96, 96, 7, 0), (5000, 129, 96, 96, 7, 0), (5000, 8, 96, 97, 7, 0), (5000, 8, 96, 96, 0, 0),
                (5000, 8, 96, 96, N.PROBE_MAX_CLASSES + 1, 0), (5000, 8, 96, 96, 7, 1025), (5000, 8, 96, 96, 7, -1025)):
        assert lib.wsae_regress_forward_workspace_bytes(*bad) == -1, bad
    assert lib.wsae_regress_forward_workspace_bytes(5000, 8, 96, 96, N.PROBE_MAX_CLASSES, -1024) > 0


def test_entry_points_reject_invalid_arguments_without_a_gpu():
    """Every check runs on the host before any HIP call: host buffers stand in for the device pointers, which a rejected
    call never follows."""
    lib = N.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)

    def gram(k=8, hidden=96, n_rows=10, col_of=None, n_cols=96, cap=80, p_lo=0, p_rows=96, ldg=96, vals=p, G=p, t_row=p, ws=p,
             ws_bytes=1 << 20):
        return lib.wsae_gram_update(vals, p, k, hidden, None, n_rows, col_of, n_cols, p, t_row, p, cap, p_lo, p_rows, G, ldg, ws,
                                    ws_bytes, None)

    for kwargs, text in ((dict(vals=None), "null pointer"), (dict(G=None), "null pointer"), (dict(k=0), "1 <= k"),
                         (dict(k=129), "1 <= k"), (dict(hidden=0), "hidden"), (dict(n_rows=-1), "n_rows"),
                         (dict(n_cols=97), "n_cols"), (dict(n_cols=50, p_rows=50, ldg=50), "without col_of"),
                         (dict(hidden=20000, n_cols=N.GRAM_MAX_COLS + 1, col_of=p, ldg=20000), "n_cols <="),
                         (dict(cap=-1), "cap"), (dict(t_row=None), "cap"), (dict(p_lo=-1), "row window"),
                         (dict(p_rows=0), "row window"), (dict(p_lo=90, p_rows=7), "row window"), (dict(ldg=95), "ldg"),
                         (dict(ws_bytes=8), "workspace too small"), (dict(ws=None), "workspace too small"),
                         (dict(ws=p + 4), "8-byte aligned")):
        rc = gram(**kwargs)
        assert rc != 0 and text in N.last_error(), (kwargs, N.last_error())
    with pytest.raises(N.WsaeError):
        N.check(gram(ldg=1), "wsae_gram_update")

    def forward(k=8, hidden=96, Y=p, ldy=3, n_rows=10, lag=0, C=3, col_of=None, n_cols=96, W=p, ldw=3, pred=p, ldp=3, n_used=p,
                stats=p, ws=p, ws_bytes=1 << 20):
        return lib.wsae_regress_forward(p, p, k, hidden, None, Y, ldy, n_rows, lag, C, col_of, n_cols, W, ldw, p, pred, ldp, n_used,
                                        stats, ws, ws_bytes, None)

    for kwargs, text in ((dict(W=None), "null pointer"), (dict(k=200), "1 <= k"), (dict(n_rows=2 ** 31), "n_rows"),
                         (dict(n_cols=11), "without col_of"), (dict(C=0), "n_targets"), (dict(C=1025), "n_targets"),
                         (dict(lag=1025), "lag"), (dict(lag=-1025), "lag"), (dict(ldw=2), "ldw"), (dict(ldp=2), "ldp"),
                         (dict(ldy=2), "ldy"), (dict(n_used=None), "n_used"), (dict(stats=None), "stats"),
                         (dict(Y=None, pred=None), "nothing to compute"), (dict(ws_bytes=8), "workspace too small"),
                         (dict(ws=None), "workspace too small"), (dict(ws=p + 4), "8-byte aligned")):
        rc = forward(**kwargs)
        assert rc != 0 and text in N.last_error(), (kwargs, N.last_error())


# ---- 3: the ridge algebra on hand-made statistics --------------------------------------------------------------------------------
def handmade(seed=0, n=400, P=7, C=2):
    rng = np.random.default_rng(seed)
    X = np.abs(rng.standard_normal((n, P))) * (rng.random((n, P)) < 0.4)
    Y = X @ rng.standard_normal((P, C)) + 0.7 + 0.2 * rng.standard_normal((n, C))
    return X, Y


@pytest.mark.parametrize("l2", [0.0, 1e-3, 0.5])
def test_ridge_from_statistics_minimises_the_objective(l2):
    X, Y = handmade()
    n, P = X.shape
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    W, b, objective, r2 = ridge_from_statistics(t(X.T @ X), t(X.T @ Y), t(X.sum(0)), t(Y.sum(0)), t((Y * Y).sum(0)), n, l2)
    W, b = W.numpy(), b.numpy()
    # the stationarity of 1/(2n) sum |y - b - W^T x|^2 + l2 / 2 |W|^2 in W and in the unpenalised intercept
    res = Y - b - X @ W
    np.testing.assert_allclose(-X.T @ res / n + l2 * W, 0, atol=1e-12)
    np.testing.assert_allclose(res.mean(0), 0, atol=1e-12)
    assert objective == pytest.approx(0.5 * (res ** 2).sum() / n + 0.5 * l2 * (W ** 2).sum(), rel=1e-10)
    np.testing.assert_allclose(r2.numpy(), 1 - (res ** 2).sum(0) / ((Y - Y.mean(0)) ** 2).sum(0), rtol=1e-9)
    # the reference solve of the oracle on the same statistics
    Wn, bn, cond = RG.ridge(X.T @ X, X.T @ Y, X.sum(0), Y.sum(0), n, l2)
    assert cond < 1e8
    np.testing.assert_allclose(W, Wn, rtol=0, atol=1e3 * np.finfo(np.float64).eps * cond * np.abs(Wn).max())
    np.testing.assert_allclose(b, bn, rtol=0, atol=1e3 * np.finfo(np.float64).eps * cond * max(np.abs(Wn).max(), 1.0))
    if l2 == 0.0:
        lstsq = np.linalg.lstsq(np.concatenate([X, np.ones((n, 1))], 1), Y, rcond=None)[0]
        np.testing.assert_allclose(np.concatenate([W, b[None]]), lstsq, atol=1e-10)


def test_ridge_from_statistics_rejects_what_it_cannot_solve():
    X, Y = handmade(1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    args = [t(X.T @ X), t(X.T @ Y), t(X.sum(0)), t(Y.sum(0)), t((Y * Y).sum(0))]
    with pytest.raises(ValueError):
        ridge_from_statistics(*args, 0, 1e-3)
    with pytest.raises(ValueError):
        ridge_from_statistics(*args, X.shape[0], -1.0)
    X[:, 3] = 0.0  # a feature that never fires: singular without a penalty
    args = [t(X.T @ X), t(X.T @ Y), t(X.sum(0)), t(Y.sum(0)), t((Y * Y).sum(0))]
    with pytest.raises(ValueError, match="positive definite"):
        ridge_from_statistics(*args, X.shape[0], 0.0)
    W = ridge_from_statistics(*args, X.shape[0], 1e-3)[0]
    assert float(W[3].abs().max()) == 0.0


# ---- 4: the Python layer before it needs a device --------------------------------------------------------------------------------
def test_constructor_and_curve_arguments():
    for kwargs in (dict(hidden=0, n_targets=1), dict(hidden=8, n_targets=0), dict(hidden=8, n_targets=N.PROBE_MAX_CLASSES),
                   dict(hidden=8, n_targets=1, lag=1025), dict(hidden=8, n_targets=1, lag=-1025),
                   dict(hidden=8, n_targets=1, features=torch.tensor([1, 1])), dict(hidden=8, n_targets=1, features=torch.tensor([8])),
                   dict(hidden=8, n_targets=1, features=torch.tensor([0.5])), dict(hidden=8, n_targets=1, features=torch.tensor([], dtype=torch.int64)),
                   dict(hidden=N.GRAM_MAX_COLS + 1, n_targets=1)):
        with pytest.raises(ValueError):
            SparseRegression(**kwargs)
    s = SparseRegression(40, 2, features=torch.tensor([7, 3, 30]), lag=-2, device="cpu")
    assert s.n_cols == 3 and s.feature_index.tolist() == [7, 3, 30] and s.n_frames == 0
    with pytest.raises(N.WsaeError):  # the kernels run on the GPU only
        s.update((torch.zeros(4, 2), torch.zeros(4, 2, dtype=torch.int32)), torch.zeros(4, 2), segments=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(TypeError):
        s.update(torch.zeros(4, 2), torch.zeros(4, 2))
    with pytest.raises(ValueError):
        regression_curve(s, (), torch.tensor([7, 3]), sizes=(1, 3))
    with pytest.raises(ValueError):
        regression_curve(s, (), torch.tensor([7, 4]), sizes=(1, 2))  # feature 4 is not among the tracker's
    assert RegressionFit._fields == ("weight", "bias", "columns", "features", "l2", "objective", "r2_train")
    assert RegressionReport._fields == ("mse", "r2", "pearson", "n_frames")
    assert RegressionCurve._fields == ("sizes", "train_r2", "test_r2", "features") and callable(top_correlated_features)
