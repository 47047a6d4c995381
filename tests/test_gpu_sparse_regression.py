"""Sparse ridge regression on the MI355X against the numpy oracle of tests/regress_oracle.py: the Gram matrix, the forward
product with its five sums and the moments (through ``wsae_probe_backward``) bit for bit; the ridge solve against
``numpy.linalg.solve`` on the ORACLE's statistics within ``1e3 eps cond`` of that system; the correlations against
``numpy.corrcoef`` of the densified code; the regression curve against independent trackers; a planted noiseless target
against the dense float64 least-squares reference; and the Python layer on real modules.  The oracle itself is held to
dense float64 algebra on the CPU in tests/test_sparse_regression.py."""

from __future__ import annotations

import re
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch

import probe_oracle as PB
import regress_oracle as RG
import runs_oracle as RO
from whisper_sae import _native as N
from whisper_sae.analysis import (RegressionCurve, RegressionFit, RegressionReport, SparseRegression, collect_regression,
                                  regression_curve, top_correlated_features)
from whisper_sae.sae.model import BatchTopKSAE, ReLUSAE, TopKSAE

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TAIL = 3  # sentinel rows / elements behind every output
PAD = 5   # ldg = n_cols + PAD, ldp = C + PAD, ...
EPS = float(np.finfo(np.float64).eps)
SOURCE = Path(__file__).resolve().parents[1] / "whisper-sae_amd" / "csrc" / "wsae_regress.hip"


def kernel_constant(name):
    return int(re.search(r"constexpr int " + name + r" = (\d+);", SOURCE.read_text()).group(1))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def stream():
    return torch.cuda.current_stream().cuda_stream


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    view = np.int64 if a.dtype == np.float64 else np.int32
    assert np.array_equal(a.view(view), b.view(view)), np.argwhere(a.view(view) != b.view(view))[:5]


class Code:
    """A code, its segments, its column map and the oracle's plan of them, on the host and on the device."""

    def __init__(self, code, seg, hidden, col_of=None, P=None):
        self.v, self.i = dev(np.asarray(code[0], np.float32)), dev(np.asarray(code[1], np.int32))
        self.seg = None if seg is None else dev(np.asarray(seg, np.int32))
        self.col_of = None if col_of is None else dev(np.asarray(col_of, np.int32))
        self.rows, self.k = self.v.shape
        self.hidden, self.P = hidden, hidden if P is None else P
        self.ent = PB.entries(code, seg, hidden, col_of)
        self.pl = PB.plan(self.ent, self.P)
        self.cap = int(self.pl[0][-1])
        self.pl_d = tuple(dev(a) for a in self.pl)


def stored_triangle(rng, p_lo, p_rows, P):
    """A stored window ``[p_rows, P]``: random values where the kernel accumulates (c >= p), the sentinel elsewhere."""
    G = rng.standard_normal((p_rows, P))
    G[np.arange(P)[None, :] < (p_lo + np.arange(p_rows))[:, None]] = RG.SENTINEL
    return G


def run_gram(c, G0, p_lo=0, p_rows=None, ldg=None, n_rows=None, cap=None):
    """``wsae_gram_update`` on the window from the stored ``G0 [p_rows, P]`` -> the window as numpy.  The sentinel behind
    the columns, behind the rows and in the cells with c < p must survive."""
    p_rows = c.P - p_lo if p_rows is None else p_rows
    ldg = c.P + PAD if ldg is None else ldg
    assert ldg > c.P
    n_rows = c.rows if n_rows is None else n_rows
    cap = c.cap if cap is None else cap
    G = torch.full((p_rows + TAIL, ldg), RG.SENTINEL, dtype=torch.float64, device=DEV)
    G[:p_rows, :c.P] = dev(G0)
    lib = N.lib()
    need = lib.wsae_gram_workspace_bytes(n_rows, c.k, c.hidden, c.P, p_rows, cap)
    assert need >= 0
    ws = torch.full((need + 64,), 0xAB, dtype=torch.uint8, device=DEV)  # (arbitrary contents on entry)
    col_ptr, t_row, t_val = c.pl_d
    N.check(lib.wsae_gram_update(c.v.data_ptr(), c.i.data_ptr(), c.k, c.hidden, N.ptr(c.seg), n_rows, N.ptr(c.col_of), c.P,
                                 col_ptr.data_ptr(), N.ptr(t_row), N.ptr(t_val), cap, p_lo, p_rows, G.data_ptr(), ldg,
                                 ws.data_ptr(), need, stream()), "wsae_gram_update")
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xAB).all())
    out = G.cpu().numpy()
    assert (out[p_rows:] == RG.SENTINEL).all() and (out[:, c.P:] == RG.SENTINEL).all()
    win = out[:p_rows, :c.P]
    below = np.arange(c.P)[None, :] < (p_lo + np.arange(p_rows))[:, None]
    assert (win[below] == RG.SENTINEL).all() and below.sum() == (G0 == RG.SENTINEL).sum()
    return win


# ---- 1: the Gram matrix -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("columns", ["identity", "subset", "permuted"])
@pytest.mark.parametrize("k", [1, 5, 32, 33, 64, 128])
@pytest.mark.parametrize("hidden", [96, 300])
def test_gram_equals_the_oracle(hidden, k, columns):
    code, seg = RG.general_case(hidden, k)
    col_of, P = RG.col_map(columns, hidden)
    c = Code(code, seg, hidden, col_of, P)
    assert 700 <= c.rows <= 3000 and c.cap > c.rows // 5
    rng = np.random.default_rng(hidden + k)
    G0 = stored_triangle(rng, 0, P, P)
    got = run_gram(c, G0)
    same_bits(got, RG.gram(c.pl, c.ent, c.rows, P, G=G0))
    # without seg every row is live: other lists, other bits - and another ldg, the same bits
    if k in (5, 33):
        c2 = Code(code, None, hidden, col_of, P)
        want = RG.gram(c2.pl, c2.ent, c2.rows, P, G=G0)
        same_bits(run_gram(c2, G0), want)
        same_bits(run_gram(c2, G0, ldg=P + 61), want)


def test_long_lists_span_chunks():
    code, seg, hidden = RG.long_case()
    c = Code(code, seg, hidden)
    n3 = int(c.pl[0][4] - c.pl[0][3])
    assert 2 * RG.CHUNK < n3 < 3 * RG.CHUNK and n3 % RG.CHUNK and c.rows > 4900
    G0 = stored_triangle(np.random.default_rng(1), 0, hidden, hidden)
    got, want = run_gram(c, G0), RG.gram(c.pl, c.ent, c.rows, hidden, G=G0)
    same_bits(got[3, 3:], want[3, 3:])  # the long list: its diagonal and its off-diagonals
    same_bits(got, want)
    # more chunks than the waves of a workgroup: the list walked in several rounds
    rows = (kernel_constant("GR_WAVES") + 1) * RG.CHUNK + 11
    rng = np.random.default_rng(2)
    vals, idx = RO.persistent_code(rng, rows, 2, 6)
    idx[:, 0] = 6  # feature 6 on every row
    c = Code((vals, idx.astype(np.int32)), None, 7)
    G0 = stored_triangle(rng, 0, 7, 7)
    same_bits(run_gram(c, G0), RG.gram(c.pl, c.ent, rows, 7, G=G0))


def test_row_windows_reproduce_the_single_call():
    code, seg = RG.general_case(96, 5)
    col_of, P = RG.col_map("permuted", 96)
    c = Code(code, seg, 96, col_of, P)
    G0 = stored_triangle(np.random.default_rng(3), 0, P, P)
    whole = run_gram(c, G0)
    for cuts in ([(0, 1), (1, 1), (2, P - 3), (P - 1, 1)], [(0, 17), (17, P - 17)]):
        parts = np.concatenate([run_gram(c, G0[a:a + n], p_lo=a, p_rows=n) for a, n in cuts])
        same_bits(parts, whole)


def test_two_calls_equal_the_oracle_over_two_calls():
    hidden, k = 96, 5
    code, seg = RG.general_case(hidden, k)
    half = int(np.nonzero(seg == 2)[0][0])  # whole utterances on both sides
    a = Code((code[0][:half], code[1][:half]), seg[:half], hidden)
    b = Code((code[0][half:], code[1][half:]), seg[half:], hidden)
    G0 = stored_triangle(np.random.default_rng(4), 0, hidden, hidden)
    got = run_gram(b, run_gram(a, G0))
    want = RG.gram(b.pl, b.ent, b.rows, hidden, G=RG.gram(a.pl, a.ent, a.rows, hidden, G=G0))
    same_bits(got, want)


def test_small_cases():
    code, seg = RG.general_case(96, 5)
    # one column
    col_of = np.full(96, -1, np.int32)
    col_of[40] = 0
    c = Code(code, seg, 96, col_of, 1)
    assert c.cap > 10
    G0 = np.array([[0.5]])
    same_bits(run_gram(c, G0), RG.gram(c.pl, c.ent, c.rows, 1, G=G0))
    one = Code((code[0][:, :1], np.zeros((c.rows, 1), np.int32)), seg, 1)  # hidden = 1
    same_bits(run_gram(one, G0), RG.gram(one.pl, one.ent, one.rows, 1, G=G0))
    # more columns than one pass of the grid, and columns without entries, which are not touched (-0.0 keeps its sign)
    hidden = kernel_constant("GR_MAX_BLOCKS") + 77
    rng = np.random.default_rng(5)
    wide = RO.spoil(rng, RO.persistent_code(rng, 400, 3, hidden), hidden)
    c = Code(wide, None, hidden)
    empty = np.diff(c.pl[0]) == 0
    assert empty.sum() > 100 and (~empty).sum() > 100 and (~empty)[-77:].any()
    G0 = np.full((hidden, hidden), -0.0)
    G0[np.tril_indices(hidden, -1)] = RG.SENTINEL
    got = run_gram(c, G0)
    same_bits(got, RG.gram(c.pl, c.ent, c.rows, hidden, G=G0))
    assert np.signbit(got[empty][:, -1]).all() and not np.signbit(got[~empty][:, -1]).any()
    # no rows: nothing is touched
    c = Code(code, seg, 96)
    G0 = stored_triangle(rng, 0, 96, 96)
    same_bits(run_gram(c, G0, n_rows=0), G0)


def test_the_column_limit():
    P = N.GRAM_MAX_COLS
    assert P >= 8192
    rng = np.random.default_rng(6)
    code = RO.persistent_code(rng, 300, 4, P)
    code[1][:, 0] = P - 3  # a full list inside the window
    c = Code(code, None, P)
    p_lo, p_rows = P - 6, 5  # only a small row window of G exists
    G0 = stored_triangle(rng, p_lo, p_rows, P)
    got = run_gram(c, G0, p_lo=p_lo, p_rows=p_rows)
    same_bits(got, RG.gram(c.pl, c.ent, c.rows, P, G=G0, p_lo=p_lo, p_rows=p_rows))
    assert got[3, P - 3] > G0[3, P - 3] + 10
    p_first = int(np.nonzero(np.diff(c.pl[0]))[0][0])  # the first row with entries: every tile of the columns
    G1 = stored_triangle(rng, p_first, 1, P)
    same_bits(run_gram(c, G1, p_lo=p_first, p_rows=1), RG.gram(c.pl, c.ent, c.rows, P, G=G1, p_lo=p_first, p_rows=1))
    assert p_first < kernel_constant("GR_TILE_WIDE")
    # one past the maximum is an argument error
    lib = N.lib()
    col_of = torch.zeros(P + 8, dtype=torch.int32, device=DEV)
    G = torch.zeros(4, dtype=torch.float64, device=DEV)
    ws = torch.empty(lib.wsae_gram_workspace_bytes(c.rows, c.k, P, P, 1, c.cap), dtype=torch.uint8, device=DEV)
    rc = lib.wsae_gram_update(c.v.data_ptr(), c.i.data_ptr(), c.k, P + 8, None, c.rows, col_of.data_ptr(), P + 1,
                              c.pl_d[0].data_ptr(), c.pl_d[1].data_ptr(), c.pl_d[2].data_ptr(), c.cap, 0, 1, G.data_ptr(), P + 1,
                              ws.data_ptr(), ws.numel(), stream())
    assert rc != 0 and "n_cols <=" in N.last_error()
    assert lib.wsae_gram_workspace_bytes(c.rows, c.k, P + 8, P + 1, 1, c.cap) == -1


# ---- 2: the forward product ---------------------------------------------------------------------------------------------------
def run_forward(c, Y, lag, W, b, C, stats0=None, n_used0=0, with_pred=True, n_rows=None):
    """``wsae_regress_forward`` -> (pred, n_used, stats) as numpy; sentinels around every output must survive and a 0xAB
    workspace must be intact past the size queried."""
    n_rows = c.rows if n_rows is None else n_rows
    ldy, ldw, ldp = C + 2, C + PAD, C + 4
    Yd = None
    if Y is not None:
        Yh = np.full((c.rows, ldy), np.nan, np.float32)  # (reading behind the C targets would drop the row)
        Yh[:, :C] = Y
        Yd = dev(Yh)
    Wh = np.full((c.P, ldw), RG.SENTINEL)
    Wh[:, :C] = W
    Wd, bd = dev(Wh), dev(np.asarray(b, np.float64))
    pred = torch.full((c.rows + TAIL, ldp), RG.SENTINEL, dtype=torch.float32, device=DEV) if with_pred else None
    n_used = torch.full((1 + TAIL,), 77, dtype=torch.int64, device=DEV)
    n_used[0] = n_used0
    stats = torch.full((5 + TAIL, C), RG.SENTINEL, dtype=torch.float64, device=DEV)
    stats[:5] = 0 if stats0 is None else dev(stats0)
    lib = N.lib()
    need = lib.wsae_regress_forward_workspace_bytes(n_rows, c.k, c.hidden, c.P, C, lag)
    assert need >= 0
    ws = torch.full((need + 64,), 0xAB, dtype=torch.uint8, device=DEV)
    N.check(lib.wsae_regress_forward(c.v.data_ptr(), c.i.data_ptr(), c.k, c.hidden, N.ptr(c.seg), N.ptr(Yd), ldy, n_rows, lag, C,
                                     N.ptr(c.col_of), c.P, Wd.data_ptr(), ldw, bd.data_ptr(), N.ptr(pred), ldp,
                                     n_used.data_ptr(), stats.data_ptr(), ws.data_ptr(), need, stream()), "wsae_regress_forward")
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xAB).all()) and bool((n_used[1:] == 77).all()) and bool((stats[5:] == RG.SENTINEL).all())
    out = None
    if with_pred:
        assert bool((pred[n_rows:] == RG.SENTINEL).all()) and bool((pred[:, C:] == RG.SENTINEL).all())
        out = pred[:c.rows, :C].cpu().numpy()
    return out, int(n_used[0]), stats[:5].cpu().numpy()


@pytest.mark.parametrize("lag", [0, 1, -1, 3, -3], ids=lambda l: f"lag{l}")
@pytest.mark.parametrize("hidden,k,C,columns", [(96, 8, 3, "permuted"), (300, 128, 70, "identity"), (96, 65, 1, "subset")])
def test_forward_equals_the_oracle(hidden, k, C, columns, lag):
    rows = 2 * RG.CHUNK + 37 if k == 8 else 700  # (k = 8: rows in three chunks of the sums, the last one ragged)
    code, seg = RG.general_case(hidden, k, rows=rows)
    col_of, P = RG.col_map(columns, hidden)
    c = Code(code, seg, hidden, col_of, P)
    rng = np.random.default_rng(100 + k + lag)
    Y = RG.targets(rng, rows, C)
    W, b = rng.standard_normal((P, C)), rng.standard_normal(C)
    used = RG.used_rows(seg, Y, rows, lag)
    live = seg >= 0
    assert 0 < used.sum() < live.sum() - 5  # borders and non-finite rows drop some
    stats0 = rng.standard_normal((5, C))
    pred, n_used, stats = run_forward(c, Y, lag, W, b, C, stats0, n_used0=1000)
    wp, wn, ws = RG.forward(code, c.ent, seg, Y, lag, W, b, C, stats0)
    same_bits(pred, wp)
    assert (pred[~live] == 0).all() and not np.signbit(pred[~live]).any()  # exact zeros on padding
    assert n_used == 1000 + wn == 1000 + int(used.sum())
    same_bits(stats, ws)
    # Y == NULL: the predictions alone; and the sums without the predictions
    only, n0, s0 = run_forward(c, None, lag, W, b, C, stats0, n_used0=5)
    same_bits(only, wp)
    assert n0 == 5
    same_bits(s0, stats0)
    _, n1, s1 = run_forward(c, Y, lag, W, b, C, stats0, with_pred=False)
    assert n1 == wn
    same_bits(s1, ws)


def test_forward_without_segments_and_without_rows():
    hidden, k, C, rows = 96, 5, 2, 700
    code, _ = RG.general_case(hidden, k, rows=rows)
    c = Code(code, None, hidden)
    rng = np.random.default_rng(7)
    Y = RG.targets(rng, rows, C)
    W, b = rng.standard_normal((hidden, C)), rng.standard_normal(C)
    pred, n_used, stats = run_forward(c, Y, 2, W, b, C)
    wp, wn, ws = RG.forward(code, c.ent, None, Y, 2, W, b, C)
    same_bits(pred, wp)
    same_bits(stats, ws)
    assert n_used == wn
    pred, n_used, stats = run_forward(c, Y, 0, W, b, C, n_rows=0)
    assert (pred == RG.SENTINEL).all() and n_used == 0 and not stats.any()


# ---- 3: the moments through wsae_probe_backward -------------------------------------------------------------------------------
@pytest.mark.parametrize("lag", [0, -2])
def test_moments_equal_the_oracle(lag):
    hidden, k, C = 96, 8, 3
    code, seg = RG.general_case(hidden, k, rows=2 * RG.CHUNK + 300)
    rows = seg.size
    col_of, P = RG.col_map("permuted", hidden)
    Y = RG.targets(np.random.default_rng(8), rows, C)
    s = RG.statistics(code, seg, Y, lag, hidden, col_of, P)
    col_ptr, t_row, t_val = (dev(a) for a in s["pl"])
    cap = int(s["pl"][0][-1])
    MX = torch.zeros(P, C + 1, dtype=torch.float64, device=DEV)
    gb = torch.zeros(C + 1, dtype=torch.float64, device=DEV)
    lib = N.lib()
    need = lib.wsae_probe_backward_workspace_bytes(rows, P, C + 1, cap)
    ws = torch.empty(need + 8, dtype=torch.uint8, device=DEV)
    E = dev(s["E"])
    N.check(lib.wsae_probe_backward(col_ptr.data_ptr(), t_row.data_ptr(), t_val.data_ptr(), cap, P, E.data_ptr(), C + 1, C + 1, rows,
                                    MX.data_ptr(), gb.data_ptr(), ws.data_ptr(), need, stream()), "wsae_probe_backward")
    same_bits(MX.cpu().numpy(), s["MX"])
    same_bits(gb.cpu().numpy(), s["gb"])
    assert gb[-1].item() == s["used"].sum()
    # the tracker hands the kernels the same rows: its whole state equals the oracle's
    reg = SparseRegression(hidden, C, features=torch.from_numpy(np.argsort(np.where(col_of < 0, hidden, col_of), kind="stable")[:P].copy()),
                           lag=lag, device=DEV)
    reg.update((dev(code[0]), dev(code[1])), dev(Y), segments=dev(seg))
    same_bits(torch.triu(reg._G).cpu().numpy(), np.triu(s["G"]))
    assert not torch.tril(reg._G, -1).any()
    same_bits(reg._MX.cpu().numpy(), s["MX"])
    same_bits(reg._sums.cpu().numpy(), s["gb"])
    assert reg.n_frames == int(s["used"].sum())
    np.testing.assert_allclose(reg.target_sq.cpu().numpy(), s["syy"], rtol=rows * EPS)
    same_bits(reg.gram().cpu().numpy(), RG.mirror_upper(s["G"]))


def test_a_dense_subset_is_planned_twice():
    """``update`` guesses the size of the plan from the subset's share of the dictionary; here every row holds all of the
    subset, the plan names more entries than the guess and is transposed again at the true count."""
    code, col_of, P = PB.dense_subset_case()
    C = 2
    rows, k = PB.DENSE_UTT * PB.DENSE_T, PB.DENSE_K
    flat = (code[0].reshape(rows, k), code[1].reshape(rows, k))
    seg = np.repeat(np.arange(PB.DENSE_UTT), PB.DENSE_T).astype(np.int32)
    Y = RG.targets(np.random.default_rng(62), rows, C)
    s = RG.statistics(flat, seg, Y, 0, PB.DENSE_HIDDEN, col_of, P)
    nnz, guess = int(s["pl"][0][-1]), 1024 + 2 * rows * k * P // PB.DENSE_HIDDEN
    assert guess == 1280 and nnz > guess and nnz == k * int(s["used"].sum())  # the precondition, from the oracle's plan
    reg = SparseRegression(PB.DENSE_HIDDEN, C, features=torch.tensor(PB.DENSE_FEATURES), device=DEV)
    reg.update((dev(code[0]), dev(code[1])), dev(Y.reshape(PB.DENSE_UTT, PB.DENSE_T, C)))
    same_bits(reg.gram().cpu().numpy(), RG.mirror_upper(s["G"]))
    same_bits(reg.moment.cpu().numpy(), s["MX"][:, :-1])
    same_bits(reg.col_sum.cpu().numpy(), s["MX"][:, -1])
    same_bits(reg.target_sum.cpu().numpy(), s["gb"][:-1])
    assert reg.n_frames == int(s["used"].sum()) > 1500
    np.testing.assert_allclose(reg.target_sq.cpu().numpy(), s["syy"], rtol=rows * EPS)


# ---- 4: the solve, the correlations, the curve --------------------------------------------------------------------------------
def tracker_of(code, seg, Y, hidden, C, features=None, lag=0):
    reg = SparseRegression(hidden, C, features=None if features is None else torch.as_tensor(features), lag=lag, device=DEV)
    reg.update((dev(code[0]), dev(code[1])), dev(Y), segments=dev(seg))
    return reg


def check_solve(fit, s, l2, columns=None):
    """A fit against ``numpy.linalg.solve`` on the oracle's statistics ``s`` (restricted to ``columns``) -> the bound."""
    G = RG.mirror_upper(s["G"])
    MX = s["MX"]
    if columns is not None:
        G, MX = G[np.ix_(columns, columns)], MX[columns]
    n = float(s["gb"][-1])
    W, b, cond = RG.ridge(G, MX[:, :-1], MX[:, -1], s["gb"][:-1], n, l2)
    assert cond <= 1e8, cond  # so that the bound means something
    bound = 1e3 * EPS * cond
    dW = np.abs(fit.weight.numpy() - W).max()
    print(f"solve: cond = {cond:.3e}, bound = {bound:.3e}, |dW| / |W| = {dW / np.abs(W).max():.3e}")
    assert dW <= bound * np.abs(W).max()
    # b = ybar - W^T xbar: the error of W times the 1-norm of xbar, and the rounding of ybar
    xbar = MX[:, -1] / n
    assert np.abs(fit.bias.numpy() - b).max() <= bound * (np.abs(W).max() * np.abs(xbar).sum() + np.abs(b).max())
    return W, b, bound


@pytest.mark.parametrize("features", [None, (3, 60, 17, 8, 41, 22, 35)], ids=["all", "subset"])
def test_fit_equals_numpy_on_the_oracle_statistics(features):
    code, seg, Y = RG.fit_case()
    hidden, C, l2 = RG.FIT_HIDDEN, RG.FIT_C, RG.FIT_L2
    col_of, P = None, hidden
    if features is not None:
        col_of = np.full(hidden, -1, np.int32)
        col_of[list(features)] = np.arange(len(features))
        P = len(features)
    s = RG.statistics(code, seg, Y, 0, hidden, col_of, P)
    reg = tracker_of(code, seg, Y, hidden, C, features)
    fit = reg.fit(l2)
    assert isinstance(fit, RegressionFit) and fit.l2 == l2 and fit.columns.tolist() == list(range(P))
    assert fit.features.tolist() == (list(range(hidden)) if features is None else list(features))
    W, b, bound = check_solve(fit, s, l2)
    # the objective and the training R^2 against the dense float64 residuals at the reference solution
    X, T = s["X"], s["T"]
    res = T - b - X @ W
    n = X.shape[0]
    assert fit.objective == pytest.approx(0.5 * (res ** 2).sum() / n + 0.5 * l2 * (W ** 2).sum(), rel=1e-9)
    np.testing.assert_allclose(fit.r2_train.numpy(), 1 - (res ** 2).sum(0) / ((T - T.mean(0)) ** 2).sum(0), atol=1e-9)
    # a sub-block of the same state: no data are read again
    cols = [5, 0, 3] if features is not None else [50, 2, 77, 31]
    check_solve(reg.fit(l2, torch.tensor(cols)), s, l2, cols)
    check_solve(reg.fit(10 * l2, torch.tensor(cols)), s, 10 * l2, cols)
    with pytest.raises(ValueError):
        reg.fit(l2, torch.tensor([0, 0]))
    with pytest.raises(ValueError):
        reg.fit(l2, torch.tensor([P]))


def test_correlations_equal_corrcoef():
    code, seg, Y = RG.fit_case(1)
    hidden, C = RG.FIT_HIDDEN, RG.FIT_C
    s = RG.statistics(code, seg, Y, 0, hidden, None, hidden)
    X, T = s["X"], s["T"]
    reg = tracker_of(code, seg, Y, hidden, C)
    r, rf = reg.correlations().cpu().numpy(), reg.feature_correlations().cpu().numpy()
    assert r.shape == (hidden, C) and rf.shape == (hidden, hidden)
    moving = X.std(0) > 0
    assert 70 < moving.sum() < hidden  # most features fire, some never do
    with np.errstate(invalid="ignore", divide="ignore"):
        full = np.corrcoef(np.concatenate([X, T], 1), rowvar=False)
    # r from raw moments: covariance and variances are differences of second moments and products of means, so their
    # rounding is eps times sqrt(E x^2 E y^2) against sigma_x sigma_y - the condition number of this computation
    m2 = np.sqrt(np.concatenate([(X * X).mean(0), (T * T).mean(0)]))
    sd = np.concatenate([X.std(0), T.std(0)])
    ok = np.concatenate([moving, np.ones(C, bool)])
    cond = (np.outer(m2[ok], m2[ok]) / np.outer(sd[ok], sd[ok])).max()
    assert cond <= 1e8
    bound = 1e3 * EPS * cond
    print(f"correlations: cond = {cond:.3e}, deviation = {np.abs(r[moving] - full[:hidden, hidden:][moving]).max():.3e}")
    assert np.abs(r[moving] - full[:hidden, hidden:][moving]).max() <= bound
    assert np.abs(rf[np.ix_(moving, moving)] - full[:hidden, :hidden][np.ix_(moving, moving)]).max() <= bound
    assert not r[~moving].any() and not rf[~moving].any() and not rf[:, ~moving].any()  # 0 where a variance is 0
    # a constant target has no variance either
    flat = tracker_of(code, seg, np.ones_like(Y), hidden, C)
    assert not flat.correlations().any()
    feats, top = top_correlated_features(reg, 1, 5)
    order = np.argsort(-np.abs(np.where(moving, r[:, 1], 0)), kind="stable")[:5]
    assert feats.tolist() == order.tolist() and np.array_equal(top.cpu().numpy(), r[order, 1])


def test_regression_curve_equals_independent_trackers():
    code, seg, Y = RG.fit_case(2)
    hidden, C, l2 = RG.FIT_HIDDEN, RG.FIT_C, RG.FIT_L2
    cut = 750  # whole utterances: the first five train, the last three test
    tr = ((code[0][:cut], code[1][:cut]), seg[:cut], Y[:cut])
    te = ((code[0][cut:], code[1][cut:]), seg[cut:], Y[cut:])
    reg = tracker_of(*tr, hidden, C)
    ranking, _ = top_correlated_features(reg, 0, 40)
    ranking = ranking.cpu()
    test_args = ((dev(te[0][0]), dev(te[0][1])), dev(te[2]), None, dev(te[1]))
    sizes = (1, 2, 4, 8, 16, 32)
    curve = regression_curve(reg, test_args, ranking, sizes=sizes, l2=l2)
    assert isinstance(curve, RegressionCurve) and curve.sizes == sizes and torch.equal(curve.features, ranking)
    assert curve.train_r2.shape == curve.test_r2.shape == (len(sizes), C)
    s_te = RG.statistics(*te[:2], te[2], 0, hidden, None, hidden)
    s_all = RG.statistics(*tr[:2], tr[2], 0, hidden, None, hidden)
    for j, n in enumerate(sizes):
        feats = ranking[:n].tolist()
        col_of = np.full(hidden, -1, np.int32)
        col_of[feats] = np.arange(n)
        s = RG.statistics(*tr[:2], tr[2], 0, hidden, col_of, n)
        alone = tracker_of(*tr, hidden, C, features=feats)
        fit_alone = alone.fit(l2)
        W, b, bound = check_solve(fit_alone, s, l2)
        where = [reg.feature_index.tolist().index(f) for f in feats]
        check_solve(reg.fit(l2, torch.tensor(where)), s_all, l2, where)
        # R^2 moves with the prediction: |d sse| <= 2 sqrt(sse) m + m^2 with m the 2-norm over the rows of
        # |dW|_max |x_r|_1 + |db|; both fits lie within the solve bound of their reference, hence the factor 2
        dW = 2 * bound * np.abs(W).max()
        db = 2 * bound * (np.abs(W).max() * np.abs(s["MX"][:, -1] / s["gb"][-1]).sum() + np.abs(b).max())
        for X, T, got in ((s["X"], s["T"], curve.train_r2[j].numpy()), (s_te["X"][:, feats], s_te["T"], curve.test_r2[j].numpy())):
            res = T - b - X @ W
            sse, sst = (res ** 2).sum(0), ((T - T.mean(0)) ** 2).sum(0)
            move = np.linalg.norm(dW * np.abs(X).sum(1) + db)
            tol = (2 * np.sqrt(sse) * move + move ** 2) / sst + 1e-12
            assert (np.abs(got - (1 - sse / sst)) <= tol).all(), (n, got, 1 - sse / sst, tol)
        rep = alone.evaluate(fit_alone, *test_args)
        np.testing.assert_allclose(rep.r2.numpy(), curve.test_r2[j].numpy(), atol=1e-9)
    tr2 = curve.train_r2[:, 0].numpy()
    assert tr2[-1] > tr2[0] + 0.05  # 32 features explain more of the training variance than one


def test_planted_target():
    (code_tr, Y_tr), (code_te, Y_te) = RG.planted_case(0), RG.planted_case(1)
    hidden, C, l2 = 32, 2, 1e-6
    reg = SparseRegression(hidden, C, device=DEV)
    reg.update((dev(code_tr[0])[None], dev(code_tr[1])[None]), dev(Y_tr))
    fit = reg.fit(l2)
    T = Y_tr.shape[1]
    s = RG.statistics(code_tr, np.zeros(T, np.int32), Y_tr[0], 0, hidden, None, hidden)
    W, b, bound = check_solve(fit, s, l2)
    # the dense float64 least-squares reference recovers the planted map (the penalty moves it by O(l2))
    np.testing.assert_allclose(W[list(RG.PLANTED)], RG.PLANTED_W, atol=1e-4)
    np.testing.assert_allclose(b, RG.PLANTED_B, atol=1e-4)
    np.testing.assert_allclose(fit.weight.numpy()[list(RG.PLANTED)], RG.PLANTED_W, atol=1e-4)
    assert np.abs(np.delete(fit.weight.numpy(), RG.PLANTED, 0)).max() < 1e-4
    # held out: the report against the dense reference prediction at the fitted weights
    te = ((dev(code_te[0])[None], dev(code_te[1])[None]), dev(Y_te))
    rep = reg.evaluate(fit, *te)
    assert isinstance(rep, RegressionReport) and rep.n_frames == T
    ent = PB.entries(code_te, None, hidden)
    X = PB.dense_design(ent, T, hidden)
    z = X @ fit.weight.numpy() + fit.bias.numpy()
    y = Y_te[0].astype(np.float64)
    sse, sst = ((y - z) ** 2).sum(0), ((y - y.mean(0)) ** 2).sum(0)
    np.testing.assert_allclose(rep.mse.numpy(), sse / T, rtol=1e-9, atol=1e-18)
    np.testing.assert_allclose(rep.r2.numpy(), 1 - sse / sst, rtol=0, atol=1e-12)
    np.testing.assert_allclose(rep.pearson.numpy(), [np.corrcoef(y[:, c], z[:, c])[0, 1] for c in range(C)], atol=1e-9)
    assert (rep.r2.numpy() > 1 - 1e-6).all()
    pred = reg.predict(fit, te[0])
    assert pred.shape == (1, T, C) and pred.dtype == torch.float32
    np.testing.assert_allclose(pred[0].cpu().numpy(), z, rtol=2.0 ** -23, atol=1e-12)  # float32 of a float64 chain
    # the planted features rank first
    for c in range(C):
        order = np.argsort(-RG.PLANTED_W[:, c])
        feats, w = reg.top_weights(fit, c, 2)
        assert feats.tolist() == [RG.PLANTED[i] for i in order[:2]] and float(w[0]) > float(w[1]) > 0.4
        feats, r = top_correlated_features(reg, c, 3)
        assert set(feats.tolist()) == set(RG.PLANTED) and float(r.abs().min()) > 0.15


# ---- 5: the Python layer ------------------------------------------------------------------------------------------------------
D, H, K, UTT, T_PY, C_PY = 32, 128, 8, 12, 40, 3


def utterances(seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(UTT, T_PY, D, generator=gen)
    y = torch.stack([x[..., 0] * 2 - x[..., 1], x[..., 2].abs(), torch.arange(T_PY).float().expand(UTT, T_PY) / T_PY], -1)
    y[2, 5, 1] = float("nan")
    mask = torch.ones(UTT, T_PY)
    for u in range(UTT):
        mask[u, 28 + (u % 5) * 3:] = 0
    mask[3, 10] = 0
    return [(x[:5], y[:5], mask[:5]), (x[5:6], y[5:6], mask[5:6]), (x[6:], y[6:], mask[6:])], x, y, mask


@pytest.mark.parametrize("kind", ["topk", "batch_topk"])
def test_python_layer_on_real_modules(kind):
    torch.manual_seed(5 if kind == "topk" else 6)
    sae = (TopKSAE(D, H, k=K) if kind == "topk" else BatchTopKSAE(D, H, k=K, max_k_per_row=16)).to(DEV)
    batches, x, y, mask = utterances(12)
    sae.train()
    lag = 1
    reg = collect_regression(sae, batches, C_PY, lag=lag, device=DEV)
    assert sae.training and isinstance(reg, SparseRegression) and reg.n_cols == H
    # the oracle on the module's own code, batch by batch as the collection made its calls
    sae.eval()
    G, MX, gb, n = None, None, None, 0
    with torch.no_grad():
        for xb, yb, mb in batches:
            v, i = sae.encode_compact(xb.to(DEV))
            kk = v.shape[-1]
            code = (v.reshape(-1, kk).float().cpu().numpy(), i.reshape(-1, kk).int().cpu().numpy())
            seg = np.where(mb.reshape(-1).numpy() != 0, np.repeat(np.arange(xb.shape[0]), T_PY), -1).astype(np.int32)
            E, used = RG.shifted_targets(seg, yb.reshape(-1, C_PY).numpy(), seg.size, lag)
            ent = PB.entries(code, np.where(used, seg, -1), H)
            pl = PB.plan(ent, H)
            G = RG.gram(pl, ent, seg.size, H, G=G)
            MX, gb = PB.backward(pl, E, C_PY + 1, MX, gb)
            n += int(used.sum())
    same_bits(torch.triu(reg._G).cpu().numpy(), np.triu(G))
    same_bits(reg._MX.cpu().numpy(), MX)
    same_bits(reg._sums.cpu().numpy(), gb)
    assert reg.n_frames == n > 250
    # merge: two shards against one tracker fed both.  The frames are an integer and agree exactly; a float64 cell is a sum
    # of at most four partials added in another order: 4 eps of the sum of the terms' magnitudes
    a = collect_regression(sae, batches[:2], C_PY, lag=lag, device=DEV)
    b = collect_regression(sae, batches[2:], C_PY, lag=lag, device=DEV)
    a.merge(b)
    assert a.n_frames == reg.n_frames
    np.testing.assert_allclose(a._G.cpu().numpy(), reg._G.cpu().numpy(), rtol=4 * EPS, atol=0)  # (positive terms)
    Xall = np.abs(reg.gram().cpu().numpy()).max()
    np.testing.assert_allclose(a._MX.cpu().numpy(), reg._MX.cpu().numpy(), rtol=0,
                               atol=4 * EPS * n * np.sqrt(Xall) * float(y[torch.isfinite(y)].abs().max()))
    np.testing.assert_allclose(a._sums.cpu().numpy(), reg._sums.cpu().numpy(), rtol=0, atol=4 * EPS * n * float(y[torch.isfinite(y)].abs().max()))
    np.testing.assert_allclose(a._syy.cpu().numpy(), reg._syy.cpu().numpy(), rtol=n * EPS)
    with pytest.raises(ValueError):
        a.merge(SparseRegression(H, C_PY, lag=0, device=DEV))
    # save / load
    with tempfile.TemporaryDirectory(prefix="wsae_regress_") as d:
        reg.save(f"{d}/r.pt")
        back = SparseRegression.load(f"{d}/r.pt", device=DEV)
    for name in ("_G", "_MX", "_sums", "_syy"):
        assert torch.equal(getattr(back, name), getattr(reg, name))
    assert (back.hidden, back.n_targets, back.lag, back.n_frames) == (H, C_PY, lag, n)
    # a fit of the loaded state, evaluated and predicted on the first batch in both forms
    fit = back.fit(1e-2)
    assert torch.equal(fit.weight, reg.fit(1e-2).weight) and bool(torch.isfinite(fit.r2_train).all())
    xb, yb, mb = batches[0]
    with torch.no_grad():
        v, i = sae.encode_compact(xb.to(DEV))
    v3, i3 = v.reshape(5, T_PY, -1), i.reshape(5, T_PY, -1)
    rep = back.evaluate(fit, (v3, i3), yb.to(DEV), mb.to(DEV))
    seg = torch.where(mb.reshape(-1) != 0, torch.arange(5).repeat_interleave(T_PY), torch.tensor(-1)).to(DEV)
    flat = back.evaluate(fit, (v3.reshape(-1, v3.shape[-1]), i3.reshape(-1, v3.shape[-1])), yb.reshape(-1, C_PY).to(DEV), segments=seg)
    assert rep.n_frames == flat.n_frames > 100 and torch.equal(rep.mse, flat.mse) and torch.equal(rep.r2, flat.r2)
    pred = back.predict(fit, (v3, i3), mb.to(DEV))
    on = (mb != 0).to(DEV)
    assert pred.shape == (5, T_PY, C_PY) and not pred[~on].any() and bool(pred[on].any())
    assert torch.equal(back.predict(fit, (v3.reshape(-1, v3.shape[-1]), i3.reshape(-1, v3.shape[-1]))).reshape(5, T_PY, C_PY)[on],
                       pred[on])
    # errors
    with pytest.raises(N.WsaeError):
        reg.update((v3, i3), yb, mb.to(DEV))  # targets on the host
    with pytest.raises(ValueError):
        reg.update((v3, i3), yb[..., :2].to(DEV))
    with pytest.raises(ValueError):
        reg.update((v3, i3), yb.to(DEV).long())
    with pytest.raises(ValueError):
        reg.update((v3.reshape(-1, v3.shape[-1]), i3.reshape(-1, v3.shape[-1])), yb.reshape(-1, C_PY).to(DEV))  # flat: segments
    with pytest.raises(ValueError):
        reg.top_weights(fit, C_PY)
    with pytest.raises(TypeError):
        collect_regression(ReLUSAE(D, H).to(DEV), batches, C_PY, device=DEV)
