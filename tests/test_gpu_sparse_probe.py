"""Sparse linear probes on the MI355X against the numpy oracle of tests/probe_oracle.py: the plan and the backward
product bit for bit, the forward product within four times the deviation of its float32 mirror from float64 (plus four
float32 ulps of 1), its integer outputs exactly, the properties that make them independent of batching and call order,
the fit against a float64 Newton fit, and the Python layer on real modules.  The inputs and the conditions that keep
them from being degenerate are checked on the CPU in tests/test_sparse_probe.py.

Observed on the MI355X: over the 82 forward comparisons of this file the device's deviation from float64 is at most 1.40
times (d + 2^-23), d being the mirror's deviation from float64 on the same inputs (2e-7 .. 4.2e-6)."""

from __future__ import annotations

import re
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch

import probe_oracle as PB
import runs_oracle as RO
from whisper_sae import _native as N
from whisper_sae.analysis import (ProbeCurve, ProbeData, ProbeFit, ProbeReport, SparseProbe, collect_probe_data,
                                  sparse_probe_curve, utterance_split)
from whisper_sae.sae.model import BatchTopKSAE, ReLUSAE, TopKSAE

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
JUNK = 0x5a5a5a5
FJUNK = -float(2 ** 39)  # (exact in float32)
TAIL = 3  # junk elements / rows behind every output
EPS = 2.0 ** -23
SOURCE = Path(__file__).resolve().parents[1] / "whisper-sae_amd" / "csrc" / "wsae_probe.hip"


def kernel_constant(name):
    return int(re.search(r"constexpr int " + name + r" = (\d+);", SOURCE.read_text()).group(1))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def stream():
    return torch.cuda.current_stream().cuda_stream


def workspace(need):
    assert need >= 0
    return torch.full((need + 64,), 0xAB, dtype=torch.uint8, device=DEV)  # (arbitrary contents on entry)


class Code:
    """A code, its segments and its column map on the device."""

    def __init__(self, code, seg, hidden, col_of=None, P=None):
        self.v, self.i = dev(np.asarray(code[0], np.float32)), dev(np.asarray(code[1], np.int32))
        self.seg = None if seg is None else dev(np.asarray(seg, np.int32))
        self.col_of = None if col_of is None else dev(np.asarray(col_of, np.int32))
        self.rows, self.k = self.v.shape
        self.hidden, self.P = hidden, hidden if P is None else P


def run_plan(c, cap=None, n_rows=None):
    """``wsae_probe_plan`` -> (col_ptr, t_row, t_val, nnz) as numpy; junk behind every output must survive, and a 0xAB
    workspace must be intact past the size queried."""
    n_rows = c.rows if n_rows is None else n_rows
    cap = c.rows * c.k if cap is None else cap
    col_ptr = torch.full((c.P + 1 + TAIL,), JUNK, dtype=torch.int64, device=DEV)
    t_row = torch.full((cap + TAIL,), JUNK, dtype=torch.int32, device=DEV)
    t_val = torch.full((cap + TAIL,), FJUNK, dtype=torch.float32, device=DEV)
    nnz = torch.full((1 + TAIL,), JUNK, dtype=torch.int64, device=DEV)
    lib = N.lib()
    need = lib.wsae_probe_plan_workspace_bytes(n_rows, c.k, c.hidden, c.P)
    ws = workspace(need)
    N.check(lib.wsae_probe_plan(c.v.data_ptr(), c.i.data_ptr(), c.k, c.hidden, N.ptr(c.seg), n_rows, N.ptr(c.col_of), c.P,
                                col_ptr.data_ptr(), t_row.data_ptr(), t_val.data_ptr(), cap, nnz.data_ptr(), ws.data_ptr(), need,
                                stream()), "wsae_probe_plan")
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xAB).all())
    assert bool((col_ptr[c.P + 1:] == JUNK).all()) and bool((nnz[1:] == JUNK).all())
    assert bool((t_row[cap:] == JUNK).all()) and bool((t_val[cap:] == FJUNK).all())
    return col_ptr[:c.P + 1].cpu().numpy(), t_row[:cap].cpu().numpy(), t_val[:cap].cpu().numpy(), int(nnz[0])


def same_plan(got, want):
    col_ptr, t_row, t_val, nnz = got
    n = int(want[0][-1])
    assert nnz == n and col_ptr.dtype == np.int64 and np.array_equal(col_ptr, want[0])
    assert np.array_equal(t_row[:n], want[1]) and np.array_equal(t_val[:n].view(np.int32), want[2].view(np.int32))


class Forward:
    """State and outputs of ``wsae_probe_forward`` with junk around them."""

    def __init__(self, C, lde=None, with_err=True, with_loss=True, with_confusion=True):
        self.C, self.lde = C, C + PB.LDE_PAD if lde is None else lde
        self.counters = [torch.zeros(1 + TAIL, dtype=torch.int64, device=DEV) for _ in range(3)]
        for t in self.counters:
            t[1:] = JUNK
        self.confusion = torch.zeros(C + TAIL, C, dtype=torch.int64, device=DEV) if with_confusion else None
        if with_confusion:
            self.confusion[C:] = JUNK
        self.with_err, self.with_loss = with_err, with_loss
        self.err, self.row_loss = [], []

    def run(self, c, labels, lag, W, bias, cw=None, n_rows=None):
        n_rows = c.rows if n_rows is None else n_rows
        lab = dev(np.asarray(labels, np.int32))
        Wd, bd, cwd = dev(W), dev(bias), None if cw is None else dev(cw)
        err = torch.full((c.rows + TAIL, self.lde), FJUNK, dtype=torch.float32, device=DEV) if self.with_err else None
        row_loss = torch.full((c.rows + TAIL,), FJUNK, dtype=torch.float32, device=DEV) if self.with_loss else None
        lib = N.lib()
        need = lib.wsae_probe_forward_workspace_bytes(n_rows, c.k, c.hidden, c.P, self.C, lag)
        ws = workspace(need)
        N.check(lib.wsae_probe_forward(c.v.data_ptr(), c.i.data_ptr(), c.k, c.hidden, N.ptr(c.seg), lab.data_ptr(), n_rows, lag,
                                       self.C, N.ptr(c.col_of), c.P, Wd.data_ptr(), W.shape[1], bd.data_ptr(), N.ptr(cwd),
                                       N.ptr(err), self.lde, N.ptr(row_loss), self.counters[0].data_ptr(),
                                       self.counters[1].data_ptr(), self.counters[2].data_ptr(), N.ptr(self.confusion),
                                       ws.data_ptr(), need, stream()), "wsae_probe_forward")
        torch.cuda.synchronize()
        assert bool((ws[need:] == 0xAB).all())
        if n_rows == 0:
            assert err is None or bool((err == FJUNK).all())
            return self
        if err is not None:
            assert bool((err[c.rows:] == FJUNK).all()) and bool((err[:, self.C:] == FJUNK).all())  # columns from C on: never written
            self.err.append(err[:c.rows, :self.C].cpu().numpy())
        if row_loss is not None:
            assert bool((row_loss[c.rows:] == FJUNK).all())
            self.row_loss.append(row_loss[:c.rows].cpu().numpy())
        return self

    def ints(self):
        assert all(bool((t[1:] == JUNK).all()) for t in self.counters)
        out = {"n_used": int(self.counters[0][0]), "n_correct": int(self.counters[1][0]), "loss_q": int(self.counters[2][0])}
        if self.confusion is not None:
            assert bool((self.confusion[self.C:] == JUNK).all())
            out["confusion"] = self.confusion[:self.C].cpu().numpy()
        return out


def run_backward(pl, cap, P, err, C, n_rows, gW0=None, gb0=None):
    """``wsae_probe_backward`` from the stored ``gW0`` / ``gb0`` (None: zeros) -> (gW, gb) as numpy."""
    col_ptr, t_row, t_val = (dev(a) for a in pl)
    err_d, lde = dev(err), err.shape[1]
    gW = torch.full((P + TAIL, C), float(FJUNK), dtype=torch.float64, device=DEV)
    gb = torch.full((C + TAIL,), float(FJUNK), dtype=torch.float64, device=DEV)
    gW[:P] = 0 if gW0 is None else dev(gW0)
    gb[:C] = 0 if gb0 is None else dev(gb0)
    lib = N.lib()
    need = lib.wsae_probe_backward_workspace_bytes(n_rows, P, C, cap)
    ws = workspace(need)
    N.check(lib.wsae_probe_backward(col_ptr.data_ptr(), N.ptr(t_row), N.ptr(t_val), cap, P, err_d.data_ptr(), lde, C, n_rows,
                                    gW.data_ptr(), gb.data_ptr(), ws.data_ptr(), need, stream()), "wsae_probe_backward")
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xAB).all()) and bool((gW[P:] == FJUNK).all()) and bool((gb[C:] == FJUNK).all())
    return gW[:P].cpu().numpy(), gb[:C].cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    view = np.int64 if a.dtype == np.float64 else np.int32
    assert np.array_equal(a.view(view), b.view(view)), np.argwhere(a.view(view) != b.view(view))[:5]


@pytest.fixture(scope="module")
def general():
    return PB.general_case()


def check_forward(fw, ref, mir, y, C, exact_argmax):
    """The forward's outputs of one call against the float64 reference and the mirror; -> the ratio observed."""
    err, row_loss = fw.err[-1], fw.row_loss[-1]
    d = max(np.abs(mir["err"] - ref["err"]).max(), np.abs(mir["row_loss"] - ref["row_loss"]).max())
    dev_err = max(np.abs(err - ref["err"]).max(), np.abs(row_loss - ref["row_loss"]).max())
    print(f"forward: d = {d:.3e}, device deviation = {dev_err:.3e}, ratio to (d + 2^-23) = {dev_err / (d + EPS):.3f}")
    assert dev_err <= 4 * d + 4 * EPS
    used = ref["used"]
    assert (err[~used] == 0).all() and (row_loss[~used] == 0).all() and not np.signbit(err[~used]).any()  # exact zeros
    got = fw.ints()
    assert got["n_used"] == int(used.sum())
    assert got["loss_q"] == PB.loss_q(row_loss)
    if exact_argmax:
        assert got["n_correct"] == int((ref["argmax"] == y)[used].sum())
        assert np.array_equal(got["confusion"], PB.confusion(y, ref["argmax"], C))
    return dev_err / (d + EPS)


# ---- 1: the plan --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("columns", PB.COLUMNS)
def test_plan_equals_the_oracle(general, columns):
    code, seg = general
    col_of, P = PB.col_map(columns)
    for s in (seg, None):
        want = PB.plan(PB.entries(code, s, PB.HIDDEN, col_of), P)
        same_plan(run_plan(Code(code, s, PB.HIDDEN, col_of, P)), want)
    # cap too small: nnz and col_ptr are right, the first cap slots are those of the full plan, nothing behind them
    want = PB.plan(PB.entries(code, seg, PB.HIDDEN, col_of), P)
    n = int(want[0][-1])
    for cap in (n - 1, n // 3, 0):
        col_ptr, t_row, t_val, nnz = run_plan(Code(code, seg, PB.HIDDEN, col_of, P), cap=cap)  # (the junk behind cap is checked there)
        assert nnz == n and np.array_equal(col_ptr, want[0])
        assert np.array_equal(t_row, want[1][:cap]) and np.array_equal(t_val, want[2][:cap])
    same_plan(run_plan(Code(code, seg, PB.HIDDEN, col_of, P), cap=n), want)  # exactly enough


# ---- 2: the backward product, on an arbitrary err -----------------------------------------------------------------------------
@pytest.mark.parametrize("C,columns", [(1, "all"), (3, "all"), (41, "all"), (70, "all"), (3, "window"), (3, "subset"),
                                       (70, "subset")])
def test_backward_equals_the_oracle(general, C, columns):
    code, seg = general
    col_of, P = PB.col_map(columns)
    pl = PB.plan(PB.entries(code, seg, PB.HIDDEN, col_of), P)
    cap = int(pl[0][-1])
    rng = np.random.default_rng(40 + C)
    lde = C + PB.LDE_PAD
    err = np.full((PB.ROWS, lde), PB.JUNK, np.float32)
    err[:, :C] = rng.standard_normal((PB.ROWS, C)).astype(np.float32) * np.exp(rng.standard_normal((PB.ROWS, 1))).astype(np.float32)
    gW, gb = run_backward(pl, cap, P, err, C, PB.ROWS)
    wW, wb = PB.backward(pl, err, C)
    same_bits(gW, wW)
    same_bits(gb, wb)
    # from stored values that are not zero, and a second shard after the first
    gW0, gb0 = rng.standard_normal((P, C)), rng.standard_normal(C)
    gW1, gb1 = run_backward(pl, cap, P, err, C, PB.ROWS, gW0, gb0)
    wW1, wb1 = PB.backward(pl, err, C, gW0, gb0)
    same_bits(gW1, wW1)
    same_bits(gb1, wb1)
    half = 301  # the second shard: the rows from here on, as a call of their own
    ent2 = PB.entries((code[0][half:], code[1][half:]), seg[half:], PB.HIDDEN, col_of)
    pl2 = PB.plan(ent2, P)
    gW2, gb2 = run_backward(pl2, int(pl2[0][-1]), P, err[half:], C, PB.ROWS - half, gW1, gb1)
    wW2, wb2 = PB.backward(pl2, err[half:], C, wW1, wb1)
    same_bits(gW2, wW2)
    same_bits(gb2, wb2)
    # another lde: the same bits
    wide = np.full((PB.ROWS, C + 29), -PB.JUNK, np.float32)
    wide[:, :C] = err[:, :C]
    gW3, gb3 = run_backward(pl, cap, P, wide, C, PB.ROWS)
    same_bits(gW3, gW)
    same_bits(gb3, gb)


# ---- 3: the forward product ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lag", PB.LAGS, ids=lambda l: f"lag{l}")
@pytest.mark.parametrize("columns", PB.COLUMNS)
@pytest.mark.parametrize("C", PB.CLASSES, ids=lambda c: f"C{c}")
def test_forward_against_the_mirror(general, C, columns, lag):
    code, seg = general
    col_of, P = PB.col_map(columns)
    labels = PB.labels_for(C)
    W, b, cw = PB.parameters(P, C, C)  # (ldw = C + 3, junk behind the classes)
    for s, weights in ((seg, cw), (None, None)):
        ent = PB.entries(code, s, PB.HIDDEN, col_of)
        y = PB.row_labels(s, labels, PB.ROWS, C, lag)
        ref, mir = PB.forward64(ent, y, W, b, C, weights), PB.mirror32(code, ent, y, W, b, C, weights)
        fw = Forward(C).run(Code(code, s, PB.HIDDEN, col_of, P), labels, lag, W, b, weights)
        # lag 0 with seg and class weights: the accuracy inputs, on which the CPU tests show every margin to hold
        check_forward(fw, ref, mir, y, C, exact_argmax=lag == 0 and s is not None)
    # every nullable output left out: the counters alone
    only = Forward(C, with_err=False, with_loss=False, with_confusion=False).run(Code(code, None, PB.HIDDEN, col_of, P), labels,
                                                                               lag, W, b, None).ints()
    full = fw.ints()
    assert only == {name: full[name] for name in ("n_used", "n_correct", "loss_q")}


@pytest.mark.parametrize("k,C", [(1, 5), (64, 5), (65, 200), (128, 1024)])
def test_width_edges(k, C):
    """Rows of one entry, of one full wave, of one more and of the widest code (two entries per lane); 4 and 16 class tiles
    per lane."""
    rng = np.random.default_rng(50 + k)
    hidden, rows = 300, 70
    code = RO.spoil(rng, RO.persistent_code(rng, rows, k, hidden), hidden)
    seg = (np.arange(rows) // 25).astype(np.int32)
    seg[rng.random(rows) < 0.05] = -1
    labels = rng.integers(-1, C, rows).astype(np.int32)
    for col_of, P in ((None, hidden), (np.where(np.arange(hidden) % 3 == 0, np.arange(hidden) // 3, -1).astype(np.int32), 100)):
        ent = PB.entries(code, seg, hidden, col_of)
        pl = PB.plan(ent, P)
        c = Code(code, seg, hidden, col_of, P)
        same_plan(run_plan(c), pl)
        W, b, cw = PB.parameters(P, C, k, scale=0.2)
        y = PB.row_labels(seg, labels, rows, C, 1)
        ref, mir = PB.forward64(ent, y, W, b, C, cw), PB.mirror32(code, ent, y, W, b, C, cw)
        fw = Forward(C).run(c, labels, 1, W, b, cw)
        check_forward(fw, ref, mir, y, C, exact_argmax=False)
        err = np.ascontiguousarray(fw.err[-1])
        gW, gb = run_backward(pl, int(pl[0][-1]), P, err, C, rows)
        wW, wb = PB.backward(pl, err, C)
        same_bits(gW, wW)
        same_bits(gb, wb)


# ---- 4: batching and call order -----------------------------------------------------------------------------------------------
def test_batching_and_call_order_do_not_matter(general):
    code, seg = general
    C, lag = 41, -2
    labels = PB.labels_for(C)
    col_of, P = PB.col_map("window")
    W, b, cw = PB.parameters(P, C, 9)
    whole = Forward(C).run(Code(code, seg, PB.HIDDEN, col_of, P), labels, lag, W, b, cw)
    cuts = [(0, 60), (60, 290), (290, PB.ROWS)]  # whole utterances
    assert all(not set(seg[:a][seg[:a] >= 0]) & set(seg[a:][seg[a:] >= 0]) for a, _ in cuts[1:])
    for order in (cuts, cuts[::-1]):
        fw = Forward(C)
        for a, e in order:
            fw.run(Code((code[0][a:e], code[1][a:e]), seg[a:e], PB.HIDDEN, col_of, P), labels[a:e], lag, W, b, cw)
        rows = sorted(zip(order, fw.err, fw.row_loss), key=lambda t: t[0][0])
        same_bits(np.concatenate([r[1] for r in rows]), whole.err[0])
        same_bits(np.concatenate([r[2] for r in rows]), whole.row_loss[0])
        got, want = fw.ints(), whole.ints()
        assert np.array_equal(got.pop("confusion"), want.pop("confusion")) and got == want and got["n_used"] > 400


# ---- 5: columns that span chunks, and more rows than one pass of the grid -----------------------------------------------------
def test_columns_that_span_chunks():
    code, seg, labels, C = PB.chunk_case()
    rows = seg.size
    assert rows == 2 * PB.CHUNK + 100
    ent = PB.entries(code, seg, PB.HIDDEN)
    pl = PB.plan(ent, PB.HIDDEN)
    c = Code(code, seg, PB.HIDDEN)
    same_plan(run_plan(c), pl)
    W, b, cw = PB.parameters(PB.HIDDEN, C, 77)
    y = PB.row_labels(seg, labels, rows, C, 0)
    fw = Forward(C).run(c, labels, 0, W, b, cw)
    check_forward(fw, PB.forward64(ent, y, W, b, C, cw), PB.mirror32(code, ent, y, W, b, C, cw), y, C, exact_argmax=False)
    err = np.ascontiguousarray(fw.err[0])
    gW0 = np.random.default_rng(5).standard_normal((PB.HIDDEN, C))
    gW, gb = run_backward(pl, int(pl[0][-1]), PB.HIDDEN, err, C, rows, gW0, None)
    wW, wb = PB.backward(pl, err, C, gW0, None)
    same_bits(gW, wW)
    same_bits(gb, wb)


def test_more_rows_than_one_pass_of_the_grid():
    rows = kernel_constant("PB_FWD_MAX_BLOCKS") * (kernel_constant("PB_FWD_BLOCK") // 64) + 301
    code, seg, labels, C = PB.long_case(rows)
    col_of, P = PB.col_map("window")
    ent = PB.entries(code, seg, PB.HIDDEN, col_of)
    c = Code(code, seg, PB.HIDDEN, col_of, P)
    same_plan(run_plan(c), PB.plan(ent, P))
    W, b, cw = PB.parameters(P, C, 78)
    y = PB.row_labels(seg, labels, rows, C, 3)
    fw = Forward(C).run(c, labels, 3, W, b, cw)
    check_forward(fw, PB.forward64(ent, y, W, b, C, cw), PB.mirror32(code, ent, y, W, b, C, cw), y, C, exact_argmax=False)


# ---- 6: no rows ---------------------------------------------------------------------------------------------------------------
def test_no_rows_touch_nothing(general):
    code, seg = general
    c = Code(code, seg, PB.HIDDEN)
    col_ptr, t_row, t_val, nnz = run_plan(c, n_rows=0)
    assert (col_ptr == JUNK).all() and (t_row == JUNK).all() and nnz == JUNK
    nnz = torch.zeros(1, dtype=torch.int64, device=DEV)
    W, b, _ = PB.parameters(PB.HIDDEN, 3, 1)
    fw = Forward(3).run(c, PB.labels_for(3), 0, W, b, None, n_rows=0)
    assert fw.ints()["n_used"] == 0 and fw.ints()["loss_q"] == 0 and not fw.ints()["confusion"].any()
    pl = PB.plan(PB.entries(code, seg, PB.HIDDEN), PB.HIDDEN)
    gW0 = np.random.default_rng(6).standard_normal((PB.HIDDEN, 3))
    gW, gb = run_backward(pl, int(pl[0][-1]), PB.HIDDEN, np.ones((PB.ROWS, 3), np.float32), 3, 0, gW0, None)
    same_bits(gW, gW0)
    assert not gb.any()
    lib = N.lib()
    assert lib.wsae_probe_plan_workspace_bytes(10, 129, 96, 96) == -1 and lib.wsae_probe_plan_workspace_bytes(10, 8, 96, 97) == -1
    assert lib.wsae_probe_forward_workspace_bytes(10, 8, 96, 96, 1025, 0) == -1
    assert lib.wsae_probe_forward_workspace_bytes(10, 8, 96, 96, 3, 1025) == -1
    assert lib.wsae_probe_backward_workspace_bytes(10, 96, 0, 80) == -1 and lib.wsae_probe_backward_workspace_bytes(-1, 96, 3, 80) == -1
    rc = lib.wsae_probe_forward(c.v.data_ptr(), c.i.data_ptr(), c.k, c.hidden, None, c.i.data_ptr(), 10, 0, 3, None, 11, c.v.data_ptr(),
                                3, c.v.data_ptr(), None, None, 3, None, nnz.data_ptr(), nnz.data_ptr(), nnz.data_ptr(), None, None, 0,
                                stream())
    assert rc != 0 and "without col_of" in N.last_error()


# ---- 7: the fit ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("features,weighted", [(None, False), (None, True), (PB.FIT_FEATURES, False)],
                         ids=["all", "class_weight", "subset"])
def test_fit_reaches_the_reference_optimum(features, weighted):
    code, seg, labels = PB.fit_case()
    C, l2, tol = PB.FIT_C, PB.FIT_L2, 1e-5
    cw = np.array([0.5, 1.0, 2.0], np.float32) if weighted else None
    col_of, P = None, PB.FIT_HIDDEN
    if features is not None:
        col_of = np.full(PB.FIT_HIDDEN, -1, np.int32)
        col_of[list(features)] = np.arange(len(features))
        P = len(features)
    fits = []
    for _ in range(2):
        probe = SparseProbe(PB.FIT_HIDDEN, C, features=None if features is None else torch.tensor(features), l2=l2,
                            class_weight=None if cw is None else torch.from_numpy(cw), device=DEV)
        cut = 300  # two shards of whole utterances
        for a, e in ((0, cut), (cut, PB.FIT_ROWS)):
            probe.add_data((dev(code[0][a:e]), dev(code[1][a:e])), dev(labels[a:e]), segments=dev(seg[a:e]))
        fit = probe.fit(max_iter=200, tolerance_grad=tol)
        assert isinstance(fit, ProbeFit) and probe.n_shards == 2
        fits.append((fit, probe.weight.cpu().numpy().copy(), probe.bias.cpu().numpy().copy()))
    (fit, W, b), (fit2, W2, b2) = fits
    same_bits(W, W2)  # two fits of the same data: bit-identical
    same_bits(b, b2)
    assert fit == fit2 and fit.converged and fit.grad_norm <= tol and fit.iterations >= 3
    # the float64 gradient at the device's parameters
    ent = PB.entries(code, seg, PB.FIT_HIDDEN, col_of)
    y = PB.row_labels(seg, labels, PB.FIT_ROWS, C, 0)
    X = PB.dense_design(ent, PB.FIT_ROWS, P)
    theta = np.concatenate([W.reshape(-1), b])
    loss64, g64 = PB.objective64(X, y, theta, C, l2, cw)
    W32, b32 = W.astype(np.float32), b.astype(np.float32)
    mir = PB.mirror32(code, ent, y, W32, b32, C, cw)
    n = int((y >= 0).sum())
    mW, mb = PB.backward(PB.plan(ent, P), mir["err"], C)
    g_mirror = np.concatenate([(mW / n + l2 * W).reshape(-1), mb / n])
    g = np.linalg.norm(g_mirror - g64)
    print(f"fit: |grad64| = {np.linalg.norm(g64):.3e}, mirror deviation g = {g:.3e}, reported {fit.grad_norm:.3e}, "
          f"{fit.iterations} iterations, {fit.evaluations} evaluations")
    assert np.linalg.norm(g64) <= tol + 4 * g
    assert abs(fit.loss - loss64) < 1e-6
    # strong convexity: the distance to the optimum is at most the gradient over l2
    best = PB.fit64(X, y, C, l2, cw)
    assert np.linalg.norm(theta - best) <= (tol + 4 * g) / l2
    # the first evaluation, at zero, in the kernel's own terms: the device gradient against the chunked oracle
    probe = SparseProbe(PB.FIT_HIDDEN, C, features=None if features is None else torch.tensor(features), l2=l2,
                        class_weight=None if cw is None else torch.from_numpy(cw), device=DEV)
    probe.add_data((dev(code[0]), dev(code[1])), dev(labels), segments=dev(seg))
    loss0, gW0, gb0 = probe.loss_and_grad()
    zero = PB.mirror32(code, ent, y, np.zeros((P, C), np.float32), np.zeros(C, np.float32), C, cw)
    np.testing.assert_allclose(float(loss0), PB.loss_q(zero["row_loss"]) / 2 ** 20 / n, rtol=0, atol=1e-6)
    oW, ob = PB.backward(PB.plan(ent, P), zero["err"], C)
    np.testing.assert_allclose(gW0.cpu().numpy(), oW / n, rtol=0, atol=1e-6)
    np.testing.assert_allclose(gb0.cpu().numpy(), ob / n, rtol=0, atol=1e-6)


def test_a_dense_subset_is_planned_twice():
    """``add_data`` guesses the size of the plan from the subset's share of the dictionary; here every row holds all of the
    subset, the plan names more entries than the guess and is transposed again at the true count."""
    code, col_of, P = PB.dense_subset_case()
    C, l2 = 3, 1e-2
    rows, k = PB.DENSE_UTT * PB.DENSE_T, PB.DENSE_K
    flat = (code[0].reshape(rows, k), code[1].reshape(rows, k))
    seg = np.repeat(np.arange(PB.DENSE_UTT), PB.DENSE_T).astype(np.int32)
    rng = np.random.default_rng(61)
    labels = rng.integers(-1, C, rows).astype(np.int32)
    ent = PB.entries(flat, seg, PB.DENSE_HIDDEN, col_of)
    pl = PB.plan(ent, P)
    nnz, guess = int(pl[0][-1]), 1024 + 2 * rows * k * P // PB.DENSE_HIDDEN
    assert guess == 1280 and nnz == rows * k == 16384 > guess  # the precondition, from the oracle's plan
    probe = SparseProbe(PB.DENSE_HIDDEN, C, features=torch.tensor(PB.DENSE_FEATURES), l2=l2, device=DEV)
    probe.add_data((dev(code[0]), dev(code[1])), dev(labels.reshape(PB.DENSE_UTT, PB.DENSE_T)))
    sh = probe._shards[0]
    assert probe.n_shards == 1 and sh["nnz"] == nnz and sh["t_row"].numel() == nnz == sh["t_val"].numel()
    same_plan((sh["col_ptr"].cpu().numpy(), sh["t_row"].cpu().numpy(), sh["t_val"].cpu().numpy(), sh["nnz"]), pl)
    loss, gW, gb = probe.loss_and_grad()
    y = PB.row_labels(seg, labels, rows, C, 0)
    n = int((y >= 0).sum())
    zero = PB.mirror32(flat, ent, y, np.zeros((P, C), np.float32), np.zeros(C, np.float32), C)
    np.testing.assert_allclose(float(loss), PB.loss_q(zero["row_loss"]) / 2 ** 20 / n, rtol=0, atol=1e-6)
    oW, ob = PB.backward(pl, zero["err"], C)
    np.testing.assert_allclose(gW.cpu().numpy(), oW / n, rtol=0, atol=1e-6)
    np.testing.assert_allclose(gb.cpu().numpy(), ob / n, rtol=0, atol=1e-6)
    assert n > 1000 and np.abs(oW / n).max() > 1e-3  # (the gradient is not the trivial one)


# ---- 8: the Python layer on real modules --------------------------------------------------------------------------------------
D, H, K, UTT, T, C_PY = 32, 128, 8, 12, 40, 4


def utterances(seed):
    """12 utterances of 40 frames in three batches with a frame mask; a frame repeats one of 14 prototypes for a stretch
    and its label is the prototype's number modulo the classes."""
    gen = torch.Generator().manual_seed(seed)
    proto = torch.randn(14, D, generator=gen)
    hold = (torch.rand(UTT, T, generator=gen) < 0.3).cumsum(1)
    which = torch.randint(0, 14, (UTT, T + 1), generator=gen).gather(1, hold)
    x = proto[which] * torch.exp(0.3 * torch.randn(UTT, T, 1, generator=gen)) + 0.05 * torch.randn(UTT, T, D, generator=gen)
    labels = which % C_PY
    labels[0, 3], labels[5, 7] = -1, C_PY + 2
    mask = torch.ones(UTT, T)
    for u in range(UTT):
        mask[u, 28 + (u % 5) * 3:] = 0
    mask[3, 10] = 0
    return [(x[:5], labels[:5], mask[:5]), (x[5:6], labels[5:6], mask[5:6]), (x[6:], labels[6:], mask[6:])], mask, labels


@pytest.mark.parametrize("kind", ["topk", "batch_topk"])
def test_python_layer_on_real_modules(kind):
    torch.manual_seed(3 if kind == "topk" else 4)
    sae = (TopKSAE(D, H, k=K) if kind == "topk" else BatchTopKSAE(D, H, k=K, max_k_per_row=16)).to(DEV)
    batches, mask, labels = utterances(11)
    sae.train()
    data = collect_probe_data(sae, batches, device=DEV)
    assert sae.training and isinstance(data, ProbeData) and data.n_utt == UTT and data.labels.shape == (UTT * T,)
    want_seg = np.where(mask.reshape(-1).numpy() != 0, np.repeat(np.arange(UTT), T), -1)
    assert np.array_equal(data.segments.cpu().numpy(), want_seg) and torch.equal(data.labels.cpu(), labels.reshape(-1))
    train, test = utterance_split(UTT, 0.25, seed=1)
    assert int(test.sum()) == 3
    l2, tol = 1e-2, 1e-5
    probe = SparseProbe(H, C_PY, l2=l2, device=DEV)
    probe.add_data(*data.subset(train))
    fit = probe.fit(tolerance_grad=tol)
    assert fit.converged and fit.grad_norm <= tol
    # the fitted objective against the float64 oracle on the same code
    code = (data.code[0].cpu().numpy(), data.code[1].cpu().numpy())
    seg_train = np.where(train.numpy()[np.maximum(want_seg, 0)] & (want_seg >= 0), want_seg, -1)
    ent = PB.entries(code, seg_train, H)
    y = PB.row_labels(seg_train, labels.reshape(-1).numpy(), UTT * T, C_PY, 0)
    X = PB.dense_design(ent, UTT * T, H)
    theta = np.concatenate([probe.weight.cpu().numpy().reshape(-1), probe.bias.cpu().numpy()])
    loss64, g64 = PB.objective64(X, y, theta, C_PY, l2)
    assert abs(loss64 - fit.loss) < 1e-6 and np.linalg.norm(g64) < 2 * tol
    # evaluate: the training frames are fitted well, the report is consistent, the held-out utterances are other frames
    rep_train, rep_test = probe.evaluate(*data.subset(train)), probe.evaluate(*data.subset(test))
    assert isinstance(rep_test, ProbeReport) and rep_train.n_frames == int((y >= 0).sum())
    ref = PB.forward64(ent, y, probe.weight.cpu().numpy(), probe.bias.cpu().numpy(), C_PY)
    assert abs(rep_train.loss - ref["row_loss"].sum() / rep_train.n_frames) < 1e-5
    assert rep_train.accuracy > 0.6 and rep_train.accuracy == pytest.approx((ref["argmax"] == y)[y >= 0].mean(), abs=0.01)
    assert int(rep_train.confusion.sum()) == rep_train.n_frames and rep_test.n_frames + rep_train.n_frames == int(
        ((want_seg >= 0) & (labels.reshape(-1).numpy() >= 0) & (labels.reshape(-1).numpy() < C_PY)).sum())
    cm = rep_test.confusion.cpu().numpy().astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        np.testing.assert_allclose(rep_test.recall.cpu().numpy(), np.diag(cm) / cm.sum(1), equal_nan=True)
        np.testing.assert_allclose(rep_test.precision.cpu().numpy(), np.diag(cm) / cm.sum(0), equal_nan=True)
        np.testing.assert_allclose(rep_test.f1.cpu().numpy(), 2 * np.diag(cm) / (cm.sum(0) + cm.sum(1)), equal_nan=True)
    assert rep_test.accuracy == pytest.approx(np.trace(cm) / cm.sum())
    # the numbered form gives the same fit as the flat one
    shaped = SparseProbe(H, C_PY, l2=l2, device=DEV)
    v3, i3 = data.code[0].reshape(UTT, T, -1), data.code[1].reshape(UTT, T, -1)
    shaped.add_data((v3, i3), data.labels.reshape(UTT, T), frame_mask=(train[:, None] & (mask != 0)).to(DEV))
    assert shaped.fit(tolerance_grad=tol) == fit and torch.equal(shaped.weight, probe.weight)
    with pytest.raises(ValueError):  # the forms cannot be mixed
        shaped.add_data(data.code, data.labels, segments=data.segments)
    # save / load
    with tempfile.TemporaryDirectory(prefix="wsae_probe_") as d:
        probe.save(f"{d}/p.pt")
        back = SparseProbe.load(f"{d}/p.pt", device=DEV)
    assert torch.equal(back.weight, probe.weight) and torch.equal(back.bias, probe.bias) and back.l2 == l2
    assert back.evaluate(*data.subset(test)).confusion.equal(rep_test.confusion)
    # the k-sparse curve over nested prefixes of a ranking: the fitted training loss does not increase
    fires = np.bincount(ent[2], minlength=H)
    ranking = torch.from_numpy(np.argsort(-fires, kind="stable")[:32].copy())
    curve = sparse_probe_curve(data.subset(train), data.subset(test), ranking, sizes=(1, 2, 4, 8, 16, 32), hidden=H,
                               n_classes=C_PY, l2=l2, device=DEV)
    assert isinstance(curve, ProbeCurve) and curve.sizes == (1, 2, 4, 8, 16, 32) and torch.equal(curve.features, ranking)
    tl = curve.train_loss.numpy()
    assert (np.diff(tl) <= 1e-6).all() and tl[-1] < tl[0] - 0.01 and tl[-1] >= fit.loss - 1e-6
    assert bool(torch.isfinite(curve.test_loss).all()) and 0 <= float(curve.test_accuracy.min()) <= float(curve.test_accuracy.max()) <= 1
    sub = SparseProbe(H, C_PY, features=ranking[:4], l2=l2, device=DEV)
    sub.add_data(*data.subset(train))
    assert sub.fit(tolerance_grad=tol).loss == float(tl[2]) and sub.feature_index.tolist() == ranking[:4].tolist()
    feats, w = sub.top_weights(1, 2)
    assert set(feats.tolist()) <= set(ranking[:4].tolist()) and float(w[0]) >= float(w[1]) and float(w[0]) == float(sub.weight[:, 1].max())
    # errors that need the device
    with pytest.raises(ValueError):
        probe.add_data(data.code, data.labels[:7], segments=data.segments)
    with pytest.raises(ValueError):
        probe.add_data(data.code, data.labels.float(), segments=data.segments)
    with pytest.raises(ValueError):
        probe.add_data(data.code, data.labels)  # a flat code needs segments
    with pytest.raises(ValueError):
        data.subset(train[:5])
    with pytest.raises(TypeError):
        collect_probe_data(ReLUSAE(D, H).to(DEV), batches, device=DEV)


def test_planted_features_carry_the_weights():
    code, labels, planted = PB.planted_case()
    probe = SparseProbe(32, 4, l2=1e-3, device=DEV)
    probe.add_data((dev(code[0])[None], dev(code[1])[None]), dev(labels))
    fit = probe.fit(max_iter=300, tolerance_grad=1e-4)
    assert fit.converged
    for c, f in enumerate(planted):
        feats, w = probe.top_weights(c + 1, 3)
        assert int(feats[0]) == f and float(w[0]) > 1.0 and float(w[0]) > float(w[1])
    rep = probe.evaluate((dev(code[0])[None], dev(code[1])[None]), dev(labels))
    assert rep.accuracy > 0.97 and rep.n_frames == labels.size
