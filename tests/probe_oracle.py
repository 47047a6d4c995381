"""numpy restatement of the sparse linear probes (include/wsae.h, ``wsae_probe_plan`` / ``wsae_probe_forward`` /
``wsae_probe_backward``): the activity, column and label rules; the plan by a stable argsort; the
forward product in float64 and its float32 MIRROR with the kernel's order of operations (one multiply and one add per
entry in ascending entry position, the class reductions as 64 partials and a butterfly); the chunked float64 backward
product as explicit loops, compared with the kernel bit for bit; a float64 reference fit by Newton's method; the inputs
the CPU and the GPU tests share."""

from __future__ import annotations

import re
from pathlib import Path

import numpy as np

import label_oracle as LO
import runs_oracle as RO

HEADER = Path(__file__).resolve().parents[1] / "include" / "wsae.h"
CHUNK = int(re.search(r"#define WSAE_PROBE_CHUNK (\d+)", HEADER.read_text()).group(1))
LOSS_SCALE = 2.0 ** 20


# ---- the rules --------------------------------------------------------------------------------------------------------------
def entries(code, seg, hidden, col_of=None):
    """``(row, position, column, value)`` of every first-active entry whose feature has a column, in ascending row and,
    within a row, ascending entry position.  Active: ``v > 0`` (NaN is not), ``0 <= idx < hidden``, ``seg >= 0``; an index
    repeated within a row counts once, with the value of its first ACTIVE entry.  ``col_of`` int ``[hidden]`` (-1: not in
    the probe; None: the identity)."""
    vals, idx = np.asarray(code[0], np.float32), np.asarray(code[1]).astype(np.int64)
    n_rows = vals.shape[0]
    live = np.ones(n_rows, bool) if seg is None else np.asarray(seg).reshape(-1) >= 0
    with np.errstate(invalid="ignore"):
        act = (vals > 0) & (idx >= 0) & (idx < hidden) & live[:, None]
    r, e = np.nonzero(act)  # ascending row, then ascending position
    f = idx[r, e]
    _, first = np.unique(r * hidden + f, return_index=True)
    first = np.sort(first)
    r, e, f = r[first], e[first], f[first]
    col = f if col_of is None else np.asarray(col_of, np.int64)[f]
    has = col >= 0
    return r[has], e[has], col[has], vals[r[has], e[has]]


def row_labels(seg, labels, n_rows, C, lag):
    """int64 ``[n_rows]``: the label of every row, -1 where the row is dropped (the pair rule of the label association)."""
    return LO.pair_classes(seg, labels, n_rows, C, lag)


def plan(ent, P):
    """``(col_ptr int64 [P + 1], t_row int32, t_val float32)``: the entries grouped by column, ascending row within."""
    r, _, col, v = ent
    order = np.argsort(col, kind="stable")
    col_ptr = np.zeros(P + 1, np.int64)
    col_ptr[1:] = np.cumsum(np.bincount(col, minlength=P))
    return col_ptr, r[order].astype(np.int32), v[order].astype(np.float32)


def plan_dense(code, seg, hidden, col_of, P):
    """The same through the dense ``[n_rows, P]`` matrix the kernels never build: its transpose, row by row."""
    vals, idx = np.asarray(code[0], np.float32), np.asarray(code[1])
    n_rows, k = vals.shape
    dense = np.zeros((n_rows, P), np.float32)
    seen = np.zeros((n_rows, P), bool)
    for r in range(n_rows):
        if seg is not None and seg[r] < 0:
            continue
        done = set()
        for e in range(k):
            f, v = int(idx[r, e]), vals[r, e]
            if not (v > 0) or not 0 <= f < hidden or f in done:
                continue
            done.add(f)
            c = f if col_of is None else int(col_of[f])
            if c >= 0:
                dense[r, c], seen[r, c] = v, True
    col_ptr, rows, out = [0], [], []
    for c in range(P):
        at = np.nonzero(seen[:, c])[0]
        rows.append(at)
        out.append(dense[at, c])
        col_ptr.append(col_ptr[-1] + at.size)
    return np.array(col_ptr, np.int64), np.concatenate(rows).astype(np.int32), np.concatenate(out).astype(np.float32)


# ---- the forward product ----------------------------------------------------------------------------------------------------
def logits64(ent, n_rows, W, bias, C):
    r, _, col, v = ent
    z = np.tile(np.asarray(bias, np.float64)[:C], (n_rows, 1))
    np.add.at(z, r, v.astype(np.float64)[:, None] * np.asarray(W, np.float64)[col, :C])
    return z


def forward64(ent, y, W, bias, C, class_weight=None):
    """float64: ``err [n_rows, C]``, ``row_loss [n_rows]`` (zeros on dropped rows), ``argmax`` (lowest class on ties) and
    ``margin``: the gap between the two largest logits (inf for C == 1)."""
    n_rows = y.size
    z = logits64(ent, n_rows, W, bias, C)
    m = z.max(1, keepdims=True)
    e = np.exp(z - m)
    s = e.sum(1, keepdims=True)
    used = y >= 0
    yc = np.where(used, y, 0)
    w = np.ones(n_rows) if class_weight is None else np.asarray(class_weight, np.float64)[yc]
    onehot = np.arange(C)[None, :] == yc[:, None]
    loss = w * (np.log(s[:, 0]) + m[:, 0] - z[np.arange(n_rows), yc])
    err = w[:, None] * (e / s - onehot)
    top = np.sort(z, 1)
    margin = top[:, -1] - top[:, -2] if C > 1 else np.full(n_rows, np.inf)
    return {"err": np.where(used[:, None], err, 0.0), "row_loss": np.where(used, loss, 0.0), "argmax": z.argmax(1),
            "margin": margin, "used": used}


def _butterfly(x, op):
    """x [n, 64] -> [n]: the kernel's reduction over the lanes, pairs at distance 32, 16, 8, 4, 2, 1."""
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        x = op(x, x[:, lanes ^ off])
    return x[:, 0]


def mirror32(code, ent, y, W, bias, C, class_weight=None):
    """The float32 mirror of ``wsae_probe_forward`` with its order of operations: the logit is a chain from the bias, per
    entry (ascending position) one float32 multiply and one float32 add; maximum and sum over the classes are 64 partials
    (partial l over the classes l, l + 64, ... ascending, from -inf / 0) and a butterfly.  ``exp``, ``log`` and the
    division are numpy's float32 ones.  -> ``err``, ``row_loss`` float32."""
    n_rows, k = np.asarray(code[0]).shape
    r, pos, col, v = ent
    W32 = np.asarray(W, np.float32)
    z = np.tile(np.asarray(bias, np.float32)[:C], (n_rows, 1))
    for j in range(k):
        at = pos == j  # (at most one entry per row and position)
        prod = (v[at].astype(np.float32)[:, None] * W32[col[at], :C]).astype(np.float32)
        z[r[at]] = (z[r[at]] + prod).astype(np.float32)
    tiles = (C + 63) // 64
    zp = np.full((n_rows, tiles * 64), -np.inf, np.float32)
    zp[:, :C] = z
    zp = zp.reshape(n_rows, tiles, 64)
    m = _butterfly(zp.max(1), np.maximum)
    with np.errstate(invalid="ignore"):
        e = np.exp((zp - m[:, None, None]).astype(np.float32)).astype(np.float32)  # (exp(-inf) = 0 on the padding)
    part = np.zeros((n_rows, 64), np.float32)
    for t in range(tiles):
        part = (part + e[:, t]).astype(np.float32)
    s = _butterfly(part, lambda a, b: (a + b).astype(np.float32))
    used = y >= 0
    yc = np.where(used, y, 0)
    w = np.ones(n_rows, np.float32) if class_weight is None else np.asarray(class_weight, np.float32)[yc]
    ly = z[np.arange(n_rows), yc]
    loss = (w * ((np.log(s).astype(np.float32) + m).astype(np.float32) - ly).astype(np.float32)).astype(np.float32)
    p = (e.reshape(n_rows, -1)[:, :C] / s[:, None]).astype(np.float32)
    onehot = (np.arange(C)[None, :] == yc[:, None]).astype(np.float32)
    err = (w[:, None] * (p - onehot).astype(np.float32)).astype(np.float32)
    return {"err": np.where(used[:, None], err, np.float32(0)), "row_loss": np.where(used, loss, np.float32(0))}


def loss_q(row_loss):
    """The integer the kernel adds to ``loss_q`` for float32 row losses: the sum of ``rint(min(loss, 1024) 2^20)``."""
    q = np.rint(np.minimum(np.asarray(row_loss, np.float32), np.float32(1024)).astype(np.float64) * LOSS_SCALE)
    return int(q.astype(np.int64).sum())


def confusion(y, argmax, C):
    cm = np.zeros((C, C), np.int64)
    used = y >= 0
    np.add.at(cm, (y[used], argmax[used]), 1)
    return cm


# ---- the backward product ---------------------------------------------------------------------------------------------------
def backward(pl, err, C, gW=None, gb=None):
    """``(gW [P, C], gb [C])`` float64 after one call of ``wsae_probe_backward`` from the stored ``gW`` / ``gb`` (None:
    zeros), as explicit loops: per column and chunk of ``CHUNK`` entries ONE chain of float64 additions from 0, the
    chunks added to the stored value in order; ``gb`` the same over chunks of ``CHUNK`` rows.  A column without entries
    is not touched."""
    col_ptr, t_row, t_val = pl
    P = col_ptr.size - 1
    err = np.asarray(err, np.float32)
    n_rows = err.shape[0]
    gW = np.zeros((P, C)) if gW is None else np.array(gW, np.float64)
    gb = np.zeros(C) if gb is None else np.array(gb, np.float64)
    e64 = err[:, :C].astype(np.float64)
    v64 = t_val.astype(np.float64)
    for p in range(P):
        for lo in range(int(col_ptr[p]), int(col_ptr[p + 1]), CHUNK):
            acc = np.zeros(C)
            for i in range(lo, min(lo + CHUNK, int(col_ptr[p + 1]))):
                acc = acc + v64[i] * e64[t_row[i]]  # (the product is exact in float64)
            gW[p] = gW[p] + acc
    for lo in range(0, n_rows, CHUNK):
        acc = np.zeros(C)
        for r in range(lo, min(lo + CHUNK, n_rows)):
            acc = acc + e64[r]
        gb = gb + acc
    return gW, gb


# ---- the objective and a reference fit in float64 ---------------------------------------------------------------------------
def dense_design(ent, n_rows, P):
    r, _, col, v = ent
    X = np.zeros((n_rows, P))
    X[r, col] = v.astype(np.float64)
    return X


def objective64(X, y, theta, C, l2, class_weight=None, hessian=False):
    """``(loss, grad[, hessian])`` of the mean weighted cross-entropy over the used rows plus ``l2 / 2 |W|^2`` at
    ``theta = [W [P, C] row-major, bias [C]]`` in float64."""
    P = X.shape[1]
    W, b = theta[:P * C].reshape(P, C), theta[P * C:]
    used = y >= 0
    Xu, yu = X[used], y[used]
    n = yu.size
    w = np.ones(n) if class_weight is None else np.asarray(class_weight, np.float64)[yu]
    z = Xu @ W + b
    m = z.max(1, keepdims=True)
    e = np.exp(z - m)
    s = e.sum(1, keepdims=True)
    p = e / s
    loss = float((w * (np.log(s[:, 0]) + m[:, 0] - z[np.arange(n), yu])).sum() / n + 0.5 * l2 * (W * W).sum())
    err = w[:, None] * (p - (np.arange(C)[None, :] == yu[:, None]))
    grad = np.concatenate([(Xu.T @ err / n + l2 * W).reshape(-1), err.sum(0) / n])
    if not hessian:
        return loss, grad
    Xa = np.concatenate([Xu, np.ones((n, 1))], 1)  # the bias as a last feature: theta is [P + 1, C] row-major
    H = np.zeros((P + 1, C, P + 1, C))
    for c in range(C):
        for d in range(C):
            coef = w * (p[:, c] * (c == d) - p[:, c] * p[:, d])
            H[:, c, :, d] = Xa.T @ (Xa * coef[:, None]) / n
    H = H.reshape((P + 1) * C, (P + 1) * C)
    H[np.arange(P * C), np.arange(P * C)] += l2
    return loss, grad, H


def fit64(X, y, C, l2, class_weight=None, tol=1e-10, max_iter=100):
    """Newton's method from zero until the gradient's 2-norm is below ``tol``.  The objective does not change when one
    constant is added to every bias; the gradient has no component in that direction, which is fixed by a rank-one term
    in the Hessian, so the biases keep the sum zero they start with."""
    P = X.shape[1]
    theta = np.zeros(P * C + C)
    u = np.zeros(theta.size)
    u[P * C:] = 1.0 / np.sqrt(C)
    for _ in range(max_iter):
        loss, g, H = objective64(X, y, theta, C, l2, class_weight, hessian=True)
        if np.linalg.norm(g) < tol:
            return theta
        step = np.linalg.solve(H + np.outer(u, u), g)
        t = 1.0
        while objective64(X, y, theta - t * step, C, l2, class_weight)[0] > loss - 1e-4 * t * float(g @ step) and t > 1e-8:
            t *= 0.5
        theta = theta - t * step
    raise RuntimeError(f"fit64: the gradient norm is still {np.linalg.norm(g):.3e} after {max_iter} iterations")


# ---- inputs -----------------------------------------------------------------------------------------------------------------
ROWS, K, HIDDEN = 700, 8, 96
CLASSES = (1, 3, 41, 70)
LAGS = (0, -2, 3)
WINDOW = (17, 50)
COLUMNS = ("all", "window", "subset")
LDW_PAD, LDE_PAD = 3, 5  # ldw = C + 3, lde = C + 5 in the GPU tests
JUNK = np.float32(3.0e30)  # behind the C weights of a row of W: reading it would show


def col_map(kind, hidden=HIDDEN):
    """``(col_of or None, P)`` for the three forms: all features, a window, a scattered subset of 11 in shuffled order."""
    if kind == "all":
        return None, hidden
    col_of = np.full(hidden, -1, np.int32)
    if kind == "window":
        col_of[WINDOW[0]:WINDOW[0] + WINDOW[1]] = np.arange(WINDOW[1])
        return col_of, WINDOW[1]
    feats = np.random.default_rng(31).choice(hidden, 11, replace=False)
    col_of[feats] = np.arange(11)
    return col_of, 11


def general_case():
    """(code, seg): a persistent code over ``HIDDEN`` features, spoiled (values <= 0, indices outside, repeats), with NaN
    values and a repeat whose first entry is not active; ~700 rows in 5 utterances of unequal length, with padding rows
    inside and a stretch of them between two utterances."""
    rng = np.random.default_rng(2100)
    vals, idx = RO.spoil(rng, RO.persistent_code(rng, ROWS, K, HIDDEN), HIDDEN)
    vals[10, 1], vals[11, 2] = np.nan, np.nan
    idx[20, 0], idx[20, 1], vals[20, 0], vals[20, 1] = 25, 25, -1.0, 0.625   # the first ACTIVE entry is the second
    idx[21, 0], idx[21, 2], vals[21, 0], vals[21, 2] = 26, 26, 0.0, 1.5
    idx[22, 3], idx[22, 5], vals[22, 3], vals[22, 5] = 27, 27, 0.75, 2.5     # both active: the first value stands
    seg = np.repeat(np.arange(5), (60, 230, 9, 301, 100)).astype(np.int32)
    assert seg.size == ROWS
    seg[rng.random(ROWS) < 0.05] = -1
    seg[296:300] = -1
    seg[16:30] = 0
    return (vals, idx), seg


def labels_for(C, seed=0):
    """Labels ``[ROWS]`` for ``general_case``: piecewise constant, some -1 and some >= C, every class on a row that lag 0
    uses."""
    rng = np.random.default_rng(2200 + 7 * C + seed)
    labels = LO.piecewise_labels(rng, ROWS, C, hold=2.5, unlabelled=0.08, beyond=0.05)
    _, seg = general_case()
    live = np.nonzero(seg >= 0)[0]
    at = live[np.linspace(0, live.size - 1, C).astype(np.int64)]
    labels[at] = np.arange(C)
    return labels


def parameters(P, C, seed, scale=0.5, ldw=None):
    """``(W float32 [P, ldw] with JUNK behind the C classes, bias float32 [C], class_weight float32 [C])``."""
    rng = np.random.default_rng(2300 + seed)
    ldw = C + LDW_PAD if ldw is None else ldw
    W = np.full((P, ldw), JUNK, np.float32)
    W[:, :C] = (scale * rng.standard_normal((P, C))).astype(np.float32)
    return W, rng.standard_normal(C).astype(np.float32), rng.uniform(0.5, 2.0, C).astype(np.float32)


def chunk_case():
    """(code, seg, labels, C): ``2 CHUNK + 100`` rows in one utterance, feature 0 active on every row and feature 1 on every
    third, so their columns span three chunks and two; the other entries are a persistent code over the features from 2."""
    rng = np.random.default_rng(2400)
    rows, k, C = 2 * CHUNK + 100, 4, 3
    vals, idx = RO.persistent_code(rng, rows, k, HIDDEN - 2)
    idx = idx + 2
    idx[:, 0] = 0
    third = np.arange(rows) % 3 == 0
    idx[third, 1] = 1
    return (vals, idx), np.zeros(rows, np.int32), rng.integers(0, C, rows).astype(np.int32), C


def long_case(rows):
    """(code, seg, labels, C) over ``rows`` rows (more than one pass of the forward grid) in utterances of 500 rows."""
    rng = np.random.default_rng(2500)
    k, C = 4, 5
    code = RO.spoil(rng, RO.persistent_code(rng, rows, k, HIDDEN), HIDDEN)
    seg = (np.arange(rows) // 500).astype(np.int32)
    seg[rng.random(rows) < 0.03] = -1
    return code, seg, LO.piecewise_labels(rng, rows, C, hold=5.0), C


FIT_ROWS, FIT_K, FIT_HIDDEN, FIT_C, FIT_L2 = 600, 4, 64, 3, 1e-2
FIT_FEATURES = (3, 60, 17, 8, 41, 22, 35)


def fit_case():
    """(code, seg, labels): ~600 rows in 6 utterances with padding; the label depends on the code through a random
    linear rule with noise, so the probe has something to find and the classes overlap."""
    rng = np.random.default_rng(2600)
    vals, idx = RO.persistent_code(rng, FIT_ROWS, FIT_K, FIT_HIDDEN)
    seg = (np.arange(FIT_ROWS) // 100).astype(np.int32)
    seg[rng.random(FIT_ROWS) < 0.04] = -1
    rule = rng.standard_normal((FIT_HIDDEN, FIT_C))
    score = np.zeros((FIT_ROWS, FIT_C))
    np.add.at(score, np.repeat(np.arange(FIT_ROWS), FIT_K), vals.reshape(-1, 1) * rule[idx.reshape(-1)])
    labels = (score + 1.5 * rng.standard_normal(score.shape)).argmax(1).astype(np.int32)
    labels[rng.random(FIT_ROWS) < 0.03] = -1
    return (vals, idx), seg, labels


def planted_case():
    """(code, labels [1, T], planted): one utterance over 32 features, k = 4; the label is a function of three planted
    features - class c + 1 where planted feature c fires, class 0 where none does - and exactly one of them fires at a
    time.  The other entries are a persistent code over the remaining features."""
    rng = np.random.default_rng(2700)
    T, k, hidden = 900, 4, 32
    planted = (5, 11, 29)
    others = np.array([f for f in range(hidden) if f not in planted])
    vals, idx = RO.persistent_code(rng, T, k, others.size)
    idx = others[idx].astype(np.int32)
    state = LO.piecewise_labels(rng, T, 4, hold=5.0, unlabelled=0.0)
    on = state > 0
    idx[on, 0] = np.array(planted)[state[on] - 1]
    vals[on, 0] = rng.uniform(0.5, 2.0, int(on.sum())).astype(np.float32)
    return (vals, idx), state.astype(np.int64)[None], planted


DENSE_UTT, DENSE_T, DENSE_K, DENSE_HIDDEN = 8, 256, 8, 1024
DENSE_FEATURES = (700, 3, 1000, 17, 512, 41, 64, 35)


def dense_subset_case():
    """(code [n_utt, T, k], col_of, P): every one of the 2048 rows holds the eight features of ``DENSE_FEATURES``, in an
    order of its own and with positive values, so that a tracker over that subset of a 1024-feature dictionary finds all
    16384 entries where its first guess - the subset's share of the dictionary, ``1024 + 2 * 16384 * 8 // 1024 = 1280`` -
    expects few: the plan is transposed twice."""
    rng = np.random.default_rng(2800)
    rows = DENSE_UTT * DENSE_T
    idx = np.array(DENSE_FEATURES, np.int32)[np.argsort(rng.random((rows, DENSE_K)), axis=1)]
    vals = rng.uniform(0.1, 2.0, (rows, DENSE_K)).astype(np.float32)
    col_of = np.full(DENSE_HIDDEN, -1, np.int32)
    col_of[list(DENSE_FEATURES)] = np.arange(DENSE_K)
    shape = (DENSE_UTT, DENSE_T, DENSE_K)
    return (vals.reshape(shape), idx.reshape(shape)), col_of, DENSE_K
