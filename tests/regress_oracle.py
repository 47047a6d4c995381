"""numpy restatement of the sparse ridge regression (include/wsae.h, ``wsae_gram_update`` / ``wsae_regress_forward``;
DESIGN.md section 22): the rule that decides which rows carry a target, the chunked float64 Gram matrix and the forward
product with its five sums as explicit sequential loops that are compared with the kernels bit for bit, the moments
through the probe oracle's chunked backward product, the ridge solve by ``numpy.linalg.solve``, and the inputs the CPU and
the GPU tests share.  The activity and column rules and the plan are those of tests/probe_oracle.py."""

from __future__ import annotations

import numpy as np

import probe_oracle as PB
import runs_oracle as RO

CHUNK = PB.CHUNK
SENTINEL = -float(2 ** 41)  # in the cells a kernel must not write


# ---- the rules --------------------------------------------------------------------------------------------------------------
def used_rows(seg, Y, n_rows, lag):
    """bool ``[n_rows]``: row r is used iff it is not padding, ``0 <= r + lag < n_rows``, ``seg[r + lag] == seg[r]`` and all
    the targets of ``Y[r + lag]`` are finite.  ``seg`` None: one segment without padding."""
    seg = np.zeros(n_rows, np.int64) if seg is None else np.asarray(seg).reshape(-1).astype(np.int64)
    Y = np.asarray(Y, np.float32).reshape(n_rows, -1)
    r = np.arange(n_rows)
    q = r + lag
    inside = (q >= 0) & (q < n_rows)
    qc = np.clip(q, 0, max(n_rows - 1, 0))
    return (seg >= 0) & inside & (seg[qc] == seg) & np.isfinite(Y[qc]).all(1)


def shifted_targets(seg, Y, n_rows, lag):
    """``(E float32 [n_rows, C + 1], used)``: the targets ``Y[r + lag]`` of the used rows with a column of ones appended, and
    exact zeros on the other rows - what the tracker hands to ``wsae_probe_backward`` in the place of the error rows."""
    Y = np.asarray(Y, np.float32).reshape(n_rows, -1)
    used = used_rows(seg, Y, n_rows, lag)
    q = np.clip(np.arange(n_rows) + lag, 0, max(n_rows - 1, 0))
    E = np.zeros((n_rows, Y.shape[1] + 1), np.float32)
    E[used, :-1] = Y[q[used]]
    E[used, -1] = 1.0
    return E, used


def rows_of(ent, n_rows):
    """Per row the ``(columns, values float64)`` of its first-active entries that have a column, in entry position."""
    r, _, col, v = ent
    cut = np.searchsorted(r, np.arange(n_rows + 1))
    return [(col[cut[i]:cut[i + 1]], v[cut[i]:cut[i + 1]].astype(np.float64)) for i in range(n_rows)]


# ---- the Gram matrix ----------------------------------------------------------------------------------------------------------
def gram(pl, ent, n_rows, P, G=None, p_lo=0, p_rows=None, cap=None):
    """``G [p_rows, P]`` float64 after one call of ``wsae_gram_update`` from the stored ``G`` (None: zeros), as explicit
    loops: per row p of the window and chunk of ``CHUNK`` entries of its list ONE chain of float64 additions per column
    c >= p, from 0, over the entries in list order on whose row c is active; the chunks are added to the stored value in
    order.  On the diagonal the row's value is the list's own.  A column without entries is not touched, cells with
    c < p never."""
    col_ptr, t_row, t_val = pl
    p_rows = P - p_lo if p_rows is None else p_rows
    cap = int(col_ptr[-1]) if cap is None else cap
    G = np.zeros((p_rows, P)) if G is None else np.array(G, np.float64)
    per_row = rows_of(ent, n_rows)
    for p in range(p_lo, p_lo + p_rows):
        beg, end = min(int(col_ptr[p]), cap), min(int(col_ptr[p + 1]), cap)
        for lo in range(beg, end, CHUNK):
            acc = np.zeros(P)
            for i in range(lo, min(lo + CHUNK, end)):
                cols, vals = per_row[t_row[i]]
                x = np.float64(t_val[i])
                u = np.where(cols == p, x, vals)
                acc[cols] = acc[cols] + x * u  # (the columns of a row are distinct; the product is exact in float64)
            G[p - p_lo, p:P] = G[p - p_lo, p:P] + acc[p:]
    return G


def gram_dense(X):
    """float64 ``X^T X`` of the densified code."""
    X = np.asarray(X, np.float64)
    return X.T @ X


def mirror_upper(G):
    """The full symmetric matrix of an upper triangle."""
    U = np.triu(G)
    return U + np.triu(G, 1).T


# ---- the forward product ------------------------------------------------------------------------------------------------------
def forward(code, ent, seg, Y, lag, W, bias, C, stats=None):
    """``(pred float32 [n_rows, C], n_used, stats float64 [5, C])`` after one call of ``wsae_regress_forward`` from the stored
    ``stats`` (None: zeros).  The prediction is a float64 chain from the bias, per entry (ascending position) one multiply
    and one add; the five sums are chains over the used rows of every chunk of ``CHUNK`` rows, added to the stored value in
    chunk order.  ``Y`` None: the predictions alone."""
    n_rows, k = np.asarray(code[0]).shape
    r, pos, col, v = ent
    W = np.asarray(W, np.float64)
    z = np.tile(np.asarray(bias, np.float64)[:C], (n_rows, 1))
    for j in range(k):
        at = pos == j  # (at most one entry per row and position)
        prod = v[at].astype(np.float64)[:, None] * W[col[at], :C]
        z[r[at]] = z[r[at]] + prod
    live = np.ones(n_rows, bool) if seg is None else np.asarray(seg).reshape(-1) >= 0
    pred = np.where(live[:, None], z, 0.0).astype(np.float32)
    if Y is None:
        return pred, 0, None
    Y = np.asarray(Y, np.float32).reshape(n_rows, -1)
    used = used_rows(seg, Y, n_rows, lag)
    stats = np.zeros((5, C)) if stats is None else np.array(stats, np.float64)
    for lo in range(0, n_rows, CHUNK):
        acc = np.zeros((5, C))
        for i in range(lo, min(lo + CHUNK, n_rows)):
            if not used[i]:
                continue
            y, p = Y[i + lag, :C].astype(np.float64), z[i]
            d = y - p
            acc[0] = acc[0] + y
            acc[1] = acc[1] + y * y
            acc[2] = acc[2] + p
            acc[3] = acc[3] + p * p
            acc[4] = acc[4] + d * d
        stats = stats + acc
    return pred, int(used.sum()), stats


# ---- the solve ----------------------------------------------------------------------------------------------------------------
def centred_system(G, M, sx, sy, n, l2):
    """``(A, B)`` of the ridge system ``A W = B``: ``A = Gc / n + l2 I``, ``B = Mc / n`` on the centred statistics."""
    xbar, ybar = sx / n, sy / n
    A = (G - n * np.outer(xbar, xbar)) / n + l2 * np.eye(G.shape[0])
    B = (M - n * np.outer(xbar, ybar)) / n
    return A, B


def ridge(G, M, sx, sy, n, l2):
    """``(W [P, C], b [C], cond)`` by ``numpy.linalg.solve`` on the full symmetric ``G``; ``cond``: the 2-norm condition
    number of the system."""
    A, B = centred_system(G, M, sx, sy, n, l2)
    W = np.linalg.solve(A, B)
    return W, sy / n - W.T @ (sx / n), float(np.linalg.cond(A))


def statistics(code, seg, Y, lag, hidden, col_of, P):
    """The oracle's statistics of one call: ``G`` (upper triangle), ``MX [P, C + 1]`` and ``gb [C + 1]`` by the chunked
    loops, ``syy [C]``, and the dense float64 design of the used rows with their targets (for references)."""
    n_rows = np.asarray(code[0]).shape[0]
    E, used = shifted_targets(seg, Y, n_rows, lag)
    seg_used = np.where(used, 0 if seg is None else np.asarray(seg).reshape(-1), -1).astype(np.int32)
    ent = PB.entries(code, seg_used, hidden, col_of)
    pl = PB.plan(ent, P)
    G = gram(pl, ent, n_rows, P)
    MX, gb = PB.backward(pl, E, E.shape[1])
    X = PB.dense_design(ent, n_rows, P)[used]
    T = E[used, :-1].astype(np.float64)
    return {"G": G, "MX": MX, "gb": gb, "syy": (T * T).sum(0), "X": X, "T": T, "ent": ent, "pl": pl, "E": E, "used": used,
            "seg_used": seg_used}


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def general_case(hidden, k, rows=None, seed=0):
    """(code, seg): a persistent code spoiled with values <= 0, indices outside, repeats and NaN, in utterances of unequal
    length with padding rows inside and a stretch of them between two utterances.  Fewer rows for the wide codes (the
    oracle's loops are per entry)."""
    rng = np.random.default_rng(3100 + 7 * hidden + k + seed)
    rows = (3000 if k <= 5 else 1500 if k <= 33 else 700) if rows is None else rows
    width = min(k, hidden)  # (persistent_code needs a feature per column)
    vals, idx = RO.persistent_code(rng, rows, width, hidden)
    if width < k:
        extra_v, extra_i = RO.persistent_code(rng, rows, k - width, hidden)
        vals, idx = np.concatenate([vals, extra_v], 1), np.concatenate([idx, extra_i], 1)  # (repeats across the halves)
    vals, idx = RO.spoil(rng, (vals, idx), hidden)
    vals[10, 0], vals[11, k - 1] = np.nan, np.nan
    if k >= 3:
        idx[20, 0], idx[20, 1], vals[20, 0], vals[20, 1] = 25, 25, -1.0, 0.625  # the first ACTIVE entry is the second
        idx[22, 0], idx[22, 2], vals[22, 0], vals[22, 2] = 27, 27, 0.75, 2.5    # both active: the first value stands
    cuts = np.sort(rng.choice(np.arange(50, rows - 50), 4, replace=False))
    seg = np.searchsorted(cuts, np.arange(rows), side="right").astype(np.int32)
    seg[rng.random(rows) < 0.05] = -1
    seg[cuts[1] - 4:cuts[1]] = -1
    return (vals, idx), seg


def col_map(kind, hidden):
    """``(col_of or None, P)``: the identity, a subset in ascending order, a permuted subset."""
    if kind == "identity":
        return None, hidden
    rng = np.random.default_rng(41 + hidden)
    n = hidden // 3
    feats = np.sort(rng.choice(hidden, n, replace=False)) if kind == "subset" else rng.choice(hidden, n, replace=False)
    col_of = np.full(hidden, -1, np.int32)
    col_of[feats] = np.arange(n)
    return col_of, n


def targets(rng, rows, C, scale=1.0):
    """float32 ``[rows, C]`` O(1) targets with a few non-finite values."""
    Y = (scale * rng.standard_normal((rows, C))).astype(np.float32)
    bad = rng.choice(rows, max(rows // 60, 3), replace=False)
    Y[bad[0::3], rng.integers(0, C)] = np.nan
    Y[bad[1::3], rng.integers(0, C)] = np.inf
    Y[bad[2::3], rng.integers(0, C)] = -np.inf
    return Y


def long_case():
    """(code, seg): ``hidden = 8``, 2 CHUNK + 900 rows, feature 3 on almost every row (a list of three chunks, the last one
    ragged) and feature 5 on every other row; the rest a persistent code over the other features."""
    rng = np.random.default_rng(3300)
    rows, k, hidden = 2 * CHUNK + 900, 3, 8
    others = np.array([0, 1, 2, 4, 6, 7])
    vals, idx = RO.persistent_code(rng, rows, k, others.size)
    idx = others[idx].astype(np.int32)
    idx[:, 0] = 3
    idx[::2, 1] = 5
    vals[rng.random(rows) < 0.01, 0] = 0.0  # almost all
    seg = (np.arange(rows) // 1000).astype(np.int32)
    seg[rng.random(rows) < 0.02] = -1
    return (vals, idx), seg, hidden


FIT_ROWS, FIT_K, FIT_HIDDEN, FIT_C, FIT_L2 = 1200, 8, 96, 3, 1e-3


def fit_case(seed=0):
    """(code, seg, Y): a random ``k = 8``, ``H = 96`` code with values O(1) in 8 utterances with padding; the targets are a
    random linear map of the code plus noise, O(1), with a few non-finite rows."""
    rng = np.random.default_rng(3400 + seed)
    vals, idx = RO.persistent_code(rng, FIT_ROWS, FIT_K, FIT_HIDDEN)
    seg = (np.arange(FIT_ROWS) // 150).astype(np.int32)
    seg[rng.random(FIT_ROWS) < 0.04] = -1
    rule = rng.standard_normal((FIT_HIDDEN, FIT_C)) / np.sqrt(FIT_K)
    Y = np.zeros((FIT_ROWS, FIT_C))
    np.add.at(Y, np.repeat(np.arange(FIT_ROWS), FIT_K), vals.reshape(-1, 1) * rule[idx.reshape(-1)])
    Y = (Y + 0.3 * rng.standard_normal(Y.shape)).astype(np.float32)
    Y[rng.choice(FIT_ROWS, 9, replace=False), rng.integers(0, FIT_C, 9)] = np.nan
    return (vals, idx), seg, Y


PLANTED = (5, 11, 29)
PLANTED_W = np.array([[1.5, -0.75], [-2.0, 0.5], [0.625, 1.25]])
PLANTED_B = np.array([0.25, -1.0])


def planted_case(seed=0):
    """(code, Y [1, T, 2]): one utterance over 32 features, k = 4; the targets are a NOISELESS linear map of the three
    planted features (weights ``PLANTED_W``, intercept ``PLANTED_B``); one planted feature fires on about half the frames.
    The other entries are a persistent code over the remaining features."""
    rng = np.random.default_rng(3500 + seed)
    T, k, hidden = 900, 4, 32
    others = np.array([f for f in range(hidden) if f not in PLANTED])
    vals, idx = RO.persistent_code(rng, T, k, others.size)
    idx = others[idx].astype(np.int32)
    which = rng.integers(-3, 3, T)
    on = which >= 0
    idx[on, 0] = np.array(PLANTED)[which[on]]
    vals[on, 0] = rng.uniform(0.5, 2.0, int(on.sum())).astype(np.float32)
    Y = np.tile(PLANTED_B, (T, 1))
    Y[on] += vals[on, 0].astype(np.float64)[:, None] * PLANTED_W[which[on]]
    return (vals, idx), Y.astype(np.float32)[None]
