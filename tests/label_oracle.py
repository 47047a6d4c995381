"""numpy restatement of the label association (include/wsae.h, ``wsae_label_update``): the counts
per (feature, lag, class, value stratum) and per (lag, class), vectorised with ``np.add.at``; the same update as a triple
Python loop; every reader of ``whisper_sae.analysis.labels`` in float64 (threshold metrics, AUROC, the selection of the
best threshold and lag, the top lists); a brute-force AUROC over frame pairs.  Compared with the kernel bit for bit.  Also
the inputs the CPU and the GPU tests share."""

from __future__ import annotations

import numpy as np

import profile_oracle as PO
import runs_oracle as RO

METRICS = ("precision", "recall", "f1", "jaccard", "phi", "mi", "auroc")


def empty(f_cols, L, C, S):
    return {"cnt": np.zeros((f_cols, L, C, S), np.int32), "pair_rows": np.zeros((L, C), np.int64)}


def pair_classes(seg, labels, n_rows, C, lag):
    """int64 ``[n_rows]``: the class of the pair (r, lag), -1 where it is none: row r padding, r + lag outside the call or
    in another segment, or its label outside ``[0, C)``."""
    seg = np.zeros(n_rows, np.int64) if seg is None else np.asarray(seg, np.int64).reshape(-1)
    labels = np.asarray(labels, np.int64).reshape(-1)
    r = np.arange(n_rows)
    q = r + lag
    inside = (q >= 0) & (q < n_rows)
    qc = np.clip(q, 0, max(n_rows - 1, 0))
    ok = (seg >= 0) & inside & (seg[qc] == seg) & (labels[qc] >= 0) & (labels[qc] < C)
    return np.where(ok, labels[qc], -1)


def update(code, seg, labels, hidden, C, lags, edges=None, window=None, state=None):
    """One call of ``wsae_label_update`` -> the state after it (``state``: the state before, not modified).
    ``lags = (lo, hi)``; ``edges [f_cols, S - 1]`` float32 (None: one stratum)."""
    f_lo, f_cols = (0, hidden) if window is None else window
    S = 1 if edges is None else edges.shape[1] + 1
    L = lags[1] - lags[0] + 1
    edges = np.zeros((f_cols, 0), np.float32) if edges is None else np.asarray(edges, np.float32)
    st = empty(f_cols, L, C, S) if state is None else {k: v.copy() for k, v in state.items()}
    n_rows = np.asarray(code[0]).shape[0]
    r, f, v, _ = PO.first_active(code, seg, hidden, window)
    col = f - f_lo
    stratum = PO.stratum_of(edges[col], v)
    for li in range(L):
        cls = pair_classes(seg, labels, n_rows, C, lags[0] + li)
        st["pair_rows"][li] += np.bincount(cls[cls >= 0], minlength=C)
        c = cls[r]
        ok = c >= 0
        np.add.at(st["cnt"], (col[ok], li, c[ok], stratum[ok]), 1)
    return st


def update_loop(code, seg, labels, hidden, C, lags, edges=None, window=None):
    """The same as three Python loops over rows, entries and lags (small inputs only)."""
    vals, idx = np.asarray(code[0], np.float32), np.asarray(code[1])
    f_lo, f_cols = (0, hidden) if window is None else window
    S = 1 if edges is None else edges.shape[1] + 1
    L = lags[1] - lags[0] + 1
    st = empty(f_cols, L, C, S)
    n_rows = vals.shape[0]
    for r in range(n_rows):
        if seg is not None and seg[r] < 0:
            continue
        pairs = []
        for li in range(L):
            q = r + lags[0] + li
            if 0 <= q < n_rows and (seg is None or seg[q] == seg[r]) and 0 <= labels[q] < C:
                pairs.append((li, int(labels[q])))
                st["pair_rows"][li, labels[q]] += 1
        done = set()
        for e in range(vals.shape[1]):
            f, v = int(idx[r, e]), vals[r, e]
            if not (v > 0) or not 0 <= f < hidden or f in done:
                continue
            done.add(f)
            if not f_lo <= f < f_lo + f_cols:
                continue
            s = 0 if edges is None else sum(1 for x in edges[f - f_lo] if x <= v)
            for li, c in pairs:
                st["cnt"][f - f_lo, li, c, s] += 1
    return st


def merge(a, b):
    return {k: a[k] + b[k] for k in a}


def same(got, want):
    for f in ("cnt", "pair_rows"):
        assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape, (f, got[f].dtype, got[f].shape, want[f].shape)
        assert np.array_equal(got[f], want[f]), (f, np.argwhere(got[f] != want[f])[:5])


# ---- readers ----------------------------------------------------------------------------------------------------------------
def _ratio(num, den):
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    num, den = np.broadcast_arrays(num, den)
    return np.where(den != 0, num / np.where(den != 0, den, 1.0), np.nan)


def threshold_counts(cnt_l, pair_l):
    """(TP [F, C, S], A [F, 1, S], P [1, C, 1], N) as int64 at one lag."""
    c = cnt_l.astype(np.int64)
    tp = np.flip(np.cumsum(np.flip(c, 2), 2), 2)
    p = pair_l.astype(np.int64)
    return tp, tp.sum(1, keepdims=True), p[None, :, None], int(p.sum())


def _plogp(n, row, col, total):
    n, row, col = np.broadcast_arrays(np.asarray(n, np.float64), np.asarray(row, np.float64), np.asarray(col, np.float64))
    ok = n > 0
    arg = np.where(ok, n * total / (np.where(ok, row, 1.0) * np.where(ok, col, 1.0)), 1.0)
    return np.where(ok, n / total * np.log2(arg), 0.0) if total > 0 else np.full(n.shape, np.nan)


def metric_table(cnt_l, pair_l, metric):
    """[F, C, S] float64 (not "auroc")."""
    tp, a, p, n = threshold_counts(cnt_l, pair_l)
    if metric == "precision":
        return _ratio(tp, a)
    if metric == "recall":
        return _ratio(tp, p)
    if metric == "f1":
        return _ratio(2 * tp, a + p)
    if metric == "jaccard":
        return _ratio(tp, a + p - tp)
    fp, fn = a - tp, p - tp
    tn = n - a - fn
    if metric == "phi":
        den = np.sqrt((a * (n - a)).astype(np.float64) * (p * (n - p)).astype(np.float64))
        return _ratio(tp * tn - fp * fn, den)
    if metric == "mi":
        total = float(n)
        return _plogp(tp, a, p, total) + _plogp(fp, a, n - p, total) + _plogp(fn, n - a, p, total) + _plogp(tn, n - a, n - p, total)
    raise ValueError(metric)


def auroc_table(cnt_l, pair_l):
    """[F, C] float64: levels inactive < stratum 0 < ... < stratum S - 1, ties count half."""
    pos = cnt_l.astype(np.int64)
    neg = pos.sum(1, keepdims=True) - pos
    p = pair_l.astype(np.int64)[None, :]
    n = int(p.sum())
    pos0, neg0 = p - pos.sum(2), (n - p) - neg.sum(2)
    below = neg0[:, :, None] + np.cumsum(neg, 2) - neg
    twice = pos0 * neg0 + (pos * (2 * below + neg)).sum(2)
    return _ratio(twice, 2 * (p * (n - p)))


def lag_order(lags, lag):
    if lag == "best":
        return sorted(range(lags[1] - lags[0] + 1), key=lambda li: (abs(lags[0] + li), lags[0] + li))
    return [lag - lags[0]]


def scores(st, lags, edges, metric="f1", lag=0, min_count=1):
    """The fields of ``LabelScores`` as a dict of ``[F, C]`` arrays.  One selection over all (threshold, lag) candidates
    of a cell: they are laid out threshold-major, and within a threshold in the order of preference of the lags (nearer
    0, then lower), so the first maximum is the best score at the lowest threshold, then the preferred lag."""
    order = lag_order(lags, lag)
    tables, tps, fires = [], [], []
    for li in order:
        cnt_l, pair_l = st["cnt"][:, li], st["pair_rows"][li]
        tp, a, _, _ = threshold_counts(cnt_l, pair_l)
        if metric == "auroc":
            table, tp, a = auroc_table(cnt_l, pair_l)[:, :, None], tp[:, :, :1], a[:, :, :1]
        else:
            table = metric_table(cnt_l, pair_l, metric)
        tables.append(np.where(tp >= min_count, table, np.nan))
        tps.append(tp)
        fires.append(np.broadcast_to(a, tp.shape))
    table, tp, a = (np.stack(x, axis=3) for x in (tables, tps, fires))  # [F, C, S', lags in order]
    F, C, S1, Lo = table.shape
    flat = table.reshape(F, C, S1 * Lo)
    pick = np.where(np.isnan(flat), -np.inf, flat).argmax(2)  # (the first of equal maxima)
    t, pos = pick // Lo, pick % Lo
    take = lambda x: np.take_along_axis(x.reshape(F, C, S1 * Lo), pick[:, :, None], 2)[:, :, 0]  # noqa: E731
    li_of = np.asarray(order)[pos]
    padded = np.concatenate([np.zeros((F, 1), np.float32), np.zeros((F, 0), np.float32) if edges is None else edges], axis=1)
    return {"score": take(table), "threshold_index": t.astype(np.int64), "threshold": np.take_along_axis(padded, t, 1),
            "lag": (lags[0] + li_of).astype(np.int64), "tp": take(tp), "fires": take(a),
            "positives": st["pair_rows"].astype(np.int64)[li_of, np.arange(C)[None, :]]}


def top_label_features(score, n, f_lo=0):
    """(features [C, n] int64, scores [C, n]): descending, ties to the lower index, -1 / NaN where candidates run out."""
    F, C = score.shape
    feats, vals = np.full((C, n), -1, np.int64), np.full((C, n), np.nan)
    for c in range(C):
        col = score[:, c]
        order = np.argsort(-np.where(np.isnan(col), -np.inf, col), kind="stable")
        order = order[~np.isnan(col[order])][:n]
        feats[c, :order.size], vals[c, :order.size] = order + f_lo, col[order]
    return feats, vals


def best_labels(sc):
    """The fields of ``BestLabels`` from ``scores``."""
    key = np.where(np.isnan(sc["score"]), -np.inf, sc["score"])
    c = key.argmax(1)[:, None]
    out = {k: np.take_along_axis(v, c, 1)[:, 0] for k, v in sc.items()}
    out["label"] = np.where(np.isnan(out["score"]), -1, c[:, 0]).astype(np.int64)
    return out


def auroc_brute(code, seg, labels, hidden, C, lag, edges, f, c):
    """AUROC of feature f for class c by counting (positive, negative) frame pairs, ties one half.  The frames are the
    pairs (r, lag); a frame's level is -1 where f is inactive, else its stratum."""
    vals, idx = np.asarray(code[0], np.float32), np.asarray(code[1])
    n_rows = vals.shape[0]
    cls = pair_classes(seg, labels, n_rows, C, lag)
    r_act, f_act, v_act, _ = PO.first_active(code, seg, hidden)
    level = np.full(n_rows, -1, np.int64)
    mine = f_act == f
    e = np.zeros((int(mine.sum()), 0), np.float32) if edges is None else np.repeat(edges[f][None], int(mine.sum()), 0)
    level[r_act[mine]] = PO.stratum_of(e, v_act[mine])
    pos, neg = level[cls == c], level[(cls >= 0) & (cls != c)]
    if pos.size == 0 or neg.size == 0:
        return np.nan
    wins = sum(int((p > neg).sum()) + 0.5 * int((p == neg).sum()) for p in pos)
    return wins / (pos.size * neg.size)


# ---- the inputs the CPU and the GPU tests share -------------------------------------------------------------------------------
ROWS, K, HIDDEN, CLASSES = 700, 5, 300, 7
WINDOW = (17, 50)
NAN_EDGES = 33       # an in-window feature that fires and whose edges are NaN
TIED = 40            # an in-window feature whose edges are all equal
STRATA = (1, 4, 16)
LAGS = ((0, 0), (-2, 3), (5, 6))
SELECTION = (4, (-2, 3), 5, 5)  # (strata, lags, n, min_count) of the top-list checks, on selection_case()
SEL_ROWS, SEL_K, SEL_HIDDEN, SEL_CLASSES = 6000, 4, 48, 5


def piecewise_labels(rng, rows, C, hold=6.0, unlabelled=0.05, beyond=0.0):
    """Labels that hold for a geometric time of mean ``hold`` rows; a share ``unlabelled`` of the stretches is -1 and a
    share ``beyond`` takes values >= C."""
    jump = rng.random(rows) < 1.0 / hold
    jump[0] = True
    visit = np.cumsum(jump) - 1
    n = int(visit[-1]) + 1
    draws = rng.integers(0, C, n)
    u = rng.random(n)
    draws[u < unlabelled] = -1
    draws[(u >= unlabelled) & (u < unlabelled + beyond)] = C + rng.integers(0, 3, int(((u >= unlabelled) & (u < unlabelled + beyond)).sum()))
    return draws[visit].astype(np.int32)


def general_case():
    """(code, seg, labels): a persistent code over ``HIDDEN`` features, spoiled (values <= 0, indices outside, repeats), with
    a repeat whose first entry is not active, NaN and +inf values; ~700 rows in uneven segments (one-row segments among
    them) with padding inside and between; labels with -1 and values >= C."""
    rng = np.random.default_rng(2000)
    code = RO.persistent_code(rng, ROWS, K, HIDDEN)
    vals, idx = RO.spoil(rng, code, HIDDEN)
    # features of the window appear often: fold a third of the indices into it
    fold = rng.random(idx.shape) < 0.35
    idx[fold & (idx >= 0) & (idx < HIDDEN)] = WINDOW[0] - 2 + idx[fold & (idx >= 0) & (idx < HIDDEN)] % (WINDOW[1] + 4)
    vals[10, 1], vals[11, 2] = np.nan, np.inf
    idx[20, 0], idx[20, 1], vals[20, 0], vals[20, 1] = 25, 25, -1.0, 0.625   # the first ACTIVE entry is the second
    idx[21, 0], idx[21, 2], vals[21, 0], vals[21, 2] = 26, 26, 0.0, 1.5
    idx[30:36, 3], vals[30:36, 3] = NAN_EDGES, 0.5
    idx[40:48, 4], vals[40:48, 4] = TIED, np.linspace(0.1, 2.0, 8, dtype=np.float32)
    seg0 = RO.uneven_segments(rng, ROWS, 23).astype(np.int32)
    seg0[16:60] = seg0[16]                 # the planted rows and every lag of theirs share one utterance ...
    seg = seg0.copy()
    seg[rng.random(ROWS) < 0.06] = -1      # padding inside
    seg[300:304] = -1                      # ... and a stretch of it
    seg[16:60] = seg0[16:60]               # ... without padding
    labels = piecewise_labels(rng, ROWS, CLASSES, hold=4.0, unlabelled=0.08, beyond=0.05)
    labels[16:60] = (np.arange(16, 60) // 3) % CLASSES  # ... and every label of theirs counts
    return (vals, idx), seg, labels


def general_edges(S, window=None):
    """Edges ``[f_cols, S - 1]`` (None for S == 1): ascending per feature, one of them equal to a value of the code, NaN for
    feature ``NAN_EDGES``, all equal for feature ``TIED``."""
    if S == 1:
        return None
    (vals, idx), _, _ = general_case()
    rng = np.random.default_rng(2001 + S)
    edges = np.sort(rng.uniform(0.05, 2.0, (HIDDEN, S - 1)).astype(np.float32), axis=1)
    edges[25, 0] = vals[20, 1]             # a value equal to an edge
    edges[25, 1:] = np.maximum(edges[25, 1:], np.float32(0.7))
    edges[NAN_EDGES] = np.nan
    edges[TIED] = np.float32(0.9)
    lo, cols = (0, HIDDEN) if window is None else window
    return np.ascontiguousarray(edges[lo:lo + cols])


def selection_case():
    """(code, seg, labels, edges) for the checks of the top lists and best labels: enough rows that the counts are large
    and no two of the scores compared are equal (tests/test_label_association.py asserts the gaps).  On half of the
    labelled rows column 0 carries one of three features tied to the row's class, so the classes have detectors."""
    rng = np.random.default_rng(2500)
    vals, idx = RO.persistent_code(rng, SEL_ROWS, SEL_K, SEL_HIDDEN)
    seg = (np.arange(SEL_ROWS) // 200).astype(np.int32)
    labels = piecewise_labels(rng, SEL_ROWS, SEL_CLASSES, hold=5.0, unlabelled=0.05)
    tied = (rng.random(SEL_ROWS) < 0.5) & (labels >= 0)
    idx[tied, 0] = (labels[tied] * SEL_K * 2 + rng.integers(0, 3, int(tied.sum())) * SEL_K) % SEL_HIDDEN // SEL_K * SEL_K
    edges = np.sort(np.random.default_rng(1).uniform(0.1, 1.6, (SEL_HIDDEN, SELECTION[0] - 1)).astype(np.float32), axis=1)
    return (vals, idx), seg, labels, edges


def selection_gaps_hold(score, n):
    """Per class: among the first n + 1 scores, descending, every two neighbours - the n-th and the (n + 1)-th among
    them - differ by more than 1e-9.  bool ``[C]``."""
    ok = np.zeros(score.shape[1], bool)
    for c in range(score.shape[1]):
        col = np.sort(score[:, c][~np.isnan(score[:, c])])[::-1]
        ok[c] = col.size >= n + 1 and bool((np.diff(col[:n + 1]) < -1e-9).all())
    return ok


def best_label_gaps_hold(score):
    """Per feature: it has no candidate class, one, or its best and second-best class differ by more than 1e-9.
    bool ``[F]``."""
    top = np.sort(np.where(np.isnan(score), -np.inf, score), axis=1)[:, ::-1]
    second = top[:, 1] if top.shape[1] > 1 else np.full(top.shape[0], -np.inf)
    with np.errstate(invalid="ignore"):
        return ~np.isfinite(second) | (top[:, 0] - second > 1e-9)


def wide_case(k, rows=70, hidden=300):
    code, seg = PO.wide_case(k, rows, hidden)
    rng = np.random.default_rng(2100 + k)
    seg = np.where(seg < 0, -1, (np.arange(rows) // 23)).astype(np.int32)
    return code, seg, piecewise_labels(rng, rows, 5, hold=3.0, unlabelled=0.1, beyond=0.05)


D, H, SAE_K, UTT, T, PY_CLASSES = 64, 256, 8, 12, 40, 6


def python_layer_labels(seed=6):
    """Labels ``[UTT, T]`` int64 for the Python-layer test: piecewise constant, some -1."""
    rng = np.random.default_rng(seed)
    return piecewise_labels(rng, UTT * T, PY_CLASSES, hold=5.0, unlabelled=0.07).astype(np.int64).reshape(UTT, T)


def planted_case():
    """(code, labels, edges, feature): feature 9 fires strongly (value 4) exactly two frames BEFORE every frame of class 3
    - the label two frames later is 3 - and weakly (0.25) on every fifth other frame; one utterance of 400 frames,
    hidden 16, k = 2."""
    rng = np.random.default_rng(2200)
    rows, hidden, f = 400, 16, 9
    labels = piecewise_labels(rng, rows, 5, hold=6.0, unlabelled=0.0)
    idx = np.stack([np.full(rows, f), rng.integers(0, 8, rows)], axis=1).astype(np.int32)
    vals = np.zeros((rows, 2), np.float32)
    vals[:, 1] = rng.uniform(0.1, 1.0, rows)
    strong = np.zeros(rows, bool)
    strong[:-2] = labels[2:] == 3
    vals[strong, 0] = 4.0
    weak = ~strong & (np.arange(rows) % 5 == 0)
    vals[weak, 0] = 0.25
    edges = np.tile(np.array([[1.0]], np.float32), (hidden, 1))
    return (vals, idx), labels, edges, f
