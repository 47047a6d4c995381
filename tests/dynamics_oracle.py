"""numpy restatement of the code dynamics (include/wsae.h, ``wsae_dyn_update`` and ``wsae_boundary_score``; DESIGN.md
section 23): sequential loops that are the definition.  The similarity of two rows is one chain of float64 additions in
the ascending entry position of the earlier row, the boundary match the literal two-pointer walk over the lists of a
stretch; the kernels are compared with both bit for bit.  Also the summary and curve formulas of
``whisper_sae.analysis.dynamics`` in float64, and the input recipes the CPU and the GPU tests share."""

from __future__ import annotations

import functools
import math

import numpy as np

import runs_oracle as RO

COSINE, DOT, JACCARD = 0, 1, 2
METRICS = {"cosine": COSINE, "dot": DOT, "jaccard": JACCARD}
BINS = 64
STATE_FIELDS = ("pairs", "sim_q", "sq_q", "hist", "total_rows")


# ---- the canonical code -------------------------------------------------------------------------------------------------------
def canonical(code, hidden, seg=None, weight=None):
    """Per row ``(entries, norm, active)``: ``entries`` the list of ``(f, u)`` of the row's active features in ascending
    entry position (``u`` a Python float holding the float32 value ``v weight[f]``), ``norm`` the float64 chain of
    ``u u`` in that order, ``active`` their number.  A padding row has none."""
    vals, idx = np.asarray(code[0], np.float32), np.asarray(code[1]).astype(np.int64)
    w = None if weight is None else np.asarray(weight, np.float32)
    rows = []
    for r in range(vals.shape[0]):
        entries, seen, norm = [], set(), 0.0
        if seg is None or seg[r] >= 0:
            for j in range(vals.shape[1]):
                v, f = vals[r, j], int(idx[r, j])
                if not v > 0:  # (NaN is not)
                    continue
                if f in seen:
                    continue
                seen.add(f)
                if not 0 <= f < hidden:
                    continue
                u = v
                if w is not None:
                    if not w[f] > 0:
                        continue
                    u = np.float32(v * w[f])
                u = float(u)
                entries.append((f, u))
                norm += u * u
        rows.append((entries, norm, len(entries)))
    return rows


def pair_terms(canon, r, q):
    """``(s, matched)`` of the rows r and q: the chain of products in the entry order of row r."""
    there = dict(canon[q][0])
    s, matched = 0.0, 0
    for f, u in canon[r][0]:
        y = there.get(f)
        if y is not None:
            s += u * y
            matched += 1
    return s, matched


def similarity_value(metric, s, matched, row_r, row_q):
    """The float32 similarity from the terms of a pair and the two canonical rows."""
    _, n_r, a_r = row_r
    _, n_q, a_q = row_q
    if metric == DOT:
        c = s
    elif metric == COSINE:
        c = 0.0
        if n_r != 0.0 and n_q != 0.0:
            c = s / math.sqrt(n_r * n_q)
            if not c <= 1.0:
                c = 1.0
    else:
        union = a_r + a_q - matched
        c = matched / union if union else 0.0
    return np.float32(c)


def pair_class(label, r, q):
    if label is None or label[r] < 0 or label[q] < 0:
        return 2
    return 0 if label[r] == label[q] else 1


def empty_state(n_lags):
    return {"pairs": np.zeros((n_lags, 3), np.int64), "sim_q": np.zeros((n_lags, 3), np.int64),
            "sq_q": np.zeros((n_lags, 3), np.int64), "hist": np.zeros((n_lags, 3, BINS), np.int64),
            "total_rows": np.zeros(1, np.int64)}


def update(code, hidden, lags, metric=COSINE, seg=None, weight=None, label=None, state=None, canon=None, terms=None):
    """One call of ``wsae_dyn_update`` -> ``(sim float32 [rows, n_lags], the state after it)``; ``state`` is the state
    before (not modified; None: zeros).  With ``metric == DOT`` the state stays as it was.  ``canon`` / ``terms``: the
    canonical rows and a ``{(r, lag): (s, matched)}`` table computed earlier for the same code, seg and weight."""
    rows = np.asarray(code[0]).shape[0]
    canon = canonical(code, hidden, seg, weight) if canon is None else canon
    st = empty_state(len(lags)) if state is None else {k: v.copy() for k, v in state.items()}
    sim = np.full((rows, len(lags)), np.nan, np.float32)
    for r in range(rows):
        if seg is not None and seg[r] < 0:
            continue
        if metric != DOT:
            st["total_rows"][0] += 1
        for li, lag in enumerate(lags):
            q = r + lag
            if q >= rows or (seg is not None and seg[q] != seg[r]):
                continue
            s, matched = terms[(r, lag)] if terms is not None else pair_terms(canon, r, q)
            c = similarity_value(metric, s, matched, canon[r], canon[q])
            sim[r, li] = c
            if metric == DOT:
                continue
            x = round(float(c) * 2.0 ** 30)  # (the product is exact; round() rounds halves to even, as llrint does)
            cls = pair_class(label, r, q)
            st["pairs"][li, cls] += 1
            st["sim_q"][li, cls] += x
            st["sq_q"][li, cls] += (x >> 15) ** 2
            st["hist"][li, cls, min(x >> 24, BINS - 1)] += 1
    return sim, st


def all_terms(canon, seg, lags):
    """``{(r, lag): (s, matched)}`` of every valid pair of the lags."""
    rows, out = len(canon), {}
    for r in range(rows):
        if seg is not None and seg[r] < 0:
            continue
        for lag in lags:
            q = r + lag
            if q < rows and (seg is None or seg[q] == seg[r]):
                out[(r, lag)] = pair_terms(canon, r, q)
    return out


def same_bits(got, want, what=""):
    """float32 arrays: equal NaN masks, equal bits elsewhere."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (what, "NaN masks differ", int((gn != wn).sum()))
    a, b = got.view(np.uint32)[~gn], want.view(np.uint32)[~wn]
    bad = np.nonzero(a != b)[0]
    assert bad.size == 0, (what, "bits differ", bad[:5], got[~gn][bad[:5]], want[~wn][bad[:5]])


def same_state(got, want, what=""):
    for name in STATE_FIELDS:
        assert np.array_equal(np.asarray(got[name]).reshape(-1), want[name].reshape(-1)), (what, name)


# ---- boundaries ---------------------------------------------------------------------------------------------------------------
def stretches(rows, seg=None):
    """``[(first, last)]`` of the maximal runs of consecutive rows with equal ``seg >= 0``."""
    if seg is None:
        return [(0, rows - 1)] if rows else []
    out, r = [], 0
    while r < rows:
        if seg[r] < 0:
            r += 1
            continue
        a = r
        while r + 1 < rows and seg[r + 1] == seg[a]:
            r += 1
        out.append((a, r))
        r += 1
    return out


def find_peaks(nov, seg=None):
    """uint8 ``[rows]``: 1 where the row is a peak of its stretch."""
    nov = np.asarray(nov, np.float32)
    peaks = np.zeros(nov.shape[0], np.uint8)
    for a, b in stretches(nov.shape[0], seg):
        for r in range(a, b + 1):
            x = nov[r]
            if np.isnan(x):
                continue
            left = nov[r - 1] if r > a and not np.isnan(nov[r - 1]) else -np.inf
            right = nov[r + 1] if r < b and not np.isnan(nov[r + 1]) else -np.inf
            peaks[r] = x > left and x >= right
    return peaks


def match(pred, ref, tol):
    """The hits of the greedy one-to-one match of two ascending lists of rows."""
    i = j = hits = 0
    while i < len(pred) and j < len(ref):
        if abs(pred[i] - ref[j]) <= tol:
            hits, i, j = hits + 1, i + 1, j + 1
        elif pred[i] < ref[j]:
            i += 1
        else:
            j += 1
    return hits


def boundary_score(nov, thr, tol, seg=None, ref=None, state=None):
    """One call of ``wsae_boundary_score`` -> ``(the counts after it, peaks uint8 [rows])``."""
    nov, thr = np.asarray(nov, np.float32), np.asarray(thr, np.float32)
    st = ({"n_pred": np.zeros(thr.size, np.int64), "n_hit": np.zeros(thr.size, np.int64), "n_ref": np.zeros(1, np.int64),
           "n_peaks": np.zeros(1, np.int64)} if state is None else {k: v.copy() for k, v in state.items()})
    peaks = find_peaks(nov, seg)
    for a, b in stretches(nov.shape[0], seg):
        rows = np.arange(a, b + 1)
        pk = rows[peaks[a:b + 1] != 0]
        rf = rows[np.asarray(ref[a:b + 1]) != 0] if ref is not None else rows[:0]
        st["n_ref"][0] += rf.size
        st["n_peaks"][0] += pk.size
        for t in range(thr.size):
            pred = pk[nov[pk] >= thr[t]]
            st["n_pred"][t] += pred.size
            st["n_hit"][t] += match(pred.tolist(), rf.tolist(), tol)
    return st, peaks


def same_counts(got, want, what=""):
    for name in ("n_pred", "n_hit", "n_ref", "n_peaks"):
        assert np.array_equal(np.asarray(got[name]).reshape(-1), want[name].reshape(-1)), (what, name, got[name], want[name])


# ---- the readers, float64 from the integers ----------------------------------------------------------------------------------
def hist_quantile(hist, p):
    """The ``p`` quantile of one histogram of 64 equal bins over [0, 1], interpolated in the bin; NaN when it is empty."""
    hist = np.asarray(hist, np.int64)
    n = int(hist.sum())
    if n == 0:
        return math.nan
    t, cum = p * n, 0
    for j in range(BINS):
        if hist[j] > 0 and cum + hist[j] >= t:
            return j / BINS + (t - cum) / hist[j] / BINS
        cum += hist[j]
    return 1.0


def group_stats(state, li, classes):
    """``(pairs, mean, std, median, q10, q90)`` of the pairs of lag index ``li`` whose class is in ``classes``."""
    n = int(sum(state["pairs"][li, c] for c in classes))
    hist = sum(state["hist"][li, c] for c in classes)
    if n == 0:
        return 0, math.nan, math.nan, math.nan, math.nan, math.nan
    mean = float(sum(int(state["sim_q"][li, c]) for c in classes)) / n / 2.0 ** 30
    second = float(sum(int(state["sq_q"][li, c]) for c in classes)) / n / 2.0 ** 30
    var = max(second - mean * mean, 0.0)
    return n, mean, math.sqrt(var), hist_quantile(hist, 0.5), hist_quantile(hist, 0.1), hist_quantile(hist, 0.9)


def separation(state, li):
    _, mw, sw, *_ = group_stats(state, li, (0,))
    _, ma, sa, *_ = group_stats(state, li, (1,))
    den = math.sqrt((sw * sw + sa * sa) / 2) if not (math.isnan(sw) or math.isnan(sa)) else math.nan
    return (mw - ma) / den if den and not math.isnan(den) else math.nan


def timescale(lags, means):
    """The lag at which the mean similarity, linear between the lags, falls below 1/e of its value at the smallest lag."""
    level = means[0] / math.e
    for i in range(1, len(lags)):
        if means[i] < level:
            return lags[i - 1] + (means[i - 1] - level) / (means[i - 1] - means[i]) * (lags[i] - lags[i - 1])
    return math.inf


def curve(counts):
    """``precision, recall, f1, over_segmentation, r_value`` float64 arrays of the counts; NaN where a denominator is 0."""
    pred, hit = counts["n_pred"].astype(np.float64), counts["n_hit"].astype(np.float64)
    ref = float(counts["n_ref"][0])
    with np.errstate(divide="ignore", invalid="ignore"):
        prec = np.where(pred > 0, hit / pred, np.nan)
        rec = hit / ref if ref > 0 else np.full_like(pred, np.nan)
        f1 = np.where(pred + ref > 0, 2 * hit / (pred + ref), np.nan)
        os_ = pred / ref - 1 if ref > 0 else np.full_like(pred, np.nan)
        r1 = np.sqrt((1 - rec) ** 2 + os_ ** 2)
        r2 = (-os_ + rec - 1) / math.sqrt(2)
        rval = 1 - (np.abs(r1) + np.abs(r2)) / 2
    return {"precision": prec, "recall": rec, "f1": f1, "over_segmentation": os_, "r_value": rval}


def best_index(values):
    """The index of the largest value that is not NaN (the first of equals), -1 when there is none."""
    key = np.where(np.isnan(values), -np.inf, values)
    return int(np.argmax(key)) if np.any(~np.isnan(values)) else -1


# ---- the inputs the CPU and the GPU tests share -------------------------------------------------------------------------------
# (rows, k, hidden, segments); the planted case stands apart
SHAPES = ((1, 1, 32, 1), (257, 5, 96, 9), (3000, 32, 3072, 4), (700, 64, 256, 3), (700, 65, 256, 3), (600, 128, 256, 4),
          (2000, 32, 40960, 7))
LAG_SETS = ((1,), (1, 2, 3, 5, 8), tuple(range(1, 17)), (1, 1024))
ALL_LAGS = tuple(range(1, 17)) + (1024,)


def spoiled_code(rng, rows, k, hidden):
    """A code with persistence (``runs_oracle.persistent_code``) and everything a TopK code never has: values <= 0, NaN
    values, indices -1 and ``hidden``, repeated indices (``runs_oracle.spoil``), silent rows (no active entry: exact zeros),
    rows that repeat their predecessor and rows drawn afresh."""
    if rows == 1:
        return np.ones((1, k), np.float32), np.zeros((1, k), np.int32)
    vals, idx = RO.persistent_code(rng, rows, k, hidden)
    fresh = rng.random(rows) < 0.08  # no feature in common with the neighbours (where hidden is large)
    for r in np.nonzero(fresh)[0]:
        idx[r] = rng.choice(hidden, k, replace=False)
    vals, idx = RO.spoil(rng, (vals, idx), hidden)
    vals[rng.random(vals.shape) < 0.01] = np.nan
    again = np.nonzero(rng.random(rows) < 0.03)[0]
    again = again[again > 0]
    vals[again], idx[again] = vals[again - 1], idx[again - 1]
    silent = rng.random(rows) < 0.04
    vals[silent] = -np.abs(vals[silent])
    return vals.astype(np.float32), idx.astype(np.int32)


@functools.lru_cache(maxsize=None)
def similarity_case(n):
    """Case ``n`` of ``SHAPES`` -> dict with ``code``, ``hidden``, ``seg`` (about 5 % padding rows), ``weight`` (zeros, a
    NaN and a negative among positive weights) and ``label`` (piecewise constant, some -1)."""
    rows, k, hidden, n_seg = SHAPES[n]
    rng = np.random.default_rng(2300 + n)
    code = spoiled_code(rng, rows, k, hidden)
    seg = (np.arange(rows) * n_seg // rows).astype(np.int32)
    if rows > 1:
        seg[rng.random(rows) < 0.05] = -1
    weight = rng.uniform(0.25, 4.0, hidden).astype(np.float32)
    weight[rng.random(hidden) < 0.1] = 0.0
    weight[3 % hidden], weight[7 % hidden] = np.nan, -1.0
    label = np.repeat(rng.integers(0, 6, rows // 4 + 1), 4)[:rows].astype(np.int32)
    label[rng.random(rows) < 0.1] = -1
    return {"code": code, "hidden": hidden, "seg": seg, "weight": weight, "label": label}


@functools.lru_cache(maxsize=None)
def case_tables(n, weighted):
    """``(canon, terms)`` of case ``n`` (``n = "planted"``: the planted case) for every lag of ``ALL_LAGS``."""
    case = planted_case() if n == "planted" else similarity_case(n)
    canon = canonical(case["code"], case["hidden"], case["seg"], case["weight"] if weighted else None)
    return canon, all_terms(canon, case["seg"], ALL_LAGS)


def case_update(n, lags, metric, weighted=False, labelled=False, state=None):
    """``update`` of a shared case through its cached tables."""
    case = planted_case() if n == "planted" else similarity_case(n)
    canon, terms = case_tables(n, weighted)
    return update(case["code"], case["hidden"], lags, metric, case["seg"], case["weight"] if weighted else None,
                  case["label"] if labelled else None, state, canon, terms)


PLANTED = {"utterances": 12, "k": 16, "hidden": 512, "classes": 40, "replace": 4}


@functools.lru_cache(maxsize=None)
def planted_case():
    """12 utterances of 80 .. 110 frames (about 1164 in all, padding behind each), k = 16, H = 512.  An utterance is a
    chain of phone-like segments of 3 .. 12 frames; a segment has a base code of 16 features, and every frame of it
    replaces 4 of the 16 entries (25 %) by features drawn at random.  ``label`` is the phone of the frame, ``ref`` the
    flags of ``boundaries_from_labels``.  A few entries are spoiled and a few frames are unlabelled."""
    rng = np.random.default_rng(1164)
    k, hidden = PLANTED["k"], PLANTED["hidden"]
    vals, idx, seg, label = [], [], [], []
    for u in range(PLANTED["utterances"]):
        T, t, phone = int(rng.integers(80, 111)), 0, -1
        while t < T:
            d = min(int(rng.integers(3, 13)), T - t)
            if T - t - d < 3:
                d = T - t
            phone = int((phone + 1 + rng.integers(0, PLANTED["classes"] - 1)) % PLANTED["classes"])  # (never the same twice)
            base_f = rng.choice(hidden, k, replace=False)
            base_v = rng.uniform(0.5, 2.0, k).astype(np.float32)
            for _ in range(d):
                f, v = base_f.copy(), base_v.copy()
                at = rng.choice(k, PLANTED["replace"], replace=False)
                free = np.setdiff1d(np.arange(hidden), f)
                f[at] = rng.choice(free, PLANTED["replace"], replace=False)
                v[at] = rng.uniform(0.5, 2.0, PLANTED["replace"]).astype(np.float32)
                idx.append(f), vals.append(v), seg.append(u), label.append(phone)
            t += d
        for _ in range(int(rng.integers(1, 4))):  # padding behind the utterance
            idx.append(rng.choice(hidden, k, replace=False)), vals.append(np.ones(k, np.float32)), seg.append(-1), label.append(-1)
    vals, idx = np.asarray(vals, np.float32), np.asarray(idx, np.int32)
    seg, label = np.asarray(seg, np.int32), np.asarray(label, np.int32)
    rows = seg.size
    for r in rng.choice(rows, 12, replace=False):  # the spoiled entries: one of each kind on a few rows
        j = int(rng.integers(1, k))
        kind = int(rng.integers(0, 5))
        if kind == 0:
            idx[r, j] = idx[r, j - 1]
        elif kind == 1:
            vals[r, j] = -vals[r, j]
        elif kind == 2:
            vals[r, j] = np.nan
        elif kind == 3:
            idx[r, j] = -1
        else:
            idx[r, j] = hidden
    ref = reference_flags(label, seg)
    label = label.copy()
    label[rng.choice(rows, 10, replace=False)] = -1  # (the references were read off the full labels)
    weight = np.ones(hidden, np.float32)
    weight[rng.random(hidden) < 0.1] = 0.0
    return {"code": (vals, idx), "hidden": hidden, "seg": seg, "label": label, "ref": ref, "weight": weight}


def reference_flags(label, seg=None):
    """uint8 ``[rows]``: 1 at r where the label changes between r and r + 1, both labelled, both in one stretch."""
    label = np.asarray(label)
    out = np.zeros(label.shape[0], np.uint8)
    for r in range(label.shape[0] - 1):
        same_stretch = seg is None or (seg[r] >= 0 and seg[r + 1] == seg[r])
        out[r] = same_stretch and label[r] >= 0 and label[r + 1] >= 0 and label[r] != label[r + 1]
    return out


@functools.lru_cache(maxsize=None)
def planted_novelty():
    """float32 ``[rows]``: 1 - the lag-1 cosine of the planted case (NaN where there is no pair)."""
    sim, _ = case_update("planted", (1,), COSINE)
    return (np.float32(1.0) - sim[:, 0]).astype(np.float32)


def planted_thresholds(n=64):
    return np.linspace(0.0, 1.0, n).astype(np.float32)


# hand-worked sequences for the match: (novelty, reference rows, seg or None, threshold, tol) -> (pred, hit, ref, peaks).
# Row 0 of a flat start is a peak too (nothing lies to its left), below every threshold used here.
def sequence(length, peaks_at, low=0.1, high=0.9):
    nov = np.full(length, low, np.float32)
    nov[list(peaks_at)] = high
    return nov


HAND_SEQUENCES = (
    # a prediction at 10 between references at 9 and 11, tol 1: one hit, not two
    {"nov": sequence(16, (10,)), "ref": (9, 11), "seg": None, "thr": 0.5, "tol": 1, "want": (1, 1, 2, 2)},
    # references at 10 and 11, one prediction at 11: the prediction takes the earlier reference
    {"nov": sequence(16, (11,)), "ref": (10, 11), "seg": None, "thr": 0.5, "tol": 1, "want": (1, 1, 2, 2)},
    # tol 0: only the same row hits
    {"nov": sequence(16, (4, 10)), "ref": (4, 11), "seg": None, "thr": 0.5, "tol": 0, "want": (2, 1, 2, 3)},
    # a plateau 5..7 peaks once, at its first row; the reference at 7 is 2 away
    {"nov": np.array([0, 0, 0, 0, 0, .8, .8, .8, 0, 0], np.float32), "ref": (7,), "seg": None, "thr": 0.5, "tol": 1,
     "want": (1, 0, 1, 2)},
    # a stretch of length 1 (row 3) peaks when its value is a number; the padding row 4 does not count
    {"nov": np.array([.1, .9, .1, .7, .9, .1, .9, .1], np.float32), "ref": (1, 3, 4), "seg": (0, 0, 0, 1, -1, 2, 2, 2),
     "thr": 0.5, "tol": 0, "want": (3, 2, 2, 3)},
    # an all-NaN stretch predicts nothing and keeps its references
    {"nov": np.array([np.nan] * 5 + [.1, .9, .1], np.float32), "ref": (2, 6), "seg": (0, 0, 0, 0, 0, 1, 1, 1), "thr": 0.5,
     "tol": 1, "want": (1, 1, 2, 1)},
    # a NaN neighbour counts as -inf: rows 1 and 3 both peak; the reference at 2 goes to the prediction of its own stretch
    {"nov": np.array([.2, .6, np.nan, .7, .1, .1], np.float32), "ref": (2,), "seg": (0, 0, 0, 1, 1, 1), "thr": 0.5, "tol": 1,
     "want": (2, 1, 1, 2)},
    # more references than predictions within tol: one to one, in time order (predictions 3, 9; references 2, 3, 4, 8)
    {"nov": sequence(12, (3, 9)), "ref": (2, 3, 4, 8), "seg": None, "thr": 0.5, "tol": 1, "want": (2, 2, 4, 3)},
)


def hand_sequence(n):
    """-> ``(nov, ref uint8, seg int32 or None, thr float32 [1], tol, want)`` of ``HAND_SEQUENCES[n]``."""
    h = HAND_SEQUENCES[n]
    ref = np.zeros(h["nov"].size, np.uint8)
    ref[list(h["ref"])] = 1
    seg = None if h["seg"] is None else np.asarray(h["seg"], np.int32)
    return h["nov"], ref, seg, np.array([h["thr"]], np.float32), h["tol"], h["want"]
