"""numpy restatement of ABX discrimination (include/wsae.h, ``wsae_dtw_matrix`` and ``wsae_abx_count``; DESIGN.md
section 26): sequential loops that are the definition.  The frame cost of an a-frame and a b-frame is one chain of
float64 additions in the ascending entry position of the B frame, the dynamic program a plain double loop with the stated
tie-break, the count a plain triple loop; the kernels are compared with all of them bit for bit.  ``frame_costs`` walks
the same chain for all a-frames of a call at once (a column of independent chains: adding nothing to a chain leaves it as
it is), and tests/test_abx.py holds it against the literal ``pair_cost``.  Also the input recipes and case tables the CPU
and the GPU tests share."""

from __future__ import annotations

import functools
import math

import numpy as np

import runs_oracle as RO
from dynamics_oracle import COSINE, JACCARD, canonical, similarity_value  # noqa: F401 (similarity_value: tests/test_abx.py)

MAX_LEN, MAX_K = 64, 128
ANY, WITHIN, ACROSS = 0, 1, 2
MODES = {"any": ANY, "within": WITHIN, "across": ACROSS}
METRIC = {"cosine": COSINE, "jaccard": JACCARD}


# ---- frame costs ---------------------------------------------------------------------------------------------------------------
def similarity_f64(metric, s, matched, row_r, row_q):
    """The float64 similarity c of the contract (``dynamics_oracle.similarity_value`` is its float32 rounding)."""
    _, n_r, a_r = row_r
    _, n_q, a_q = row_q
    if metric == COSINE:
        c = 0.0
        if n_r != 0.0 and n_q != 0.0:
            c = s / math.sqrt(n_r * n_q)
            if not c <= 1.0:
                c = 1.0
        return c
    union = a_r + a_q - matched
    return matched / union if union else 0.0


def pair_terms_b(canon, r, q):
    """``(s, matched)`` of a-frame r and b-frame q: the chain of products in the entry order of row q."""
    there = dict(canon[r][0])
    s, matched = 0.0, 0
    for f, u in canon[q][0]:
        y = there.get(f)
        if y is not None:
            s += u * y
            matched += 1
    return s, matched


def pair_cost(canon, r, q, metric):
    """float32 ``e = float(1.0 - c)`` of a-frame r and b-frame q, literally."""
    s, matched = pair_terms_b(canon, r, q)
    return np.float32(1.0 - similarity_f64(metric, s, matched, canon[r], canon[q]))


def frame_costs(canon, a_rows, b_rows, metric, hidden):
    """float32 ``[len(a_rows), len(b_rows)]`` of ``pair_cost``: per b-frame one pass over its entries in ascending
    position, every a-frame's chain advanced where it holds the feature."""
    a_rows, b_rows = list(a_rows), list(b_rows)
    feats = sorted({f for r in a_rows for f, _ in canon[r][0]})
    col = {f: j for j, f in enumerate(feats)}
    U = np.zeros((len(a_rows), len(feats) + 1), np.float64)
    P = np.zeros((len(a_rows), len(feats) + 1), bool)
    for i, r in enumerate(a_rows):
        for f, u in canon[r][0]:
            U[i, col[f]], P[i, col[f]] = u, True
    n_r = np.array([canon[r][1] for r in a_rows], np.float64)
    a_r = np.array([canon[r][2] for r in a_rows], np.int64)
    out = np.empty((len(a_rows), len(b_rows)), np.float32)
    for j, q in enumerate(b_rows):
        s = np.zeros(len(a_rows), np.float64)
        inter = np.zeros(len(a_rows), np.int64)
        for f, u in canon[q][0]:
            c = col.get(f)
            if c is None:
                continue
            hit = P[:, c]
            s[hit] = s[hit] + u * U[hit, c]
            inter += hit
        _, n_q, a_q = canon[q]
        if metric == COSINE:
            ok = (n_r != 0.0) & (n_q != 0.0)
            with np.errstate(divide="ignore", invalid="ignore"):
                c = np.where(ok, s / np.sqrt(n_r * n_q), 0.0)
            c = np.where(c <= 1.0, c, 1.0)
        else:
            union = a_r + a_q - inter
            c = np.where(union != 0, inter / np.where(union != 0, union, 1).astype(np.float64), 0.0)
        out[:, j] = (1.0 - c).astype(np.float32)
    return out


# ---- the dynamic program --------------------------------------------------------------------------------------------------------
PREFERENCE = ((-1, -1), (-1, 0), (0, -1))  # ties go to the earlier one


def dtw(e, preference=PREFERENCE):
    """``(D[n-1][m-1] float64, L[n-1][m-1])`` of the cost matrix ``e`` float32 ``[n, m]``: a plain double loop."""
    n, m = e.shape
    D = [[0.0] * m for _ in range(n)]
    L = [[0] * m for _ in range(n)]
    for i in range(n):
        for j in range(m):
            if i == 0 and j == 0:
                D[0][0], L[0][0] = float(e[0, 0]), 1
                continue
            best = None
            for di, dj in preference:
                pi, pj = i + di, j + dj
                if pi < 0 or pj < 0:
                    continue
                if best is None or D[pi][pj] < D[best[0]][best[1]]:
                    best = (pi, pj)
            D[i][j] = float(e[i, j]) + D[best[0]][best[1]]
            L[i][j] = L[best[0]][best[1]] + 1
    return D[n - 1][m - 1], L[n - 1][m - 1]


def item_ok(start, length, rows):
    return 1 <= length <= MAX_LEN and start >= 0 and start + length <= rows


def dtw_tables(code, hidden, a_items, b_items, metric, seg=None, weight=None, preference=PREFERENCE):
    """``(D float64 [n_a, n_b], L int64 [n_a, n_b])`` of the end cells; NaN and 0 for a pair with an invalid item.
    ``a_items`` / ``b_items``: ``(starts, lengths)``."""
    rows = np.asarray(code[0]).shape[0]
    canon = canonical(code, hidden, seg, weight)
    a_st, a_ln = (np.asarray(x).astype(np.int64) for x in a_items)
    b_st, b_ln = (np.asarray(x).astype(np.int64) for x in b_items)
    a_ok = [item_ok(s, n, rows) for s, n in zip(a_st, a_ln)]
    b_ok = [item_ok(s, n, rows) for s, n in zip(b_st, b_ln)]
    a_rows = sorted({r for s, n, ok in zip(a_st, a_ln, a_ok) if ok for r in range(s, s + n)})
    b_rows = sorted({r for s, n, ok in zip(b_st, b_ln, b_ok) if ok for r in range(s, s + n)})
    D = np.full((a_st.size, b_st.size), np.nan, np.float64)
    L = np.zeros((a_st.size, b_st.size), np.int64)
    if not a_rows or not b_rows:
        return D, L
    cost = frame_costs(canon, a_rows, b_rows, metric, hidden)
    a_at, b_at = {r: i for i, r in enumerate(a_rows)}, {r: i for i, r in enumerate(b_rows)}
    for ia in range(a_st.size):
        if not a_ok[ia]:
            continue
        ra = [a_at[r] for r in range(a_st[ia], a_st[ia] + a_ln[ia])]
        for ib in range(b_st.size):
            if not b_ok[ib]:
                continue
            cb = [b_at[r] for r in range(b_st[ib], b_st[ib] + b_ln[ib])]
            D[ia, ib], L[ia, ib] = dtw(cost[np.ix_(ra, cb)], preference)
    return D, L


def distances(D, L, normalize):
    """``(dist float32, steps int32)`` of the outputs from the end cells."""
    with np.errstate(invalid="ignore", divide="ignore"):
        d = D / np.where(L > 0, L, 1).astype(np.float64) if normalize else D
    return np.where(L > 0, d, np.nan).astype(np.float32), L.astype(np.int32)


def dtw_matrix(code, hidden, a_items, b_items, metric=COSINE, normalize=True, seg=None, weight=None):
    """One call of ``wsae_dtw_matrix`` -> ``(dist float32 [n_a, n_b], steps int32 [n_a, n_b])``."""
    return distances(*dtw_tables(code, hidden, a_items, b_items, metric, seg, weight), normalize)


# ---- the triple count -------------------------------------------------------------------------------------------------------------
def takes_part(i, cat, ctx, spk, n_cats, mode):
    return 0 <= cat[i] < n_cats and (ctx is None or ctx[i] >= 0) and (mode == ANY or spk[i] >= 0)


def abx_count(dist, x_lo, n_x, cat, ctx, spk, n_cats, mode):
    """One call of ``wsae_abx_count`` on zero tables -> ``(wins2 int64 [n_cats, n_cats], total, skipped int)``;
    ``dist [n_x, >= n_items]`` holds the rows of the window.  A plain triple loop."""
    n = len(cat)
    wins2, total, skipped = np.zeros((n_cats, n_cats), np.int64), np.zeros((n_cats, n_cats), np.int64), 0
    part = [takes_part(i, cat, ctx, spk, n_cats, mode) for i in range(n)]
    for xr in range(n_x):
        x = x_lo + xr
        if not part[x]:
            continue
        for a in range(n):
            if a == x or not part[a] or cat[a] != cat[x] or (ctx is not None and ctx[a] != ctx[x]):
                continue
            if (mode == WITHIN and spk[a] != spk[x]) or (mode == ACROSS and spk[a] == spk[x]):
                continue
            for b in range(n):
                if b == x or b == a or not part[b] or cat[b] == cat[x] or (ctx is not None and ctx[b] != ctx[x]):
                    continue
                if mode != ANY and spk[b] != spk[a]:
                    continue
                da, db = dist[xr, a], dist[xr, b]
                if np.isnan(da) or np.isnan(db):
                    skipped += 1
                    continue
                total[cat[x], cat[b]] += 1
                wins2[cat[x], cat[b]] += 2 if da < db else (1 if da == db else 0)
    return wins2, total, skipped


def tied_triples(dist, cat, ctx, spk, n_cats, mode):
    """``(ties, counted)``: the counted triples with ``dist[x][a] == dist[x][b]``, and all counted triples."""
    wins2, total, _ = abx_count(dist, 0, len(cat), cat, ctx, spk, n_cats, mode)
    w_lt, _, _ = abx_count_strict(dist, cat, ctx, spk, n_cats, mode)
    return int((wins2 - 2 * w_lt).sum()), int(total.sum())


def abx_count_strict(dist, cat, ctx, spk, n_cats, mode):
    """The count with a tie scored 0: ``(wins int64, total, skipped)`` of the strict ``<`` alone."""
    n = len(cat)
    wins, total, skipped = np.zeros((n_cats, n_cats), np.int64), np.zeros((n_cats, n_cats), np.int64), 0
    part = [takes_part(i, cat, ctx, spk, n_cats, mode) for i in range(n)]
    for x in range(n):
        if not part[x]:
            continue
        for a in range(n):
            if a == x or not part[a] or cat[a] != cat[x] or (ctx is not None and ctx[a] != ctx[x]):
                continue
            if (mode == WITHIN and spk[a] != spk[x]) or (mode == ACROSS and spk[a] == spk[x]):
                continue
            for b in range(n):
                if b == x or b == a or not part[b] or cat[b] == cat[x] or (ctx is not None and ctx[b] != ctx[x]):
                    continue
                if mode != ANY and spk[b] != spk[a]:
                    continue
                da, db = dist[x, a], dist[x, b]
                if np.isnan(da) or np.isnan(db):
                    skipped += 1
                    continue
                total[cat[x], cat[b]] += 1
                wins[cat[x], cat[b]] += 1 if da < db else 0
    return wins, total, skipped


def scores(wins2, total):
    """``(score float64 [n_cats, n_cats] with NaN where total == 0, error)``: score = wins2 / (2 total), error = 1 - the
    mean of score over the cells with total > 0 (NaN without any)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        score = np.where(total > 0, wins2 / (2.0 * np.where(total > 0, total, 1)), np.nan)
    return score, (1.0 - float(np.nanmean(score)) if (total > 0).any() else math.nan)


# ---- items from labels --------------------------------------------------------------------------------------------------------------
def items_from_labels(labels, seg=None, min_len=1, max_len=MAX_LEN, n_classes=None):
    """``(starts, lengths, category, context, dropped_short, dropped_long)`` of flat labels: a maximal run of one label
    >= 0 inside one stretch of equal ``seg >= 0``; context = (previous label + 1) (n_classes + 1) + (next label + 1), the
    neighbours being the runs next to it in the same stretch (a run of labels < 0 and the edge count as none = -1)."""
    labels = np.asarray(labels).astype(np.int64)
    rows = labels.size
    if n_classes is None:
        n_classes = int(labels.max()) + 1 if rows and labels.max() >= 0 else 1
    runs, r = [], 0
    while r < rows:
        a = r
        while r + 1 < rows and labels[r + 1] == labels[a] and (seg is None or seg[r + 1] == seg[a]):
            r += 1
        runs.append((a, r - a + 1, int(labels[a]) if seg is None or seg[a] >= 0 else -1, 0 if seg is None else int(seg[a])))
        r += 1
    out, short, long_ = [], 0, 0
    for i, (a, n, lab, s) in enumerate(runs):
        if lab < 0:
            continue
        if n < min_len:
            short += 1
            continue
        if n > max_len:
            long_ += 1
            continue
        prev = runs[i - 1][2] if i > 0 and runs[i - 1][3] == s else -1
        nxt = runs[i + 1][2] if i + 1 < len(runs) and runs[i + 1][3] == s else -1
        out.append((a, n, lab, (max(prev, -1) + 1) * (n_classes + 1) + max(nxt, -1) + 1))
    arr = np.asarray(out, np.int64).reshape(-1, 4)
    return arr[:, 0], arr[:, 1], arr[:, 2], arr[:, 3], short, long_


# ---- the inputs the CPU and the GPU tests share -----------------------------------------------------------------------------------
# (rows, k, hidden, n_a, n_b): small hidden forces dense matches and table collisions; 65 and 128 take two entries per lane
DIST_SHAPES = ((40, 1, 2, 20, 20), (300, 5, 32, 7, 131), (3000, 32, 3072, 7, 131), (700, 64, 256, 6, 40), (700, 65, 256, 6, 40),
               (600, 128, 64, 6, 40))
TIE_CASE = 0


def dense_code(rng, rows, k, hidden):
    """A code whose rows draw their k indices with repeats (k may exceed hidden) and keep about half of the previous row."""
    idx = rng.integers(0, hidden, (rows, k)).astype(np.int32)
    keep = rng.random((rows, k)) < 0.5
    for r in range(1, rows):
        idx[r, keep[r]] = idx[r - 1, keep[r]]
    vals = (np.abs(rng.standard_normal((rows, k))) + 0.05).astype(np.float32)
    return vals, idx


def make_items(rng, rows, n, invalid=True):
    """``(starts, lengths) int32 [n]``: lengths 1, 2, 63 and 64 where the rows allow, short lengths of 3 .. 13 otherwise
    (so that the b-frames of consecutive items straddle every multiple of 64 lanes), two items that are identical, two
    that overlap, and (``invalid``) one of every invalid kind: length 0, length 65, a negative start, past the end."""
    lengths = [n_ for n_ in (64, 1, 63, 2) if n_ <= rows][:max(n - 1, 0)]
    while len(lengths) < n:
        lengths.append(int(rng.integers(3, min(14, rows + 1))))
    lengths = np.asarray(lengths[:n], np.int64)
    starts = np.array([int(rng.integers(0, rows - ln + 1)) for ln in lengths], np.int64)
    if n >= 12:
        starts[5], lengths[5] = starts[4], lengths[4]                      # identical
        starts[7], lengths[7] = min(starts[6] + 1, rows - lengths[6]), lengths[6]  # overlapping
        if invalid:
            lengths[8] = 0
            lengths[9] = MAX_LEN + 1
            starts[10] = -1
            starts[11] = rows - lengths[11] + 1
    return starts.astype(np.int32), lengths.astype(np.int32)


@functools.lru_cache(maxsize=None)
def distance_case(n):
    """Case ``n`` of ``DIST_SHAPES`` -> dict with ``code`` (spoiled: NaN, values <= 0, repeated and out-of-range indices;
    no +inf), ``hidden``, ``seg`` (about 5 % padding rows, so items hold padding), ``weight`` (zeros, a NaN and a negative
    among positive weights), ``a`` and ``b`` (the item lists)."""
    rows, k, hidden, n_a, n_b = DIST_SHAPES[n]
    rng = np.random.default_rng(2500 + n)
    if n == TIE_CASE:
        vals, idx = np.ones((rows, k), np.float32), rng.integers(0, hidden, (rows, k)).astype(np.int32)
        seg = np.zeros(rows, np.int32)
        weight = np.ones(hidden, np.float32)
        lengths = rng.integers(3, 9, n_a).astype(np.int32)
        starts = np.array([rng.integers(0, rows - ln + 1) for ln in lengths], np.int32)
        return {"code": (vals, idx), "hidden": hidden, "seg": seg, "weight": weight, "a": (starts, lengths), "b": (starts, lengths)}
    vals, idx = dense_code(rng, rows, k, hidden) if hidden < k else RO.persistent_code(rng, rows, k, hidden)
    vals, idx = RO.spoil(rng, (vals, idx), hidden)
    vals[rng.random(vals.shape) < 0.01] = np.nan
    vals[np.isinf(vals)] = 1.0
    seg = (np.arange(rows) * 3 // rows).astype(np.int32)
    seg[rng.random(rows) < 0.05] = -1
    weight = rng.uniform(0.25, 4.0, hidden).astype(np.float32)
    weight[rng.random(hidden) < 0.1] = 0.0
    weight[3 % hidden], weight[7 % hidden] = np.nan, -1.0
    return {"code": (vals.astype(np.float32), idx.astype(np.int32)), "hidden": hidden, "seg": seg, "weight": weight,
            "a": make_items(rng, rows, n_a, invalid=False) if n_a < 12 else make_items(rng, rows, n_a),
            "b": make_items(rng, rows, n_b)}


@functools.lru_cache(maxsize=None)
def case_tables(n, metric, weighted, reverse=False):
    """``(D, L)`` of distance case ``n``."""
    c = distance_case(n)
    return dtw_tables(c["code"], c["hidden"], c["a"], c["b"], metric, c["seg"], c["weight"] if weighted else None,
                      PREFERENCE[::-1] if reverse else PREFERENCE)


def case_distances(n, metric, weighted, normalize):
    return distances(*case_tables(n, metric, weighted), normalize)


# the planted ABX case: 6 utterances, 5 classes, k = 8, hidden = 64, items of 2 .. 6 frames
PLANTED = {"utterances": 6, "classes": 5, "k": 8, "hidden": 64, "items": 16}


@functools.lru_cache(maxsize=None)
def planted_case(core, shuffled=False):
    """Every frame of an item of class c holds the ``core`` features ``c core .. c core + core - 1`` and ``k - core``
    features drawn afresh from the rest of the dictionary; values uniform in [0.5, 2).  -> dict with ``code``, ``hidden``,
    ``seg``, ``label`` (one run per item, runs of the same class never adjacent), ``items`` (starts, lengths, category),
    ``speaker`` (the utterance modulo 3) per item.  ``shuffled``: the categories of the items permuted at random."""
    rng = np.random.default_rng(2525 + core)
    k, hidden, n_cls = PLANTED["k"], PLANTED["hidden"], PLANTED["classes"]
    rest = np.arange(n_cls * 3, hidden)
    vals, idx, seg, label, items, speaker = [], [], [], [], [], []
    for u in range(PLANTED["utterances"]):
        c = -1
        for _ in range(PLANTED["items"]):
            c = int((c + 1 + rng.integers(0, n_cls - 1)) % n_cls)
            n = int(rng.integers(2, 7))
            items.append((len(vals), n, c))
            speaker.append(u % 3)
            for _ in range(n):
                f = np.concatenate([np.arange(c * core, c * core + core), rng.choice(rest, k - core, replace=False)])
                order = rng.permutation(k)
                idx.append(f[order]), vals.append(rng.uniform(0.5, 2.0, k).astype(np.float32))
                seg.append(u), label.append(c)
    items = np.asarray(items, np.int64)
    cat = items[:, 2].copy()
    if shuffled:
        cat = cat[rng.permutation(cat.size)]
    return {"code": (np.asarray(vals, np.float32), np.asarray(idx, np.int32)), "hidden": hidden, "seg": np.asarray(seg, np.int32),
            "label": np.asarray(label, np.int32), "items": (items[:, 0].astype(np.int32), items[:, 1].astype(np.int32), cat.astype(np.int32)),
            "speaker": np.asarray(speaker, np.int32)}


@functools.lru_cache(maxsize=None)
def planted_distances(core, metric=COSINE):
    c = planted_case(core)
    it = (c["items"][0], c["items"][1])
    return dtw_matrix(c["code"], c["hidden"], it, it, metric, True, c["seg"])[0]


def planted_error(core, shuffled=False):
    c = planted_case(core, shuffled)
    wins2, total, _ = abx_count(planted_distances(core), 0, len(c["items"][2]), c["items"][2], None, None, PLANTED["classes"], ANY)
    return scores(wins2, total)[1]


# the count case: about 150 items, 5 categories, 3 contexts, 4 speakers; ids out of range and negative; NaN rows
COUNT = {"items": 150, "cats": 5, "contexts": 3, "speakers": 4}


@functools.lru_cache(maxsize=None)
def count_case(tied=False):
    """-> dict with ``dist`` float32 [n, n] (``tied``: the Jaccard distances of the tie case tiled, else distinct random
    values that lean towards the category, with NaN rows and columns), ``cat``, ``ctx``, ``spk`` int32 [n], ``n_cats``."""
    rng = np.random.default_rng(2550 + tied)
    n, n_cats = COUNT["items"], COUNT["cats"]
    cat = rng.integers(0, n_cats, n).astype(np.int32)
    ctx = rng.integers(0, COUNT["contexts"], n).astype(np.int32)
    spk = rng.integers(0, COUNT["speakers"], n).astype(np.int32)
    cat[rng.choice(n, 6, replace=False)] = np.array([-1, n_cats, n_cats + 7, -3, n_cats, -1], np.int32)
    ctx[rng.choice(n, 3, replace=False)] = -1
    spk[rng.choice(n, 3, replace=False)] = -2
    if tied:
        small = distances(*case_tables(TIE_CASE, JACCARD, False), True)[0]
        reps = -(-n // small.shape[0])
        dist = np.tile(small, (reps, reps))[:n, :n].copy()
    else:
        same = cat[:, None] == cat[None, :]
        dist = (rng.random((n, n)) * 0.8 + np.where(same, 0.0, 0.15)).astype(np.float32)
        bad = rng.choice(n, 4, replace=False)
        dist[bad, :] = np.nan
        dist[:, bad[:2]] = np.nan
    return {"dist": dist.astype(np.float32), "cat": cat, "ctx": ctx, "spk": spk, "n_cats": n_cats}


@functools.lru_cache(maxsize=None)
def count_result(tied, mode, with_ctx=True):
    c = count_case(tied)
    return abx_count(c["dist"], 0, COUNT["items"], c["cat"], c["ctx"] if with_ctx else None, c["spk"], c["n_cats"], mode)


def all_monotone_paths(n, m):
    """Every path from (0, 0) to (n - 1, m - 1) by the steps (1, 1), (1, 0), (0, 1), as lists of cells."""
    def walk(i, j):
        if i == n - 1 and j == m - 1:
            yield [(i, j)]
            return
        for di, dj in ((1, 1), (1, 0), (0, 1)):
            if i + di < n and j + dj < m:
                for rest in walk(i + di, j + dj):
                    yield [(i, j)] + rest
    return list(walk(0, 0))

