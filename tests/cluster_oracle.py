"""Sequential numpy statement of code clustering: ``wsae_cluster_assign`` and
``wsae_cluster_accumulate`` as literal loops - ``np.float32`` multiply then add per entry, one float64 chain for the
norm, Python integers for the state - a literal Lloyd loop on them, the scores of a contingency table, and the inputs the
CPU and the GPU tests share."""

from __future__ import annotations

import functools
import math

import numpy as np

MAX_K, MAX_CLUSTERS = 128, 1024
Q_SCALE, Q_CLIP = np.float32(1048576.0), np.float32(4096.0)
F32 = np.float32


# ---- the two definitions ------------------------------------------------------------------------------------------------------
def row_entries(vals_row, idx_row, hidden, col_of=None):
    """``[(value, column)]`` of the first-active entries of one row that have a column, in ascending entry position."""
    seen, out = set(), []
    for v, f in zip(vals_row, idx_row):
        f = int(f)
        if not v > 0:  # (NaN is not)
            continue
        if f in seen:
            continue
        seen.add(f)
        if not 0 <= f < hidden:
            continue
        col = f if col_of is None else int(col_of[f])
        if col >= 0:
            out.append((F32(v), col))
    return out


def quantise_b(b):
    return int(np.rint(np.minimum(np.maximum(F32(b), -Q_CLIP), Q_CLIP) * Q_SCALE))


def empty_state(n_clusters, n_classes=0):
    return {"count": [0] * n_clusters, "best_q": [0] * n_clusters,
            "contingency": [[0] * n_classes for _ in range(n_clusters)], "totals": [0, 0, 0]}


def assign(code, hidden, Ct, n_clusters, seg=None, col_of=None, bias=None, normalize=False, labels=None, n_classes=0,
           state=None):
    """``(assign int32, best, second, inv_norm float32 [rows], state)``; ``Ct [n_cols, >= n_clusters]`` float32."""
    vals, idx = code
    rows = vals.shape[0]
    C = n_clusters
    assert not (normalize and bias is not None)
    state = empty_state(C, n_classes if labels is not None else 0) if state is None else state
    a_out = np.full(rows, -1, np.int32)
    best, second, inv_norm = (np.zeros(rows, np.float32) for _ in range(3))
    Ct = np.asarray(Ct, np.float32)
    with np.errstate(all="ignore"):
        for r in range(rows):
            if seg is not None and seg[r] < 0:
                continue
            ent = row_entries(vals[r], idx[r], hidden, col_of)
            if not ent:
                state["totals"][1] += 1
                continue
            score = np.zeros(C, np.float32) if bias is None else np.asarray(bias, np.float32)[:C].copy()
            n = np.float64(0.0)
            for v, col in ent:
                prod = v * Ct[col, :C]  # an fp32 multiply
                score = score + prod    # and then an fp32 add
                n = n + np.float64(v) * np.float64(v)
            a = int(np.argmax(score))  # (the lowest index at the maximum)
            b1 = score[a]
            if C > 1:
                others = np.delete(np.arange(C), a)
                a2 = int(others[np.argmax(score[others])])
                b2 = score[a2]
            else:
                b2 = F32(-np.inf)
            inv = F32(np.float64(1.0) / np.sqrt(n))
            b = b1 * inv if normalize else b1
            a_out[r], best[r], second[r], inv_norm[r] = a, b1, b2, inv
            state["count"][a] += 1
            state["best_q"][a] += quantise_b(b)
            state["totals"][0] += 1
            if labels is not None and 0 <= int(labels[r]) < n_classes:
                state["totals"][2] += 1
                state["contingency"][a][int(labels[r])] += 1
    return a_out, best, second, inv_norm, state


def plan(code, hidden, seg=None, col_of=None, n_cols=None):
    """The transposition of ``wsae_probe_plan``: ``(col_ptr [n_cols + 1], t_row, t_val)``, columns ascending and rows
    ascending within a column."""
    vals, idx = code
    P = hidden if n_cols is None else n_cols
    lists = [[] for _ in range(P)]
    for r in range(vals.shape[0]):
        if seg is not None and seg[r] < 0:
            continue
        for v, col in row_entries(vals[r], idx[r], hidden, col_of):
            lists[col].append((r, v))
    col_ptr = np.zeros(P + 1, np.int64)
    col_ptr[1:] = np.cumsum([len(x) for x in lists])
    flat = [e for x in lists for e in x]
    return (col_ptr, np.asarray([e[0] for e in flat], np.int32).reshape(-1),
            np.asarray([e[1] for e in flat], np.float32).reshape(-1))


def accumulate(col_ptr, t_row, t_val, cap, assign_rows, n_clusters, n_rows=None, row_weight=None, S_q=None):
    """``S_q``: a list of ``n_cols`` lists of ``n_clusters`` Python integers, added to in place when given."""
    P = len(col_ptr) - 1
    n_rows = len(assign_rows) if n_rows is None else n_rows
    S_q = [[0] * n_clusters for _ in range(P)] if S_q is None else S_q
    with np.errstate(all="ignore"):
        for p in range(P):
            for i in range(min(int(col_ptr[p]), cap), min(int(col_ptr[p + 1]), cap)):
                r = int(t_row[i])
                if not 0 <= r < n_rows:
                    continue
                c = int(assign_rows[r])
                if not 0 <= c < n_clusters:
                    continue
                x = F32(t_val[i])
                if row_weight is not None:
                    x = x * F32(row_weight[r])  # one fp32 product
                if not x > 0:
                    continue
                S_q[p][c] += int(np.rint(np.minimum(x, Q_CLIP) * Q_SCALE))
    return S_q


def same_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert bad.size == 0, (what, bad[:5], got[bad[:5]], want[bad[:5]])


def state_arrays(state):
    """The state as int64 numpy arrays."""
    C = len(state["count"])
    cont = np.asarray(state["contingency"], np.int64).reshape(C, -1)
    return {"count": np.asarray(state["count"], np.int64), "best_q": np.asarray(state["best_q"], np.int64),
            "contingency": cont, "totals": np.asarray(state["totals"], np.int64)}


# ---- a literal Lloyd loop -----------------------------------------------------------------------------------------------------
def dense_row(vals_row, idx_row, hidden, col_of, n_cols):
    x = np.zeros(n_cols, np.float64)
    for v, col in row_entries(vals_row, idx_row, hidden, col_of):
        x[col] = np.float64(v)
    return x


def finish_centroid(c64, metric):
    """float32 ``[n_cols]`` from the float64 mean: divided by its float64 norm for cosine, rounded once."""
    if metric == "cosine":
        nrm = math.sqrt(float(np.sum(c64 * c64)))
        c64 = c64 / nrm if nrm > 0 else c64
    return c64.astype(np.float32)


def euclid_bias(Ct, n_clusters):
    c = np.asarray(Ct, np.float32)[:, :n_clusters].astype(np.float64)
    return (-0.5 * np.sum(c * c, axis=0)).astype(np.float32)


def update_centroids(S_q, count, Ct_old, metric):
    """``Ct [n_cols, n_clusters]`` float32 from the integers; a cluster with count 0 keeps its old column."""
    P, C = len(S_q), len(count)
    Ct = np.array(Ct_old, np.float32)[:, :C].copy()
    for c in range(C):
        if count[c] == 0:
            continue
        col = np.asarray([np.float64(S_q[p][c]) for p in range(P)], np.float64) / (np.float64(count[c]) * np.float64(2.0 ** 20))
        Ct[:, c] = finish_centroid(col, metric)
    return Ct


def sample_rows(code, hidden, seg, col_of, n_clusters, seed):
    """``n_clusters`` distinct non-empty frames: a seeded permutation of the non-empty frames, its head in ascending
    row order."""
    import torch
    vals, idx = code
    ok = [r for r in range(vals.shape[0]) if (seg is None or seg[r] >= 0) and row_entries(vals[r], idx[r], hidden, col_of)]
    perm = torch.randperm(len(ok), generator=torch.Generator().manual_seed(int(seed))).tolist()
    return sorted(ok[j] for j in perm[:n_clusters])


def init_sample(code, hidden, seg, col_of, n_cols, n_clusters, metric, seed):
    rows = sample_rows(code, hidden, seg, col_of, n_clusters, seed)
    Ct = np.zeros((n_cols, n_clusters), np.float32)
    for c, r in enumerate(rows):
        Ct[:, c] = finish_centroid(dense_row(code[0][r], code[1][r], hidden, col_of, n_cols), metric)
    return Ct


def lloyd(code, hidden, n_clusters, metric="cosine", seg=None, col_of=None, n_cols=None, seed=0, max_iter=20, Ct=None):
    """The literal loop: assign, accumulate, update - until no assignment changes.  Returns ``(Ct, assign, iterations,
    counts)``; no re-seeding: a cluster that empties keeps its centroid."""
    P = hidden if n_cols is None else n_cols
    Ct = init_sample(code, hidden, seg, col_of, P, n_clusters, metric, seed) if Ct is None else Ct
    col_ptr, t_row, t_val = plan(code, hidden, seg, col_of, P)
    prev, it = None, 0
    for it in range(1, max_iter + 1):
        bias = euclid_bias(Ct, n_clusters) if metric == "euclidean" else None
        a, _, _, inv, st = assign(code, hidden, Ct, n_clusters, seg, col_of, bias, metric == "cosine")
        if prev is not None and np.array_equal(a, prev):
            break
        S_q = accumulate(col_ptr, t_row, t_val, t_row.size, a, n_clusters, row_weight=inv if metric == "cosine" else None)
        Ct = update_centroids(S_q, st["count"], Ct, metric)
        prev = a
    return Ct, a, it, st["count"]


# ---- the scores of a contingency table ----------------------------------------------------------------------------------------
def scores(table):
    """dict of the scores of an int table ``[clusters, classes]`` in float64."""
    t = np.asarray(table, np.float64)
    n = t.sum()
    rows, cols = t.sum(1), t.sum(0)

    def entropy(m):
        p = m[m > 0] / n
        return float(-(p * np.log(p)).sum())

    h_k, h_c = entropy(rows), entropy(cols)
    nz = t > 0
    mi = float((t[nz] / n * np.log(t[nz] * n / np.outer(rows, cols)[nz])).sum())
    hom = 1.0 if h_c == 0 else mi / h_c          # = 1 - H(class | cluster) / H(class)
    com = 1.0 if h_k == 0 else mi / h_k
    comb2 = lambda x: x * (x - 1.0) / 2.0
    s_ij, s_a, s_b = comb2(t).sum(), comb2(rows).sum(), comb2(cols).sum()
    expected, max_index = s_a * s_b / comb2(n), 0.5 * (s_a + s_b)
    return {"n": int(n), "cluster_purity": float(t.max(1).sum() / n), "class_purity": float(t.max(0).sum() / n),
            "mutual_information": mi, "pnmi": mi / h_c if h_c > 0 else math.nan,
            "nmi": 2.0 * mi / (h_k + h_c) if h_k + h_c > 0 else math.nan,
            "v_measure": 2.0 * hom * com / (hom + com) if hom + com > 0 else 0.0,
            "ari": float((s_ij - expected) / (max_index - expected)) if max_index != expected else 1.0,
            "best_class": t.argmax(1)}


def table_of(a, b, n_a, n_b):
    t = np.zeros((n_a, n_b), np.int64)
    for x, y in zip(a, b):
        if x >= 0 and y >= 0:
            t[x, y] += 1
    return t


def unit_sequences(assign_rows, seg):
    """``(units, lengths, utterance ids)``: runs of equal units within an utterance; -1 dropped (it also ends a run)."""
    units, lengths, utts = [], [], []
    prev_u, prev_s = -1, None
    for a, s in zip(assign_rows, seg):
        a, s = int(a), int(s)
        if a < 0 or s < 0:
            prev_u, prev_s = -1, None
            continue
        if a == prev_u and s == prev_s:
            lengths[-1] += 1
        else:
            units.append(a), lengths.append(1), utts.append(s)
        prev_u, prev_s = a, s
    return np.asarray(units, np.int64), np.asarray(lengths, np.int64), np.asarray(utts, np.int64)


# ---- the inputs the CPU and the GPU tests share -------------------------------------------------------------------------------
# name: (rows, k, hidden, n_cols or None, n_clusters, n_classes, segments, ties, all-rows feature)
CASES = {
    "one": (1, 1, 32, None, 1, 3, 1, False, False),
    "two": (257, 16, 96, None, 2, 5, 9, False, False),
    "c63": (300, 64, 256, None, 63, 7, 3, False, False),
    "c64": (300, 65, 256, None, 64, 40, 3, False, False),
    "c65": (300, 128, 256, None, 65, 40, 4, False, False),
    "c100": (500, 16, 512, None, 100, 40, 5, False, True),
    "ties": (400, 16, 128, None, 6, 4, 4, True, False),
    "wide": (2000, 32, 40960, 512, 1024, 41, 7, False, False),
}
LDC_EXTRA = 5  # columns of junk behind the clusters in Ct and S_q
# (bias, normalize, labels, seg)
COMBOS = ((False, True, True, True), (True, False, False, True), (False, False, True, False))


@functools.lru_cache(maxsize=None)
def case(name):
    rows, k, hidden, n_cols, C, n_classes, n_seg, ties, all_rows = CASES[name]
    rng = np.random.default_rng(2400 + sorted(CASES).index(name))
    if n_cols is None:
        col_of, P, pool = None, hidden, np.arange(hidden)
    else:
        feats = np.sort(rng.choice(hidden, n_cols, replace=False))
        col_of = np.full(hidden, -1, np.int32)
        col_of[feats] = rng.permutation(n_cols).astype(np.int32)
        P = n_cols
        pool = np.concatenate([feats, rng.choice(hidden, n_cols // 4, replace=False)])  # mostly features with a column
    vals = rng.uniform(0.1, 3.0, (rows, k)).astype(np.float32)
    idx = np.stack([rng.choice(pool, k, replace=False) for _ in range(rows)]).astype(np.int32)
    seg = (np.arange(rows) * n_seg // rows).astype(np.int32)
    if rows > 1:
        spoil = rng.random((rows, k))
        vals[spoil < 0.03] *= -1
        vals[(spoil >= 0.03) & (spoil < 0.04)] = 0.0
        vals[(spoil >= 0.04) & (spoil < 0.05)] = np.nan
        vals[(spoil >= 0.05) & (spoil < 0.055)] = 5000.0  # above the clip of the quantisation
        idx[(spoil >= 0.06) & (spoil < 0.07)] = -1
        idx[(spoil >= 0.07) & (spoil < 0.08)] = hidden
        if k > 1:
            dup = np.nonzero(rng.random(rows) < 0.1)[0]
            j = rng.integers(1, k, dup.size)
            idx[dup, j] = idx[dup, j - 1]
        silent = rng.random(rows) < 0.04
        vals[silent] = -np.abs(vals[silent])
        silent[0] = False
        seg[rng.random(rows) < 0.05] = -1
        if all_rows:
            for r in range(rows):  # feature 0 fires on every row (silent rows stay silent)
                at = np.nonzero(idx[r] == 0)[0]
                if at.size == 0:
                    idx[r, 0] = 0
                    at = [0]
                if not silent[r]:
                    vals[r, at[0]] = abs(vals[r, at[0]]) if vals[r, at[0]] > 0 else F32(1.0)
                    idx[r, :at[0]][idx[r, :at[0]] == 0] = 1
    Ct = np.full((P, C + LDC_EXTRA), 1e30, np.float32)
    Ct[:, :C] = rng.normal(0, 1, (P, C)).astype(np.float32)
    if ties:
        Ct[:, 3] = Ct[:, 1]  # clusters 1 and 3 tie exactly wherever one of them wins
        Ct[:, 5] = Ct[:, 1]
    bias = rng.normal(0, 0.5, C).astype(np.float32)
    if ties:
        bias[3] = bias[5] = bias[1]
    labels = np.repeat(rng.integers(0, n_classes, rows // 4 + 1), 4)[:rows].astype(np.int32)
    if rows > 1:
        out = rng.random(rows)
        labels[out < 0.05] = -1
        labels[(out >= 0.05) & (out < 0.08)] = n_classes
    return {"code": (vals, idx), "hidden": hidden, "col_of": col_of, "n_cols": P, "n_clusters": C, "n_classes": n_classes,
            "seg": seg, "Ct": Ct, "bias": bias, "labels": labels, "k": k, "rows": rows}


@functools.lru_cache(maxsize=None)
def case_assign(name, combo):
    """``assign`` of a shared case under ``COMBOS[combo]``."""
    c = case(name)
    with_bias, normalize, labelled, with_seg = COMBOS[combo]
    return assign(c["code"], c["hidden"], c["Ct"], c["n_clusters"], c["seg"] if with_seg else None, c["col_of"],
                  c["bias"] if with_bias else None, normalize, c["labels"] if labelled else None, c["n_classes"])


@functools.lru_cache(maxsize=None)
def case_plan(name, with_seg=True):
    c = case(name)
    return plan(c["code"], c["hidden"], c["seg"] if with_seg else None, c["col_of"], c["n_cols"])


PLANTED = {"rows": 1181, "utterances": 12, "k": 16, "hidden": 512, "prototypes": 8, "replace": 4, "seed": 1062}


@functools.lru_cache(maxsize=None)
def planted_case(seed=None):
    """12 utterances (1157 frames, two padding rows behind each: 1181 rows), k = 16, H = 512.  An utterance is a chain
    of runs of 3 .. 12 frames; a run holds one of 8 prototypes (16 features, fixed values), and every frame of it replaces
    4 of the 16 entries (25 %) by features drawn at random.  ``proto`` is the prototype of the frame (-1: padding)."""
    seed = PLANTED["seed"] if seed is None else seed
    rng = np.random.default_rng(2424 + seed)
    k, hidden, n_proto = PLANTED["k"], PLANTED["hidden"], PLANTED["prototypes"]
    proto_f = [rng.choice(hidden, k, replace=False) for _ in range(n_proto)]
    proto_v = [rng.uniform(0.5, 2.0, k).astype(np.float32) for _ in range(n_proto)]
    vals, idx, seg, proto = [], [], [], []
    for u in range(PLANTED["utterances"]):
        T, t, p = 96 + (1 if u < 5 else 0), 0, -1
        while t < T:
            d = min(int(rng.integers(3, 13)), T - t)
            p = int((p + 1 + rng.integers(0, n_proto - 1)) % n_proto)  # (never the same twice)
            for _ in range(d):
                f, v = proto_f[p].copy(), proto_v[p].copy()
                at = rng.choice(k, PLANTED["replace"], replace=False)
                free = np.setdiff1d(np.arange(hidden), f)
                f[at] = rng.choice(free, PLANTED["replace"], replace=False)
                v[at] = rng.uniform(0.5, 2.0, PLANTED["replace"]).astype(np.float32)
                idx.append(f), vals.append(v), seg.append(u), proto.append(p)
            t += d
        for _ in range(2):
            idx.append(rng.choice(hidden, k, replace=False)), vals.append(np.ones(k, np.float32)), seg.append(-1), proto.append(-1)
    vals, idx = np.asarray(vals, np.float32), np.asarray(idx, np.int32)
    seg, proto = np.asarray(seg, np.int32), np.asarray(proto, np.int32)
    assert seg.size == PLANTED["rows"]
    return {"code": (vals, idx), "hidden": hidden, "seg": seg, "proto": proto, "n_clusters": n_proto, "k": k}


@functools.lru_cache(maxsize=None)
def planted_fit(seed=None):
    """The oracle's own cosine fit of the planted case from the "sample" initialisation (seed 0 of the generator)."""
    c = planted_case(seed)
    return lloyd(c["code"], c["hidden"], c["n_clusters"], "cosine", c["seg"], seed=0, max_iter=20)
