"""Sequential numpy / dict restatement of the token association (include/wsae.h, ``wsae_pair_update`` / ``wsae_pair_merge``
/ ``wsae_pair_top``): the pair rule, the integer state as a dict ``key -> [cnt, sum_q]`` with the
three marginals, the published hash and a sequential linear-probing table (to build colliding keys and to show what an
overfull table holds), the canonical export and the float64 scores and selections.  Compared with the kernels exactly:
integers, and float64 scores bit for bit.  Also the inputs the CPU and the GPU tests share."""

from __future__ import annotations

import numpy as np

import profile_oracle as PO
import runs_oracle as RO

M64 = (1 << 64) - 1
EMPTY = M64
SCORES = ("count", "precision", "recall", "f1", "jaccard", "lift", "mean")
BY_FEATURE, BY_TOKEN = 0, 1


# ---- the hash and the table ---------------------------------------------------------------------------------------------------
def splitmix64(x: int) -> int:
    x &= M64
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & M64
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & M64
    x ^= x >> 31
    return x


def key_of(f: int, t: int) -> int:
    return int(f) << 32 | int(t)


def home_slot(key: int, cap: int) -> int:
    return splitmix64(key) & (cap - 1)


def keys_with_home(cap, slot, count, hidden, n_tokens, avoid=()):
    """``count`` keys (f, t) in range whose first slot is ``slot``, found by search in a fixed order."""
    out, avoid = [], set(avoid)
    for f in range(hidden):
        for t in range(n_tokens):
            key = key_of(f, t)
            if key not in avoid and home_slot(key, cap) == slot:
                out.append(key)
                if len(out) == count:
                    return out
    raise ValueError("not enough keys")


def probe_table(keys, cap):
    """Insert ``keys`` one after the other (linear probing with wrap-around): ``(slots, placed)`` - the table as a list of
    keys (``EMPTY`` where unused) and per key the slot it ended in, or -1 where ``cap`` probes found none."""
    slots, placed = [EMPTY] * cap, []
    for key in keys:
        s, at = home_slot(key, cap), -1
        for _ in range(cap):
            if slots[s] in (EMPTY, key):
                slots[s], at = key, s
                break
            s = (s + 1) & (cap - 1)
        placed.append(at)
    return slots, placed


# ---- update, merge, export ----------------------------------------------------------------------------------------------------
def pair_tokens(seg, tokens, n_rows, n_tokens, lag):
    """int64 ``[n_rows]``: the token of the pair row r forms, -1 where it forms none."""
    tokens = np.asarray(tokens).astype(np.int64).reshape(-1)
    seg = np.zeros(n_rows, np.int64) if seg is None else np.asarray(seg).astype(np.int64).reshape(-1)
    out = np.full(n_rows, -1, np.int64)
    for r in range(n_rows):
        q = r + lag
        if seg[r] < 0 or q < 0 or q >= n_rows or seg[q] != seg[r]:
            continue
        if 0 <= tokens[q] < n_tokens:
            out[r] = tokens[q]
    return out


def empty_state(hidden, n_tokens):
    return {"table": {}, "feat_rows": np.zeros(hidden, np.int64), "tok_rows": np.zeros(n_tokens, np.int64),
            "pair_rows": np.zeros(1, np.int64)}


def copy_state(st):
    return {"table": {k: list(v) for k, v in st["table"].items()}, "feat_rows": st["feat_rows"].copy(),
            "tok_rows": st["tok_rows"].copy(), "pair_rows": st["pair_rows"].copy()}


def update(code, seg, tokens, hidden, n_tokens, lag=0, state=None):
    """One call of ``wsae_pair_update`` on an unbounded table -> the state after it (``state`` is not modified)."""
    st = empty_state(hidden, n_tokens) if state is None else copy_state(state)
    n_rows = np.asarray(code[0]).shape[0]
    tok = pair_tokens(seg, tokens, n_rows, n_tokens, lag)
    paired = tok >= 0
    st["pair_rows"] += int(paired.sum())
    np.add.at(st["tok_rows"], tok[paired], 1)
    r, f, v, _ = PO.first_active(code, seg, hidden)
    q = PO.sum_q_terms(v)
    table = st["table"]
    for ri, fi, qi in zip(r.tolist(), f.tolist(), q.tolist()):
        t = int(tok[ri])
        if t < 0:
            continue
        st["feat_rows"][fi] += 1
        cell = table.setdefault(key_of(fi, t), [0, 0])
        cell[0] += 1
        cell[1] += qi
    return st


def update_dense(code, seg, tokens, hidden, n_tokens, lag=0):
    """The same by brute force over a dense ``[hidden, n_tokens]`` table, entry by entry: ``(cnt, sum_q, feat_rows,
    tok_rows, pair_rows)``."""
    vals, idx = np.asarray(code[0], np.float32), np.asarray(code[1])
    n_rows, k = vals.shape
    cnt, sums = np.zeros((hidden, n_tokens), np.int64), np.zeros((hidden, n_tokens), np.int64)
    feat, tokr, pairs = np.zeros(hidden, np.int64), np.zeros(n_tokens, np.int64), 0
    for r in range(n_rows):
        if seg is not None and seg[r] < 0:
            continue
        q = r + lag
        if q < 0 or q >= n_rows or (seg is not None and seg[q] != seg[r]) or not 0 <= tokens[q] < n_tokens:
            continue
        t = int(tokens[q])
        pairs += 1
        tokr[t] += 1
        seen = set()
        for e in range(k):
            f, v = int(idx[r, e]), vals[r, e]
            if not v > 0 or not 0 <= f < hidden or f in seen:
                continue
            seen.add(f)
            feat[f] += 1
            cnt[f, t] += 1
            sums[f, t] += int(np.rint(np.float64(np.minimum(v, np.float32(4096)) * np.float32(2 ** 20))))
    return cnt, sums, feat, tokr, pairs


def merge(a, b):
    out = copy_state(a)
    for key, (c, q) in b["table"].items():
        cell = out["table"].setdefault(key, [0, 0])
        cell[0] += c
        cell[1] += q
    for name in ("feat_rows", "tok_rows", "pair_rows"):
        out[name] += b[name]
    return out


def export(st):
    """The canonical export: ``{"feature", "token", "count", "sum_q"}`` int64, keys ascending."""
    keys = sorted(st["table"])
    return {"feature": np.array([k >> 32 for k in keys], np.int64), "token": np.array([k & 0xFFFFFFFF for k in keys], np.int64),
            "count": np.array([st["table"][k][0] for k in keys], np.int64),
            "sum_q": np.array([st["table"][k][1] for k in keys], np.int64)}


def same_export(got, want):
    for name in ("feature", "token", "count", "sum_q"):
        g, w = np.asarray(got[name]), np.asarray(want[name])
        assert g.shape == w.shape, (name, g.shape, w.shape)
        assert np.array_equal(g, w), (name, int((g != w).sum()))


def same_marginals(got, want):
    for name in ("feat_rows", "tok_rows", "pair_rows"):
        assert np.array_equal(np.asarray(got[name]).reshape(-1), want[name].reshape(-1)), name


# ---- scores and selections ----------------------------------------------------------------------------------------------------
def score_of(score, c, q, a, b, n):
    """float64 from the integers, in the operation order of include/wsae.h (Python floats are IEEE doubles)."""
    c, a, b, n = float(c), float(a), float(b), float(n)
    if score == "count":
        return c
    if score == "precision":
        return c / a
    if score == "recall":
        return c / b
    if score == "f1":
        return (2.0 * c) / (a + b)
    if score == "jaccard":
        return c / ((a + b) - c)
    if score == "lift":
        return (c * n) / (a * b)
    if score == "mean":
        return (float(q) * 2.0 ** -20) / c
    raise ValueError(score)


def top(st, by, score, min_count, n):
    """``wsae_pair_top``: ``{"ids" int32, "scores" float64, "counts" int32, "sums" int64}``, each ``[n_groups, n]``."""
    groups = st["feat_rows"].size if by == BY_FEATURE else st["tok_rows"].size
    lists = {}
    total = int(st["pair_rows"][0])
    for key, (c, q) in st["table"].items():
        if c < min_count:
            continue
        f, t = key >> 32, key & 0xFFFFFFFF
        s = score_of(score, c, q, st["feat_rows"][f], st["tok_rows"][t], total)
        grp, ident = (f, t) if by == BY_FEATURE else (t, f)
        lists.setdefault(grp, []).append((-s, ident, c, q))
    out = {"ids": np.full((groups, n), -1, np.int32), "scores": np.full((groups, n), -np.inf, np.float64),
           "counts": np.zeros((groups, n), np.int32), "sums": np.zeros((groups, n), np.int64)}
    for grp, cells in lists.items():
        for j, (neg, ident, c, q) in enumerate(sorted(cells)[:n]):
            out["ids"][grp, j], out["scores"][grp, j], out["counts"][grp, j], out["sums"][grp, j] = ident, -neg, c, q
    return out


def same_top(got, want, what=""):
    for name in ("ids", "counts", "sums"):
        assert np.array_equal(got[name], want[name]), (what, name, int((got[name] != want[name]).sum()))
    g, w = np.ascontiguousarray(got["scores"], np.float64), np.ascontiguousarray(want["scores"], np.float64)
    assert np.array_equal(g.view(np.int64), w.view(np.int64)), (what, "scores", int((g.view(np.int64) != w.view(np.int64)).sum()))


# ---- the inputs the CPU and the GPU tests share ---------------------------------------------------------------------------------
HIDDEN, TOKENS, ROWS, K, UTTS = 300, 5000, 3011, 32, 12
LAGS = (-2, 0, 3)
SILENT, TWIN_A, TWIN_B = 297, 298, 299  # a feature that never fires; two that fire together, at one value, on few tokens
TWIN_VALUE = np.float32(50.0)


def zipf_tokens(rng, rows, n_tokens, lo=5, hi=25):
    """int32 ``[rows]``: runs of ``lo .. hi`` frames with one token each, drawn from a Zipf law (p ~ 1 / rank)."""
    n_runs = rows // lo + 1
    p = 1.0 / np.arange(1, n_tokens + 1)
    ids = rng.choice(n_tokens, n_runs, p=p / p.sum())
    return np.repeat(ids, rng.integers(lo, hi + 1, n_runs))[:rows].astype(np.int32)


def general_case():
    """``(code, seg, tokens)``: hidden 300, 5000 tokens, 3011 rows in a dozen utterances, k = 32.  A spoiled persistent
    code; padding rows, frames without a token and with a token outside the vocabulary; feature 297 never fires, features
    298 and 299 fire together at one value on three stretches, so that mean activations tie in both directions; the last
    token lies on three frames of a stretch with three active entries a row, so that a token has a short list."""
    rng = np.random.default_rng(2700)
    vals, idx = RO.spoil(rng, RO.persistent_code(rng, ROWS, K, HIDDEN), HIDDEN)
    rare = (idx >= SILENT) & (idx < HIDDEN)
    idx[rare] -= 64
    for lo in (200, 1210, 2405):
        idx[lo:lo + 40, 0], idx[lo:lo + 40, 1] = TWIN_A, TWIN_B
        vals[lo:lo + 40, :2] = TWIN_VALUE
    vals[5, 3], vals[6, 4] = np.nan, np.inf
    seg = np.sort(rng.integers(0, UTTS, ROWS)).astype(np.int32)
    seg[rng.random(ROWS) < 0.04] = -1
    tokens = zipf_tokens(rng, ROWS, TOKENS)
    tokens[rng.random(ROWS) < 0.03] = -1
    tokens[rng.random(ROWS) < 0.01] = TOKENS + 3
    # the last token occurs on three frames of a stretch with three active entries a row: a token with a short list
    tokens[tokens == TOKENS - 1] = TOKENS - 2
    vals[95:111, 3:], seg[95:111], tokens[100:103] = -1.0, 0, TOKENS - 1
    return (vals, idx), seg, tokens


def wide_case(k):
    """``(code, seg, tokens)`` with rows of ``k`` entries that straddle the 256-entry blocks: 300 features, 40 tokens,
    211 rows; row 7 repeats one index in every entry, row 8 holds NaN and non-positive values only."""
    rng = np.random.default_rng(2710 + k)
    rows, hidden = 211, 300
    vals, idx = RO.spoil(rng, RO.persistent_code(rng, rows, k, hidden), hidden)
    idx[7] = 11
    vals[7] = np.abs(vals[7]) + 1
    vals[7, 0] = -1.0  # (the first ACTIVE entry gives the value: entry 1 where k > 1)
    vals[8] = np.where(np.arange(k) % 2 == 0, np.nan, -np.abs(vals[8])).astype(np.float32)
    seg = (np.arange(rows) // 37).astype(np.int32)
    seg[rng.random(rows) < 0.05] = -1
    seg[7], seg[8] = seg[6] if seg[6] >= 0 else 0, seg[6] if seg[6] >= 0 else 0
    tokens = zipf_tokens(rng, rows, 40, 2, 6)
    tokens[rng.random(rows) < 0.05] = -1
    tokens[7] = tokens[8] = 3
    return (vals, idx), seg, tokens


def collision_case(cap=1024, per_slot=8, others=400, hidden=64, n_tokens=4096):
    """``(code, tokens, keys)``: one row per key (k = 1, value 1 + i / 8), every key a number of times of its own
    (1 + i % 5): ``per_slot`` keys whose first slot is ``cap - 1``, as many with ``cap - 2``, and ``others`` further ones."""
    keys = keys_with_home(cap, cap - 1, per_slot, hidden, n_tokens) + keys_with_home(cap, cap - 2, per_slot, hidden, n_tokens)
    rng = np.random.default_rng(2720)
    taken = set(keys)
    while len(keys) < 2 * per_slot + others:
        key = key_of(int(rng.integers(hidden)), int(rng.integers(n_tokens)))
        if key not in taken:
            taken.add(key)
            keys.append(key)
    rows = [(key, i) for i, key in enumerate(keys) for _ in range(1 + i % 5)]
    order = rng.permutation(len(rows))
    vals = np.array([[1 + rows[j][1] / 8] for j in order], np.float32)
    idx = np.array([[rows[j][0] >> 32] for j in order], np.int32)
    tokens = np.array([rows[j][0] & 0xFFFFFFFF for j in order], np.int32)
    return (vals, idx), tokens, keys
