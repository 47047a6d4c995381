"""numpy restatement of the activation profiles (include/wsae.h, ``wsae_profile_update`` / ``wsae_sample_update``;
DESIGN.md section 19): the value histogram and moments of every feature, the bottom-m sample of every (feature, stratum)
list written as a sort, the priority hash, and the float64 formulas of ``whisper_sae.analysis.profile`` (quantiles read off
the histogram, the summary).  Compared with the kernels bit for bit.  Also the inputs the CPU and the GPU tests share."""

from __future__ import annotations

import numpy as np

BINS = 192
MIN_INIT = 0x7F800000            # min_bits before anything fired: the bits of +inf
EMPTY = np.uint64(2 ** 64 - 1)   # an unused slot of a sample list
INT_FIELDS = ("fires", "hist", "max_bits", "min_bits", "over", "sum_q", "total_rows")
SAMPLE_FIELDS = ("keys", "svals", "seen")


def bin_of(v):
    """The bin of positive float32 values: ``clamp((bits >> 20) - 920, 0, 191)``."""
    b = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64).reshape(np.shape(v))
    return np.clip((b >> 20) - 920, 0, BINS - 1)


def bin_lower(j):
    """The lower edge of bin ``j`` as float64, ``2^(j // 8 - 12) (1 + (j % 8) / 8)``, read back from the bit pattern
    ``(j + 920) << 20``; ``j = 192`` gives 4096."""
    return ((np.asarray(j, np.int64) + 920) << 20).astype(np.int32).view(np.float32).astype(np.float64)


def first_active(code, seg, hidden, window=None):
    """``(row, feature, value)`` of the first active entry of every (row, feature) pair with the feature in the window,
    and the number of non-padding rows.  Active: ``v > 0`` (NaN is not), ``0 <= idx < hidden``, ``seg >= 0``."""
    vals, idx = np.asarray(code[0], np.float32), np.asarray(code[1]).astype(np.int64)
    n_rows = vals.shape[0]
    live = np.ones(n_rows, bool) if seg is None else np.asarray(seg).reshape(-1) >= 0
    f_lo, f_cols = (0, hidden) if window is None else window
    with np.errstate(invalid="ignore"):
        act = (vals > 0) & (idx >= 0) & (idx < hidden) & live[:, None]
    r, e = np.nonzero(act)  # ascending row, then ascending entry
    f = idx[r, e]
    _, keep = np.unique(r * hidden + f, return_index=True)
    r, f, v = r[keep], f[keep], vals[r[keep], e[keep]]
    inside = (f >= f_lo) & (f < f_lo + f_cols)
    return r[inside], f[inside], v[inside], int(live.sum())


def empty_profile(f_cols):
    return {"fires": np.zeros(f_cols, np.int32), "hist": np.zeros((f_cols, BINS), np.int32),
            "max_bits": np.zeros(f_cols, np.int32), "min_bits": np.full(f_cols, MIN_INIT, np.int32),
            "over": np.zeros(f_cols, np.int32), "sum_q": np.zeros(f_cols, np.int64), "total_rows": np.zeros(1, np.int64)}


def sum_q_terms(v):
    """``rint(min(v, 4096) * 2^20)`` in float32 (the product is exact), round to nearest even, as int64."""
    prod = np.minimum(np.asarray(v, np.float32), np.float32(4096)) * np.float32(2 ** 20)
    return np.rint(prod.astype(np.float64)).astype(np.int64)


def profile(code, seg, hidden, window=None, state=None):
    """One call of ``wsae_profile_update`` -> the state after it (``state``: the state before, not modified)."""
    f_lo, f_cols = (0, hidden) if window is None else window
    st = empty_profile(f_cols) if state is None else {k: v.copy() for k, v in state.items()}
    _, f, v, rows = first_active(code, seg, hidden, window)
    c = f - f_lo
    bits = v.view(np.int32)
    st["fires"] += np.bincount(c, minlength=f_cols).astype(np.int32)
    np.add.at(st["hist"], (c, bin_of(v)), 1)
    np.maximum.at(st["max_bits"], c, bits)
    np.minimum.at(st["min_bits"], c, bits)
    st["over"] += np.bincount(c[v >= 4096], minlength=f_cols).astype(np.int32)
    np.add.at(st["sum_q"], c, sum_q_terms(v))
    st["total_rows"] += rows
    return st


def merge_profiles(a, b):
    out = {k: a[k] + b[k] for k in ("fires", "hist", "over", "sum_q", "total_rows")}
    out["max_bits"], out["min_bits"] = np.maximum(a["max_bits"], b["max_bits"]), np.minimum(a["min_bits"], b["min_bits"])
    return out


# ---- readers ----------------------------------------------------------------------------------------------------------------
def bits_to_value(bits, fires):
    return np.where(fires > 0, np.asarray(bits, np.int32).view(np.float32).astype(np.float64), np.nan)


def quantile(st, q):
    """Per feature the ``q`` quantile (0 <= q <= 1) read off the histogram, float64.  With N = fires and t = q N: bin j is
    the first bin with hist[j] > 0 whose cumulative count reaches t; lo / hi are its edges (0 below bin 0, +inf above bin
    191) clipped to [min, max]; the result is lo + (t - cum[j - 1]) / hist[j] * (hi - lo), and lo where that fraction
    is 0.  NaN where the feature never fired."""
    hist = st["hist"].astype(np.int64)
    cum = np.cumsum(hist, axis=1)
    n = st["fires"].astype(np.float64)
    t = q * n
    reached = (cum.astype(np.float64) >= t[:, None]) & (hist > 0)
    j = np.argmax(reached, axis=1)
    rows = np.arange(hist.shape[0])
    lo = np.where(j == 0, 0.0, bin_lower(j))
    hi = np.where(j == BINS - 1, np.inf, bin_lower(j + 1))
    vmin, vmax = bits_to_value(st["min_bits"], st["fires"]), bits_to_value(st["max_bits"], st["fires"])
    with np.errstate(invalid="ignore", divide="ignore"):
        lo, hi = np.maximum(lo, vmin), np.minimum(hi, vmax)
        frac = (t - (cum[rows, j] - hist[rows, j]).astype(np.float64)) / hist[rows, j].astype(np.float64)
        out = np.where(frac == 0, lo, lo + frac * (hi - lo))
    return np.where(st["fires"] > 0, out, np.nan)


def summary(st):
    """The formulas of ``ActivationProfile.summary`` in float64."""
    fires = st["fires"].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = st["sum_q"].astype(np.float64) * 2.0 ** -20 / fires
        density = fires / float(st["total_rows"][0])
    return {"fires": st["fires"].astype(np.int64), "density": density, "mean": np.where(st["fires"] > 0, mean, np.nan),
            "max": bits_to_value(st["max_bits"], st["fires"]), "min": bits_to_value(st["min_bits"], st["fires"]),
            "median": quantile(st, 0.5), "q10": quantile(st, 0.1), "q90": quantile(st, 0.9), "q99": quantile(st, 0.99),
            "over": st["over"].astype(np.int64)}


def quantile_edges(st, n_strata):
    """``[f_cols, n_strata - 1]`` float32: the quantiles j / n_strata of every feature (NaN where it never fired)."""
    cols = [quantile(st, j / n_strata) for j in range(1, n_strata)]
    return np.stack(cols, axis=1).astype(np.float32) if cols else np.zeros((st["fires"].size, 0), np.float32)


# ---- the sampler ------------------------------------------------------------------------------------------------------------
def priority(ordinal, f, seed):
    """The uint32 priority of (ordinal, feature) under ``seed``."""
    m = np.uint64(0xFFFFFFFF)
    x = (np.asarray(ordinal, np.uint64) * np.uint64(0x9E3779B1) & m) ^ (np.asarray(f, np.uint64) * np.uint64(0x85EBCA77) & m)
    x = x ^ np.uint64(seed)
    x ^= x >> np.uint64(16)
    x = x * np.uint64(0x85EBCA6B) & m
    x ^= x >> np.uint64(13)
    x = x * np.uint64(0xC2B2AE35) & m
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


def key_of(ordinal, f, seed):
    return (priority(ordinal, f, seed).astype(np.uint64) << np.uint64(32)) | np.asarray(ordinal, np.uint64)


def stratum_of(edges_f, v):
    """The number of edges ``<= v`` per value (``edges_f [n, S - 1]``: the edges of each value's feature)."""
    with np.errstate(invalid="ignore"):
        return (edges_f <= np.asarray(v, np.float32)[:, None]).sum(1)


def empty_sample(f_cols, S, m):
    return {"keys": np.full((f_cols, S, m), EMPTY, np.uint64), "svals": np.zeros((f_cols, S, m), np.float32),
            "seen": np.zeros((f_cols, S), np.int32)}


def keep_smallest(lists, keys, vals, shape):
    """The ``m`` smallest keys of every list with their values, ``shape = (n_lists, m)``, unused slots (EMPTY, 0)."""
    n_lists, m = shape
    order = np.lexsort((keys, lists))
    lists, keys, vals = lists[order], keys[order], vals[order]
    start = np.searchsorted(lists, lists, side="left")
    rank = np.arange(lists.size) - start
    top = rank < m
    out_k, out_v = np.full(shape, EMPTY, np.uint64), np.zeros(shape, np.float32)
    out_k[lists[top], rank[top]] = keys[top]
    out_v[lists[top], rank[top]] = vals[top]
    return out_k, out_v


def sample(code, seg, ord_base, edges, keep, seed, hidden, window=None, state=None):
    """One call of ``wsae_sample_update`` as a sort -> the state after it.  ``edges [f_cols, S - 1]`` float32 (None: one
    stratum)."""
    f_lo, f_cols = (0, hidden) if window is None else window
    S = 1 if edges is None else edges.shape[1] + 1
    edges = np.zeros((f_cols, 0), np.float32) if edges is None else np.asarray(edges, np.float32)
    st = empty_sample(f_cols, S, keep) if state is None else {k: v.copy() for k, v in state.items()}
    r, f, v, _ = first_active(code, seg, hidden, window)
    c = f - f_lo
    lists = c * S + stratum_of(edges[c], v)
    st["seen"] += np.bincount(lists, minlength=f_cols * S).astype(np.int32).reshape(f_cols, S)
    held = st["keys"].reshape(-1) != EMPTY
    old_lists = np.repeat(np.arange(f_cols * S), keep)[held]
    all_l = np.concatenate([old_lists, lists])
    all_k = np.concatenate([st["keys"].reshape(-1)[held], key_of(ord_base + r, f, seed)])
    all_v = np.concatenate([st["svals"].reshape(-1)[held], v])
    k2, v2 = keep_smallest(all_l, all_k, all_v, (f_cols * S, keep))
    st["keys"], st["svals"] = k2.reshape(f_cols, S, keep), v2.reshape(f_cols, S, keep)
    return st


def merge_samples(a, b):
    f_cols, S, m = a["keys"].shape
    keys = np.concatenate([a["keys"], b["keys"]], axis=2).reshape(-1)
    vals = np.concatenate([a["svals"], b["svals"]], axis=2).reshape(-1)
    lists = np.repeat(np.arange(f_cols * S), 2 * m)
    held = keys != EMPTY
    k2, v2 = keep_smallest(lists[held], keys[held], vals[held], (f_cols * S, m))
    return {"keys": k2.reshape(f_cols, S, m), "svals": v2.reshape(f_cols, S, m), "seen": a["seen"] + b["seen"]}


# ---- the inputs the CPU and the GPU tests share -------------------------------------------------------------------------------
ROWS, K, HIDDEN = 700, 5, 96       # not a multiple of 64 or 256
WINDOW = (17, 50)
SILENT, RARE, TIED = 20, 30, 40    # in-window features: never fires / fires twice / gets equal edges in the sampler cases
SAMPLER_SHAPES = ((1, 1), (3, 4), (8, 16), (16, 64))


def general_case():
    """(code, seg) of the general shape: values 2^U(-14, 13) with every exact bin edge and the float just below it
    planted, zeros, negatives, NaN, +inf, denormals, values >= 4096, indices outside [0, hidden), repeated indices,
    padding rows, a feature that never fires and one that fires twice."""
    rng = np.random.default_rng(1900)
    vals = (2.0 ** rng.uniform(-14, 13, (ROWS, K))).astype(np.float32)
    idx = rng.integers(0, HIDDEN, (ROWS, K)).astype(np.int32)
    idx[(idx == SILENT) | (idx == RARE)] = SILENT + 1
    edges = bin_lower(np.arange(BINS + 1)).astype(np.float32)
    plant = np.concatenate([edges, np.nextafter(edges, np.float32(0))])
    where = rng.choice(ROWS * K, plant.size, replace=False)
    vals.reshape(-1)[where] = plant
    special = np.array([0.0, -1.5, np.nan, np.inf, 1e-40, 1.4e-45, 4096.0, 1e9, -np.inf, -0.0], np.float32)
    where = rng.choice(ROWS * K, 12 * special.size, replace=False)
    vals.reshape(-1)[where] = np.tile(special, 12)
    bad = rng.random((ROWS, K)) < 0.02
    idx[bad] = rng.choice(np.array([-1, HIDDEN, HIDDEN + 7, -2 ** 31, 2 ** 31 - 1], np.int64), int(bad.sum())).astype(np.int32)
    rep = rng.random((ROWS, K)) < 0.05  # an entry copies the index of an earlier entry of its row, with its own value
    rep[:, 0] = False
    rr, cc = np.nonzero(rep)
    idx[rr, cc] = idx[rr, (cc * rng.random(cc.size)).astype(np.int64)]
    idx[idx == RARE] = SILENT + 1
    idx[100, 0], vals[100, 0] = RARE, 0.75
    idx[400, 2], vals[400, 2] = RARE, 3.0
    seg = np.zeros(ROWS, np.int32)
    seg[rng.random(ROWS) < 0.1] = -1
    seg[[0, 255, 256, ROWS - 1]] = -1
    seg[[100, 400]] = 0
    seg[5] = 7  # (any id >= 0 is a live row)
    return (vals, idx), seg


def wide_case(k, rows=70, hidden=300):
    """k = 1 and k = 128: indices drawn with repeats within a row (hidden is small against k = 128)."""
    rng = np.random.default_rng(1901 + k)
    vals = (2.0 ** rng.uniform(-6, 6, (rows, k))).astype(np.float32)
    vals[rng.random((rows, k)) < 0.1] *= -1
    idx = rng.integers(-2, hidden + 2, (rows, k)).astype(np.int32)
    seg = np.where(rng.random(rows) < 0.1, -1, 0).astype(np.int32)
    return (vals, idx), seg


def sampler_edges(st, S):
    """The oracle's quantile edges for ``S`` strata with feature TIED's edges made equal (an empty stratum when S > 2;
    NaN rows of silent features stay)."""
    edges = quantile_edges(st, S)
    if S > 1:
        edges[TIED] = edges[TIED, 0]
    return edges
