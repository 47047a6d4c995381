"""numpy restatement of the temporal run statistics (include/wsae.h, ``wsae_runs_update``): the
runs of every feature in every segment of a call, their lengths, gaps, histograms and event records, compared with the
kernel bit for bit (the ``total`` of a run by sequential ``float32`` adds in row order), and the summary formulas of
``whisper_sae.analysis.temporal`` in float64.  Also the synthetic code with persistence that the tests and
``profiles/temporal_timing.py`` share, and the input recipes of the CPU and the GPU tests."""

from __future__ import annotations

import numpy as np

BINS = 48
INT_FIELDS = ("frames", "runs", "dur_max", "dur_sq", "dur_hist", "gap_hist", "total_rows")
EVENT_FIELDS = ("feature", "segment", "start", "length", "total", "peak")


def bin_of(x):
    """The histogram bin of a length or gap ``x >= 1``: exact up to 32, then bin 32 + j holds (2^(5+j), 2^(6+j)], the
    last bin everything above 2^20."""
    x = np.asarray(x, np.int64)
    big = np.maximum(x - 1, 1)
    log2 = np.zeros(x.shape, np.int64)
    for s in (32, 16, 8, 4, 2, 1):  # floor(log2(big)) in integers
        step = (big >> (log2 + s)) > 0
        log2 = log2 + np.where(step, s, 0)
    return np.where(x <= 32, x - 1, np.minimum(32 + log2 - 5, BINS - 1))


def bin_lower(b):
    """The smallest length of bin ``b``."""
    b = np.asarray(b, np.int64)
    return np.where(b < 32, b + 1, (1 << np.clip(b - 27, 0, 62)) + 1)


def find_runs(code, hidden, seg, n_seg, f_lo=0, f_cols=None):
    """Every run of the call and its gaps.  -> dict of arrays, one element per run, in canonical order (feature, segment,
    start): ``feature`` (absolute), ``segment`` (local id), ``start`` (frame offset in the segment), ``length``,
    ``total`` / ``peak`` float32, ``gap_before`` (0 for the first run of a feature in a segment); and ``rows``: the
    non-padding rows."""
    vals, idx = np.asarray(code[0], np.float32), np.asarray(code[1]).astype(np.int64)
    seg = np.asarray(seg).astype(np.int64).reshape(-1)
    n_rows = vals.shape[0]
    f_cols = hidden - f_lo if f_cols is None else f_cols
    ok_row = (seg >= 0) & (seg < n_seg)
    first_row = np.full(n_seg, n_rows, np.int64)
    np.minimum.at(first_row, seg[ok_row], np.nonzero(ok_row)[0])
    act = (vals > 0) & (idx >= 0) & (idx < hidden) & ok_row[:, None]
    r, e = np.nonzero(act)  # ascending row, then ascending entry
    f = idx[r, e]
    _, keep = np.unique(r * hidden + f, return_index=True)  # the first active entry of a (row, feature) pair
    r, f, v = r[keep], f[keep], vals[r[keep], e[keep]]
    inside = (f >= f_lo) & (f < f_lo + f_cols)
    r, f, v = r[inside], f[inside], v[inside]
    s = seg[r]
    order = np.lexsort((r, s, f))
    r, f, v, s = r[order], f[order], v[order], s[order]
    n = r.size
    head = np.ones(n, bool)
    head[1:] = (f[1:] != f[:-1]) | (s[1:] != s[:-1]) | (r[1:] != r[:-1] + 1)
    at = np.nonzero(head)[0]
    length = np.diff(np.append(at, n))
    a = r[at]
    b = a + length - 1
    gap = np.zeros(at.size, np.int64)
    if at.size > 1:
        same = (f[at][1:] == f[at][:-1]) & (s[at][1:] == s[at][:-1])
        gap[1:] = np.where(same, a[1:] - b[:-1] - 1, 0)
    # total: one float32 add per run and step, in row order
    total = v[at].copy() if n else np.zeros(0, np.float32)
    pos = np.arange(n) - np.repeat(at, length)
    by_pos = np.argsort(pos, kind="stable")
    counts = np.bincount(pos, minlength=1) if n else np.zeros(1, np.int64)
    run_of = np.repeat(np.arange(at.size), length)
    lo = counts[0]
    for t in range(1, counts.size):
        sel = by_pos[lo:lo + counts[t]]
        total[run_of[sel]] = total[run_of[sel]] + v[sel]
        lo += counts[t]
    peak = np.maximum.reduceat(v, at) if n else np.zeros(0, np.float32)
    return {"feature": f[at], "segment": s[at], "start": a - first_row[s[at]], "length": length,
            "total": total.astype(np.float32), "peak": peak.astype(np.float32), "gap_before": gap, "rows": int(ok_row.sum())}


def empty_state(f_cols):
    return {"frames": np.zeros(f_cols, np.int32), "runs": np.zeros(f_cols, np.int32), "dur_max": np.zeros(f_cols, np.int32),
            "dur_sq": np.zeros(f_cols, np.int64), "dur_hist": np.zeros((f_cols, BINS), np.int32),
            "gap_hist": np.zeros((f_cols, BINS), np.int32), "total_rows": np.zeros(1, np.int64),
            "events": {k: np.zeros(0, np.float32 if k in ("total", "peak") else np.int32) for k in EVENT_FIELDS}}


def update(code, hidden, seg, n_seg, seg_base=0, f_lo=0, f_cols=None, ev_min_len=1, state=None):
    """One call of ``wsae_runs_update`` -> the state after it (``state``: the state before, not modified).  ``events``
    holds every run with ``length >= ev_min_len`` of all calls so far in the canonical order (feature, segment, start),
    ``segment`` being ``seg_base`` + the local id."""
    f_cols = hidden - f_lo if f_cols is None else f_cols
    st = empty_state(f_cols) if state is None else {k: (dict(v) if k == "events" else v.copy()) for k, v in state.items()}
    rn = find_runs(code, hidden, seg, n_seg, f_lo, f_cols)
    c, d = rn["feature"] - f_lo, rn["length"]
    st["runs"] += np.bincount(c, minlength=f_cols).astype(np.int32)
    st["frames"] += np.bincount(c, weights=d, minlength=f_cols).astype(np.int32)
    st["dur_sq"] += np.bincount(c, weights=(d * d).astype(np.float64), minlength=f_cols).astype(np.int64)  # (exact below 2^53)
    np.maximum.at(st["dur_max"], c, d.astype(np.int32))
    np.add.at(st["dur_hist"], (c, bin_of(d)), 1)
    g = rn["gap_before"] > 0
    np.add.at(st["gap_hist"], (c[g], bin_of(rn["gap_before"][g])), 1)
    st["total_rows"] += rn["rows"]
    ev = d >= ev_min_len
    new = {"feature": rn["feature"][ev].astype(np.int32), "segment": (rn["segment"][ev] + seg_base).astype(np.int32),
           "start": rn["start"][ev].astype(np.int32), "length": d[ev].astype(np.int32), "total": rn["total"][ev],
           "peak": rn["peak"][ev]}
    both = {k: np.concatenate([st["events"][k], new[k]]) for k in EVENT_FIELDS}
    order = np.lexsort((both["start"], both["segment"], both["feature"]))
    st["events"] = {k: both[k][order] for k in EVENT_FIELDS}
    return st


def hist_quantile(hist, q):
    """Per row of ``hist [F, 48]``: the lower length of the smallest bin whose cumulative count reaches ``q`` times the
    row's total (NaN for an empty row)."""
    hist = np.asarray(hist, np.int64)
    cum = np.cumsum(hist, axis=1)
    total = cum[:, -1]
    b = np.argmax(cum.astype(np.float64) >= q * total[:, None].astype(np.float64), axis=1)
    return np.where(total > 0, bin_lower(b).astype(np.float64), np.nan)


def summary(st, frame_ms=None):
    """The formulas of ``RunTracker.summary`` in float64."""
    runs, frames = st["runs"].astype(np.float64), st["frames"].astype(np.float64)
    rows = float(st["total_rows"][0])
    unit = 1.0 if frame_ms is None else float(frame_ms)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = frames / runs
        std = np.sqrt(np.maximum(st["dur_sq"].astype(np.float64) / runs - mean * mean, 0.0))
        out = {"runs": st["runs"].astype(np.int64), "frames": st["frames"].astype(np.int64),
               "max_duration": st["dur_max"].astype(np.float64) * unit,
               "mean_duration": mean * unit, "std_duration": std * unit,
               "median_duration": hist_quantile(st["dur_hist"], 0.5) * unit,
               "persistence": 1.0 - runs / frames, "duty": np.where(runs > 0, frames / rows, np.nan),
               "event_rate": np.where(runs > 0, runs / rows, np.nan),
               "median_gap": hist_quantile(st["gap_hist"], 0.5) * unit}
    return out


# ---- the synthetic code with persistence ---------------------------------------------------------------------------------
def holding_times(k):
    """Mean holding time of each of the k columns of the code, in rows: a geometric spread from 1 to 256."""
    return np.array([3.0]) if k == 1 else 2.0 ** (8.0 * np.arange(k) / (k - 1))


def persistent_code(rng, rows, k, hidden):
    """A compact code ``(vals float32, idx int32) [rows, k]`` whose features persist.  Column j of the code is an on/off
    Markov chain over the features ``f = j (mod k)``: it holds its feature for a geometric time of mean
    ``holding_times(k)[j]`` rows, then jumps to another feature of its class, so a feature of class j is switched on and
    off with that holding time and indices never repeat within a row.  The chains run on across segment boundaries.  All
    values are positive."""
    per_class = (hidden - np.arange(k) + k - 1) // k  # features of class j below hidden
    if np.any(per_class < 1):
        raise ValueError(f"hidden = {hidden} has no feature for every one of the {k} columns")
    jump = rng.random((rows, k), dtype=np.float32) < (1.0 / holding_times(k)).astype(np.float32)[None, :]
    jump[0] = True
    visit = np.cumsum(jump, axis=0, dtype=np.int32) - 1  # the number of the column's current visit
    idx = np.empty((rows, k), np.int32)
    for j in range(k):
        draws = rng.integers(0, per_class[j], int(visit[-1, j]) + 1, dtype=np.int32)
        idx[:, j] = draws[visit[:, j]] * k + j
    vals = np.abs(rng.standard_normal((rows, k), dtype=np.float32)) + np.float32(0.05)
    return vals, idx


def spoil(rng, code, hidden):
    """Mix into a code what a TopK code never has: values <= 0 (about 4 %, some exactly 0), indices outside
    ``[0, hidden)`` (1 %) and indices repeated within a row (2 % of the entries copy their left neighbour's index, with a
    value of their own, positive or not)."""
    vals, idx = code[0].copy(), code[1].copy()
    shape = vals.shape
    neg = rng.random(shape) < 0.03
    vals[neg] = -vals[neg]
    vals[rng.random(shape) < 0.01] = 0.0
    bad = rng.random(shape) < 0.01
    idx[bad] = rng.choice(np.array([-1, hidden, hidden + 9, -5], np.int32), int(bad.sum()))
    if shape[1] > 1:
        rep = rng.random(shape) < 0.02
        rep[:, 0] = False
        rr, cc = np.nonzero(rep)
        idx[rr, cc] = idx[rr, cc - 1]
    return vals, idx


def uneven_segments(rng, rows, n_seg):
    """Non-decreasing ids over ``rows`` rows, every segment present, the first three of length 1 where there is room."""
    if n_seg == 1:
        return np.zeros(rows, np.int32)
    cuts = np.sort(rng.choice(np.arange(4, rows), n_seg - 4, replace=False)) if n_seg > 4 else np.array([], np.int64)
    starts = np.concatenate([[0, 1, 2, 3][:min(4, n_seg)], cuts]).astype(np.int64)
    seg = np.zeros(rows, np.int32)
    seg[starts[1:]] = 1
    return np.cumsum(seg).astype(np.int32)


# ---- the cases the CPU and the GPU tests share --------------------------------------------------------------------------
TILE, TILE_EV = 3072, 1536          # the kernel's feature tiles without and with events
WIDE = 6500                         # more than twice the wider tile
TWINS = ((3071, 3072), (1535, 1536), (6143, 6144))  # either side of a tile boundary (both widths)
WINDOW = (1000, 4200)               # starts and ends inside tiles of both widths
# (rows, k, hidden, n_seg)
SHAPES = [(1, 1, 32, 1), (257, 5, 96, 9), (3000, 32, 3072, 1), (4099, 32, WIDE, 7), (600, 128, 256, 4), (6000, 3, 40, 5000)]
LARGE = SHAPES[2:4]


def case(shape):
    """(code, seg) of one shape: the persistent code, spoiled, with padding rows at the start, in the middle and at the
    end, ids >= n_seg and non-monotonic ids, plus the shape's planted features."""
    rows, k, hidden, n_seg = shape
    rng = np.random.default_rng(4000 + SHAPES.index(shape))
    code = spoil(rng, persistent_code(rng, rows, k, hidden), hidden)
    if rows == 1:
        return (np.array([[1.5]], np.float32), np.array([[7]], np.int32)), np.zeros(1, np.int32)
    vals, idx = code
    seg = np.sort(rng.integers(0, n_seg, rows)).astype(np.int32) if n_seg > rows // 2 else uneven_segments(rng, rows, n_seg)
    if shape == (3000, 32, 3072, 1):
        idx[idx == 5] = 6
        idx[idx == 9] = 10
        idx[:, 0], vals[:, 0] = 5, np.abs(vals[:, 0]) + np.float32(0.1)          # on every row: one run of 3000
        idx[::2, 1], vals[::2, 1] = 9, np.abs(vals[::2, 1]) + np.float32(0.1)    # on every other row: 1500 runs, gaps of 1
        return (vals, idx), seg                                                     # (one clean segment)
    if hidden == WIDE:
        for p, (a, b) in enumerate(TWINS):  # b fires exactly where a does, with the same values, in the neighbouring tile
            idx[(idx == a) | (idx == b)] = b + 1
            on = np.cumsum(rng.random(rows) < 0.15) % 2 == 1  # an on/off chain of their own, in columns 2p and 2p + 1
            idx[on, 2 * p], idx[on, 2 * p + 1] = a, b
            vals[on, 2 * p] = np.abs(vals[on, 2 * p]) + np.float32(0.1)
            vals[on, 2 * p + 1] = vals[on, 2 * p]
    seg[:2] = -1                      # padding at the start,
    mid = rows // 2
    seg[mid:mid + 2] = -1             # in the middle of a segment
    seg[-1] = -3                      # and at the end
    seg[rows // 3] = n_seg            # ids >= n_seg
    seg[rows // 3 + 1] = 2 ** 31 - 1
    if n_seg > 2:                     # non-monotonic: a stretch of segment 0 inside the last segment, and [.., s, s - 1, s, ..]
        seg[-6:-4] = 0
        q = 2 * rows // 3
        seg[q] = seg[q] - 1 if seg[q] > 0 else 1
    return (vals, idx), seg
