"""numpy restatement of the feature-triggered sums (include/wsae.h, ``wsae_sta_update``), compared
with the kernels bit for bit: the triggers of a call by the rules of the header, then a literal sequential loop over them
in row order, vectorised over lag and channel only - every cell of ``acc`` and ``wsum`` is one chain of float64
additions in ascending trigger row.  ``update_loops`` is the same thing as a plain-Python triple loop and pins the
vectorised form on tiny inputs.  Also the input recipes the CPU and the GPU tests share (codes from the persistent
generator of tests/runs_oracle.py)."""

from __future__ import annotations

import numpy as np

import runs_oracle as RO

ALL, ONSET = 0, 1
VALUE, ONE = 0, 1
MODES = [(ALL, VALUE), (ALL, ONE), (ONSET, VALUE), (ONSET, ONE)]
FIELDS = ("acc", "wsum", "cnt")


def find_triggers(code, hidden, seg, f_lo=0, f_cols=None, trigger=ALL, weight=VALUE):
    """The triggers of a call in ascending (row, feature): ``(rows int64, features int64 (absolute), weights float32)``.
    ``seg`` None: one segment."""
    vals, idx = np.asarray(code[0], np.float32), np.asarray(code[1]).astype(np.int64)
    n_rows = vals.shape[0]
    seg = np.zeros(n_rows, np.int64) if seg is None else np.asarray(seg).astype(np.int64).reshape(-1)
    f_cols = hidden - f_lo if f_cols is None else f_cols
    act = (vals > 0) & (idx >= 0) & (idx < hidden) & (seg >= 0)[:, None]
    r, e = np.nonzero(act)  # ascending row, then ascending entry
    f = idx[r, e]
    key, keep = np.unique(r * hidden + f, return_index=True)  # the first active entry of a (row, feature) pair
    r, f, v = r[keep], f[keep], vals[r[keep], e[keep]]
    if trigger == ONSET:
        same = np.zeros(n_rows, bool)
        same[1:] = seg[1:] == seg[:-1]
        held = np.isin(key - hidden, key) & same[r]  # active on row r - 1, which has the segment of r
        r, f, v = r[~held], f[~held], v[~held]
    inside = (f >= f_lo) & (f < f_lo + f_cols)
    r, f, v = r[inside], f[inside], v[inside]
    return r, f, (np.ones(v.shape, np.float32) if weight == ONE else v.astype(np.float32))


def empty_state(f_cols, n_lags, channels):
    return {"acc": np.zeros((f_cols, n_lags, channels), np.float64), "wsum": np.zeros((f_cols, n_lags), np.float64),
            "cnt": np.zeros((f_cols, n_lags), np.int64)}


def update(code, hidden, seg, y, lags, f_lo=0, f_cols=None, trigger=ALL, weight=VALUE, state=None, channels=None):
    """One call of ``wsae_sta_update`` -> the state after it (``state``: the state before, not modified).  ``y``
    ``[n_rows, >= channels]`` float32 (a bf16 signal: float32 holding the same values); ``lags = (lo, hi)``."""
    y = np.asarray(y, np.float32)
    n_rows = y.shape[0]
    channels = y.shape[1] if channels is None else channels
    f_cols = hidden - f_lo if f_cols is None else f_cols
    lag = np.arange(lags[0], lags[1] + 1)
    st = empty_state(f_cols, lag.size, channels) if state is None else {k: v.copy() for k, v in state.items()}
    sg = np.zeros(n_rows, np.int64) if seg is None else np.asarray(seg).astype(np.int64).reshape(-1)
    r, f, w = find_triggers(code, hidden, seg, f_lo, f_cols, trigger, weight)
    y64 = y[:, :channels].astype(np.float64)
    acc, wsum, cnt = st["acc"], st["wsum"], st["cnt"]
    for n in range(r.size):  # the triggers in row order; per (feature, lag, channel) that is the order of the additions
        rows = r[n] + lag
        ok = (rows >= 0) & (rows < n_rows)
        ok[ok] = sg[rows[ok]] == sg[r[n]]
        j = np.nonzero(ok)[0]
        c, wd = f[n] - f_lo, np.float64(w[n])
        acc[c, j] += wd * y64[rows[j]]  # (float32 x float32 is exact in float64)
        wsum[c, j] += wd
        cnt[c, j] += 1
    return st


def update_loops(code, hidden, seg, y, lags, trigger=ALL, weight=VALUE):
    """The definition as plain loops over rows, entries, lags and channels (whole dictionary, zero state)."""
    vals, idx = code
    n_rows, k = len(vals), len(vals[0])
    C, L = len(y[0]), lags[1] - lags[0] + 1
    seg = [0] * n_rows if seg is None else list(seg)
    st = empty_state(hidden, L, C)

    def value(r, f):  # the value of the first active entry of f on row r, None if f is not active there
        if r < 0 or seg[r] < 0:
            return None
        for e in range(k):
            if int(idx[r][e]) == f and vals[r][e] > 0:
                return vals[r][e]
        return None

    for f in range(hidden):
        for r in range(n_rows):
            v = value(r, f)
            if v is None:
                continue
            if trigger == ONSET and r > 0 and seg[r - 1] == seg[r] and value(r - 1, f) is not None:
                continue
            w = np.float64(np.float32(1.0 if weight == ONE else v))
            for j in range(L):
                t = r + lags[0] + j
                if 0 <= t < n_rows and seg[t] == seg[r]:
                    for c in range(C):
                        st["acc"][f, j, c] = st["acc"][f, j, c] + w * np.float64(np.float32(y[t][c]))
                    st["wsum"][f, j] = st["wsum"][f, j] + w
                    st["cnt"][f, j] += 1
    return st


def same_bits(a, b):
    """Equal shapes, dtypes and bit patterns (NaN payloads and the sign of zero included)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int64), b.view(np.int64))


def to_bf16_values(y):
    """float32 values that bfloat16 holds exactly (the low 16 bits cut)."""
    y = np.ascontiguousarray(y, np.float32)
    return (y.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


# ---- the cases the CPU and the GPU tests share --------------------------------------------------------------------------
TILE = 4096                        # the feature tile of the transposition
WIDE = 6500
WINDOW = (1000, 4200)              # [1000, 5200): starts and ends inside tiles, and puts a boundary at feature 5096
TWINS = ((4095, 4096), (5095, 5096))  # either side of the tile boundary of the whole read and of the window's
# name -> (rows, k, hidden, channels, (lag_lo, lag_hi), segments)
CASES = {
    "one": (1, 1, 32, 1, (0, 0), 1),
    "small": (257, 5, 96, 7, (-3, 4), 9),
    "flagship": (1500, 32, 3072, 160, (-8, 8), 1),
    "wide": (4099, 32, WIDE, 5, (0, 2), 7),
    "two_pass": (600, 128, 256, 3, (-1, 1), 4),
    "tiny_segments": (6000, 3, 40, 4, (-2, 2), 5000),
    "lags64": (300, 4, 64, 2, (-32, 31), 3),
    "ahead": (257, 5, 96, 7, (3, 5), 9),
    "behind": (257, 5, 96, 7, (-5, -3), 9),
    "channels4096": (64, 4, 32, 4096, (-1, 1), 2),
    "order": (20000, 1, 8, 1, (0, 0), 1),
}
PLANTED = (5, 9)  # "flagship": on every row / on every other row


def case(name):
    """-> (code, seg, y): the persistent code, spoiled (repeated indices, values <= 0, indices out of range), ids with
    padding rows at the start, in the middle and at the end and not monotonic, a float32 signal."""
    rows, k, hidden, C, _, n_seg = CASES[name]
    rng = np.random.default_rng(7100 + list(CASES).index(name) if name not in ("ahead", "behind") else 7101)
    if name == "one":
        return (np.array([[1.5]], np.float32), np.array([[7]], np.int32)), np.zeros(1, np.int32), np.array([[-2.25]], np.float32)
    if name == "order":  # one feature on every row; |v y| spreads over 2^-40 .. 2^40, so the order of the adds shows
        vals = np.ldexp(1.0 + rng.random(rows), rng.integers(-20, 21, rows)).astype(np.float32).reshape(rows, 1)
        y = np.ldexp(rng.standard_normal(rows), rng.integers(-20, 21, rows)).astype(np.float32).reshape(rows, 1)
        return (vals, np.full((rows, 1), 3, np.int32)), np.zeros(rows, np.int32), y
    vals, idx = RO.spoil(rng, RO.persistent_code(rng, rows, k, hidden), hidden)
    seg = np.sort(rng.integers(0, n_seg, rows)).astype(np.int32) if n_seg > rows // 2 else RO.uneven_segments(rng, rows, n_seg)
    y = rng.standard_normal((rows, C), dtype=np.float32)
    if name == "flagship":
        idx[idx == PLANTED[0]] = PLANTED[0] + 1
        idx[idx == PLANTED[1]] = PLANTED[1] + 1
        idx[:, 0], vals[:, 0] = PLANTED[0], np.abs(vals[:, 0]) + np.float32(0.1)
        idx[::2, 1], vals[::2, 1] = PLANTED[1], np.abs(vals[::2, 1]) + np.float32(0.1)
        return (vals, idx), seg, y  # (one clean segment)
    if name == "wide":
        for p, (a, b) in enumerate(TWINS):  # b fires exactly where a does, with the same values, in the neighbouring tile
            idx[(idx == a) | (idx == b)] = b + 1
            on = np.cumsum(rng.random(rows) < 0.15) % 2 == 1
            idx[on, 2 * p], idx[on, 2 * p + 1] = a, b
            vals[on, 2 * p] = np.abs(vals[on, 2 * p]) + np.float32(0.1)
            vals[on, 2 * p + 1] = vals[on, 2 * p]
    seg[:2] = -1                      # padding at the start,
    mid = rows // 2
    seg[mid:mid + 2] = -1             # in the middle of a segment
    seg[-1] = -3                      # and at the end
    seg[rows // 3] = 2 ** 31 - 1      # a segment of one row with a large id
    if n_seg > 2:                     # not monotonic: a stretch of segment 0 inside the last segment, and [.., s, s - 1, s, ..]
        seg[-6:-4] = 0
        q = 2 * rows // 3
        seg[q] = seg[q] - 1 if seg[q] > 0 else 1
    return (vals, idx), seg, y


def whole_utterances(seg):
    """Ids made non-decreasing (padding stays padding, and joins the utterance in front of it): an input of whole
    utterances that can be cut between them."""
    seg = np.asarray(seg, np.int64)
    seg = np.where(seg == 2 ** 31 - 1, -1, seg)
    up = np.maximum.accumulate(seg)
    return np.where(seg >= 0, up, -1).astype(np.int32)
