"""Sequential numpy oracle of the token alignment (include/wsae.h): ``wsae_align_cost`` and
``wsae_align_dtw`` restated as plain loops, one IEEE operation per line, so that the kernels can be compared bit for bit.

``cost``: per (head, frame) the fp64 mean and population variance of the attention weights over the token rows (ONE chain
of additions each, product then add), the z-score rounded once to fp32 (+ 0.0f: never -0), the median over ``width``
frames with reflected borders, the negative head mean.  ``dtw``: the fp32 recurrence of Whisper with its tie rule, the
trace walked back from the last cell, and the per-frame / per-row tables read off the path.  ``dtw_wavefront`` computes
the same cells anti-diagonal by anti-diagonal with numpy vectors - the same single fp32 addition and the same comparisons
per cell, so the same bits - for the sizes at which the double loop is too slow for a test."""

from __future__ import annotations

import numpy as np

MAX_TOK, MAX_FRAMES, MAX_HEADS, MAX_WIDTH = 512, 2048, 32, 15  # WSAE_ALIGN_MAX_*
FILL = np.float32(np.inf)  # WSAE_ALIGN_FILL: cost outside the valid rows / frames and of invalid utterances


def reflect(q: int, n: int) -> int:
    """``F.pad(mode="reflect")``: -q below 0, 2 (n - 1) - q at and above n."""
    if q < 0:
        return -q
    if q >= n:
        return 2 * (n - 1) - q
    return q


def width_ok(width) -> bool:
    return 1 <= width <= MAX_WIDTH and width % 2 == 1


def cost_one(w: np.ndarray, n_tok: int, n_frames: int, width: int):
    """``w [n_heads, ld_t, ld_f]`` of one utterance (any float dtype; converted to float64 exactly).  Returns
    ``(cost float32 [ld_t, ld_f], n_bad)``: n_bad is 0 for a valid utterance, -1 where the sizes are invalid, else the
    number of non-finite values among ``w[:, :n_tok, :n_frames]``."""
    n_heads, ld_t, ld_f = w.shape
    cost = np.full((ld_t, ld_f), FILL, np.float32)
    p = width // 2
    if n_tok < 1 or n_tok > min(ld_t, MAX_TOK) or n_frames <= p or n_frames > min(ld_f, MAX_FRAMES):
        return cost, -1
    wd = w[:, :n_tok, :n_frames].astype(np.float64)
    bad = int((~np.isfinite(wd)).sum())
    if bad:
        return cost, bad
    z = np.zeros((n_heads, n_tok, n_frames), np.float32)
    for h in range(n_heads):
        for j in range(n_frames):
            s = np.float64(0.0)
            for i in range(n_tok):
                s = s + wd[h, i, j]
            mean = s / np.float64(n_tok)
            v = np.float64(0.0)
            for i in range(n_tok):
                d = wd[h, i, j] - mean
                v = v + d * d
            sd = np.sqrt(v / np.float64(n_tok))
            for i in range(n_tok):
                if sd == 0.0:
                    z[h, i, j] = np.float32(0.0)
                else:
                    z[h, i, j] = np.float32((wd[h, i, j] - mean) / sd) + np.float32(0.0)
    for i in range(n_tok):
        for j in range(n_frames):
            s = np.float64(0.0)
            for h in range(n_heads):
                win = sorted(z[h, i, reflect(q, n_frames)] for q in range(j - p, j + p + 1))
                s = s + np.float64(win[p])
            cost[i, j] = np.float32(np.float64(0.0) - s / np.float64(n_heads))
    return cost, 0


def cost(w: np.ndarray, n_tok, n_frames, width: int):
    """``w [n_utt, n_heads, ld_t, ld_f]`` -> ``(cost [n_utt, ld_t, ld_f], n_bad int32 [n_utt], status int64 [2])``."""
    n_utt = w.shape[0]
    out = np.empty((n_utt,) + w.shape[2:], np.float32)
    n_bad = np.zeros(n_utt, np.int32)
    status = np.zeros(2, np.int64)
    for u in range(n_utt):
        out[u], n_bad[u] = cost_one(w[u], int(n_tok[u]), int(n_frames[u]), width)
        status[0] += n_bad[u] != 0
        status[1] += max(int(n_bad[u]), 0)
    return out, n_bad, status


def _choose(c0, c1, c2):
    if c0 < c1 and c0 < c2:
        return c0, 0
    if c1 < c0 and c1 < c2:
        return c1, 1
    return c2, 2


def dtw_cells(m: np.ndarray):
    """The double loop: ``(D float32 [n + 1, k + 1], trace int8 [n, k])`` of the cost matrix ``m float32 [n, k]``."""
    n, k = m.shape
    inf = np.float32(np.inf)
    D = np.full((n + 1, k + 1), inf, np.float32)
    D[0, 0] = np.float32(0.0)
    trace = np.zeros((n, k), np.int8)
    for i in range(1, n + 1):
        for j in range(1, k + 1):
            c, t = _choose(D[i - 1, j - 1], D[i - 1, j], D[i, j - 1])
            D[i, j] = m[i - 1, j - 1] + c
            trace[i - 1, j - 1] = t
    return D, trace


def dtw_cells_wavefront(m: np.ndarray):
    """The same cells, one anti-diagonal at a time."""
    n, k = m.shape
    D = np.full((n + 1, k + 1), np.inf, np.float32)
    D[0, 0] = 0.0
    trace = np.zeros((n, k), np.int8)
    m = np.ascontiguousarray(m, np.float32)
    for d in range(2, n + k + 1):
        i = np.arange(max(1, d - k), min(n, d - 1) + 1)
        j = d - i
        c0, c1, c2 = D[i - 1, j - 1], D[i - 1, j], D[i, j - 1]
        diag = (c0 < c1) & (c0 < c2)
        up = ~diag & (c1 < c0) & (c1 < c2)
        c = np.where(diag, c0, np.where(up, c1, c2))
        D[i, j] = m[i - 1, j - 1] + c
        trace[i - 1, j - 1] = np.where(diag, 0, np.where(up, 1, 2))
    return D, trace


def walk(trace: np.ndarray):
    """The path from the last cell back to (0, 0) as ``(rows, frames)`` in forward order.  Row 0 goes left, column 0 up."""
    n, k = trace.shape
    i, j = n - 1, k - 1
    rows, frames = [], []
    while i >= 0 and j >= 0:
        rows.append(i)
        frames.append(j)
        t = trace[i, j]
        if i == 0 and j == 0:
            t = 0
        elif i == 0:
            t = 2
        elif j == 0:
            t = 1
        if t == 0:
            i, j = i - 1, j - 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    return np.array(rows[::-1], np.int64), np.array(frames[::-1], np.int64)


def tables(rows: np.ndarray, frames: np.ndarray, n: int, k: int):
    """``(frame_pos [k], tok_start [n], tok_end [n])`` read directly off a path over rows 0 .. n - 1."""
    frame_pos = np.full(k, -1, np.int32)
    tok_start = np.full(n, -1, np.int32)
    for r, f in zip(rows, frames):
        frame_pos[f] = max(frame_pos[f], r)
        if tok_start[r] < 0:
            tok_start[r] = f  # (the path is in forward order: the first cell of a row)
    tok_end = np.empty(n, np.int32)
    tok_end[:-1] = tok_start[1:]
    tok_end[-1] = k
    return frame_pos, tok_start, tok_end


def dtw(cost_m: np.ndarray, row_first, row_count, n_frames, n_bad=None, wavefront: bool = False) -> dict:
    """``cost_m float32 [n_utt, ld_t, ld_f]`` -> the outputs of ``wsae_align_dtw`` (rows are numbered as in ``cost_m``)."""
    n_utt, ld_t, ld_f = cost_m.shape
    out = {"frame_pos": np.full((n_utt, ld_f), -1, np.int32), "tok_start": np.full((n_utt, ld_t), -1, np.int32),
           "tok_end": np.full((n_utt, ld_t), -1, np.int32), "path_cost": np.full(n_utt, FILL, np.float32),
           "path_len": np.zeros(n_utt, np.int32), "status": np.zeros(2, np.int64)}
    for u in range(n_utt):
        first, n, k = int(row_first[u]), int(row_count[u]), int(n_frames[u])
        ok = (n_bad is None or n_bad[u] == 0) and first >= 0 and 1 <= n <= MAX_TOK and first + n <= ld_t \
            and 1 <= k <= min(ld_f, MAX_FRAMES)
        bad = 0
        if ok:
            m = cost_m[u, first:first + n, :k]
            bad = int((~np.isfinite(m)).sum())
        if not ok or bad:
            out["status"] += (1, bad)
            continue
        D, trace = (dtw_cells_wavefront if wavefront else dtw_cells)(m)
        rows, frames = walk(trace)
        fp, ts, te = tables(rows, frames, n, k)
        out["frame_pos"][u, :k] = fp + first
        out["tok_start"][u, first:first + n] = ts
        out["tok_end"][u, first:first + n] = te
        out["path_cost"][u] = D[n, k]
        out["path_len"][u] = len(rows)
    return out


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def attention(n_heads: int, n_tok: int, n_frames: int, seed: int, ridge: float = 4.0, dtype=np.float32) -> np.ndarray:
    """Softmaxed random logits with a diagonal ridge, ``[n_heads, n_tok, n_frames]``: rows sum to 1 like attention
    probabilities, and the ridge gives the alignment a path to find."""
    rng = np.random.default_rng(seed)
    logits = rng.standard_normal((n_heads, n_tok, n_frames))
    centre = (np.arange(n_tok)[:, None] + 0.5) * n_frames / n_tok
    logits += ridge * np.exp(-0.5 * ((np.arange(n_frames)[None, :] - centre) / max(n_frames / n_tok, 1.0)) ** 2)
    e = np.exp(logits - logits.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(dtype)


def quantised(n: int, k: int, seed: int) -> np.ndarray:
    """A cost matrix of multiples of 0.5 in -1 .. 1: sums are exact in fp32, and three-way ties are everywhere."""
    rng = np.random.default_rng(seed)
    return (rng.integers(-2, 3, size=(n, k)) * 0.5).astype(np.float32)


def tied_fraction(m: np.ndarray) -> float:
    """The fraction of interior cells whose three predecessors do not have one strict minimum."""
    D, _ = dtw_cells_wavefront(m)
    c0, c1, c2 = D[1:-1, 1:-1], D[1:-1, 2:], D[2:, 1:-1]
    strict = ((c0 < c1) & (c0 < c2)) | ((c1 < c0) & (c1 < c2)) | ((c2 < c0) & (c2 < c1))
    return float(1.0 - strict.mean())
