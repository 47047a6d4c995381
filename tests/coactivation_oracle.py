"""numpy restatement of the co-activation statistics (include/wsae.h, ``wsae_coact_update`` / ``wsae_coact_top``) in
int64 / float64: the same activity rule, window and mask, the same formulas with the same operation order, the same
candidate and tie rules.  Everything here is exact integer arithmetic or correctly rounded IEEE double arithmetic, so
the kernels are compared with it bit for bit."""

from __future__ import annotations

import numpy as np

METRICS = ("count", "cond", "jaccard", "phi")


def active(vals, idx, hidden):
    """An entry fires iff its value is positive and its index names a feature."""
    vals, idx = np.asarray(vals), np.asarray(idx)
    return (vals > 0) & (idx >= 0) & (idx < hidden)


def accumulate(code_a, hidden_a, code_b, hidden_b, row_mask=None, a_lo=0, a_rows=None, chunk=256):
    """-> (counts int64 [a_rows, hidden_b], fire_a int64 [hidden_a], fire_b int64 [hidden_b], rows) of the rows of the
    two codes ``(vals [R, k], idx [R, k])``.  A repeated index counts once per occurrence."""
    va, ia = np.asarray(code_a[0]), np.asarray(code_a[1]).astype(np.int64)
    vb, ib = np.asarray(code_b[0]), np.asarray(code_b[1]).astype(np.int64)
    a_rows = hidden_a - a_lo if a_rows is None else a_rows
    keep = np.ones(va.shape[0], bool) if row_mask is None else np.asarray(row_mask).reshape(-1) != 0
    act_a = active(va, ia, hidden_a) & keep[:, None]
    act_b = active(vb, ib, hidden_b) & keep[:, None]
    fire_a = np.bincount(ia[act_a], minlength=hidden_a).astype(np.int64)
    fire_b = np.bincount(ib[act_b], minlength=hidden_b).astype(np.int64)
    win_a = act_a & (ia >= a_lo) & (ia < a_lo + a_rows)
    counts = np.zeros(a_rows * hidden_b, np.int64)
    for r0 in range(0, va.shape[0], chunk):
        s = slice(r0, r0 + chunk)
        pair = win_a[s, :, None] & act_b[s, None, :]
        flat = ((ia[s] - a_lo)[:, :, None] * hidden_b + ib[s][:, None, :])[pair]
        counts += np.bincount(flat, minlength=a_rows * hidden_b)
    return counts.reshape(a_rows, hidden_b), fire_a, fire_b, int(keep.sum())


def scores(counts, fire_a, fire_b, total, metric, a_lo=0):
    """float32 [a_rows, hidden_b]: the score of every cell, fp64 from the integers, rounded once to fp32."""
    c = np.asarray(counts).astype(np.int64)
    n = np.asarray(fire_a).astype(np.int64)[a_lo:a_lo + c.shape[0], None]
    m = np.asarray(fire_b).astype(np.int64)[None, :c.shape[1]]
    big = np.int64(total)
    cf = c.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        if metric == "count":
            s = cf
        elif metric == "cond":
            s = np.where(n != 0, cf / n.astype(np.float64), 0.0)
        elif metric == "jaccard":
            d = n + m - c
            s = np.where(d != 0, cf / d.astype(np.float64), 0.0)
        elif metric == "phi":
            pa, pb = n * (big - n), m * (big - m)
            num = (big * c - n * m).astype(np.float64)
            den = np.sqrt(pa.astype(np.float64)) * np.sqrt(pb.astype(np.float64))
            s = np.where((pa != 0) & (pb != 0), num / den, 0.0)
        else:
            raise ValueError(metric)
    return np.broadcast_to(s, c.shape).astype(np.float32)


def top(counts, fire_a, fire_b, total, metric, n, min_count=1, exclude_self=False, a_lo=0):
    """-> (values float32, indices int32, counts int32), each [a_rows, n].  Candidates: c >= min_count and, with
    exclude_self, j != a_lo + r.  Order: fp32 value descending, then index ascending; the tail is (-inf, -1, 0)."""
    c = np.asarray(counts).astype(np.int64)
    s = scores(c, fire_a, fire_b, total, metric, a_lo)
    rows, width = c.shape
    cand = c >= min_count
    if exclude_self:
        r = np.arange(rows)
        inside = r + a_lo < width
        cand[r[inside], r[inside] + a_lo] = False
    out_v = np.full((rows, n), -np.inf, np.float32)
    out_i = np.full((rows, n), -1, np.int32)
    out_c = np.zeros((rows, n), np.int32)
    for r in range(rows):
        js = np.nonzero(cand[r])[0]
        order = js[np.argsort(-s[r, js].astype(np.float64), kind="stable")][:n]  # stable: ties keep ascending index
        out_v[r, :len(order)] = s[r, order]
        out_i[r, :len(order)] = order
        out_c[r, :len(order)] = c[r, order]
    return out_v, out_i, out_c
