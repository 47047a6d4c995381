"""Test-side oracle of the gradient-based feature attribution, a numpy float64 restatement of the
arithmetic of ``wsae_attribute``.  The reference has no code for it, and ``oracle/`` is frozen, so it lives here, next to
``intervention_oracle.py`` whose setting it shares.

Per row, with ``sigma = sqrt(var + eps)`` (biased variance) of ``h`` frozen and ``G`` the metric's gradient with respect
to the tapped output:

    act_j   = max(v_j, 0)                              for the code (v, i) the caller hands in
    w_j     = (scale[i_j] - 1) * act_j                 (selected rows; scale None: w_j = -act_j; unselected rows: 0)
    s_j     = sum_d (G_d / gamma_d) * W_dT[i_j, d]     (no norm: G_d itself, sigma = 1)
    attr_j  = sigma * w_j * s_j

the exact first-order term of ``intervention_oracle.intervene(mode="keep_error")`` for a metric with gradient ``G``
(for a linear metric ``m = sum_d C_d h'_d`` it is the whole effect: ``sum_j attr_j == sum_d C_d (h'_d - h_d)``).  Per
feature ``f``: ``feat_sum[f]`` / ``feat_abs[f]`` = the sum of ``attr_j`` / ``|attr_j|`` over all entries with
``i_j == f``, ``feat_rows[f]`` = the number of those with ``w_j != 0``.  The selection is an *input*.

Bounds an fp32 implementation has to meet.  Per entry:

    (D + 8) * 2^-23 * sigma * |w_j| * sum_d |G_d / gamma_d| |W_dT[i_j, d]|

A D-term fp32 dot product, summed in any order with or without fused multiply-adds, is within
``D * 2^-24 * sum |x_d y_d|`` of the exact one to first order (every partial sum is rounded once, and a product enters at
most D - 1 sums and one product rounding); the factor above allows twice that, D * 2^-23, for the second-order terms and
for inputs that carry a rounding of their own: ``G_d / gamma_d`` (one division), ``w_j`` (a subtraction and a product),
``sigma`` (a mean, a sum of D non-negative squares whose relative error is at most its depth in roundings, halved by the
square root) and the two products of the result - the "+ 8" half-ulp-pairs, each relative to the entry's magnitude
``sigma |w_j| sum_d |u_d W_d|`` which is no smaller than ``|attr_j|``.

Per feature: the sum of its entries' bounds, plus ``n_f * q / 2`` for the fixed-point quantisation (``q = 2^(e - 36)``,
``A = max |attr| < 2^e``; n_f = entries with ``w_j != 0``), plus one fp32 rounding of the result (``2^-24 |x|``, and
``2^-149`` where the result is subnormal).  ``A`` is the maximum of the call's own fp32 ``attr``: tests hand in
``a_max`` of the output they check (the oracle's own maximum otherwise), since the two may sit on either side of a
power of two.
"""

from __future__ import annotations

import math

import numpy as np

F64 = np.float64
FRAC_BITS = 36
MAX_ENTRIES = 1 << 26


def entry_weights(vals, idx, hidden_dim, scale=None, row_mask=None):
    """``w [rows, k]`` in float64."""
    vals = np.asarray(vals, dtype=F64)
    idx = np.asarray(idx, dtype=np.int64)
    rows = vals.shape[0]
    sel = np.ones(rows, dtype=bool) if row_mask is None else np.asarray(row_mask).astype(bool)
    act = np.maximum(vals, 0.0)
    inside = (idx >= 0) & (idx < hidden_dim)
    safe = np.where(inside, idx, 0)
    factor = -np.ones_like(act) if scale is None else np.asarray(scale, F64)[safe] - 1.0
    return np.where(sel[:, None] & inside, factor * act, 0.0)


def quantum(a_max: float) -> float:
    """``q = 2^(e - 36)`` with ``a_max < 2^e`` (``a_max = f 2^e``, 0.5 <= f < 1); 0 for ``a_max == 0``."""
    if a_max == 0.0:
        return 0.0
    return math.ldexp(1.0, math.frexp(a_max)[1] - FRAC_BITS)


def fixed_point_sums(attr, idx, hidden_dim, active=None):
    """The fixed-point accumulation of ``wsae_attribute`` restated with Python integers: ``(feat_sum, feat_abs)`` as
    float32 arrays.  ``attr`` / ``idx``: flat or ``[rows, k]``; ``active``: entries that take part (default: all)."""
    if np.size(attr) > MAX_ENTRIES:
        raise ValueError(f"{np.size(attr)} entries: at most 2^26 per call (the 64-bit sums could overflow)")
    attr = np.asarray(attr, dtype=np.float32).ravel()
    idx = np.asarray(idx, dtype=np.int64).ravel()
    take = np.ones(attr.size, dtype=bool) if active is None else np.asarray(active, dtype=bool).ravel()
    feat_sum = np.zeros(hidden_dim, np.float32)
    feat_abs = np.zeros(hidden_dim, np.float32)
    a_max = float(np.abs(attr[take]).max()) if take.any() else 0.0
    if a_max == 0.0:
        return feat_sum, feat_abs
    e = math.frexp(a_max)[1]
    acc_sum = [0] * hidden_dim
    acc_abs = [0] * hidden_dim
    for a, f in zip(attr[take].tolist(), idx[take].tolist()):
        qv = int(np.rint(math.ldexp(a, FRAC_BITS - e)))  # exact scaling, one rounding to an integer (ties to even)
        acc_sum[f] += qv
        acc_abs[f] += abs(qv)
    for f in range(hidden_dim):
        # int -> fp32 in one rounding, then a power of two (exact above the subnormal range)
        feat_sum[f] = np.float32(math.ldexp(_int_to_f32(acc_sum[f]), e - FRAC_BITS))
        feat_abs[f] = np.float32(math.ldexp(_int_to_f32(acc_abs[f]), e - FRAC_BITS))
    return feat_sum, feat_abs


def _int_to_f32(n: int) -> float:
    """Nearest float32 of an integer of any size, rounded once (ties to even)."""
    sign, m = (-1.0, -n) if n < 0 else (1.0, n)
    bits = m.bit_length()
    if bits <= 24:
        return sign * float(m)
    shift = bits - 24
    top, rest = m >> shift, m & ((1 << shift) - 1)
    half = 1 << (shift - 1)
    if rest > half or (rest == half and (top & 1)):
        top += 1
    return sign * math.ldexp(float(top), shift)


def attribute(h, grad, vals, idx, w_dT, gamma=None, eps=0.0, scale=None, row_mask=None, a_max=None):
    """``dict`` of ``attr``, ``attr_bound`` ``[rows, k]``; ``feat_sum``, ``feat_abs``, ``feat_bound`` ``[H]`` (the bound
    of both sums) and ``feat_rows`` ``[H]`` (int64); ``w``, ``sigma`` and the quantum ``q``.  All from float64 arithmetic."""
    h = np.asarray(h, dtype=F64)
    grad = np.asarray(grad, dtype=F64)
    w_dT = np.asarray(w_dT, dtype=F64)
    idx = np.asarray(idx, dtype=np.int64)
    rows, dim = h.shape
    hidden_dim = w_dT.shape[0]
    if gamma is None:
        u, sigma = grad, np.ones((rows, 1), F64)
    else:
        mu = h.mean(axis=1, keepdims=True)
        sigma = np.sqrt(((h - mu) ** 2).mean(axis=1, keepdims=True) + eps)
        u = grad / np.asarray(gamma, F64)
    w = entry_weights(vals, idx, hidden_dim, scale, row_mask)
    inside = (idx >= 0) & (idx < hidden_dim)
    safe = np.where(inside, idx, 0)
    s = np.empty_like(w)
    mag = np.empty_like(w)
    for r in range(rows):  # (row by row: no [rows, k, D] array)
        rows_w = w_dT[safe[r]]
        s[r] = rows_w @ u[r]
        mag[r] = np.abs(rows_w) @ np.abs(u[r])
    attr = sigma * w * s
    attr_bound = (dim + 8) * 2.0 ** -23 * sigma * np.abs(w) * mag
    active = w != 0
    flat = safe[active]
    feat_sum = np.bincount(flat, weights=attr[active], minlength=hidden_dim)
    feat_abs = np.bincount(flat, weights=np.abs(attr[active]), minlength=hidden_dim)
    feat_rows = np.bincount(flat, minlength=hidden_dim).astype(np.int64)
    if a_max is None:
        a_max = float(np.abs(attr).max()) if attr.size else 0.0
    q = quantum(float(a_max))
    feat_bound = np.bincount(flat, weights=attr_bound[active], minlength=hidden_dim) + feat_rows * q / 2.0
    feat_bound = feat_bound + 2.0 ** -24 * (feat_abs + feat_bound) + 2.0 ** -149
    return {"attr": attr, "attr_bound": attr_bound, "feat_sum": feat_sum, "feat_abs": feat_abs, "feat_bound": feat_bound,
            "feat_rows": feat_rows, "w": w, "sigma": sigma, "q": q}
