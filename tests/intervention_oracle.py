"""Test-side oracle of the causal feature intervention, a numpy float64 restatement of the
arithmetic of ``wsae_intervene``.  The reference has no code for it, and ``oracle/`` is frozen, so it lives here.

Per row, with ``mu`` and ``sigma = sqrt(var + eps)`` (biased variance) of ``h`` frozen:

    a       = gamma * (h - mu) / sigma + beta          (a = h, sigma = 1, gamma = 1, beta = 0 without a norm)
    act_j   = max(v_j, 0)                              for the code (v, i) the caller hands in
    act'_j  = c_f if i_j is a forced feature f, else scale[i_j] * act_j     (selected rows; act'_j = act_j otherwise)
    keep_error:  delta = sum_j (act'_j - act_j) W_dT[i_j] + sum_{forced f not in the row's code} c_f W_dT[f]
                 h' = h + sigma * delta / gamma
    replace:     a' = b_d + b_pre + sum_j act'_j W_dT[i_j] + the same forced terms
                 h' = mu + sigma * (a' - beta) / gamma

The selection is an *input*: tests hand in the code the product selected, so nothing depends on near-tie ordering.

Next to the value the oracle returns the bound an fp32 implementation has to meet, element by element:

    (n_terms + 4) * 2^-23 * (|h_d| + sigma / |gamma_d| * (|a_d| + |beta_d| + sum_j |w_j| |W_dT[i_j, d]|))

with ``w_j`` the weights of the ``n_terms`` decoder rows that enter the row's sum (an fp32 fmaf chain of that many
products, then a handful of single operations: the statistics, one product, one division, one sum).
"""

from __future__ import annotations

import numpy as np

F64 = np.float64


def bf16_round(x: np.ndarray) -> np.ndarray:
    """fp32 -> bf16 (round to nearest even) -> fp32."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def bf16_ulp(y: np.ndarray) -> np.ndarray:
    """Spacing of bf16 numbers at |y| (8 significant bits)."""
    m = np.maximum(np.abs(np.asarray(y, dtype=F64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(m)) - 7)


def layernorm(h, gamma, beta, eps):
    """(a, mu, sigma) in float64."""
    h = np.asarray(h, dtype=F64)
    mu = h.mean(axis=1, keepdims=True)
    sigma = np.sqrt(((h - mu) ** 2).mean(axis=1, keepdims=True) + eps)
    return np.asarray(gamma, F64) * (h - mu) / sigma + np.asarray(beta, F64), mu, sigma


def weights(vals, idx, hidden_dim, scale=None, force_idx=(), force_val=(), row_mask=None, mode="keep_error"):
    """Dense weight matrix ``[rows, H]`` of the decoder rows in each row's sum, and the per-row term count."""
    vals = np.asarray(vals, dtype=F64)
    idx = np.asarray(idx, dtype=np.int64)
    rows, k = vals.shape
    sel = np.ones(rows, dtype=bool) if row_mask is None else np.asarray(row_mask).astype(bool)
    act = np.maximum(vals, 0.0)
    sc = np.ones(hidden_dim, F64) if scale is None else np.asarray(scale, F64)
    edited = np.where(sel[:, None], sc[idx] * act, act)
    r = np.arange(rows)[:, None]
    extra = np.zeros((rows, hidden_dim), F64)  # forced features outside the row's code
    for f, c in zip(force_idx, force_val):
        f, c = int(f), float(c)
        hit = (idx == f) & sel[:, None]
        edited = np.where(hit, c, edited)
        extra[sel & ~hit.any(axis=1), f] = c
    w = edited if mode == "replace" else edited - act
    dense = np.zeros((rows, hidden_dim), F64)
    dense[r, idx] = w  # (a code holds a feature at most once per row)
    dense += extra
    return dense, (dense != 0).sum(axis=1)


def intervene(h, vals, idx, w_dT, b_d, b_pre, gamma=None, beta=None, eps=0.0, scale=None, force_idx=(), force_val=(),
              row_mask=None, mode="keep_error"):
    """``(h' [rows, D], bound [rows, D], changed [rows] bool)``, all from float64 arithmetic."""
    assert mode in ("keep_error", "replace")
    h = np.asarray(h, dtype=F64)
    w_dT = np.asarray(w_dT, dtype=F64)
    rows, dim = h.shape
    if gamma is None:
        g, b = np.ones(dim, F64), np.zeros(dim, F64)
        a, mu, sigma = h, np.zeros((rows, 1), F64), np.ones((rows, 1), F64)
    else:
        g, b = np.asarray(gamma, F64), np.asarray(beta, F64)
        a, mu, sigma = layernorm(h, g, b, eps)
    dense, n_terms = weights(vals, idx, w_dT.shape[0], scale, force_idx, force_val, row_mask, mode)
    total = dense @ w_dT
    if mode == "replace":
        out = mu + sigma * (np.asarray(b_d, F64) + np.asarray(b_pre, F64) + total - b) / g
        changed = np.ones(rows, dtype=bool)
    else:
        out = h + sigma * total / g
        changed = n_terms > 0
    magnitude = np.abs(h) + sigma / np.abs(g) * (np.abs(a) + np.abs(b) + np.abs(dense) @ np.abs(w_dT))
    bound = (n_terms[:, None] + 4) * 2.0 ** -23 * magnitude
    return out, bound, changed
