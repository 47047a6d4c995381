"""Test-side oracle of the dictionary comparison, a numpy float64 restatement of the arithmetic
of ``wsae_match_rows``.  The reference has no code for it, and ``oracle/`` is frozen, so it lives here, next to
``attribution_oracle.py``.

    cosine:  a^ = a * (1 / max(sqrt(sum_d a_d^2), 1e-12)),  sim_ij = sum_d a^_id b^_jd   (a zero row: 0 to everything)
    dot:     sim_ij = sum_d a_id b_jd
    per row of A: the top_n largest sim_ij, value descending then index ascending (ties go to the lowest index);
    exclude_self skips column j == i; with fewer than top_n candidates the tail is idx = -1, val = -inf.

Bounds an implementation in fp32 (``u = 2^-24``) has to meet per similarity, ``bound()`` below.

``E_fp32 = (2 dim + 16) u`` for the cosine.  (1) The squared norm is a sum of ``dim`` non-negative terms: in any
summation order, with or without fused multiply-adds, its relative error is at most ``dim u`` to first order (every
term passes through at most ``dim - 1`` additions and one product rounding), and the square root halves a relative
error: ``dim u / 2`` per operand, ``dim u`` for the pair.  (2) The square root, the reciprocal, the ``max`` and the
scaling product are one rounding each (the device's sqrt and division may be off by an ulp more): at most ``8 u`` per
operand, ``16 u`` for the pair.  (3) A ``dim``-term fp32 accumulation in any order is within ``dim u sum_d |x_d y_d|``
of the exact sum, and ``sum_d |a^_d b^_d| <= |a^| |b^| <= 1`` (Cauchy-Schwarz).  (1) and (2) are relative to
``|sim| <= 1``, so the three add up to ``(2 dim + 16) u`` absolute.

``E_bf16 = 2^-8 + 2^-18 + E_fp32``: every normalised operand element is rounded once to bf16 (relative error at most
``2^-9``), so a product is off by at most ``(1 + 2^-9)^2 - 1 = 2^-8 + 2^-18`` of its magnitude, and the magnitudes sum
to at most 1 as above; products of bf16 values are exact in fp32 and the accumulation is covered by (3).

Dot metric: the same without the normalisation terms (1) and (2), ``dim u`` in fp32 and ``2^-8 + 2^-18 + dim u`` in
bf16, times ``sum_d |a_d| |b_d|`` of the pair (``abs_similarity``).

Order statistics: if every computed similarity of a row is within ``E`` of the exact one, the j-th largest computed
value is within ``E`` of the j-th largest exact value, whatever the indices are; so a test can check values against
the sorted exact row without assuming that near-ties resolve the same way.
"""

from __future__ import annotations

import numpy as np

F64 = np.float64
U = 2.0 ** -24


def normalise(m):
    m = np.asarray(m, dtype=F64)
    return m * (1.0 / np.maximum(np.sqrt((m * m).sum(axis=1, keepdims=True)), 1e-12))


def similarity(a, b, metric="cosine"):
    """``[rows_a, rows_b]`` float64."""
    a, b = np.asarray(a, dtype=F64), np.asarray(b, dtype=F64)
    if metric == "cosine":
        a, b = normalise(a), normalise(b)
    elif metric != "dot":
        raise ValueError(metric)
    return a @ b.T


def abs_similarity(a, b):
    """``sum_d |a_id| |b_jd|``: what the dot metric's bound is relative to."""
    return np.abs(np.asarray(a, dtype=F64)) @ np.abs(np.asarray(b, dtype=F64)).T


def top_n(sim, n, exclude_self=False):
    """``(values [rows_a, n] float64, indices [rows_a, n] int32)`` of a similarity matrix."""
    sim = np.array(sim, dtype=F64)
    ra, rb = sim.shape
    if exclude_self:
        d = np.arange(min(ra, rb))
        sim[d, d] = -np.inf
    order = np.argsort(-sim, axis=1, kind="stable")[:, :n]  # stable: equal values keep ascending index
    vals = np.take_along_axis(sim, order, axis=1)
    idx = order.astype(np.int32)
    idx[vals == -np.inf] = -1
    if n > rb:
        vals = np.concatenate([vals, np.full((ra, n - rb), -np.inf)], axis=1)
        idx = np.concatenate([idx, np.full((ra, n - rb), -1, dtype=np.int32)], axis=1)
    return vals, idx


def bound(dim, precision="fp32", metric="cosine"):
    """Per-similarity error bound (module docstring); for the dot metric a factor of ``abs_similarity``."""
    e = (2 * dim + 16) * U if metric == "cosine" else dim * U
    if precision == "bf16":
        e += 2.0 ** -8 + 2.0 ** -18
    elif precision != "fp32":
        raise ValueError(precision)
    return e
