"""Test-side oracle of the BatchTopK SAE, put together from ``oracle.sae_oracle`` pieces (the oracle itself has no
BatchTopK: the reference does not implement it).  Semantics:

* candidates = the per-row top-``k_max`` of ``pre`` (``O.topk_select``);
* training: ``t`` = the ``B k``-th largest positive candidate (the smallest positive one when there are fewer); a
  candidate is kept iff ``v > 0`` and ``v >= t``;
* eval with a trained threshold ``theta >= 0``: kept iff ``v > 0`` and ``v > theta``;
* dropped candidates become 0; ``hidden``, recon, loss, l0, the dead clock and the gradients follow from the masked code.
"""

from __future__ import annotations

import numpy as np

from oracle import sae_oracle as O

F32 = np.float32


def batch_select(vals: np.ndarray, k: int, hidden_dim: int, theta: float = -1.0, eval_mode: bool = False):
    """Selection over sorted candidates ``vals [B, k_max]``: (masked vals, t, saturated rows, kept entries)."""
    v = np.asarray(vals, dtype=F32)
    B, km = v.shape
    pos = v > 0
    if eval_mode and theta >= 0:
        keep = pos & (v > F32(theta))
        t = F32(theta)
    elif not pos.any():
        keep = np.zeros_like(pos)
        t = F32(-1.0)
    else:
        p = np.sort(v[pos])[::-1]
        t = p[min(B * k, p.size) - 1]
        keep = pos & (v >= t)
    sat = int(keep[:, km - 1].sum()) if km < hidden_dim else 0
    return np.where(keep, v, F32(0)).astype(F32), F32(t), sat, int(keep.sum())


def ema(theta: float, t: float, beta: float) -> np.float32:
    """theta <- t while theta < 0, else beta theta + (1 - beta) t, every operation rounded to fp32 once."""
    theta, t, beta = F32(theta), F32(t), F32(beta)
    if theta < 0:
        return t
    return F32(F32(beta * theta) + F32(F32(F32(1) - beta) * t))


def dense_selection(st: O.SAEState, x: np.ndarray, mode: str, k: int, k_max: int, idx_dev: np.ndarray,
                    keep_dev: np.ndarray | None = None, theta: float = -1.0, eval_mode: bool = False, band: float = 1e-5):
    """The oracle's kept set as a dense ``[B, H]`` bool matrix, plus (pre, t, n_disagree_clear).

    Candidate sets follow ``O.reconcile_selection`` (exact on clear-margin rows, the device's elsewhere).  When
    ``keep_dev`` (dense bool, the device's kept set) is given, entries within ``band`` (relative) of the cut take the
    device's decision and the count of disagreements OUTSIDE the band is returned (must be 0)."""
    pre = O.pre_activation(st, x, mode)
    sel, _ = O.reconcile_selection(st, x, idx_dev, k_max, mode)
    cand_vals = np.take_along_axis(pre, sel, axis=1).astype(F32)
    _, t, _, _ = batch_select(cand_vals, k, st.W_e.shape[0], theta, eval_mode)
    B, H = pre.shape
    cand = np.zeros((B, H), dtype=bool)
    np.put_along_axis(cand, sel, True, axis=1)
    thr_mode = eval_mode and theta >= 0
    keep = cand & (pre > 0) & ((pre > t) if thr_mode else (pre >= t))
    bad = 0
    if keep_dev is not None:
        near = cand & (np.abs(pre.astype(np.float64) - float(t)) <= band * max(abs(float(t)), 1e-30))
        bad = int((keep != keep_dev)[~near].sum())
        keep = np.where(near, keep_dev, keep)
    return keep, pre, t, bad


def forward_from_keep(st: O.SAEState, x: np.ndarray, keep: np.ndarray, pre: np.ndarray, mode: str) -> dict:
    """The ``fwd`` dict ``O.backward`` needs (hidden, reconstructed, loss, l0) for a given kept set."""
    hidden = np.where(keep, pre, 0).astype(F32)
    recon = O.decode(st, hidden, mode)
    r = recon.astype(np.float64) - np.asarray(x, np.float64)
    loss = F32(np.mean(r * r))
    l0 = F32((hidden > 0).sum(axis=1).astype(np.float64).mean())
    return {"hidden": hidden, "reconstructed": recon, "loss": loss, "reconstruction_loss": loss, "l0": l0}


def train_step(st: O.SAEState, x: np.ndarray, keep: np.ndarray, pre: np.ndarray, lr: float, mode: str,
               max_norm: float = 1.0) -> dict:
    """``O.train_step`` on a batch-selected code: forward -> backward -> clip -> AdamW -> decoder renorm."""
    fwd = forward_from_keep(st, x, keep, pre, mode)
    O.update_dead_features(st, fwd["hidden"])
    grads = O.backward(st, x, fwd, mode)
    total = O.grad_total_norm(grads)
    coef = O.clip_coef(total, max_norm)
    st.adam_t += 1
    for name in O.SAEState.PARAMS:
        p = getattr(st, name)
        gcl = (grads[name].astype(np.float64) * coef).astype(F32)
        m = st.adam_m.get(name, np.zeros_like(p))
        v = st.adam_v.get(name, np.zeros_like(p))
        p, m, v = O.adamw_update(p, gcl, m, v, st.adam_t, lr)
        setattr(st, name, p)
        st.adam_m[name], st.adam_v[name] = m, v
    st.W_d = O.normalize_decoder(st.W_d)
    return {"loss": float(fwd["loss"]), "l0": float(fwd["l0"]), "fwd": fwd, "grads": grads}


def resample_dead_features(st: O.SAEState, inputs: np.ndarray, keep: np.ndarray, pre: np.ndarray, mode: str,
                           num_resample: int | None = None) -> dict:
    """``O.resample_dead_features`` with the forward on the batch-selected code ``keep`` (train mode: the clock moves)."""
    inputs = np.asarray(inputs, dtype=F32)
    dead = np.nonzero(O.dead_mask(st))[0]
    if len(dead) == 0:
        return {"returned": 0, "rewritten": dead}
    if num_resample is not None:
        dead = dead[:num_resample]
    fwd = forward_from_keep(st, inputs, keep, pre, mode)
    O.update_dead_features(st, fwd["hidden"])
    resid = inputs.astype(np.float64) - fwd["reconstructed"].astype(np.float64)
    errors = (resid * resid).sum(axis=1).astype(F32)
    rows = np.argsort(-errors.astype(np.float64), kind="stable")[:min(len(dead), len(errors))]
    hi = inputs[rows].astype(np.float64)
    hi = (hi / np.maximum(np.sqrt((hi * hi).sum(axis=1, keepdims=True)), 1e-12)).astype(F32)
    for i in range(len(rows)):
        f = dead[i]
        st.W_e[f, :] = hi[i]
        st.b_e[f] = 0.0
        st.W_d[:, f] = hi[i]
        st.last_activated[f] = st.step_count
    return {"returned": len(dead), "rewritten": dead[:len(rows)].copy(), "rows": rows}
