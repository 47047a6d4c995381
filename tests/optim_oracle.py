"""float64 reference of the optimizer tail and the weight-maintenance kernels (``wsae_optim.hip``), plain numpy.

TEST INFRASTRUCTURE, in the style of the other ``tests/*_oracle.py`` helpers.  Everything is float64 arithmetic on the
float32 inputs, with no intermediate rounding: what a kernel may differ by is its own fp32 rounding, which the GPU tests
bound by counting operations (tests/test_gpu_optimizer_tail.py).  The flat pack is ``[W_e | W_dT | b_e | b_d | b_pre]``
(include/wsae.h); the same layout holds the gradients and both Adam moments.

``tail``     clip_grad_norm_ -> AdamW -> per-row decoder renorm -> dead count and clock merge (training.py:186-198, :212)
``resample`` the resample chain of model.py:197-257 from fabricated row errors (``dec_src``: transcoder.py:247-249)
``row_errors`` / ``dead_scan`` / ``shadow_pre``  the small kernels around them.
"""

from __future__ import annotations

import math

import numpy as np

from oracle import sae_oracle as O
from oracle.synth import bf16_round

F32 = np.float32
F64 = np.float64

SEGMENTS = ("W_e", "W_dT", "b_e", "b_d", "b_pre")


def layout(D: int, H: int):
    """(total, offsets[5]) of the flat pack; the same numbers as ``whisper_sae._native.pack_layout``."""
    return 2 * D * H + H + 2 * D, [0, D * H, 2 * D * H, 2 * D * H + H, 2 * D * H + H + D]


def segment(buf: np.ndarray, lay, name: str, D: int, H: int) -> np.ndarray:
    """View of one segment of a pack-shaped array (matrices as [H, D])."""
    total, off = lay
    i = SEGMENTS.index(name)
    end = off[i + 1] if i < 4 else total
    v = buf[off[i]:end]
    return v.reshape(H, D) if i < 2 else v


def bf16(a: np.ndarray) -> np.ndarray:
    """float32 -> nearest bfloat16, ties to even, returned as float32 (the hardware conversion of the shadows)."""
    return bf16_round(np.asarray(a, dtype=F32))


def adam_constants(hyper: dict, step: int) -> dict:
    """The constants of one AdamW step as float64 numbers.

    ``hyper``: lr, beta1, beta2, eps, weight_decay (Python doubles) and ``mode``:

    * ``"as_passed"``: the hyper-parameters exactly as the C ABI receives them (doubles), every derived constant exact
      in double; the kernel's single fp32 rounding of each constant is part of its error budget.
    * ``"torch"``: what ``torch.optim.AdamW`` multiplies a tensor of ``hyper["dtype"]`` (default float32) by: ``1 - beta``
      and ``1 - lr * wd`` are formed in double and rounded ONCE to the tensor's dtype (``lerp_(g, 1 - beta1)``,
      ``addcmul_(g, g, value=1 - beta2)``, ``mul_(beta2)``, ``mul_(1 - lr * wd)``); the bias corrections stay double.
    """
    lr, b1, b2 = float(hyper["lr"]), float(hyper["beta1"]), float(hyper["beta2"])
    eps, wd = float(hyper["eps"]), float(hyper["weight_decay"])
    mode = hyper.get("mode", "as_passed")
    c = {"beta2": b2, "omb1": 1.0 - b1, "omb2": 1.0 - b2, "decay": 1.0 - lr * wd, "eps": eps,
         "step_size": lr / (1.0 - b1 ** step), "bc2_sqrt": math.sqrt(1.0 - b2 ** step)}
    if mode == "torch":
        dt = np.dtype(hyper.get("dtype", F32)).type
        for key in ("beta2", "omb1", "omb2", "decay"):
            c[key] = float(dt(c[key]))
    elif mode != "as_passed":
        raise ValueError(mode)
    return c


def tail(pack, grads, m, v, lay, hyper, step, max_norm, grad_scale, normalize, last=None, step_count=None, thr=0,
         fired=None) -> dict:
    """One optimizer tail.  ``pack, grads, m, v``: float32 (or float64) arrays of the pack's length; ``lay`` from
    ``layout``.  The norm is that of ``grad_scale * g`` over the gradient pack; clip = min(1, max_norm / (norm + 1e-6)),
    1 when ``max_norm <= 0``; gc = g * grad_scale * clip; AdamW as ``oracle.sae_oracle.adamw_update`` states it, without
    its float32 stores; renorm (``normalize``): every W_dT row / max(||row||, 1e-12).  Dead features: ``last`` merged with
    ``fired`` (last = step_count where fired > 0), dead iff step_count - last > thr (strict)."""
    total, off = lay
    H = off[3] - off[2]
    D = off[4] - off[3]
    p64, g64 = np.asarray(pack, F64), np.asarray(grads, F64)[:total]
    m64, v64 = np.asarray(m, F64), np.asarray(v, F64)
    norm = math.sqrt(float(((g64 * float(grad_scale)) ** 2).sum()))
    coef = O.clip_coef(norm, float(max_norm)) if max_norm > 0 else 1.0
    gs = coef * float(grad_scale)
    c = adam_constants(hyper, step)
    gc = g64 * gs
    m_new = m64 + (gc - m64) * c["omb1"]
    v_new = c["beta2"] * v64 + c["omb2"] * gc * gc
    denom = np.sqrt(v_new) / c["bc2_sqrt"] + c["eps"]
    update = c["step_size"] * (m_new / denom)
    p_new = p64 * c["decay"] - update
    pre_norm = p_new.copy()
    row_norm = None
    if normalize:
        wd = p_new[off[1]:off[2]].reshape(H, D)
        row_norm = np.sqrt((wd * wd).sum(axis=1))
        p_new = p_new.copy()
        p_new[off[1]:off[2]] = (wd / np.maximum(row_norm, 1e-12)[:, None]).reshape(-1)
    out = {"pack": p_new, "pre_norm": pre_norm, "row_norm": row_norm, "m": m_new, "v": v_new, "gc": gc, "denom": denom,
           "update": update, "grad_norm": norm, "clip_coef": coef, "gs": gs, "constants": c, "dead_count": None,
           "last": None}
    if last is not None:
        merged = np.asarray(last, np.int64).copy()
        if fired is not None:
            merged[np.asarray(fired) > 0] = int(step_count)
        out["last"] = merged
        out["dead_count"] = int(((int(step_count) - merged) > int(thr)).sum())
    return out


def dead_scan(last, step_count: int, thr: int):
    """(mask uint8 [H], count): step_count - last > thr, strict (model.py:183-190)."""
    mask = (int(step_count) - np.asarray(last, np.int64)) > int(thr)
    return mask.astype(np.uint8), int(mask.sum())


def row_errors(x, recon, rows=None):
    """(row_err [B], resid [B, D]) = (sum_d (x - recon)^2, x - recon) in float64; ``rows`` gathers x (model.py:230-231)."""
    x64 = np.asarray(x, F64)
    if rows is not None:
        x64 = x64[np.asarray(rows, np.int64)]
    resid = x64 - np.asarray(recon, F64)
    return (resid * resid).sum(axis=1), resid


def resample(pack, lay, inputs, row_err, dead_mask, last, step_count: int, num_cap: int, rows=None, dec_src=None) -> dict:
    """model.py:197-257 from given row errors.  Dead features ascending, capped (``num_cap < 0``: all); rows by
    ``np.argsort(-err, kind="stable")`` (ties: the lower row first); feature i of the list takes the i-th row:
    W_e[f] = x / max(||x||, 1e-12), W_dT[f] the same or the normalised row of ``dec_src``, b_e[f] = 0,
    last[f] = step_count.  ``rows`` gathers the inputs (``dec_src`` is indexed by the batch row, not the gathered one).
    Returns the float64 pack, the new ``last``, ``n_dead_out`` (the capped dead count, even with fewer rows),
    ``features`` rewritten in order and the batch ``order`` rows they took."""
    total, off = lay
    H = off[3] - off[2]
    D = off[4] - off[3]
    p = np.asarray(pack, F64).copy()
    new_last = np.asarray(last, np.int64).copy()
    dead = np.nonzero(np.asarray(dead_mask) != 0)[0]
    cap = H if num_cap < 0 else min(int(num_cap), H)
    dead = dead[:cap]
    err = np.asarray(row_err, F32)
    order = np.argsort(-err.astype(F64), kind="stable")
    n = min(len(dead), len(err))
    x64 = np.asarray(inputs, F64)
    We, WdT, be = p[off[0]:off[1]].reshape(H, D), p[off[1]:off[2]].reshape(H, D), p[off[2]:off[3]]
    for i in range(n):
        f, r = int(dead[i]), int(order[i])
        src = int(rows[r]) if rows is not None else r
        xr = x64[src]
        direction = xr / max(math.sqrt(float((xr * xr).sum())), 1e-12)
        We[f] = direction
        if dec_src is not None:
            dr = np.asarray(dec_src, F64)[r]
            WdT[f] = dr / max(math.sqrt(float((dr * dr).sum())), 1e-12)
        else:
            WdT[f] = direction
        be[f] = 0.0
        new_last[f] = int(step_count)
    return {"pack": p, "last": new_last, "n_dead_out": int(len(dead)), "features": dead[:n].copy(), "order": order[:n].copy()}


def shadow_pre(pack, lay, x) -> np.ndarray:
    """Pre-activations of the bf16 path from a float32 pack: bf16(W_e) . bf16(x) + (b_e - bf16(W_e) . b_pre), the folded
    bias rounded to float32 as the device stores it; float64 otherwise."""
    total, off = lay
    H = off[3] - off[2]
    D = off[4] - off[3]
    p = np.asarray(pack, F32)
    w = bf16(p[off[0]:off[1]].reshape(H, D)).astype(F64)
    c = (p[off[2]:off[3]].astype(F64) - w @ p[off[4]:off[4] + D].astype(F64)).astype(F32)
    return bf16(np.asarray(x, F32)).astype(F64) @ w.T + c.astype(F64)
