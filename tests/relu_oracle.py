"""Float64 reference of the ReLU + L1 step (``wsae_relu.hip``, ``wsae_gemm256x.hip``) with derived bounds, stage by stage.

TEST INFRASTRUCTURE, plain numpy in the style of ``tests/optim_oracle.py`` and ``tests/ring_oracle.py``: no torch, nothing
from the reference tree.  Every function returns ``(value, bound)`` per element.  Each stage takes the DEVICE's output of
the stage before it, so a bound never has to carry a bf16 rounding of a value that is itself only known to within a
bound: the one place where that cannot be avoided (dpre, an internal buffer) is handled element by element below.

Where a value is rounded (read from the kernels; B rows, D columns, H features, ldT = B rounded up to 128).

General flow (``forward_t`` / ``backward_t``; T = bf16_t in BF16 mode, float in FP32 mode):
  xb       ``stage_batch_kernel``: T(x - b_pre), b_pre = 0 here.  One defined rounding of an input: mirrored exactly.
  pre      fp32 accumulation over K = D of T x T products (``encode_direct_kernel`` / ``encode_gemm_kernel`` /
           ``encode_gemm256d_kernel``), plus the bias: one add.  bf16 x bf16 products are exact in fp32; fp32 x fp32
           products sit inside an fma, one rounding per step either way.
  hidden   ``relu_act_kernel``: fmaxf(pre, 0), exact; stored as fp32 (the API copy) AND as T (hid, hidT): the bf16 store
           is the bf16 of the fp32 value the API returns - mirrored exactly from the device's hidden.
  recon    ``gemm_nt`` over K = H of T(hidden) x T(W_d), bias added on slab 0: fp32 store.
  loss     r = recon - x in fp32 from the STORED recon and the caller's x (not xb), r r, two-level partial sums.
  g        fp32((recon - x)) * scale in fp32, scale = 2.0f / ((float)B * (float)loss_cols): mirrored exactly in
           np.float32.  Stored as T (row-major into xb, transposed into gT): bf16 of the mirrored value.
  part_dbd column sums of the fp32 products r * scale, taken BEFORE the T store (the LDS tile holds fp32).
  dh       fp32 accumulation over K = D of T(g) x T(W_d), no bias; fp32 store (into ctx->pre).
  dpre     ``dpre_kernel``: hidden > 0 ? dh + fl(l1 w) : 0 with l1 = weight / ((float)B * (float)H) in fp32; stored as T
           (dpreT).  colpart (db_e) sums the fp32 values BEFORE the T store.
  dW_e     fp32 accumulation over K = ldT (zero padded) of T(dpre) x xb, split in nz K ranges; ``slab_sum_kernel`` adds
           the nz slabs.  dW_d^T likewise from T(hidden) x T(g).

Row-major-GEMM flow (``forward_x`` / ``backward_x``, BF16 mode only):
  xb       ``stage_batch_kernel`` / ``stage_rows_copy_kernel``: bf16(x), as above.
  hidden   ``GX_EPI_RELU``: fmaxf(acc + bias, 0) in fp32, stored as bf16 (ws.hid) and, when asked for, as fp32: the same
           value twice, so bf16(hidden_dev) is again what the decoder GEMM reads.  The activity bits are v > 0 of the
           fp32 value, which is also bf16(v) > 0.
  recon    two split-K slabs over H / 2 each (``GX_EPI_PLAIN``, bias on slab 0), added in ``resid_kernel`` (one more
           rounding) and stored as fp32 from there.
  g, part_dbd   the same ``resid_kernel`` as above, g as bf16 into ctx->gb.
  dpre     ``GX_EPI_DPRE``: bit ? acc + l1 w : 0 (the product may be contracted into an fma), stored as bf16; the column
           sums (colpart, db_e) are of the fp32 values BEFORE the bf16 store.
  dW_e, dW_d^T  ``wgrad2d_kernel`` + ``grad_finish_kernel`` (D > 256) or two ``gemm256x`` contractions +
           ``slab_sum8_kernel``: fp32 accumulation over K = B of bf16 x bf16, at most 8 slabs added.

Error model (that of tests/test_gpu_optimizer_tail.py).  u = 2^-24 per correctly rounded fp32 operation.  A length-K fp32
accumulation of products is within (K + c) u sum|a||b| of the exact sum, c counting the additional roundings a term
passes through: the bias add (1), the sum of two recon slabs (1), nz slab sums.  Bounds are first order; ``SECOND`` covers
the products of errors and ``FLOOR`` the exact zeros.

dpre is internal and is rounded to bf16 AFTER a computation that is only known to within a bound.  Its float64 value p
and bound e give the interval [p - e, p + e]; where both ends round to the same bfloat16 the device's value is
determined and the allowance is zero, elsewhere it is the distance to the farther candidate (one bf16 ulp).  The bound
holds for every element and is zero on nearly all of them; the weight-gradient bound carries sum_b delta_b |x_b| of it.

Counts of the reductions (non-negative terms: relative to the sum).
  sparsity  general: product with the weight 1, sums inside the float4 2, 4 accumulations, ``block_sum`` 6 + 4, the finish
            Tp = ceil(nblk / 256) adds, ``block_sum`` 10, the product (float)B (float)H and the division 2: 29 + Tp.
            row-major-GEMM: 32 accumulations per lane, 6 wave steps, 8 serial adds, the same finish: 61 + Tp.
  mse       r carries 1 (its square 2), the square 1, float4 sums 2, 4 accumulations, ``block_sum`` 10, the finish
            Tp + 12: 31 + Tp.
  loss      mse + weight * sparsity: one product, one add.   l0: the counts are integers below 2^24, one division.
  db_d      64 serial adds per tile, then ceil(B / 64) serial adds (``colsum_kernel``) or a quarter of them and 2
            (``colsum2_kernel``): 64 + ceil(B / 64).
  db_e      the same count (the epilogue's 32 + 2 per 128 rows is below it), on top of the carried dh bounds.
"""

from __future__ import annotations

import numpy as np

from oracle.synth import bf16_round

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
SECOND = 1.02
FLOOR = 2.0 ** -124
MAX_SPLIT = 8  # WSAE_WGRAD_MAX_SPLIT


def bf16_of_f64(v):
    """Nearest bfloat16 (ties to even) of float64 values in the normal range, as float64: no detour through fp32."""
    v = np.asarray(v, F64)
    _, e = np.frexp(v)
    q = np.ldexp(1.0, e - 8)
    return np.rint(v / q) * q


def operands(W_e, W_dT, x, rows, prec):
    """(W_e, W_dT, xs, xr) as the kernels read them: the bf16 shadows and bf16(x) in bf16 mode; xr is the caller's x
    gathered through ``rows``, what the residual is taken against."""
    xr = np.asarray(x, F32) if rows is None else np.asarray(x, F32)[np.asarray(rows, np.int64)]
    if prec == "bf16":
        return bf16_round(W_e), bf16_round(W_dT), bf16_round(xr), xr
    return np.asarray(W_e, F32), np.asarray(W_dT, F32), xr, xr


def _gemm(a, b, k_extra):
    """a @ b in float64 with the (K + k_extra) u sum|a||b| bound."""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    return a @ b, (a.shape[1] + k_extra) * U * (np.abs(a) @ np.abs(b))


def hidden(xs, W_e, b_e, c=2):
    """Stage a.  (pre, hidden, bound, exact): relu is 1-Lipschitz, so hidden shares the bound of pre.  ``exact`` marks
    the elements whose every term is zero: the device computes those exactly."""
    pre, bnd = _gemm(xs, np.asarray(W_e, F64).T, c)
    b = np.asarray(b_e, F64)[None, :]
    pre = pre + b
    bnd = bnd + (xs.shape[1] + c) * U * np.abs(b)
    exact = bnd == 0
    return pre, np.maximum(pre, 0.0), bnd * SECOND + FLOOR, exact


def unsure(pre, bound, exact):
    """Stage b.  Where the device's ``hidden > 0`` may differ from the reference's."""
    return (np.abs(pre) <= bound) & ~exact


def recon(hidden_dev, W_dT, b_d, prec, c=3):
    """Stage c.  From the device's hidden, rounded as the decoder GEMM reads it."""
    hs = bf16_round(hidden_dev) if prec == "bf16" else np.asarray(hidden_dev, F32)
    val, bnd = _gemm(hs, W_dT, c)
    b = np.asarray(b_d, F64)[None, :]
    return val + b, (bnd + (hs.shape[1] + c) * U * np.abs(b)) * SECOND + FLOOR


def n_partials(B, D, H):
    ldT = -(-B // 128) * 128
    return -(-(-(-max(D, H) // 64) * (ldT // 64)) // 256)


def scalars(hidden_dev, recon_dev, xr, weight, l1w, loss_cols, flow):
    """Stage d.  {"sparsity", "mse", "loss", "l0"}: (value, bound) each, from the device's hidden and recon."""
    B, H = hidden_dev.shape
    D = recon_dev.shape[1]
    tp = n_partials(B, D, H)
    w = np.ones(H, F64) if l1w is None else np.asarray(l1w, F64)
    h = np.asarray(hidden_dev, F64)
    sp = float((h * w[None, :]).sum() / (B * H))
    d_sp = ((61 if flow == "xgemm" else 29) + tp) * U * sp * SECOND + FLOOR
    r = np.asarray(recon_dev, F64) - np.asarray(xr, F64)
    mse = float((r * r).sum() / (B * loss_cols))
    d_mse = (31 + tp) * U * mse * SECOND + FLOOR
    wt = float(F32(weight))
    loss = mse + wt * sp
    d_loss = d_mse + wt * d_sp + U * wt * sp + U * loss
    l0 = float((np.asarray(hidden_dev) > 0).sum() / B)
    return {"sparsity": (sp, d_sp), "mse": (mse, d_mse), "loss": (loss, d_loss * SECOND + FLOOR), "l0": (l0, U * l0 + FLOOR)}


def g_exact(recon_dev, xr, B, loss_cols):
    """Stage e.  The fp32 g of ``resid_kernel``, operation for operation."""
    scale = F32(2.0) / (F32(B) * F32(loss_cols))
    return ((np.asarray(recon_dev, F32) - np.asarray(xr, F32)).astype(F32) * scale).astype(F32)


def g_operand(g32, prec):
    return bf16_round(g32) if prec == "bf16" else g32


def db_d(g32):
    B = g32.shape[0]
    g = np.asarray(g32, F64)
    return g.sum(axis=0), (64 + -(-B // 64)) * U * np.abs(g).sum(axis=0) * SECOND + FLOOR


def l1_term(weight, l1w, B, H):
    l1 = F32(weight) / (F32(B) * F32(H))
    w = np.ones(H, F32) if l1w is None else np.asarray(l1w, F32)
    return float(l1) * w.astype(F64)


def dpre(gs, W_dT, active, weight, l1w, prec, c=2):
    """Stage f.  (dpre as the contraction reads it, its allowance delta, the fp32 dpre in float64, its bound).
    ``active`` is the DEVICE's hidden > 0."""
    B, H = active.shape
    dh, bnd = _gemm(gs, np.asarray(W_dT, F64).T, c)
    l1 = l1_term(weight, l1w, B, H)[None, :]
    p = np.where(active, dh + l1, 0.0)
    e = np.where(active, (bnd + U * np.abs(l1) + U * np.abs(dh + l1)) * SECOND + FLOOR, 0.0)
    if prec != "bf16":
        return p, e, p, e
    pb = bf16_of_f64(p)
    delta = np.maximum(np.abs(bf16_of_f64(p + e) - pb), np.abs(bf16_of_f64(p - e) - pb))
    return pb, delta, p, e


def db_e(p, e):
    B = p.shape[0]
    return p.sum(axis=0), (e.sum(axis=0) + (64 + -(-B // 64)) * U * np.abs(p).sum(axis=0)) * SECOND + FLOOR


def wgrads(dpre_b, delta, xs, hidden_dev, gs, prec, nz=MAX_SPLIT, c=2):
    """Stage g.  ((dW_e, bound), (dW_d^T, bound)), both [H, D]."""
    B = dpre_b.shape[0]
    n = (B + nz + c) * U
    xa = np.abs(np.asarray(xs, F64))
    dWe = dpre_b.T @ np.asarray(xs, F64)
    bWe = (delta.T @ xa + n * ((np.abs(dpre_b) + delta).T @ xa)) * SECOND + FLOOR
    hs = (bf16_round(hidden_dev) if prec == "bf16" else np.asarray(hidden_dev, F32)).astype(F64)
    g = np.asarray(gs, F64)
    dWd = hs.T @ g
    bWd = n * (np.abs(hs).T @ np.abs(g)) * SECOND + FLOOR
    return (dWe, bWe), (dWd, bWd)


def check_step(W_e, W_dT, b_e, b_d, x, rows, prec, flow, weight, l1w, loss_cols, out):
    """Every stage against ``out`` = {"hidden", "recon", "loss", "l0", "sparsity", "dW_e", "dW_dT", "db_e", "db_d"} (the
    device's outputs, or an emulation's).  Returns {name: worst error / bound} and {"unsure_share", "conflicts"}."""
    We_s, Wd_s, xs, xr = operands(W_e, W_dT, x, rows, prec)
    B = xs.shape[0]
    res = {}

    def ratio(name, got, ref, bound):
        res[name] = float((np.abs(np.asarray(got, F64) - ref) / bound).max())

    pre, hid_ref, b_h, exact = hidden(xs, We_s, b_e)
    ratio("hidden", out["hidden"], hid_ref, b_h)
    un = unsure(pre, b_h, exact)
    active = np.asarray(out["hidden"]) > 0
    res["unsure_share"] = float(un.mean())
    res["conflicts"] = int(((active != (pre > 0)) & ~un).sum())
    ratio("recon", out["recon"], *recon(out["hidden"], Wd_s, b_d, prec))
    sc = scalars(out["hidden"], out["recon"], xr, weight, l1w, loss_cols, flow)
    for k in ("loss", "l0", "sparsity"):
        ratio(k, out[k], *sc[k])
    g32 = g_exact(out["recon"], xr, B, loss_cols)
    ratio("db_d", out["db_d"], *db_d(g32))
    gs = g_operand(g32, prec)
    pb, delta, p, e = dpre(gs, Wd_s, active, weight, l1w, prec)
    res["dpre_allowed_share"] = float((delta > 0).mean()) if prec == "bf16" else 1.0
    ratio("db_e", out["db_e"], *db_e(p, e))
    (dWe, bWe), (dWd, bWd) = wgrads(pb, delta, xs, out["hidden"], gs, prec)
    ratio("dW_e", out["dW_e"], dWe, bWe)
    ratio("dW_dT", out["dW_dT"], dWd, bWd)
    # where dW_e is closest to its bound: the share of that bound which is the dpre allowance (a dpre that took the other
    # bf16 candidate moves the entry by ulp |x|, which is that allowance: a ratio near 1 there is one flipped rounding)
    at = np.unravel_index(int(np.argmax(np.abs(np.asarray(out["dW_e"], F64) - dWe) / bWe)), bWe.shape)
    res["dW_e_worst_allowance_part"] = float((delta.T[at[0]] @ np.abs(np.asarray(xs, F64))[:, at[1]]) * SECOND / bWe[at])
    return res
