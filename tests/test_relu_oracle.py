"""The ReLU-step oracle (tests/relu_oracle.py) on the CPU: its values, its bounds, and what the bounds can see.

* Reference check: with exact (fp32-mode) inputs the staged float64 values agree with ``O.relu_forward`` /
  ``O.relu_backward`` inside the oracle's own bounds, and with the g8 golden at that test's tolerance.
* Bound check: an ``np.float32`` emulation of the device chain - one rounded add per product, K walked backwards (not the
  device's order), every bf16 store, two batch slabs - stays inside every bound, in bf16 and in fp32 mode.
* Sensitivity: ten plausible faults, injected into that emulation at the smallest case of tests/test_gpu_relu_step.py
  (96 x 352 at B = 200, bf16, with ``rows``, per-feature L1 weights and ``loss_cols = D / 2``), each exceed the bound on
  the tensor they touch.  That is what makes the GPU file's assertions able to fail.
"""

from __future__ import annotations

import numpy as np
import pytest

import relu_oracle as RO
from oracle import sae_oracle as O
from oracle import synth

F32, F64 = np.float32, np.float64
WEIGHT = 0.05
DEAD = 3  # a planted feature with a zero encoder row and a zero bias: pre == 0 exactly


def problem(D, H, B, seed, with_rows, with_l1w, half_cols):
    w = synth.sae_weights(D, H, seed=seed, bf16=False)
    W_e, b_e = w["encoder.weight"].copy(), w["encoder.bias"].copy()
    W_e[DEAD], b_e[DEAD] = 0, 0
    n_src = 2 * B + 5 if with_rows else B
    x = synth.activations(n_src, D, seed=seed, stream=5, bf16=False)
    rows = ((n_src - 1 - (np.arange(B) * 3) % n_src) % n_src).astype(np.int32) if with_rows else None
    if with_rows:
        rows[5] = rows[4]  # a repeated index
    l1w = synth.uniform((H,), seed, 21, 0.5, 1.5) if with_l1w else None
    return dict(W_e=W_e, W_dT=np.ascontiguousarray(w["decoder.weight"].T), b_e=b_e, b_d=w["decoder.bias"], x=x, rows=rows,
                weight=WEIGHT, l1w=l1w, loss_cols=D // 2 if half_cols else D)


def seq_gemm(a, b):
    """a [M, K] . b [K, N] with one fp32 rounding per product and per add, K walked from the far end."""
    acc = np.zeros((a.shape[0], b.shape[1]), F32)
    for k in range(a.shape[1] - 1, -1, -1):
        acc = (acc + (a[:, k, None] * b[None, k, :]).astype(F32)).astype(F32)
    return acc


def emulate(p, prec, fault=None):
    """The device chain in np.float32.  ``fault`` names one deliberate mistake."""
    rnd = synth.bf16_round if prec == "bf16" else (lambda a: np.asarray(a, F32))
    W_e, W_dT = rnd(p["W_e"]), rnd(p["W_dT"])
    B = len(p["rows"]) if p["rows"] is not None else p["x"].shape[0]
    H, D = W_e.shape
    xg = p["x"][:B] if (fault == "rows_ignored" or p["rows"] is None) else p["x"][p["rows"]]
    xs = rnd(xg)
    pre = (seq_gemm(xs, W_e.T.copy()) + p["b_e"][None, :]).astype(F32)
    hid = np.maximum(pre, F32(0))
    hs = hid if fault == "hidden_unrounded" else rnd(hid)
    rec = (seq_gemm(hs, W_dT) + p["b_d"][None, :]).astype(F32)
    w = np.ones(H, F32) if p["l1w"] is None else p["l1w"].astype(F32)
    sp = (hid * w[None, :]).astype(F32).sum(dtype=F32) / (F32(B) * F32(H))
    r = (rec - xg).astype(F32)
    mse = (r * r).astype(F32).sum(dtype=F32) / (F32(B) * F32(p["loss_cols"]))
    loss = F32(mse + F32(F32(p["weight"]) * sp))
    cols = D if fault == "loss_cols_is_D" else p["loss_cols"]
    g32 = (r * (F32(2.0) / (F32(B) * F32(cols)))).astype(F32)
    gs = rnd(g32)
    dh = seq_gemm(gs, W_dT.T.copy())
    l1 = F32(p["weight"]) / (F32(B) * F32(H))
    l1v = (l1 * (np.ones(H, F32) if fault == "l1_weights_ignored" else w)).astype(F32)
    if fault == "no_l1":
        l1v = np.zeros(H, F32)
    active = (pre >= 0) if fault == "mask_ge" else (hid > 0)
    dp = np.where(active, (dh + l1v[None, :]).astype(F32), F32(0)).astype(F32)
    dpb = rnd(dp)
    sel = np.arange(B)
    if fault == "row_dropped":
        sel = np.delete(sel, 7)
    if fault == "last_row_twice":
        sel = np.append(sel, B - 1)
    halves = [sel[:len(sel) // 2], sel[len(sel) // 2:]]
    if fault == "slab_missing":
        halves = halves[:1]
    if fault == "slab_twice":
        halves = halves + halves[1:]

    def contract(a, b):
        out = np.zeros((H, D), F32)
        for s in halves:
            out = (out + seq_gemm(a[s].T.copy(), b[s])).astype(F32)
        return out

    return {"hidden": hid, "recon": rec, "loss": loss, "l0": F32((hid > 0).sum()) / F32(B), "sparsity": sp,
            "dW_e": contract(dpb, xs), "dW_dT": contract(hs if fault != "hidden_unrounded" else rnd(hid), gs),
            "db_e": dp.sum(axis=0, dtype=F32), "db_d": g32.sum(axis=0, dtype=F32)}


def staged(p, prec, flow, out):
    return RO.check_step(p["W_e"], p["W_dT"], p["b_e"], p["b_d"], p["x"], p["rows"], prec, flow, p["weight"], p["l1w"],
                         p["loss_cols"], out)


TENSORS = ("hidden", "recon", "loss", "l0", "sparsity", "db_d", "db_e", "dW_e", "dW_dT")
SMALLEST = dict(D=96, H=352, B=200, seed=200)


@pytest.fixture(scope="module")
def smallest():
    return problem(SMALLEST["D"], SMALLEST["H"], SMALLEST["B"], SMALLEST["seed"], True, True, True)


def test_bf16_of_f64_equals_the_fp32_rounding():
    v = np.concatenate([synth.normal((4096,), 3, 1) * F32(s) for s in (1e-6, 1.0, 300.0)])
    ties = np.array([1.00390625, 1.01171875, -1.00390625, 0.0], F32)  # halfway between two bfloat16: to even
    v = np.concatenate([v, ties])
    assert np.array_equal(RO.bf16_of_f64(v.astype(F64)), synth.bf16_round(v).astype(F64))


def test_values_agree_with_the_step_oracle_and_the_g8_golden(golden_dir):
    g = np.load(golden_dir / "g8_relu.npz")
    D, H, B = (int(v) for v in g["dims"])
    w = synth.sae_weights(D, H, seed=11, bf16=False)
    x = synth.activations(B, D, seed=11, stream=5, bf16=False)
    args = (w["encoder.weight"], w["encoder.bias"], w["decoder.weight"], w["decoder.bias"], x)
    f = O.relu_forward(*args, sparsity_weight=0.01)
    b = O.relu_backward(*args, f, sparsity_weight=0.01)
    out = {"hidden": f["hidden"], "recon": f["reconstructed"], "loss": f["loss"], "l0": f["l0"], "sparsity": f["sparsity_loss"],
           "dW_e": b["W_e"], "dW_dT": b["W_d"].T, "db_e": b["b_e"], "db_d": b["b_d"]}
    res = RO.check_step(args[0], np.ascontiguousarray(args[2].T), args[1], args[3], x, None, "fp32", "general", 0.01, None, D, out)
    print({k: round(v, 4) for k, v in res.items()})
    assert res["conflicts"] == 0
    for k in TENSORS:
        assert res[k] <= 1.0, (k, res[k])
    # the staged values themselves against the golden (the tolerance of tests/test_oracle_golden.py::TestReLUG8)
    We_s, Wd_s, xs, xr = RO.operands(args[0], np.ascontiguousarray(args[2].T), x, None, "fp32")
    g32 = RO.g_exact(f["reconstructed"], xr, B, D)
    pb, delta, p, e = RO.dpre(g32, Wd_s, f["hidden"] > 0, 0.01, None, "fp32")
    (dWe, _), (dWd, _) = RO.wgrads(pb, delta, xs, f["hidden"], g32, "fp32")

    def rel(a, ref):
        return float(np.abs(a - ref).max() / np.abs(ref).max())

    assert rel(RO.recon(f["hidden"], Wd_s, args[3], "fp32")[0], g["recon"]) < 1e-5
    assert rel(dWe, g["dW_e"]) < 2e-5 and rel(dWd.T, g["dW_d"]) < 2e-5
    assert rel(RO.db_e(p, e)[0], g["db_e"]) < 2e-5 and rel(RO.db_d(g32)[0], g["db_d"]) < 2e-5


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_emulation_stays_inside_every_bound(smallest, prec):
    res = staged(smallest, prec, "general", emulate(smallest, prec))
    print(prec, {k: round(v, 4) for k, v in res.items()})
    print(f"worst error / bound ({prec}): {max(res[k] for k in TENSORS):.3f}")
    assert res["conflicts"] == 0 and res["unsure_share"] <= 1e-3
    for k in TENSORS:
        assert res[k] <= 1.0, (k, res[k])
    if prec == "bf16":
        # the allowance is zero on nearly every element: the interval is 2 (D + 2) u sum|g||W| wide against a bf16 ulp of
        # >= 2^-8 |dpre|, i.e. at most ~2 x 6e-6 x sqrt(D) x 256 = 3% of an ulp here
        assert res["dpre_allowed_share"] < 0.1


def test_emulation_without_the_extras_stays_inside_every_bound():
    p = problem(128, 256, 256, 201, False, False, False)
    res = staged(p, "bf16", "xgemm", emulate(p, "bf16"))
    print({k: round(v, 4) for k, v in res.items()})
    assert res["conflicts"] == 0 and res["unsure_share"] <= 1e-3
    for k in TENSORS:
        assert res[k] <= 1.0, (k, res[k])


FAULTS = [("row_dropped", ("dW_e", "dW_dT")), ("last_row_twice", ("dW_e", "dW_dT")), ("slab_missing", ("dW_e", "dW_dT")),
          ("slab_twice", ("dW_e", "dW_dT")), ("no_l1", ("db_e", "dW_e")), ("l1_weights_ignored", ("db_e",)),
          ("loss_cols_is_D", ("db_d",)), ("hidden_unrounded", ("recon",)), ("rows_ignored", ("hidden",)), ("mask_ge", ("db_e",))]


@pytest.mark.parametrize("fault,touched", FAULTS, ids=[f[0] for f in FAULTS])
def test_each_fault_exceeds_its_bound(smallest, fault, touched):
    res = staged(smallest, "bf16", "general", emulate(smallest, "bf16", fault))
    print(fault, {k: round(res[k], 3) for k in touched})
    for k in touched:
        assert res[k] > 1.0, (fault, k, res[k])
