"""The float64 optimizer-tail oracle (tests/optim_oracle.py) against torch itself, on the CPU.

``clip_grad_norm_`` + ``torch.optim.AdamW`` + ``F.normalize(W_d, dim=0)`` on float64 tensors are the reference: a 32 -> 64
pack with non-zero moments and ``weight_decay = 0.01``, update counts 1, 2 and 1000, ``"torch"`` mode, 1e-12 relative.
The last test pins the arithmetic fact behind the double hyper-parameters of ``wsae_adamw_step``: torch multiplies
``g * g`` by ``float32(1 - beta2)``, which is not ``1 - float32(beta2)``.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import optim_oracle as OO
from oracle import sae_oracle as O
from oracle import synth

D, H = 32, 64
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01)


def _state(seed=3):
    lay = OO.layout(D, H)
    total = lay[0]
    pack = synth.normal((total,), seed, 1) * np.float32(0.2)
    grads = synth.normal((total,), seed, 2)
    m = synth.normal((total,), seed, 3) * np.float32(0.5)
    v = synth.uniform((total,), seed, 4, 0.25, 1.5)
    return lay, pack, grads, m, v


def _torch_step(lay, pack, grads, m, v, step, max_norm, dtype):
    """The reference's tail on torch tensors of ``dtype``: five parameters carved out of the pack, moments loaded through
    the optimizer's state dict with ``step - 1`` updates behind them."""
    names = OO.SEGMENTS
    params = []
    for name in names:
        t = torch.tensor(np.ascontiguousarray(OO.segment(pack, lay, name, D, H)), dtype=dtype)
        if name == "W_dT":
            t = t.t().contiguous()  # decoder.weight [D, H]
        params.append(torch.nn.Parameter(t))
    opt = torch.optim.AdamW(params, lr=HYPER["lr"], betas=(HYPER["beta1"], HYPER["beta2"]), eps=HYPER["eps"],
                            weight_decay=HYPER["weight_decay"], foreach=False)
    for name, p in zip(names, params):
        tr = (lambda a: a.t().contiguous()) if name == "W_dT" else (lambda a: a)
        p.grad = tr(torch.tensor(np.ascontiguousarray(OO.segment(grads, lay, name, D, H)), dtype=dtype))
        opt.state[p] = {"step": torch.tensor(float(step - 1)),
                        "exp_avg": tr(torch.tensor(np.ascontiguousarray(OO.segment(m, lay, name, D, H)), dtype=dtype)),
                        "exp_avg_sq": tr(torch.tensor(np.ascontiguousarray(OO.segment(v, lay, name, D, H)), dtype=dtype))}
    norm = torch.nn.utils.clip_grad_norm_(params, max_norm) if max_norm > 0 else None
    opt.step()
    with torch.no_grad():
        params[1].copy_(F.normalize(params[1], dim=0))
    back = lambda name, t: (t.t() if name == "W_dT" else t).detach().numpy().reshape(-1)  # noqa: E731
    cat = lambda key: np.concatenate([back(n, p if key is None else opt.state[p][key]) for n, p in zip(names, params)])  # noqa: E731
    return cat(None), cat("exp_avg"), cat("exp_avg_sq"), None if norm is None else float(norm)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("step", [1, 2, 1000])
@pytest.mark.parametrize("max_norm", [1.0, 0.0])
def test_tail_matches_torch_in_float64(step, max_norm):
    lay, pack, grads, m, v = _state()
    hyper = dict(HYPER, mode="torch", dtype=np.float64)
    got = OO.tail(pack, grads, m, v, lay, hyper, step, max_norm, 1.0, True)
    p_t, m_t, v_t, norm_t = _torch_step(lay, pack, grads, m, v, step, max_norm, torch.float64)
    assert _rel(got["pack"], p_t) <= 1e-12
    assert _rel(got["m"], m_t) <= 1e-12
    assert _rel(got["v"], v_t) <= 1e-12
    if max_norm > 0:
        assert abs(got["grad_norm"] - norm_t) / norm_t <= 1e-12
        assert got["clip_coef"] < 1.0  # ||g|| ~ 65: the clip is active
    else:
        assert got["clip_coef"] == 1.0


def test_tail_agrees_with_the_step_oracle():
    """The same update through ``oracle.sae_oracle.adamw_update`` / ``normalize_decoder`` (which store float32 moments
    and parameters as the reference does): equal up to those float32 stores."""
    lay, pack, grads, m, v = _state(5)
    got = OO.tail(pack, grads, m, v, lay, dict(HYPER, mode="as_passed"), 7, 1.0, 1.0, True)
    coef = O.clip_coef(got["grad_norm"], 1.0)
    p2, m2, v2 = O.adamw_update(pack, (grads.astype(np.float64) * coef).astype(np.float32), m, v, 7, HYPER["lr"],
                                HYPER["beta1"], HYPER["beta2"], HYPER["eps"], HYPER["weight_decay"])
    assert _rel(got["m"], m2) < 2e-7 and _rel(got["v"], v2) < 2e-7
    wd = OO.segment(p2, lay, "W_dT", D, H)
    OO.segment(p2, lay, "W_dT", D, H)[:] = O.normalize_decoder(wd.T).T
    assert _rel(got["pack"], p2) < 3e-7


def test_dead_clock_resample_and_small_helpers():
    last = np.array([5, 90, 89, -3, 100], np.int64)
    out = OO.tail(np.zeros(2 * 32 * 32 + 96, np.float32), np.zeros(2144, np.float32), np.zeros(2144, np.float32),
                  np.zeros(2144, np.float32), OO.layout(32, 32), dict(HYPER, mode="as_passed"), 1, 0.0, 1.0, False,
                  last=np.resize(last, 32), step_count=100, thr=10, fired=np.resize(np.array([1.0, 0, 0, 0, 0]), 32))
    merged = np.resize(last, 32).copy()
    merged[np.resize(np.array([1.0, 0, 0, 0, 0]), 32) > 0] = 100
    assert np.array_equal(out["last"], merged)
    assert out["dead_count"] == int(((100 - merged) > 10).sum())  # 100 - 90 = 10 is alive (strict)
    mask, cnt = OO.dead_scan(last, 100, 10)
    assert mask.tolist() == [1, 0, 1, 1, 0] and cnt == 3
    # resample: ties go to the lower row, a zero row gives a zero feature, the count is capped but not by the rows
    lay = OO.layout(32, 32)
    pack = synth.normal((lay[0],), 9, 1)
    x = synth.normal((3, 32), 9, 2)
    x[1] = 0
    dm = np.zeros(32, np.uint8)
    dm[[4, 7, 9, 20]] = 1
    r = OO.resample(pack, lay, x, np.array([2.0, 5.0, 5.0], np.float32), dm, np.zeros(32, np.int64), 77, -1)
    assert r["n_dead_out"] == 4 and r["features"].tolist() == [4, 7, 9] and r["order"].tolist() == [1, 2, 0]
    We = OO.segment(r["pack"], lay, "W_e", 32, 32)
    assert not We[4].any() and abs(np.linalg.norm(We[7]) - 1) < 1e-12 and np.array_equal(We[20], OO.segment(pack, lay, "W_e", 32, 32)[20])
    assert r["last"][[4, 7, 9, 20]].tolist() == [77, 77, 77, 0]
    assert OO.resample(pack, lay, x, np.ones(3, np.float32), dm, np.zeros(32, np.int64), 1, 2)["n_dead_out"] == 2
    assert OO.bf16(np.array([1.00390625, 1.01171875], np.float32)).tolist() == [1.0, 1.015625]  # ties to even, both ways
    err, resid = OO.row_errors(x, np.zeros((2, 32), np.float32), rows=[2, 0])
    assert np.allclose(err, (x[[2, 0]].astype(np.float64) ** 2).sum(1), rtol=1e-15) and np.array_equal(resid, x[[2, 0]])


def test_torch_scales_g_squared_by_float32_of_one_minus_beta2():
    """float32 tensors, zero moments, one step, gradients that are powers of two: ``exp_avg_sq / g^2`` is exactly
    ``float32(0.001)`` - torch forms ``1 - beta2`` in double and rounds once.  ``1 - float32(0.999)``, what fp32 kernel
    arithmetic on a float32 ``beta2`` gives, is 1.29e-5 away; the oracle's ``"torch"`` mode carries torch's constant."""
    g = np.array([2.0, -0.5, 8.0, 1.0], np.float32)
    p = torch.nn.Parameter(torch.zeros(4))
    opt = torch.optim.AdamW([p], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, foreach=False)
    p.grad = torch.from_numpy(g.copy())
    opt.step()
    ratio = opt.state[p]["exp_avg_sq"].numpy().astype(np.float64) / (g.astype(np.float64) ** 2)
    assert np.all(ratio == float(np.float32(0.001)))
    wrong = float(np.float32(1.0) - np.float32(0.999))
    assert abs(wrong - 0.001) / 0.001 == pytest.approx(1.2875e-5, rel=1e-3)
    assert np.all(ratio != wrong)
    c = OO.adam_constants(dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, mode="torch"), 1)
    assert c["omb2"] == float(np.float32(0.001)) and c["omb1"] == float(np.float32(1.0 - 0.9))
    lay = (4, [0, 0, 0, 0, 0])  # (a four-element pack that is all b_pre: the arithmetic of `tail` is per element)
    out = OO.tail(np.zeros(4, np.float32), g, np.zeros(4, np.float32), np.zeros(4, np.float32), (4, [0, 0, 0, 0, 0]),
                  dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, mode="torch"), 1, 0.0, 1.0, False)
    assert np.array_equal(out["v"].astype(np.float32), opt.state[p]["exp_avg_sq"].numpy())
    assert np.array_equal(out["m"].astype(np.float32), opt.state[p]["exp_avg"].numpy())
    assert lay[0] == 4
