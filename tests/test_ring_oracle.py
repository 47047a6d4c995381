"""The ring oracle (tests/ring_oracle.py) against independent restatements, on the CPU.

* ``feistel_rows``: a bijection at every size class of the domain sizing, equal to a scalar Python-int restatement.
* ``RingModel``: equal to a row-at-a-time list model over a scripted push sequence.
* ``layernorm``: the value against torch's float64 ``layer_norm``; the BOUND against an fp32 numpy emulation of the kernel's
  exact order (64 lanes, ``vpl`` registers, xor butterfly 32 .. 1).  The faithful emulation stays below the bound on
  every input family the GPU test uses, and each of five deliberately wrong variants exceeds it on at least one: that
  is what makes ``tests/test_gpu_ring.py``'s assertion able to fail.
* ``decode_dense``: value and bound against an fp32 emulation of the fmaf chain.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

import ring_oracle as RO
from oracle import synth

F32, F64 = np.float32, np.float64
M64 = (1 << 64) - 1


# ---- feistel_rows ------------------------------------------------------------------------------------------------------
def _mix64_int(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _sample_scalar(size, seed, epoch, offset, n):
    """``wsae_ring_sample`` + ``feistel_perm`` on Python integers, one index at a time."""
    bits = 1
    while (1 << bits) < size:
        bits += 1
    half = (bits + 1) // 2
    mask = (1 << half) - 1
    key = _mix64_int(_mix64_int(seed & M64) ^ (((epoch & M64) * 0xD1342543DE82EF95) & M64))
    out = []
    for i in range(n):
        v = (offset + i) % size
        while True:
            l, r = v >> half, v & mask
            for rnd in range(4):
                f = _mix64_int(r ^ key ^ (rnd << 56)) & mask
                l, r = r, l ^ f
            v = (l << half) | r
            if v < size:
                break
        out.append(v)
    return np.array(out, np.int64)


SIZES = [1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 1000, 1023, 1024, 1025, 4097, 70001]


@pytest.mark.parametrize("size", SIZES)
def test_feistel_rows_is_a_bijection(size):
    for seed, epoch in ((42, 0), (42, 1), ((1 << 63) + 5, 1 << 40)):
        p = RO.feistel_rows(size, seed, epoch, 0, size)
        assert p.dtype == np.int64 and np.array_equal(np.sort(p), np.arange(size)), (size, seed, epoch)


@pytest.mark.parametrize("size", [1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 1000, 1025])
def test_feistel_rows_equals_the_scalar_restatement(size):
    for seed, epoch, offset in ((42, 0, 0), ((1 << 63) + 5, 1 << 40, size // 2 + 1), (0, 3, 2 * size + 1)):
        n = min(size + 3, 300)
        assert np.array_equal(RO.feistel_rows(size, seed, epoch, offset, n), _sample_scalar(size, seed, epoch, offset, n))


def test_feistel_rows_epochs_seeds_and_wrap():
    size = 1000
    base = RO.feistel_rows(size, 42, 0, 0, size)
    assert not np.array_equal(base, RO.feistel_rows(size, 42, 1, 0, size))
    assert not np.array_equal(base, RO.feistel_rows(size, 43, 0, 0, size))
    assert not np.array_equal(base, RO.feistel_rows(size, 42, 1 << 40, 0, size))
    big = RO.feistel_rows(size, (1 << 63) + 5, 0, 0, size)  # a seed that does not fit a signed 64-bit word
    assert np.array_equal(np.sort(big), np.arange(size)) and not np.array_equal(big, RO.feistel_rows(size, 5, 0, 0, size))
    w = RO.feistel_rows(size, 42, 0, 900, 250)  # offset + n > size: positions 900 .. 999, 0 .. 149
    assert np.array_equal(w, np.concatenate([base[900:], base[:150]]))
    assert np.array_equal(RO.feistel_rows(size, 42, 0, 2300, 10), base[300:310])
    assert RO.feistel_rows(size, 42, 0, 5, 0).size == 0


# ---- RingModel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_ring_model_equals_row_at_a_time_pushes(dtype):
    cap, dim = 10, 3
    model = RO.RingModel(cap, dim, dtype)
    store, head, size = [[0.0] * dim for _ in range(cap)], 0, 0
    rnd = (lambda a: synth.bf16_round(a)) if dtype == "bfloat16" else (lambda a: a)
    script = [("push", 7), ("push", 6), ("push", 0), ("push", 25), ("push", 10), ("fill", 4), ("push", 3), ("push", 11)]
    for step, (op, n) in enumerate(script):
        if op == "fill":
            model.fill(n, seed=9)
            want = rnd(synth.normal((n, dim), 9, 0))
            for r in range(n):
                store[r] = [float(x) for x in want[r]]
            head, size = n % cap, n
        else:
            rows = synth.normal((n, dim), 100 + step, 0) * F32(1.37)
            slots = model.push(rows)
            first = head
            for r in range(n):  # one row at a time: the oldest is overwritten
                store[head] = [float(x) for x in rnd(rows[r])]
                head, size = (head + 1) % cap, min(cap, size + 1)
            assert np.array_equal(slots[max(0, n - cap):], (first + np.arange(n)[max(0, n - cap):]) % cap)
            assert (slots[:max(0, n - cap)] == -1).all()
        assert np.array_equal(model.data, np.array(store, F64)), (step, op, n)
        assert (model.head, model.size) == (head, size), (step, op, n)


# ---- layernorm: value --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 65, 384])
def test_layernorm_value_is_torchs_float64_layer_norm(dim):
    h = RO.ln_inputs("ordinary", 5, dim, 3)
    g, b = RO.ln_params(dim, 4)
    y, bound = RO.layernorm(h, g, b, 1e-5, RO.ln_vpl(dim))
    ref = torch.nn.functional.layer_norm(torch.from_numpy(h).double(), (dim,), torch.from_numpy(g).double(),
                                         torch.from_numpy(b).double(), float(F32(1e-5))).numpy()
    assert np.abs(y - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    assert np.isfinite(bound).all() and (bound > 0).all()


# ---- layernorm: bound --------------------------------------------------------------------------------------------------
def _wave_sum(x):
    lanes = np.arange(64)
    for sh in (32, 16, 8, 4, 2, 1):
        x = x + x[:, lanes ^ sh]  # float32 + float32: one rounding per step, every lane ends with the same total
    return x[:, :1]


def _fma(a, b, c):
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)  # a b exact in float64


def emulate_ln(h, gamma, beta, eps, vpl, wrong=None):
    """fp32 emulation of ``ring_push_ln_kernel`` for float32 rows ``h``; ``wrong`` selects one deliberate mistake."""
    h = np.asarray(h, F32)
    rows, dim = h.shape
    assert dim <= 64 * vpl
    flat = np.zeros((rows, vpl * 64), F32)
    flat[:, :dim] = h
    v = flat.reshape(rows, vpl, 64)  # v[:, i, lane] = column lane + 64 i
    valid = (np.arange(vpl * 64) < dim).reshape(vpl, 64)
    s = np.zeros((rows, 64), F32)
    for i in range(vpl):
        s = s + v[:, i]
    mean = _wave_sum(s) / F32(dim)
    sq = np.zeros((rows, 64), F32)
    for i in range(vpl):
        c = np.where(valid[i], v[:, i] - mean, F32(0)).astype(F32)
        sq = _fma(c, c, sq)
    divisor = F32(dim - 1) if wrong == "unbiased" else F32(dim)
    var = _wave_sum(sq) / divisor
    if wrong == "one_pass":
        s2 = np.zeros((rows, 64), F32)
        for i in range(vpl):
            s2 = _fma(v[:, i], v[:, i], s2)
        var = np.maximum(_wave_sum(s2) / F32(dim) - mean * mean, F32(0))  # clamped, as one-pass kernels do: no NaN to spot
    assert var.dtype == F32 and mean.dtype == F32
    if wrong == "eps_outside":
        rstd = (1.0 / (np.sqrt(np.maximum(var, 0).astype(F64)) + F64(F32(eps)))).astype(F32)
    else:
        rstd = (1.0 / np.sqrt((var + F32(eps)).astype(F64))).astype(F32)
    g = np.asarray(gamma, F32)
    if wrong == "gamma_by_lane":
        g = g[np.arange(dim) % 64]
    y = (h - mean) * rstd * g
    if wrong != "no_beta":
        y = y + np.asarray(beta, F32)
    assert y.dtype == F32
    return y


def _ln_cases():
    out = [("ordinary", dim) for dim in (1, 63, 64, 65, 384, 512, 513, 1280, 2048)]
    out += [(fam, dim) for fam in RO.LN_FAMILIES[1:] for dim in (384, 1280)]
    return out


LN_CASES = _ln_cases()
WRONG = {"one_pass": "large_mean", "unbiased": "ordinary", "eps_outside": "small", "no_beta": "ordinary",
         "gamma_by_lane": "ordinary"}


@pytest.fixture(scope="module")
def ln_ratios():
    """worst |emulation - y| / bound per (family, dim, source dtype, variant), computed once."""
    table = {}
    for fam, dim in LN_CASES:
        g, b = RO.ln_params(dim, 20 + dim)
        vpl = RO.ln_vpl(dim)
        for src in ("float32", "bfloat16"):
            h = RO.ln_inputs(fam, 37, dim, 7 + dim)
            if src == "bfloat16":
                h = synth.bf16_round(h)
            y, bound = RO.layernorm(h, g, b, 1e-5, vpl)
            assert np.isfinite(bound).all(), (fam, dim, src)
            for wrong in (None,) + tuple(WRONG):
                if wrong == "unbiased" and dim == 1:
                    continue
                got = emulate_ln(h, g, b, 1e-5, vpl, wrong)
                ratio = np.abs(got - y) / bound
                table[(fam, dim, src, wrong)] = float(np.where(np.isfinite(got), ratio, np.inf).max())
                if wrong is None:  # the bf16 destination's extra rounding
                    err16 = np.abs(synth.bf16_round(got).astype(F64) - y)
                    table[(fam, dim, src, "bf16_dst")] = float((err16 / RO.accept_bf16(y, bound)).max())
            table[(fam, dim, src, "tightness")] = float((bound / np.maximum(np.abs(y), 0.05)).max())
    return table


def test_faithful_emulation_stays_inside_the_bound(ln_ratios):
    worst = {}
    for (fam, dim, src, wrong), ratio in ln_ratios.items():
        if wrong in (None, "bf16_dst"):
            worst[fam] = max(worst.get(fam, 0.0), ratio)
            assert ratio <= 1.0, (fam, dim, src, wrong, ratio)
    print("faithful emulation, worst error / bound per family:", {k: round(v, 3) for k, v in worst.items()})


def test_the_bound_is_tight_on_well_conditioned_rows(ln_ratios):
    """bound / max(|y|, 0.05) on the families whose rows are well conditioned: (vpl + 6) u = 2.3e-6 of the mean's
    magnitude and about as much again through rstd, on outputs of up to 4 sigma: below 2e-4.  (Large-mean and constant
    rows are ill conditioned by construction: there the worst-case mean error times rstd is O(0.1) and the bound says so.)"""
    for (fam, dim, src, wrong), t in ln_ratios.items():
        if wrong == "tightness" and fam in ("ordinary", "outlier", "small") and dim > 1:
            assert t < 2e-4, (fam, dim, src, t)


@pytest.mark.parametrize("wrong", list(WRONG))
def test_wrong_variants_exceed_the_bound(ln_ratios, wrong):
    """Each mistake is caught by the family the module docstring of the oracle names for it, at both register counts
    (dims 384 and 1280; ``gamma_by_lane`` needs a dim above 64), from either source dtype.  (bf16 cannot hold
    1000 + 0.01 n: from a bf16 source the large-mean rows are constant rows, and the one-pass variance is judged on the
    float32 source alone.)"""
    fam = WRONG[wrong]
    seen = {k: v for k, v in ln_ratios.items() if k[3] == wrong}
    print(wrong, {f"{k[0]}-{k[1]}-{k[2]}": round(v, 2) for k, v in seen.items() if k[0] == fam})
    for dim in (384, 1280):
        for src in ("float32",) if wrong == "one_pass" else ("float32", "bfloat16"):
            assert seen[(fam, dim, src, wrong)] > 1.0, (wrong, fam, dim, src, seen[(fam, dim, src, wrong)])


# ---- decode_dense ------------------------------------------------------------------------------------------------------
def test_decode_dense_value_and_bound():
    D, H, B = 70, 130, 6
    w = synth.normal((H, D), 5, 1) * F32(0.1)
    bd, bp = synth.normal((D,), 5, 2) * F32(0.1), synth.normal((D,), 5, 3) * F32(0.1)
    hid = synth.normal((B, H), 5, 4)
    hid[np.abs(hid) < 0.8] = 0
    hid[0] = 0
    hid[1, 3] = F32(-0.0)
    recon, bound = RO.decode_dense(hid, w, bd, bp)
    slow = np.array([[float(bd[d]) + float(bp[d]) + sum(float(hid[r, j]) * float(w[j, d]) for j in range(H))
                      for d in range(D)] for r in range(B)])
    assert np.abs(recon - slow).max() < 1e-13
    assert np.abs(recon[0] - (bd.astype(F64) + bp.astype(F64))).max() == 0
    acc = np.broadcast_to(bd + bp, (B, D)).astype(F32)
    for j in range(H):  # the kernel's order: ascending feature, one fmaf each, zeros skipped (a zero term is exact anyway)
        acc = _fma(np.repeat(hid[:, j:j + 1], D, axis=1), np.repeat(w[j:j + 1], B, axis=0), acc)
    ratio = float((np.abs(acc - recon) / bound).max())
    print(f"decode_dense emulation: worst error / bound {ratio:.3f}")
    assert ratio <= 1.0
    j = int(np.argmax((hid != 0).sum(axis=0)))
    dropped = acc - hid[:, j:j + 1] * w[j:j + 1]  # one feature left out: far outside
    assert (np.abs(dropped - recon) / bound).max() > 1e3
