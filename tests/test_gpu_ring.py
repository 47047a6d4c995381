"""Exact and float64 parity of ``wsae_ring.hip``: the path from a tensor or a hooked layer into the on-device ring, the
shuffle that draws from it, and the dense-code decode.  The reference is tests/ring_oracle.py (numpy, float64 / integer).

Pinned bit for bit: slot placement and the counters of ``push`` / ``push_layernorm`` (wrap-around, oversized pushes, the
grid-stride loop), all four dtype conversions, every value ``ring.sample`` returns.  Checked by a DERIVED element-wise
bound (the oracle's module docstring; tests/test_ring_oracle.py shows it separates the kernel from five plausible
mistakes): the row LayerNorm of ``push_layernorm`` and ``wsae_layernorm_rows``, and ``decode_dense``.  The measured
worst error / bound of every float comparison goes to ``parity_notes.jsonl``.

Measured on the MI355X (profiles/ring_parity_notes.jsonl), worst error as a fraction of its bound.  LayerNorm to a
float32 destination: 0.60 from either source dtype (the ``small`` rows, where the bound is little more than the final
add's own rounding); by family: ordinary 0.10, outlier 0.33, large_mean 0.12, small 0.60, constant 0.13.  To a bf16
destination 0.9999: the half-ulp of the final conversion is most of that allowance, so a ratio near 1 is what a correct
kernel gives.  The push script: 0.09 (float32 ring), 0.999 (bf16 ring).  ``decode_dense``: 0.42, 0.51, 0.49.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

import ring_oracle as RO
from oracle import synth

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
TORCH_DT = {"float32": torch.float32, "bfloat16": torch.bfloat16}
PAIRS = [(s, d) for s in ("float32", "bfloat16") for d in ("float32", "bfloat16")]
EPS = 1e-5


def native():
    from whisper_sae import _native as N
    return N


def new_ring(device, capacity, dim, dtype):
    from whisper_sae.data.feature_cache import ActivationRing
    return ActivationRing(capacity, dim, device=device, dtype=TORCH_DT[dtype])


def as_source(a: np.ndarray, dtype: str) -> np.ndarray:
    """The float32 values a source tensor of ``dtype`` holds."""
    a = np.ascontiguousarray(a, F32)
    return synth.bf16_round(a) if dtype == "bfloat16" else a


def to_device(a: np.ndarray, dtype: str, device) -> torch.Tensor:
    """``a`` (already representable in ``dtype``) as a device tensor of that dtype: the cast is exact."""
    return torch.from_numpy(np.ascontiguousarray(a, F32)).to(device).to(TORCH_DT[dtype])


def storage(ring) -> np.ndarray:
    """The ring's whole storage as float32 values (bf16 widens exactly)."""
    torch.cuda.synchronize()
    return ring.data.float().cpu().numpy()


def bits32(a) -> np.ndarray:
    return np.ascontiguousarray(a, F32).view(np.int32)


def sentinel_rows(capacity: int, dim: int) -> np.ndarray:
    """-(256 + 2 slot) in every column: distinct per slot for capacity <= 128, exact in float32 and in bf16."""
    return np.repeat(-(256.0 + 2.0 * np.arange(capacity, dtype=F32))[:, None], dim, axis=1).astype(F32)


def poke(ring, model: RO.RingModel) -> None:
    """Write the sentinel through the ``ring.data`` view and into the model."""
    model.poke(sentinel_rows(model.capacity, model.dim))
    ring.data.copy_(torch.from_numpy(model.data.astype(F32)).to(ring.data.device).to(ring.data.dtype))
    torch.cuda.synchronize()


def worst_ratio(got, want, bound) -> float:
    assert np.isfinite(got).all()
    return float((np.abs(np.asarray(got, F64) - want) / bound).max()) if got.size else 0.0


# ---- push bookkeeping --------------------------------------------------------------------------------------------------
CAP, DIM = 100, 64
SCRIPT = [("push", 70), ("push", 60), ("push", 0), ("push", 250), ("push", 100), ("fill", 40), ("push", 30)]


@pytest.mark.parametrize("src,dst", PAIRS, ids=[f"{s}-{d}" for s, d in PAIRS])
def test_push_bookkeeping_is_exact(device, src, dst):
    """70, 60 (wraps), 0, 250 (oversized, head = 30), 100 (the capacity), ``fill_synthetic(40)``, 30 rows into a ring of 100:
    after every step the WHOLE storage and ``len(ring)`` equal the host model, bit for bit; the slots never written hold
    the sentinel until the first wrap.

    Catches: ``head`` advanced by the capped instead of the full row count of an oversized push, or its source pointer
    moved by the wrong element size (bf16 sources); ``% cap`` applied to the element and not to the row; a push that
    touches a slot outside its range; ``size`` that keeps growing past the capacity."""
    ring, model = new_ring(device, CAP, DIM, dst), RO.RingModel(CAP, DIM, dst)
    poke(ring, model)
    for step, (op, n) in enumerate(SCRIPT):
        if op == "fill":
            ring.fill_synthetic(n, seed=5)
            model.fill(n, seed=5)
        else:
            rows = as_source(synth.normal((n, DIM), 60 + step, 1) * F32(1.5), src)
            ring.push(to_device(rows, src, device).reshape(n, DIM))
            model.push(rows)
        got = storage(ring)
        assert np.array_equal(bits32(got), bits32(model.data.astype(F32))), (step, op, n)
        assert len(ring) == model.size, (step, op, n)
        if step == 0:
            assert np.array_equal(got[70:], sentinel_rows(CAP, DIM)[70:]) and model.head == 70
    assert (model.head, model.size) == (70, 70)
    ring.close()


@pytest.mark.parametrize("src,dst", PAIRS, ids=[f"{s}-{d}" for s, d in PAIRS])
def test_layernorm_push_bookkeeping(device, parity_note, src, dst):
    """The same script through ``push_layernorm``: which slot every row lands in is exact (slots the script did not
    write, or wrote by ``fill_synthetic``, are compared bit for bit; the rows differ from one another by O(1), the bound
    is ~1e-6), the values are held to the oracle's bound, ``len(ring)`` to the model.

    Catches: the oversized path of the LayerNorm push (a copy of the plain one: skip, head, source pointer); a wave that
    normalises row r but stores to the slot of another; rows of the last, partly filled block of four dropped."""
    ring, ym = new_ring(device, CAP, DIM, dst), RO.RingModel(CAP, DIM, dst)
    poke(ring, ym)
    bound = np.zeros((CAP, DIM), F64)  # 0: the slot holds a value the oracle knows exactly
    gamma, beta = RO.ln_params(DIM, 3)
    g_t, b_t = torch.from_numpy(gamma).to(device), torch.from_numpy(beta).to(device)
    worst = 0.0
    for step, (op, n) in enumerate(SCRIPT):
        if op == "fill":
            ring.fill_synthetic(n, seed=5)
            ym.fill(n, seed=5)
            bound[:n] = 0
        else:
            rows = as_source(RO.ln_inputs("ordinary", n, DIM, 80 + step), src).reshape(n, DIM)
            ring.push_layernorm(to_device(rows, src, device).reshape(n, DIM), g_t, b_t, EPS)
            y, bd = RO.layernorm(rows, gamma, beta, EPS, RO.ln_vpl(DIM)) if n else (np.zeros((0, DIM)), np.zeros((0, DIM)))
            slots = ym.push(y, exact=True)
            bound[slots[slots >= 0]] = bd[slots >= 0]
        got = storage(ring)
        assert len(ring) == ym.size, (step, op, n)
        exact = bound == 0
        assert np.array_equal(bits32(got[exact]), bits32(ym.data[exact].astype(F32))), (step, op, n)
        allowed = RO.accept_bf16(ym.data, bound) if dst == "bfloat16" else bound
        ratio = worst_ratio(got[~exact], ym.data[~exact], allowed[~exact])
        worst = max(worst, ratio)
        assert ratio <= 1.0, (step, op, n, ratio)
        if step == 0:
            assert exact[70:].all() and not exact[:70].any()
    print(f"[ring] push_layernorm script {src} -> {dst}: worst error / bound {worst:.3f}")
    parity_note(f"ring_ln_script_{src}_{dst}_over_bound", worst, 1.0)
    ring.close()


# ---- push conversions --------------------------------------------------------------------------------------------------
def conversion_values(n_rows: int, dim: int) -> np.ndarray:
    """Normal finite float32 values: exact bf16 ties in both directions and their neighbours, signed zeros, the ends of
    the range, and magnitudes across 40 decades.  (Subnormals stay out: their conversion is pinned nowhere.)"""
    e8, e23 = 2.0 ** -8, 2.0 ** -23
    special = [1 + e8, 1 + 3 * e8, 1 + 5 * e8, 1 + e8 + e23, 1 + e8 - e23, 1 + 3 * e8 + e23, 1 + 3 * e8 - e23, 1.0, 1 + 2 * e8,
               0.0, 3.0e38, 3.3e38, 1e30, 2.0 ** 127, 2.0 ** -126, 1.5 * 2.0 ** -126, 1e-30, 255.5, 256.5, 257.5, 65535.0]
    special = np.array(special + [-x for x in special], F32)
    total = n_rows * dim
    mant = synth.normal((total,), 91, 1)
    mant[mant == 0] = 1
    decade = np.floor(synth.uniform((total,), 91, 2, -35.0, 36.0)).astype(F64)
    vals = (mant.astype(F64) * 10.0 ** decade).astype(F32)
    vals[np.abs(vals) < 2.0 ** -125] = F32(0.75)
    vals[:special.size] = special
    assert np.isfinite(vals).all() and np.isfinite(synth.bf16_round(vals)).all()
    assert ((vals == 0) | (np.abs(vals) >= 2.0 ** -126)).all()
    return vals.reshape(n_rows, dim)


@pytest.mark.parametrize("src,dst", PAIRS, ids=[f"{s}-{d}" for s, d in PAIRS])
def test_push_conversions_are_exact(device, src, dst):
    """float32 -> bf16 is ``synth.bf16_round`` bit for bit (ties to even both ways, signed zeros, large magnitudes),
    bf16 -> float32 widens exactly, equal dtypes copy bits.

    Catches: truncation instead of rounding, ties away from zero, a lost sign of zero, the wrong template instance
    behind a dtype pair (a bf16 source read as float32 or the reverse)."""
    rows, dim = 40, 33
    vals = as_source(conversion_values(rows, dim), src)
    ring = new_ring(device, rows + 2, dim, dst)
    ring.data.fill_(-7.0)
    ring.push(to_device(vals, src, device))
    torch.cuda.synchronize()
    if dst == "bfloat16":
        got = ring.data[:rows].view(torch.int16).cpu().numpy().view(np.uint16)
        assert np.array_equal(got, synth.bf16_bits(vals))
        if src == "float32":  # the ties really are in there and went to even
            assert got[0, 0] == 0x3F80 and got[0, 1] == 0x3F82
    else:
        assert np.array_equal(bits32(ring.data[:rows].cpu().numpy()), bits32(vals))
    assert (ring.data[rows:].float() == -7.0).all() and len(ring) == rows
    ring.close()


def test_push_larger_than_one_grid_pass(device):
    """4100 x 384 float32 rows into a bf16 ring whose head stands at 5: 1 574 400 elements against 4096 x 256 threads, so
    the grid-stride loop takes a second pass, and the push wraps.  Compared in full, bit for bit.

    Catches: a stride of the block count instead of the thread count, an int32 element index, a second pass that
    starts from the wrong element."""
    cap, dim = 4100, 384
    ring, model = new_ring(device, cap, dim, "bfloat16"), RO.RingModel(cap, dim, "bfloat16")
    first = synth.normal((5, dim), 70, 1)
    rows = synth.normal((cap, dim), 71, 1) * F32(2.5)
    for part in (first, rows):
        ring.push(torch.from_numpy(part).to(device))
        model.push(part)
    assert len(ring) == model.size == cap and model.head == 5
    got = ring.data.view(torch.int16).cpu().numpy().view(np.uint16)
    assert np.array_equal(got, synth.bf16_bits(model.data.astype(F32)))
    ring.close()


# ---- LayerNorm numerics ------------------------------------------------------------------------------------------------
LN_CASES = [("ordinary", d) for d in (1, 63, 64, 65, 384, 512, 513, 1280, 2048)]
LN_CASES += [(fam, d) for fam in RO.LN_FAMILIES[1:] for d in (384, 1280)]


def layernorm_rows(h_t, gamma_t, beta_t, eps, dst_t, n_rows, dim):
    N = native()
    code = lambda t: N.DT_BF16 if t.dtype == torch.bfloat16 else N.DT_F32  # noqa: E731
    return N.lib().wsae_layernorm_rows(h_t.data_ptr(), code(h_t), n_rows, dim, gamma_t.data_ptr(), beta_t.data_ptr(), eps,
                                       dst_t.data_ptr(), code(dst_t), torch.cuda.current_stream(h_t.device).cuda_stream)


@pytest.mark.parametrize("family,dim", LN_CASES, ids=[f"{f}-{d}" for f, d in LN_CASES])
def test_layernorm_matches_float64(device, parity_note, family, dim):
    """Every element of ``push_layernorm`` and of ``wsae_layernorm_rows`` within the oracle's bound of the float64
    LayerNorm: 1, 5 and 37 rows, both source and both destination dtypes; the two entry points give the same bits; the
    slots and the guard row behind the rows stay untouched.

    Catches (tests/test_ring_oracle.py: each leaves the bound on the family named): a one-pass variance (large_mean), a
    division by dim - 1 (ordinary), eps outside the root (small), a dropped beta, gamma indexed by the lane; a wrong
    register count at 512 -> 513 or a column dropped at 2048; lanes beyond dim counted into the statistics (1, 63, 65)."""
    N = native()
    gamma, beta = RO.ln_params(dim, 20 + dim)
    g_t, b_t = torch.from_numpy(gamma).to(device), torch.from_numpy(beta).to(device)
    worst = {}
    for src in ("float32", "bfloat16"):
        for rows in (1, 5, 37):
            h = as_source(RO.ln_inputs(family, rows, dim, 7 + dim + rows), src)
            y, bound = RO.layernorm(h, gamma, beta, EPS, RO.ln_vpl(dim))
            assert np.isfinite(bound).all()
            h_t = to_device(h, src, device)
            for dst in ("float32", "bfloat16"):
                ring = new_ring(device, rows + 3, dim, dst)
                ring.data.fill_(-7.0)
                ring.push_layernorm(h_t, g_t, b_t, EPS)
                plain = torch.full((rows + 1, dim), -7.0, dtype=TORCH_DT[dst], device=device)
                N.check(layernorm_rows(h_t, g_t, b_t, EPS, plain, rows, dim), "wsae_layernorm_rows")
                torch.cuda.synchronize()
                assert len(ring) == rows
                assert (ring.data[rows:].float() == -7.0).all() and (plain[rows:].float() == -7.0).all()
                assert torch.equal(ring.data[:rows].float().view(torch.int32), plain[:rows].float().view(torch.int32))
                got = plain[:rows].float().cpu().numpy()
                allowed = RO.accept_bf16(y, bound) if dst == "bfloat16" else bound
                ratio = worst_ratio(got, y, allowed)
                worst[(src, dst)] = max(worst.get((src, dst), 0.0), ratio)
                assert ratio <= 1.0, (family, dim, src, dst, rows, ratio)
                if family == "constant" and dst == "float32":  # the output is beta, within the bound
                    assert (np.abs(got - beta.astype(F64)) <= bound).all()
                ring.close()
    for (src, dst), ratio in worst.items():
        parity_note(f"ring_ln_{family}_{dim}_{src}_{dst}_over_bound", ratio, 1.0)
    print(f"[ring] layernorm {family} dim {dim}: worst error / bound " + ", ".join(f"{s[:2]}->{d[:2]} {r:.3f}" for (s, d), r in worst.items()))


def test_layernorm_rejects_rows_wider_than_2048(device):
    """dim 2049: both entry points return WSAE_ERR_INVALID before any launch and write nothing.
    Catches: a limit that lets a row wider than 64 lanes x 32 registers through (its tail would be dropped silently)."""
    N = native()
    dim, rows = 2049, 3
    h_t = torch.from_numpy(RO.ln_inputs("ordinary", rows, dim, 1)).to(device)
    g_t, b_t = torch.ones(dim, device=device), torch.zeros(dim, device=device)
    ring = new_ring(device, 4, dim, "float32")
    ring.data.fill_(-7.0)
    stream = torch.cuda.current_stream(device).cuda_stream
    rc = N.lib().wsae_ring_push_layernorm(ring._h, h_t.data_ptr(), N.DT_F32, rows, g_t.data_ptr(), b_t.data_ptr(), EPS, stream)
    assert rc == -1 and "2048" in N.last_error()  # WSAE_ERR_INVALID
    with pytest.raises(N.WsaeError):
        ring.push_layernorm(h_t, g_t, b_t, EPS)
    plain = torch.full((rows, dim), -7.0, device=device)
    assert layernorm_rows(h_t, g_t, b_t, EPS, plain, rows, dim) == -1 and "2048" in N.last_error()
    torch.cuda.synchronize()
    assert len(ring) == 0 and (ring.data == -7.0).all() and (plain == -7.0).all()
    ring.close()


# ---- sample ------------------------------------------------------------------------------------------------------------
SEEDS, EPOCHS = (42, (1 << 63) + 5), (0, 1, 1 << 40)


def filled_ring(device, capacity, n_rows):
    ring = new_ring(device, capacity, 1, "float32")
    ring.fill_synthetic(n_rows, seed=1)
    return ring


@pytest.mark.parametrize("size", [1, 2, 3, 4, 5, 1000, 1024, 1025, 70001])
def test_sample_equals_the_feistel_oracle(device, size):
    """``ring.sample`` element for element: 300 positions (no multiple of 256; more than the ring holds at the small
    sizes) from offset 0 and from seven before the end (wraps), epochs 0, 1 and 2^40, seeds 42 and 2^63 + 5; the whole
    permutation once.  70001 rows carry indices above 65535.

    Catches: a domain one bit short at a power of two (1024) or wide at its successor (1025), ``half_bits`` rounded down, a
    degenerate domain at sizes 1 and 2, the epoch multiplied in 32 bits, a seed passed as a signed word, a cycle walk
    that stops after one step, ``offset + i`` not reduced modulo the size."""
    ring = filled_ring(device, size, size)
    assert len(ring) == size
    for seed in SEEDS:
        for epoch in EPOCHS:
            for offset in (0, max(0, size - 7)):
                got = ring.sample(300, seed, epoch, offset).cpu().numpy()
                assert got.dtype == np.int32
                assert np.array_equal(got.astype(np.int64), RO.feistel_rows(size, seed, epoch, offset, 300)), (seed, epoch, offset)
    whole = ring.sample(size, 42, 0, 0).cpu().numpy().astype(np.int64)
    assert np.array_equal(whole, RO.feistel_rows(size, 42, 0, 0, size))
    assert np.array_equal(np.sort(whole), np.arange(size))
    ring.close()


def test_sample_of_a_partly_filled_ring(device):
    """37 rows in a ring of 64: the permutation is over the 37 rows present, never over the capacity.
    Catches: the domain sized from the capacity (indices of rows that were never written)."""
    ring = filled_ring(device, 64, 37)
    assert len(ring) == 37
    for seed in SEEDS:
        got = ring.sample(101, seed, 3, 30).cpu().numpy().astype(np.int64)
        assert (got < 37).all() and (got >= 0).all()
        assert np.array_equal(got, RO.feistel_rows(37, seed, 3, 30, 101))
    ring.close()


def test_sample_of_a_million_rows(device):
    """2^20 + 1 rows (x 1 float): a 22-bit domain, most of it outside the ring, so nearly every index is cycle-walked.
    Windows of 4096 at offset 0 and across the end.  Catches: a walk or a left half truncated to 16 bits."""
    size = (1 << 20) + 1
    ring = filled_ring(device, size, size)
    for seed, epoch, offset in ((42, 0, 0), (42, 1 << 40, size - 1000), ((1 << 63) + 5, 1, size - 4095)):
        got = ring.sample(4096, seed, epoch, offset).cpu().numpy().astype(np.int64)
        assert got.max() > (1 << 16) and got.max() < size
        assert np.array_equal(got, RO.feistel_rows(size, seed, epoch, offset, 4096)), (seed, epoch, offset)
    ring.close()


# ---- decode_dense ------------------------------------------------------------------------------------------------------
def code_rows(B: int, H: int, seed: int) -> np.ndarray:
    """Dense codes [B, H]: signed entries, exact +0 and -0, row 0 all zero, row 1 fully dense, row 2 with its only
    non-zero in the last feature (the ragged last 64-feature group when H % 64 != 0)."""
    hid = synth.normal((B, H), seed, 1)
    keep = synth.uniform((B, H), seed, 2, 0.0, 1.0) < 0.3
    hid = np.where(keep, hid, F32(0)).astype(F32)
    hid[3:, 1::7] = F32(-0.0)
    hid[0] = 0
    dense = synth.normal((H,), seed, 3)
    dense[dense == 0] = 1
    hid[1] = dense
    hid[2] = 0
    hid[2, H - 1] = F32(-1.75)
    assert (hid[1] != 0).all() and (hid[3:] > 0).any() and (hid[3:] < 0).any() and np.signbit(hid[hid == 0]).any()
    return hid


@pytest.mark.parametrize("D,H,B", [(32, 96, 5), (544, 96, 5), (384, 3072, 9)])
def test_decode_dense_matches_float64(device, parity_note, D, H, B):
    """``decode_dense`` per element against float64 within (n_terms + 2) u (|b_d| + |b_pre| + sum |h_j| |W_dT[j, d]|),
    weights fed through the module.  D = 32 leaves half the wave idle, D = 544 needs the second pass of the 512-column
    loop, H = 96 ends in a ragged 64-feature group, B = 5 and 9 leave the last block of four partly filled.

    Catches: a second pass that starts from the wrong column or keeps the first pass's accumulators; features of the
    ragged group read past H or skipped; a -0 entry treated as a term; b_pre left out; rows of the last block dropped."""
    from whisper_sae.sae.model import TopKSAE
    w = synth.sae_weights(D, H, seed=7 + D, bf16=False, b_pre_scale=0.1)
    m = TopKSAE(D, H, k=8, precision="fp32")
    sd = m.state_dict()
    for key in ("encoder.weight", "encoder.bias", "decoder.weight", "decoder.bias", "b_pre"):
        sd[key] = torch.from_numpy(w[key])
    m.load_state_dict(sd)
    m.to(device)
    assert np.count_nonzero(w["decoder.bias"]) > D // 2 and np.count_nonzero(w["b_pre"]) > D // 2
    hid = code_rows(B, H, 40 + D)
    got = m.decode(torch.from_numpy(hid).to(device)).cpu().numpy()
    assert got.shape == (B, D)
    recon, bound = RO.decode_dense(hid, w["decoder.weight"].T, w["decoder.bias"], w["b_pre"])
    ratio = worst_ratio(got, recon, bound)
    print(f"[ring] decode_dense {D}x{H}x{B}: worst error / bound {ratio:.3f}")
    parity_note(f"decode_dense_{D}x{H}x{B}_over_bound", ratio, 1.0)
    assert ratio <= 1.0, (D, H, B, ratio)
    bias = (w["decoder.bias"].astype(F64) + w["b_pre"].astype(F64))
    assert (np.abs(got[0] - bias) <= 2 * RO.U * (np.abs(w["decoder.bias"]) + np.abs(w["b_pre"])) + RO.FLOOR).all()
