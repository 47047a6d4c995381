"""The weight-gradient contraction on the 2:4 sparse MFMA (``wgrad2s_kernel``) against a float64 contraction of the same
bf16 operands, through the C ABI alone.

The code is HAND-BUILT, so every case decides which 4-row groups hold one, two, three or four entries of a feature (three
and four go to the kernel's second 2:4 layer).  A case runs ``wsae_encode_topk`` (stages the batch), ``wsae_decode_loss``
on the hand-built code (leaves g and writes dpre) and then ``wsae_weight_grads`` or the two ``wsae_weight_grads_wire``
halves.  The operands of the contraction are read back: hidden = bf16(relu(vals)), dpre -> bf16(dpre) (the casts of the
sort), g -> bf16(g) (``wsae_last_residual_grad``; the decode launch stores bf16 of the same fp32 value), x as given.  b_pre is
zero, so dW_e is the contraction itself.

Bound (derived, not measured).  A bf16 x bf16 product is exact in fp32.  An output element is an fp32 sum of its non-zero
products, each added once (adding a zero product is exact), and the running sum is added once more per chunk (the MFMA's
sum into the accumulator) and per split-K slab (``grad_finish_kernel``).  Every addition rounds with relative error
2^-24 of a partial sum that is at most S = sum |terms|.  So
    |error| <= (n_terms + n_chunks + n_split) * 2^-24 * S,
held as error / ((n_terms + n_chunks + n_split) * 2^-24 * S) <= 1 for every element with S > 0 (elements with S = 0 must be
exactly 0).  n_terms counts, per matrix, the entries of the feature whose bf16 left value is not zero (an entry whose hidden
value is 0 after the ReLU is no term of dW_dT; its dpre is 0 too).  n_chunks = all chunks of the batch (an upper count: a
split walks its share).  n_split = the largest split-K the launch form can pick: 1 below 8 chunks (the library asks for 4
chunks per split), else 8 for both matrices in one launch and 16 for one matrix per launch.
db_e the same with terms = the bf16 dpre entries of a feature.  The dense route (``WSAE_WGRAD_SPARSE=0`` at context creation)
is held to the same bound.  Sparse and dense results are NOT asserted equal bit for bit: the probe
(profiles/wgrad2_sparse_probe.txt, part d) found 99.59 % of the elements equal, not all; the equal share is only noted.

The partial last tile is taken at H = 224: ``wsae_ctx_create`` accepts multiples of 32 only, so H = 200 cannot be run.
Partial column tile: the sparse kernel serves every D the MFMA decode launch serves above 256 (384, 768, 1280).  D = 1280 is
four column tiles, the last one 128 of 384 columns wide (the clamped DMA columns, the B fragments read from them, the
``d >= D`` guard of the non-interior epilogue, tn > 0); D = 768 is two full column tiles (tn > 0 on the interior epilogue).
D = 320 is NOT served by the MFMA decode launch, so the library contracts it on the K-contiguous route, which the switch
does not touch: ``switch_inert_d320`` only shows that the switch changes nothing there (both routes bit-equal); it does not
test the new kernel.

Measured on the MI355X (profiles/wgrad2_sparse_parity_notes.jsonl): the largest error is 0.32 of its bound (D = 1280, both
routes alike), 0.27 at D = 768; the sparse and the dense route agree bit for bit on 59 % .. 99.5 % of the matrix elements,
depending on the case, on every db_e element, and on everything at D = 320.
"""

from __future__ import annotations

import os

import numpy as np
import pytest
import torch

from oracle import synth

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TILE = 192  # features per workgroup tile of the contraction


def max_split(nchunks, form):
    """the largest split-K the launch form can pick (pick_nsplit: >= 4 chunks per split; 8 / 16 slab slots)"""
    return 1 if nchunks < 8 else (8 if form == "all" else 16)


# id -> (D, H, k, B, code kind, launch forms)
CASES = {
    "plain": (384, 384, 32, 192, "random", ("all", "parts")),
    "layers": (384, 384, 32, 192, "built", ("all", "parts")),
    "b200": (384, 384, 32, 200, "built", ("all",)),
    "h224": (384, 224, 32, 192, "built", ("all",)),  # partial last tile (32 of 192 features), the non-interior epilogue
    "d768": (768, 384, 32, 192, "built", ("all", "parts")),  # two column tiles: tn > 0
    "d1280": (1280, 384, 32, 192, "built", ("all", "parts")),  # four column tiles, the last one 128 of 384 columns
    "d1280_h224": (1280, 224, 32, 200, "built", ("all",)),  # partial column tile x partial feature tile x partial chunk
    "switch_inert_d320": (320, 384, 32, 192, "built", ("all",)),  # the K-contiguous route: not the new kernel (docstring)
    "k64": (384, 384, 64, 192, "built", ("all",)),
    "split": (384, 384, 32, 2048, "built", ("all",)),
    "bench": (384, 3072, 32, 16384, "built", ("all", "parts")),
}


def build_code(D, H, k, B, kind, seed=7):
    """idx int32 [B, k] (distinct per row), vals fp32 [B, k]: mixed magnitudes, one in ten <= 0 (hidden 0 after the ReLU)."""
    rng = np.random.default_rng(seed)
    nchunks = -(-B // 64)
    special = sorted({f for t0 in range(0, H, TILE) for f in (t0, t0 + 31, t0 + 32, t0 + 95, t0 + 96, t0 + 191) if f < H} | {H - 1})
    plain = np.array([f for f in range(H) if f not in set(special)])
    idx = np.stack([rng.choice(plain, size=k, replace=False) for _ in range(B)]).astype(np.int32)
    if kind == "built":
        # three and four entries of a group: every special feature (features 0, 31, 32, 95, 96, 191 of each tile, the last
        # feature of the last tile), in the first and the last group of the first chunk, of the last chunk of the first split
        # (chunk 7 where the batch has one) and of the last chunk
        used = np.zeros(B, dtype=np.int64)
        chunks = sorted({0, min(7, nchunks - 1), nchunks - 1})
        patterns = [(0, 1, 2, 3), (1, 2, 3), (0, 2, 3), (0, 1, 3), (0, 1, 2)]
        for i, f in enumerate(special):
            for c in chunks:
                rows_c = min(64, B - 64 * c)
                for gi, g in enumerate((0, (rows_c - 1) // 4)):
                    for r in patterns[(i + gi + c) % len(patterns)]:
                        row = 64 * c + 4 * g + r
                        if row < B and used[row] < k:
                            idx[row, used[row]] = f
                            used[row] += 1
        if nchunks >= 3:
            # chunk 1: all 64 x k entries in tile 0 (nothing for the other tiles; most groups hold three or four), and
            # feature 5 on all 64 rows
            lo, hi = 64, 128
            for row in range(lo, hi):
                others = rng.choice(np.array([f for f in range(min(TILE, H)) if f != 5]), size=k - 1, replace=False)
                idx[row] = np.concatenate([[5], others]).astype(np.int32)
    assert all(len(set(r.tolist())) == k for r in idx[: min(B, 256)])
    vals = (0.05 + rng.random((B, k))) * (2.0 ** rng.integers(-6, 7, size=(B, k)))
    vals[rng.random((B, k)) < 0.1] *= -1.0
    return idx, vals.astype(np.float32)


@pytest.fixture(scope="module")
def engines(device):
    from whisper_sae.sae.engine import SAEEngine
    from whisper_sae import _native as N
    cache = {}

    def get(D, H, k, B, sparse):
        key = (D, H, k, sparse)
        if key not in cache:
            eng = SAEEngine(device, D, H, k)
            w = synth.sae_weights(D, H, seed=3, bf16=True)
            for name, v in w.items():
                eng.view(name).copy_(torch.from_numpy(np.ascontiguousarray(v)).to(device))
            old = os.environ.get("WSAE_WGRAD_SPARSE")
            os.environ["WSAE_WGRAD_SPARSE"] = "1" if sparse else "0"  # read when the context is created
            try:
                eng.ctx(N.PREC_BF16, max(B, 16384 if H == 3072 else 2048))
            finally:
                if old is None:
                    del os.environ["WSAE_WGRAD_SPARSE"]
                else:
                    os.environ["WSAE_WGRAD_SPARSE"] = old
            cache[key] = eng
        return cache[key]

    yield get
    torch.cuda.synchronize()
    for eng in cache.values():
        for handle, _ in eng._ctx.values():
            eng.lib.wsae_ctx_set_fired(handle, 0)
        eng.close()


_inputs = {}


def inputs(device, cid):
    """Per case, once: the batch, the code and (after the first run) the float64 reference."""
    if cid not in _inputs:
        D, H, k, B, kind, _ = CASES[cid]
        idx, vals = build_code(D, H, k, B, kind)
        x = synth.activations(B, D, seed=11, stream=2, bf16=True)
        _inputs[cid] = dict(x=torch.from_numpy(x).to(device).to(torch.bfloat16), idx=torch.from_numpy(idx).to(device),
                            vals=torch.from_numpy(vals).to(device), ref=None)
    return _inputs[cid]


def contract(left, idx, right, H):
    """float64 [H, D] = sum over entries of left[b, j] * right[b, :] into row idx[b, j]; and the same of absolute values."""
    B, k = idx.shape
    D = right.shape[1]
    flat = idx.reshape(-1).long()
    l64 = left.double().reshape(-1, 1)
    r64 = right.double().repeat_interleave(k, dim=0)
    out = torch.zeros(H, D, dtype=torch.float64, device=idx.device).index_add_(0, flat, l64 * r64)
    mag = torch.zeros(H, D, dtype=torch.float64, device=idx.device).index_add_(0, flat, l64.abs() * r64.abs())
    return out, mag


def contract_big(left, idx, right, H, rows=2048):
    out = mag = None
    for b0 in range(0, idx.shape[0], rows):
        o, m = contract(left[b0:b0 + rows], idx[b0:b0 + rows], right[b0:b0 + rows], H)
        out = o if out is None else out + o
        mag = m if mag is None else mag + m
    return out, mag


def run(device, engines, cid, sparse, form):
    from whisper_sae import _native as N
    D, H, k, B, _, _ = CASES[cid]
    eng = engines(D, H, k, B, sparse)
    lib, st = eng.lib, eng.stream()
    inp = inputs(device, cid)
    x, idx, vals = inp["x"], inp["idx"], inp["vals"]
    handle = eng.prepare(N.PREC_BF16, B, force=True)
    pk = eng.pack.data_ptr()
    tv, ti = torch.empty_like(vals), torch.empty_like(idx)
    dpre = torch.empty_like(vals)
    N.check(lib.wsae_ctx_set_loss_cols(handle, D), "wsae_ctx_set_loss_cols")
    N.check(lib.wsae_encode_topk(handle, pk, x.data_ptr(), N.DT_BF16, 0, B, tv.data_ptr(), ti.data_ptr(), 0, eng.stats.data_ptr(), st),
            "wsae_encode_topk")
    N.check(lib.wsae_decode_loss(handle, pk, x.data_ptr(), N.DT_BF16, 0, vals.data_ptr(), idx.data_ptr(), B, 0, 3, dpre.data_ptr(),
                                 0, 0, eng.stats.data_ptr(), st), "wsae_decode_loss")
    g32 = torch.empty(B, D, dtype=torch.float32, device=device)
    N.check(lib.wsae_last_residual_grad(handle, B, g32.data_ptr(), st), "wsae_last_residual_grad")
    HD = H * D
    if form == "all":
        grads = torch.full((eng.P,), float("nan"), dtype=torch.float32, device=device)
        N.check(lib.wsae_weight_grads(handle, pk, x.data_ptr(), N.DT_BF16, 0, vals.data_ptr(), idx.data_ptr(), dpre.data_ptr(), B,
                                      grads.data_ptr(), st), "wsae_weight_grads")
        o = eng.off
        got = dict(dWe=grads[o[0]:o[0] + HD].view(H, D), dWdT=grads[o[1]:o[1] + HD].view(H, D), dbe=grads[o[2]:o[2] + H])
    else:
        fired = torch.zeros(H, dtype=torch.float32, device=device)
        wire = torch.full((eng.P + H + N.WIRE_METRIC_SLOTS,), float("nan"), dtype=torch.float32, device=device)
        N.check(lib.wsae_ctx_set_fired(handle, fired.data_ptr()), "wsae_ctx_set_fired")
        args = (handle, pk, x.data_ptr(), N.DT_BF16, 0, vals.data_ptr(), idx.data_ptr(), dpre.data_ptr(), B)
        N.check(lib.wsae_weight_grads_wire(*args, N.PART_DECODER, wire.data_ptr(), N.DT_F32, st), "wsae_weight_grads_wire")
        N.check(lib.wsae_weight_grads_wire(*args, N.PART_ENCODER, wire.data_ptr(), N.DT_F32, st), "wsae_weight_grads_wire")
        torch.cuda.synchronize()
        N.check(lib.wsae_ctx_set_fired(handle, 0), "wsae_ctx_set_fired")
        got = dict(dWdT=wire[:HD].view(H, D), dWe=wire[HD:2 * HD].view(H, D), dbe=wire[2 * HD:2 * HD + H])
    torch.cuda.synchronize()
    if inp["ref"] is None:
        hid = vals.clamp_min(0.0).to(torch.bfloat16)
        dp = dpre.to(torch.bfloat16)
        gb = g32.to(torch.bfloat16)
        wd, wd_mag = contract_big(hid, idx, gb, H)
        we, we_mag = contract_big(dp, idx, x, H)
        ones = torch.ones(B, 1, dtype=torch.bfloat16, device=device)
        be, be_mag = contract_big(dp, idx, ones, H)

        def terms(left):  # per feature: the entries whose bf16 left value is not zero
            return torch.zeros(H, dtype=torch.float64, device=device).index_add_(
                0, idx.reshape(-1).long(), (left.reshape(-1) != 0).double())

        n_hid, n_dp = terms(hid), terms(dp)
        inp["ref"] = dict(dWdT=(wd, wd_mag, n_hid), dWe=(we, we_mag, n_dp), dbe=(be[:, 0], be_mag[:, 0], n_dp), dpre=dpre.clone())
    else:
        assert torch.equal(dpre, inp["ref"]["dpre"]), "the decode launch wrote another dpre for the same inputs"
    return got


def worst(got, ref, mag, cnt, nchunks, nsplit):
    """max over elements of |error| / bound; elements with no term must be exactly zero."""
    n = (cnt + nchunks + nsplit).reshape(-1, *([1] * (ref.dim() - 1)))
    bound = n * U * mag
    err = (got.double() - ref).abs()
    assert torch.isfinite(got).all()
    assert bool((err[mag == 0] == 0).all()), "an element without any term is not zero"
    return float((err[mag > 0] / bound[mag > 0]).max())


def case_params():
    return [(cid, form) for cid, c in CASES.items() for form in c[5]]


@pytest.mark.parametrize("cid,form", case_params(), ids=[f"{c}-{f}" for c, f in case_params()])
def test_sparse_contraction_against_float64(device, engines, parity_note, cid, form):
    D, H, k, B, _, _ = CASES[cid]
    nchunks = -(-B // 64)
    got = run(device, engines, cid, True, form)
    keep = {n: v.clone() for n, v in got.items()}
    again = run(device, engines, cid, True, form)
    ref = _inputs[cid]["ref"]
    ratios = {n: worst(got[n], *ref[n], nchunks, max_split(nchunks, form)) for n in ("dWdT", "dWe", "dbe")}
    for n, r in ratios.items():
        parity_note(f"wgrad_sparse_{cid}_{form}_{n}_error_over_bound", r, 1.0)
    for n in keep:  # two launches on the same inputs: the same bits
        assert torch.equal(keep[n].view(torch.int32), again[n].view(torch.int32)), f"{n}: two launches differ"
    for n, r in ratios.items():
        assert r <= 1.0, f"{cid}/{form}/{n}: error is {r:.3f} of the derived bound"


@pytest.mark.parametrize("cid,form", case_params(), ids=[f"{c}-{f}" for c, f in case_params()])
def test_dense_route_same_bound(device, engines, parity_note, cid, form):
    D, H, k, B, _, _ = CASES[cid]
    nchunks = -(-B // 64)
    sparse = {n: v.clone() for n, v in run(device, engines, cid, True, form).items()}
    dense = run(device, engines, cid, False, form)
    ref = _inputs[cid]["ref"]
    for n in ("dWdT", "dWe", "dbe"):
        r = worst(dense[n], *ref[n], nchunks, max_split(nchunks, form))
        same = float((dense[n].view(torch.int32) == sparse[n].view(torch.int32)).double().mean())
        parity_note(f"wgrad_dense_{cid}_{form}_{n}_error_over_bound", r, 1.0)
        parity_note(f"wgrad_sparse_equals_dense_{cid}_{form}_{n}_share", same, 0.0)
        assert r <= 1.0, f"{cid}/{form}/{n}: the dense route's error is {r:.3f} of the derived bound"
        if cid.startswith("switch_inert"):  # the K-contiguous route runs whatever the switch says
            assert same == 1.0, f"{cid}/{n}: the switch changed a route it does not serve"
