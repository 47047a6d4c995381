"""Stage-wise float64 parity of the ReLU + L1 step, every route of ``wsae_relu.hip`` / ``wsae_gemm256x.hip``, through the
C ABI alone (``wsae_ctx_reserve_relu``, ``wsae_relu_forward``, ``wsae_relu_backward`` on an ``SAEEngine`` rig).

The reference and every bound are tests/relu_oracle.py: each stage is compared with float64 computed from the device's
own output of the stage before it, so a failure names the stage, and the bounds are DERIVED (the rounding points and the
counts are in that module's docstring; tests/test_relu_oracle.py shows that an fp32 emulation stays inside them and that
ten plausible faults do not).  Per case, element by element: hidden (a), recon (c), loss / sparsity / l0 (d), db_d (e),
db_e (f), dW_e and dW_d^T (g); the device's activity mask may differ from the reference's only on the unsure set (b),
which may hold at most 1e-3 of the elements.  ``hidden``, ``recon`` and the gradient pack sit between sentinel guards.

Which kernels each case launches is on record in profiles/relu_step_trace.txt (one kernel-trace run of this file); the
measured error / bound ratios in profiles/relu_step_parity_notes.jsonl.  The smallest batch at which ``pick_nsplit``
returns more than 1 for 384 x 768 on 256 CUs is B = 512 (8 tiles, 8 chunks of 64 rows: cost 152 unsplit, 112 at 2, and a
split of 3 would leave fewer than 4 chunks per range): it chooses 2.

``backward_x`` with ``relu_g_B != B``.  Only ``decode_launch`` (``wsae_decode_loss``, ``wsae_encode_decode``) clears
``relu_g_B`` and leaves ``relu_x_B``.  ``wsae_decode_loss`` writes ctx->gb and the db_d partials and nothing else the
backward reads (xb, the workspace's bf16 hidden and the activity bits are untouched), so the rebuild from ``recon`` is
reachable and valid: ``test_backward_rebuilds_g_after_a_decode`` holds it to the same bounds and to bit-equality with
the direct backward.

Measured on the MI355X (profiles/relu_step_parity_notes.jsonl), worst error / bound per stage over all 48 tests: hidden
0.034, recon 0.015, loss 0.064, sparsity 0.034, l0 0.70, db_d 0.016, db_e 0.002, dW_d^T 0.027, dW_e 0.89; the largest unsure
share is 2.9e-4 (384 x 768 at B = 384) and no activity bit outside the unsure set differs.  Two figures are above 0.5 and both
are what a single rounding looks like, not a bound cut to fit.  l0 is ONE correctly rounded division of an exact count: its
error is anywhere in [0, u] (0.69 .. 0.70 on four cases).  dW_e reaches 0.5 .. 0.89 on seven cases, always on an entry whose bound is 93 .. 99% dpre
allowance (``dW_e_worst_allowance_part`` in the notes): there one dpre sat within its dh bound of a bf16 rounding boundary,
the device took the other candidate, and the entry moved by ulp |x| - exactly the allowance.  Where no dpre flipped the
ratio is 0.002 .. 0.2.  The two 1024-feature rows (384 x 1024 and 512 x 1024 at B = 256) enter the element-wise epilogue of
``wgrad2d_kernel``, which the 384 x 768 cases never do (every tile of theirs is interior): unsure shares 2.7e-4 and 4.4e-4, dW_d^T
at most 0.008, dW_e 0.11 .. 0.50.  No kernel fault was found; ``bias_sq_kernel`` had no launch left anywhere and was removed.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

import relu_oracle as RO
from oracle import synth

pytestmark = pytest.mark.gpu

WEIGHT = 0.05
GUARD = 64
DEAD = 3  # planted: zero encoder row and zero bias, pre == 0 exactly (a mask taken from pre >= 0 would count it active)
UNSURE_CAP = 1e-3
TENSORS = ("hidden", "recon", "loss", "l0", "sparsity", "db_d", "db_e", "dW_e", "dW_dT")

# (precision, D, H, B, flow, what it enters); the kernels are listed per case id in profiles/relu_step_trace.txt
CASES = [
    ("bf16", 96, 352, 200, "general", "simple gemm_nt_kernel everywhere, nz = 1, ragged 64-row and 128-column tiles"),
    ("bf16", 96, 352, 1000, "general", "ldT = 1024: nz = 2 on the simple kernel (H < 512 keeps gemm256d out)"),
    ("bf16", 96, 352, 1100, "general", "ldT = 1152: the split whose ranges are not slab pairs"),
    ("bf16", 128, 512, 520, "general", "ragged: encode_gemm256d_kernel for the decoder GEMM, dh and both contractions"),
    ("bf16", 128, 512, 1000, "general", "the gemm256d split ns = 2"),
    ("bf16", 128, 512, 1100, "general", "the fallback from nz = 2 to ns = 1"),
    ("fp32", 96, 352, 200, "general", "forward_t<float> / backward_t<float>"),
    ("fp32", 128, 512, 1000, "general", "forward_t<float> / backward_t<float>, KT = 32"),
    ("bf16", 128, 256, 256, "xgemm", "two gemm256x contractions + slab_sum8_kernel, x_split = 1"),
    ("bf16", 128, 256, 384, "xgemm", "a partly filled 256-row tile"),
    ("bf16", 128, 256, 1024, "xgemm", "x_split = 2"),
    ("bf16", 128, 256, 4096, "xgemm", "x_split = 8"),
    ("bf16", 256, 512, 2048, "xgemm", "x_split = 4"),
    ("bf16", 384, 768, 256, "xgemm", "wsae_internal_relu_wgrad, nsplit = 1"),
    ("bf16", 384, 768, 384, "xgemm", "wsae_internal_relu_wgrad, a partly filled 256-row tile"),
    ("bf16", 384, 768, 512, "xgemm", "wsae_internal_relu_wgrad: the smallest B at which pick_nsplit splits (it picks 2)"),
    ("bf16", 384, 1024, 256, "xgemm", "wsae_internal_relu_wgrad, nsplit = 1: partial last feature tile (64 of 192), interior "
                                      "columns - the epilogue's element-wise stores"),
    ("bf16", 512, 1024, 256, "xgemm", "wsae_internal_relu_wgrad, nsplit = 1: partial column tile (128 of 384) x partial feature tile"),
]
MAXB = {}
for _c in CASES:
    MAXB[(_c[1], _c[2])] = max(MAXB.get((_c[1], _c[2]), 0), _c[3])


def case_id(c):
    return f"{c[0]}-{c[1]}x{c[2]}-B{c[3]}"


# ---- rig ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rigs(device):
    from whisper_sae.sae.engine import SAEEngine
    cache = {}

    def get(D, H):
        if (D, H) not in cache:
            cache[(D, H)] = SAEEngine(device, D, H, 8)
        return cache[(D, H)]

    yield get
    torch.cuda.synchronize()
    for eng in cache.values():
        eng.close()


class Guarded:
    """A float32 device buffer with GUARD sentinel floats on either side; ``ptr`` is the address of the payload."""

    def __init__(self, device, n: int, tag: int):
        host = np.full(n + 2 * GUARD, 777.0, np.float32)
        self.sentinel = (np.arange(2 * GUARD, dtype=np.float32) + np.float32(1000.25 * (tag + 1))) * np.float32(-1.0)
        host[:GUARD], host[GUARD + n:] = self.sentinel[:GUARD], self.sentinel[GUARD:]
        self.n = n
        self.t = torch.from_numpy(host).to(device)
        self.ptr = self.t.data_ptr() + 4 * GUARD

    def payload(self) -> np.ndarray:
        return self.t[GUARD:GUARD + self.n].cpu().numpy()

    def sentinels_intact(self) -> bool:
        host = self.t.cpu().numpy()
        got = np.concatenate([host[:GUARD], host[GUARD + self.n:]])
        return bool(np.array_equal(got.view(np.int32), self.sentinel.view(np.int32)))


def make_problem(D, H, B, x_dtype, with_rows=False, with_l1w=False, half_cols=False):
    w = synth.sae_weights(D, H, seed=D + H, bf16=False)
    W_e, b_e = w["encoder.weight"].copy(), w["encoder.bias"].copy()
    W_e[DEAD], b_e[DEAD] = 0, 0
    n_src = 2 * B + 5 if with_rows else B
    x = synth.activations(n_src, D, seed=D + H + 1, stream=B % 97, bf16=(x_dtype == "bf16"))
    rows = None
    if with_rows:  # descending through a source with more rows than B, one index repeated
        rows = ((n_src - 1 - (np.arange(B) * 3) % n_src) % n_src).astype(np.int32)
        rows[5] = rows[4]
    l1w = synth.uniform((H,), D + H, 21, 0.5, 1.5) if with_l1w else None
    return dict(D=D, H=H, B=B, x_dtype=x_dtype, W_e=W_e, W_dT=np.ascontiguousarray(w["decoder.weight"].T), b_e=b_e,
                b_d=w["decoder.bias"], x=x, rows=rows, weight=WEIGHT, l1w=l1w, loss_cols=D // 2 if half_cols else D)


class Step:
    """One problem on the device: the pack, x, rows, and the calls."""

    def __init__(self, eng, device, p, prec):
        from whisper_sae import _native as N
        self.N, self.eng, self.device, self.p, self.prec = N, eng, device, p, prec
        D, H = p["D"], p["H"]
        self.handle = eng.ctx(N.PREC_BF16 if prec == "bf16" else N.PREC_FP32, MAXB[(D, H)])
        eng.reserve_relu(self.handle)
        self.total, self.off = N.pack_layout(D, H)
        pack = np.concatenate([p["W_e"].ravel(), p["W_dT"].ravel(), p["b_e"], p["b_d"], np.zeros(D, np.float32)]).astype(np.float32)
        assert pack.size == self.total
        self.params = torch.from_numpy(pack).to(device)
        N.check(eng.lib.wsae_prepare(self.handle, self.params.data_ptr(), eng.stream()), "wsae_prepare")
        self.x = torch.from_numpy(p["x"]).to(device)
        if p["x_dtype"] == "bf16":
            self.x = self.x.to(torch.bfloat16)
            assert np.array_equal(self.x.float().cpu().numpy(), p["x"])
        self.dt = N.DT_BF16 if p["x_dtype"] == "bf16" else N.DT_F32
        self.rows = None if p["rows"] is None else torch.from_numpy(p["rows"]).to(device)
        self.rows_ptr = 0 if self.rows is None else self.rows.data_ptr()

    def forward(self, hidden_ptr, recon_ptr):
        p, eng = self.p, self.eng
        eng.stats.zero_()
        self.sp_out = torch.full((1,), -1.0, dtype=torch.float32, device=self.device)
        return eng.lib.wsae_relu_forward(self.handle, self.params.data_ptr(), self.x.data_ptr(), self.dt, self.rows_ptr, p["B"],
                                         p["weight"], hidden_ptr, recon_ptr, eng.stats.data_ptr(), self.sp_out.data_ptr(), eng.stream())

    def backward(self, hidden_ptr, recon_ptr, grads_ptr):
        p, eng = self.p, self.eng
        return eng.lib.wsae_relu_backward(self.handle, self.params.data_ptr(), self.x.data_ptr(), self.dt, self.rows_ptr, p["B"],
                                          p["weight"], hidden_ptr, recon_ptr, grads_ptr, eng.stream())

    def run(self, with_buffers=True, between=None):
        """Forward and backward with guarded buffers; returns the outputs as numpy and asserts the guards."""
        N, p = self.N, self.p
        B, D, H = p["B"], p["D"], p["H"]
        hid, rec, grads = Guarded(self.device, B * H, 0), Guarded(self.device, B * D, 1), Guarded(self.device, self.total, 2)
        hp, rp = (hid.ptr, rec.ptr) if with_buffers else (0, 0)
        N.check(self.forward(hp, rp), "wsae_relu_forward")
        stats = self.eng.stats.cpu().numpy().copy()
        sp_out = self.sp_out.cpu().numpy().copy()
        if between is not None:
            between()
        N.check(self.backward(hp, rp, grads.ptr), "wsae_relu_backward")
        torch.cuda.synchronize()
        for b in (hid, rec, grads):
            assert b.sentinels_intact()
        g, off = grads.payload(), self.off
        f = stats.view(np.float32)
        assert stats[7] == sp_out.view(np.int32)[0]  # stats.reserved carries the bits of *sparsity_loss_out
        assert not g[off[4]:off[4] + D].view(np.int32).any()  # no pre-bias in this module: its slot is exactly 0
        return {"hidden": hid.payload().reshape(B, H), "recon": rec.payload().reshape(B, D), "loss": f[0], "l0": f[1],
                "sparsity": sp_out[0], "dW_e": g[off[0]:off[1]].reshape(H, D), "dW_dT": g[off[1]:off[2]].reshape(H, D),
                "db_e": g[off[2]:off[3]], "db_d": g[off[3]:off[4]], "grads": g, "stats": stats}


def same_bits(a, b, keys=("hidden", "recon", "grads", "stats")):
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.int32), np.ascontiguousarray(b[k]).view(np.int32)) for k in keys)


def check(p, prec, flow, out, note, key):
    res = RO.check_step(p["W_e"], p["W_dT"], p["b_e"], p["b_d"], p["x"], p["rows"], prec, flow, p["weight"], p["l1w"],
                        p["loss_cols"], out)
    print(key, {k: round(v, 4) for k, v in res.items()})
    for k in TENSORS:
        note(f"relu_{key}_{k}_over_bound", res[k], 1.0)
    note(f"relu_{key}_unsure_share", res["unsure_share"], UNSURE_CAP)
    note(f"relu_{key}_dW_e_worst_allowance_part", res["dW_e_worst_allowance_part"], 1.0)
    for k in ("hidden", "recon", "dW_e", "dW_dT", "db_e", "db_d"):
        assert np.isfinite(out[k]).all(), k
    assert res["conflicts"] == 0, "the device's activity mask differs from the reference's outside the unsure set"
    assert res["unsure_share"] <= UNSURE_CAP
    for k in TENSORS:
        assert res[k] <= 1.0, (k, res[k])
    return res


def expect_flow(step, flow):
    assert step.eng.lib.wsae_relu_needs_hidden(step.handle, step.p["B"]) == (0 if flow == "xgemm" else 1)


# ---- every route, float32 and bf16 activations ---------------------------------------------------------------------------
@pytest.mark.parametrize("x_dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_step_matches_float64_stage_by_stage(rigs, device, parity_note, case, x_dtype):
    """Stages a, c, d, e, f, g within their derived bounds, the unsure set under its cap, guards intact, and the same
    case twice bit-identical (no float atomics in this file).

    Catches: a batch row dropped from or repeated in a contraction (a ragged last tile, a partly filled 256-row tile); a
    split-K slab left out or summed twice (``grid.z`` smaller than the ``nz`` asked for, the ``gemm256d`` fallback,
    ``slab_sum8_kernel`` at ``nz`` 2, 4, 8, ``grad_finish_kernel`` at ``nsplit`` 2); a missing L1 term; hidden read unrounded
    by the decoder GEMM; a bf16 ``x`` read as float32; an activity bit from the wrong row or word."""
    prec, D, H, B, flow, _ = case
    p = make_problem(D, H, B, x_dtype)
    step = Step(rigs(D, H), device, p, prec)
    expect_flow(step, flow)
    out = step.run()
    check(p, prec, flow, out, parity_note, f"{case_id(case)}-x{x_dtype}")
    assert same_bits(out, step.run())


# ---- rows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x_dtype", ["f32", "bf16"])
@pytest.mark.parametrize("prec,D,H,B,flow", [("bf16", 96, 352, 200, "general"), ("bf16", 128, 256, 256, "xgemm"),
                                             ("bf16", 384, 768, 256, "xgemm")])
def test_rows_gather(rigs, device, parity_note, prec, D, H, B, flow, x_dtype):
    """The batch gathered through ``rows`` from a source of 2 B + 5 rows, descending with one index repeated: staging,
    the residual and (bf16 x) ``stage_rows_copy_kernel`` all read x[rows[b]].
    Catches: ``rows`` ignored by the staging or by the residual pass alone (hidden right, g wrong)."""
    p = make_problem(D, H, B, x_dtype, with_rows=True)
    step = Step(rigs(D, H), device, p, prec)
    expect_flow(step, flow)
    check(p, prec, flow, step.run(), parity_note, f"rows-{D}x{H}-B{B}-x{x_dtype}")


# ---- per-feature L1 weights with loss_cols != D -----------------------------------------------------------------------------
@pytest.mark.parametrize("prec,D,H,B,flow", [("bf16", 96, 352, 200, "general"), ("bf16", 128, 256, 256, "xgemm")])
def test_l1_weights_and_loss_cols(rigs, device, parity_note, prec, D, H, B, flow):
    """``wsae_ctx_set_relu_l1_weights`` (weights in [0.5, 1.5]) with ``wsae_ctx_set_loss_cols(D / 2)``.
    Catches: the weight ignored in the forward's sparsity or in dpre; ``loss_cols`` replaced by D in ``scale`` or the mse."""
    from whisper_sae import _native as N
    p = make_problem(D, H, B, "f32", with_l1w=True, half_cols=True)
    step = Step(rigs(D, H), device, p, prec)
    l1w = torch.from_numpy(p["l1w"]).to(device)
    try:
        N.check(step.eng.lib.wsae_ctx_set_relu_l1_weights(step.handle, l1w.data_ptr()), "wsae_ctx_set_relu_l1_weights")
        N.check(step.eng.lib.wsae_ctx_set_loss_cols(step.handle, D // 2), "wsae_ctx_set_loss_cols")
        out = step.run()
    finally:
        step.eng.lib.wsae_ctx_set_relu_l1_weights(step.handle, 0)
        step.eng.lib.wsae_ctx_set_loss_cols(step.handle, D)
    check(p, prec, flow, out, parity_note, f"l1w-{D}x{H}-B{B}")


# ---- hidden == recon == NULL ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,H,B", [(128, 256, 256), (384, 768, 256)])
def test_without_hidden_and_recon(rigs, device, D, H, B):
    """What the trainer passes on the row-major-GEMM flow: gradients and the step record are bit-identical to the run with
    both buffers (the launches are the same).  Catches: a store through a null ``e.c`` / ``recon_out``; a loss or g taken
    from the caller's buffer rather than the slabs."""
    p = make_problem(D, H, B, "bf16")
    step = Step(rigs(D, H), device, p, "bf16")
    expect_flow(step, "xgemm")
    assert same_bits(step.run(), step.run(with_buffers=False), keys=("grads", "stats"))


def test_general_path_refuses_null_buffers(rigs, device):
    """The same call on the general path returns -1 and says why, before anything is launched."""
    from whisper_sae import _native as N
    p = make_problem(96, 352, 200, "f32")
    step = Step(rigs(96, 352), device, p, "bf16")
    expect_flow(step, "general")
    assert step.forward(0, 0) == -1
    assert "this shape needs the fp32 hidden and recon buffers" in N.last_error()


# ---- backward_x with relu_g_B != B ---------------------------------------------------------------------------------------
def test_backward_rebuilds_g_after_a_decode(rigs, device, parity_note):
    """``wsae_decode_loss`` between the forward and the backward takes ctx->gb and the db_d partials (``relu_g_B`` = 0,
    ``relu_x_B`` kept) and nothing else ``backward_x`` reads: the backward rebuilds g from ``recon`` with the same kernel
    and the same arithmetic, so the gradients are within the bounds AND bit-identical to the direct run.  Without ``recon`` the
    call is refused.  Catches: a rebuild skipped (dW_d^T and db_d from the decode's residual), or one that reads x without ``rows``."""
    from whisper_sae import _native as N
    D, H, B, K = 128, 256, 256, 8
    p = make_problem(D, H, B, "f32", with_rows=True)
    eng = rigs(D, H)
    step = Step(eng, device, p, "bf16")
    expect_flow(step, "xgemm")
    direct = step.run()
    vals = torch.from_numpy(synth.uniform((B, K), 5, 1, 0.1, 1.0)).to(device)
    idx = torch.from_numpy(((np.arange(B)[:, None] * 7 + np.arange(K)[None, :] * 31) % H).astype(np.int32)).to(device)
    scratch = {"recon": torch.empty(B, D, dtype=torch.float32, device=device),
               "dpre": torch.empty(B, K, dtype=torch.float32, device=device),
               "stats": torch.zeros(N.STATS_WORDS, dtype=torch.int32, device=device)}

    def decode():
        N.check(eng.lib.wsae_decode_loss(step.handle, step.params.data_ptr(), step.x.data_ptr(), step.dt, step.rows_ptr, vals.data_ptr(),
                                         idx.data_ptr(), B, scratch["recon"].data_ptr(), 1, scratch["dpre"].data_ptr(), 0, 0,
                                         scratch["stats"].data_ptr(), eng.stream()), "wsae_decode_loss")

    rebuilt = step.run(between=decode)
    check(p, "bf16", "xgemm", rebuilt, parity_note, f"rebuild-{D}x{H}-B{B}")
    assert same_bits(direct, rebuilt)
    # ... and with no recon to rebuild from
    hid, rec, grads = Guarded(device, B * H, 0), Guarded(device, B * D, 1), Guarded(device, step.total, 2)
    N.check(step.forward(hid.ptr, rec.ptr), "wsae_relu_forward")
    decode()
    assert step.backward(0, 0, grads.ptr) == -1
    assert "no recon was passed to rebuild it" in N.last_error()
    torch.cuda.synchronize()
    assert grads.sentinels_intact() and (grads.payload() == 777.0).all()
