"""Gradient-based feature attribution, the parts that need no GPU: the float64 oracle against
the intervention oracle (a linear metric's attribution is the whole effect of the edit), the fixed-point per-feature
sums restated in Python, the gradient-capturing hooks on a seeded tiny Whisper (plain torch), and the host-side errors.
The kernel itself is checked on the device in tests/test_gpu_attribution.py."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import attribution_oracle as AO
import intervention_oracle as IO
from whisper_sae import _native as N
from whisper_sae.causal import FeatureEdit, SAEAttribution, WhisperAttribution, attribution_effects
from whisper_sae.sae.model import BatchTopKSAE, ReLUSAE, TopKSAE


def tiny_whisper(seed: int = 0):
    """The recipe of tests/test_hooks.py and tests/test_causal.py."""
    from transformers import WhisperConfig, WhisperForConditionalGeneration
    cfg = WhisperConfig(vocab_size=200, num_mel_bins=80, encoder_layers=2, decoder_layers=2, encoder_attention_heads=2,
                        decoder_attention_heads=2, encoder_ffn_dim=128, decoder_ffn_dim=128, d_model=64,
                        max_source_positions=50, max_target_positions=16, decoder_start_token_id=1, pad_token_id=0,
                        bos_token_id=1, eos_token_id=2)
    torch.manual_seed(seed)
    return WhisperForConditionalGeneration(cfg).eval()


def mel(seed: int, batch: int = 3) -> torch.Tensor:
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((batch, 80, 100)).astype(np.float32))


# ---- the oracle ------------------------------------------------------------------------------------------------------
def synthetic_case(rows=37, D=48, H=96, k=8, seed=0):
    rng = np.random.default_rng(seed)
    h = rng.standard_normal((rows, D)) * rng.uniform(0.5, 3.0, (rows, 1)) + rng.normal(0.0, 1.0, (rows, 1))
    w_dT = rng.standard_normal((H, D)) / np.sqrt(D)
    idx = np.stack([rng.choice(H, k, replace=False) for _ in range(rows)]).astype(np.int32)
    vals = rng.standard_normal((rows, k)).astype(np.float32)  # about half the entries are inactive (v <= 0)
    gamma = rng.uniform(0.5, 1.5, D) * rng.choice([-1.0, 1.0], D)
    beta = rng.normal(0.0, 0.3, D)
    scale = np.ones(H)
    scale[rng.choice(H, H // 2, replace=False)] = rng.choice([0.0, 0.5, 2.5], H // 2)
    mask = (rng.uniform(size=rows) < 0.6).astype(np.uint8)
    c = rng.standard_normal(D)
    return h, w_dT, idx, vals, gamma, beta, scale, mask, c


@pytest.mark.parametrize("with_norm", [True, False])
@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("ablate_all", [False, True])
def test_oracle_attribution_of_a_linear_metric_is_the_effect_of_the_intervention(with_norm, with_mask, ablate_all):
    """``m = sum_d C_d h'_d``: ``sum_j attr_rj == sum_d C_d (h'_rd - h_rd)`` in float64, row by row."""
    h, w_dT, idx, vals, gamma, beta, scale, mask, c = synthetic_case()
    rows, D = h.shape
    H = w_dT.shape[0]
    g, b, eps = (gamma, beta, 1e-5) if with_norm else (None, None, 0.0)
    m = mask if with_mask else None
    edit = np.zeros(H) if ablate_all else scale
    out, _, changed = IO.intervene(h, vals, idx, w_dT, np.zeros(D), np.zeros(D), g, b, eps, scale=edit, row_mask=m,
                                   mode="keep_error")
    effect = (out - h) @ c
    got = AO.attribute(h, np.broadcast_to(c, h.shape), vals, idx, w_dT, g, eps, scale=None if ablate_all else scale,
                       row_mask=m)
    total = got["attr"].sum(axis=1)
    size = np.abs(got["attr"]).sum(axis=1) + np.abs(h) @ np.abs(c)
    assert changed.any() and np.abs(effect).max() > 0
    assert np.all(np.abs(total - effect) <= 1e-12 * size)
    # rows the edit leaves alone have no attribution at all, and entries with w == 0 are exact zeros
    assert np.all(got["attr"][~changed] == 0.0) and np.all(got["attr"][got["w"] == 0] == 0.0)
    # per-feature outputs are the sums of the entries
    for f in range(H):
        at = (idx == f) & (got["w"] != 0)
        assert got["feat_rows"][f] == at.sum()
        assert np.isclose(got["feat_sum"][f], got["attr"][at].sum(), rtol=1e-12, atol=1e-300)
        assert np.isclose(got["feat_abs"][f], np.abs(got["attr"][at]).sum(), rtol=1e-12, atol=1e-300)
    assert np.all(got["attr_bound"] >= 0) and np.all(got["feat_bound"] > 0)
    if with_mask:
        assert np.all(got["attr"][mask == 0] == 0.0)


# ---- the fixed-point sums ----------------------------------------------------------------------------------------------
class TestFixedPoint:
    H = 64

    def entries(self, n=5000, seed=1):
        rng = np.random.default_rng(seed)
        # eleven decades of magnitude and both signs: an fp32 sum of these depends on the order
        attr = (rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 3, n)).astype(np.float32)
        idx = rng.integers(0, self.H, n)
        return attr, idx

    def test_invariant_under_permutation(self):
        attr, idx = self.entries()
        base = AO.fixed_point_sums(attr, idx, self.H)
        for seed in range(4):
            order = np.random.default_rng(100 + seed).permutation(attr.size)
            again = AO.fixed_point_sums(attr[order], idx[order], self.H)
            assert np.array_equal(base[0].view(np.uint32), again[0].view(np.uint32))
            assert np.array_equal(base[1].view(np.uint32), again[1].view(np.uint32))
        assert base[0].dtype == np.float32 and np.any(base[0] != 0)

    def test_within_the_stated_bound_of_the_float64_sum(self):
        attr, idx = self.entries(seed=2)
        fs, fa = AO.fixed_point_sums(attr, idx, self.H)
        q = AO.quantum(float(np.abs(attr).max()))
        assert q == 2.0 ** (np.floor(np.log2(np.abs(attr).max())) + 1 - 36)
        want = np.bincount(idx, weights=attr.astype(np.float64), minlength=self.H)
        want_abs = np.bincount(idx, weights=np.abs(attr.astype(np.float64)), minlength=self.H)
        n_f = np.bincount(idx, minlength=self.H)
        for got, ref in ((fs, want), (fa, want_abs)):
            bound = n_f * q / 2 + 2.0 ** -24 * (np.abs(ref) + n_f * q / 2) + 2.0 ** -149
            assert np.all(np.abs(got.astype(np.float64) - ref) <= bound)
        assert np.all(fa >= np.abs(fs))

    def test_power_of_two_maximum_and_exact_small_sums(self):
        # A = 2^3 exactly: e = 4 (A < 2^e), q = 2^-32; multiples of q are summed exactly
        attr = np.array([8.0, -8.0, 2.0 ** -32, 3 * 2.0 ** -32, -2.0 ** -34], np.float32)
        idx = np.array([0, 0, 0, 1, 2])
        assert AO.quantum(8.0) == 2.0 ** -32
        fs, fa = AO.fixed_point_sums(attr, idx, 4)
        assert fs.tolist() == [2.0 ** -32, 3 * 2.0 ** -32, 0.0, 0.0]  # the float sum (8 - 8 + 2^-32) in another order loses it
        assert fa.tolist() == [16.0, 3 * 2.0 ** -32, 0.0, 0.0]  # 16 + 2^-32 rounds to 16 once; |-2^-34| < q / 2 rounds to 0

    def test_all_zero_input_gives_exact_zeros(self):
        fs, fa = AO.fixed_point_sums(np.zeros(100, np.float32), np.arange(100) % self.H, self.H)
        assert not fs.any() and not fa.any() and not np.signbit(fs).any()
        assert AO.quantum(0.0) == 0.0
        fs, fa = AO.fixed_point_sums(np.ones(10, np.float32), np.zeros(10, int), self.H, active=np.zeros(10, bool))
        assert not fs.any() and not fa.any()

    def test_more_than_2_26_entries_are_rejected(self):
        assert AO.MAX_ENTRIES == 1 << 26
        zeros = np.broadcast_to(np.float32(0.0), (8193, 8192))  # 2^26 + 8192 entries, no memory behind them
        with pytest.raises(ValueError, match="2\\^26"):
            AO.fixed_point_sums(zeros, np.broadcast_to(np.int64(0), zeros.shape), 1)
        AO.fixed_point_sums(zeros[:4], np.broadcast_to(np.int64(0), (4, 8192)), 1)

    def test_library_argument_errors_come_before_any_launch(self):
        """``wsae_attribute`` checks its arguments before any launch: NULL arguments are refused without a GPU (its own
        2^26 limit needs a ctx: tests/test_gpu_attribution.py)."""
        lib = N.lib()
        assert lib.wsae_attribute(None, None, None, 0, None, 0, 4, None, None, None, 0.0, None, None, None, None, None,
                                  None, None, 0, None) == -1
        assert "wsae_attribute" in N.last_error()
        assert lib.wsae_attribute_workspace_bytes(3072) >= 3072 * 20 and lib.wsae_attribute_workspace_bytes(0) == 0
        assert len(N.SIGNATURES["wsae_attribute"][1]) == 20


# ---- the hooks (plain torch, CPU) --------------------------------------------------------------------------------------
ENC, DEC = ("encoder", 1), ("decoder", 0)


def metric_of(logits: torch.Tensor) -> torch.Tensor:
    return torch.log_softmax(logits.double(), dim=-1)[:, :, 7].mean()


def reference_gradients(model, x, ids, taps):
    """Logits of the unhooked model and ``torch.autograd.grad`` of the metric with respect to the tapped outputs."""
    kept = {}

    def grab(tap):
        def hook(module, inputs, output):
            hidden = output[0] if isinstance(output, (tuple, list)) else output
            if not hidden.requires_grad:  # frozen model: make the tapped output the start of the graph
                hidden = hidden.detach().requires_grad_(True)
                kept[tap] = hidden
                return (hidden, *output[1:]) if isinstance(output, tuple) else hidden
            kept[tap] = hidden
            return None
        return hook

    handles = [getattr(model.model, c).layers[i].register_forward_hook(grab((c, i))) for c, i in taps]
    try:
        logits = model(input_features=x, decoder_input_ids=ids).logits
        grads = torch.autograd.grad(metric_of(logits), [kept[t] for t in taps])
    finally:
        for hnd in handles:
            hnd.remove()
    return logits.detach(), dict(zip(taps, grads))


@pytest.mark.parametrize("frozen", [False, True])
@pytest.mark.parametrize("taps", [[ENC], [DEC], [ENC, DEC]])
def test_hooks_capture_the_gradient_and_leave_the_logits_alone(frozen, taps):
    model = tiny_whisper(0)
    model.requires_grad_(not frozen)
    x, ids = mel(10), torch.tensor([[1, 5, 7]] * 3)
    with torch.no_grad():
        plain = model(input_features=x, decoder_input_ids=ids).logits
    ref_logits, ref = reference_gradients(model, x, ids, taps)
    assert torch.equal(ref_logits.view(torch.int32), plain.view(torch.int32))
    sae = TopKSAE(64, 128, k=8)
    hooked = WhisperAttribution(model, {t: SAEAttribution(sae) for t in taps})
    with hooked:
        logits = model(input_features=x, decoder_input_ids=ids).logits
        assert torch.equal(logits.detach().view(torch.int32), plain.view(torch.int32))
        assert set(hooked.hidden) == set(taps) and not hooked.grads
        with pytest.raises(RuntimeError, match="no gradient"):
            hooked.compute()
        metric_of(logits).backward()
    assert set(hooked.grads) == set(taps)
    for t in taps:
        assert hooked.grads[t].shape == hooked.hidden[t].shape == ((3, 50, 64) if t == ENC else (3, 3, 64))
        assert torch.equal(hooked.grads[t].view(torch.int32), ref[t].view(torch.int32)), t
        assert float(hooked.grads[t].abs().max()) > 0
    if frozen:
        assert all(p.grad is None for p in model.parameters())
    # the hooks are gone, and the model is what it was
    assert not model.model.encoder.layers[1]._forward_hooks and not model.model.decoder.layers[0]._forward_hooks
    with torch.no_grad():
        assert torch.equal(model(input_features=x, decoder_input_ids=ids).logits, plain)
    # the gradients of the taps alone, without touching any parameter's .grad
    model.zero_grad(set_to_none=True)
    with hooked:
        hooked.backward(metric_of(model(input_features=x, decoder_input_ids=ids).logits))
    for t in taps:
        assert torch.equal(hooked.grads[t].view(torch.int32), ref[t].view(torch.int32)), t
    assert all(p.grad is None for p in model.parameters())
    assert not hooked._tapped  # the graph from the taps onwards is not kept beyond the hooks
    # compute() has no CPU path: the kernel is the only implementation
    with pytest.raises(N.WsaeError, match="no CPU path"):
        hooked.compute()


def test_forward_without_grad_leaves_nothing_to_compute():
    model = tiny_whisper(0)
    hooked = WhisperAttribution(model, {ENC: SAEAttribution(TopKSAE(64, 128, k=8))})
    with hooked, torch.no_grad():
        model.model.encoder(mel(1))
    assert ENC in hooked.hidden and ENC not in hooked.grads
    with pytest.raises(RuntimeError, match="no gradient"):
        hooked.compute()
    with pytest.raises(TypeError):
        WhisperAttribution(model, {ENC: FeatureEdit()})
    with pytest.raises(ValueError, match="does not exist"):
        WhisperAttribution(model, {("encoder", 2): SAEAttribution(TopKSAE(64, 128, k=8))})


# ---- host-side errors ----------------------------------------------------------------------------------------------------
class TestSAEAttribution:
    def test_only_topk_codes(self):
        from whisper_sae.sae.crosscoder import create_crosscoder
        from whisper_sae.sae.transcoder import create_transcoder
        SAEAttribution(TopKSAE(64, 128, k=8))
        SAEAttribution(BatchTopKSAE(64, 128, k=8), edit=FeatureEdit.scale([1, 2], 0.5) | FeatureEdit.ablate([3]))
        for other in (ReLUSAE(64, 128), create_transcoder(64, 64, 128, k=8), create_crosscoder(64, 2, 128, k=8)):
            with pytest.raises(TypeError):
                SAEAttribution(other)
        with pytest.raises(TypeError):
            SAEAttribution(TopKSAE(64, 128, k=8), edit={3: 0.0})

    def test_clamped_features_are_out_of_scope(self):
        with pytest.raises(ValueError, match="clamped"):
            SAEAttribution(TopKSAE(64, 128, k=8), edit=FeatureEdit.clamp([3], 1.0))
        with pytest.raises(ValueError, match="clamped"):
            SAEAttribution(TopKSAE(64, 128, k=8), edit=FeatureEdit.ablate([1]) | FeatureEdit.clamp([3], 1.0))

    def test_cpu_tensors_raise_wsae_error(self):
        at = SAEAttribution(TopKSAE(64, 128, k=8))
        with pytest.raises(N.WsaeError, match="no CPU path"):
            at.attribute(torch.zeros(5, 64), torch.zeros(5, 64))
        assert at.total_sum is None and at.calls == 0 and at.top(3) == []

    def test_attribution_effects_has_no_cpu_path(self):
        model = tiny_whisper(0)
        with pytest.raises(N.WsaeError):
            attribution_effects(model, mel(2), TopKSAE(64, 128, k=8), ("encoder", 1))
        assert len(model.model.encoder.layers[1]._forward_hooks) == 0
        assert all(p.grad is None for p in model.parameters())
