"""Gradient-based feature attribution on the device: ``wsae_attribute`` against the float64
oracle of tests/attribution_oracle.py, its determinism, the cross-check against ``wsae_intervene`` through a linear
metric, and the hooks on a seeded tiny Whisper.

The oracle is always handed the code the product selected (``AttributionResult.vals`` / ``.idx``), so no case depends
on the order of near-ties, and no row or entry is excluded from any comparison.  The tolerances are the oracle's own
bounds (its docstring); every case prints the worst ratio error / bound it met.
"""

from __future__ import annotations

import json

import numpy as np
import pytest
import torch

import attribution_oracle as AO
import intervention_oracle as IO
from whisper_sae.causal import (FeatureEdit, SAEAttribution, SAEIntervention, WhisperAttribution, attribution_effects)
from whisper_sae import _native as N
from whisper_sae.sae.engine import _dtype_code
from whisper_sae.sae.model import BatchTopKSAE, TopKSAE

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROWS_SHAPE = (31, 97)  # 3007 rows: a multiple of nothing the kernels tile by


def make_sae(D, H, k, precision, seed=0, cls=TopKSAE):
    torch.manual_seed(seed)
    sae = cls(D, H, k=k, precision=precision)
    with torch.no_grad():
        sae.decoder.weight.mul_(10.0)  # unit-norm decoder columns
        sae.b_pre.normal_(0.0, 0.1)
        sae.decoder.bias.normal_(0.0, 0.1)
    return sae.to(DEV).eval()


def make_hidden(shape, D, seed, dtype=torch.float32):
    rng = np.random.default_rng(seed)
    rows = int(np.prod(shape))
    h = rng.standard_normal((rows, D)) * rng.uniform(0.5, 3.0, (rows, 1)) + rng.normal(0.0, 1.0, (rows, 1))
    return torch.from_numpy(h.astype(np.float32)).reshape(*shape, D).to(DEV).to(dtype)


def make_grad(shape, D, seed, dtype=torch.float32):
    rng = np.random.default_rng(seed)
    rows = int(np.prod(shape))
    g = rng.standard_normal((rows, D)) * 10.0 ** rng.uniform(-3, 0, (rows, 1))
    return torch.from_numpy(g.astype(np.float32)).reshape(*shape, D).to(DEV).to(dtype)


def make_norm(D, seed):
    rng = np.random.default_rng(seed)
    norm = torch.nn.LayerNorm(D, eps=1e-5)
    with torch.no_grad():
        norm.weight.copy_(torch.from_numpy((rng.uniform(0.5, 1.5, D) * rng.choice([-1.0, 1.0], D)).astype(np.float32)))
        norm.bias.copy_(torch.from_numpy(rng.normal(0.0, 0.3, D).astype(np.float32)))
    return norm.to(DEV)


def decoder_rows(sae) -> np.ndarray:
    """W_dT [H, D] as the ctx's decode reads it in the module's precision mode."""
    w = sae.decoder.weight.detach().t().contiguous().float().cpu().numpy()
    return IO.bf16_round(w) if sae.precision == "bf16" else w


def oracle_for(sae, at, result, h, grad, norm):
    D = h.shape[-1]
    k = result.idx.shape[-1]
    gamma, eps = (None, 0.0) if norm is None else (norm.weight.detach().cpu().numpy(), norm.eps)
    scale = None if at.edit is None else at.edit.tables(sae.hidden_dim, DEV)[0].cpu().numpy()
    mask = None if at.positions is None else at._ops.row_mask(h.shape, torch.device(DEV)).cpu().numpy()
    a_max = float(result.attr.abs().max()) if result.attr.numel() else 0.0
    return AO.attribute(h.reshape(-1, D).float().cpu().numpy(), grad.reshape(-1, D).float().cpu().numpy(),
                        result.vals.reshape(-1, k).cpu().numpy(), result.idx.reshape(-1, k).cpu().numpy(),
                        decoder_rows(sae), gamma, eps, scale, mask, a_max=a_max)


def ratio(got, want, bound) -> float:
    g = got.detach().reshape(want.shape).cpu().numpy().astype(np.float64)
    assert np.isfinite(g).all()
    err = np.abs(g - want)
    # (a zero bound means a zero value that must be met exactly)
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))


def check_case(sae, h, grad, edit, norm, positions=None, label=""):
    at = SAEAttribution(sae, layer_norm=norm, edit=edit, positions=positions)
    res = at.attribute(h, grad)
    k = res.idx.shape[-1]
    assert k == sae.bind().k
    assert res.attr.shape == (*h.shape[:-1], k) and res.idx.shape == res.attr.shape and res.attr.dtype == torch.float32
    assert res.feat_sum.shape == res.feat_abs.shape == res.feat_rows.shape == (sae.hidden_dim,)
    want = oracle_for(sae, at, res, h, grad, norm)
    r_attr = ratio(res.attr, want["attr"], want["attr_bound"])
    r_sum = ratio(res.feat_sum, want["feat_sum"], want["feat_bound"])
    r_abs = ratio(res.feat_abs, want["feat_abs"], want["feat_bound"])
    n_active = int((want["w"] != 0).sum())
    print(f"[attribute] {label} h={h.dtype} G={grad.dtype} rows={want['attr'].shape[0]} entries with w != 0: {n_active} "
          f"worst error/bound: attr {r_attr:.3f}, feat_sum {r_sum:.3f}, feat_abs {r_abs:.3f}")
    assert r_attr <= 1.0, f"{label}: attr error is {r_attr:.3f} x the derived bound"
    assert r_sum <= 1.0, f"{label}: feat_sum error is {r_sum:.3f} x the derived bound"
    assert r_abs <= 1.0, f"{label}: feat_abs error is {r_abs:.3f} x the derived bound"
    assert np.array_equal(res.feat_rows.cpu().numpy().astype(np.int64), want["feat_rows"]), f"{label}: feat_rows"
    # entries with w == 0 are bit-exact zeros (+0.0)
    zero = torch.from_numpy(want["w"] == 0).to(DEV)
    assert bool((res.attr.reshape(-1, k).view(torch.int32)[zero] == 0).all()), f"{label}: zero entries"
    return at, res, want


def feature_counts(sae, h, norm) -> np.ndarray:
    iv = SAEIntervention(sae, FeatureEdit(), layer_norm=norm)
    iv.apply(h)
    vals, idx = (t.cpu().numpy() for t in iv.last_code)
    return np.bincount(idx[vals > 0].ravel(), minlength=sae.hidden_dim)


def mixed_scale_edit(counts) -> FeatureEdit:
    """Factors 0, 0.5, 1 and 2.5 on frequently active features and on (almost) never active ones."""
    order = np.argsort(-counts, kind="stable")
    top, rare = order[:24].tolist(), order[-8:].tolist()
    return (FeatureEdit.scale(top[0:6] + rare[0:2], 0.0) | FeatureEdit.scale(top[6:12] + rare[2:4], 0.5)
            | FeatureEdit.scale(top[12:18] + rare[4:6], 1.0) | FeatureEdit.scale(top[18:24] + rare[6:8], 2.5))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("k", [8, 32, 64])
@pytest.mark.parametrize("D", [64, 384, 768, 1280])
def test_kernel_matches_the_oracle(D, k, precision):
    H = 1024
    sae = make_sae(D, H, k, precision, seed=D + k)
    norm = make_norm(D, seed=D)
    h = make_hidden(ROWS_SHAPE, D, seed=k)
    grad = make_grad(ROWS_SHAPE, D, seed=k + 7)
    hb, gb = h.to(torch.bfloat16), grad.to(torch.bfloat16)
    mixed = mixed_scale_edit(feature_counts(sae, h, norm))
    tag = f"D={D} k={k} {precision}"
    check_case(sae, h, grad, None, norm, label=f"{tag} ablate all")
    check_case(sae, h, grad, mixed, norm, label=f"{tag} mixed scales")
    check_case(sae, h, grad, None, None, label=f"{tag} ablate all, no norm")
    check_case(sae, h, grad, mixed, norm, positions=[0, 5, 96], label=f"{tag} mixed scales, row mask")
    check_case(sae, hb, gb, None, norm, label=f"{tag} ablate all")
    check_case(sae, h, gb, mixed, norm, label=f"{tag} mixed scales")
    check_case(sae, hb, grad, mixed, None, positions=[1, 2, 3, 50], label=f"{tag} mixed scales, no norm, row mask")
    # a single row
    check_case(sae, h[:1, :1], grad[:1, :1], None, norm, label=f"{tag} one row, ablate all")
    check_case(sae, hb[:1, :1], gb[:1, :1], mixed, norm, label=f"{tag} one row, mixed scales")
    # an edit that changes nothing and a mask that selects nothing: exact zeros everywhere
    for edit, positions in ((FeatureEdit.scale([1, 2], 1.0), None), (None, [])):
        at = SAEAttribution(sae, layer_norm=norm, edit=edit, positions=positions)
        res = at.attribute(h, grad)
        assert not res.attr.view(torch.int32).any() and not res.feat_sum.view(torch.int32).any()
        assert not res.feat_abs.view(torch.int32).any() and not res.feat_rows.any()


def test_two_calls_and_any_row_order_give_the_same_bits():
    D, H, k = 768, 1024, 32
    sae = make_sae(D, H, k, "bf16", seed=11)
    norm = make_norm(D, seed=12)
    h = make_hidden((3007,), D, seed=13)
    grad = make_grad((3007,), D, seed=14)
    mixed = mixed_scale_edit(feature_counts(sae, h, norm))
    bits = lambda t: t.view(torch.int32)  # noqa: E731
    for edit in (None, mixed):
        at = SAEAttribution(sae, layer_norm=norm, edit=edit)
        first, second = at.attribute(h, grad), at.attribute(h, grad)
        for name in ("attr", "idx", "feat_sum", "feat_abs", "feat_rows"):
            assert torch.equal(bits(getattr(first, name)), bits(getattr(second, name))), name
        assert bool(first.feat_sum.abs().max() > 0)
        for seed in (0, 1):
            perm = torch.from_numpy(np.random.default_rng(seed).permutation(3007)).to(DEV)
            moved = at.attribute(h[perm].contiguous(), grad[perm].contiguous())
            assert torch.equal(moved.idx, first.idx[perm])  # the code of a row depends on the row alone
            assert torch.equal(bits(moved.attr), bits(first.attr[perm]))
            assert torch.equal(bits(moved.feat_sum), bits(first.feat_sum))
            assert torch.equal(bits(moved.feat_abs), bits(first.feat_abs))
            assert torch.equal(moved.feat_rows, first.feat_rows)
        # a different launch geometry: the first 1000 rows on their own give the attr bits they had in the full call
        part = at.attribute(h[:1000], grad[:1000])
        assert torch.equal(bits(part.attr), bits(first.attr[:1000]))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("with_norm", [True, False])
def test_attribution_of_a_linear_metric_is_the_effect_of_the_intervention(precision, with_norm):
    """G = C on every row: ``sum_j attr_rj`` against ``sum_d C_d (h'_rd - h_rd)`` of ``SAEIntervention.apply`` with the
    same edit, within ``sum_d |C_d| (intervention bound_d) + sum_j (attribution bound_j)`` of the two oracles."""
    D, H, k = 384, 1024, 32
    sae = make_sae(D, H, k, precision, seed=21)
    norm = make_norm(D, seed=22) if with_norm else None
    h = make_hidden(ROWS_SHAPE, D, seed=23)
    c = torch.from_numpy(np.random.default_rng(24).standard_normal(D).astype(np.float32)).to(DEV)
    grad = c.expand(*ROWS_SHAPE, D).contiguous()
    counts = feature_counts(sae, h, norm)
    for label, edit, iv_edit in (("mixed scales", mixed_scale_edit(counts), mixed_scale_edit(counts)),
                                 ("ablate all", None, FeatureEdit.ablate(range(H)))):
        iv = SAEIntervention(sae, iv_edit, layer_norm=norm, mode="keep_error")
        out = iv.apply(h)
        at, res, want = check_case(sae, h, grad, edit, norm, label=f"linear metric {precision} {label}")
        assert torch.equal(res.idx.reshape(-1, k), iv.last_code[1]) and torch.equal(res.vals.reshape(-1, k), iv.last_code[0])
        vals, idx = (t.cpu().numpy() for t in iv.last_code)
        scale = iv_edit.tables(H, DEV)[0].cpu().numpy()
        gamma, beta, eps = (None, None, 0.0) if norm is None else (norm.weight.detach().cpu().numpy(),
                                                                    norm.bias.detach().cpu().numpy(), norm.eps)
        _, iv_bound, changed = IO.intervene(h.reshape(-1, D).cpu().numpy(), vals, idx, decoder_rows(sae),
                                            sae.decoder.bias.detach().cpu().numpy(), sae.b_pre.detach().cpu().numpy(),
                                            gamma, beta, eps, scale, mode="keep_error")
        c64 = c.double().cpu().numpy()
        effect = (out.double().cpu().numpy() - h.double().cpu().numpy()).reshape(-1, D) @ c64
        total = res.attr.double().cpu().numpy().reshape(-1, k).sum(axis=1)
        bound = iv_bound @ np.abs(c64) + want["attr_bound"].sum(axis=1)
        worst = float(np.max(np.abs(total - effect) / np.maximum(bound, 1e-300)))
        print(f"[attribute] linear metric {precision} norm={with_norm} {label}: rows changed {int(changed.sum())}, "
              f"worst |sum attr - C.(h' - h)| / bound = {worst:.3f}")
        assert changed.any() and np.abs(effect).max() > 0
        assert np.all(np.abs(total - effect) <= bound)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("k", [96, 128])
def test_codes_wider_than_a_wave(k, precision):
    """k > 64: the second code entry per lane (entries 64 .. k - 1), up to the 128 the C ABI accepts."""
    D, H = 384, 1024
    sae = make_sae(D, H, k, precision, seed=k)
    norm = make_norm(D, seed=3)
    h = make_hidden(ROWS_SHAPE, D, seed=k + 1)
    grad = make_grad(ROWS_SHAPE, D, seed=k + 2)
    mixed = mixed_scale_edit(feature_counts(sae, h, norm))
    tag = f"D={D} k={k} {precision}"
    _, res, want = check_case(sae, h, grad, None, norm, label=f"{tag} ablate all")
    assert (want["w"][:, 64:] != 0).any() and float(res.attr[..., 64:].abs().max()) > 0
    check_case(sae, h, grad, mixed, norm, positions=[0, 5, 96], label=f"{tag} mixed scales, row mask")
    check_case(sae, h.to(torch.bfloat16), grad.to(torch.bfloat16), mixed, None, label=f"{tag} mixed scales, no norm")
    check_case(sae, h[:1, :1], grad[:1, :1], None, norm, label=f"{tag} one row")


def test_batch_topk_eval_code():
    """A ``BatchTopKSAE`` goes through its eval-mode threshold selection: rows hold different numbers of active entries."""
    D, H, k = 384, 1024, 8
    sae = make_sae(D, H, k, "bf16", seed=31, cls=BatchTopKSAE)
    norm = make_norm(D, seed=32)
    h = make_hidden(ROWS_SHAPE, D, seed=33)
    grad = make_grad(ROWS_SHAPE, D, seed=34)
    sae.train()
    with torch.no_grad():
        sae(torch.nn.functional.layer_norm(h, (D,), norm.weight, norm.bias, norm.eps))  # trains the threshold
    theta = float(sae.threshold)
    sae.eval()
    assert theta > 0
    _, res, want = check_case(sae, h, grad, None, norm, label="BatchTopK eval, ablate all")
    per_row = (res.vals.reshape(3007, -1) > 0).sum(dim=1)
    assert int(per_row.min()) != int(per_row.max())  # a threshold, not k per row
    check_case(sae, h, grad, mixed_scale_edit(want["feat_rows"]), norm, label="BatchTopK eval, mixed scales")
    assert float(sae.threshold) == theta and sae.training is False


def raw_call(sae, at, h, grad, n_rows, vals, idx, outputs):
    eng = sae.bind()
    handle = eng.prepare(N.PREC_BF16 if sae.precision == "bf16" else N.PREC_FP32, max(h.shape[0], 64), force=True)
    attr, fsum, fabs, frows, ws = outputs
    return eng.lib.wsae_attribute(handle, eng.pack.data_ptr(), h.data_ptr(), _dtype_code(h), grad.data_ptr(),
                                  _dtype_code(grad), n_rows, vals.data_ptr(), idx.data_ptr(), 0, 0.0, 0, 0, attr.data_ptr(),
                                  fsum.data_ptr(), fabs.data_ptr(), frows.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                  eng.stream())


def test_the_library_rejects_more_than_2_26_entries_and_a_short_workspace():
    """Both checks come before the memset node and any launch: the oversized row count is never used as an extent."""
    D, H, k = 64, 256, 32
    sae = make_sae(D, H, k, "fp32", seed=1)
    at = SAEAttribution(sae)
    h = make_hidden((64,), D, seed=2)
    grad = make_grad((64,), D, seed=3)
    res = at.attribute(h, grad)
    vals, idx = res.vals.contiguous(), res.idx.contiguous()
    need = int(N.lib().wsae_attribute_workspace_bytes(H))
    outputs = (torch.zeros(64, k, device=DEV), torch.zeros(H, device=DEV), torch.zeros(H, device=DEV),
               torch.zeros(H, dtype=torch.int32, device=DEV), torch.zeros((need + 7) // 8, dtype=torch.int64, device=DEV))
    assert raw_call(sae, at, h, grad, 64, vals, idx, outputs) == 0
    torch.cuda.synchronize()
    assert torch.equal(outputs[0], res.attr) and torch.equal(outputs[1], res.feat_sum)
    limit = (1 << 26) // k
    assert raw_call(sae, at, h, grad, limit + 1, vals, idx, outputs) == -1
    assert "2^26" in N.last_error() and "wsae_attribute" in N.last_error()
    short = outputs[:4] + (outputs[4][:8],)
    assert raw_call(sae, at, h, grad, 64, vals, idx, short) == -1 and "workspace" in N.last_error()
    torch.cuda.synchronize()
    assert torch.equal(outputs[0], res.attr)  # the refused calls wrote nothing


def test_a_non_finite_gradient_is_propagated_not_hidden():
    """An Inf (or NaN) in ``attr`` cannot go through the fixed-point sums: ``feat_sum`` / ``feat_abs`` are NaN for the whole
    call, ``attr`` carries the non-finite entries themselves and ``feat_rows`` stays exact."""
    D, H, k = 384, 1024, 32
    sae = make_sae(D, H, k, "bf16", seed=5)
    norm = make_norm(D, seed=6)
    h = make_hidden((500,), D, seed=7)
    grad = make_grad((500,), D, seed=8)
    clean = SAEAttribution(sae, layer_norm=norm).attribute(h, grad)
    for bad in (float("inf"), float("nan")):
        g = grad.clone()
        g[17, 5] = bad
        res = SAEAttribution(sae, layer_norm=norm).attribute(h, g)
        assert not bool(torch.isfinite(res.attr[17]).all())
        keep = torch.ones(500, dtype=torch.bool, device=DEV)
        keep[17] = False
        assert torch.equal(res.attr[keep].view(torch.int32), clean.attr[keep].view(torch.int32))
        assert bool(torch.isnan(res.feat_sum).all()) and bool(torch.isnan(res.feat_abs).all())
        assert torch.equal(res.feat_rows, clean.feat_rows)


# ---- end to end on the seeded tiny Whisper -------------------------------------------------------------------------
def tiny_whisper(seed: int = 0):
    from transformers import WhisperConfig, WhisperForConditionalGeneration
    cfg = WhisperConfig(vocab_size=200, num_mel_bins=80, encoder_layers=2, decoder_layers=2, encoder_attention_heads=2,
                        decoder_attention_heads=2, encoder_ffn_dim=128, decoder_ffn_dim=128, d_model=64,
                        max_source_positions=50, max_target_positions=16, decoder_start_token_id=1, pad_token_id=0,
                        bos_token_id=1, eos_token_id=2)
    torch.manual_seed(seed)
    return WhisperForConditionalGeneration(cfg).eval()


class TestTinyWhisper:
    ENC, DEC = ("encoder", 1), ("decoder", 0)

    @pytest.fixture(scope="class")
    def setup(self):
        model = tiny_whisper(0).to(DEV)
        mels = [torch.from_numpy(np.random.default_rng(s).standard_normal((4, 80, 100)).astype(np.float32)).to(DEV)
                for s in (5, 6)]
        ids = torch.tensor([[1, 5, 7]] * 4, device=DEV)
        sae_enc = make_sae(64, 512, 8, "fp32", seed=50)
        sae_dec = make_sae(64, 512, 8, "fp32", seed=51)
        return model, mels, ids, sae_enc, sae_dec

    @staticmethod
    def metric(logits):
        return torch.log_softmax(logits.double(), dim=-1)[:, :, 7].mean()

    @pytest.mark.parametrize("frozen", [False, True])
    def test_compute_equals_the_oracle_and_totals_add_up(self, setup, frozen):
        model, mels, ids, sae_enc, sae_dec = setup
        model.requires_grad_(not frozen)
        try:
            with torch.no_grad():
                plain = model(input_features=mels[0], decoder_input_ids=ids).logits
            taps = {self.ENC: SAEAttribution(sae_enc), self.DEC: SAEAttribution(sae_dec, edit=FeatureEdit.scale(range(0, 512, 2), 0.5))}
            norms = {self.ENC: model.model.encoder.layer_norm, self.DEC: model.model.decoder.layer_norm}
            saes = {self.ENC: sae_enc, self.DEC: sae_dec}
            kept = {t: [] for t in taps}
            with WhisperAttribution(model, taps) as hooked:
                for x in mels:
                    logits = model(input_features=x, decoder_input_ids=ids).logits
                    if x is mels[0]:
                        assert torch.equal(logits.detach().view(torch.int32), plain.view(torch.int32))
                    hooked.backward(self.metric(logits))
                    results = hooked.compute()
                    assert set(results) == set(taps)
                    for tap, res in results.items():
                        h, g = hooked.hidden[tap], hooked.grads[tap]
                        assert h.shape == g.shape == ((4, 50, 64) if tap == self.ENC else (4, 3, 64))
                        want = oracle_for(saes[tap], taps[tap], res, h, g, norms[tap])
                        r_attr = ratio(res.attr, want["attr"], want["attr_bound"])
                        r_sum = ratio(res.feat_sum, want["feat_sum"], want["feat_bound"])
                        r_abs = ratio(res.feat_abs, want["feat_abs"], want["feat_bound"])
                        print(f"[attribute] tiny Whisper {tap} frozen={frozen}: worst error/bound attr {r_attr:.3f}, "
                              f"feat_sum {r_sum:.3f}, feat_abs {r_abs:.3f}")
                        assert max(r_attr, r_sum, r_abs) <= 1.0 and float(res.attr.abs().max()) > 0
                        assert np.array_equal(res.feat_rows.cpu().numpy(), want["feat_rows"])
                        kept[tap].append(res)
            assert all(p.grad is None for p in model.parameters())
            for tap, at in taps.items():
                a, b = kept[tap]
                assert at.calls == 2 and at.total_sum.dtype == torch.float64 and at.total_sum.device.type == "cuda"
                assert torch.equal(at.total_sum, a.feat_sum.double() + b.feat_sum.double())
                assert torch.equal(at.total_abs, a.feat_abs.double() + b.feat_abs.double())
                assert torch.equal(at.total_rows, a.feat_rows.long() + b.feat_rows.long())
                top = at.top(5)
                assert len(top) == 5 and abs(top[0][1]) == float(at.total_sum.abs().max())
                assert [abs(t[1]) for t in top] == sorted((abs(t[1]) for t in top), reverse=True)
                at.reset()
                assert at.total_sum is None and at.calls == 0 and at.top(5) == []
            assert not model.model.encoder.layers[1]._forward_hooks and not model.model.decoder.layers[0]._forward_hooks
        finally:
            model.requires_grad_(True)

    def test_attribution_effects(self, setup):
        model, mels, _, sae_enc, _ = setup
        counts = feature_counts(sae_enc, self.encoder_tap(model, mels[0]), model.model.encoder.layer_norm)
        silent = np.flatnonzero(counts == 0)
        assert silent.size > 0 and (counts > 0).sum() > 8
        full = attribution_effects(model, mels[0], sae_enc, self.ENC)
        assert json.loads(json.dumps(full)) == full and full["tap"] == ["encoder", 1] and full["n_samples"] == 4
        print(f"[attribute] attribution_effects: {len(full['features'])} features, metric {full['metric_value']:.6f}")
        assert set(full["features"]) == {str(f) for f in np.flatnonzero(counts > 0)}  # never-firing features are absent
        for f, entry in full["features"].items():
            assert set(entry) == {"attribution", "abs_attribution", "rows_active"}
            assert np.isfinite(list(entry.values())).all() and entry["abs_attribution"] >= abs(entry["attribution"])
            assert entry["rows_active"] == counts[int(f)] / 200
        everything = attribution_effects(model, mels[0], sae_enc, self.ENC, top_n=512)
        assert json.loads(json.dumps(everything)) == everything and len(everything["features"]) == 512
        for f in silent:
            assert everything["features"][str(f)] == {"attribution": 0.0, "abs_attribution": 0.0, "rows_active": 0.0}
        for f, entry in full["features"].items():
            assert everything["features"][f] == entry
        top = attribution_effects(model, mels[0], sae_enc, self.ENC, top_n=3)
        ranked = sorted(full["features"], key=lambda f: -abs(full["features"][f]["attribution"]))
        assert list(top["features"]) == ranked[:3]
        assert not model.model.encoder.layers[1]._forward_hooks and all(p.grad is None for p in model.parameters())

    def encoder_tap(self, model, x):
        from whisper_sae.causal import ActivationPatch
        patch = ActivationPatch(model, [self.ENC])
        with torch.no_grad():
            patch.record(lambda: model.model.encoder(x))
        return patch.clean[self.ENC]
