"""Causal interventions on the device (row N5): ``wsae_layernorm_rows`` + ``wsae_intervene`` against the float64
oracle of tests/intervention_oracle.py, the exact no-op of the identity edit, and the hooks on a seeded tiny Whisper.

The oracle is always handed the code the product selected (``SAEIntervention.last_code``), so no case depends on the
order of near-ties and no row is excluded.  The tolerance is the oracle's own element-wise bound (its docstring), plus
one bf16 ulp of the result where the output is bf16; every case prints the worst ratio error / bound it met.
"""

from __future__ import annotations

import json

import numpy as np
import pytest
import torch

import intervention_oracle as IO
from whisper_sae import _native as N
from whisper_sae.causal import ActivationPatch, FeatureEdit, SAEIntervention, WhisperIntervention, ablation_effects
from whisper_sae.sae.engine import _dtype_code
from whisper_sae.sae.model import BatchTopKSAE, TopKSAE

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROWS_SHAPE = (31, 97)  # 3007 rows: a multiple of nothing the kernels tile by


def make_sae(D, H, k, precision, seed=0, cls=TopKSAE, **kw):
    torch.manual_seed(seed)
    sae = cls(D, H, k=k, precision=precision, **kw)
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


def oracle_for(sae, iv, h, norm, out_dtype=None):
    vals, idx = (t.cpu().numpy() for t in iv.last_code)
    scale, fidx, fval, n = iv.edit.tables(sae.hidden_dim, DEV)
    mask = None if iv.positions is None else iv._row_mask(h.shape, torch.device(DEV)).cpu().numpy()
    gamma = beta = None
    eps = 0.0
    if norm is not None:
        gamma, beta, eps = norm.weight.detach().cpu().numpy(), norm.bias.detach().cpu().numpy(), norm.eps
    want, bound, changed = IO.intervene(
        h.reshape(-1, h.shape[-1]).float().cpu().numpy(), vals, idx, decoder_rows(sae),
        sae.decoder.bias.detach().cpu().numpy(), sae.b_pre.detach().cpu().numpy(), gamma, beta, eps,
        scale.cpu().numpy(), fidx[:n].cpu().tolist(), fval[:n].cpu().tolist(), mask, iv.mode)
    if (out_dtype or h.dtype) == torch.bfloat16:
        bound = bound + IO.bf16_ulp(want)
    return want, bound, changed


def worst_ratio(got: torch.Tensor, want: np.ndarray, bound: np.ndarray) -> float:
    g = got.reshape(want.shape).float().cpu().numpy().astype(np.float64)
    assert np.isfinite(g).all()
    return float((np.abs(g - want) / bound).max())


def check_case(sae, h, edit, norm, mode, positions=None, label=""):
    iv = SAEIntervention(sae, edit, layer_norm=norm, mode=mode, positions=positions)
    out = iv.apply(h)
    assert out.shape == h.shape and out.dtype == h.dtype and out.data_ptr() != h.data_ptr()
    want, bound, changed = oracle_for(sae, iv, h, norm)
    ratio = worst_ratio(out, want, bound)
    n_changed = iv.last_changed_rows
    print(f"[intervene] {label} mode={mode} dtype={h.dtype} rows={want.shape[0]} changed={n_changed} "
          f"worst error/bound={ratio:.3f}")
    assert ratio <= 1.0, f"{label}: error is {ratio:.3f} x the derived bound"
    assert n_changed == int(changed.sum())
    if mode == "keep_error":  # rows without an edit are bit-identical copies
        same = torch.from_numpy(~changed).to(DEV)
        assert torch.equal(out.reshape(-1, h.shape[-1])[same], h.reshape(-1, h.shape[-1])[same])
    return iv, out


def feature_counts(sae, h, norm) -> np.ndarray:
    iv = SAEIntervention(sae, FeatureEdit(), layer_norm=norm)
    iv.apply(h)
    vals, idx = (t.cpu().numpy() for t in iv.last_code)
    return np.bincount(idx[vals > 0].ravel(), minlength=sae.hidden_dim)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("k", [8, 32, 64])
@pytest.mark.parametrize("D", [64, 384, 768, 1280])
def test_kernel_matches_the_oracle(D, k, precision):
    H = 1024
    sae = make_sae(D, H, k, precision, seed=D + k)
    norm = make_norm(D, seed=D)
    h = make_hidden(ROWS_SHAPE, D, seed=k)
    counts = feature_counts(sae, h, norm)
    fa, fi = int(counts.argmax()), int(counts.argmin())  # on most rows' code / on (almost) none
    assert counts[fa] > 0 and fa != fi
    cases = [("ablate active", FeatureEdit.ablate([fa]), norm, None),
             ("scale+clamp same feature, ablate inactive",
              FeatureEdit.scale([fa], 0.5) | FeatureEdit.clamp([fa], 2.0) | FeatureEdit.ablate([fi]), norm, None),
             ("clamp inactive", FeatureEdit.clamp([fi], 1.5), norm, None)]
    if D == 384:
        cases += [("scale active and inactive", FeatureEdit.scale([fa], 2.5) | FeatureEdit.scale([fi], 0.25), norm, None),
                  ("clamp active", FeatureEdit.clamp([fa], 3.0), norm, None),
                  ("ablate inactive", FeatureEdit.ablate([fi]), norm, None),
                  ("row mask", FeatureEdit.ablate([fa]) | FeatureEdit.clamp([fi], 1.0), norm, [0, 5, 96]),
                  ("no norm", FeatureEdit.ablate([fa]) | FeatureEdit.clamp([fi], 1.0), None, None)]
    for label, edit, nm, positions in cases:
        for mode in ("keep_error", "replace"):
            check_case(sae, h, edit, nm, mode, positions, label=f"D={D} k={k} {precision} {label}")
    # bf16 hidden states in and out, and a single row
    hb = make_hidden(ROWS_SHAPE, D, seed=k + 1, dtype=torch.bfloat16)
    for mode in ("keep_error", "replace"):
        check_case(sae, hb, cases[1][1], norm, mode, label=f"D={D} k={k} {precision} bf16")
        check_case(sae, h[:1, :1], cases[1][1], norm, mode, label=f"D={D} k={k} {precision} one row")
    check_case(sae, hb[:1, :1], FeatureEdit.clamp([fi], 1.5), None, "keep_error", label=f"D={D} k={k} {precision} one bf16 row")


@pytest.mark.parametrize("h_dtype,out_dtype", [(torch.float32, torch.bfloat16), (torch.bfloat16, torch.float32)])
def test_kernel_converts_between_dtypes(h_dtype, out_dtype):
    """The C entry point takes any pair of input and output dtypes (``SAEIntervention`` keeps the input's)."""
    D, H, k = 384, 1024, 32
    sae = make_sae(D, H, k, "bf16", seed=5)
    norm = make_norm(D, seed=6)
    h = make_hidden(ROWS_SHAPE, D, seed=7, dtype=h_dtype)
    counts = feature_counts(sae, h, norm)
    edit = FeatureEdit.ablate([int(counts.argmax())]) | FeatureEdit.clamp([int(counts.argmin())], 1.0)
    for mode in ("keep_error", "replace"):
        iv = SAEIntervention(sae, edit, layer_norm=norm, mode=mode)
        iv.apply(h)  # leaves the code and the prepared ctx
        eng = sae.bind()
        handle = eng.prepare(N.PREC_BF16, 3007, force=True)
        vals, idx = iv.last_code
        gamma, beta, eps = iv._norm_tensors(norm, eng.device)
        scale, fidx, fval, n = edit.tables(H, DEV)
        h2 = h.reshape(-1, D)
        out = torch.empty(3007, D, dtype=out_dtype, device=DEV)
        changed = torch.full((1,), -1, dtype=torch.int32, device=DEV)
        N.check(eng.lib.wsae_intervene(handle, eng.pack.data_ptr(), h2.data_ptr(), _dtype_code(h2), 3007, vals.data_ptr(),
                                       idx.data_ptr(), gamma.data_ptr(), beta.data_ptr(), eps, scale.data_ptr(),
                                       fidx.data_ptr(), fval.data_ptr(), n, 0, N.IV_KEEP_ERROR if mode == "keep_error"
                                       else N.IV_REPLACE, out.data_ptr(), _dtype_code(out), changed.data_ptr(),
                                       eng.stream()), "wsae_intervene")
        want, bound, ch = oracle_for(sae, iv, h, norm, out_dtype=out_dtype)
        ratio = worst_ratio(out, want, bound)
        print(f"[intervene] {h_dtype} -> {out_dtype} mode={mode} worst error/bound={ratio:.3f}")
        assert ratio <= 1.0 and int(changed.item()) == int(ch.sum())
        if mode == "keep_error":  # untouched rows are the conversion of the input, nothing else
            same = torch.from_numpy(~ch).to(DEV)
            assert torch.equal(out[same], h2[same].to(out_dtype))
        # an in-place call cannot change the dtype
        rc = eng.lib.wsae_intervene(handle, eng.pack.data_ptr(), h2.data_ptr(), _dtype_code(h2), 3007, vals.data_ptr(),
                                    idx.data_ptr(), 0, 0, 0.0, 0, 0, 0, 0, 0, 0, h2.data_ptr(), _dtype_code(out), 0,
                                    eng.stream())
        assert rc == -1 and "in-place" in N.last_error()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_identity_edit_is_an_exact_no_op(precision, dtype):
    D, H, k = 384, 1024, 32
    sae = make_sae(D, H, k, precision, seed=1)
    norm = make_norm(D, seed=2)
    h = make_hidden(ROWS_SHAPE, D, seed=3, dtype=dtype)
    keep = h.clone()
    for edit in (FeatureEdit(), FeatureEdit.scale([5, 9], 1.0)):
        iv = SAEIntervention(sae, edit, layer_norm=norm)
        out = iv.apply(h)
        bits = torch.int16 if dtype == torch.bfloat16 else torch.int32
        assert out.data_ptr() != h.data_ptr() and torch.equal(out.view(bits), keep.view(bits))
        assert iv.last_changed_rows == 0
        same = iv.apply(h, inplace=True)
        assert same is h and torch.equal(h, keep) and iv.last_changed_rows == 0
    # a row mask that selects nothing makes any edit the identity
    iv = SAEIntervention(sae, FeatureEdit.ablate(range(0, H, 2)), layer_norm=norm, positions=[])
    assert torch.equal(iv.apply(h), keep) and iv.last_changed_rows == 0


def test_two_runs_are_bit_identical_and_in_place_equals_out_of_place():
    D, H, k = 768, 1024, 32
    sae = make_sae(D, H, k, "bf16", seed=11)
    norm = make_norm(D, seed=12)
    h = make_hidden(ROWS_SHAPE, D, seed=13)
    counts = feature_counts(sae, h, norm)
    order = np.argsort(-counts)
    edit = (FeatureEdit.ablate(order[:3].tolist()) | FeatureEdit.scale(order[3:6].tolist(), 1.7)
            | FeatureEdit.clamp(order[-5:].tolist() + [int(order[6])], 2.0))
    for mode in ("keep_error", "replace"):
        iv = SAEIntervention(sae, edit, layer_norm=norm, mode=mode)
        first = iv.apply(h)
        n1 = iv.last_changed_rows
        second = iv.apply(h)
        assert torch.equal(first.view(torch.int32), second.view(torch.int32)) and n1 == iv.last_changed_rows > 0
        assert not torch.equal(first, h)
        work = h.clone()
        assert iv.apply(work, inplace=True) is work
        assert torch.equal(work.view(torch.int32), first.view(torch.int32))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_identity_replace_is_the_reconstruction(precision):
    """``replace`` with the identity edit and no norm splices ``sae(x).reconstructed`` in."""
    D, H, k = 384, 1024, 32
    sae = make_sae(D, H, k, precision, seed=21)
    x = make_hidden(ROWS_SHAPE, D, seed=22)
    iv = SAEIntervention(sae, FeatureEdit(), mode="replace")
    out = iv.apply(x)
    want, bound, changed = oracle_for(sae, iv, x, None)
    assert changed.all() and iv.last_changed_rows == 3007
    with torch.no_grad():
        recon = sae(x).reconstructed
    ratio_oracle = worst_ratio(out, want, bound)
    ratio_recon = worst_ratio(out, recon.reshape(-1, D).float().cpu().numpy().astype(np.float64), bound)
    print(f"[intervene] identity replace {precision}: vs oracle {ratio_oracle:.3f}, vs sae(x).reconstructed {ratio_recon:.3f} "
          f"(x the derived bound)")
    assert ratio_oracle <= 1.0 and ratio_recon <= 1.0


def test_layernorm_rows_is_the_ring_producers_layernorm():
    """``wsae_layernorm_rows`` and ``wsae_ring_push_layernorm`` run one kernel: the same bits, for every dtype pair."""
    from whisper_sae.data.feature_cache import ActivationRing
    lib = N.lib()
    for D in (64, 384, 1280):
        norm = make_norm(D, seed=D)
        gamma, beta = norm.weight.detach().contiguous(), norm.bias.detach().contiguous()
        st = torch.cuda.current_stream(DEV).cuda_stream
        for src_dtype in (torch.float32, torch.bfloat16):
            h = make_hidden((203,), D, seed=D + 1, dtype=src_dtype)
            for dst_dtype in (torch.float32, torch.bfloat16):
                dst = torch.empty(203, D, dtype=dst_dtype, device=DEV)
                N.check(lib.wsae_layernorm_rows(h.data_ptr(), _dtype_code(h), 203, D, gamma.data_ptr(), beta.data_ptr(),
                                                norm.eps, dst.data_ptr(), _dtype_code(dst), st), "wsae_layernorm_rows")
                ring = ActivationRing(256, D, device=DEV, dtype=dst_dtype)
                ring.push_layernorm(h, norm.weight, norm.bias, norm.eps)
                assert torch.equal(ring.data[:203], dst)
                ref = torch.nn.functional.layer_norm(h.float(), (D,), gamma, beta, norm.eps)
                tol = 2e-2 if dst_dtype == torch.bfloat16 else 1e-5
                assert torch.allclose(dst.float(), ref, atol=tol * float(ref.abs().max()), rtol=0)


def test_batch_topk_eval_threshold_selection():
    D, H, k = 384, 1024, 8
    sae = make_sae(D, H, k, "bf16", seed=31, cls=BatchTopKSAE)
    norm = make_norm(D, seed=32)
    h = make_hidden(ROWS_SHAPE, D, seed=33)
    sae.train()
    with torch.no_grad():
        sae(torch.nn.functional.layer_norm(h, (D,), norm.weight, norm.bias, norm.eps))  # trains the threshold
    theta = float(sae.threshold)
    assert theta > 0
    counts = None
    for training in (False, True):
        sae.train(training)
        iv = SAEIntervention(sae, FeatureEdit(), layer_norm=norm)
        iv.apply(h)
        vals, idx = iv.last_code
        assert sae.training is training and float(sae.threshold) == theta
        # the per-row candidates with the selection switched off, and the threshold applied to them by hand
        eng = sae.bind()
        lib = eng.lib
        a_k = torch.empty(3007, D, dtype=torch.float32, device=DEV)
        N.check(lib.wsae_layernorm_rows(h.data_ptr(), N.DT_F32, 3007, D, norm.weight.data_ptr(), norm.bias.data_ptr(),
                                        norm.eps, a_k.data_ptr(), N.DT_F32, eng.stream()), "wsae_layernorm_rows")
        handle = eng.prepare(N.PREC_BF16, 3007, force=True)
        sae._arm_selection(handle, None)
        cand = torch.empty(3007, eng.k, dtype=torch.float32, device=DEV)
        cidx = torch.empty(3007, eng.k, dtype=torch.int32, device=DEV)
        N.check(lib.wsae_encode_topk(handle, eng.pack.data_ptr(), a_k.data_ptr(), N.DT_F32, 0, 3007, cand.data_ptr(),
                                     cidx.data_ptr(), 0, eng.stats.data_ptr(), eng.stream()), "wsae_encode_topk")
        eng.generation += 1
        expect = torch.where((cand > 0) & (cand > theta), cand, torch.zeros_like(cand))
        assert torch.equal(idx, cidx) and torch.equal(vals, expect)
        per_row = (vals > 0).sum(dim=1)
        assert int(per_row.min()) != int(per_row.max())  # a threshold, not k per row
        counts = np.bincount(idx[vals > 0].cpu().numpy().ravel(), minlength=H)
    sae.eval()
    edit = FeatureEdit.ablate([int(counts.argmax())]) | FeatureEdit.clamp([int(counts.argmin())], 1.0)
    for mode in ("keep_error", "replace"):
        check_case(sae, h, edit, norm, mode, label="BatchTopK eval")
    assert float(sae.threshold) == theta and sae.training is False


def test_intervention_between_two_train_steps_changes_nothing():
    from whisper_sae.config import TrainingConfig
    from whisper_sae.sae.training import SAETrainer
    import tempfile
    D, H, k, B = 384, 1024, 32, 256
    x1, x2 = make_hidden((B,), D, seed=41), make_hidden((B,), D, seed=42)
    h = make_hidden((200,), D, seed=43)
    norm = make_norm(D, seed=44)
    packs = []
    for intervene in (False, True):
        sae = make_sae(D, H, k, "bf16", seed=40)
        with tempfile.TemporaryDirectory(prefix="wsae_causal_") as run_dir:
            trainer = SAETrainer(sae, TrainingConfig(batch_size=B, learning_rate=1e-3, warmup_steps=0, use_amp=True,
                                                     num_workers=0), device=DEV, run_dir=run_dir)
            trainer.train_step(x1)
            if intervene:
                gen = sae._engine.generation
                out = SAEIntervention(sae, FeatureEdit.ablate([1, 2, 3]), layer_norm=norm).apply(h)
                assert sae._engine.generation > gen and out.shape == h.shape and sae.training
            trainer.train_step(x2)
            torch.cuda.synchronize()
            packs.append((sae._engine.pack.clone(), sae.feature_last_activated.clone(), int(sae.step_count)))
    assert torch.equal(packs[0][0], packs[1][0]) and torch.equal(packs[0][1], packs[1][1]) and packs[0][2] == packs[1][2]


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
        mel = torch.from_numpy(np.random.default_rng(5).standard_normal((4, 80, 100)).astype(np.float32)).to(DEV)
        ids = torch.tensor([[1, 5, 7]] * 4, device=DEV)
        sae_enc = make_sae(64, 512, 8, "fp32", seed=50)
        sae_dec = make_sae(64, 512, 8, "fp32", seed=51)
        return model, mel, ids, sae_enc, sae_dec

    @staticmethod
    def logits(model, mel, ids):
        with torch.no_grad():
            return model(input_features=mel, decoder_input_ids=ids).logits

    def test_identity_hooks_leave_the_logits_bit_identical(self, setup):
        model, mel, ids, sae_enc, sae_dec = setup
        plain = self.logits(model, mel, ids)
        taps = {self.ENC: SAEIntervention(sae_enc, FeatureEdit()), self.DEC: SAEIntervention(sae_dec, FeatureEdit())}
        with WhisperIntervention(model, taps) as hooked:
            hooked_logits = self.logits(model, mel, ids)
        assert set(hooked.last_output) == {self.ENC, self.DEC}
        assert hooked.last_output[self.ENC].shape == (4, 50, 64) and hooked.last_output[self.DEC].shape == (4, 3, 64)
        assert torch.equal(hooked_logits.view(torch.int32), plain.view(torch.int32))
        assert taps[self.ENC].last_changed_rows == 0 and taps[self.DEC].last_changed_rows == 0
        assert torch.equal(self.logits(model, mel, ids), plain) and not model.model.encoder.layers[1]._forward_hooks

    def test_ablating_the_most_frequent_feature(self, setup):
        model, mel, ids, sae_enc, _ = setup
        plain = self.logits(model, mel, ids)
        patch = ActivationPatch(model, [self.ENC])
        patch.record(lambda: self.logits(model, mel, ids))
        h = patch.clean[self.ENC]  # the block's own output
        norm = model.model.encoder.layer_norm
        counts = feature_counts(sae_enc, h, norm)
        feature = int(counts.argmax())
        assert counts[feature] > 0
        iv = SAEIntervention(sae_enc, FeatureEdit.ablate([feature]))
        with WhisperIntervention(model, {self.ENC: iv}) as hooked:
            ablated = self.logits(model, mel, ids)
        assert not torch.equal(ablated, plain) and bool(torch.isfinite(ablated).all())
        assert iv.last_changed_rows == int(counts[feature])
        iv.layer_norm = norm  # (what the hook passed per call; the oracle helper reads the edit, the code and the mode)
        want, bound, changed = oracle_for(sae_enc, iv, h, norm)
        ratio = worst_ratio(hooked.last_output[self.ENC], want, bound)
        print(f"[intervene] tiny Whisper encoder layer 1, feature {feature}: worst error/bound={ratio:.3f}")
        assert ratio <= 1.0 and int(changed.sum()) == int(counts[feature])

    def test_ablation_effects(self, setup):
        model, mel, _, sae_enc, _ = setup
        patch = ActivationPatch(model, [self.ENC])
        with torch.no_grad():
            patch.record(lambda: model.model.encoder(mel))
        counts = feature_counts(sae_enc, patch.clean[self.ENC], model.model.encoder.layer_norm)
        silent = np.flatnonzero(counts == 0)
        assert silent.size > 0
        firing, never = int(counts.argmax()), int(silent[0])
        result = ablation_effects(model, mel, sae_enc, self.ENC, [firing, never])
        assert json.loads(json.dumps(result)) == result and result["tap"] == ["encoder", 1]
        print(f"[intervene] ablation_effects: {json.dumps(result)}")
        for entry in result["features"].values():
            assert all(np.isfinite(v) and v >= 0.0 for v in entry.values())
        hit, miss = result["features"][str(firing)], result["features"][str(never)]
        assert hit["kl"] > 0.0 and hit["encoder_rel_change"] > 0.0 and hit["rows_changed"] > 0.0
        assert miss == {"kl": 0.0, "encoder_rel_change": 0.0, "rows_changed": 0.0}
        assert not model.model.encoder.layers[1]._forward_hooks
