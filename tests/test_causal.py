"""Causal interventions (row N5), the parts that need no GPU: the C ABI's two new symbols, ``FeatureEdit`` tables,
hook registration on a seeded tiny Whisper, layer-level activation patching on the CPU, and the loud failure of the
kernel path on CPU tensors.  The kernel itself is checked on the device in tests/test_gpu_causal.py."""

from __future__ import annotations

import json
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from whisper_sae import _native as N
from whisper_sae.causal import (MAX_FORCED, ActivationPatch, FeatureEdit, SAEIntervention, WhisperIntervention,
                                ablation_effects)
from whisper_sae.sae.model import BatchTopKSAE, ReLUSAE, TopKSAE

ROOT = Path(__file__).resolve().parents[1]


def tiny_whisper(seed: int = 0):
    """The recipe of tests/test_hooks.py."""
    from transformers import WhisperConfig, WhisperForConditionalGeneration
    cfg = WhisperConfig(vocab_size=200, num_mel_bins=80, encoder_layers=2, decoder_layers=2, encoder_attention_heads=2,
                        decoder_attention_heads=2, encoder_ffn_dim=128, decoder_ffn_dim=128, d_model=64,
                        max_source_positions=50, max_target_positions=16, decoder_start_token_id=1, pad_token_id=0,
                        bos_token_id=1, eos_token_id=2)
    torch.manual_seed(seed)
    return WhisperForConditionalGeneration(cfg).eval()


@pytest.fixture(scope="module")
def model():
    return tiny_whisper(0)


def mel(seed: int, batch: int = 3) -> torch.Tensor:
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((batch, 80, 100)).astype(np.float32))


class TestAbi:
    def test_header_declares_and_library_exports_the_two_symbols(self):
        text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "wsae.h").read_text(), flags=re.S)
        declared = set(re.findall(r"\b(wsae_[a-z0-9_]+)\s*\(", text))
        assert {"wsae_intervene", "wsae_layernorm_rows"} <= declared
        assert {"wsae_intervene", "wsae_layernorm_rows"} <= set(N.SIGNATURES)
        lib = N.lib()
        out = subprocess.run(["nm", "-D", "--defined-only", str(N.library_path())], capture_output=True, text=True,
                             check=True).stdout
        exported = set(re.findall(r"\bT (wsae_[a-z0-9_]+)\b", out))
        assert {"wsae_intervene", "wsae_layernorm_rows"} <= exported
        assert lib.wsae_intervene is not None and lib.wsae_layernorm_rows is not None
        assert len(N.SIGNATURES["wsae_intervene"][1]) == 20 and len(N.SIGNATURES["wsae_layernorm_rows"][1]) == 10

    def test_argument_errors_come_before_any_launch(self):
        lib = N.lib()
        assert lib.wsae_layernorm_rows(None, 0, 4, 64, None, None, 1e-5, None, 0, None) == -1
        assert "wsae_layernorm_rows" in N.last_error()
        assert lib.wsae_intervene(None, None, None, 0, 4, None, None, None, None, 0.0, None, None, None, 0, None, 0,
                                  None, 0, None, None) == -1
        assert "wsae_intervene" in N.last_error()


class TestFeatureEdit:
    def test_tables_of_a_combined_edit(self):
        edit = FeatureEdit.ablate([3, 7]) | FeatureEdit.scale(5, 2.5) | FeatureEdit.clamp([9, 2], 4.0)
        scale, force_idx, force_val, n = edit.tables(16, "cpu")
        want = np.ones(16, np.float32)
        want[[3, 7]] = 0.0
        want[5] = 2.5
        np.testing.assert_array_equal(scale.numpy(), want)
        assert n == 2 and force_idx.dtype == torch.int32 and scale.dtype == force_val.dtype == torch.float32
        assert force_idx[:n].tolist() == [9, 2] and force_val[:n].tolist() == [4.0, 4.0]  # list order = sum order
        assert edit.tables(16, "cpu")[0] is scale  # built once per (H, device)
        assert edit.features() == [2, 3, 5, 7, 9] and not edit.is_identity

    def test_identity(self):
        edit = FeatureEdit()
        scale, force_idx, force_val, n = edit.tables(8, "cpu")
        assert edit.is_identity and n == 0 and scale.tolist() == [1.0] * 8
        assert force_idx.numel() >= 1 and force_val.numel() >= 1  # never an empty table behind a pointer
        assert FeatureEdit.scale([1], 1.0).is_identity

    def test_scale_and_clamp_may_share_a_feature(self):
        edit = FeatureEdit.scale(4, 0.5) | FeatureEdit.clamp(4, 2.0)  # the clamp wins in the kernel
        scale, force_idx, force_val, n = edit.tables(8, "cpu")
        assert scale[4] == 0.5 and n == 1 and force_idx[0] == 4 and force_val[0] == 2.0

    def test_duplicates_raise(self):
        with pytest.raises(ValueError, match="twice"):
            FeatureEdit.ablate([1, 2, 1])
        with pytest.raises(ValueError, match="both operands"):
            FeatureEdit.ablate([1]) | FeatureEdit.scale([1], 2.0)
        with pytest.raises(ValueError, match="both operands"):
            FeatureEdit.clamp([6], 1.0) | FeatureEdit.clamp([6], 2.0)

    def test_too_many_forced_features_raise(self):
        assert MAX_FORCED == 64
        FeatureEdit.clamp(range(64), 1.0)
        with pytest.raises(ValueError, match="at most 64"):
            FeatureEdit.clamp(range(65), 1.0)
        with pytest.raises(ValueError, match="at most 64"):
            FeatureEdit.clamp(range(40), 1.0) | FeatureEdit.clamp(range(40, 80), 1.0)

    def test_out_of_range_ids_raise(self):
        with pytest.raises(ValueError, match="negative"):
            FeatureEdit.ablate([-1])
        with pytest.raises(ValueError, match="outside the dictionary"):
            FeatureEdit.ablate([16]).tables(16, "cpu")
        with pytest.raises(ValueError, match="outside the dictionary"):
            FeatureEdit.clamp([99], 1.0).tables(16, "cpu")
        with pytest.raises(ValueError, match="integers"):
            FeatureEdit.ablate([1.5])


class TestSAEIntervention:
    def test_only_topk_codes(self):
        from whisper_sae.sae.crosscoder import create_crosscoder
        from whisper_sae.sae.transcoder import create_transcoder
        SAEIntervention(TopKSAE(64, 128, k=8), FeatureEdit.ablate([1]))
        SAEIntervention(BatchTopKSAE(64, 128, k=8), FeatureEdit.ablate([1]))
        for other in (ReLUSAE(64, 128), create_transcoder(64, 64, 128, k=8), create_crosscoder(64, 2, 128, k=8)):
            with pytest.raises(TypeError):
                SAEIntervention(other, FeatureEdit.ablate([1]))
        with pytest.raises(ValueError, match="mode"):
            SAEIntervention(TopKSAE(64, 128, k=8), FeatureEdit(), mode="zero")

    def test_cpu_tensor_raises_wsae_error(self):
        iv = SAEIntervention(TopKSAE(64, 128, k=8), FeatureEdit.ablate([1]))
        with pytest.raises(N.WsaeError, match="no CPU path"):
            iv.apply(torch.zeros(5, 64))
        assert iv.last_changed_rows == 0


class TestHooks:
    def test_hooks_register_and_are_removed(self, model):
        sae = TopKSAE(64, 128, k=8)
        taps = {("encoder", 1): SAEIntervention(sae, FeatureEdit.ablate([3])),
                ("decoder", 0): SAEIntervention(sae, FeatureEdit())}
        before = [len(model.model.encoder.layers[1]._forward_hooks), len(model.model.decoder.layers[0]._forward_hooks)]
        hooked = WhisperIntervention(model, taps)
        with hooked:
            assert len(model.model.encoder.layers[1]._forward_hooks) == before[0] + 1
            assert len(model.model.decoder.layers[0]._forward_hooks) == before[1] + 1
            assert len(model.model.encoder.layers[0]._forward_hooks) == 0
        assert [len(model.model.encoder.layers[1]._forward_hooks),
                len(model.model.decoder.layers[0]._forward_hooks)] == before
        hooked.register_hooks()
        hooked.register_hooks()  # idempotent
        assert len(model.model.encoder.layers[1]._forward_hooks) == before[0] + 1
        hooked.remove_hooks()
        assert len(model.model.encoder.layers[1]._forward_hooks) == before[0]

    def test_bad_taps_raise(self, model):
        sae = TopKSAE(64, 128, k=8)
        with pytest.raises(ValueError, match="component"):
            WhisperIntervention(model, {("middle", 0): SAEIntervention(sae, FeatureEdit())})
        with pytest.raises(ValueError, match="does not exist"):
            ActivationPatch(model, [("encoder", 2)])
        with pytest.raises(TypeError):
            WhisperIntervention(model, {("encoder", 0): FeatureEdit()})

    def test_a_hooked_cpu_model_fails_loudly_and_cleans_up(self, model):
        """No quiet fall-back: the intervention has no CPU path, and the hooks do not outlive the ``with``."""
        hooked = WhisperIntervention(model, {("encoder", 0): SAEIntervention(TopKSAE(64, 128, k=8), FeatureEdit())})
        with pytest.raises(N.WsaeError):
            with hooked, torch.no_grad():
                model.model.encoder(mel(1))
        assert len(model.model.encoder.layers[0]._forward_hooks) == 0


class TestActivationPatch:
    TAPS = [("encoder", 0), ("encoder", 1), ("decoder", 0), ("decoder", 1)]

    def run(self, model, x):
        ids = torch.tensor([[1, 5, 7]] * x.shape[0])
        with torch.no_grad():
            return model(input_features=x, decoder_input_ids=ids).logits

    def test_patching_every_tap_restores_the_clean_logits(self, model):
        clean, corrupted = mel(10), mel(11)
        logits_clean = self.run(model, clean)
        logits_corrupted = self.run(model, corrupted)
        assert not torch.equal(logits_clean, logits_corrupted)
        patch = ActivationPatch(model, self.TAPS)
        recorded = patch.record(lambda: self.run(model, clean))
        assert torch.equal(recorded, logits_clean) and set(patch.clean) == set(self.TAPS)
        assert patch.clean[("decoder", 1)].shape == (3, 3, 64)  # the block's real hidden states, every batch element
        with patch:
            patched = self.run(model, corrupted)
        assert torch.equal(patched, logits_clean)
        assert torch.equal(self.run(model, corrupted), logits_corrupted)  # hooks gone

    def test_patching_nothing_changes_nothing(self, model):
        clean, corrupted = mel(10), mel(11)
        logits_corrupted = self.run(model, corrupted)
        patch = ActivationPatch(model, [])
        patch.record(lambda: self.run(model, clean))
        with patch:
            assert torch.equal(self.run(model, corrupted), logits_corrupted)

    def test_patching_the_last_encoder_layer_alone_moves_the_logits_towards_clean(self, model):
        clean, corrupted = mel(10), mel(11)
        logits_clean, logits_corrupted = self.run(model, clean), self.run(model, corrupted)
        patch = ActivationPatch(model, [("encoder", 1)])
        patch.record({"input_features": clean, "decoder_input_ids": torch.tensor([[1, 5, 7]] * 3)})
        with patch:
            patched = self.run(model, corrupted)
        # the decoder sees the encoder only through its last layer: patching it is patching the whole encoder
        assert torch.equal(patched, logits_clean) and not torch.equal(patched, logits_corrupted)

    def test_unrecorded_patch_raises(self, model):
        patch = ActivationPatch(model, [("encoder", 0)])
        with pytest.raises(RuntimeError, match="record"):
            with patch:
                self.run(model, mel(3))
        assert len(model.model.encoder.layers[0]._forward_hooks) == 0


def test_ablation_effects_has_no_cpu_path(model):
    with pytest.raises(N.WsaeError):
        ablation_effects(model, mel(2), TopKSAE(64, 128, k=8), ("encoder", 1), [1, 2])
    assert len(model.model.encoder.layers[1]._forward_hooks) == 0
    json.dumps({"features": {}})  # (the result layout itself is checked on the device)
