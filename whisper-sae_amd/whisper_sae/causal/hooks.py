"""Writing hooks on a Whisper model: feature interventions, layer-level activation patching and ablation effects.

``sae/hooks.py`` (row N2) *reads* a tapped block's output; this module (row N5) *writes* it: one forward hook class,
``_WriteTap``, hands the block's hidden states to a function and **returns** what the function gives back in the
structure the block returned (a tensor, or a tuple with the hidden states first), so the rest of the forward pass runs
on the modified stream.

Unlike the extraction tap, a write tap takes the block's real hidden states for decoder layers too.  The extraction
hook reproduces the reference's ``output[0]`` for decoder layers whatever the layer returns - with decoder layers that
return a bare tensor that selects batch element 0 (golden set G14 pins it) - and a slice like that cannot be written
back; here a bare tensor is the hidden states, for either component.
"""

from __future__ import annotations

from typing import Callable, Optional

import torch
from torch import Tensor

from ..sae.hooks import COMPONENTS
from .edit import FeatureEdit
from .intervention import SAEIntervention


def _check_tap(model, tap) -> tuple:
    component, layer = tap
    if component not in COMPONENTS:
        raise ValueError(f"component must be one of {COMPONENTS}, got {component!r}")
    layers = getattr(model.model, component).layers
    if not 0 <= int(layer) < len(layers):
        raise ValueError(f"{component} layer {layer} does not exist (the model has {len(layers)})")
    return component, int(layer)


class _WriteTap:
    """Forward hook of one tapped block: ``fn(hidden) -> Tensor | None`` (``None`` leaves the output alone)."""

    def __init__(self, tap: tuple, fn: Callable):
        self.tap, self.fn = tap, fn

    def __call__(self, module, inputs, output):
        nested = isinstance(output, (tuple, list))
        hidden = output[0] if nested else output
        new = self.fn(self.tap, hidden)
        if new is None:
            return None
        if nested:
            return type(output)((new, *output[1:])) if isinstance(output, tuple) else [new, *output[1:]]
        return new


class _HookSet:
    """Registration and removal of write taps (context manager)."""

    def __init__(self, model, taps):
        self.model = model
        self.taps = [_check_tap(model, t) for t in taps]
        self._hooks: list = []

    def _fn(self, tap, hidden):  # pragma: no cover - abstract
        raise NotImplementedError

    def register_hooks(self) -> None:
        self.remove_hooks()
        for component, layer in self.taps:
            block = getattr(self.model.model, component).layers[layer]
            self._hooks.append(block.register_forward_hook(_WriteTap((component, layer), self._fn)))

    def remove_hooks(self) -> None:
        while self._hooks:
            self._hooks.pop().remove()

    def __enter__(self):
        self.register_hooks()
        return self

    def __exit__(self, *exc) -> None:
        self.remove_hooks()


class WhisperIntervention(_HookSet):
    """``with WhisperIntervention(model, {("encoder", 2): SAEIntervention(sae, edit)}): model(...)``.

    Every tapped block's output goes through its ``SAEIntervention`` on the way to the next block.
    ``apply_layer_norm=True`` (default) puts the component's final LayerNorm between the hidden states and the SAE,
    exactly as ``WhisperActivationExtractor`` does on extraction, for every intervention that was not given a norm of
    its own; the norm is undone with each row's own statistics, so the model sees its own coordinates.
    ``last_output[tap]`` keeps the modified hidden states of the last forward pass.

    Decoder taps receive the block's real hidden states (all batch elements), not the extraction hook's
    ``output[0]`` (see the module docstring).
    """

    def __init__(self, model, interventions: dict, apply_layer_norm: bool = True):
        super().__init__(model, list(interventions))
        self.interventions = {}
        for tap, intervention in interventions.items():
            if not isinstance(intervention, SAEIntervention):
                raise TypeError(f"tap {tap}: expected an SAEIntervention, got {type(intervention).__name__}")
            self.interventions[_check_tap(model, tap)] = intervention
        self.apply_layer_norm = apply_layer_norm
        self._final_norm = {"encoder": model.model.encoder.layer_norm, "decoder": model.model.decoder.layer_norm}
        self.last_output: dict = {}

    def _fn(self, tap, hidden: Tensor) -> Tensor:
        intervention = self.interventions[tap]
        norm = None
        if self.apply_layer_norm and intervention.layer_norm is None:
            norm = self._final_norm[tap[0]]
        out = intervention.apply(hidden.detach(), layer_norm=norm)
        self.last_output[tap] = out
        return out


class ActivationPatch(_HookSet):
    """Layer-level activation patching: run the model on clean inputs once, then substitute the tapped layers'
    clean outputs into a run on other inputs.

        patch = ActivationPatch(model, [("encoder", 1)])
        patch.record(lambda: model(input_features=clean, decoder_input_ids=ids))
        with patch:
            logits = model(input_features=corrupted, decoder_input_ids=ids).logits

    ``record`` takes a callable that drives the model (or a dict of keyword arguments for ``model(**inputs)``) and
    keeps the tapped outputs where they were produced.  Pure hook plumbing: no kernel is involved, so it works on any
    device.
    """

    def __init__(self, model, taps):
        super().__init__(model, taps)
        self.clean: dict = {}
        self._recording = False

    def _fn(self, tap, hidden: Tensor) -> Optional[Tensor]:
        if self._recording:
            self.clean[tap] = hidden.detach().clone()
            return None
        clean = self.clean.get(tap)
        if clean is None:
            raise RuntimeError(f"tap {tap} has no recorded activation: call record() first")
        if clean.shape != hidden.shape:
            raise ValueError(f"tap {tap}: recorded {tuple(clean.shape)}, this run produced {tuple(hidden.shape)}")
        return clean.to(hidden.dtype)

    @torch.no_grad()
    def record(self, clean_inputs):
        """Run the model on the clean inputs with recording taps; returns what the run returned."""
        self.clean.clear()
        self._recording = True
        try:
            with self:
                return clean_inputs() if callable(clean_inputs) else self.model(**clean_inputs)
        finally:
            self._recording = False


def _first_step(model, input_features: Tensor, decoder_input_ids: Optional[Tensor]) -> tuple:
    """Encoder pass and one decoder pass from the start token (what ``run_whisper_taps`` drives), plus the output
    projection: ``(encoder hidden states, log-probabilities of the first decoder step [B, vocab])``."""
    device = input_features.device
    encoder_hidden = model.model.encoder(input_features).last_hidden_state
    if decoder_input_ids is None:
        decoder_input_ids = torch.full((input_features.size(0), 1), model.config.decoder_start_token_id, dtype=torch.long,
                                       device=device)
    decoded = model.model.decoder(input_ids=decoder_input_ids.to(device), encoder_hidden_states=encoder_hidden)
    logits = model.proj_out(decoded.last_hidden_state[:, 0, :])
    return encoder_hidden, torch.log_softmax(logits.double(), dim=-1)


@torch.no_grad()
def ablation_effects(model, input_features: Tensor, sae, tap, features, decoder_input_ids: Optional[Tensor] = None,
                     apply_layer_norm: bool = True) -> dict:
    """Causal effect of single features: one clean run, then one run per feature with that feature ablated at ``tap``.

    Returns a dict that ``json.dump`` accepts (the reference's output layout calls it ``ablation_results.json``):
    per feature the mean over the batch of ``KL(clean || ablated)`` of the first decoder step's token distribution,
    the relative change of the encoder output ``||enc' - enc|| / ||enc||`` and the fraction of rows the ablation
    touched.  A feature that never fires on the batch leaves the model bit-identical: all three are 0.0.
    """
    tap = _check_tap(model, tap)
    model.eval()
    enc0, logp0 = _first_step(model, input_features, decoder_input_ids)
    p0 = logp0.exp()
    enc_norm = float(enc0.double().norm())
    results = {}
    for f in features:
        intervention = SAEIntervention(sae, FeatureEdit.ablate([int(f)]))
        with WhisperIntervention(model, {tap: intervention}, apply_layer_norm=apply_layer_norm) as hooked:
            enc1, logp1 = _first_step(model, input_features, decoder_input_ids)
            rows = hooked.last_output[tap].numel() // hooked.last_output[tap].shape[-1]
        kl = float((p0 * (logp0 - logp1)).sum(dim=-1).mean())
        rel = float((enc1.double() - enc0.double()).norm()) / enc_norm if enc_norm > 0 else 0.0
        results[str(int(f))] = {"kl": max(kl, 0.0), "encoder_rel_change": rel,
                                "rows_changed": intervention.last_changed_rows / max(rows, 1)}
    return {"tap": [tap[0], tap[1]], "mode": "keep_error", "n_samples": int(input_features.size(0)), "features": results}
