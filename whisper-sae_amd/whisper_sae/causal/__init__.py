"""Causal validation of SAE features: edit features inside a running Whisper, patch layers.

The reference names this step ("Activation Patching: measure causal importance of layers", an
``ablation_results.json`` in its output layout) and ships a package ``whisper_sae.causal`` that holds a docstring; the
code here is this build's own.

* ``FeatureEdit`` - ablate / scale / clamp features, combined with ``|``;
* ``SAEIntervention`` - apply an edit to a tensor of hidden states through a ``TopKSAE`` / ``BatchTopKSAE``
  (``wsae_layernorm_rows`` -> compact code -> ``wsae_intervene``; no ``[rows, H]`` matrix is ever built);
* ``WhisperIntervention`` - forward hooks that splice interventions into a Whisper forward pass;
* ``ActivationPatch`` - layer-level patching of clean activations into another run;
* ``ablation_effects`` - per-feature KL of the first decoder step and change of the encoder output;
* ``SAEAttribution`` / ``WhisperAttribution`` / ``attribution_effects`` - attribution patching: the first-order effect of
  every feature of every tapped layer from one forward and one backward (``wsae_attribute``).
"""

from .attribution import AttributionResult, SAEAttribution, WhisperAttribution, attribution_effects
from .edit import MAX_FORCED, FeatureEdit
from .hooks import ActivationPatch, WhisperIntervention, ablation_effects
from .intervention import SAEIntervention

__all__ = ["FeatureEdit", "SAEIntervention", "WhisperIntervention", "ActivationPatch", "ablation_effects", "MAX_FORCED",
           "SAEAttribution", "WhisperAttribution", "AttributionResult", "attribution_effects"]
