"""Gradient-based feature attribution (attribution patching).

``ablation_effects`` costs one model forward per feature.  The first-order estimate needs one forward and one backward
for *every* feature of every tapped layer: with ``G = d metric / d h'`` at the tapped block's output, the effect of the
``keep_error`` edit ``h' = h + sigma (sum_j (act'_j - act_j) W_dT[i_j]) / gamma`` on the metric is, per row and code
entry, ``sigma * (act'_j - act_j) * <G / gamma, W_dT[i_j]>`` (``wsae_attribute``).  That is the exact first-order term of
what ``WhisperIntervention`` does - the row statistics are frozen because the intervention freezes them - and not the
derivative through a differentiated LayerNorm.

* ``SAEAttribution`` - ``wsae_layernorm_rows`` -> the module's eval code -> ``wsae_attribute`` on hidden states and a
  gradient; per-entry attributions, per-feature sums and float64 running totals, all on the device;
* ``WhisperAttribution`` - hooks that keep the tapped hidden states of a forward pass and capture their gradient;
* ``attribution_effects`` - the sibling of ``ablation_effects``: a feature table from one forward and one backward.

Out of scope: forced (clamped) features, ``replace`` mode, integrated gradients, ReLU SAEs, transcoders, crosscoders.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Iterable, Optional

import torch
from torch import Tensor

from .. import _native as N
from ..sae.engine import _dtype_code, require_device_tensor
from ..sae.model import TopKSAE
from .edit import FeatureEdit
from .hooks import _check_tap, _first_step, _HookSet
from .intervention import _Operands

METRIC = "mean_logprob_of_clean_argmax_first_decoder_step"


@dataclass
class AttributionResult:
    """What one ``SAEAttribution.attribute`` call computed (device tensors)."""

    attr: Tensor  # [.., k] float32: first-order effect of each code entry
    idx: Tensor  # [.., k] int32: the feature of each entry (the code the kernel was handed)
    vals: Tensor  # [.., k] float32: its activation
    feat_sum: Tensor  # [H] float32: sum of attr per feature
    feat_abs: Tensor  # [H] float32: sum of |attr| per feature
    feat_rows: Tensor  # [H] int32: entries of the feature the edit changes


def _rows(t: Tensor, width: int) -> Tensor:
    t2 = t.reshape(-1, width)
    if t2.dtype not in (torch.float32, torch.bfloat16):
        t2 = t2.float()
    return t2.contiguous()


class SAEAttribution:
    """First-order effect of an edit of ``sae``'s features on a metric, from the metric's gradient.

    ``edit=None`` is the ablation of every feature (each entry's effect is that of switching its feature off on its
    row); a ``FeatureEdit`` with scale factors attributes that edit.  Forced (clamped) features raise ``ValueError``:
    terms outside a row's code are out of scope.  ``layer_norm`` and ``positions`` as in ``SAEIntervention``.

    ``TopKSAE`` and ``BatchTopKSAE`` only (``TypeError`` otherwise).  Runs under ``no_grad``; there is no CPU path
    (``WsaeError``).  ``total_sum`` / ``total_abs`` (float64) and ``total_rows`` (int64) accumulate every call's
    per-feature outputs on the device until ``reset()``.
    """

    def __init__(self, sae, layer_norm=None, edit: Optional[FeatureEdit] = None, positions: Optional[Iterable[int]] = None):
        if not isinstance(sae, TopKSAE):
            raise TypeError(f"attribution runs through TopKSAE / BatchTopKSAE codes, not {type(sae).__name__}")
        if edit is not None:
            if not isinstance(edit, FeatureEdit):
                raise TypeError("edit must be a FeatureEdit (or None: ablate every feature)")
            if edit.forced:
                raise ValueError(f"features {sorted(edit.forced)} are clamped: attribution covers scale edits only "
                                 f"(a forced term outside a row's code is out of scope)")
        self.sae = sae
        self.edit = edit
        self.layer_norm = layer_norm
        self._ops = _Operands(positions)  # norm tensors and row mask, built as the intervention builds them
        self.positions = self._ops.positions
        self._workspace: Optional[Tensor] = None
        self.total_sum: Optional[Tensor] = None
        self.total_abs: Optional[Tensor] = None
        self.total_rows: Optional[Tensor] = None
        self.calls = 0

    # -- running totals ----------------------------------------------------------------------------
    def reset(self) -> None:
        self.total_sum = self.total_abs = self.total_rows = None
        self.calls = 0

    def _accumulate(self, result: AttributionResult) -> None:
        if self.total_sum is None or self.total_sum.device != result.feat_sum.device:
            self.total_sum = torch.zeros_like(result.feat_sum, dtype=torch.float64)
            self.total_abs = torch.zeros_like(result.feat_abs, dtype=torch.float64)
            self.total_rows = torch.zeros_like(result.feat_rows, dtype=torch.int64)
        self.total_sum += result.feat_sum
        self.total_abs += result.feat_abs
        self.total_rows += result.feat_rows
        self.calls += 1

    def top(self, n: int) -> list:
        """The ``n`` features with the largest ``|total_sum|``: ``[(feature, total_sum, total_abs, total_rows)]``."""
        if self.total_sum is None:
            return []
        n = min(int(n), self.total_sum.numel())
        order = torch.argsort(self.total_sum.abs(), descending=True, stable=True)[:n]
        rows = zip(order.tolist(), self.total_sum[order].tolist(), self.total_abs[order].tolist(),
                   self.total_rows[order].tolist())
        return [(int(f), float(s), float(a), int(c)) for f, s, a, c in rows]

    # -- the attribution ---------------------------------------------------------------------------
    @torch.no_grad()
    def attribute(self, hidden: Tensor, grad: Tensor, layer_norm=None) -> AttributionResult:
        """``hidden [.., D]``: the tapped hidden states of the clean run; ``grad``: the metric's gradient with respect to
        them (same shape).  ``layer_norm`` overrides the one given at construction for this call."""
        require_device_tensor(hidden, "hidden states")
        require_device_tensor(grad, "the gradient")
        sae = self.sae
        eng = sae.bind()
        if hidden.device != eng.device or grad.device != eng.device:
            raise N.WsaeError(f"hidden states are on {hidden.device}, the gradient on {grad.device}, the SAE on {eng.device}")
        if hidden.shape != grad.shape:
            raise ValueError(f"hidden states {tuple(hidden.shape)} and gradient {tuple(grad.shape)} differ in shape")
        if hidden.shape[-1] != eng.D:
            raise ValueError(f"hidden states have width {hidden.shape[-1]}, the SAE reads {eng.D}")
        h2, g2 = _rows(hidden, eng.D), _rows(grad, eng.D)
        rows = h2.shape[0]
        lib = eng.lib
        norm = self.layer_norm if layer_norm is None else layer_norm
        gamma = None
        eps = 0.0
        a = h2
        if norm is not None:
            gamma, beta, eps = self._ops.norm_tensors(norm, eng.device)
            a = torch.empty(rows, eng.D, dtype=torch.float32, device=eng.device)
            N.check(lib.wsae_layernorm_rows(h2.data_ptr(), _dtype_code(h2), rows, eng.D, gamma.data_ptr(), beta.data_ptr(),
                                            eps, a.data_ptr(), N.DT_F32, eng.stream()), "wsae_layernorm_rows")
        _, handle, _, vals, idx = sae._code(a, training=False)
        scale = None if self.edit is None else self.edit.tables(eng.H, eng.device)[0]
        mask = self._ops.row_mask(hidden.shape, eng.device)
        need = int(lib.wsae_attribute_workspace_bytes(eng.H))
        if self._workspace is None or self._workspace.device != eng.device or self._workspace.numel() * 8 < need:
            self._workspace = torch.empty((need + 7) // 8, dtype=torch.int64, device=eng.device)
        attr = torch.empty(rows, eng.k, dtype=torch.float32, device=eng.device)
        feat_sum = torch.empty(eng.H, dtype=torch.float32, device=eng.device)
        feat_abs = torch.empty(eng.H, dtype=torch.float32, device=eng.device)
        feat_rows = torch.empty(eng.H, dtype=torch.int32, device=eng.device)
        N.check(lib.wsae_attribute(handle, eng.pack.data_ptr(), h2.data_ptr(), _dtype_code(h2), g2.data_ptr(),
                                   _dtype_code(g2), rows, vals.data_ptr(), idx.data_ptr(), N.ptr(gamma), eps, N.ptr(scale),
                                   N.ptr(mask), attr.data_ptr(), feat_sum.data_ptr(), feat_abs.data_ptr(),
                                   feat_rows.data_ptr(), self._workspace.data_ptr(), self._workspace.numel() * 8,
                                   eng.stream()), "wsae_attribute")
        eng.generation += 1  # the ctx holds this call's staged batch: an earlier forward must restage before its backward
        lead = hidden.shape[:-1]
        result = AttributionResult(attr.reshape(*lead, eng.k), idx.reshape(*lead, eng.k), vals.reshape(*lead, eng.k),
                                   feat_sum, feat_abs, feat_rows)
        self._accumulate(result)
        return result

    __call__ = attribute


class WhisperAttribution(_HookSet):
    """Capture the tapped hidden states of a forward pass and the gradient a metric sends back to them:

        with WhisperAttribution(model, {("encoder", 2): SAEAttribution(sae)}) as hooked:
            metric = f(model(...))
            metric.backward()          # or hooked.backward(metric): gradients of the taps only
            results = hooked.compute() # {tap: AttributionResult}

    A tapped output that requires grad is left untouched and gets a tensor hook.  One that does not (a frozen model)
    is replaced by a detached leaf that does, so the forward is differentiable from the tap onwards and nothing before
    it is.  Either way the values the rest of the forward pass sees are the block's own: the logits are bit-identical
    to the unhooked model's.  ``apply_layer_norm`` as in ``WhisperIntervention``.  The hooks are plain torch; only
    ``compute()`` needs the device.  The graph tensors of the taps are dropped by ``compute()`` and when the hooks are
    removed; ``clear()`` also drops the kept hidden states and gradients.
    """

    def __init__(self, model, attributions: dict, apply_layer_norm: bool = True):
        super().__init__(model, list(attributions))
        self.attributions = {}
        for tap, attribution in attributions.items():
            if not isinstance(attribution, SAEAttribution):
                raise TypeError(f"tap {tap}: expected an SAEAttribution, got {type(attribution).__name__}")
            self.attributions[_check_tap(model, tap)] = attribution
        self.apply_layer_norm = apply_layer_norm
        self._final_norm = {"encoder": model.model.encoder.layer_norm, "decoder": model.model.decoder.layer_norm}
        self.hidden: dict = {}  # tap -> hidden states of the last forward pass (detached)
        self.grads: dict = {}  # tap -> their gradient, once a backward pass has reached them
        self._tapped: dict = {}  # tap -> the tensor in the graph

    def _fn(self, tap, hidden: Tensor) -> Optional[Tensor]:
        self.grads.pop(tap, None)
        self.hidden[tap] = hidden.detach()
        replaced = not hidden.requires_grad
        node = hidden.detach().requires_grad_(True) if replaced else hidden
        self._tapped[tap] = node

        def keep(grad: Tensor, tap=tap) -> None:
            self.grads[tap] = grad.detach()

        node.register_hook(keep)
        return node if replaced else None

    def remove_hooks(self) -> None:
        super().remove_hooks()
        self._tapped.clear()  # the graph from the taps onwards goes with the hooks; hidden / grads stay for compute()

    def clear(self) -> None:
        """Drop the kept hidden states, gradients and graph tensors."""
        self.hidden.clear()
        self.grads.clear()
        self._tapped.clear()

    def backward(self, metric: Tensor) -> None:
        """Gradients of ``metric`` with respect to the tapped outputs only: no parameter's ``.grad`` is touched."""
        taps = [t for t in self.taps if t in self._tapped]
        if not taps:
            raise RuntimeError("no tapped forward pass to differentiate: run the model inside the hooks first")
        grads = torch.autograd.grad(metric, [self._tapped[t] for t in taps], allow_unused=True)
        for tap, grad in zip(taps, grads):
            if grad is not None:
                self.grads[tap] = grad.detach()

    def compute(self) -> dict:
        """``{tap: AttributionResult}`` from the kept hidden states and the captured gradients."""
        results = {}
        for tap in self.taps:
            if tap not in self.grads or tap not in self.hidden:
                raise RuntimeError(f"tap {tap} has no gradient: run the model inside the hooks with grad enabled and "
                                   f"call metric.backward() before compute()")
            attribution = self.attributions[tap]
            norm = None
            if self.apply_layer_norm and attribution.layer_norm is None:
                norm = self._final_norm[tap[0]]
            results[tap] = attribution.attribute(self.hidden[tap], self.grads[tap], layer_norm=norm)
        self._tapped.clear()  # the gradients are in: nothing needs the graph any more
        return results


def attribution_effects(model, input_features: Tensor, sae, tap, decoder_input_ids: Optional[Tensor] = None,
                        top_n: Optional[int] = None, apply_layer_norm: bool = True) -> dict:
    """First-order effect of ablating each feature of ``sae`` at ``tap``: one forward and one backward in all.

    The metric is the batch mean of the first decoder step's log-probability of the clean run's argmax token.  Returns
    a dict that ``json.dump`` accepts: per feature the summed attribution (the estimated change of the metric when the
    feature is ablated everywhere), the summed ``|attribution|`` and the fraction of rows that hold the feature; every
    feature that fires on the batch, or the ``top_n`` largest by ``|attribution|`` (a feature that never fires is then
    exactly 0.0).  ``ablation_effects`` confirms the top few exactly.
    """
    tap = _check_tap(model, tap)
    model.eval()
    attribution = SAEAttribution(sae)
    with WhisperAttribution(model, {tap: attribution}, apply_layer_norm=apply_layer_norm) as hooked:
        with torch.enable_grad():
            _, logp = _first_step(model, input_features, decoder_input_ids)
            token = logp.detach().argmax(dim=-1, keepdim=True)
            metric = logp.gather(1, token).mean()
            hooked.backward(metric)
        result = hooked.compute()[tap]
    rows = max(result.attr.numel() // max(result.attr.shape[-1], 1), 1)
    if top_n is None:
        chosen = torch.nonzero(result.feat_rows > 0).flatten()
    else:
        chosen = torch.argsort(result.feat_sum.abs(), descending=True, stable=True)[:max(int(top_n), 0)]
    table = zip(chosen.tolist(), result.feat_sum[chosen].tolist(), result.feat_abs[chosen].tolist(),
                result.feat_rows[chosen].tolist())
    features = {str(int(f)): {"attribution": float(s), "abs_attribution": float(a), "rows_active": int(n) / rows}
                for f, s, a, n in table}
    return {"tap": [tap[0], tap[1]], "metric": METRIC, "metric_value": float(metric.detach()),
            "n_samples": int(input_features.size(0)), "features": features}
