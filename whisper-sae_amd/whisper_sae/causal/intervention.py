"""``SAEIntervention``: edit SAE features inside a tensor of hidden states.

``apply`` is three launches on the caller's stream and never builds a ``[rows, H]`` matrix: ``wsae_layernorm_rows``
(the component's final LayerNorm, what the SAE was trained on) -> the module's own compact code in eval mode
(``wsae_encode_topk``; ``BatchTopKSAE``: its threshold selection) -> ``wsae_intervene``, which turns the edited code
into a change of the hidden states themselves, undoing the LayerNorm with each row's frozen statistics.
"""

from __future__ import annotations

from typing import Iterable, Optional

import torch
from torch import Tensor

from .. import _native as N
from ..sae.engine import _dtype_code, require_device_tensor
from ..sae.model import TopKSAE
from .edit import FeatureEdit

MODES = {"keep_error": N.IV_KEEP_ERROR, "replace": N.IV_REPLACE}


def _norm_parts(layer_norm) -> tuple:
    """``(weight, bias, eps)`` of an ``nn.LayerNorm`` (or of such a triple)."""
    if isinstance(layer_norm, (tuple, list)):
        weight, bias, eps = layer_norm
    else:
        weight, bias, eps = layer_norm.weight, layer_norm.bias, layer_norm.eps
    if weight is None or bias is None:
        raise ValueError("the LayerNorm of an intervention needs both weight and bias")
    return weight, bias, float(eps)


def _positions(positions: Optional[Iterable[int]]) -> Optional[list]:
    if positions is None:
        return None
    out = sorted({int(p) for p in positions})
    if out and out[0] < 0:
        raise ValueError("positions are non-negative indices")
    return out


class _Operands:
    """Device operands shared by the kernels that read hidden states through a LayerNorm (``SAEIntervention``,
    ``SAEAttribution``): the norm's fp32 tensors and the row mask of ``positions``, each built once and cached."""

    def __init__(self, positions: Optional[Iterable[int]] = None):
        self.positions = _positions(positions)
        self._norm_cache: dict = {}
        self._mask_cache: dict = {}

    def norm_tensors(self, layer_norm, device) -> tuple:
        weight, bias, eps = _norm_parts(layer_norm)
        key = (weight.data_ptr(), weight._version, bias.data_ptr(), bias._version, str(device))
        have = self._norm_cache.get(key)
        if have is None:
            gamma = weight.detach().to(device=device, dtype=torch.float32).contiguous()
            beta = bias.detach().to(device=device, dtype=torch.float32).contiguous()
            if bool((gamma == 0).any()):
                raise ValueError("the LayerNorm weight has a zero entry: its inverse does not exist there")
            self._norm_cache.clear()
            have = self._norm_cache[key] = (gamma, beta)
        return have[0], have[1], eps

    def row_mask(self, shape, device) -> Optional[Tensor]:
        if self.positions is None:
            return None
        if len(shape) < 2:
            raise ValueError("positions need hidden states with a time dimension ([.., T, D])")
        key = (tuple(shape[:-1]), str(device))
        mask = self._mask_cache.get(key)
        if mask is None:
            steps = shape[-2]
            if self.positions and self.positions[-1] >= steps:
                raise ValueError(f"position {self.positions[-1]} is outside the {steps} time steps of the hidden states")
            line = torch.zeros(steps, dtype=torch.uint8)
            line[self.positions] = 1
            mask = line.expand(*shape[:-1]).reshape(-1).contiguous().to(device)
            self._mask_cache.clear()
            self._mask_cache[key] = mask
        return mask


class SAEIntervention:
    """Switch features of ``sae`` off, up or to a constant inside hidden states.

    ``layer_norm``: the norm between the hidden states and the SAE's input (Whisper's final encoder / decoder norm, as
    ``sae/hooks.py`` applies it on extraction) - an ``nn.LayerNorm`` or ``(weight, bias, eps)``; ``None``: the SAE reads
    the hidden states as they are.  ``mode``: ``"keep_error"`` adds only the change of the edited features (the SAE's
    reconstruction error stays in the stream; the identity edit is an exact no-op), ``"replace"`` splices the edited
    reconstruction in.  ``positions``: indices along the second-to-last dimension (time) the edit is restricted to.

    ``TopKSAE`` and ``BatchTopKSAE`` only: ReLU SAEs, transcoders and crosscoders raise ``TypeError``.  Runs under
    ``no_grad``; there is no CPU path (``WsaeError``).
    """

    def __init__(self, sae, edit: Optional[FeatureEdit] = None, layer_norm=None, mode: str = "keep_error",
                 positions: Optional[Iterable[int]] = None):
        if not isinstance(sae, TopKSAE):
            raise TypeError(f"interventions run through TopKSAE / BatchTopKSAE codes, not {type(sae).__name__}")
        if mode not in MODES:
            raise ValueError(f"mode must be one of {sorted(MODES)}, got {mode!r}")
        self.sae = sae
        self.edit = FeatureEdit() if edit is None else edit
        if not isinstance(self.edit, FeatureEdit):
            raise TypeError("edit must be a FeatureEdit")
        self.layer_norm = layer_norm
        self.mode = mode
        self._ops = _Operands(positions)
        self.positions = self._ops.positions
        self._changed: Optional[Tensor] = None
        self.last_code = None  # (vals, idx) of the last apply: the code the kernel was handed

    # -- operands --------------------------------------------------------------------------------
    def _norm_tensors(self, layer_norm, device) -> tuple:
        return self._ops.norm_tensors(layer_norm, device)

    def _row_mask(self, shape, device) -> Optional[Tensor]:
        return self._ops.row_mask(shape, device)

    # -- the intervention --------------------------------------------------------------------------
    @torch.no_grad()
    def apply(self, hidden: Tensor, inplace: bool = False, layer_norm=None) -> Tensor:
        """Hidden states ``[.., D]`` with the edit applied (a new tensor, or ``hidden`` itself with ``inplace=True``).
        ``layer_norm`` overrides the one given at construction for this call."""
        require_device_tensor(hidden, "hidden states")
        sae = self.sae
        eng = sae.bind()
        if hidden.device != eng.device:
            raise N.WsaeError(f"hidden states are on {hidden.device}, the SAE on {eng.device}")
        if hidden.shape[-1] != eng.D:
            raise ValueError(f"hidden states have width {hidden.shape[-1]}, the SAE reads {eng.D}")
        direct = hidden.dtype in (torch.float32, torch.bfloat16) and hidden.is_contiguous()
        if inplace and not direct:
            raise ValueError("inplace=True needs contiguous float32 or bfloat16 hidden states")
        h2 = hidden.reshape(-1, eng.D)
        if not direct:
            h2 = (h2 if h2.dtype in (torch.float32, torch.bfloat16) else h2.float()).contiguous()
        rows = h2.shape[0]
        lib = eng.lib
        norm = self.layer_norm if layer_norm is None else layer_norm
        gamma = beta = None
        eps = 0.0
        a = h2
        if norm is not None:
            gamma, beta, eps = self._norm_tensors(norm, eng.device)
            a = torch.empty(rows, eng.D, dtype=torch.float32, device=eng.device)
            N.check(lib.wsae_layernorm_rows(h2.data_ptr(), _dtype_code(h2), rows, eng.D, gamma.data_ptr(), beta.data_ptr(),
                                            eps, a.data_ptr(), N.DT_F32, eng.stream()), "wsae_layernorm_rows")
        _, handle, _, vals, idx = sae._code(a, training=False)
        scale, force_idx, force_val, n_force = self.edit.tables(eng.H, eng.device)
        mask = self._row_mask(hidden.shape, eng.device)
        if self._changed is None or self._changed.device != eng.device:
            self._changed = torch.zeros(1, dtype=torch.int32, device=eng.device)
        out = h2 if inplace else torch.empty_like(h2)
        N.check(lib.wsae_intervene(handle, eng.pack.data_ptr(), h2.data_ptr(), _dtype_code(h2), rows, vals.data_ptr(),
                                   idx.data_ptr(), N.ptr(gamma), N.ptr(beta), eps, scale.data_ptr(), force_idx.data_ptr(),
                                   force_val.data_ptr(), n_force, N.ptr(mask), MODES[self.mode], out.data_ptr(),
                                   _dtype_code(out), self._changed.data_ptr(), eng.stream()), "wsae_intervene")
        eng.generation += 1  # the ctx holds this call's staged batch: an earlier forward must restage before its backward
        self.last_code = (vals, idx)
        if inplace:
            return hidden
        return out.to(hidden.dtype).reshape(hidden.shape)

    __call__ = apply

    @property
    def last_changed_rows(self) -> int:
        """Rows the last ``apply`` wrote with an edit (read from the device counter when asked: one sync then)."""
        return 0 if self._changed is None else int(self._changed.item())
