"""Transcoders for MI355X: same classes, constructor arguments, attributes and state-dict keys as the reference's
``src/whisper_sae/sae/transcoder.py`` (``TopKTranscoder`` :32-252, ``SkipTranscoder`` :255-422, ``create_transcoder``
:425-460), on the TopK-SAE kernels of ``libwsae_hip.so``.

A transcoder is the TopK SAE with three differences: the target of the MSE is a second tensor
(``mlp_output``), there is no pre-encoder bias, and input and output widths may differ.  The kernels take all three
without a new code path:

* ``wsae_encode_topk`` runs on the input, ``wsae_decode_loss`` gets the TARGET as its ``x``, ``wsae_weight_grads`` the
  input again (its ``dW_e`` contraction pairs ``dpre`` with the input rows);
* the pre-bias slot of the parameter pack stays zero and is not a parameter (as for ``ReLUSAE``);
* the engine works at ``D = max(input_dim, output_dim)`` rounded up to 32: narrower tensors are zero-padded on the way
  in, the padded weight columns start at zero and receive exactly zero gradient, and ``wsae_ctx_set_loss_cols`` keeps
  the MSE a mean over the real ``output_dim`` columns.

``SkipTranscoder`` adds the dense affine skip path ``skip(x)``: a plain library GEMM (``torch.nn.functional.linear``)
whose output is subtracted from the target before the sparse path sees it, so ``predicted = decoder(hidden) + skip(x)``
and the gradient of the loss reaches the skip parameters through ordinary autograd.

The binding to the parameter pack, ``encode`` / ``decode``, the dead-feature methods and the autograd node
(``_SparsePath`` with ``mlp_output`` as its target) are the shared ones of ``packed.py``; this file holds the padded
two-width layout and the skip path.

Like the reference, there is no trainer route for these modules: they are trained by the caller's own optimizer loop
(``loss.backward()`` fills ``.grad`` of every parameter through the HIP backward kernels).
"""

from __future__ import annotations

from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F
from torch import Tensor, nn

from .packed import SparseCodeModule


class TranscoderOutput(NamedTuple):
    """What ``forward`` returns (field order of the reference, transcoder.py:21-29)."""

    predicted: Tensor
    hidden: Tensor
    loss: Tensor
    reconstruction_loss: Tensor
    sparsity_loss: Tensor
    l0: Tensor


class _TranscoderBase(SparseCodeModule):
    """What both transcoders (and the crosscoders) share: an input and an output width on one padded parameter pack
    without a pre-encoder bias.  Binding, encode / decode, the sparse path and the dead-feature clock are
    ``SparseCodeModule``'s."""

    def __init__(self, input_dim, output_dim, hidden_dim, k, normalize_decoder, dead_feature_threshold, precision):
        super().__init__()
        self.input_dim, self.output_dim, self.hidden_dim, self.k = input_dim, output_dim, hidden_dim, k
        self.normalize_decoder = normalize_decoder
        self.dead_feature_threshold = dead_feature_threshold
        self.precision = precision

    def _make_linears(self) -> None:
        self.encoder = nn.Linear(self.input_dim, self.hidden_dim, bias=True)
        self.decoder = nn.Linear(self.hidden_dim, self.output_dim, bias=True)

    def _sliced(self, name: str, base: Optional[Tensor] = None) -> Tensor:
        """The reference-shaped view of parameter ``name`` inside the (padded) pack layout of ``base``."""
        v = self._engine.view(name, base)
        if name == "encoder.weight":
            return v[:, :self.input_dim]
        if name == "decoder.weight":
            return v[:self.output_dim, :]
        if name == "decoder.bias":
            return v[:self.output_dim]
        return v

    def _engine_shape(self) -> tuple:
        _, H, k = super()._engine_shape()
        return (max(self.input_dim, self.output_dim) + 31) // 32 * 32, H, k

    def _widths(self) -> tuple:
        return self.input_dim, self.output_dim

    def _mse_cols(self) -> int:
        return self.output_dim

    def extra_repr(self) -> str:
        return f"input_dim={self.input_dim}, output_dim={self.output_dim}, hidden_dim={self.hidden_dim}, k={self.k}"


class TopKTranscoder(_TranscoderBase):
    """TopK transcoder: predicts the MLP output from the MLP input through a k-sparse code (reference
    transcoder.py:32-252).  ``precision`` as for ``TopKSAE``."""

    def __init__(self, input_dim: int, output_dim: int, hidden_dim: int, k: int = 32, normalize_decoder: bool = True,
                 dead_feature_threshold: int = 10_000, precision: Optional[str] = None):
        super().__init__(input_dim, output_dim, hidden_dim, k, normalize_decoder, dead_feature_threshold, precision)
        # same construction (and RNG draw) order as the reference: encoder, decoder, then the decoder initialisation
        self._make_linears()
        with torch.no_grad():  # reference transcoder.py:96-103: xavier -> unit-norm columns -> x0.1
            nn.init.xavier_uniform_(self.decoder.weight)
            self.decoder.weight.data = F.normalize(self.decoder.weight.data, dim=0)
            self.decoder.weight.data *= 0.1
        self._register_clock()

    def forward(self, mlp_input: Tensor, mlp_output: Tensor) -> TranscoderOutput:
        """Reference transcoder.py:142-176.  In training mode also advances the dead-feature clock."""
        pred, hidden, loss, l0 = self._sparse(mlp_input, mlp_output, names=("mlp_input", "mlp_output"))
        return TranscoderOutput(predicted=pred, hidden=hidden, loss=loss, reconstruction_loss=loss,
                                sparsity_loss=torch.zeros((), device=mlp_input.device), l0=l0)

    def resample_dead_features(self, mlp_inputs: Tensor, mlp_outputs: Tensor, num_resample: Optional[int] = None) -> int:
        """Reference transcoder.py:198-252: dead features (ascending, capped) are rewritten from the highest-error
        rows - encoder row = the L2-normalised INPUT row, decoder column = the L2-normalised RESIDUAL row - with the
        reference's quirks (the forward advances the clock in train mode; the capped dead count is returned)."""
        return self._resample_dead(mlp_inputs, mlp_outputs, num_resample)


class SkipTranscoder(_TranscoderBase):
    """Transcoder with an affine skip connection: ``predicted = decoder(hidden) + skip(x)`` (reference
    transcoder.py:255-422).  Decoder and skip start at zero (the reference's "paper" initialisation)."""

    def __init__(self, input_dim: int, output_dim: int, hidden_dim: int, k: int = 32, normalize_decoder: bool = True,
                 dead_feature_threshold: int = 10_000, precision: Optional[str] = None):
        super().__init__(input_dim, output_dim, hidden_dim, k, normalize_decoder, dead_feature_threshold, precision)
        # construction order of the reference: encoder, decoder, skip (then zeros for decoder and skip)
        self._make_linears()
        self.skip = nn.Linear(input_dim, output_dim, bias=True)
        with torch.no_grad():  # reference transcoder.py:314-330
            for p in (self.decoder.weight, self.decoder.bias, self.skip.weight, self.skip.bias):
                p.zero_()
        self._register_clock()

    def set_output_bias(self, mean_output: Tensor) -> None:
        """Decoder bias <- empirical mean of the MLP outputs (reference transcoder.py:332-344)."""
        with torch.no_grad():
            self.decoder.bias.copy_(mean_output.to(self.decoder.bias.device))
        if self._engine is not None:
            self._engine.invalidate()

    def forward(self, mlp_input: Tensor, mlp_output: Tensor) -> TranscoderOutput:
        """Reference transcoder.py:365-403."""
        skip_out = self.skip(mlp_input.float())              # dense affine path: a plain library GEMM
        pred_sparse, hidden, loss, l0 = self._sparse(mlp_input, mlp_output.float() - skip_out,
                                                     names=("mlp_input", "mlp_output"))
        return TranscoderOutput(predicted=pred_sparse + skip_out.detach(), hidden=hidden, loss=loss,
                                reconstruction_loss=loss, sparsity_loss=torch.zeros((), device=mlp_input.device), l0=l0)

    @torch.no_grad()
    def get_skip_contribution(self, mlp_input: Tensor, mlp_output: Tensor) -> float:
        """Fraction of the output variance the skip path alone explains (reference transcoder.py:405-422)."""
        skip_pred = self.skip(mlp_input.float())
        skip_var = ((skip_pred - mlp_output) ** 2).mean()
        total_var = ((mlp_output - mlp_output.mean(dim=0)) ** 2).mean()
        return float((1 - skip_var / (total_var + 1e-8)).item())


def create_transcoder(input_dim: int, output_dim: int, hidden_dim: int, k: int = 32, use_skip: bool = True,
                      **kwargs) -> nn.Module:
    """Reference transcoder.py:425-460."""
    cls = SkipTranscoder if use_skip else TopKTranscoder
    return cls(input_dim=input_dim, output_dim=output_dim, hidden_dim=hidden_dim, k=k, **kwargs)
