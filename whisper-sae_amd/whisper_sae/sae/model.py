"""SAE modules for MI355X: same classes, constructor arguments, attributes and state-dict keys as
the reference's ``src/whisper_sae/sae/model.py``, with the arithmetic in ``libwsae_hip.so``.

* ``TopKSAE``  (reference model.py:26-257)  encode -> TopK -> sparse decode -> MSE, dead-feature
  tracking and resampling, all as HIP kernels working on a compact ``(values, indices)[B, k]`` code;
  the dense ``hidden [B, H]`` tensor of ``SAEOutput`` is materialised only for API callers.
* ``BatchTopKSAE`` (not in the reference; its V2 requirements ask for it): the TopK path with a batch-wide
  selection of the ``B * k`` largest activations and a learned inference threshold.
* ``ReLUSAE``  (reference model.py:260-322).
* ``create_sae`` (reference model.py:325-354), additionally forwarding ``config.sparsity_weight``.

What the families share (the binding of the parameters to one engine pack, the compact-code methods, the dead-feature
routines and the two autograd nodes) lives in ``packed.py``; this file holds what is each class's own.

Host-side torch is used for tensor storage, initial random initialisation (same RNG draw order as
the reference, so ``torch.manual_seed(s)`` gives the same initial weights) and autograd plumbing.
There is no CPU compute path: tensors must live on a ROCm device or ``WsaeError`` is raised.
"""

from __future__ import annotations

from typing import NamedTuple, Optional

import torch
from torch import Tensor, nn

from .. import _native as N
from ..config import SAEConfig
from .engine import SAEEngine, _dtype_code, require_device_tensor
from .packed import PackedModule, SparseCodeModule, _as_rows, _precision_code, _ReLUPath


class SAEOutput(NamedTuple):
    """What ``forward`` returns (field order of the reference, model.py:15-23)."""

    reconstructed: Tensor
    hidden: Tensor
    loss: Tensor
    reconstruction_loss: Tensor
    sparsity_loss: Tensor
    l0: Tensor


def relu_fp8_flag(module) -> int:
    """1 when the module asks for the fp8 forward (``ReLUSAE(precision="fp8")``, BASELINE.json configs[4])."""
    return 1 if getattr(module, "precision", None) == "fp8" else 0


class TopKSAE(SparseCodeModule):
    """TopK sparse autoencoder (reference model.py:26-257).

    ``precision``: ``"bf16"`` (bf16 MFMA contractions, fp32 accumulate -- what ``use_amp`` selects in
    the trainer), ``"fp32"`` (fp32 MFMA, the reference's CPU semantics) or ``None`` = follow
    ``torch.autocast`` (bf16 inside an autocast region, fp32 otherwise).
    """

    def __init__(self, input_dim: int, hidden_dim: int, k: int = 32, normalize_decoder: bool = True,
                 dead_feature_threshold: int = 10_000, precision: Optional[str] = None):
        super().__init__()
        self.input_dim = input_dim
        self.hidden_dim = hidden_dim
        self.k = k
        self.normalize_decoder = normalize_decoder
        self.dead_feature_threshold = dead_feature_threshold
        self.precision = precision
        # same construction (and RNG draw) order as the reference: encoder, decoder, xavier(decoder.weight)
        self.encoder = nn.Linear(input_dim, hidden_dim, bias=True)
        self.decoder = nn.Linear(hidden_dim, input_dim, bias=True)
        self.b_pre = nn.Parameter(torch.zeros(input_dim))
        with torch.no_grad():  # reference model.py:79-89: xavier -> unit-norm columns -> x0.1
            nn.init.xavier_uniform_(self.decoder.weight)
            w = self.decoder.weight.data
            self.decoder.weight.data = w / w.norm(dim=0, keepdim=True).clamp_min(1e-12) * 0.1
        self._register_clock()

    def _named_core_params(self):
        return {"encoder.weight": self.encoder.weight, "decoder.weight": self.decoder.weight,
                "encoder.bias": self.encoder.bias, "decoder.bias": self.decoder.bias, "b_pre": self.b_pre}

    # -- reference API -----------------------------------------------------------------------------
    @torch.no_grad()
    def encode_compact(self, x: Tensor):
        """TopK code without the dense scatter: ``(values [B,k] f32 pre-activations, indices [B,k] i32)``."""
        _, _, _, vals, idx = self._code(x, self.training)
        return vals, idx

    @torch.no_grad()
    def pre_activation(self, x: Tensor) -> Tensor:
        """Dense ``encoder(x - b_pre)`` [B, H] (reference model.py:108-111)."""
        eng = self.bind()
        require_device_tensor(x, "input")
        x2 = _as_rows(x, eng.D, eng.D)
        B = x2.shape[0]
        handle = eng.prepare(_precision_code(self.precision), B, force=True)
        pre = torch.empty(B, eng.H, dtype=torch.float32, device=eng.device)
        N.check(eng.lib.wsae_encode_dense(handle, eng.pack.data_ptr(), x2.data_ptr(), _dtype_code(x2), 0, B,
                                          pre.data_ptr(), eng.stream()), "wsae_encode_dense")
        eng.generation += 1
        return pre.reshape(*x.shape[:-1], eng.H)

    def forward(self, x: Tensor) -> SAEOutput:
        """Reference model.py:131-166.  In training mode also advances the dead-feature clock."""
        recon, hidden, loss, l0 = self._sparse(x)
        return SAEOutput(reconstructed=recon, hidden=hidden, loss=loss, reconstruction_loss=loss,
                         sparsity_loss=torch.zeros((), device=x.device), l0=l0)

    def resample_dead_features(self, inputs: Tensor, num_resample: Optional[int] = None) -> int:
        """Reference model.py:197-257 (``SparseCodeModule._resample_dead`` with the inputs as their own target)."""
        return self._resample_dead(inputs, None, num_resample)

    def extra_repr(self) -> str:
        return f"input_dim={self.input_dim}, hidden_dim={self.hidden_dim}, k={self.k}"


class BatchSelection(NamedTuple):
    """Record of the last batch-wide selection of a ``BatchTopKSAE`` (``last_selection()``)."""

    threshold: float      # t: the smallest kept value (theta in eval mode once trained); -1 when nothing was positive
    saturated_rows: int   # rows whose max_k_per_row-th candidate was kept (0 when max_k_per_row = hidden_dim)
    kept: int             # entries kept in the batch


def default_max_k_per_row(k: int, hidden_dim: int) -> int:
    """Per-row cap of ``BatchTopKSAE`` when none is given: ``min(2 k, 128, hidden_dim)`` (2 k keeps k = 32 on the
    MFMA decode, which serves code widths up to 64)."""
    return min(2 * int(k), 128, int(hidden_dim))


class BatchTopKSAE(TopKSAE):
    """BatchTopK sparse autoencoder (Bussmann, Leask & Nanda 2024).

    Training mode keeps the ``B * k`` largest positive pre-activations of the whole batch instead of ``k`` per row,
    with at most ``max_k_per_row`` per row (the candidates are the per-row TopK of that width); rows with more signal get
    more latents.  Every training-mode ``forward`` moves the scalar ``threshold`` (a buffer, in the state dict) towards
    the batch's cut ``t``: ``t`` itself the first time, then ``threshold_beta * threshold + (1 - threshold_beta) * t``.
    Eval mode keeps the candidates above ``threshold`` (JumpReLU style, independent of the batch), or selects over the
    batch while ``threshold`` is still -1 (never trained).  ``encode``, ``encode_compact`` and
    ``resample_dead_features`` select the same way by ``self.training`` but leave ``threshold`` unchanged.  The
    selection runs on the device between the TopK and the decode launches; the rest of the step is ``TopKSAE``'s.
    """

    def __init__(self, input_dim: int, hidden_dim: int, k: int = 32, max_k_per_row: Optional[int] = None,
                 threshold_beta: float = 0.999, normalize_decoder: bool = True, dead_feature_threshold: int = 10_000,
                 precision: Optional[str] = None):
        super().__init__(input_dim, hidden_dim, k=k, normalize_decoder=normalize_decoder,
                         dead_feature_threshold=dead_feature_threshold, precision=precision)
        cap = default_max_k_per_row(k, hidden_dim) if max_k_per_row is None else int(max_k_per_row)
        if not 1 <= k <= cap <= min(128, hidden_dim):
            raise ValueError(f"BatchTopKSAE needs 1 <= k <= max_k_per_row <= min(128, hidden_dim), got k={k}, "
                             f"max_k_per_row={cap}, hidden_dim={hidden_dim}")
        if not 0.0 <= float(threshold_beta) < 1.0:
            raise ValueError(f"threshold_beta must be in [0, 1), got {threshold_beta}")
        self.max_k_per_row = cap
        self.threshold_beta = float(threshold_beta)
        self.register_buffer("threshold", torch.tensor(-1.0, dtype=torch.float32))
        self._btk_state: Optional[Tensor] = None  # device record wsae_batch_topk_state; `threshold` is a view of word 0
        self._btk_beta: Optional[float] = None

    def _engine_k(self) -> int:
        return self.max_k_per_row

    def bind(self) -> SAEEngine:
        eng = super().bind()
        rec = self._btk_state
        if rec is None or rec.device != eng.device or self.threshold.data_ptr() != rec.data_ptr():
            rec = torch.zeros(N.BTK_STATE_WORDS, dtype=torch.int32, device=eng.device)
            f = rec.view(torch.float32)
            with torch.no_grad():
                f[0].copy_(self.threshold.detach().reshape(()))
                f[2].fill_(-1.0)
            self._btk_state = rec
            self.threshold = f[0]  # the buffer becomes a view of the record the kernels update
            self._btk_beta = None
        if self._btk_beta != self.threshold_beta:
            rec.view(torch.float32)[1].fill_(self.threshold_beta)
            self._btk_beta = self.threshold_beta
        return eng

    def _arm_selection(self, handle: int, mode: Optional[str]) -> None:
        """mode: "train" (select, update the threshold), "select" (select only), "eval", or None (off)."""
        if mode is None:
            kb, code, rec = 0, N.BTK_TRAIN, 0
        else:
            kb, code = self.k, {"train": N.BTK_TRAIN, "eval": N.BTK_EVAL, "select": N.BTK_SELECT}[mode]
            rec = self._btk_state.data_ptr()
        N.check(self._engine.lib.wsae_ctx_set_batch_topk(handle, kb, code, rec), "wsae_ctx_set_batch_topk")

    def last_selection(self) -> BatchSelection:
        """(t, saturated rows, kept entries) of the last selection on this module.  Read from the device record only
        when called (one sync then); the selection itself never waits for the host."""
        if self._btk_state is None:
            return BatchSelection(-1.0, 0, 0)
        rec = self._btk_state.cpu()
        return BatchSelection(float(rec.view(torch.float32)[2]), int(rec[3]), int(rec[4]))

    def extra_repr(self) -> str:
        return (f"input_dim={self.input_dim}, hidden_dim={self.hidden_dim}, k={self.k}, "
                f"max_k_per_row={self.max_k_per_row}, threshold_beta={self.threshold_beta}")


class ReLUSAE(PackedModule):
    """ReLU + L1 sparse autoencoder (reference model.py:260-322).

    No ``b_pre``, default ``nn.Linear`` initialisation with (optionally) unit-norm decoder columns; the
    loss is ``mse + sparsity_weight * mean|hidden|``.  The kernels (``wsae_relu_forward/backward``) run on
    the TopK parameter pack with the pre-bias slot held at zero.  Unlike the reference (whose trainer
    crashes on it) it can be trained by ``SAETrainer``: there is no dead-feature
    bookkeeping for this module, as in the reference.
    """

    is_relu = True

    def __init__(self, input_dim: int, hidden_dim: int, sparsity_weight: float = 0.01,
                 normalize_decoder: bool = True, precision: Optional[str] = None):
        super().__init__()
        self.input_dim = input_dim
        self.hidden_dim = hidden_dim
        self.sparsity_weight = sparsity_weight
        self.normalize_decoder = normalize_decoder
        self.precision = precision
        self.encoder = nn.Linear(input_dim, hidden_dim)
        self.decoder = nn.Linear(hidden_dim, input_dim)
        if normalize_decoder:
            with torch.no_grad():  # reference model.py:285-286 (F.normalize(dim=0))
                w = self.decoder.weight.data
                self.decoder.weight.data = w / w.norm(dim=0, keepdim=True).clamp_min(1e-12)

    def normalize_decoder_weights(self) -> None:
        """Unit-norm decoder columns when ``normalize_decoder`` is set (reference model.py:296-302)."""
        if not self.normalize_decoder:
            return
        super().normalize_decoder_weights()

    def forward(self, x: Tensor) -> SAEOutput:
        """Reference model.py:304-322."""
        self.bind()
        require_device_tensor(x, "input")
        prec = _precision_code(self.precision)
        recon, hidden, loss, sparsity, l0 = _ReLUPath.apply(x, self, prec, float(self.sparsity_weight), relu_fp8_flag(self),
                                                            None, *self._named_core_params().values())
        return SAEOutput(reconstructed=recon, hidden=hidden, loss=loss,
                         reconstruction_loss=(loss - self.sparsity_weight * sparsity).detach(),
                         sparsity_loss=sparsity, l0=l0)

    def extra_repr(self) -> str:
        return f"input_dim={self.input_dim}, hidden_dim={self.hidden_dim}, sparsity_weight={self.sparsity_weight}"


def create_sae(config: SAEConfig, input_dim: int) -> nn.Module:
    """Build the SAE a config describes (reference model.py:325-354)."""
    hidden_dim = config.get_hidden_dim(input_dim)
    if config.activation == "batchtopk":
        return BatchTopKSAE(input_dim=input_dim, hidden_dim=hidden_dim, k=config.k,
                            max_k_per_row=config.batch_topk_max_k, threshold_beta=config.batch_topk_threshold_beta,
                            normalize_decoder=config.normalize_decoder,
                            dead_feature_threshold=config.dead_feature_threshold)
    if config.activation == "topk":
        return TopKSAE(input_dim=input_dim, hidden_dim=hidden_dim, k=config.k,
                       normalize_decoder=config.normalize_decoder,
                       dead_feature_threshold=config.dead_feature_threshold)
    # "relu" and (as in the reference) "gelu" both map to the ReLU SAE
    return ReLUSAE(input_dim=input_dim, hidden_dim=hidden_dim, sparsity_weight=config.sparsity_weight,
                   normalize_decoder=config.normalize_decoder)
