"""What every SAE-family module shares: parameters that are views of one ``SAEEngine`` pack, and the two autograd
nodes that drive ``libwsae_hip.so``.

* ``PackedModule``: ``bind()`` / ``param_token()`` / ``normalize_decoder_weights()`` for any module whose parameters
  live in one engine pack.  A subclass declares its parameters (``_named_core_params``), their reference-shaped views
  (``_sliced``), the engine shape (``_engine_shape``), its row widths (``_widths``) and the MSE columns (``_mse_cols``).
* ``SparseCodeModule``: the modules with a compact TopK code and the dead-feature clock (TopK / BatchTopK SAE,
  transcoders, crosscoders): ``_code`` / ``encode`` / ``decode``, the dead-feature scan and the resample routine.
  ``ReLUSAE`` is a ``PackedModule`` only: it has no code, no clock and (as in the reference) none of those methods, which
  is what the trainer and the analysis tools look at to tell the families apart.
* ``_SparsePath``: encode_topk -> decode_loss (-> weight_grads / input_grad in backward) for every TopK family; the target
  of the MSE is the input itself (SAEs) or a second tensor (transcoders, crosscoders).
* ``_ReLUPath``: relu_forward (-> relu_backward), with optional per-feature L1 weights (the ReLU crosscoder).

Both nodes keep the workspace-generation protocol in one place: a ctx holds the staged operands of the LAST batch that
went through it (``SAEEngine.generation``), so a backward whose forward is no longer the last call restages first.
"""

from __future__ import annotations

from contextlib import contextmanager
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F
from torch import Tensor, nn

from .. import _native as N
from .engine import SAEEngine, _dtype_code, require_device_tensor


def _precision_code(precision: Optional[str]) -> int:
    if precision is None:
        precision = "bf16" if torch.is_autocast_enabled() else "fp32"
    if precision in ("bf16", "amp", "fp8"):  # "fp8" (ReLUSAE only): BF16 mode with e4m3 operands in the two forward GEMMs
        return N.PREC_BF16
    if precision == "fp32":
        return N.PREC_FP32
    raise ValueError(f"precision must be 'bf16', 'fp32', 'fp8' (ReLUSAE) or None, got {precision!r}")


def _as_rows(t: Tensor, width: int, padded: int) -> Tensor:
    """``[.., width]`` -> contiguous ``[rows, padded]`` float32 / bfloat16 (zero columns beyond ``width``)."""
    t2 = t.reshape(-1, width)
    if t2.dtype not in (torch.float32, torch.bfloat16):
        t2 = t2.float()
    if padded != width:
        t2 = F.pad(t2, (0, padded - width))
    return t2.contiguous()


class PackedModule(nn.Module):
    """A module whose parameters are views of one engine pack."""

    def __init__(self):
        super().__init__()
        self._engine: Optional[SAEEngine] = None
        self._bound_ptrs = None
        self._last_code = None  # (values, indices) of the last sparse forward

    # -- what a subclass declares ---------------------------------------------------------------------
    def _named_core_params(self):
        return {"encoder.weight": self.encoder.weight, "decoder.weight": self.decoder.weight,
                "encoder.bias": self.encoder.bias, "decoder.bias": self.decoder.bias}

    def _sliced(self, name: str, base: Optional[Tensor] = None) -> Tensor:
        """The reference-shaped view of parameter ``name`` inside the pack layout of ``base`` (default: the pack)."""
        return self._engine.view(name, base)

    def _engine_shape(self) -> tuple:
        """``(D, H, k)`` of the engine: row width, dictionary size and width of the compact code (none here)."""
        return self.input_dim, self.hidden_dim, 1

    def _widths(self) -> tuple:
        """Real widths of ``(input rows, target / output rows)``; the engine may work on a padded width."""
        return self.input_dim, self.input_dim

    def _mse_cols(self) -> int:
        """Columns the reconstruction MSE averages over (``wsae_ctx_set_loss_cols``)."""
        return self._engine.D

    def _clock(self) -> tuple:
        """The dead-feature clock buffers the kernels write (none here)."""
        return ()

    def _l1_weight_grads(self, grads: Tensor, hidden: Tensor, l1: "WeightedL1") -> None:
        """Hook of a ``_ReLUPath`` caller whose L1 weights depend on its parameters: add that term of the gradient to the
        flat buffer ``grads`` (pack layout, before it is scaled by the incoming gradient).  Constant weights: nothing."""

    # -- device binding -------------------------------------------------------------------------------
    def _pointers(self, params) -> tuple:
        return tuple([t.data_ptr() for t in params.values()] + [t.data_ptr() for t in self._clock()])

    def bind(self) -> SAEEngine:
        """Make the parameters views of one device pack (idempotent; re-binds after ``.to()``, ``param.data = ...``
        or anything else that re-pointed a parameter)."""
        params = self._named_core_params()
        anchor = params["encoder.weight"]
        dev = anchor.device
        require_device_tensor(anchor, type(self).__name__)
        shape = self._engine_shape()
        eng = self._engine
        if eng is not None and eng.device == dev and eng.k == shape[2]:
            # fast path (every train step comes through here twice): nothing was re-pointed since the last full check
            if self._pointers(params) == self._bound_ptrs:
                return eng
        else:
            if eng is not None:
                eng.close()
            eng = SAEEngine(dev, *shape)  # (the pack is zero-initialised: padding, an unused pre-bias slot)
            self._engine = eng
        with torch.no_grad():
            for name, p in params.items():
                v = self._sliced(name)
                if p.data_ptr() != v.data_ptr() or p.shape != v.shape or p.stride() != v.stride():
                    v.copy_(p.detach().to(device=dev, dtype=torch.float32))
                    p.data = v
                    eng.invalidate()
        for buf in self._clock():
            if buf.device != dev:
                raise N.WsaeError("module buffers and parameters are on different devices; use module.to(device)")
        # (the views are slices of the engine's pack: equal pointers = same device, shape and stride as checked above)
        self._bound_ptrs = self._pointers(params)
        return eng

    def param_token(self) -> tuple:
        """Changes whenever a parameter was re-pointed or modified in place through autograd-visible ops."""
        return tuple((p.data_ptr(), p._version) for p in self._named_core_params().values())

    def normalize_decoder_weights(self) -> None:
        """Unit-norm decoder columns (always normalises, like the reference's TopK modules)."""
        eng = self.bind()
        handle = eng.ctx(_precision_code(self.precision), 64)
        N.check(eng.lib.wsae_normalize_decoder(handle, eng.pack.data_ptr(), eng.stream()), "wsae_normalize_decoder")
        eng.invalidate()


class SparseCodeModule(PackedModule):
    """A packed module with a compact TopK code ``(values, indices)[B, k]`` and the dead-feature clock."""

    def _register_clock(self) -> None:
        self.register_buffer("feature_last_activated", torch.zeros(self.hidden_dim, dtype=torch.long))
        self.register_buffer("step_count", torch.tensor(0, dtype=torch.long))

    def _clock(self) -> tuple:
        return self.feature_last_activated, self.step_count

    def _engine_shape(self) -> tuple:
        if self.k > self.hidden_dim:
            raise ValueError(f"k={self.k} exceeds hidden_dim={self.hidden_dim}")
        return self.input_dim, self.hidden_dim, self._engine_k()

    def _engine_k(self) -> int:
        """Width of the compact code the kernels produce (the TopK k; BatchTopKSAE: its per-row cap)."""
        return self.k

    def _arm_selection(self, handle: int, mode: Optional[str]) -> None:
        """Hook of BatchTopKSAE (sets the batch-wide selection of the ctx before an encode); otherwise nothing."""

    # -- code -----------------------------------------------------------------------------------------
    def _code(self, x: Tensor, training: bool):
        """Compact code of ``x``: ``(engine, ctx handle, staged rows, values, indices)``."""
        eng = self.bind()
        require_device_tensor(x, "input")
        x2 = _as_rows(x, self._widths()[0], eng.D)
        B = x2.shape[0]
        handle = eng.prepare(_precision_code(self.precision), B, force=True)
        self._arm_selection(handle, "select" if training else "eval")
        vals = torch.empty(B, eng.k, dtype=torch.float32, device=eng.device)
        idx = torch.empty(B, eng.k, dtype=torch.int32, device=eng.device)
        N.check(eng.lib.wsae_encode_topk(handle, eng.pack.data_ptr(), x2.data_ptr(), _dtype_code(x2), 0, B,
                                         vals.data_ptr(), idx.data_ptr(), 0, eng.stats.data_ptr(), eng.stream()),
                "wsae_encode_topk")
        eng.generation += 1  # the ctx now holds THIS batch's staged operands: an earlier forward must restage
        return eng, handle, x2, vals, idx

    @torch.no_grad()
    def encode(self, x: Tensor) -> Tensor:
        """Dense sparse code ``[.., H]`` with at most ``k`` non-zeros per row."""
        eng, handle, x2, vals, idx = self._code(x, self.training)
        hidden = torch.empty(x2.shape[0], eng.H, dtype=torch.float32, device=eng.device)
        N.check(eng.lib.wsae_densify(handle, vals.data_ptr(), idx.data_ptr(), x2.shape[0], hidden.data_ptr(),
                                     eng.stream()), "wsae_densify")
        return hidden.reshape(*x.shape[:-1], eng.H)

    @torch.no_grad()
    def decode(self, hidden: Tensor) -> Tensor:
        """``decoder(hidden)`` (``+ b_pre`` where the module has one) for any dense code."""
        eng = self.bind()
        require_device_tensor(hidden, "hidden")
        h2 = hidden.reshape(-1, eng.H).float().contiguous()
        handle = eng.ctx(_precision_code(self.precision), 64)
        out = torch.empty(h2.shape[0], eng.D, dtype=torch.float32, device=eng.device)
        N.check(eng.lib.wsae_decode_dense(handle, eng.pack.data_ptr(), h2.data_ptr(), h2.shape[0], out.data_ptr(),
                                          eng.stream()), "wsae_decode_dense")
        dout = self._widths()[1]
        return out[:, :dout].reshape(*hidden.shape[:-1], dout)

    def _sparse(self, x: Tensor, target: Optional[Tensor] = None, names=("input", "target")):
        """``(output, hidden, loss, l0)`` of the sparse path; ``target = None``: the target of the MSE is ``x``."""
        self.bind()
        require_device_tensor(x, names[0])
        if target is not None:
            require_device_tensor(target, names[1])
        return _SparsePath.apply(x, target, self, _precision_code(self.precision), *self._named_core_params().values())

    # -- dead features --------------------------------------------------------------------------------
    def _dead_scan(self, eng: SAEEngine, handle: int) -> Tensor:
        mask = torch.empty(eng.H, dtype=torch.uint8, device=eng.device)
        N.check(eng.lib.wsae_dead_scan(handle, self.feature_last_activated.data_ptr(), self.step_count.data_ptr(),
                                       int(self.dead_feature_threshold), mask.data_ptr(), eng.stats.data_ptr(),
                                       eng.stream()), "wsae_dead_scan")
        return mask

    def get_dead_features(self) -> Tensor:
        eng = self.bind()
        return self._dead_scan(eng, eng.ctx(_precision_code(self.precision), 64)).bool()

    def get_dead_feature_ratio(self) -> float:
        self.get_dead_features()
        return float(self._engine.stats_f32()[4].item())

    @torch.no_grad()
    def _resample_dead(self, inputs: Tensor, target: Optional[Tensor], num_resample: Optional[int]) -> int:
        """Dead features (ascending, capped) are rewritten from the highest-error rows: encoder row = the L2-normalised
        input row, decoder column = the same row (no target) or the L2-normalised residual row (target).  With the
        reference's quirks: the forward on ``inputs`` advances the dead-feature clock in train mode, and the returned
        count is the capped number of dead features even when fewer rows than that were available to rewrite them."""
        eng = self.bind()
        require_device_tensor(inputs, "inputs")
        lib, st = eng.lib, eng.stream()
        din, dout = self._widths()
        x2 = _as_rows(inputs, din, eng.D)
        t2 = x2 if target is None else _as_rows(target, dout, eng.D)
        Br = x2.shape[0]
        handle = eng.prepare(_precision_code(self.precision), Br, force=True)
        mask = self._dead_scan(eng, handle)
        if int(eng.stats[5].item()) == 0:  # host decision, as in the reference (model.py:219-220)
            return 0
        training = self.training
        N.check(lib.wsae_ctx_set_loss_cols(handle, self._mse_cols()), "wsae_ctx_set_loss_cols")
        # (data parallel: this forward runs identically on every rank, so its clock stamps need no exchange - keep
        # them out of the indicator buffer that rides on the next gradient all-reduce)
        N.check(lib.wsae_ctx_set_fired(handle, 0), "wsae_ctx_set_fired")
        self._arm_selection(handle, "select" if training else "eval")
        vals = torch.empty(Br, eng.k, dtype=torch.float32, device=eng.device)
        idx = torch.empty(Br, eng.k, dtype=torch.int32, device=eng.device)
        out = torch.empty(Br, eng.D, dtype=torch.float32, device=eng.device)
        pk, xd, td = eng.pack.data_ptr(), _dtype_code(x2), _dtype_code(t2)
        step_ptr = self.step_count.data_ptr() if training else 0
        last_ptr = self.feature_last_activated.data_ptr() if training else 0
        N.check(lib.wsae_encode_topk(handle, pk, x2.data_ptr(), xd, 0, Br, vals.data_ptr(), idx.data_ptr(), step_ptr,
                                     eng.stats.data_ptr(), st), "wsae_encode_topk")
        N.check(lib.wsae_decode_loss(handle, pk, t2.data_ptr(), td, 0, vals.data_ptr(), idx.data_ptr(), Br, out.data_ptr(),
                                     0, 0, last_ptr, step_ptr, eng.stats.data_ptr(), st), "wsae_decode_loss")
        eng.generation += 1
        row_err = torch.empty(Br, dtype=torch.float32, device=eng.device)
        resid = None if target is None else torch.empty(Br, eng.D, dtype=torch.float32, device=eng.device)
        N.check(lib.wsae_row_errors(handle, t2.data_ptr(), td, 0, out.data_ptr(), Br, row_err.data_ptr(), N.ptr(resid), st),
                "wsae_row_errors")
        n_out = torch.zeros(1, dtype=torch.int32, device=eng.device)
        cap = -1 if num_resample is None else int(num_resample)
        N.check(lib.wsae_resample_dead(handle, pk, x2.data_ptr(), xd, 0, Br, row_err.data_ptr(), mask.data_ptr(),
                                       self.feature_last_activated.data_ptr(), self.step_count.data_ptr(), cap,
                                       n_out.data_ptr(), N.ptr(resid), st), "wsae_resample_dead")
        eng.invalidate()
        return int(n_out.item())


class _SparsePath(torch.autograd.Function):
    """encode_topk(input) -> decode_loss(target) (-> weight_grads in backward) as one autograd node.

    Gradients are defined for ``loss`` with respect to the module's parameters (in ``_named_core_params()`` order), the
    input and the target; the output / ``hidden`` / ``l0`` are returned detached.  ``target = None``: the target IS the
    input (one fused encode + decode call, and ``dL/dx`` includes the residual term)."""

    @staticmethod
    def forward(ctx, x, target, module, prec, *params):
        eng: SAEEngine = module._engine
        lib = eng.lib
        din, dout = module._widths()
        x2 = _as_rows(x, din, eng.D)
        t2 = x2 if target is None else _as_rows(target, dout, eng.D)
        B = x2.shape[0]
        if t2.shape[0] != B:
            raise ValueError(f"the input has {B} rows, the target {t2.shape[0]}")
        handle = eng.prepare(prec, B, force=True)
        st = eng.stream()
        training = module.training
        need_bwd = any(ctx.needs_input_grad)
        vals = torch.empty(B, eng.k, dtype=torch.float32, device=eng.device)
        idx = torch.empty(B, eng.k, dtype=torch.int32, device=eng.device)
        out = torch.empty(B, eng.D, dtype=torch.float32, device=eng.device)
        dpre = torch.empty(B, eng.k, dtype=torch.float32, device=eng.device) if need_bwd else None
        step_ptr = module.step_count.data_ptr() if training else 0
        last_ptr = module.feature_last_activated.data_ptr() if training else 0
        pk, xd = eng.pack.data_ptr(), _dtype_code(x2)
        N.check(lib.wsae_ctx_set_loss_cols(handle, module._mse_cols()), "wsae_ctx_set_loss_cols")
        N.check(lib.wsae_ctx_set_fired(handle, 0), "wsae_ctx_set_fired")  # the trainer's DDP clock exchange is per step
        module._arm_selection(handle, "train" if training else "eval")
        # want_bwd: bit 0 = keep g / dpre for the weight gradients, bit 1 = also the fp32 g, which dL/dx reads when the
        # target is the input and d loss / d target otherwise (the skip path trains through it)
        keep_g = ctx.needs_input_grad[0 if target is None else 1]
        want = (1 if need_bwd else 0) | (2 if (need_bwd and keep_g) else 0)
        if target is None:
            N.check(lib.wsae_encode_decode(handle, pk, x2.data_ptr(), xd, 0, B, vals.data_ptr(), idx.data_ptr(), step_ptr,
                                           out.data_ptr(), want, N.ptr(dpre), last_ptr, eng.stats.data_ptr(), st),
                    "wsae_encode_decode")
        else:
            N.check(lib.wsae_encode_topk(handle, pk, x2.data_ptr(), xd, 0, B, vals.data_ptr(), idx.data_ptr(), step_ptr,
                                         eng.stats.data_ptr(), st), "wsae_encode_topk")
            N.check(lib.wsae_decode_loss(handle, pk, t2.data_ptr(), _dtype_code(t2), 0, vals.data_ptr(), idx.data_ptr(), B,
                                         out.data_ptr(), want, N.ptr(dpre), last_ptr, step_ptr, eng.stats.data_ptr(), st),
                    "wsae_decode_loss")
        hidden = torch.empty(B, eng.H, dtype=torch.float32, device=eng.device)
        N.check(lib.wsae_densify(handle, vals.data_ptr(), idx.data_ptr(), B, hidden.data_ptr(), st), "wsae_densify")
        sf = eng.stats_f32()
        loss, l0 = sf[0].clone(), sf[1].clone()
        eng.generation += 1
        ctx.module, ctx.prec, ctx.gen, ctx.B, ctx.keep_g = module, prec, eng.generation, B, keep_g
        ctx.x_shape, ctx.t_shape = x.shape, None if target is None else target.shape
        ctx.save_for_backward(x2, t2, vals, idx, dpre if dpre is not None else vals)
        ctx.has_dpre = dpre is not None
        ctx.set_materialize_grads(False)
        out = out[:, :dout].reshape(*x.shape[:-1], dout)
        hidden = hidden.reshape(*x.shape[:-1], eng.H)
        ctx.mark_non_differentiable(out, hidden, l0)
        module._last_code = (vals, idx)
        return out, hidden, loss, l0

    @staticmethod
    def backward(ctx, g_out, g_hidden, g_loss, g_l0):
        need = ctx.needs_input_grad
        if g_loss is None:
            return (None,) * len(need)
        module, prec, B = ctx.module, ctx.prec, ctx.B
        eng: SAEEngine = module._engine
        lib = eng.lib
        din, dout = module._widths()
        x2, t2, vals, idx, dpre = ctx.saved_tensors
        st = eng.stream()
        handle = eng.prepare(prec, B, force=True)
        pk, xd = eng.pack.data_ptr(), _dtype_code(x2)
        N.check(lib.wsae_ctx_set_loss_cols(handle, module._mse_cols()), "wsae_ctx_set_loss_cols")
        if eng.generation != ctx.gen or not ctx.has_dpre:
            # another call has reused the ctx workspace since: restage this batch (input, then g / dpre from the target)
            tmp_v, tmp_i = torch.empty_like(vals), torch.empty_like(idx)
            dpre = torch.empty_like(vals)
            module._arm_selection(handle, None)  # (restaging only: the saved code is the one the forward selected)
            N.check(lib.wsae_encode_topk(handle, pk, x2.data_ptr(), xd, 0, B, tmp_v.data_ptr(), tmp_i.data_ptr(), 0,
                                         eng.stats.data_ptr(), st), "wsae_encode_topk")
            scratch = torch.zeros(N.STATS_WORDS, dtype=torch.int32, device=eng.device)
            N.check(lib.wsae_decode_loss(handle, pk, t2.data_ptr(), _dtype_code(t2), 0, vals.data_ptr(), idx.data_ptr(), B, 0,
                                         3 if ctx.keep_g else 1, dpre.data_ptr(), 0, 0, scratch.data_ptr(), st),
                    "wsae_decode_loss")
            eng.generation += 1
        grads = torch.empty(eng.P, dtype=torch.float32, device=eng.device)
        N.check(lib.wsae_weight_grads(handle, pk, x2.data_ptr(), xd, 0, vals.data_ptr(), idx.data_ptr(), dpre.data_ptr(), B,
                                      grads.data_ptr(), st), "wsae_weight_grads")
        grads.mul_(g_loss)
        dx = dt = None
        if need[0]:  # (the target is the input: dx = dpre W_e - g, the residual term included)
            dx = torch.empty(B, eng.D, dtype=torch.float32, device=eng.device)
            N.check(lib.wsae_input_grad(handle, pk, idx.data_ptr(), dpre.data_ptr(), B, dx.data_ptr(),
                                        1 if ctx.t_shape is None else 0, st), "wsae_input_grad")
            dx = (dx[:, :din] * g_loss).reshape(ctx.x_shape)
        if need[1]:  # d loss / d target = -g   (g = 2 (output - target) / (B cols): the fp32 copy kept by decode)
            g32 = torch.empty(B, eng.D, dtype=torch.float32, device=eng.device)
            N.check(lib.wsae_last_residual_grad(handle, B, g32.data_ptr(), st), "wsae_last_residual_grad")
            dt = (g32[:, :dout] * (-g_loss)).reshape(ctx.t_shape)
        names = module._named_core_params()
        return (dx, dt, None, None, *(module._sliced(name, grads) if on else None for name, on in zip(names, need[4:])))


class WeightedL1(NamedTuple):
    """Per-feature weights of the L1 term of one ``_ReLUPath`` call, with what goes with them: the columns the MSE
    averages over and the caller's own coefficient (handed back to its ``_l1_weight_grads``)."""

    weights: Tensor
    loss_cols: int
    sparsity_weight: float


@contextmanager
def _relu_ctx(eng: SAEEngine, handle: int, fp8: int, l1: Optional[WeightedL1]):
    """The ctx set up for one ReLU launch sequence; with ``l1`` it is handed back as the ReLU SAE expects it."""
    lib = eng.lib
    N.check(lib.wsae_ctx_set_relu_fp8(handle, fp8), "wsae_ctx_set_relu_fp8")
    if l1 is None:
        yield
        return
    N.check(lib.wsae_ctx_set_loss_cols(handle, l1.loss_cols), "wsae_ctx_set_loss_cols")
    N.check(lib.wsae_ctx_set_relu_l1_weights(handle, l1.weights.data_ptr()), "wsae_ctx_set_relu_l1_weights")
    try:
        yield
    finally:  # the weights are this call's
        lib.wsae_ctx_set_relu_l1_weights(handle, 0)
        lib.wsae_ctx_set_loss_cols(handle, eng.D)


class _ReLUPath(torch.autograd.Function):
    """wsae_relu_forward (-> wsae_relu_backward) as one autograd node; gradients are defined for ``loss`` with respect to
    the four parameters (the reference computes no ``dL/dx`` either).

    ``coef``: coefficient of the kernels' L1 term ``mean_{b,s} w_s |h_bs|``, which is also the ``sparsity`` returned;
    ``fp8``: e4m3 operands in the two forward GEMMs; ``l1``: ``None`` (``w = 1`` and the MSE over the engine width, the
    ctx defaults) or a ``WeightedL1``, whose gradient through the weights ``module._l1_weight_grads`` adds."""

    @staticmethod
    def forward(ctx, x, module, prec, coef, fp8, l1, *params):
        eng: SAEEngine = module._engine
        din = module._widths()[0]
        x2 = _as_rows(x, din, eng.D)
        B = x2.shape[0]
        handle = eng.prepare(prec, B, force=True)
        eng.reserve_relu(handle)
        hidden = torch.empty(B, eng.H, dtype=torch.float32, device=eng.device)
        recon = torch.empty(B, eng.D, dtype=torch.float32, device=eng.device)
        sparsity = torch.empty((), dtype=torch.float32, device=eng.device)
        with _relu_ctx(eng, handle, fp8, l1):
            N.check(eng.lib.wsae_relu_forward(handle, eng.pack.data_ptr(), x2.data_ptr(), _dtype_code(x2), 0, B, coef,
                                              hidden.data_ptr(), recon.data_ptr(), eng.stats.data_ptr(), sparsity.data_ptr(),
                                              eng.stream()), "wsae_relu_forward")
        sf = eng.stats_f32()
        loss, l0 = sf[0].clone(), sf[1].clone()
        eng.generation += 1
        ctx.module, ctx.prec, ctx.gen, ctx.B = module, prec, eng.generation, B
        ctx.coef, ctx.fp8, ctx.l1 = coef, fp8, l1
        ctx.save_for_backward(x2, hidden, recon)
        ctx.set_materialize_grads(False)
        recon = recon[:, :din].reshape(*x.shape[:-1], din)
        hidden = hidden.reshape(*x.shape[:-1], eng.H)
        ctx.mark_non_differentiable(recon, hidden, sparsity, l0)
        return recon, hidden, loss, sparsity, l0

    @staticmethod
    def backward(ctx, g_recon, g_hidden, g_loss, g_sparsity, g_l0):
        need = ctx.needs_input_grad
        if g_loss is None:
            return (None,) * len(need)
        module, prec, B, coef, l1 = ctx.module, ctx.prec, ctx.B, ctx.coef, ctx.l1
        eng: SAEEngine = module._engine
        x2, hidden, recon = ctx.saved_tensors
        handle = eng.prepare(prec, B, force=True)
        eng.reserve_relu(handle)
        lib, st, pk, xd = eng.lib, eng.stream(), eng.pack.data_ptr(), _dtype_code(x2)
        with _relu_ctx(eng, handle, ctx.fp8, l1):
            grads = torch.empty(eng.P, dtype=torch.float32, device=eng.device)
            if eng.generation != ctx.gen:  # another call reused the ctx workspace since: rebuild xT / hidden^T for this batch
                h2, r2 = torch.empty_like(hidden), torch.empty_like(recon)
                N.check(lib.wsae_relu_forward(handle, pk, x2.data_ptr(), xd, 0, B, coef, h2.data_ptr(), r2.data_ptr(), 0, 0, st),
                        "wsae_relu_forward")
                eng.generation += 1
            N.check(lib.wsae_relu_backward(handle, pk, x2.data_ptr(), xd, 0, B, coef, hidden.data_ptr(), recon.data_ptr(),
                                           grads.data_ptr(), st), "wsae_relu_backward")
        if l1 is not None:
            module._l1_weight_grads(grads, hidden, l1)
        grads.mul_(g_loss)
        names = module._named_core_params()
        return (None,) * 6 + tuple(module._sliced(name, grads) if on else None for name, on in zip(names, need[6:]))
