"""One ``wsae_ctx`` across batch sizes, dtypes and intruding calls (case tables: tests/ctx_history_cases.py).

Every other GPU parity test builds a fresh module per case, whose ctx is created for exactly the batch under test, zeroed
at creation and used once.  Here a ctx is sized by a larger batch first and then serves the *victim* (one training forward
+ backward) after, or around, other work.  Determinism is part of the contract (no float atomics), so every
comparison is BIT EQUALITY (``torch.equal`` on integer views) between the *undisturbed* run - a fresh module doing only the
victim - and the *history* run on a module with the same weights: loss, l0, output, ``hidden``, ``_last_code``, the
gradient of every parameter, ``x.grad`` / ``target.grad`` where the family defines them, the clock buffers, BatchTopK's
``threshold`` and ``last_selection()``.  No tolerance is introduced here.

* anchor: once per victim with B <= 2320 the undisturbed run is held to the float64 oracle with the family's own helpers
  and bounds (tests/test_gpu_kernel_variants.py, test_gpu_batch_topk.py, test_transcoder.py, test_crosscoder.py,
  test_gpu_relu_step.py), so the equalities below hang on something.  The two chunked-decode victims (V3, V4: B >= 64 x
  CUs) run no CPU oracle: their undisturbed configuration - 384 -> 3072, k = 32, bf16, chunked decode, presorted wgrad2s,
  with and without a ragged last chunk - is held to the oracle by test_gpu_kernel_variants.py rows r14 / r18 / r19;
* determinism: two undisturbed runs on two fresh modules are bit-identical (the precondition of everything else);
* part A: a victim after a history equals the victim on a fresh ctx;
* part B: victim forward, intruder, victim backward: the restage protocol of sae/packed.py;
* part C: an epoch with a ragged batch through ``SAETrainer`` on one ctx and on a fresh ctx per step;
* part D: the control - without the restage the backward really reads the intruder's state.

Witnesses: the ctx handle is the same from before the history to after the victim where the table says "kept".  Where it
says "replaced" the handle value is no witness - the allocator gives the new ctx the address of the one just destroyed
(seen on the MI355X in every such case) - so the cap and ``SAEEngine.generation`` are held instead: ``SAEEngine.ctx``
replaces the ctx exactly when the cap grows, and counts the new one.  The launch counts of the built-in kernel timing prove the path (a restaged backward,
a presorted chunked victim without a ``bucket`` launch, a direct-gather victim without a ``stage_batch`` launch).

A history that ran in training mode advanced the module's clock buffers (and BatchTopK's ``threshold``): they are module
state, not ctx state, and are put back to the fresh values with ``copy_`` before the victim.

``last_selection()`` in part B: every selection - ``encode_compact`` and the causal tools included - writes the record
(``wsae_batch_topk.hip``: ``last_t``, ``saturated_rows``, ``kept``), so after a selecting intruder it is the intruder's by
definition.  What the restage owes is to leave it alone: the record after the backward equals the record right after the
intruder, and equals the undisturbed run's where the intruder selects nothing (``pre_activation``); ``threshold`` equals
the undisturbed run's after every intruder that does not train.
"""

from __future__ import annotations

import functools
import types

import numpy as np
import pytest
import torch

import batch_topk_oracle as BO
import ctx_history_cases as T
import test_crosscoder as TC
import test_gpu_batch_topk as BT
import test_gpu_relu_step as RS
import test_transcoder as TT
from oracle import sae_oracle as O
from oracle import synth
from test_gpu_kernel_variants import DX_REL, GRAD_REL, LOSS_REL, RECON_REL, check, make, oracle_step, run, to_device, weights  # noqa: F401

pytestmark = pytest.mark.gpu

SEED = 61
DT = {"bf16": torch.bfloat16, "fp32": torch.float32}
OTHER = {"bf16": "fp32", "fp32": "bf16"}


def cus() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


def victims() -> dict:
    return {v.vid: v for v in T.victims(cus())}


# -- pure tables: the ids do not depend on the device ------------------------------------------------------------------
VIDS = [v.vid for v in T.victims(256)]
ANCHORED = [v.vid for v in T.victims(256) if not v.chunked]
A_IDS = [c.cid for c in T.history_cases(256)]
B_IDS = [c.cid for c in T.intruder_cases(256)]


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.is_floating_point:
        view = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
        a, b = a.contiguous().view(view), b.contiguous().view(view)
    return bool(torch.equal(a, b))


def differing(got: dict, want: dict, keys=None) -> list:
    keys = sorted(want) if keys is None else keys
    assert set(keys) <= set(got) and set(keys) <= set(want), (sorted(got), sorted(want))
    return [k for k in keys if not same_bits(got[k], want[k])]


@functools.lru_cache(maxsize=64)
def rows(n: int, d: int, seed: int, stream: int) -> np.ndarray:
    return synth.activations(n, d, seed=seed, stream=stream, bf16=True)


# ------------------------------------------------------------------------------------------------------------------------
# rigs: one per family - a fresh module with fixed weights, its data, its call
# ------------------------------------------------------------------------------------------------------------------------
class Rig:
    """``module()``: a fresh module in train mode; ``data(B, stream, dtype)``: the argument tensors of one call (stream 0 =
    the victim's rows); ``call(m, args)``: the forward."""

    def __init__(self, v: T.Victim, device, golden_dir):
        self.v, self.device, self.golden = v, device, golden_dir
        self.prec_code = None

    # -- modules -------------------------------------------------------------------------------------------------------
    def module(self):
        v, dev = self.v, self.device
        f = v.family
        if f == "topk":
            D, H, K = v.dims
            self.w = weights(D, H, SEED)
            m, _ = make(dev, self.w, K, v.prec)
        elif f == "batchtopk":
            D, H, K = v.dims
            self.w = weights(D, H, SEED)
            m, _ = BT.make(dev, self.w, v.prec)
            assert (m.k, m.max_k_per_row) == (K, 64)
        elif f == "transcoder":
            from whisper_sae.sae.transcoder import TopKTranscoder
            D, H, K = v.dims
            w = synth.sae_weights(D, H, seed=29, bf16=False)
            self.W = (w["encoder.weight"], w["encoder.bias"], w["decoder.weight"], w["decoder.bias"])
            m = TopKTranscoder(D, D, H, k=K, precision=v.prec)
            TT.load(m, self.W)
        elif f in ("skip", "narrow"):
            from whisper_sae.sae.transcoder import SkipTranscoder, TopKTranscoder
            g = np.load(self.golden / "g12_transcoders.npz")
            tag = "eq" if f == "skip" else "narrow"
            (Din, Dout, H, K, B), self.W, self.gx, self.gt = TT.case(g, tag)
            assert (Din, Dout, H, K, B) == T.G12_DIMS[tag]
            self.g12 = g
            if f == "skip":
                m = SkipTranscoder(Din, Dout, H, k=K, precision=v.prec)
                TT.load(m, self.W)
                with torch.no_grad():
                    m.skip.weight.copy_(torch.from_numpy(g["skip.W_s"]))
                    m.skip.bias.copy_(torch.from_numpy(g["skip.b_s"]))
            else:
                m = TopKTranscoder(Din, Dout, H, k=K, dead_feature_threshold=20, precision=v.prec)
                TT.load(m, self.W)
        elif f == "crosscoder":
            from whisper_sae.sae.crosscoder import TopKCrossLayerCrosscoder
            d, L, S, K = v.dims
            torch.manual_seed(3)
            m = TopKCrossLayerCrosscoder(d, L, S, k=K, precision=v.prec)
            self.W = [p.detach().numpy().copy() for p in (m.W_enc, m.b_enc, m.W_dec, m.b_dec)]
        elif f == "relu":
            from whisper_sae.sae.model import ReLUSAE
            D, H = v.dims
            self.p = RS.make_problem(D, H, v.B, "bf16")
            p = self.p
            m = ReLUSAE(D, H, sparsity_weight=RS.WEIGHT, precision=v.prec)
            sd = m.state_dict()
            for key, val in (("encoder.weight", p["W_e"]), ("encoder.bias", p["b_e"]),
                             ("decoder.weight", np.ascontiguousarray(p["W_dT"].T)), ("decoder.bias", p["b_d"])):
                sd[key] = torch.from_numpy(np.array(val))
            m.load_state_dict(sd)
        elif f == "relu_crosscoder":
            from whisper_sae.sae.crosscoder import CrossLayerCrosscoder
            d, L, S = v.dims
            torch.manual_seed(2)
            m = CrossLayerCrosscoder(d_model=d, n_layers=L, d_sae=S, sparsity_weight=0.02, precision=v.prec)
            self.W = [p.detach().numpy().copy() for p in (m.W_enc, m.b_enc, m.W_dec, m.b_dec)]
        else:
            raise KeyError(f)
        m.to(dev).train()
        from whisper_sae.sae.packed import _precision_code
        self.prec_code = _precision_code(v.prec)
        return m

    def clone(self, src):
        """A fresh module carrying ``src``'s ``state_dict()``."""
        m = self.module()
        m.load_state_dict({k: t.detach().clone() for k, t in src.state_dict().items()})
        return m.to(self.device).train()

    # -- data ----------------------------------------------------------------------------------------------------------
    def widths(self) -> tuple:
        v = self.v
        if v.family in ("skip", "narrow"):
            return v.dims[0], v.dims[1]
        if v.family in ("crosscoder", "relu_crosscoder"):
            return (v.dims[0],) * v.dims[1]
        if v.family == "transcoder":
            return v.dims[0], v.dims[0]
        return (v.dims[0],)

    def numpy_rows(self, B: int, stream: int) -> list:
        v = self.v
        if stream == 0 and B == v.B:
            if v.family in ("skip", "narrow"):
                return [self.gx, self.gt]
            if v.family == "relu":
                return [self.p["x"]]
            if v.family == "crosscoder":
                return [synth.activations(B, v.dims[0], seed=31, stream=i, bf16=False) for i in range(v.dims[1])]
        bf = v.family not in ("skip", "narrow", "crosscoder")
        return [rows(B, w, SEED, 10 * stream + i) if bf else synth.activations(B, w, seed=SEED, stream=10 * stream + i, bf16=False)
                for i, w in enumerate(self.widths())]

    def data(self, B: int, stream: int, dtype: str = None, leaf: bool = None) -> list:
        v = self.v
        dtype = v.x_dtype if dtype is None else dtype
        leaf = v.dx if leaf is None else leaf
        out = [torch.from_numpy(a).to(device=self.device, dtype=DT[dtype]) for a in self.numpy_rows(B, stream)]
        if leaf:
            for t in out:
                t.requires_grad_(True)
        return out

    def call(self, m, args):
        f = self.v.family
        if f in ("crosscoder", "relu_crosscoder"):
            return m(dict(enumerate(args)))
        return m(*args)

    def encode_small(self, m, args):
        f = self.v.family
        if f in ("topk", "batchtopk"):
            return m.encode_compact(args[0])
        if f == "crosscoder":
            return m.encode(dict(enumerate(args)))
        return m.encode(args[0])

    def handle(self, m) -> int:
        return m._engine._ctx[self.prec_code][0]


@pytest.fixture(scope="module")
def rigs(device, golden_dir):
    cache = {}

    def get(vid: str) -> Rig:
        if vid not in cache:
            cache[vid] = Rig(victims()[vid], device, golden_dir)
        return cache[vid]

    return get


# ------------------------------------------------------------------------------------------------------------------------
# running a step and collecting its products
# ------------------------------------------------------------------------------------------------------------------------
def products(m, out, args, grads=True) -> dict:
    p = {}
    for name in out._fields:
        val = getattr(out, name)
        if isinstance(val, dict):
            for k, t in val.items():
                p[f"out.{name}.{k}"] = t
        elif torch.is_tensor(val):
            p[f"out.{name}"] = val
    if m._last_code is not None:
        p["code.vals"], p["code.idx"] = m._last_code
    for n, b in m.named_buffers():
        p[f"buf.{n}"] = b
    if hasattr(m, "last_selection"):
        p["last_selection"] = torch.tensor(list(m.last_selection()), dtype=torch.float64)
    if grads:
        p.update(gradients(m, args))
    return {k: t.detach().clone() for k, t in p.items()}


def gradients(m, args) -> dict:
    p = {}
    for n, prm in m.named_parameters():
        assert prm.grad is not None, n
        p[f"grad.{n}"] = prm.grad
    for i, a in enumerate(args):
        if a.requires_grad:
            assert a.grad is not None, i
            p[f"grad.arg{i}"] = a.grad
    return {k: t.detach().clone() for k, t in p.items()}


def zero_grads(m) -> None:
    for prm in m.parameters():
        prm.grad = None


def step(rig: Rig, m, args) -> tuple:
    """One training forward + backward; returns ``(out, products)``."""
    zero_grads(m)
    out = rig.call(m, args)
    out.loss.backward()
    torch.cuda.synchronize()
    return out, products(m, out, args)


class Undisturbed:
    def __init__(self, rig: Rig, src=None):
        self.m = rig.module() if src is None else rig.clone(src)
        self.args = rig.data(rig.v.B, 0)
        self.out, self.products = step(rig, self.m, self.args)


@pytest.fixture(scope="module")
def undisturbed(rigs):
    """The victim alone on a fresh module: computed once per victim and left unchanged."""
    cache = {}

    def get(vid: str) -> Undisturbed:
        if vid not in cache:
            cache[vid] = Undisturbed(rigs(vid))
        return cache[vid]

    return get


def fresh_buffers(rig: Rig) -> dict:
    if not hasattr(rig, "_fresh_buffers"):
        rig._fresh_buffers = {n: b.detach().clone() for n, b in rig.module().named_buffers()}
    return rig._fresh_buffers


def restore_buffers(rig: Rig, m) -> None:
    """The clock buffers (and BatchTopK's threshold) are module state, not ctx state: back to the fresh values, in place."""
    with torch.no_grad():
        for n, b in m.named_buffers():
            b.copy_(fresh_buffers(rig)[n])


def profile_on(handle: int) -> None:
    from whisper_sae import _native as N
    N.check(N.lib().wsae_profile_enable(handle, -1, 64), "wsae_profile_enable")


def profile_counts(handle: int) -> dict:
    from whisper_sae import _native as N
    torch.cuda.synchronize()
    got = {k: n for k, (n, _) in N.profile_read(handle).items()}
    N.check(N.lib().wsae_profile_disable(handle), "wsae_profile_disable")
    return got


def hold_counts(case: T.Case, got: dict) -> None:
    if case.counts is not None:
        assert {k: got.get(k, 0) for k in case.counts} == case.counts, (case.cid, got)


# ------------------------------------------------------------------------------------------------------------------------
# oracle anchors (the family's own helpers and bounds) and the determinism precondition
# ------------------------------------------------------------------------------------------------------------------------
def rel(a, b) -> float:
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def cpu(t) -> np.ndarray:
    return t.detach().float().cpu().numpy()


def held(note, key, measured, bound) -> None:
    note(key, measured, bound)
    assert measured < bound, (key, measured, bound)


def anchor_topk(rig, u, note):
    v = rig.v
    st = O.SAEState.from_state_dict(rig.w, k=v.dims[2], dead_feature_threshold=1000)
    check(u.m, st, u.out, rig.numpy_rows(v.B, 0)[0], v.prec, f"ctx_{v.vid}", note, want_dx=v.dx, xt=u.args[0], hidden=True)


def anchor_batchtopk(rig, u, note):
    """The body of test_gpu_batch_topk.py::test_forward_and_grads_match_oracle on the undisturbed run."""
    v, m, out = rig.v, u.m, u.out
    mode = BT.MODE[v.prec]
    x = rig.numpy_rows(v.B, 0)[0]
    st = O.SAEState.from_state_dict(rig.w, k=BT.KMAX, dead_feature_threshold=1000)
    _, idx = (cpu(t) for t in m._last_code)
    keep_dev = cpu(out.hidden) > 0
    keep, pre, t, bad = BO.dense_selection(st, x, mode, BT.K, BT.KMAX, idx.astype(np.int64), keep_dev)
    assert bad == 0, f"{bad} kept/dropped decisions differ clear of t"
    sel = m.last_selection()
    assert abs(sel.threshold - float(t)) <= 1e-5 * abs(float(t)) and sel.kept == int(keep_dev.sum())
    assert float(m.threshold) == sel.threshold
    fwd = BO.forward_from_keep(st, x, keep, pre, mode)
    ora = O.backward(st, x, fwd, mode)
    r = fwd["reconstructed"].astype(np.float64) - x.astype(np.float64)
    loss = float((r * r).sum()) / x.size
    held(note, f"ctx_{v.vid}_loss", abs(float(out.loss.detach()) - loss) / loss, 1e-5)
    held(note, f"ctx_{v.vid}_recon", rel(cpu(out.reconstructed), fwd["reconstructed"]), 1e-5)
    assert float(out.l0) == np.float32(keep.sum() / v.B)
    last = np.zeros(v.dims[1], np.int64)
    last[(fwd["hidden"] > 0).any(axis=0)] = 1
    assert np.array_equal(m.feature_last_activated.cpu().numpy(), last) and int(m.step_count) == 1
    params = dict(m.named_parameters())
    for n, key in BT.GRADS.items():
        held(note, f"ctx_{v.vid}_{n}", rel(cpu(params[key].grad), ora[n]), BT.GRAD_REL[v.prec][n])


def anchor_transcoder(rig, u, note):
    """test_transcoder.py::test_bf16_at_whisper_tiny_width_against_amp_oracle's comparison; the input and target gradients
    (bf16 leaves: rounded by autograd to the leaf's dtype) within test_gpu_kernel_variants.py's DX_REL."""
    v, m, o = rig.v, u.m, u.out
    K = v.dims[2]
    x, tgt = rig.numpy_rows(v.B, 0)
    idx = m._last_code[1].cpu().numpy()
    pre = O.transcoder_forward(*rig.W, K, x, tgt, "amp")["pre"]
    assert O.check_selection(pre, idx, K).all()
    assert (synth.topk_margin(pre, K) > 1e-5).mean() > 0.98
    f = O.transcoder_forward(*rig.W, K, x, tgt, "amp", select=idx)
    held(note, f"ctx_{v.vid}_loss", abs(float(o.loss.detach()) - float(f["loss"])) / float(f["loss"]), 1e-5)
    held(note, f"ctx_{v.vid}_pred", rel(cpu(o.predicted), f["predicted"]), 1e-5)
    b = O.transcoder_backward(*rig.W, x, tgt, f, "amp")
    for n, t in (("W_e", m.encoder.weight.grad), ("b_e", m.encoder.bias.grad), ("W_d", m.decoder.weight.grad),
                 ("b_d", m.decoder.bias.grad)):
        held(note, f"ctx_{v.vid}_{n}", rel(cpu(t), b[n]), 2e-3)
    held(note, f"ctx_{v.vid}_dx", rel(cpu(u.args[0].grad), b["x"]), DX_REL["bf16"])
    dt = -2.0 * (f["predicted"].astype(np.float64) - tgt.astype(np.float64)) / tgt.size  # d mean((pred - tgt)^2) / d tgt
    held(note, f"ctx_{v.vid}_dtarget", rel(cpu(u.args[1].grad), dt), DX_REL["bf16"])


def anchor_g12(rig, u, note):
    """test_transcoder.py::test_skip_transcoder_fp32 / test_topk_transcoder_fp32 against golden G12."""
    v, m, o, g = rig.v, u.m, u.out, rig.g12
    tag = "skip" if v.family == "skip" else "narrow"
    held(note, f"ctx_{v.vid}_pred", rel(cpu(o.predicted), g[f"{tag}.pred"]), 1e-5)
    held(note, f"ctx_{v.vid}_loss", abs(float(o.loss.detach()) - float(g[f"{tag}.loss"])) / float(g[f"{tag}.loss"]), 1e-5)
    got = {"dW_e": m.encoder.weight.grad, "dW_d": m.decoder.weight.grad, "db_d": m.decoder.bias.grad, "dx": u.args[0].grad}
    if v.family == "skip":
        got.update({"dW_s": m.skip.weight.grad, "db_s": m.skip.bias.grad})
    else:
        got["db_e"] = m.encoder.bias.grad
        assert np.array_equal(np.sort(m._last_code[1].cpu().numpy(), axis=1).astype(np.int16), g[f"{tag}.idx"])
        assert float(o.l0) == float(g[f"{tag}.l0"])
    for key, t in got.items():
        held(note, f"ctx_{v.vid}_{key}", rel(cpu(t), g[f"{tag}.{key}"]), 2e-5)


def anchor_crosscoder(rig, u, note):
    """test_crosscoder.py::test_padded_width_and_missing_layer's comparison."""
    v, m, o = rig.v, u.m, u.out
    d, L, S, K = v.dims
    a = rig.numpy_rows(v.B, 0)
    f = O.crosscoder_forward(*rig.W, K, a)
    b = O.crosscoder_backward(*rig.W, a, f)
    held(note, f"ctx_{v.vid}_loss", abs(float(o.loss.detach()) - float(f["loss"])) / float(f["loss"]), 1e-5)
    held(note, f"ctx_{v.vid}_recon", rel(cpu(torch.stack([o.reconstructed[i] for i in range(L)])), np.stack(f["recon"])), 1e-5)
    for n, p in (("W_enc", m.W_enc), ("b_enc", m.b_enc), ("W_dec", m.W_dec), ("b_dec", m.b_dec)):
        held(note, f"ctx_{v.vid}_{n}", rel(cpu(p.grad), b[n]), 2e-5)


def anchor_relu(rig, u, note):
    """tests/relu_oracle.py's stage-wise derived bounds (``test_gpu_relu_step.check``) on the module's products."""
    v, m, o, p = rig.v, u.m, u.out, rig.p
    eng = m._engine
    RS.expect_flow(types.SimpleNamespace(eng=eng, handle=rig.handle(m), p=p), v.flow)
    D, H = v.dims
    out = {"hidden": cpu(o.hidden).reshape(v.B, H), "recon": cpu(o.reconstructed).reshape(v.B, D),
           "loss": np.float32(float(o.loss.detach())), "l0": np.float32(float(o.l0)), "sparsity": np.float32(float(o.sparsity_loss)),
           "dW_e": cpu(m.encoder.weight.grad), "dW_dT": np.ascontiguousarray(cpu(m.decoder.weight.grad).T),
           "db_e": cpu(m.encoder.bias.grad), "db_d": cpu(m.decoder.bias.grad)}
    RS.check(p, v.prec, v.flow, out, note, f"ctx_{v.vid}")


def anchor_relu_crosscoder(rig, u, note):
    """test_crosscoder.py::test_bf16_mode_against_the_oracle's comparison (a plain fp32 oracle: direction and size)."""
    v, m, o = rig.v, u.m, u.out
    lam = 0.02
    a = rig.numpy_rows(v.B, 0)
    f = O.crosscoder_relu_forward(*rig.W, a, lam)
    b = O.crosscoder_relu_backward(*rig.W, a, f, lam)
    held(note, f"ctx_{v.vid}_loss", abs(float(o.loss.detach()) - float(f["loss"])) / float(f["loss"]), 5e-3)
    held(note, f"ctx_{v.vid}_sparsity", abs(float(o.sparsity_loss) - float(f["sparsity_loss"])) / float(f["sparsity_loss"]), 5e-3)
    for n, p in (("W_enc", m.W_enc), ("b_enc", m.b_enc), ("W_dec", m.W_dec), ("b_dec", m.b_dec)):
        got, ref = cpu(p.grad).astype(np.float64).ravel(), b[n].astype(np.float64).ravel()
        cos = float(got @ ref / np.sqrt((got @ got) * (ref @ ref)))
        held(note, f"ctx_{v.vid}_{n}_one_minus_cos", 1 - cos, 1e-3)
        held(note, f"ctx_{v.vid}_{n}_norm", abs(np.linalg.norm(got) / np.linalg.norm(ref) - 1), 2e-2)


ANCHORS = {"topk": anchor_topk, "batchtopk": anchor_batchtopk, "transcoder": anchor_transcoder, "skip": anchor_g12,
           "narrow": anchor_g12, "crosscoder": anchor_crosscoder, "relu": anchor_relu, "relu_crosscoder": anchor_relu_crosscoder}


@pytest.mark.parametrize("vid", ANCHORED)
def test_undisturbed_run_against_the_oracle(rigs, undisturbed, parity_note, vid):
    rig = rigs(vid)
    assert rig.v.B <= T.ANCHOR_MAX_B
    ANCHORS[rig.v.family](rig, undisturbed(vid), parity_note)


@pytest.mark.parametrize("vid", VIDS)
def test_two_undisturbed_runs_are_bit_identical(rigs, undisturbed, vid):
    again = Undisturbed(rigs(vid))
    assert differing(again.products, undisturbed(vid).products) == []


# ------------------------------------------------------------------------------------------------------------------------
# part A: a victim after a history equals the victim on a fresh ctx
# ------------------------------------------------------------------------------------------------------------------------
def trainer_for(m, v: T.Victim, device, tmp_path):
    from whisper_sae.config import TrainingConfig
    from whisper_sae.sae.training import SAETrainer
    cfg = TrainingConfig(batch_size=v.B, learning_rate=1e-3, weight_decay=0.0, epochs=1, warmup_steps=0, gradient_clip=1.0,
                         use_amp=v.prec == "bf16", num_workers=0)
    return SAETrainer(m, cfg, device=device, run_dir=tmp_path)


def causal_intruders(rig: Rig, m, which=("intervention", "attribution")) -> None:
    from whisper_sae.causal import FeatureEdit, SAEAttribution, SAEIntervention
    h, g = rig.data(T.CAUSAL_ROWS, 3, leaf=False)[0], rig.data(T.CAUSAL_ROWS, 4, leaf=False)[0]
    if "intervention" in which:
        iv = SAEIntervention(m, FeatureEdit.ablate([5, 9]))
        iv.apply(h)
        assert iv.last_changed_rows >= 0
    if "attribution" in which:
        SAEAttribution(m).attribute(h, g)


@pytest.mark.parametrize("cid", A_IDS)
def test_victim_after_a_history(rigs, undisturbed, device, tmp_path, cid):
    case = next(c for c in T.history_cases(cus()) if c.cid == cid)
    rig = rigs(case.vid)
    v = rig.v
    want = undisturbed(v.vid).products
    m = rig.module()
    step(rig, m, rig.data(v.big, 1))  # ``big``: the cap is fixed before the victim
    handle = rig.handle(m)
    assert m._engine._ctx[rig.prec_code][1] == v.big
    profile_on(handle)
    kind = case.kind
    if kind == "same":
        with torch.no_grad():
            rig.call(m, rig.data(v.B, 2, leaf=False))
    elif kind == "dtype":
        step(rig, m, rig.data(v.B, 2, dtype=OTHER[v.x_dtype]))
    elif kind == "pending":
        out = rig.call(m, rig.data(v.B, 2))
        assert out.loss.requires_grad
        del out
    elif kind == "causal":
        causal_intruders(rig, m)
    elif kind == "params":
        before = {n: p.detach().clone() for n, p in m.named_parameters()}
        if v.vid == "V5":  # one resample that really rewrites features
            with torch.no_grad():
                m.feature_last_activated[:7] = -100_000
            assert m.resample_dead_features(rig.data(v.B, 2, leaf=False)[0]) > 0
        else:
            float(trainer_for(m, v, device, tmp_path).train_step(rig.data(v.B, 2, leaf=False)[0]).loss)
        assert any(not same_bits(p.detach(), before[n]) for n, p in m.named_parameters())
        want = Undisturbed(rig, src=m).products  # a fresh module loaded from the history module's state_dict()
    if kind != "params":
        restore_buffers(rig, m)
    _, got = step(rig, m, rig.data(v.B, 0))
    assert rig.handle(m) == handle, "the ctx was replaced: the case does not test what it claims"
    hold_counts(case, profile_counts(handle))
    assert differing(got, want) == []


# ------------------------------------------------------------------------------------------------------------------------
# part B: a backward after an intruder on the kept ctx
# ------------------------------------------------------------------------------------------------------------------------
def grad_keys(products_: dict) -> list:
    return sorted(k for k in products_ if k.startswith("grad."))


def intrude(rig: Rig, m, kind: str) -> None:
    v = rig.v
    if kind == "nograd_same":
        m.train(v.family != "batchtopk")  # (BatchTopK: eval mode, so that the intruder leaves ``threshold`` alone)
        with torch.no_grad():
            rig.call(m, rig.data(v.B, 2, leaf=False))
        m.train()
    elif kind == "encode_small":
        rig.encode_small(m, rig.data(T.small(v), 2, leaf=False))
    elif kind == "pre_activation":
        m.pre_activation(rig.data(T.small(v), 2, leaf=False)[0])
    elif kind in ("intervention", "attribution"):
        causal_intruders(rig, m, (kind,))
    elif kind == "over_cap":
        with torch.no_grad():
            rig.call(m, rig.data(T.over_cap(v), 2, leaf=False))
    else:
        raise KeyError(kind)


@pytest.mark.parametrize("cid", B_IDS)
def test_backward_after_an_intruder(rigs, undisturbed, cid):
    case = next(c for c in T.intruder_cases(cus()) if c.cid == cid)
    rig = rigs(case.vid)
    v = rig.v
    want = undisturbed(v.vid).products
    m = rig.module()
    step(rig, m, rig.data(v.big, 1))
    handle, cap = m._engine._ctx[rig.prec_code]
    zero_grads(m)
    if case.ctx == "kept":
        profile_on(handle)
    args = rig.data(v.B, 0)
    out = rig.call(m, args)
    gen = m._engine.generation
    if case.kind in ("second_ab", "second_ba"):
        # a second grad-mode forward whose backward also runs, in both orders: each equals its own undisturbed run
        rig_b = Rig(v, rig.device, rig.golden)
        mb = rig_b.module()
        args_b_ref = rig_b.data(v.B, 2)
        _, want_b = step(rig_b, mb, args_b_ref)
        args_b = rig.data(v.B, 2)
        out_b = rig.call(m, args_b)
        order = [(out, args, want), (out_b, args_b, want_b)]
        if case.kind == "second_ba":
            order.reverse()
        bad = []
        for o, a, w in order:
            zero_grads(m)
            o.loss.backward()
            torch.cuda.synchronize()
            bad += differing(gradients(m, a), w, grad_keys(w))
    else:
        intrude(rig, m, case.kind)
        out.loss.backward()
        torch.cuda.synchronize()
        bad = differing(gradients(m, args), want, grad_keys(want))
    if case.ctx == "kept":
        assert rig.handle(m) == handle, "the ctx was replaced: the case does not test what it claims"
        hold_counts(case, profile_counts(handle))
    else:
        # (the handle VALUE proves nothing here: the allocator hands the address of the destroyed ctx to the new one, as
        # measured on the MI355X for all eleven cases; SAEEngine.ctx replaces the ctx exactly when the cap grows)
        assert m._engine._ctx[rig.prec_code][1] == T.over_cap(v) > cap, "the intruder fitted the cap: the case does not test what it claims"
        assert m._engine.generation == gen + 3  # the new ctx, the intruder and the restage each moved it on by one
    assert bad == []


@pytest.mark.parametrize("kind", ["pre_activation", "encode_small", "intervention", "attribution", "nograd_same"])
def test_batch_topk_restage_leaves_the_selection_alone(rigs, kind):
    """BatchTopK: the restage runs with the selection switched off and the saved code.  After the backward ``threshold``
    equals the undisturbed run's and ``last_selection()`` is what it was before the backward (the undisturbed run's when
    the intruder selects nothing); a following training forward selects again, as in the undisturbed sequence."""
    rig = rigs("V7")
    v = rig.v
    nxt = rig.data(v.B, 5)

    def sequence(intruder):
        m = rig.module()
        step(rig, m, rig.data(v.big, 1))
        restore_buffers(rig, m)
        zero_grads(m)
        handle = rig.handle(m)
        args = rig.data(v.B, 0)
        out = rig.call(m, args)
        sel_fwd = m.last_selection()
        if intruder is not None:
            intrude(rig, m, intruder)
        sel_before = m.last_selection()
        out.loss.backward()
        torch.cuda.synchronize()
        rec = {"threshold": m.threshold.detach().clone(), "sel_fwd": sel_fwd, "sel_before": sel_before,
               "sel_after": m.last_selection(), "grads": gradients(m, args)}
        zero_grads(m)
        out2 = rig.call(m, nxt)
        rec["next"] = products(m, out2, nxt, grads=False)
        assert rig.handle(m) == handle
        return rec

    clean, hist = sequence(None), sequence(kind)
    assert differing(hist["grads"], clean["grads"]) == []
    assert same_bits(hist["threshold"], clean["threshold"])
    assert hist["sel_after"] == hist["sel_before"]
    assert hist["sel_fwd"] == clean["sel_fwd"] == clean["sel_after"]
    if kind == "pre_activation":
        assert hist["sel_after"] == clean["sel_after"]
    assert differing(hist["next"], clean["next"]) == []
    assert hist["next"]["last_selection"][2] > 0 and not same_bits(hist["next"]["buf.threshold"], clean["threshold"])


# ------------------------------------------------------------------------------------------------------------------------
# part C: an epoch with a ragged batch through the trainer, on one ctx and on a fresh ctx per step
# ------------------------------------------------------------------------------------------------------------------------
def drop_contexts(eng) -> None:
    """Leave the engine as a newly built one apart from the pack: no ctx, no record of prepared shadows, no record of a
    reserved ReLU workspace (a handle value the allocator hands out again must not be taken for a reserved one), no
    cached scratch."""
    torch.cuda.synchronize(eng.device)
    eng.close()
    eng._fresh.clear()
    eng._relu_reserved.clear()
    eng._work.clear()


@pytest.mark.parametrize("eid", [e[0] for e in T.EPOCHS])
def test_epoch_with_a_ragged_batch(rigs, device, tmp_path, eid):
    _, family, prec, dims, sizes, _ = next(e for e in T.EPOCHS if e[0] == eid)
    v = next(x for x in victims().values() if x.family == family and x.prec == prec and x.dims == dims)
    rig = Rig(v, device, None)
    D = dims[0]
    data = rows(sum(sizes), D, SEED, 77)

    def epoch(fresh_ctx_per_step: bool):
        m = rig.module()
        tr = trainer_for(m, v, device, tmp_path)
        eng = m.bind()
        mets, handles, at = [], [], 0
        for n in sizes:
            if fresh_ctx_per_step:
                drop_contexts(eng)
            x = torch.from_numpy(data[at:at + n]).to(device=device, dtype=DT[v.x_dtype])
            at += n
            met = tr.train_step(x)
            rec = [met.loss, met.l0, met.grad_norm, met.dead_feature_ratio, met.sparsity_loss]
            if hasattr(m, "threshold"):
                rec.append(float(m.threshold))
            assert all(np.isfinite(r) for r in rec), rec
            mets.append(rec)
            handles.append((eng._ctx[rig.prec_code][0], eng._ctx[rig.prec_code][1]))
        torch.cuda.synchronize()
        state = {f"sd.{k}": t.detach().clone() for k, t in m.state_dict().items()}
        state["opt.m"], state["opt.v"] = tr.optimizer._m.clone(), tr.optimizer._v.clone()
        return mets, state, handles

    mets_one, state_one, handles_one = epoch(False)
    mets_each, state_each, handles_each = epoch(True)
    assert len({h for h, _ in handles_one}) == 1 and {c for _, c in handles_one} == {max(sizes)}  # one ctx, sized by the largest
    assert [c for _, c in handles_each] == [max(n, 64) for n in sizes]                            # exactly sized each step
    assert [np.array(r, np.float64).view(np.int64).tolist() for r in mets_one] == \
           [np.array(r, np.float64).view(np.int64).tolist() for r in mets_each], (mets_one, mets_each)
    assert differing(state_one, state_each) == []


# ------------------------------------------------------------------------------------------------------------------------
# part D: the control - without the restage the backward reads the intruder's state
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c[0] for c in T.CONTROLS])
def test_without_the_restage_the_backward_reads_the_intruder(rigs, undisturbed, cid):
    """The backward through the C ABI after an intruder of the SAME B, without restaging: either the call is refused with
    a message naming the missing staged state, or its gradients differ from the undisturbed ones.  Part B's equality is
    earned by the restage.  (Same B only: every index the stale state can produce lies inside buffers the victim sized.)"""
    from whisper_sae import _native as N
    from whisper_sae.sae.engine import _dtype_code
    vid = next(c[1] for c in T.CONTROLS if c[0] == cid)
    rig = rigs(vid)
    v = rig.v
    want = undisturbed(vid).products
    m = rig.module()
    step(rig, m, rig.data(v.big, 1))
    zero_grads(m)
    eng, handle = m._engine, rig.handle(m)
    out = rig.call(m, rig.data(v.B, 0))
    saved = out.loss.grad_fn.saved_tensors
    other = rig.call(m, rig.data(v.B, 2))  # the intruder: a grad-mode forward of other rows, same B
    assert other.loss.requires_grad and rig.handle(m) == handle
    grads = torch.zeros(eng.P, dtype=torch.float32, device=eng.device)
    pk, st = eng.pack.data_ptr(), eng.stream()
    if v.family == "topk":
        x2, _, vals, idx, dpre = saved
        assert x2.shape[0] == v.B
        rc = eng.lib.wsae_weight_grads(handle, pk, x2.data_ptr(), _dtype_code(x2), 0, vals.data_ptr(), idx.data_ptr(),
                                       dpre.data_ptr(), v.B, grads.data_ptr(), st)
    else:
        x2, hidden, recon = saved
        assert x2.shape[0] == v.B
        rc = eng.lib.wsae_relu_backward(handle, pk, x2.data_ptr(), _dtype_code(x2), 0, v.B, float(m.sparsity_weight),
                                        hidden.data_ptr(), recon.data_ptr(), grads.data_ptr(), st)
    torch.cuda.synchronize()
    if rc != 0:
        assert "staged" in N.last_error() or "forward" in N.last_error(), N.last_error()
        return
    got = {f"grad.{n}": m._sliced(n, grads).detach().clone() for n in m._named_core_params()}
    keys = sorted(got)
    assert differing(got, want, keys) != [], "the stale state gave the undisturbed gradients: part B proves nothing"
    assert "grad.decoder.weight" in differing(got, want, keys)
