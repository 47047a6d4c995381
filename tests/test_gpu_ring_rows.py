"""Row-list parity for every kernel variant of the TopK step.

Production batches reach the kernels as ``(buffer, int32 row list)``: batch row b is ``buffer[rows[b], :]``
(include/wsae.h).  Each kernel gathers through the list in a branch of its own, and the per-variant parity files
(tests/test_gpu_kernel_variants.py, tests/test_gpu_parity.py) feed contiguous tensors only.  Here every case of
``ring_rows_cases.SPECS`` - one per gather branch, the smallest shape that reaches it - and of ``PREFETCH_SPECS`` runs ONE
``SAETrainer.train_step(RingBatch(buffer, rows))`` on the adversarial buffer and list of ``ring_rows_cases.make_case``
(no entry names its own position, repeats, both buffer ends named from the batch ends, NaN in every row the list does not
name and behind every list entry outside the view handed over), and is held to two tiers:

* equality: the same step on a fresh trainer fed the contiguous tensor ``buffer[rows.long()]`` in the same dtype.  No
  dispatch decision depends on ``rows``, so the two runs launch the same kernels with the same summation order: the code,
  ``dpre``, the five gradients, the metrics, the updated pack and the dead clock must be bit-identical, and finite;
* oracle (cases with B <= 2100): the ring run against the float64 oracle on ``buffer_host[rows]``, with the suite's stated
  bounds (``ring_rows_cases.compare_with_oracle``; what that comparison can see is shown on the CPU in
  tests/test_ring_rows_cases.py).  Measured gaps: profiles/ring_rows_parity_notes.jsonl.

Also: the strip-TopK repair on a ragged batch (``fix.arows``), BatchTopK through the trainer, the data-parallel wire forms
of the weight gradients, and ``wsae_encode_dense``.  The kernels each test launched: profiles/ring_rows_trace.txt.

What the file can see was checked once on the MI355X against four scratch builds, each with ONE stage's list lookup replaced
by the batch position (still inside the buffer): the decode kernels' (every case failed except those whose waves decode a
single row and the dense encoder calls - hence ``PREFETCH_SPECS``, all five of which failed), the weight-gradient
launches' (every direct-gather case and both wire tests failed, the staged cases rightly passed), the encoder's four
gathers (every step and every dense call failed) and the strip repair's (the forced-repair test alone failed).
"""

from __future__ import annotations

import os

import numpy as np
import pytest
import torch

import ring_rows_cases as R

pytestmark = pytest.mark.gpu

TORCH_DT = {"bf16": torch.bfloat16, "fp32": torch.float32}
_cases = {}


def on_device(device, spec):
    """Per (B, D, seed, buffer dtype), once: the case, the buffer on the device, the list as the view [64 : 64 + B] of the
    longer int32 tensor, and the gathered contiguous tensor."""
    key = (spec.B, spec.D, spec.seed, spec.buffer)
    if key not in _cases:
        host_key = key[:3]
        if host_key not in _cases:
            _cases[host_key] = R.make_case(spec.B, spec.D, spec.seed)
        c = _cases[host_key]
        buf = torch.from_numpy(c.buffer).to(device=device, dtype=TORCH_DT[spec.buffer])
        padded = torch.from_numpy(c.padded).to(device)
        rows = padded[R.FRONT:R.FRONT + spec.B]
        assert rows.data_ptr() % 256 == 0 and rows.is_contiguous() and rows.dtype == torch.int32
        gathered = buf[rows.long()].contiguous()
        assert torch.equal(gathered.float().cpu(), torch.from_numpy(c.buffer[c.rows]))  # (finite, and the same values)
        _cases[key] = (c, buf, rows, gathered)
    return _cases[key]


def new_model(spec, cls=None):
    from whisper_sae.sae.model import TopKSAE
    m = (cls or TopKSAE)(spec.D, spec.H, k=spec.K, dead_feature_threshold=R.DEAD_THRESHOLD, precision=spec.mode)
    w = R.weights(spec.D, spec.H)
    sd = m.state_dict()
    for key in R.KEYS:
        sd[key] = torch.from_numpy(np.ascontiguousarray(w[key]))
    m.load_state_dict(sd)
    return m


def dense_wgrad_ctx(eng, prec, B):
    """The step's context created with WSAE_WGRAD_SPARSE=0 (read when the context is created), the variable restored."""
    old = os.environ.get("WSAE_WGRAD_SPARSE")
    os.environ["WSAE_WGRAD_SPARSE"] = "0"
    try:
        eng.ctx(prec, B)
    finally:
        if old is None:
            del os.environ["WSAE_WGRAD_SPARSE"]
        else:
            os.environ["WSAE_WGRAD_SPARSE"] = old


def one_step(device, run_dir, spec, batch, cls=None, before=None):
    """One train step of a fresh trainer on ``batch``; returns (every product read back, model, trainer)."""
    from whisper_sae import _native as N
    from whisper_sae.config import TrainingConfig
    from whisper_sae.sae.training import SAETrainer
    m = new_model(spec, cls)
    cfg = TrainingConfig(batch_size=spec.B, learning_rate=R.LR, weight_decay=0.0, epochs=1, warmup_steps=0, gradient_clip=1.0,
                         use_amp=spec.mode == "bf16", num_workers=0)
    tr = SAETrainer(m, cfg, device=device, run_dir=run_dir)
    if spec.dense_wgrad:
        dense_wgrad_ctx(m.bind(), N.PREC_BF16 if tr.use_amp else N.PREC_FP32, spec.B)
    if before is not None:
        before(m)
    met = tr.train_step(batch)
    torch.cuda.synchronize()
    work = m._engine.work(spec.B)
    out = {n: work[n].clone() for n in ("vals", "idx", "dpre")}
    for n, key in R.GRADS.items():
        out[f"grad_{n}"] = tr.optimizer.grad_view(key).clone()
    out["pack"] = m._engine.pack.clone()
    out["feature_last_activated"] = m.feature_last_activated.clone()
    out["step_count"] = m.step_count.clone()
    out["metrics"] = {n: getattr(met, n) for n in ("loss", "l0", "grad_norm", "clip_coef", "dead_feature_ratio")}
    return out, m, tr


def assert_finite(out, tag):
    for n, v in out.items():
        if n == "metrics":
            assert all(np.isfinite(x) for x in v.values()), (tag, v)
        elif v.is_floating_point():
            assert bool(torch.isfinite(v).all()), f"{tag}: {n} is not finite"


def assert_same(ring, tensor, tag):
    """Bit-identical products of two device runs (finite first: a NaN would only say 'differs')."""
    assert_finite(ring, f"{tag} (row list)")
    assert_finite(tensor, f"{tag} (tensor)")
    for n, v in ring.items():
        if n == "metrics":
            for k, a in v.items():
                assert a == tensor[n][k], f"{tag}: {k} {a!r} with the row list, {tensor[n][k]!r} with the gathered tensor"
        else:
            same = torch.equal(v, tensor[n])
            assert same, f"{tag}: {n} differs in {int((v != tensor[n]).sum())} of {v.numel()} elements"


@pytest.fixture(scope="module")
def ring_step(device, tmp_path_factory):
    """``ring_step(spec)``: the row-list run of a case, once per module (g1's is shared by the repair and the wire tests)."""
    from whisper_sae.sae.training import RingBatch
    done = {}

    def get(spec):
        if spec.cid not in done:
            _, buf, rows, _ = on_device(device, spec)
            done[spec.cid] = one_step(device, tmp_path_factory.mktemp(f"ring_{spec.cid}"), spec, RingBatch(buf, rows))
        return done[spec.cid]

    yield get
    torch.cuda.synchronize()
    done.clear()


# ------------------------------------------------------------------------------------------------------------------------
# 1. every gather branch of the step: equality with the gathered tensor, and the float64 oracle
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [s.cid for s in R.ALL_SPECS])
def test_row_list_step(device, tmp_path, ring_step, parity_note, cid):
    spec = R.SPEC[cid]
    c, _, _, gathered = on_device(device, spec)
    ring, m, _ = ring_step(spec)
    tensor, _, _ = one_step(device, tmp_path, spec, gathered)
    assert_same(ring, tensor, cid)
    assert int(ring["step_count"]) == 1
    if not spec.oracle:
        return
    dev = {"idx": ring["idx"].cpu().numpy(), "vals": ring["vals"].cpu().numpy(),
           "grads": {n: ring[f"grad_{n}"].float().cpu().numpy() for n in R.GRADS},
           "last_activated": ring["feature_last_activated"].cpu().numpy(), "step_count": int(ring["step_count"]),
           **ring["metrics"]}
    gaps = R.compare_with_oracle(dev, R.oracle_state(spec), c.buffer[c.rows], spec.K, spec.mode, parity_note, f"rowlist_{cid}")
    print(cid, {k: f"{v:.3g}" for k, v in gaps.items()})


def test_forced_strip_repair_on_the_ragged_batch(device, tmp_path, ring_step):
    """g1 again with a store threshold no strip reaches: the GEMM stores nothing in its full tiles and every row of them
    rebuilds its candidate strips in the TopK launch, reading x through ``fix.arows``.  The same bits as the plain run."""
    from test_gpu_strip_predict import predict, stats
    from whisper_sae.sae.training import RingBatch
    spec = R.SPEC["g1"]
    _, buf, rows, _ = on_device(device, spec)
    plain, _, _ = ring_step(spec)
    forced, m, _ = one_step(device, tmp_path, spec, RingBatch(buf, rows), before=lambda mod: predict(mod, spec.B, True, 1e30))
    assert stats(m, spec.B)[0] >= spec.B // 256 * 256, "the repair did not run"
    assert_same(forced, plain, "g1 forced repair")


def test_batch_topk_step(device, tmp_path, ring_step):
    """b1: the batch-wide selection sits between the TopK and the decode on the row-list route."""
    from whisper_sae.sae.model import BatchTopKSAE
    from whisper_sae.sae.training import RingBatch
    spec = R.B1
    _, buf, rows, gathered = on_device(device, spec)
    ring, m_r, _ = one_step(device, tmp_path / "ring", spec, RingBatch(buf, rows), cls=BatchTopKSAE)
    tensor, m_t, _ = one_step(device, tmp_path / "tensor", spec, gathered, cls=BatchTopKSAE)
    assert_same(ring, tensor, "b1")
    sel = m_r.last_selection()
    assert sel == m_t.last_selection() and sel.kept > 0 and np.isfinite(sel.threshold)
    assert float(m_r.threshold) == float(m_t.threshold) == sel.threshold


# ------------------------------------------------------------------------------------------------------------------------
# 2. the data-parallel wire forms of the weight gradients, after g1's forward on g1's context and work buffers
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parts", ["all", "halves"], ids=["w1-all", "w2-decoder-encoder"])
def test_weight_grads_wire(device, ring_step, parts):
    from whisper_sae import _native as N
    spec = R.SPEC["g1"]
    _, buf, rows, gathered = on_device(device, spec)
    _, m, _ = ring_step(spec)
    eng = m._engine
    lib, st, B = eng.lib, eng.stream(), spec.B
    handle = eng.prepare(N.PREC_BF16, B, force=True)
    if parts == "halves":
        assert lib.wsae_wgrad_parts_supported(handle)
    w = eng.work(B)
    pk = eng.pack.data_ptr()
    N.check(lib.wsae_encode_decode(handle, pk, buf.data_ptr(), N.DT_BF16, rows.data_ptr(), B, w["vals"].data_ptr(),
                                   w["idx"].data_ptr(), 0, 0, 1, w["dpre"].data_ptr(), 0, eng.stats.data_ptr(), st),
            "wsae_encode_decode")
    eng.generation += 1

    def wire_of(x, rows_ptr):
        fired = torch.zeros(eng.H, dtype=torch.float32, device=device)
        wire = torch.full((eng.P + eng.H + N.WIRE_METRIC_SLOTS,), float("nan"), dtype=torch.float32, device=device)
        N.check(lib.wsae_ctx_set_fired(handle, fired.data_ptr()), "wsae_ctx_set_fired")
        args = (handle, pk, x.data_ptr(), N.DT_BF16, rows_ptr, w["vals"].data_ptr(), w["idx"].data_ptr(), w["dpre"].data_ptr(), B)
        for part in ((N.PART_ALL,) if parts == "all" else (N.PART_DECODER, N.PART_ENCODER)):
            N.check(lib.wsae_weight_grads_wire(*args, part, wire.data_ptr(), N.DT_F32, st), "wsae_weight_grads_wire")
        torch.cuda.synchronize()
        N.check(lib.wsae_ctx_set_fired(handle, 0), "wsae_ctx_set_fired")
        return wire

    with_list = wire_of(buf, rows.data_ptr())
    with_tensor = wire_of(gathered, 0)
    grads = with_list[:eng.P]
    assert bool(torch.isfinite(grads).all()), "the wire's gradients are not finite"
    assert float(grads[:2 * eng.H * eng.D].abs().max()) > 0
    assert torch.equal(with_list.view(torch.int32), with_tensor.view(torch.int32)), \
        f"{int((with_list.view(torch.int32) != with_tensor.view(torch.int32)).sum())} wire elements differ"


# ------------------------------------------------------------------------------------------------------------------------
# 3. wsae_encode_dense: stages through the list even in bf16 mode
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", R.DENSE_SHAPES, ids=[f"d1-{c}" for c in R.DENSE_SHAPES])
def test_encode_dense(device, cid):
    from whisper_sae import _native as N
    spec = R.SPEC[cid]
    _, buf, rows, gathered = on_device(device, spec)
    m = new_model(spec).to(device)
    eng = m.bind()
    handle = eng.prepare(N.PREC_BF16, spec.B, force=True)

    def pre_of(x, rows_ptr):
        pre = torch.full((spec.B, spec.H), float("nan"), dtype=torch.float32, device=device)
        N.check(eng.lib.wsae_encode_dense(handle, eng.pack.data_ptr(), x.data_ptr(), N.DT_BF16, rows_ptr, spec.B, pre.data_ptr(),
                                          eng.stream()), "wsae_encode_dense")
        eng.generation += 1
        torch.cuda.synchronize()
        return pre

    with_list = pre_of(buf, rows.data_ptr())
    with_tensor = pre_of(gathered, 0)
    assert bool(torch.isfinite(with_list).all()) and bool(torch.isfinite(with_tensor).all())
    assert torch.equal(with_list, with_tensor), f"{int((with_list != with_tensor).sum())} pre-activations differ"
