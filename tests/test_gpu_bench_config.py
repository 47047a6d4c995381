"""GPU parity at the configurations that are actually benchmarked.

``bench.py`` runs 384 -> 3072, k = 32, bf16, B = 16384 rows drawn from the on-device ring: the persistent
encoder GEMM with the XCD-aware tile walk (needs B / 256 to be a multiple of 8), the strip-guided TopK, the
register-resident decode kernel and the weight-gradient kernel with split-K 8.  The tests here feed exactly
that launch configuration - ring rows, non-zero weights, the trainer's fused step - and compare every product of
the step with the float64 oracle in its ``"amp"`` mode (which mirrors the device's bf16 roundings):

* TopK index sets: bit-exact on every row whose k-th / (k+1)-th pre-activations are further apart than fp32
  summation-order noise (relative 1e-5); on the remaining rows (a few per ten thousand) the
  device's selection must be a valid TopK up to that noise, and the oracle then continues from it so that
  everything downstream compares element-wise;
* loss 1e-5 relative, l0 exact, global gradient norm 1e-4, the five gradients 2e-3 of the tensor maximum
  (single entries of the bf16-rounded MFMA operands land on the other side of a rounding boundary when fp32
  sums are taken in a different order: one bf16 ulp = 0.4 % of that entry), parameters after the step.

Also here: a 20-step bf16 trajectory at these dimensions, BASELINE.json configs[3] dimensions (768 -> 12288,
k = 64) with one train step and one ``resample_dead_features`` call, and the interleaved-call case of the
autograd path (forward(x); encode(y); backward).
"""

from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import sae_oracle as O
from oracle import synth

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
KEYS = ("encoder.weight", "encoder.bias", "decoder.weight", "decoder.bias", "b_pre")
GRAD_OF = {"W_e": "encoder.weight", "b_e": "encoder.bias", "W_d": "decoder.weight", "b_d": "decoder.bias",
           "b_pre": "b_pre"}


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def cpu(t):
    return t.detach().float().cpu().numpy()


def note(name: str, payload: dict) -> None:
    """Leave the measured differences next to the logs (gpurun_out/ travels back from the GPU box)."""
    out = ROOT / "gpurun_out"
    try:
        out.mkdir(exist_ok=True)
        with open(out / "parity_notes.jsonl", "a") as f:
            f.write(json.dumps({"test": name, **payload}) + "\n")
    except OSError:
        pass


def build(D, H, k, seed, thr, precision=None, bf16=False, b_pre_scale=0.1):
    from whisper_sae.sae.model import TopKSAE
    w = synth.sae_weights(D, H, seed=seed, bf16=bf16, b_pre_scale=b_pre_scale)
    m = TopKSAE(D, H, k=k, dead_feature_threshold=thr, precision=precision)
    sd = m.state_dict()
    for key in KEYS:
        sd[key] = torch.from_numpy(w[key])
    m.load_state_dict(sd)
    st = O.SAEState.from_state_dict(w, k=k, dead_feature_threshold=thr)
    return m, st


def ring_batch(device, D, B, seed, n_rows):
    """B rows drawn from a synthetic on-device ring, and the same rows on the host."""
    from whisper_sae.data import ActivationRing
    ring = ActivationRing(n_rows, D, device=device, dtype=torch.bfloat16)
    ring.fill_synthetic(n_rows, seed=seed)
    batch = ring.batch(B, 42, 0, 0)
    rows = batch.rows.cpu().numpy().astype(np.int64)
    x = synth.activations(n_rows, D, seed=seed, stream=0, bf16=True)[rows]
    return ring, batch, x


def one_step_against_oracle(device, tmp_path, D, H, K, B, seed, tag, lr=1e-4, n_rows=None):
    from whisper_sae.config import TrainingConfig
    from whisper_sae.sae.training import SAETrainer
    m, st = build(D, H, K, seed, 1000)
    cfg = TrainingConfig(batch_size=B, learning_rate=lr, weight_decay=0.0, epochs=1, warmup_steps=0,
                         gradient_clip=1.0, use_amp=True, num_workers=0)
    tr = SAETrainer(m, cfg, device=device, run_dir=tmp_path)
    ring, batch, x = ring_batch(device, D, B, seed, n_rows or max(4 * B, 1 << 16))
    before = {k: cpu(v).copy() for k, v in m.state_dict().items() if v.is_floating_point()}
    met = tr.train_step(batch)
    eng = m._engine
    work = eng.work(B)
    idx_dev = work["idx"].cpu().numpy()
    assert idx_dev.shape == (B, K)
    sel, clear_frac = O.reconcile_selection(st, x, idx_dev, K, "amp")
    assert clear_frac > 0.98
    st0 = st.copy()
    r = O.train_step(st, x, lr, "amp", max_norm=1.0, select=sel)
    # ---- forward products ----
    d_loss = abs(met.loss - r["loss"]) / r["loss"]
    assert d_loss < 1e-5, d_loss
    assert met.l0 == r["l0"]
    vals_o = np.take_along_axis(r["fwd"]["pre"], np.sort(sel, axis=1), axis=1)
    order = np.argsort(idx_dev, axis=1)
    vals_d = np.take_along_axis(work["vals"].cpu().numpy(), order, axis=1)
    assert rel(vals_d, vals_o) < 1e-5
    # ---- the five gradients (the optimizer kernel leaves its input untouched) ----
    d_grads = {}
    for n, key in GRAD_OF.items():
        d_grads[n] = rel(cpu(tr.optimizer.grad_view(key)), r["grads"][n])
        assert d_grads[n] < 2e-3, (n, d_grads[n])
    d_norm = abs(met.grad_norm - r["grad_norm"]) / r["grad_norm"]
    assert d_norm < 1e-4, d_norm
    assert abs(met.clip_coef - r["clip_coef"]) < 1e-4
    assert met.dead_feature_ratio == r["dead_feature_ratio"]
    # ---- parameters: the first AdamW step moves every entry by lr * g / (|g| + eps), i.e. +-lr unless g ~ 0; an
    # entry whose tiny gradient differs in sign between the two computations moves the other way (2 lr apart)
    after = {k: cpu(v) for k, v in m.state_dict().items() if v.is_floating_point()}
    want = {"encoder.weight": st.W_e, "encoder.bias": st.b_e, "decoder.weight": st.W_d, "decoder.bias": st.b_d,
            "b_pre": st.b_pre}
    agree = {}
    for key in KEYS:
        diff = np.abs(after[key].astype(np.float64) - want[key].astype(np.float64))
        agree[key] = float(np.mean(diff < 0.02 * lr))
        assert agree[key] > 0.999, (key, agree[key])
        assert diff.max() < 2.5 * lr, (key, diff.max())
        moved = np.abs(after[key] - before[key]).max()
        assert moved > 0.5 * lr, key  # the step did something
    cn = np.linalg.norm(after["decoder.weight"].astype(np.float64), axis=0)
    assert abs(cn.min() - 1) < 1e-5 and abs(cn.max() - 1) < 1e-5
    assert np.array_equal(m.feature_last_activated.cpu().numpy(), st.last_activated)
    assert int(m.step_count.item()) == st.step_count == 1
    # ---- a second step from the updated parameters: the loss keeps tracking the oracle ----
    batch2 = ring.batch(B, 42, 0, B)
    x2 = synth.activations(len(ring), D, seed=seed, stream=0, bf16=True)[batch2.rows.cpu().numpy().astype(np.int64)]
    met2 = tr.train_step(batch2)
    r2 = O.train_step(st, x2, lr, "amp", max_norm=1.0)
    d_loss2 = abs(met2.loss - r2["loss"]) / r2["loss"]
    assert d_loss2 < 2e-4, d_loss2
    note(tag, {"B": B, "dims": [D, H, K], "clear_frac": clear_frac, "d_loss": d_loss, "d_norm": d_norm,
               "d_grads": d_grads, "agree": agree, "d_loss_step2": d_loss2,
               "fallback_rows": int(eng.stats[6].item())})
    del st0
    return m, tr, ring


class TestBenchConfiguration:
    """384 -> 3072, k = 32, bf16, ring rows: B = 4096 (XCD walk with 2 batch tiles per XCD, split-K 8) and the bench's
    own B = 16384."""

    @pytest.mark.parametrize("B", [4096, 16384])
    def test_train_step_matches_amp_oracle(self, device, tmp_path, B):
        one_step_against_oracle(device, tmp_path, 384, 3072, 32, B, 42, f"cfg2_B{B}")

    def test_module_forward_backward_at_bench_batch(self, device):
        """The autograd route (module(x); loss.backward()) at B = 16384: same kernels, gradients land in .grad."""
        D, H, K, B = 384, 3072, 32, 16384
        m, st = build(D, H, K, 7, 1000, precision="bf16")
        m.to(device).train()
        _, batch, x = ring_batch(device, D, B, 7, 1 << 16)
        xt = batch.data[batch.rows.long()]
        out = m(xt)
        out.loss.backward()
        _, idx = m._last_code
        sel, _ = O.reconcile_selection(st, x, idx.cpu().numpy(), K, "amp")
        fwd = O.forward(st.copy(), x, "amp", select=sel)
        ora = O.backward(st, x, fwd, "amp")
        assert abs(float(out.loss.detach()) - float(fwd["loss"])) / float(fwd["loss"]) < 1e-5
        assert rel(cpu(out.reconstructed), fwd["reconstructed"]) < 1e-5
        got = {"W_e": m.encoder.weight.grad, "b_e": m.encoder.bias.grad, "W_d": m.decoder.weight.grad,
               "b_d": m.decoder.bias.grad, "b_pre": m.b_pre.grad}
        for n, g in got.items():
            assert rel(cpu(g), ora[n]) < 2e-3, (n, rel(cpu(g), ora[n]))


class TestBf16Trajectory:
    def test_twenty_steps_track_the_amp_oracle(self, device, tmp_path):
        """20 optimisation steps in the benchmarked arithmetic (bf16 mode, cfg-2 dimensions, LR schedule, clip,
        AdamW, renorm, dead clock) against the oracle's ``"amp"`` mode fed the same batches.  Unlike the fp32
        trajectory (G4) the two computations may part ways wherever a bf16 rounding of g / dpre / hidden falls on
        the other side, so the band is wider: losses within 1e-3 (measured 1e-4), the parameter difference below
        10 % of the 20-step update in L2 norm and 2 % of the weights' range for the renormalised decoder."""
        from whisper_sae.config import TrainingConfig
        from whisper_sae.sae.training import SAETrainer
        D, H, K, B, STEPS, lr = 384, 3072, 32, 2048, 20, 1e-3
        m, st = build(D, H, K, 11, 5, b_pre_scale=0.05)
        cfg = TrainingConfig(batch_size=B, learning_rate=lr, weight_decay=0.01, epochs=1, warmup_steps=5,
                             gradient_clip=1.0, use_amp=True, num_workers=0)
        tr = SAETrainer(m, cfg, device=device, run_dir=tmp_path)
        tr.setup_scheduler(200)
        lrs = O.lr_sequence(STEPS, lr, 5, 200)
        xs = synth.activations(B * STEPS, D, seed=11, stream=2, bf16=True).reshape(STEPS, B, D)
        w0 = st.W_e.copy()
        worst = 0.0
        for s in range(STEPS):
            assert abs(tr.optimizer.param_groups[0]["lr"] - lrs[s]) < 1e-12
            met = tr.train_step(torch.from_numpy(xs[s]))
            r = O.train_step(st, xs[s], lrs[s], "amp", max_norm=1.0, weight_decay=0.01)
            d = abs(met.loss - r["loss"]) / r["loss"]
            worst = max(worst, d)
            assert d < 1e-3, (s, d)
            assert abs(met.l0 - r["l0"]) < 0.05, s
            assert abs(met.dead_feature_ratio - r["dead_feature_ratio"]) < 2e-3, s
        sd = {k: cpu(v) for k, v in m.state_dict().items() if v.is_floating_point()}
        upd = np.abs(st.W_e - w0).max()
        d_we = np.abs(sd["encoder.weight"] - st.W_e).max() / upd
        d_wd = np.abs(sd["decoder.weight"] - st.W_d).max() / np.abs(st.W_d).max()
        d_bp = np.abs(sd["b_pre"] - st.b_pre).max() / max(np.abs(st.b_pre).max(), 1e-30)
        frac = float(np.mean(np.abs(sd["encoder.weight"] - st.W_e) < 0.02 * upd))
        l2 = float(np.linalg.norm((sd["encoder.weight"] - st.W_e).astype(np.float64))
                   / np.linalg.norm((st.W_e - w0).astype(np.float64)))
        note("bf16_trajectory", {"worst_loss": worst, "d_we_over_update": float(d_we), "d_wd": float(d_wd),
                                 "d_bpre": float(d_bp), "frac_close": frac, "l2_diff_over_update": l2})
        assert frac > 0.95 and d_we < 0.5 and l2 < 0.1   # measured: 0.977, 0.18
        assert d_wd < 2e-2 and d_bp < 2e-2
        assert int(m.step_count.item()) == st.step_count == STEPS
        assert np.mean(m.feature_last_activated.cpu().numpy() == st.last_activated) > 0.995
        osd = tr.optimizer.state_dict()
        assert float(osd["state"][1]["step"]) == STEPS


class TestConfigs3:
    """BASELINE.json configs[3] dimensions: 768 -> 12288, k = 64, resampling on.  B = 2048 takes the persistent GEMM
    (8 batch tiles x 48 feature tiles), the two-maxima strip TopK, the generic decode kernel and the weight-gradient
    kernel with two column tiles."""

    def test_train_step_then_resample(self, device, tmp_path):
        D, H, K, B = 768, 12288, 64, 2048
        m, tr, ring = one_step_against_oracle(device, tmp_path, D, H, K, B, 31, "cfg4_B2048", n_rows=1 << 14)
        # ---- resample_dead_features on the trained-once model, against the oracle from the SAME parameters ----
        w = {k: cpu(v) for k, v in m.state_dict().items() if v.is_floating_point()}
        st = O.SAEState.from_state_dict(w, k=K, dead_feature_threshold=20)
        m.dead_feature_threshold = 20
        dead_idx = np.unique((synth.counter_u64(400, 31, 50) % np.uint64(H)).astype(np.int64))[:57]
        with torch.no_grad():
            m.step_count.fill_(100)
            la = torch.full((H,), 95, dtype=torch.long)
            la[torch.from_numpy(dead_idx)] = 3
            m.feature_last_activated.copy_(la.to(device))
        st.step_count = 100
        st.last_activated = la.numpy().copy()
        xr = synth.activations(B, D, seed=31, stream=9, bf16=True)
        m.precision = "bf16"
        m.train()
        ret = m.resample_dead_features(torch.from_numpy(xr).to(device))
        res = O.resample_dead_features(st, xr, None, mode="amp", training=True)
        assert ret == res["returned"] == len(dead_idx)
        after = {k: (cpu(v) if v.is_floating_point() else v.cpu().numpy()) for k, v in m.state_dict().items()}
        assert int(after["step_count"]) == st.step_count == 101
        assert np.array_equal(after["feature_last_activated"], st.last_activated)
        assert np.array_equal(np.sort(res["rewritten"]), dead_idx)
        assert rel(after["encoder.weight"][dead_idx], st.W_e[dead_idx]) < 1e-6
        assert rel(after["decoder.weight"][:, dead_idx], st.W_d[:, dead_idx]) < 1e-6
        assert np.array_equal(after["encoder.bias"][dead_idx], np.zeros(len(dead_idx), np.float32))
        untouched = np.setdiff1d(np.arange(H), dead_idx)
        assert np.array_equal(after["encoder.weight"][untouched], w["encoder.weight"][untouched])
        # the trainer keeps stepping on the rewritten parameters (shadows refreshed by the resample call)
        met = tr.train_step(ring.batch(B, 42, 0, 2 * B))
        assert np.isfinite(met.loss) and met.loss > 0


class TestInterleavedCalls:
    """a forward's staged operands (xT, g, gT in the ctx) are overwritten by any later call that stages
    a batch; backward must notice and rebuild them."""

    @pytest.mark.parametrize("intruder", ["encode", "pre_activation", "encode_compact", "resample", "forward"])
    def test_backward_after_another_call(self, device, intruder):
        D, H, K = 128, 1024, 16
        m, st = build(D, H, K, 13, 20, precision="fp32")
        m.to(device).train()
        x = synth.activations(96, D, seed=13, stream=1, bf16=False)
        y = torch.from_numpy(synth.activations(160, D, seed=13, stream=2, bf16=False)).to(device)
        out = m(torch.from_numpy(x).to(device))
        if intruder == "encode":
            m.encode(y)
        elif intruder == "pre_activation":
            m.pre_activation(y)
        elif intruder == "encode_compact":
            m.encode_compact(y)
        elif intruder == "forward":
            m.eval()
            m(y)
            m.train()
        else:
            with torch.no_grad():
                m.feature_last_activated[:7] = -100  # a few dead features -> the resample forward really runs
            m.eval()  # (eval: the resample forward leaves the clock alone; it still rewrites 7 features)
            m.resample_dead_features(y)
            m.train()
        out.loss.backward()
        if intruder == "resample":  # parameters changed under the graph: only shapes / finiteness are defined
            assert torch.isfinite(m.encoder.weight.grad).all()
            return
        fwd = O.forward(st.copy(), x, "fp32")
        ora = O.backward(st, x, fwd, "fp32")
        got = {"W_e": m.encoder.weight.grad, "b_e": m.encoder.bias.grad, "W_d": m.decoder.weight.grad,
               "b_d": m.decoder.bias.grad, "b_pre": m.b_pre.grad}
        for n, g in got.items():
            assert rel(cpu(g), ora[n]) < 2e-5, (n, rel(cpu(g), ora[n]))


class TestConfigs4:
    """BASELINE.json configs[4] dimensions: 1280 -> 40960 ReLU + L1 (whisper-large-v3, 32x).  One trainer step in
    bf16 mode against the float64 oracle's forward / backward on the same weights (ragged batch: the persistent
    split-K GEMMs with a partly filled last tile)."""

    @pytest.mark.parametrize("B", [600, 512])  # 600: ragged (general path); 512: the row-major-GEMM flow, no fp32 hidden at all
    def test_relu_step_at_1280_40960(self, device, tmp_path, B):
        from whisper_sae.config import TrainingConfig
        from whisper_sae.sae.model import ReLUSAE
        from whisper_sae.sae.training import SAETrainer
        D, H, weight = 1280, 40960, 0.01
        w = synth.sae_weights(D, H, seed=17, bf16=True)
        m = ReLUSAE(D, H, sparsity_weight=weight)
        sd = m.state_dict()
        for key in ("encoder.weight", "encoder.bias", "decoder.weight", "decoder.bias"):
            sd[key] = torch.from_numpy(w[key])
        m.load_state_dict(sd)
        cfg = TrainingConfig(batch_size=B, learning_rate=1e-4, weight_decay=0.0, epochs=1, warmup_steps=0,
                             gradient_clip=1.0, use_amp=True, num_workers=0)
        tr = SAETrainer(m, cfg, device=device, run_dir=tmp_path)
        x = synth.activations(B, D, seed=17, stream=2, bf16=True)
        met = tr.train_step(torch.from_numpy(x).to(device))
        args = (w["encoder.weight"], w["encoder.bias"], w["decoder.weight"], w["decoder.bias"], x)
        f = O.relu_forward(*args, sparsity_weight=weight)
        gr = O.relu_backward(*args, f, sparsity_weight=weight)
        d_loss = abs(met.loss - float(f["loss"])) / float(f["loss"])
        d_l1 = abs(met.sparsity_loss - float(f["sparsity_loss"])) / float(f["sparsity_loss"])
        assert d_loss < 5e-3 and d_l1 < 5e-3, (d_loss, d_l1)   # bf16 operands against the fp32 reference values
        assert abs(met.l0 - float(f["l0"])) / float(f["l0"]) < 5e-3
        d = {}
        for n, key in (("W_e", "encoder.weight"), ("b_e", "encoder.bias"), ("W_d", "decoder.weight"),
                       ("b_d", "decoder.bias")):
            got, want = cpu(tr.optimizer.grad_view(key)).astype(np.float64), gr[n].astype(np.float64)
            d[n] = float(np.linalg.norm(got - want) / np.linalg.norm(want))
            assert d[n] < 2e-2, (n, d[n])
        note(f"cfg5_relu_B{B}", {"d_loss": d_loss, "d_l1": d_l1, "grad_rel_l2": d})
        cn = m.decoder.weight.detach().norm(dim=0)
        assert torch.allclose(cn, torch.ones_like(cn), atol=1e-5)
