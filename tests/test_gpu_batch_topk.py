"""BatchTopK SAE on the MI355X: the selection kernel against numpy (exact), the module's forward and gradients against
the test oracle at the shapes that take each encode / decode branch, the trainer over 20 steps, eval mode, resampling,
and a TopK step that must not notice the feature."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import batch_topk_oracle as BO
from oracle import sae_oracle as O
from oracle import synth

pytestmark = pytest.mark.gpu

KEYS = ("encoder.weight", "encoder.bias", "decoder.weight", "decoder.bias", "b_pre")
GRADS = {"W_e": "encoder.weight", "b_e": "encoder.bias", "W_d": "decoder.weight", "b_d": "decoder.bias", "b_pre": "b_pre"}
MODE = {"bf16": "amp", "fp32": "fp32"}
# the bounds of test_gpu_kernel_variants.py (suite bounds 1e-5 for loss / recon, gradients per precision)
GRAD_REL = {"fp32": dict.fromkeys(GRADS, 2.5e-6),
            "bf16": {"W_e": 2e-3, "b_e": 2e-3, "W_d": 2e-3, "b_d": 2.5e-6, "b_pre": 2.5e-6}}
D, H, K, KMAX = 384, 3072, 32, 64


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def cpu(t):
    return t.detach().float().cpu().numpy()


def load(m, w, device):
    sd = m.state_dict()
    for key in KEYS:
        sd[key] = torch.from_numpy(np.ascontiguousarray(w[key]))
    m.load_state_dict(sd)
    return m.to(device)


def make(device, w, precision, k=K, kmax=KMAX, thr=1000, beta=0.999):
    from whisper_sae.sae import BatchTopKSAE
    d, h = w["b_pre"].shape[0], w["encoder.bias"].shape[0]
    m = load(BatchTopKSAE(d, h, k=k, max_k_per_row=kmax, threshold_beta=beta, dead_feature_threshold=thr,
                          precision=precision), w, device).train()
    return m, O.SAEState.from_state_dict(w, k=kmax, dead_feature_threshold=thr)


# ---- 1. the selection kernel alone ------------------------------------------------------------------------------------
class Selector:
    """A ctx of code width ``km`` and hidden width ``H_`` for calls of ``wsae_batch_topk_select`` alone."""

    def __init__(self, device, B, km, H_):
        from whisper_sae import _native as N
        from whisper_sae.sae.engine import SAEEngine
        self.N, self.device = N, device
        self.eng = SAEEngine(device, 32, H_, km)
        self.handle = self.eng.ctx(N.PREC_FP32, B)

    def __call__(self, vals, k, mode=0, theta=-1.0, beta=0.999):
        N, eng = self.N, self.eng
        rec = torch.zeros(N.BTK_STATE_WORDS, dtype=torch.int32, device=self.device)
        rec.view(torch.float32)[0] = theta
        rec.view(torch.float32)[1] = beta
        v = torch.from_numpy(vals).to(self.device)
        N.check(eng.lib.wsae_batch_topk_select(self.handle, v.data_ptr(), vals.shape[0], k, mode, rec.data_ptr(),
                                               eng.stream()), "wsae_batch_topk_select")
        out, r = v.cpu().numpy(), rec.cpu()
        return out, r.view(torch.float32)[:3].tolist(), int(r[3]), int(r[4])


def select_on_device(device, vals, k, H_, mode=0, theta=-1.0, beta=0.999):
    sel = Selector(device, vals.shape[0], vals.shape[1], H_)
    try:
        return sel(vals, k, mode, theta, beta)
    finally:
        sel.eng.close()


def candidates(B, km, seed, kind):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((B, km)).astype(np.float32) * np.float32(0.5) + np.float32(0.3)
    if kind == "ties":  # many exact duplicates, some of them at the cut
        v = np.round(v * 8) / 8
    elif kind == "neg_rows":  # a third of the rows have no positive candidate
        v[::3] = -np.abs(v[::3]) - 0.01
    elif kind == "few_pos":  # fewer positives than B k
        v = v - 2.0
    elif kind == "saturated":  # row 0 outranks the batch
        v[0] = np.abs(v[0]) + 100.0
    return -np.sort(-v, axis=1).astype(np.float32)


@pytest.mark.parametrize("km", [32, 64, 128])
@pytest.mark.parametrize("B", [1, 7, 300, 2048, 16384])
def test_selection_kernel_exact(device, B, km):
    run = Selector(device, B, km, 4096)
    for kind in ("plain", "ties", "neg_rows", "few_pos", "saturated"):
        k = max(1, km // 2)
        vals = candidates(B, km, B * 131 + km, kind)
        want, t, sat, kept = BO.batch_select(vals, k, 4096)
        got, (theta, _, last_t), dsat, dkept = run(vals, k)
        assert np.array_equal(got, want), (kind, int((got != want).sum()))
        assert (dkept, dsat) == (kept, sat), kind
        assert np.float32(last_t) == t, kind
        assert np.float32(theta) == (t if kept else np.float32(-1.0)), kind  # first training selection: theta = t
        if kind == "saturated" and B > 1:
            assert sat >= 1
        again = run(vals, k)
        assert np.array_equal(again[0].view(np.uint32), got.view(np.uint32)) and again[1:] == (
            [theta, float(np.float32(0.999)), last_t], dsat, dkept)
    run.eng.close()


def test_selection_kernel_modes_and_ema(device):
    vals = candidates(300, 64, 5, "plain")
    want, t, _, _ = BO.batch_select(vals, 16, 4096)
    # training with a trained threshold: the EMA, rounded once per operation
    _, (theta, _, last_t), _, _ = select_on_device(device, vals, 16, 4096, mode=0, theta=0.4, beta=0.9)
    assert np.float32(theta) == BO.ema(0.4, t, 0.9) and np.float32(last_t) == t
    # eval with a trained threshold: strict v > theta, theta unchanged
    got, (theta, _, last_t), sat, kept = select_on_device(device, vals, 16, 4096, mode=1, theta=0.4)
    w2, _, s2, k2 = BO.batch_select(vals, 16, 4096, theta=0.4, eval_mode=True)
    assert np.array_equal(got, w2) and (sat, kept) == (s2, k2) and np.float32(theta) == np.float32(0.4)
    # eval before any training and "select": the batch selection, theta left at -1
    for mode in (1, 2):
        got, (theta, _, _), _, _ = select_on_device(device, vals, 16, 4096, mode=mode)
        assert np.array_equal(got, want) and theta == -1.0
    # k_max = H: no row counts as saturated
    _, _, sat, _ = select_on_device(device, candidates(7, 64, 9, "saturated"), 8, 64)
    assert sat == 0


# ---- 2 + 3. forward and gradients against the oracle ----------------------------------------------------------------
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("B", [300, 2048, 16384])
def test_forward_and_grads_match_oracle(device, B, prec):
    mode = MODE[prec]
    w = synth.sae_weights(D, H, seed=B + 7, bf16=True, b_pre_scale=0.1)
    x = synth.activations(B, D, seed=B + 7, stream=1, bf16=True)
    m, st = make(device, w, prec)
    out = m(torch.from_numpy(x).to(device))
    out.loss.backward()
    vals, idx = (cpu(t) for t in m._last_code)
    keep_dev = cpu(out.hidden) > 0
    keep, pre, t, bad = BO.dense_selection(st, x, mode, K, KMAX, idx.astype(np.int64), keep_dev)
    assert bad == 0, f"{bad} kept/dropped decisions differ clear of t"
    sel = m.last_selection()
    assert abs(sel.threshold - float(t)) <= 1e-5 * abs(float(t)) and sel.kept == int(keep_dev.sum())
    assert float(m.threshold) == sel.threshold  # first training forward: theta = t
    nblk = 8 if B >= 16384 else 1
    bs = B // nblk
    sse, fired, grads, recon = 0.0, np.zeros(H, bool), {n: 0.0 for n in GRADS}, []
    for b in range(nblk):
        rows = slice(b * bs, (b + 1) * bs)
        fwd = BO.forward_from_keep(st, x[rows], keep[rows], pre[rows], mode)
        ora = O.backward(st, x[rows], fwd, mode)
        r = fwd["reconstructed"].astype(np.float64) - x[rows].astype(np.float64)
        sse += float((r * r).sum())
        fired |= (fwd["hidden"] > 0).any(axis=0)
        recon.append(fwd["reconstructed"])
        for n in GRADS:
            grads[n] = grads[n] + ora[n].astype(np.float64) / nblk
    loss = sse / x.size
    assert abs(float(out.loss.detach()) - loss) / loss < 1e-5
    assert rel(cpu(out.reconstructed), np.concatenate(recon)) < 1e-5
    assert float(out.l0) == np.float32(keep.sum() / B)
    st.step_count += 1
    st.last_activated[fired] = st.step_count
    assert np.array_equal(m.feature_last_activated.cpu().numpy(), st.last_activated)
    params = dict(m.named_parameters())
    for n, key in GRADS.items():
        assert rel(cpu(params[key].grad), grads[n]) < GRAD_REL[prec][n], (n, rel(cpu(params[key].grad), grads[n]))


# ---- 4. the trainer ---------------------------------------------------------------------------------------------------
def test_trainer_tracks_oracle_over_20_steps(device, tmp_path):
    from whisper_sae.config import TrainingConfig
    from whisper_sae.sae import SAETrainer
    B, steps, lr = 512, 20, 1e-3
    w = synth.sae_weights(D, H, seed=11, bf16=True, b_pre_scale=0.1)
    m, st = make(device, w, "fp32", beta=0.9)
    tr = SAETrainer(m, TrainingConfig(batch_size=B, learning_rate=lr, warmup_steps=0, use_amp=False, num_workers=0),
                    device=str(device), run_dir=tmp_path)
    theta_o, theta_dev_chain = np.float32(-1), np.float32(-1)
    for s in range(steps):
        x = synth.activations(B, D, seed=11, stream=s + 1, bf16=True)
        met = tr.train_step(torch.from_numpy(x))
        work = m._engine.work(B)
        idx, vals = cpu(work["idx"]).astype(np.int64), cpu(work["vals"])
        keep_dev = np.zeros((B, H), bool)
        np.put_along_axis(keep_dev, idx, vals > 0, axis=1)
        keep, pre, t, bad = BO.dense_selection(st, x, "fp32", K, KMAX, idx, keep_dev)
        assert bad == 0, (s, bad)
        ref = BO.train_step(st, x, keep, pre, lr, "fp32")
        assert abs(met.loss - ref["loss"]) / ref["loss"] < 1e-4 and met.l0 == np.float32(ref["l0"])
        sel = m.last_selection()
        theta_o = BO.ema(theta_o, t, 0.9)
        theta_dev_chain = BO.ema(theta_dev_chain, sel.threshold, 0.9)
        assert np.float32(float(m.threshold)) == theta_dev_chain  # the device EMA, exact to fp32 rounding
    assert abs(float(m.threshold) - float(theta_o)) <= 1e-5 * abs(float(theta_o))
    sd = m.state_dict()
    for n, key in GRADS.items():
        got = sd[key].cpu().numpy()
        assert rel(got, getattr(st, n)) < 1e-4, (n, rel(got, getattr(st, n)))
    assert np.array_equal(m.feature_last_activated.cpu().numpy(), st.last_activated)
    path = tr.save_checkpoint("c.pt")
    ck = torch.load(path, map_location="cpu")
    assert float(ck["model_state_dict"]["threshold"]) == float(m.threshold)
    m2, _ = make(device, w, "fp32")
    m2.load_state_dict(ck["model_state_dict"])
    assert float(m2.threshold) == float(m.threshold)


# ---- 5. eval mode ----------------------------------------------------------------------------------------------------
def test_eval_mode_uses_the_threshold(device):
    from whisper_sae.sae import TopKSAE
    B = 2048
    w = synth.sae_weights(D, H, seed=3, bf16=True, b_pre_scale=0.1)
    x = torch.from_numpy(synth.activations(B, D, seed=3, stream=1, bf16=True)).to(device)
    m, _ = make(device, w, "bf16")
    with torch.no_grad():
        m(x)  # one training forward: theta = t of this batch
        theta = float(m.threshold)
        assert theta > 0
        m.threshold.mul_(1.1)  # a threshold that is not this batch's own cut
        theta = float(m.threshold)
        m.eval()
        out = m(x)
        vals, idx = m.encode_compact(x)
    assert float(m.threshold) == theta  # eval forwards and encodes leave it alone
    plain = load(TopKSAE(D, H, k=KMAX, precision="bf16"), w, device).eval()
    cv, ci = plain.encode_compact(x)
    cv = cv.cpu().numpy()
    want = np.where((cv > 0) & (cv > np.float32(theta)), cv, 0)
    assert np.array_equal(ci.cpu().numpy(), idx.cpu().numpy()) and np.array_equal(vals.cpu().numpy(), want)
    assert float(out.l0) == np.float32((want > 0).sum() / B)


def test_single_row_equals_topk(device):
    """B = 1, k_max = k, a row with >= k positive candidates: BatchTopK is TopK, bit for bit."""
    from whisper_sae.sae import TopKSAE
    for prec in ("bf16", "fp32"):
        w = synth.sae_weights(D, H, seed=21, bf16=True, b_pre_scale=0.1)
        x = torch.from_numpy(synth.activations(1, D, seed=21, stream=1, bf16=True)).to(device)
        m, _ = make(device, w, prec, k=K, kmax=K)
        t = load(TopKSAE(D, H, k=K, precision=prec), w, device).train()
        a, b = m(x), t(x)
        assert (cpu(b.hidden) > 0).sum() == K
        a.loss.backward()
        b.loss.backward()
        for f in ("reconstructed", "hidden", "loss", "l0"):
            assert torch.equal(getattr(a, f), getattr(b, f)), f
        pa, pb = dict(m.named_parameters()), dict(t.named_parameters())
        for key in KEYS:
            assert torch.equal(pa[key].grad, pb[key].grad), key


# ---- 6. resampling ---------------------------------------------------------------------------------------------------
def test_resample_over_batch_selected_code(device):
    B = 1024
    w = synth.sae_weights(D, H, seed=5, bf16=True, b_pre_scale=0.1)
    x = synth.activations(B, D, seed=5, stream=2, bf16=True)
    m, st = make(device, w, "fp32", thr=10)
    la = np.zeros(H, np.int64)
    la[: H // 2] = 100  # the first half fired recently; the second half is dead at step 100
    with torch.no_grad():
        m.feature_last_activated.copy_(torch.from_numpy(la))
        m.step_count.fill_(100)
        m.threshold.fill_(0.5)
    st.last_activated, st.step_count = la.copy(), 100
    xd = torch.from_numpy(x).to(device)
    vals, idx = m.encode_compact(xd)  # training mode: the batch selection, threshold untouched
    assert float(m.threshold) == 0.5
    keep_dev = np.zeros((B, H), bool)
    np.put_along_axis(keep_dev, cpu(idx).astype(np.int64), cpu(vals) > 0, axis=1)
    keep, pre, _, bad = BO.dense_selection(st, x, "fp32", K, KMAX, cpu(idx).astype(np.int64), keep_dev)
    assert bad == 0
    n = m.resample_dead_features(xd, num_resample=64)
    ref = BO.resample_dead_features(st, x, keep, pre, "fp32", num_resample=64)
    assert n == ref["returned"] == 64
    assert float(m.threshold) == 0.5
    sd = m.state_dict()
    assert np.array_equal(m.feature_last_activated.cpu().numpy(), st.last_activated)
    for n_, key in GRADS.items():
        assert rel(sd[key].cpu().numpy(), getattr(st, n_)) < 1e-6, n_


# ---- 7. TopK does not notice the feature --------------------------------------------------------------------------------
def test_topk_step_unchanged_by_an_idle_selection(device, tmp_path):
    """A TopKSAE ctx that had the selection set and cleared again computes the same step, bit for bit."""
    from whisper_sae import _native as N
    from whisper_sae.config import TrainingConfig
    from whisper_sae.sae import SAETrainer, TopKSAE
    B = 2048
    w = synth.sae_weights(D, H, seed=8, bf16=True, b_pre_scale=0.1)
    x = torch.from_numpy(synth.activations(B, D, seed=8, stream=1, bf16=True))
    res = []
    for touch in (False, True):
        m = load(TopKSAE(D, H, k=K), w, device).train()
        tr = SAETrainer(m, TrainingConfig(batch_size=B, learning_rate=1e-4, warmup_steps=0, use_amp=True, num_workers=0),
                        device=str(device), run_dir=tmp_path)
        if touch:
            eng = m.bind()
            handle = eng.prepare(N.PREC_BF16, B)
            rec = torch.zeros(N.BTK_STATE_WORDS, dtype=torch.int32, device=device)
            N.check(eng.lib.wsae_ctx_set_batch_topk(handle, 8, N.BTK_TRAIN, rec.data_ptr()), "set")
            N.check(eng.lib.wsae_ctx_set_batch_topk(handle, 0, N.BTK_TRAIN, 0), "clear")
        met = tr.train_step(x)
        res.append((met.loss, met.l0, {k_: v.clone() for k_, v in m.state_dict().items()}))
    assert res[0][:2] == res[1][:2]
    for key in res[0][2]:
        assert torch.equal(res[0][2][key], res[1][2][key]), key
