"""BatchTopK SAE without a GPU: the test oracle against plain restatements of the definition, the config surface, the
module's construction and state dict, and the C ABI symbols."""

from __future__ import annotations

import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import batch_topk_oracle as BO

ROOT = Path(__file__).resolve().parents[1]


def sorted_candidates(pre: np.ndarray, k_max: int) -> tuple:
    order = np.argsort(-pre.astype(np.float64), axis=1, kind="stable")[:, :k_max]
    return np.take_along_axis(pre, order, axis=1).astype(np.float32), order


def dense(vals, idx, H):
    out = np.zeros((vals.shape[0], H), np.float32)
    np.put_along_axis(out, idx, vals, axis=1)
    return out


@pytest.mark.parametrize("B,H,k", [(1, 64, 8), (7, 128, 5), (64, 256, 16)])
def test_uncapped_equals_flat_topk_of_relu(B, H, k):
    """k_max = H: the selection is BatchTopK without a cap, relu(pre).flatten().topk(B k)."""
    rng = np.random.default_rng(B * 1000 + H)
    pre = rng.standard_normal((B, H)).astype(np.float32)
    vals, idx = sorted_candidates(pre, H)
    masked, t, sat, kept = BO.batch_select(vals, k, H)
    flat = torch.relu(torch.from_numpy(pre)).flatten()
    top = flat.topk(B * k)
    want = torch.zeros_like(flat)
    want[top.indices] = top.values
    got = dense(masked, idx, H)
    assert np.array_equal(got, want.view(B, H).numpy())
    assert kept == int((want > 0).sum()) and sat == 0
    assert t == float(top.values[top.values > 0].min())


def test_capped_equals_largest_subject_to_cap():
    """One row carries most of the signal: it saturates at k_max, and the rest goes to the other rows in value order."""
    B, H, k, km = 16, 256, 4, 8
    rng = np.random.default_rng(3)
    pre = rng.standard_normal((B, H)).astype(np.float32)
    pre[5] += 6.0  # row 5 outranks everything else
    vals, idx = sorted_candidates(pre, km)
    masked, t, sat, kept = BO.batch_select(vals, k, H)
    # greedy restatement: global value order, skip a row once it holds k_max, stop at B k
    order = np.argsort(-pre.ravel(), kind="stable")
    want = np.zeros_like(pre)
    per_row = np.zeros(B, int)
    n = 0
    for flat in order:
        r, c = divmod(int(flat), H)
        if pre[r, c] <= 0 or n == B * k:
            break
        if per_row[r] == km:
            continue
        want[r, c] = pre[r, c]
        per_row[r] += 1
        n += 1
    assert np.array_equal(dense(masked, idx, H), want)
    assert sat == 1 and per_row[5] == km and kept == B * k


def test_ties_negatives_and_too_few_positives():
    vals = np.array([[3, 2, 2, 2], [2, 1, -1, -2], [-1, -2, -3, -4]], np.float32)
    masked, t, sat, kept = BO.batch_select(vals, 1, 16)  # B k = 3: the third largest positive is 2, all ties kept
    assert t == 2 and kept == 5 and sat == 1
    assert masked.tolist() == [[3, 2, 2, 2], [2, 0, 0, 0], [0, 0, 0, 0]]
    masked, t, sat, kept = BO.batch_select(vals, 4, 16)  # 12 wanted, 6 positive: keep every positive candidate
    assert t == 1 and kept == 6
    masked, t, sat, kept = BO.batch_select(-np.abs(vals) - 1, 2, 16)
    assert t == -1 and kept == 0 and not masked.any()
    masked, t, sat, kept = BO.batch_select(vals, 1, 16, theta=1.5, eval_mode=True)
    assert kept == 5 and t == np.float32(1.5)


def test_ema_rounds_once_per_operation():
    assert BO.ema(-1.0, 0.25, 0.999) == np.float32(0.25)
    th = np.float32(0.3)
    want = np.float32(np.float32(np.float32(0.999) * th) + np.float32(np.float32(1 - np.float32(0.999)) * np.float32(0.5)))
    assert BO.ema(th, 0.5, 0.999) == want


def test_config_accepts_batchtopk_and_validates(tmp_path):
    from whisper_sae.config import ExperimentConfig, SAEConfig
    c = SAEConfig(activation="batchtopk", k=32, batch_topk_max_k=64, batch_topk_threshold_beta=0.99)
    assert c.batch_topk_max_k == 64 and c.batch_topk_threshold_beta == 0.99
    assert SAEConfig().batch_topk_max_k is None and SAEConfig().batch_topk_threshold_beta == 0.999
    for bad in (dict(batch_topk_max_k=16), dict(batch_topk_max_k=129), dict(batch_topk_threshold_beta=1.0),
                dict(batch_topk_threshold_beta=-0.1), dict(k=129)):
        with pytest.raises(ValueError):
            SAEConfig(activation="batchtopk", **{"k": 32, **bad})
    e = ExperimentConfig(sae=c)
    e.to_yaml(tmp_path / "c.yaml")
    back = ExperimentConfig.from_yaml(tmp_path / "c.yaml")
    assert back.sae == c
    shipped = ExperimentConfig.from_yaml(ROOT / "configs" / "batchtopk_default.yaml")
    assert shipped.sae.activation == "batchtopk"


def test_create_sae_builds_batchtopk_with_cap_and_beta():
    from whisper_sae.config import SAEConfig
    from whisper_sae.sae import BatchTopKSAE, create_sae
    m = create_sae(SAEConfig(activation="batchtopk", k=32, expansion_factor=8), 384)
    assert isinstance(m, BatchTopKSAE)
    assert (m.k, m.max_k_per_row, m.threshold_beta, m.hidden_dim) == (32, 64, 0.999, 3072)
    m = create_sae(SAEConfig(activation="batchtopk", k=80, batch_topk_max_k=100, batch_topk_threshold_beta=0.9), 64)
    assert (m.k, m.max_k_per_row, m.threshold_beta) == (80, 100, 0.9)
    assert BatchTopKSAE(32, 64, k=40).max_k_per_row == 64  # min(2 k, 128, H)
    assert BatchTopKSAE(384, 3072, k=100).max_k_per_row == 128
    with pytest.raises(ValueError):
        BatchTopKSAE(32, 64, k=8, max_k_per_row=4)
    with pytest.raises(ValueError):
        BatchTopKSAE(32, 64, k=8, threshold_beta=1.0)


def test_state_dict_carries_the_threshold():
    from whisper_sae.sae import BatchTopKSAE, TopKSAE
    m = BatchTopKSAE(64, 256, k=8)
    sd = m.state_dict()
    assert "threshold" in sd and float(sd["threshold"]) == -1.0 and sd["threshold"].dtype == torch.float32
    sd["threshold"] = torch.tensor(0.75)
    m.load_state_dict(sd)
    assert float(m.threshold) == 0.75
    assert set(sd) - set(TopKSAE(64, 256, k=8).state_dict()) == {"threshold"}
    torch.manual_seed(0)
    a = BatchTopKSAE(64, 256, k=8).state_dict()
    torch.manual_seed(0)
    b = TopKSAE(64, 256, k=8).state_dict()
    for key in b:  # same construction and RNG draws as TopKSAE
        assert torch.equal(a[key], b[key])


def test_header_and_library_export_the_batch_topk_abi():
    from whisper_sae import _native as N
    text = (ROOT / "include" / "wsae.h").read_text()
    for name in ("wsae_batch_topk_select", "wsae_ctx_set_batch_topk"):
        assert re.search(rf"\b{name}\s*\(", text) and name in N.SIGNATURES
    assert "typedef struct wsae_batch_topk_state" in text
    for macro, val in (("WSAE_BTK_TRAIN", N.BTK_TRAIN), ("WSAE_BTK_EVAL", N.BTK_EVAL), ("WSAE_BTK_SELECT", N.BTK_SELECT)):
        assert re.search(rf"#define {macro} {val}\b", text)
    lib = N.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", str(N.library_path())], capture_output=True, text=True,
                         check=True).stdout
    assert {"wsae_batch_topk_select", "wsae_ctx_set_batch_topk"} <= set(re.findall(r"\bT (wsae_[a-z0-9_]+)\b", out))
    assert lib.wsae_ctx_set_batch_topk(None, 8, 0, None) == -1 and "null ctx" in N.last_error()
    assert lib.wsae_batch_topk_select(None, None, 1, 1, 0, None, None) == -1

