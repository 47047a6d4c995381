"""Group effect sizes without a GPU: the numpy oracle against closed forms and against itself under another summation
order (on the inputs the GPU test uses), ``bootstrap_weights``, every argument error of ``wsae_pool_update`` /
``wsae_group_effect`` (raised before any HIP call), the header / ``SIGNATURES`` / exports, the Python layer's errors."""

from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest

import group_stats_oracle as GO

HEADER = Path(__file__).resolve().parents[1] / "include" / "wsae.h"
NAMES = ("wsae_pool_workspace_bytes", "wsae_pool_update", "wsae_group_effect_workspace_bytes", "wsae_group_effect")


def test_oracle_pooling_is_sequential_float32_in_row_order():
    big = np.float32(2 ** 24)
    # rows 0..2 of segment 1 hit feature 3: 2^24 + 1 + 1 stays 2^24 in float32, 1 + 1 + 2^24 does not
    vals = np.array([[big, 2.0], [1.0, -1.0], [1.0, 0.0], [5.0, 7.0]], np.float32)
    idx = np.array([[3, 0], [3, 1], [3, 2], [9, 3]], np.int32)
    sums, cnt, rows = GO.pool((vals, idx), 8, [1, 1, 1, 0], 2)
    assert sums[1, 3] == big and cnt[1, 3] == 3 and sums[1, 0] == 2.0 and rows.tolist() == [1, 3]
    assert sums[0, 3] == 7.0 and sums[0].sum() == 7.0  # index 9 >= hidden is ignored
    assert cnt[1, 1] == 0 and cnt[1, 2] == 0            # values <= 0 do not fire
    back = GO.pool((vals[::-1], idx[::-1]), 8, [0, 1, 1, 1], 2)[0]
    assert back[1, 3] == big + 2
    # padding rows, a window, and a continuation equal to the single call
    seg = np.array([-1, 1, 2, 0])
    win = GO.pool((vals, idx), 8, seg, 2, f_lo=2, f_cols=3)
    assert win[2].tolist() == [1, 1] and win[0][1].tolist() == [0.0, 1.0, 0.0] and win[0][0].tolist() == [0.0, 7.0, 0.0]
    rng = np.random.default_rng(0)
    code = GO.random_code(rng, 90, 5, 16)
    seg = np.sort(rng.integers(-1, 5, 90))
    one = GO.pool(code, 16, seg, 4)
    two = GO.pool((code[0][40:], code[1][40:]), 16, seg[40:], 4, state=GO.pool((code[0][:40], code[1][:40]), 16, seg[:40], 4))
    assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(one, two))
    # a repeated index within a row: every occurrence is added, in entry order
    rep = GO.pool((np.array([[big, 1.0, 1.0]], np.float32), np.array([[2, 2, 2]], np.int32)), 4, [0], 1)
    assert rep[0][0, 2] == big and rep[1][0, 2] == 3


def test_oracle_effect_sizes_against_closed_forms():
    # two tiny groups by hand: a = (1, 2, 3), b = (2, 4, 6): means 2 and 4, variances 1 and 4
    X = np.array([[1, 5], [2, 7], [2, 5], [4, 7], [3, 5], [6, 7], [100, 100]], np.float32)
    group = [0, 1, 0, 1, 0, 1, 2]
    out = GO.effect(X, group)
    d = -2.0 / np.sqrt(2.5)
    assert out["record"] == (3, 3, 0)
    assert np.isclose(out["mean_a"][0], 2.0, rtol=0, atol=1e-15) and np.isclose(out["mean_b"][0], 4.0, rtol=0, atol=1e-15)
    assert abs(out["d"][0] - d) < 1e-15 and abs(out["g"][0] - d * (1 - 3 / 15)) < 1e-15
    assert out["d"][1] == 0.0 and out["g"][1] == 0.0  # s_p = 0 gives d = 0, not inf
    assert np.all(np.isnan(out["ci_lo"])) and np.all(np.isnan(out["se"]))
    # a divisor rescales, div <= 0 leaves the utterance out, fewer than two members give NaN
    out2 = GO.effect(2 * X, group, div=[2, 2, 2, 2, 2, 2, 0])
    assert abs(out2["d"][0] - d) < 1e-15
    assert np.all(np.isnan(GO.effect(X, group, div=[1, 1, 0, 1, 0, 1, 1])["d"]))
    # d of a pure mean shift is shift / sd
    rng = np.random.default_rng(1)
    a = rng.standard_normal(50).astype(np.float32)
    Y = np.concatenate([a, a + np.float32(0.5)])[:, None]
    shift = GO.effect(Y, [0] * 50 + [1] * 50)
    want = -np.mean(Y[50:, 0].astype(np.float64) - Y[:50, 0]) / np.sqrt(0.5 * (Y[:50, 0].astype(np.float64).var(ddof=1)
                                                                             + Y[50:, 0].astype(np.float64).var(ddof=1)))
    assert abs(shift["d"][0] - want) < 1e-12
    # replicates that redraw every member once reproduce d; a replicate with N < 2 is dropped; negative weights are 0
    boot = np.ones((4, 100), np.int16)
    boot[1, :50] = 0
    boot[1, 0] = 1
    boot[2, ::2] = -3
    rep = GO.effect(Y, [0] * 50 + [1] * 50, boot=boot)
    assert rep["record"] == (50, 50, 3)
    assert rep["ci_lo"][0] <= shift["d"][0] + 1e-12 <= rep["ci_hi"][0] + 2e-12
    same = GO.effect(Y, [0] * 50 + [1] * 50, boot=np.ones((5, 100), np.int16))
    assert abs(same["ci_lo"][0] - shift["d"][0]) < 1e-12 and abs(same["ci_hi"][0] - shift["d"][0]) < 1e-12
    assert same["se"][0] < 1e-12
    # the quantile is numpy's default: position (R' - 1) q, linear
    ds = np.sort(rng.standard_normal(7))
    assert abs(np.quantile(ds, 0.025) - (ds[0] + (ds[1] - ds[0]) * 0.15)) < 1e-15


@pytest.mark.parametrize("shape", GO.EFFECT_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_oracle_agrees_with_itself_under_another_summation_order(shape):
    X, div, group, boot = GO.effect_case(shape)
    fwd, bwd = GO.effect(X, group, div, boot), GO.effect(X, group, div, boot, reverse=True)
    assert fwd["record"] == bwd["record"] and fwd["record"][0] >= 2 and fwd["record"][1] >= 2
    for k in GO.FIELDS:
        np.testing.assert_allclose(fwd[k], bwd[k], rtol=GO.RTOL, atol=GO.ATOL, equal_nan=True, err_msg=k)
    if boot is not None:
        assert fwd["record"][2] == shape[2] and np.all(np.isfinite(fwd["se"]))


def test_bootstrap_weights():
    import torch

    from whisper_sae.analysis import bootstrap_weights
    labels = torch.tensor([0, 1, 2, 0, 1, 1, 0, 1, 3, 1, 0, 1])
    w = bootstrap_weights(labels, 50, seed=3)
    assert w.dtype == torch.int16 and tuple(w.shape) == (50, 12) and w.device.type == "cpu"
    a, b, other = labels == 0, labels == 1, labels > 1
    assert bool((w[:, a].sum(1) == 4).all()) and bool((w[:, b].sum(1) == 6).all()) and bool((w[:, other] == 0).all())
    assert bool((w >= 0).all()) and len({tuple(r.tolist()) for r in w}) > 25
    assert torch.equal(w, bootstrap_weights(labels, 50, seed=3)) and not torch.equal(w, bootstrap_weights(labels, 50, seed=4))
    bal = bootstrap_weights(labels, 50, seed=3, balanced=True)
    assert bool((bal[:, a].sum(1) == 4).all()) and bool((bal[:, b].sum(1) == 4).all()) and bool((bal[:, other] == 0).all())
    named = bootstrap_weights([2, 3, 3, 9, 2], 8, group_a=2, group_b=3)
    assert bool((named[:, [0, 4]].sum(1) == 2).all()) and bool((named[:, [1, 2]].sum(1) == 2).all()) and bool((named[:, 3] == 0).all())
    with pytest.raises(ValueError):
        bootstrap_weights(labels, 5, group_a=0, group_b=7)
    with pytest.raises(ValueError):
        bootstrap_weights(labels, 0)


# ---- argument errors: made-up (aligned, never dereferenced) pointers, every case fails its checks first -----------------
def _pool(N, k=32, hidden=64, n_rows=16, n_seg=4, f_lo=0, f_cols=64, ld=64, ws=4096, ws_bytes=32, vals=4096, cnt=None):
    return N.lib().wsae_pool_update(vals, 4096, k, hidden, 4096, n_rows, n_seg, f_lo, f_cols, 4096, cnt, ld, 4096, ws, ws_bytes,
                                    None)


def _effect(N, ld=64, n_seg=16, f_cols=64, boot=4096, n_boot=100, alpha=0.05, ws=4096, ws_bytes=None, X=4096, div=None):
    if ws_bytes is None:
        ws_bytes = max(N.lib().wsae_group_effect_workspace_bytes(16, 64, 100), 0)
    return N.lib().wsae_group_effect(X, ld, div, 4096, n_seg, f_cols, boot, n_boot, alpha, 4096, 4096, 4096, 4096, 4096, 4096,
                                     4096, 4096, ws, ws_bytes, None)


POOL_ERRORS = {"k0": dict(k=0), "k129": dict(k=129), "window_past_end": dict(f_lo=40, f_cols=25, ld=64),
               "window_negative": dict(f_lo=-1), "window_empty": dict(f_cols=0), "ld_lt_f_cols": dict(ld=63),
               "n_rows_2p31": dict(n_rows=2 ** 31), "n_rows_negative": dict(n_rows=-1), "n_seg0": dict(n_seg=0),
               "hidden0": dict(hidden=0), "null": dict(vals=None), "workspace_short": dict(ws_bytes=31),
               "workspace_null": dict(ws=None)}
EFFECT_ERRORS = {"R1": dict(n_boot=1), "R2049": dict(n_boot=2049), "R_without_boot": dict(boot=None, n_boot=5),
                 "boot_without_R": dict(n_boot=0), "alpha0": dict(alpha=0.0), "alpha1": dict(alpha=1.0),
                 "alpha_negative": dict(alpha=-0.1), "alpha_nan": dict(alpha=float("nan")), "ld_lt_f_cols": dict(ld=63),
                 "n_seg0": dict(n_seg=0), "f_cols0": dict(f_cols=0, ld=64), "null": dict(X=None),
                 "workspace_short": dict(ws_bytes=63), "workspace_null": dict(ws=None), "workspace_unaligned": dict(ws=4100)}


@pytest.mark.parametrize("kw", list(POOL_ERRORS.values()), ids=list(POOL_ERRORS))
def test_pool_argument_errors_do_not_need_a_gpu(kw):
    from whisper_sae import _native as N
    assert _pool(N, **kw) == -1
    assert "wsae_pool_update" in N.last_error()


@pytest.mark.parametrize("kw", list(EFFECT_ERRORS.values()), ids=list(EFFECT_ERRORS))
def test_effect_argument_errors_do_not_need_a_gpu(kw):
    from whisper_sae import _native as N
    assert _effect(N, **kw) == -1
    assert "wsae_group_effect" in N.last_error()


def test_workspace_queries():
    from whisper_sae import _native as N
    lib = N.lib()
    assert lib.wsae_pool_workspace_bytes(3_000_000, 32, 3072, 2048, 0, 3072) == 8 * 2048
    wp = lib.wsae_pool_workspace_bytes
    assert wp(16, 0, 64, 4, 0, 64) == -1 and wp(16, 129, 64, 4, 0, 64) == -1 and wp(2 ** 31, 32, 64, 4, 0, 64) == -1
    assert wp(16, 32, 64, 4, 60, 5) == -1 and wp(16, 32, 64, 0, 0, 64) == -1
    we = lib.wsae_group_effect_workspace_bytes
    point, boot = we(2048, 3072, 0), we(2048, 3072, 1000)
    assert 0 < point < 2048 * 64 and point < boot < 2048 * 3072  # no [S, H] fp64 copy and no [R, H] replicate matrix
    assert boot >= 2048 * 1000 * 2  # the transposed int16 weights
    assert we(16, 64, 1) == -1 and we(16, 64, 2049) == -1 and we(0, 64, 0) == -1 and we(16, 0, 0) == -1
    assert we(16, 64, 2) > 0 and we(16, 64, 2048) > 0


def test_header_signatures_and_exports_agree():
    from whisper_sae import _native as N
    import whisper_sae.analysis as A
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    lib = N.lib()
    for name in NAMES:
        proto = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert proto, name
        assert len(proto.group(1).split(",")) == len(N.SIGNATURES[name][1]), name
        assert getattr(lib, name) is not None
    defines = dict(re.findall(r"#define (WSAE_(?:POOL|BOOT)_[A-Z_]+) (\d+)", text))
    assert {k: int(v) for k, v in defines.items()} == {"WSAE_POOL_MAX_K": N.POOL_MAX_K, "WSAE_BOOT_MAX_R": N.BOOT_MAX_R}
    for name in ("SegmentPooler", "GroupEffects", "bootstrap_weights", "group_effect_sizes", "top_group_features",
                 "collect_pooled"):
        assert name in A.__all__ and hasattr(A, name)


def test_python_layer_argument_errors():
    import torch

    from whisper_sae import _native as N
    from whisper_sae.analysis import SegmentPooler, collect_pooled, group_effect_sizes, top_group_features
    from whisper_sae.analysis.group_stats import GroupEffects
    from whisper_sae.sae.model import ReLUSAE
    code = (torch.ones(2, 3, 2), torch.zeros(2, 3, 2, dtype=torch.int32))
    with pytest.raises(N.WsaeError):
        SegmentPooler(8, 4).update(code)  # CPU tensors
    with pytest.raises(N.WsaeError):
        group_effect_sizes(torch.zeros(6, 8), [0, 1, 0, 1, 0, 1])  # a CPU matrix
    with pytest.raises(ValueError):
        SegmentPooler(8, 4, f_window=(4, 5))
    with pytest.raises(ValueError):
        SegmentPooler(8, 0)
    with pytest.raises(TypeError):
        SegmentPooler(8, 4).update(torch.ones(2, 3, 2))
    with pytest.raises(TypeError):
        group_effect_sizes([[1.0, 2.0]], [0, 1])
    with pytest.raises(ValueError):
        group_effect_sizes(torch.zeros(6, 8), [0, 1] * 3, alpha=1.5)
    with pytest.raises(ValueError):
        group_effect_sizes(torch.zeros(6, 8), [0, 1] * 3, n_boot=1)
    with pytest.raises(ValueError):
        group_effect_sizes(torch.zeros(6, 8), [0, 1] * 3, n_boot=4096)
    with pytest.raises(ValueError):
        group_effect_sizes(torch.zeros(6, 8), [0, 1] * 3, use="max")
    with pytest.raises(TypeError):
        collect_pooled(ReLUSAE(16, 32), [torch.zeros(2, 4, 16)])
    # top_group_features is plain torch
    f64 = lambda *v: torch.tensor(v, dtype=torch.float64)  # noqa: E731
    eff = GroupEffects(d=f64(0.1, -2.0, 1.0, 3.0, float("nan")), g=f64(0.1, -1.9, 0.9, 2.9, float("nan")),
                       mean_a=f64(0, 0, 0, 0, 0), mean_b=f64(0, 0, 0, 0, 0), ci_lo=f64(-0.2, -2.5, -0.1, 2.0, float("nan")),
                       ci_hi=f64(0.4, -1.0, 1.8, 3.5, float("nan")), se=f64(0.1, 0.3, 0.5, 0.3, float("nan")), n_a=5, n_b=5,
                       n_boot=10)
    idx, g = top_group_features(eff, n=3)
    assert idx.tolist() == [3, 1] and g.tolist() == [2.9, -1.9]  # features 0 and 2 straddle zero, 4 is NaN
    idx, g = top_group_features(eff, n=3, require_ci_excludes_zero=False)
    assert idx.tolist() == [3, 1, 2]
