"""Dictionary comparison without a GPU: the float64 oracle checked against brute force, the argument errors of
``wsae_match_rows`` (raised before any HIP call) and the size of its workspace."""

from __future__ import annotations

import numpy as np
import pytest

import match_oracle as MO


def test_oracle_cosine_equals_brute_force():
    rng = np.random.default_rng(0)
    a = rng.standard_normal((7, 32)) * rng.uniform(1e-3, 1e3, (7, 1))
    b = rng.standard_normal((11, 32)) * rng.uniform(1e-3, 1e3, (11, 1))
    a[2] = 0.0
    sim = MO.similarity(a, b, "cosine")
    for i in range(7):
        for j in range(11):
            na, nb = np.linalg.norm(a[i]), np.linalg.norm(b[j])
            want = 0.0 if na == 0 else float(np.dot(a[i], b[j]) / (na * nb))
            assert abs(sim[i, j] - want) < 1e-12
    assert np.all(sim[2] == 0.0)
    vals, idx = MO.top_n(sim, 3)
    for i in range(7):
        order = sorted(range(11), key=lambda j: (-sim[i, j], j))[:3]
        assert idx[i].tolist() == order and vals[i].tolist() == [sim[i, j] for j in order]
    assert np.array_equal(MO.similarity(a, b, "dot"), a @ b.T)


def test_oracle_tie_rule_and_padding():
    sim = np.array([[1.0, 2.0, 2.0, 1.0, 2.0], [0.0, 0.0, 0.0, 0.0, 0.0], [3.0, 3.0, 3.0, 3.0, 3.0]])
    vals, idx = MO.top_n(sim, 4)
    assert idx.tolist() == [[1, 2, 4, 0], [0, 1, 2, 3], [0, 1, 2, 3]]  # ties: lowest index first
    assert vals[0].tolist() == [2.0, 2.0, 2.0, 1.0]
    vals, idx = MO.top_n(sim, 4, exclude_self=True)
    assert idx.tolist() == [[1, 2, 4, 3], [0, 2, 3, 4], [0, 1, 3, 4]]
    vals, idx = MO.top_n(sim[:, :2], 4)  # fewer candidates than top_n
    assert idx[0].tolist() == [1, 0, -1, -1] and vals[0].tolist() == [2.0, 1.0, -np.inf, -np.inf]
    vals, idx = MO.top_n(sim[:2, :2], 2, exclude_self=True)
    assert idx.tolist() == [[1, -1], [0, -1]] and vals[:, 1].tolist() == [-np.inf, -np.inf]


def test_oracle_bounds():
    u = 2.0 ** -24
    assert MO.bound(384) == (2 * 384 + 16) * u
    assert MO.bound(384, "bf16") == 2.0 ** -8 + 2.0 ** -18 + (2 * 384 + 16) * u
    assert MO.bound(64, "fp32", "dot") == 64 * u


def _call(N, rows_a=64, rows_b=64, dim=32, top_n=4, lda=None, ldb=None, ws_bytes=None, prec=None, metric=0):
    """wsae_match_rows with made-up (aligned, never dereferenced) pointers: every case here fails its checks first."""
    prec = N.PREC_FP32 if prec is None else prec
    if ws_bytes is None:
        ws_bytes = 1 << 40
    return N.lib().wsae_match_rows(4096, rows_a, dim if lda is None else lda, 8192, rows_b, dim if ldb is None else ldb, dim,
                                   metric, prec, top_n, 0, 4096, 4096, 4096, ws_bytes, None)


@pytest.mark.parametrize("kw", [dict(dim=48), dict(top_n=0), dict(top_n=17), dict(dim=64, lda=32), dict(dim=2080),
                                dict(lda=34), dict(rows_b=0), dict(metric=2), dict(prec=7)],
                         ids=["dim48", "n0", "n17", "lda_lt_dim", "dim2080", "lda_unaligned", "rows_b0", "metric", "precision"])
def test_argument_errors_do_not_need_a_gpu(kw):
    from whisper_sae import _native as N
    assert _call(N, **kw) == -1
    assert "wsae_match_rows" in N.last_error()


def test_workspace_one_byte_short_is_an_error():
    from whisper_sae import _native as N
    need = N.lib().wsae_match_workspace_bytes(64, 64, 32, 4, N.PREC_FP32)
    assert need > 0
    assert _call(N, ws_bytes=need - 1) == -1
    assert "wsae_match_rows" in N.last_error() and "workspace" in N.last_error()


def test_workspace_size():
    from whisper_sae import _native as N
    ws = N.lib().wsae_match_workspace_bytes
    big = ws(40960, 40960, 1280, 16, N.PREC_BF16)
    assert 0 < big < 40960 * 40960 * 4 // 4  # the similarity matrix is never materialised
    for prec in (N.PREC_BF16, N.PREC_FP32):
        for shape in ((40960, 40960, 1280), (3072, 3072, 384), (1, 1, 32), (130, 4099, 64)):
            sizes = [ws(*shape, n, prec) for n in range(1, N.MATCH_MAX_N + 1)]
            assert all(s > 0 for s in sizes) and sizes == sorted(sizes)  # monotone in top_n
            # at least the two staged operands
            assert sizes[0] >= (shape[0] + shape[1]) * shape[2] * (2 if prec == N.PREC_BF16 else 4)
    assert ws(64, 64, 48, 4, N.PREC_FP32) == -1 and ws(64, 64, 32, 17, N.PREC_FP32) == -1 and ws(0, 64, 32, 1, 0) == -1


def test_python_layer_argument_errors():
    import torch

    from whisper_sae import _native as N
    from whisper_sae.analysis import compare_dictionaries, duplicate_features, nearest_features  # noqa: F401
    with pytest.raises(N.WsaeError):
        nearest_features(torch.zeros(8, 32), torch.zeros(8, 32))
    with pytest.raises(ValueError):
        nearest_features(torch.zeros(8, 32), metric="euclid")
    with pytest.raises(ValueError):
        nearest_features(torch.zeros(8, 32), n=17)
    with pytest.raises(ValueError):
        nearest_features(torch.zeros(8, 32), which="bias")
