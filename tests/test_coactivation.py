"""Co-activation statistics without a GPU: the numpy oracle against a brute-force dense product and its own rules, every
argument error of ``wsae_coact_update`` / ``wsae_coact_top`` (raised before any HIP call), and the agreement of the
header, ``SIGNATURES`` and the package exports for the new names."""

from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest

import coactivation_oracle as CO

HEADER = Path(__file__).resolve().parents[1] / "include" / "wsae.h"
NAMES = ("wsae_coact_workspace_bytes", "wsae_coact_update", "wsae_coact_top_workspace_bytes", "wsae_coact_top")


def topk_like_code(rng, rows, k, hidden):
    """Distinct indices per row (as a TopK code has them), about a third of the values <= 0."""
    idx = np.stack([rng.permutation(hidden)[:k] for _ in range(rows)]).astype(np.int32)
    vals = rng.standard_normal((rows, k)).astype(np.float32) + 0.4
    vals[rng.random((rows, k)) < 0.1] = 0.0
    return vals, idx


def dense(code, hidden):
    vals, idx = code
    out = np.zeros((vals.shape[0], hidden), np.float32)
    ok = (idx >= 0) & (idx < hidden)
    r = np.broadcast_to(np.arange(vals.shape[0])[:, None], vals.shape)
    out[r[ok], idx[ok]] = vals[ok]
    return out


def test_oracle_equals_the_dense_product():
    rng = np.random.default_rng(0)
    ha, hb = 40, 56
    a, b = topk_like_code(rng, 300, 6, ha), topk_like_code(rng, 300, 9, hb)
    a[1][5, 2], b[1][7, 0], b[1][8, 1] = -1, hb, hb + 7  # out-of-range indices are ignored
    mask = (rng.random(300) < 0.7).astype(np.uint8)
    da, db = dense(a, ha) > 0, dense(b, hb) > 0
    for m in (None, mask):
        keep = np.ones(300, bool) if m is None else m != 0
        want = da[keep].astype(np.int64).T @ db[keep].astype(np.int64)
        counts, fa, fb, rows = CO.accumulate(a, ha, b, hb, row_mask=m)
        assert np.array_equal(counts, want) and rows == keep.sum()
        assert np.array_equal(fa, da[keep].sum(0)) and np.array_equal(fb, db[keep].sum(0))
        for lo, span in ((0, 8), (13, 17), (39, 1)):
            win, fa2, fb2, _ = CO.accumulate(a, ha, b, hb, row_mask=m, a_lo=lo, a_rows=span)
            assert np.array_equal(win, want[lo:lo + span]) and np.array_equal(fa2, fa) and np.array_equal(fb2, fb)
    # a code with itself: symmetric, the diagonal is the firing count; a small chunk does not change anything
    counts, fa, fb, _ = CO.accumulate(a, ha, a, ha, chunk=7)
    assert np.array_equal(counts, counts.T) and np.array_equal(np.diag(counts), fa) and np.array_equal(fa, fb)
    # a repeated index counts once per occurrence
    rep = (np.ones((1, 3), np.float32), np.array([[2, 2, 5]], np.int32))
    counts, fa, _, _ = CO.accumulate(rep, 8, rep, 8)
    assert counts[2, 2] == 4 and counts[2, 5] == 2 and counts[5, 5] == 1 and fa[2] == 2


def test_oracle_scores_match_scalar_formulas():
    rng = np.random.default_rng(1)
    ha, hb = 24, 30
    a, b = topk_like_code(rng, 200, 5, ha), topk_like_code(rng, 200, 7, hb)
    counts, fa, fb, rows = CO.accumulate(a, ha, b, hb)
    got = {m: CO.scores(counts, fa, fb, rows, m) for m in CO.METRICS}
    for i in range(ha):
        for j in range(hb):
            c, n, m, big = int(counts[i, j]), int(fa[i]), int(fb[j]), rows
            assert got["count"][i, j] == np.float32(c)
            assert got["cond"][i, j] == np.float32(c / n if n else 0.0)
            assert got["jaccard"][i, j] == np.float32(c / (n + m - c) if n + m - c else 0.0)
            pa, pb = n * (big - n), m * (big - m)
            want = float(big * c - n * m) / (np.sqrt(float(pa)) * np.sqrt(float(pb))) if pa and pb else 0.0
            assert got["phi"][i, j] == np.float32(want)
    # phi of two indicator vectors is their Pearson correlation
    da, db = (dense(a, ha) > 0).astype(np.float64), (dense(b, hb) > 0).astype(np.float64)
    i, j = int(np.argmax(fa)), int(np.argmax(fb))
    assert abs(got["phi"][i, j] - np.corrcoef(da[:, i], db[:, j])[0, 1]) < 1e-6


def test_oracle_tie_min_count_and_degenerate_rules():
    counts = np.array([[2, 4, 4, 0, 4], [0, 0, 0, 0, 0], [1, 1, 1, 1, 1]], np.int64)
    fa, fb = np.array([5, 0, 1]), np.array([4, 4, 4, 2, 4])
    v, i, c = CO.top(counts, fa, fb, 10, "count", 4, min_count=0)
    assert i.tolist() == [[1, 2, 4, 0], [0, 1, 2, 3], [0, 1, 2, 3]]  # ties: lowest index first
    assert v[0].tolist() == [4.0, 4.0, 4.0, 2.0] and c[0].tolist() == [4, 4, 4, 2]
    v, i, c = CO.top(counts, fa, fb, 10, "count", 4, min_count=1)
    assert i.tolist() == [[1, 2, 4, 0], [-1, -1, -1, -1], [0, 1, 2, 3]]
    assert np.all(v[1] == -np.inf) and c[1].tolist() == [0, 0, 0, 0]  # the tail is (-inf, -1, 0)
    v, i, c = CO.top(counts, fa, fb, 10, "count", 4, min_count=3)
    assert i.tolist() == [[1, 2, 4, -1], [-1] * 4, [-1] * 4]
    v, i, c = CO.top(counts, fa, fb, 10, "jaccard", 2, min_count=0, exclude_self=True)
    assert i[0].tolist() == [1, 2] and i[1].tolist() == [0, 2] and i[2].tolist() == [3, 0]
    v, i, c = CO.top(counts[1:], fa, fb, 10, "count", 5, min_count=0, exclude_self=True, a_lo=1)
    assert i.tolist() == [[0, 2, 3, 4, -1], [0, 1, 3, 4, -1]]  # the window's row r is feature a_lo + r
    # degenerate marginals: a feature that never fires (n = 0), one that always fires (n = N), an empty stream
    for metric in ("cond", "jaccard", "phi"):
        assert np.all(CO.scores(counts, fa, fb, 10, metric)[1] == 0.0)
    assert np.all(CO.scores(counts, np.array([10, 0, 1]), fb, 10, "phi")[0] == 0.0)
    assert np.all(CO.scores(counts, fa, np.array([10, 4, 0, 2, 4]), 10, "phi")[:, [0, 2]] == 0.0)
    assert np.all(CO.scores(np.zeros((2, 2)), np.zeros(2), np.zeros(2), 0, "phi") == 0.0)
    assert np.all(CO.scores(np.zeros((2, 2)), np.zeros(2), np.zeros(2), 0, "jaccard") == 0.0)
    # int64 numerators: N = 2^31 - 1 and counts of its order (N c alone is about 2^61)
    big, h = 2 ** 31 - 1, 2 ** 30
    s = CO.scores(np.array([[h - 5]]), np.array([h]), np.array([h + 3]), big, "phi")
    want = float(big * (h - 5) - h * (h + 3)) / (np.sqrt(float(h * (big - h))) * np.sqrt(float((h + 3) * (big - h - 3))))
    assert s[0, 0] == np.float32(want) and 0.5 < s[0, 0] <= 1.0


# ---- argument errors: made-up (aligned, never dereferenced) pointers, every case fails its checks first -----------------
def _update(N, k_a=32, hidden_a=64, k_b=32, hidden_b=64, n_rows=16, a_lo=0, a_rows=64, ldc=64, ws_bytes=0, vals_a=4096):
    return N.lib().wsae_coact_update(vals_a, 4096, k_a, hidden_a, 4096, 4096, k_b, hidden_b, n_rows, None, a_lo, a_rows, 4096,
                                     ldc, 4096, 4096, 4096, None, ws_bytes, None)


def _top(N, ldc=64, a_lo=0, a_rows=64, hidden_b=64, metric=0, min_count=1, top_n=4, ws_bytes=0, fire_b=4096):
    return N.lib().wsae_coact_top(4096, ldc, a_lo, a_rows, hidden_b, 4096, fire_b, 4096, metric, min_count, 0, top_n, 4096, 4096,
                                  None, None, ws_bytes, None)


UPDATE_ERRORS = {"k_a0": dict(k_a=0), "k_a129": dict(k_a=129), "k_b0": dict(k_b=0), "k_b129": dict(k_b=129),
                 "ldc_lt_hidden_b": dict(ldc=63), "window_past_end": dict(a_lo=40, a_rows=25),
                 "window_negative": dict(a_lo=-1), "window_empty": dict(a_rows=0), "n_rows_2p31": dict(n_rows=2 ** 31),
                 "n_rows_negative": dict(n_rows=-1), "hidden_b0": dict(hidden_b=0, ldc=64), "null": dict(vals_a=None)}
TOP_ERRORS = {"n0": dict(top_n=0), "n17": dict(top_n=17), "ldc_lt_hidden_b": dict(ldc=63), "window_negative": dict(a_lo=-1),
              "window_empty": dict(a_rows=0), "window_past_int32": dict(a_lo=2 ** 31 - 10, a_rows=11),
              "metric4": dict(metric=4), "metric_negative": dict(metric=-1), "min_count_negative": dict(min_count=-1),
              "phi_without_fire_b": dict(metric=3, fire_b=None), "hidden_b0": dict(hidden_b=0)}


@pytest.mark.parametrize("kw", list(UPDATE_ERRORS.values()), ids=list(UPDATE_ERRORS))
def test_update_argument_errors_do_not_need_a_gpu(kw):
    from whisper_sae import _native as N
    assert _update(N, **kw) == -1
    assert "wsae_coact_update" in N.last_error()


@pytest.mark.parametrize("kw", list(TOP_ERRORS.values()), ids=list(TOP_ERRORS))
def test_top_argument_errors_do_not_need_a_gpu(kw):
    from whisper_sae import _native as N
    assert _top(N, **kw) == -1
    assert "wsae_coact_top" in N.last_error()


def test_workspace_queries_and_one_byte_short():
    from whisper_sae import _native as N
    lib = N.lib()
    need_u = lib.wsae_coact_workspace_bytes(16384, 32, 40960, 32, 40960, 4096, 4096)
    need_t = lib.wsae_coact_top_workspace_bytes(4096, 4096, 40960, 16)
    assert need_u >= 0 and need_t >= 0  # (0: neither call needs scratch - and no [B, H] or score matrix either)
    assert need_u < 16384 * 40960 and need_t < 4096 * 40960
    assert _update(N, ws_bytes=lib.wsae_coact_workspace_bytes(16, 32, 64, 32, 64, 0, 64) - 1) == -1
    assert "wsae_coact_update" in N.last_error() and "workspace" in N.last_error()
    assert _top(N, ws_bytes=lib.wsae_coact_top_workspace_bytes(0, 64, 64, 4) - 1) == -1
    assert "wsae_coact_top" in N.last_error() and "workspace" in N.last_error()
    ws = lib.wsae_coact_workspace_bytes
    assert ws(16, 0, 64, 32, 64, 0, 64) == -1 and ws(16, 32, 64, 129, 64, 0, 64) == -1
    assert ws(2 ** 31, 32, 64, 32, 64, 0, 64) == -1 and ws(16, 32, 64, 32, 64, 60, 5) == -1
    wt = lib.wsae_coact_top_workspace_bytes
    assert wt(0, 64, 64, 0) == -1 and wt(0, 64, 64, 17) == -1 and wt(-1, 64, 64, 4) == -1 and wt(0, 64, 0, 4) == -1


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
    defines = dict(re.findall(r"#define (WSAE_COACT_[A-Z_]+) (\d+)", text))
    assert {k: int(v) for k, v in defines.items()} == {
        "WSAE_COACT_COUNT": N.COACT_COUNT, "WSAE_COACT_COND": N.COACT_COND, "WSAE_COACT_JACCARD": N.COACT_JACCARD,
        "WSAE_COACT_PHI": N.COACT_PHI, "WSAE_COACT_MAX_K": N.COACT_MAX_K}
    for name in ("CoactivationTracker", "CoactivationNeighbors", "collect_coactivation", "compare_activations"):
        assert name in A.__all__ and hasattr(A, name)


def test_python_layer_argument_errors():
    import torch

    from whisper_sae import _native as N
    from whisper_sae.analysis import CoactivationTracker, collect_coactivation
    from whisper_sae.sae.model import ReLUSAE
    code = (torch.ones(4, 2), torch.zeros(4, 2, dtype=torch.int32))
    with pytest.raises(N.WsaeError):
        CoactivationTracker(8).update(code)  # CPU tensors
    with pytest.raises(ValueError):
        CoactivationTracker(8, a_window=(4, 5))
    with pytest.raises(ValueError):
        CoactivationTracker(8).neighbors(metric="pearson")
    with pytest.raises(ValueError):
        CoactivationTracker(8).neighbors(n=17)
    with pytest.raises(ValueError):
        CoactivationTracker(8).neighbors(min_count=-1)
    with pytest.raises(TypeError):
        collect_coactivation(ReLUSAE(16, 32), dataloader=[torch.zeros(4, 16)])
