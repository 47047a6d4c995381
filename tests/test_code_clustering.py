"""Code clustering on the CPU: the two definitions of tests/cluster_oracle.py on hand-worked
rows, the score formulas on hand-made tables, ``unit_sequences``, the conditions that keep the inputs of the GPU tests from
being degenerate (checked on the oracle, so that the reference alone meets them), and the host checks, which need no GPU."""

from __future__ import annotations

import math
import re
from pathlib import Path

import numpy as np
import pytest

import cluster_oracle as CO

HEADER = Path(__file__).resolve().parents[1] / "include" / "wsae.h"
NAMES = ("wsae_cluster_assign_workspace_bytes", "wsae_cluster_assign", "wsae_cluster_accumulate_workspace_bytes",
         "wsae_cluster_accumulate")
NAN = float("nan")
f32 = np.float32


def code_of(rows):
    """``rows``: per row a list of (value, index)."""
    k = max(len(r) for r in rows)
    vals, idx = np.zeros((len(rows), k), np.float32), np.full((len(rows), k), -1, np.int32)
    for r, row in enumerate(rows):
        for j, (v, f) in enumerate(row):
            vals[r, j], idx[r, j] = v, f
    return vals, idx


# ---- 1: hand-worked rows ------------------------------------------------------------------------------------------------------
def test_assign_by_hand():
    hidden = 8
    col_of = np.array([0, 1, 2, -1, 3, 4, 5, 6], np.int32)  # feature 3 has no column
    # Ct [7 columns, 3 clusters]: clusters 0 and 2 are equal on columns 0 and 1
    Ct = np.array([[1, 0, 1], [0.5, 1, 0.5], [0, 1, 3], [0, 0, 0], [4, 0, 0], [0, 0, 0], [0, 0, 0]], np.float32)
    code = code_of([
        [(2.0, 0), (3.0, 0), (1.0, 1)],        # a duplicate index: the first entry counts
        [(-1.0, 0), (0.0, 1), (NAN, 2)],       # v <= 0 and NaN: an empty row
        [(1.0, -1), (1.0, 8), (1.0, 3)],       # an index of -1, of hidden and a feature without a column: empty
        [(1.0, 0), (2.0, 1), (1.0, 2)],        # a padding row (seg below)
        [(2.0, 0), (2.0, 1)],                  # an exact tie of clusters 0 and 2: the lowest wins
        [(1.0, 2), (5000.0, 4)],               # cluster 2; the value above 4096 takes part in the norm
    ])
    seg = np.array([0, 0, 0, -1, 1, 1], np.int32)
    labels = np.array([1, 0, 0, 1, 2, 0], np.int32)
    a, best, second, inv, st = CO.assign(code, hidden, Ct, 3, seg, col_of, None, False, labels, 2)
    assert a.tolist() == [0, -1, -1, -1, 0, 2]
    # row 0: scores (2 + 0.5, 2, 2 + 0.5) -> a tie of 0 and 2 as well
    assert best[0] == 2.5 and second[0] == 2.5 and inv[0] == f32(1 / math.sqrt(5.0))
    assert best[4] == 3.0 and second[4] == 3.0 and inv[4] == f32(1 / math.sqrt(8.0))
    assert best[5] == 3.0 and second[5] == 1.0 and inv[5] == f32(1 / math.sqrt(1.0 + 25e6))
    for r in (1, 2, 3):
        assert best[r] == 0 and second[r] == 0 and inv[r] == 0
    assert st["count"] == [2, 0, 1] and st["totals"] == [3, 2, 2]  # (row 4 carries label 2, outside [0, 2))
    assert st["best_q"] == [int(5.5 * 2 ** 20), 0, 3 * 2 ** 20]
    assert st["contingency"] == [[0, 1], [0, 0], [1, 0]]
    # normalize: the quality is best * inv_norm, one fp32 product
    _, _, _, _, st_n = CO.assign(code, hidden, Ct, 3, seg, col_of, None, True)
    q = lambda b, i: int(np.rint(f32(b) * f32(i) * f32(2 ** 20)))
    assert st_n["best_q"] == [q(2.5, inv[0]) + q(3.0, inv[4]), 0, q(3.0, inv[5])]
    # a bias breaks the tie; one cluster: second is -inf; the clip of the quality at +-4096
    a_b, best_b, second_b, _, _ = CO.assign(code, hidden, Ct, 3, seg, col_of, np.array([0, 0, 0.25], np.float32))
    assert a_b.tolist() == [2, -1, -1, -1, 2, 2] and best_b[0] == 2.75 and second_b[0] == 2.5
    a1, best1, second1, _, st1 = CO.assign(code, hidden, Ct[:, :1] * f32(5000), 1, seg, col_of)
    assert a1.tolist() == [0, -1, -1, -1, 0, 0] and np.isneginf(second1[[0, 4, 5]]).all() and second1[1] == 0
    assert best1[0] == 12500 and st1["best_q"] == [2 * 4096 * 2 ** 20 + 0]  # rows 0 and 4 clip, row 5 scores 0


def test_accumulate_by_hand():
    hidden = 6
    code = code_of([[(2.0, 0), (1.5, 2)], [(5000.0, 0), (0.5, 5)], [(1.0, 0), (1.0, 2)], [(3.0, 2), (1.0, 1)]])
    seg = np.array([0, 0, -1, 1], np.int32)
    col_ptr, t_row, t_val = CO.plan(code, hidden, seg)
    assert col_ptr.tolist() == [0, 2, 3, 5, 5, 5, 6] and t_row.tolist() == [0, 1, 3, 0, 3, 1] and t_val[1] == 5000
    one = 2 ** 20
    S = CO.accumulate(col_ptr, t_row, t_val, 6, [1, 0, 0, 1], 2)
    assert S[0] == [4096 * one, 2 * one]          # the value above 4096 is clipped
    assert S[1] == [0, one] and S[2] == [0, int(4.5 * one)] and S[5] == [one // 2, 0] and S[3] == S[4] == [0, 0]
    # assign -1 and out of range add nothing; cap cuts the lists; a stored state is added to
    S = CO.accumulate(col_ptr, t_row, t_val, 4, [1, -1, 0, 2], 2, S_q=[[7, 7] for _ in range(6)])
    assert S[0] == [7, 7 + 2 * one] and S[2] == [7, 7 + int(1.5 * one)] and S[1] == S[5] == [7, 7]
    # row weights: negative, NaN and zero weights add nothing; the product is one fp32 product
    w = np.array([-1.0, NAN, 1.0, 0.3], np.float32)
    S = CO.accumulate(col_ptr, t_row, t_val, 6, [0, 0, 0, 0], 1, row_weight=w)
    assert S[0] == [0] and S[5] == [0] and S[2] == [int(np.rint(f32(3.0) * f32(0.3) * f32(one)))]
    w[0] = 0.0
    assert CO.accumulate(col_ptr, t_row, t_val, 6, [0, 0, 0, 0], 1, row_weight=w)[0] == [0]
    # rows outside [0, n_rows) add nothing
    assert CO.accumulate(col_ptr, t_row, t_val, 6, [0, 0, 0, 0], 1, n_rows=1)[2] == [int(1.5 * one)]


# ---- 2: the score formulas ----------------------------------------------------------------------------------------------------
def both_scores(table):
    import torch

    from whisper_sae.analysis import cluster_scores
    want, got = CO.scores(table), cluster_scores(torch.tensor(table))
    for name in ("cluster_purity", "class_purity", "mutual_information", "pnmi", "nmi", "v_measure", "ari"):
        assert getattr(got, name) == pytest.approx(want[name], abs=1e-12), name
    assert got.many_to_one == got.cluster_purity and got.n_frames == want["n"]
    assert got.best_class.tolist() == want["best_class"].tolist()
    return got


def test_scores_of_hand_made_tables():
    perfect = both_scores([[5, 0, 0], [0, 0, 7], [0, 3, 0]])
    assert perfect.cluster_purity == 1 and perfect.class_purity == 1 and perfect.ari == pytest.approx(1, abs=1e-12)
    assert perfect.pnmi == pytest.approx(1, abs=1e-12) and perfect.nmi == pytest.approx(1, abs=1e-12)
    assert perfect.v_measure == pytest.approx(1, abs=1e-12) and perfect.best_class.tolist() == [0, 2, 1]
    product = both_scores([[2 * 3, 2 * 5], [4 * 3, 4 * 5]])  # independent: the outer product of (2, 4) and (3, 5)
    assert product.mutual_information == pytest.approx(0, abs=1e-12) and product.pnmi == pytest.approx(0, abs=1e-12)
    # ARI = (sum_ij C2 - E) / (M - E): sum_ij = 15 + 45 + 66 + 190 = 316, rows C2(16) + C2(32) = 616, columns C2(18) +
    # C2(30) = 588, E = 616 * 588 / C2(48) = 321.1..: slightly below 0, as for any exact product table
    assert product.ari == pytest.approx((316 - 616 * 588 / 1128) / (0.5 * (616 + 588) - 616 * 588 / 1128), abs=1e-12)
    # (the index is 0 in expectation under fixed margins; the exact product table lies O(1 / n) below it: -0.018 at n = 48,
    # and 0 to five places at n = 48000)
    large = both_scores([[6000, 10000], [12000, 20000]])
    assert large.mutual_information == pytest.approx(0, abs=1e-12) and abs(large.ari) < 2e-5 and abs(product.ari) < 0.02
    # one table by hand: [[3, 1], [0, 4]], n = 8
    hand = both_scores([[3, 1], [0, 4]])
    assert hand.cluster_purity == 7 / 8 and hand.class_purity == 7 / 8 and hand.best_class.tolist() == [0, 1]
    ln = math.log
    mi = 3 / 8 * ln(3 * 8 / (4 * 3)) + 1 / 8 * ln(1 * 8 / (4 * 5)) + 4 / 8 * ln(4 * 8 / (4 * 5))
    h_c = -(3 / 8 * ln(3 / 8) + 5 / 8 * ln(5 / 8))
    h_k = ln(2)
    assert hand.mutual_information == pytest.approx(mi, abs=1e-12) and hand.pnmi == pytest.approx(mi / h_c, abs=1e-12)
    assert hand.nmi == pytest.approx(2 * mi / (h_c + h_k), abs=1e-12)
    assert hand.v_measure == pytest.approx(2 * (mi / h_c) * (mi / h_k) / (mi / h_c + mi / h_k), abs=1e-12)
    # pairs: sum_ij = 3 + 0 + 0 + 6 = 9, rows 6 + 6 = 12, columns 3 + 10 = 13, all pairs 28
    assert hand.ari == pytest.approx((9 - 12 * 13 / 28) / (12.5 - 12 * 13 / 28), abs=1e-12)
    from whisper_sae.analysis import cluster_scores
    import torch
    for bad in (torch.zeros(2, 2, dtype=torch.int64), torch.ones(2, 2), torch.ones(4, dtype=torch.int64),
                torch.tensor([[1, -1], [2, 2]])):
        with pytest.raises(ValueError):
            cluster_scores(bad)


def test_unit_sequences():
    import torch

    from whisper_sae.analysis import unit_sequences
    a = np.array([3, 3, 3, -1, 3, 5, 5, 5, 2, 2, -1, -1, 2], np.int32)
    seg = np.array([0, 0, 0, 0, 0, 0, 1, 1, 1, -1, 1, 1, 1], np.int32)
    want = CO.unit_sequences(a, seg)
    assert want[0].tolist() == [3, 3, 5, 5, 2, 2] and want[1].tolist() == [3, 1, 1, 2, 1, 1] and want[2].tolist() == [0, 0, 0, 1, 1, 1]
    got = unit_sequences(torch.from_numpy(a), torch.from_numpy(seg))
    for g, w in zip(got, want):
        assert g.dtype == torch.int64 and g.tolist() == w.tolist()
    two = torch.tensor([[1, 1, 2], [2, 2, -1]])
    u, n, s = unit_sequences(two)
    assert u.tolist() == [1, 2, 2] and n.tolist() == [2, 1, 2] and s.tolist() == [0, 0, 1]
    u, n, s = unit_sequences(torch.full((4,), -1), torch.zeros(4, dtype=torch.int64))
    assert u.numel() == 0 and n.numel() == 0 and s.numel() == 0
    for bad in (dict(assign=two.float()), dict(assign=two, segments=two), dict(assign=two[0]),
                dict(assign=two[0], segments=torch.zeros(2, dtype=torch.int64))):
        with pytest.raises(ValueError):
            unit_sequences(**bad)


# ---- 3: the conditions on the inputs of the GPU tests -------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CO.CASES))
def test_conditions_on_the_cases(name):
    c = CO.case(name)
    rows, k, hidden, n_cols, C, n_classes, n_seg, ties, all_rows = CO.CASES[name]
    vals, idx = c["code"]
    assert vals.shape == (rows, k) and c["Ct"].shape == (c["n_cols"], C + CO.LDC_EXTRA) and 1 <= k <= CO.MAX_K
    for combo in range(len(CO.COMBOS)):
        a, best, second, inv, st = CO.case_assign(name, combo)
        ok = a >= 0
        assert st["totals"][0] == ok.sum() and (best[~ok] == 0).all() and (inv[~ok] == 0).all()
        assert np.isfinite(best[ok]).all() and (inv[ok] > 0).all()
        if name != "one" and not ties:
            assert (best[ok] > second[ok]).mean() >= 0.5
        if ties:
            tied = best[ok] == second[ok]
            assert tied.sum() >= 20 and set(a[ok][tied]) == {1}  # the lowest of the tied clusters 1, 3 and 5
        if rows > 1:
            with_seg = CO.COMBOS[combo][3]
            assert st["totals"][1] >= 5 and (not with_seg or (c["seg"] < 0).sum() >= 5)  # empty rows, padding
            assert ok.sum() >= rows // 2
            if CO.COMBOS[combo][2]:
                assert 0 < st["totals"][2] < st["totals"][0] and np.asarray(st["contingency"]).sum() == st["totals"][2]
    if all_rows:
        col_ptr, t_row, _ = CO.case_plan(name, False)
        silent = np.array([not CO.row_entries(vals[r], idx[r], hidden) for r in range(rows)])
        assert col_ptr[1] - col_ptr[0] == (~silent).sum() >= 0.9 * rows  # feature 0 fires on every row that is not silent
    if rows > 1:
        assert (vals > 4096).any() and np.isnan(vals).any() and (idx == -1).any() and (idx == hidden).any() and (vals <= 0).any()
    if n_cols is not None:
        assert (c["col_of"] >= 0).sum() == n_cols and hidden == 40960


def test_conditions_on_the_planted_case():
    c = CO.planted_case()
    vals, idx = c["code"]
    assert vals.shape == (1181, 16) and c["hidden"] == 512 and c["seg"].max() == 11 and (c["seg"] < 0).sum() == 24
    assert set(c["proto"][c["seg"] >= 0]) == set(range(8))
    Ct, a, iterations, count = CO.planted_fit()
    assert iterations <= 7 and min(count) > 0 and len(count) == 8
    assert (a[c["seg"] < 0] == -1).all() and (a[c["seg"] >= 0] >= 0).all()
    sc = CO.scores(CO.table_of(a, c["proto"], 8, 8))
    assert sc["ari"] == 1.0 and sc["cluster_purity"] == 1.0 and sc["n"] == 1157
    assert np.allclose(np.sqrt((Ct.astype(np.float64) ** 2).sum(0)), 1.0, atol=1e-6)  # unit centroids


# ---- 4: host argument errors: made-up (aligned, never dereferenced) pointers ---------------------------------------------------
def _assign(N, k=32, hidden=64, n_rows=16, n_cols=64, ldc=8, n_clusters=8, normalize=0, n_classes=4, vals=4096, idx=4096,
            seg=4096, col_of=None, Ct=4096, bias=None, labels=4096, assign=4096, best=4096, second=4096, inv_norm=4096,
            count=4096, best_q=4096, contingency=4096, totals=4096, ws=None, ws_bytes=0):
    return N.lib().wsae_cluster_assign(vals, idx, k, hidden, seg, n_rows, col_of, n_cols, Ct, ldc, bias, n_clusters, normalize, labels,
                                       n_classes, assign, best, second, inv_norm, count, best_q, contingency, totals, ws, ws_bytes,
                                       None)


ASSIGN_ERRORS = {"k0": dict(k=0), "k129": dict(k=129), "hidden0": dict(hidden=0), "n_rows_2p31": dict(n_rows=2 ** 31),
                 "n_rows_negative": dict(n_rows=-1), "null_vals": dict(vals=None), "null_idx": dict(idx=None),
                 "null_Ct": dict(Ct=None), "n_cols0": dict(n_cols=0, col_of=4096), "n_cols_above_hidden": dict(n_cols=65, col_of=4096),
                 "subset_without_col_of": dict(n_cols=32), "clusters0": dict(n_clusters=0), "clusters1025": dict(n_clusters=1025, ldc=2048),
                 "ldc_small": dict(ldc=7), "normalize_with_bias": dict(normalize=1, bias=4096), "classes0": dict(n_classes=0),
                 "classes1025": dict(n_classes=1025), "contingency_without_labels": dict(labels=None),
                 "workspace_negative": dict(ws_bytes=-1)}


@pytest.mark.parametrize("kw", list(ASSIGN_ERRORS.values()), ids=list(ASSIGN_ERRORS))
def test_assign_argument_errors_do_not_need_a_gpu(kw):
    from whisper_sae import _native as N
    assert _assign(N, **kw) == -1
    assert "wsae_cluster_assign" in N.last_error()


def _acc(N, cap=100, n_cols=64, n_rows=16, n_clusters=8, lds=8, col_ptr=4096, t_row=4096, t_val=4096, assign=4096, row_weight=None,
         S_q=4096, ws=None, ws_bytes=0):
    return N.lib().wsae_cluster_accumulate(col_ptr, t_row, t_val, cap, n_cols, assign, row_weight, n_rows, n_clusters, S_q, lds, ws,
                                           ws_bytes, None)


ACC_ERRORS = {"null_col_ptr": dict(col_ptr=None), "null_assign": dict(assign=None), "null_S_q": dict(S_q=None),
              "n_rows_2p31": dict(n_rows=2 ** 31), "n_rows_negative": dict(n_rows=-1), "n_cols0": dict(n_cols=0),
              "clusters0": dict(n_clusters=0), "clusters1025": dict(n_clusters=1025, lds=2048), "cap_negative": dict(cap=-1),
              "lists_missing": dict(t_row=None), "values_missing": dict(t_val=None), "lds_small": dict(lds=7),
              "workspace_negative": dict(ws_bytes=-1)}


@pytest.mark.parametrize("kw", list(ACC_ERRORS.values()), ids=list(ACC_ERRORS))
def test_accumulate_argument_errors_do_not_need_a_gpu(kw):
    from whisper_sae import _native as N
    assert _acc(N, **kw) == -1
    assert "wsae_cluster_accumulate" in N.last_error()


def test_messages_empty_calls_and_the_workspace_queries():
    from whisper_sae import _native as N
    assert _assign(N, n_clusters=1025, ldc=2048) == -1 and "need 1 <= n_clusters <= 1024 (got 1025)" in N.last_error()
    assert _assign(N, normalize=1, bias=4096) == -1 and "normalize needs bias == NULL" in N.last_error()
    assert _assign(N, k=129) == -1 and "need 1 <= k <= 128 (got 129)" in N.last_error()
    assert _acc(N, lds=7) == -1 and "lds 7 is smaller than the 8 clusters" in N.last_error()
    assert _assign(N, n_rows=0) == 0 and _assign(N, n_rows=0, seg=None, labels=None, contingency=None) == 0
    assert _assign(N, n_rows=0, assign=None, best=None, second=None, inv_norm=None, count=None, best_q=None, totals=None) == 0
    assert _assign(N, n_rows=0, k=128, n_clusters=1024, ldc=1024, n_classes=1024) == 0
    assert _acc(N, n_rows=0) == 0 and _acc(N, n_rows=0, cap=0, t_row=None, t_val=None) == 0
    q = N.lib().wsae_cluster_assign_workspace_bytes
    assert q(0, 1, 1, 1, 1) == 0 and q(2048 * 1500, 32, 40960, 4096, 500) == 0 and q(2 ** 31 - 1, 128, 64, 64, 1024) == 0
    for bad in ((16, 0, 64, 64, 8), (16, 129, 64, 64, 8), (-1, 32, 64, 64, 8), (2 ** 31, 32, 64, 64, 8), (16, 32, 0, 1, 8),
                (16, 32, 64, 0, 8), (16, 32, 64, 65, 8), (16, 32, 64, 64, 0), (16, 32, 64, 64, 1025)):
        assert q(*bad) == -1, bad
    b = N.lib().wsae_cluster_accumulate_workspace_bytes
    assert b(0, 1, 1, 0) == 0 and b(2048 * 1500, 4096, 500, 10 ** 8) == 0
    for bad in ((-1, 64, 8, 10), (2 ** 31, 64, 8, 10), (16, 0, 8, 10), (16, 64, 0, 10), (16, 64, 1025, 10), (16, 64, 8, -1)):
        assert b(*bad) == -1, bad


# ---- 5: header, SIGNATURES and exports ----------------------------------------------------------------------------------------
def test_header_signatures_and_exports_agree():
    import whisper_sae.analysis as A
    from whisper_sae import _native as N
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    lib = N.lib()
    for name in NAMES:
        proto = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert proto, name
        assert len(proto.group(1).split(",")) == len(N.SIGNATURES[name][1]), name
        assert getattr(lib, name) is not None
    defines = {k: int(v) for k, v in re.findall(r"#define (WSAE_CLUSTER_[A-Z_]+) (\d+)", text)}
    assert defines == {"WSAE_CLUSTER_MAX_K": N.CLUSTER_MAX_K, "WSAE_CLUSTER_MAX": N.CLUSTER_MAX}
    assert (N.CLUSTER_MAX_K, N.CLUSTER_MAX) == (128, 1024) == (CO.MAX_K, CO.MAX_CLUSTERS)
    for name in ("CodeKMeans", "ClusterScores", "IterationStats", "cluster_scores", "unit_sequences", "collect_code_clusters"):
        assert name in A.__all__ and hasattr(A, name)
    src = (HEADER.parents[1] / "whisper-sae_amd" / "csrc" / "wsae_cluster.hip").read_text()
    assert "#pragma clang fp contract(off)" in src and "atomicAdd(float" not in src


# ---- 6: the Python layer ------------------------------------------------------------------------------------------------------
def test_python_layer_argument_errors():
    import torch

    from whisper_sae import _native as N
    from whisper_sae.analysis import CodeKMeans, collect_code_clusters
    from whisper_sae.sae.model import ReLUSAE
    for kw in (dict(n_clusters=0), dict(n_clusters=1025), dict(hidden=0), dict(metric="manhattan"), dict(n_classes=-1),
               dict(n_classes=1025), dict(features=torch.tensor([1, 1])), dict(features=torch.tensor([64])),
               dict(features=torch.ones(2, 2, dtype=torch.int64)), dict(features=torch.tensor([0.5]))):
        with pytest.raises(ValueError):
            CodeKMeans(**{"n_clusters": 4, "hidden": 64, **kw})
    km = CodeKMeans(4, 64, features=torch.tensor([5, 3, 9]), metric="euclidean", seed=7)
    assert (km.n_clusters, km.hidden, km.n_cols, km.metric, km.seed) == (4, 64, 3, "euclidean", 7)
    code = (torch.ones(2, 3, 2), torch.zeros(2, 3, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match="init_centroids first"):
        km.accumulate(code)
    with pytest.raises(ValueError, match="init_centroids first"):
        km.predict(code)
    with pytest.raises(N.WsaeError):
        km.init_centroids(code)  # CPU tensors
    with pytest.raises(TypeError):
        km.init_centroids(torch.ones(2, 3, 2))
    with pytest.raises(ValueError):
        km.init_centroids(code, init="kmeans++")
    with pytest.raises(ValueError):
        km.init_centroids(None)
    with pytest.raises(N.WsaeError):
        CodeKMeans(4, 64, device="cpu").centroids
    with pytest.raises(TypeError):
        km.merge_sums(object())
    with pytest.raises(ValueError):
        km.merge_sums(CodeKMeans(5, 64, features=torch.tensor([5, 3, 9]), metric="euclidean"))
    with pytest.raises(TypeError):
        collect_code_clusters(ReLUSAE(16, 32), [torch.zeros(2, 4, 16)], 4)
    with pytest.raises(TypeError, match="re-iterable"):
        collect_code_clusters(ReLUSAE(16, 32), iter([torch.zeros(2, 4, 16)]), 4)
