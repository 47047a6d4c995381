"""ABX discrimination on the CPU: the oracle of tests/abx_oracle.py against brute force and hand cases, the plain-torch
parts of ``whisper_sae.analysis.discrimination`` (``items_from_labels``, ``AbxScores``) against the oracle, and the
conditions that keep the GPU cases of tests/test_gpu_abx.py from being degenerate."""

from __future__ import annotations

import math

import numpy as np
import pytest
import torch

import abx_oracle as AO
from dynamics_oracle import canonical
from whisper_sae.analysis import AbxScores, items_from_labels


# ---- the dynamic program against brute force ------------------------------------------------------------------------------------
def brute_force(e):
    """``(minimal total, path length of the stated tie-break)`` by enumeration: the total of a path is the chain of
    float64 additions along it; the best total of every prefix cell comes from the enumeration too, and the path is read
    backwards from the end cell, the predecessor with the smallest best total winning, ties to the earlier of diagonal,
    above, left."""
    n, m = e.shape
    best = {}
    for path in AO.all_monotone_paths(n, m):
        total = None
        for (i, j) in path:
            total = float(e[i, j]) if total is None else float(e[i, j]) + total
            if (i, j) not in best or total < best[(i, j)]:
                best[(i, j)] = total
    cell, length = (n - 1, m - 1), 1
    while cell != (0, 0):
        cands = [(cell[0] + di, cell[1] + dj) for di, dj in AO.PREFERENCE if cell[0] + di >= 0 and cell[1] + dj >= 0]
        pick = cands[0]
        for c in cands[1:]:
            if best[c] < best[pick]:
                pick = c
        cell, length = pick, length + 1
    return best[(n - 1, m - 1)], length


@pytest.mark.parametrize("tied", [False, True], ids=["random", "tied"])
def test_the_dynamic_program_equals_brute_force(tied):
    rng = np.random.default_rng(25 + tied)
    for n in range(1, 5):
        for m in range(1, 5):
            for _ in range(12):
                e = (rng.integers(0, 2, (n, m)) if tied else rng.random((n, m))).astype(np.float32)
                assert AO.dtw(e) == brute_force(e), (n, m, e)


def test_hand_cases_of_the_dynamic_program():
    f = lambda rows: np.asarray(rows, np.float32)  # noqa: E731
    assert AO.dtw(f([[0.5]])) == (0.5, 1)
    assert AO.dtw(f([[0, 1], [1, 0]])) == (0.0, 2)
    assert AO.dtw(f([[1, 2, 3]])) == (6.0, 3) and AO.dtw(f([[1], [2], [3]])) == (6.0, 3)
    assert AO.dtw(f([[0, 0], [0, 0]])) == (0.0, 2)                       # all tied: the diagonal
    assert AO.dtw(f([[0, 0], [0, 0]]), AO.PREFERENCE[::-1]) == (0.0, 3)  # the reversed preference walks around
    assert AO.dtw(f([[0, 0, 9], [9, 0, 0]])) == (0.0, 3)
    assert AO.dtw(f([[0, 9], [0, 9], [0, 0]])) == (0.0, 3)               # down the first column, the last step diagonal
    assert AO.dtw(f([[1, 0, 0], [0, 1, 0], [0, 0, 1]]))[0] == 2.0  # (both corners are on every path)
    assert AO.distances(np.array([[3.0, np.nan]]), np.array([[4, 0]]), True)[0].tolist()[0][0] == 0.75
    d, s = AO.distances(np.array([[3.0, np.nan]]), np.array([[4, 0]]), False)
    assert d[0, 0] == 3.0 and np.isnan(d[0, 1]) and s.tolist() == [[4, 0]]


def test_frame_costs_equal_the_literal_chain():
    c = AO.distance_case(1)
    canon = canonical(c["code"], c["hidden"], c["seg"], c["weight"])
    rows_a, rows_b = list(range(0, 60, 3)), list(range(100, 160, 2))
    for metric in (AO.COSINE, AO.JACCARD):
        got = AO.frame_costs(canon, rows_a, rows_b, metric, c["hidden"])
        for i, r in enumerate(rows_a):
            for j, q in enumerate(rows_b):
                want = AO.pair_cost(canon, r, q, metric)
                assert got[i, j].view(np.uint32) == want.view(np.uint32), (metric, r, q)
                s, matched = AO.pair_terms_b(canon, r, q)
                c64 = AO.similarity_f64(metric, s, matched, canon[r], canon[q])
                assert np.float32(c64) == AO.similarity_value(metric, s, matched, canon[r], canon[q])
    assert (got > 0).any() and (got < 1).any()
    # a hand case: rows (f: u) {1: 2, 5: 1} and {5: 3, 1: 1, 7: 2}, the chain in the order of the B frame
    code = (np.array([[2, 1, 0], [3, 1, 2]], np.float32), np.array([[1, 5, 0], [5, 1, 7]], np.int32))
    canon = canonical(code, 8)
    assert AO.pair_terms_b(canon, 0, 1) == (1.0 * 3.0 + 2.0 * 1.0, 2)
    assert AO.pair_cost(canon, 0, 1, AO.JACCARD) == np.float32(1.0 - 2 / 3)
    assert AO.pair_cost(canon, 0, 1, AO.COSINE) == np.float32(1.0 - 5.0 / math.sqrt(5.0 * 14.0))
    assert AO.pair_cost(canon, 0, 0, AO.COSINE) == 0.0


def test_invalid_items_and_the_shape_of_the_cases():
    for n in range(1, len(AO.DIST_SHAPES)):
        c = AO.distance_case(n)
        rows = c["code"][0].shape[0]
        lengths = np.asarray(c["b"][1])
        for wanted in (1, 2, 63, 64, 0, 65):
            assert wanted in lengths, (n, wanted)
        assert (np.asarray(c["b"][0]) < 0).any() and (np.asarray(c["b"][0]).astype(np.int64) + lengths > rows).any()
        ok = [AO.item_ok(s, ln, rows) for s, ln in zip(*c["b"])]
        frames = np.cumsum(lengths[ok])
        assert len({int(f) // 64 for f in frames}) > 3  # the b-frames run over several multiples of 64 lanes
        assert (c["seg"] < 0).any() and np.isnan(c["code"][0]).any() and not np.isinf(c["code"][0]).any()
        D, L = AO.case_tables(n, AO.COSINE, True)
        assert np.isnan(D).sum() == (L == 0).sum() == 4 * D.shape[0] and len(ok) - sum(ok) == 4


# ---- the conditions that keep the GPU cases honest ----------------------------------------------------------------------------------
def test_the_tie_case_tells_the_preference():
    D, L = AO.case_tables(AO.TIE_CASE, AO.JACCARD, False)
    D_rev, L_rev = AO.case_tables(AO.TIE_CASE, AO.JACCARD, False, True)
    assert np.array_equal(D, D_rev) and set(np.unique(AO.frame_costs(canonical(AO.distance_case(0)["code"], 2), range(40), range(40),
                                                                     AO.JACCARD, 2)).tolist()) == {0.0, 1.0}
    assert (L != L_rev).sum() * 2 >= L.size


def test_the_planted_case_separates_with_its_core():
    one, two = AO.planted_error(1), AO.planted_error(2)
    assert 0.05 < one < 0.30, one
    assert two <= 0.05 and two < one, two
    assert 0.4 <= AO.planted_error(1, shuffled=True) <= 0.6


def test_tied_triples_are_rare_except_in_the_tie_case():
    for tied in (False, True):
        c = AO.count_case(tied)
        for mode in (AO.ANY, AO.WITHIN, AO.ACROSS):
            ties, counted = AO.tied_triples(c["dist"], c["cat"], c["ctx"], c["spk"], c["n_cats"], mode)
            assert counted > 1000
            assert (ties * 10 >= counted) if tied else (ties * 100 <= counted), (tied, mode, ties, counted)
    assert AO.count_result(False, AO.ANY)[2] > 0  # NaN rows are skipped, not counted


def test_hand_cases_of_the_count():
    # items 0, 1 of category 0 and 2 of category 1; x = 0: a = 1, b = 2
    dist = np.array([[0, 1, 2], [1, 0, 1], [2, 2, 0]], np.float32)
    cat = np.array([0, 0, 1], np.int32)
    w, t, s = AO.abx_count(dist, 0, 3, cat, None, None, 2, AO.ANY)
    assert t.tolist() == [[0, 2], [0, 0]] and w.tolist() == [[0, 3], [0, 0]] and s == 0  # x = 0 wins (2), x = 1 ties (1)
    spk = np.array([0, 1, 1], np.int32)
    assert AO.abx_count(dist, 0, 3, cat, None, spk, 2, AO.WITHIN)[1].sum() == 0
    w, t, s = AO.abx_count(dist, 0, 3, cat, None, spk, 2, AO.ACROSS)  # only x = 0: a = 1 and b = 2 share speaker 1
    assert t.tolist() == [[0, 1], [0, 0]] and w.tolist() == [[0, 2], [0, 0]]
    ctx = np.array([0, 0, 1], np.int32)
    assert AO.abx_count(dist, 0, 3, cat, ctx, None, 2, AO.ANY)[1].sum() == 0
    dist[0, 2] = np.nan
    w, t, s = AO.abx_count(dist, 0, 3, cat, None, None, 2, AO.ANY)
    assert s == 1 and t.sum() == 1
    # windows add
    a, b = AO.abx_count(dist, 0, 1, cat, None, None, 2, AO.ANY), AO.abx_count(dist[1:], 1, 2, cat, None, None, 2, AO.ANY)
    assert np.array_equal(a[0] + b[0], w) and np.array_equal(a[1] + b[1], t) and a[2] + b[2] == s


# ---- the plain-torch parts of the package ---------------------------------------------------------------------------------------------
def test_items_from_labels_equals_the_oracle():
    rng = np.random.default_rng(12)
    for trial in range(6):
        n_utt, T = 4, 50
        lab = np.repeat(rng.integers(-1, 5, (n_utt, 25)), 2, axis=1)
        lab[rng.random((n_utt, T)) < 0.15] = rng.integers(-2, 5)
        mask = rng.random((n_utt, T)) > 0.08
        seg = np.where(mask, np.arange(n_utt)[:, None].repeat(T, 1), -1).reshape(-1)
        min_len, max_len = (1, 64) if trial % 2 == 0 else (2, 3)
        want = AO.items_from_labels(np.where(seg >= 0, lab.reshape(-1), -1), seg, min_len, max_len, n_classes=5)
        got = items_from_labels(torch.from_numpy(lab), frame_mask=torch.from_numpy(mask), min_len=min_len, max_len=max_len,
                                with_context=True, n_classes=5)
        assert len(got) == 4 and all(t.dtype == torch.int32 for t in got)
        for g, w in zip(got, want[:4]):
            assert g.tolist() == w.tolist()
        assert (got.dropped_short, got.dropped_long) == want[4:]
        flat = items_from_labels(torch.from_numpy(lab.reshape(-1)), segments=torch.from_numpy(seg))
        assert len(flat) == 3
        want_flat = AO.items_from_labels(np.where(seg >= 0, lab.reshape(-1), -1), seg)
        assert flat[0].tolist() == want_flat[0].tolist() and flat[2].tolist() == want_flat[2].tolist()
    assert want[4] > 0 and want[5] > 0
    # a hand case: none at the edges and next to unlabelled frames
    it = items_from_labels(torch.tensor([[0, 0, 1, 1, 1, -1, 2, 2]]), with_context=True, n_classes=3)
    assert [t.tolist() for t in it] == [[0, 2, 6], [2, 3, 2], [0, 1, 2], [0 * 4 + 2, 1 * 4 + 0, 0]]
    with pytest.raises(ValueError, match="integer"):
        items_from_labels(torch.zeros(4))
    with pytest.raises(ValueError, match="max_len"):
        items_from_labels(torch.zeros(4, dtype=torch.int64), max_len=65)
    with pytest.raises(ValueError, match="segments"):
        items_from_labels(torch.zeros(2, 4, dtype=torch.int64), segments=torch.zeros(8, dtype=torch.int64))


def test_abx_scores_arithmetic():
    wins2, total, skipped = AO.count_result(False, AO.ANY)
    s = AbxScores(torch.from_numpy(wins2), torch.from_numpy(total), skipped)
    score, error = AO.scores(wins2, total)
    assert s.score.dtype == torch.float64 and np.array_equal(np.isnan(s.score.numpy()), np.isnan(score))
    assert np.array_equal(np.nan_to_num(s.score.numpy()), np.nan_to_num(score))
    assert abs(s.error - error) < 1e-12 and s.n_triples == int(total.sum()) and s.skipped == skipped
    assert 0.0 < s.error < 0.5  # (the distances of the case lean towards the category)
    by = s.by_category.numpy()
    for c in range(5):
        row = score[c][~np.isnan(score[c])]
        assert abs(by[c] - row.mean()) < 1e-12
    worst = s.confusable(3)
    flat = sorted((score[c, d], c, d) for c in range(5) for d in range(5) if total[c, d] > 0)[:3]
    assert [(c, d) for c, d, _ in worst] == [(c, d) for _, c, d in flat] and worst[0][2] == flat[0][0]
    two = s + s
    assert np.array_equal(two.total.numpy(), 2 * total) and two.skipped == 2 * skipped and abs(two.error - s.error) < 1e-15
    empty = AbxScores(torch.zeros(2, 2, dtype=torch.int64), torch.zeros(2, 2, dtype=torch.int64), 0)
    assert math.isnan(empty.error) and bool(torch.isnan(empty.score).all()) and empty.confusable(2) == []
    with pytest.raises(ValueError, match="same categories"):
        s + empty
