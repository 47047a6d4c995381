"""What the analysis trackers share, seen through their public API and without a GPU: the feature window of the
constructors, the ranking behind the ``top_*_features`` functions, and the first two steps of every ``update`` (a code
that is not a pair is a ``TypeError``; CPU tensors are a ``WsaeError``, before anything needs a device).  Then the plain
functions of ``whisper_sae.analysis._stream`` that the newer trackers share: the column map of a feature subset, the
labels of a frame, the arguments of a k-sparse curve and the row bound of an int32 state."""

from __future__ import annotations

import pytest
import torch

from whisper_sae import _native as N
from whisper_sae.analysis import (ActivationProfile, CoactivationTracker, GroupEffects, LabelAssociation, RunSummary, RunTracker,
                                  SegmentPooler, SparseProbe, SparseRegression, TriggeredAverageTracker, regression_curve,
                                  sparse_probe_curve, top_group_features, top_temporal_features, top_template_features)
from whisper_sae.analysis import _stream

HIDDEN = 32
TRACKERS = {
    "pooler": lambda w: SegmentPooler(HIDDEN, 4, f_window=w),
    "runs": lambda w: RunTracker(HIDDEN, f_window=w),
    "triggered": lambda w: TriggeredAverageTracker(HIDDEN, 3, f_window=w),
    "coactivation": lambda w: CoactivationTracker(HIDDEN, a_window=w),
}


def window_of(t):
    return (t.a_lo, t.a_rows) if isinstance(t, CoactivationTracker) else (t.f_lo, t.f_cols)


@pytest.mark.parametrize("kind", sorted(TRACKERS))
def test_feature_window(kind):
    make = TRACKERS[kind]
    assert window_of(make(None)) == (0, HIDDEN)
    assert window_of(make((0, HIDDEN))) == (0, HIDDEN)
    assert window_of(make((HIDDEN - 1, 1))) == (HIDDEN - 1, 1)  # one column at the top end
    for bad in ((-1, 4), (4, 0), (HIDDEN - 2, 3)):  # a negative start, no columns, past the end
        with pytest.raises(ValueError, match="outside"):
            make(bad)


# six features: a tie (1 and 2), a NaN (3), and the largest score on a feature that is no candidate (4)
SCORE = [3.0, 5.0, 5.0, float("nan"), 9.0, 1.0]
CANDIDATE = [True, True, True, True, False, True]
RANKED = [1, 2, 0, 5]  # descending, the tie to the lower index; neither 3 nor 4


def rank_temporal(n):
    score, zero = torch.tensor(SCORE, dtype=torch.float64), torch.zeros(6, dtype=torch.float64)
    fields = {name: zero for name in RunSummary._fields}
    fields.update(runs=torch.tensor(CANDIDATE).to(torch.int64), mean_duration=score)
    order, values = top_temporal_features(RunSummary(**fields), by="mean_duration", n=n, min_runs=1)
    return order, values, score


def rank_template(n):
    score = torch.tensor(SCORE, dtype=torch.float64)
    counts = torch.tensor(CANDIDATE).to(torch.int64)[:, None]
    order, values = top_template_features(score[:, None, None], by="contrast_peak", n=n, min_count=1, counts=counts)
    return order, values, score


def rank_group(n):
    score = torch.tensor(SCORE, dtype=torch.float64)
    lo = torch.where(torch.tensor(CANDIDATE), 0.5, -0.5).double()  # (no candidate: the interval holds zero)
    zero = torch.zeros(6, dtype=torch.float64)
    eff = GroupEffects(d=score, g=score, mean_a=zero, mean_b=zero, ci_lo=lo, ci_hi=lo + 1.0, se=zero, n_a=3, n_b=3, n_boot=9)
    order, values = top_group_features(eff, n=n)
    return order, values, score


@pytest.mark.parametrize("rank", [rank_temporal, rank_template, rank_group])
def test_ranking(rank):
    for n, want in ((3, RANKED[:3]), (4, RANKED), (10, RANKED), (1, RANKED[:1]), (0, [])):
        order, values, score = rank(n)
        assert order.tolist() == want, (n, order.tolist())
        assert torch.equal(values, score[order])
    assert len(rank(10)[0]) < 10


def test_smallest_first_keeps_the_tie_rule():
    score, zero = torch.tensor(SCORE, dtype=torch.float64), torch.zeros(6, dtype=torch.float64)
    fields = {name: zero for name in RunSummary._fields}
    fields.update(runs=torch.tensor(CANDIDATE).to(torch.int64), mean_duration=score)
    order, _ = top_temporal_features(RunSummary(**fields), by="mean_duration", n=6, largest=False)
    assert order.tolist() == [5, 0, 1, 2]


def update_of(kind):
    t = TRACKERS[kind](None)
    if kind == "triggered":
        return lambda code: t.update(code, torch.zeros(2, 3, 3))
    return t.update


@pytest.mark.parametrize("kind", sorted(TRACKERS))
def test_update_checks_the_pair_then_the_device(kind):
    update = update_of(kind)
    with pytest.raises(TypeError, match="pair"):
        update(torch.ones(2, 3, 2))
    with pytest.raises(N.WsaeError):
        update((torch.ones(2, 3, 2), torch.zeros(2, 3, 2, dtype=torch.int32)))
    with pytest.raises(N.WsaeError):  # ... before the shapes are looked at
        update((torch.ones(2, 3, 2), torch.zeros(2, 3, dtype=torch.int32)))


# ---- the column map: built on the CPU, by one function for both trackers ---------------------------------------------------------
SUBSET_TRACKERS = {"probe": lambda **kw: SparseProbe(16, 3, **kw), "regression": lambda **kw: SparseRegression(16, 2, **kw)}


@pytest.mark.parametrize("kind", sorted(SUBSET_TRACKERS))
def test_column_map(kind):
    make = SUBSET_TRACKERS[kind]
    t = make()
    assert t._col_of is None and t.n_cols == 16 and t.feature_index.dtype == torch.int64
    assert t.feature_index.tolist() == list(range(16))
    for features in (torch.tensor([7, 2, 9]), torch.tensor([7, 2, 9], dtype=torch.int32), [7, 2, 9]):  # a permuted subset
        t = make(features=features)
        assert t.n_cols == 3 and t.feature_index.tolist() == [7, 2, 9] and t.feature_index.dtype == torch.int64
        assert t._col_of.dtype == torch.int32 and t._col_of.device.type == "cpu"
        want = [-1] * 16
        want[7], want[2], want[9] = 0, 1, 2
        assert t._col_of.tolist() == want
    for bad, text in ((torch.tensor([[1, 2]]), "features must be a 1-D tensor of at least one index, got (1, 2) torch.int64"),
                      (torch.tensor([], dtype=torch.int64),
                       "features must be a 1-D tensor of at least one index, got (0,) torch.int64"),
                      (torch.tensor([0.5]), "features must be a 1-D tensor of at least one index, got (1,) torch.float32"),
                      (torch.tensor([True]), "features must be a 1-D tensor of at least one index, got (1,) torch.bool"),
                      (torch.tensor([3, -1]), "features must lie in [0, 16)"), (torch.tensor([16]), "features must lie in [0, 16)"),
                      (torch.tensor([4, 9, 4]), "features holds an index twice")):
        with pytest.raises(ValueError) as e:
            make(features=bad)
        assert str(e.value) == text
    for lag in (-1025, 1025):  # the lag is looked at before the features
        with pytest.raises(ValueError) as e:
            make(lag=lag, features=torch.tensor([16]))
        assert str(e.value) == f"lag must be in -1024..1024, got {lag}"
    assert make(lag=-1024).lag == -1024 and make(lag=1024).lag == 1024


def test_column_table_is_the_map_of_a_fit():
    feats = torch.tensor([5, 0, 3])
    assert _stream.column_table(feats, 6).tolist() == [1, -1, -1, 2, -1, 0]
    assert torch.equal(_stream.column_map(feats, 6)[1], _stream.column_table(feats, 6))


# ---- the labels of a frame ------------------------------------------------------------------------------------------------------
def test_frame_labels():
    vals = torch.zeros(2, 3, 4)  # [n_utt, T, k]
    C = 5
    labels = torch.tensor([[0, -1, C], [C - 1, 2 ** 31 + 1, -2 ** 40]])  # unlabelled, one past the classes, beyond int32
    got = _stream.frame_labels(vals, labels, C)
    assert got.dtype == torch.int32 and got.is_contiguous() and got.tolist() == [0, -1, -1, C - 1, -1, -1]
    for dtype in (torch.int8, torch.int16, torch.int32, torch.uint8):
        assert _stream.frame_labels(vals, torch.tensor([[0, 1, 2], [3, 4, 5]], dtype=dtype), C).tolist() == [0, 1, 2, 3, 4, -1]
    assert _stream.frame_labels(torch.zeros(0, 4), torch.zeros(0, dtype=torch.int64), C).shape == (0,)
    text = "labels must hold one integer per frame, in the shape (2, 3) of the code's frames: got {} {}"
    for bad, shape in ((torch.zeros(2, 3, dtype=torch.bool), "(2, 3)"), (torch.zeros(2, 3), "(2, 3)"),
                       (torch.zeros(2, 3, dtype=torch.float64), "(2, 3)"), (torch.zeros(6, dtype=torch.int64), "(6,)"),
                       (torch.zeros(2, 3, 1, dtype=torch.int64), "(2, 3, 1)")):
        for check in (lambda: _stream.frame_labels(vals, bad, C), lambda: _stream.check_frame_labels(vals, bad)):
            with pytest.raises(ValueError) as e:
                check()
            assert str(e.value) == text.format(shape, bad.dtype)


# ---- the arguments of a k-sparse curve ------------------------------------------------------------------------------------------
def test_curve_arguments():
    ranking, sizes = _stream.curve_arguments(torch.tensor([[7, 3], [30, 1]], dtype=torch.int32), [1, 4.0, 2])
    assert ranking.dtype == torch.int64 and ranking.tolist() == [7, 3, 30, 1] and sizes == (1, 4, 2)
    assert _stream.curve_arguments([4, 2], (2,))[0].tolist() == [4, 2]
    for bad in ((), (0, 1), (1, 5), (-1,)):
        with pytest.raises(ValueError) as e:
            _stream.curve_arguments(torch.tensor([7, 3, 30, 1]), bad)
        assert str(e.value) == f"sizes must lie in 1..4, the length of the ranking: got {tuple(bad)}"
    # both curves make this check first, before they need data or a device
    stats = SparseRegression(40, 2, features=torch.tensor([7, 3, 30]), device="cpu")
    for curve in (lambda: regression_curve(stats, (), torch.tensor([7, 3]), sizes=(1, 3)),
                  lambda: sparse_probe_curve((), (), torch.tensor([7, 3]), sizes=(1, 3), hidden=40, n_classes=2)):
        with pytest.raises(ValueError) as e:
            curve()
        assert str(e.value) == "sizes must lie in 1..2, the length of the ranking: got (1, 3)"


def test_check_index():
    assert _stream.check_index(torch.tensor(2), 3, "class") == 2 and _stream.check_index(0, 1, "target") == 0
    for c in (-1, 3):
        with pytest.raises(ValueError) as e:
            _stream.check_index(c, 3, "class")
        assert str(e.value) == f"class {c} is outside [0, 3)"
    with pytest.raises(ValueError) as e:  # before the probe needs its parameters on a device
        SparseProbe(16, 3).top_weights(3)
    assert str(e.value) == "class 3 is outside [0, 3)"


# ---- the row bound of an int32 state --------------------------------------------------------------------------------------------
BOUNDED = {"LabelAssociation": lambda: LabelAssociation(HIDDEN, 3), "ActivationProfile": lambda: ActivationProfile(HIDDEN),
           "RunTracker": lambda: RunTracker(HIDDEN), "SegmentPooler": lambda: SegmentPooler(HIDDEN, 4)}


@pytest.mark.parametrize("name", sorted(BOUNDED))
def test_row_bound(name):
    assert _stream.MAX_ROWS == 2 ** 31 - 1
    t = BOUNDED[name]()
    t._submitted = 2 ** 31 - 1 - 100
    _stream.check_row_bound(t, 100)  # exactly MAX_ROWS frames
    _stream.check_row_bound(t, 100, merging=True)
    with pytest.raises(N.WsaeError) as e:
        _stream.check_row_bound(t, 101)
    assert str(e.value) == f"{name}: 2147483547 + 101 frames exceed 2147483647, the range of the int32 state"
    with pytest.raises(N.WsaeError) as e:
        _stream.check_row_bound(t, 101, merging=True)
    assert str(e.value) == f"{name}.merge: 2147483547 + 101 frames exceed 2147483647"


@pytest.mark.parametrize("name", ["ActivationProfile", "LabelAssociation", "RunTracker"])
def test_merge_checks_the_row_bound_before_it_needs_a_device(name):
    a, b = BOUNDED[name](), BOUNDED[name]()
    a._submitted, b._submitted = 2 ** 31 - 1 - 100, 100
    a.merge(b)  # exactly MAX_ROWS frames (neither has a state yet: nothing to add, no device)
    a._submitted, b._submitted = 2 ** 31 - 1 - 100, 101
    with pytest.raises(N.WsaeError) as e:
        a.merge(b)
    assert str(e.value) == f"{name}.merge: 2147483547 + 101 frames exceed 2147483647"
