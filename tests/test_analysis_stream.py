"""What the four analysis trackers share, seen through their public API and without a GPU: the feature window of the
constructors, the ranking behind the ``top_*_features`` functions, and the first two steps of every ``update`` (a code
that is not a pair is a ``TypeError``; CPU tensors are a ``WsaeError``, before anything needs a device)."""

from __future__ import annotations

import pytest
import torch

from whisper_sae import _native as N
from whisper_sae.analysis import (CoactivationTracker, GroupEffects, RunSummary, RunTracker, SegmentPooler,
                                  TriggeredAverageTracker, top_group_features, top_temporal_features,
                                  top_template_features)

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
