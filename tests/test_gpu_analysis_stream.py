"""The forms in which the analysis trackers take a code, on the MI355X: one small batch given as ``[n_utt, T, k]`` with a
``frame_mask``, as flat rows whose padding is segment -1, and as flat rows with a flat ``frame_mask`` must leave the same
state, bit for bit (the float sums included: the order of the additions is fixed).  Three frames are padding: one
inside an utterance, where it splits a run, the last frame of an utterance and the first frame of another.  And the
files of the trackers that keep their tensors in a ``_state`` dict: their keys, and that they load into the same state."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from whisper_sae.analysis import (ActivationProfile, ActivationSampler, CoactivationTracker, LabelAssociation, RunTracker,
                                  SegmentPooler, TriggeredAverageTracker)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_UTT, T, K, HIDDEN, CHANNELS, LAGS = 3, 7, 4, 32, 3, (-2, 2)
ALWAYS = 5  # the feature that is active on every frame
MASKED = ((1, 3), (0, T - 1), (2, 0))  # (utterance, frame): inside utterance 1, the last of 0, the first of 2


def runs_of(active):
    """Maximal stretches of True in a 1-D array."""
    a = np.concatenate(([False], active))
    return int((a[1:] & ~a[:-1]).sum())


@pytest.fixture(scope="module")
def batch():
    rng = np.random.default_rng(20240611)
    others = np.array([f for f in range(HIDDEN) if f != ALWAYS])
    idx = np.empty((N_UTT, T, K), np.int32)
    vals = rng.uniform(0.1, 2.0, (N_UTT, T, K)).astype(np.float32)
    idx[..., 0] = ALWAYS
    vals[..., 0] = (0.5 + np.arange(N_UTT * T, dtype=np.float32) / 32).reshape(N_UTT, T)  # distinct on every frame
    for u in range(N_UTT):
        for t in range(T):
            idx[u, t, 1:] = rng.choice(others, K - 1, replace=False)
    mask = np.ones((N_UTT, T), bool)
    for u, t in MASKED:
        mask[u, t] = False
    signal = rng.standard_normal((N_UTT, T, CHANNELS)).astype(np.float32)
    # the host arrays are what the test means them to be
    assert (vals > 0).all() and len(set(vals[..., 0].ravel().tolist())) == N_UTT * T
    assert all(len(set(idx[u, t].tolist())) == K for u in range(N_UTT) for t in range(T))
    u, t = MASKED[0]
    assert 0 < t < T - 1 and mask[u, t - 1] and mask[u, t + 1]  # the padding frame has a live frame on both sides,
    assert idx[u, t - 1, 0] == ALWAYS and idx[u, t + 1, 0] == ALWAYS  # ... on which the feature is active:
    assert sum(runs_of(mask[u]) for u in range(N_UTT)) == 4  # it has 4 runs, not 3
    assert mask.any(1).all()  # every utterance keeps a live frame
    utt = np.repeat(np.arange(N_UTT, dtype=np.int32), T)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    return {"code3": (dev(vals), dev(idx)), "code2": (dev(vals.reshape(-1, K)), dev(idx.reshape(-1, K))),
            "mask3": dev(mask), "mask2": dev(mask.reshape(-1)), "utt": dev(utt),
            "utt_or_pad": dev(np.where(mask.reshape(-1), utt, -1).astype(np.int32)),
            "signal3": dev(signal), "signal2": dev(signal.reshape(-1, CHANNELS))}


def three_forms(make, b, with_signal=False):
    """Three trackers: (a) numbered with a frame mask, (b) flat with -1 segments, (c) flat with a flat frame mask."""
    sig3, sig2 = ((b["signal3"],), (b["signal2"],)) if with_signal else ((), ())
    ta, tb, tc = make(), make(), make()
    ta.update(b["code3"], *sig3, frame_mask=b["mask3"])
    tb.update(b["code2"], *sig2, segments=b["utt_or_pad"])
    tc.update(b["code2"], *sig2, segments=b["utt"], frame_mask=b["mask2"])
    torch.cuda.synchronize()
    return ta, tb, tc


def same_fields(trackers, fields):
    a = trackers[0]
    for other in trackers[1:]:
        for f in fields:
            x, y = getattr(a, f), getattr(other, f)
            assert x.dtype == y.dtype and torch.equal(x, y), f


def test_segment_pooler(batch):
    trackers = three_forms(lambda: SegmentPooler(HIDDEN, N_UTT, counts=True, device=DEV), batch)
    same_fields(trackers, ("sums", "counts", "frames"))
    a = trackers[0]
    assert a.frames.tolist() == [T - 1] * N_UTT and a.counts[:, ALWAYS].tolist() == [T - 1] * N_UTT


def test_run_tracker(batch):
    trackers = three_forms(lambda: RunTracker(HIDDEN, max_events=64, device=DEV), batch)
    same_fields(trackers, ("frames", "runs", "max_run", "sum_squares", "duration_hist", "gap_hist", "total_rows"))
    a = trackers[0]
    assert int(a.runs[ALWAYS]) == 4 and int(a.frames[ALWAYS]) == N_UTT * T - len(MASKED) == int(a.total_rows)
    ev = [t.events() for t in trackers]
    assert ev[0].feature.numel() == a.event_count > 0
    for other in ev[1:]:
        for f in ev[0]._fields:
            x, y = getattr(ev[0], f), getattr(other, f)
            assert x.dtype == y.dtype and torch.equal(x, y), f


def test_triggered_average_tracker(batch):
    make = lambda: TriggeredAverageTracker(HIDDEN, CHANNELS, lags=LAGS, device=DEV)  # noqa: E731
    trackers = three_forms(make, batch, with_signal=True)
    same_fields(trackers, ("sums", "weights", "counts", "sig_sum", "sig_sq", "total_rows"))
    a = trackers[0]
    assert int(a.total_rows) == N_UTT * T - len(MASKED) == int(a.counts[ALWAYS, -LAGS[0]])  # (lag 0)


def test_coactivation_tracker(batch):
    ta, tb = CoactivationTracker(HIDDEN, device=DEV), CoactivationTracker(HIDDEN, device=DEV)
    ta.update(batch["code3"], row_mask=batch["mask3"])
    tb.update(batch["code2"], row_mask=batch["mask2"])
    same_fields((ta, tb), ("counts", "fire_a"))
    assert ta.rows == tb.rows == N_UTT * T - len(MASKED) == int(ta.fire_a[ALWAYS])


# ---- saved files: the keys a file has had since the tracker was added (a file written then must load now, and back) -------------
EDGES = torch.tensor([[0.5, 1.0]]).repeat(HIDDEN, 1)
SAVED = {
    "label_association": (lambda: LabelAssociation(HIDDEN, 3, EDGES, lags=(-1, 1), device=DEV),
                          ("hidden", "n_classes", "lags", "f_window", "edges", "form", "submitted", "state"),
                          ("cnt", "pair_rows")),
    "activation_profile": (lambda: ActivationProfile(HIDDEN, device=DEV), ("hidden", "f_window", "submitted", "state"),
                           ("fires", "hist", "max_bits", "min_bits", "over", "sum_q", "total_rows")),
    "activation_sampler": (lambda: ActivationSampler(HIDDEN, EDGES, keep=4, seed=3, device=DEV),
                           ("hidden", "f_window", "keep", "seed", "ordinal_base", "next", "records", "edges", "state"),
                           ("keys", "svals", "seen")),
    "run_tracker": (lambda: RunTracker(HIDDEN, max_events=64, device=DEV),
                    ("hidden", "f_window", "gaps", "max_events", "min_event_len", "next", "form", "submitted", "state"),
                    ("frames", "runs", "dur_max", "dur_sq", "dur_hist", "gap_hist", "total_rows", "ev_int", "ev_flt", "ev_count")),
    "run_tracker_bare": (lambda: RunTracker(HIDDEN, gaps=False, device=DEV),  # (no gap histogram, no events: None in the file)
                         ("hidden", "f_window", "gaps", "max_events", "min_event_len", "next", "form", "submitted", "state"),
                         ("frames", "runs", "dur_max", "dur_sq", "dur_hist", "gap_hist", "total_rows", "ev_int", "ev_flt",
                          "ev_count")),
    "triggered_average": (lambda: TriggeredAverageTracker(HIDDEN, CHANNELS, lags=LAGS, device=DEV),
                          ("hidden", "channels", "lags", "trigger", "weight", "f_window", "form", "state"),
                          ("acc", "wsum", "cnt", "sig_sum", "sig_sq", "total_rows")),
}


@pytest.mark.parametrize("kind", sorted(SAVED))
def test_saved_file_keys_and_round_trip(batch, kind, tmp_path):
    make, top_keys, state_keys = SAVED[kind]
    t = make()
    if kind == "label_association":
        t.update(batch["code3"], torch.arange(N_UTT * T, device=DEV).reshape(N_UTT, T) % 4 - 1, frame_mask=batch["mask3"])
    elif kind == "triggered_average":
        t.update(batch["code3"], batch["signal3"], frame_mask=batch["mask3"])
    else:
        t.update(batch["code3"], frame_mask=batch["mask3"])
    t.save(tmp_path / "t.pt")
    data = torch.load(tmp_path / "t.pt", map_location="cpu", weights_only=True)
    assert tuple(data) == top_keys and tuple(data["state"]) == state_keys
    assert all(v is None or v.device.type == "cpu" for v in data["state"].values())
    assert [name for name, v in data["state"].items() if v is None] == (
        ["gap_hist", "ev_int", "ev_flt", "ev_count"] if kind == "run_tracker_bare" else [])
    back = type(t).load(tmp_path / "t.pt", device=DEV)
    assert tuple(back._state) == state_keys
    for name, v in t._state.items():
        w = back._state[name]
        assert (v is None and w is None) or (v.dtype == w.dtype and v.device == w.device and torch.equal(v, w)), name
    for attr in ("_form", "_submitted", "_next", "_records"):
        assert getattr(back, attr, None) == getattr(t, attr, None), attr
    assert int(t._state[state_keys[0]].ne(0).sum()) > 0  # (a state that has seen the batch)
