"""Temporal run statistics without a GPU: the numpy oracle of tests/runs_oracle.py against hand-worked sequences, the
bin function, the identities on every input the GPU test uses (and the conditions that keep those inputs from being
degenerate), every argument error of ``wsae_runs_update`` (raised before any HIP call), the workspace query, the header /
``SIGNATURES`` / exports, the Python layer's errors, ``summarize_runs`` / ``top_temporal_features`` on hand-made integer
state and ``FeatureEvents.sample_bounds``."""

from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest

import runs_oracle as RO

HEADER = Path(__file__).resolve().parents[1] / "include" / "wsae.h"
NAMES = ("wsae_runs_workspace_bytes", "wsae_runs_update")


def code_of(rows, k=2):
    """rows: per row a list of (index, value) -> (vals, idx) padded with (0, 0.0) entries."""
    vals, idx = np.zeros((len(rows), k), np.float32), np.zeros((len(rows), k), np.int32)
    for r, entries in enumerate(rows):
        for e, (i, v) in enumerate(entries):
            idx[r, e], vals[r, e] = i, v
    return vals, idx


def events_of(st, feature=None):
    ev = st["events"]
    keep = np.ones(ev["feature"].size, bool) if feature is None else ev["feature"] == feature
    return [tuple(ev[k][keep][n].item() for k in RO.EVENT_FIELDS) for n in range(int(keep.sum()))]


def test_oracle_on_hand_worked_sequences():
    # a single frame
    st = RO.update(code_of([[(3, 2.0)]]), 8, [0], 1)
    assert st["runs"].tolist() == [0, 0, 0, 1, 0, 0, 0, 0] and st["frames"][3] == 1 and st["dur_max"][3] == 1
    assert st["dur_hist"][3, 0] == 1 and st["dur_hist"].sum() == 1 and st["gap_hist"].sum() == 0 and st["total_rows"][0] == 1
    assert events_of(st) == [(3, 0, 0, 1, 2.0, 2.0)]
    # feature 1: rows 0-1, 4-5 (to the last row of the segment); feature 2: row 2 alone; sums in row order
    big = np.float32(2 ** 24)
    rows = [[(1, big)], [(1, 1.0), (2, -1.0)], [(2, 5.0)], [], [(1, 1.0)], [(1, 0.5), (1, 7.0)]]
    st = RO.update(code_of(rows), 4, [0] * 6, 1, seg_base=10)
    assert st["runs"].tolist() == [0, 2, 1, 0] and st["frames"].tolist() == [0, 4, 1, 0] and st["dur_sq"].tolist() == [0, 8, 1, 0]
    assert st["dur_hist"][1, 1] == 2 and st["gap_hist"][1, 1] == 1 and st["gap_hist"].sum() == 1  # one gap of 2
    assert events_of(st, 1) == [(1, 10, 0, 2, float(big), float(big)), (1, 10, 4, 2, 1.5, 1.0)]  # 2^24 + 1 = 2^24; first entry wins
    assert events_of(st, 2) == [(2, 10, 2, 1, 5.0, 5.0)]
    # the last row of segment 0 and the first row of segment 1: two runs and no gap
    st = RO.update(code_of([[(0, 1.0)], [(0, 1.0)], [(0, 2.0)], [(0, 1.0)]]), 2, [0, 0, 1, 1], 2)
    assert st["runs"][0] == 2 and st["frames"][0] == 4 and st["dur_hist"][0, 1] == 2 and st["gap_hist"].sum() == 0
    assert events_of(st) == [(0, 0, 0, 2, 2.0, 1.0), (0, 1, 0, 2, 3.0, 2.0)]
    # a padding row inside a run: two runs with gap 1; the start still counts rows from the segment's first row
    st = RO.update(code_of([[(0, 1.0)], [(0, 1.0)], [(0, 1.0)]]), 2, [0, -1, 0], 1)
    assert st["runs"][0] == 2 and st["frames"][0] == 2 and st["gap_hist"][0, 0] == 1 and st["total_rows"][0] == 2
    assert [e[2] for e in events_of(st)] == [0, 2]
    # non-monotonic ids [0, 1, 0]: segment 0 has two runs with gap 1, segment 1 one run
    st = RO.update(code_of([[(0, 1.0)], [(0, 1.0)], [(0, 1.0)]]), 2, [0, 1, 0], 2)
    assert st["runs"][0] == 3 and st["gap_hist"][0, 0] == 1 and st["gap_hist"].sum() == 1 and st["total_rows"][0] == 3
    assert [e[1:4] for e in events_of(st)] == [(0, 0, 1), (0, 2, 1), (1, 0, 1)]
    # a repeated index with mixed signs (the first ACTIVE entry gives the value), a value <= 0, an index out of range
    rows = [[(1, -3.0), (1, 4.0), (1, 9.0)], [(1, 0.0), (2, -1.0), (5, 1.0)], [(1, 2.0), (-1, 1.0), (4, 1.0)]]
    st = RO.update(code_of(rows, 3), 4, [0, 0, 0], 1)
    assert st["runs"].tolist() == [0, 2, 0, 0] and st["gap_hist"][1, 0] == 1
    assert events_of(st) == [(1, 0, 0, 1, 4.0, 4.0), (1, 0, 2, 1, 2.0, 2.0)]
    # an id >= n_seg is padding; a window keeps its features only; ev_min_len filters the events and nothing else
    st = RO.update(code_of(rows, 3), 8, [0, 7, 0], 2, f_lo=4, f_cols=2, ev_min_len=2)
    assert st["runs"].tolist() == [1, 0] and st["total_rows"][0] == 2 and events_of(st) == []
    # continuing from a state adds, and keeps the events in the canonical order
    one = RO.update(code_of([[(0, 1.0)], [(0, 1.0)]]), 2, [0, 0], 1, seg_base=1)
    two = RO.update(code_of([[(0, 1.0)]]), 2, [0], 1, seg_base=0, state=one)
    assert two["runs"][0] == 2 and two["dur_max"][0] == 2 and one["runs"][0] == 1 and two["total_rows"][0] == 3
    assert [e[1] for e in events_of(two)] == [0, 1]


def test_bin_function():
    want = {1: 0, 2: 1, 32: 31, 33: 32, 64: 32, 65: 33, 128: 33, 129: 34, 2 ** 20: 46, 2 ** 20 + 1: 47, 2 ** 31 - 1: 47}
    assert RO.bin_of(np.array(list(want))).tolist() == list(want.values())
    assert RO.BINS == 48 and RO.bin_of(np.arange(1, 200000)).max() == 44
    # a bin's lower length falls into the bin, and the length before it does not
    lower = RO.bin_lower(np.arange(48))
    assert lower[:33].tolist() == list(range(1, 33)) + [33] and lower[33] == 65 and lower[47] == 2 ** 20 + 1
    assert RO.bin_of(lower).tolist() == list(range(48)) and RO.bin_of(lower[1:] - 1).tolist() == list(range(47))


def test_persistent_generator_and_spoiling():
    rng = np.random.default_rng(0)
    vals, idx = RO.persistent_code(rng, 4000, 8, 256)
    assert vals.dtype == np.float32 and idx.dtype == np.int32 and bool((vals > 0).all())
    assert bool((idx >= 0).all()) and bool((idx < 256).all()) and bool((idx % 8 == np.arange(8)).all())  # distinct in a row
    stay = (idx[1:] == idx[:-1]).mean(0)
    assert stay[0] < 0.1 and stay[-1] > 0.98 and bool((np.diff(stay) > -0.02).all())  # holding times from 1 to 256 rows
    st = RO.update((vals, idx), 256, np.zeros(4000), 1)
    mean = st["frames"].sum() / st["runs"].sum()
    assert mean > 3 and st["dur_max"].max() > 100  # an i.i.d. code would have a mean run length of about 1
    sv, si = RO.spoil(rng, (vals, idx), 256)
    assert (sv <= 0).mean() > 0.02 and ((si < 0) | (si >= 256)).mean() > 0.004 and (si[:, 1:] == si[:, :-1]).mean() > 0.01
    with pytest.raises(ValueError):
        RO.persistent_code(rng, 10, 8, 4)


@pytest.fixture(scope="module")
def cases():
    out = {}
    for shape in RO.SHAPES:
        code, seg = RO.case(shape)
        out[shape] = (code, seg, RO.find_runs(code, shape[2], seg, shape[3]), RO.update(code, shape[2], seg, shape[3]))
    return out


@pytest.mark.parametrize("shape", RO.SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_identities_and_conditions_on_the_gpu_test_inputs(cases, shape):
    code, seg, rn, st = cases[shape]
    rows, k, hidden, n_seg = shape
    assert code[0].shape == (rows, k) and seg.shape == (rows,)
    # identities
    assert np.array_equal(st["frames"], np.bincount(rn["feature"], weights=rn["length"], minlength=hidden).astype(np.int32))
    assert np.array_equal(st["dur_hist"].sum(1), st["runs"])
    pairs = np.unique(rn["feature"] * n_seg + rn["segment"]) // n_seg  # one element per (feature, segment) that has a run
    assert np.array_equal(st["gap_hist"].sum(1), st["runs"] - np.bincount(pairs, minlength=hidden))
    assert st["total_rows"][0] == ((seg >= 0) & (seg < n_seg)).sum() and st["events"]["feature"].size == st["runs"].sum()
    dense = np.zeros((rows, hidden), bool)
    ok = (code[0] > 0) & (code[1] >= 0) & (code[1] < hidden) & ((seg >= 0) & (seg < n_seg))[:, None]
    dense[np.nonzero(ok)[0], code[1][ok]] = True
    assert np.array_equal(st["frames"], dense.sum(0))
    # conditions: no degenerate input
    if rows > 1:
        assert rn["length"].max() >= 2 and rn["gap_before"].max() >= 1
        assert (np.bincount(rn["feature"] * n_seg + rn["segment"]) > 1).any()
        assert (seg < 0).any() and (seg >= n_seg).any() or n_seg == 1
    if shape in RO.LARGE:
        assert rn["length"].max() > 32 and rn["gap_before"].max() > 32
    if shape == (3000, 32, 3072, 1):
        assert st["runs"][5] == 1 and st["dur_max"][5] == 3000 and st["dur_hist"][5, RO.bin_of(3000)] == 1 and RO.bin_of(3000) == 38
        assert st["runs"][9] == 1500 and st["dur_hist"][9, 0] == 1500 and st["gap_hist"][9, 0] == 1499
    if hidden == RO.WIDE:
        assert hidden > 2 * RO.TILE
        for a, b in RO.TWINS:
            assert st["runs"][a] > 3 and all(np.array_equal(st[f][a], st[f][b]) for f in RO.INT_FIELDS[:-1])
        lo, span = RO.WINDOW
        win = RO.update(code, hidden, seg, n_seg, f_lo=lo, f_cols=span)
        assert all(np.array_equal(win[f], st[f][lo:lo + span]) for f in RO.INT_FIELDS[:-1])
        assert lo % RO.TILE_EV and (lo + span) % RO.TILE_EV and lo % RO.TILE and (lo + span) % RO.TILE
    if n_seg > 2 and rows > 1:
        assert (np.diff(seg[(seg >= 0) & (seg < n_seg)]) < 0).any()  # non-monotonic ids


def test_oracle_grouping_of_whole_utterances_does_not_matter(cases):
    shape = RO.SHAPES[1]
    code, seg, _, want = cases[shape]
    hidden, n_seg = shape[2], shape[3]
    seg = np.where((seg >= 0) & (seg < n_seg), seg, -1)
    seg = np.maximum.accumulate(np.where(seg >= 0, seg, -1))  # whole utterances: non-decreasing, padding joins its neighbour
    want = RO.update(code, hidden, seg, n_seg)
    st = None
    for lo, hi in ((5, 9), (0, 2), (2, 5)):  # utterances lo .. hi - 1 per call, local ids, any order of the calls
        rows = (seg >= lo) & (seg < hi)
        st = RO.update((code[0][rows], code[1][rows]), hidden, seg[rows] - lo, hi - lo, seg_base=lo, state=st)
    assert all(np.array_equal(st[f], want[f]) for f in RO.INT_FIELDS)
    assert all(np.array_equal(st["events"][f].view(np.int32), want["events"][f].view(np.int32)) for f in RO.EVENT_FIELDS)


# ---- argument errors: made-up (aligned, never dereferenced) pointers, every case fails its checks first -----------------
def _runs(N, k=32, hidden=64, n_rows=16, n_seg=4, seg_base=0, f_lo=0, f_cols=64, ws=4096, ws_bytes=32, vals=4096, idx=4096,
          seg=4096, frames=4096, runs=4096, dur_max=4096, dur_sq=4096, dur_hist=4096, total=4096, gap=4096, ev_int=4096,
          ev_flt=4096, ev_cap=8, ev_min_len=1, ev_count=4096):
    return N.lib().wsae_runs_update(vals, idx, k, hidden, seg, n_rows, n_seg, seg_base, f_lo, f_cols, frames, runs, dur_max,
                                    dur_sq, dur_hist, gap, total, ev_int, ev_flt, ev_cap, ev_min_len, ev_count, ws, ws_bytes,
                                    None)


RUNS_ERRORS = {"k0": dict(k=0), "k129": dict(k=129), "window_past_end": dict(f_lo=40, f_cols=25),
               "window_negative": dict(f_lo=-1), "window_empty": dict(f_cols=0), "n_rows_2p31": dict(n_rows=2 ** 31),
               "n_rows_negative": dict(n_rows=-1), "n_seg0": dict(n_seg=0), "n_seg_negative": dict(n_seg=-3),
               "hidden0": dict(hidden=0), "seg_base_negative": dict(seg_base=-1), "seg_base_overflow": dict(seg_base=2 ** 31 - 2),
               "null_vals": dict(vals=None), "null_idx": dict(idx=None), "null_seg": dict(seg=None),
               "null_frames": dict(frames=None), "null_runs": dict(runs=None), "null_dur_max": dict(dur_max=None),
               "null_dur_sq": dict(dur_sq=None), "null_dur_hist": dict(dur_hist=None), "null_total": dict(total=None), "workspace_short": dict(ws_bytes=31), "workspace_null": dict(ws=None),
               "events_without_records": dict(ev_int=None), "events_without_values": dict(ev_flt=None),
               "events_without_cursor": dict(ev_count=None), "ev_cap_negative": dict(ev_cap=-1), "ev_min_len0": dict(ev_min_len=0),
               "ev_min_len0_without_events": dict(ev_min_len=0, ev_cap=0, ev_int=None, ev_flt=None, ev_count=None)}


@pytest.mark.parametrize("kw", list(RUNS_ERRORS.values()), ids=list(RUNS_ERRORS))
def test_runs_argument_errors_do_not_need_a_gpu(kw):
    from whisper_sae import _native as N
    assert _runs(N, **kw) == -1
    assert "wsae_runs_update" in N.last_error()


def test_an_empty_call_is_accepted_without_a_gpu():
    from whisper_sae import _native as N
    assert _runs(N, n_rows=0) == 0 and _runs(N, n_rows=0, ws=None, gap=None, ev_cap=0, ev_int=None, ev_flt=None, ev_count=None) == 0


def test_workspace_queries():
    from whisper_sae import _native as N
    wq = N.lib().wsae_runs_workspace_bytes
    assert wq(3_072_000, 32, 3072, 2048, 0, 3072) == 8 * 2048 and wq(0, 1, 1, 1, 0, 1) == 8
    assert wq(16, 128, 40960, 5, 40000, 960) == 40
    assert wq(16, 0, 64, 4, 0, 64) == -1 and wq(16, 129, 64, 4, 0, 64) == -1 and wq(2 ** 31, 32, 64, 4, 0, 64) == -1
    assert wq(-1, 32, 64, 4, 0, 64) == -1 and wq(16, 32, 64, 4, 60, 5) == -1 and wq(16, 32, 64, 4, -1, 5) == -1
    assert wq(16, 32, 64, 0, 0, 64) == -1 and wq(16, 32, 0, 4, 0, 64) == -1 and wq(16, 32, 64, 4, 0, 0) == -1


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
    defines = dict(re.findall(r"#define (WSAE_RUNS_[A-Z_]+) (\d+)", text))
    assert {k: int(v) for k, v in defines.items()} == {"WSAE_RUNS_MAX_K": N.RUNS_MAX_K, "WSAE_RUNS_BINS": N.RUNS_BINS}
    assert N.RUNS_BINS == RO.BINS
    for name in ("RunTracker", "RunSummary", "FeatureEvents", "summarize_runs", "top_temporal_features", "collect_runs"):
        assert name in A.__all__ and hasattr(A, name)


def test_python_layer_argument_errors():
    import torch

    from whisper_sae import _native as N
    from whisper_sae.analysis import RunTracker, collect_runs
    from whisper_sae.analysis.temporal import histogram_quantile
    from whisper_sae.sae.model import ReLUSAE
    code = (torch.ones(2, 3, 2), torch.zeros(2, 3, 2, dtype=torch.int32))
    with pytest.raises(N.WsaeError):
        RunTracker(8).update(code)  # CPU tensors
    with pytest.raises(N.WsaeError):
        RunTracker(8, device="cpu").summary()
    with pytest.raises(ValueError):
        RunTracker(8, f_window=(4, 5))
    with pytest.raises(ValueError):
        RunTracker(0)
    with pytest.raises(ValueError):
        RunTracker(8, max_events=-1)
    with pytest.raises(ValueError):
        RunTracker(8, max_events=4, min_event_len=0)
    with pytest.raises(TypeError):
        RunTracker(8).update(torch.ones(2, 3, 2))
    with pytest.raises(ValueError):
        RunTracker(8).events()  # no event list
    with pytest.raises(ValueError):
        RunTracker(8, gaps=False).gap_hist
    with pytest.raises(ValueError):
        RunTracker(8).merge(RunTracker(9))
    with pytest.raises(ValueError):
        histogram_quantile(torch.zeros(2, 48, dtype=torch.int32), 0.0)
    with pytest.raises(TypeError):
        collect_runs(ReLUSAE(16, 32), [torch.zeros(2, 4, 16)])


def test_summary_and_top_features_on_hand_made_state():
    import torch

    from whisper_sae.analysis import summarize_runs, top_temporal_features
    from whisper_sae.analysis.temporal import histogram_quantile
    # feature 0: runs of 1, 1, 2, 40 (gaps 3, 3, 70); feature 1: never on; feature 2: one run of 10; feature 3: 5 runs of 1
    lengths = {0: [1, 1, 2, 40], 1: [], 2: [10], 3: [1] * 5}
    gaps = {0: [3, 3, 70], 1: [], 2: [], 3: [2, 2, 2, 2]}
    st = RO.empty_state(4)
    for f, ds in lengths.items():
        d = np.array(ds, np.int64)
        st["runs"][f], st["frames"][f], st["dur_sq"][f] = d.size, d.sum(), (d * d).sum()
        st["dur_max"][f] = d.max() if d.size else 0
        np.add.at(st["dur_hist"][f], RO.bin_of(d), 1)
        np.add.at(st["gap_hist"][f], RO.bin_of(np.array(gaps[f], np.int64)), 1)
    st["total_rows"][0] = 200
    t = {k: torch.from_numpy(st[k]) for k in RO.INT_FIELDS}
    for frame_ms in (None, 20.0):
        got = summarize_runs(t["frames"], t["runs"], t["dur_max"], t["dur_sq"], t["dur_hist"], t["gap_hist"], t["total_rows"],
                             frame_ms=frame_ms)
        want = RO.summary(st, frame_ms)
        for name in got._fields:
            g = getattr(got, name)
            assert g.dtype == (torch.int64 if name in ("runs", "frames") else torch.float64) and tuple(g.shape) == (4,), name
            np.testing.assert_allclose(g.numpy(), want[name], rtol=1e-15, atol=0, equal_nan=True, err_msg=name)
    got = summarize_runs(t["frames"], t["runs"], t["dur_max"], t["dur_sq"], t["dur_hist"], t["gap_hist"], t["total_rows"])
    assert got.mean_duration.tolist()[0] == 11.0 and got.median_duration.tolist()[0] == 1.0 and got.max_duration.tolist() == [40, 0, 10, 1]
    assert got.median_gap.tolist()[0] == 3.0 and got.median_gap.tolist()[3] == 2.0 and bool(torch.isnan(got.median_gap[1:3]).all())
    assert got.persistence.tolist()[0] == 1 - 4 / 44 and got.persistence.tolist()[2:] == [0.9, 0.0]
    assert got.duty.tolist()[0] == 44 / 200 and got.event_rate.tolist()[3] == 5 / 200
    assert abs(got.std_duration[0].item() - np.std([1, 1, 2, 40])) < 1e-12 and got.std_duration.tolist()[2:] == [0.0, 0.0]
    for name in ("mean_duration", "std_duration", "median_duration", "persistence", "duty", "event_rate"):
        assert bool(torch.isnan(getattr(got, name)[1])), name
    assert histogram_quantile(t["dur_hist"], 1.0).tolist()[0] == 33.0  # the lower length of the bin (32, 64] that holds 40
    assert histogram_quantile(t["dur_hist"], 0.75).tolist()[0] == 2.0
    no_gaps = summarize_runs(t["frames"], t["runs"], t["dur_max"], t["dur_sq"], t["dur_hist"], None, t["total_rows"])
    assert bool(torch.isnan(no_gaps.median_gap).all())
    # ranking: NaN and features below min_runs are no candidates; ties go to the lower index
    idx, val = top_temporal_features(got, by="mean_duration", n=3)
    assert idx.tolist() == [0, 2, 3] and val.tolist() == [11.0, 10.0, 1.0]
    idx, val = top_temporal_features(got, by="mean_duration", n=3, min_runs=2)
    assert idx.tolist() == [0, 3]
    idx, val = top_temporal_features(got, by="persistence", n=2, largest=False)
    assert idx.tolist() == [3, 2] and val.tolist() == [0.0, 0.9]
    idx, _ = top_temporal_features(got, by="runs", n=10)
    assert idx.tolist() == [3, 0, 2]  # feature 1 has no run
    with pytest.raises(ValueError):
        top_temporal_features(got, by="loudness")


def test_sample_bounds():
    import torch

    from whisper_sae.analysis import FeatureEvents
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)  # noqa: E731
    ev = FeatureEvents(feature=i32(1, 1, 4), utterance=i32(0, 2, 2), start=i32(0, 3, 1499), length=i32(1, 10, 1),
                       total=torch.ones(3), peak=torch.ones(3))
    lo, hi = ev.sample_bounds(320)
    assert lo.dtype == torch.int64 and lo.tolist() == [0, 960, 479680] and hi.tolist() == [320, 4160, 480000]
    lo, hi = ev.sample_bounds(320, context_frames=5)
    assert lo.tolist() == [0, 0, 1494 * 320] and hi.tolist() == [6 * 320, 18 * 320, 1505 * 320]
    big = FeatureEvents(feature=i32(0), utterance=i32(0), start=i32(2 ** 31 - 2), length=i32(1), total=torch.ones(1),
                        peak=torch.ones(1))
    assert big.sample_bounds(320)[1].tolist() == [(2 ** 31 - 1) * 320]  # int64: no wrap
    with pytest.raises(ValueError):
        ev.sample_bounds(0)
    with pytest.raises(ValueError):
        ev.sample_bounds(320, context_frames=-1)
