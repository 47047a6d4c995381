"""Feature-triggered averages without a GPU: the numpy oracle of tests/sta_oracle.py against hand-worked sequences and
against its own plain-loop form, the identities that tie it to the run statistics of tests/runs_oracle.py on every input
the GPU test uses (and the conditions that keep those inputs from being degenerate), every argument error of
``wsae_sta_update`` (raised before any HIP call), the workspace query, the header / ``SIGNATURES`` / exports, the Python
layer's errors, ``mel_frames`` / ``as_spectrogram`` and the averages, contrast and ranking on hand-made state.

Which input can show what: terms are truncated "at both ends" only where the lags have both signs (with one-sided lags
the far end must be truncated against the near one; with the single lag 0 nothing is), and a segment can be shorter
than the lag span only where there is more than one segment - the inputs "one", "flagship" and "order" are one clean
segment by their definition."""

from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest

import runs_oracle as RO
import sta_oracle as SO

HEADER = Path(__file__).resolve().parents[1] / "include" / "wsae.h"
NAMES = ("wsae_sta_workspace_bytes", "wsae_sta_update")
NAN = float("nan")


def code_of(rows, k=2):
    """rows: per row a list of (index, value) -> (vals, idx) padded with (0, 0.0) entries."""
    vals, idx = np.zeros((len(rows), k), np.float32), np.zeros((len(rows), k), np.int32)
    for r, entries in enumerate(rows):
        for e, (i, v) in enumerate(entries):
            idx[r, e], vals[r, e] = i, v
    return vals, idx


def col(*v):
    return np.array(v, np.float32).reshape(-1, 1)


def test_oracle_on_hand_worked_sequences():
    # a single frame: only lag 0 has a row
    st = SO.update(code_of([[(3, 2.0)]]), 8, [0], col(5.0), (-1, 1))
    assert st["acc"][3, :, 0].tolist() == [0.0, 10.0, 0.0] and st["wsum"][3].tolist() == [0.0, 2.0, 0.0]
    assert st["cnt"][3].tolist() == [0, 1, 0] and st["cnt"].sum() == 1 and st["acc"].shape == (8, 3, 1)
    # a run that reaches its segment's last row: positive lags are cut off, cnt differs per lag
    run = code_of([[], [], [(1, 1.0)], [(1, 3.0)], [(1, 1.0)], []])
    seg, y = [0, 0, 0, 0, 1, 1], col(1, 2, 4, 8, 16, 32)
    st = SO.update(run, 4, seg, y, (0, 2))
    assert st["acc"][1, :, 0].tolist() == [1 * 4 + 3 * 8 + 16.0, 8.0 + 32.0, 0.0]
    assert st["wsum"][1].tolist() == [5.0, 2.0, 0.0] and st["cnt"][1].tolist() == [3, 2, 0]
    # lags that do not contain 0: the same cells
    ahead = SO.update(run, 4, seg, y, (1, 2))
    assert all(SO.same_bits(ahead[f], st[f][:, 1:]) for f in SO.FIELDS)
    # a padding row inside the window: its (NaN) signal is never read, and it triggers nothing
    st = SO.update(code_of([[(0, 2.0)], [(0, 7.0)], [(0, 1.0)]]), 2, [0, -1, 0], col(1, NAN, 4), (-2, 2))
    assert st["acc"][0, :, 0].tolist() == [1.0, 0.0, 6.0, 0.0, 8.0] and st["wsum"][0].tolist() == [1.0, 0.0, 3.0, 0.0, 2.0]
    assert st["cnt"][0].tolist() == [1, 0, 2, 0, 1]
    # ids [0, 1, 0]: row 2 belongs to the segment of row 0, row 1 to neither
    for trigger in (SO.ALL, SO.ONSET):  # (every row starts a run: the ids differ)
        st = SO.update(code_of([[(0, 1.0)], [(0, 1.0)], [(0, 1.0)]]), 2, [0, 1, 0], col(1, 2, 4), (-2, 2), trigger=trigger)
        assert st["acc"][0, :, 0].tolist() == [1.0, 0.0, 7.0, 0.0, 4.0] and st["cnt"][0].tolist() == [1, 0, 3, 0, 1]
    # a repeated index with mixed signs (the first ACTIVE entry gives the weight), a value <= 0, an index out of range
    rows = [[(1, -3.0), (1, 4.0), (1, 9.0)], [(1, 0.0), (2, -1.0), (5, 1.0)], [(1, 2.0), (-1, 1.0), (4, 1.0)]]
    st = SO.update(code_of(rows, 3), 4, None, col(1, 10, 100), (0, 0))
    assert st["acc"][:, 0, 0].tolist() == [0.0, 204.0, 0.0, 0.0] and st["wsum"][:, 0].tolist() == [0.0, 6.0, 0.0, 0.0]
    assert st["cnt"][:, 0].tolist() == [0, 2, 0, 0]
    one = SO.update(code_of(rows, 3), 4, None, col(1, 10, 100), (0, 0), weight=SO.ONE)
    assert one["acc"][1, 0, 0] == 101.0 and one["wsum"][1, 0] == 2.0
    # a window keeps its features only (4 and 5 are features now, outside it)
    st = SO.update(code_of(rows, 3), 8, None, col(1, 10, 100), (0, 0), f_lo=1, f_cols=2)
    assert st["acc"][:, 0, 0].tolist() == [204.0, 0.0] and st["cnt"][:, 0].tolist() == [2, 0]
    # the onset rule on a run of 3: one trigger
    held = code_of([[], [(0, 2.0)], [(0, 3.0)], [(0, 4.0)], []])
    st = SO.update(held, 2, None, col(1, 2, 4, 8, 16), (0, 1), trigger=SO.ONSET)
    assert st["acc"][0, :, 0].tolist() == [4.0, 8.0] and st["cnt"][0].tolist() == [1, 1] and st["wsum"][0].tolist() == [2.0, 2.0]
    st = SO.update(held, 2, None, col(1, 2, 4, 8, 16), (0, 1))
    assert st["acc"][0, :, 0].tolist() == [2 * 2 + 3 * 4 + 4 * 8.0, 2 * 4 + 3 * 8 + 4 * 16.0] and st["cnt"][0].tolist() == [3, 3]
    # a padding row ends a run: the row behind it is an onset again
    st = SO.update(code_of([[(0, 1.0)], [(0, 1.0)], [(0, 1.0)]]), 2, [0, -1, 0], col(1, 2, 4), (0, 0), trigger=SO.ONSET)
    assert st["cnt"][0, 0] == 2 and st["acc"][0, 0, 0] == 5.0
    # continuing from a state adds to it in order and leaves the old state alone
    first = SO.update(run, 4, seg, y, (0, 2))
    second = SO.update(code_of([[(1, 0.5)]]), 4, [0], col(3), (0, 2), state=first)
    assert second["acc"][1, :, 0].tolist() == [45.5, 40.0, 0.0] and second["cnt"][1].tolist() == [4, 2, 0]
    assert first["cnt"][1].tolist() == [3, 2, 0]


@pytest.mark.parametrize("mode", SO.MODES, ids=lambda m: f"trigger{m[0]}_weight{m[1]}")
def test_plain_loops_pin_the_vectorised_oracle(mode):
    rng = np.random.default_rng(11)
    code = RO.spoil(rng, RO.persistent_code(rng, 40, 3, 6), 6)
    seg = np.array([-1] + [0] * 9 + [1] * 3 + [0] * 2 + [-2] + [2] * 20 + [3] * 4, np.int32)
    y = np.ldexp(rng.standard_normal((40, 2)), rng.integers(-20, 21, (40, 2))).astype(np.float32)
    for lags in ((-2, 3), (2, 4), (0, 0)):
        fast = SO.update(code, 6, seg, y, lags, trigger=mode[0], weight=mode[1])
        slow = SO.update_loops(code, 6, seg, y, lags, trigger=mode[0], weight=mode[1])
        assert fast["cnt"].sum() > 0 and all(SO.same_bits(fast[f], slow[f]) for f in SO.FIELDS)
    window = SO.update(code, 6, seg, y, (-2, 3), f_lo=2, f_cols=3, trigger=mode[0], weight=mode[1])
    whole = SO.update(code, 6, seg, y, (-2, 3), trigger=mode[0], weight=mode[1])
    assert all(SO.same_bits(window[f], whole[f][2:5]) for f in SO.FIELDS)


@pytest.fixture(scope="module")
def inputs():
    return {name: SO.case(name) for name in SO.CASES}


@pytest.mark.parametrize("name", list(SO.CASES))
def test_gpu_inputs_are_not_degenerate(inputs, name):
    (vals, idx), seg, y = inputs[name]
    rows, k, hidden, C, lags, n_seg = SO.CASES[name]
    assert vals.shape == idx.shape == (rows, k) and y.shape == (rows, C) and seg.shape == (rows,)
    cnt = SO.update((vals, idx), hidden, seg, np.zeros((rows, 1), np.float32), lags, weight=SO.ONE)["cnt"]
    assert cnt.sum() > 0
    L = lags[1] - lags[0] + 1
    if lags[0] < 0 < lags[1]:  # terms truncated at both ends
        at0 = cnt[:, -lags[0]]
        assert bool(((cnt[:, 0] < at0) & (cnt[:, -1] < at0) & (cnt[:, 0] > 0) & (cnt[:, -1] > 0)).any())
    elif L > 1:  # one-sided lags: the far end loses terms the near end has
        near, far = (cnt[:, 0], cnt[:, -1]) if lags[0] >= 0 else (cnt[:, -1], cnt[:, 0])
        assert bool(((far < near) & (far > 0)).any())
    if n_seg > 1:  # a segment shorter than the lag span
        live = np.nonzero(seg >= 0)[0]
        starts = np.nonzero(np.diff(seg, prepend=-9) != 0)[0]
        lengths = np.diff(np.append(starts, rows))[seg[starts] >= 0]
        assert live.size and lengths.min() < L or L == 1
        assert seg[0] < 0 and seg[-1] < 0 and bool((seg[1:-1] < 0).any())  # padding at the start, inside and at the end
        assert bool((np.diff(seg[seg >= 0].astype(np.int64)) < 0).any())  # ids that are not monotonic
    if name not in ("one", "order"):  # the spoiled code
        assert bool((vals <= 0).any()) and bool(((idx < 0) | (idx >= hidden)).any())
        assert k == 1 or bool((idx[:, 1:] == idx[:, :-1]).any())


def test_the_order_case_shows_the_order():
    (vals, idx), seg, y = SO.case("order")
    terms = vals[:, 0].astype(np.float64) * y[:, 0].astype(np.float64)
    st = SO.update((vals, idx), 8, seg, y, (0, 0))
    forward, backward = np.cumsum(terms)[-1], np.cumsum(terms[::-1])[-1]  # (cumsum adds one after the other)
    assert st["acc"][3, 0, 0] == forward and st["cnt"][3, 0] == terms.size
    assert forward != backward
    span = np.log2(np.abs(terms[terms != 0]))
    assert span.min() < -30 and span.max() > 30


@pytest.mark.parametrize("name", list(SO.CASES))
def test_counts_at_lag_zero_are_the_run_statistics(inputs, name):
    """Without non-contiguous segments the triggers of the onset rule are the runs of section 16, and all triggers its
    active frames."""
    code, seg, _ = inputs[name]
    rows, _, hidden, _, _, _ = SO.CASES[name]
    seg = SO.whole_utterances(seg)
    n_seg = int(seg.max()) + 1
    runs = RO.update(code, hidden, seg, n_seg)
    zeros = np.zeros((rows, 1), np.float32)
    onset = SO.update(code, hidden, seg, zeros, (0, 0), trigger=SO.ONSET, weight=SO.ONE)
    every = SO.update(code, hidden, seg, zeros, (0, 0), trigger=SO.ALL, weight=SO.ONE)
    assert np.array_equal(onset["cnt"][:, 0], runs["runs"]) and np.array_equal(every["cnt"][:, 0], runs["frames"])
    assert np.array_equal(every["wsum"][:, 0], runs["frames"].astype(np.float64)) and runs["runs"].sum() > 0


# ---- argument errors: made-up (aligned, never dereferenced) pointers, every case fails its checks first -----------------
def _sta(N, k=32, hidden=64, n_rows=16, y_dtype=0, channels=8, ldy=8, lag_lo=-2, lag_hi=2, f_lo=0, f_cols=64, trigger=0,
         weight=0, ws=4096, ws_bytes=1 << 20, vals=4096, idx=4096, seg=4096, y=4096, acc=4096, wsum=4096, cnt=4096):
    return N.lib().wsae_sta_update(vals, idx, k, hidden, seg, n_rows, y, y_dtype, channels, ldy, lag_lo, lag_hi, f_lo, f_cols,
                                   trigger, weight, acc, wsum, cnt, ws, ws_bytes, None)


def workspace_bytes(n_rows, k, f_cols):
    """The layout the header describes: two lists of n_rows k entries, the [chunks, f_cols] table (at most 1024 chunks of
    at least 64 rows), three vectors of f_cols; every part rounded up to 256 bytes."""
    up = lambda b: (b + 255) // 256 * 256  # noqa: E731
    chunk = max(64, -(-n_rows // 1024))
    chunks = max(1, -(-n_rows // chunk))
    return 2 * up(4 * n_rows * k) + up(4 * chunks * f_cols) + 2 * up(4 * f_cols) + up(8 * f_cols)


STA_ERRORS = {"k0": dict(k=0), "k129": dict(k=129), "hidden0": dict(hidden=0), "n_rows_2p31": dict(n_rows=2 ** 31),
              "n_rows_negative": dict(n_rows=-1), "y_dtype": dict(y_dtype=2), "channels0": dict(channels=0),
              "channels4097": dict(channels=4097, ldy=4097), "ldy_short": dict(ldy=7), "lags_reversed": dict(lag_lo=3, lag_hi=2),
              "lag_lo_far": dict(lag_lo=-1025, lag_hi=-1000), "lag_hi_far": dict(lag_lo=1000, lag_hi=1025),
              "lags65": dict(lag_lo=-32, lag_hi=32), "window_past_end": dict(f_lo=40, f_cols=25),
              "window_negative": dict(f_lo=-1), "window_empty": dict(f_cols=0), "trigger2": dict(trigger=2),
              "trigger_negative": dict(trigger=-1), "weight2": dict(weight=2), "null_vals": dict(vals=None),
              "null_idx": dict(idx=None), "null_y": dict(y=None), "null_acc": dict(acc=None), "null_wsum": dict(wsum=None),
              "null_cnt": dict(cnt=None), "workspace_short": dict(ws_bytes=workspace_bytes(16, 32, 64) - 1),
              "workspace_null": dict(ws=None), "workspace_misaligned": dict(ws=4100)}


@pytest.mark.parametrize("kw", list(STA_ERRORS.values()), ids=list(STA_ERRORS))
def test_sta_argument_errors_do_not_need_a_gpu(kw):
    from whisper_sae import _native as N
    assert _sta(N, **kw) == -1
    assert "wsae_sta_update" in N.last_error()


def test_an_empty_call_is_accepted_without_a_gpu():
    from whisper_sae import _native as N
    assert _sta(N, n_rows=0) == 0 and _sta(N, n_rows=0, ws=None, seg=None) == 0
    assert _sta(N, n_rows=0, lag_lo=-32, lag_hi=31, channels=4096, ldy=5000, y_dtype=1, trigger=1, weight=1) == 0


def test_workspace_queries():
    from whisper_sae import _native as N
    wq = N.lib().wsae_sta_workspace_bytes
    for n_rows, k, hidden, f_lo, f_cols in ((3_072_000, 32, 3072, 0, 3072), (0, 1, 1, 0, 1), (16, 128, 40960, 40000, 960),
                                            (1000, 32, 3072, 0, 3072), (2 ** 31 - 1, 128, 40960, 0, 4096), (65, 3, 5, 1, 3)):
        assert wq(n_rows, k, hidden, f_lo, f_cols) == workspace_bytes(n_rows, k, f_cols), (n_rows, k, f_cols)
    assert wq(16, 0, 64, 0, 64) == -1 and wq(16, 129, 64, 0, 64) == -1 and wq(2 ** 31, 32, 64, 0, 64) == -1
    assert wq(-1, 32, 64, 0, 64) == -1 and wq(16, 32, 64, 60, 5) == -1 and wq(16, 32, 64, -1, 5) == -1
    assert wq(16, 32, 0, 0, 64) == -1 and wq(16, 32, 64, 0, 0) == -1


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
    defines = dict(re.findall(r"#define (WSAE_STA_[A-Z_]+) (\d+)", text))
    assert {k: int(v) for k, v in defines.items()} == {
        "WSAE_STA_TRIGGER_ALL": N.STA_TRIGGER_ALL, "WSAE_STA_TRIGGER_ONSET": N.STA_TRIGGER_ONSET,
        "WSAE_STA_WEIGHT_VALUE": N.STA_WEIGHT_VALUE, "WSAE_STA_WEIGHT_ONE": N.STA_WEIGHT_ONE, "WSAE_STA_MAX_K": N.STA_MAX_K,
        "WSAE_STA_MAX_LAGS": N.STA_MAX_LAGS, "WSAE_STA_MAX_CH": N.STA_MAX_CH}
    assert (N.STA_TRIGGER_ALL, N.STA_TRIGGER_ONSET, N.STA_WEIGHT_VALUE, N.STA_WEIGHT_ONE) == (SO.ALL, SO.ONSET, SO.VALUE, SO.ONE)
    assert (N.STA_MAX_K, N.STA_MAX_LAGS, N.STA_MAX_CH) == (128, 64, 4096)
    for name in ("TriggeredAverageTracker", "collect_triggered_averages", "mel_frames", "as_spectrogram",
                 "top_template_features"):
        assert name in A.__all__ and hasattr(A, name)
    assert len(set(A.__all__)) == len(A.__all__) and all(hasattr(A, name) for name in A.__all__)


def test_python_layer_argument_errors():
    import torch

    from whisper_sae import _native as N
    from whisper_sae.analysis import TriggeredAverageTracker as T, collect_triggered_averages, top_template_features
    from whisper_sae.sae.model import ReLUSAE
    code = (torch.ones(2, 3, 2), torch.zeros(2, 3, 2, dtype=torch.int32))
    with pytest.raises(N.WsaeError):
        T(8, 4).update(code, torch.zeros(2, 3, 4))  # CPU tensors
    with pytest.raises(N.WsaeError):
        T(8, 4, device="cpu").averages()
    for bad in (dict(hidden=0), dict(channels=0), dict(channels=4097), dict(lags=(2, 1)), dict(lags=(-32, 32)),
                dict(lags=(-1025, -1000)), dict(lags=(1000, 1025)), dict(trigger="offset"), dict(weight="two"),
                dict(f_window=(4, 5)), dict(f_window=(-1, 2)), dict(f_window=(0, 0))):
        kw = dict(hidden=8, channels=4)
        kw.update(bad)
        with pytest.raises(ValueError):
            T(kw.pop("hidden"), kw.pop("channels"), **kw)
    t = T(8, 4, lags=(3, 5), trigger="onset", weight="one", f_window=(2, 3))
    assert (t.n_lags, t.f_lo, t.f_cols) == (3, 2, 3)
    with pytest.raises(TypeError):
        T(8, 4).update(torch.ones(2, 3, 2), torch.zeros(2, 3, 4))
    with pytest.raises(ValueError):
        T(8, 4).merge(T(8, 4, lags=(-8, 7)))
    with pytest.raises(ValueError):
        T(8, 4).merge(T(8, 4, trigger="onset"))
    with pytest.raises(TypeError):
        collect_triggered_averages(ReLUSAE(16, 32), [(torch.zeros(2, 4, 16), torch.zeros(2, 4, 3))])
    with pytest.raises(ValueError):
        top_template_features(torch.zeros(2, 1, 1), by="loudness", counts=torch.ones(2, 1))
    with pytest.raises(ValueError):
        top_template_features(torch.zeros(2, 1, 1))  # a tensor without counts


def test_mel_frames_and_back():
    import torch

    from whisper_sae.analysis import as_spectrogram, mel_frames
    mel = torch.arange(2 * 5 * 12, dtype=torch.float32).reshape(2, 5, 12)
    fr = mel_frames(mel)
    assert fr.shape == (2, 6, 10)
    for t in range(6):  # encoder position t sees the mel columns 2 t and 2 t + 1, sub-frame major
        assert torch.equal(fr[:, t, :5], mel[:, :, 2 * t]) and torch.equal(fr[:, t, 5:], mel[:, :, 2 * t + 1])
    assert torch.equal(as_spectrogram(fr, 5), mel)
    three = mel_frames(mel, stride=3)
    assert three.shape == (2, 4, 15) and torch.equal(three[1, 2, 10:], mel[1, :, 8])
    assert torch.equal(as_spectrogram(three, 5, stride=3), mel)
    one = mel_frames(mel, stride=1)
    assert torch.equal(one, mel.transpose(1, 2)) and torch.equal(as_spectrogram(one, 5, stride=1), mel)
    # a template [F, L, C] of a tracker: lags become pairs of columns; a window of frames maps back onto its mel patch
    tmpl = fr[:, 1:4].reshape(1, 2, 3, 10)
    assert as_spectrogram(tmpl, 5).shape == (1, 2, 5, 6) and torch.equal(as_spectrogram(tmpl, 5)[0], mel[:, :, 2:8])
    for bad in (lambda: mel_frames(mel, stride=5), lambda: mel_frames(mel[0]), lambda: mel_frames(mel, stride=0),
                lambda: as_spectrogram(fr, 4), lambda: as_spectrogram(fr[0, 0], 5)):
        with pytest.raises(ValueError):
            bad()


def test_averages_contrast_and_ranking_on_hand_made_state():
    import torch

    from whisper_sae.analysis import top_template_features
    from whisper_sae.analysis.triggered import signal_baseline, template_contrast, triggered_average
    # 4 features, 2 lags, 2 channels; the signal: channel 0 has mean 1 and std 2, channel 1 is constant 3
    sums = torch.tensor([[[6.0, 6.0], [10.0, 6.0]], [[0.0, 0.0], [0.0, 0.0]], [[-3.0, 3.0], [0.0, 0.0]],
                         [[50.0, 150.0], [50.0, 150.0]]], dtype=torch.float64)
    weights = torch.tensor([[2.0, 2.0], [0.0, 0.0], [1.0, 0.0], [50.0, 50.0]], dtype=torch.float64)
    counts = torch.tensor([[2, 2], [0, 0], [1, 0], [50, 50]])
    avg = triggered_average(sums, weights)
    assert avg.dtype == torch.float64 and avg[0].tolist() == [[3.0, 3.0], [5.0, 3.0]] and avg[3].tolist() == [[1.0, 3.0]] * 2
    assert bool(torch.isnan(avg[1]).all()) and avg[2, 0].tolist() == [-3.0, 3.0] and bool(torch.isnan(avg[2, 1]).all())
    mean, std = signal_baseline(torch.tensor([10.0, 30.0]), torch.tensor([50.0, 90.0]), torch.tensor([10]))
    assert mean.tolist() == [1.0, 3.0] and std.tolist() == [2.0, 0.0]
    z = template_contrast(avg, mean, std)
    assert z[0, :, 0].tolist() == [1.0, 2.0] and z[2, 0, 0].item() == -2.0 and z[3, :, 0].tolist() == [0.0, 0.0]
    assert bool(torch.isnan(z[..., 1]).all())  # a constant channel has no contrast
    nothing = signal_baseline(torch.zeros(2), torch.zeros(2), torch.zeros(1, dtype=torch.int64))
    assert bool(torch.isnan(nothing[0]).all())
    # ranking: feature 1 has no cell, ties go to the lower index, min_count filters
    top, score = top_template_features(z, by="contrast_peak", n=10, counts=counts)
    assert top.tolist() == [0, 2, 3] and score.tolist() == [2.0, 2.0, 0.0]
    top, score = top_template_features(z, by="contrast_energy", n=10, counts=counts)
    assert top.tolist() == [2, 0, 3] and score.tolist() == [4.0, 2.5, 0.0]
    top, _ = top_template_features(z, by="contrast_peak", n=10, min_count=2, counts=counts)
    assert top.tolist() == [0, 3]
    top, _ = top_template_features(z, by="contrast_peak", n=1, counts=counts)
    assert top.tolist() == [0]
