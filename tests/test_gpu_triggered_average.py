"""Feature-triggered averages on the MI355X: ``acc``, ``wsum`` and ``cnt`` of ``wsae_sta_update`` bit for bit against
the numpy oracle of tests/sta_oracle.py on every shape, mode and signal type, the properties that make the state
independent of batching, windows and ``ldy``, and the Python layer on real modules.  The inputs and the conditions that
keep them from being degenerate are checked on the CPU in tests/test_triggered_average.py.  Every signal handed to the
kernel carries NaN in the columns behind ``channels`` and in its padding rows: neither may reach the state."""

from __future__ import annotations

import tempfile

import numpy as np
import pytest
import torch

import sta_oracle as SO
from whisper_sae import _native as N
from whisper_sae.analysis import (RunTracker, TriggeredAverageTracker, as_spectrogram, collect_runs,
                                  collect_triggered_averages, top_template_features)
from whisper_sae.sae.model import BatchTopKSAE, TopKSAE

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
JUNK = 123.25
PAD = 3  # columns behind the channels


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class StaState:
    """Device state of the C ABI.  Every array has two more features than the window, filled with junk that must
    survive."""

    def __init__(self, hidden, channels, lags, f_lo=0, f_cols=None, trigger=SO.ALL, weight=SO.VALUE):
        self.hidden, self.C, self.lags, self.f_lo = hidden, channels, lags, f_lo
        self.f_cols = hidden - f_lo if f_cols is None else f_cols
        self.trigger, self.weight = trigger, weight
        F, L = self.f_cols, lags[1] - lags[0] + 1
        self.acc = torch.zeros(F + 2, L, channels, dtype=torch.float64, device=DEV)
        self.wsum = torch.zeros(F + 2, L, dtype=torch.float64, device=DEV)
        self.cnt = torch.zeros(F + 2, L, dtype=torch.int64, device=DEV)
        self.acc[F:], self.wsum[F:], self.cnt[F:] = JUNK, JUNK, 77

    def update(self, code, seg, y, bf16=False, poison=True):
        """``y`` float32 numpy [rows, C].  With ``poison`` the kernel's copy has ``ldy = C + 3`` with NaN behind the
        channels, and NaN in the rows that are padding."""
        v, i = dev(code[0]), dev(code[1])
        rows, k = v.shape
        s = None if seg is None else dev(np.asarray(seg, np.int32))
        wide = np.full((rows, self.C + PAD), np.nan, np.float32) if poison else np.empty((rows, self.C), np.float32)
        wide[:, :self.C] = y[:, :self.C]
        if poison and seg is not None:
            wide[np.asarray(seg) < 0] = np.nan
        yd = dev(wide).to(torch.bfloat16) if bf16 else dev(wide)
        lib = N.lib()
        need = lib.wsae_sta_workspace_bytes(rows, k, self.hidden, self.f_lo, self.f_cols)
        assert need > 0
        ws = torch.full((need,), 0xAB, dtype=torch.uint8, device=DEV)  # (arbitrary contents on entry)
        N.check(lib.wsae_sta_update(v.data_ptr(), i.data_ptr(), k, self.hidden, N.ptr(s), rows, yd.data_ptr(),
                                    N.DT_BF16 if bf16 else N.DT_F32, self.C, wide.shape[1], self.lags[0], self.lags[1],
                                    self.f_lo, self.f_cols, self.trigger, self.weight, self.acc.data_ptr(),
                                    self.wsum.data_ptr(), self.cnt.data_ptr(), ws.data_ptr(), need,
                                    torch.cuda.current_stream().cuda_stream), "wsae_sta_update")
        torch.cuda.synchronize()
        return self

    def state(self):
        """The fields as numpy arrays (the junk behind the window checked on the way)."""
        F = self.f_cols
        assert bool((self.acc[F:] == JUNK).all()) and bool((self.wsum[F:] == JUNK).all()) and bool((self.cnt[F:] == 77).all())
        return {"acc": self.acc[:F].cpu().numpy(), "wsum": self.wsum[:F].cpu().numpy(), "cnt": self.cnt[:F].cpu().numpy()}


def same_state(got, want):
    for f in SO.FIELDS:
        assert got[f].shape == want[f].shape and got[f].dtype == want[f].dtype, f
        diff = np.argwhere(np.ascontiguousarray(got[f]).view(np.int64) != np.ascontiguousarray(want[f]).view(np.int64))
        assert diff.size == 0, (f, diff[:5], got[f][tuple(diff[0])], want[f][tuple(diff[0])])


_inputs, _wants = {}, {}


def inputs(name):
    if name not in _inputs:
        _inputs[name] = SO.case(name)
    return _inputs[name]


def oracle(name, trigger=SO.ALL, weight=SO.VALUE):
    """Computed once per (input, mode) and shared; never modified."""
    key = (name, trigger, weight)
    if key not in _wants:
        code, seg, y = inputs(name)
        _, _, hidden, _, lags, _ = SO.CASES[name]
        _wants[key] = SO.update(code, hidden, seg, y, lags, trigger=trigger, weight=weight)
    return _wants[key]


@pytest.mark.parametrize("name", list(SO.CASES))
def test_sums_equal_the_oracle(name):
    code, seg, y = inputs(name)
    _, _, hidden, C, lags, _ = SO.CASES[name]
    want = oracle(name)
    got = StaState(hidden, C, lags).update(code, seg, y).state()
    assert not np.isnan(got["acc"]).any()
    same_state(got, want)
    if name == "flagship":  # the planted features: on every row, and on every other row
        assert got["cnt"][SO.PLANTED[0], 8] == 1500 and got["cnt"][SO.PLANTED[1], 8] == 750
        assert got["cnt"][SO.PLANTED[0], 0] == 1492 and got["cnt"][SO.PLANTED[1], 16] == 746
    if name == "wide":
        for a, b in SO.TWINS:  # twins on either side of a tile boundary
            assert got["cnt"][a].min() > 3
            assert all(SO.same_bits(got[f][a], got[f][b]) for f in SO.FIELDS), (a, b)
        lo, span = SO.WINDOW  # a window that starts and ends inside tiles equals the slice, twins included
        win = StaState(hidden, C, lags, f_lo=lo, f_cols=span).update(code, seg, y).state()
        same_state(win, {f: want[f][lo:lo + span] for f in SO.FIELDS})
    if name == "one":  # seg = NULL is one segment
        none = StaState(hidden, C, lags).update(code, None, y).state()
        same_state(none, want)


@pytest.mark.parametrize("mode", SO.MODES[1:], ids=lambda m: f"trigger{m[0]}_weight{m[1]}")
@pytest.mark.parametrize("name", ["small", "two_pass", "lags64"])
def test_trigger_and_weight_modes(name, mode):
    code, seg, y = inputs(name)
    _, _, hidden, C, lags, _ = SO.CASES[name]
    want = oracle(name, *mode)
    plain = oracle(name)
    assert 0 < want["cnt"].sum() and (mode[0] == SO.ALL or want["cnt"].sum() < plain["cnt"].sum())
    same_state(StaState(hidden, C, lags, trigger=mode[0], weight=mode[1]).update(code, seg, y).state(), want)


@pytest.mark.parametrize("name", ["small", "flagship"])
def test_bf16_signal_equals_fp32_holding_the_same_values(name):
    code, seg, y = inputs(name)
    _, _, hidden, C, lags, _ = SO.CASES[name]
    yb = SO.to_bf16_values(y)
    assert not np.array_equal(yb, y)
    want = SO.update(code, hidden, seg, yb, lags)
    same_state(StaState(hidden, C, lags).update(code, seg, yb, bf16=True).state(), want)
    same_state(StaState(hidden, C, lags).update(code, seg, yb).state(), want)


def test_ldy_and_poison_do_not_matter():
    code, seg, y = inputs("small")
    _, _, hidden, C, lags, _ = SO.CASES["small"]
    same_state(StaState(hidden, C, lags).update(code, seg, y, poison=False).state(), oracle("small"))


@pytest.mark.parametrize("name", ["small", "wide"])
def test_grouping_of_whole_utterances_does_not_matter(name):
    code, seg, y = inputs(name)
    _, _, hidden, C, lags, _ = SO.CASES[name]
    seg = SO.whole_utterances(seg)
    n_seg = int(seg.max()) + 1
    want = SO.update(code, hidden, seg, y, lags)

    def run(groups):
        st = StaState(hidden, C, lags)
        for lo, hi in groups:  # utterances lo .. hi - 1 per call, in their order
            rows = np.nonzero((seg >= lo) & (seg < hi))[0]
            if rows.size == 0:
                continue
            a, b = rows[0], rows[-1] + 1  # (the padding rows between them travel along)
            st.update((code[0][a:b], code[1][a:b]), seg[a:b], y[a:b])
        return st.state()

    five = [(n_seg * j // 5, n_seg * (j + 1) // 5) for j in range(5)]
    half = n_seg // 2
    for groups in ([(0, n_seg)], [(0, half), (half, n_seg)], five, [(s, s + 1) for s in range(n_seg)]):
        same_state(run(groups), want)


def test_two_runs_give_the_same_bits():
    code, seg, y = inputs("flagship")
    _, _, hidden, C, lags, _ = SO.CASES["flagship"]
    a = StaState(hidden, C, lags, trigger=SO.ONSET).update(code, seg, y).state()
    b = StaState(hidden, C, lags, trigger=SO.ONSET).update(code, seg, y).state()
    same_state(a, b)
    same_state(a, oracle("flagship", SO.ONSET, SO.VALUE))


# ---- the Python layer --------------------------------------------------------------------------------------------------
D, H, K, UTT, T, C = 64, 256, 8, 12, 40, 6
LAGS = (-3, 3)


def utterances(seed):
    """12 utterances of 40 frames in three batches, with a signal and a frame mask.  A frame repeats for a stretch of
    about three frames at a slightly varying loudness, so the features persist; the tail of every utterance and one
    frame inside one of them are masked."""
    gen = torch.Generator().manual_seed(seed)
    proto = torch.randn(UTT, 14, D, generator=gen)
    hold = (torch.rand(UTT, T, generator=gen) < 0.3).cumsum(1) % 14
    x = torch.gather(proto, 1, hold[:, :, None].expand(UTT, T, D)) * (0.9 + 0.2 * torch.rand(UTT, T, 1, generator=gen))
    signal = torch.randn(UTT, T, C, generator=gen)
    mask = torch.ones(UTT, T)
    for u in range(UTT):
        mask[u, 24 + (u % 5) * 3:] = 0
    mask[3, 10] = 0
    cuts = ((0, 5), (5, 6), (6, UTT))
    return [(x[a:b], signal[a:b], mask[a:b]) for a, b in cuts], signal, mask


def make_sae(cls, seed, **kw):
    torch.manual_seed(seed)
    return cls(D, H, k=K, **kw).to(DEV)


def tracker_state(t):
    return {"acc": t.sums.cpu().numpy(), "wsum": t.weights.cpu().numpy(), "cnt": t.counts.cpu().numpy()}


@pytest.mark.parametrize("kind", ["topk", "batch_topk"])
def test_python_layer_on_real_modules(kind):
    sae = make_sae(TopKSAE, 1) if kind == "topk" else make_sae(BatchTopKSAE, 2, max_k_per_row=16)
    batches, signal, mask = utterances(5)
    sae.train()
    tracker = collect_triggered_averages(sae, batches, lags=LAGS)
    assert sae.training and (tracker.hidden, tracker.channels, tracker.n_lags) == (H, C, 7)
    # the oracle on the codes the module emits
    sae.eval()
    codes = [sae.encode_compact(x.to(DEV)) for x, _, _ in batches]
    vals, idx = (np.concatenate([c[i].reshape(-1, c[i].shape[-1]).cpu().numpy() for c in codes]) for i in (0, 1))
    seg = np.where(mask.reshape(-1).numpy() != 0, np.repeat(np.arange(UTT), T), -1).astype(np.int32)
    y = signal.reshape(-1, C).numpy()
    want = SO.update((vals, idx), H, seg, y, LAGS)
    assert want["cnt"].sum() > 0 and (want["cnt"][:, 0] < want["cnt"][:, 3]).any()
    same_state(tracker_state(tracker), want)
    live = seg >= 0
    assert int(tracker.total_rows.item()) == live.sum() == mask.sum()
    np.testing.assert_allclose(tracker.sig_sum.cpu().numpy(), y[live].astype(np.float64).sum(0), rtol=1e-12)
    np.testing.assert_allclose(tracker.sig_sq.cpu().numpy(), (y[live].astype(np.float64) ** 2).sum(0), rtol=1e-12)
    with np.errstate(divide="ignore", invalid="ignore"):
        avg = np.where(want["wsum"][..., None] != 0, want["acc"] / want["wsum"][..., None], np.nan)
    np.testing.assert_array_equal(tracker.averages().cpu().numpy(), avg)
    mean, std = tracker.baseline()
    np.testing.assert_allclose(mean.cpu().numpy(), y[live].astype(np.float64).mean(0), rtol=1e-12)
    np.testing.assert_allclose(std.cpu().numpy(), y[live].astype(np.float64).std(0), rtol=1e-10)
    z = tracker.contrast()
    np.testing.assert_allclose(z.cpu().numpy(), (avg - mean.cpu().numpy()) / std.cpu().numpy(), rtol=1e-12, equal_nan=True)
    for by in ("contrast_peak", "contrast_energy"):
        top, score = top_template_features(tracker, by=by, n=5, min_count=3)
        assert top.numel() == 5 and bool((tracker.counts[top].amax(1) >= 3).all()) and bool((score[:-1] >= score[1:]).all())
    assert as_spectrogram(tracker.averages()[top], C // 2).shape == (5, C // 2, 14)
    # the flat form through a window; a bf16 signal; CPU tensors
    flat = TriggeredAverageTracker(H, C, lags=LAGS, f_window=(64, 100), device=DEV)
    flat.update((dev(vals), dev(idx)), dev(y), segments=dev(seg))
    same_state(tracker_state(flat), {f: want[f][64:164] for f in SO.FIELDS})
    assert torch.equal(flat.total_rows, tracker.total_rows)
    with pytest.raises(ValueError):
        flat.update((dev(vals).reshape(UTT, T, -1), dev(idx).reshape(UTT, T, -1)), dev(y).reshape(UTT, T, C))
    with pytest.raises(N.WsaeError):
        flat.update((torch.from_numpy(vals), torch.from_numpy(idx)), torch.from_numpy(y), segments=torch.from_numpy(seg))
    half = TriggeredAverageTracker(H, C, lags=LAGS, device=DEV)
    yb = dev(y).to(torch.bfloat16)  # (rounded, not cut: the oracle gets what bfloat16 holds)
    half.update((dev(vals), dev(idx)), yb, segments=dev(seg))
    same_state(tracker_state(half), SO.update((vals, idx), H, seg, yb.float().cpu().numpy(), LAGS))
    # the cross-check against the run statistics on the same code: onsets are runs, triggers are active frames
    runs = collect_runs(sae, [(x, m) for x, _, m in batches])
    onset = collect_triggered_averages(sae, batches, lags=LAGS, trigger="onset", weight="one")
    assert torch.equal(onset.counts[:, 3], runs.runs.long()) and torch.equal(tracker.counts[:, 3], runs.frames.long())
    assert torch.equal(onset.weights[:, 3], runs.runs.double()) and isinstance(runs, RunTracker)
    # two shards merged equal the whole up to the one add per cell that joins them; save / load; a loaded tracker goes on
    a = collect_triggered_averages(sae, batches[:1], lags=LAGS)
    b = collect_triggered_averages(sae, batches[1:], lags=LAGS)
    a.merge(b)
    assert torch.equal(a.counts, tracker.counts) and torch.equal(a.total_rows, tracker.total_rows)
    np.testing.assert_allclose(a.sums.cpu().numpy(), want["acc"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(a.weights.cpu().numpy(), want["wsum"], rtol=1e-13)
    with tempfile.TemporaryDirectory(prefix="wsae_sta_") as d:
        tracker.save(f"{d}/t.pt")
        back = TriggeredAverageTracker.load(f"{d}/t.pt", device=DEV)
    same_state(tracker_state(back), want)
    assert torch.equal(back.sig_sq, tracker.sig_sq) and (back.trigger, back.weight, back.lag_lo, back.lag_hi) == ("all", "value", -3, 3)
    x0, s0, m0 = batches[1]
    c0 = sae.encode_compact(x0.to(DEV))
    back.update((c0[0].reshape(1, T, -1), c0[1].reshape(1, T, -1)), s0.to(DEV), frame_mask=m0.to(DEV))
    again = SO.update((vals[5 * T:6 * T], idx[5 * T:6 * T]), H, seg[5 * T:6 * T], y[5 * T:6 * T], LAGS, state=want)
    same_state(tracker_state(back), again)
    assert int(back.total_rows.item()) == int(mask.sum() + m0.sum())
