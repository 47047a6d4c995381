"""Temporal run statistics on the MI355X: every integer output of ``wsae_runs_update`` bit for bit against the numpy
oracle of tests/runs_oracle.py, the events after the canonical sort bit for bit too (the fp32 ``total`` included), the
properties that make the state independent of batching, and the Python layer on real modules.  The inputs and the
conditions that keep them from being degenerate are checked on the CPU in tests/test_temporal.py."""

from __future__ import annotations

import tempfile

import numpy as np
import pytest
import torch

import runs_oracle as RO
from whisper_sae import _native as N
from whisper_sae.analysis import FeatureEvents, RunTracker, collect_runs, top_temporal_features
from whisper_sae.sae.model import BatchTopKSAE, TopKSAE

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
JUNK = 0x5a5a5a5
SHARED = ("frames", "runs", "dur_max", "dur_sq", "dur_hist", "total_rows")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype.itemsize == 4 else np.int64)


class RunsState:
    """Device state of the C ABI.  Every per-feature array has three more rows than the window, filled with junk that
    must survive; so have the event buffers behind their capacity.  ``ev_cap=None``: no events (no cursor)."""

    def __init__(self, hidden, f_lo=0, f_cols=None, gaps=True, ev_cap=None, ev_min_len=1):
        self.hidden, self.f_lo = hidden, f_lo
        self.f_cols = hidden - f_lo if f_cols is None else f_cols
        self.ev_cap, self.ev_min_len = ev_cap, ev_min_len
        F = self.f_cols

        def state(*tail, dtype=torch.int32):
            t = torch.zeros(F + 3, *tail, dtype=dtype, device=DEV)
            t[F:] = JUNK
            return t

        self.t = {"frames": state(), "runs": state(), "dur_max": state(), "dur_sq": state(dtype=torch.int64),
                  "dur_hist": state(RO.BINS), "gap_hist": state(RO.BINS) if gaps else None,
                  "total_rows": torch.zeros(1, dtype=torch.int64, device=DEV)}
        self.ev_int = self.ev_flt = self.ev_count = None
        if ev_cap is not None:
            self.ev_int = torch.full((ev_cap + 2, 4), JUNK, dtype=torch.int32, device=DEV)
            self.ev_flt = torch.full((ev_cap + 2, 2), 123.25, dtype=torch.float32, device=DEV)
            self.ev_count = torch.zeros(1, dtype=torch.int64, device=DEV)

    def update(self, code, seg, n_seg, seg_base=0):
        v, i, s = dev(code[0]), dev(code[1]), dev(np.asarray(seg, np.int32))
        lib = N.lib()
        need = lib.wsae_runs_workspace_bytes(v.shape[0], v.shape[1], self.hidden, n_seg, self.f_lo, self.f_cols)
        assert need == 8 * n_seg
        ws = torch.full((need,), 0xAB, dtype=torch.uint8, device=DEV)  # (arbitrary contents on entry)
        t = self.t
        N.check(lib.wsae_runs_update(v.data_ptr(), i.data_ptr(), v.shape[1], self.hidden, s.data_ptr(), v.shape[0], n_seg,
                                     seg_base, self.f_lo, self.f_cols, t["frames"].data_ptr(), t["runs"].data_ptr(),
                                     t["dur_max"].data_ptr(), t["dur_sq"].data_ptr(), t["dur_hist"].data_ptr(),
                                     N.ptr(t["gap_hist"]), t["total_rows"].data_ptr(), N.ptr(self.ev_int), N.ptr(self.ev_flt),
                                     self.ev_cap or 0, self.ev_min_len, N.ptr(self.ev_count), ws.data_ptr(), need,
                                     torch.cuda.current_stream().cuda_stream), "wsae_runs_update")
        torch.cuda.synchronize()
        return self

    def ints(self):
        """The integer fields as numpy arrays (the junk behind the window checked on the way)."""
        out = {}
        for name, t in self.t.items():
            if t is None:
                continue
            if name != "total_rows":
                assert bool((t[self.f_cols:] == JUNK).all()), name
                t = t[:self.f_cols]
            out[name] = t.cpu().numpy()
        return out

    def events(self):
        """(the cursor, the stored records in the canonical order as a dict of numpy arrays)."""
        n = int(self.ev_count.item())
        kept = min(n, self.ev_cap)
        assert bool((self.ev_int[self.ev_cap:] == JUNK).all()) and bool((self.ev_flt[self.ev_cap:] == 123.25).all())
        ei, ef = self.ev_int[:kept].cpu().numpy(), self.ev_flt[:kept].cpu().numpy()
        order = np.lexsort((ei[:, 2], ei[:, 1], ei[:, 0]))
        ei, ef = ei[order], ef[order]
        return n, {"feature": ei[:, 0], "segment": ei[:, 1], "start": ei[:, 2], "length": ei[:, 3], "total": ef[:, 0],
                   "peak": ef[:, 1]}


def same_ints(got, want, fields=RO.INT_FIELDS):
    for f in fields:
        assert got[f].dtype == want[f].dtype and np.array_equal(got[f], want[f]), (f, np.argwhere(got[f] != want[f])[:5])


def same_events(got, want):
    for f in RO.EVENT_FIELDS:
        assert got[f].shape == want[f].shape, (f, got[f].shape, want[f].shape)
        assert np.array_equal(bits(got[f]), bits(want[f])), (f, np.argwhere(bits(got[f]) != bits(want[f]))[:5])


@pytest.fixture(scope="module")
def cases():
    out = {}
    for shape in RO.SHAPES:
        code, seg = RO.case(shape)
        out[shape] = (code, seg, RO.update(code, shape[2], seg, shape[3]))
    return out


@pytest.mark.parametrize("shape", RO.SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_runs_equal_the_oracle(cases, shape):
    code, seg, want = cases[shape]
    _, _, hidden, n_seg = shape
    n_ev = want["events"]["feature"].size
    assert n_ev == want["runs"].sum() > 0
    with_ev = RunsState(hidden, ev_cap=n_ev + 5).update(code, seg, n_seg)
    same_ints(with_ev.ints(), want)
    count, events = with_ev.events()
    assert count == n_ev
    same_events(events, want["events"])
    plain = RunsState(hidden).update(code, seg, n_seg)  # the kernel without events has another tile width
    same_ints(plain.ints(), want)
    if hidden == RO.WIDE:
        got = plain.ints()
        for a, b in RO.TWINS:  # twins on either side of a tile boundary
            assert got["runs"][a] > 3
            for f in RO.INT_FIELDS[:-1]:
                assert np.array_equal(got[f][a], got[f][b]), (f, a, b)
            ea, eb = events["feature"] == a, events["feature"] == b
            for f in RO.EVENT_FIELDS[1:]:
                assert np.array_equal(bits(events[f][ea]), bits(events[f][eb])), (f, a, b)
        lo, span = RO.WINDOW  # a window that starts and ends inside tiles equals the slice
        in_window = (want["events"]["feature"] >= lo) & (want["events"]["feature"] < lo + span)
        for ev_cap in (None, int(in_window.sum())):
            win = RunsState(hidden, f_lo=lo, f_cols=span, ev_cap=ev_cap).update(code, seg, n_seg)
            got_w = win.ints()
            for f in RO.INT_FIELDS[:-1]:
                assert np.array_equal(got_w[f], want[f][lo:lo + span]), f
            assert got_w["total_rows"][0] == want["total_rows"][0]
            if ev_cap is not None:
                count, ev_w = win.events()
                assert count == ev_cap
                same_events(ev_w, {f: want["events"][f][in_window] for f in RO.EVENT_FIELDS})


def whole_utterances(seg, n_seg):
    """Ids made non-decreasing (padding stays padding): an input of whole utterances that can be cut between them."""
    seg = np.where((seg >= 0) & (seg < n_seg), seg, -1)
    up = np.maximum.accumulate(seg)
    return np.where(seg >= 0, up, -1).astype(np.int32)


@pytest.mark.parametrize("shape", [RO.SHAPES[1], RO.SHAPES[3]], ids=lambda s: "x".join(str(v) for v in s))
def test_grouping_and_order_of_whole_utterances_do_not_matter(cases, shape):
    code, seg, _ = cases[shape]
    _, _, hidden, n_seg = shape
    seg = whole_utterances(seg, n_seg)
    want = RO.update(code, hidden, seg, n_seg)
    cap = want["events"]["feature"].size

    def run(groups):
        st = RunsState(hidden, ev_cap=cap)
        for lo, hi in groups:  # utterances lo .. hi - 1 per call under local ids
            last = np.nonzero((seg >= lo) & (seg < hi))[0]
            if last.size == 0:
                continue
            a, b = last[0], last[-1] + 1  # (the padding rows between them travel along)
            local = np.where(seg[a:b] >= 0, seg[a:b] - lo, -1)
            st.update((code[0][a:b], code[1][a:b]), local, hi - lo, seg_base=lo)
        return st

    five = [(n_seg * j // 5, n_seg * (j + 1) // 5) for j in range(5)]
    half = n_seg // 2
    results = [run(g) for g in ([(0, n_seg)], [(0, half), (half, n_seg)], five, five[::-1],
                                [(s, s + 1) for s in range(n_seg)][::-1])]
    for st in results:
        same_ints(st.ints(), want)
        count, events = st.events()
        assert count == cap
        same_events(events, want["events"])


def test_optional_outputs_leave_the_shared_fields_alone(cases):
    for shape in (RO.SHAPES[1], RO.SHAPES[4]):
        code, seg, want = cases[shape]
        hidden, n_seg = shape[2], shape[3]
        for gaps in (True, False):
            for ev_cap in (None, 0, 7, 100000):
                st = RunsState(hidden, gaps=gaps, ev_cap=ev_cap).update(code, seg, n_seg)
                got = st.ints()
                same_ints(got, want, SHARED + (("gap_hist",) if gaps else ()))
                if ev_cap is not None:  # the cursor counts whatever the capacity, even none at all
                    assert int(st.ev_count.item()) == want["runs"].sum()


def test_min_event_len_filters_exactly(cases):
    shape = RO.SHAPES[3]
    code, seg, want = cases[shape]
    hidden, n_seg = shape[2], shape[3]
    for min_len in (2, 33):
        keep = want["events"]["length"] >= min_len
        assert 0 < keep.sum() < keep.size
        st = RunsState(hidden, ev_cap=int(keep.sum()), ev_min_len=min_len).update(code, seg, n_seg)
        same_ints(st.ints(), want)
        count, events = st.events()
        assert count == keep.sum()
        same_events(events, {f: want["events"][f][keep] for f in RO.EVENT_FIELDS})
        same_events(events, RO.update(code, hidden, seg, n_seg, ev_min_len=min_len)["events"])


def test_a_full_event_list_keeps_counting(cases):
    shape = RO.SHAPES[1]
    code, seg, want = cases[shape]
    hidden, n_seg = shape[2], shape[3]
    n_ev = want["events"]["feature"].size
    st = RunsState(hidden, ev_cap=n_ev // 3).update(code, seg, n_seg)
    same_ints(st.ints(), want)
    count, events = st.events()
    assert count == n_ev and events["feature"].size == n_ev // 3
    # what was stored are records of the oracle's list, each once
    key = lambda e: set(zip(*(bits(e[f]).tolist() for f in RO.EVENT_FIELDS)))  # noqa: E731
    assert len(key(events)) == n_ev // 3 and key(events) <= key(want["events"])
    # the Python layer refuses to hand out a cut list, and names the capacity it needs
    tracker = RunTracker(hidden, max_events=n_ev // 3, device=DEV)
    tracker.update((dev(code[0]), dev(code[1])), segments=dev(np.where(seg < n_seg, seg, -1)))
    assert tracker.event_count == n_ev
    with pytest.raises(N.WsaeError, match=str(n_ev)):
        tracker.events()
    assert np.array_equal(tracker.runs.cpu().numpy(), want["runs"]) and np.array_equal(tracker.gap_hist.cpu().numpy(), want["gap_hist"])


# ---- the Python layer --------------------------------------------------------------------------------------------------
D, H, K, UTT, T = 64, 256, 8, 12, 40


def utterances(seed):
    """12 utterances of 40 frames in three batches, with a frame mask.  A frame repeats for a stretch of about three
    frames at a slightly varying loudness, so the features persist; the tail of every utterance and one frame inside one
    of them are masked."""
    gen = torch.Generator().manual_seed(seed)
    proto = torch.randn(UTT, 14, D, generator=gen)
    hold = (torch.rand(UTT, T, generator=gen) < 0.3).cumsum(1) % 14
    x = torch.gather(proto, 1, hold[:, :, None].expand(UTT, T, D)) * (0.9 + 0.2 * torch.rand(UTT, T, 1, generator=gen))
    mask = torch.ones(UTT, T)
    for u in range(UTT):
        mask[u, 24 + (u % 5) * 3:] = 0
    mask[3, 10] = 0
    return [(x[:5], mask[:5]), (x[5:6], mask[5:6]), (x[6:], mask[6:])], mask


def make_sae(cls, seed, **kw):
    torch.manual_seed(seed)
    return cls(D, H, k=K, **kw).to(DEV)


@pytest.mark.parametrize("kind", ["topk", "batch_topk"])
def test_python_layer_on_real_modules(kind):
    sae = make_sae(TopKSAE, 1) if kind == "topk" else make_sae(BatchTopKSAE, 2, max_k_per_row=16)
    batches, mask = utterances(5)
    sae.train()
    tracker = collect_runs(sae, batches, max_events=20000, min_event_len=2)
    assert sae.training and tracker._next == UTT
    # the oracle on the codes the module emits
    sae.eval()
    codes = [sae.encode_compact(x.to(DEV)) for x, _ in batches]
    vals, idx = (np.concatenate([c[i].reshape(-1, c[i].shape[-1]).cpu().numpy() for c in codes]) for i in (0, 1))
    seg = np.where(mask.reshape(-1).numpy() != 0, np.repeat(np.arange(UTT), T), -1)
    want = RO.update((vals, idx), H, seg, UTT, ev_min_len=2)
    assert want["dur_max"].max() >= 3 and want["gap_hist"].sum() > 0 and want["total_rows"][0] == mask.sum()
    got = {"frames": tracker.frames, "runs": tracker.runs, "dur_max": tracker.max_run, "dur_sq": tracker.sum_squares,
           "dur_hist": tracker.duration_hist, "gap_hist": tracker.gap_hist, "total_rows": tracker.total_rows}
    same_ints({f: t.cpu().numpy() for f, t in got.items()}, want)
    ev = tracker.events()
    assert isinstance(ev, FeatureEvents) and tracker.event_count == want["events"]["feature"].size > 0
    same_events({"feature": ev.feature.cpu().numpy(), "segment": ev.utterance.cpu().numpy(), "start": ev.start.cpu().numpy(),
                 "length": ev.length.cpu().numpy(), "total": ev.total.cpu().numpy(), "peak": ev.peak.cpu().numpy()},
                want["events"])
    f = int(want["events"]["feature"][0])
    one = tracker.events(feature=f)
    assert one.feature.numel() == (want["events"]["feature"] == f).sum() and bool((one.feature == f).all())
    lo, hi = ev.sample_bounds(320, context_frames=2)
    assert bool((hi - lo <= (ev.length.long() + 4) * 320).all()) and bool((lo >= 0).all())
    # the summary against the oracle's formulas, in frames and in milliseconds
    for frame_ms in (None, 20.0):
        summ, ref = tracker.summary(frame_ms), RO.summary(want, frame_ms)
        for name in summ._fields:
            np.testing.assert_allclose(getattr(summ, name).cpu().numpy(), ref[name], rtol=1e-14, atol=0, equal_nan=True,
                                       err_msg=name)
    summ = tracker.summary()
    q = tracker.duration_quantile(0.9).cpu().numpy()
    np.testing.assert_array_equal(q, RO.hist_quantile(want["dur_hist"], 0.9))
    top, val = top_temporal_features(summ, by="mean_duration", n=5, min_runs=3)
    assert top.numel() == 5 and bool((summ.runs[top] >= 3).all()) and bool((val[:-1] >= val[1:]).all())
    # flat form with the caller's utterance numbers, a window, no gaps and no events
    flat = RunTracker(H, f_window=(64, 100), gaps=False, device=DEV)
    flat.update((dev(vals), dev(idx)), segments=dev(seg.astype(np.int32)))
    assert torch.equal(flat.runs, tracker.runs[64:164]) and torch.equal(flat.sum_squares, tracker.sum_squares[64:164])
    assert torch.equal(flat.duration_hist, tracker.duration_hist[64:164]) and torch.equal(flat.total_rows, tracker.total_rows)
    assert bool(torch.isnan(flat.summary().median_gap).all())
    with pytest.raises(N.WsaeError):
        flat.update((torch.from_numpy(vals), torch.from_numpy(idx)), segments=torch.from_numpy(seg))
    # two shards merged equal the whole, events included; save / load; a loaded tracker goes on counting
    a = collect_runs(sae, batches[:1], max_events=20000, min_event_len=2)
    b = collect_runs(sae, batches[1:], max_events=tracker.event_count, min_event_len=2)
    a.merge(b)
    same_ints({f: getattr(a, p).cpu().numpy() for f, p in (("frames", "frames"), ("runs", "runs"), ("dur_max", "max_run"),
                                                           ("dur_sq", "sum_squares"), ("dur_hist", "duration_hist"),
                                                           ("gap_hist", "gap_hist"), ("total_rows", "total_rows"))}, want)
    assert a._next == UTT and a.event_count == tracker.event_count
    assert all(torch.equal(x, y) for x, y in zip(a.events(), ev))
    short = collect_runs(sae, batches[1:], max_events=3, min_event_len=2)  # a shard that dropped records: the merge says so
    whole = collect_runs(sae, batches[:1], max_events=20000, min_event_len=2)
    whole.merge(short)
    assert whole.event_count == tracker.event_count and torch.equal(whole.runs, tracker.runs)
    with pytest.raises(N.WsaeError):
        whole.events()
    with tempfile.TemporaryDirectory(prefix="wsae_runs_") as d:
        tracker.save(f"{d}/r.pt")
        back = RunTracker.load(f"{d}/r.pt", device=DEV)
    assert all(torch.equal(x, y) for x, y in zip(back.events(), ev)) and torch.equal(back.gap_hist, tracker.gap_hist)
    assert torch.equal(back.sum_squares, tracker.sum_squares) and back._next == UTT and back._submitted == UTT * T
    x0, m0 = batches[1]
    c0 = sae.encode_compact(x0.to(DEV))
    back.update((c0[0].reshape(1, T, -1), c0[1].reshape(1, T, -1)), frame_mask=m0.to(DEV))
    assert back._next == UTT + 1 and int(back.total_rows.item()) == int(mask.sum() + m0.sum())
    assert int(back.events().utterance.max()) == UTT


def test_flat_form_takes_global_utterance_numbers(cases):
    shape = RO.SHAPES[1]
    code, seg, _ = cases[shape]
    hidden, n_seg = shape[2], shape[3]
    seg = whole_utterances(seg, n_seg)
    want = RO.update(code, hidden, seg, n_seg)
    base = 10 ** 8 + 7
    far = np.where(seg >= 0, seg + base, seg).astype(np.int32)
    cut = int(np.nonzero(seg >= 5)[0][0])  # two shards, cut between utterances
    parts = []
    for a, b in ((0, cut), (cut, len(seg))):
        t = RunTracker(hidden, max_events=5000, device=DEV)
        t.update((dev(code[0][a:b]), dev(code[1][a:b])), segments=dev(far[a:b]))
        assert t._ws.numel() <= 2 * n_seg  # the workspace follows the span of the numbers, not their size
        parts.append(t)
    whole = RunTracker(hidden, max_events=5000, device=DEV)
    whole.update((dev(code[0]), dev(code[1])), segments=dev(far))
    parts[0].merge(parts[1])  # flat trackers keep the caller's numbers
    for t in (whole, parts[0]):
        got = {"frames": t.frames, "runs": t.runs, "dur_max": t.max_run, "dur_sq": t.sum_squares, "dur_hist": t.duration_hist,
               "gap_hist": t.gap_hist, "total_rows": t.total_rows}
        same_ints({f: x.cpu().numpy() for f, x in got.items()}, want)
        ev = t.events()
        shifted = dict(want["events"], segment=want["events"]["segment"] + np.int32(base))
        same_events({"feature": ev.feature.cpu().numpy(), "segment": ev.utterance.cpu().numpy(), "start": ev.start.cpu().numpy(),
                     "length": ev.length.cpu().numpy(), "total": ev.total.cpu().numpy(), "peak": ev.peak.cpu().numpy()}, shifted)
    # padding only, and the two ways of numbering do not mix
    whole.update((dev(code[0][:4]), dev(code[1][:4])), segments=dev(np.full(4, -1, np.int32)))
    assert int(whole.total_rows.item()) == want["total_rows"][0]
    with pytest.raises(ValueError):
        whole.update((dev(code[0][:4]).reshape(1, 4, -1), dev(code[1][:4]).reshape(1, 4, -1)))
    numbered = RunTracker(hidden, max_events=5000, device=DEV)
    numbered.update((dev(code[0][:4]).reshape(1, 4, -1), dev(code[1][:4]).reshape(1, 4, -1)))
    with pytest.raises(ValueError):
        whole.merge(numbered)
