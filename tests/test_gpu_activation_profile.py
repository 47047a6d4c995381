"""Activation profiles on the MI355X: every output of ``wsae_profile_update`` and ``wsae_sample_update`` bit for bit
against the numpy oracle of tests/profile_oracle.py, the properties that make the states independent of batching and
call order, the pre-filter of the sampler, and the Python layer on real modules.  The inputs and the conditions that keep
them from being degenerate are checked on the CPU in tests/test_activation_profile.py."""

from __future__ import annotations

import tempfile

import numpy as np
import pytest
import torch

import profile_oracle as PO
from whisper_sae import _native as N
from whisper_sae.analysis import (ActivationProfile, ActivationSampler, ProfileSummary, SampledActivations,
                                  collect_activation_profile, collect_activation_samples, top_profile_features)
from whisper_sae.sae.model import BatchTopKSAE, ReLUSAE, TopKSAE

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
JUNK = 0x5a5a5a5
TAIL = 3  # junk rows behind every state array


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def code_args(code, seg):
    v, i = dev(code[0]), dev(code[1])
    s = None if seg is None else dev(np.asarray(seg, np.int32))
    return v, i, s


class ProfileState:
    """Device state of ``wsae_profile_update``: every per-feature array has three more rows than the window, filled with
    junk that must survive."""

    def __init__(self, hidden, window=None):
        self.hidden = hidden
        self.f_lo, self.f_cols = (0, hidden) if window is None else window
        F = self.f_cols

        def state(*tail, dtype=torch.int32, fill=0):
            t = torch.full((F + TAIL, *tail), fill, dtype=dtype, device=DEV)
            t[F:] = JUNK
            return t

        self.t = {"fires": state(), "hist": state(PO.BINS), "max_bits": state(), "min_bits": state(fill=PO.MIN_INIT),
                  "over": state(), "sum_q": state(dtype=torch.int64), "total_rows": torch.zeros(1, dtype=torch.int64, device=DEV)}

    def update(self, code, seg, n_rows=None):
        v, i, s = code_args(code, seg)
        t = self.t
        n_rows = v.shape[0] if n_rows is None else n_rows
        N.check(N.lib().wsae_profile_update(v.data_ptr(), i.data_ptr(), v.shape[1], self.hidden, N.ptr(s), n_rows, self.f_lo,
                                            self.f_cols, t["fires"].data_ptr(), t["hist"].data_ptr(), t["max_bits"].data_ptr(),
                                            t["min_bits"].data_ptr(), t["over"].data_ptr(), t["sum_q"].data_ptr(),
                                            t["total_rows"].data_ptr(), None, 0, torch.cuda.current_stream().cuda_stream),
                "wsae_profile_update")
        torch.cuda.synchronize()
        return self

    def ints(self):
        out = {}
        for name, t in self.t.items():
            if name != "total_rows":
                assert bool((t[self.f_cols:] == JUNK).all()), name
                t = t[:self.f_cols]
            out[name] = t.cpu().numpy()
        return out


class SampleState:
    """Device state of ``wsae_sample_update``, with junk behind the window; the workspace holds arbitrary bytes on entry."""

    def __init__(self, hidden, edges, m, seed, window=None):
        self.hidden, self.m, self.seed = hidden, m, seed
        self.f_lo, self.f_cols = (0, hidden) if window is None else window
        self.S = 1 if edges is None else edges.shape[1] + 1
        self.edges = None if edges is None or self.S == 1 else dev(np.asarray(edges, np.float32))
        F = self.f_cols
        self.keys = torch.full((F + TAIL, self.S, m), -1, dtype=torch.int64, device=DEV)
        self.svals = torch.zeros(F + TAIL, self.S, m, dtype=torch.float32, device=DEV)
        self.seen = torch.zeros(F + TAIL, self.S, dtype=torch.int32, device=DEV)
        self.keys[F:], self.svals[F:], self.seen[F:] = JUNK, 123.25, JUNK

    def load(self, st):
        F = self.f_cols
        self.keys[:F] = dev(st["keys"].view(np.int64))
        self.svals[:F], self.seen[:F] = dev(st["svals"]), dev(st["seen"])
        return self

    def update(self, code, seg, ord_base, n_rows=None):
        v, i, s = code_args(code, seg)
        lib = N.lib()
        n_rows = v.shape[0] if n_rows is None else n_rows
        need = lib.wsae_sample_workspace_bytes(n_rows, v.shape[1], self.hidden, self.f_lo, self.f_cols, self.S, self.m)
        assert need >= 12 * n_rows * v.shape[1]
        ws = torch.full((need + 8,), 0xAB, dtype=torch.uint8, device=DEV)  # (arbitrary contents on entry)
        N.check(lib.wsae_sample_update(v.data_ptr(), i.data_ptr(), v.shape[1], self.hidden, N.ptr(s), n_rows, ord_base,
                                       self.f_lo, self.f_cols, N.ptr(self.edges), self.S, self.m, self.seed,
                                       self.keys.data_ptr(), self.svals.data_ptr(), self.seen.data_ptr(), ws.data_ptr(), need,
                                       torch.cuda.current_stream().cuda_stream), "wsae_sample_update")
        torch.cuda.synchronize()
        assert bool((ws[need:] == 0xAB).all())
        if n_rows:  # the entries that passed the pre-filter: the total behind the per-list offsets (counts | offsets | cursors)
            n_lists = self.f_cols * self.S
            self.survivors = int(ws[:4 * (2 * n_lists + 1)].view(torch.int32)[2 * n_lists].item())
        return self

    def arrays(self):
        F = self.f_cols
        assert bool((self.keys[F:] == JUNK).all()) and bool((self.svals[F:] == 123.25).all()) and bool((self.seen[F:] == JUNK).all())
        return {"keys": self.keys[:F].cpu().numpy().view(np.uint64), "svals": self.svals[:F].cpu().numpy(),
                "seen": self.seen[:F].cpu().numpy()}


def same_ints(got, want, fields=PO.INT_FIELDS):
    for f in fields:
        assert got[f].dtype == want[f].dtype and np.array_equal(got[f], want[f]), (f, np.argwhere(got[f] != want[f])[:5])


def same_samples(got, want):
    for f in PO.SAMPLE_FIELDS:
        a, b = got[f], want[f]
        assert a.dtype == b.dtype and a.shape == b.shape, (f, a.dtype, b.dtype, a.shape, b.shape)
        if f == "svals":
            a, b = a.view(np.int32), b.view(np.int32)
        assert np.array_equal(a, b), (f, np.argwhere(a != b)[:5])


@pytest.fixture(scope="module")
def general():
    code, seg = PO.general_case()
    return code, seg, PO.profile(code, seg, PO.HIDDEN)


# ---- the profile -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [None, PO.WINDOW], ids=["all", "window"])
def test_profile_equals_the_oracle(general, window):
    code, seg, want = general
    if window is not None:
        want = PO.profile(code, seg, PO.HIDDEN, window)
    same_ints(ProfileState(PO.HIDDEN, window).update(code, seg).ints(), want)
    # without seg every row is live
    same_ints(ProfileState(PO.HIDDEN, window).update(code, None).ints(), PO.profile(code, None, PO.HIDDEN, window))


@pytest.mark.parametrize("k", [1, 128])
def test_profile_width_edges(k):
    code, seg = PO.wide_case(k)
    same_ints(ProfileState(300).update(code, seg).ints(), PO.profile(code, seg, 300))
    same_ints(ProfileState(300, (250, 50)).update(code, seg).ints(), PO.profile(code, seg, 300, (250, 50)))


def test_profile_without_rows_leaves_the_state_untouched(general):
    code, seg, want = general
    st = ProfileState(PO.HIDDEN).update(code, seg)
    st.update(code, seg, n_rows=0)
    st.update(code, None, n_rows=0)
    same_ints(st.ints(), want)


def test_profile_counts_exactly_under_contention():
    rows = 5000
    vals = np.where(np.arange(rows) % 2 == 0, 1.0, 1.125).astype(np.float32)[:, None].repeat(2, 1)
    idx = np.stack([np.full(rows, 3), np.arange(rows) % 7 + 4], axis=1).astype(np.int32)  # feature 3 on every row
    want = PO.profile((vals, idx), None, 16)
    assert want["fires"][3] == rows and want["hist"][3, 96] == want["hist"][3, 97] == rows // 2
    assert want["sum_q"][3] == (rows // 2) * (2 ** 20 + 9 * 2 ** 17)
    same_ints(ProfileState(16).update((vals, idx), None).ints(), want)


def test_profile_batching_and_call_order_do_not_matter(general):
    code, seg, want = general
    cuts = [(0, 130), (130, 131), (131, PO.ROWS)]
    for order in (cuts, cuts[::-1]):
        st = ProfileState(PO.HIDDEN)
        for a, b in order:
            st.update((code[0][a:b], code[1][a:b]), seg[a:b])
        same_ints(st.ints(), want)


# ---- the sampler -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", PO.SAMPLER_SHAPES, ids=lambda s: f"S{s[0]}m{s[1]}")
def test_sampler_equals_the_oracle(general, shape):
    code, seg, prof = general
    S, m = shape
    edges = PO.sampler_edges(prof, S)
    want = PO.sample(code, seg, 77, edges, m, 5, PO.HIDDEN)
    same_samples(SampleState(PO.HIDDEN, edges, m, 5).update(code, seg, 77).arrays(), want)
    lo, cols = PO.WINDOW
    win = SampleState(PO.HIDDEN, edges[lo:lo + cols], m, 5, PO.WINDOW).update(code, seg, 77).arrays()
    same_samples(win, {f: want[f][lo:lo + cols] for f in PO.SAMPLE_FIELDS})  # (the priority mixes the feature, not the column)


@pytest.mark.parametrize("k", [1, 128])
def test_sampler_width_edges(k):
    code, seg = PO.wide_case(k)
    edges = PO.quantile_edges(PO.profile(code, seg, 300), 4)
    want = PO.sample(code, seg, 2 ** 31 - code[0].shape[0], edges, 2, 9, 300)  # the last ordinals there are
    same_samples(SampleState(300, edges, 2, 9).update(code, seg, 2 ** 31 - code[0].shape[0]).arrays(), want)


def test_sampler_batching_and_call_order_do_not_matter(general):
    code, seg, prof = general
    edges = PO.sampler_edges(prof, 3)
    want = PO.sample(code, seg, 1000, edges, 4, 5, PO.HIDDEN)
    cuts = [(0, 100), (100, 101), (101, 400), (400, PO.ROWS)]
    for order in (cuts, cuts[::-1]):
        st = SampleState(PO.HIDDEN, edges, 4, 5)
        for a, b in order:
            st.update((code[0][a:b], code[1][a:b]), seg[a:b], 1000 + a)
        same_samples(st.arrays(), want)
    st = SampleState(PO.HIDDEN, edges, 4, 5).update(code, seg, 1000)
    st.update(code, seg, 5, n_rows=0)  # no rows: untouched
    same_samples(st.arrays(), want)


def test_sampler_pre_filter():
    """Lists that are full of smaller keys reject everything: the state changes in ``seen`` alone.  Then one entry with a
    key below a list's last displaces it."""
    hidden, m, seed = 8, 4, 3
    rng = np.random.default_rng(8)
    rows = 400
    vals = rng.uniform(0.5, 2.0, (rows, 2)).astype(np.float32)
    idx = np.stack([rng.integers(0, 4, rows), rng.integers(4, 8, rows)], axis=1).astype(np.int32)
    first = PO.sample((vals, idx), None, 0, None, m, seed, hidden)
    assert first["seen"].min() > 3 * m
    # a second batch whose keys all lie above every list's last key
    last = first["keys"][:, 0, m - 1]
    ordinal = np.arange(rows, 40 * rows)
    f0, f1 = idx[ordinal % rows, 0], idx[ordinal % rows, 1]
    above = (PO.key_of(ordinal, f0, seed) > last[f0]) & (PO.key_of(ordinal, f1, seed) > last[f1])
    pick = ordinal[above][:300]
    assert pick.size == 300
    # rows between the picked ordinals are padding, so that every picked row keeps its ordinal
    span = int(pick[-1]) + 1 - rows
    v2, i2 = np.ones((span, 2), np.float32), np.zeros((span, 2), np.int32)
    seg2 = np.full(span, -1, np.int32)
    seg2[pick - rows] = 0
    v2[pick - rows], i2[pick - rows] = vals[pick % rows], idx[pick % rows]
    st = SampleState(hidden, None, m, seed).load(first)
    got = st.update((v2, i2), seg2, rows).arrays()
    assert st.survivors == 0  # (a filter that let everything through would leave the same state)
    want = PO.sample((v2, i2), seg2, rows, None, m, seed, hidden, state=first)
    assert np.array_equal(want["keys"], first["keys"]) and np.array_equal(want["seen"].sum(), first["seen"].sum() + 600)
    same_samples(got, want)
    # one entry of feature 5 that beats the last element of its list, found by search
    cand = np.arange(40 * rows, 80 * rows)
    better = cand[(PO.key_of(cand, 5, seed) < last[5]) & (PO.key_of(cand, 5, seed) > first["keys"][5, 0, m - 2])]
    assert better.size > 0
    o = int(better[0])
    one = (np.array([[0.75, -1.0]], np.float32), np.array([[5, 5]], np.int32))
    got = st.update(one, None, o).arrays()
    assert st.survivors == 1
    want2 = PO.sample(one, None, o, None, m, seed, hidden, state=want)
    assert want2["keys"][5, 0, m - 1] == PO.key_of(o, 5, seed) and want2["svals"][5, 0, m - 1] == 0.75
    assert np.array_equal(want2["keys"][5, 0, :m - 1], want["keys"][5, 0, :m - 1]) and want2["seen"][5, 0] == want["seen"][5, 0] + 1
    same_samples(got, want2)


# ---- the Python layer --------------------------------------------------------------------------------------------------
D, H, K, UTT, T = 64, 256, 8, 12, 40


def utterances(seed):
    """12 utterances of 40 frames in three batches, with a frame mask.  A frame repeats for a stretch of about three
    frames at a loudness that varies over a few octaves, so a feature fires often and over a range of values."""
    gen = torch.Generator().manual_seed(seed)
    proto = torch.randn(UTT, 14, D, generator=gen)
    hold = (torch.rand(UTT, T, generator=gen) < 0.3).cumsum(1) % 14
    x = torch.gather(proto, 1, hold[:, :, None].expand(UTT, T, D)) * torch.exp(torch.randn(UTT, T, 1, generator=gen))
    mask = torch.ones(UTT, T)
    for u in range(UTT):
        mask[u, 24 + (u % 5) * 3:] = 0
    mask[3, 10] = 0
    return [(x[:5], mask[:5]), (x[5:6], mask[5:6]), (x[6:], mask[6:])], mask


def make_sae(cls, seed, **kw):
    torch.manual_seed(seed)
    return cls(D, H, k=K, **kw).to(DEV)


def profile_ints(p):
    return {f: getattr(p, f).cpu().numpy() for f in PO.INT_FIELDS}


def sampler_arrays(s):
    return {"keys": s.keys.cpu().numpy().view(np.uint64), "svals": s.values.cpu().numpy(), "seen": s.seen.cpu().numpy()}


@pytest.mark.parametrize("kind", ["topk", "batch_topk"])
def test_python_layer_on_real_modules(kind):
    sae = make_sae(TopKSAE, 1) if kind == "topk" else make_sae(BatchTopKSAE, 2, max_k_per_row=16)
    batches, mask = utterances(5)
    sae.train()
    prof = collect_activation_profile(sae, batches)
    assert sae.training
    sae.eval()
    codes = [sae.encode_compact(x.to(DEV)) for x, _ in batches]
    vals, idx = (np.concatenate([c[i].reshape(-1, c[i].shape[-1]).cpu().numpy() for c in codes]) for i in (0, 1))
    seg = np.where(mask.reshape(-1).numpy() != 0, 0, -1).astype(np.int32)
    want = PO.profile((vals, idx), seg, H)
    assert want["total_rows"][0] == mask.sum() and (want["fires"] >= 10).sum() >= 10
    same_ints(profile_ints(prof), want)
    # the summary: equality where the formula is integer or a bitcast, rtol 1e-12 for the float64 divisions
    summ, ref = prof.summary(), PO.summary(want)
    assert isinstance(summ, ProfileSummary)
    for name in summ._fields:
        got = getattr(summ, name).cpu().numpy()
        if name in ("fires", "over", "max", "min"):
            assert got.dtype == ref[name].dtype and np.array_equal(got, ref[name], equal_nan=True), name
        else:
            np.testing.assert_allclose(got, ref[name], rtol=1e-12, atol=0, equal_nan=True, err_msg=name)
    for q in (0.0, 0.3, 1.0):
        np.testing.assert_allclose(prof.quantile(q).cpu().numpy(), PO.quantile(want, q), rtol=1e-12, atol=0, equal_nan=True)
    S, m, seed = 5, 3, 11
    edges = prof.quantile_edges(S)
    assert edges.dtype == torch.float32 and np.array_equal(edges.cpu().numpy(), PO.quantile_edges(want, S), equal_nan=True)
    fm = prof.fraction_of_max_edges(4).cpu().numpy()
    top_v = PO.bits_to_value(want["max_bits"], want["fires"])
    assert np.array_equal(fm, (top_v[:, None] * (np.arange(1, 4) / 4)[None, :]).astype(np.float32), equal_nan=True)
    dens = prof.density_histogram(bins=12)
    assert dens.dead == (want["fires"] == 0).sum() and int(dens.counts.sum()) + dens.dead == H and dens.edges.numel() == 13
    top, val = top_profile_features(summ, by="mean", n=5, min_fires=10)
    assert top.numel() == 5 and bool((summ.fires[top] >= 10).all()) and bool((val[:-1] >= val[1:]).all())
    with pytest.raises(ValueError):
        top_profile_features(summ, by="nope")
    # the second pass: samples per quantile band
    smp = collect_activation_samples(sae, batches, prof, n_strata=S, keep=m, seed=seed)
    want_s = PO.sample((vals, idx), seg, 0, PO.quantile_edges(want, S), m, seed, H)
    assert (want_s["seen"] > m).any() and np.array_equal(want_s["seen"].sum(1), want["fires"])
    same_samples(sampler_arrays(smp), want_s)
    f = int(np.argmax(want["fires"]))
    ex = smp.examples(f)
    held = want_s["keys"][f] != PO.EMPTY
    assert isinstance(ex, SampledActivations) and ex.value.numel() == held.sum()
    assert np.array_equal(ex.stratum.numpy(), np.nonzero(held)[0]) and np.array_equal(ex.seen.numpy(), want_s["seen"][f])
    assert np.array_equal(ex.value.numpy().view(np.int32), want_s["svals"][f][held].view(np.int32))
    ordinal = (want_s["keys"][f][held] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert np.array_equal(ex.ordinal.numpy(), ordinal)
    assert np.array_equal(ex.utterance.numpy(), ordinal // T) and np.array_equal(ex.frame.numpy(), ordinal % T)
    act_row = np.any((idx[ordinal] == f) & (vals[ordinal] > 0), axis=1)  # every sampled frame is one where f fired
    assert bool(act_row.all()) and bool((seg[ordinal] == 0).all())
    # two shards with disjoint ordinals merge into the sampler fed both; merged profiles likewise
    n0 = sum(x.shape[0] * x.shape[1] for x, _ in batches[:1])
    a = collect_activation_samples(sae, batches[:1], edges, keep=m, seed=seed)
    b = collect_activation_samples(sae, batches[1:], edges, keep=m, seed=seed, ordinal_base=n0)
    a.merge(b)
    same_samples(sampler_arrays(a), want_s)
    assert all(torch.equal(p, q) for p, q in zip(a.examples(f), ex)) and (a.ordinal_base, a._next) == (0, UTT * T)
    with pytest.raises(ValueError):
        a.merge(collect_activation_samples(sae, batches[:1], edges, keep=m, seed=seed))  # the same ordinals again
    pa, pb = collect_activation_profile(sae, batches[:2]), collect_activation_profile(sae, batches[2:])
    pb.merge(pa)
    same_ints(profile_ints(pb), want)
    # flat codes: no utterance to name; a window; save / load; a loaded object goes on counting
    flat = ActivationSampler(H, edges[64:164], keep=m, seed=seed, f_window=(64, 100), device=DEV)
    flat.update((dev(vals), dev(idx)), frame_mask=dev((seg >= 0).astype(np.float32)))
    same_samples(sampler_arrays(flat), {k: v[64:164] for k, v in want_s.items()})
    fx = flat.examples(64 + int(np.argmax(want["fires"][64:164])))
    assert fx.value.numel() > 0 and bool((fx.utterance == -1).all()) and bool((fx.frame == -1).all())
    with tempfile.TemporaryDirectory(prefix="wsae_profile_") as d:
        prof.save(f"{d}/p.pt")
        smp.save(f"{d}/s.pt")
        back_p, back_s = ActivationProfile.load(f"{d}/p.pt", device=DEV), ActivationSampler.load(f"{d}/s.pt", device=DEV)
    same_ints(profile_ints(back_p), want)
    same_samples(sampler_arrays(back_s), want_s)
    assert all(torch.equal(p, q) for p, q in zip(back_s.examples(f), ex)) and back_s._next == UTT * T
    x0, m0 = batches[1]
    c0 = sae.encode_compact(x0.to(DEV))
    c0 = (c0[0].reshape(1, T, -1), c0[1].reshape(1, T, -1))
    back_p.update(c0, frame_mask=m0.to(DEV))
    back_s.update(c0, frame_mask=m0.to(DEV))
    assert int(back_p.total_rows.item()) == int(mask.sum() + m0.sum()) and back_s._next == (UTT + 1) * T
    again = (c0[0].reshape(T, -1).cpu().numpy(), c0[1].reshape(T, -1).cpu().numpy())
    seg0 = np.where(m0.reshape(-1).numpy() != 0, 0, -1)
    same_ints(profile_ints(back_p), PO.profile(again, seg0, H, state=want))
    same_samples(sampler_arrays(back_s), PO.sample(again, seg0, UTT * T, PO.quantile_edges(want, S), m, seed, H, state=want_s))
    # errors that need the device
    with pytest.raises(N.WsaeError):
        prof.update((torch.from_numpy(vals), torch.from_numpy(idx)))
    with pytest.raises(N.WsaeError):
        smp.update((torch.from_numpy(vals), torch.from_numpy(idx)))
    with pytest.raises(ValueError):
        prof.update((dev(vals), dev(idx)), frame_mask=dev(np.ones(3, np.float32)))
    with pytest.raises(TypeError):
        collect_activation_profile(ReLUSAE(D, H).to(DEV), batches)
    with pytest.raises(TypeError):
        collect_activation_samples(ReLUSAE(D, H).to(DEV), batches, prof)
