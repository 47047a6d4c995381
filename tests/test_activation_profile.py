"""Activation profiles without a GPU: the numpy oracle of tests/profile_oracle.py against hand-worked cases (every bin
edge and the float just below it, the rounding of ``sum_q`` on ties, the repeated-index rule, the sampler as a brute-force
loop), the uniformity of the priority hash, the conditions that keep the GPU test inputs from being degenerate, every
argument error of ``wsae_profile_update`` / ``wsae_sample_update`` (raised before any HIP call), the workspace query, the
header / ``SIGNATURES`` / exports, the Python layer's errors and its float64 readers on the oracle's integer state."""

from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest

import profile_oracle as PO

HEADER = Path(__file__).resolve().parents[1] / "include" / "wsae.h"
NAMES = ("wsae_profile_workspace_bytes", "wsae_profile_update", "wsae_sample_workspace_bytes", "wsae_sample_update")


def code_of(rows, k=3):
    """rows: per row a list of (index, value) -> (vals, idx) padded with (0, 0.0) entries."""
    vals, idx = np.zeros((len(rows), k), np.float32), np.zeros((len(rows), k), np.int32)
    for r, entries in enumerate(rows):
        for e, (i, v) in enumerate(entries):
            idx[r, e], vals[r, e] = i, v
    return vals, idx


# ---- the oracle against hand-worked cases -----------------------------------------------------------------------------------
def test_bins_at_every_edge_and_just_below():
    assert PO.bin_of(np.array([2.0 ** -12, 1.0, 1.125, 4096.0], np.float32)).tolist() == [0, 96, 97, 191]
    for e in range(24):
        for s in range(8):
            edge = np.float32(2.0 ** (e - 12) * (1 + s / 8))  # exact
            j = 8 * e + s
            assert PO.bin_lower(j) == float(edge)
            assert PO.bin_of(edge) == j and PO.bin_of(np.nextafter(edge, np.float32(0))) == max(j - 1, 0), (e, s)
    assert PO.bin_lower(192) == 4096.0 and PO.bin_of(np.nextafter(np.float32(4096), np.float32(0))) == 191
    low = np.array([1.4e-45, 1e-40, 1.1754944e-38, 2.0 ** -13, 2.0 ** -12 * 1.124], np.float32)  # denormals and below 2^-12
    assert PO.bin_of(low).tolist() == [0] * 5
    assert PO.bin_of(np.array([4097.0, 1e9, 3e38, np.inf], np.float32)).tolist() == [191] * 4


def test_sum_q_rounds_ties_to_even_and_saturates():
    u = 2.0 ** -21  # half a unit of the fixed point
    v = np.array([u, 3 * u, 5 * u, 7 * u, 2 * u, 1.0, 1.5 + u, 4096.0, 1e9, np.inf, 1e-40], np.float32)
    want = [0, 2, 2, 4, 1, 2 ** 20, 3 * 2 ** 19 + 0, 2 ** 32, 2 ** 32, 2 ** 32, 0]  # (1.5 + 2^-21) 2^20 = 1572864.5 -> even
    assert PO.sum_q_terms(v).tolist() == want
    st = PO.profile(code_of([[(0, u), (1, 3 * u), (2, 1e9)], [(0, 5 * u), (1, 7 * u), (2, np.inf)]]), None, 3)
    assert st["sum_q"].tolist() == [2, 6, 2 ** 33] and st["over"].tolist() == [0, 0, 2] and st["hist"][2, 191] == 2


def test_activity_rule_on_hand_worked_rows():
    nan = float("nan")
    rows = [[(1, -3.0), (1, 4.0), (1, 9.0)],   # the first ACTIVE entry of a repeated index gives the value
            [(1, 0.0), (2, nan), (5, 1.0)],    # zero and NaN are not active; index 5 is outside hidden = 4
            [(1, 2.0), (-1, 1.0), (3, 0.5)],
            [(3, 8.0), (3, 0.25), (0, 1.0)]]   # a padding row (below)
    st = PO.profile(code_of(rows), [0, 5, 0, -1], 4)
    assert st["fires"].tolist() == [0, 2, 0, 1] and st["total_rows"][0] == 3
    assert st["hist"][1, PO.bin_of(np.float32(4))] == 1 and st["hist"][1, PO.bin_of(np.float32(2))] == 1 and st["hist"].sum() == 3
    assert st["sum_q"].tolist() == [0, 6 << 20, 0, 1 << 19]
    as_bits = lambda x: int(np.float32(x).view(np.int32))  # noqa: E731
    assert st["max_bits"].tolist() == [0, as_bits(4), 0, as_bits(0.5)]
    assert st["min_bits"].tolist() == [PO.MIN_INIT, as_bits(2), PO.MIN_INIT, as_bits(0.5)]
    # a window keeps its features; all rows live without seg; a second call adds
    win = PO.profile(code_of(rows), None, 4, window=(3, 1))
    assert win["fires"].tolist() == [2] and win["total_rows"][0] == 4 and win["max_bits"][0] == as_bits(8)
    two = PO.profile(code_of(rows), [0, 5, 0, -1], 4, state=st)
    assert two["fires"].tolist() == [0, 4, 0, 2] and st["fires"].tolist() == [0, 2, 0, 1] and two["total_rows"][0] == 6
    merged = PO.merge_profiles(st, st)
    assert all(np.array_equal(merged[f], two[f]) for f in PO.INT_FIELDS)


def py_priority(o, f, seed):
    m = 0xFFFFFFFF
    x = ((o * 0x9E3779B1) & m) ^ ((f * 0x85EBCA77) & m) ^ seed
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & m
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & m
    x ^= x >> 16
    return x


def test_priority_and_key_against_plain_integers():
    rng = np.random.default_rng(3)
    o = rng.integers(0, 2 ** 31, 200)
    f = rng.integers(0, 40960, 200)
    for seed in (0, 7, 2 ** 32 - 1):
        got = PO.priority(o, f, seed)
        assert got.dtype == np.uint32 and got.tolist() == [py_priority(int(a), int(b), seed) for a, b in zip(o, f)]
        key = PO.key_of(o, f, seed)
        assert key.dtype == np.uint64 and key.tolist() == [(py_priority(int(a), int(b), seed) << 32) | int(a) for a, b in zip(o, f)]
        assert bool((key < PO.EMPTY).all())
    # for a fixed feature the map ordinal -> priority is a bijection (checked on a range): no two keys tie on the priority
    assert np.unique(PO.priority(np.arange(1 << 16), 5, 7)).size == 1 << 16


def test_sampler_oracle_against_a_brute_force_loop():
    (vals, idx), seg = PO.general_case()
    hidden, m, seed, base = PO.HIDDEN, 3, 11, 1000
    st_p = PO.profile((vals, idx), seg, hidden)
    edges = PO.sampler_edges(st_p, 4)
    got = PO.sample((vals, idx), seg, base, edges, m, seed, hidden)
    offered = {}
    for r in range(vals.shape[0]):
        if seg[r] < 0:
            continue
        done = set()
        for e in range(vals.shape[1]):
            f, v = int(idx[r, e]), vals[r, e]
            if not (v > 0) or not 0 <= f < hidden or f in done:
                continue
            done.add(f)
            finite = edges[f][~np.isnan(edges[f])]
            s = int(np.searchsorted(finite, v, side="right")) if finite.size else 0
            offered.setdefault((f, s), []).append(((py_priority(base + r, f, seed) << 32) | (base + r), v))
    for f in range(hidden):
        for s in range(4):
            cand = sorted(offered.get((f, s), []))
            assert got["seen"][f, s] == len(cand)
            keys = [c[0] for c in cand[:m]] + [int(PO.EMPTY)] * (m - min(m, len(cand)))
            assert got["keys"][f, s].tolist() == keys
            assert got["svals"][f, s].tolist() == [float(c[1]) for c in cand[:m]] + [0.0] * (m - min(m, len(cand)))
    # two calls in either order, and the merge of two shards, equal one call
    cut = 300
    a = PO.sample((vals[:cut], idx[:cut]), seg[:cut], base, edges, m, seed, hidden)
    b = PO.sample((vals[cut:], idx[cut:]), seg[cut:], base + cut, edges, m, seed, hidden)
    ab = PO.sample((vals[cut:], idx[cut:]), seg[cut:], base + cut, edges, m, seed, hidden, state=a)
    ba = PO.sample((vals[:cut], idx[:cut]), seg[:cut], base, edges, m, seed, hidden, state=b)
    for st in (ab, ba, PO.merge_samples(a, b), PO.merge_samples(b, a)):
        assert all(np.array_equal(st[f], got[f]) for f in PO.SAMPLE_FIELDS)


def test_priority_is_uniform_and_differs_between_features():
    """For 64 features the bottom-2000 sample of 200 000 consecutive ordinals: chi^2 over 16 equal ordinal ranges stays
    below 56 (the tail of chi^2 with 15 degrees of freedom at about 1e-6 per feature), and two features' samples overlap
    like independent draws: the overlap is hypergeometric with mean 2000^2 / 200 000 = 20 and about Poisson, whose tail
    beyond 50 is below 1e-8 per pair (2016 pairs)."""
    n, m, seed = 200_000, 2000, 7
    ordinals = np.arange(n)
    picks, worst = [], 0.0
    for f in range(64):
        chosen = np.argpartition(PO.key_of(ordinals, f, seed), m)[:m]
        count = np.bincount(chosen * 16 // n, minlength=16)
        chi2 = float(((count - m / 16) ** 2 / (m / 16)).sum())
        worst = max(worst, chi2)
        member = np.zeros(n, bool)
        member[chosen] = True
        picks.append(member)
    assert worst < 56, worst
    picks = np.stack(picks).astype(np.int32)
    overlap = picks @ picks.T
    off = overlap[~np.eye(64, dtype=bool)]
    assert off.max() < 50 and 15 < off.mean() < 25, (off.max(), off.mean())


# ---- the GPU test inputs are not degenerate -----------------------------------------------------------------------------------
def test_conditions_on_the_gpu_test_inputs():
    (vals, idx), seg = PO.general_case()
    assert vals.shape == (PO.ROWS, PO.K) and PO.ROWS % 64 and PO.ROWS * PO.K > 256
    st = PO.profile((vals, idx), seg, PO.HIDDEN)
    hit = st["hist"].sum(0) > 0
    assert hit[0] and hit[191] and hit[1:191].sum() >= 100
    assert st["over"].max() > 0 and np.array_equal(st["hist"].sum(1), st["fires"])
    assert np.isnan(vals).any() and np.isinf(vals).any() and (vals < 0).any() and (vals == 0).any()
    assert ((vals > 0) & (vals < 1.1754944e-38)).any()  # denormals
    assert ((idx < 0) | (idx >= PO.HIDDEN)).any() and (seg < 0).any() and 0 < st["total_rows"][0] < PO.ROWS
    live = seg >= 0
    repeats = [r for r in np.nonzero(live)[0] if np.unique(idx[r][vals[r] > 0]).size < (vals[r] > 0).sum()]
    assert len(repeats) > 5  # rows that repeat an active index
    lo, cols = PO.WINDOW
    assert lo <= PO.SILENT < lo + cols and st["fires"][PO.SILENT] == 0 and st["fires"][PO.RARE] == 2
    assert st["fires"][lo - 1] > 0 and st["fires"][lo + cols] > 0  # the features next to the window fire
    win = PO.profile((vals, idx), seg, PO.HIDDEN, PO.WINDOW)
    assert all(np.array_equal(win[f], st[f][lo:lo + cols]) for f in PO.INT_FIELDS[:-1])
    for S, m in PO.SAMPLER_SHAPES:
        edges = PO.sampler_edges(st, S)
        sm = PO.sample((vals, idx), seg, 0, edges, m, 5, PO.HIDDEN)
        assert np.array_equal(sm["seen"].sum(1), st["fires"])
        held = (sm["keys"] != PO.EMPTY).sum(2)
        assert np.array_equal(held, np.minimum(sm["seen"], m))
        if (S, m) == (3, 4):
            assert (sm["seen"] > m).any() and ((sm["seen"] > 0) & (sm["seen"] < m)).any() and (sm["seen"] == 0).any()
        if S > 2:
            assert (sm["seen"][PO.TIED] == 0).any() and st["fires"][PO.TIED] > 0  # equal edges: an empty stratum
        assert bool((np.diff(sm["keys"].astype(np.float64), axis=2) >= 0).all())  # ascending, the unused slots last
    for k in (1, 128):
        code, sg = PO.wide_case(k)
        wide = PO.profile(code, sg, 300)
        assert wide["fires"].sum() > 0 and wide["total_rows"][0] < code[0].shape[0]
        if k == 128:
            assert wide["fires"].sum() < ((code[0] > 0) & (code[1] >= 0) & (code[1] < 300) & (sg >= 0)[:, None]).sum()  # repeats


# ---- argument errors: made-up (aligned, never dereferenced) pointers, every case fails its checks first -----------------
def _profile(N, k=32, hidden=64, n_rows=16, f_lo=0, f_cols=64, vals=4096, idx=4096, seg=4096, fires=4096, hist=4096,
             max_bits=4096, min_bits=4096, over=4096, sum_q=4096, total=4096, ws=None, ws_bytes=0):
    return N.lib().wsae_profile_update(vals, idx, k, hidden, seg, n_rows, f_lo, f_cols, fires, hist, max_bits, min_bits, over,
                                       sum_q, total, ws, ws_bytes, None)


def _sample(N, k=32, hidden=64, n_rows=16, ord_base=0, f_lo=0, f_cols=64, edges=4096, S=4, m=8, seed=1, vals=4096, idx=4096,
            seg=4096, keys=4096, svals=4096, seen=4096, ws=4096, ws_bytes=1 << 20):
    return N.lib().wsae_sample_update(vals, idx, k, hidden, seg, n_rows, ord_base, f_lo, f_cols, edges, S, m, seed, keys,
                                      svals, seen, ws, ws_bytes, None)


CODE_ERRORS = {"k0": dict(k=0), "k129": dict(k=129), "window_past_end": dict(f_lo=40, f_cols=25),
               "window_negative": dict(f_lo=-1), "window_empty": dict(f_cols=0), "n_rows_2p31": dict(n_rows=2 ** 31),
               "n_rows_negative": dict(n_rows=-1), "hidden0": dict(hidden=0), "null_vals": dict(vals=None),
               "null_idx": dict(idx=None)}
PROFILE_ERRORS = dict(CODE_ERRORS, null_fires=dict(fires=None), null_hist=dict(hist=None), null_max=dict(max_bits=None),
                      null_min=dict(min_bits=None), null_over=dict(over=None), null_sum=dict(sum_q=None),
                      null_total=dict(total=None), workspace_negative=dict(ws_bytes=-1))
SAMPLE_ERRORS = dict(CODE_ERRORS, null_keys=dict(keys=None), null_svals=dict(svals=None), null_seen=dict(seen=None),
                     strata0=dict(S=0), strata17=dict(S=17), keep0=dict(m=0), keep65=dict(m=65),
                     edges_missing=dict(edges=None, S=2), ord_negative=dict(ord_base=-1),
                     ord_past_2p31=dict(ord_base=2 ** 31 - 15), too_many_entries=dict(n_rows=2 ** 26, k=32),
                     workspace_short=dict(ws_bytes=3328 + 12 * 16 * 32 - 1), workspace_null=dict(ws=None),
                     too_many_lists=dict(hidden=2 ** 28, f_cols=2 ** 28, S=8, ws_bytes=2 ** 40))


@pytest.mark.parametrize("kw", list(PROFILE_ERRORS.values()), ids=list(PROFILE_ERRORS))
def test_profile_argument_errors_do_not_need_a_gpu(kw):
    from whisper_sae import _native as N
    assert _profile(N, **kw) == -1
    assert "wsae_profile_update" in N.last_error()


@pytest.mark.parametrize("kw", list(SAMPLE_ERRORS.values()), ids=list(SAMPLE_ERRORS))
def test_sample_argument_errors_do_not_need_a_gpu(kw):
    from whisper_sae import _native as N
    assert _sample(N, **kw) == -1
    assert "wsae_sample_update" in N.last_error()


def test_empty_calls_and_the_workspace_query():
    from whisper_sae import _native as N
    assert _profile(N, n_rows=0) == 0 and _profile(N, n_rows=0, seg=None) == 0 and _profile(N, n_rows=0, ws=4096, ws_bytes=64) == 0
    pq = N.lib().wsae_profile_workspace_bytes
    assert pq(3_072_000, 32, 3072, 0, 3072) == 0 and pq(0, 1, 1, 0, 1) == 0 and pq(16, 128, 40960, 40000, 960) == 0
    assert pq(16, 0, 64, 0, 64) == -1 and pq(16, 129, 64, 0, 64) == -1 and pq(2 ** 31, 32, 64, 0, 64) == -1
    assert pq(16, 32, 64, 60, 5) == -1 and pq(16, 32, 0, 0, 64) == -1
    assert _sample(N, n_rows=0) == 0 and _sample(N, n_rows=0, ws=None, seg=None) == 0
    assert _sample(N, n_rows=0, S=1, edges=None) == 0 and _sample(N, n_rows=0, ord_base=2 ** 31) == 0
    wq = N.lib().wsae_sample_workspace_bytes
    assert wq(16, 32, 64, 0, 64, 4, 8) == 3328 + 12 * 16 * 32  # three int32 vectors over 256 lists (+ 1), rounded to 256 B
    assert wq(0, 1, 1, 0, 1, 1, 1) == 256 and wq(3_072_000, 32, 40960, 0, 4096, 10, 8) == 491776 + 12 * 3_072_000 * 32
    for bad in ((16, 0, 64, 0, 64, 4, 8), (16, 129, 64, 0, 64, 4, 8), (-1, 32, 64, 0, 64, 4, 8), (2 ** 31, 1, 64, 0, 64, 4, 8),
                (2 ** 26, 32, 64, 0, 64, 4, 8), (16, 32, 64, 60, 5, 4, 8), (16, 32, 64, 0, 64, 0, 8), (16, 32, 64, 0, 64, 17, 8),
                (16, 32, 64, 0, 64, 4, 0), (16, 32, 64, 0, 64, 4, 65), (16, 32, 0, 0, 64, 4, 8),
                (16, 32, 2 ** 28, 0, 2 ** 28, 8, 8)):
        assert wq(*bad) == -1, bad


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
    defines = {k: int(v) for k, v in re.findall(r"#define (WSAE_(?:PROFILE|SAMPLE)_[A-Z_]+) (\d+)", text)}
    assert defines == {"WSAE_PROFILE_MAX_K": N.PROFILE_MAX_K, "WSAE_PROFILE_BINS": N.PROFILE_BINS,
                       "WSAE_SAMPLE_MAX_STRATA": N.SAMPLE_MAX_STRATA, "WSAE_SAMPLE_MAX_KEEP": N.SAMPLE_MAX_KEEP}
    assert N.PROFILE_BINS == PO.BINS
    for name in ("ActivationProfile", "ActivationSampler", "ProfileSummary", "SampledActivations", "DensityHistogram",
                 "collect_activation_profile", "collect_activation_samples", "top_profile_features"):
        assert name in A.__all__ and hasattr(A, name)


# ---- the Python layer ---------------------------------------------------------------------------------------------------------
def test_python_layer_argument_errors():
    import torch

    from whisper_sae import _native as N
    from whisper_sae.analysis import (ActivationProfile, ActivationSampler, collect_activation_profile,
                                      collect_activation_samples)
    from whisper_sae.analysis.profile import histogram_quantile
    from whisper_sae.sae.model import ReLUSAE
    code = (torch.ones(2, 3, 2), torch.zeros(2, 3, 2, dtype=torch.int32))
    for make in (lambda **kw: ActivationProfile(8, **kw), lambda **kw: ActivationSampler(8, **kw)):
        with pytest.raises(N.WsaeError):
            make().update(code)  # CPU tensors
        with pytest.raises(TypeError):
            make().update(torch.ones(2, 3, 2))
        with pytest.raises(ValueError):
            make(f_window=(4, 5))
    with pytest.raises(N.WsaeError):
        ActivationProfile(8, device="cpu").summary()
    with pytest.raises(N.WsaeError):
        ActivationSampler(8, device="cpu").examples(0)
    with pytest.raises(ValueError):
        ActivationProfile(0)
    with pytest.raises(ValueError):
        ActivationProfile(8).merge(ActivationProfile(9))
    with pytest.raises(ValueError):
        ActivationProfile(8).merge(ActivationProfile(8, f_window=(0, 4)))
    for kw in (dict(keep=0), dict(keep=65), dict(seed=-1), dict(seed=2 ** 32), dict(ordinal_base=-1), dict(ordinal_base=2 ** 31),
               dict(edges=torch.zeros(7, 2)), dict(edges=torch.zeros(8, 16)), dict(edges=torch.zeros(8)), dict(edges=[0.5])):
        with pytest.raises(ValueError):
            ActivationSampler(8, **kw)
    with pytest.raises(ValueError):
        ActivationSampler(8, f_window=(2, 4)).examples(1)
    edges = torch.tensor([[0.5, 1.0]] * 8)
    for other in (ActivationSampler(8, edges, seed=1), ActivationSampler(8, edges, keep=4), ActivationSampler(8, edges + 1),
                  ActivationSampler(8), ActivationSampler(9, torch.tensor([[0.5, 1.0]] * 9))):
        with pytest.raises(ValueError):
            ActivationSampler(8, edges).merge(other)
    a, b = ActivationSampler(8, edges), ActivationSampler(8, edges, ordinal_base=5)
    a._next, b._next = 10, 20  # (as after updates of 10 and 15 frames)
    with pytest.raises(ValueError, match="overlap"):
        a.merge(b)
    with pytest.raises(ValueError):
        histogram_quantile(torch.zeros(2, 192, dtype=torch.int32), torch.zeros(2, dtype=torch.int32),
                           torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), 1.5)
    for collect in (collect_activation_profile, lambda m, u: collect_activation_samples(m, u, None)):
        with pytest.raises(TypeError):
            collect(ReLUSAE(16, 32), [torch.zeros(2, 4, 16)])


def test_merging_samplers_with_nan_edges_and_disjoint_ordinals_needs_no_gpu_until_there_is_state():
    import torch

    from whisper_sae.analysis import ActivationSampler
    edges = torch.tensor([[float("nan")] * 2, [0.5, 1.0]])
    a, b = ActivationSampler(2, edges), ActivationSampler(2, edges.clone(), ordinal_base=100)
    a._next, b._next = 40, 130
    a._records, b._records = [(0, 2, 20)], [(100, 3, 10)]
    a.merge(b)  # (neither has state: only the bookkeeping moves)
    assert (a.ordinal_base, a._next) == (0, 130) and a._records == [(0, 2, 20), (100, 3, 10)]
    utt, frame = a._locate(torch.tensor([0, 19, 20, 39, 40, 99, 100, 109, 110, 129, 130]))
    assert utt.tolist() == [0, 0, 1, 1, -1, -1, 2, 2, 3, 4, -1] and frame.tolist() == [0, 19, 0, 19, -1, -1, 0, 9, 0, 9, -1]


def test_readers_on_the_oracles_integer_state():
    import torch

    from whisper_sae.analysis.profile import bin_lower_edge, histogram_quantile
    assert np.array_equal(bin_lower_edge(torch.arange(193)).numpy(), PO.bin_lower(np.arange(193)))
    (vals, idx), seg = PO.general_case()
    st = PO.profile((vals, idx), seg, PO.HIDDEN)
    t = {k: torch.from_numpy(v) for k, v in st.items()}
    r, f, v, _ = PO.first_active((vals, idx), seg, PO.HIDDEN)
    for q in (0.0, 0.1, 0.25, 0.5, 0.9, 0.99, 1.0):
        got = histogram_quantile(t["hist"], t["fires"], t["min_bits"], t["max_bits"], q).numpy()
        want = PO.quantile(st, q)
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0, equal_nan=True)
        for feat in np.nonzero(st["fires"] > 0)[0]:
            # accurate to one bin: the result lies in the bin of an order statistic next to rank q N (or at its edge)
            mine = np.sort(v[f == feat].astype(np.float64))
            pos = q * mine.size
            near = mine[max(int(np.ceil(pos)) - 1, 0)]
            if np.isfinite(near) and np.isfinite(want[feat]):
                assert abs(int(PO.bin_of(np.float32(want[feat]))) - int(PO.bin_of(np.float32(near)))) <= 1, (q, feat)
    assert np.isnan(PO.quantile(st, 0.5)[PO.SILENT])
    vmin, vmax = PO.bits_to_value(st["min_bits"], st["fires"]), PO.bits_to_value(st["max_bits"], st["fires"])
    fired = st["fires"] > 0
    assert np.array_equal(PO.quantile(st, 0.0)[fired], vmin[fired]) and np.array_equal(PO.quantile(st, 1.0)[fired], vmax[fired])
    # hand-worked: 4 values in one bin [1, 1.125), min 1.0, max 1.0625 -> the median is half way between them
    one = PO.profile(code_of([[(0, 1.0)], [(0, 1.03125)], [(0, 1.0625)], [(0, 1.046875)]], 1), None, 1)
    assert PO.quantile(one, 0.5)[0] == 1.03125 and PO.quantile(one, 0.25)[0] == 1.015625
    # {1.0, 1.0} in bin 96 = [1, 1.125) and 2.0, 3.0 in bins 104, 108: the median is the upper edge of bin 96 (one bin off
    # the sample median 1.5 at most), q = 0.75 the upper edge of bin 104 = [2, 2.25)
    two = PO.profile(code_of([[(0, 1.0)], [(0, 1.0)], [(0, 2.0)], [(0, 3.0)]], 1), None, 1)
    assert PO.quantile(two, 0.5)[0] == 1.125 and PO.quantile(two, 0.25)[0] == 1.0625 and PO.quantile(two, 0.75)[0] == 2.25 and PO.quantile(two, 1.0)[0] == 3.0
    summ = PO.summary(two)
    assert summ["mean"][0] == 1.75 and summ["density"][0] == 1.0 and summ["max"][0] == 3.0 and summ["min"][0] == 1.0
