"""Group effect sizes on the MI355X: ``wsae_pool_update`` bit for bit against the sequential-float32 oracle of
tests/group_stats_oracle.py with nothing excluded, ``wsae_group_effect`` against its float64 oracle at
rtol 1e-9 / atol 1e-12 on every output (both sides are fp64 and sums of at most 4096 terms differ by their order alone,
about 5e-13 relative; tests/test_group_stats.py checks that the oracle agrees with itself to this bound on the same
inputs), the planted columns and bit-level properties, and the Python layer on real modules."""

from __future__ import annotations

import tempfile

import numpy as np
import pytest
import torch

import group_stats_oracle as GO
from whisper_sae import _native as N
from whisper_sae.analysis import (SegmentPooler, bootstrap_weights, collect_pooled, group_effect_sizes,
                                  top_group_features)
from whisper_sae.sae.model import BatchTopKSAE, TopKSAE

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
JUNK_F, JUNK_I = 123.25, 0x5a5a5a5


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype.itemsize == 4 else np.int64)


class PoolState:
    """Device state of the C ABI: sums / counts [n_seg, ld] (columns from f_cols on hold junk), the rows per segment."""

    def __init__(self, hidden, n_seg, f_lo=0, f_cols=None, ld=None, with_cnt=True):
        self.hidden, self.n_seg, self.f_lo = hidden, n_seg, f_lo
        self.f_cols = hidden - f_lo if f_cols is None else f_cols
        self.ld = self.f_cols if ld is None else ld
        self.sums = torch.zeros(n_seg, self.ld, dtype=torch.float32, device=DEV)
        self.sums[:, self.f_cols:] = JUNK_F
        self.cnt = None
        if with_cnt:
            self.cnt = torch.zeros(n_seg, self.ld, dtype=torch.int32, device=DEV)
            self.cnt[:, self.f_cols:] = JUNK_I
        self.rows = torch.zeros(n_seg, dtype=torch.int32, device=DEV)

    def update(self, code, seg):
        v, i, s = dev(code[0]), dev(code[1]), dev(np.asarray(seg, np.int32))
        lib = N.lib()
        need = lib.wsae_pool_workspace_bytes(v.shape[0], v.shape[1], self.hidden, self.n_seg, self.f_lo, self.f_cols)
        assert need == 8 * self.n_seg
        ws = torch.full((need,), 0xAB, dtype=torch.uint8, device=DEV)  # (arbitrary contents on entry)
        N.check(lib.wsae_pool_update(v.data_ptr(), i.data_ptr(), v.shape[1], self.hidden, s.data_ptr(), v.shape[0], self.n_seg,
                                     self.f_lo, self.f_cols, self.sums.data_ptr(), N.ptr(self.cnt), self.ld,
                                     self.rows.data_ptr(), ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream),
                "wsae_pool_update")
        torch.cuda.synchronize()
        return self

    def check(self, want):
        """Sums (bits), counts and rows equal the oracle's; the padding columns still hold the junk."""
        sums = self.sums[:, :self.f_cols].cpu().numpy()
        assert np.array_equal(bits(sums), bits(want[0])), np.argwhere(bits(sums) != bits(want[0]))[:5]
        assert np.array_equal(self.rows.cpu().numpy(), want[2])
        assert bool((self.sums[:, self.f_cols:] == JUNK_F).all())
        if self.cnt is not None:
            assert np.array_equal(self.cnt[:, :self.f_cols].cpu().numpy(), want[1])
            assert bool((self.cnt[:, self.f_cols:] == JUNK_I).all())


def uneven_segments(rng, rows, n_seg):
    """Non-decreasing ids over ``rows`` rows, every segment present, the first three of length 1 where there is room."""
    if n_seg == 1:
        return np.zeros(rows, np.int32)
    cuts = np.sort(rng.choice(np.arange(4, rows), n_seg - 4, replace=False)) if n_seg > 4 else np.array([], np.int64)
    starts = np.concatenate([[0, 1, 2, 3][:min(4, n_seg)], cuts]).astype(np.int64)
    seg = np.zeros(rows, np.int32)
    seg[starts[1:]] = 1
    return np.cumsum(seg).astype(np.int32)


# (rows, k, hidden, n_seg, ld - f_cols): one row; odd sizes with segments of length 1; one long segment (the in-order sum
# crosses every block of four rows); seven segments with padding columns; more segments than the grid (2560 workgroups);
# k = 128 (two passes of the lanes per row); 4000 features (two feature tiles of 3072 per segment)
POOL = [(1, 1, 32, 1, 0), (257, 5, 96, 9, 0), (3000, 32, 3072, 1, 0), (4099, 32, 3072, 7, 5), (6000, 3, 40, 5000, 0),
        (600, 128, 256, 4, 0), (300, 16, 4000, 3, 3)]


@pytest.fixture(scope="module")
def pool_cases():
    out = {}
    for n, (rows, k, hidden, n_seg, _) in enumerate(POOL):
        rng = np.random.default_rng(300 + n)
        code = GO.random_code(rng, rows, k, hidden)
        while not ((code[0] > 0) & (code[1] >= 0) & (code[1] < hidden)).any():  # the one-entry case: draw an active entry
            code = GO.random_code(rng, rows, k, hidden)
        seg = np.sort(rng.integers(0, n_seg, rows)).astype(np.int32) if n_seg > rows // 2 else uneven_segments(rng, rows, n_seg)
        out[POOL[n]] = (code, seg, GO.pool(code, hidden, seg, n_seg))
    return out


@pytest.mark.parametrize("case", POOL, ids=lambda c: "x".join(str(v) for v in c))
def test_pool_equals_the_oracle(pool_cases, case):
    code, seg, want = pool_cases[case]
    _, _, hidden, n_seg, pad = case
    PoolState(hidden, n_seg, ld=hidden + pad).update(code, seg).check(want)
    assert want[0].max() > 0 and want[2].sum() == case[0]


def test_pool_without_counts_and_twice(pool_cases):
    code, seg, want = pool_cases[POOL[1]]
    a = PoolState(96, 9, ld=101, with_cnt=False).update(code, seg)
    a.check(want)
    b = PoolState(96, 9, with_cnt=False).update(code, seg)
    assert torch.equal(a.sums[:, :96].view(torch.int32), b.sums.view(torch.int32))


def test_pool_padding_rows(pool_cases):
    code, seg, _ = pool_cases[POOL[1]]
    seg = seg.copy()
    seg[:3] = -1                # at the start
    seg[100:104] = -1           # in the middle of a segment
    seg[130] = -7
    seg[-2:] = -1               # at the end
    seg[200:203] = 9            # >= n_seg
    seg[203] = 2 ** 31 - 1
    want = GO.pool(code, 96, seg, 9)
    assert want[2].sum() == 257 - 14
    PoolState(96, 9, ld=99).update(code, seg).check(want)
    none = PoolState(96, 9).update(code, np.full(257, -1, np.int32))
    none.check((np.zeros((9, 96), np.float32), np.zeros((9, 96), np.int32), np.zeros(9, np.int32)))


@pytest.mark.parametrize("window", [(40, 17), (0, 32), (95, 1)], ids=lambda w: f"{w[0]}+{w[1]}")
def test_pool_window_equals_the_slice(pool_cases, window):
    code, seg, want = pool_cases[POOL[1]]
    lo, span = window
    st = PoolState(96, 9, f_lo=lo, f_cols=span, ld=span + 2).update(code, seg)
    st.check((want[0][:, lo:lo + span], want[1][:, lo:lo + span], want[2]))
    st.check(GO.pool(code, 96, seg, 9, f_lo=lo, f_cols=span))
    big, bseg, bwant = pool_cases[POOL[6]]  # a window across the tile boundary of the full table
    PoolState(4000, 3, f_lo=3000, f_cols=200).update(big, bseg).check((bwant[0][:, 3000:3200], bwant[1][:, 3000:3200], bwant[2]))


def test_pool_segment_split_over_calls(pool_cases):
    for case, cuts in ((POOL[1], (0, 1, 130, 257)), (POOL[2], (0, 1001, 1002, 3000))):
        code, seg, want = pool_cases[case]
        st = PoolState(case[2], case[3])
        for lo, hi in zip(cuts[:-1], cuts[1:]):  # the cuts fall inside segments
            st.update((code[0][lo:hi], code[1][lo:hi]), seg[lo:hi])
        st.check(want)
    # the oracle continues from a state as well: sums that did not start at zero
    code, seg, _ = pool_cases[POOL[1]]
    first = GO.pool(code, 96, seg, 9)
    PoolState(96, 9).update(code, seg).update(code, seg).check(GO.pool(code, 96, seg, 9, state=first))


# ---- effect sizes ------------------------------------------------------------------------------------------------------
def run_effect(X, group, div=None, boot=None, alpha=0.05, ld=None, f_cols=None):
    """``wsae_group_effect`` on numpy inputs -> dict of GO.FIELDS (float64 [f_cols]) and ``record``."""
    S, F = X.shape
    f_cols = F if f_cols is None else f_cols
    ld = F if ld is None else ld
    Xd = torch.full((S, ld), JUNK_F, dtype=torch.float32, device=DEV)
    Xd[:, :F] = dev(np.asarray(X, np.float32))
    g = dev(np.asarray(group, np.int32))
    dv = None if div is None else dev(np.asarray(div, np.int32))
    b = None if boot is None else dev(np.asarray(boot, np.int16))
    R = 0 if boot is None else boot.shape[0]
    lib = N.lib()
    need = lib.wsae_group_effect_workspace_bytes(S, f_cols, R)
    assert need > 0
    ws = torch.full((need,), 0xAB, dtype=torch.uint8, device=DEV)
    out = torch.full((7, f_cols), 777.0, dtype=torch.float64, device=DEV)
    rec = torch.full((3,), -7, dtype=torch.int32, device=DEV)
    o = [out[i].data_ptr() for i in range(7)]
    N.check(lib.wsae_group_effect(Xd.data_ptr(), ld, N.ptr(dv), g.data_ptr(), S, f_cols, N.ptr(b), R, alpha, *o, rec.data_ptr(),
                                  ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream), "wsae_group_effect")
    torch.cuda.synchronize()
    res = {k: out[i].cpu().numpy() for i, k in enumerate(GO.FIELDS)}
    res["record"] = tuple(int(v) for v in rec.cpu())
    return res


def check_effect(got, want, what=""):
    assert got["record"] == want["record"], (got["record"], want["record"])
    worst = 0.0
    for k in GO.FIELDS:
        both = np.isfinite(got[k]) & np.isfinite(want[k])
        if both.any():
            worst = max(worst, float(np.max(np.abs(got[k] - want[k])[both] / (GO.ATOL / GO.RTOL + np.abs(want[k][both])))))
    print(f"group effect {what}: largest |got - want| / (1e-3 + |want|) = {worst:.3e}")
    for k in GO.FIELDS:
        np.testing.assert_allclose(got[k], want[k], rtol=GO.RTOL, atol=GO.ATOL, equal_nan=True, err_msg=f"{what} {k}")


@pytest.fixture(scope="module")
def effect_cases():
    out = {}
    for shape in GO.EFFECT_SHAPES:
        X, div, group, boot = GO.effect_case(shape)
        out[shape] = (X, div, group, boot, GO.effect(X, group, div, boot))
    return out


@pytest.mark.parametrize("shape", GO.EFFECT_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_effect_equals_the_oracle(effect_cases, shape):
    X, div, group, boot, want = effect_cases[shape]
    ld = shape[1] + 7 if shape == (4096, 3072, 64) else None
    got = run_effect(X, group, div, boot, ld=ld)
    check_effect(got, want, str(shape))
    assert got["record"][2] == shape[2]
    if boot is None:
        assert all(np.all(np.isnan(got[k])) for k in ("ci_lo", "ci_hi", "se")) and np.all(np.isfinite(got["d"]))
    else:
        assert np.all(got["ci_lo"] <= got["ci_hi"]) and np.all(got["se"] >= 0)


def test_effect_planted_columns_and_bit_properties(effect_cases):
    X, div, group, boot, _ = effect_cases[(257, 96, 1000)]
    X = X.copy()
    X[:, 5] = 0.0                   # never fires
    X[group == 1, 6] = 0.0          # fires in group a only
    X[:, 70] = X[:, 7]              # a twin in another tile of four (and another slot of it)
    X[:, 41] = X[:, 7]
    want = GO.effect(X, group, div, boot)
    got = run_effect(X, group, div, boot)
    check_effect(got, want, "planted")
    for k in GO.FIELDS:
        assert got[k][5] == 0.0, k  # exactly
    assert got["mean_b"][6] == 0.0 and got["mean_a"][6] > 0 and got["d"][6] > 0 and got["ci_lo"][6] > 0
    for k in GO.FIELDS:
        assert bits(got[k])[70] == bits(got[k])[7] == bits(got[k])[41], k
    # the same matrix under another ld and a narrower window; a second call
    narrow = run_effect(X[:, :50], group, div, boot, ld=131, f_cols=50)
    again = run_effect(X, group, div, boot)
    for k in GO.FIELDS:
        assert np.array_equal(bits(narrow[k]), bits(got[k])[:50]), k
        assert np.array_equal(bits(again[k]), bits(got[k])), k
    assert narrow["record"] == got["record"] == again["record"]
    # alpha moves the interval only
    wide = run_effect(X, group, div, boot, alpha=0.5)
    check_effect(wide, GO.effect(X, group, div, boot, alpha=0.5), "alpha 0.5")
    assert np.array_equal(bits(wide["d"]), bits(got["d"])) and np.all(wide["ci_lo"] >= got["ci_lo"])


def test_effect_weights_rules(effect_cases):
    X, div, group, boot, _ = effect_cases[(257, 96, 1000)]
    inc = np.where(div > 0, group, -1)
    rng = np.random.default_rng(77)
    bal = GO.stratified_weights(rng, inc, 300, balanced=True)
    n_min = min(int((inc == 0).sum()), int((inc == 1).sum()))
    assert np.all(bal[:, inc == 0].sum(1) == n_min) and np.all(bal[:, inc == 1].sum(1) == n_min)
    check_effect(run_effect(X, group, div, bal), GO.effect(X, group, div, bal), "balanced")
    # negative weights count as zero; weights on ignored utterances count for nothing
    neg = boot[:64].copy()
    flip = rng.random(neg.shape) < 0.1
    zeroed = np.where(flip, 0, neg)
    neg[flip] = -neg[flip] - 1
    neg[:, inc < 0] = 5
    a, b = run_effect(X, group, div, neg), run_effect(X, group, div, zeroed.astype(np.int16))
    check_effect(a, GO.effect(X, group, div, neg), "negative weights")
    assert all(np.array_equal(bits(a[k]), bits(b[k])) for k in GO.FIELDS)
    # a replicate with N < 2 in a group is dropped, and the record says so
    drop = boot[:50].copy()
    drop[3, inc == 0] = 0
    drop[3, np.nonzero(inc == 0)[0][0]] = 1     # N_a = 1
    drop[10, inc == 1] = 0                      # N_b = 0
    drop[20, inc == 1] = -2                     # N_b = 0 after clamping
    got = run_effect(X, group, div, drop)
    assert got["record"][2] == 47
    check_effect(got, GO.effect(X, group, div, drop), "dropped replicates")
    # every replicate dropped: the point statistics stand, the interval is NaN
    dead = run_effect(X, group, div, np.zeros((4, 257), np.int16))
    assert dead["record"][2] == 0 and np.all(np.isnan(dead["ci_lo"])) and np.all(np.isnan(dead["se"]))
    assert np.array_equal(bits(dead["d"]), bits(got["d"]))


def test_effect_with_fewer_than_two_members_is_nan(effect_cases):
    X, div, group, boot, _ = effect_cases[(5, 33, 7)]
    div = div.copy()
    div[2], div[0] = 6, 0  # the utterance without frames is now a member of group a: n_a = 1
    got = run_effect(X, group, div, boot)
    assert got["record"][:2] == (1, 2) and all(np.all(np.isnan(got[k])) for k in GO.FIELDS)
    check_effect(got, GO.effect(X, group, div, boot), "n_a = 1")
    point = run_effect(X, [0, 1, 1, 1, 1], None, None)
    assert point["record"] == (1, 4, 0) and all(np.all(np.isnan(point[k])) for k in GO.FIELDS)


# ---- the Python layer --------------------------------------------------------------------------------------------------
D, H, K, UTT, T = 64, 256, 8, 12, 40
LABELS = [0, 1, 1, 0, 2, 1, 0, 0, 1, 1, 0, 2]


def utterances(seed):
    """12 utterances of 40 frames in three batches, with a frame mask.  Each utterance speaks the same 24 frames at its
    own loudness per frame (the rest is masked or silence-like repetition): a feature then fires in every utterance or in
    none, so that no bootstrap replicate is a ratio of rounding errors, while the values differ between utterances."""
    gen = torch.Generator().manual_seed(seed)
    proto = torch.randn(24, D, generator=gen)
    x = proto[torch.arange(T) % 24][None].repeat(UTT, 1, 1) * (0.5 + torch.rand(UTT, T, 1, generator=gen))
    mask = torch.ones(UTT, T)
    for u in range(UTT):
        mask[u, 24 + (u % 5) * 3:] = 0  # utterances of different lengths: the tail is padding
    mask[3, 30] = 0
    return [(x[:5], mask[:5]), (x[5:6], mask[5:6]), (x[6:], mask[6:])], mask


def make_sae(cls, seed, **kw):
    torch.manual_seed(seed)
    sae = cls(D, H, k=K, **kw).to(DEV)
    with torch.no_grad():
        sae.encoder.bias.zero_()  # scaling a frame then keeps its selection
    return sae


@pytest.mark.parametrize("kind", ["topk", "batch_topk"])
def test_python_layer_on_real_modules(kind):
    sae = make_sae(TopKSAE, 1) if kind == "topk" else make_sae(BatchTopKSAE, 2, max_k_per_row=16)
    batches, mask = utterances(5)
    sae.train()
    pooler = collect_pooled(sae, batches, counts=True)
    assert sae.training and pooler.n_segments == UTT
    # the oracle on the codes the module emits
    sae.eval()
    codes = [sae.encode_compact(x.to(DEV)) for x, _ in batches]
    vals, idx = (np.concatenate([c[i].cpu().numpy() for c in codes]) for i in (0, 1))
    seg = np.where(mask.reshape(-1).numpy() != 0, np.repeat(np.arange(UTT), T), -1)
    sums, cnt, rows = GO.pool((vals, idx), H, seg, UTT)
    assert np.array_equal(bits(pooler.sums.cpu().numpy()), bits(sums)) and np.array_equal(pooler.counts.cpu().numpy(), cnt)
    assert np.array_equal(pooler.frames.cpu().numpy(), rows) and rows.tolist() == mask.sum(1).int().tolist()
    assert np.allclose(pooler.means().cpu().numpy(), sums.astype(np.float64) / rows[:, None], rtol=1e-15)
    assert np.array_equal(pooler.rates().cpu().numpy(), cnt.astype(np.float64) / rows[:, None])
    group = np.array([l if l < 2 else -1 for l in LABELS])
    boot = bootstrap_weights(LABELS, 200, seed=9)
    for use, X, div in (("mean", sums, rows), ("sum", sums, None), ("rate", cnt.astype(np.float32), rows)):
        eff = group_effect_sizes(pooler, LABELS, n_boot=200, seed=9, use=use)
        want = GO.effect(X, group, div, boot.numpy())
        got = {k: getattr(eff, k).cpu().numpy() for k in GO.FIELDS}
        got["record"] = (eff.n_a, eff.n_b, eff.n_boot)
        check_effect(got, want, f"{kind} {use}")
        assert (eff.n_a, eff.n_b, eff.n_boot) == (5, 5, 200) and eff.d.dtype == torch.float64
    # a dense matrix in place of the pooler; other group names; point statistics only
    eff = group_effect_sizes(pooler, LABELS, n_boot=200, seed=9, use="sum")
    dense = group_effect_sizes(pooler.sums.clone(), LABELS, n_boot=200, seed=9)
    swapped = group_effect_sizes(pooler, LABELS, group_a=1, group_b=0, n_boot=0, use="sum")
    for k in GO.FIELDS:
        assert torch.equal(getattr(dense, k).view(torch.int64), getattr(eff, k).view(torch.int64)), k
    assert torch.allclose(swapped.d, -eff.d, rtol=1e-14, atol=0) and bool(torch.isnan(swapped.ci_lo).all())
    assert swapped.n_boot == 0 and torch.equal(swapped.mean_a, eff.mean_b)
    # the CI filter
    idx_f, g_f = top_group_features(eff, n=10)
    idx_all, g_all = top_group_features(eff, n=10, require_ci_excludes_zero=False)
    assert idx_all.numel() == 10 and idx_f.numel() <= 10
    assert bool(((eff.ci_lo[idx_f] > 0) | (eff.ci_hi[idx_f] < 0)).all())
    assert bool((g_all.abs()[:-1] >= g_all.abs()[1:]).all()) and torch.equal(g_all, eff.g[idx_all])
    fired = torch.from_numpy(sums.sum(0) > 0).to(DEV)
    assert bool(fired[idx_all].all())  # a feature that never fires has g = 0 exactly and cannot lead
    assert bool((eff.g[~fired] == 0).all()) and bool((eff.se[~fired] == 0).all())
    # save / load, and a loaded pooler goes on pooling
    with tempfile.TemporaryDirectory(prefix="wsae_pool_") as d:
        pooler.save(f"{d}/p.pt")
        back = SegmentPooler.load(f"{d}/p.pt", device=DEV)
    assert torch.equal(back.sums.view(torch.int32), pooler.sums.view(torch.int32)) and torch.equal(back.counts, pooler.counts)
    assert torch.equal(back.frames, pooler.frames) and back._next == UTT
    with pytest.raises(ValueError):
        back.update(codes[1] if codes[1][0].dim() == 3 else tuple(t.reshape(1, T, -1) for t in codes[1]))  # a 13th utterance
    flat = SegmentPooler(H, UTT, f_window=(64, 100), device=DEV)
    flat.update((dev(vals), dev(idx)), segments=dev(seg.astype(np.int32)))
    assert torch.equal(flat.sums.view(torch.int32), pooler.sums[:, 64:164].view(torch.int32))
    with pytest.raises(N.WsaeError):
        flat.update((torch.from_numpy(vals), torch.from_numpy(idx)), segments=torch.from_numpy(seg))
    with pytest.raises(ValueError):
        flat.counts
