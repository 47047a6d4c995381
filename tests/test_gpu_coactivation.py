"""Co-activation statistics on the MI355X: ``wsae_coact_update`` and ``wsae_coact_top`` against the integer / float64
oracle of tests/coactivation_oracle.py, bit for bit with nothing excluded - shapes on every path of the update, mask,
padding, self mode, windows, contention, call splits and row order, all four scores with planted ties, degenerate
marginals and int64-sized numerators - and the Python layer on real modules."""

from __future__ import annotations

import json
import tempfile

import numpy as np
import pytest
import torch

import coactivation_oracle as CO
from whisper_sae import _native as N
from whisper_sae.analysis import CoactivationTracker, collect_coactivation, compare_activations
from whisper_sae.config import TrainingConfig
from whisper_sae.sae.model import BatchTopKSAE, TopKSAE
from whisper_sae.sae.training import SAETrainer

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
METRIC = {"count": N.COACT_COUNT, "cond": N.COACT_COND, "jaccard": N.COACT_JACCARD, "phi": N.COACT_PHI}


def random_code(rng, rows, k, hidden):
    """A random code: about a third of the values <= 0, some exactly 0, a few indices -1 and >= hidden."""
    idx = rng.integers(0, hidden, (rows, k)).astype(np.int32)
    vals = (rng.standard_normal((rows, k)) + 0.45).astype(np.float32)
    vals[rng.random((rows, k)) < 0.05] = 0.0
    bad = rng.random((rows, k)) < 0.01
    idx[bad] = rng.choice(np.array([-1, hidden, hidden + 9, -5], np.int32), int(bad.sum()))
    return vals, idx


class State:
    """Device state of the C ABI: counts [a_rows, ldc] (columns from hidden_b on hold junk), the marginals, the total."""

    JUNK = 0x5a5a5a5

    def __init__(self, hidden_a, hidden_b, a_lo=0, a_rows=None, ldc=None, with_fire_b=True):
        self.ha, self.hb, self.a_lo = hidden_a, hidden_b, a_lo
        self.a_rows = hidden_a - a_lo if a_rows is None else a_rows
        self.ldc = hidden_b if ldc is None else ldc
        self.counts = torch.zeros(self.a_rows, self.ldc, dtype=torch.int32, device=DEV)
        self.counts[:, hidden_b:] = self.JUNK
        self.fire_a = torch.zeros(hidden_a, dtype=torch.int32, device=DEV)
        self.fire_b = torch.zeros(hidden_b, dtype=torch.int32, device=DEV) if with_fire_b else None
        self.total = torch.zeros(1, dtype=torch.int64, device=DEV)

    def update(self, code_a, code_b=None, mask=None):
        va, ia = (torch.from_numpy(np.ascontiguousarray(t)).to(DEV) for t in code_a)
        vb, ib = (va, ia) if code_b is None else (torch.from_numpy(np.ascontiguousarray(t)).to(DEV) for t in code_b)
        m = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask, dtype=np.uint8)).to(DEV)
        lib = N.lib()
        assert lib.wsae_coact_workspace_bytes(va.shape[0], va.shape[1], self.ha, vb.shape[1], self.hb, self.a_lo,
                                              self.a_rows) == 0
        N.check(lib.wsae_coact_update(va.data_ptr(), ia.data_ptr(), va.shape[1], self.ha, vb.data_ptr(), ib.data_ptr(),
                                      vb.shape[1], self.hb, va.shape[0], N.ptr(m), self.a_lo, self.a_rows,
                                      self.counts.data_ptr(), self.ldc, self.fire_a.data_ptr(), N.ptr(self.fire_b),
                                      self.total.data_ptr(), None, 0, torch.cuda.current_stream().cuda_stream),
                "wsae_coact_update")
        torch.cuda.synchronize()
        return self

    def host(self):
        return (self.counts[:, :self.hb].cpu().numpy(), self.fire_a.cpu().numpy(),
                None if self.fire_b is None else self.fire_b.cpu().numpy(), int(self.total.item()))

    def check(self, want):
        """Everything equals the oracle's (counts, fire_a, fire_b, rows) and the padding columns still hold the junk."""
        counts, fa, fb, rows = self.host()
        assert np.array_equal(counts, want[0]), np.argwhere(counts != want[0])[:5]
        assert np.array_equal(fa, want[1]) and rows == want[3]
        if fb is not None:
            assert np.array_equal(fb, want[2])
        assert bool((self.counts[:, self.hb:] == self.JUNK).all())


def same_state(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a.host(), b.host()))


# ---- 1. update ---------------------------------------------------------------------------------------------------------
# (rows, k_a, k_b, H_a, H_b, ldc): one wave and one pair; odd sizes with k below and at half a wave's width; k = 128 (two
# passes over the lanes per code, 16384 pairs per row); 1025 workgroups with ldc > H_b.  The grid-stride loop (more than
# 4 waves x 2048 workgroups of rows) has its own case below.
UPDATE = [(1, 1, 1, 32, 32, 32), (257, 5, 32, 96, 160, 160), (1000, 128, 128, 256, 128, 128),
          (4099, 32, 32, 3072, 3072, 3077)]


@pytest.fixture(scope="module")
def update_cases():
    out = {}
    for n, (rows, ka, kb, ha, hb, ldc) in enumerate(UPDATE):
        rng = np.random.default_rng(200 + n)
        a, b = random_code(rng, rows, ka, ha), random_code(rng, rows, kb, hb)
        out[(rows, ka, kb, ha, hb, ldc)] = (a, b, CO.accumulate(a, ha, b, hb))
    return out


@pytest.mark.parametrize("case", UPDATE, ids=lambda c: "x".join(str(v) for v in c))
def test_update_equals_the_oracle(update_cases, case):
    a, b, want = update_cases[case]
    _, _, _, ha, hb, ldc = case
    State(ha, hb, ldc=ldc).update(a, b).check(want)


def test_grid_stride_rows():
    rng = np.random.default_rng(11)
    a, b = random_code(rng, 20000, 3, 40), random_code(rng, 20000, 2, 24)  # 20000 rows > 4 waves x 2048 workgroups
    State(40, 24).update(a, b).check(CO.accumulate(a, 40, b, 24))


def test_row_mask_and_padding_columns(update_cases):
    a, b, _ = update_cases[UPDATE[1]]
    mask = (np.random.default_rng(3).random(257) < 0.6).astype(np.uint8)
    mask[::50] = 7  # any non-zero flag counts
    want = CO.accumulate(a, 96, b, 160, row_mask=mask)
    assert 0 < want[3] < 257
    State(96, 160, ldc=167).update(a, b, mask).check(want)
    none = State(96, 160, ldc=167).update(a, b, np.zeros(257, np.uint8))
    none.check((np.zeros((96, 160)), np.zeros(96), np.zeros(160), 0))


def test_self_mode_is_symmetric_with_the_marginals_on_the_diagonal(update_cases):
    a, _, _ = update_cases[UPDATE[1]]
    want = CO.accumulate(a, 96, a, 96)
    st = State(96, 96, with_fire_b=False).update(a)  # fire_b = NULL is accepted
    st.check(want)
    counts, fa, _, _ = st.host()
    assert np.array_equal(counts, counts.T)
    # (the oracle's rule for a repeated index, k_a = 5 from 96: the diagonal counts pairs of occurrences)
    assert np.array_equal(np.diag(counts), np.diag(want[0])) and np.all(np.diag(counts) >= fa)
    rng = np.random.default_rng(8)
    idx = np.stack([rng.permutation(96)[:5] for _ in range(300)]).astype(np.int32)  # a TopK code: no repeats
    code = ((rng.standard_normal((300, 5)) + 0.4).astype(np.float32), idx)
    counts, fa, _, _ = State(96, 96, with_fire_b=False).update(code).host()
    assert np.array_equal(counts, counts.T) and np.array_equal(np.diag(counts), fa)


@pytest.mark.parametrize("window", [(0, 32), (40, 17), (0, 96)], ids=lambda w: f"{w[0]}+{w[1]}")
def test_window_equals_the_slice_of_the_full_table(update_cases, window):
    a, b, want = update_cases[UPDATE[1]]
    lo, span = window
    st = State(96, 160, a_lo=lo, a_rows=span).update(a, b)
    st.check((want[0][lo:lo + span], want[1], want[2], want[3]))
    st.check(CO.accumulate(a, 96, b, 160, a_lo=lo, a_rows=span))


def test_contention():
    rng = np.random.default_rng(5)
    ia = np.tile(rng.permutation(64)[:8].astype(np.int32), (4096, 1))
    ib = np.tile(rng.permutation(48)[:6].astype(np.int32), (4096, 1))
    a, b = (np.ones_like(ia, dtype=np.float32), ia), (np.ones_like(ib, dtype=np.float32), ib)
    counts, fa, fb, rows = State(64, 48).update(a, b).host()
    want = np.zeros((64, 48), np.int32)
    want[np.ix_(ia[0], ib[0])] = 4096
    assert np.array_equal(counts, want) and rows == 4096  # every touched cell exactly 4096, nothing else
    assert np.array_equal(np.nonzero(fa)[0], np.sort(ia[0])) and np.all(fa[ia[0]] == 4096) and np.all(fb[ib[0]] == 4096)
    # one feature of A active in every row beside random others: its table row is B's firing count
    va, xa = random_code(rng, 3000, 8, 64)
    xa[xa == 7] = 8
    va[:, 0], xa[:, 0] = 1.5, 7
    b = random_code(rng, 3000, 8, 48)
    st = State(64, 48).update((va, xa), b)
    st.check(CO.accumulate((va, xa), 64, b, 48))
    counts, fa, fb, rows = st.host()
    assert fa[7] == 3000 == rows and np.array_equal(counts[7], fb)


def test_call_split_row_order_and_repeatability(update_cases):
    a, b, want = update_cases[UPDATE[1]]
    one = State(96, 160).update(a, b)
    again = State(96, 160).update(a, b)
    three = State(96, 160)
    for lo, hi in ((0, 1), (1, 200), (200, 257)):
        three.update((a[0][lo:hi], a[1][lo:hi]), (b[0][lo:hi], b[1][lo:hi]))
    perm = np.random.default_rng(6).permutation(257)
    shuffled = State(96, 160).update((a[0][perm], a[1][perm]), (b[0][perm], b[1][perm]))
    one.check(want)
    assert same_state(one, again) and same_state(one, three) and same_state(one, shuffled)


# ---- 2. top ------------------------------------------------------------------------------------------------------------
def run_top(counts, fire_a, fire_b, total, metric, n, min_count=1, exclude_self=False, a_lo=0, pad=0, want_cnt=True):
    """``wsae_coact_top`` on a numpy state -> (values, indices, counts) as numpy.  ``pad`` > 0: ldc = hidden_b + pad with
    junk in the padding (pad = 0 and hidden_b % 4 == 0 take the 16-byte loads, anything else the 4-byte ones)."""
    rows, hb = counts.shape
    table = torch.full((rows, hb + pad), 2 ** 31 - 1, dtype=torch.int32, device=DEV)
    table[:, :hb] = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int32)).to(DEV)
    fa = torch.from_numpy(np.ascontiguousarray(fire_a, dtype=np.int32)).to(DEV)
    fb = torch.from_numpy(np.ascontiguousarray(fire_b, dtype=np.int32)).to(DEV)
    tot = torch.tensor([total], dtype=torch.int64, device=DEV)
    vals = torch.full((rows, n), 123.0, dtype=torch.float32, device=DEV)
    idx = torch.full((rows, n), -7, dtype=torch.int32, device=DEV)
    cnt = torch.full((rows, n), -7, dtype=torch.int32, device=DEV) if want_cnt else None
    lib = N.lib()
    assert lib.wsae_coact_top_workspace_bytes(a_lo, rows, hb, n) == 0
    N.check(lib.wsae_coact_top(table.data_ptr(), hb + pad, a_lo, rows, hb, fa.data_ptr(), fb.data_ptr(), tot.data_ptr(),
                               METRIC[metric], min_count, int(exclude_self), n, vals.data_ptr(), idx.data_ptr(), N.ptr(cnt),
                               None, 0, torch.cuda.current_stream().cuda_stream), "wsae_coact_top")
    torch.cuda.synchronize()
    return vals.cpu().numpy(), idx.cpu().numpy(), None if cnt is None else cnt.cpu().numpy()


def check_top(counts, fire_a, fire_b, total, metric, n, **kw):
    """Indices, counts and the bits of the fp32 values equal the oracle's.  A value off by one unit in the last place
    would mean that the fp64 division or root is not correctly rounded: a kernel or flag defect, not a tolerance."""
    okw = {k: v for k, v in kw.items() if k in ("min_count", "exclude_self", "a_lo")}
    want_v, want_i, want_c = CO.top(counts, fire_a, fire_b, total, metric, n, **okw)
    vals, idx, cnt = run_top(counts, fire_a, fire_b, total, metric, n, **kw)
    assert np.array_equal(idx, want_i), np.argwhere(idx != want_i)[:5]
    assert np.array_equal(vals.view(np.uint32), want_v.view(np.uint32)), np.argwhere(vals != want_v)[:5]
    if cnt is not None:
        assert np.array_equal(cnt, want_c)
    return vals, idx, cnt


def fabricated(rng, rows, hb, total, a_lo=0, fill=0.5):
    """A consistent state: 0 <= c <= min(n, m), n, m <= N; row 0 never fired (n = 0), row 1 always did (n = N)."""
    fa = rng.integers(0, total + 1, a_lo + rows)
    fa[a_lo], fa[a_lo + 1] = 0, total
    fb = rng.integers(0, total + 1, hb)
    fb[:2] = (0, total)
    cap = np.minimum(fa[a_lo:, None], fb[None, :])
    counts = (rng.random((rows, hb)) * (cap + 1)).astype(np.int64)
    counts[rng.random((rows, hb)) > fill] = 0
    return np.minimum(counts, cap), fa, fb


@pytest.mark.parametrize("n", [1, 4, 16])
@pytest.mark.parametrize("metric", CO.METRICS)
def test_top_on_a_fabricated_state(metric, n):
    rng = np.random.default_rng(31)
    counts, fa, fb = fabricated(rng, 70, 300, 1000, a_lo=25)  # the window's features 25..94 are columns too
    for min_count in (0, 1, 3):
        for exclude_self in (False, True):
            check_top(counts, fa, fb, 1000, metric, n, min_count=min_count, exclude_self=exclude_self, a_lo=25)
    _, idx, _ = check_top(counts, fa, fb, 1000, metric, n, min_count=0, exclude_self=True, a_lo=25, pad=3)
    assert not np.any(idx == 25 + np.arange(70)[:, None])
    run = run_top(counts, fa, fb, 1000, metric, n, want_cnt=False)  # out_cnt = NULL
    assert np.array_equal(run[1], CO.top(counts, fa, fb, 1000, metric, n)[1])


@pytest.mark.parametrize("metric", CO.METRICS)
def test_top_planted_ties_across_33000_columns(metric):
    rng = np.random.default_rng(32)
    hb, total = 33000, 5000
    counts, fa, fb = fabricated(rng, 3, hb, total, fill=0.002)
    counts = np.minimum(counts, 300)  # (whatever else there is scores below the planted cells under every metric)
    fa[:] = (900, 1200, 0)
    cols = np.array([32999, 5, 20000, 1023, 1024, 16384, 255, 256, 31000, 7777, 12, 29000, 4096, 8191, 3, 25000, 18000, 600])
    fb[cols] = 700
    counts[:, cols] = 650  # equal (c, m) under one n: equal scores in distant columns, above everything else
    counts[2] = 0
    counts[2, cols] = 1    # a row that never fired: every score is 0 there
    for n in (4, 16):
        vals, idx, _ = check_top(counts, fa, fb, total, metric, n, min_count=1)
        assert np.array_equal(idx[0], np.sort(cols)[:n]) and np.array_equal(idx[1], np.sort(cols)[:n])  # lowest index first
        assert np.all(vals[0] == vals[0, 0])
    check_top(counts, fa, fb, total, metric, 16, min_count=0, pad=1)


@pytest.mark.parametrize("metric", CO.METRICS)
def test_top_with_fewer_columns_than_top_n(metric):
    rng = np.random.default_rng(33)
    counts, fa, fb = fabricated(rng, 9, 5, 50, fill=0.8)
    vals, idx, cnt = check_top(counts, fa, fb, 50, metric, 16, min_count=0)
    assert np.all(idx[:, 5:] == -1) and np.all(np.isneginf(vals[:, 5:])) and np.all(cnt[:, 5:] == 0)
    assert np.all(np.sort(idx[:, :5], axis=1) == np.arange(5))
    check_top(counts, fa, fb, 50, metric, 16, min_count=1, exclude_self=True)


@pytest.mark.parametrize("metric", CO.METRICS)
def test_top_with_int64_sized_numerators(metric):
    rng = np.random.default_rng(34)
    total = 2 ** 31 - 1
    rows, hb = 9, 70
    fa = rng.integers(2 ** 29, total, rows)
    fb = rng.integers(2 ** 29, total, hb)
    fa[:3], fb[:3] = (0, total, total - 1), (total, 0, total - 1)
    lo = np.maximum(0, fa[:, None] + fb[None, :] - total)
    hi = np.minimum(fa[:, None], fb[None, :])
    counts = lo + (rng.random((rows, hb)) * (hi - lo + 1)).astype(np.int64)
    counts = np.clip(counts, lo, hi)
    assert counts.max() > 2 ** 30 and (total * counts).max() > 2 ** 61
    for n in (1, 16):
        check_top(counts, fa, fb, total, metric, n, min_count=0)
        check_top(counts, fa, fb, total, metric, n, min_count=3, pad=2)


@pytest.mark.parametrize("metric", CO.METRICS)
def test_top_on_accumulated_states(update_cases, metric):
    for case, n in ((UPDATE[1], 16), (UPDATE[3], 4)):
        _, _, (counts, fa, fb, rows) = update_cases[case]
        check_top(counts, fa, fb, rows, metric, n, min_count=1)
    counts, fa, fb, rows = CO.accumulate(update_cases[UPDATE[1]][0], 96, update_cases[UPDATE[1]][0], 96)
    check_top(counts, fa, fb, rows, metric, 4, min_count=1, exclude_self=True)
    check_top(counts[40:57], fa, fb, rows, metric, 4, min_count=0, exclude_self=True, a_lo=40)


# ---- 3. the Python layer -----------------------------------------------------------------------------------------------
def make_sae(D, H, seed, cls=TopKSAE, **kw):
    torch.manual_seed(seed)
    return cls(D, H, **kw).to(DEV)


def oracle_of(codes_a, ha, codes_b, hb):
    a = tuple(np.concatenate([c[i].reshape(-1, c[i].shape[-1]).cpu().numpy() for c in codes_a]) for i in (0, 1))
    b = tuple(np.concatenate([c[i].reshape(-1, c[i].shape[-1]).cpu().numpy() for c in codes_b]) for i in (0, 1))
    return CO.accumulate(a, ha, b, hb)


def tracker_equals(t, want):
    return (np.array_equal(t.counts.cpu().numpy(), want[0]) and np.array_equal(t.fire_a.cpu().numpy(), want[1])
            and np.array_equal(t.fire_b.cpu().numpy(), want[2]) and t.rows == want[3])


def test_permuted_sae_is_recovered_by_phi():
    D, H, K = 64, 256, 8
    sae = make_sae(D, H, 1, k=K, precision="fp32")
    other = make_sae(D, H, 2, k=K, precision="fp32")
    perm = torch.randperm(H, generator=torch.Generator().manual_seed(3)).to(DEV)
    with torch.no_grad():
        other.encoder.weight.copy_(sae.encoder.weight[perm])
        other.encoder.bias.copy_(sae.encoder.bias[perm])
        other.b_pre.copy_(sae.b_pre)
        # four rows per feature along its own encoder direction, so that every feature fires and no two fire alike
        w = sae.encoder.weight.detach()
        x = (3.0 * w / w.norm(dim=1, keepdim=True)).repeat(4, 1) + 0.3 * torch.randn(4 * H, D, device=DEV)
    inv = torch.argsort(perm).int()  # feature i of sae is feature inv[i] of other
    loader = [x[:300].reshape(3, 100, D), x[300:]]
    tracker = collect_coactivation(sae, other, loader)
    assert tracker.rows == 4 * H
    fa = tracker.fire_a
    assert int(fa.min()) > 0 and int(fa.max()) < 4 * H  # (what the construction of x is for)
    assert torch.equal(tracker.fire_b[inv.long()], fa)
    nb = tracker.neighbors(n=2, metric="phi")
    assert torch.equal(nb.indices[:, 0], inv)
    assert bool((nb.values[:, 0] == 1.0).all()) and bool((nb.values[:, 1] < 1.0).all())
    assert torch.equal(nb.counts[:, 0], fa)
    rep = compare_activations(tracker)
    json.dumps(rep)
    assert rep["mean_best_phi_a_to_b"] == 1.0 and rep["mean_best_phi_b_to_a"] == 1.0 and rep["rows"] == 4 * H
    assert rep["mutual_best"] == H and rep["mutual_pairs"] == [[i, int(inv[i])] for i in range(H)]
    assert rep["fraction_at_least"]["a"] == {"0.5": 1.0, "0.7": 1.0, "0.9": 1.0}
    assert sum(rep["histogram"]["a"]["counts"]) == H and rep["histogram"]["b"]["counts"][-1] == H
    # the table itself, against the oracle on the codes the modules emit
    codes_a = [sae.eval().encode_compact(b) for b in loader]
    codes_b = [other.eval().encode_compact(b) for b in loader]
    assert tracker_equals(tracker, oracle_of(codes_a, H, codes_b, H))


def test_batch_topk_code_with_masked_zeros():
    D, H = 64, 256
    sae = make_sae(D, H, 4, cls=BatchTopKSAE, k=8, max_k_per_row=16)
    x = torch.randn(512, D, device=DEV, generator=torch.Generator(DEV).manual_seed(5))
    tracker = collect_coactivation(sae, dataloader=[x[:200], (x[200:], {"transcriptions": None})])
    codes = [sae.eval().encode_compact(b) for b in (x[:200], x[200:])]
    assert all(c[0].shape[-1] == 16 for c in codes) and any(bool((c[0] == 0).any()) for c in codes)  # masked entries
    want = oracle_of(codes, H, codes, H)
    assert tracker_equals(tracker, want) and tracker.is_self
    assert np.array_equal(np.diag(want[0]), want[1])
    nb = tracker.neighbors(n=4)  # jaccard, min_count 1, self excluded
    want_v, want_i, want_c = CO.top(want[0], want[1], want[2], want[3], "jaccard", 4, min_count=1, exclude_self=True)
    assert np.array_equal(nb.indices.cpu().numpy(), want_i) and np.array_equal(nb.counts.cpu().numpy(), want_c)
    assert np.array_equal(nb.values.cpu().numpy().view(np.uint32), want_v.view(np.uint32))


def test_tracker_sides_merge_window_and_round_trip(update_cases):
    a, b, want = update_cases[UPDATE[1]]
    dev = lambda code: tuple(torch.from_numpy(t).to(DEV) for t in code)  # noqa: E731
    ta, tb = dev(a), dev(b)
    ab = CoactivationTracker(96, 160)
    ab.update(ta, tb)
    assert tracker_equals(ab, want)
    ba = CoactivationTracker(160, 96)
    ba.update(tb, ta)
    assert torch.equal(ba.counts, ab.counts.t())
    for metric in CO.METRICS:  # side="b" is the tracker with the roles swapped
        x, y = ab.neighbors(n=4, metric=metric, side="b"), ba.neighbors(n=4, metric=metric, side="a")
        assert torch.equal(x.indices, y.indices) and torch.equal(x.counts, y.counts)
        assert torch.equal(x.values.view(torch.int32), y.values.view(torch.int32))
    # two halves of the dataset, leading shapes and a mask on the way
    h1, h2 = CoactivationTracker(96, 160), CoactivationTracker(96, 160)
    h1.update((ta[0][:128].reshape(4, 32, 5), ta[1][:128].reshape(4, 32, 5)),
              (tb[0][:128].reshape(4, 32, 32), tb[1][:128].reshape(4, 32, 32)))
    h2.update((ta[0][128:], ta[1][128:]), (tb[0][128:], tb[1][128:]), row_mask=torch.ones(129, device=DEV))
    h1.merge(h2)
    assert tracker_equals(h1, want)
    # a window keeps its rows of the table; side="b" and compare_activations need all of it
    win = CoactivationTracker(96, 160, a_window=(40, 17))
    win.update(ta, tb)
    assert torch.equal(win.counts, ab.counts[40:57]) and torch.equal(win.fire_a, ab.fire_a)
    x, y = win.neighbors(n=3, metric="phi"), ab.neighbors(n=3, metric="phi")
    assert torch.equal(x.indices, y.indices[40:57]) and torch.equal(x.values, y.values[40:57])
    with pytest.raises(ValueError):
        win.neighbors(side="b")
    with pytest.raises(ValueError):
        compare_activations(win)
    with pytest.raises(ValueError):
        win.merge(ab)
    with tempfile.TemporaryDirectory(prefix="wsae_coact_") as d:
        ab.save(f"{d}/t.pt")
        win.save(f"{d}/w.pt")
        back, wback = CoactivationTracker.load(f"{d}/t.pt", device=DEV), CoactivationTracker.load(f"{d}/w.pt", device=DEV)
    assert tracker_equals(back, want) and not back.is_self and (wback.a_lo, wback.a_rows) == (40, 17)
    assert torch.equal(wback.counts, win.counts)
    back.update(ta, tb)  # a loaded tracker goes on counting
    assert torch.equal(back.counts, 2 * ab.counts) and back.rows == 2 * want[3]
    # errors: CPU tensors, the kind of tracker, the cumulative row guard (host arithmetic, before any launch)
    with pytest.raises(N.WsaeError):
        ab.update((ta[0].cpu(), ta[1].cpu()), tb)
    with pytest.raises(ValueError):
        ab.update(ta)
    with pytest.raises(ValueError):
        CoactivationTracker(96).update(ta, tb)
    ab._submitted = 2 ** 31 - 1 - 256
    before = ab.counts.clone()
    with pytest.raises(N.WsaeError, match="exceed"):
        ab.update(ta, tb)
    assert torch.equal(ab.counts, before)


def test_collecting_leaves_the_next_train_step_alone():
    D, H, K, B = 64, 512, 8, 256
    x = torch.randn(B, D, generator=torch.Generator().manual_seed(9))
    losses, packs = [], []
    for probe in (False, True):
        sae = make_sae(D, H, 11, k=K)
        with tempfile.TemporaryDirectory(prefix="wsae_coact_") as run_dir:
            trainer = SAETrainer(sae, TrainingConfig(batch_size=B, learning_rate=1e-3, warmup_steps=0, use_amp=True,
                                                     num_workers=0), device=DEV, run_dir=run_dir)
            trainer.train_step(x)
            before = {k: v.detach().clone() for k, v in sae.state_dict().items()}
            mode = sae.training
            if probe:
                tracker = collect_coactivation(sae, dataloader=[x, x[:100]])
                tracker.neighbors(n=4, metric="phi")
                assert tracker.rows == B + 100 and sae.training == mode
                for k, v in sae.state_dict().items():
                    assert torch.equal(v, before[k]), k
            losses.append(trainer.train_step(x).loss)
            packs.append({k: v.detach().clone() for k, v in sae.state_dict().items()})
    assert np.float32(losses[0]).view(np.uint32) == np.float32(losses[1]).view(np.uint32)
    for k in packs[0]:
        assert torch.equal(packs[0][k], packs[1][k]), k
