"""ABX discrimination on the MI355X: ``wsae_dtw_matrix`` and ``wsae_abx_count`` bit for bit against the sequential numpy
oracle of tests/abx_oracle.py - the ``uint32`` view of every distance that is not NaN, the NaN masks, ``steps`` and every
integer of the tables - the properties that make a cell independent of the other items and of the split into calls, and
the Python layer on real modules.  The inputs and the conditions that keep them from being degenerate are checked on the
CPU in tests/test_abx.py."""

from __future__ import annotations

import tempfile

import numpy as np
import pytest
import torch

import abx_oracle as AO
from dynamics_oracle import same_bits
from whisper_sae import _native as N
from whisper_sae.analysis import AbxItems, AbxScores, collect_abx, segment_distances
from whisper_sae.analysis.discrimination import compact_module
from whisper_sae.sae.model import BatchTopKSAE, ReLUSAE, TopKSAE

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
JUNK = 0x5a5a5a5
JUNK_F = 123.25
TAIL = 3  # junk rows behind every output


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def dtw_call(code, hidden, a, b, metric, normalize, seg=None, weight=None, want_steps=True, pad=0, rows=None, expect=0):
    """One call -> ``(dist [n_a, n_b], steps or None)`` as numpy; ``pad`` junk columns behind column n_b (ldd = n_b + pad)
    and ``TAIL`` junk rows must survive, and so must the 0xAB behind the workspace."""
    v, i = dev(code[0]), dev(code[1])
    s = None if seg is None else dev(np.asarray(seg, np.int32))
    w = None if weight is None else dev(np.asarray(weight, np.float32))
    a_st, a_ln, b_st, b_ln = (dev(np.asarray(x, np.int32)) for x in (a[0], a[1], b[0], b[1]))
    n_rows, k, n_a, n_b = (v.shape[0] if rows is None else rows), v.shape[1], a_st.numel(), b_st.numel()
    ldd = n_b + pad
    lib = N.lib()
    need = lib.wsae_dtw_workspace_bytes(n_rows, k, hidden, n_a, n_b)
    assert need >= 0
    ws = torch.full((need + 64,), 0xAB, dtype=torch.uint8, device=DEV)
    dist = torch.full((n_a + TAIL, ldd), JUNK_F, dtype=torch.float32, device=DEV)
    steps = torch.full((n_a + TAIL, ldd), JUNK, dtype=torch.int32, device=DEV) if want_steps else None
    rc = lib.wsae_dtw_matrix(v.data_ptr(), i.data_ptr(), k, hidden, N.ptr(s), N.ptr(w), n_rows, a_st.data_ptr(), a_ln.data_ptr(),
                             n_a, b_st.data_ptr(), b_ln.data_ptr(), n_b, metric, int(normalize), dist.data_ptr(), N.ptr(steps),
                             ldd, ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    assert rc == expect, N.last_error()
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xAB).all())
    touched = n_a if (n_a and n_b and n_rows) else 0
    assert bool((dist[touched:] == JUNK_F).all()) and bool((dist[:, n_b:] == JUNK_F).all())
    if steps is not None:
        assert bool((steps[touched:] == JUNK).all()) and bool((steps[:, n_b:] == JUNK).all())
    return dist[:n_a, :n_b].cpu().numpy(), None if steps is None else steps[:n_a, :n_b].cpu().numpy()


def same_cells(got, want, what=""):
    same_bits(got[0], want[0], what)
    if got[1] is not None:
        assert np.array_equal(got[1], want[1]), (what, "steps")


CASES = list(range(len(AO.DIST_SHAPES)))
# (metric, weighted)
COMBOS = ((AO.COSINE, False), (AO.COSINE, True), (AO.JACCARD, False), (AO.JACCARD, True))


# ---- 1: distances, every case and metric -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", CASES, ids=["x".join(map(str, s)) for s in AO.DIST_SHAPES])
def test_distances_and_steps_equal_the_oracle(n):
    c = AO.distance_case(n)
    for metric, weighted in COMBOS:
        for normalize in (True, False):
            want = AO.case_distances(n, metric, weighted, normalize)
            got = dtw_call(c["code"], c["hidden"], c["a"], c["b"], metric, normalize, c["seg"], c["weight"] if weighted else None)
            same_cells(got, want, (n, metric, weighted, normalize))
    if n != AO.TIE_CASE:
        assert np.isnan(want[0]).any() and (want[1] == 0).sum() == np.isnan(want[0]).sum()  # the invalid items


def test_the_tie_case_takes_the_stated_predecessor():
    c = AO.distance_case(AO.TIE_CASE)
    _, L = AO.case_tables(AO.TIE_CASE, AO.JACCARD, False)
    _, L_rev = AO.case_tables(AO.TIE_CASE, AO.JACCARD, False, True)
    got = dtw_call(c["code"], c["hidden"], c["a"], c["b"], AO.JACCARD, True, c["seg"])
    assert np.array_equal(got[1], L) and (got[1] != L_rev).sum() * 2 >= L.size


def test_one_by_one_and_without_segments():
    c = AO.distance_case(1)
    for item in ((np.array([17]), np.array([1])), (np.array([0]), np.array([64])), (np.array([236]), np.array([64]))):
        want = AO.dtw_matrix(c["code"], c["hidden"], item, item, AO.COSINE, True, None, c["weight"])
        same_cells(dtw_call(c["code"], c["hidden"], item, item, AO.COSINE, True, None, c["weight"]), want, item)
        assert want[1][0, 0] == item[1][0]  # (an item against itself walks the diagonal)


# ---- 2: the properties ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 4])
def test_a_cell_depends_on_its_two_items_alone(n):
    c = AO.distance_case(n)
    for metric in (AO.COSINE, AO.JACCARD):
        whole = dtw_call(c["code"], c["hidden"], c["a"], c["b"], metric, True, c["seg"], c["weight"])
        n_a, n_b = whole[0].shape
        # the lists split into calls of uneven sizes
        for a_lo, a_hi in ((0, 1), (1, 4), (4, n_a)):
            for b_lo, b_hi in ((0, 5), (5, 22), (22, n_b)):
                part = dtw_call(c["code"], c["hidden"], tuple(x[a_lo:a_hi] for x in c["a"]), tuple(x[b_lo:b_hi] for x in c["b"]),
                                metric, True, c["seg"], c["weight"])
                same_cells(part, (whole[0][a_lo:a_hi, b_lo:b_hi], whole[1][a_lo:a_hi, b_lo:b_hi]), (n, metric, a_lo, b_lo))
        # other items in front: every item moves to other lanes, passes and groups
        more = tuple(np.concatenate([np.asarray(x[:9]), np.asarray(x)]) for x in c["b"])
        shifted = dtw_call(c["code"], c["hidden"], c["a"], more, metric, True, c["seg"], c["weight"])
        same_cells((shifted[0][:, 9:], shifted[1][:, 9:]), whole, (n, metric, "shifted"))
        # steps == NULL and ldd > n_b
        same_bits(dtw_call(c["code"], c["hidden"], c["a"], c["b"], metric, True, c["seg"], c["weight"], want_steps=False)[0], whole[0])
        same_cells(dtw_call(c["code"], c["hidden"], c["a"], c["b"], metric, True, c["seg"], c["weight"], pad=5), whole)


def test_empty_calls_touch_nothing():
    c = AO.distance_case(1)
    none = (np.zeros(0, np.int32), np.zeros(0, np.int32))
    assert dtw_call(c["code"], c["hidden"], none, c["b"], AO.COSINE, True)[0].shape == (0, 131)
    assert dtw_call(c["code"], c["hidden"], c["a"], none, AO.COSINE, True)[0].shape == (7, 0)
    dtw_call(c["code"], c["hidden"], c["a"], c["b"], AO.COSINE, True, rows=0)  # (the helper checks that the junk survives)


def test_bad_arguments_are_refused_with_a_message():
    lib = N.lib()
    c = AO.distance_case(1)
    v, i = dev(c["code"][0]), dev(c["code"][1])
    st, ln = dev(c["a"][0]), dev(c["a"][1])
    out = torch.full((7, 7), JUNK_F, dtype=torch.float32, device=DEV)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)

    def call(k=5, hidden=32, rows=300, n_a=7, n_b=7, metric=0, ldd=7, ws_bytes=1 << 20, vals=v.data_ptr()):
        return lib.wsae_dtw_matrix(vals, i.data_ptr(), k, hidden, 0, 0, rows, st.data_ptr(), ln.data_ptr(), n_a, st.data_ptr(),
                                   ln.data_ptr(), n_b, metric, 1, out.data_ptr(), 0, ldd, ws.data_ptr(), ws_bytes, 0)

    for kwargs, word in (({"k": 0}, "k"), ({"k": 129}, "k"), ({"hidden": 0}, "hidden"), ({"rows": -1}, "n_rows"), ({"n_a": -1}, "n_a"),
                         ({"metric": 1}, "metric"), ({"ldd": 6}, "ldd"), ({"ws_bytes": 16}, "workspace"), ({"vals": 0}, "null")):
        assert call(**kwargs) == -1 and word in N.last_error(), (kwargs, N.last_error())
    torch.cuda.synchronize()
    assert bool((out == JUNK_F).all())
    assert lib.wsae_dtw_workspace_bytes(300, 0, 32, 1, 1) == -1 and lib.wsae_dtw_workspace_bytes(300, 5, 32, -1, 1) == -1
    assert lib.wsae_abx_workspace_bytes(10, 11, 5) == -1 and lib.wsae_abx_workspace_bytes(10, 5, 1025) == -1
    cat = torch.zeros(7, dtype=torch.int32, device=DEV)
    tab = torch.zeros(4, 4, dtype=torch.int64, device=DEV)

    def count(x_lo=0, n_x=7, n_items=7, n_cats=4, mode=0, ldd=7, spk=0, ws_bytes=1 << 20):
        return lib.wsae_abx_count(out.data_ptr(), ldd, x_lo, n_x, n_items, cat.data_ptr(), 0, spk, n_cats, mode, tab.data_ptr(),
                                  tab.data_ptr(), tab.data_ptr(), ws.data_ptr(), ws_bytes, 0)

    for kwargs, word in (({"x_lo": 1}, "window"), ({"n_cats": 0}, "n_cats"), ({"n_cats": 1025}, "n_cats"), ({"mode": 3}, "mode"),
                         ({"ldd": 6}, "ldd"), ({"mode": 1}, "spk"), ({"ws_bytes": 16}, "workspace")):
        assert count(**kwargs) == -1 and word in N.last_error(), (kwargs, N.last_error())
    torch.cuda.synchronize()
    assert int(tab.abs().sum()) == 0


# ---- 3: the counts ---------------------------------------------------------------------------------------------------------------
def count_call(c, mode, x_lo=0, n_x=None, with_ctx=True, tables=None, pad=0):
    """One call on ``tables`` (a dict of device tensors with junk behind them; None: fresh ones) -> the tables."""
    n, n_cats = len(c["cat"]), c["n_cats"]
    n_x = n - x_lo if n_x is None else n_x
    if tables is None:
        tables = {"wins2": torch.zeros(n_cats + TAIL, n_cats, dtype=torch.int64, device=DEV),
                  "total": torch.zeros(n_cats + TAIL, n_cats, dtype=torch.int64, device=DEV),
                  "skipped": torch.zeros(1 + TAIL, dtype=torch.int64, device=DEV)}
        for name, t in tables.items():
            t[(1 if name == "skipped" else n_cats):] = JUNK
    dist = torch.full((n_x + TAIL, n + pad), JUNK_F, dtype=torch.float32, device=DEV)
    dist[:n_x, :n] = dev(c["dist"][x_lo:x_lo + n_x])
    cat, ctx, spk = dev(c["cat"]), dev(c["ctx"]) if with_ctx else None, dev(c["spk"])
    lib = N.lib()
    need = lib.wsae_abx_workspace_bytes(n, n_x, n_cats)
    assert need >= 0
    ws = torch.full((need + 64,), 0xAB, dtype=torch.uint8, device=DEV)
    rc = lib.wsae_abx_count(dist.data_ptr(), n + pad, x_lo, n_x, n, cat.data_ptr(), N.ptr(ctx), spk.data_ptr(), n_cats, mode,
                            tables["wins2"].data_ptr(), tables["total"].data_ptr(), tables["skipped"].data_ptr(), ws.data_ptr(),
                            need, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, N.last_error()
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xAB).all())
    return tables


def read_tables(tables, n_cats):
    assert bool((tables["wins2"][n_cats:] == JUNK).all()) and bool((tables["total"][n_cats:] == JUNK).all())
    assert bool((tables["skipped"][1:] == JUNK).all())
    return tables["wins2"][:n_cats].cpu().numpy(), tables["total"][:n_cats].cpu().numpy(), int(tables["skipped"][0])


def same_counts(got, want, what=""):
    assert np.array_equal(got[0], want[0]), (what, "wins2")
    assert np.array_equal(got[1], want[1]), (what, "total")
    assert got[2] == want[2], (what, "skipped", got[2], want[2])


@pytest.mark.parametrize("tied", [False, True], ids=["distinct", "tied"])
def test_counts_equal_the_oracle(tied):
    c = AO.count_case(tied)
    for mode in (AO.ANY, AO.WITHIN, AO.ACROSS):
        for with_ctx in (True, False):
            want = AO.count_result(tied, mode, with_ctx)
            assert want[1].sum() > 1000
            same_counts(read_tables(count_call(c, mode, with_ctx=with_ctx, pad=3), c["n_cats"]), want, (tied, mode, with_ctx))


def test_windows_and_shards_add():
    c = AO.count_case(False)
    n = len(c["cat"])
    for mode in (AO.ANY, AO.ACROSS):
        want = AO.count_result(False, mode)
        tables = None
        for lo, hi in ((0, 1), (1, 38), (38, 39), (39, 150)):  # windows of uneven sizes on one set of tables
            tables = count_call(c, mode, lo, hi - lo, tables=tables)
        same_counts(read_tables(tables, c["n_cats"]), want, mode)
        one = read_tables(count_call(c, mode, 0, 77), c["n_cats"])  # two shards, each with tables of its own
        two = read_tables(count_call(c, mode, 77, n - 77), c["n_cats"])
        same_counts((one[0] + two[0], one[1] + two[1], one[2] + two[2]), want, mode)
    assert read_tables(count_call(c, AO.ANY, 5, 0), c["n_cats"])[1].sum() == 0  # an empty window


# ---- 4: the Python layer -----------------------------------------------------------------------------------------------------------
def planted_batches(n_batches=2):
    """``(x [n_utt, T, D], labels [n_utt, T], frame_mask)`` batches: utterances of phone-like runs whose frames share a
    direction per phone, with unlabelled frames and padding behind every utterance."""
    rng = np.random.default_rng(77)
    D, T, n_cls = 64, 40, 5
    proto = rng.standard_normal((n_cls, D)).astype(np.float32)
    out = []
    for _ in range(n_batches):
        x = np.zeros((3, T, D), np.float32)
        lab = np.full((3, T), -1, np.int64)
        mask = np.ones((3, T), bool)
        for u in range(3):
            t, c = 0, -1
            end = T - int(rng.integers(2, 6))
            mask[u, end:] = False
            while t < end:
                d = min(int(rng.integers(2, 7)), end - t)
                c = int((c + 1 + rng.integers(0, n_cls - 1)) % n_cls)
                x[u, t:t + d] = proto[c] + 0.6 * rng.standard_normal((d, D)).astype(np.float32)
                lab[u, t:t + d] = c if rng.random() > 0.1 else -1
                t += d
            x[u, end:] = rng.standard_normal((T - end, D)).astype(np.float32)
        out.append((torch.from_numpy(x), torch.from_numpy(lab), torch.from_numpy(mask)))
    return out


def oracle_scores(model, batches, mode, with_context, speakers, metric="cosine"):
    """The oracle on the compact code the module itself gives: items, distances, counts."""
    vals, idx, seg, labels = [], [], [], []
    with torch.no_grad():
        for bi, (x, lab, mask) in enumerate(batches):
            v, i = compact_module(model).encode_compact(x.to(DEV))
            k = v.shape[-1]
            vals.append(v.reshape(-1, k).float().cpu().numpy()), idx.append(i.reshape(-1, k).cpu().numpy().astype(np.int32))
            s = np.arange(bi * x.shape[0], (bi + 1) * x.shape[0])[:, None].repeat(x.shape[1], 1)
            seg.append(np.where(mask.numpy(), s, -1).reshape(-1)), labels.append(lab.numpy().reshape(-1))
    code = (np.concatenate(vals), np.concatenate(idx))
    seg, labels = np.concatenate(seg).astype(np.int32), np.concatenate(labels)
    labels = np.where(seg >= 0, labels, -1)
    st, ln, cat, ctx, _, _ = AO.items_from_labels(labels, seg, n_classes=5)
    dist, _ = AO.dtw_matrix(code, model.hidden_dim, (st, ln), (st, ln), AO.METRIC[metric], True, seg)
    spk = None if speakers is None else np.asarray(speakers)[seg[st]].astype(np.int32)
    return AO.abx_count(dist, 0, len(cat), cat, ctx if with_context else None, spk, 5, AO.MODES[mode]), dist, (st, ln, cat)


@pytest.mark.parametrize("kind", ["topk", "batchtopk", "relu"])
def test_collect_abx_equals_the_oracle_on_real_modules(kind):
    torch.manual_seed(5)
    model = {"topk": lambda: TopKSAE(64, 256, k=8), "batchtopk": lambda: BatchTopKSAE(64, 256, k=8, max_k_per_row=16),
             "relu": lambda: ReLUSAE(64, 256)}[kind]()
    if kind == "relu":  # a dense code with few active entries per frame (the compact view holds at most 128)
        with torch.no_grad():
            model.encoder.bias.fill_(-1.0)
    model = model.to(DEV)
    batches = planted_batches(3)
    speakers = [0, 1, 2] * 3  # per utterance
    for mode, with_context in (("any", True), ("within", False), ("across", False)):
        model.eval()
        want, dist, items = oracle_scores(model, batches, mode, with_context, speakers)
        model.train()
        got = collect_abx(model, batches, mode=mode, with_context=with_context, speakers=speakers, n_classes=5, row_block=17)
        assert isinstance(got, AbxScores)
        same_counts((got.wins2.numpy(), got.total.numpy(), got.skipped), want, (kind, mode))
        assert want[1].sum() > 0
        score, error = AO.scores(want[0], want[1])
        assert np.array_equal(np.isnan(got.score.numpy()), np.isnan(score)) and np.allclose(np.nan_to_num(got.score.numpy()), np.nan_to_num(score), rtol=0, atol=0)
        assert abs(got.error - error) < 1e-12 and got.n_triples == int(want[1].sum())  # (a float64 mean of <= 25 cells)
    assert model.training


def test_items_store_distances_save_load_merge_subsample():
    torch.manual_seed(6)
    model = TopKSAE(64, 256, k=8).to(DEV).eval()
    batches = planted_batches(2)
    want, dist, (st, ln, cat) = oracle_scores(model, batches, "any", False, None)
    stores = []
    with torch.no_grad():
        for x, lab, mask in batches:
            s = AbxItems(256)
            v, i = model.encode_compact(x.to(DEV))
            s.add((v.reshape(3, 40, -1), i.reshape(3, 40, -1)), labels=lab.to(DEV), frame_mask=mask.to(DEV), n_classes=5)
            stores.append(s)
    n0 = stores[0].n_items
    with tempfile.TemporaryDirectory() as tmp:
        stores[0].save(f"{tmp}/a.pt")
        both = AbxItems.load(f"{tmp}/a.pt", device=DEV)
    assert both.n_items == n0 and both.n_rows == int(ln[:n0].sum())  # (only the rows of the items are kept)
    both.merge(stores[1])
    assert both.n_items == len(cat)
    same_bits(both.distances().cpu().numpy(), dist)
    same_bits(both.distances(rows=(3, 9)).cpu().numpy(), dist[3:9])
    got = both.score("any", row_block=13, with_context=False)
    same_counts((got.wins2.numpy(), got.total.numpy(), got.skipped), want)
    half = stores[0].score("any") + stores[0].score("any")  # shards add
    assert np.array_equal(half.total.numpy(), 2 * stores[0].score("any").total.numpy())
    sub = both.subsample(20, seed=1)
    assert sub.n_items == 20 and both.subsample(20, seed=1).category.tolist() == sub.category.tolist()
    assert both.subsample(10 ** 6, seed=1).n_items == both.n_items
    # the query-by-example entry point on the raw code
    v, i = model.encode_compact(batches[0][0].to(DEV))
    code = (v.reshape(-1, v.shape[-1]), i.reshape(-1, v.shape[-1]))
    starts, lengths = torch.tensor([0, 5, 30], device=DEV), torch.tensor([4, 64, 7], device=DEV)
    d, steps = segment_distances(code, starts, lengths, hidden=256, metric="jaccard", return_steps=True)
    wd, ws = AO.dtw_matrix((code[0].cpu().numpy(), code[1].cpu().numpy().astype(np.int32)), 256, (starts.cpu().numpy(), lengths.cpu().numpy()),
                           (starts.cpu().numpy(), lengths.cpu().numpy()), AO.JACCARD, True)
    same_bits(d.cpu().numpy(), wd)
    assert np.array_equal(steps.cpu().numpy(), ws)
    d2 = segment_distances(code, starts, lengths, other=(starts[:2], lengths[:2]), hidden=256, metric="jaccard")
    same_bits(d2.cpu().numpy(), wd[:, :2])


def test_error_messages():
    v = torch.rand(30, 4, device=DEV)
    i = torch.randint(0, 64, (30, 4), device=DEV, dtype=torch.int32)
    st, ln = torch.tensor([0, 4], device=DEV), torch.tensor([3, 5], device=DEV)
    with pytest.raises(TypeError, match="pair"):
        segment_distances(v, st, ln, hidden=64)
    with pytest.raises(N.WsaeError):
        segment_distances((v.cpu(), i.cpu()), st, ln, hidden=64)
    with pytest.raises(ValueError, match="metric"):
        segment_distances((v, i), st, ln, hidden=64, metric="dot")
    with pytest.raises(ValueError, match="k must be"):
        segment_distances((torch.rand(30, 129, device=DEV), torch.zeros(30, 129, device=DEV, dtype=torch.int32)), st, ln, hidden=64)
    with pytest.raises(ValueError, match="starts"):
        segment_distances((v, i), st, ln[:1], hidden=64)
    with pytest.raises(TypeError, match="pair"):
        segment_distances((v, i), st, ln, other=st, hidden=64)
    with pytest.raises(ValueError, match="metric"):
        AbxItems(64, metric="angular")
    with pytest.raises(ValueError, match="mode"):
        AbxItems(64).score("between")
    s = AbxItems(64)
    with pytest.raises(ValueError, match="labels or items"):
        s.add((v, i))
    with pytest.raises(TypeError, match="pair"):
        s.add(v, labels=torch.zeros(30, dtype=torch.int64, device=DEV))
    s.add((v, i), items=(st, ln, torch.tensor([0, 1], device=DEV)))
    with pytest.raises(ValueError, match="speakers"):
        s.score("within")
    with pytest.raises(ValueError, match="merge"):
        s.merge(AbxItems(32))
    with pytest.raises(TypeError, match="encode_compact"):
        collect_abx(torch.nn.Linear(4, 4), [])
