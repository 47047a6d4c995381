"""Code clustering on the MI355X: ``wsae_cluster_assign`` and ``wsae_cluster_accumulate`` bit for bit against the
sequential numpy oracle of tests/cluster_oracle.py - ``assign``, the ``uint32`` views of ``best`` / ``second`` /
``inv_norm``, every integer of the state and of ``S_q`` - the properties that make the sums independent of the batching
and of the call order, and the Python layer on the planted case and on real modules.  The inputs and the conditions that
keep them from being degenerate are checked on the CPU in tests/test_code_clustering.py."""

from __future__ import annotations

import tempfile

import numpy as np
import pytest
import torch

import cluster_oracle as CO
from whisper_sae import _native as N
from whisper_sae.analysis import CodeKMeans, IterationStats, cluster_scores, collect_code_clusters, unit_sequences
from whisper_sae.sae.model import BatchTopKSAE, ReLUSAE, TopKSAE

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
JUNK = 0x5a5a5a5
JUNK_F = 123.25
TAIL = 3  # junk elements behind every output
OUTPUTS = ("assign", "best", "second", "inv_norm")
STATE = ("count", "best_q", "contingency", "totals")


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class AssignState:
    """Device state of ``wsae_cluster_assign`` with junk behind every array, which must survive."""

    def __init__(self, C, n_classes):
        self.n = {"count": C, "best_q": C, "contingency": C * n_classes, "totals": 3}
        self.shape = {"count": (C,), "best_q": (C,), "contingency": (C, n_classes), "totals": (3,)}
        self.t = {name: torch.zeros(n + TAIL, dtype=torch.int64, device=DEV) for name, n in self.n.items()}
        for name, n in self.n.items():
            self.t[name][n:] = JUNK

    def arrays(self):
        out = {}
        for name, n in self.n.items():
            assert bool((self.t[name][n:] == JUNK).all()), name
            out[name] = self.t[name][:n].cpu().numpy().reshape(self.shape[name])
        return out


def assign_call(c, combo, state=None, skip=(), rows=slice(None), expect=0):
    """One call over the rows ``rows`` of case ``c`` under ``CO.COMBOS[combo]`` -> dict of the outputs as numpy (those in
    ``skip`` are passed as NULL); ``state``: an ``AssignState`` to add to (its fields in ``skip`` NULL)."""
    with_bias, normalize, labelled, with_seg = CO.COMBOS[combo]
    v, i = dev(c["code"][0][rows]), dev(c["code"][1][rows])
    n_rows, k, C = v.shape[0], v.shape[1], c["n_clusters"]
    seg = dev(c["seg"][rows]) if with_seg else None
    lab = dev(c["labels"][rows]) if labelled else None
    Ct, bias = dev(c["Ct"]), dev(c["bias"]) if with_bias else None
    out = {"assign": torch.full((n_rows + TAIL,), JUNK, dtype=torch.int32, device=DEV)}
    for name in OUTPUTS[1:]:
        out[name] = torch.full((n_rows + TAIL,), JUNK_F, dtype=torch.float32, device=DEV)
    st = {} if state is None else state.t
    ws = torch.full((64,), 0xAB, dtype=torch.uint8, device=DEV)
    assert N.lib().wsae_cluster_assign_workspace_bytes(n_rows, k, c["hidden"], c["n_cols"], C) == 0
    ptr = lambda d, name: None if name in skip else N.ptr(d.get(name))
    rc = N.lib().wsae_cluster_assign(
        v.data_ptr(), i.data_ptr(), k, c["hidden"], N.ptr(seg), n_rows, N.ptr(dev(c["col_of"])), c["n_cols"], Ct.data_ptr(),
        Ct.shape[1], N.ptr(bias), C, int(normalize), N.ptr(lab), c["n_classes"] if labelled else 0, ptr(out, "assign"),
        ptr(out, "best"), ptr(out, "second"), ptr(out, "inv_norm"), ptr(st, "count"), ptr(st, "best_q"),
        ptr(st, "contingency") if labelled else None, ptr(st, "totals"), ws.data_ptr(), 64, torch.cuda.current_stream().cuda_stream)
    assert rc == expect, N.last_error()
    torch.cuda.synchronize()
    assert bool((ws == 0xAB).all())
    got = {}
    for name, t in out.items():
        junk = JUNK if name == "assign" else JUNK_F
        assert bool((t[n_rows:] == junk).all()), name
        if name in skip:
            assert bool((t == junk).all()), name
        else:
            got[name] = t[:n_rows].cpu().numpy()
    return got


def check_outputs(got, want, what, rows=slice(None)):
    a, best, second, inv, _ = want
    if "assign" in got:
        assert np.array_equal(got["assign"], a[rows]), what
    for name, w in (("best", best), ("second", second), ("inv_norm", inv)):
        if name in got:
            CO.same_bits(got[name], w[rows], (what, name))


def check_state(arrays, want_state, labelled, what, skip=()):
    want = CO.state_arrays(want_state)
    for name in STATE:
        if name in skip or (name == "contingency" and not labelled):
            assert not arrays[name].any(), (what, name)
        else:
            assert np.array_equal(arrays[name].reshape(want[name].shape), want[name]), (what, name)


# ---- 1: the assign kernel, every case and combination ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CO.CASES))
def test_assign_equals_the_oracle(name):
    c = CO.case(name)
    for combo in range(len(CO.COMBOS)):
        want = CO.case_assign(name, combo)
        st = AssignState(c["n_clusters"], c["n_classes"])
        got = assign_call(c, combo, st)
        check_outputs(got, want, (name, combo))
        check_state(st.arrays(), want[4], CO.COMBOS[combo][2], (name, combo))
        if name == "one":
            assert np.isneginf(got["second"][0]) and got["assign"][0] == 0


@pytest.mark.parametrize("name", ["c65", "wide"])
def test_every_output_null_in_turn(name):
    c = CO.case(name)
    want = CO.case_assign(name, 0)
    for skip in OUTPUTS + STATE:
        st = AssignState(c["n_clusters"], c["n_classes"])
        got = assign_call(c, 0, st, skip=(skip,))
        assert skip not in got
        check_outputs(got, want, (name, skip))
        check_state(st.arrays(), want[4], True, (name, skip), skip=(skip,))
    got = assign_call(c, 0, None)  # no state at all
    check_outputs(got, want, (name, "stateless"))


@pytest.mark.parametrize("name", ["c100", "ties"])
def test_calls_split_at_utterance_ends_add_in_any_order(name):
    c = CO.case(name)
    rows = c["rows"]
    utt = np.arange(rows) * CO.CASES[name][6] // rows  # (the utterance of every row, padding included)
    cuts = [0] + [r for r in range(1, rows) if utt[r] != utt[r - 1]] + [rows]
    pieces = [slice(cuts[j], cuts[j + 1]) for j in range(len(cuts) - 1)]
    assert len(pieces) >= 4
    for combo in (0, 1):
        want = CO.case_assign(name, combo)
        for order in (list(range(len(pieces))), list(reversed(range(len(pieces)))), [2, 0, 3, 1] + list(range(4, len(pieces)))):
            st = AssignState(c["n_clusters"], c["n_classes"])
            for j in order:
                check_outputs(assign_call(c, combo, st, rows=pieces[j]), want, (name, combo, j), pieces[j])
            check_state(st.arrays(), want[4], CO.COMBOS[combo][2], (name, combo, order))


# ---- 2: the accumulate kernel ---------------------------------------------------------------------------------------------------
def gpu_plan(c, rows=slice(None), cap=None):
    v, i, seg = dev(c["code"][0][rows]), dev(c["code"][1][rows]), dev(c["seg"][rows])
    n_rows, k, P = v.shape[0], v.shape[1], c["n_cols"]
    cap = n_rows * k if cap is None else cap
    col_ptr = torch.empty(P + 1, dtype=torch.int64, device=DEV)
    nnz = torch.zeros(1, dtype=torch.int64, device=DEV)
    t_row = torch.full((cap + TAIL,), -7, dtype=torch.int32, device=DEV)
    t_val = torch.full((cap + TAIL,), JUNK_F, dtype=torch.float32, device=DEV)
    need = N.lib().wsae_probe_plan_workspace_bytes(n_rows, k, c["hidden"], P)
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=DEV)
    N.check(N.lib().wsae_probe_plan(v.data_ptr(), i.data_ptr(), k, c["hidden"], seg.data_ptr(), n_rows, N.ptr(dev(c["col_of"])), P,
                                    col_ptr.data_ptr(), t_row.data_ptr(), t_val.data_ptr(), cap, nnz.data_ptr(), ws.data_ptr(), need,
                                    torch.cuda.current_stream().cuda_stream), "wsae_probe_plan")
    return col_ptr, t_row, t_val, int(nnz.item())


def acc_call(plan, cap, P, a, C, S, n_rows, weight=None):
    col_ptr, t_row, t_val, _ = plan
    assert N.lib().wsae_cluster_accumulate_workspace_bytes(n_rows, P, C, cap) == 0
    ws = torch.full((64,), 0xAB, dtype=torch.uint8, device=DEV)
    rc = N.lib().wsae_cluster_accumulate(col_ptr.data_ptr(), t_row.data_ptr(), t_val.data_ptr(), cap, P, a.data_ptr(), N.ptr(weight),
                                         n_rows, C, S.data_ptr(), S.shape[1], ws.data_ptr(), 64, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, N.last_error()
    torch.cuda.synchronize()
    assert bool((ws == 0xAB).all())


def spoiled_assign(name):
    """The oracle's assignment of the case with a few values out of range, and row weights with a NaN, a negative one
    and zeros among the inverse norms."""
    c = CO.case(name)
    a, _, _, inv, _ = CO.case_assign(name, 0)
    a, w = a.copy(), inv.copy()
    rng = np.random.default_rng(7)
    if c["rows"] > 8:
        at = rng.choice(c["rows"], 8, replace=False)
        a[at[:4]] = [c["n_clusters"], 10 ** 6, -5, -(2 ** 31)]
        w[at[4:]] = [np.nan, -1.0, 0.0, 2.5]
    return a, w


@pytest.mark.parametrize("name", ["one", "two", "c100", "wide"])
def test_accumulate_equals_the_oracle(name):
    c = CO.case(name)
    C, P, rows = c["n_clusters"], c["n_cols"], c["rows"]
    col_ptr, t_row, t_val = CO.case_plan(name)
    plan = gpu_plan(c)
    nnz = plan[3]
    assert nnz == t_row.size and np.array_equal(plan[0].cpu().numpy(), col_ptr)
    assert np.array_equal(plan[1][:nnz].cpu().numpy(), t_row)
    CO.same_bits(plan[2][:nnz].cpu().numpy(), t_val)
    a, w = spoiled_assign(name)
    stored = np.random.default_rng(11).integers(-2 ** 40, 2 ** 40, (P, C))
    for weight, cap, start in ((None, nnz, None), (w, nnz, None), (w, nnz // 2, stored), (None, nnz + 100, stored)):
        S = torch.full((P, C + CO.LDC_EXTRA), JUNK, dtype=torch.int64, device=DEV)
        S[:, :C] = 0 if start is None else dev(start)
        acc_call(plan, min(cap, plan[1].numel()), P, dev(a), C, S, rows, dev(weight))
        want = CO.accumulate(col_ptr, t_row, t_val, min(cap, nnz), a, C, rows, weight,
                             None if start is None else [[int(x) for x in row] for row in start])
        assert bool((S[:, C:] == JUNK).all())
        assert np.array_equal(S[:, :C].cpu().numpy(), np.asarray(want, np.int64)), (name, weight is not None, cap)
    if name == "c100":  # the feature that fires on every row is one long list: more than one piece of the kernel
        assert col_ptr[1] - col_ptr[0] > 400


@pytest.mark.parametrize("name", ["c100", "wide"])
def test_two_shards_add_to_the_whole(name):
    c = CO.case(name)
    C, P, rows = c["n_clusters"], c["n_cols"], c["rows"]
    a, w = spoiled_assign(name)
    col_ptr, t_row, t_val = CO.case_plan(name)
    want = np.asarray(CO.accumulate(col_ptr, t_row, t_val, t_row.size, a, C, rows, w), np.int64)
    cut = next(r for r in range(rows // 2, rows) if c["seg"][r] >= 0 and c["seg"][r - 1] >= 0 and c["seg"][r] != c["seg"][r - 1])
    for order in ((0, 1), (1, 0)):
        S = torch.zeros(P, C, dtype=torch.int64, device=DEV)
        for j in order:
            rs = (slice(0, cut), slice(cut, rows))[j]
            plan = gpu_plan(c, rs)
            acc_call(plan, plan[3], P, dev(a[rs]), C, S, rs.stop - rs.start, dev(w[rs]))
        assert np.array_equal(S.cpu().numpy(), want), (name, order)


# ---- 3: the Python layer on the planted case ------------------------------------------------------------------------------------
def within_one_ulp(got, want, what=""):
    g, w = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert g.shape == w.shape and (np.signbit(g) == np.signbit(w))[(g != 0) | (w != 0)].all(), what
    d = np.abs(g.view(np.int32).astype(np.int64) - w.view(np.int32).astype(np.int64))
    assert d.max() <= 1, (what, d.max())


def planted():
    c = CO.planted_case()
    return c, (dev(c["code"][0]), dev(c["code"][1])), dev(c["seg"])


def manual_fit(km, code, seg, c, check=True):
    """Drive ``accumulate`` / ``step`` by hand until no assignment changes; with ``check`` every iteration against the
    oracle from the very centroids the layer holds."""
    hidden, C = c["hidden"], c["n_clusters"]
    col_ptr, t_row, t_val = CO.plan(c["code"], hidden, c["seg"])
    stats = []
    for _ in range(10):
        Ct = km.centroids.t().contiguous().cpu().numpy()
        a = km.accumulate(code, segments=seg)
        if check:
            want_a, _, _, inv, st = CO.assign(c["code"], hidden, Ct, C, c["seg"], None, None, True)
            assert np.array_equal(a.cpu().numpy(), want_a)
            assert np.array_equal(km.counts.cpu().numpy(), CO.state_arrays(st)["count"])
            S_q = CO.accumulate(col_ptr, t_row, t_val, t_row.size, want_a, C, row_weight=inv)
            assert np.array_equal(km.sums.cpu().numpy(), np.asarray(S_q, np.int64))
        stats.append(km.step())
        assert isinstance(stats[-1], IterationStats)
        if check:
            within_one_ulp(km.centroids.t().cpu().numpy(), CO.update_centroids(S_q, st["count"], Ct, "cosine"), "step")
            assert stats[-1].objective == sum(st["best_q"]) / 2 ** 20 / st["totals"][0] and stats[-1].n_empty == 0
            assert not km.counts.any() and not km.sums.any()  # the sums are cleared
        if stats[-1].n_changed == 0:
            break
    return a, stats


def test_python_layer_on_the_planted_case():
    c, code, seg = planted()
    km = CodeKMeans(8, c["hidden"], device=DEV, seed=0)
    km.init_centroids(code, segments=seg)
    within_one_ulp(km.centroids.t().cpu().numpy(), CO.init_sample(c["code"], c["hidden"], c["seg"], None, 512, 8, "cosine", 0), "init")
    a, stats = manual_fit(km, code, seg, c)
    assert stats[0].n_changed is None and stats[-1].n_changed == 0 and len(stats) <= 7
    table = CO.table_of(a.cpu().numpy(), c["proto"], 8, 8)
    assert CO.scores(table)["ari"] == 1.0 and cluster_scores(torch.from_numpy(table)).ari == 1.0
    assert stats[-1].objective >= stats[0].objective and int(stats[-1].counts.sum()) == 1157
    # fit is the manual loop
    fitted = CodeKMeans(8, c["hidden"], device=DEV, seed=0)
    history = fitted.fit(code, segments=seg, max_iter=10, tol=0.0)
    assert len(history) == len(stats) and [h.objective for h in history] == [s.objective for s in stats]
    assert torch.equal(fitted.centroids, km.centroids)
    # predict, and the round trip through a file
    pa, score, margin = km.predict(code, segments=seg)
    Ct = km.centroids.t().contiguous().cpu().numpy()
    want_a, best, second, inv, _ = CO.assign(c["code"], c["hidden"], Ct, 8, c["seg"], None, None, True)
    assert np.array_equal(pa.cpu().numpy(), want_a) and np.array_equal(pa.cpu().numpy(), a.cpu().numpy())
    CO.same_bits(score.cpu().numpy(), best * inv, "score")
    CO.same_bits(margin.cpu().numpy(), best - second, "margin")
    assert not km.counts.any()  # predict adds nothing
    with tempfile.TemporaryDirectory(prefix="wsae_cluster_") as d:
        km.save(f"{d}/a.pt")
        back = CodeKMeans.load(f"{d}/a.pt", device=DEV)
    assert torch.equal(back.centroids, km.centroids) and back.metric == "cosine" and back.n_clusters == 8
    assert torch.equal(back.predict(code, segments=seg)[0], pa)
    units, lengths, utts = unit_sequences(pa, seg)
    want_u = CO.unit_sequences(want_a, c["seg"])
    assert units.tolist() == want_u[0].tolist() and lengths.tolist() == want_u[1].tolist() and utts.tolist() == want_u[2].tolist()
    feats, weights = km.top_features(4)
    assert feats.shape == (8, 4) and bool((weights[:, 0] >= weights[:, 1]).all())
    order = np.argsort(-Ct[:, 0], kind="stable")[:4]
    assert feats[0].tolist() == order.tolist()


def test_merge_sums_of_two_halves_is_one_pass():
    c, code, seg = planted()
    cut = int(np.nonzero(c["seg"] == 6)[0][0])
    whole, left, right = (CodeKMeans(8, c["hidden"], device=DEV, seed=0, n_classes=8) for _ in range(3))
    proto = dev(c["proto"])
    whole.init_centroids(code, segments=seg)
    for km in (left, right):
        km.init_centroids(init=whole.centroids)
    whole.accumulate(code, segments=seg, labels=proto)
    left.accumulate((code[0][:cut], code[1][:cut]), segments=seg[:cut], labels=proto[:cut])
    right.accumulate((code[0][cut:], code[1][cut:]), segments=seg[cut:], labels=proto[cut:])
    left.merge_sums(right)
    for name in ("sums", "counts", "contingency", "totals"):
        assert torch.equal(getattr(left, name), getattr(whole, name)), name
    assert int(whole.totals[2]) == 1157 and int(whole.contingency.sum()) == 1157
    a, b = whole.step(), left.step()
    assert a.objective == b.objective and torch.equal(whole.centroids, left.centroids)
    assert torch.equal(whole.last_contingency, left.last_contingency)
    with pytest.raises(ValueError, match="different centroids"):
        whole.merge_sums(right)


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_an_empty_cluster_is_reseeded(metric):
    c, code, seg = planted()
    hidden = c["hidden"]
    init = np.zeros((3, hidden), np.float32)
    init[0] = CO.dense_row(c["code"][0][0], c["code"][1][0], hidden, None, hidden)
    init[1] = CO.dense_row(c["code"][0][500], c["code"][1][500], hidden, None, hidden)
    init[2] = -1.0  # every frame scores below 0 against it, and at least 0 against the two others (cosine)
    km = CodeKMeans(3, hidden, metric=metric, device=DEV)
    km.init_centroids(init=torch.from_numpy(init))
    Ct = km.centroids.t().contiguous().cpu().numpy()
    a = km.accumulate(code, segments=seg).cpu().numpy()
    cosine = metric == "cosine"
    bias = None if cosine else CO.euclid_bias(Ct, 3)
    if not cosine:
        within_one_ulp(km._state["bias"].cpu().numpy(), bias, "bias")
        bias = km._state["bias"].cpu().numpy()  # (the oracle assigns under the very bias the layer holds)
    want_a, best, _, inv, st = CO.assign(c["code"], hidden, Ct, 3, c["seg"], None, bias, cosine)
    assert np.array_equal(a, want_a) and st["count"][2] == 0 and st["count"][0] > 0 and st["count"][1] > 0
    stats = km.step()
    assert stats.n_empty == 1 and stats.counts.tolist() == st["count"]
    b = np.where(want_a >= 0, best * inv if cosine else best, np.inf)
    r = int(np.argmin(b))  # (the lowest row at the minimum)
    want = CO.finish_centroid(CO.dense_row(c["code"][0][r], c["code"][1][r], hidden, None, hidden), metric)
    within_one_ulp(km.centroids[2].cpu().numpy(), want, "reseed")
    assert km.accumulate(code, segments=seg).cpu().numpy()[r] == 2 and int(km.counts[2]) >= 1


# ---- 4: real modules ------------------------------------------------------------------------------------------------------------
D, H, K, UTT, T = 64, 256, 8, 12, 40


def utterances(seed):
    """12 utterances of 40 frames in three batches with labels and a frame mask; a frame is one of 6 prototypes, noisy."""
    gen = torch.Generator().manual_seed(seed)
    proto = torch.randn(6, D, generator=gen)
    labels = ((torch.rand(UTT, T, generator=gen) < 0.3).cumsum(1) + torch.arange(UTT)[:, None]) % 6
    x = proto[labels] * torch.exp(0.2 * torch.randn(UTT, T, 1, generator=gen)) + 0.2 * torch.randn(UTT, T, D, generator=gen)
    mask = torch.ones(UTT, T)
    for u in range(UTT):
        mask[u, 24 + (u % 5) * 3:] = 0
    return [(x[:5], labels[:5], mask[:5]), (x[5:6], labels[5:6], mask[5:6]), (x[6:], labels[6:], mask[6:])], mask, labels


@pytest.mark.parametrize("kind", ["topk", "batch_topk"])
def test_collect_code_clusters_on_real_modules(kind):
    torch.manual_seed(1 if kind == "topk" else 2)
    sae = (TopKSAE(D, H, k=K) if kind == "topk" else BatchTopKSAE(D, H, k=K, max_k_per_row=16)).to(DEV)
    batches, mask, labels = utterances(5)
    sae.train()
    km, history = collect_code_clusters(sae, batches, 6, n_classes=6, max_iter=4, tol=0.0)
    assert sae.training and km.hidden == H and 1 <= len(history) <= 4
    sae.eval()
    with torch.no_grad():
        codes = [sae.encode_compact(x.to(DEV)) for x, _, _ in batches]
    vals, idx = (np.concatenate([cc[i].reshape(-1, cc[i].shape[-1]).cpu().numpy() for cc in codes]) for i in (0, 1))
    seg = np.where(mask.reshape(-1).numpy() != 0, np.repeat(np.arange(UTT), T), -1).astype(np.int32)
    # the same walk by hand: seeded from the first item, every iteration's sums from the oracle
    first = slice(0, 5 * T)
    Ct = CO.init_sample((vals[first], idx[first]), H, seg[first], None, H, 6, "cosine", 0)
    ref = CodeKMeans(6, H, device=DEV, n_classes=6)
    ref.init_centroids((dev(vals[first]), dev(idx[first])), segments=dev(seg[first]))
    within_one_ulp(ref.centroids.t().cpu().numpy(), Ct, "init")
    flat = (dev(vals), dev(idx))
    again = ref.fit(flat, segments=dev(seg), labels=labels.reshape(-1).to(DEV), max_iter=len(history), tol=0.0)
    assert [h.objective for h in again] == [h.objective for h in history] and torch.equal(ref.centroids, km.centroids)
    a, _, _ = km.predict(flat, segments=dev(seg))
    Cn = km.centroids.t().contiguous().cpu().numpy()
    want_a = CO.assign((vals, idx), H, Cn, 6, seg, None, None, True)[0]
    assert np.array_equal(a.cpu().numpy(), want_a) and (want_a[seg < 0] == -1).all()
    sc = km.score(flat, labels.reshape(-1).to(DEV), segments=dev(seg))
    table = CO.table_of(want_a, labels.reshape(-1).numpy(), 6, 6)
    assert sc.n_frames == table.sum() and sc.ari == pytest.approx(CO.scores(table)["ari"], abs=1e-12)
    with pytest.raises(TypeError):
        collect_code_clusters(ReLUSAE(D, H).to(DEV), [x for x, _, _ in batches], 4)
