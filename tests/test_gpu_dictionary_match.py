"""Dictionary comparison on the MI355X: ``wsae_match_rows`` against the float64 oracle of tests/match_oracle.py - exact
cases bit for bit, planted ties across tiles and splits, random cosines within the derived bounds, a recovered
permutation, determinism - and the Python layer on real bound modules, reading the parameter pack in place."""

from __future__ import annotations

import tempfile

import numpy as np
import pytest
import torch

import match_oracle as MO
from whisper_sae import _native as N
from whisper_sae.analysis import compare_dictionaries, duplicate_features, nearest_features
from whisper_sae.config import TrainingConfig
from whisper_sae.sae.crosscoder import TopKCrossLayerCrosscoder
from whisper_sae.sae.model import ReLUSAE, TopKSAE
from whisper_sae.sae.training import SAETrainer
from whisper_sae.sae.transcoder import TopKTranscoder

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PREC = {"fp32": N.PREC_FP32, "bf16": N.PREC_BF16}
METRIC = {"cosine": N.MATCH_COSINE, "dot": N.MATCH_DOT}


def match(a, b, n, metric="cosine", precision="fp32", exclude_self=False, pad_cols=0):
    """``wsae_match_rows`` on numpy float32 matrices -> (values, indices) as numpy.  ``pad_cols`` > 0: the operands are
    column slices of wider device matrices (lda, ldb > dim), the other columns filled with junk."""
    def dev(m):
        m = np.ascontiguousarray(m, dtype=np.float32)
        if not pad_cols:
            return torch.from_numpy(m).to(DEV)
        wide = torch.full((m.shape[0], m.shape[1] + 2 * pad_cols), 7.5, dtype=torch.float32, device=DEV)
        wide[:, pad_cols:pad_cols + m.shape[1]] = torch.from_numpy(m).to(DEV)
        return wide[:, pad_cols:pad_cols + m.shape[1]]
    ta, tb = dev(a), dev(b)
    ha, hb, dim = ta.shape[0], tb.shape[0], ta.shape[1]
    lib = N.lib()
    need = lib.wsae_match_workspace_bytes(ha, hb, dim, n, PREC[precision])
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    vals = torch.full((ha, n), 123.0, dtype=torch.float32, device=DEV)
    idx = torch.full((ha, n), -7, dtype=torch.int32, device=DEV)
    N.check(lib.wsae_match_rows(ta.data_ptr(), ha, ta.stride(0), tb.data_ptr(), hb, tb.stride(0), dim, METRIC[metric],
                                PREC[precision], n, int(exclude_self), vals.data_ptr(), idx.data_ptr(), ws.data_ptr(), need,
                                torch.cuda.current_stream().cuda_stream), "wsae_match_rows")
    torch.cuda.synchronize()
    return vals.cpu().numpy(), idx.cpu().numpy()


# ---- 1. exact cases ----------------------------------------------------------------------------------------------------
# (130, 33000, 32, 16): with two row tiles the splits take two column tiles each from 32769 columns on, so this is the
# case in which one workgroup carries its lists across tiles
EXACT = [(1, 1, 32, 1, False), (33, 5, 32, 16, False), (257, 129, 96, 4, False), (130, 4099, 64, 16, False),
         (300, 300, 64, 8, True), (130, 33000, 32, 16, False)]


@pytest.fixture(scope="module")
def exact_cases():
    out = {}
    for k, (ra, rb, dim, n, ex) in enumerate(EXACT):
        rng = np.random.default_rng(100 + k)
        a = rng.integers(-2, 3, (ra, dim)).astype(np.float32)
        b = a if ex else rng.integers(-2, 3, (rb, dim)).astype(np.float32)
        out[(ra, rb, dim, n, ex)] = (a, b, MO.top_n(MO.similarity(a, b, "dot"), n, exclude_self=ex))
    return out


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("case", EXACT, ids=lambda c: "x".join(str(v) for v in c))
def test_exact_integer_dot_products_bit_for_bit(exact_cases, case, precision):
    a, b, (want_v, want_i) = exact_cases[case]
    n, ex = case[3], case[4]
    vals, idx = match(a, b, n, metric="dot", precision=precision, exclude_self=ex)
    assert np.array_equal(idx, want_i), np.argwhere(idx != want_i)[:5]
    assert np.array_equal(vals.astype(np.float64), want_v)
    if case[1] < n:
        assert np.all(idx[:, case[1]:] == -1) and np.all(np.isneginf(vals[:, case[1]:]))


# ---- 2. planted ties ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("rows_b,copies", [(700, (5, 133, 300, 697)), (33000, (7, 200, 290, 16500, 32997))],
                         ids=["one_tile_per_split", "two_tiles_per_split"])
def test_planted_ties_across_tiles_and_splits(rows_b, copies, precision):
    rng = np.random.default_rng(7)
    dim, n = 32, len(copies)
    a = rng.standard_normal((130, dim)).astype(np.float32)
    b = rng.standard_normal((rows_b, dim)).astype(np.float32)
    planted = (3, 64, 129)
    for t, i in enumerate(planted):
        for c in copies:
            b[c + t] = a[i] * np.float32(0.37)  # bit-identical copies of one row, in different tiles and splits
    vals, idx = match(a, b, n, precision=precision)
    for t, i in enumerate(planted):
        assert idx[i].tolist() == [c + t for c in copies]
        assert np.all(vals[i] == vals[i, 0]) and abs(vals[i, 0] - 1.0) <= MO.bound(dim, precision)


# ---- 3. random cosines against the float64 oracle ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_cases():
    out = {}
    for dim in (32, 384, 1280):
        rng = np.random.default_rng(dim)
        ra, rb = 197, 333
        a = rng.standard_normal((ra, dim)) * 10.0 ** rng.uniform(-3, 3, (ra, 1))
        b = rng.standard_normal((rb, dim)) * 10.0 ** rng.uniform(-3, 3, (rb, 1))
        a[11] = 0.0
        b[17] = 0.0
        a, b = a.astype(np.float32), b.astype(np.float32)
        sim = MO.similarity(a, b)
        sim_ex = sim.copy()
        d = np.arange(min(ra, rb))
        sim_ex[d, d] = -np.inf
        out[dim] = (a, b, sim, -np.sort(-sim, axis=1), -np.sort(-sim_ex, axis=1))
    return out


@pytest.mark.parametrize("exclude_self", [False, True], ids=["all", "exclude_self"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("n", [1, 4, 16])
@pytest.mark.parametrize("dim", [32, 384, 1280])
def test_random_cosine_within_the_derived_bound(random_cases, dim, n, precision, exclude_self):
    a, b, sim, sorted_all, sorted_ex = random_cases[dim]
    vals, idx = match(a, b, n, precision=precision, exclude_self=exclude_self, pad_cols=8)
    e = MO.bound(dim, precision)
    rows = np.arange(a.shape[0])[:, None]
    assert idx.min() >= 0 and idx.max() < b.shape[0]
    err_pair = np.abs(vals - sim[rows, idx])
    err_rank = np.abs(vals - (sorted_ex if exclude_self else sorted_all)[:, :n])
    print(f"dim {dim} n {n} {precision}: worst error / bound = {max(err_pair.max(), err_rank.max()) / e:.3f}")
    assert err_pair.max() <= e and err_rank.max() <= e
    assert np.all(np.diff(vals, axis=1) <= 0)
    for i in range(a.shape[0]):
        assert len(set(idx[i].tolist())) == n
    if exclude_self:
        assert not np.any(idx == rows)
    assert np.all(vals[11] == 0.0)  # the all-zero row of A


# ---- 4. recovered permutation ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_recovered_permutation(precision):
    rng = np.random.default_rng(4)
    H, D = 1024, 384
    a = rng.standard_normal((H, D))
    a = (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)
    perm = rng.permutation(H)
    b = (a[perm] + 1e-3 * rng.standard_normal((H, D))).astype(np.float32)
    inv = np.argsort(perm).astype(np.int32)
    top = -np.sort(-MO.similarity(a, b), axis=1)[:, :2]
    assert np.array_equal(MO.top_n(MO.similarity(a, b), 1)[1][:, 0], inv)
    assert (top[:, 0] - top[:, 1]).min() > 100 * MO.bound(D, "bf16")  # the gap to the runner-up dwarfs the error
    vals, idx = match(a, b, 2, precision=precision)
    assert np.array_equal(idx[:, 0], inv)


# ---- 5. determinism ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_two_calls_and_appended_rows_give_the_same_bits(precision):
    rng = np.random.default_rng(5)
    a = rng.standard_normal((150, 64)).astype(np.float32)
    b = rng.standard_normal((300, 64)).astype(np.float32)
    assert MO.top_n(MO.similarity(a, b), 4)[0].min() > 0.05  # zero rows cannot enter
    v1, i1 = match(a, b, 4, precision=precision)
    v2, i2 = match(a, b, 4, precision=precision)
    assert np.array_equal(v1.view(np.uint32), v2.view(np.uint32)) and np.array_equal(i1, i2)
    for extra in (1, 5000):  # other tile counts, other splits
        v3, i3 = match(a, np.concatenate([b, np.zeros((extra, 64), np.float32)]), 4, precision=precision)
        assert np.array_equal(v1.view(np.uint32), v3.view(np.uint32)) and np.array_equal(i1, i3)


# ---- 6. the Python layer on bound modules ------------------------------------------------------------------------------
def make_sae(D, H, seed, cls=TopKSAE, **kw):
    torch.manual_seed(seed)
    return cls(D, H, **kw).to(DEV)


def test_compare_a_dictionary_with_itself_and_with_a_permutation():
    D, H = 64, 384
    sae = make_sae(D, H, 1, k=8)
    for precision in ("fp32", "bf16"):
        rep = compare_dictionaries(sae, sae, precision=precision)
        e = MO.bound(D, precision)
        assert abs(rep["mmcs_a_to_b"] - 1.0) <= e and abs(rep["mmcs_b_to_a"] - 1.0) <= e
        assert rep["mutual_nearest"] == H and rep["mutual_pairs"] == [[i, i] for i in range(H)]
        assert rep["fraction_at_least"]["a"] == {"0.5": 1.0, "0.7": 1.0, "0.9": 1.0}
        assert sum(rep["histogram"]["a"]["counts"]) == H and rep["histogram"]["b"]["counts"][-1] == H
    import json
    json.dumps(rep)
    # the rows were read in place: a bound module's decoder rows are the pack's W_dT rows
    eng = sae.bind()
    assert sae.decoder.weight.data_ptr() == eng.pack.data_ptr() + 4 * eng.off[1]
    other = make_sae(D, H, 2, k=8)
    perm = torch.randperm(H, generator=torch.Generator().manual_seed(3)).to(DEV)
    with torch.no_grad():
        other.decoder.weight.copy_(sae.decoder.weight[:, perm])
        other.encoder.weight.copy_(sae.encoder.weight[perm])
    inv = torch.argsort(perm).int()
    for which in ("decoder", "encoder"):
        nf = nearest_features(sae, other, n=1, which=which)
        assert torch.equal(nf.indices[:, 0], inv)
    rep = compare_dictionaries(sae, other)
    assert rep["mutual_pairs"] == [[i, int(inv[i])] for i in range(H)]


def test_other_module_families_and_tensors():
    D, H = 64, 256
    relu = make_sae(D, H, 5, cls=ReLUSAE)
    tc = TopKTranscoder(D, 40, H, k=8).to(DEV)  # output width 40: the pack rows are 64 wide, zero beyond column 40
    for mod in (relu, tc):
        nf = nearest_features(mod, n=3)
        w = mod.decoder.weight.detach().t().cpu().numpy()
        want_v, want_i = MO.top_n(MO.similarity(w, w), 3, exclude_self=True)
        err = np.abs(nf.values.cpu().numpy() - MO.similarity(w, w)[np.arange(H)[:, None], nf.indices.cpu().numpy()])
        assert err.max() <= MO.bound(D) and np.abs(nf.values.cpu().numpy() - want_v).max() <= MO.bound(D)
    # tensors: a non-contiguous one, a width that is no multiple of 32
    t = torch.randn(40, 100, device=DEV).t()
    nf = nearest_features(t, t.clone(), n=1)
    assert torch.equal(nf.indices[:, 0], torch.arange(100, device=DEV, dtype=torch.int32))
    with pytest.raises(ValueError):
        nearest_features(torch.zeros(8, 32, device=DEV), torch.zeros(8, 64, device=DEV))
    with pytest.raises(N.WsaeError):
        nearest_features(torch.zeros(8, 32), torch.zeros(8, 32))


def test_duplicate_features_finds_the_planted_pairs():
    D, H = 64, 384
    sae = make_sae(D, H, 6, k=8)
    planted = [(3, 200), (17, 18), (100, 383)]
    with torch.no_grad():
        for t, (i, j) in enumerate(planted):
            noise = torch.randn(D, device=DEV) * (0.04 * (t + 1)) * sae.decoder.weight[:, i].norm() / D ** 0.5
            sae.decoder.weight[:, j] = 2.0 * sae.decoder.weight[:, i] + noise
    w = sae.decoder.weight.detach().t().cpu().numpy()
    sim = MO.similarity(w, w)
    want = sorted(((i, j, sim[i, j]) for i in range(H) for j in range(i + 1, H) if sim[i, j] >= 0.9),
                  key=lambda t: (-t[2], t[0], t[1]))
    assert [(i, j) for i, j, _ in want] == planted  # random 64-dimensional directions stay far below 0.9
    got = duplicate_features(sae, threshold=0.9)
    assert [(i, j) for i, j, _ in got] == planted
    assert all(abs(g[2] - w_[2]) <= MO.bound(D) for g, w_ in zip(got, want))


def test_crosscoder_layer_slice_equals_its_contiguous_copy():
    cc = TopKCrossLayerCrosscoder(d_model=64, n_layers=3, d_sae=320, k=8, layer_indices=[1, 4, 6]).to(DEV)
    with torch.no_grad():
        cc.W_dec.copy_(torch.randn_like(cc.W_dec))
    sae = make_sae(64, 256, 8, k=8)
    for layer, i in ((1, 0), (6, 2)):
        for which in ("decoder", "encoder"):
            src = cc.W_dec[:, i, :] if which == "decoder" else cc.W_enc[i].t()
            copy = src.detach().contiguous().clone()
            a = nearest_features(cc, n=4, layer=layer, which=which)
            b = nearest_features(copy, n=4, which=which)
            assert torch.equal(a.indices, b.indices) and torch.equal(a.values, b.values)
    x = nearest_features(cc, sae, n=2, layer=4)
    y = nearest_features(cc.W_dec[:, 1, :].detach().contiguous(), sae.decoder.weight.detach().t().contiguous(), n=2)
    assert torch.equal(x.indices, y.indices) and torch.equal(x.values, y.values)
    with pytest.raises(ValueError):
        nearest_features(cc, n=2)          # a crosscoder needs layer=
    with pytest.raises(ValueError):
        nearest_features(cc, n=2, layer=2)  # not one of its layers


def test_nearest_features_leaves_parameters_and_the_next_train_step_alone():
    D, H, K, B = 64, 512, 8, 256
    x = torch.randn(B, D, generator=torch.Generator().manual_seed(9))
    losses, packs = [], []
    for probe in (False, True):
        sae = make_sae(D, H, 11, k=K)
        with tempfile.TemporaryDirectory(prefix="wsae_match_") as run_dir:
            trainer = SAETrainer(sae, TrainingConfig(batch_size=B, learning_rate=1e-3, warmup_steps=0, use_amp=True,
                                                     num_workers=0), device=DEV, run_dir=run_dir)
            trainer.train_step(x)
            before = {k: v.detach().clone() for k, v in sae.state_dict().items()}
            if probe:
                nearest_features(sae, n=4, precision="bf16")
                nearest_features(sae, sae, n=16, which="encoder")
                compare_dictionaries(sae, sae)
                for k, v in sae.state_dict().items():
                    assert torch.equal(v, before[k]), k
            losses.append(trainer.train_step(x).loss)
            packs.append({k: v.detach().clone() for k, v in sae.state_dict().items()})
    assert np.float32(losses[0]).view(np.uint32) == np.float32(losses[1]).view(np.uint32)
    for k in packs[0]:
        assert torch.equal(packs[0][k], packs[1][k]), k
