"""The list-building plumbing that ``wsae_sta_update``, ``wsae_probe_plan`` / ``wsae_probe_backward``,
``wsae_feature_topk_update`` and ``wsae_sample_update`` share (csrc/wsae_lists.h), on the MI355X, at the sizes where a scan
or an offsets kernel can go wrong: one list, one list fewer and one more than the 1024 threads of the single-workgroup
kernels and than their 1024-wide steps, a column count that crosses the 4096-column walk tile, a ragged last chunk of rows,
lists that are empty, and a workspace that ends exactly where the query says.  Every entry point is called through the C
ABI and compared exactly with the numpy oracle its own test file uses; the oracles themselves are pinned there."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import probe_oracle as PB
import profile_oracle as PO
import sta_oracle as SO
from oracle.feature_topk import FeatureTopK
from whisper_sae import _native as N

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROWS = 200  # with 64-row chunks: four chunks, the last one of 8 rows
GUARD = 4096
SEG = (np.arange(ROWS) // 50).astype(np.int32)
SEG[[7, 63, 64, 130, 199]] = -1  # padding rows, at chunk edges too


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def stream():
    return torch.cuda.current_stream().cuda_stream


def guarded(need):
    """A workspace of exactly ``need`` bytes with a poisoned guard behind it."""
    assert need >= 0
    return torch.full((need + GUARD,), 0xAB, dtype=torch.uint8, device=DEV)


def guard_intact(ws, need):
    return bool((ws[need:] == 0xAB).all())


def make_code(seed, rows, k, hidden):
    """A code with long and empty lists: four entries in ten name one of a few hot features (the first, the last and three
    between), the rest any feature; a fifth of the values is not positive, one index in a hundred is out of range, and an
    index may repeat within a row."""
    rng = np.random.default_rng(seed)
    vals = (rng.standard_normal((rows, k)) + 0.8).astype(np.float32)
    idx = rng.integers(0, hidden, (rows, k)).astype(np.int32)
    hot = np.unique(np.array([0, hidden // 3, hidden // 2, hidden - 2, hidden - 1]).clip(0, hidden - 1)).astype(np.int32)
    pick = rng.random((rows, k)) < 0.4
    idx[pick] = rng.choice(hot, int(pick.sum()))
    bad = rng.random((rows, k)) < 0.01
    idx[bad] = rng.choice(np.array([-1, hidden, hidden + 9], np.int32), int(bad.sum()))
    return vals, idx


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    view = {8: np.int64, 4: np.int32}[a.dtype.itemsize]
    assert np.array_equal(a.view(view), b.view(view)), np.argwhere(a.view(view) != b.view(view))[:5]


# ---- wsae_probe_plan and wsae_probe_backward ----------------------------------------------------------------------------------
def probe_plan_and_backward(code, seg, hidden, col_of, P, C=3):
    vals, idx = code
    rows, k = vals.shape
    want = PB.plan(PB.entries(code, seg, hidden, col_of), P)
    nnz = int(want[0][-1])
    lib = N.lib()
    v, i, s = dev(vals), dev(idx), dev(seg)
    cmap = None if col_of is None else dev(col_of)
    cap = rows * k
    col_ptr = torch.full((P + 1 + 3,), 0x5a5a5a5, dtype=torch.int64, device=DEV)
    t_row = torch.full((cap,), -7, dtype=torch.int32, device=DEV)
    t_val = torch.full((cap,), -7.0, dtype=torch.float32, device=DEV)
    out_nnz = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    need = lib.wsae_probe_plan_workspace_bytes(rows, k, hidden, P)
    ws = guarded(need)
    N.check(lib.wsae_probe_plan(v.data_ptr(), i.data_ptr(), k, hidden, s.data_ptr(), rows, N.ptr(cmap), P, col_ptr.data_ptr(),
                                t_row.data_ptr(), t_val.data_ptr(), cap, out_nnz.data_ptr(), ws.data_ptr(), need, stream()),
            "wsae_probe_plan")
    torch.cuda.synchronize()
    assert guard_intact(ws, need) and bool((col_ptr[P + 1:] == 0x5a5a5a5).all())  # col_ptr has P + 1 elements, no more
    assert int(out_nnz[0]) == nnz and np.array_equal(col_ptr[:P + 1].cpu().numpy(), want[0])
    assert np.array_equal(t_row[:nnz].cpu().numpy(), want[1])
    same_bits(t_val[:nnz].cpu().numpy(), want[2])
    assert bool((t_row[nnz:] == -7).all())
    # the backward product over the lists cut to two thirds: columns behind the cut are clipped or empty
    cut = 2 * nnz // 3
    rng = np.random.default_rng(rows + P)
    lde = C + 2
    err = rng.standard_normal((rows, lde)).astype(np.float32)
    gW0, gb0 = rng.standard_normal((P, C)), rng.standard_normal(C)
    gW, gb = dev(gW0), dev(gb0)
    need = lib.wsae_probe_backward_workspace_bytes(rows, P, C, cut)
    ws = guarded(need)
    N.check(lib.wsae_probe_backward(col_ptr.data_ptr(), t_row.data_ptr(), t_val.data_ptr(), cut, P, dev(err).data_ptr(), lde, C,
                                    rows, gW.data_ptr(), gb.data_ptr(), ws.data_ptr(), need, stream()), "wsae_probe_backward")
    torch.cuda.synchronize()
    assert guard_intact(ws, need)
    wW, wb = PB.backward((np.minimum(want[0], cut), want[1][:cut], want[2][:cut]), err, C, gW0, gb0)
    same_bits(gW.cpu().numpy(), wW)
    same_bits(gb.cpu().numpy(), wb)
    return want


@pytest.mark.parametrize("subset", [False, True], ids=["identity", "subset"])
@pytest.mark.parametrize("P", [1, 63, 1023, 1024, 1025, 4097])
@pytest.mark.parametrize("k", [8, 72])
def test_probe_plan_and_backward(k, P, subset):
    hidden = 2 * P if subset else P
    col_of = np.where(np.arange(hidden) % 2 == 0, np.arange(hidden) // 2, -1).astype(np.int32) if subset else None
    want = probe_plan_and_backward(make_code(100 + k, ROWS, k, hidden), SEG, hidden, col_of, P)
    lens = np.diff(want[0])
    assert lens.max() > 64 and (P < 64 or k > 8 or (lens == 0).any())  # a list longer than a wave; empty ones in the sparse code


def test_probe_columns_of_no_and_of_exactly_one_chunk_of_entries():
    rows, k, P = 5000, 8, 70
    vals, idx = make_code(7, rows, k, P)
    idx[idx == 1] = 3
    idx[idx == 2] = 3
    idx[:, 0], vals[:, 0] = 0, np.abs(vals[:, 0]) + 0.1      # column 0: every row, two full pieces and a ragged one
    at = np.random.default_rng(8).choice(rows, PB.CHUNK, replace=False)
    idx[at, 1], vals[at, 1] = 1, 0.5                         # column 1: exactly one piece; column 2: nothing
    seg = (np.arange(rows) // 700).astype(np.int32)
    want = probe_plan_and_backward((vals, idx), seg, P, None, P)
    lens = np.diff(want[0])
    assert lens[0] == rows and lens[1] == PB.CHUNK and lens[2] == 0 and 2 * int(want[0][-1]) // 3 > int(want[0][3])


# ---- wsae_sta_update ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trigger", [SO.ALL, SO.ONSET], ids=["all", "onset"])
@pytest.mark.parametrize("f_cols", [1, 1023, 1025, 4097])
def test_sta_update(f_cols, trigger):
    k, C, lags, f_lo = 8, 2, (-1, 1), 3
    hidden = f_cols + 7
    code = make_code(200 + f_cols, ROWS, k, hidden)
    code[1][code[1] == 0] = f_lo  # (the first hot feature moves into the window)
    y = np.random.default_rng(f_cols).standard_normal((ROWS, C)).astype(np.float32)
    want = SO.update(code, hidden, SEG, y, lags, f_lo, f_cols, trigger, SO.VALUE)
    L = lags[1] - lags[0] + 1
    acc = torch.zeros(f_cols, L, C, dtype=torch.float64, device=DEV)
    wsum = torch.zeros(f_cols, L, dtype=torch.float64, device=DEV)
    cnt = torch.zeros(f_cols, L, dtype=torch.int64, device=DEV)
    lib = N.lib()
    need = lib.wsae_sta_workspace_bytes(ROWS, k, hidden, f_lo, f_cols)
    ws = guarded(need)
    v, i, s, yd = dev(code[0]), dev(code[1]), dev(SEG), dev(y)
    N.check(lib.wsae_sta_update(v.data_ptr(), i.data_ptr(), k, hidden, s.data_ptr(), ROWS, yd.data_ptr(), N.DT_F32, C, C, lags[0],
                                lags[1], f_lo, f_cols, trigger, SO.VALUE, acc.data_ptr(), wsum.data_ptr(), cnt.data_ptr(),
                                ws.data_ptr(), need, stream()), "wsae_sta_update")
    torch.cuda.synchronize()
    assert guard_intact(ws, need)  # (nothing is written behind the last section)
    for name, got in (("acc", acc), ("wsum", wsum), ("cnt", cnt)):
        same_bits(got.cpu().numpy(), want[name])
    assert want["cnt"].max() > 20 and (f_cols == 1 or (want["cnt"].sum(1) == 0).any())


# ---- wsae_feature_topk_update -------------------------------------------------------------------------------------------------
def topk_case(H, only_ends=False):
    """300 rows of distinct features per row and values on a grid of quarters: many equal values inside the lists and at
    their boundary, some not positive."""
    rng = np.random.default_rng(300 + H + only_ends)
    rows = 300
    if only_ends:
        idx = np.tile(np.array([0, H - 1], np.int32), (rows, 1))
    else:
        width = min(4, H)
        hot = np.array([0, H // 2, H - 1])
        idx = np.stack([rng.permutation(H)[:width] if rng.random() < 0.5 or H < 4 else
                        np.concatenate([hot, rng.choice(np.setdiff1d(np.arange(H), hot), 1)]) for _ in range(rows)]).astype(np.int32)
    vals = (rng.integers(-2, 12, idx.shape) / 4.0).astype(np.float32)
    return vals, idx


def run_topk(vals, idx, H, keep, dense):
    """Two calls (180 rows, then the rest, which meets the lists of the first) -> (values, ordinals, counts, total)."""
    lib = N.lib()
    top_v = torch.zeros(H, keep, dtype=torch.float32, device=DEV)
    top_o = torch.zeros(H, keep, dtype=torch.int64, device=DEV)
    top_c = torch.zeros(H, dtype=torch.int32, device=DEV)
    total = torch.zeros(1, dtype=torch.int64, device=DEV)
    for lo, hi in ((0, 180), (180, vals.shape[0])):
        v, i = vals[lo:hi], idx[lo:hi]
        if dense:
            full = np.zeros((hi - lo, H), np.float32)
            np.put_along_axis(full, i.astype(np.int64), v, axis=1)
            v, i = full, None
        vd, idd = dev(v), None if i is None else dev(i)
        need = lib.wsae_feature_topk_workspace_bytes(v.size, H)
        ws = guarded(need)
        N.check(lib.wsae_feature_topk_update(vd.data_ptr(), N.ptr(idd), hi - lo, v.shape[1], H, keep, lo, top_v.data_ptr(),
                                             top_o.data_ptr(), top_c.data_ptr(), total.data_ptr(), ws.data_ptr(), need, stream()),
                "wsae_feature_topk_update")
        torch.cuda.synchronize()
        assert guard_intact(ws, need)
    return top_v.cpu().numpy(), top_o.cpu().numpy(), top_c.cpu().numpy(), int(total[0])


_topk_wants = {}


def topk_want(H, keep, only_ends):
    """Computed once per shape and shared by the two forms; never modified."""
    key = (H, keep, only_ends)
    if key not in _topk_wants:
        vals, idx = topk_case(H, only_ends)
        o = FeatureTopK(H, keep)
        o.update_compact(vals[:180], idx[:180])
        o.update_compact(vals[180:], idx[180:])
        _topk_wants[key] = (vals, idx, o.arrays(), o.total_activations)
    return _topk_wants[key]


def check_topk(H, keep, dense, only_ends=False):
    vals, idx, (wv, wo, wc), total = topk_want(H, keep, only_ends)
    gv, go, gc, gt = run_topk(vals, idx, H, keep, dense)
    assert gt == total and np.array_equal(gc, wc)
    held = np.arange(keep)[None, :] < wc[:, None]
    assert np.array_equal(gv[held], wv[held]) and np.array_equal(go[held], wo[held])
    return wc


@pytest.mark.parametrize("dense", [False, True], ids=["compact", "dense"])
@pytest.mark.parametrize("keep", [1, 5, 64])
@pytest.mark.parametrize("H", [1, 1023, 1024, 1025, 2049])
def test_feature_topk_update(H, keep, dense):
    wc = check_topk(H, keep, dense)
    assert wc.max() == keep and wc[-1] == keep and (H == 1 or (wc < keep).any())


@pytest.mark.parametrize("dense", [False, True], ids=["compact", "dense"])
def test_feature_topk_update_with_empty_lists_between_the_first_and_the_last(dense):
    wc = check_topk(2049, 64, dense, only_ends=True)
    assert wc[0] == 64 and wc[-1] == 64 and not wc[1:-1].any()


# ---- wsae_sample_update -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep", [1, 64])
@pytest.mark.parametrize("f_cols,S", [(1, 1), (341, 3), (205, 5), (683, 3)], ids=lambda x: str(x))
def test_sample_update(f_cols, S, keep):
    """``f_cols * S`` = 1, 1023, 1025 and 2049 lists; two calls of 800 rows, the second of which meets lists that are full: the
    first feature of the window is active on every row."""
    k, seed, f_lo, rows = 8, 12345, 2, 800
    seg = (np.arange(rows) // 200).astype(np.int32)
    seg[[7, 255, 256, 799]] = -1
    hidden = f_cols + 5
    window = (f_lo, f_cols)
    edges = None if S == 1 else np.tile(np.linspace(0.3, 1.5, S - 1, dtype=np.float32), (f_cols, 1))
    lib = N.lib()
    keys = torch.full((f_cols, S, keep), -1, dtype=torch.int64, device=DEV)
    svals = torch.zeros(f_cols, S, keep, dtype=torch.float32, device=DEV)
    seen = torch.zeros(f_cols, S, dtype=torch.int32, device=DEV)
    ed = None if edges is None else dev(edges)
    want = None
    for call in range(2):
        vals, idx = make_code(400 + f_cols + call, rows, k, hidden)
        idx[:, 0], vals[:, 0] = f_lo, np.abs(vals[:, 0]) + np.float32(0.05)
        want = PO.sample((vals, idx), seg, call * rows, edges, keep, seed, hidden, window, want)
        if call == 0:
            assert (want["keys"][0, :, -1] != PO.EMPTY).all()  # full lists for the second call to meet
        v, i, s = dev(vals), dev(idx), dev(seg)
        need = lib.wsae_sample_workspace_bytes(rows, k, hidden, f_lo, f_cols, S, keep)
        ws = guarded(need)
        N.check(lib.wsae_sample_update(v.data_ptr(), i.data_ptr(), k, hidden, s.data_ptr(), rows, call * rows, f_lo, f_cols,
                                       N.ptr(ed), S, keep, seed, keys.data_ptr(), svals.data_ptr(), seen.data_ptr(), ws.data_ptr(),
                                       need, stream()), "wsae_sample_update")
        torch.cuda.synchronize()
        assert guard_intact(ws, need)
        assert np.array_equal(keys.cpu().numpy().view(np.uint64), want["keys"])
        same_bits(svals.cpu().numpy(), want["svals"])
        assert np.array_equal(seen.cpu().numpy(), want["seen"])
    assert f_cols == 1 or (want["seen"] == 0).any()
