"""Token association without a GPU: the dict oracle of tests/token_oracle.py against a brute-force dense count, the
published hash against hand-checked values and a sequential probing table (wrap-around, a full table), the conditions that
keep the GPU test inputs from being degenerate, every argument error of the three entry points (raised before any HIP
call), the workspace query, the header / ``SIGNATURES`` / constants / exports, and the Python layer's argument errors."""

from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest

import profile_oracle as PO
import token_oracle as TO

HEADER = Path(__file__).resolve().parents[1] / "include" / "wsae.h"
NAMES = ("wsae_pair_update", "wsae_pair_merge", "wsae_pair_top_workspace_bytes", "wsae_pair_top")


# ---- the oracle -----------------------------------------------------------------------------------------------------------------
def test_oracle_equals_a_brute_force_dense_count():
    rng = np.random.default_rng(11)
    rows, k, hidden, n_tokens = 400, 6, 40, 300
    vals = rng.uniform(-0.3, 2.0, (rows, k)).astype(np.float32)
    vals[3, 1], vals[4, 2], vals[9, 0] = np.nan, np.inf, 5000.0
    idx = rng.integers(-1, hidden + 1, (rows, k)).astype(np.int32)
    seg = (np.arange(rows) // 23).astype(np.int32)
    seg[rng.random(rows) < 0.1] = -1
    tokens = TO.zipf_tokens(rng, rows, n_tokens, 2, 7)
    tokens[rng.random(rows) < 0.1] = -1
    tokens[rng.random(rows) < 0.05] = n_tokens
    for lag in (0, -3, 2, 30):
        for s in (seg, None):
            st = TO.update((vals, idx), s, tokens, hidden, n_tokens, lag)
            cnt, sums, feat, tokr, pairs = TO.update_dense((vals, idx), s, tokens, hidden, n_tokens, lag)
            ex = TO.export(st)
            f, t = np.nonzero(cnt)
            assert np.array_equal(ex["feature"], f) and np.array_equal(ex["token"], t)  # (both ascending by feature, token)
            assert np.array_equal(ex["count"], cnt[f, t]) and np.array_equal(ex["sum_q"], sums[f, t])
            assert np.array_equal(st["feat_rows"], feat) and np.array_equal(st["tok_rows"], tokr) and st["pair_rows"][0] == pairs
            assert np.array_equal(feat, cnt.sum(1)) and (lag == 30 or pairs > 100)
    # two calls over whole utterances, in either order, and the merge of two shards equal one call
    cut = 23 * 9
    whole = TO.update((vals, idx), seg, tokens, hidden, n_tokens, -3)
    a = TO.update((vals[:cut], idx[:cut]), seg[:cut], tokens[:cut], hidden, n_tokens, -3)
    b = TO.update((vals[cut:], idx[cut:]), seg[cut:], tokens[cut:], hidden, n_tokens, -3)
    ab = TO.update((vals[cut:], idx[cut:]), seg[cut:], tokens[cut:], hidden, n_tokens, -3, state=a)
    for st in (ab, TO.merge(a, b), TO.merge(b, a)):
        TO.same_export(TO.export(st), TO.export(whole))
        TO.same_marginals(st, whole)


def test_pair_rule_one_row_per_drop_reason():
    vals, idx = np.ones((8, 1), np.float32), np.ones((8, 1), np.int32)
    seg = [0, 0, -1, 0, 1, 1, 1, 1]
    tokens = [2, 1, 0, 0, 1, -1, 3, 2]
    # lag +1, 3 tokens.  (0): token 1, kept.  (1): neighbour 2 is padding.  (2): row 2 is padding.  (3): neighbour 4 is in
    # utterance 1.  (4): token -1.  (5): token 3 is outside.  (6): token 2, kept.  (7): 8 is outside the call.
    assert TO.pair_tokens(seg, tokens, 8, 3, 1).tolist() == [1, -1, -1, -1, -1, -1, 2, -1]
    assert TO.pair_tokens(None, tokens, 8, 3, 1).tolist() == [1, 0, 0, 1, -1, -1, 2, -1]
    st = TO.update((vals, idx), seg, tokens, 4, 3, 1)
    assert st["table"] == {TO.key_of(1, 1): [1, 1 << 20], TO.key_of(1, 2): [1, 1 << 20]}
    assert st["feat_rows"].tolist() == [0, 2, 0, 0] and st["tok_rows"].tolist() == [0, 1, 1] and st["pair_rows"][0] == 2
    # the value of a repeated index is that of its first ACTIVE entry; values saturate at 4096
    st = TO.update((np.array([[-1.0, 0.5, 2.0], [np.nan, 8192.0, 1.0]], np.float32), np.full((2, 3), 2, np.int32)), None, [0, 0], 4, 1)
    assert st["table"] == {TO.key_of(2, 0): [2, (1 << 19) + (4096 << 20)]}


def test_hash_and_probing():
    assert TO.splitmix64(0) == 0  # (the finaliser of splitmix64, without the increment)
    x = 0x123456789ABCDEF
    y = x ^ x >> 30
    y = y * 0xBF58476D1CE4E5B9 % 2 ** 64
    y ^= y >> 27
    y = y * 0x94D049BB133111EB % 2 ** 64
    assert TO.splitmix64(x) == y ^ y >> 31
    assert TO.key_of(2 ** 31 - 1, 2 ** 24 - 1) < TO.EMPTY
    # the collision case: 8 keys start in the last slot and 8 in the one before, so some wrap around to slots 0, 1, ...
    code, tokens, keys = TO.collision_case()
    assert len(set(keys)) == 416 and sum(TO.home_slot(k, 1024) == 1023 for k in keys) >= 8
    assert sum(TO.home_slot(k, 1024) == 1022 for k in keys) >= 8
    slots, placed = TO.probe_table(keys, 1024)
    assert min(placed) >= 0 and sorted(k for k in slots if k != TO.EMPTY) == sorted(keys)
    wrapped = [k for k, s in zip(keys, placed) if s < TO.home_slot(k, 1024)]
    assert len(wrapped) >= 14 and {0, 1, 2, 3} <= {placed[keys.index(k)] for k in wrapped}
    st = TO.update(code, None, tokens, 64, 4096)
    assert sorted(st["table"]) == sorted(keys) and [st["table"][k][0] for k in keys] == [1 + i % 5 for i in range(416)]
    # an overfull table: cap probes find nothing, exactly cap keys land
    many = [TO.key_of(i % 50, i) for i in range(2000)]
    slots, placed = TO.probe_table(many, 1024)
    assert sum(p >= 0 for p in placed) == 1024 and TO.EMPTY not in slots


def test_conditions_on_the_gpu_test_inputs():
    code, seg, tokens = TO.general_case()
    vals, idx = code
    assert vals.shape == (TO.ROWS, TO.K) and TO.ROWS * TO.K > 256 and np.unique(seg[seg >= 0]).size == TO.UTTS
    assert (seg < 0).any() and (tokens < 0).any() and (tokens >= TO.TOKENS).any() and np.isnan(vals).any() and np.isinf(vals).any()
    live = seg >= 0
    for lag in TO.LAGS:
        tok = TO.pair_tokens(seg, tokens, TO.ROWS, TO.TOKENS, lag)
        q = np.arange(TO.ROWS) + lag
        inside = (q >= 0) & (q < TO.ROWS)
        qc = np.clip(q, 0, TO.ROWS - 1)
        cut = live & inside & (seg[qc] >= 0) & (seg[qc] != seg)
        assert (lag == 0 or cut.any()) and (tok[cut] < 0).all()  # cut by the lag at an utterance edge
        assert (live & inside & (seg[qc] == seg) & (tokens[qc] < 0)).any()  # no token
        st = TO.update(code, seg, tokens, TO.HIDDEN, TO.TOKENS, lag)
        counts = np.array([c for c, _ in st["table"].values()])
        assert 10_000 < counts.size and (counts < 3).any() and (counts >= 3).sum() > 2000  # some pairs fall below min_count
        assert st["feat_rows"][TO.SILENT] == 0 and (st["tok_rows"] == 0).any()  # a group with no pair in either direction
        for by in (TO.BY_FEATURE, TO.BY_TOKEN):
            for score in TO.SCORES:
                want = TO.top(st, by, score, 1, 32)
                ok = want["ids"][:, 1:] >= 0
                ties = ok & (want["scores"][:, 1:] == want["scores"][:, :-1])
                assert ties.any(), (lag, by, score)  # the id breaks ties
                assert (want["ids"][:, 1:][ties] > want["ids"][:, :-1][ties]).all()
                short = (want["ids"][:, 0] >= 0) & (want["ids"][:, 31] < 0)
                assert short.any() and (want["ids"][:, 0] < 0).any(), (lag, by, score)  # a short list and an empty one
                assert (TO.top(st, by, score, 3, 32)["ids"] >= 0).sum() < (want["ids"] >= 0).sum()
    for k in (1, 31, 32, 33, 128):
        wcode, wseg, wtok = TO.wide_case(k)
        st = TO.update(wcode, wseg, wtok, 300, 40, 1)
        assert len(st["table"]) > 20 and (wseg < 0).any() and (256 % k or k == 1 or 256 // k * k == 256)
        if k > 1:  # row 7: one index in every entry, the first entry not active: its value is that of entry 1
            lone = TO.update((wcode[0][7:8], wcode[1][7:8]), None, [3], 300, 40, 0)
            assert lone["table"] == {TO.key_of(11, 3): [1, int(PO.sum_q_terms(wcode[0][7:8, 1])[0])]}
        assert not TO.update((wcode[0][8:9], wcode[1][8:9]), None, [3], 300, 40, 0)["table"]  # row 8: nothing is active


# ---- argument errors: made-up (aligned, never dereferenced) pointers, every case fails its checks first -------------------------
P = 4096


def _update(N, k=32, hidden=64, n_rows=16, n_tokens=100, lag=0, cap=1024, vals=P, idx=P, seg=P, tokens=P, keys=P, cnt=P, sum_q=P,
            status=P, feat_rows=P, tok_rows=P, pair_rows=P):
    return N.lib().wsae_pair_update(vals, idx, k, hidden, seg, tokens, n_rows, n_tokens, lag, keys, cnt, sum_q, cap, status,
                                    feat_rows, tok_rows, pair_rows, None)


UPDATE_ERRORS = {"k0": dict(k=0), "k129": dict(k=129), "hidden0": dict(hidden=0), "n_rows_negative": dict(n_rows=-1),
                 "n_rows_2p31": dict(n_rows=2 ** 31), "tokens0": dict(n_tokens=0), "tokens_over": dict(n_tokens=(1 << 24) + 1),
                 "lag_below": dict(lag=-1025), "lag_above": dict(lag=1025), "cap_small": dict(cap=512),
                 "cap_not_pow2": dict(cap=1500), "cap_large": dict(cap=2 ** 32), "null_vals": dict(vals=None),
                 "null_idx": dict(idx=None), "null_tokens": dict(tokens=None), "null_keys": dict(keys=None),
                 "null_cnt": dict(cnt=None), "null_sum_q": dict(sum_q=None), "null_status": dict(status=None),
                 "null_feat_rows": dict(feat_rows=None), "null_tok_rows": dict(tok_rows=None), "null_pair_rows": dict(pair_rows=None)}


@pytest.mark.parametrize("kw", list(UPDATE_ERRORS.values()), ids=list(UPDATE_ERRORS))
def test_update_argument_errors_do_not_need_a_gpu(kw):
    from whisper_sae import _native as N
    assert _update(N, **kw) == -1
    assert "wsae_pair_update" in N.last_error()


def _top(N, cap=1024, hidden=64, n_tokens=100, by=0, n_groups=64, score=0, min_count=1, n=10, keys=P, ws=P, ws_bytes=1 << 20,
         ids=P):
    return N.lib().wsae_pair_top(keys, P, P, cap, P, P, P, hidden, n_tokens, by, n_groups, score, min_count, n, ids, P, P, P, ws,
                                 ws_bytes, None)


TOP_ERRORS = {"cap": dict(cap=1000), "hidden0": dict(hidden=0), "tokens_over": dict(n_tokens=(1 << 24) + 1), "by": dict(by=2),
              "groups_feature": dict(n_groups=100), "groups_token": dict(by=1, n_groups=64), "score_low": dict(score=-1),
              "score_high": dict(score=7), "n0": dict(n=0), "n33": dict(n=33), "null_keys": dict(keys=None),
              "null_ids": dict(ids=None), "ws_small": dict(ws_bytes=100), "ws_null": dict(ws=None),
              "ws_unaligned": dict(ws=P + 4)}


@pytest.mark.parametrize("kw", list(TOP_ERRORS.values()), ids=list(TOP_ERRORS))
def test_top_argument_errors_do_not_need_a_gpu(kw):
    from whisper_sae import _native as N
    assert _top(N, **kw) == -1
    assert "wsae_pair_top" in N.last_error()


def test_merge_argument_errors_empty_calls_and_the_workspace_query():
    from whisper_sae import _native as N
    lib = N.lib()
    for args in ((None, P, P, 8, 2 * P, 2 * P, 2 * P, 1024, P), (P, P, P, 0, 2 * P, 2 * P, 2 * P, 1024, P),
                 (P, P, P, 8, 2 * P, 2 * P, 2 * P, 1000, P), (P, P, P, 8, P, 2 * P, 2 * P, 1024, P),
                 (P, P, P, 8, 2 * P, 2 * P, 2 * P, 1024, None), (P, P, P, 2 ** 31 + 1, 2 * P, 2 * P, 2 * P, 1024, P)):
        assert lib.wsae_pair_merge(*args, None) == -1 and "wsae_pair_merge" in N.last_error()
    assert _update(N, n_rows=0) == 0 and _update(N, n_rows=0, seg=None, lag=-1024, n_tokens=1 << 24, cap=1 << 31, k=128) == 0
    q = lib.wsae_pair_top_workspace_bytes
    assert q(1024, 1) >= 4 * 1024 + 8 and q(1 << 31, 1 << 24) >= 4 * (1 << 31) + 8 * (1 << 24)
    assert q(1 << 20, 51865) < (1 << 20) * 4 + 51865 * 8 + 2048  # two words per group, one per slot
    for bad in ((1000, 5), (512, 5), (1 << 32, 5), (1024, 0), (1024, -1)):
        assert q(*bad) == -1, bad


def test_header_signatures_constants_and_exports_agree():
    import whisper_sae.analysis as A
    from whisper_sae import _native as N
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    lib = N.lib()
    for name in NAMES:
        proto = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert proto, name
        assert len(proto.group(1).split(",")) == len(N.SIGNATURES[name][1]), name
        assert getattr(lib, name) is not None
    assert {n for n in N.SIGNATURES if n.startswith("wsae_pair_")} == set(NAMES)
    defines = dict(re.findall(r"#define (WSAE_PAIR_[A-Z0-9_]+) (\(1 << 24\)|\d+)", text))
    assert defines.pop("WSAE_PAIR_MAX_TOKENS") == "(1 << 24)" and N.PAIR_MAX_TOKENS == 1 << 24
    assert {k: int(v) for k, v in defines.items()} == {
        "WSAE_PAIR_MAX_K": N.PAIR_MAX_K, "WSAE_PAIR_MAX_N": N.PAIR_MAX_N, "WSAE_PAIR_BY_FEATURE": N.PAIR_BY_FEATURE,
        "WSAE_PAIR_BY_TOKEN": N.PAIR_BY_TOKEN, **{"WSAE_PAIR_" + s.upper(): i for i, s in enumerate(N.PAIR_SCORES)}}
    assert (N.PAIR_MAX_K, N.PAIR_MAX_N) == (128, 32) and N.PAIR_SCORES == TO.SCORES
    for name in ("TokenAssociation", "TopPairs", "PairExport", "collect_token_association"):
        assert name in A.__all__ and hasattr(A, name)


# ---- the Python layer -----------------------------------------------------------------------------------------------------------
def test_python_layer_argument_errors():
    import torch

    from whisper_sae import _native as N
    from whisper_sae.analysis import TokenAssociation, collect_token_association
    from whisper_sae.sae.model import ReLUSAE
    code = (torch.ones(2, 3, 2), torch.zeros(2, 3, 2, dtype=torch.int32))
    tokens = torch.zeros(2, 3, dtype=torch.int64)
    with pytest.raises(N.WsaeError):
        TokenAssociation(8, 30).update(code, tokens)  # CPU tensors
    with pytest.raises(TypeError):
        TokenAssociation(8, 30).update(torch.ones(2, 3, 2), tokens)
    with pytest.raises(N.WsaeError):
        TokenAssociation(8, 30, device="cpu").top_tokens()
    for kw in (dict(hidden=0), dict(n_tokens=0), dict(n_tokens=(1 << 24) + 1), dict(lag=1025), dict(lag=-1025),
               dict(capacity=1000), dict(capacity=512), dict(capacity=1 << 32)):
        with pytest.raises(ValueError):
            TokenAssociation(**{"hidden": 8, "n_tokens": 30, **kw})
    assert TokenAssociation(8, 1 << 24, lag=-1024, capacity=1024).capacity == 1024
    for bad in (dict(score="nope"), dict(n=0), dict(n=33)):
        with pytest.raises(ValueError):
            TokenAssociation(8, 30).top_tokens(**bad)
        with pytest.raises(ValueError):
            TokenAssociation(8, 30).top_features(**bad)
    for other in (TokenAssociation(9, 30), TokenAssociation(8, 31), TokenAssociation(8, 30, lag=1)):
        with pytest.raises(ValueError):
            TokenAssociation(8, 30).merge(other)
    a, b = TokenAssociation(8, 30), TokenAssociation(8, 30)
    a._submitted, b._submitted = 10, 20
    a.merge(b)  # neither has state: only the bookkeeping moves
    assert a._submitted == 30
    b._submitted = 2 ** 31 - 20
    with pytest.raises(N.WsaeError):
        a.merge(b)
    with pytest.raises(TypeError):
        collect_token_association(ReLUSAE(16, 32), [(torch.zeros(2, 4, 16), torch.zeros(2, 4, dtype=torch.int64))], 30)
