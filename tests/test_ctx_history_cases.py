"""CPU checks of tests/ctx_history_cases.py: every row of the tables is what it claims to be, for a 256-CU and a 304-CU
device.  (The GPU file asserts the handles and the launch counts; this file holds the arithmetic the tables rest on.)"""

from __future__ import annotations

import numpy as np
import pytest

import ctx_history_cases as T

CUS = [256, 304]


def ceil_div(a: int, b: int) -> int:
    return -(-a // b)


@pytest.mark.parametrize("cus", CUS)
def test_kept_and_replaced(cus):
    """"kept": every batch that goes through the ctx after ``big`` fits the cap ``max(big, 64)``; "replaced": the last one
    does not (``SAEEngine.ctx`` destroys and recreates)."""
    cases = T.history_cases(cus) + T.intruder_cases(cus)
    assert {c.ctx for c in cases} == {"kept", "replaced"}
    for c in cases:
        v = T.victim(cus, c.vid)
        cap = max(c.batches[0], 64)
        assert c.batches[0] == v.big and v.B <= cap, c.cid
        assert all(1 <= b for b in c.batches), c.cid
        if c.ctx == "kept":
            assert all(b <= cap for b in c.batches[1:]), c.cid
        else:
            assert c.batches[-1] > cap and all(b <= cap for b in c.batches[1:-1]), c.cid
    for fam in set(T.B_VICTIMS.values()):  # one intruder larger than the cap per family
        assert "over_cap" in T.INTRUDERS[fam]


@pytest.mark.parametrize("cus", CUS)
def test_ragged_and_chunked_victims(cus):
    for v in T.victims(cus):
        for tile in v.ragged:
            assert v.B % tile != 0, (v.vid, tile)
        nchunks = ceil_div(v.B, 64)
        if v.chunked:
            assert cus <= nchunks <= T.WSAE_MAX_PARTIALS, v.vid  # (row r19 of test_gpu_kernel_variants.py: the limit)
            assert cus <= ceil_div(v.big, 64) <= T.WSAE_MAX_PARTIALS, v.vid
            assert (v.family, v.prec, v.x_dtype, v.dims) == ("topk", "bf16", "bf16", (384, 3072, 32)), v.vid
        elif v.family in ("topk", "batchtopk", "transcoder") and v.prec == "bf16":
            assert nchunks < cus, v.vid  # the one-round decode
    v3, v4 = T.victim(cus, "V3"), T.victim(cus, "V4")
    assert v3.B % 64 == 0 and v4.B % 64 == 40 and v3.big > v3.B and v4.big > v4.B
    v2 = T.victim(cus, "V2")
    assert v2.B >= 2048 and v2.dims[1] % 256 == 0 and v2.big >= 2048  # persistent_ok (wsae_encode.hip)
    assert T.victim(cus, "V1").B < 2048 and T.victim(cus, "V5").B < 2048


@pytest.mark.parametrize("cus", CUS)
def test_anchor_set_is_small(cus):
    for v in T.victims(cus):
        assert v.chunked or v.B <= T.ANCHOR_MAX_B, v.vid
        assert v.big > v.B, v.vid
    assert [v.vid for v in T.victims(cus) if v.chunked] == ["V3", "V4"]


@pytest.mark.parametrize("cus", CUS)
def test_ids_are_unique_and_independent_of_the_device(cus):
    ids = ([c.cid for c in T.history_cases(cus)] + [c.cid for c in T.intruder_cases(cus)] + [e[0] for e in T.EPOCHS] +
           [c[0] for c in T.CONTROLS])
    assert len(ids) == len(set(ids))
    assert len({v.vid for v in T.victims(cus)}) == len(T.victims(cus))
    assert [c.cid for c in T.history_cases(cus)] == [c.cid for c in T.history_cases(256)]
    assert [c.cid for c in T.intruder_cases(cus)] == [c.cid for c in T.intruder_cases(256)]


@pytest.mark.parametrize("cus", CUS)
def test_every_flag_is_named(cus):
    text = " ".join(T.all_there_for(cus))
    import re
    words = set(re.findall(r"[A-Za-z_0-9]+", text))
    assert [f for f in T.FLAGS if f not in words] == []


@pytest.mark.parametrize("cus", CUS)
def test_coverage_of_the_tables(cus):
    hist = T.history_cases(cus)
    by_v = {}
    for c in hist:
        by_v.setdefault(c.vid, []).append(c.kind)
    assert set(by_v) == {v.vid for v in T.victims(cus)}
    for vid, kinds in by_v.items():
        assert kinds[:2] == ["big", "same"], vid
    for vid in ("V2", "V3", "V4", "V5"):
        assert by_v[vid] == ["big", "same", "dtype", "pending", "causal", "params"]
    assert by_v["V7"] == ["big", "same", "dtype", "pending", "causal", "params"]
    for vid in ("V11x", "V11g"):
        assert by_v[vid] == ["big", "same", "dtype", "pending", "params"]  # (the causal tools take TopK codes only)
    assert 40 <= len(hist) <= 60
    intr = {c.vid for c in T.intruder_cases(cus)}
    assert intr == {"V2", "V3", "V5", "V6", "V7", "V8", "V9s", "V10", "V11x", "V11g", "V12"}
    for vid in intr:
        kinds = [c.kind for c in T.intruder_cases(cus) if c.vid == vid]
        assert {"nograd_same", "second_ab", "second_ba", "over_cap"} <= set(kinds), vid
    # the other flow runs first on the ReLU victims (x_flow needs whole 128-row groups: 520 and 200 are general, 512 and 256 not)
    vx, vg = T.victim(cus, "V11x"), T.victim(cus, "V11g")
    assert (vx.B % 128, vx.big % 128, vg.B % 128, vg.big % 128) == (0, 8, 72, 0)


@pytest.mark.parametrize("cus", CUS)
def test_launch_counts_follow_the_rules(cus):
    """The counts in the tables against the rules in the module docstring, recomputed here independently."""
    for c in T.history_cases(cus):
        v = T.victim(cus, c.vid)
        if c.counts is None:
            assert v.family not in T.DIRECT or c.kind in ("causal", "params"), c.cid
            continue
        fwd = {"big": 1, "same": 2, "dtype": 2, "pending": 2}[c.kind]
        bwd = 2 if c.kind == "dtype" else 1
        assert c.counts["encode_gemm"] == c.counts["decode"] == fwd and c.counts["wgrad"] == bwd, c.cid
        assert c.counts["bucket"] == (0 if v.chunked else bwd), c.cid
        dtypes = [v.x_dtype] * fwd
        if c.kind == "dtype":
            dtypes[0] = "fp32" if v.x_dtype == "bf16" else "bf16"
        staged = sum(1 for d in dtypes if not (v.prec == "bf16" and d == "bf16"))
        assert c.counts["stage_batch"] == staged, c.cid
    # a direct-gather bf16 victim shows no stage_batch launch, an fp32-input history one
    byid = {c.cid: c for c in T.history_cases(cus)}
    assert byid["A-V2-same"].counts["stage_batch"] == 0 and byid["A-V2-dtype"].counts["stage_batch"] == 1
    assert byid["A-V3-pending"].counts["bucket"] == 0 and byid["A-V2-pending"].counts["bucket"] == 1
    for c in T.intruder_cases(cus):
        if c.counts is None:
            continue
        fwd_full = {"nograd_same": 2, "second_ab": 2, "second_ba": 2}.get(c.kind, 1)
        enc_only = 0 if c.kind in ("nograd_same", "second_ab", "second_ba") else 1
        restages = 2 if c.kind == "second_ab" else 1
        assert c.counts["encode_gemm"] == fwd_full + enc_only + restages, c.cid
        assert c.counts["decode"] == fwd_full + restages, c.cid


def test_g12_dimensions_match_the_golden_file(golden_dir):
    g = np.load(golden_dir / "g12_transcoders.npz")
    for tag, dims in T.G12_DIMS.items():
        assert tuple(int(x) for x in g[f"{tag}.dims"]) == dims
    for cus in CUS:
        assert T.victim(cus, "V9s").big == 4 * T.G12_DIMS["eq"][4] and T.victim(cus, "V9n").big == 4 * T.G12_DIMS["narrow"][4]


def test_epochs_have_a_ragged_batch_inside():
    for eid, _, _, _, sizes, _ in T.EPOCHS:
        assert len(sizes) == 4 and sizes[2] < sizes[0] == sizes[1] == sizes[3], eid
        assert sizes[2] % 64 != 0 and max(sizes) == sizes[0], eid
