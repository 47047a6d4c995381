"""The row-list cases (tests/ring_rows_cases.py) on the CPU: the builder's properties, the TopK margin of every
oracle-tier fixture, and what the oracle-tier comparison can see.

* Builder: every property ``make_case`` promises, for every (B, D) of the case table.
* Fixture margin: the oracle's own selection on ``buffer[rows]`` reconciles with itself at ``clear > 0.98`` for every case
  held to the oracle, so a GPU failure of that requirement is the device's, not the fixture's.
* Teeth: oracle results computed with ONE stage reading the wrong rows (the batch position instead of the list entry, or
  the list shifted by one), at g4's shape in fp32 mode, each fail the comparison on the product that stage writes; the
  unfaulted result passes.  The faults are built from the buffer without its NaN rows: the comparison has to see wrong
  finite numbers, which is what a real mix-up between two referenced rows gives.
"""

from __future__ import annotations

import numpy as np
import pytest

import ring_rows_cases as R
from oracle import sae_oracle as O

F32, F64 = np.float32, np.float64
SHAPES = sorted({(s.B, s.D, s.seed) for s in R.ALL_SPECS + [R.B1]})


@pytest.mark.parametrize("B,D,seed", SHAPES, ids=[f"B{b}-D{d}" for b, d, _ in SHAPES])
def test_builder_properties(B, D, seed):
    c = R.make_case(B, D, seed)
    N = B + B // 2 + 37
    rows = c.rows.astype(np.int64)
    assert c.buffer.shape == c.clean.shape == (N, D) and c.buffer.dtype == np.float32
    assert c.rows.dtype == np.int32 and c.rows.shape == (B,)
    assert c.padded.dtype == np.int32 and c.padded.shape == (R.FRONT + B + R.BACK,) and (R.FRONT * 4) % 256 == 0
    assert np.shares_memory(c.rows, c.padded) and np.array_equal(c.padded[R.FRONT:R.FRONT + B], c.rows)
    # bf16-representable: a bf16 and an fp32 copy hold the same values
    assert np.array_equal(R.synth.bf16_round(c.clean), c.clean)
    # every index anywhere in the array is inside the buffer
    assert c.padded.min() >= 0 and c.padded.max() < N
    assert (rows != np.arange(B)).all()
    d = np.diff(rows)
    assert (d > 0).any() and (d < 0).any()
    assert rows[0] == N - 1 and rows[B - 1] == 0
    # repeats of an earlier entry
    first = {}
    repeats = []
    for b, r in enumerate(rows):
        if r in first:
            repeats.append((b, first[r]))
        else:
            first[r] = b
    assert abs(len(repeats) - B // 16) <= 2 and len(repeats) >= 2, len(repeats)
    earlier = lambda p: [q for q in range(p) if rows[q] == rows[p]]  # noqa: E731
    assert any(any(q // 4 == p // 4 for q in earlier(p)) for p, _ in repeats), "no repeat inside a 4-row group"
    assert any(any(q // 64 != p // 64 for q in earlier(p)) for p, _ in repeats), "no repeat from another 64-row chunk"
    # poison: exactly the rows the list never names, at least B // 2 - B // 16 of them; the list's surroundings name them
    used = np.zeros(N, bool)
    used[rows] = True
    assert np.array_equal(np.nonzero(~used)[0], c.unused) and len(c.unused) >= B // 2 - B // 16
    assert np.isnan(c.buffer[~used]).all() and np.isfinite(c.buffer[used]).all()
    assert np.array_equal(c.buffer[used], c.clean[used])
    outside = np.concatenate([c.padded[:R.FRONT], c.padded[R.FRONT + B:]])
    assert (~used[outside]).all() and np.isnan(c.buffer[outside]).all()
    assert np.isfinite(c.buffer[rows]).all()
    # deterministic
    again = R.make_case(B, D, seed)
    assert np.array_equal(again.padded, c.padded) and np.array_equal(again.buffer, c.buffer, equal_nan=True)


def test_case_table():
    assert [s.cid for s in R.SPECS] == [f"g{i}" for i in range(1, 11)] + [f"s{i}" for i in range(1, 7)]
    for s in R.SPECS:
        assert s.oracle == (s.B <= 2100), s.cid
        assert s.dense_wgrad == (s.cid == "g10")
    for s in R.PREFETCH_SPECS:  # every wave of the MFMA decode gets a second row
        assert s.mode == "bf16" and s.B > 4 * 1024 and not s.oracle


ORACLE_SPECS = [s for s in R.SPECS if s.oracle]


@pytest.mark.parametrize("spec", ORACLE_SPECS, ids=[s.cid for s in ORACLE_SPECS])
def test_fixture_keeps_the_topk_margin(spec):
    c = R.make_case(spec.B, spec.D, spec.seed)
    st = R.oracle_state(spec)
    x = c.buffer[c.rows]
    mode = R.MODE[spec.mode]
    _, idx = O.topk_select(O.pre_activation(st, x, mode), spec.K)
    sel, clear = O.reconcile_selection(st, x, idx, spec.K, mode)
    print(spec.cid, "clear", clear)
    assert clear > 0.98, clear
    assert np.array_equal(np.sort(sel, axis=1), np.sort(idx, axis=1))


# ------------------------------------------------------------------------------------------------------------------------
# what the comparison can see: g4's shape, fp32 mode
# ------------------------------------------------------------------------------------------------------------------------
G4 = R.SPEC["g4"]._replace(mode="fp32")


def device_like(st, x, fault, case):
    """The products of one fp32 step as a device would hand them over, from the oracle; ``fault`` names the one stage that
    reads ``buffer[b]`` in place of ``buffer[rows[b]]`` (or the list rolled by one)."""
    B = x.shape[0]
    wrong = case.clean[:B]
    if fault == "list_shifted_by_one":
        x = case.clean[np.roll(case.rows, 1)]
    st = st.copy()
    code = O.forward(st.copy(), wrong if fault == "encoder_ignores_rows" else x, "fp32", training=False)
    fwd = O.forward(st, x, "fp32", training=True, select=code["idx"])
    vals, loss = code["vals"], fwd["loss"]
    xr = wrong if fault == "decode_ignores_rows" else x  # what the residual is taken against
    if fault == "decode_ignores_rows":
        resid = fwd["reconstructed"].astype(F64) - xr.astype(F64)
        loss = F32(np.mean(resid * resid))
    g = O.backward(st, xr, fwd, "fp32")
    xe = wrong if fault == "wgrad_ignores_rows" else x  # what dW_e is contracted with
    grads = {n: g[n] for n in R.GRADS}
    grads["W_e"] = (g["dpre"].astype(F64).T @ (xe - st.b_pre).astype(F64)).astype(F32)
    return {"idx": code["idx"], "vals": vals, "grads": grads, "loss": float(loss), "l0": float(fwd["l0"]),
            "grad_norm": O.grad_total_norm(grads), "dead_feature_ratio": O.dead_ratio(st),
            "last_activated": st.last_activated.copy(), "step_count": st.step_count}


@pytest.fixture(scope="module")
def g4():
    c = R.make_case(G4.B, G4.D, G4.seed)
    return c, R.oracle_state(G4), c.buffer[c.rows]


def test_the_unfaulted_result_passes(g4):
    c, st, x = g4
    gaps = R.compare_with_oracle(device_like(st, x, None, c), st.copy(), x, G4.K, "fp32")
    print(gaps)
    assert gaps["clear"] > 0.98


FAULTS = [("encoder_ignores_rows", "selection"), ("decode_ignores_rows", "loss"), ("wgrad_ignores_rows", "W_e"),
          ("list_shifted_by_one", "selection")]


@pytest.mark.parametrize("fault,caught_by", FAULTS, ids=[f[0] for f in FAULTS])
def test_each_fault_fails_on_its_own_assertion(g4, fault, caught_by):
    c, st, x = g4
    with pytest.raises(R.Mismatch) as e:
        R.compare_with_oracle(device_like(st, x, fault, c), st.copy(), x, G4.K, "fp32")
    print(fault, "->", e.value)
    assert e.value.what == caught_by, (fault, str(e.value))
