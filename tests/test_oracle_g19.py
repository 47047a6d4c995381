"""The oracle against the reference golden G19 (cfg-2 dimensions at the benchmarked batch, B = 16384): the link that
lets the GPU tests of the bench path, which compare with the oracle, stand for a comparison with the reference."""

from __future__ import annotations

import numpy as np
import pytest

from oracle import sae_oracle as O
from oracle import synth


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.mark.parametrize("mode,tol", [("fp32", 2e-5), ("amp", 2e-2)])
def test_oracle_matches_g19(golden_dir, mode, tol):
    g = np.load(golden_dir / "g19_bench_batch.npz")
    D, H, K, B = (int(v) for v in g["dims"])
    assert g["rows"].shape == (B,) and np.all(np.diff(g["rows"]) > 0)
    x = synth.activations(int(g["stream_rows"][0]), D, seed=42, stream=19, bf16=True)[g["rows"]]
    st = O.SAEState.from_state_dict(synth.sae_weights(D, H, seed=42, bf16=True, b_pre_scale=0.1), k=K,
                                    dead_feature_threshold=1000)
    fwd = O.forward(st, x, mode)
    assert synth.topk_margin(fwd["pre"], K).min() > 5e-5  # the fixture's rows all have a clear k / k+1 margin
    sets = np.sort(fwd["idx"], axis=1)
    assert np.array_equal(synth.index_set_digest(sets), g["idx_digest"])
    member = np.zeros((B, H), dtype=bool)
    np.put_along_axis(member, sets, True, axis=1)
    other = sets.copy()  # the digest tells each set from the one with its first member replaced by a non-member
    other[:, 0] = np.argmin(member, axis=1)
    assert not (synth.index_set_digest(other) == g["idx_digest"]).any()
    assert np.array_equal(sets[g["recon_rows"]], g["idx_rows"].astype(np.int64))
    assert abs(float(fwd["loss"]) - float(g["loss"])) / float(g["loss"]) < 1e-5
    assert float(fwd["l0"]) == float(g["l0"])
    assert rel(fwd["reconstructed"][g["recon_rows"]], g["recon"]) < 1e-5
    resid = fwd["reconstructed"].astype(np.float64) - x.astype(np.float64)
    assert rel((resid * resid).sum(axis=1), g["row_sse"]) < 1e-5
    assert st.step_count == int(g["step_count"]) and np.array_equal(st.last_activated, g["last_activated"])
    gr = O.backward(st, x, fwd, mode)
    norms = [np.sqrt((gr[n].astype(np.float64) ** 2).sum()) for n in ("W_e", "b_e", "W_d", "b_d", "b_pre")]
    assert np.allclose(norms, g["norms"], rtol=tol)
    for n in ("b_e", "b_d", "b_pre"):
        assert rel(gr[n], g[n]) < tol, n
    assert rel(gr["W_e"].reshape(-1)[g["pos_e"]], g["W_e_samples"]) < tol * 5
    assert rel(gr["W_d"].reshape(-1)[g["pos_d"]], g["W_d_samples"]) < tol * 5
