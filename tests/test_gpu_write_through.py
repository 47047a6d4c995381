"""The bf16 shadows ``update_rows_kernel`` leaves, read back exactly, through the C ABI alone.

The row stores of the optimizer tail carry a cache policy (write-through p / m / v).  A policy bit
changes no value and cannot be observed; what can go wrong with such a change is WHICH lane stores WHICH bytes, and for
the shadows nothing else in the suite sees that element by element (tests/test_gpu_optimizer_tail.py compares
pre-activations of a random batch to 1e-5).  The shadow stores themselves are still the plain 8-byte ones (the widened
16-byte form lost in the probe); this file pins them for whoever regroups them.  Here the shadows are read back exactly:

* ``bf16(W_e)``: the dense pre-activations of the D one-hot rows e_d.  With b_e = b_pre = 0 before and after the step
  (zero value, zero gradient and zero moments stay exactly zero under AdamW) the folded bias is 0 and
  pre[d, h] = 1 * bf16(W_e)[h, d] + zeros: exact in the fp32 accumulators.
* ``bf16(W_dT)``: ``wsae_intervene`` in REPLACE mode without a norm, code (1.0, h) in row h, b_d = b_pre = 0:
  out[h, :] = 1 * bf16(W_dT)[h, :].

Both must equal the bf16 rounding of the fp32 parameters the SAME launch wrote, and what ``wsae_prepare`` then makes of
that pack.  Equality is exact (as numbers: a -0.0 weight reads back as +0.0 through the accumulator).
D = 32: one partial lane group (8 of 64 lanes); 96; 384 (NI = 2, the second group half full); 1280: NI = 8, the route that
does the two rows one after the other.  H = 32 and 96: 8 and 24 blocks.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

import optim_oracle as OO
from oracle import synth
from test_gpu_optimizer_tail import HYPER, Guarded, adamw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines(device):
    from whisper_sae.sae.engine import SAEEngine
    cache = {}

    def get(D, H):
        if (D, H) not in cache:
            cache[(D, H)] = SAEEngine(device, D, H, 1)
        return cache[(D, H)]

    yield get
    torch.cuda.synchronize()
    for eng in cache.values():
        eng.close()


def read_shadows(eng, handle, params_ptr, device):
    """(bf16(W_e) [H, D], bf16(W_dT) [H, D]) as float32, as the ctx holds them right now."""
    from whisper_sae import _native as N
    D, H = eng.D, eng.H
    x = torch.eye(D, dtype=torch.float32, device=device)
    pre = torch.full((D, H), -7.0, dtype=torch.float32, device=device)
    N.check(eng.lib.wsae_encode_dense(handle, params_ptr, x.data_ptr(), N.DT_F32, 0, D, pre.data_ptr(), eng.stream()),
            "wsae_encode_dense")
    h = torch.zeros(H, D, dtype=torch.float32, device=device)
    out = torch.full((H, D), -7.0, dtype=torch.float32, device=device)
    vals = torch.ones(H, 1, dtype=torch.float32, device=device)
    idx = torch.arange(H, dtype=torch.int32, device=device).reshape(H, 1)
    N.check(eng.lib.wsae_intervene(handle, params_ptr, h.data_ptr(), N.DT_F32, H, vals.data_ptr(), idx.data_ptr(), 0, 0, 0.0,
                                   0, 0, 0, 0, 0, N.IV_REPLACE, out.data_ptr(), N.DT_F32, 0, eng.stream()), "wsae_intervene")
    return pre.cpu().numpy().T.copy(), out.cpu().numpy()


@pytest.mark.parametrize("H", [32, 96])
@pytest.mark.parametrize("D", [32, 96, 384, 1280])
def test_shadows_are_the_rounded_parameters_of_the_same_launch(engines, device, D, H):
    """Catches: a shadow store that lands in another lane's bytes, drops or repeats a group of a row (a widened or
    regrouped store), takes the row before the update or before the renorm, or the other matrix's row; a store past the
    row (the sentinels and the neighbouring row)."""
    from whisper_sae import _native as N
    eng = engines(D, H)
    handle = eng.ctx(N.PREC_BF16, max(D, H))
    lay = OO.layout(D, H)
    total, off = lay
    pack = synth.normal((total,), 500 + D + H, 1) * np.float32(0.1)
    grads = synth.normal((total,), 500 + D + H, 2)
    m = synth.normal((total,), 500 + D + H, 3) * np.float32(0.5)
    v = synth.uniform((total,), 500 + D + H, 4, 0.25, 1.5)
    for a in (pack, grads, m, v):
        a[off[2]:] = 0  # b_e, b_d, b_pre: zero and staying zero
    bufs = [Guarded(device, a, i) for i, a in enumerate((pack, grads, m, v))]
    adamw(eng, handle, bufs, dict(HYPER, weight_decay=0.01), 2, 1.0, 1.0, 1)
    fused_e, fused_d = read_shadows(eng, handle, bufs[0].ptr, device)
    new = bufs[0].payload()
    assert not new[off[2]:].any()
    we, wd = new[off[0]:off[1]].reshape(H, D), new[off[1]:off[2]].reshape(H, D)
    # the step moved the rows far enough that a shadow taken BEFORE the update would be seen: its bf16 image differs
    assert (OO.bf16(we) != OO.bf16(pack[off[0]:off[1]].reshape(H, D))).mean() > 0.01
    assert np.abs(np.linalg.norm(wd.astype(np.float64), axis=1) - 1.0).max() < 1e-5  # ... and renormalised W_dT
    assert np.array_equal(fused_e, OO.bf16(we))
    assert np.array_equal(fused_d, OO.bf16(wd))
    N.check(eng.lib.wsae_prepare(handle, bufs[0].ptr, eng.stream()), "wsae_prepare")
    fresh_e, fresh_d = read_shadows(eng, handle, bufs[0].ptr, device)
    assert np.array_equal(fresh_e, fused_e) and np.array_equal(fresh_d, fused_d)
    for b in bufs:
        assert b.sentinels_intact()
    assert np.array_equal(bufs[0].payload().view(np.int32), new.view(np.int32))  # reading the shadows wrote no parameter
