"""Direct float64 parity of ``wsae_optim.hip``: the optimizer tail and the maintenance kernels, through the C ABI alone.

No trainer and no module: ``whisper_sae._native`` with an ``SAEEngine`` for the ctx, the step record and the stream, so a
failure names the kernel.  The reference is tests/optim_oracle.py (float64 numpy).  Every bound below is DERIVED by
counting roundings, not measured; the measured maxima go to ``parity_notes.jsonl`` next to them.

Error model.  u = 2^-24 is the relative error of one correctly rounded fp32 operation (multiply, add, fma, division,
``sqrtf``, the single rounding of a host double constant to fp32); ``v_sqrt_f32`` and ``v_rcp_f32`` are 1 ulp = 2u.  A sum
of non-negative terms in which every term passes through at most n roundings has relative error <= n u.  Bounds are first
order; ``SECOND`` (1.02) covers the products of errors (< 1e-5 of the bound) and ``FLOOR`` the results that leave the
normal fp32 range.

Norm pass (``sqnorm_kernel`` + the prologue of ``update_rows_kernel``).  A square (g s)^2 carries 2u from the scaling and
1u of its own; it then passes 3 adds inside its float4, T accumulations (T = trips per thread), 6 wave steps and 4 serial
adds of ``block_sum``; the partials pass Tp = ceil(nparts / 256) adds, 6 wave steps and 4 adds again:
e_sq = (26 + T + Tp) u and e_norm = e_sq / 2 + 2u (``sqrtf``, ``* part_scale``).  After ``wire_unpack_kernel`` a square is
exact inside its ``fmaf`` and passes 8 T8 of them: e_sq = (8 T8 + 20 + Tp) u.  stats.grad_norm is held to e_norm,
stats.clip_coef to e_norm + 2u (the add of 1e-6 and the division).

``adam1``.  gc = g gs with gs = coef * grad_scale: e_g = e_norm + 5u with the clip on (add, division, product, g gs and one
spare), 1u with it off (coef = 1 and gs = grad_scale are exact).  With A = max(|m|, |gc|) and V = max(v, gc^2):
  m' = m + (gc - m) c1        |dm| <= A (c1 (e_g + 6u) + u)       gc; the subtraction (|gc - m| <= 2A), c1's rounding, the
                                                                  product; the final add (|m'| <= A)
  v' = b2 v + c2 gc gc        |dv| <= V (c2 (2 e_g + 3u) + 2u b2 + u)
  s  = sqrt(v')               |ds| <= the move of sqrt over [v' - dv, v' + dv] + 2u s
  den = s ibc + eps           |dden| <= ibc ds + 2u s ibc + u eps + u den
  q  = m' rcp(den)            |dq| <= dm / den + |q| (dden / den + 2u) + u |q|
  U  = step_size q            |dU| <= step_size dq + 2u |U|
  p' = p decay - U            |dp| <= 2u |p| + dU + u (|p| + |U|)
The parameter bound is therefore 3u (|p| + |U|) plus the carried terms, which are themselves proportional to |U| except
where m' cancels (then dm, relative to A, is what the kernel can be off by).
Renorm: a squared entry of the row passes 1 + 3 + NI + 6 roundings, so the norm n carries (NI + 10) / 2 u + 2u
(``sqrtf``) plus ||dp||_2 / n from the entries' own errors; the division and the product add 3u:
|d(p / n)| <= dp / n + |p| / n (||dp||_2 / n + ((NI + 10) / 2 + 5) u).  ``refresh_kernel`` walks 8 groups: NI = 8 there.
Row errors: a residual is 1u, its square 2u, then ceil(D / 64) ``fmaf`` steps and 6 wave steps: (8 + ceil(D / 64)) u.

Measured on the MI355X (profiles/optimizer_tail_parity_notes.jsonl), worst case as a fraction of its bound: m 0.58, v 0.40,
parameters 0.40, grad_norm 0.05 (4.8e-8 against 1.0e-6), clip_coef 0.05, renorm alone 0.19, row errors 0.25, the first
step's moments 1 ulp against 2, the shadow pre-activations 5.7e-7 against 1e-5.  Two findings came out of this file: every
``exp_avg_sq`` was 218 ulp from torch's while the hyper-parameters were floats (``test_first_moments_carry_torch_constants``),
and the b_pre behind the fused folded bias was up to 1 ulp from the one written to the pack, because hipcc contracted the
two inlined copies of ``adam1`` differently (``test_fused_shadows_equal_the_refresh``; ``adam1`` now spells its fmas out).
The 128 KB row sort of 8193 .. 16384 resample rows launched on this runtime with and without the dynamic-LDS attribute.
"""

from __future__ import annotations

import math

import numpy as np
import pytest
import torch

import optim_oracle as OO
from oracle import synth

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SECOND = 1.02
FLOOR = 2.0 ** -124
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
PRE_BF16_REL = 1e-5  # the pre-activation bound of tests/test_gpu_kernel_variants.py (hidden against the "amp" oracle)
GUARD = 64  # floats of sentinel on either side of each of the four buffers
MAX_PARTIALS = 1024  # WSAE_MAX_PARTIALS

# (D, H): every NI = ceil(D / 256) in {1, 2, 3, 4, 8}, ragged (288, 544, 800, 1056) and full last groups, the minimum
# width; (256, 160): 40 blocks over 32 ticket groups; (1024, 1024): P > 2^21, the norm pass at its 1024-block cap
SHAPES = [(32, 32), (256, 160), (288, 64), (512, 64), (544, 64), (768, 96), (800, 64), (1024, 1024), (1056, 64),
          (1280, 64), (2048, 32)]
STEPS, WDS, NORMZ, MAXN, GSC = [1, 2, 1000, 100000], [0.0, 0.01], [1, 0], [0.0, 1.0, 1e9], [1.0, 0.5]


def template_ni(D):
    ni = -(-D // 256)
    return ni if ni <= 4 else 8


def _cases():
    out, seen = [], {}
    for D, H in SHAPES:
        ni = template_ni(D)
        g = [1, 2, 3, 4, 8].index(ni)
        for prec in ("bf16", "fp32"):
            j = seen.get(ni, 0)
            seen[ni] = j + 1
            t = j + g
            out.append(dict(D=D, H=H, prec=prec, step=STEPS[t % 4], wd=WDS[(t // 2) % 2], normalize=NORMZ[t % 2],
                            max_norm=MAXN[t % 3], grad_scale=GSC[(t // 2 + t) % 2]))
    return out


CASES = _cases()


def _check_coverage():
    """Every value of every argument at least once per NI and at least once in each precision (not the full product)."""
    for key, values in (("step", STEPS), ("wd", WDS), ("normalize", NORMZ), ("max_norm", MAXN), ("grad_scale", GSC)):
        for ni in (1, 2, 3, 4, 8):
            assert {c[key] for c in CASES if template_ni(c["D"]) == ni} == set(values), (key, ni)
        for prec in ("bf16", "fp32"):
            assert {c[key] for c in CASES if c["prec"] == prec} == set(values), (key, prec)


_check_coverage()


def case_id(c):
    return f"{c['D']}x{c['H']}-{c['prec']}-t{c['step']}-wd{c['wd']}-n{c['normalize']}-mx{c['max_norm']:g}-gs{c['grad_scale']}"


# ---- rig ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rigs(device):
    from whisper_sae.sae.engine import SAEEngine
    cache = {}

    def get(D, H, k=1):
        key = (D, H, k)
        if key not in cache:
            cache[key] = SAEEngine(device, D, H, k)
        return cache[key]

    yield get
    torch.cuda.synchronize()
    for eng in cache.values():
        for handle, _ in eng._ctx.values():
            eng.lib.wsae_ctx_set_fired(handle, 0)
        eng.close()


def prec_code(prec):
    from whisper_sae import _native as N
    return N.PREC_BF16 if prec == "bf16" else N.PREC_FP32


class Guarded:
    """A device buffer with GUARD sentinel floats on either side; ``ptr`` is the address of the payload."""

    def __init__(self, device, payload: np.ndarray, tag: int):
        n = payload.size
        host = np.empty(n + 2 * GUARD, np.float32)
        self.sentinel = (np.arange(2 * GUARD, dtype=np.float32) + np.float32(1000.25 * (tag + 1))) * np.float32(-1.0)
        host[:GUARD], host[GUARD + n:] = self.sentinel[:GUARD], self.sentinel[GUARD:]
        host[GUARD:GUARD + n] = payload
        self.n = n
        self.t = torch.from_numpy(host).to(device)
        self.ptr = self.t.data_ptr() + 4 * GUARD

    def payload(self) -> np.ndarray:
        return self.t[GUARD:GUARD + self.n].cpu().numpy()

    def sentinels_intact(self) -> bool:
        host = self.t.cpu().numpy()
        got = np.concatenate([host[:GUARD], host[GUARD + self.n:]])
        return bool(np.array_equal(got.view(np.int32), self.sentinel.view(np.int32)))


def read_stats(eng):
    s = eng.stats.cpu().numpy()
    f = s.view(np.float32)
    return dict(loss=float(f[0]), l0=float(f[1]), grad_norm=float(f[2]), clip_coef=float(f[3]), dead_ratio=f[4],
                dead_count=int(s[5]))


def adamw(eng, handle, bufs, hyper, step, max_norm, grad_scale, normalize, nfw=0, last=None, sc=None, thr=0, grads_ptr=None):
    from whisper_sae import _native as N
    p, g, m, v = bufs
    N.check(eng.lib.wsae_adamw_step(handle, p.ptr, grads_ptr if grads_ptr is not None else g.ptr, m.ptr, v.ptr,
                                    hyper["lr"], hyper["beta1"], hyper["beta2"], hyper["eps"], hyper["weight_decay"],
                                    int(step), float(max_norm), float(grad_scale), int(normalize), int(nfw),
                                    0 if last is None else last.data_ptr(), 0 if sc is None else sc.data_ptr(), int(thr),
                                    eng.stats.data_ptr(), eng.stream()), "wsae_adamw_step")


# ---- inputs ------------------------------------------------------------------------------------------------------------
ROW_E_ZERO, ROW_D_ZERO, ROW_D_NULL = 1, 2, 3  # planted rows (H >= 32)
TINY_AT, HUGE_AT = 5, 9  # columns of W_e row 0 that carry the 1e-30 and the 1e15 gradient


def make_inputs(D, H, seed, max_norm, grad_scale, zero_moments=False, huge=True):
    """Pack, gradients and moments with the planted elements.  The moments are drawn at the scale gs the clipped
    gradients will have (max_norm / 1e15 once the 1e15 gradient sets the norm), so that m, v and gc stay comparable."""
    lay = OO.layout(D, H)
    total, off = lay
    clip = max_norm > 0
    s = (max_norm * 1e-15) if (clip and huge) else grad_scale
    pack = synth.normal((total,), seed, 1) * np.float32(0.1)
    grads = synth.normal((total,), seed, 2)
    m = (synth.normal((total,), seed, 3).astype(np.float64) * 0.5 * s).astype(np.float32)
    v = (synth.uniform((total,), seed, 4, 0.25, 1.5).astype(np.float64) * s * s).astype(np.float32)
    if zero_moments:
        m[:], v[:] = 0, 0
    for o, row in ((off[0], ROW_E_ZERO), (off[1], ROW_D_ZERO), (off[1], ROW_D_NULL)):
        sl = slice(o + row * D, o + (row + 1) * D)
        grads[sl], m[sl], v[sl] = 0, 0, 0
    pack[off[1] + ROW_D_NULL * D: off[1] + (ROW_D_NULL + 1) * D] = 0
    grads[off[0] + TINY_AT] = np.float32(1e-30)
    if clip and huge:
        grads[off[0] + HUGE_AT] = np.float32(1e15)
    return lay, pack, grads, m, v


# ---- derived bounds ----------------------------------------------------------------------------------------------------
def norm_error(P, H, wire: bool) -> float:
    """e_norm of the module docstring for a pack of P elements."""
    if wire:
        n8 = (P + H) // 8
        nparts = min(MAX_PARTIALS, -(-n8 // 256))
        depth = 8 * -(-n8 // (nparts * 256)) + 20 + -(-nparts // 256)
    else:
        n4 = P // 4
        nparts = min(MAX_PARTIALS, -(-n4 // 512))
        depth = 26 + -(-n4 // (nparts * 256)) + -(-nparts // 256)
    return depth * U / 2 + 2 * U


def tail_bounds(ref, pack, m, v, lay, D, H, e_norm, clip_on, normalize, ni):
    """Element-wise absolute bounds (m, v, pack) of the module docstring, from the oracle's float64 intermediates."""
    total, off = lay
    c = ref["constants"]
    e_g = (e_norm + 5 * U) if clip_on else U
    gc = np.abs(ref["gc"])
    A = np.maximum(np.abs(np.asarray(m, np.float64)), gc)
    V = np.maximum(np.asarray(v, np.float64), gc * gc)
    dm = A * (c["omb1"] * (e_g + 6 * U) + U) * SECOND + FLOOR
    dv = V * (c["omb2"] * (2 * e_g + 3 * U) + 2 * U * c["beta2"] + U) * SECOND + FLOOR
    vn = ref["v"]
    s = np.sqrt(vn)
    ds = np.maximum(np.sqrt(vn + dv) - s, s - np.sqrt(np.maximum(vn - dv, 0.0))) + 2 * U * s
    ibc = 1.0 / c["bc2_sqrt"]
    den = ref["denom"]
    dden = ibc * ds + 2 * U * s * ibc + U * c["eps"] + U * den
    q = np.abs(ref["m"]) / den
    dq = dm / den + q * (dden / den + 2 * U) + U * q
    upd = np.abs(ref["update"])
    dU = c["step_size"] * dq + 2 * U * upd
    p_abs = np.abs(np.asarray(pack, np.float64))
    dp = (2 * U * p_abs + dU + U * (p_abs + upd)) * SECOND + FLOOR
    if normalize:
        pre = ref["pre_norm"][off[1]:off[2]].reshape(H, D)
        n = np.maximum(ref["row_norm"], 1e-12)[:, None]
        dpr = dp[off[1]:off[2]].reshape(H, D)
        carried = np.sqrt((dpr * dpr).sum(axis=1))[:, None] / n
        dn = dpr / n + np.abs(pre) / n * (carried + ((ni + 10) / 2 + 5) * U)
        dp = dp.copy()
        dp[off[1]:off[2]] = (dn * SECOND + FLOOR).reshape(-1)
    return dm, dv, dp


def assert_within(name, got, ref, bound, note, key, scale=None):
    err = np.abs(np.asarray(got, np.float64) - ref)
    ratio = float((err / bound).max())
    if scale is not None:
        ok = scale > 0
        note(f"{key}_{name}_rel", float((err[ok] / scale[ok]).max()), float((bound[ok] / scale[ok]).max()))
    note(f"{key}_{name}_over_bound", ratio, 1.0)
    assert np.isfinite(np.asarray(got)).all(), name
    worst = int(np.argmax(err / bound))
    assert ratio <= 1.0, (name, worst, float(got[worst]), float(ref[worst]), float(bound[worst]))


def check_tail(eng, bufs, ref, inputs, D, H, e_norm, clip_on, normalize, note, key):
    """Pack, both moments, the two stats words, the planted elements and the sentinels of one tail."""
    check_values(bufs[0].payload(), bufs[2].payload(), bufs[3].payload(), read_stats(eng), ref, inputs, D, H, e_norm,
                 clip_on, normalize, note, key)
    for b in bufs:
        assert b.sentinels_intact()
    assert np.array_equal(bufs[1].payload().view(np.int32), inputs[2].view(np.int32))  # the gradients are only read


def check_values(got_p, got_m, got_v, st, ref, inputs, D, H, e_norm, clip_on, normalize, note, key):
    lay, pack, grads, m, v = inputs
    total, off = lay
    ni = template_ni(D)
    dm, dv, dp = tail_bounds(ref, pack, m, v, lay, D, H, e_norm, clip_on, normalize, ni)
    print(f"{key}: grad_norm {st['grad_norm']!r} vs {ref['grad_norm']!r}, clip {st['clip_coef']!r} vs {ref['clip_coef']!r}")
    gn_rel = abs(st["grad_norm"] - ref["grad_norm"]) / ref["grad_norm"]
    note(f"{key}_grad_norm_rel", gn_rel, e_norm * SECOND)
    assert gn_rel <= e_norm * SECOND, (st["grad_norm"], ref["grad_norm"])
    cc_rel = abs(st["clip_coef"] - ref["clip_coef"]) / ref["clip_coef"]
    note(f"{key}_clip_coef_rel", cc_rel, (e_norm + 2 * U) * SECOND if clip_on else 0.0)
    assert cc_rel <= ((e_norm + 2 * U) * SECOND if clip_on else 0.0), (st["clip_coef"], ref["clip_coef"])
    gc = np.abs(ref["gc"])
    upd = np.abs(ref["update"])
    assert_within("m", got_m, ref["m"], dm, note, key, np.maximum(np.abs(m.astype(np.float64)), gc))
    assert_within("v", got_v, ref["v"], dv, note, key, np.maximum(v.astype(np.float64), gc * gc))
    assert_within("p", got_p, ref["pack"], dp, note, key, np.abs(pack.astype(np.float64)) + upd)
    # planted: zero gradient and zero moments leave exactly fl(p * decay), decay as the kernel holds it (one fp32 rounding)
    decay32 = float(np.float32(ref["constants"]["decay"]))
    sl = slice(off[0] + ROW_E_ZERO * D, off[0] + (ROW_E_ZERO + 1) * D)
    assert np.array_equal(got_p[sl], (pack[sl].astype(np.float64) * decay32).astype(np.float32))
    assert not got_m[sl].any() and not got_v[sl].any()
    sl = slice(off[1] + ROW_D_ZERO * D, off[1] + (ROW_D_ZERO + 1) * D)
    if not normalize:
        assert np.array_equal(got_p[sl], (pack[sl].astype(np.float64) * decay32).astype(np.float32))
    else:
        assert abs(float(np.linalg.norm(got_p[sl].astype(np.float64))) - 1.0) < (ni + 20) * U
    sl = slice(off[1] + ROW_D_NULL * D, off[1] + (ROW_D_NULL + 1) * D)
    assert np.array_equal(got_p[sl].view(np.int32) & 0x7FFFFFFF, np.zeros(D, np.int32))  # stays zero: no NaN from 0 / 1e-12


# ---- a. AdamW tail, b. written exactly once --------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_adamw_tail_matches_float64(rigs, device, parity_note, case):
    """Every element of the pack, exp_avg, exp_avg_sq, stats.grad_norm and stats.clip_coef against the oracle in
    ``as_passed`` mode, within the derived bounds of the module docstring; planted exact elements; sentinels.

    Catches: the wrong tail clamp (a ragged last group, D = 288 / 544 / 800 / 1056, would update a row's last float4 from
    the wrong address or twice: off by a whole update); a missing reload of the W_dT row at NI = 8 (W_dT would receive
    W_e's update); a double write of the shared biases (b_d / b_pre and their moments off by a whole update, the bound is
    ~1e-7 of it); a stale clip or a dropped grad_scale (every m and v); a NaN from the all-zero row's 0 / 1e-12."""
    D, H = case["D"], case["H"]
    eng = rigs(D, H)
    handle = eng.ctx(prec_code(case["prec"]), 64)
    inputs = make_inputs(D, H, 100 + D + H, case["max_norm"], case["grad_scale"])
    lay, pack, grads, m, v = inputs
    bufs = [Guarded(device, a, i) for i, a in enumerate((pack, grads, m, v))]
    hyper = dict(HYPER, weight_decay=case["wd"])
    adamw(eng, handle, bufs, hyper, case["step"], case["max_norm"], case["grad_scale"], case["normalize"])
    ref = OO.tail(pack, grads, m, v, lay, dict(hyper, mode="as_passed"), case["step"], case["max_norm"], case["grad_scale"],
                  bool(case["normalize"]))
    clip_on = case["max_norm"] > 0
    assert (ref["clip_coef"] < 1e-3) if clip_on else (ref["clip_coef"] == 1.0)  # ||g|| >> max_norm: 1e15 planted
    check_tail(eng, bufs, ref, inputs, D, H, norm_error(lay[0], H, False), clip_on, bool(case["normalize"]), parity_note,
               "tail_" + case_id(case))
    if clip_on:  # the two extreme gradients: finite results that match (they are inside the element-wise check as well)
        o = lay[1][0]
        got_v = bufs[3].payload()
        assert np.isfinite(got_v[o + HUGE_AT]) and got_v[o + HUGE_AT] > 0.5 * ref["v"][o + HUGE_AT] > 0


def test_nan_gradient_is_propagated(rigs, device):
    """One NaN gradient: stats.grad_norm is non-finite and that element's parameter is non-finite - propagated, not
    hidden (a kernel that tested ``nrm > max_norm`` and skipped the element, or zeroed it, would pass every finite
    case).  Nothing is asserted about the other elements."""
    D, H = 32, 32
    eng = rigs(D, H)
    handle = eng.ctx(prec_code("fp32"), 64)
    lay, pack, grads, m, v = make_inputs(D, H, 7, 1.0, 1.0, huge=False)
    at = lay[1][0] + 3
    grads[at] = np.float32("nan")
    bufs = [Guarded(device, a, i) for i, a in enumerate((pack, grads, m, v))]
    adamw(eng, handle, bufs, dict(HYPER, weight_decay=0.0), 3, 1.0, 1.0, 1)
    assert not math.isfinite(read_stats(eng)["grad_norm"])
    assert not np.isfinite(bufs[0].payload()[at])
    for b in bufs:
        assert b.sentinels_intact()


def ulp_distance(a, b):
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


@pytest.mark.parametrize("D,H", [(32, 32), (384, 64)])
def test_first_moments_carry_torch_constants(rigs, device, parity_note, D, H):
    """``torch`` mode, m = v = 0, one step, clip off: v = float32(float32(0.001) gc^2) and m = float32(0.1 gc) to within
    2 ulp - what ``torch.optim.AdamW`` leaves in exp_avg_sq / exp_avg (tests/test_optim_oracle.py pins torch's side).
    With float hyper-parameters and ``1.f - beta2`` in the kernel every v was 1.29e-5 (216 ulp) away.

    Catches: forming 1 - beta in fp32 from a float32 beta anywhere between the binding and the kernel."""
    eng = rigs(D, H)
    handle = eng.ctx(prec_code("fp32"), 64)
    lay, pack, grads, m, v = make_inputs(D, H, 11, 0.0, 1.0, zero_moments=True)
    bufs = [Guarded(device, a, i) for i, a in enumerate((pack, grads, m, v))]
    hyper = dict(HYPER, weight_decay=0.0)
    adamw(eng, handle, bufs, hyper, 1, 0.0, 1.0, 1)
    ref = OO.tail(pack, grads, m, v, lay, dict(hyper, mode="torch"), 1, 0.0, 1.0, True)
    v_ref = (float(np.float32(0.001)) * grads.astype(np.float64) ** 2).astype(np.float32)
    m_ref = (0.1 * grads.astype(np.float64)).astype(np.float32)
    assert np.array_equal(v_ref, ref["v"].astype(np.float32))
    got_m, got_v = bufs[2].payload(), bufs[3].payload()
    normal = v_ref > 1e-30  # (the 1e-30 gradient's square is below the fp32 range)
    dv, dm = int(ulp_distance(got_v, v_ref)[normal].max()), int(ulp_distance(got_m, m_ref)[normal].max())
    print(f"torch-mode first moments at {D}x{H}: v {dv} ulp, m {dm} ulp")
    parity_note(f"torch_mode_v_ulp_{D}x{H}", dv, 2)
    parity_note(f"torch_mode_m_ulp_{D}x{H}", dm, 2)
    assert dv <= 2 and dm <= 2
    assert not got_v[~normal].any() or np.all(got_v[~normal] < 1e-37)


# ---- c. fused shadows == stand-alone refresh ---------------------------------------------------------------------------
def encode_dense(eng, handle, params_ptr, x):
    from whisper_sae import _native as N
    pre = torch.empty(x.shape[0], eng.H, dtype=torch.float32, device=x.device)
    N.check(eng.lib.wsae_encode_dense(handle, params_ptr, x.data_ptr(), N.DT_F32, 0, x.shape[0], pre.data_ptr(),
                                      eng.stream()), "wsae_encode_dense")
    return pre


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("D,H", [(288, 64), (768, 96), (1056, 64), (1280, 64)])
def test_fused_shadows_equal_the_refresh(rigs, device, parity_note, D, H, normalize):
    """bf16 ctx: the dense pre-activations of a fixed 64-row batch right after ``wsae_adamw_step`` (its fused bf16 W_e and
    folded bias) are bit-identical with those after a forced ``wsae_prepare`` on the same pack, and both match the
    oracle's bf16(W_e) . x + (b_e - bf16(W_e) . b_pre) from the NEW pack; the same after ``wsae_normalize_decoder``.

    Catches: a stale b_pre in the folded bias (the step moves b_pre by lr = 1e-3: the pre-activations would be ~1e-3 of
    their maximum off, bound 1e-5); a shadow taken before the update or from the other row; the wrong tail clamp in the shadow stores."""
    from whisper_sae import _native as N
    eng = rigs(D, H)
    handle = eng.ctx(N.PREC_BF16, 64)
    lay, pack, grads, m, v = make_inputs(D, H, 300 + D, 0.0, 1.0, zero_moments=True)  # first step: every entry moves by lr
    bufs = [Guarded(device, a, i) for i, a in enumerate((pack, grads, m, v))]
    x_np = synth.activations(64, D, seed=17, stream=5, bf16=True)
    x = torch.from_numpy(x_np).to(device)
    adamw(eng, handle, bufs, dict(HYPER, weight_decay=0.01), 1, 0.0, 1.0, normalize)
    fused = encode_dense(eng, handle, bufs[0].ptr, x)
    N.check(eng.lib.wsae_prepare(handle, bufs[0].ptr, eng.stream()), "wsae_prepare")
    fresh = encode_dense(eng, handle, bufs[0].ptr, x)
    assert torch.equal(fused.view(torch.int32), fresh.view(torch.int32))
    new_pack = bufs[0].payload()
    off = lay[1]
    assert np.median(np.abs(new_pack[off[4]:off[4] + D] - pack[off[4]:off[4] + D])) > 5e-4  # b_pre really moved (by lr)
    ref = OO.shadow_pre(new_pack, lay, x_np)
    gap = float(np.abs(fused.cpu().numpy() - ref).max() / np.abs(ref).max())
    stale = OO.shadow_pre(np.concatenate([new_pack[:off[4]], pack[off[4]:]]), lay, x_np)
    assert np.abs(stale - ref).max() / np.abs(ref).max() > 10 * PRE_BF16_REL  # the slip this test is for is visible
    parity_note(f"shadow_pre_rel_{D}x{H}_n{normalize}", gap, PRE_BF16_REL)
    assert gap < PRE_BF16_REL
    # wsae_normalize_decoder alone (refresh_kernel<true, true>) on a fresh pack
    again = Guarded(device, pack, 9)
    N.check(eng.lib.wsae_normalize_decoder(handle, again.ptr, eng.stream()), "wsae_normalize_decoder")
    fused = encode_dense(eng, handle, again.ptr, x)
    N.check(eng.lib.wsae_prepare(handle, again.ptr, eng.stream()), "wsae_prepare")
    fresh = encode_dense(eng, handle, again.ptr, x)
    assert torch.equal(fused.view(torch.int32), fresh.view(torch.int32))
    got = again.payload()
    ref = OO.shadow_pre(got, lay, x_np)
    assert float(np.abs(fused.cpu().numpy() - ref).max() / np.abs(ref).max()) < PRE_BF16_REL
    wd = pack[off[1]:off[2]].reshape(H, D).astype(np.float64)
    n = np.maximum(np.sqrt((wd * wd).sum(axis=1)), 1e-12)[:, None]
    bound = np.abs(wd / n) * ((8 + 10) / 2 + 5) * U * SECOND + FLOOR
    err = np.abs(got[off[1]:off[2]].reshape(H, D) - wd / n)
    parity_note(f"normalize_decoder_over_bound_{D}x{H}", float((err / bound).max()), 1.0)
    assert (err <= bound).all()
    assert np.array_equal(np.delete(got, np.s_[off[1]:off[2]]).view(np.int32), np.delete(pack, np.s_[off[1]:off[2]]).view(np.int32))
    assert again.sentinels_intact()


# ---- d. dead count and clock merge -------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_fired", [False, True])
@pytest.mark.parametrize("H", [32, 160, 1056, 4128])
def test_dead_count_and_clock_merge(rigs, device, H, with_fired):
    """stats.dead_count / dead_ratio and the merged ``last`` of ``wsae_adamw_step`` (exact), twice in a row, then
    ``wsae_dead_scan`` on the same clocks.  ``last`` holds values on both sides of the threshold, exactly at it (alive)
    and negative ones; H / 4 = 8, 40, 264 and 1032 blocks: equal, unequal and many-per-group ticket layouts.

    Catches: ``>=`` for ``>`` in the dead test (the entries at the threshold); a wrong last-arriver decision (the count
    would be a partial sum or never written; the second launch shows the ticket words were left zeroed); a count that
    ignores the merge; ``fired`` not cleared."""
    from whisper_sae import _native as N
    D, SC, THR = 32, 1000, 50
    eng = rigs(D, H)
    handle = eng.ctx(prec_code("bf16" if H in (160, 4128) else "fp32"), 64)
    lay, pack, grads, m, v = make_inputs(D, H, 40 + H, 0.0, 1.0)
    bufs = [Guarded(device, a, i) for i, a in enumerate((pack, grads, m, v))]
    w = synth.counter_u64(H, 5, H)
    last_np = (SC - THR + (w % np.uint64(7)).astype(np.int64) - 3).astype(np.int64)  # 947 .. 953: three dead values, 950 alive
    last_np[(w >> np.uint64(8)) % np.uint64(11) == 0] = -5
    last_np[(w >> np.uint64(16)) % np.uint64(13) == 0] = SC
    last_np[:3] = [SC - THR, SC - THR - 1, -1]
    fired_np = ((w >> np.uint64(24)) % np.uint64(3)).astype(np.float32)  # 0, 1 or 2 ranks saw the feature fire
    assert ((SC - last_np > THR) & (fired_np > 0)).any() and (SC - last_np == THR).sum() >= 2
    last = torch.from_numpy(last_np.copy()).to(device)
    sc = torch.tensor([SC], dtype=torch.int64, device=device)
    fired = torch.from_numpy(fired_np.copy()).to(device)
    ref = OO.tail(pack, grads, m, v, lay, dict(HYPER, weight_decay=0.0, mode="as_passed"), 1, 0.0, 1.0, True, last=last_np,
                  step_count=SC, thr=THR, fired=fired_np if with_fired else None)
    assert 0 < ref["dead_count"] < H
    hyper = dict(HYPER, weight_decay=0.0)
    try:
        N.check(eng.lib.wsae_ctx_set_fired(handle, fired.data_ptr() if with_fired else 0), "wsae_ctx_set_fired")
        for step in (1, 2):  # the second launch: fired is all zero by now, the merged clocks give the same count
            eng.stats.zero_()
            adamw(eng, handle, bufs, hyper, step, 0.0, 1.0, 1, last=last, sc=sc, thr=THR)
            st = read_stats(eng)
            assert st["dead_count"] == ref["dead_count"], (step, st["dead_count"], ref["dead_count"])
            assert st["dead_ratio"] == np.float32(ref["dead_count"]) / np.float32(H)
            assert np.array_equal(last.cpu().numpy(), ref["last"])
            if with_fired:
                assert not fired.cpu().numpy().any()
            else:
                assert np.array_equal(fired.cpu().numpy(), fired_np)
    finally:
        eng.lib.wsae_ctx_set_fired(handle, 0)
    for b in bufs:
        assert b.sentinels_intact()
    # wsae_dead_scan on the merged clocks: with / without the mask and the record
    mask_ref, cnt_ref = OO.dead_scan(ref["last"], SC, THR)
    assert cnt_ref == ref["dead_count"]
    for want_mask in (True, False):
        for want_stats in (True, False):
            mask = torch.full((H,), 7, dtype=torch.uint8, device=device)
            eng.stats.fill_(-7)
            N.check(eng.lib.wsae_dead_scan(handle, last.data_ptr(), sc.data_ptr(), THR, mask.data_ptr() if want_mask else 0,
                                           eng.stats.data_ptr() if want_stats else 0, eng.stream()), "wsae_dead_scan")
            st = read_stats(eng)
            assert np.array_equal(mask.cpu().numpy(), mask_ref if want_mask else np.full(H, 7, np.uint8))
            if want_stats:
                assert st["dead_count"] == cnt_ref and st["dead_ratio"] == np.float32(cnt_ref) / np.float32(H)
            else:
                assert st["dead_count"] == -7


# ---- e. wire unpack ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wire_dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("D,H", [(32, 32), (288, 64)])
def test_wire_unpack_and_the_norm_it_leaves(rigs, device, parity_note, D, H, wire_dtype):
    """``wsae_grads_unpack_wire``: grads_ext is the wire [W_dT | W_e | b_e | b_d | b_pre | fired] permuted into
    [W_e | W_dT | b_e | b_d | b_pre | fired], bit for bit; explicit ``metrics_sum`` gives the rank means; the following
    ``wsae_adamw_step(norm_from_wgrad = 1, grad_scale = 1/2)`` takes its norm from the partials the unpack left and stays
    within the derived bounds of the tail.

    Catches: the two matrices not swapped (or the tail shifted); the fired indicators counted into the norm; grad_scale
    applied twice or not at all to the left-over partials."""
    from whisper_sae import _native as N
    eng = rigs(D, H)
    handle = eng.ctx(prec_code("fp32"), 64)
    lay, pack, grads, m, v = make_inputs(D, H, 70 + D, 1.0, 0.5, huge=False)
    total, off = lay
    hd = D * H
    wire_np = np.zeros(total + H + N.WIRE_METRIC_SLOTS, np.float32)
    body = synth.normal((total,), 23, 1)
    if wire_dtype == "bf16":
        body = synth.bf16_round(body)
    for o, row in ((off[0], ROW_E_ZERO), (off[1], ROW_D_ZERO), (off[1], ROW_D_NULL)):  # keep the planted zero-gradient rows
        body[o + row * D: o + (row + 1) * D] = 0
    body[off[0] + TINY_AT] = np.float32(1e-30) if wire_dtype == "fp32" else synth.bf16_round(np.float32([1e-30]))[0]
    fired_np = (synth.counter_u64(H, 3, D) % np.uint64(3)).astype(np.float32)
    wire_np[:hd], wire_np[hd:2 * hd], wire_np[2 * hd:total] = body[off[1]:off[2]], body[off[0]:off[1]], body[off[2]:]
    wire_np[total:total + H] = fired_np
    wire = torch.from_numpy(wire_np).to(device)
    if wire_dtype == "bf16":
        wire = wire.to(torch.bfloat16)
        assert np.array_equal(wire.float().cpu().numpy(), wire_np)
    ext = Guarded(device, np.full(total + H, 123.0, np.float32), 5)
    metrics = torch.tensor([3.5, 41.0], dtype=torch.float32, device=device)
    eng.stats.zero_()
    N.check(eng.lib.wsae_grads_unpack_wire(handle, wire.data_ptr(), N.DT_BF16 if wire_dtype == "bf16" else N.DT_F32, ext.ptr,
                                           metrics.data_ptr(), 2, eng.stats.data_ptr(), eng.stream()), "wsae_grads_unpack_wire")
    expect = np.concatenate([body, fired_np])
    assert np.array_equal(ext.payload().view(np.int32), expect.view(np.int32))
    assert ext.sentinels_intact()
    st = read_stats(eng)
    assert st["loss"] == 1.75 and st["l0"] == 20.5
    bufs = [Guarded(device, a, i) for i, a in enumerate((pack, body, m, v))]
    hyper = dict(HYPER, weight_decay=0.01)
    adamw(eng, handle, bufs, hyper, 2, 1.0, 0.5, 1, nfw=1, grads_ptr=ext.ptr)
    ref = OO.tail(pack, body, m, v, lay, dict(hyper, mode="as_passed"), 2, 1.0, 0.5, True)
    assert ref["clip_coef"] < 0.2
    check_tail(eng, bufs, ref, (lay, pack, body, m, v), D, H, norm_error(total, H, True), True, True, parity_note,
               f"wire_{wire_dtype}_{D}x{H}")
    assert np.array_equal(ext.payload().view(np.int32), expect.view(np.int32))  # no fired vector set on the ctx: left alone


# ---- f. row errors -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x_dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("B", [1, 5, 64])
@pytest.mark.parametrize("D", [32, 1280])
def test_row_errors(rigs, device, parity_note, D, B, x_dtype):
    """``wsae_row_errors`` with and without ``rows`` and ``resid`` against float64: the sums within (8 + ceil(D / 64)) u
    (module docstring), the residuals within 1u (one subtraction).

    Catches: a gather that ignores ``rows`` or applies it to ``recon``; a last block that skips rows when B % 4 != 0; a
    lane stride that drops or repeats columns (D = 32 leaves half the wave idle)."""
    from whisper_sae import _native as N
    eng = rigs(D, 64)
    handle = eng.ctx(prec_code("fp32"), 64)
    src_np = synth.activations(2 * B + 3, D, seed=31, stream=B, bf16=(x_dtype == "bf16"))
    recon_np = (src_np[:B] * np.float32(0.75) + synth.normal((B, D), 32, B) * np.float32(0.1)).astype(np.float32)
    rows_np = ((np.arange(B) * 2 + 3) % (2 * B + 3)).astype(np.int32)
    src = torch.from_numpy(src_np).to(device)
    if x_dtype == "bf16":
        src = src.to(torch.bfloat16)
    recon = torch.from_numpy(recon_np).to(device)
    rows = torch.from_numpy(rows_np).to(device)
    bound_rel = (8 + -(-D // 64)) * U * SECOND
    worst = 0.0
    for use_rows in (False, True):
        for use_resid in (False, True):
            err = torch.full((B + 2,), -1.0, dtype=torch.float32, device=device)
            resid = torch.full((B + 1, D), -2.0, dtype=torch.float32, device=device)
            N.check(eng.lib.wsae_row_errors(handle, src.data_ptr(), N.DT_BF16 if x_dtype == "bf16" else N.DT_F32,
                                            rows.data_ptr() if use_rows else 0, recon.data_ptr(), B, err.data_ptr(),
                                            resid.data_ptr() if use_resid else 0, eng.stream()), "wsae_row_errors")
            e_ref, r_ref = OO.row_errors(src_np, recon_np, rows_np if use_rows else np.arange(B))
            got = err.cpu().numpy()
            assert (got[B:] == -1.0).all()
            worst = max(worst, float((np.abs(got[:B] - e_ref) / e_ref).max()))
            assert (np.abs(got[:B] - e_ref) <= bound_rel * e_ref).all()
            got_r = resid.cpu().numpy()
            assert (got_r[B:] == -2.0).all()
            if use_resid:
                assert (np.abs(got_r[:B] - r_ref) <= U * np.abs(r_ref) + FLOOR).all()
            else:
                assert (got_r == -2.0).all()
    parity_note(f"row_err_rel_{D}_{B}_{x_dtype}", worst, bound_rel)


# ---- g. resample chain, direct -----------------------------------------------------------------------------------------
RESAMPLE_REL = 1e-6  # the bound of tests/test_gpu_parity.py::TestDeadFeatures::test_g7_resample


def run_resample(eng, device, prec, D, H, Br, max_batch, n_dead, num_cap, x_dtype="fp32", use_rows=False, use_dec=False,
                 zero_row=None, seed=1):
    """One ``wsae_resample_dead`` call on fabricated row errors (runs of exact ties) against ``OO.resample``."""
    from whisper_sae import _native as N
    handle = eng.ctx(prec_code(prec), max_batch)
    lay = OO.layout(D, H)
    total, off = lay
    pack = synth.normal((total,), 50 + seed, 1) * np.float32(0.1)
    n_src = Br + 5 if use_rows else Br
    src_np = synth.activations(n_src, D, seed=51 + seed, stream=Br % 97, bf16=(x_dtype == "bf16"))
    rows_np = ((np.arange(Br, dtype=np.int64) * 3 + 2) % n_src).astype(np.int32) if use_rows else None
    if zero_row is not None:
        src_np[rows_np[zero_row] if use_rows else zero_row] = 0
    # errors on a coarse grid: long runs of exactly tied values; the zero row gets the single highest error
    err_np = ((synth.counter_u64(Br, 52 + seed, 1) % np.uint64(max(2, min(Br // 4, 29)))).astype(np.float32) * np.float32(0.5))
    if zero_row is not None:
        err_np[zero_row] = np.float32(1e6)
    dec_np = synth.normal((Br, D), 53 + seed, 2) if use_dec else None
    mask_np = np.zeros(H, np.uint8)
    mask_np[(np.arange(n_dead) * 5 + 1) % H] = 1
    assert int(mask_np.sum()) == n_dead
    last_np = np.arange(H, dtype=np.int64) - 4
    SC = 4242
    ref = OO.resample(pack, lay, src_np, err_np, mask_np, last_np, SC, num_cap, rows=rows_np, dec_src=dec_np)
    params = Guarded(device, pack, 3)
    src = torch.from_numpy(src_np).to(device)
    if x_dtype == "bf16":
        src = src.to(torch.bfloat16)
    rows = None if rows_np is None else torch.from_numpy(rows_np).to(device)
    err = torch.from_numpy(err_np).to(device)
    dec = None if dec_np is None else torch.from_numpy(dec_np).to(device)
    mask = torch.from_numpy(mask_np).to(device)
    last = torch.from_numpy(last_np.copy()).to(device)
    sc = torch.tensor([SC], dtype=torch.int64, device=device)
    n_out = torch.full((1,), -1, dtype=torch.int32, device=device)
    rc = eng.lib.wsae_resample_dead(handle, params.ptr, src.data_ptr(), N.DT_BF16 if x_dtype == "bf16" else N.DT_F32,
                                    0 if rows is None else rows.data_ptr(), Br, err.data_ptr(), mask.data_ptr(),
                                    last.data_ptr(), sc.data_ptr(), num_cap, n_out.data_ptr(),
                                    0 if dec is None else dec.data_ptr(), eng.stream())
    N.check(rc, f"wsae_resample_dead(Br = {Br})")
    torch.cuda.synchronize()
    got = params.payload()
    assert int(n_out.item()) == ref["n_dead_out"]
    assert np.array_equal(last.cpu().numpy(), ref["last"])
    feats = ref["features"]
    We_g, Wd_g = got[off[0]:off[1]].reshape(H, D), got[off[1]:off[2]].reshape(H, D)
    We_r, Wd_r = ref["pack"][off[0]:off[1]].reshape(H, D), ref["pack"][off[1]:off[2]].reshape(H, D)
    if len(feats):
        # the 1e-6 bound separates any two candidate rows: a feature that took another row of a tie is ~1 away
        assert np.abs(We_g[feats] - We_r[feats]).max() / np.abs(We_r[feats]).max() < RESAMPLE_REL
        assert np.abs(Wd_g[feats] - Wd_r[feats]).max() / np.abs(Wd_r[feats]).max() < RESAMPLE_REL
        assert not got[off[2]:off[3]][feats].any()
    keep = np.ones(total, bool)
    for f in feats:
        keep[off[0] + f * D: off[0] + (f + 1) * D] = False
        keep[off[1] + f * D: off[1] + (f + 1) * D] = False
        keep[off[2] + f] = False
    assert np.array_equal(got[keep].view(np.int32), pack[keep].view(np.int32))  # every other feature, b_d and b_pre: untouched
    assert params.sentinels_intact()  # (the Adam moments are not even passed to this call)
    if zero_row is not None and len(feats):
        assert ref["order"][0] == zero_row and not We_g[feats[0]].any()  # 0 / max(0, 1e-12): zeros, not NaN
        assert use_dec or not Wd_g[feats[0]].any()  # (with dec_src the decoder row is the residual's direction)
    return ref


@pytest.mark.parametrize("cid,prec,D,Br,n_dead,cap,x_dtype,use_rows,use_dec,zero_row", [
    ("one_row_many_dead", "fp32", 32, 1, 5, -1, "fp32", False, False, None),
    ("ties_zero_row", "fp32", 32, 3, 3, -1, "fp32", False, False, 1),
    ("cap0", "fp32", 32, 3, 4, 0, "fp32", False, False, None),
    ("cap5_bf16_rows", "bf16", 1280, 1000, 40, 5, "bf16", True, False, 17),
    ("dec_src", "fp32", 1280, 1000, 40, -1, "fp32", False, True, None),
    ("dec_src_rows_bf16", "bf16", 32, 1000, 64, -1, "bf16", True, True, 3),
    ("more_dead_than_rows", "fp32", 1280, 3, 40, -1, "fp32", True, False, None),
])
def test_resample_chain(rigs, device, cid, prec, D, Br, n_dead, cap, x_dtype, use_rows, use_dec, zero_row):
    """``wsae_resample_dead`` direct: dead list (ascending, capped), row sort, rewritten rows, b_e = 0, last = step_count,
    n_dead_out, everything else bit-identical; fp32 and bf16 inputs, through ``rows``, the ``dec_src`` variant, a
    zero-norm row, more dead features than rows, caps 0 / 5 / all.

    Catches: an unstable tie order in the row sort (the errors sit on a coarse grid: most rows are tied); n_dead_out
    clamped to the row count; ``dec_src`` indexed by the gathered row; a NaN from the zero-norm row."""
    eng = rigs(D, 64)
    ref = run_resample(eng, device, prec, D, 64, Br, 1024, n_dead, cap, x_dtype, use_rows, use_dec, zero_row)
    if cid == "cap0":
        assert ref["n_dead_out"] == 0 and len(ref["features"]) == 0


def test_resample_rejects_more_than_16384_rows(rigs, device):
    """The documented limit: 16385 rows need a 32768-key sort (256 KB of LDS) and are refused before any launch.
    Catches: a limit raised past what a block's LDS can hold, or an error text that no longer names it."""
    from whisper_sae import _native as N
    eng = rigs(32, 64)
    handle = eng.ctx(prec_code("fp32"), 16384)
    z = torch.zeros(64, dtype=torch.int64, device=device)
    rc = eng.lib.wsae_resample_dead(handle, z.data_ptr(), z.data_ptr(), N.DT_F32, 0, 16385, z.data_ptr(), z.data_ptr(),
                                    z.data_ptr(), z.data_ptr(), -1, z.data_ptr(), 0, eng.stream())
    assert rc == -1 and "max 16384 rows" in N.last_error()


def test_resample_8192_rows(rigs, device):
    """The trainer's default resample batch: exactly 64 KB of sort keys, 8 keys per thread, long runs of tied errors.
    Catches: an unstable tie order in the row sort at a size where every thread holds several keys."""
    run_resample(rigs(32, 64), device, "fp32", 32, 64, 8192, 16384, 40, -1, zero_row=100, seed=2)


# (the two launches above 64 KB of dynamic LDS run last, each on its own: a rejected launch is WSAE_ERR_HIP, a clean failure)
def test_resample_8193_rows(rigs, device):
    """One row past 64 KB: a 16384-key sort, 128 KB of dynamic LDS (``wsae_ctx_create`` raises the kernel's dynamic-LDS
    limit for it).  Catches: a runtime that rejects the launch (WSAE_ERR_HIP), padding keys sorted among the rows."""
    run_resample(rigs(32, 64), device, "fp32", 32, 64, 8193, 16384, 64, -1, use_rows=True, seed=3)


def test_resample_16384_rows(rigs, device):
    """The documented maximum: 16384 rows, every key slot a real row, the ``dec_src`` variant, a cap of 33.
    Catches: a rejected 128 KB launch; a sort that relies on padding keys being present; n_dead_out ignoring the cap."""
    run_resample(rigs(32, 64), device, "fp32", 32, 64, 16384, 16384, 40, 33, use_dec=True, zero_row=9000, seed=4)

