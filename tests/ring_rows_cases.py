"""Row-list cases of the TopK step (tests/test_gpu_ring_rows.py, tests/test_ring_rows_cases.py): the adversarial buffer and
list, the case table, and the comparison of a device step with the float64 oracle.  Pure numpy; runs anywhere.

``make_case(B, D, seed)``: a buffer of N = B + B // 2 + 37 rows and an int32 list of B of them, built so that every way of
reading the wrong row changes the numbers and none of them can fault:

* ``rows[b] != b`` everywhere, the list is not monotone, ``rows[0] == N - 1`` and ``rows[B - 1] == 0``;
* B // 16 entries repeat an earlier one (one inside its own 4-row group, one from another 64-row chunk);
* every buffer row the list never names is NaN, and the list is handed over as the middle of a longer array
  (``padded[64 : 64 + B]``) whose other entries name NaN rows: reading past either end of the list, or a row the list does
  not name, gives NaN, and every index anywhere in the array is inside the buffer.
"""

from __future__ import annotations

from typing import NamedTuple

import numpy as np

from oracle import sae_oracle as O
from oracle import synth

KEYS = ("encoder.weight", "encoder.bias", "decoder.weight", "decoder.bias", "b_pre")
GRADS = {"W_e": "encoder.weight", "b_e": "encoder.bias", "W_d": "decoder.weight", "b_d": "decoder.bias", "b_pre": "b_pre"}
MODE = {"bf16": "amp", "fp32": "fp32"}
LR = 1e-4
DEAD_THRESHOLD = 1000
WEIGHT_SEED = 31   # the weights of tests/test_gpu_kernel_variants.py::CASES
X_STREAM, ROW_STREAM, REPEAT_STREAM, PAD_STREAM = 5, 41, 42, 43
FRONT, BACK = 64, 256  # list entries in front of and behind the view (64 int32 = 256 bytes: the view stays 256-byte aligned)

# the suite's bounds (tests/test_gpu_bench_config.py, tests/test_gpu_parity.py): relative to the tensor maximum
LOSS_REL = 1e-5
VALS_REL = 1e-5
GRAD_REL = {"bf16": 2e-3, "fp32": 2e-5}
NORM_REL = {"bf16": 1e-4, "fp32": 1e-5}


class Spec(NamedTuple):
    cid: str
    mode: str      # arithmetic mode of the step: "bf16" (use_amp) or "fp32"
    buffer: str    # element type of the buffer the list points into
    D: int
    H: int
    K: int
    B: int
    oracle: bool   # held to the float64 oracle as well (every case with B <= 2100)
    dense_wgrad: bool
    why: str
    seed: int = 31


# Direct gather: a bf16 buffer in bf16 mode; the GEMM, the decode and the weight-gradient launch read the caller's buffer
# through the list.  Staged gather: stage_batch_kernel reads through the list, the decode reads the caller's buffer in its
# own dtype.
SPECS = [
    Spec("g1", "bf16", "bf16", 384, 3072, 32, 2100, True, False,
         "persistent GEMM a_rows on a ragged last 256-row tile, strip TopK, MFMA decode 4-wave prefetch, wgrad2s xrows with a "
         "ragged last chunk"),
    Spec("g2", "bf16", "bf16", 128, 1024, 16, 1100, True, False,
         "encode_gemm_kernel slab_load_rows (ragged tile), MFMA decode width 128, bucket_kernel x->xT 16-byte path, wgrad_kernel"),
    Spec("g3", "bf16", "bf16", 224, 2048, 32, 1100, True, False,
         "slab_load_rows K tail, VALU decode_kernel, bucket_kernel scalar-tail path (d0 + 64 > D), wgrad_kernel<..., 2>"),
    Spec("g4", "bf16", "bf16", 96, 1024, 16, 300, True, False,
         "encode_direct_kernel (ragged 128-row block), decode_kernel NCH = 1, scalar-tail transposition, wgrad_kernel<..., 1>"),
    Spec("g5", "bf16", "bf16", 256, 2048, 32, 300, True, False, "MFMA decode width 256"),
    Spec("g6", "bf16", "bf16", 1280, 5120, 64, 200, True, False,
         "MFMA decode k > 32 at ten pieces, wgrad2s xrows with the partial column tile, 8-row last chunk"),
    Spec("g7", "bf16", "bf16", 512, 4096, 32, 2048, True, False,
         "persistent GEMM + strips, decode_kernel ROUND_DPRE, x->xT blocks in front of wgrad2_kernel<bf16, false>"),
    Spec("g8", "bf16", "bf16", 64, 512, 8, 300, True, False, "decode_fast_kernel<bf16, 2, 4>"),
    # equality tier only: tests/test_gpu_kernel_variants.py r18 pins the tensor run of this shape to the oracle
    Spec("g9", "bf16", "bf16", 384, 3072, 32, 16424, False, False,
         "chunked decode (one block per 64-row chunk) with a ragged last chunk, presorted wgrad2s"),
    Spec("g10", "bf16", "bf16", 384, 3072, 32, 300, True, True, "WSAE_WGRAD_SPARSE=0: wgrad2_kernel<bf16, true> / W2RowDma"),
    Spec("s1", "bf16", "fp32", 384, 3072, 32, 300, True, False, "stage_batch_kernel<F32, bf16>, MFMA decode XDT = F32"),
    Spec("s2", "bf16", "fp32", 96, 1024, 16, 300, True, False, "decode_kernel<bf16, ..., XDT = F32>"),
    Spec("s3", "fp32", "fp32", 384, 3072, 32, 300, True, False, "stage_batch_kernel<F32, float>, decode_fast<float, 12, 16>"),
    Spec("s4", "fp32", "bf16", 384, 3072, 32, 300, True, False, "stage_batch_kernel<BF16, float>, decode_fast<float, ..., XDT = BF16>"),
    Spec("s5", "fp32", "fp32", 160, 1024, 100, 500, True, False, "decode_kernel<float>, k > 64, wgrad_kernel<float, 2>"),
    Spec("s6", "fp32", "bf16", 64, 512, 8, 300, True, False, "decode_fast<float, 2, 4>"),
]
# The MFMA decode fetches a row's list entry in two places: the first row of a wave before its loop, and every later row one
# row ahead inside it.  A wave gets a second row only when the batch is larger than one resident round of workgroups (at
# most WSAE_MAX_PARTIALS = 1024 blocks of four waves), which of the cases above only g1 (4-wave form) and g9 (chunked form)
# are.  These put the other instantiations through the one-row-ahead fetch: B = 4200 > 4 * 1024.  Equality tier only.
PREFETCH_SPECS = [
    Spec("p1", "bf16", "bf16", 128, 1024, 16, 4200, False, False, "MFMA decode width 128, second row of a wave"),
    Spec("p2", "bf16", "bf16", 256, 2048, 32, 4200, False, False, "MFMA decode width 256, second row of a wave"),
    Spec("p3", "bf16", "bf16", 1280, 5120, 64, 4200, False, False, "MFMA decode k > 32 at ten pieces, second row of a wave"),
    Spec("p4", "bf16", "fp32", 384, 3072, 32, 4200, False, False, "MFMA decode XDT = F32, 4-wave form, second row of a wave"),
    Spec("p5", "bf16", "fp32", 384, 3072, 32, 16424, False, False, "MFMA decode XDT = F32, chunked form with a ragged last chunk"),
]
ALL_SPECS = SPECS + PREFETCH_SPECS
SPEC = {s.cid: s for s in ALL_SPECS}
# equality tier only, at (384, 3072, 32, 300) on a bf16 buffer: BatchTopK through the trainer
B1 = Spec("b1", "bf16", "bf16", 384, 3072, 32, 300, False, False, "BatchTopKSAE: the selection between TopK and decode")
DENSE_SHAPES = ("g1", "g2", "g4")  # wsae_encode_dense (stages even in bf16 mode)


class Case(NamedTuple):
    buffer: np.ndarray   # float32 [N, D], bf16-representable, NaN in every row the list does not name
    clean: np.ndarray    # the same values without the NaN rows (CPU tests build faulted results from it)
    rows: np.ndarray     # int32 [B] == padded[FRONT : FRONT + B]
    padded: np.ndarray   # int32 [FRONT + B + BACK]; outside the view: indices of NaN rows
    unused: np.ndarray   # the buffer rows the list does not name


def build_rows(B: int, N: int, seed: int) -> np.ndarray:
    assert B >= 72 and N >= B + 2
    order = np.argsort(synth.counter_u64(N - 2, seed, ROW_STREAM), kind="stable") + 1  # a permutation of 1 .. N - 2
    rows = np.empty(B, dtype=np.int64)
    rows[1:B - 1] = order[:B - 2]
    rows[0], rows[B - 1] = N - 1, 0
    for b in range(1, B - 1):  # no entry names its own position (the values are distinct, so a swap mends both places)
        if rows[b] == b:
            o = b + 1 if b + 1 < B - 1 else b - 1
            rows[b], rows[o] = rows[o], rows[b]
    words = synth.counter_u64(4 * B, seed, REPEAT_STREAM)
    n_rep = B // 16
    same_group = next((p, q) for p in (5, 6, 7) for q in range(4, p) if rows[q] != p)
    far_p = B - 3
    far_q = next(q for q in range(1, 64) if rows[q] != far_p)
    taken = {same_group[0], far_p}
    targets, i = [], 0
    while len(targets) < n_rep - 2:  # positions 8 .. B - 4 that take the value of an earlier position
        p = 8 + int(words[i] % np.uint64(B - 11))
        i += 1
        if p not in taken:
            taken.add(p)
            targets.append(p)
    for j, p in enumerate(sorted(targets)):
        q = int(words[2 * B + j] % np.uint64(p))
        while rows[q] == p:
            q = (q + 1) % p
        rows[p] = rows[q]
    rows[same_group[0]] = rows[same_group[1]]
    rows[far_p] = rows[far_q]
    return rows.astype(np.int32)


def make_case(B: int, D: int, seed: int) -> Case:
    N = B + B // 2 + 37
    clean = synth.activations(N, D, seed, X_STREAM, bf16=True)
    rows = build_rows(B, N, seed)
    used = np.zeros(N, dtype=bool)
    used[rows] = True
    unused = np.nonzero(~used)[0]
    buffer = clean.copy()
    buffer[unused] = np.nan
    pick = (synth.counter_u64(FRONT + B + BACK, seed, PAD_STREAM) % np.uint64(len(unused))).astype(np.int64)
    padded = unused[pick].astype(np.int32)
    padded[FRONT:FRONT + B] = rows
    return Case(buffer, clean, padded[FRONT:FRONT + B], padded, unused)


def weights(D: int, H: int) -> dict:
    return synth.sae_weights(D, H, seed=WEIGHT_SEED, bf16=True, b_pre_scale=0.1)


def oracle_state(spec: Spec) -> O.SAEState:
    return O.SAEState.from_state_dict(weights(spec.D, spec.H), k=spec.K, dead_feature_threshold=DEAD_THRESHOLD)


def rel(a, b) -> float:
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


class Mismatch(AssertionError):
    """A product of the step outside its bound; ``what`` names the product."""

    def __init__(self, what: str, detail=""):
        super().__init__(f"{what}: {detail}")
        self.what = what


def _hold(ok: bool, what: str, detail="") -> None:
    if not ok:
        raise Mismatch(what, detail)


def compare_with_oracle(dev: dict, st: O.SAEState, x: np.ndarray, K: int, mode: str, note=None, tag: str = "") -> dict:
    """One train step's products ``dev`` against ``O.train_step`` on ``x`` from ``st`` (advanced by the call).

    ``dev``: idx int [B, K], vals float32 [B, K], grads {W_e, b_e, W_d, b_d, b_pre}, loss, l0, grad_norm,
    dead_feature_ratio, last_activated int64 [H], step_count.  Raises ``Mismatch`` naming the first product outside its
    bound, in the order of the step (selection, loss, l0, vals, the five gradients, grad_norm, the dead clock); returns the
    measured gaps, each also handed to ``note(key, measured, bound)``.
    """
    gaps = {}

    def gap(name, measured, bound):
        gaps[name] = measured
        if note is not None:
            note(f"{tag}_{name}", measured, bound)
        _hold(measured < bound, name, f"{measured:.3e} against {bound:.0e}")

    idx = np.asarray(dev["idx"])
    try:
        sel, clear = O.reconcile_selection(st, x, idx, K, MODE[mode])
    except AssertionError as e:
        raise Mismatch("selection", str(e)) from None
    gaps["clear"] = clear
    _hold(clear > 0.98, "selection", f"only {clear:.4f} of the rows have a clear TopK margin")
    r = O.train_step(st, x, LR, MODE[mode], max_norm=1.0, select=sel)
    gap("loss", abs(float(dev["loss"]) - r["loss"]) / r["loss"], LOSS_REL)
    _hold(float(dev["l0"]) == r["l0"], "l0", f"{dev['l0']} against {r['l0']}")
    vals_o = np.take_along_axis(r["fwd"]["pre"], np.sort(sel, axis=1), axis=1)
    vals_d = np.take_along_axis(np.asarray(dev["vals"]), np.argsort(idx, axis=1), axis=1)
    _hold(bool(np.isfinite(vals_d).all()), "vals", "not finite")
    gap("vals", rel(vals_d, vals_o), VALS_REL)
    for n in GRADS:
        g = np.asarray(dev["grads"][n])
        _hold(bool(np.isfinite(g).all()), n, "not finite")
        gap(n, rel(g, r["grads"][n]), GRAD_REL[mode])
    gap("grad_norm", abs(float(dev["grad_norm"]) - r["grad_norm"]) / r["grad_norm"], NORM_REL[mode])
    _hold(float(dev["dead_feature_ratio"]) == r["dead_feature_ratio"], "dead_feature_ratio",
          f"{dev['dead_feature_ratio']} against {r['dead_feature_ratio']}")
    _hold(np.array_equal(np.asarray(dev["last_activated"]), st.last_activated), "feature_last_activated")
    _hold(int(dev["step_count"]) == st.step_count, "step_count", f"{dev['step_count']} against {st.step_count}")
    return gaps
