"""Host model of the activation ring and float64 references of the kernels of ``wsae_ring.hip``, plain numpy.

TEST INFRASTRUCTURE, in the style of the other ``tests/*_oracle.py`` helpers: no torch, nothing from the reference tree.

``RingModel``     the ring's bookkeeping (``wsae_ring_push``, ``wsae_ring_push_layernorm``, ``wsae_ring_fill_synthetic``)
``feistel_rows``  ``wsae_ring_sample`` restated on uint64 arrays: exact
``layernorm``     ``ring_push_ln_kernel`` / ``wsae_layernorm_rows``: float64 value and a derived element-wise bound
``decode_dense``  ``decode_dense_kernel``: float64 value and a derived element-wise bound
``ln_inputs``     the input families the LayerNorm bound is exercised on (CPU emulation and GPU kernel alike)

Bound of the row LayerNorm.  u = 2^-24 is the relative error of one correctly rounded fp32 operation (add, multiply,
fma, division); loads are exact (bf16 -> fp32 widens).  A sum of terms in which every term passes through at most n
roundings is off by at most n u sum|term|.  The kernel (``wsae_layernorm.h``), one wave per row, lane l owning the
columns l, l + 64, .. in ``vpl`` registers, with h the row, D its width and m|h| = sum|h| / D:

  mean   a lane adds its vpl registers (vpl - 1 roundings, the first add is to 0), the xor butterfly adds 6 times, one
         division by D (exact in fp32):                       dmu  = (vpl + 6) u m|h|
  c      c = v - mean, one subtraction of the carried mean:    dc   = dmu + u (|c| + dmu)
  var    a lane's fmaf chain rounds vpl times (c c is exact inside the fma), 6 tree adds, one division, one add of eps.
         The terms are non-negative, so their own roundings are relative to the result; the carried c moves each
         square by at most 2 |c| dc + dc^2:
                                                               dve  = mean(2 |c| dc + dc^2) + (vpl + 7) u var + u ve
  rstd   rsqrtf(ve).  The carried part is taken exactly, not to first order, since dve / ve reaches 0.4 on rows with
         a large mean and a small spread:  move = max(sqrt(ve / (ve - dve)) - 1, 1 - sqrt(ve / (ve + dve))),
         plus the function's own error.  ``rsqrtf`` is allowed 2 ulp = 4u: an allowance, not a figure quoted from
         ROCm's HIP math documentation, whose ulp table was not at hand when this was written (``v_rsq_f32`` itself
         is a 1 ulp instruction):                              drel = move + 4u
  y      (c rstd) gamma + beta: two products and one sum (one rounding fewer where the compiler contracts the last two
         into an fma).  The product of the carried c and the carried rstd is kept with its cross term:
           |dy| <= |gamma| rstd (dc + (|c| + dc) drel) + 2u |gamma c rstd| + u |y|

Everything u-sized that is second order (u^2 n^2 < 1e-10) is covered by ``SECOND`` = 1.02; ``FLOOR`` keeps an exact zero
from dividing by zero in a ratio.  No intermediate leaves the normal range on inputs with |c| = 0 or |c| > 2^-60.  The
bound is derived from the operation sequence alone; tests/test_ring_oracle.py shows that an fp32 emulation of the
kernel stays below it and that five plausible mistakes do not.  A bf16 destination rounds once more:
|out - y| <= bound + bf16_ulp(|y| + bound) / 2 (``accept_bf16``).

Bound of the dense decode.  acc = b_d + b_pre (one rounding), then one fmaf per non-zero entry of the code row (one
rounding each), so every term passes through at most n_terms + 1 roundings:
  |drecon| <= (n_terms + 2) u (|b_d| + |b_pre| + sum_j |h_j| |W_dT[j, d]|).
"""

from __future__ import annotations

import numpy as np

from oracle.synth import _splitmix64 as mix64
from oracle.synth import bf16_round, normal

F32 = np.float32
F64 = np.float64
U = 2.0 ** -24
SECOND = 1.02
FLOOR = 2.0 ** -140
RSQRT_U = 4.0  # rsqrtf: 2 ulp, in units of u (see the module docstring)
LN_MAX_DIM = 2048
_M64 = (1 << 64) - 1


def ln_vpl(dim: int) -> int:
    """Registers per lane of the LayerNorm kernel's two instantiations."""
    return 8 if dim <= 512 else 32


def bf16_ulp(y) -> np.ndarray:
    """Spacing of bf16 numbers at |y| (8 significant bits)."""
    m = np.maximum(np.abs(np.asarray(y, dtype=F64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(m)) - 7)


def accept_bf16(y, bound) -> np.ndarray:
    """What a bf16 destination may differ from ``y`` by, given the fp32 bound."""
    return bound + 0.5 * bf16_ulp(np.abs(y) + bound)


# ---- bookkeeping -------------------------------------------------------------------------------------------------------
class RingModel:
    """``capacity`` rows of ``dim`` values and the two counters, as ``wsae.h`` states them: a push writes row r of its
    argument to slot ``(head + r) % capacity``; of a push of more than ``capacity`` rows only the newest ``capacity``
    survive, and ``head`` moves by the full row count; ``size`` saturates at ``capacity``.

    ``dtype``: ``"float32"`` or ``"bfloat16"`` (stores are rounded with ``oracle.synth.bf16_round``).  ``data`` is a
    float64 array holding exactly the stored values, so it can also carry a float64 reference (``push(.., exact=True)``)
    through the same slots."""

    def __init__(self, capacity: int, dim: int, dtype: str = "float32"):
        if dtype not in ("float32", "bfloat16"):
            raise ValueError(dtype)
        self.capacity, self.dim, self.dtype = int(capacity), int(dim), dtype
        self.data = np.zeros((self.capacity, self.dim), F64)
        self.head = 0
        self.size = 0

    def _store(self, a) -> np.ndarray:
        a = np.asarray(a, F32)
        return (bf16_round(a) if self.dtype == "bfloat16" else a).astype(F64)

    def poke(self, values) -> None:
        """Write the whole storage directly (the ``ring.data`` view), counters untouched."""
        self.data[:] = self._store(np.asarray(values).reshape(self.capacity, self.dim))

    def push(self, rows, exact: bool = False) -> np.ndarray:
        """Append ``rows [n, dim]``; returns the slot every row of the argument went to (-1: dropped)."""
        rows = np.asarray(rows).reshape(-1, self.dim)
        n = rows.shape[0]
        slots = np.full(n, -1, np.int64)
        if n == 0:
            return slots
        skip = max(0, n - self.capacity)
        self.head = (self.head + skip) % self.capacity
        kept = np.asarray(rows[skip:], F64) if exact else self._store(rows[skip:])
        where = (self.head + np.arange(n - skip)) % self.capacity
        self.data[where] = kept
        slots[skip:] = where
        self.head = (self.head + (n - skip)) % self.capacity
        self.size = min(self.capacity, self.size + (n - skip))
        return slots

    def fill(self, n: int, seed: int = 42) -> None:
        """``fill_synthetic``: rows 0 .. n - 1 = ``oracle.synth.normal((n, dim), seed, 0)``; size = n, head = n % capacity."""
        if not 1 <= n <= self.capacity:
            raise ValueError(n)
        self.data[:n] = self._store(normal((n, self.dim), seed, 0))
        self.size = int(n)
        self.head = int(n) % self.capacity


# ---- shuffle -----------------------------------------------------------------------------------------------------------
def feistel_key(seed: int, epoch: int) -> np.uint64:
    e = ((int(epoch) & _M64) * 0xD1342543DE82EF95) & _M64
    k = mix64(np.array([int(seed) & _M64], dtype=np.uint64))[0]
    return mix64(np.array([int(k) ^ e], dtype=np.uint64))[0]


def feistel_rows(size: int, seed: int, epoch: int, offset: int, n: int) -> np.ndarray:
    """Row indices ``perm_{seed, epoch}((offset + i) % size)``, i < n, as int64: a four-round Feistel network on the
    enclosing domain of 2^(2 half_bits) values, walked until the value falls below ``size``."""
    size = int(size)
    if size < 1 or n < 0 or offset < 0:
        raise ValueError((size, offset, n))
    bits = 1
    while (1 << bits) < size:
        bits += 1
    half = np.uint64((bits + 1) // 2)
    mask = np.uint64((1 << int(half)) - 1)
    key = feistel_key(seed, epoch)
    v = ((int(offset) + np.arange(n, dtype=np.int64)) % size).astype(np.uint64)
    todo = np.arange(n)
    while todo.size:
        w = v[todo]
        left, right = w >> half, w & mask
        for rnd in range(4):
            f = mix64(right ^ key ^ np.uint64(rnd << 56)) & mask
            left, right = right, left ^ f
        w = (left << half) | right
        v[todo] = w
        todo = todo[w >= np.uint64(size)]
    return v.astype(np.int64)


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------
def layernorm(h, gamma, beta, eps: float, vpl: int):
    """``(y, bound)`` in float64 of gamma (h - mean) / sqrt(var + eps) + beta per row (biased variance); ``bound`` per
    element as the module docstring derives it.  ``h``: the values the kernel loads (bf16 sources already rounded)."""
    h = np.asarray(h, F64)
    g, b = np.asarray(gamma, F64), np.asarray(beta, F64)
    eps = float(F32(eps))  # the ABI passes eps as a float
    mu = h.mean(axis=1, keepdims=True)
    c = h - mu
    var = (c * c).mean(axis=1, keepdims=True)
    ve = var + eps
    rstd = 1.0 / np.sqrt(ve)
    y = g * c * rstd + b
    dmu = (vpl + 6) * U * np.abs(h).mean(axis=1, keepdims=True)
    dc = dmu + U * (np.abs(c) + dmu)
    dve = (2 * np.abs(c) * dc + dc * dc).mean(axis=1, keepdims=True) + (vpl + 7) * U * var + U * ve
    with np.errstate(divide="ignore", invalid="ignore"):
        up = np.where(dve < ve, np.sqrt(ve / np.maximum(ve - dve, 1e-300)) - 1.0, np.inf)
    drel = np.maximum(up, 1.0 - np.sqrt(ve / (ve + dve))) + RSQRT_U * U
    bound = np.abs(g) * rstd * (dc + (np.abs(c) + dc) * drel) + 2 * U * np.abs(g * c * rstd) + U * np.abs(y)
    return y, bound * SECOND + FLOOR


LN_FAMILIES = ("ordinary", "outlier", "large_mean", "small", "constant")


def ln_inputs(family: str, rows: int, dim: int, seed: int) -> np.ndarray:
    """float32 rows of one input family.  ``outlier`` needs dim > 100 (its two loud channels are columns 7 and 100)."""
    n = normal((rows, dim), seed, 11)
    if family == "ordinary":
        return (n * F32(3) + F32(1)).astype(F32)
    if family == "outlier":  # the loud channels of a Whisper residual stream
        out = n.copy()
        out[:, 7], out[:, 100] = F32(3000), F32(-800)
        return out
    if family == "large_mean":  # where a one-pass variance cancels
        return (F32(1000) + F32(0.01) * n).astype(F32)
    if family == "small":  # eps dominates the variance
        return (F32(1e-4) * n).astype(F32)
    if family == "constant":  # the output is beta
        vals = normal((rows,), seed, 12) * F32(3) + F32(2.5)
        return np.repeat(vals[:, None], dim, axis=1).astype(F32)
    raise ValueError(family)


def ln_params(dim: int, seed: int):
    """gamma ~ N(1, 0.2), beta ~ N(0, 0.2), float32."""
    return ((F32(1) + F32(0.2) * normal((dim,), seed, 13)).astype(F32), (F32(0.2) * normal((dim,), seed, 14)).astype(F32))


# ---- dense decode ------------------------------------------------------------------------------------------------------
def decode_dense(hidden, W_dT, b_d, b_pre):
    """``(recon, bound)``: hidden [B, H] @ W_dT [H, D] + b_d + b_pre in float64, and the bound of the module docstring."""
    hid, w = np.asarray(hidden, F64), np.asarray(W_dT, F64)
    bd, bp = np.asarray(b_d, F64), np.asarray(b_pre, F64)
    recon = hid @ w + bd + bp
    n_terms = (hid != 0).sum(axis=1, keepdims=True)
    mag = np.abs(hid) @ np.abs(w) + np.abs(bd) + np.abs(bp)
    return recon, (n_terms + 2) * U * mag + FLOOR
