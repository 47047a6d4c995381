"""numpy restatement of the group statistics (include/wsae.h, ``wsae_pool_update`` / ``wsae_group_effect``): pooling by
sequential ``float32`` adds in row order (within a row: entry order), compared with the kernel bit for bit; effect sizes
and the bootstrap in ``float64`` exactly as the header defines them, the quantile being ``np.quantile`` with its default
(linear) method.  Also the input recipes the CPU and the GPU tests share."""

from __future__ import annotations

import numpy as np

FIELDS = ("mean_a", "mean_b", "d", "g", "ci_lo", "ci_hi", "se")
RTOL, ATOL = 1e-9, 1e-12  # both sides fp64; sums of <= 4096 terms differ by their order alone (<= 4096 * 2^-53 ~ 5e-13)


def random_code(rng, rows, k, hidden):
    """The recipe of the co-activation test: about a third of the values <= 0, some exactly 0, a few indices -1 and
    >= hidden; indices may repeat within a row."""
    idx = rng.integers(0, hidden, (rows, k)).astype(np.int32)
    vals = (rng.standard_normal((rows, k)) + 0.45).astype(np.float32)
    vals[rng.random((rows, k)) < 0.05] = 0.0
    bad = rng.random((rows, k)) < 0.01
    idx[bad] = rng.choice(np.array([-1, hidden, hidden + 9, -5], np.int32), int(bad.sum()))
    return vals, idx


def pool(code, hidden, seg, n_seg, f_lo=0, f_cols=None, state=None):
    """-> (sums float32 [n_seg, f_cols], cnt int32 [n_seg, f_cols], rows int32 [n_seg]); ``state``: such a triple to
    continue from (it is not modified)."""
    vals, idx = np.asarray(code[0], np.float32), np.asarray(code[1]).astype(np.int64)
    seg = np.asarray(seg).astype(np.int64)
    f_cols = hidden - f_lo if f_cols is None else f_cols
    if state is None:
        sums, cnt = np.zeros((n_seg, f_cols), np.float32), np.zeros((n_seg, f_cols), np.int32)
        rows = np.zeros(n_seg, np.int32)
    else:
        sums, cnt, rows = (a.copy() for a in state)
    ok_row = (seg >= 0) & (seg < n_seg)
    rows += np.bincount(seg[ok_row], minlength=n_seg).astype(np.int32)
    act = (vals > 0) & (idx >= 0) & (idx < hidden) & (idx >= f_lo) & (idx < f_lo + f_cols) & ok_row[:, None]
    r, e = np.nonzero(act)  # ascending row, then ascending entry
    cell = seg[r] * f_cols + idx[r, e] - f_lo
    v = vals[r, e]
    order = np.argsort(cell, kind="stable")
    cell, v = cell[order], v[order]
    pos = np.arange(cell.size)
    start = np.ones(cell.size, bool)
    start[1:] = cell[1:] != cell[:-1]
    rank = pos - np.maximum.accumulate(np.where(start, pos, 0))  # the occurrence number within the cell
    flat, flat_c = sums.reshape(-1), cnt.reshape(-1)
    for t in range(int(rank.max()) + 1 if cell.size else 0):
        m = rank == t
        flat[cell[m]] = flat[cell[m]] + v[m]  # one float32 add per cell and step
        flat_c[cell[m]] += 1
    return sums, cnt, rows


def cohen_d(ma, va, na, mb, vb, nb):
    sp = np.sqrt(((na - 1.0) * va + (nb - 1.0) * vb) / (na + nb - 2.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(sp == 0.0, 0.0, (ma - mb) / sp)


def effect(X, group, div=None, boot=None, alpha=0.05, reverse=False):
    """-> dict of FIELDS (float64 [F]) and ``record`` (n_a, n_b, kept).  ``reverse``: sum over the members of a group in
    descending instead of ascending order (the oracle's own sensitivity to the order)."""
    X = np.asarray(X, np.float32)
    S, F = X.shape
    group = np.asarray(group).astype(np.int64)
    dv = np.ones(S, np.int64) if div is None else np.asarray(div).astype(np.int64)
    x = X.astype(np.float64) / np.where(dv > 0, dv, 1).astype(np.float64)[:, None]
    members = [np.nonzero((group == g) & (dv > 0))[0] for g in (0, 1)]
    if reverse:
        members = [m[::-1] for m in members]
    na, nb = float(len(members[0])), float(len(members[1]))
    nan = np.full(F, np.nan)
    out = {k: nan.copy() for k in FIELDS}
    out["record"] = (int(na), int(nb), 0)
    if na < 2 or nb < 2:
        return out
    mean = [x[m].sum(0) / len(m) for m in members]
    var = [((x[m] - mu) ** 2).sum(0) / (len(m) - 1.0) for m, mu in zip(members, mean)]
    d = cohen_d(mean[0], var[0], na, mean[1], var[1], nb)
    out.update(mean_a=mean[0], mean_b=mean[1], d=d, g=d * (1.0 - 3.0 / (4.0 * (na + nb) - 9.0)))
    if boot is None:
        return out
    w = np.maximum(np.asarray(boot).astype(np.int64), 0).astype(np.float64)
    tot, rm, rv = [], [], []
    for m, mu in zip(members, mean):
        wg = w[:, m]
        n = wg.sum(1)[:, None]
        z = x[m] - mu
        s1, s2 = wg @ z, wg @ (z * z)
        with np.errstate(divide="ignore", invalid="ignore"):
            rm.append(mu + s1 / n)
            rv.append(np.maximum(s2 - s1 * s1 / n, 0.0) / (n - 1.0))
        tot.append(n)
    keep = (tot[0][:, 0] >= 2) & (tot[1][:, 0] >= 2)
    kept = int(keep.sum())
    out["record"] = (int(na), int(nb), kept)
    if kept == 0:
        return out
    ds = np.sort(cohen_d(rm[0][keep], rv[0][keep], tot[0][keep], rm[1][keep], rv[1][keep], tot[1][keep]), axis=0)
    out["ci_lo"], out["ci_hi"] = np.quantile(ds, [0.5 * alpha, 1.0 - 0.5 * alpha], axis=0)
    if kept >= 2:
        out["se"] = np.std(ds, axis=0, ddof=1)
    return out


def stratified_weights(rng, group, R, balanced=False):
    """int16 [R, S]: every replicate draws n_g (or min(n_a, n_b)) members of each group with replacement."""
    group = np.asarray(group)
    w = np.zeros((R, len(group)), np.int16)
    sizes = [int((group == g).sum()) for g in (0, 1)]
    for g in (0, 1):
        m = np.nonzero(group == g)[0]
        n = min(sizes) if balanced else sizes[g]
        pick = m[rng.integers(0, len(m), (R, n))]
        for r in range(R):
            w[r] += np.bincount(pick[r], minlength=len(group)).astype(np.int16)
    return w


# (n_seg, f_cols, R) of the effect-size cases; the last is point statistics only
EFFECT_SHAPES = [(4, 1, 2), (5, 33, 7), (257, 96, 1000), (4096, 3072, 64), (300, 40, 2048), (64, 50, 0)]


def effect_case(shape, seed=None):
    """Inputs of one effect-size case, from pooled random codes: (X float32 [S, F], div int32 [S], group int32 [S],
    boot int16 [R, S] or None).  Six frames per utterance; every feature has non-zero variance in both groups (asserted),
    so no replicate statistic is a ratio of rounding errors."""
    S, F, R = shape
    rng = np.random.default_rng(1000 + S + F + R if seed is None else seed)
    frames = 6
    k = max(1, min(32, F // 3))
    for _ in range(20):
        vals, idx = random_code(rng, S * frames, k, F)
        X, _, rows = pool((np.abs(vals) + np.float32(0.01), idx % F), F, np.repeat(np.arange(S), frames), S)
        group = (np.arange(S) % 2).astype(np.int32)
        rng.shuffle(group)
        div = rows.astype(np.int32)
        if shape == (5, 33, 7):
            group[:] = (0, 1, 2, 0, 1)  # one ignored label ...
            div[2] = 0                  # ... and one utterance without frames (the same one: two members per group remain)
        if S >= 64:  # ignored labels and utterances without frames, on different utterances
            pick = rng.permutation(S)[:8]
            group[pick[:5]] = 7
            div[pick[5:]] = 0
        x = X / np.maximum(div, 1)[:, None]
        inc = div > 0
        if all(np.all(x[(group == g) & inc].var(0) > 0) for g in (0, 1)):
            break
    else:
        raise AssertionError(f"no draw of {shape} with non-zero variance everywhere")
    boot = stratified_weights(rng, np.where(inc, group, -1), R) if R else None
    return X, div, group, boot
