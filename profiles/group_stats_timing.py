"""Time the two kernels of the group statistics against their plain-torch formulations (profiles/group_stats_note.md):

pooling    (a) ``wsae_pool_update`` straight from the compact code (ordered fp32 sums, no float atomics);
           (b) ``index_add_`` of the active values into a dense ``[S, H]`` fp32 matrix (float atomics: its sums depend on
               the order the hardware happens to take).  The flat cell index and the masked values of (b) are prepared
               outside the timed region; that preparation is timed on its own.
bootstrap  (a) ``wsae_group_effect`` (point statistics, R replicates, quantiles and standard error, fp64);
           (b) torch in fp64: per group two ``matmul``s ``[R, n_g] x [n_g, H]`` (weights times z and z^2), the replicate
               statistic, ``torch.quantile`` and ``std`` over the replicates.

384 -> 3072 shape: H = 3072, k = 32, 1500 frames per utterance, S = 2048 utterances, R = 1000; and H = 40960 through a
window of 4096 features.  Distinct indices per row, a fifth of the values <= 0.  One process, alternating windows of (a)
and (b), device events, median and p10-p90.

    python profiles/group_stats_timing.py [--out outputs/group_stats_timing.json]
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "whisper-sae_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from whisper_sae import _native as N  # noqa: E402
from whisper_sae.analysis import bootstrap_weights  # noqa: E402

K, T, S, R, ALPHA = 32, 1500, 2048, 1000, 0.05
SHAPES = [(3072, 0, 3072), (40960, 8192, 4096)]  # (H, f_lo, f_cols)


def timed(fn, iters: int) -> list:
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for start, end in pairs:
        start.record()
        fn()
        end.record()
    torch.cuda.synchronize()
    return [start.elapsed_time(end) * 1e3 for start, end in pairs]


def summary(samples: list) -> dict:
    a = np.asarray(samples)
    return {"median_us": float(np.median(a)), "p10_us": float(np.percentile(a, 10)), "p90_us": float(np.percentile(a, 90)),
            "n": int(a.size)}


def draw_code(H: int, rows: int, gen):
    """[rows, K] code with distinct indices per row (Gumbel top-k) and about a fifth of the values <= 0."""
    idx = torch.empty(rows, K, dtype=torch.int32, device="cuda:0")
    step = max(256, (1 << 25) // H)
    for r0 in range(0, rows, step):
        n = min(step, rows - r0)
        idx[r0:r0 + n] = torch.rand(n, H, device="cuda:0", generator=gen).topk(K, dim=1).indices.int()
    vals = torch.randn(rows, K, device="cuda:0", generator=gen) + 0.85
    return vals.contiguous(), idx.contiguous()


def torch_effect(X, div, group, boot, alpha):
    """The plain-torch formulation of wsae_group_effect -> (d, ci_lo, ci_hi, se)."""
    x = X.double() / div.double()[:, None]
    stat = []
    w = boot.clamp(min=0).double()
    for g in (0, 1):
        m = torch.nonzero((group == g) & (div > 0)).flatten()
        xg = x[m]
        mu = xg.mean(0)
        z = xg - mu
        var = (z * z).sum(0) / (m.numel() - 1)
        wg = w[:, m]
        n = wg.sum(1, keepdim=True)
        s1, s2 = wg @ z, wg @ (z * z)
        stat.append((mu, var, float(m.numel()), mu + s1 / n, (s2 - s1 * s1 / n).clamp(min=0) / (n - 1), n))

    def cohen(ma, va, na, mb, vb, nb):
        sp = torch.sqrt(((na - 1) * va + (nb - 1) * vb) / (na + nb - 2))
        return torch.where(sp == 0, torch.zeros_like(sp), (ma - mb) / sp)

    (ma, va, na, ra, rva, nra), (mb, vb, nb, rb, rvb, nrb) = stat
    d = cohen(ma, va, na, mb, vb, nb)
    ds = cohen(ra, rva, nra, rb, rvb, nrb)
    q = torch.quantile(ds, torch.tensor([0.5 * alpha, 1 - 0.5 * alpha], dtype=torch.float64, device=ds.device), dim=0)
    return d, q[0], q[1], ds.std(0)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--utterances", type=int, default=S)
    ap.add_argument("--frames", type=int, default=T)
    ap.add_argument("--out", default="outputs/group_stats_timing.json")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    lib = N.lib()
    stream = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    n_seg, frames = args.utterances, args.frames
    rows = n_seg * frames
    seg = torch.arange(n_seg, dtype=torch.int32, device=dev).repeat_interleave(frames).contiguous()
    labels = torch.arange(n_seg) % 2
    group = labels.int().to(dev)
    boot = bootstrap_weights(labels, R, seed=0, device=dev).contiguous()
    results = []
    for H, f_lo, f_cols in SHAPES:
        vals, idx = draw_code(H, rows, gen)
        sums = torch.zeros(n_seg, f_cols, dtype=torch.float32, device=dev)
        cnt_rows = torch.zeros(n_seg, dtype=torch.int32, device=dev)
        ws = torch.empty(lib.wsae_pool_workspace_bytes(rows, K, H, n_seg, f_lo, f_cols), dtype=torch.uint8, device=dev)

        def pool_new():
            N.check(lib.wsae_pool_update(vals.data_ptr(), idx.data_ptr(), K, H, seg.data_ptr(), rows, n_seg, f_lo, f_cols,
                                         sums.data_ptr(), None, f_cols, cnt_rows.data_ptr(), ws.data_ptr(), ws.numel(),
                                         stream()), "wsae_pool_update")

        def prepare():
            act = (vals > 0) & (idx >= f_lo) & (idx < f_lo + f_cols)
            cell = (seg[:, None].long() * f_cols + (idx.long() - f_lo))[act]
            return cell, vals[act]

        cell, active = prepare()
        dense = torch.zeros(n_seg * f_cols, dtype=torch.float32, device=dev)

        def pool_torch():
            dense.index_add_(0, cell, active)

        sums.zero_()
        cnt_rows.zero_()
        pool_new()
        pool_torch()
        torch.cuda.synchronize()
        pool_diff = float((sums.double() - dense.view(n_seg, f_cols).double()).abs().max())
        pool_scale = float(sums.abs().max())
        for fn in (pool_new, pool_torch, prepare):
            fn()
        torch.cuda.synchronize()
        t_new, t_old, t_prep = [], [], []
        for _ in range(args.windows):
            t_new += timed(pool_new, args.iters)
            t_old += timed(pool_torch, args.iters)
            t_prep += timed(prepare, 2)
        sn, so = summary(t_new), summary(t_old)
        entries = int(active.numel())
        del dense, cell, active

        # the effect sizes on one pass of pooled sums
        sums.zero_()
        cnt_rows.zero_()
        pool_new()
        need = lib.wsae_group_effect_workspace_bytes(n_seg, f_cols, R)
        ews = torch.empty(need, dtype=torch.uint8, device=dev)
        out = torch.empty(7, f_cols, dtype=torch.float64, device=dev)
        rec = torch.zeros(3, dtype=torch.int32, device=dev)
        o = [out[i].data_ptr() for i in range(7)]

        def effect_new(boot_ptr=boot.data_ptr(), n_boot=R):
            N.check(lib.wsae_group_effect(sums.data_ptr(), f_cols, cnt_rows.data_ptr(), group.data_ptr(), n_seg, f_cols,
                                          boot_ptr, n_boot, ALPHA, *o, rec.data_ptr(), ews.data_ptr(), need, stream()),
                    "wsae_group_effect")

        def effect_point():
            effect_new(None, 0)

        def effect_torch():
            return torch_effect(sums, cnt_rows, group, boot, ALPHA)

        effect_new()
        ref = effect_torch()
        torch.cuda.synchronize()
        got = (out[2], out[4], out[5], out[6])
        eff_diff = [float(((a - b).abs() / (1e-3 + b.abs())).max()) for a, b in zip(got, ref)]
        for fn in (effect_new, effect_torch, effect_point):
            fn()
        torch.cuda.synchronize()
        e_new, e_old, e_point = [], [], []
        for _ in range(args.windows):
            e_new += timed(effect_new, args.iters)
            e_old += timed(effect_torch, args.iters)
            e_point += timed(effect_point, args.iters)
        effect_new()
        torch.cuda.synchronize()
        en, eo = summary(e_new), summary(e_old)
        fma = 2.0 * R * n_seg * f_cols  # S1 and S2 of every (replicate, feature), one group per utterance
        row = {"hidden": H, "f_lo": f_lo, "f_cols": f_cols, "k": K, "utterances": n_seg, "frames_per_utterance": frames,
               "rows": rows, "active_entries_in_window": entries, "replicates": R,
               "wsae_pool_update": sn, "torch_index_add": so, "torch_index_add_preparation": summary(t_prep),
               "pool_ratio_torch_over_new": so["median_us"] / sn["median_us"],
               "pool_code_gbytes_per_s": rows * K * 8 / sn["median_us"] / 1e3,
               "pool_max_abs_difference_to_index_add": pool_diff, "pool_max_abs_sum": pool_scale,
               "wsae_group_effect": en, "wsae_group_effect_point_only": summary(e_point), "torch_fp64_matmul_quantile": eo,
               "effect_ratio_torch_over_new": eo["median_us"] / en["median_us"],
               "effect_fp64_fma_per_call": fma, "effect_fp64_tflops": 2.0 * fma / en["median_us"] / 1e6,
               "effect_max_rel_difference_to_torch": dict(zip(("d", "ci_lo", "ci_hi", "se"), eff_diff)),
               "kept_replicates": int(rec[2])}
        print(json.dumps(row), flush=True)
        results.append(row)
        del vals, idx, sums, ews, out
        torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "windows": args.windows,
           "iters_per_window": args.iters, "results": results}
    out_path = Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
