"""Time ``wsae_profile_update`` and ``wsae_sample_update`` against the torch paths a user would otherwise write
(profiles/activation_profile_note.md):

profile  kernel: one call over the whole code.
         torch:  ``bincount`` of ``feature * 192 + bin`` over the masked entries, ``bincount`` for the counts,
                 ``index_add_`` for the fixed-point sums, ``scatter_reduce_`` for the minimum and maximum.  It yields the
                 same integers, which the script checks before it times anything.
sampler  kernel: S = 10 strata (the profile's quantile edges), m = 8, timed on the first call (empty lists: every entry
                 passes the pre-filter) and on later calls with fresh ordinals (warm lists), with the fraction of the
                 entries that survive the pre-filter.
         torch:  the priority hash in int64 arithmetic, one stable ``sort`` of ``list << 32 | priority`` (entries arrive in
                 ordinal order, so ties keep it), segment heads by ``searchsorted``, the first m of every list.  It yields
                 the same lists as the kernel's first call, which the script checks.

The code is ``persistent_code`` of tests/runs_oracle.py, the code the other notes use (distinct indices per row, all
values positive, no padding - the torch paths rely on that): 2048 utterances of 1500 frames, k = 32, H = 3072 whole width
and H = 40960 through a window of 4096 features.  One shape per process (``--shape``), device events, median and p10-p90;
every process adds its row to the output file.

    python profiles/activation_profile_timing.py --shape 0 [--out outputs/activation_profile_timing.json]
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "whisper-sae_amd"), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import runs_oracle as RO  # noqa: E402
from whisper_sae import _native as N  # noqa: E402
from whisper_sae.analysis.profile import histogram_quantile  # noqa: E402

K, T, UTT = 32, 1500, 2048
SHAPES = [(3072, 0, 3072), (40960, 8192, 4096)]  # (H, f_lo, f_cols)
BINS = N.PROFILE_BINS
STRATA, KEEP, SEED = 10, 8, 7
PROFILE_FIELDS = ("fires", "hist", "max_bits", "min_bits", "over", "sum_q", "total_rows")
M32 = 0xFFFFFFFF


def timed(fn, iters: int, before=None) -> list:
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for n, (start, end) in enumerate(pairs):
        if before is not None:
            before(n)
        start.record()
        fn(n)
        end.record()
    torch.cuda.synchronize()
    return [start.elapsed_time(end) * 1e3 for start, end in pairs]


def summary(samples: list) -> dict:
    a = np.asarray(samples)
    return {"median_us": float(np.median(a)), "p10_us": float(np.percentile(a, 10)), "p90_us": float(np.percentile(a, 90)),
            "n": int(a.size)}


def new_profile(f_cols: int, dev) -> dict:
    z = lambda *shape, dtype=torch.int32: torch.zeros(*shape, dtype=dtype, device=dev)  # noqa: E731
    return {"fires": z(f_cols), "hist": z(f_cols, BINS), "max_bits": z(f_cols),
            "min_bits": torch.full((f_cols,), 0x7F800000, dtype=torch.int32, device=dev), "over": z(f_cols),
            "sum_q": z(f_cols, dtype=torch.int64), "total_rows": z(1, dtype=torch.int64)}


def torch_profile(vals, idx, f_lo: int, f_cols: int, st: dict) -> None:
    """The plain-torch formulation, added into ``st``."""
    dev = vals.device
    i = idx.long() - f_lo
    inside = (vals > 0) & (i >= 0) & (i < f_cols)
    f, v = i[inside], vals[inside]
    bits = v.view(torch.int32)
    cell = ((bits >> 20) - 920).clamp(0, BINS - 1).long()
    st["hist"] += torch.bincount(f * BINS + cell, minlength=f_cols * BINS).view(f_cols, BINS).int()
    st["fires"] += torch.bincount(f, minlength=f_cols).int()
    st["over"] += torch.bincount(f[v >= 4096], minlength=f_cols).int()
    st["sum_q"].index_add_(0, f, torch.round(v.clamp(max=4096.0) * 1048576.0).long())  # (torch.round: half to even)
    st["max_bits"].copy_(torch.maximum(st["max_bits"], torch.zeros(f_cols, dtype=torch.int32, device=dev)
                                       .scatter_reduce_(0, f, bits, "amax")))
    st["min_bits"].copy_(torch.minimum(st["min_bits"], torch.full((f_cols,), 0x7F800000, dtype=torch.int32, device=dev)
                                       .scatter_reduce_(0, f, bits, "amin")))
    st["total_rows"] += vals.shape[0]


def torch_priority(ordinal, f, seed: int):
    """The uint32 priority in int64 arithmetic."""
    x = ((ordinal * 0x9E3779B1) & M32) ^ ((f * 0x85EBCA77) & M32) ^ seed
    x = x ^ (x >> 16)
    x = (x * 0x85EBCA6B) & M32
    x = x ^ (x >> 13)
    x = (x * 0xC2B2AE35) & M32
    return x ^ (x >> 16)


def torch_sample(vals, idx, ord_base: int, f_lo: int, f_cols: int, edges, m: int, seed: int):
    """The first call of the sampler in plain torch -> (keys int64 [f_cols, S, m], svals, seen)."""
    dev = vals.device
    S = edges.shape[1] + 1
    i = idx.long() - f_lo
    inside = (vals > 0) & (i >= 0) & (i < f_cols)
    rows = torch.arange(vals.shape[0], device=dev)[:, None].expand_as(idx)[inside] + ord_base
    c, v = i[inside], vals[inside]
    stratum = torch.zeros_like(c)
    for j in range(S - 1):
        stratum += edges[:, j][c] <= v
    lists = c * S + stratum
    x = torch_priority(rows, c + f_lo, seed)
    order = torch.sort((lists << 32) | x, stable=True).indices
    lists, x, rows, v = lists[order], x[order], rows[order], v[order]
    seen = torch.bincount(lists, minlength=f_cols * S)
    start = torch.cumsum(seen, 0) - seen
    rank = torch.arange(lists.numel(), device=dev) - start[lists]
    top = rank < m
    keys = torch.full((f_cols * S, m), -1, dtype=torch.int64, device=dev)
    svals = torch.zeros(f_cols * S, m, dtype=torch.float32, device=dev)
    keys[lists[top], rank[top]] = (x[top] << 32) | rows[top]
    svals[lists[top], rank[top]] = v[top]
    return keys.view(f_cols, S, m), svals.view(f_cols, S, m), seen.int().view(f_cols, S)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, required=True, choices=range(len(SHAPES)))
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--utterances", type=int, default=UTT)
    ap.add_argument("--frames", type=int, default=T)
    ap.add_argument("--label", default="", help="a name for the build under test (A/B runs)")
    ap.add_argument("--out", default="outputs/activation_profile_timing.json")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    lib = N.lib()
    stream = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    H, f_lo, f_cols = SHAPES[args.shape]
    rows = args.utterances * args.frames
    code = RO.persistent_code(np.random.default_rng(H), rows, K, H)
    vals, idx = torch.from_numpy(code[0]).to(dev), torch.from_numpy(code[1]).to(dev)
    del code

    # ---- the profile ---------------------------------------------------------------------------------------------
    st, st_torch = new_profile(f_cols, dev), new_profile(f_cols, dev)

    def profile_call(_=0):
        N.check(lib.wsae_profile_update(vals.data_ptr(), idx.data_ptr(), K, H, None, rows, f_lo, f_cols, st["fires"].data_ptr(),
                                        st["hist"].data_ptr(), st["max_bits"].data_ptr(), st["min_bits"].data_ptr(),
                                        st["over"].data_ptr(), st["sum_q"].data_ptr(), st["total_rows"].data_ptr(), None, 0, stream()),
                "wsae_profile_update")

    profile_call()
    torch_profile(vals, idx, f_lo, f_cols, st_torch)
    torch.cuda.synchronize()
    same_profile = all(torch.equal(st[f], st_torch[f]) for f in PROFILE_FIELDS)
    active = int(st["fires"].sum())
    edges = torch.stack([histogram_quantile(st["hist"], st["fires"], st["min_bits"], st["max_bits"], j / STRATA)
                         for j in range(1, STRATA)], dim=1).float().contiguous()
    profile_call()  # (warm: the minimum and maximum have settled)
    t_profile = timed(profile_call, args.iters)
    t_profile_torch = timed(lambda _: torch_profile(vals, idx, f_lo, f_cols, st_torch), max(2, args.iters // 3))

    # ---- the sampler ---------------------------------------------------------------------------------------------
    n_lists = f_cols * STRATA
    need = lib.wsae_sample_workspace_bytes(rows, K, H, f_lo, f_cols, STRATA, KEEP)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    keys = torch.full((f_cols, STRATA, KEEP), -1, dtype=torch.int64, device=dev)
    svals = torch.zeros(f_cols, STRATA, KEEP, dtype=torch.float32, device=dev)
    seen = torch.zeros(f_cols, STRATA, dtype=torch.int32, device=dev)

    def reset(_=0):
        keys.fill_(-1)
        svals.zero_()
        seen.zero_()

    def sample_call(ord_base: int):
        N.check(lib.wsae_sample_update(vals.data_ptr(), idx.data_ptr(), K, H, None, rows, ord_base, f_lo, f_cols,
                                       edges.data_ptr(), STRATA, KEEP, SEED, keys.data_ptr(), svals.data_ptr(), seen.data_ptr(),
                                       ws.data_ptr(), need, stream()), "wsae_sample_update")

    def survivors() -> int:
        """The entries that passed the pre-filter of the last call: the total behind the per-list offsets, which the
        workspace holds after its n_lists counts (the layout of wsae_profile.hip)."""
        return int(ws[:4 * (2 * n_lists + 1)].view(torch.int32)[2 * n_lists].item())

    sample_call(0)
    torch.cuda.synchronize()
    first_survivors = survivors()
    tk, tv, tseen = torch_sample(vals, idx, 0, f_lo, f_cols, edges, KEEP, SEED)
    same_sample = torch.equal(tk, keys) and torch.equal(tv, svals) and torch.equal(tseen, seen)
    del tk, tv, tseen
    t_first = timed(lambda _: sample_call(0), args.iters, before=reset)
    # warm lists: every later call brings fresh ordinals (the same code behind them)
    reset()
    sample_call(0)
    warm_fraction = []
    t_warm = []
    for n in range(1, args.iters + 1):
        t_warm += timed(lambda _: sample_call(n * rows), 1)
        warm_fraction.append(survivors() / active)
    t_sample_torch = timed(lambda _: torch_sample(vals, idx, 0, f_lo, f_cols, edges, KEEP, SEED), max(2, args.iters // 3))

    sp, spt, sf, sw, sst = (summary(t) for t in (t_profile, t_profile_torch, t_first, t_warm, t_sample_torch))
    row = {"label": args.label, "hidden": H, "f_lo": f_lo, "f_cols": f_cols, "k": K, "utterances": args.utterances,
           "frames_per_utterance": args.frames, "rows": rows, "active_entries_in_window": active,
           "same_integers_as_torch": bool(same_profile), "wsae_profile_update": sp, "torch_bincount_index_add": spt,
           "ratio_torch_over_kernel_profile": spt["median_us"] / sp["median_us"],
           "profile_code_gbytes_per_s": rows * K * 8 / sp["median_us"] / 1e3,
           "strata": STRATA, "keep": KEEP, "same_lists_as_torch": bool(same_sample),
           "wsae_sample_update_first_call": sf, "wsae_sample_update_warm_calls": sw, "torch_sort_segment_heads": sst,
           "survivor_fraction_first_call": first_survivors / active, "survivor_fraction_warm_calls": warm_fraction,
           "ratio_torch_over_kernel_first_call": sst["median_us"] / sf["median_us"],
           "ratio_torch_over_kernel_warm_calls": sst["median_us"] / sw["median_us"]}
    print(json.dumps(row), flush=True)
    out_path = Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    res = json.loads(out_path.read_text()) if out_path.exists() else {"results": []}
    res.update(device=torch.cuda.get_device_name(0), torch=torch.__version__, iters=args.iters)
    res["results"] = [r for r in res["results"] if (r["hidden"], r.get("label", "")) != (H, args.label)] + [row]
    out_path.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
