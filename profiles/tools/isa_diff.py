#!/usr/bin/env python3
"""Compare the gfx950 instructions of two source trees, kernel by kernel.  Needs hipcc, no GPU.

    python profiles/tools/isa_diff.py PARENT_TREE NEW_TREE [--out DIR] [--jobs N]

Every ``whisper-sae_amd/csrc/*.hip`` of both trees is compiled with

    hipcc --offload-arch=gfx950 --cuda-device-only -S -O3 -std=c++17 -I include -I whisper-sae_amd/csrc FILE.hip

Blank lines, comment lines, directive lines (a leading ``.``, labels of basic blocks among them) and trailing comments are
dropped.  What is compared PER KERNEL SYMBOL is the instruction sequence between the symbol's label and the end of the
function, and the ``.amdhsa_*`` resource lines of its kernel descriptor (VGPR, SGPR, accum offset, LDS, scratch, ...).
The comparison is textual: it knows no instruction names.  Verdict per kernel:

    identical    same instructions in the same order, same resource lines
    permuted     same multiset of instructions, another order in [first, last]; resource lines as stated
    differs      another multiset; the counts and the differing range are printed

With ``--out DIR`` the report goes to DIR/summary.txt too, and a unified diff of every kernel that is not identical to
DIR/<file>.<symbol>.diff.  Exit status 0 when every kernel is identical, 1 otherwise (a refactor may tolerate some: read
the report).
"""
from __future__ import annotations

import argparse
import collections
import concurrent.futures
import difflib
import os
import re
import subprocess
import sys
import tempfile
from pathlib import Path

CSRC = Path("whisper-sae_amd") / "csrc"
BLOCK_LABEL = re.compile(r"\.LBB\d+_")


def compile_asm(tree: Path, src: Path, out: Path) -> None:
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-S", "-O3", "-std=c++17", "-I", str(tree / "include"),
                    "-I", str(tree / CSRC), str(src), "-o", str(out)], check=True, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)


def parse(text: str) -> dict[str, tuple[list[str], list[str]]]:
    """symbol -> (instructions, resource lines) of every kernel of one assembly file."""
    functions: set[str] = set()
    insts: dict[str, list[str]] = {}
    res: dict[str, list[str]] = {}
    cur_fn = cur_desc = None
    for raw in text.splitlines():
        line = raw.split(";", 1)[0].strip()
        if not line or line.startswith("//"):
            continue
        if line.startswith(".type") and line.endswith("@function"):
            functions.add(line.split()[1].split(",")[0])
        elif line.startswith(".amdhsa_kernel "):
            cur_desc = line.split()[1]
            res[cur_desc] = []
        elif line.startswith(".end_amdhsa_kernel"):
            cur_desc = None
        elif cur_desc is not None and line.startswith(".amdhsa_"):
            res[cur_desc].append(" ".join(line.split()))
        elif line.endswith(":") and line[:-1] in functions:
            cur_fn = line[:-1]
            insts[cur_fn] = []
        elif line.startswith(".Lfunc_end"):
            cur_fn = None
        elif cur_fn is not None and not line.startswith("."):
            insts[cur_fn].append(BLOCK_LABEL.sub(".LBB_", " ".join(line.split())))
    return {k: (insts.get(k, []), r) for k, r in res.items()}


def compare(name: str, a, b, out_dir: Path | None, stem: str) -> tuple[str, str]:
    (ia, ra), (ib, rb) = a, b
    same_res = ra == rb
    res_txt = "resources identical" if same_res else "RESOURCES DIFFER: " + "; ".join(
        f"{x} -> {y}" for x, y in zip(ra, rb) if x != y)
    if ia == ib:
        return ("identical" if same_res else "differs"), f"{len(ia)} instructions, {res_txt}"
    first = next(i for i, (x, y) in enumerate(zip(ia, ib)) if x != y) if len(ia) and len(ib) else 0
    tail = 0
    while tail < min(len(ia), len(ib)) - first and ia[-1 - tail] == ib[-1 - tail]:
        tail += 1
    span = f"differing range: parent [{first}, {len(ia) - tail}) of {len(ia)}, new [{first}, {len(ib) - tail}) of {len(ib)}"
    if out_dir is not None:
        diff = difflib.unified_diff(ia, ib, "parent", "new", lineterm="", n=2)
        (out_dir / f"{stem}.{name}.diff").write_text("\n".join(diff) + "\n")
    if collections.Counter(ia) == collections.Counter(ib):
        return ("permuted" if same_res else "differs"), f"same multiset, {span}, {res_txt}"
    return "differs", f"{span}, {res_txt}"


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent", type=Path)
    ap.add_argument("new", type=Path)
    ap.add_argument("--out", type=Path, default=None)
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--only", action="append", default=[], metavar="STEM", help="compare this file only (repeatable)")
    args = ap.parse_args()
    if args.out is not None:
        args.out.mkdir(parents=True, exist_ok=True)
    names = sorted({p.name for t in (args.parent, args.new) for p in (t / CSRC).glob("*.hip")})
    if args.only:
        names = [n for n in names if n[:-len(".hip")] in args.only]
    report: list[str] = []
    worst = 0
    with tempfile.TemporaryDirectory(prefix="isa_diff_") as tmp:
        jobs = {}
        with concurrent.futures.ThreadPoolExecutor(args.jobs) as pool:
            for side, tree in (("parent", args.parent), ("new", args.new)):
                for n in names:
                    if (tree / CSRC / n).exists():
                        out = Path(tmp) / f"{side}.{n}.s"
                        jobs[(side, n)] = (pool.submit(compile_asm, tree, tree / CSRC / n, out), out)
        for n in names:
            stem = n[:-len(".hip")]
            if ("parent", n) not in jobs or ("new", n) not in jobs:
                report.append(f"{stem}: only in {'parent' if ('parent', n) in jobs else 'new'}")
                worst = 1
                continue
            sides = []
            for side in ("parent", "new"):
                fut, out = jobs[(side, n)]
                fut.result()
                sides.append(parse(out.read_text()))
            ka, kb = sides
            counts = collections.Counter()
            lines = []
            for sym in sorted(set(ka) | set(kb)):
                if sym not in ka or sym not in kb:
                    verdict, detail = "differs", f"only in {'parent' if sym in ka else 'new'}"
                else:
                    verdict, detail = compare(sym, ka[sym], kb[sym], args.out, stem)
                counts[verdict] += 1
                if verdict != "identical":
                    lines.append(f"    {verdict:9s} {sym}: {detail}")
                    worst = 1
            report.append(f"{stem}: {len(set(ka) | set(kb))} kernels, " +
                          ", ".join(f"{counts[v]} {v}" for v in ("identical", "permuted", "differs") if counts[v]))
            report.extend(lines)
    text = "\n".join(report) + "\n"
    sys.stdout.write(text)
    if args.out is not None:
        (args.out / "summary.txt").write_text(text)
    return worst


if __name__ == "__main__":
    sys.exit(main())
