#!/usr/bin/env python3
"""Static instruction account of a kernel image by source region: the
image's assembly (hipcc -S -gline-tables-only with the Makefile's flags and
defines) split by the source function each instruction's line belongs to, per
instruction class (SALU / SMEM / VALU / VMEM / LDS / branch / other), with the
leading SALU mnemonics per region.

  python3 scripts/salu_account.py IMAGE.s [--top N] > account.json

The .loc line of an instruction is the innermost inlined function's, so a
region is "the code of function f wherever it was inlined".  Counts are
static: a region inlined at several sites counts every copy, and a wave's
dynamic count follows from the path it takes (DESIGN.md 4.1 states the paths
of a background wave and of a heavy wave over these regions)."""
import argparse
import collections
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNC = re.compile(r"^(?:template\s*<[^>]*>\s*)?(?:static\s+|extern\s+\"C\"\s+)?(?:__device__|__global__|inline|VX_MAIN\w*)"
                  r"[^;]*?\b([A-Za-z_]\w*)\s*\(")
SKIP = {"__attribute__", "__launch_bounds__", "if", "for", "while", "switch"}


def functions(path):
    """[(first line, name)] of the function definitions of a source file"""
    out = []
    try:
        lines = open(path, errors="replace").read().split("\n")
    except OSError:
        return out
    for i, ln in enumerate(lines, 1):
        if ln.startswith(("VX_MAIN", "VX_MAIN_OCC")):
            out.append((i, "main"))
            continue
        if not ln.startswith(("__device__", "static", "inline", "extern", "__global__")):
            continue
        m = FUNC.match(ln)
        if m and m.group(1) not in SKIP:
            out.append((i, m.group(1)))
    return out


def classify(mn):
    if mn.startswith(("s_cbranch", "s_branch", "s_setpc", "s_swappc", "s_call")):
        return "branch"
    if mn.startswith(("s_load", "s_buffer_load", "s_memtime", "s_memrealtime", "s_dcache_inv")):
        return "smem"
    if mn.startswith(("s_waitcnt", "s_nop", "s_barrier", "s_endpgm", "s_sleep", "s_sethalt", "s_setprio")):
        return "other"
    if mn.startswith("s_"):
        return "salu"
    if mn.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "vmem"
    if mn.startswith("ds_"):
        return "lds"
    if mn.startswith("v_"):
        return "valu"
    return "other"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("--top", type=int, default=6)
    args = ap.parse_args()
    files, funcs = {}, {}
    region = "?"
    acc = collections.defaultdict(lambda: collections.Counter())
    mnem = collections.defaultdict(lambda: collections.Counter())
    total = collections.Counter()
    in_text = False
    for ln in open(args.asm, errors="replace"):
        s = ln.strip()
        if s.startswith(".file"):
            m = re.match(r'\.file\s+(\d+)\s+"([^"]*)"\s+"([^"]*)"', s)
            if m:
                p = os.path.join(m.group(2), m.group(3))
                files[int(m.group(1))] = p
                funcs[int(m.group(1))] = functions(p)
            continue
        if s.startswith(".loc"):
            p = s.split()
            f, line = int(p[1]), int(p[2])
            name = "?"
            for first, n in funcs.get(f, ()):
                if first <= line:
                    name = n
                else:
                    break
            region = f"{os.path.basename(files.get(f, '?'))}:{name}"
            continue
        if s.startswith(".text"):
            in_text = True
        if not in_text or not s or s.startswith((".", ";", "//")) or s.endswith(":"):
            continue
        mn = s.split()[0]
        if not re.match(r"^(s_|v_|ds_|buffer_|global_|flat_|scratch_)", mn):
            continue
        c = classify(mn)
        acc[region][c] += 1
        total[c] += 1
        if c == "salu":
            mnem[region][mn] += 1
    regions = []
    for r, c in sorted(acc.items(), key=lambda kv: -kv[1]["salu"]):
        regions.append({"region": r, **{k: c.get(k, 0) for k in ("salu", "smem", "valu", "vmem", "lds", "branch", "other")},
                        "salu_top": dict(mnem[r].most_common(args.top))})
    json.dump({"asm": os.path.basename(args.asm), "total": dict(total), "regions": regions}, sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()
