#!/usr/bin/env python3
"""Compare the kernel images (*.co) of two lib/ directories, variants/ included.

    scripts/image_identity.py <lib_a> <lib_b>

An image is equal when the two files are byte-identical ("identical"), or, failing
that, when .text, .rodata and .data have equal contents, .bss has equal size and
every kernel's note metadata agrees on VGPR count, SGPR count, both spill counts,
group segment size and private segment size ("sections+metadata": what a renamed
source file or a define the code never reads leaves).  One line per image; exit
status 1 on any difference and on any image found on one side only.

Needs the ROCm LLVM tools (llvm-readelf, llvm-objcopy): $ROCM_PATH/llvm/bin, else PATH.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

CONTENT_SECTIONS = (".text", ".rodata", ".data")
META_KEYS = (".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
             ".group_segment_fixed_size", ".private_segment_fixed_size")


def tool(name):
    p = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", name)
    p = p if os.path.exists(p) else shutil.which(name)
    if not p:
        sys.exit(f"{name} not found (set ROCM_PATH)")
    return p


def images(lib):
    return {os.path.relpath(os.path.join(d, f), lib)
            for d, _, fs in os.walk(lib) for f in fs if f.endswith(".co")}


def section_sizes(co):
    """{name: size} from the section table."""
    out = subprocess.check_output([tool("llvm-readelf"), "-S", "-W", co], text=True)
    return {m.group(1): int(m.group(2), 16)
            for m in re.finditer(r"^\s*\[\s*\d+\]\s+(\S+)\s+\S+\s+[0-9a-f]+\s+[0-9a-f]+\s+([0-9a-f]+)", out, re.M)}


def section_bytes(co, name, tmp):
    dump = os.path.join(tmp, "section")
    subprocess.check_call([tool("llvm-objcopy"), f"--dump-section={name}={dump}", co, os.path.join(tmp, "copy")])
    with open(dump, "rb") as f:
        return f.read()


def kernel_metadata(co):
    """{kernel name: {key: value}} from the AMDGPU metadata note."""
    out = subprocess.check_output([tool("llvm-readelf"), "--notes", co], text=True)
    kernels, cur = {}, None
    for line in out.splitlines():
        m = re.match(r"\s*(- )?(\.\w+):\s*(\S.*)?$", line)
        if not m:
            continue
        if m.group(1):  # a new list entry: a kernel once it has .name and the counts
            cur = {}
            kernels[id(cur)] = cur
        if cur is not None and (m.group(2) in META_KEYS or m.group(2) == ".name"):
            cur.setdefault(m.group(2), (m.group(3) or "").strip())
    return {k[".name"]: {m: k.get(m) for m in META_KEYS} for k in kernels.values() if ".vgpr_count" in k}


def differences(a, b, tmp):
    sa, sb = section_sizes(a), section_sizes(b)
    diff = []
    for s in CONTENT_SECTIONS:
        if (s in sa) != (s in sb) or (s in sa and section_bytes(a, s, tmp) != section_bytes(b, s, tmp)):
            diff.append(s)
    if sa.get(".bss", 0) != sb.get(".bss", 0):
        diff.append(".bss size")
    ma, mb = kernel_metadata(a), kernel_metadata(b)
    if not ma or ma != mb:
        diff.append("kernel metadata")
    return diff


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    la, lb = sys.argv[1], sys.argv[2]
    ia, ib = images(la), images(lb)
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for name in sorted(ia | ib):
            if name not in ia or name not in ib:
                print(f"{name}: ONLY IN {la if name in ia else lb}")
                bad += 1
                continue
            a, b = os.path.join(la, name), os.path.join(lb, name)
            with open(a, "rb") as fa, open(b, "rb") as fb:
                same = fa.read() == fb.read()
            if same:
                print(f"{name}: identical")
                continue
            diff = differences(a, b, tmp)
            if diff:
                print(f"{name}: DIFFERENT ({', '.join(diff)})")
                bad += 1
            else:
                print(f"{name}: equal sections+metadata")
    print(f"{len(ia | ib)} images, {bad} different")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
