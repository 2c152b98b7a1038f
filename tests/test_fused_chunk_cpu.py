"""The conditions under which a configuration's frames carry RT_FLAG_FUSED
(skybox_rt_amd/csrc/app/fused_chunk.h: env RT_FUSED_CHUNK and the render
flags) on the CPU: tests/native/fused_chunk_check.cpp, a stand-alone program
with its own main, is built against the header -- with AddressSanitizer and
UBSan, their runtimes linked statically, when the host toolchain has them --
and run in the caller's environment as it is.  And the flag's value is a bit
of rt_kernel_arg_t.flags no other flag uses.  No GPU."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "fused_chunk_check.cpp")
INC = os.path.join(ROOT, "skybox_rt_amd", "csrc", "app")


def test_fused_chunk_flag_program(tmp_path):
    exe = os.path.join(str(tmp_path), "fused_chunk_check")
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    builds = [("address,undefined sanitizers, static runtime",
               ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]),
              ("plain build (no static sanitizer runtime in this toolchain)", [])]
    for what, flags in builds:
        p = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags, "-I", INC,
                            "-o", exe, SRC], capture_output=True, text=True)
        if p.returncode == 0:
            break
        print(f"{what}: not available:", p.stderr[-400:])
    assert p.returncode == 0, p.stderr
    print("fused_chunk_check built as:", what)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failure(s)" in r.stdout


def test_flag_is_a_bit_of_its_own():
    with open(os.path.join(ROOT, "skybox_rt_amd", "csrc", "kernels", "rt_common.h")) as f:
        flags = dict(re.findall(r"^#define (RT_FLAG_\w+)\s+(0x[0-9a-fA-F]+)u", f.read(), re.M))
    vals = {k: int(v, 16) for k, v in flags.items()}
    assert "RT_FLAG_FUSED" in vals and "RT_FLAG_SHADOWS" in vals
    for k, v in vals.items():
        assert v != 0 and v & (v - 1) == 0, k  # one bit each
    assert len(set(vals.values())) == len(vals)  # no two flags share a bit
