"""The driver's lane / join decision (skybox_rt_amd/csrc/runtime/lanes.h) on
the CPU: tests/native/frame_lanes_check.cpp, a stand-alone program with its
own main, is built against the header -- with AddressSanitizer and UBSan,
their runtimes linked statically, when the host toolchain has them -- and run
in the caller's environment as it is.  It checks that frames alternating
between the two lanes insert no cross-lane wait, that an ordinary operation
behind laned launches joins lane 1 into lane 0 exactly once, that the first
lane-1 launch behind ordinary work waits for lane 0, and that with overlap
disabled everything is lane 0.  No GPU."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "frame_lanes_check.cpp")
INC = os.path.join(ROOT, "skybox_rt_amd", "csrc", "runtime")


def _build(tmp, flags):
    exe = os.path.join(tmp, "frame_lanes_check")
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    p = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags, "-I", INC,
                        "-o", exe, SRC], capture_output=True, text=True)
    return exe, p


def test_lane_order_program(tmp_path):
    # the sanitizer runtimes linked statically: the program then runs in the
    # caller's environment as it is, whatever that preloads (a dynamic ASan
    # runtime insists on being the first library loaded)
    builds = [("address,undefined sanitizers, static runtime",
               ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]),
              ("plain build (no static sanitizer runtime in this toolchain)", [])]
    for what, flags in builds:
        exe, p = _build(str(tmp_path), flags)
        if p.returncode == 0:
            break
        print(f"{what}: not available:", p.stderr[-400:])
    assert p.returncode == 0, p.stderr
    print("frame_lanes_check built as:", what)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failure(s)" in r.stdout
    for case in ("alternating", "ordinary joins lane 1 once", "lane 1 waits for ordinary work", "overlap off"):
        assert f"ok   {case}" in r.stdout
