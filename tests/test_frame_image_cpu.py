"""The RT host app's image table, its path resolver and the choice of a frame's
image (skybox_rt_amd/csrc/app/frame_image.h) on the CPU:
tests/native/frame_image_check.cpp, a stand-alone program with its own main,
is built against the header -- with AddressSanitizer and UBSan, their runtimes
linked statically, when the host toolchain has them -- and run in the caller's
environment as it is.  It checks the image a frame runs against known answers
written out for every configuration the API can reach, that over the whole
input product one image comes back (two exactly for the two-kernel path
tracer) and never an instrumented one for a frame that is not, and the three
source rules of the image files under a fake "file exists": the per-file
fallback to the library directory, the path-queue group taken whole from the
kernel directory or not at all, and the images that must lie next to their
anchor image (refused with -2 otherwise: the pt_compact directory).  No GPU."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "frame_image_check.cpp")
INC = os.path.join(ROOT, "skybox_rt_amd", "csrc", "app")


def _build(tmp, flags):
    exe = os.path.join(tmp, "frame_image_check")
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    p = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags, "-I", INC,
                        "-o", exe, SRC], capture_output=True, text=True)
    return exe, p


def test_frame_image_program(tmp_path):
    # the sanitizer runtimes linked statically: the program then runs in the
    # caller's environment as it is, whatever that preloads
    builds = [("address,undefined sanitizers, static runtime",
               ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]),
              ("plain build (no static sanitizer runtime in this toolchain)", [])]
    for what, flags in builds:
        exe, p = _build(str(tmp_path), flags)
        if p.returncode == 0:
            break
        print(f"{what}: not available:", p.stderr[-400:])
    assert p.returncode == 0, p.stderr
    print("frame_image_check built as:", what)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failure(s)" in r.stdout
    for case in ("image table", "known answers", "input product", "rule 1: per-file fallback",
                 "rule 2: the whole group from the kernel directory or nothing",
                 "rule 3: next to the anchor image, or refused"):
        assert f"ok   {case}" in r.stdout
