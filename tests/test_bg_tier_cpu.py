"""The background tier's split (skybox_rt_amd/csrc/runtime/bg_tier.h) on the
CPU: tests/native/bg_tier_check.cpp, a stand-alone program with its own main,
is built against the header -- with AddressSanitizer and UBSan, their runtimes
linked statically, when the host toolchain has them -- and run in the caller's
environment as it is.  It sweeps chunk counts 1..600, every heavy-tile count,
grids from 1 up to the chunk count, 1 / 2 / 4 waves per workgroup and several
costs of a geometry chunk, and checks for every case that every chunk is dealt
to exactly one wave, geometry chunks to the workgroups below the tag only and
background chunks to the rest, that no tier of a tiered launch is empty and no
geometry wave is left without a chunk, and that the tag is 0 exactly in the
cases that must stay untiered.  No GPU.

(That every chunk descriptor at or past 16 * heavy tiles has count 0 is
asserted on the device's table, tests/test_gpu_bg_tier.py: the host setup
path builds no descriptor table.)"""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "bg_tier_check.cpp")
INC = os.path.join(ROOT, "skybox_rt_amd", "csrc", "runtime")


def _build(tmp, flags):
    exe = os.path.join(tmp, "bg_tier_check")
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    p = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags, "-I", INC,
                        "-o", exe, SRC], capture_output=True, text=True)
    return exe, p


def test_bg_tier_split_program(tmp_path):
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
    print("bg_tier_check built as:", what)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failure(s)" in r.stdout
