"""The host arithmetic of the label co-occurrence (csrc/label_band_plan.h: the bins and tiles in LDS, the bands of a pass, the
permutations of a launch chain, the grid that keeps a workgroup's 32-bit bins from overflowing, the packed result) under the address
and undefined-behaviour sanitizers: a stand-alone program (csrc/hosttest/label_band_plan_asan.cpp), compiled with g++ and run as it
is - no GPU, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_label_band_plan_under_address_and_ub_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    csrc = os.path.join(ROOT, "flashdeconv_amd", "csrc")
    exe = str(tmp_path / "label_band_plan_asan")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Werror",
                        "-I", csrc, os.path.join(csrc, "hosttest", "label_band_plan_asan.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    if r.returncode != 0 and ("cannot find -lasan" in r.stderr or "libasan" in r.stderr):
        pytest.skip("no sanitizer runtime")
    assert r.returncode == 0, r.stdout + r.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "ok under the sanitizers" in run.stdout
