"""csrc/ensemble_layout.h without a GPU: tests/ensemble_layout_check.cpp is built by the host compiler alone, with the
address and undefined-behaviour sanitizers, and run as a process of its own.  It holds the assertions: the arrays of
``mir_block_ensemble_search`` follow one another in the documented order at multiples of 256, no two overlap, the upload
and the download spans are contiguous and hold exactly their arrays, two vector legs on the same queries upload them
once, sum k = 512 is the last that fits the fusion kernel, and shapes that are malformed or would not fit a scratch are
refused instead of wrapped.  The sweep: 1-4 legs with the keyword leg at every place or absent, shared and distinct
query pointers, b in {0, 1, 257}, k in {1, 7, 128}, empty tables."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_carve_holds_in_a_sanitized_host_build(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.fail("no host C++ compiler found (CXX, c++, g++, clang++)")
    exe = str(tmp_path / "ensemble_layout_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "ai-dial-rag_amd", "csrc"),
                            os.path.join(ROOT, "tests", "ensemble_layout_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "ensemble_layout: ok" in run.stdout
