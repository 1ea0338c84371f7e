"""csrc/hybrid_layout.h without a GPU: tests/hybrid_layout_check.cpp is built by the host compiler alone, with the address
and undefined-behaviour sanitizers, and run as a process of its own.  It holds the assertions: the arrays of
``mir_block_hybrid_search`` follow one another in the documented order at multiples of 256, no two overlap, the upload and
the download spans hold exactly their arrays, 2k = 512 is the last k that fits the fusion kernel, and shapes that are
negative or would not fit a scratch are refused instead of wrapped."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_carve_holds_in_a_sanitized_host_build(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.fail("no host C++ compiler found (CXX, c++, g++, clang++)")
    exe = str(tmp_path / "hybrid_layout_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "ai-dial-rag_amd", "csrc"),
                            os.path.join(ROOT, "tests", "hybrid_layout_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "hybrid_layout: ok" in run.stdout
