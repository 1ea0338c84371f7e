"""csrc/bm25_layout.h without a GPU: tests/bm25_layout_check.cpp is built by the host compiler alone, with the address and
undefined-behaviour sanitizers, and run as a process of its own.  It holds the assertions: the model route's scratch
layout equals its closed form for b in {1, 2, 64, 65, 1025} x T in {1, 3} x k in {1, 64}, its arrays follow one another
in the documented order, and scoped queries are grouped as the two search entries group them."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_and_grouping_hold_in_a_sanitized_host_build(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.fail("no host C++ compiler found (CXX, c++, g++, clang++)")
    exe = str(tmp_path / "bm25_layout_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "ai-dial-rag_amd", "csrc"),
                            os.path.join(ROOT, "tests", "bm25_layout_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "bm25_layout: ok" in run.stdout
