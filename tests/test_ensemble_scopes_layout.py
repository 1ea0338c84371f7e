"""csrc/ensemble_scopes_layout.h without a GPU: tests/ensemble_scopes_layout_check.cpp is built by the host compiler alone,
with the address and undefined-behaviour sanitizers, and run as a process of its own.  It holds the assertions: the arrays
of ``mir_block_ensemble_search_scopes`` follow one another in the documented order at multiples of 256, no two overlap,
the upload span (the reference records among its arrays) and the download span are contiguous and hold exactly their
arrays, the tables the gather kernel writes lie outside both, a scope's own allocation holds one descriptor array per
slot and a fan-out array per paged slot, and shapes that are malformed or would not fit are refused instead of wrapped.
The sweep: 0-3 slots, the keyword leg at every place or absent, b in {0, 1, 257}, n_docs in {0, 1, 65, 300}, paged and
plain slots."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_carves_hold_in_a_sanitized_host_build(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.fail("no host C++ compiler found (CXX, c++, g++, clang++)")
    exe = str(tmp_path / "ensemble_scopes_layout_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "ai-dial-rag_amd", "csrc"),
                            os.path.join(ROOT, "tests", "ensemble_scopes_layout_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "ensemble_scopes_layout: ok" in run.stdout
