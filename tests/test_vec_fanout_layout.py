"""csrc/vec_fanout_layout.h without a GPU: tests/vec_fanout_layout_check.cpp is built by the host compiler alone, with the
address and undefined-behaviour sanitizers, and run as a process of its own.  It holds the assertions about the fan-out of
the expanded block search (mir_blocks_search_expanded): check_fanout accepts hand-made and seeded random valid maps and
refuses each violation with a message of its own; expand_reference - the definition the device kernel is held to - equals
a brute-force stable sort of the fully expanded scope on seeded random scopes with ties, -0 / +0, NaN, blocks without a
fan-out, blocks listed twice, k from 1 to beyond the expanded rows and k > 64; the stored-row lists' piece of the
workspace lies behind carve_scoped's layout, the fan-out table inside its input span."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fanout_checks_and_the_expansion_reference_hold_in_a_sanitized_host_build(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.fail("no host C++ compiler found (CXX, c++, g++, clang++)")
    exe = str(tmp_path / "vec_fanout_layout_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "ai-dial-rag_amd", "csrc"),
                            os.path.join(ROOT, "tests", "vec_fanout_layout_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "vec_fanout_layout: ok" in run.stdout
