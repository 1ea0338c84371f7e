"""csrc/vec_pieces_layout.h without a GPU: tests/vec_pieces_layout_check.cpp is built by the host compiler alone, with the
address and undefined-behaviour sanitizers, and run as a process of its own.  It holds the assertions: what the pieces
search's host form refuses (with the texts), the 2^32-row limit of a flattened scope, the plan - occurrences, ordinal
maps, group_ptr / scope_ptr as the shared search expects them - on hand-made and on seeded random calls, the workspace's
pieces in the documented order, and the merge's rule against std::stable_sort on (key, ordinal, row)."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_refusals_plan_layout_and_merge_rule_hold_in_a_sanitized_host_build(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.fail("no host C++ compiler found (CXX, c++, g++, clang++)")
    exe = str(tmp_path / "vec_pieces_layout_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "ai-dial-rag_amd", "csrc"),
                            os.path.join(ROOT, "tests", "vec_pieces_layout_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "vec_pieces_layout: ok" in run.stdout
