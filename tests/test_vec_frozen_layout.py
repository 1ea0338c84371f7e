"""csrc/vec_frozen_layout.h without a GPU: tests/vec_frozen_layout_check.cpp is built by the host compiler alone, with the
address and undefined-behaviour sanitizers, and run as a process of its own.  It holds the assertions about the plan of a
pieces call with index pieces (mir_blocks_search_pieces_indexed), on hand-made and on seeded random calls: the occurrences
flatten to each query's scope with every ordinal once; an index piece is a group from one ride on, behind the shared
groups, and sizes nothing of the shared search; the row prefix maps every index row to its (block, row), around empty
blocks too; a call without index pieces has plan_pieces' plan and carve_pieces' layout; the workspace's pieces lie in the
documented order without overlap."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_index_occurrences_prefixes_and_layout_hold_in_a_sanitized_host_build(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.fail("no host C++ compiler found (CXX, c++, g++, clang++)")
    exe = str(tmp_path / "vec_frozen_layout_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "ai-dial-rag_amd", "csrc"),
                            os.path.join(ROOT, "tests", "vec_frozen_layout_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "vec_frozen_layout: ok" in run.stdout
