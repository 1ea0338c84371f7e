"""csrc/bm25_scope_batch_layout.h without a GPU: tests/bm25_scope_batch_layout_check.cpp is built by the host compiler
alone, with the address and undefined-behaviour sanitizers, and run as a process of its own.  It holds the assertions: a
sub-batch's arrays follow one another without overlap and stay within the cap, every scope lands in exactly one sub-batch
or on the host route, the key bits hold the largest ordinal and position, a sub-batch is split at the 64-bit boundary, a
scope over ``table_chunks`` and a scope alone over the workspace cap take the host route, and a call without scopes."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_plan_holds_in_a_sanitized_host_build(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.fail("no host C++ compiler found (CXX, c++, g++, clang++)")
    exe = str(tmp_path / "bm25_scope_batch_layout_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "ai-dial-rag_amd", "csrc"),
                            os.path.join(ROOT, "tests", "bm25_scope_batch_layout_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "bm25_scope_batch_layout: ok" in run.stdout
