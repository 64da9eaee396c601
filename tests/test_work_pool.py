"""CPU: the library's host threads under ThreadSanitizer.

tests/cxx/test_work_pool.cc includes ilias_net2_amd/csrc/net2_pool.h alone
(WorkPool, the pack pool, and SliceWorker, the per-device slice threads: no
HIP in either) and drives them the way the host pipelines do: two callers on
one pool with widths 1 to 16 and pauses on both sides of both spin windows,
several callers running shard_batch's countdown over a few slice workers.
Built here with -fsanitize=thread as a stand-alone program and run as a child
process; it exits non-zero on a wrong count or on the first sanitizer report.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"    # the compiler of tests/test_aes_host.py
FLAGS = ["-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
         "-fsanitize=thread", "-pthread"]


def test_pool_classes_under_tsan(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("ROCm clang not present")
    exe = tmp_path / "test_work_pool"
    build = subprocess.run(
        [CLANG, *FLAGS, "-I", os.path.join(ROOT, "ilias_net2_amd", "csrc"),
         "-o", str(exe), os.path.join(ROOT, "tests", "cxx", "test_work_pool.cc")],
        cwd=ROOT, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1")
    run = subprocess.run([str(exe)], cwd=tmp_path, capture_output=True, text=True,
                         env=env, timeout=300)
    assert run.returncode == 0, (run.stderr + run.stdout)[-4000:]
    assert "test_work_pool: ok" in run.stdout
