"""CPU: the device cipher-key table's entry and the per-datagram rx key choice
on the host.

tests/cxx/test_aes_tab_host.cc includes aes_tab.h (the entry of
``struct net2_burst_ciphertab`` and how it is filled from keys), aes_sched.h
and aes_device.h (aes_rx_alt, aes_block) with plain arrays plugged in, and
aes_cbc.h (the _mc kernels' connection checks and key pick) over an exact-size
table: what the _mc cipher kernels of aes_kernels.hip read and decide, run
without a GPU.
Built here under AddressSanitizer and UBSan as a stand-alone program and run
as a child process; it exits non-zero with a message on the first mismatch.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"    # the compiler of tests/test_aes_host.py
FLAGS = ["-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
         "-Wno-unknown-pragmas", "-Wno-pass-failed",    # aes_device.h's unroll hints
         "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_cipher_table_entry_on_the_host(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("ROCm clang not present")
    exe = tmp_path / "test_aes_tab_host"
    build = subprocess.run(
        [CLANG, *FLAGS, "-I", os.path.join(ROOT, "ilias_net2_amd", "csrc"),
         "-o", str(exe), os.path.join(ROOT, "tests", "cxx", "test_aes_tab_host.cc")],
        cwd=ROOT, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    assert "warning" not in build.stderr, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([str(exe)], cwd=tmp_path, capture_output=True, text=True,
                         env=env, timeout=300)
    assert run.returncode == 0, (run.stderr + run.stdout)[-4000:]
    assert "test_aes_tab_host: ok" in run.stdout
