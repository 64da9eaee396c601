"""CPU: the bulk table updates' op reduction and per-record bodies on the host.

tests/cxx/test_tab_ops_host.cc includes net2_tab_ops.h (the op list of a launch
reduced to one record per slot; the records) and tab_update.h (what one lane of
the update kernels of tab_kernels.hip does with a record) with the host's
compressions and a plain S-box plugged in, and compares the tables they leave,
byte for byte, with tables built the per-slot way (hmac_key_mids plus
keytab_set_kernel's meta rules; aes_tab_fill_rx / aes_tab_fill_tx).
Built here under AddressSanitizer and UBSan as a stand-alone program and run
as a child process; it exits non-zero with a message on the first mismatch.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"    # the compiler of tests/test_aes_host.py
FLAGS = ["-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
         "-Wno-unknown-pragmas", "-Wno-pass-failed",    # the headers' unroll hints
         "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_table_update_ops_on_the_host(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("ROCm clang not present")
    exe = tmp_path / "test_tab_ops_host"
    build = subprocess.run(
        [CLANG, *FLAGS, "-I", os.path.join(ROOT, "ilias_net2_amd", "csrc"),
         "-I", os.path.join(ROOT, "tests", "cxx", "hipstub"),
         "-o", str(exe), os.path.join(ROOT, "tests", "cxx", "test_tab_ops_host.cc")],
        cwd=ROOT, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    assert "warning" not in build.stderr, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([str(exe)], cwd=tmp_path, capture_output=True, text=True,
                         env=env, timeout=300)
    assert run.returncode == 0, (run.stderr + run.stdout)[-4000:]
    assert "test_tab_ops_host: ok" in run.stdout
