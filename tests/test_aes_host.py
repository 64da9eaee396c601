"""CPU: the burst cipher's block code and key schedules on the host.

tests/cxx/test_aes_host.cc includes aes_device.h (the T-table rounds, the
last round's S-box recovery, the PKCS#7 check) and aes_sched.h (the key
schedules the launches make) with plain arrays plugged in, and holds them to
FIPS 197 and to libcrypto's EVP: the arithmetic of the kernels in
aes_kernels.hip, run without a GPU.  It then runs the lane kernels' own
per-datagram code (aes_cbc.h: the prep steps and the CBC chain of each
direction) over one-datagram bursts in exact-size heap buffers, bit for bit
against EVP and the documented codes.  Built here under AddressSanitizer and
UBSan as a stand-alone program and run as a child process; it exits non-zero
with a message on the first mismatch.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"    # the compiler of tests/test_fuzz_host.py
FLAGS = ["-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
         "-Wno-unknown-pragmas", "-Wno-pass-failed",    # aes_device.h's unroll hints
         "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_aes_block_code_on_the_host(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("ROCm clang not present")
    exe = tmp_path / "test_aes_host"
    build = subprocess.run(
        [CLANG, *FLAGS, "-I", os.path.join(ROOT, "ilias_net2_amd", "csrc"),
         "-o", str(exe), os.path.join(ROOT, "tests", "cxx", "test_aes_host.cc"),
         "-lcrypto"], cwd=ROOT, capture_output=True, text=True)
    if build.returncode != 0 and "openssl/evp.h" in build.stderr:
        pytest.skip("libcrypto's headers not present")
    assert build.returncode == 0, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([str(exe)], cwd=tmp_path, capture_output=True, text=True,
                         env=env, timeout=300)
    assert run.returncode == 0, (run.stderr + run.stdout)[-4000:]
    assert "test_aes_host: ok" in run.stdout
