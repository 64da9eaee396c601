"""CPU: the quad form of the burst cipher's TX encrypt, modelled on the host.

tests/cxx/test_aes_quad_host.cc includes aes_quad.h (which column and which
schedule words a lane owns, the word it contributes to a block, the steps of a
block), aes_device.h, aes_sched.h and aes_cbc.h, and steps four lanes in
lockstep over them the way aes_cbc_encrypt_quad_kernel does: per round every
lane's exchange before any lane's round.  One-datagram bursts in exact-size
heap buffers against libcrypto's EVP for 1, 2, 3, 4, 88, 89, 90 and 93 blocks,
every plen mod 16, the payload 8, 40, 56 and 72 bytes into a datagram at an
odd offset, the slot's bytes past plen filled two ways, both key sources; and
the codes the prep steps settle.  Built here under AddressSanitizer and UBSan
as a stand-alone program and run as a child process, like
tests/test_aes_wave_host.py.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"    # the compiler of tests/test_aes_host.py
FLAGS = ["-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
         "-Wno-unknown-pragmas", "-Wno-pass-failed",    # aes_device.h's unroll hints
         "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_quad_schedule_on_the_host(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("ROCm clang not present")
    exe = tmp_path / "test_aes_quad_host"
    build = subprocess.run(
        [CLANG, *FLAGS, "-I", os.path.join(ROOT, "ilias_net2_amd", "csrc"),
         "-o", str(exe), os.path.join(ROOT, "tests", "cxx", "test_aes_quad_host.cc"),
         "-lcrypto"], cwd=ROOT, capture_output=True, text=True)
    if build.returncode != 0 and "openssl/evp.h" in build.stderr:
        pytest.skip("libcrypto's headers not present")
    assert build.returncode == 0, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([str(exe)], cwd=tmp_path, capture_output=True, text=True,
                         env=env, timeout=300)
    assert run.returncode == 0, (run.stderr + run.stdout)[-4000:]
    assert "test_aes_quad_host: ok" in run.stdout
