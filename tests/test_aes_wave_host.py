"""CPU: the wave form of the burst cipher's RX decrypt, modelled on the host.

tests/cxx/test_aes_wave_host.cc includes aes_wave.h (which block a lane takes
in a pass, the order of the passes, a block's prev, when the padding verdict
is taken), aes_device.h and aes_sched.h, and runs a 64-lane wave in lockstep
over them the way aes_cbc_decrypt_wave_kernel does: per run every lane's loads
before any lane's stores.  In place and to a separate buffer against
libcrypto's EVP for 1 to 200 blocks and 4,090; every block visited once; with
broken padding nothing of either buffer changes.  Built here under
AddressSanitizer and UBSan as a stand-alone program and run as a child
process, like tests/test_aes_host.py.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"    # the compiler of tests/test_aes_host.py
FLAGS = ["-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
         "-Wno-unknown-pragmas", "-Wno-pass-failed",    # aes_device.h's unroll hints
         "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_wave_schedule_on_the_host(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("ROCm clang not present")
    exe = tmp_path / "test_aes_wave_host"
    build = subprocess.run(
        [CLANG, *FLAGS, "-I", os.path.join(ROOT, "ilias_net2_amd", "csrc"),
         "-o", str(exe), os.path.join(ROOT, "tests", "cxx", "test_aes_wave_host.cc"),
         "-lcrypto"], cwd=ROOT, capture_output=True, text=True)
    if build.returncode != 0 and "openssl/evp.h" in build.stderr:
        pytest.skip("libcrypto's headers not present")
    assert build.returncode == 0, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([str(exe)], cwd=tmp_path, capture_output=True, text=True,
                         env=env, timeout=300)
    assert run.returncode == 0, (run.stderr + run.stdout)[-4000:]
    assert "test_aes_wave_host: ok" in run.stdout
