"""CPU: the prepared-key arithmetic of the P-521 verification on the host.

tests/cxx/test_ecdsa_key_host.cc includes p521_keytab.h -- the code the lanes
of ecdsa_key_kernels.hip run -- with a plain array as the register file and
holds it to libcrypto: the tables of G and of the keys d = 1, 2, n - 1 and a
random one entry by entry to EC_POINT_mul, refused keys to valid = 0, and the
verification from tables to ECDSA_do_verify over the vectors of
test_ecdsa_host.host_cases().  Built under AddressSanitizer and UBSan as a
stand-alone program with the flags of tests/test_ecdsa_host.py, and run as a
child process.
"""
import os
import struct
import subprocess

import pytest

import ecdsa_ref
from test_ecdsa_host import CLANG, FLAGS, host_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_p521_key_tables_on_the_host(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("ROCm clang not present")
    header = os.path.join(ROOT, "ilias_net2_amd", "csrc", "p521_keytab.h")
    assert os.path.exists(header), "p521_keytab.h is missing"
    exe = tmp_path / "test_ecdsa_key_host"
    build = subprocess.run(
        [CLANG, *FLAGS, "-I", os.path.join(ROOT, "ilias_net2_amd", "csrc"),
         "-o", str(exe), os.path.join(ROOT, "tests", "cxx", "test_ecdsa_key_host.cc"),
         "-lcrypto"], cwd=ROOT, capture_output=True, text=True)
    if build.returncode != 0 and "openssl/bn.h" in build.stderr:
        pytest.skip("libcrypto's headers not present")
    assert build.returncode == 0, build.stderr[-3000:]
    cases = host_cases()
    assert sum(c[4] for c in cases) > 300 and sum(1 - c[4] for c in cases) > 100
    vec = tmp_path / "vectors.bin"
    with open(vec, "wb") as f:
        for pub, r, s, dig, want in cases:
            f.write(struct.pack("<132s132sI128sB3x", pub, ecdsa_ref.be66(r) +
                                ecdsa_ref.be66(s), len(dig), dig, want))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([str(exe), str(vec)], cwd=tmp_path, capture_output=True,
                         text=True, env=env, timeout=600)
    assert run.returncode == 0, (run.stderr + run.stdout)[-4000:]
    assert "test_ecdsa_key_host: ok" in run.stdout
    assert f"{len(cases)} vectors" in run.stdout
