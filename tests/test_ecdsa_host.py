"""CPU: the P-521 verification's arithmetic on the host.

tests/cxx/test_ecdsa_host.cc includes the headers the device kernel is made of
(p521_field.h, p521_scalar.h, p521_point.h, ecdsa_p521.h) with a plain array
as the register file, and holds them to libcrypto: field and scalar
operations to BN_mod_*, the point programs to EC_POINT_dbl / EC_POINT_add on
random points and on every exceptional case, the last comparison on crafted
(X, Z, r), and ecdsa_p521_verify_one to ECDSA_do_verify over vectors written
here: a cut through the construction lattice (tests/ecdsa_ref.py) and
OpenSSL-signed messages.  Built under AddressSanitizer and UBSan as a
stand-alone program, as tests/test_aes_host.py builds its own, and run as a
child process.
"""
import hashlib
import os
import random
import struct
import subprocess

import pytest

import ecdsa_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
FLAGS = ["-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
         "-Wno-unknown-pragmas", "-Wno-pass-failed",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def host_cases():
    """A few hundred verifications: every lattice scalar at least once under
    every key, the small scalars crossed in full under the small keys (where
    the running point meets G and Q themselves), infinity cases, signed
    messages of every digest-length class, and corrupted signatures."""
    n = ecdsa_ref.order()
    keys = ecdsa_ref.lattice_keys()
    u1s, u2s = ecdsa_ref.lattice_scalars()
    cases = []
    for ki, d in enumerate(keys):
        pairs = {(u1, u2s[(5 * i + ki) % len(u2s)]) for i, u1 in enumerate(u1s)}
        pairs |= {(u1s[(7 * j + ki) % len(u1s)], u2) for j, u2 in enumerate(u2s)}
        cases += ecdsa_ref.lattice([d], sorted(pairs))
    small = [(a, b) for a in range(6) for b in range(1, 6)]
    cases += ecdsa_ref.lattice(keys[:3], small)
    rng = random.Random(7)
    for i, dlen in enumerate([0, 1, 20, 32, 48, 64, 65, 66, 67, 100] * 3):
        d = rng.randrange(1, n)
        dig = hashlib.shake_256(b"msg %d" % i).digest(dlen)
        if i % 10 == 7:
            dig = b"\xff" * dlen        # e = 2^521 - 1, above n
        r, s = ecdsa_ref.sign(d, dig)
        pub = ecdsa_ref.public_key(d)
        for rr, ss, dd in ((r, s, dig), (r ^ 1, s, dig), (r, n - s, dig),
                           (r, s, dig[:-1] + bytes([dig[-1] ^ 1]) if dig else dig),
                           (0, s, dig), (r, n, dig), (r + n, s, dig)):
            cases.append((pub, rr, ss, dd, ecdsa_ref.verify(pub, rr, ss, dd)))
        bad = bytearray(pub)
        bad[131] ^= 1                   # off the curve
        cases.append((bytes(bad), r, s, dig, ecdsa_ref.verify(bytes(bad), r, s, dig)))
    return cases


def test_p521_arithmetic_on_the_host(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("ROCm clang not present")
    exe = tmp_path / "test_ecdsa_host"
    build = subprocess.run(
        [CLANG, *FLAGS, "-I", os.path.join(ROOT, "ilias_net2_amd", "csrc"),
         "-o", str(exe), os.path.join(ROOT, "tests", "cxx", "test_ecdsa_host.cc"),
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
                         text=True, env=env, timeout=300)
    assert run.returncode == 0, (run.stderr + run.stdout)[-4000:]
    assert "test_ecdsa_host: ok" in run.stdout
    assert f"{len(cases)} vectors" in run.stdout
