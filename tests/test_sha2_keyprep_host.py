"""CPU: what the keyed launchers compute on the host before a launch.

tests/cxx/test_sha2_keyprep_host.cc includes sha2_keyprep.h (the HMAC key
blocks' midstates, ``hmac_key_mids`` / ``hmac_midstates``, and the constant pad
block's schedule, ``pad_kw256`` / ``pad_kw512``): the launchers' product code,
run without a GPU.  Built here under AddressSanitizer and UBSan as a
stand-alone program and run as a child process over a file of cases whose
expected values are worked out below with ``hmac`` / ``hashlib`` and plain
integer arithmetic; it exits non-zero with a message on the first mismatch.
"""
import hashlib
import hmac
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"    # the compiler of tests/test_aes_tab_host.py
FLAGS = ["-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

# SHA row -> (hashlib name, block, digest length, LENBYTES of the padding)
ROWS = {1: ("sha256", 64, 32, 8), 2: ("sha384", 128, 48, 16), 3: ("sha512", 128, 64, 16)}

# RFC 4231 test cases 1-4 (the keys that fit a block), with the HMAC-SHA-256
# digests the RFC prints
RFC4231 = [
    (b"\x0b" * 20, b"Hi There",
     "b0344c61d8db38535ca8afceaf0bf12b881dc200c9833da726e9376c2e32cff7"),
    (b"Jefe", b"what do ya want for nothing?",
     "5bdcc146bf60754e6a042426089575c75a003f089d2739839dec58b964ec3843"),
    (b"\xaa" * 20, b"\xdd" * 50,
     "773ea91e36800e46854db8ebd09181a72959098b3ef8c122d9635514ced565fe"),
    (bytes(range(1, 26)), b"\xcd" * 50,
     "82558a389a443c0ea4cc819899f2083a85f0faa3e578f8077a2e3ff46729665b"),
]


def _hex(b: bytes) -> str:
    return b.hex() if b else "-"


def _bytes(seed: int, n: int) -> bytes:
    return hashlib.shake_128(seed.to_bytes(4, "big")).digest(n) if n else b""


def _key_cases():
    """(halg, key, alt or None, [messages]): key lengths 1, the digest length,
    block - 1 and block, with and without an alternate key as long; messages
    of 0, 1, block - LENBYTES - 1, block - LENBYTES and 2 block + 3 bytes
    (after the key block: one pad block, the length field just fitting, one
    byte more than fits, several blocks)."""
    seed = 0
    for halg, (_, blk, dlen, lenbytes) in ROWS.items():
        msgs = [_bytes(1000 + halg * 10 + i, n) for i, n in
                enumerate((0, 1, blk - lenbytes - 1, blk - lenbytes, 2 * blk + 3))]
        for klen in (1, dlen, blk - 1, blk):
            for with_alt in (False, True):
                seed += 2
                yield (halg, _bytes(seed, klen),
                       _bytes(seed + 1, klen) if with_alt else None, msgs)
        for key, msg, _ in RFC4231:
            yield halg, key, None, [msg]


def _primes(n):
    out, c = [], 2
    while len(out) < n:
        if all(c % p for p in out):
            out.append(c)
        c += 1
    return out


def _icbrt(x: int) -> int:
    r = 1 << ((x.bit_length() + 2) // 3)    # Newton's iteration from above
    while True:
        y = (2 * r + x // (r * r)) // 3
        if y >= r:
            return r
        r = y


def _pad_kw(bits_w: int, rounds: int, rot, count: int):
    """K[t] + W[t] of the pad block of a message of `count` bits (a multiple
    of the block), FIPS 180-4: K from the primes' cube roots, W from the
    message schedule of 0x80, zeros, the bit count."""
    mask = (1 << bits_w) - 1
    k = [_icbrt(p << (3 * bits_w)) & mask for p in _primes(rounds)]
    ror = lambda x, n: ((x >> n) | (x << (bits_w - n))) & mask  # noqa: E731
    w = [0] * rounds
    w[0] = 1 << (bits_w - 1)
    w[14], w[15] = (count >> bits_w) & mask, count & mask
    (a, b, c), (d, e, f) = rot
    for t in range(16, rounds):
        s0 = ror(w[t - 15], a) ^ ror(w[t - 15], b) ^ (w[t - 15] >> c)
        s1 = ror(w[t - 2], d) ^ ror(w[t - 2], e) ^ (w[t - 2] >> f)
        w[t] = (w[t - 16] + s0 + w[t - 7] + s1) & mask
    return [(k[t] + w[t]) & mask for t in range(rounds)]


def _cases_text() -> str:
    lines = []
    for halg, key, alt, msgs in _key_cases():
        name = ROWS[halg][0]
        lines.append(f"K {halg} {_hex(key)} {_hex(alt or b'')}")
        for m in msgs:
            dig = hmac.new(key, m, name).digest()
            adig = hmac.new(alt, m, name).digest() if alt else b""
            lines.append(f"M {_hex(m)} {_hex(dig)} {_hex(adig)}")
    for halg, (_, blk, _, _) in ROWS.items():
        lines.append(f"R {halg} {_hex(_bytes(77 + halg, blk + 1))}")
    for blocks in (1, 2, 24):
        kw = _pad_kw(32, 64, ((7, 18, 3), (17, 19, 10)), blocks * 64 * 8)
        lines.append(f"P 256 {blocks * 64 * 8} " + " ".join(f"{x:x}" for x in kw))
        kw = _pad_kw(64, 80, ((1, 8, 7), (19, 61, 6)), blocks * 128 * 8)
        lines.append(f"P 512 {blocks * 128 * 8} " + " ".join(f"{x:x}" for x in kw))
    return "\n".join(lines) + "\n"


def test_rfc4231_digests_are_hashlibs():
    """The independent side of the check agrees with the RFC's printed values."""
    for key, msg, want in RFC4231:
        assert hmac.new(key, msg, "sha256").hexdigest() == want


def test_key_preparation_on_the_host(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("ROCm clang not present")
    exe = tmp_path / "test_sha2_keyprep_host"
    build = subprocess.run(
        [CLANG, *FLAGS, "-I", os.path.join(ROOT, "ilias_net2_amd", "csrc"),
         "-o", str(exe), os.path.join(ROOT, "tests", "cxx", "test_sha2_keyprep_host.cc")],
        cwd=ROOT, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    assert "warning" not in build.stderr, build.stderr[-3000:]
    cases = tmp_path / "cases.txt"
    cases.write_text(_cases_text())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([str(exe), str(cases)], cwd=tmp_path, capture_output=True,
                         text=True, env=env, timeout=300)
    assert run.returncode == 0, (run.stderr + run.stdout)[-4000:]
    # 3 hashes x (4 key lengths x 2 + 4 RFC keys); x 5 messages, or the RFC's one
    assert "test_sha2_keyprep_host: ok (36 keys, 132 messages, 3 refusals, " \
        "6 pad schedules)" in run.stdout
