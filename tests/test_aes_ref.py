"""CPU: the EVP helper the burst cipher tests take their expected values from
(tests/aes_ref.py) against the published vector, and EVP's accept / reject
behaviour that net2_packet_decrypt_burst restates on the device."""
import json
import os

import pytest

import aes_ref

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def kat():
    with open(os.path.join(HERE, "golden", "aes256_cbc_kat.json")) as f:
        k = json.load(f)
    return {n: bytes.fromhex(k[n]) for n in ("key", "iv", "plaintext",
                                             "ciphertext_padded")} | {
        "blocks": [bytes.fromhex(b) for b in k["ciphertext_blocks"]]}


def test_helper_reproduces_the_fixture(kat):
    ct = aes_ref.encrypt(kat["key"], kat["iv"], kat["plaintext"])
    assert ct == kat["ciphertext_padded"] and len(ct) == 80
    assert aes_ref.decrypt(kat["key"], kat["iv"], ct) == kat["plaintext"]
    # without padding: exactly the four published blocks
    assert aes_ref.encrypt(kat["key"], kat["iv"], kat["plaintext"],
                           pad=False) == ct[:64]


def test_fixture_starts_with_the_published_blocks(kat):
    assert kat["ciphertext_padded"][:64] == b"".join(kat["blocks"])
    assert kat["blocks"][0].hex().startswith("f58c4c04")
    assert kat["blocks"][0].hex().endswith("fbd6")
    assert kat["blocks"][1].hex().startswith("9cfc4e96")
    assert kat["blocks"][1].hex().endswith("2c7d")
    assert kat["blocks"][2].hex().startswith("39f23369")
    assert kat["blocks"][2].hex().endswith("1461")
    assert kat["blocks"][3].hex().startswith("b2eb05e2")
    assert kat["blocks"][3].hex().endswith("9d1b")


def _with_tail(kat, tail: bytes):
    """A two-block ciphertext whose plaintext ends in ``tail``."""
    plain = (bytes(range(32)) + tail)[-32:]
    return aes_ref.encrypt(kat["key"], kat["iv"], plain, pad=False), plain


def test_evp_rejects(kat):
    key, iv, ct = kat["key"], kat["iv"], kat["ciphertext_padded"]
    assert aes_ref.decrypt(key, iv, b"") is None          # empty
    assert aes_ref.decrypt(key, iv, ct[:15]) is None      # ragged
    assert aes_ref.decrypt(key, iv, ct[:17]) is None
    assert aes_ref.decrypt(key, iv, ct[:64]) is None      # no padding block
    for tail in (b"\x00", b"\x11", b"\x03\x02\x03"):
        c, _ = _with_tail(kat, tail)
        assert aes_ref.decrypt(key, iv, c) is None, tail


def test_evp_accepts(kat):
    key, iv = kat["key"], kat["iv"]
    for tail, plen in ((b"\x01", 31), (b"\x02\x02", 30), (b"\x10" * 16, 16)):
        c, plain = _with_tail(kat, tail)
        assert aes_ref.decrypt(key, iv, c) == plain[:plen], tail
    assert aes_ref.encrypt(key, iv, b"") is not None
    assert len(aes_ref.encrypt(key, iv, b"")) == 16       # EVP always pads
    assert aes_ref.decrypt(key, iv, aes_ref.encrypt(key, iv, b"")) == b""
