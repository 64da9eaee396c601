"""CPU: tests/tab_ref.py, the plain-Python restatement of the table entries the
table-update GPU tests compare fingerprints with, against hashlib, hmac and
the FIPS 197 vectors -- so that yardstick is pinned without a GPU."""
import hashlib
import hmac
import struct

import pytest

import tab_ref

ROWS = {4: ("sha256", False), 5: ("sha384", True), 6: ("sha512", True)}


def _digest(row, msg):
    """SHA-2 of msg through tab_ref.compress."""
    iv, wide = tab_ref.row_iv(row)
    blk = 128 if wide else 64
    m = msg + b"\x80" + bytes((blk - 1 - (len(msg) + (16 if wide else 8))) % blk)
    m += (8 * len(msg)).to_bytes(16 if wide else 8, "big")
    st = iv
    for i in range(0, len(m), blk):
        st = tab_ref.compress(st, m[i:i + blk], wide)
    out = b"".join(x.to_bytes(8 if wide else 4, "big") for x in st)
    return out[:{4: 32, 5: 48, 6: 64}[row]]


@pytest.mark.parametrize("row", [4, 5, 6])
def test_compressions_against_hashlib(row):
    for n in (0, 1, 55, 56, 63, 64, 111, 112, 127, 128, 300):
        msg = bytes((7 * i + n) & 0xff for i in range(n))
        assert _digest(row, msg) == hashlib.new(ROWS[row][0], msg).digest(), n


@pytest.mark.parametrize("row", [4, 5, 6])
def test_midstates_finish_to_hmac(row):
    """An entry's ipad / opad midstates, carried on over a message, give
    HMAC (RFC 2104)."""
    name, wide = ROWS[row]
    blk, hl = (128 if wide else 64), {4: 32, 5: 48, 6: 64}[row]
    key = bytes(range(1, hl + 1))
    msg = b"the quick brown fox" * 7

    def state(b):
        w = struct.unpack("<16I", b)
        return ([w[2 * i] << 32 | w[2 * i + 1] for i in range(8)] if wide
                else list(w[:8]))

    def finish(st, data):
        total = blk + len(data)
        m = data + b"\x80" + bytes((blk - 1 - (len(data) + (16 if wide else 8))) % blk)
        m += (8 * total).to_bytes(16 if wide else 8, "big")
        for i in range(0, len(m), blk):
            st = tab_ref.compress(st, m[i:i + blk], wide)
        return b"".join(x.to_bytes(8 if wide else 4, "big") for x in st)[:hl]

    ipad, opad = tab_ref.midstates(row, key)
    if not wide:
        assert ipad[32:] == bytes(32) and opad[32:] == bytes(32)
    got = finish(state(opad), finish(state(ipad), msg))
    assert got == hmac.new(key, msg, name).digest()


def test_aes_key_expansion_fips197_a3():
    key = bytes.fromhex("603deb1015ca71be2b73aef0857d7781"
                        "1f352c073b6108d72d9810a30914dff4")
    w = tab_ref.enc_schedule(key)
    assert w[:8] == list(struct.unpack(">8I", key))
    assert (w[8], w[9], w[12], w[59]) == (0x9ba35411, 0x8e6925af, 0xa8b09c1a,
                                          0x706c631e)
    assert tab_ref.SBOX[0x00] == 0x63 and tab_ref.SBOX[0x53] == 0xed


def test_decryption_schedule_inverts_the_cipher():
    """One block through the equivalent inverse cipher (FIPS 197 5.3.5) under
    dec_schedule gives the C.3 plaintext back."""
    key = bytes(range(32))
    ct = bytes.fromhex("8ea2b7ca516745bfeafc49904b496089")
    inv = [0] * 256
    for x, s in enumerate(tab_ref.SBOX):
        inv[s] = x
    dk = tab_ref.dec_schedule(key)
    st = [a ^ b for a, b in zip(struct.unpack(">4I", ct), dk[:4])]
    for r in range(1, 15):
        b = [[(st[c] >> s) & 0xff for s in (24, 16, 8, 0)] for c in range(4)]
        # InvShiftRows then InvSubBytes: row i of column c comes from column c - i
        cols = [sum(inv[b[(c - i) % 4][i]] << (24 - 8 * i) for i in range(4))
                for c in range(4)]
        if r < 14:
            cols = [tab_ref._inv_mix(x) for x in cols]
        st = [x ^ k for x, k in zip(cols, dk[4 * r:4 * r + 4])]
    assert struct.pack(">4I", *st).hex() == "00112233445566778899aabbccddeeff"


def test_entry_layout_and_meta_rules():
    e = tab_ref.KeyEntry(6)
    assert len(e.bytes()) == tab_ref.KEY_ENT_BYTES and e.bytes() == bytes(400)
    e.set_rx(b"k" * 64, enc_set=True, alt_cutoff=9, rx_start=5)   # no alternate key
    assert e.meta == [0x11, 0, 0, 0] and e.rx[128:] == bytes(128)
    e.set_tx(b"t" * 64)
    assert e.meta[0] == 0x13
    e.set_rx(b"k" * 64, alt_key=b"a" * 64, alt_no_cutoff=True, alt_cutoff=9, rx_start=5)
    assert e.meta == [0x0f, 9, 5, 0]
    before = e.bytes()
    e.clear()
    assert e.bytes()[:4] == bytes(4) and e.bytes()[4:] == before[4:]
    c = tab_ref.CipherEntry()
    assert len(c.bytes()) == tab_ref.CIPHER_ENT_BYTES
    c.set_tx(bytes(32))
    c.set_rx(bytes(32), alt_key=bytes(range(32)), alt_cutoff=7, rx_start=3)
    assert c.meta == [7, 7, 3, 0]
    c.clear()
    assert c.bytes() == bytes(736)
