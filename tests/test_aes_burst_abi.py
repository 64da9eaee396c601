"""CPU: net2_packet_decrypt_burst / net2_packet_encrypt_burst
(include/net2/packet.h) are exported and bound, and their argument checks come
before the device check, as check_burst_args' do.  No kernel is launched
here."""
import ctypes
import errno
import os

import pytest

from ilias_net2_amd import _lib

NAMES = ("net2_packet_decrypt_burst", "net2_packet_encrypt_burst")
vp = ctypes.c_void_p
u32, u64 = ctypes.c_uint32, ctypes.c_uint64


def test_symbols_exported_and_bound():
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.SIGNATURES, name
        fn = getattr(L, name)
        res, args = _lib.SIGNATURES[name]
        assert fn.restype is res and list(fn.argtypes) == args, name
    # the declared signatures are packet.h's: 13 and 12 arguments, n a
    # uint64, hashlen a uint32, everything else a pointer
    assert _lib.SIGNATURES[NAMES[0]] == (ctypes.c_int, [
        vp, vp, vp, vp, vp, u64, vp, vp, vp, vp, vp, vp, vp])
    assert _lib.SIGNATURES[NAMES[1]] == (ctypes.c_int, [
        vp, u32, vp, vp, vp, vp, vp, vp, u64, vp, vp, vp])


def test_cipher_keys_layout():
    """struct net2_burst_cipher_keys as packet.h declares it (LP64)."""
    K = _lib.BurstCipherKeys
    assert [f for f, _ in K._fields_] == ["enc_alg", "enc_key", "enc_keylen",
                                          "alt_enc_key", "alt_enc_keylen"]
    assert (K.enc_alg.offset, K.enc_key.offset, K.enc_keylen.offset,
            K.alt_enc_key.offset, K.alt_enc_keylen.offset) == (0, 8, 16, 24, 32)
    assert ctypes.sizeof(K) == 40


def test_enc_defines_are_in_the_header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "net2", "packet.h")).read()
    assert "#define NET2_ENC_NIL\t\t0" in hdr
    assert "#define NET2_ENC_AES256\t\t1" in hdr
    assert (_lib.ENC_NIL, _lib.ENC_AES256) == (0, 1)


class Args:
    """A well-formed call of each entry point; the tests break one thing at a
    time.  Every pointer is host memory, which no check reads through except
    the key structs."""

    def __init__(self):
        self.buf = ctypes.create_string_buffer(4096)
        self.p = ctypes.addressof(self.buf)
        self.key = ctypes.create_string_buffer(bytes(range(32)), 32)
        self.alt = ctypes.create_string_buffer(bytes(range(32, 64)), 32)
        self.hkey = ctypes.create_string_buffer(b"h" * 64, 64)
        self.ck = _lib.BurstCipherKeys(_lib.ENC_AES256,
                                       ctypes.cast(self.key, vp), 32, None, 0)
        self.rk = _lib.BurstRxKeys(6, ctypes.cast(self.hkey, vp), 64, 1, None, 0,
                                   0, 0, 0)
        self.n = 1
        self.hashlen = 64
        p = self.p
        # base, offsets, lens | seq, flags, iv, result, out, plen
        self.dec = [p, p, p, p, p, p, p, p, p]
        # flags, iv, base, offsets, lens, plen | result, wire_len
        self.enc = [p, p, p, p, p, p, p, p]

    def decrypt(self):
        d = self.dec
        return _lib.lib().net2_packet_decrypt_burst(
            ctypes.byref(self.rk) if self.rk is not None else None,
            ctypes.byref(self.ck) if self.ck is not None else None,
            d[0], d[1], d[2], self.n, d[3], d[4], d[5], d[6], d[7], d[8], None)

    def encrypt(self):
        e = self.enc
        return _lib.lib().net2_packet_encrypt_burst(
            ctypes.byref(self.ck) if self.ck is not None else None, self.hashlen,
            e[0], e[1], e[2], e[3], e[4], e[5], self.n, e[6], e[7], None)

    def install_alt(self):
        self.rk.alt_hash_key = ctypes.cast(self.hkey, vp)
        self.rk.alt_hash_keylen = 64
        self.ck.alt_enc_key = ctypes.cast(self.alt, vp)
        self.ck.alt_enc_keylen = 32


BOTH = ("decrypt", "encrypt")


@pytest.mark.parametrize("call", BOTH)
def test_enc_alg_must_be_aes256(call):
    for alg in (_lib.ENC_NIL, 2, -1):
        a = Args()
        a.ck.enc_alg = alg
        assert getattr(a, call)() == errno.EINVAL, alg


@pytest.mark.parametrize("call", BOTH)
def test_key_must_be_32_bytes(call):
    for keylen in (0, 16, 24, 31, 33, 64):
        a = Args()
        a.ck.enc_keylen = keylen
        assert getattr(a, call)() == errno.EINVAL, keylen
    a = Args()
    a.ck.enc_key = None
    assert getattr(a, call)() == errno.EINVAL
    a = Args()
    a.ck = None
    assert getattr(a, call)() == errno.EINVAL


@pytest.mark.parametrize("call", BOTH)
def test_alternate_key_must_be_32_bytes(call):
    for keylen in (0, 16, 31, 33):
        a = Args()
        a.install_alt()
        a.ck.alt_enc_keylen = keylen
        assert getattr(a, call)() == errno.EINVAL, keylen


def test_hashlen_must_be_a_digest_length():
    for hl in (1, 16, 20, 31, 33, 47, 63, 65, 128, 0xffffffff):
        a = Args()
        a.hashlen = hl
        assert a.encrypt() == errno.EINVAL, hl
    # decrypt takes it from keys->hash_alg, which must be 0 or an HMAC row
    for alg in (1, 2, 3, 7, -1):
        a = Args()
        a.rk.hash_alg = alg
        assert a.decrypt() == errno.EINVAL, alg


def test_alternate_key_mismatches():
    # an alternate hash key installed, but no alternate cipher key
    a = Args()
    a.install_alt()
    a.ck.alt_enc_key = None
    a.ck.alt_enc_keylen = 0
    assert a.decrypt() == errno.EINVAL
    # an alternate key without a keyed hash: there is no selection to follow
    a = Args()
    a.install_alt()
    a.rk.hash_alg = 0
    assert a.decrypt() == errno.EINVAL
    # the selection needs the sequence numbers
    a = Args()
    a.install_alt()
    a.dec[3] = None
    assert a.decrypt() == errno.EINVAL
    a = Args()
    a.rk = None
    assert a.decrypt() == errno.EINVAL


def test_null_pointers_with_n_positive():
    for k in range(9):
        if k == 3:
            continue                # d_seq: only with an alternate key (above)
        a = Args()
        a.dec[k] = None
        assert a.decrypt() == errno.EINVAL, k
    for k in range(8):
        a = Args()
        a.enc[k] = None
        assert a.encrypt() == errno.EINVAL, k


@pytest.mark.parametrize("call", BOTH)
def test_n_zero_is_zero_and_needs_no_pointers(call):
    a = Args()
    a.n = 0
    a.dec = [None] * 9
    a.enc = [None] * 8
    assert getattr(a, call)() == 0
    # ... but the key checks still come first
    a.ck.enc_keylen = 31
    assert getattr(a, call)() == errno.EINVAL


@pytest.mark.skipif(_lib.device_count() > 0, reason="a GPU is present")
@pytest.mark.parametrize("call", BOTH)
def test_well_formed_call_reaches_the_device_check(call):
    """ENODEV without a device: every argument check passed."""
    for hashlen, alg in ((0, 0), (32, 4), (48, 5), (64, 6)):
        a = Args()
        a.hashlen = hashlen
        a.rk.hash_alg = alg
        assert getattr(a, call)() == errno.ENODEV
    a = Args()
    a.install_alt()
    assert getattr(a, call)() == errno.ENODEV
