"""CPU: the device cipher-key table and the multi-connection cipher calls
(include/net2/packet.h: net2_burst_ciphertab_*, net2_packet_{decrypt,encrypt}_
burst_mc) are exported and bound with the header's signatures, and their
argument checks come before the device check.  No kernel is launched here: a
table cannot be made without a device, so the calls that take one are given a
stand-in that holds a device number no thread has and a slot count -- every
check under test returns before anything else of it is read."""
import ctypes
import errno
import os

import pytest

from ilias_net2_amd import _lib

NAMES = ("net2_burst_ciphertab_create", "net2_burst_ciphertab_destroy",
         "net2_burst_ciphertab_set_rx", "net2_burst_ciphertab_set_tx",
         "net2_burst_ciphertab_clear", "net2_packet_decrypt_burst_mc",
         "net2_packet_encrypt_burst_mc")
vp = ctypes.c_void_p
u32, u64 = ctypes.c_uint32, ctypes.c_uint64
HAVE_GPU = _lib.device_count() > 0


def test_symbols_exported_and_bound():
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.SIGNATURES, name
        fn = getattr(L, name)
        res, args = _lib.SIGNATURES[name]
        assert fn.restype is res and list(fn.argtypes) == args, name
    S = _lib.SIGNATURES
    assert S[NAMES[0]] == (ctypes.c_int, [ctypes.c_int, u32, ctypes.POINTER(vp)])
    assert S[NAMES[1]] == (None, [vp])
    assert S[NAMES[2]] == (ctypes.c_int, [vp, u32, vp, vp, vp])
    assert S[NAMES[3]] == (ctypes.c_int, [vp, u32, vp, vp])
    assert S[NAMES[4]] == (ctypes.c_int, [vp, u32, vp])
    # tab, conn, hashlen, then the single-connection call's arrays
    assert S[NAMES[5]] == (ctypes.c_int, [
        vp, vp, u32, vp, vp, vp, u64, vp, vp, vp, vp, vp, vp, vp])
    assert S[NAMES[6]] == (ctypes.c_int, [
        vp, vp, u32, vp, vp, vp, vp, vp, vp, u64, vp, vp, vp])


def test_declared_in_the_header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "net2", "packet.h")).read()
    assert "struct net2_burst_ciphertab;" in hdr
    for name in NAMES:
        assert name + "(" in hdr, name
    from ilias_net2_amd import cipher_burst
    assert cipher_burst.NOCONN == 5


def test_create_argument_errors_precede_the_device_check():
    L = _lib.lib()
    tab = vp(0x1234)
    for alg, slots in ((_lib.ENC_NIL, 4), (2, 4), (-1, 4), (_lib.ENC_AES256, 0)):
        assert L.net2_burst_ciphertab_create(alg, slots, ctypes.byref(tab)) == errno.EINVAL
        assert not tab.value          # and no table is handed out
        tab.value = 0x1234
    assert L.net2_burst_ciphertab_create(_lib.ENC_AES256, 4, None) == errno.EINVAL
    # a well-formed request reaches the device check (or a device)
    rc = L.net2_burst_ciphertab_create(_lib.ENC_AES256, 4, ctypes.byref(tab))
    if not HAVE_GPU:
        assert rc == errno.ENODEV and not tab.value
    else:
        assert rc == 0 and tab.value
        L.net2_burst_ciphertab_destroy(tab)


class StandIn(ctypes.Structure):
    """The head of struct net2_burst_ciphertab (net2_dgram.cpp): the table's
    device and its slot count.  Device -2 is no thread's current device."""
    _fields_ = [("device", ctypes.c_int), ("slots", u32), ("ents", vp)]


class Args:
    """A well-formed call of each entry point; the tests break one thing at a
    time.  Every pointer is host memory, which no check reads through except
    the key structs and the stand-in table."""

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
        self.tab = StandIn(-2, 4, None)
        self.slot = 3
        self.n = 1
        self.hashlen = 64
        p = self.p
        # conn, base, offsets, lens | seq, flags, iv, result, out, plen
        self.dec = [p] * 10
        # conn, flags, iv, base, offsets, lens, plen | result, wire_len
        self.enc = [p] * 9

    def _tab(self):
        return ctypes.byref(self.tab) if self.tab is not None else None

    def _ck(self):
        return ctypes.byref(self.ck) if self.ck is not None else None

    def set_rx(self):
        return _lib.lib().net2_burst_ciphertab_set_rx(
            self._tab(), self.slot,
            ctypes.byref(self.rk) if self.rk is not None else None, self._ck(), None)

    def set_tx(self):
        return _lib.lib().net2_burst_ciphertab_set_tx(self._tab(), self.slot,
                                                      self._ck(), None)

    def clear(self):
        return _lib.lib().net2_burst_ciphertab_clear(self._tab(), self.slot, None)

    def decrypt(self):
        d = self.dec
        return _lib.lib().net2_packet_decrypt_burst_mc(
            self._tab(), d[0], self.hashlen, d[1], d[2], d[3], self.n, d[4], d[5],
            d[6], d[7], d[8], d[9], None)

    def encrypt(self):
        e = self.enc
        return _lib.lib().net2_packet_encrypt_burst_mc(
            self._tab(), e[0], self.hashlen, e[1], e[2], e[3], e[4], e[5], e[6],
            self.n, e[7], e[8], None)

    def install_alt(self):
        self.rk.alt_hash_key = ctypes.cast(self.hkey, vp)
        self.rk.alt_hash_keylen = 64
        self.ck.alt_enc_key = ctypes.cast(self.alt, vp)
        self.ck.alt_enc_keylen = 32


# what a well-formed call returns once every argument check has passed: the
# device check's ENODEV without a device, else EINVAL for the stand-in's
# device, which is not the calling thread's
PASSED = errno.EINVAL if HAVE_GPU else errno.ENODEV
ALL = ("set_rx", "set_tx", "clear", "decrypt", "encrypt")
SETS = ("set_rx", "set_tx")


@pytest.mark.parametrize("call", ALL)
def test_null_table_is_einval(call):
    a = Args()
    a.tab = None
    assert getattr(a, call)() == errno.EINVAL
    a.n = 0
    assert getattr(a, call)() == errno.EINVAL
    _lib.lib().net2_burst_ciphertab_destroy(None)         # a no-op


@pytest.mark.parametrize("call", ("set_rx", "set_tx", "clear"))
def test_slot_must_be_in_range(call):
    for slot in (4, 5, 0xffffffff):
        a = Args()
        a.slot = slot
        assert getattr(a, call)() == errno.EINVAL, slot


@pytest.mark.parametrize("call", SETS)
def test_enc_alg_must_be_aes256(call):
    for alg in (_lib.ENC_NIL, 2, -1):
        a = Args()
        a.ck.enc_alg = alg
        assert getattr(a, call)() == errno.EINVAL, alg


@pytest.mark.parametrize("call", SETS)
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


@pytest.mark.parametrize("call", SETS)
def test_alternate_key_must_be_32_bytes(call):
    for keylen in (0, 16, 31, 33):
        a = Args()
        a.install_alt()
        a.ck.alt_enc_keylen = keylen
        assert getattr(a, call)() == errno.EINVAL, keylen


def test_set_rx_key_state_checks():
    # keys->hash_alg is 0 or an HMAC row
    for alg in (1, 2, 3, 7, -1):
        a = Args()
        a.rk.hash_alg = alg
        assert a.set_rx() == errno.EINVAL, alg
    # an alternate hash key installed, but no alternate cipher key
    a = Args()
    a.install_alt()
    a.ck.alt_enc_key = None
    a.ck.alt_enc_keylen = 0
    assert a.set_rx() == errno.EINVAL
    # an alternate key without a keyed hash: there is no selection to follow
    a = Args()
    a.install_alt()
    a.rk.hash_alg = 0
    assert a.set_rx() == errno.EINVAL
    a = Args()
    a.rk = None
    assert a.set_rx() == errno.EINVAL


@pytest.mark.parametrize("call", ("decrypt", "encrypt"))
def test_hashlen_must_be_a_digest_length(call):
    for hl in (1, 16, 20, 31, 33, 47, 63, 65, 128, 0xffffffff):
        a = Args()
        a.hashlen = hl
        assert getattr(a, call)() == errno.EINVAL, hl


def test_null_pointers_with_n_positive():
    # d_seq (4) included: any slot may have an alternate key
    for k in range(10):
        a = Args()
        a.dec[k] = None
        a.tab.device = 0 if HAVE_GPU else -2    # a passing device check: EINVAL is the pointer's
        assert a.decrypt() == errno.EINVAL, k
    for k in range(9):
        a = Args()
        a.enc[k] = None
        a.tab.device = 0 if HAVE_GPU else -2
        assert a.encrypt() == errno.EINVAL, k


def test_n_past_32_bits_is_einval():
    for call in ("decrypt", "encrypt"):
        a = Args()
        a.n = 1 << 32
        a.tab.device = 0 if HAVE_GPU else -2
        assert getattr(a, call)() == errno.EINVAL


@pytest.mark.parametrize("call", ("decrypt", "encrypt"))
def test_n_zero_is_zero_and_needs_no_pointers(call):
    a = Args()
    a.n = 0
    a.dec = [None] * 10
    a.enc = [None] * 9
    assert getattr(a, call)() == 0
    # ... but the table and hashlen checks still come first
    a.hashlen = 31
    assert getattr(a, call)() == errno.EINVAL
    a.hashlen = 64
    a.tab = None
    assert getattr(a, call)() == errno.EINVAL


@pytest.mark.parametrize("call", ALL)
def test_well_formed_call_reaches_the_device_check(call):
    """Every argument check passed: what is left is the device check."""
    for hashlen, alg in ((0, 0), (32, 4), (48, 5), (64, 6)):
        a = Args()
        a.hashlen = hashlen
        a.rk.hash_alg = alg
        assert getattr(a, call)() == PASSED, (hashlen, alg)
    a = Args()
    a.install_alt()
    assert getattr(a, call)() == PASSED
    a = Args()
    a.slot = 0
    assert getattr(a, call)() == PASSED
