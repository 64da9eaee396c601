"""CPU: the host bursts over many connections (include/net2/packet.h:
net2_packet_{decode,encode}_burst_mc_host) are exported, bound with the
header's signatures and declared, and every argument check comes before the
device check.  No kernel is launched here: a table cannot be made without a
device, so the calls are given stand-ins that hold a device number no thread
has -- every check under test returns before anything else of them is read."""
import ctypes
import errno
import os

import pytest

from ilias_net2_amd import _lib

NAMES = ("net2_packet_decode_burst_mc_host", "net2_packet_encode_burst_mc_host")
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
    # tab, ctab, conn, ivlen, base, offsets, lens, n, result, iv, seq, flags,
    # out, plen, table_stream
    assert S[NAMES[0]] == (ctypes.c_int, [
        vp, vp, vp, u32, vp, vp, vp, u64, vp, vp, vp, vp, vp, vp, vp])
    # tab, ctab, conn, seq, flags, base, offsets, lens, plen, n, result,
    # wire_len, table_stream
    assert S[NAMES[1]] == (ctypes.c_int, [
        vp, vp, vp, vp, vp, vp, vp, vp, vp, u64, vp, vp, vp])


def test_declared_in_the_header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "net2", "packet.h")).read()
    for name in NAMES:
        assert "int " + name + "(" in hdr, name


class KeyTab(ctypes.Structure):
    """The head of struct net2_burst_keytab (net2_dgram.cpp).  Device -2 is no
    thread's current device."""
    _fields_ = [("device", ctypes.c_int), ("hash_alg", ctypes.c_int),
                ("slots", u32), ("ents", vp)]


class CipherTab(ctypes.Structure):
    """The head of struct net2_burst_ciphertab (net2_dgram.cpp)."""
    _fields_ = [("device", ctypes.c_int), ("slots", u32), ("ents", vp)]


class Args:
    """A well-formed call of each entry point; the tests break one thing at a
    time.  Every array is host memory that no check reads through."""

    def __init__(self, cipher=True, broken=False):
        self.buf = ctypes.create_string_buffer(4096)
        p = ctypes.addressof(self.buf)
        # broken: the caller breaks an argument.  Where there is a device the
        # tables are then on it, so the EINVAL is the argument's and not the
        # device check's.
        dev = 0 if broken and HAVE_GPU else -2
        self.tab = KeyTab(dev, 6, 4, None)
        self.ctab = CipherTab(dev, 4, None) if cipher else None
        self.n = 1
        self.ivlen = 16
        # RX: conn, base, offsets, lens, result | iv, seq, flags | out, plen
        self.rx = [p] * 10
        # TX: conn, seq, flags, base, offsets, lens | plen | result | wire_len
        self.tx = [p] * 9

    def _tab(self):
        return ctypes.byref(self.tab) if self.tab is not None else None

    def _ctab(self):
        return ctypes.byref(self.ctab) if self.ctab is not None else None

    def decode(self):
        r = self.rx
        return _lib.lib().net2_packet_decode_burst_mc_host(
            self._tab(), self._ctab(), r[0], self.ivlen, r[1], r[2], r[3], self.n,
            r[4], r[5], r[6], r[7], r[8], r[9], None)

    def encode(self):
        t = self.tx
        return _lib.lib().net2_packet_encode_burst_mc_host(
            self._tab(), self._ctab(), t[0], t[1], t[2], t[3], t[4], t[5], t[6],
            self.n, t[7], t[8], None)


# what a well-formed call returns once every argument check has passed: the
# device check's ENODEV without a device, else EINVAL for the stand-in's
# device, which is not the calling thread's
PASSED = errno.EINVAL if HAVE_GPU else errno.ENODEV
CALLS = ("decode", "encode")


@pytest.mark.parametrize("cipher", [False, True])
@pytest.mark.parametrize("call", CALLS)
def test_well_formed_call_reaches_the_device_check(call, cipher):
    for alg in (4, 5, 6):
        a = Args(cipher)
        a.tab.hash_alg = alg
        assert getattr(a, call)() == PASSED, alg
    # what is optional: iv; RX seq and flags together
    a = Args(cipher)
    a.rx[5] = None
    assert a.decode() == PASSED
    a.rx[6] = a.rx[7] = None
    assert a.decode() == PASSED


@pytest.mark.parametrize("call", CALLS)
def test_hash_step_only_ignores_the_cipher_arrays(call):
    a = Args(cipher=False)
    a.rx[8] = a.rx[9] = None            # out, plen
    a.tx[6] = a.tx[8] = None            # plen, wire_len
    for ivlen in (0, 16, 24, 64):       # any IV length the hash burst takes
        a.ivlen = ivlen
        assert getattr(a, call)() == PASSED, ivlen


@pytest.mark.parametrize("cipher", [False, True])
@pytest.mark.parametrize("call", CALLS)
def test_null_table_is_einval(call, cipher):
    a = Args(cipher, broken=True)
    a.tab = None
    assert getattr(a, call)() == errno.EINVAL
    a.n = 0                              # ... before the empty burst's 0
    assert getattr(a, call)() == errno.EINVAL


@pytest.mark.parametrize("cipher", [False, True])
def test_array_checks(cipher):
    # check_burst_arrays: base, offsets, lens, result; then conn
    for k in (1, 2, 3, 4, 0):
        a = Args(cipher, broken=True)
        a.rx[k] = None
        assert a.decode() == errno.EINVAL, k
    for k in (3, 4, 5, 7, 0):
        a = Args(cipher, broken=True)
        a.tx[k] = None
        assert a.encode() == errno.EINVAL, k
    for call in CALLS:
        a = Args(cipher, broken=True)
        a.n = 1 << 32
        assert getattr(a, call)() == errno.EINVAL
    a = Args(cipher, broken=True)
    a.ivlen = 65
    assert a.decode() == errno.EINVAL
    a.n = 0                              # the IV length is checked first
    assert a.decode() == errno.EINVAL


@pytest.mark.parametrize("cipher", [False, True])
def test_header_arrays(cipher):
    # RX: both or neither
    for k in (6, 7):
        a = Args(cipher, broken=True)
        a.rx[k] = None
        assert a.decode() == errno.EINVAL, k
    # TX: both required
    for ks in ((1,), (2,), (1, 2)):
        a = Args(cipher, broken=True)
        for k in ks:
            a.tx[k] = None
        assert a.encode() == errno.EINVAL, ks


def test_cipher_checks():
    for ivlen in (0, 8, 15, 17, 32, 64):
        a = Args(broken=True)
        a.ivlen = ivlen
        assert a.decode() == errno.EINVAL, ivlen
    for k in (8, 9):                     # out, plen
        a = Args(broken=True)
        a.rx[k] = None
        assert a.decode() == errno.EINVAL, k
    for k in (6, 8):                     # plen, wire_len
        a = Args(broken=True)
        a.tx[k] = None
        assert a.encode() == errno.EINVAL, k
    for call in CALLS:                   # the two tables on one device
        a = Args(broken=True)
        a.ctab.device = -3
        assert getattr(a, call)() == errno.EINVAL


@pytest.mark.parametrize("cipher", [False, True])
@pytest.mark.parametrize("call", CALLS)
def test_n_zero_is_zero_and_needs_no_arrays(call, cipher):
    a = Args(cipher)
    a.n = 0
    a.rx = [None] * 10
    a.tx = [None] * 9
    assert getattr(a, call)() == 0
    assert bytes(a.buf) == bytes(4096)
