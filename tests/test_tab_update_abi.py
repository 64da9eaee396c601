"""CPU: the bulk table updates and the fingerprints (include/net2/packet.h:
net2_burst_keytab_update, net2_burst_ciphertab_update, net2_burst_tab_limits,
net2_burst_tab_stats, net2_burst_*_fingerprint) are exported, bound and
declared, and every argument check comes before the device check -- whichever
op of the list is the bad one.  No kernel is launched here: a table cannot be
made without a device, so the calls are given a stand-in that holds a device
number no thread has, the row and a slot count; every check under test returns
before anything else of it is read."""
import ctypes
import errno
import os

import pytest

from ilias_net2_amd import _lib

NAMES = ("net2_burst_keytab_update", "net2_burst_ciphertab_update",
         "net2_burst_tab_limits", "net2_burst_tab_stats",
         "net2_burst_keytab_fingerprint", "net2_burst_ciphertab_fingerprint")
vp = ctypes.c_void_p
u32, u64 = ctypes.c_uint32, ctypes.c_uint64
HAVE_GPU = _lib.device_count() > 0
# what a well-formed call returns once every argument check has passed: the
# device check's ENODEV without a device, else EINVAL for the stand-in's
# device, which is not the calling thread's
PASSED = errno.EINVAL if HAVE_GPU else errno.ENODEV
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 9                       # ops per list; the bad one first, in the middle, last
PLACES = (0, N // 2, N - 1)
SLOTS = 4


def test_symbols_exported_and_bound():
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.SIGNATURES, name
        fn = getattr(L, name)
        res, args = _lib.SIGNATURES[name]
        assert fn.restype is res and list(fn.argtypes) == args, name
    S = _lib.SIGNATURES
    assert S[NAMES[0]] == (ctypes.c_int, [vp, vp, ctypes.c_size_t, vp])
    assert S[NAMES[1]] == (ctypes.c_int, [vp, vp, ctypes.c_size_t, vp])
    assert S[NAMES[2]] == (ctypes.c_int, [ctypes.c_int64])
    assert S[NAMES[3]] == (ctypes.c_int, [ctypes.POINTER(u64), ctypes.POINTER(u64)])
    assert S[NAMES[4]] == (ctypes.c_int, [vp, u32, u32, vp, vp])
    assert S[NAMES[5]] == (ctypes.c_int, [vp, u32, u32, vp, vp])


def test_declared_in_the_header():
    hdr = open(os.path.join(ROOT, "include", "net2", "packet.h")).read()
    for name in NAMES:
        assert name + "(" in hdr, name
    for text in ("struct net2_burst_keytab_op {", "struct net2_burst_ciphertab_op {",
                 "#define NET2_BURST_TAB_CLEAR 0u", "#define NET2_BURST_TAB_RX    1u",
                 "#define NET2_BURST_TAB_TX    2u"):
        assert text in hdr, text
    assert (_lib.TAB_CLEAR, _lib.TAB_RX, _lib.TAB_TX) == (0, 1, 2)


def test_op_structs_have_the_header_layout(tmp_path):
    """The binding's structs against the header's, as the C compiler lays
    them out."""
    import shutil
    import subprocess
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no C compiler")
    K, C = _lib.BurstKeytabOp, _lib.BurstCiphertabOp
    fields = [("keytab", K, f) for f, _ in K._fields_] + \
             [("ciphertab", C, f) for f, _ in C._fields_]
    src = tmp_path / "layout.c"
    src.write_text(
        "#include <stddef.h>\n#include <stdio.h>\n#include <net2/packet.h>\n"
        "int main(void) {\n" +
        "".join(f'printf("%zu\\n", offsetof(struct net2_burst_{t}_op, {f}));\n'
                for t, _, f in fields) +
        'printf("%zu %zu\\n", sizeof(struct net2_burst_keytab_op), '
        "sizeof(struct net2_burst_ciphertab_op));\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)],
                   check=True, capture_output=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True,
                         text=True).stdout.split()
    assert [int(x) for x in out[:len(fields)]] == [
        getattr(cls, f).offset for _, cls, f in fields]
    assert [int(x) for x in out[len(fields):]] == [ctypes.sizeof(K), ctypes.sizeof(C)]


class KeyStandIn(ctypes.Structure):
    """The head of struct net2_burst_keytab (net2_host.h).  Device -2 is no
    thread's current device."""
    _fields_ = [("device", ctypes.c_int), ("hash_alg", ctypes.c_int),
                ("slots", u32), ("ents", vp), ("stage", vp)]


class CipherStandIn(ctypes.Structure):
    """The head of struct net2_burst_ciphertab (net2_host.h)."""
    _fields_ = [("device", ctypes.c_int), ("slots", u32), ("ents", vp),
                ("stage", vp)]


class KeyList:
    """A well-formed list of N key-table ops of every kind for a row's table;
    the tests break one op at a time."""

    def __init__(self, row=6):
        self.row, self.keylen = row, {4: 32, 5: 48, 6: 64}[row]
        self.key = ctypes.create_string_buffer(bytes(range(64)), 64)
        self.alt = ctypes.create_string_buffer(bytes(range(64, 128)), 64)
        self.tab = KeyStandIn(-2, row, SLOTS, None, None)
        self.ops = (_lib.BurstKeytabOp * N)()
        self.n = N
        for i, o in enumerate(self.ops):
            o.slot, o.op = i % SLOTS, (_lib.TAB_RX, _lib.TAB_TX, _lib.TAB_CLEAR)[i % 3]
            o.rx = _lib.BurstRxKeys(row, ctypes.cast(self.key, vp), self.keylen,
                                    i & 1, None, 0, 0, 0, 0)
            if i % 2:
                o.rx.alt_hash_key = ctypes.cast(self.alt, vp)
                o.rx.alt_hash_keylen = self.keylen
            o.tx_key = ctypes.cast(self.key, vp)
            o.tx_keylen = self.keylen

    def make(self, i, kind):
        self.ops[i].op = kind
        return self.ops[i]

    def call(self, stream=None):
        return _lib.lib().net2_burst_keytab_update(
            ctypes.byref(self.tab) if self.tab is not None else None,
            self.ops, self.n, stream)


class CipherList:
    """The same for the cipher table."""

    def __init__(self):
        self.key = ctypes.create_string_buffer(bytes(range(32)), 32)
        self.alt = ctypes.create_string_buffer(bytes(range(32, 64)), 32)
        self.tab = CipherStandIn(-2, SLOTS, None, None)
        self.ops = (_lib.BurstCiphertabOp * N)()
        self.n = N
        for i, o in enumerate(self.ops):
            o.slot, o.op = i % SLOTS, (_lib.TAB_RX, _lib.TAB_TX, _lib.TAB_CLEAR)[i % 3]
            o.ck = _lib.BurstCipherKeys(_lib.ENC_AES256, ctypes.cast(self.key, vp),
                                        32, None, 0)
            o.rx = _lib.BurstRxKeys(6, None, 0, 1, None, 0, 0, 0, 0)
            if i % 2:
                o.rx.alt_hash_key = ctypes.cast(self.alt, vp)
                o.ck.alt_enc_key = ctypes.cast(self.alt, vp)
                o.ck.alt_enc_keylen = 32

    make = KeyList.make

    def call(self, stream=None):
        return _lib.lib().net2_burst_ciphertab_update(
            ctypes.byref(self.tab) if self.tab is not None else None,
            self.ops, self.n, stream)


LISTS = (KeyList, CipherList)


def counters():
    a, b = u64(0), u64(0)
    assert _lib.lib().net2_burst_tab_stats(ctypes.byref(a), ctypes.byref(b)) == 0
    return a.value, b.value


@pytest.mark.parametrize("cls", LISTS)
def test_well_formed_list_reaches_the_device_check(cls):
    before = counters()
    assert cls().call() == PASSED
    if cls is KeyList:
        for row in (4, 5):
            assert KeyList(row).call() == PASSED
    assert counters() == before


@pytest.mark.parametrize("cls", LISTS)
def test_null_table_null_ops_and_n(cls):
    a = cls()
    a.tab = None
    assert a.call() == errno.EINVAL
    a.n = 0
    assert a.call() == errno.EINVAL          # the table check comes first
    a = cls()
    a.ops = None
    assert a.call() == errno.EINVAL
    a.n = 0
    assert a.call() == 0                     # n == 0 needs no ops ...
    assert cls().call() == PASSED
    a = cls()
    a.n = 0
    assert a.call() == 0                     # ... and reaches no device check
    a = cls()
    a.n = (1 << 32)                          # (refused before any op is read)
    assert a.call() == errno.EINVAL


@pytest.mark.parametrize("at", PLACES)
@pytest.mark.parametrize("cls", LISTS)
def test_unknown_op_and_slot_out_of_range(cls, at):
    for kind in (3, 4, 0xffffffff):
        a = cls()
        a.make(at, kind)
        assert a.call() == errno.EINVAL, kind
    for kind in (_lib.TAB_CLEAR, _lib.TAB_RX, _lib.TAB_TX):
        for slot in (SLOTS, SLOTS + 1, 0xffffffff):
            a = cls()
            a.make(at, kind).slot = slot
            assert a.call() == errno.EINVAL, (kind, slot)


@pytest.mark.parametrize("at", PLACES)
def test_key_table_rx_checks(at):
    """net2_burst_keytab_set_rx's, op by op."""
    for row in (4, 5, 6):
        for bad in (0, 16, (row - 2) * 16 - 1, (row - 2) * 16 + 1, 128):
            a = KeyList(row)
            a.make(at, _lib.TAB_RX).rx.hash_keylen = bad
            assert a.call() == errno.EINVAL, (row, bad)
        a = KeyList(row)
        a.make(at, _lib.TAB_RX).rx.hash_alg = 4 + (row - 3) % 3    # another row
        assert a.call() == errno.EINVAL
    a = KeyList()
    a.make(at, _lib.TAB_RX).rx.hash_key = None
    assert a.call() == errno.EINVAL
    a = KeyList()
    o = a.make(at, _lib.TAB_RX)
    o.rx.alt_hash_key = ctypes.cast(a.alt, vp)
    o.rx.alt_hash_keylen = 32                   # not the key's length
    assert a.call() == errno.EINVAL
    # the same fields in an op of another kind are not looked at
    a = KeyList()
    o = a.make(at, _lib.TAB_CLEAR)
    o.rx.hash_key, o.rx.hash_keylen, o.tx_key = None, 1, None
    assert a.call() == PASSED
    a = KeyList()
    o = a.make(at, _lib.TAB_TX)
    o.rx.hash_key, o.rx.hash_keylen, o.rx.hash_alg = None, 1, 0
    assert a.call() == PASSED


@pytest.mark.parametrize("at", PLACES)
def test_key_table_tx_checks(at):
    """net2_burst_keytab_set_tx's, op by op."""
    for row in (4, 5, 6):
        for bad in (0, 16, (row - 2) * 16 - 1, (row - 2) * 16 + 1, 128):
            a = KeyList(row)
            a.make(at, _lib.TAB_TX).tx_keylen = bad
            assert a.call() == errno.EINVAL, (row, bad)
    a = KeyList()
    a.make(at, _lib.TAB_TX).tx_key = None
    assert a.call() == errno.EINVAL
    a = KeyList()
    o = a.make(at, _lib.TAB_RX)
    o.tx_key, o.tx_keylen = None, 1             # not an RX op's fields
    assert a.call() == PASSED


@pytest.mark.parametrize("at", PLACES)
@pytest.mark.parametrize("kind", (_lib.TAB_RX, _lib.TAB_TX))
def test_cipher_table_key_checks(kind, at):
    """check_cipher_keys, as net2_burst_ciphertab_set_rx / _set_tx make it."""
    for alg in (_lib.ENC_NIL, 2, -1):
        a = CipherList()
        a.make(at, kind).ck.enc_alg = alg
        assert a.call() == errno.EINVAL, alg
    for keylen in (0, 16, 24, 31, 33, 64):
        a = CipherList()
        a.make(at, kind).ck.enc_keylen = keylen
        assert a.call() == errno.EINVAL, keylen
    a = CipherList()
    a.make(at, kind).ck.enc_key = None
    assert a.call() == errno.EINVAL
    for keylen in (0, 16, 31, 33):
        a = CipherList()
        o = a.make(at, kind)
        o.ck.alt_enc_key, o.ck.alt_enc_keylen = ctypes.cast(a.alt, vp), keylen
        assert a.call() == errno.EINVAL, keylen
    a = CipherList()
    o = a.make(at, _lib.TAB_CLEAR)
    o.ck.enc_key, o.ck.enc_alg = None, 0        # a CLEAR has no keys
    assert a.call() == PASSED


@pytest.mark.parametrize("at", PLACES)
def test_cipher_table_rx_key_state_checks(at):
    for alg in (1, 2, 3, 7, -1):
        a = CipherList()
        a.make(at, _lib.TAB_RX).rx.hash_alg = alg
        assert a.call() == errno.EINVAL, alg
    # an alternate hash key installed, but no alternate cipher key
    a = CipherList()
    o = a.make(at, _lib.TAB_RX)
    o.rx.alt_hash_key = ctypes.cast(a.alt, vp)
    o.ck.alt_enc_key, o.ck.alt_enc_keylen = None, 0
    assert a.call() == errno.EINVAL
    # an alternate key without a keyed hash
    a = CipherList()
    o = a.make(at, _lib.TAB_RX)
    o.rx.alt_hash_key = ctypes.cast(a.alt, vp)
    o.ck.alt_enc_key, o.ck.alt_enc_keylen = ctypes.cast(a.alt, vp), 32
    o.rx.hash_alg = 0
    assert a.call() == errno.EINVAL
    # a TX op's rx state is not looked at
    a = CipherList()
    a.make(at, _lib.TAB_TX).rx.hash_alg = 7
    assert a.call() == PASSED


def test_first_bad_op_decides_and_counters_stay():
    """Checks run in array order over the whole list before the device check:
    with a bad op anywhere the result is EINVAL, not the device check's."""
    before = counters()
    a = KeyList()
    a.make(N - 1, 7)
    assert a.call() == errno.EINVAL
    a = CipherList()
    a.make(N - 1, 7)
    assert a.call() == errno.EINVAL
    assert counters() == before


def test_limits_and_stats_need_no_device():
    L = _lib.lib()
    for v in (64, 1, 0, 1 << 40, -1, -7):
        assert L.net2_burst_tab_limits(v) == 0
    assert L.net2_burst_tab_stats(None, None) == 0
    a, b = u64(7), u64(9)
    assert L.net2_burst_tab_stats(ctypes.byref(a), None) == 0
    assert L.net2_burst_tab_stats(None, ctypes.byref(b)) == 0
    assert (a.value, b.value) == counters()
    from ilias_net2_amd import conn_burst
    conn_burst.tab_limits(-1)
    assert conn_burst.tab_stats() == counters()


@pytest.mark.parametrize("name,standin", (
    ("net2_burst_keytab_fingerprint", lambda: KeyStandIn(-2, 6, SLOTS, None, None)),
    ("net2_burst_ciphertab_fingerprint", lambda: CipherStandIn(-2, SLOTS, None, None))))
def test_fingerprint_argument_checks(name, standin):
    fn = getattr(_lib.lib(), name)
    tab = standin()
    out = ctypes.create_string_buffer(32 * SLOTS)
    t, p = ctypes.byref(tab), ctypes.addressof(out)
    assert fn(None, 0, 1, p, None) == errno.EINVAL
    assert fn(None, 0, 0, p, None) == errno.EINVAL
    for first, n in ((0, SLOTS + 1), (SLOTS, 1), (1, SLOTS), (0xffffffff, 1),
                     (1, 0xffffffff), (SLOTS + 1, 0)):
        assert fn(t, first, n, p, None) == errno.EINVAL, (first, n)
    assert fn(t, 0, 1, None, None) == errno.EINVAL
    assert fn(t, 0, 0, None, None) == 0          # n == 0: nothing to write
    assert fn(t, SLOTS, 0, None, None) == 0
    assert fn(t, 0, SLOTS, p, None) == PASSED
    assert fn(t, SLOTS - 1, 1, p, None) == PASSED


def test_python_op_constructors_mirror_the_setters():
    import inspect
    from ilias_net2_amd import cipher_burst, conn_burst

    def params(f, drop):
        return [(n, p.default) for n, p in inspect.signature(f).parameters.items()
                if n not in drop]
    for mod, cls in ((conn_burst, conn_burst.KeyTable),
                     (cipher_burst, cipher_burst.CipherTable)):
        assert params(mod.rx_op, ()) == params(cls.set_rx, ("self", "stream"))
        assert params(mod.tx_op, ()) == params(cls.set_tx, ("self", "stream"))
        assert params(mod.clear_op, ()) == params(cls.clear, ("self", "stream"))
        assert hasattr(cls, "update") and hasattr(cls, "fingerprints")
    assert conn_burst.rx_op(3, b"k")[:2] == (_lib.TAB_RX, 3)
    assert cipher_burst.tx_op(2, b"k")[:2] == (_lib.TAB_TX, 2)
    assert conn_burst.clear_op(1) == (_lib.TAB_CLEAR, 1, {})
