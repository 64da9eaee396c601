"""CPU: the C ABI of the prepared ECDSA P-521 keys (net2/ecdsa_key.h): the
binding's prototype table against the header, keytab sizes, the argument
checks (which come before the device check, so they need no GPU and never
touch the pointers they are given), ENODEV where no device is present, and
the sign layer's net2x_signctx_prepare_dev on another curve."""
import ctypes
import errno
import os
import re

import pytest

from ilias_net2_amd import _lib, ecdsa, ecdsa_key

import ecdsa_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAVE_GPU = _lib.device_count() > 0
TABLE = 16 + 131 * 15 * 136
vp = ctypes.c_void_p


def test_prototype_table_is_the_header():
    with open(os.path.join(ROOT, "include", "net2", "ecdsa_key.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = re.findall(r"^\s*(int|size_t|void)\s+(net2_\w+)\s*\(", text, flags=re.M)
    names = [name for _, name in declared]
    assert sorted(names) == sorted(ecdsa_key.SIGNATURES)
    assert len(names) == len(set(names)) == 6
    restypes = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "void": None}
    L = ecdsa_key.lib()
    for kind, name in declared:
        params = re.search(name + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        res, args = ecdsa_key.SIGNATURES[name]
        assert len(params.split(",")) == len(args), name
        assert res is restypes[kind], name
        assert getattr(L, name).restype is res
    # a table of their own: neither the four headers' nor net2/ecdsa.h's
    assert not set(names) & set(_lib.SIGNATURES)
    assert not set(names) & set(ecdsa.SIGNATURES)
    with open(os.path.join(ROOT, "include", "net2", "ecdsa.h")) as f:
        assert "keytab" not in f.read()
    assert f"NET2_ECDSA_P521_KEYTAB_TABLE_BYTES {TABLE}" in text
    assert ecdsa_key.TABLE_BYTES == TABLE == 267256
    assert f"NET2_ECDSA_P521_KEYTAB_MAGIC 0x{ecdsa_key.MAGIC:08x}u" in text
    assert f"NET2_ECDSA_P521_KEYTAB_MAX_KEYS {ecdsa_key.MAX_KEYS}" in text


def test_keytab_bytes():
    f = ecdsa_key.lib().net2_ecdsa_p521_keytab_bytes
    assert f(0) == 0                    # no such keytab
    assert f(1) == 2 * TABLE            # G's table and the key's
    assert f(2) == 3 * TABLE
    assert f(ecdsa_key.MAX_KEYS) == (ecdsa_key.MAX_KEYS + 1) * TABLE
    assert f(ecdsa_key.MAX_KEYS + 1) == 0
    assert f(2 ** 64 - 1) == 0
    assert ecdsa_key.keytab_bytes(2) == 3 * TABLE
    for bad in (0, ecdsa_key.MAX_KEYS + 1):
        with pytest.raises(ValueError):
            ecdsa_key.keytab_bytes(bad)


def _aligned(nbytes):
    """A host buffer and an 8-byte aligned address within it."""
    buf = ctypes.create_string_buffer(nbytes + 8)
    return buf, (ctypes.addressof(buf) + 7) & ~7


def test_argument_checks_come_first():
    """Every refusal is made on host pointers, before any device is looked
    for: nothing is dereferenced, nothing is launched."""
    L = ecdsa_key.lib()
    E = errno.EINVAL
    pub = ctypes.create_string_buffer(132 * 2)
    rs = ctypes.create_string_buffer(132 * 2)
    dig = ctypes.create_string_buffer(64 * 2)
    lens = (ctypes.c_uint32 * 2)(64, 64)
    kidx = (ctypes.c_uint32 * 2)(0, 0)
    valid = ctypes.create_string_buffer(b"\x07\x07", 2)
    ok = ctypes.create_string_buffer(b"\x07\x07", 2)
    keep, tab = _aligned(64)            # never written: far too small on purpose
    pub_p, rs_p, dig_p, valid_p, ok_p = (ctypes.addressof(b)
                                         for b in (pub, rs, dig, valid, ok))

    prep = L.net2_ecdsa_p521_keytab_prepare_dev
    assert prep(pub_p, 132, 0, tab, ok_p, None) == E                 # nkeys == 0
    assert prep(pub_p, 132, ecdsa_key.MAX_KEYS + 1, tab, ok_p, None) == E
    assert prep(pub_p, 132, 2 ** 63, tab, ok_p, None) == E
    for off in (1, 2, 4, 7):
        assert prep(pub_p, 132, 2, tab + off, ok_p, None) == E       # misaligned
    assert prep(pub_p, 132, 2, None, ok_p, None) == E
    assert prep(None, 132, 2, tab, ok_p, None) == E
    for stride in (0, 1, 131):
        assert prep(pub_p, stride, 2, tab, ok_p, None) == E

    ver = L.net2_ecdsa_p521_verify_keytab_dev

    def v(keytab=tab, nkeys=2, idx=kidx, rs_=rs_p, dig_=dig_p, ds=64, lens_=None,
          dlen=64, n=2, valid_=valid_p):
        return ver(keytab, nkeys, idx, rs_, dig_, ds, lens_, dlen, n, valid_, None)
    # n == 0: nothing to do, whatever else is passed
    assert ver(None, 0, None, None, None, 0, None, 0, 0, None, None) == 0
    assert v(n=0) == 0
    assert v(nkeys=0) == E
    assert v(nkeys=ecdsa_key.MAX_KEYS + 1) == E
    assert v(keytab=None) == E
    for off in (1, 4):
        assert v(keytab=tab + off) == E
    assert v(rs_=None) == E
    assert v(valid_=None) == E
    assert v(dig_=None) == E
    assert v(dig_=None, lens_=lens, dlen=0) == E
    assert v(ds=63) == E                # a digest longer than its slot
    assert v(ds=0, dlen=1) == E
    assert v(n=2 ** 32) == E

    new = L.net2_ecdsa_p521_keys_new
    h = vp(0x1234)
    assert new(pub_p, 132, 0, ctypes.byref(h), ok_p) == E and h.value is None
    assert new(pub_p, 132, ecdsa_key.MAX_KEYS + 1, ctypes.byref(h), ok_p) == E
    assert new(None, 132, 2, ctypes.byref(h), ok_p) == E
    assert new(pub_p, 131, 2, ctypes.byref(h), ok_p) == E
    assert new(pub_p, 132, 2, None, ok_p) == E
    vk = L.net2_ecdsa_p521_verify_keys
    assert vk(None, None, None, None, 0, None, 0, 0, None) == 0      # n == 0
    assert vk(None, kidx, rs_p, dig_p, 64, None, 64, 2, valid_p) == E
    L.net2_ecdsa_p521_keys_free(None)   # as free(NULL)

    assert valid.raw == b"\x07\x07" and ok.raw == b"\x07\x07"
    assert keep.raw == bytes(len(keep.raw))


@pytest.mark.skipif(HAVE_GPU, reason="a GPU is present")
def test_no_device_fails_loudly():
    """No CPU fallback: well-formed calls report ENODEV and write nothing."""
    L = ecdsa_key.lib()
    pub = ctypes.create_string_buffer(ecdsa_ref.public_key(5), 132)
    rs = ctypes.create_string_buffer(132)
    dig = ctypes.create_string_buffer(64)
    valid = ctypes.create_string_buffer(b"\x07", 1)
    ok = ctypes.create_string_buffer(b"\x07", 1)
    keep, tab = _aligned(2 * TABLE)
    a = ctypes.addressof
    assert L.net2_ecdsa_p521_keytab_prepare_dev(a(pub), 132, 1, tab, a(ok),
                                                None) == errno.ENODEV
    assert L.net2_ecdsa_p521_verify_keytab_dev(tab, 1, None, a(rs), a(dig), 64, None, 64,
                                               1, a(valid), None) == errno.ENODEV
    h = vp()
    assert L.net2_ecdsa_p521_keys_new(a(pub), 132, 1, ctypes.byref(h),
                                      a(ok)) == errno.ENODEV
    assert h.value is None
    assert valid.raw == b"\x07" and ok.raw == b"\x07"
    assert keep.raw == bytes(len(keep.raw))
    with pytest.raises(_lib.Net2Error) as ei:
        ecdsa_key.KeysP521(ecdsa_ref.public_key(5))
    assert ei.value.errno == errno.ENODEV


SIGN_LIB = os.path.join(ROOT, "ilias_net2_amd", "libnet2_sign.so")
PUB_PEM = os.path.join(ROOT, "tests", "golden", "keys", "ecdsa_p521_pub.pem")


def test_prepare_dev_of_the_sign_layer():
    _lib.lib()      # libnet2_sha2.so first: one HIP runtime in the process
    S = ctypes.CDLL(SIGN_LIB)
    S.net2x_signctx_pubnew.restype = vp
    S.net2x_signctx_pubnew.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
    S.net2x_signctx_free.argtypes = [vp]
    S.net2x_signctx_prepare_dev.argtypes = [vp]
    S.net2x_signctx_prepare_dev.restype = ctypes.c_int
    assert S.net2x_signctx_prepare_dev(None) == errno.EINVAL
    _, pub = ecdsa_ref.pem_keypair(ecdsa_ref.NID_P256)
    ctx = S.net2x_signctx_pubnew(0, pub, len(pub))
    assert ctx
    try:
        assert S.net2x_signctx_prepare_dev(ctx) == errno.EOPNOTSUPP
    finally:
        S.net2x_signctx_free(ctx)
    if not HAVE_GPU:        # a P-521 context needs the device: no fallback
        with open(PUB_PEM, "rb") as f:
            pem = f.read()
        ctx = S.net2x_signctx_pubnew(0, pem, len(pem))
        assert ctx
        try:
            assert S.net2x_signctx_prepare_dev(ctx) == errno.ENODEV
        finally:
            S.net2x_signctx_free(ctx)
