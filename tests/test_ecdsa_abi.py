"""CPU: the C ABI of the batched ECDSA P-521 verification (net2/ecdsa.h):
the binding's prototype table against the header, the argument checks (which
come before the device check, so they need no GPU), n == 0, and ENODEV where
no device is present; then the sign layer's host part
(net2x_signctx_validate_batch): the DER signatures it settles without the
device, and EOPNOTSUPP for a context on another curve."""
import ctypes
import errno
import os
import re

import pytest

from ilias_net2_amd import _lib, ecdsa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAVE_GPU = _lib.device_count() > 0


def test_prototype_table_is_the_header():
    with open(os.path.join(ROOT, "include", "net2", "ecdsa.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = re.findall(r"^\s*int\s+(net2_\w+)\s*\(", text, flags=re.M)
    assert sorted(declared) == sorted(ecdsa.SIGNATURES)
    assert len(declared) == len(set(declared)) == 2
    # parameter counts: a pointer or an integer each
    for name in declared:
        params = re.search(name + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        assert len(params.split(",")) == len(ecdsa.SIGNATURES[name][1]), name
    # ... and none of them has crept into the four headers' table
    assert not set(declared) & set(_lib.SIGNATURES)
    L = ecdsa.lib()
    for name in declared:
        assert getattr(L, name).restype is ctypes.c_int


def _calls():
    """Both entry points behind one signature (the device form with a null
    stream); the pointers are host buffers, never reached where the checks
    refuse the call."""
    L = ecdsa.lib()

    def dev(pub, ps, rs, dig, ds, dlens, dlen, n, valid):
        return L.net2_ecdsa_p521_verify_dev(pub, ps, rs, dig, ds, dlens, dlen, n,
                                            valid, None)
    return (("dev", dev), ("host", L.net2_ecdsa_p521_verify))


@pytest.mark.parametrize("which", [0, 1], ids=["dev", "host"])
def test_argument_checks_come_first(which):
    call = _calls()[which][1]
    pub = ctypes.create_string_buffer(132 * 2)
    rs = ctypes.create_string_buffer(132 * 2)
    dig = ctypes.create_string_buffer(64 * 2)
    lens = (ctypes.c_uint32 * 2)(64, 64)
    valid = ctypes.create_string_buffer(b"\x07\x07", 2)
    # n == 0: nothing to do, whatever else is passed
    assert call(None, 0, None, None, 0, None, 0, 0, None) == 0
    assert call(pub, 132, rs, dig, 64, None, 64, 0, valid) == 0
    # NULL arrays with n > 0
    assert call(None, 132, rs, dig, 64, None, 64, 2, valid) == errno.EINVAL
    assert call(pub, 132, None, dig, 64, None, 64, 2, valid) == errno.EINVAL
    assert call(pub, 132, rs, None, 64, None, 64, 2, valid) == errno.EINVAL
    assert call(pub, 132, rs, None, 64, lens, 0, 2, valid) == errno.EINVAL
    assert call(pub, 132, rs, dig, 64, None, 64, 2, None) == errno.EINVAL
    # a digest longer than its slot; a key stride inside a key
    assert call(pub, 132, rs, dig, 63, None, 64, 2, valid) == errno.EINVAL
    assert call(pub, 132, rs, dig, 0, None, 1, 2, valid) == errno.EINVAL
    assert call(pub, 131, rs, dig, 64, None, 64, 2, valid) == errno.EINVAL
    assert call(pub, 1, rs, dig, 64, None, 64, 2, valid) == errno.EINVAL
    # more signatures than the kernel's 32-bit index holds
    assert call(pub, 0, rs, dig, 64, None, 64, 2 ** 32, valid) == errno.EINVAL
    assert valid.raw == b"\x07\x07"         # nothing was launched or written


@pytest.mark.skipif(HAVE_GPU, reason="a GPU is present")
@pytest.mark.parametrize("which", [0, 1], ids=["dev", "host"])
def test_no_device_fails_loudly(which):
    """No CPU fallback: a well-formed call reports ENODEV."""
    call = _calls()[which][1]
    pub = ctypes.create_string_buffer(132)
    rs = ctypes.create_string_buffer(132)
    dig = ctypes.create_string_buffer(64)
    valid = ctypes.create_string_buffer(b"\x07", 1)
    assert call(pub, 0, rs, dig, 64, None, 64, 1, valid) == errno.ENODEV
    assert call(pub, 132, rs, None, 0, None, 0, 1, valid) == errno.ENODEV
    assert valid.raw == b"\x07"
    import numpy as np
    with pytest.raises(_lib.Net2Error) as ei:
        ecdsa.verify_p521_host(bytes(132), np.zeros((1, 132), np.uint8),
                               np.zeros((1, 64), np.uint8))
    assert ei.value.errno == errno.ENODEV


# ---- the sign layer: what the host settles before the device is needed -------

import ecdsa_ref  # noqa: E402

SIGN_LIB = os.path.join(ROOT, "ilias_net2_amd", "libnet2_sign.so")
PUB_PEM = os.path.join(ROOT, "tests", "golden", "keys", "ecdsa_p521_pub.pem")
vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def sign_lib():
    _lib.lib()      # libnet2_sha2.so first: one HIP runtime in the process
    S = ctypes.CDLL(SIGN_LIB)
    S.net2x_signctx_pubnew.restype = vp
    S.net2x_signctx_pubnew.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
    S.net2x_signctx_free.argtypes = [vp]
    S.net2x_signctx_maxmsglen.restype = ctypes.c_size_t
    S.net2x_signctx_maxmsglen.argtypes = [vp]
    S.net2x_signctx_validate.argtypes = [vp, ctypes.c_char_p, ctypes.c_size_t,
                                         ctypes.c_char_p, ctypes.c_size_t]
    S.net2x_signctx_validate_batch.argtypes = [
        vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_size_t),
        ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
        ctypes.POINTER(ctypes.c_int)]
    return S


def _batch(S, ctx, sigs, digests, dlen):
    n = len(sigs)
    ptrs = (ctypes.c_char_p * n)(*sigs)
    lens = (ctypes.c_size_t * n)(*[len(s) for s in sigs])
    valid = (ctypes.c_int * n)(*([7] * n))
    rc = S.net2x_signctx_validate_batch(ctx, ptrs, lens, b"".join(digests), dlen, dlen,
                                        n, valid)
    return rc, list(valid)


def _der_int(v: bytes) -> bytes:
    assert len(v) < 128
    return b"\x02" + bytes([len(v)]) + v


def _der_seq(body: bytes, long_form: bool = True) -> bytes:
    if len(body) < 128 and not long_form:
        return b"\x30" + bytes([len(body)]) + body
    assert len(body) < 256
    return b"\x30\x81" + bytes([len(body)]) + body


def test_der_handling_needs_no_device(sign_lib):
    """Signatures the host part refuses are 0 without a launch, so the call
    succeeds on a machine with no GPU; each is held to what ECDSA_verify
    (net2x_signctx_validate) makes of the same bytes."""
    S = sign_lib
    with open(PUB_PEM, "rb") as f:
        pem = f.read()
    ctx = S.net2x_signctx_pubnew(0, pem, len(pem))
    assert ctx
    try:
        n = ecdsa_ref.order()
        r, s = 0x1234567 + (1 << 518), n - 5
        good = ecdsa_ref.der(r, s)
        rb, sb = r.to_bytes(66, "big").lstrip(b"\0"), s.to_bytes(66, "big")
        # neither leading byte has its top bit: the minimal encodings, by hand
        assert good == _der_seq(_der_int(rb) + _der_int(sb.lstrip(b"\0")))
        body = good[3:]
        cases = {
            "trailing byte": good + b"\0",
            "trailing byte inside the length": _der_seq(body + b"\0"),
            "non-minimal sequence length": b"\x30\x82\x00" + good[2:],
            "non-minimal integer length":
                _der_seq(b"\x02\x81" + bytes([len(rb)]) + rb + _der_int(sb.lstrip(b"\0"))),
            "padded integer": _der_seq(_der_int(b"\0" + rb) + _der_int(sb.lstrip(b"\0"))),
            "negative integer": _der_seq(_der_int(b"\x81" + rb[1:]) +
                                         _der_int(sb.lstrip(b"\0"))),
            "67-byte r": _der_seq(_der_int(b"\x01" + bytes(66)) + _der_int(b"\x05")),
            "longer than any signature": _der_seq(_der_int(b"\x01" + bytes(70)) +
                                                  _der_int(b"\x01" + bytes(70))),
            "truncated": good[:-1],
            "empty": b"",
            "not DER": b"\xff" * 20,
        }
        dig = bytes(range(64))
        assert len(cases["longer than any signature"]) > S.net2x_signctx_maxmsglen(ctx)
        for name, sig in cases.items():
            assert S.net2x_signctx_validate(ctx, sig, len(sig), dig, 64) == 0, name
        rc, valid = _batch(S, ctx, list(cases.values()), [dig] * len(cases), 64)
        assert rc == 0 and valid == [0] * len(cases)
        # n == 0 and the argument checks
        assert S.net2x_signctx_validate_batch(ctx, None, None, None, 0, 0, 0, None) == 0
        assert _batch(S, None, [good], [dig], 64)[0] == errno.EINVAL
        ptrs, lens = (ctypes.c_char_p * 2)(good, good), (ctypes.c_size_t * 2)(9, 9)
        valid = (ctypes.c_int * 2)()
        assert S.net2x_signctx_validate_batch(ctx, ptrs, lens, dig * 2, 63, 64, 2,
                                              valid) == errno.EINVAL
        # a well-formed signature does need the device
        if not HAVE_GPU:
            rc, valid = _batch(S, ctx, [cases["truncated"], good], [dig] * 2, 64)
            assert rc == errno.ENODEV and valid == [0, 0]
    finally:
        S.net2x_signctx_free(ctx)


def test_other_curves_are_not_supported(sign_lib):
    S = sign_lib
    _, pub = ecdsa_ref.pem_keypair(ecdsa_ref.NID_P256)
    ctx = S.net2x_signctx_pubnew(0, pub, len(pub))
    assert ctx
    try:
        rc, valid = _batch(S, ctx, [ecdsa_ref.der(1, 2)], [bytes(32)], 32)
        assert rc == errno.EOPNOTSUPP and valid == [7]
    finally:
        S.net2x_signctx_free(ctx)
