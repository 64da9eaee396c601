"""ECDSA over secp521r1 through the system libcrypto (ctypes): the checker of
the device verification's tests, as aes_ref.py is the burst cipher's.

Keys from a chosen private scalar, ECDSA_do_sign, ECDSA_do_verify on any
(r, s) -- zero, n or 2^528 - 1 included --, EC_POINT_mul, DER through
i2d_ECDSA_SIG, and the construction lattice that walks valid signatures
through the exceptional cases of the point addition.  Every expected verdict
is OpenSSL's own; the one case it cannot express, a public key that is not on
the curve, is 0 by the verification's contract.
"""
import ctypes
import ctypes.util
import functools
import random

NID_SECP521R1 = 716
NID_P256 = 415
BYTES = 66
P = 2 ** 521 - 1


@functools.lru_cache(maxsize=None)
def lib():
    name = ctypes.util.find_library("crypto")
    if name is None:
        raise ImportError("libcrypto not found")
    L = ctypes.CDLL(name)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    protos = {
        "EC_GROUP_new_by_curve_name": (vp, [ci]),
        "EC_GROUP_get_order": (ci, [vp, vp, vp]),
        "EC_POINT_new": (vp, [vp]),
        "EC_POINT_free": (None, [vp]),
        "EC_POINT_mul": (ci, [vp, vp, vp, vp, vp, vp]),
        "EC_POINT_is_at_infinity": (ci, [vp, vp]),
        "EC_POINT_get_affine_coordinates": (ci, [vp, vp, vp, vp, vp]),
        "EC_POINT_set_affine_coordinates": (ci, [vp, vp, vp, vp, vp]),
        "EC_KEY_new_by_curve_name": (vp, [ci]),
        "EC_KEY_free": (None, [vp]),
        "EC_KEY_set_private_key": (ci, [vp, vp]),
        "EC_KEY_set_public_key": (ci, [vp, vp]),
        "EC_KEY_set_public_key_affine_coordinates": (ci, [vp, vp, vp]),
        "ECDSA_do_sign": (vp, [ctypes.c_char_p, ci, vp]),
        "ECDSA_do_verify": (ci, [ctypes.c_char_p, ci, vp, vp]),
        "ECDSA_SIG_new": (vp, []),
        "ECDSA_SIG_free": (None, [vp]),
        "ECDSA_SIG_set0": (ci, [vp, vp, vp]),
        "ECDSA_SIG_get0_r": (vp, [vp]),
        "ECDSA_SIG_get0_s": (vp, [vp]),
        "i2d_ECDSA_SIG": (ci, [vp, ctypes.POINTER(ctypes.c_char_p)]),
        "BN_new": (vp, []),
        "BN_free": (None, [vp]),
        "BN_bin2bn": (vp, [ctypes.c_char_p, ci, vp]),
        "BN_bn2binpad": (ci, [vp, ctypes.c_char_p, ci]),
        "BN_num_bits": (ci, [vp]),
        "BN_CTX_new": (vp, []),
        "ERR_clear_error": (None, []),
        "EC_KEY_generate_key": (ci, [vp]),
        "BIO_new": (vp, [vp]),
        "BIO_s_mem": (vp, []),
        "BIO_free": (ci, [vp]),
        "BIO_read": (ci, [vp, ctypes.c_char_p, ci]),
        "PEM_write_bio_ECPrivateKey": (ci, [vp, vp, vp, vp, ci, vp, vp]),
        "PEM_write_bio_EC_PUBKEY": (ci, [vp, vp]),
    }
    for fname, (res, args) in protos.items():
        fn = getattr(L, fname)
        fn.restype, fn.argtypes = res, args
    return L


@functools.lru_cache(maxsize=None)
def _group():
    g = lib().EC_GROUP_new_by_curve_name(NID_SECP521R1)
    assert g
    return g


@functools.lru_cache(maxsize=None)
def _ctx():
    return lib().BN_CTX_new()


def _bn(v: int):
    raw = v.to_bytes(max(1, (v.bit_length() + 7) // 8), "big")
    return lib().BN_bin2bn(raw, len(raw), None)


def _int(bn) -> int:
    n = (lib().BN_num_bits(bn) + 7) // 8
    buf = ctypes.create_string_buffer(max(n, 1))
    lib().BN_bn2binpad(bn, buf, max(n, 1))
    return int.from_bytes(buf.raw, "big")


@functools.lru_cache(maxsize=None)
def order() -> int:
    L = lib()
    n = L.BN_new()
    assert L.EC_GROUP_get_order(_group(), n, _ctx()) == 1
    v = _int(n)
    L.BN_free(n)
    return v


def be66(v: int) -> bytes:
    return v.to_bytes(BYTES, "big")


def point_mul2(u1: int, pub: bytes = None, u2: int = 0):
    """u1 G + u2 Q through EC_POINT_mul, as (x, y); None for infinity."""
    L, g = lib(), _group()
    r, q = L.EC_POINT_new(g), None
    b1, b2 = _bn(u1), _bn(u2)
    x, y = L.BN_new(), L.BN_new()
    try:
        if pub is not None:
            q = L.EC_POINT_new(g)
            qx, qy = _bn(int.from_bytes(pub[:BYTES], "big")), _bn(
                int.from_bytes(pub[BYTES:], "big"))
            ok = L.EC_POINT_set_affine_coordinates(g, q, qx, qy, _ctx())
            L.BN_free(qx)
            L.BN_free(qy)
            assert ok == 1, "public key not on the curve"
        assert L.EC_POINT_mul(g, r, b1, q, b2 if q else None, _ctx()) == 1
        if L.EC_POINT_is_at_infinity(g, r):
            return None
        assert L.EC_POINT_get_affine_coordinates(g, r, x, y, _ctx()) == 1
        return _int(x), _int(y)
    finally:
        for b in (b1, b2, x, y):
            L.BN_free(b)
        L.EC_POINT_free(r)
        if q:
            L.EC_POINT_free(q)


@functools.lru_cache(maxsize=None)
def public_key(d: int) -> bytes:
    """x || y of d G, 66 big-endian bytes each."""
    x, y = point_mul2(d % order())
    return be66(x) + be66(y)


def sign(d: int, digest: bytes):
    """ECDSA_do_sign under the private scalar d: (r, s)."""
    L = lib()
    key = L.EC_KEY_new_by_curve_name(NID_SECP521R1)
    bd = _bn(d)
    try:
        assert L.EC_KEY_set_private_key(key, bd) == 1
        sig = L.ECDSA_do_sign(bytes(digest), len(digest), key)
        assert sig
        r, s = _int(L.ECDSA_SIG_get0_r(sig)), _int(L.ECDSA_SIG_get0_s(sig))
        L.ECDSA_SIG_free(sig)
        return r, s
    finally:
        L.BN_free(bd)
        L.EC_KEY_free(key)


def verify(pub: bytes, r: int, s: int, digest: bytes) -> int:
    """ECDSA_do_verify on a chosen (r, s): 1 or 0.  0 as well where OpenSSL
    refuses the public key (coordinates out of range or off the curve) or
    reports an error: the device call's contract for those."""
    L = lib()
    key = L.EC_KEY_new_by_curve_name(NID_SECP521R1)
    qx = _bn(int.from_bytes(pub[:BYTES], "big"))
    qy = _bn(int.from_bytes(pub[BYTES:], "big"))
    sig = L.ECDSA_SIG_new()
    try:
        if L.EC_KEY_set_public_key_affine_coordinates(key, qx, qy) != 1:
            L.ERR_clear_error()
            return 0
        assert L.ECDSA_SIG_set0(sig, _bn(r), _bn(s)) == 1
        rc = L.ECDSA_do_verify(bytes(digest), len(digest), sig, key)
        L.ERR_clear_error()
        return 1 if rc == 1 else 0
    finally:
        L.ECDSA_SIG_free(sig)
        L.BN_free(qx)
        L.BN_free(qy)
        L.EC_KEY_free(key)


def pem_keypair(nid: int = NID_SECP521R1):
    """A fresh key on the curve as (private PEM, public PEM): what
    net2x_signctx_privnew / net2x_signctx_pubnew read."""
    L = lib()
    key = L.EC_KEY_new_by_curve_name(nid)
    assert key and L.EC_KEY_generate_key(key) == 1
    out = []
    for write in (lambda b: L.PEM_write_bio_ECPrivateKey(b, key, None, None, 0,
                                                         None, None),
                  lambda b: L.PEM_write_bio_EC_PUBKEY(b, key)):
        bio = L.BIO_new(L.BIO_s_mem())
        assert write(bio) == 1
        buf = ctypes.create_string_buffer(4096)
        n = L.BIO_read(bio, buf, 4096)
        assert n > 0
        out.append(buf.raw[:n])
        L.BIO_free(bio)
    L.EC_KEY_free(key)
    return tuple(out)


def der(r: int, s: int) -> bytes:
    """i2d_ECDSA_SIG of (r, s)."""
    L = lib()
    sig = L.ECDSA_SIG_new()
    assert L.ECDSA_SIG_set0(sig, _bn(r), _bn(s)) == 1
    n = L.i2d_ECDSA_SIG(sig, None)
    buf = ctypes.create_string_buffer(n)
    p = ctypes.c_char_p(ctypes.addressof(buf))
    assert L.i2d_ECDSA_SIG(sig, ctypes.byref(p)) == n
    L.ECDSA_SIG_free(sig)
    return buf.raw


# ---- the construction lattice ---------------------------------------------

_KS = (31, 32, 33, 63, 64, 511, 512, 519, 520)


def lattice_scalars():
    n = order()
    around = [v for k in _KS for v in (2 ** k - 1, 2 ** k, 2 ** k + 1)]
    u1 = list(range(6)) + [n - 2, n - 1] + around
    u2 = list(range(1, 6)) + [n - 2, n - 1] + around
    return u1, u2


def lattice_keys(seed: int = 521):
    n, rng = order(), random.Random(seed)
    return [1, 2, 3, n - 2, n - 1, rng.randrange(1, n), rng.randrange(1, n)]


def _digest_of(e: int) -> bytes:
    """A digest whose e is the given value: 65 bytes where e < 2^520, else the
    66 bytes e << 7 (a fixed key cannot be re-rolled until e fits 65)."""
    if e < 2 ** 520:
        return e.to_bytes(65, "big")
    return (e << 7).to_bytes(BYTES, "big")


def lattice_case(d: int, u1: int, u2: int, rng: random.Random = None):
    """The valid signature whose verification computes u1 G + u2 (d G), as
    (pub, r, s, digest); None where that point is infinity.  With rng, d is
    re-rolled until e fits a 65-byte digest."""
    n = order()
    while True:
        pub = public_key(d)
        R = point_mul2(u1, pub, u2)
        if R is None:
            return None
        r = R[0] % n
        s = r * pow(u2, -1, n) % n
        e = u1 * s % n
        if r == 0 or s == 0:
            return None
        if rng is None or e < 2 ** 520:
            return pub, r, s, _digest_of(e)
        d = rng.randrange(1, n)


def infinity_case(d: int, u2: int, s: int):
    """(pub, r, s, digest) whose u1 G + u2 Q is infinity: u1 = -u2 d, with r
    and e derived from an arbitrary s.  OpenSSL rejects it."""
    n = order()
    u1 = -u2 * d % n
    return public_key(d), u2 * s % n, s, _digest_of(u1 * s % n)


def lattice(keys=None, pairs=None):
    """[(pub, r, s, digest, verdict)] over keys x u1 x u2 (or the given
    (u1, u2) pairs), the verdict OpenSSL's, plus infinity cases."""
    n, rng = order(), random.Random(1042)
    keys = lattice_keys() if keys is None else keys
    if pairs is None:
        u1s, u2s = lattice_scalars()
        pairs = [(a, b) for a in u1s for b in u2s]
    out = []
    for ki, d in enumerate(keys):
        roll = rng if ki >= 5 else None
        for u1, u2 in pairs:
            c = lattice_case(d, u1, u2, roll)
            if c is None:
                continue
            out.append(c + (verify(c[0], c[1], c[2], c[3]),))
    for d in keys[:5]:
        for u2 in (1, 2, n - 1, 2 ** 64):
            c = infinity_case(d, u2, rng.randrange(1, n))
            out.append(c + (verify(c[0], c[1], c[2], c[3]),))
    return out


def pack(cases, dig_stride: int = 128):
    """cases as the flat arrays of the device call: pub (n x 132), rs
    (n x 132), digests (n x dig_stride), dlens, verdicts."""
    import numpy as np
    k = len(cases)
    pub = np.zeros((k, 2 * BYTES), dtype=np.uint8)
    rs = np.zeros((k, 2 * BYTES), dtype=np.uint8)
    dig = np.zeros((k, dig_stride), dtype=np.uint8)
    dlens = np.zeros(k, dtype=np.uint32)
    want = np.zeros(k, dtype=np.uint8)
    for i, (p, r, s, d, v) in enumerate(cases):
        pub[i] = np.frombuffer(p, dtype=np.uint8)
        rs[i] = np.frombuffer(r.to_bytes(BYTES, "big") + s.to_bytes(BYTES, "big"),
                              dtype=np.uint8)
        dig[i, :len(d)] = np.frombuffer(d, dtype=np.uint8)
        dlens[i] = len(d)
        want[i] = v
    return pub, rs, dig, dlens, want
