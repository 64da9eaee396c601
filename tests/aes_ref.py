"""AES-256-CBC through the system libcrypto's EVP interface (ctypes): the
very calls the reference's src/enc.c makes (EVP_aes_256_cbc, :70-74,
:316-413), as the expected values of the burst cipher tests.

encrypt / decrypt work on one datagram's payload; ``pad=False`` turns EVP's
PKCS#7 padding off (EVP_CIPHER_CTX_set_padding), which is how the tests craft
ciphertexts whose padding is wrong.  decrypt returns None where EVP fails.
"""
import ctypes
import ctypes.util
import functools

KEYLEN, IVLEN, BLOCK = 32, 16, 16


@functools.lru_cache(maxsize=None)
def lib():
    name = ctypes.util.find_library("crypto")
    if name is None:
        raise ImportError("libcrypto not found")
    L = ctypes.CDLL(name)
    vp, ip = ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)
    L.EVP_CIPHER_CTX_new.restype = vp
    L.EVP_CIPHER_CTX_new.argtypes = []
    L.EVP_CIPHER_CTX_free.restype = None
    L.EVP_CIPHER_CTX_free.argtypes = [vp]
    L.EVP_aes_256_cbc.restype = vp
    L.EVP_aes_256_cbc.argtypes = []
    L.EVP_CIPHER_CTX_set_padding.restype = ctypes.c_int
    L.EVP_CIPHER_CTX_set_padding.argtypes = [vp, ctypes.c_int]
    for name in ("EVP_EncryptInit_ex", "EVP_DecryptInit_ex"):
        fn = getattr(L, name)
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, vp, vp, ctypes.c_char_p, ctypes.c_char_p]
    for name in ("EVP_EncryptUpdate", "EVP_DecryptUpdate"):
        fn = getattr(L, name)
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, ctypes.c_char_p, ip, ctypes.c_char_p, ctypes.c_int]
    for name in ("EVP_EncryptFinal_ex", "EVP_DecryptFinal_ex"):
        fn = getattr(L, name)
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, ctypes.c_void_p, ip]
    return L


def _run(enc: bool, key: bytes, iv: bytes, data: bytes, pad: bool):
    assert len(key) == KEYLEN and len(iv) == IVLEN
    L = lib()
    init, update, final = (
        (L.EVP_EncryptInit_ex, L.EVP_EncryptUpdate, L.EVP_EncryptFinal_ex) if enc
        else (L.EVP_DecryptInit_ex, L.EVP_DecryptUpdate, L.EVP_DecryptFinal_ex))
    ctx = L.EVP_CIPHER_CTX_new()
    assert ctx
    try:
        if init(ctx, L.EVP_aes_256_cbc(), None, bytes(key), bytes(iv)) != 1:
            return None
        L.EVP_CIPHER_CTX_set_padding(ctx, int(pad))
        out = ctypes.create_string_buffer(len(data) + 2 * BLOCK)
        n1, n2 = ctypes.c_int(0), ctypes.c_int(0)
        if update(ctx, out, ctypes.byref(n1), bytes(data), len(data)) != 1:
            return None
        if final(ctx, ctypes.byref(out, n1.value), ctypes.byref(n2)) != 1:
            return None
        return out.raw[:n1.value + n2.value]
    finally:
        L.EVP_CIPHER_CTX_free(ctx)


def encrypt(key: bytes, iv: bytes, plain: bytes, pad: bool = True):
    """EVP_Encrypt{Init_ex,Update,Final_ex}; None where EVP fails (without
    padding: a length that is no multiple of 16)."""
    return _run(True, key, iv, plain, pad)


def decrypt(key: bytes, iv: bytes, cipher: bytes, pad: bool = True):
    """EVP_Decrypt{Init_ex,Update,Final_ex}; None where EVP fails: a ragged
    or empty ciphertext, or (with padding) a last block whose padding is
    wrong."""
    return _run(False, key, iv, cipher, pad)
