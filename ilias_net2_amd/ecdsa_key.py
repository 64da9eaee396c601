"""Prepared keys for the batched ECDSA P-521 verification on the MI355X
(include/net2/ecdsa_key.h): prepare public keys once into a keytab of
fixed-window tables, then verify batches from it without the per-signature
doublings of ``ecdsa.verify_p521``.  The verdicts are the same, bit for bit.

``prepare_p521`` and ``verify_p521_keytab`` work on torch device tensors on
the current stream and allocate nothing when ``keytab`` / ``out`` are given
(both can be captured into a graph); ``KeysP521`` is the host-memory object
that owns a device keytab and takes numpy arrays.  The entry points are
declared in net2/ecdsa_key.h alone and bound here, with a prototype table of
their own, onto the library ``_lib.lib()`` loaded.  There is no CPU fallback:
without the library or a gfx950 device the calls raise.
"""
from __future__ import annotations

import ctypes

from . import _lib
from ._lib import check
from .ecdsa import PUB_BYTES, SIG_BYTES, _rows

WINDOWS = 131               # of 4 bits
DIGITS = 15                 # entries per window: d = 1..15
HEAD_BYTES = 16             # u32 magic, u32 valid, 8 zero bytes
ENTRY_BYTES = 136           # x then y, 17 little-endian u32 limbs each
TABLE_BYTES = HEAD_BYTES + WINDOWS * DIGITS * ENTRY_BYTES
MAGIC = 0x4b543531
MAX_KEYS = 1 << 20

_vp, _sz, _u32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32

# name -> (restype, argtypes): include/net2/ecdsa_key.h
SIGNATURES = {
    "net2_ecdsa_p521_keytab_bytes": (_sz, [_sz]),
    "net2_ecdsa_p521_keytab_prepare_dev": (ctypes.c_int, [
        _vp, _sz, _sz, _vp, _vp, _vp]),
    "net2_ecdsa_p521_verify_keytab_dev": (ctypes.c_int, [
        _vp, _sz, _vp, _vp, _vp, _sz, _vp, _u32, _sz, _vp, _vp]),
    "net2_ecdsa_p521_keys_new": (ctypes.c_int, [
        _vp, _sz, _sz, ctypes.POINTER(_vp), _vp]),
    "net2_ecdsa_p521_keys_free": (None, [_vp]),
    "net2_ecdsa_p521_verify_keys": (ctypes.c_int, [
        _vp, _vp, _vp, _vp, _sz, _vp, _u32, _sz, _vp]),
}

_bound = None


def lib() -> ctypes.CDLL:
    """The loaded library with this module's prototypes applied; raises if an
    entry point is missing (a library built before the prepared keys)."""
    global _bound
    if _bound is None:
        handle = _lib.lib()
        missing = [name for name in SIGNATURES if not hasattr(handle, name)]
        if missing:
            raise ImportError(f"{handle._name} lacks {', '.join(missing)}")
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = res, args
        _bound = handle
    return _bound


def keytab_bytes(nkeys: int) -> int:
    """Bytes of a keytab for ``nkeys`` keys, G's table included."""
    if not 1 <= nkeys <= MAX_KEYS:
        raise ValueError(f"nkeys: 1 .. {MAX_KEYS} keys are needed")
    return lib().net2_ecdsa_p521_keytab_bytes(nkeys)


def _keytab_ptr(keytab, nkeys: int) -> int:
    import torch
    if (keytab.dtype != torch.uint8 or not keytab.is_cuda or keytab.dim() != 1 or
            keytab.numel() < keytab_bytes(nkeys) or
            (keytab.numel() > 1 and keytab.stride(0) != 1) or keytab.data_ptr() % 8):
        raise ValueError("keytab: keytab_bytes(nkeys) contiguous uint8 device bytes, "
                         "8-byte aligned, are needed")
    return keytab.data_ptr()


def prepare_p521(pub, keytab=None, ok=None, stream=None):
    """Build the keytab of the keys in ``pub``; returns ``(keytab, ok)``.

    pub:    (nkeys, >=132) uint8 device tensor, x || y per row, or (132,)
    keytab: (keytab_bytes(nkeys),) uint8, 8-byte aligned, else allocated
    ok:     (nkeys,) uint8, 1 where the key is one a verification accepts,
            else allocated
    """
    import torch
    from .batch import _launch_stream
    p_ptr, p_stride, nkeys = _rows(pub, "pub", PUB_BYTES)
    if pub.dim() == 1 or nkeys == 1:
        p_stride = PUB_BYTES
    if keytab is None:
        keytab = torch.empty((keytab_bytes(nkeys),), dtype=torch.uint8, device=pub.device)
    if ok is None:
        ok = torch.empty((nkeys,), dtype=torch.uint8, device=pub.device)
    elif (ok.dtype != torch.uint8 or not ok.is_cuda or ok.shape != (nkeys,) or
          (nkeys > 1 and ok.stride(0) != 1)):
        raise ValueError("ok: an (nkeys,) uint8 device tensor is needed")
    k_ptr = _keytab_ptr(keytab, nkeys)
    s = _launch_stream(stream, pub.device)
    with torch.cuda.device(pub.device):
        check(lib().net2_ecdsa_p521_keytab_prepare_dev(
            p_ptr, p_stride, nkeys, k_ptr, ok.data_ptr(), s.cuda_stream),
            "net2_ecdsa_p521_keytab_prepare_dev")
    return keytab, ok


def verify_p521_keytab(keytab, nkeys, rs, digests, dlens=None, kidx=None, out=None,
                       stream=None):
    """Verify n signatures from a prepared keytab; returns the uint8 verdicts.

    keytab:  what ``prepare_p521`` built for ``nkeys`` keys
    rs, digests, dlens, out: as ``ecdsa.verify_p521``
    kidx:    None (key 0 for all) or an (n,) int32/uint32 device tensor: the
             key of each signature; an index of nkeys or more gives verdict 0
    """
    import torch
    from .batch import _launch_stream
    k_ptr = _keytab_ptr(keytab, nkeys)
    r_ptr, r_stride, n = _rows(rs, "rs", SIG_BYTES)
    if rs.dim() != 2 or (n > 1 and r_stride != SIG_BYTES) or rs.shape[1] != SIG_BYTES:
        raise ValueError("rs: an (n, 132) tensor of dense rows is needed")
    d_ptr, d_stride, d_rows = _rows(digests, "digests", 0)
    if digests.dim() != 2 or d_rows != n:
        raise ValueError("rs and digests disagree about n")
    ints = (torch.int32, getattr(torch, "uint32", torch.int32))
    width, l_ptr, i_ptr = digests.shape[1], None, None
    if dlens is None:
        dlen = width
    elif isinstance(dlens, int):
        if not 0 <= dlens <= width:
            raise ValueError("dlens: beyond the digest rows")
        dlen = dlens
    else:
        if (dlens.dtype not in ints or not dlens.is_cuda or dlens.shape != (n,) or
                (n > 1 and dlens.stride(0) != 1)):
            raise ValueError("dlens: an (n,) int32 device tensor is needed")
        dlen, l_ptr = 0, dlens.data_ptr()
    if kidx is not None:
        if (kidx.dtype not in ints or not kidx.is_cuda or kidx.shape != (n,) or
                (n > 1 and kidx.stride(0) != 1)):
            raise ValueError("kidx: an (n,) int32 device tensor is needed")
        i_ptr = kidx.data_ptr()
    if n > 1 and d_stride < width:
        raise ValueError("digests: overlapping rows")
    slot = d_stride if n > 1 else width
    if out is None:
        out = torch.empty((n,), dtype=torch.uint8, device=rs.device)
    elif (out.dtype != torch.uint8 or not out.is_cuda or out.shape != (n,) or
          (n > 1 and out.stride(0) != 1)):
        raise ValueError("out: an (n,) uint8 device tensor is needed")
    s = _launch_stream(stream, rs.device)
    with torch.cuda.device(rs.device):
        check(lib().net2_ecdsa_p521_verify_keytab_dev(
            k_ptr, nkeys, i_ptr, r_ptr, d_ptr if width else r_ptr, slot, l_ptr, dlen, n,
            out.data_ptr(), s.cuda_stream), "net2_ecdsa_p521_verify_keytab_dev")
    return out


class KeysP521:
    """Keys prepared from host memory (net2_ecdsa_p521_keys): owns a device
    keytab on the device selected when it was made; ``verify`` runs there
    whatever device the calling thread has selected since."""

    def __init__(self, pub):
        import numpy as np
        if isinstance(pub, (bytes, bytearray)):
            pub = np.frombuffer(bytes(pub), dtype=np.uint8)
        pub = np.ascontiguousarray(pub, dtype=np.uint8)
        if pub.ndim == 1:
            pub = pub.reshape(1, -1)
        if pub.ndim != 2 or pub.shape[1] != PUB_BYTES or pub.shape[0] == 0:
            raise ValueError("pub: (132,) or (nkeys, 132) is needed")
        self.nkeys = pub.shape[0]
        self.ok = np.zeros(self.nkeys, dtype=np.uint8)
        self._h = _vp()
        check(lib().net2_ecdsa_p521_keys_new(
            pub.ctypes.data, PUB_BYTES, self.nkeys, ctypes.byref(self._h),
            self.ok.ctypes.data), "net2_ecdsa_p521_keys_new")

    def verify(self, rs, digests, dlens=None, kidx=None):
        """numpy arrays in, a numpy uint8 array of verdicts out; synchronous."""
        import numpy as np
        if not self._h:
            raise ValueError("the keys were closed")
        rs, digests = (np.ascontiguousarray(a, dtype=np.uint8) for a in (rs, digests))
        if rs.ndim != 2 or rs.shape[1] != SIG_BYTES:
            raise ValueError("rs: an (n, 132) array is needed")
        n = rs.shape[0]
        if digests.ndim != 2 or digests.shape[0] != n:
            raise ValueError("digests: an (n, width) array is needed")
        width, lens, idx = digests.shape[1], None, None
        if dlens is None:
            dlen = width
        elif isinstance(dlens, int):
            dlen = dlens
        else:
            dlen, lens = 0, np.ascontiguousarray(dlens, dtype=np.uint32)
            if lens.shape != (n,):
                raise ValueError("dlens: an (n,) array is needed")
        if kidx is not None:
            idx = np.ascontiguousarray(kidx, dtype=np.uint32)
            if idx.shape != (n,):
                raise ValueError("kidx: an (n,) array is needed")
        valid = np.zeros(n, dtype=np.uint8)
        check(lib().net2_ecdsa_p521_verify_keys(
            self._h, None if idx is None else idx.ctypes.data, rs.ctypes.data,
            digests.ctypes.data if width else rs.ctypes.data, width,
            None if lens is None else lens.ctypes.data, dlen, n, valid.ctypes.data),
            "net2_ecdsa_p521_verify_keys")
        return valid

    def close(self):
        if self._h:
            lib().net2_ecdsa_p521_keys_free(self._h)
            self._h = _vp()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
