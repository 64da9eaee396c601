"""Batched ECDSA P-521 signature verification on the MI355X
(include/net2/ecdsa.h): one lane per signature, OpenSSL's ECDSA_do_verify
verdict bit for bit.

``verify_p521`` works on torch device tensors on the current stream and
allocates nothing when ``out`` is given (it can be captured into a graph);
``verify_p521_host`` takes numpy arrays or bytes and is synchronous.  The two
entry points are declared in net2/ecdsa.h alone and bound here, with a
prototype table of their own, onto the library ``_lib.lib()`` loaded.  There
is no CPU fallback: without the library or a gfx950 device the calls raise.
"""
from __future__ import annotations

import ctypes

from . import _lib
from ._lib import check

PUB_BYTES = 132     # x || y, 66 big-endian bytes each
SIG_BYTES = 132     # r || s

# name -> (restype, argtypes): include/net2/ecdsa.h
SIGNATURES = {
    "net2_ecdsa_p521_verify_dev": (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_size_t,
        ctypes.c_void_p, ctypes.c_void_p]),
    "net2_ecdsa_p521_verify": (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_size_t,
        ctypes.c_void_p]),
}

_bound = None


def lib() -> ctypes.CDLL:
    """The loaded library with this module's prototypes applied; raises if an
    entry point is missing (a library built before the verification)."""
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


def _rows(t, what: str, width: int):
    """(pointer, row stride, rows) of a uint8 device tensor of rows at least
    ``width`` bytes wide; a 1-D tensor is one row, stride 0."""
    import torch
    if t.dtype != torch.uint8 or not t.is_cuda:
        raise ValueError(f"{what}: a uint8 device tensor is needed")
    if t.dim() == 1:
        if t.numel() < width or (t.numel() > 1 and t.stride(0) != 1):
            raise ValueError(f"{what}: {width} contiguous bytes are needed")
        return t.data_ptr(), 0, 1
    if t.dim() != 2 or t.shape[1] < width or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError(f"{what}: rows of at least {width} contiguous bytes are needed")
    return t.data_ptr(), t.stride(0), t.shape[0]


def verify_p521(pub, rs, digests, dlens=None, out=None, stream=None):
    """Verify n signatures on the device; returns the uint8 tensor of verdicts.

    pub:     (n, >=132) uint8, one key per signature, or (132,) for one key
    rs:      (n, 132) uint8, r || s
    digests: (n, width) uint8; row strides are taken from the tensors
    dlens:   None (every digest is ``width`` bytes), an int (that many bytes
             of each row) or an (n,) int32/uint32 tensor of per-item lengths
    out:     (n,) uint8, else allocated
    """
    import torch
    from .batch import _launch_stream
    p_ptr, p_stride, p_rows = _rows(pub, "pub", PUB_BYTES)
    r_ptr, r_stride, n = _rows(rs, "rs", SIG_BYTES)
    if rs.dim() != 2 or (n > 1 and r_stride != SIG_BYTES) or rs.shape[1] != SIG_BYTES:
        raise ValueError("rs: an (n, 132) tensor of dense rows is needed")
    d_ptr, d_stride, d_rows = _rows(digests, "digests", 0)
    if digests.dim() != 2 or d_rows != n or (pub.dim() == 2 and p_rows != n):
        raise ValueError("pub, rs and digests disagree about n")
    width, l_ptr = digests.shape[1], None
    if dlens is None:
        dlen = width
    elif isinstance(dlens, int):
        if not 0 <= dlens <= width:
            raise ValueError("dlens: beyond the digest rows")
        dlen = dlens
    else:
        if (dlens.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or
                not dlens.is_cuda or
                dlens.shape != (n,) or (n > 1 and dlens.stride(0) != 1)):
            raise ValueError("dlens: an (n,) int32 device tensor is needed")
        dlen, l_ptr = 0, dlens.data_ptr()
    if n > 1 and d_stride < width:
        raise ValueError("digests: overlapping rows")
    # the C ABI's stride is the slot a digest may fill; for one row, its width
    slot = d_stride if n > 1 else width
    if out is None:
        out = torch.empty((n,), dtype=torch.uint8, device=rs.device)
    elif (out.dtype != torch.uint8 or not out.is_cuda or out.shape != (n,) or
          (n > 1 and out.stride(0) != 1)):
        raise ValueError("out: an (n,) uint8 device tensor is needed")
    s = _launch_stream(stream, rs.device)
    with torch.cuda.device(rs.device):
        check(lib().net2_ecdsa_p521_verify_dev(
            p_ptr, p_stride if pub.dim() == 2 else 0, r_ptr, d_ptr if width else r_ptr,
            slot, l_ptr, dlen, n, out.data_ptr(), s.cuda_stream),
            "net2_ecdsa_p521_verify_dev")
    return out


def verify_p521_host(pub, rs, digests, dlens=None):
    """The same from host memory, synchronous: numpy uint8 arrays (or bytes for
    ``pub``: one key for all); returns a numpy uint8 array of verdicts."""
    import numpy as np
    if isinstance(pub, (bytes, bytearray)):
        pub = np.frombuffer(bytes(pub), dtype=np.uint8)
    pub, rs, digests = (np.ascontiguousarray(a, dtype=np.uint8)
                        for a in (pub, rs, digests))
    if rs.ndim != 2 or rs.shape[1] != SIG_BYTES:
        raise ValueError("rs: an (n, 132) array is needed")
    n = rs.shape[0]
    if digests.ndim != 2 or digests.shape[0] != n:
        raise ValueError("digests: an (n, width) array is needed")
    if pub.shape not in ((PUB_BYTES,), (n, PUB_BYTES)):
        raise ValueError("pub: (132,) or (n, 132) is needed")
    width, lens = digests.shape[1], None
    if dlens is None:
        dlen = width
    elif isinstance(dlens, int):
        dlen = dlens
    else:
        dlen, lens = 0, np.ascontiguousarray(dlens, dtype=np.uint32)
        if lens.shape != (n,):
            raise ValueError("dlens: an (n,) array is needed")
    valid = np.zeros(n, dtype=np.uint8)
    check(lib().net2_ecdsa_p521_verify(
        pub.ctypes.data, PUB_BYTES if pub.ndim == 2 else 0, rs.ctypes.data,
        digests.ctypes.data if width else rs.ctypes.data, width,
        None if lens is None else lens.ctypes.data, dlen, n, valid.ctypes.data),
        "net2_ecdsa_p521_verify")
    return valid
