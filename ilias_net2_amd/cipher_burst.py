"""The payload cipher of the packet bursts (torch glue).

``decrypt_burst`` runs after ``net2_packet_decode_burst{,_ck}`` and
``encrypt_burst`` before ``net2_packet_encode_burst``, each on the stream of
its hash burst: AES-256-CBC with PKCS#7 padding, the reference's ``aes256``
(src/enc.c:70-74), over the payloads of a device-resident burst, bit for bit
what OpenSSL's EVP computes.  PyTorch owns the memory and the streams; the
work is the HIP kernels behind ``net2_packet_{decrypt,encrypt}_burst``
(include/net2/packet.h).

For a burst that interleaves many connections, ``CipherTable`` mirrors
``struct net2_burst_ciphertab`` -- every connection's cipher keys on the
device, one slot per connection, beside ``conn_burst.KeyTable`` -- and
``decrypt_burst_mc`` / ``encrypt_burst_mc`` run each datagram under the keys
of slot ``conn[i]`` in one call.
"""
from __future__ import annotations

import ctypes
from typing import Optional

from . import _lib
from ._lib import check
from .batch import _launch_stream, _need

KEYLEN = 32         # AES-256
IVLEN = 16


def limits(wave_max: int) -> None:
    """``net2_aes_burst_limits``: the largest burst that ``decrypt_burst`` and
    ``decrypt_burst_mc`` decrypt one wave per datagram (0: never; < 0: the
    default).  Process-wide; results do not depend on it, only the time."""
    check(_lib.lib().net2_aes_burst_limits(wave_max), "net2_aes_burst_limits")


def stats() -> dict:
    """``net2_aes_burst_stats``: this process's decrypt launches so far, by
    form: ``{"lane_launches": ..., "wave_launches": ...}``."""
    lane, wave = ctypes.c_uint64(0), ctypes.c_uint64(0)
    check(_lib.lib().net2_aes_burst_stats(ctypes.byref(lane), ctypes.byref(wave)),
          "net2_aes_burst_stats")
    return {"lane_launches": lane.value, "wave_launches": wave.value}


def encrypt_limits(quad_max: int) -> None:
    """``net2_aes_encrypt_limits``: the largest burst that ``encrypt_burst`` and
    ``encrypt_burst_mc`` encrypt four lanes per datagram (0: never; < 0: the
    default).  Process-wide; results do not depend on it, only the time."""
    check(_lib.lib().net2_aes_encrypt_limits(quad_max), "net2_aes_encrypt_limits")


def encrypt_stats() -> dict:
    """``net2_aes_encrypt_stats``: this process's encrypt launches so far, by
    form: ``{"lane_launches": ..., "quad_launches": ...}``."""
    lane, quad = ctypes.c_uint64(0), ctypes.c_uint64(0)
    check(_lib.lib().net2_aes_encrypt_stats(ctypes.byref(lane), ctypes.byref(quad)),
          "net2_aes_encrypt_stats")
    return {"lane_launches": lane.value, "quad_launches": quad.value}


def _cipher_keys(key: bytes, alt_key: Optional[bytes]):
    """struct net2_burst_cipher_keys and the buffers it points into."""
    kb = ctypes.create_string_buffer(bytes(key), max(len(key), 1))
    ab = (None if alt_key is None else
          ctypes.create_string_buffer(bytes(alt_key), max(len(alt_key), 1)))
    ck = _lib.BurstCipherKeys(
        _lib.ENC_AES256, ctypes.cast(kb, ctypes.c_void_p), len(key),
        None if ab is None else ctypes.cast(ab, ctypes.c_void_p),
        0 if alt_key is None else len(alt_key))
    return ck, (kb, ab)


def _burst_args(data, offsets, lens, flags, iv):
    import torch
    _need(data, torch.uint8, "data")
    _need(offsets, torch.int64, "offsets")
    _need(lens, torch.int32, "lens")
    _need(flags, torch.int32, "flags")
    _need(iv, torch.uint8, "iv")
    n = int(offsets.numel())
    if lens.numel() != n or flags.numel() != n:
        raise ValueError("offsets, lens and flags differ in length")
    if iv.numel() != n * IVLEN:
        raise ValueError("iv must hold 16 bytes per datagram")
    return n


def decrypt_burst(hash_alg: int, key: bytes, data, offsets, lens, seq, flags,
                  iv, result, alt_key: Optional[bytes] = None,
                  alt_no_cutoff: bool = False, alt_cutoff: int = 0,
                  rx_start: int = 0, out=None, stream=None):
    """RX: decrypt the payloads of the datagrams that the hash burst left OK
    with PH_ENCRYPTED.  ``hash_alg`` is that burst's keyed hash (0: none;
    it sets where a signed datagram's payload starts); seq, flags (int32),
    iv (uint8[n, 16]) and result (uint8[n]) are its outputs.  ``alt_key``:
    the alternate key set's cipher key, when the hash burst ran with an
    alternate key installed -- with the same cutoff arguments.  ``out``: where
    the plaintexts go, at the datagrams' offsets (default: a new buffer;
    ``data`` itself decrypts in place).  ``result`` is updated in place (BAD
    for a ciphertext EVP would reject).  Returns (result, out, plen int32[n]);
    asynchronous on ``stream`` (default: torch's current stream)."""
    import torch
    n = _burst_args(data, offsets, lens, flags, iv)
    _need(seq, torch.int32, "seq")
    _need(result, torch.uint8, "result")
    if seq.numel() != n or result.numel() != n:
        raise ValueError("seq and result must have one entry per datagram")
    s = _launch_stream(stream, data.device)
    with torch.cuda.stream(s):
        if out is None:
            out = torch.empty_like(data)
        plen = torch.empty((n,), dtype=torch.int32, device=data.device)
    _need(out, torch.uint8, "out")
    if out.numel() < data.numel():
        raise ValueError("out is smaller than the burst")
    ck, keep = _cipher_keys(key, alt_key)
    # an alternate key is installed when alt_hash_key is set; the cipher
    # step reads only that much of the hash keys
    rk = _lib.BurstRxKeys(hash_alg, None, 0, _lib.ENC_AES256,
                          ck.alt_enc_key, 0, int(bool(alt_no_cutoff)),
                          alt_cutoff & 0xffffffff, rx_start & 0xffffffff)
    rc = _lib.lib().net2_packet_decrypt_burst(
        ctypes.byref(rk), ctypes.byref(ck), data.data_ptr(), offsets.data_ptr(),
        lens.data_ptr(), n, seq.data_ptr(), flags.data_ptr(), iv.data_ptr(),
        result.data_ptr(), out.data_ptr(), plen.data_ptr(), s.cuda_stream)
    del keep
    check(rc, "net2_packet_decrypt_burst")
    return result, out, plen


def encrypt_burst(key: bytes, hashlen: int, flags, iv, data, offsets, lens,
                  plen, stream=None):
    """TX: slot i of ``data`` holds plen[i] (int32) plaintext bytes after the
    header and, with PH_SIGNED, ``hashlen`` reserved bytes; with PH_ENCRYPTED
    they are encrypted in place under iv[i] (net2_ph_to_iv_dev's output).
    Returns (result uint8[n], wire_len int32[n]); wire_len is the ``lens`` of
    the encode burst that follows.  Asynchronous on ``stream``."""
    import torch
    n = _burst_args(data, offsets, lens, flags, iv)
    _need(plen, torch.int32, "plen")
    if plen.numel() != n:
        raise ValueError("plen must have one entry per datagram")
    s = _launch_stream(stream, data.device)
    with torch.cuda.stream(s):
        res = torch.empty((n,), dtype=torch.uint8, device=data.device)
        wire = torch.empty((n,), dtype=torch.int32, device=data.device)
    ck, keep = _cipher_keys(key, None)
    rc = _lib.lib().net2_packet_encrypt_burst(
        ctypes.byref(ck), hashlen, flags.data_ptr(), iv.data_ptr(),
        data.data_ptr(), offsets.data_ptr(), lens.data_ptr(), plen.data_ptr(),
        n, res.data_ptr(), wire.data_ptr(), s.cuda_stream)
    del keep
    check(rc, "net2_packet_encrypt_burst")
    return res, wire


# ---- the cipher over many connections -----------------------------------------

NOCONN = 5          # NET2_PBURST_NOCONN


# The ops of CipherTable.update: plain tuples (kind, slot, keyword arguments),
# made by constructors that mirror set_rx / set_tx / clear.
def rx_op(slot: int, key: bytes, hash_alg: int = 0,
          alt_key: Optional[bytes] = None, alt_no_cutoff: bool = False,
          alt_cutoff: int = 0, rx_start: int = 0):
    """``CipherTable.set_rx(slot, key, ...)`` as an op of ``update``."""
    return (_lib.TAB_RX, slot, dict(key=key, hash_alg=hash_alg, alt_key=alt_key,
                                    alt_no_cutoff=alt_no_cutoff,
                                    alt_cutoff=alt_cutoff, rx_start=rx_start))


def tx_op(slot: int, key: bytes):
    """``CipherTable.set_tx(slot, key)`` as an op of ``update``."""
    return (_lib.TAB_TX, slot, dict(key=key))


def clear_op(slot: int):
    """``CipherTable.clear(slot)`` as an op of ``update``."""
    return (_lib.TAB_CLEAR, slot, {})


class CipherTable:
    """A device cipher-key table of ``slots`` connections (AES-256-CBC), on
    ``device`` (default: torch's current device): ``struct
    net2_burst_ciphertab`` (include/net2/packet.h), the companion of
    ``conn_burst.KeyTable`` under the same ``conn`` indices.  Updates are
    asynchronous on ``stream`` and ordered with the bursts there."""

    def __init__(self, slots: int, device=None):
        import torch
        self._tab = ctypes.c_void_p()
        self.slots = slots
        self.device = torch.device("cuda", torch.cuda.current_device()
                                   if device is None else
                                   torch.device(device).index or 0)
        with torch.cuda.device(self.device):
            check(_lib.lib().net2_burst_ciphertab_create(
                _lib.ENC_AES256, slots, ctypes.byref(self._tab)),
                "net2_burst_ciphertab_create")

    @property
    def ptr(self) -> int:
        if not self._tab:
            raise ValueError("the cipher table is closed")
        return self._tab.value

    def _stream(self, stream):
        return _launch_stream(stream, self.device).cuda_stream

    def set_rx(self, slot: int, key: bytes, hash_alg: int = 0,
               alt_key: Optional[bytes] = None, alt_no_cutoff: bool = False,
               alt_cutoff: int = 0, rx_start: int = 0, stream=None) -> None:
        """The slot's rx side: the connection's cipher key and, during a
        rollover, the alternate key with the cutoff arguments its hash keys
        were set with (``hash_alg``: the connection's keyed hash; an
        alternate key needs one)."""
        import torch
        ck, keep = _cipher_keys(key, alt_key)
        rk = _lib.BurstRxKeys(hash_alg, None, 0, _lib.ENC_AES256,
                              ck.alt_enc_key, 0, int(bool(alt_no_cutoff)),
                              alt_cutoff & 0xffffffff, rx_start & 0xffffffff)
        with torch.cuda.device(self.device):
            rc = _lib.lib().net2_burst_ciphertab_set_rx(
                self.ptr, slot, ctypes.byref(rk), ctypes.byref(ck),
                self._stream(stream))
        del keep
        check(rc, "net2_burst_ciphertab_set_rx")

    def set_tx(self, slot: int, key: bytes, stream=None) -> None:
        """The slot's tx side: the key the transmitter encrypts with."""
        import torch
        ck, keep = _cipher_keys(key, None)
        with torch.cuda.device(self.device):
            rc = _lib.lib().net2_burst_ciphertab_set_tx(
                self.ptr, slot, ctypes.byref(ck), self._stream(stream))
        del keep
        check(rc, "net2_burst_ciphertab_set_tx")

    def clear(self, slot: int, stream=None) -> None:
        """Both sides of the slot unset."""
        import torch
        with torch.cuda.device(self.device):
            check(_lib.lib().net2_burst_ciphertab_clear(
                self.ptr, slot, self._stream(stream)),
                "net2_burst_ciphertab_clear")

    def build_ops(self, ops):
        """``ops`` (``rx_op`` / ``tx_op`` / ``clear_op``) as the array
        ``net2_burst_ciphertab_update`` takes, and the key buffers it points
        into: ``(array, buffers)``."""
        arr = (_lib.BurstCiphertabOp * max(len(ops), 1))()
        keep = []
        for o, (kind, slot, kw) in zip(arr, ops):
            o.slot, o.op = slot, kind
            if kind == _lib.TAB_RX:
                ck, bufs = _cipher_keys(kw["key"], kw["alt_key"])
                keep.append(bufs)
                o.ck = ck
                o.rx = _lib.BurstRxKeys(
                    kw["hash_alg"], None, 0, _lib.ENC_AES256, ck.alt_enc_key, 0,
                    int(bool(kw["alt_no_cutoff"])), kw["alt_cutoff"] & 0xffffffff,
                    kw["rx_start"] & 0xffffffff)
            elif kind == _lib.TAB_TX:
                ck, bufs = _cipher_keys(kw["key"], None)
                keep.append(bufs)
                o.ck = ck
        return arr, keep

    def update(self, ops, stream=None) -> None:
        """Many slots in one call (``net2_burst_ciphertab_update``): ``ops``
        is a list of ``rx_op`` / ``tx_op`` / ``clear_op``, applied in order;
        the table ends as the per-slot calls in that order would leave it.
        All or nothing: a bad op raises and nothing is enqueued."""
        import torch
        ops = list(ops)
        arr, keep = self.build_ops(ops)
        with torch.cuda.device(self.device):
            rc = _lib.lib().net2_burst_ciphertab_update(
                self.ptr, arr, len(ops), self._stream(stream))
        del keep
        check(rc, "net2_burst_ciphertab_update")

    def fingerprints(self, stream=None):
        """The SHA-256 of every entry, a (slots, 32) uint8 CUDA tensor
        (``net2_burst_ciphertab_fingerprint``)."""
        from .conn_burst import _fingerprints
        return _fingerprints(_lib.lib().net2_burst_ciphertab_fingerprint,
                             "net2_burst_ciphertab_fingerprint", self, stream)

    def close(self) -> None:
        if self._tab:
            _lib.lib().net2_burst_ciphertab_destroy(self._tab)
            self._tab = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _conn_arg(conn, n):
    import torch
    _need(conn, torch.int32, "conn")
    if conn.numel() != n:
        raise ValueError("conn must have one entry per datagram")


def decrypt_burst_mc(table: CipherTable, conn, hashlen: int, data, offsets, lens,
                     seq, flags, iv, result, out=None, stream=None):
    """``decrypt_burst`` under the rx keys of slot conn[i] (int32 CUDA tensor,
    read as uint32) of ``table``; ``hashlen`` is the digest length of the hash
    burst's row (0: none).  An OK PH_ENCRYPTED datagram without a connection
    becomes NOCONN.  Returns (result, out, plen int32[n]); asynchronous on
    ``stream``."""
    import torch
    n = _burst_args(data, offsets, lens, flags, iv)
    _conn_arg(conn, n)
    _need(seq, torch.int32, "seq")
    _need(result, torch.uint8, "result")
    if seq.numel() != n or result.numel() != n:
        raise ValueError("seq and result must have one entry per datagram")
    s = _launch_stream(stream, data.device)
    with torch.cuda.stream(s):
        if out is None:
            out = torch.empty_like(data)
        plen = torch.empty((n,), dtype=torch.int32, device=data.device)
    _need(out, torch.uint8, "out")
    if out.numel() < data.numel():
        raise ValueError("out is smaller than the burst")
    rc = _lib.lib().net2_packet_decrypt_burst_mc(
        table.ptr, conn.data_ptr(), hashlen, data.data_ptr(), offsets.data_ptr(),
        lens.data_ptr(), n, seq.data_ptr(), flags.data_ptr(), iv.data_ptr(),
        result.data_ptr(), out.data_ptr(), plen.data_ptr(), s.cuda_stream)
    check(rc, "net2_packet_decrypt_burst_mc")
    return result, out, plen


def encrypt_burst_mc(table: CipherTable, conn, hashlen: int, flags, iv, data,
                     offsets, lens, plen, stream=None):
    """``encrypt_burst`` under the tx key of slot conn[i] of ``table``.  A
    PH_ENCRYPTED slot with room but without a connection is NOCONN, untouched,
    wire_len 0.  Returns (result uint8[n], wire_len int32[n]); asynchronous on
    ``stream``."""
    import torch
    n = _burst_args(data, offsets, lens, flags, iv)
    _conn_arg(conn, n)
    _need(plen, torch.int32, "plen")
    if plen.numel() != n:
        raise ValueError("plen must have one entry per datagram")
    s = _launch_stream(stream, data.device)
    with torch.cuda.stream(s):
        res = torch.empty((n,), dtype=torch.uint8, device=data.device)
        wire = torch.empty((n,), dtype=torch.int32, device=data.device)
    rc = _lib.lib().net2_packet_encrypt_burst_mc(
        table.ptr, conn.data_ptr(), hashlen, flags.data_ptr(), iv.data_ptr(),
        data.data_ptr(), offsets.data_ptr(), lens.data_ptr(), plen.data_ptr(),
        n, res.data_ptr(), wire.data_ptr(), s.cuda_stream)
    check(rc, "net2_packet_encrypt_burst_mc")
    return res, wire
