"""Keyed packet bursts over many connections (torch glue).

A shared UDP socket hands its receive loop the datagrams of many connections
interleaved (src/udp_connection.c:81-170), each connection with its own
negotiated HMAC key and rollover state.  ``KeyTable`` mirrors
``struct net2_burst_keytab`` (include/net2/packet.h): that state on the
device, one slot per connection; ``decode_burst_mc`` / ``encode_burst_mc``
hash every datagram under the keys of slot ``conn[i]`` in one call.  PyTorch
owns the memory and the streams; the work is the HIP kernels behind
``net2_packet_{decode,encode}_burst_mc``.
"""
from __future__ import annotations

import ctypes
from typing import Optional

from . import _lib
from ._lib import check
from .batch import _launch_stream, _need

NOCONN = 5          # NET2_PBURST_NOCONN


class KeyTable:
    """A device key table of ``slots`` connections under one HMAC row
    (4..6), on ``device`` (default: torch's current device).  Updates are
    asynchronous on ``stream`` and ordered with the bursts there."""

    def __init__(self, hash_alg: int, slots: int, device=None):
        import torch
        self._tab = ctypes.c_void_p()
        self.hash_alg, self.slots = hash_alg, slots
        self.device = torch.device("cuda", torch.cuda.current_device()
                                   if device is None else
                                   torch.device(device).index or 0)
        with torch.cuda.device(self.device):
            check(_lib.lib().net2_burst_keytab_create(
                hash_alg, slots, ctypes.byref(self._tab)),
                "net2_burst_keytab_create")

    @property
    def ptr(self) -> int:
        if not self._tab:
            raise ValueError("the key table is closed")
        return self._tab.value

    def _stream(self, stream):
        return _launch_stream(stream, self.device).cuda_stream

    def set_rx(self, slot: int, key: bytes, enc_set: bool = False,
               alt_key: Optional[bytes] = None, alt_no_cutoff: bool = False,
               alt_cutoff: int = 0, rx_start: int = 0, stream=None) -> None:
        """The slot's rx side: a connection's rx key state, as
        net2_packet_decode_burst_ck takes it."""
        import torch
        kb = ctypes.create_string_buffer(bytes(key), max(len(key), 1))
        ab = (None if alt_key is None else
              ctypes.create_string_buffer(bytes(alt_key), max(len(alt_key), 1)))
        keys = _lib.BurstRxKeys(
            self.hash_alg, ctypes.cast(kb, ctypes.c_void_p), len(key),
            int(bool(enc_set)),
            None if ab is None else ctypes.cast(ab, ctypes.c_void_p),
            0 if alt_key is None else len(alt_key), int(bool(alt_no_cutoff)),
            alt_cutoff & 0xffffffff, rx_start & 0xffffffff)
        with torch.cuda.device(self.device):
            check(_lib.lib().net2_burst_keytab_set_rx(
                self.ptr, slot, ctypes.byref(keys), self._stream(stream)),
                "net2_burst_keytab_set_rx")

    def set_tx(self, slot: int, key: bytes, enc_set: bool = False,
               stream=None) -> None:
        """The slot's tx side: the key the transmitter seals with."""
        import torch
        kb = ctypes.create_string_buffer(bytes(key), max(len(key), 1))
        with torch.cuda.device(self.device):
            check(_lib.lib().net2_burst_keytab_set_tx(
                self.ptr, slot, kb, len(key), int(bool(enc_set)),
                self._stream(stream)), "net2_burst_keytab_set_tx")

    def clear(self, slot: int, stream=None) -> None:
        """Both sides of the slot unset."""
        import torch
        with torch.cuda.device(self.device):
            check(_lib.lib().net2_burst_keytab_clear(
                self.ptr, slot, self._stream(stream)),
                "net2_burst_keytab_clear")

    def close(self) -> None:
        if self._tab:
            _lib.lib().net2_burst_keytab_destroy(self._tab)
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


def burst_workspace(n: int, device, stream=None):
    """Scratch of an n-datagram burst (net2_packet_burst_workspace),
    allocated in ``stream``'s order and prepared so its first binning bins."""
    import torch
    L = _lib.lib()
    s = _launch_stream(stream, device)
    with torch.cuda.stream(s):
        ws = torch.empty((L.net2_packet_burst_workspace(n),), dtype=torch.uint8,
                         device=device)
    check(L.net2_sha2_workspace_init(ws.data_ptr(), ws.numel(), s.cuda_stream),
          "net2_sha2_workspace_init")
    return ws


def burst_stats():
    """``net2_sha2_burst_stats``: this process's keyed hash-burst launches so
    far as ``(lane, wave)`` -- one datagram per lane, or the one-launch
    small-burst form.  Host state; needs no device."""
    lane, wave = ctypes.c_uint64(0), ctypes.c_uint64(0)
    check(_lib.lib().net2_sha2_burst_stats(ctypes.byref(lane), ctypes.byref(wave)),
          "net2_sha2_burst_stats")
    return lane.value, wave.value


def _burst_args(data, conn, offsets, lens):
    import torch
    _need(data, torch.uint8, "data")
    _need(conn, torch.int32, "conn")
    _need(offsets, torch.int64, "offsets")
    _need(lens, torch.int32, "lens")
    n = int(offsets.numel())
    if lens.numel() != n or conn.numel() != n:
        raise ValueError("conn, offsets and lens differ in length")
    return n


def decode_burst_mc(table: KeyTable, conn, data, offsets, lens, ivlen: int = 0,
                    workspace=None, stream=None):
    """RX: datagram i = data[offsets[i] : offsets[i] + lens[i]] under the rx
    keys of slot conn[i] (int32 CUDA tensor, read as uint32).  Returns
    (result uint8[n], iv uint8[n, ivlen] or None, seq int32[n], flags
    int32[n]); IV rows where none is due are zero.  Asynchronous on
    ``stream`` (default: torch's current stream)."""
    import torch
    n = _burst_args(data, conn, offsets, lens)
    s = _launch_stream(stream, data.device)
    with torch.cuda.stream(s):
        res = torch.empty((n,), dtype=torch.uint8, device=data.device)
        iv = (torch.zeros((n, ivlen), dtype=torch.uint8, device=data.device)
              if ivlen else None)
        seq = torch.empty((n,), dtype=torch.int32, device=data.device)
        fl = torch.empty((n,), dtype=torch.int32, device=data.device)
    if workspace is None and n:
        workspace = burst_workspace(n, data.device, s)
    rc = _lib.lib().net2_packet_decode_burst_mc(
        table.ptr, conn.data_ptr(), ivlen, data.data_ptr(), offsets.data_ptr(),
        lens.data_ptr(), n, res.data_ptr(), None if iv is None else iv.data_ptr(),
        seq.data_ptr(), fl.data_ptr(),
        None if workspace is None else workspace.data_ptr(),
        0 if workspace is None else workspace.numel(), s.cuda_stream)
    check(rc, "net2_packet_decode_burst_mc")
    return res, iv, seq, fl


def encode_burst_mc(table: KeyTable, conn, seq, flags, data, offsets, lens,
                    workspace=None, stream=None):
    """TX: slot i of ``data`` sealed in place (header, HMAC field) under the
    tx key of slot conn[i]; seq / flags: int32 CUDA tensors.  Returns the
    codes (uint8[n]).  Asynchronous on ``stream``."""
    import torch
    n = _burst_args(data, conn, offsets, lens)
    _need(seq, torch.int32, "seq")
    _need(flags, torch.int32, "flags")
    if seq.numel() != n or flags.numel() != n:
        raise ValueError("seq and flags must have one entry per datagram")
    s = _launch_stream(stream, data.device)
    with torch.cuda.stream(s):
        res = torch.empty((n,), dtype=torch.uint8, device=data.device)
    if workspace is None and n:
        workspace = burst_workspace(n, data.device, s)
    rc = _lib.lib().net2_packet_encode_burst_mc(
        table.ptr, conn.data_ptr(), seq.data_ptr(), flags.data_ptr(),
        data.data_ptr(), offsets.data_ptr(), lens.data_ptr(), n, res.data_ptr(),
        None if workspace is None else workspace.data_ptr(),
        0 if workspace is None else workspace.numel(), s.cuda_stream)
    check(rc, "net2_packet_encode_burst_mc")
    return res
