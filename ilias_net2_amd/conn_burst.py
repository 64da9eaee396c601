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


# The ops of KeyTable.update: plain tuples (kind, slot, keyword arguments),
# made by constructors that mirror set_rx / set_tx / clear.
def rx_op(slot: int, key: bytes, enc_set: bool = False,
          alt_key: Optional[bytes] = None, alt_no_cutoff: bool = False,
          alt_cutoff: int = 0, rx_start: int = 0):
    """``KeyTable.set_rx(slot, key, ...)`` as an op of ``KeyTable.update``."""
    return (_lib.TAB_RX, slot, dict(key=key, enc_set=enc_set, alt_key=alt_key,
                                    alt_no_cutoff=alt_no_cutoff,
                                    alt_cutoff=alt_cutoff, rx_start=rx_start))


def tx_op(slot: int, key: bytes, enc_set: bool = False):
    """``KeyTable.set_tx(slot, key, ...)`` as an op of ``KeyTable.update``."""
    return (_lib.TAB_TX, slot, dict(key=key, enc_set=enc_set))


def clear_op(slot: int):
    """``clear(slot)`` as an op of ``update`` (either table)."""
    return (_lib.TAB_CLEAR, slot, {})


def tab_limits(ops_per_launch: int) -> None:
    """``net2_burst_tab_limits``: the most ops one launch of a bulk update
    takes (< 0: the default, 65,536).  A test knob; results do not depend on
    it."""
    check(_lib.lib().net2_burst_tab_limits(ops_per_launch), "net2_burst_tab_limits")


def tab_stats():
    """``net2_burst_tab_stats``: this process's table-update launches so far
    as ``(slot, bulk)`` -- those of the per-slot calls and those of the bulk
    updates, both tables.  Host state; needs no device."""
    slot, bulk = ctypes.c_uint64(0), ctypes.c_uint64(0)
    check(_lib.lib().net2_burst_tab_stats(ctypes.byref(slot), ctypes.byref(bulk)),
          "net2_burst_tab_stats")
    return slot.value, bulk.value


def _key_buf(key: bytes):
    return ctypes.create_string_buffer(bytes(key), max(len(key), 1))


def _fingerprints(fn, what, table, stream):
    """(slots, 32) uint8 CUDA tensor: the SHA-256 of every entry."""
    import torch
    s = _launch_stream(stream, table.device)
    with torch.cuda.stream(s):
        out = torch.empty((table.slots, 32), dtype=torch.uint8, device=table.device)
    with torch.cuda.device(table.device):
        check(fn(table.ptr, 0, table.slots, out.data_ptr(), s.cuda_stream), what)
    return out


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

    def build_ops(self, ops):
        """``ops`` (``rx_op`` / ``tx_op`` / ``clear_op``) as the array
        ``net2_burst_keytab_update`` takes, and the key buffers it points
        into: ``(array, buffers)``."""
        arr = (_lib.BurstKeytabOp * max(len(ops), 1))()
        keep = []
        for o, (kind, slot, kw) in zip(arr, ops):
            o.slot, o.op = slot, kind
            if kind == _lib.TAB_RX:
                kb = _key_buf(kw["key"])
                ab = None if kw["alt_key"] is None else _key_buf(kw["alt_key"])
                keep += [kb, ab]
                o.rx = _lib.BurstRxKeys(
                    self.hash_alg, ctypes.cast(kb, ctypes.c_void_p),
                    len(kw["key"]), int(bool(kw["enc_set"])),
                    None if ab is None else ctypes.cast(ab, ctypes.c_void_p),
                    0 if ab is None else len(kw["alt_key"]),
                    int(bool(kw["alt_no_cutoff"])), kw["alt_cutoff"] & 0xffffffff,
                    kw["rx_start"] & 0xffffffff)
            elif kind == _lib.TAB_TX:
                kb = _key_buf(kw["key"])
                keep.append(kb)
                o.tx_key = ctypes.cast(kb, ctypes.c_void_p)
                o.tx_keylen = len(kw["key"])
                o.tx_enc_alg = int(bool(kw["enc_set"]))
        return arr, keep

    def update(self, ops, stream=None) -> None:
        """Many slots in one call (``net2_burst_keytab_update``): ``ops`` is
        a list of ``rx_op`` / ``tx_op`` / ``clear_op``, applied in order; the
        table ends as the per-slot calls in that order would leave it.  All
        or nothing: a bad op raises and nothing is enqueued."""
        import torch
        ops = list(ops)
        arr, keep = self.build_ops(ops)
        with torch.cuda.device(self.device):
            rc = _lib.lib().net2_burst_keytab_update(
                self.ptr, arr, len(ops), self._stream(stream))
        del keep
        check(rc, "net2_burst_keytab_update")

    def fingerprints(self, stream=None):
        """The SHA-256 of every entry, a (slots, 32) uint8 CUDA tensor
        (``net2_burst_keytab_fingerprint``): equal for two tables that hold
        the same keys and state."""
        return _fingerprints(_lib.lib().net2_burst_keytab_fingerprint,
                             "net2_burst_keytab_fingerprint", self, stream)

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
