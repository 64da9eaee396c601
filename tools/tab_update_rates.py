#!/usr/bin/env python3
"""Table updates: the per-slot calls against the bulk updates.

Two measurements, the variants alternating round by round in one process, every
time on a host clock (time.perf_counter) that ends in a stream synchronise:

  fill   both sides of both tables (HMAC-SHA512 key table, cipher table) for K
         connections: the per-slot calls issued directly through ctypes in a
         tight loop (4 K calls, their argument structs built beforehand)
         against one net2_burst_keytab_update and one
         net2_burst_ciphertab_update (2 K ops each, arrays built beforehand);
  storm  `--storm` set_rx between two `--burst`-datagram
         net2_packet_decode_burst_mc on one stream, from the first enqueue to
         the second burst's completion: per-slot calls against one bulk call.

One JSON object per point: per variant the median, min and max milliseconds
of the rounds and the rounds themselves, with net2_sha2_build_id and the
device.  After the first round of a fill the two variants' tables are
compared through their fingerprints.

  python tools/tab_update_rates.py [--conns 1024,65536] [--rounds 5] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ilias_net2_amd import _lib, cipher_burst, conn_burst  # noqa: E402

ALG, HL = 6, 64
vp = ctypes.c_void_p


def summary(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms),
            "rounds": [round(x, 4) for x in ms]}


class Keys:
    """K connections' keys in two flat buffers, and every argument struct of
    both variants built over them once."""

    def __init__(self, K, seed):
        rng = np.random.default_rng(seed)
        self.K = K
        self.hk = rng.integers(0, 256, (K, HL), dtype=np.uint8)
        self.ek = rng.integers(0, 256, (K, 32), dtype=np.uint8)
        hp, ep = self.hk.ctypes.data, self.ek.ctypes.data
        self.rx = (_lib.BurstRxKeys * K)()
        self.ck = (_lib.BurstCipherKeys * K)()
        self.kops = (_lib.BurstKeytabOp * (2 * K))()
        self.cops = (_lib.BurstCiphertabOp * (2 * K))()
        for k in range(K):
            self.rx[k] = _lib.BurstRxKeys(ALG, hp + HL * k, HL, 1, None, 0, 0, 0, 0)
            self.ck[k] = _lib.BurstCipherKeys(_lib.ENC_AES256, ep + 32 * k, 32, None, 0)
            a, b = self.kops[2 * k], self.kops[2 * k + 1]
            a.slot, a.op, a.rx = k, _lib.TAB_RX, self.rx[k]
            b.slot, b.op, b.tx_key, b.tx_keylen, b.tx_enc_alg = k, _lib.TAB_TX, hp + HL * k, HL, 1
            a, b = self.cops[2 * k], self.cops[2 * k + 1]
            a.slot, a.op, a.rx, a.ck = k, _lib.TAB_RX, self.rx[k], self.ck[k]
            b.slot, b.op, b.ck = k, _lib.TAB_TX, self.ck[k]


def fill_point(L, K, rounds, st, info):
    keys = Keys(K, 31 + K)
    tabs = {v: (conn_burst.KeyTable(ALG, K), cipher_burst.CipherTable(K))
            for v in ("per_slot", "bulk")}
    hp = keys.hk.ctypes.data

    def per_slot():
        kt, ct = (t.ptr for t in tabs["per_slot"])
        set_rx, set_tx = L.net2_burst_keytab_set_rx, L.net2_burst_keytab_set_tx
        cset_rx, cset_tx = L.net2_burst_ciphertab_set_rx, L.net2_burst_ciphertab_set_tx
        rx, ck, rc = keys.rx, keys.ck, 0
        for k in range(K):
            rc |= set_rx(kt, k, ctypes.byref(rx[k]), st)
            rc |= set_tx(kt, k, hp + HL * k, HL, 1, st)
            rc |= cset_rx(ct, k, ctypes.byref(rx[k]), ctypes.byref(ck[k]), st)
            rc |= cset_tx(ct, k, ctypes.byref(ck[k]), st)
        assert rc == 0

    def bulk():
        kt, ct = (t.ptr for t in tabs["bulk"])
        _lib.check(L.net2_burst_keytab_update(kt, keys.kops, 2 * K, st))
        _lib.check(L.net2_burst_ciphertab_update(ct, keys.cops, 2 * K, st))
    fns = {"per_slot": per_slot, "bulk": bulk}
    ms = {v: [] for v in fns}
    for r in range(rounds + 1):                 # round 0 warms up, not kept
        for v, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r:
                ms[v].append(1e3 * (time.perf_counter() - t0))
        if r == 0:
            for a, b in zip(tabs["per_slot"], tabs["bulk"]):
                assert torch.equal(a.fingerprints(), b.fingerprints()), "tables differ"
    for pair in tabs.values():
        for t in pair:
            t.close()
    out = dict(info, what="fill", conns=K, calls_per_slot=4 * K, calls_bulk=2,
               per_slot_ms=summary(ms["per_slot"]), bulk_ms=summary(ms["bulk"]))
    out["ratio"] = out["per_slot_ms"]["median"] / out["bulk_ms"]["median"]
    return out


def storm_point(L, dev, nset, n, rounds, st, info):
    """Two n-datagram decode bursts with nset rx rollovers between them."""
    K = max(nset, 1024)
    keys = Keys(K, 77)
    tab = conn_burst.KeyTable(ALG, K)
    _lib.check(L.net2_burst_keytab_update(tab.ptr, keys.kops, 2 * K, st))
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    lens = torch.full((n,), 584, dtype=torch.int32, device=dev)
    offs = torch.arange(n, dtype=torch.int64, device=dev) * 584
    conn = torch.randint(0, K, (n,), dtype=torch.int32, device=dev, generator=g)
    data = torch.randint(0, 256, (n * 584,), dtype=torch.uint8, device=dev, generator=g)
    seq = torch.arange(n, dtype=torch.int32, device=dev)
    flags = torch.full((n,), 3, dtype=torch.int32, device=dev)
    ws = conn_burst.burst_workspace(n, dev)
    res = conn_burst.encode_burst_mc(tab, conn, seq, flags, data, offs, lens, workspace=ws)
    assert int((res != 0).sum()) == 0
    out = [torch.full((n,), 9, dtype=torch.uint8, device=dev) for _ in range(2)]
    iv = torch.zeros((n, 16), dtype=torch.uint8, device=dev)
    rops = (_lib.BurstKeytabOp * nset)(*[keys.kops[2 * k] for k in range(nset)])

    def decode(o):
        _lib.check(L.net2_packet_decode_burst_mc(
            tab.ptr, conn.data_ptr(), 16, data.data_ptr(), offs.data_ptr(),
            lens.data_ptr(), n, o.data_ptr(), iv.data_ptr(), None, None, ws.data_ptr(),
            ws.numel(), st))

    def per_slot():
        rc, set_rx, rx, kt = 0, L.net2_burst_keytab_set_rx, keys.rx, tab.ptr
        decode(out[0])
        for k in range(nset):
            rc |= set_rx(kt, k, ctypes.byref(rx[k]), st)
        decode(out[1])
        assert rc == 0

    def bulk():
        decode(out[0])
        _lib.check(L.net2_burst_keytab_update(tab.ptr, rops, nset, st))
        decode(out[1])
    fns = {"per_slot": per_slot, "bulk": bulk}
    ms = {v: [] for v in fns}
    for r in range(rounds + 1):
        for v, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r:
                ms[v].append(1e3 * (time.perf_counter() - t0))
            assert int((out[0] != 0).sum()) == 0 and int((out[1] != 0).sum()) == 0
    tab.close()
    o = dict(info, what="storm", set_rx=nset, burst=n, slots=K,
             per_slot_ms=summary(ms["per_slot"]), bulk_ms=summary(ms["bulk"]))
    o["ratio"] = o["per_slot_ms"]["median"] / o["bulk_ms"]["median"]
    return o


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--conns", default="1024,65536")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--storm", type=int, default=1024)
    ap.add_argument("--burst", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tab_update_rates: no GPU (nothing is measured without one)")
    if args.rounds < 5:
        sys.exit("tab_update_rates: at least five rounds")
    L = _lib.lib()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    info = {"hash": "HMAC-SHA512", "cipher": "AES-256",
            "build_id": L.net2_sha2_build_id().decode(),
            "device": torch.cuda.get_device_name(0), "timed_rounds": args.rounds}
    out = open(args.out, "w") if args.out else None
    def emit(p):
        line = json.dumps(p)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    for k in args.conns.split(","):
        emit(fill_point(L, int(k), args.rounds, st, info))
    emit(storm_point(L, dev, args.storm, args.burst, args.rounds, st, info))
    if out:
        out.close()


if __name__ == "__main__":
    main()
