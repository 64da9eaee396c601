#!/usr/bin/env python3
"""Host packet bursts by burst size.

net2_packet_decode_burst_host / _encode_burst_host (HMAC-SHA512, 16-byte
IVs, wire datagrams of {136, 584, 1500} B, every one PH_SIGNED|PH_ENCRYPTED)
at n in {64, 256, 1024, 4096, 16 K, 64 K, 1 M} datagrams from pinned and
from pageable host memory, one GPU (max_devices 1): per-call latency (median
and best of the repetitions after a warm-up) and datagrams/s.  Beside each
size, the oracle's restatement of the same calls (oracle_packet_*_batch,
test infrastructure, here only as the CPU figure) on 1 and 16 threads.  One
JSON object per line; every GPU result is checked against the oracle once per
size.

  python tools/burst_sizes.py [--sizes 64,256,...] [--out FILE]

With --conns K the bursts are those of a shared socket: K connections, each
with its own HMAC-SHA512 key (and, with --cipher, its own AES-256 key) in the
device tables, datagrams of {136, 584, 1496} B dealt out over them, through
net2_packet_{decode,encode}_burst_mc_host.  Every row carries two yardsticks
taken in the same run on the same burst: the single-connection _host call
(`host_single_us`) and the device-resident _mc sequence, the bytes already on
the device (`dev_mc_us`: the share the kernels take).  RX decrypts in place;
the sealed burst is put back before every call, outside the timing.  Every
output of the host calls is checked against the device-resident sequence once
per size.

  python tools/burst_sizes.py --conns 1024 [--cipher] [--sizes ...] [--out FILE]
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

from ilias_net2_amd import _lib  # noqa: E402
from oracle import oracle  # noqa: E402

SIZES = [64, 256, 1024, 4096, 16384, 65536, 1 << 20]
KEY = bytes(range(64))
ALG, IVLEN = 6, 16


def reps_for(n):
    return max(20, min(400, (1 << 22) // n))


def host(shape, dt, pinned):
    if pinned:
        t = torch.empty(shape, dtype={np.uint8: torch.uint8, np.uint32: torch.int32}[dt],
                        pin_memory=True)
        return t.numpy().view(dt)
    return np.empty(shape, dtype=dt)


def timed(fn, reps, budget_s=3.0, before=None):
    """before: run ahead of every call, outside its timing."""
    before = before or (lambda: None)
    for _ in range(2):
        before()
        fn()
    ts = []
    t_all = time.perf_counter()
    for _ in range(reps):
        before()
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
        if time.perf_counter() - t_all > budget_s and len(ts) >= 5:
            break
    return statistics.median(ts), min(ts), len(ts)


def main_mc(args, sizes):
    """The bursts of a shared socket: --conns connections, with or without the
    payload cipher."""
    from ilias_net2_amd import cipher_burst, conn_burst
    L = _lib.lib()
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    dev = torch.device("cuda:0")
    K, cipher = args.conns, args.cipher
    out = open(args.out, "a" if args.append else "w") if args.out else None
    rng = np.random.default_rng(12)
    hkeys = [rng.integers(0, 256, 64, dtype=np.uint8).tobytes() for _ in range(K)]
    kt = conn_burst.KeyTable(ALG, K)
    ct = cipher_burst.CipherTable(K) if cipher else None
    for k in range(K):
        kt.set_rx(k, hkeys[k], enc_set=True)
        kt.set_tx(k, hkeys[k], enc_set=True)
        if cipher:
            ek = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
            ct.set_rx(k, ek, hash_alg=ALG)
            ct.set_tx(k, ek)
    torch.cuda.synchronize()
    ctp = ct.ptr if cipher else None
    kb = ctypes.create_string_buffer(hkeys[0], 64)
    keys = _lib.BurstRxKeys(ALG, ctypes.cast(kb, ctypes.c_void_p), 64, 1, None, 0, 0, 0, 0)
    lens_all = rng.choice(np.array([136, 584, 1496], dtype=np.uint32), max(sizes))
    i32 = lambda a: torch.from_numpy(a.view(np.int32).copy()).to(dev)  # noqa: E731
    for memory in ("pinned", "pageable"):
        pin = memory == "pinned"
        for n in sizes:
            lens = lens_all[:n].copy()
            offs = np.zeros(n, dtype=np.uint64)
            offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
            total = int(lens.sum())
            plain = rng.integers(0, 256, total, dtype=np.uint8)
            data = host((total,), np.uint8, pin)
            conn = (np.arange(n, dtype=np.uint32) * 7) % K
            seq = np.arange(n, dtype=np.uint32)
            flags = np.full(n, 3, dtype=np.uint32)
            plen = (lens - 72 - 1).astype(np.uint32)
            res = host((n,), np.uint8, pin)
            wire = host((n,), np.uint32, pin)
            iv = host((n, IVLEN), np.uint8, pin)
            oseq, ofl = host((n,), np.uint32, pin), host((n,), np.uint32, pin)
            oplen = host((n,), np.uint32, pin)
            s0 = torch.cuda.current_stream().cuda_stream

            def tx():
                _lib.check(L.net2_packet_encode_burst_mc_host(
                    kt.ptr, ctp, p(conn), p(seq), p(flags), p(data), p(offs), p(lens),
                    p(plen) if cipher else None, n, p(res), p(wire) if cipher else None,
                    None), "encode_burst_mc_host")

            def rx():
                _lib.check(L.net2_packet_decode_burst_mc_host(
                    kt.ptr, ctp, p(conn), IVLEN, p(data), p(offs), p(lens), n, p(res),
                    p(iv), p(oseq), p(ofl), p(data) if cipher else None,
                    p(oplen) if cipher else None, None), "decode_burst_mc_host")

            def tx_single():
                _lib.check(L.net2_packet_encode_burst_host(
                    ALG, hkeys[0], 64, 1, p(seq), p(flags), p(data), p(offs), p(lens), n,
                    p(res), 1), "encode_burst_host")

            def rx_single():
                _lib.check(L.net2_packet_decode_burst_host(
                    ctypes.byref(keys), IVLEN, p(data), p(offs), p(lens), n, p(res),
                    p(iv), p(oseq), p(ofl), 1), "decode_burst_host")

            # the device-resident sequence on the same burst
            d = torch.from_numpy(plain).to(dev)
            d_off = torch.from_numpy(offs.view(np.int64).copy()).to(dev)
            d_len, d_conn, d_seq, d_fl, d_plen = (i32(a) for a in
                                                  (lens, conn, seq, flags, plen))
            d_res = torch.empty(n, dtype=torch.uint8, device=dev)
            d_eres = torch.empty(n, dtype=torch.uint8, device=dev)
            d_wire = torch.empty(n, dtype=torch.int32, device=dev)
            d_iv = torch.zeros((n, IVLEN), dtype=torch.uint8, device=dev)
            d_oseq, d_ofl, d_oplen = (torch.empty(n, dtype=torch.int32, device=dev)
                                      for _ in range(3))
            ws = conn_burst.burst_workspace(n, dev)

            def tx_dev():
                if cipher:
                    _lib.check(L.net2_ph_to_iv_dev(d_seq.data_ptr(), d_fl.data_ptr(), n, 16,
                                                   d_iv.data_ptr(), s0))
                    _lib.check(L.net2_packet_encrypt_burst_mc(
                        ctp, d_conn.data_ptr(), 64, d_fl.data_ptr(), d_iv.data_ptr(),
                        d.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), d_plen.data_ptr(),
                        n, d_eres.data_ptr(), d_wire.data_ptr(), s0))
                _lib.check(L.net2_packet_encode_burst_mc(
                    kt.ptr, d_conn.data_ptr(), d_seq.data_ptr(), d_fl.data_ptr(),
                    d.data_ptr(), d_off.data_ptr(),
                    d_wire.data_ptr() if cipher else d_len.data_ptr(), n, d_res.data_ptr(),
                    ws.data_ptr(), ws.numel(), s0))
                torch.cuda.synchronize()

            def rx_dev():
                _lib.check(L.net2_packet_decode_burst_mc(
                    kt.ptr, d_conn.data_ptr(), IVLEN, d.data_ptr(), d_off.data_ptr(),
                    d_len.data_ptr(), n, d_res.data_ptr(), d_iv.data_ptr(),
                    d_oseq.data_ptr(), d_ofl.data_ptr(), ws.data_ptr(), ws.numel(), s0))
                if cipher:
                    _lib.check(L.net2_packet_decrypt_burst_mc(
                        ctp, d_conn.data_ptr(), 64, d.data_ptr(), d_off.data_ptr(),
                        d_len.data_ptr(), n, d_oseq.data_ptr(), d_ofl.data_ptr(),
                        d_iv.data_ptr(), d_res.data_ptr(), d.data_ptr(),
                        d_oplen.data_ptr(), s0))
                torch.cuda.synchronize()

            # parity once per size: every output against the device sequence
            data[:] = plain
            tx()
            tx_dev()
            assert (res == 0).all(), (memory, n)
            assert np.array_equal(res, d_res.cpu().numpy()), (memory, n)
            sealed = d.cpu().numpy()
            assert np.array_equal(data, sealed), (memory, n)
            if cipher:
                assert np.array_equal(wire, d_wire.cpu().numpy().view(np.uint32))
            d_sealed = d.clone()
            rx()
            rx_dev()
            assert (res == 0).all() and np.array_equal(res, d_res.cpu().numpy()), (memory, n)
            assert np.array_equal(iv, d_iv.cpu().numpy()), (memory, n)
            assert np.array_equal(oseq, seq) and np.array_equal(ofl, flags), (memory, n)
            if cipher:
                assert np.array_equal(oplen, plen), (memory, n)
                # first and last plaintext byte of every datagram (what
                # follows a plaintext in its datagram is unspecified)
                for a in ((offs + 72).astype(np.int64),
                          (offs + 71 + plen).astype(np.int64)):
                    assert np.array_equal(data[a], plain[a]), (memory, n)

            def restore():
                data[:] = sealed

            def restore_dev():
                d.copy_(d_sealed)
                torch.cuda.synchronize()
            reps = reps_for(n)
            if n >= 1 << 18:
                reps = min(reps, 12)
            if args.zc_ab:
                # copy-then-HBM against reads through the host mapping
                # (NET2_BURST_MC_ZC_MAX, read per chunk): alternating in this
                # process, the order flipped every round
                for rnd in range(4):
                    order = ("copy", "mapped") if rnd % 2 == 0 else ("mapped", "copy")
                    for variant in order:
                        os.environ["NET2_BURST_MC_ZC_MAX"] = \
                            "0" if variant == "copy" else str(1 << 30)
                        for kind, fn in (("rx", rx), ("tx", tx)):
                            put = restore if kind == "rx" and cipher else None
                            if kind == "tx":    # the variant's outputs, once more
                                data[:] = plain
                                fn()
                                assert np.array_equal(data, sealed), (variant, n)
                            restore()
                            med, best, k = timed(fn, reps, before=put, budget_s=1.5)
                            if kind == "rx":
                                assert (res == 0).all() and np.array_equal(oplen, plen)
                                a = (offs + 71 + plen).astype(np.int64)
                                assert np.array_equal(data[a], plain[a]), (variant, n)
                            row = {"ab": "zc", "variant": variant, "round": rnd,
                                   "kind": kind, "memory": memory, "n": n, "conns": K,
                                   "reps": k, "median_us": round(med * 1e6, 1),
                                   "best_us": round(best * 1e6, 1)}
                            line = json.dumps(row)
                            print(line, flush=True)
                            if out:
                                out.write(line + "\n")
                                out.flush()
                del os.environ["NET2_BURST_MC_ZC_MAX"]
                continue
            for kind, fn, single, on_dev in (("rx", rx, rx_single, rx_dev),
                                             ("tx", tx, tx_single, tx_dev)):
                put = restore if kind == "rx" and cipher else None
                restore()
                med, best, k = timed(fn, reps, before=put)
                restore()
                m1, _, _ = timed(single, reps)
                restore_dev()
                m2, _, _ = timed(on_dev, reps,
                                 before=restore_dev if kind == "rx" and cipher else None)
                row = {"kind": kind, "memory": memory, "n": n, "conns": K,
                       "cipher": bool(cipher), "bytes": total, "reps": k,
                       "median_us": round(med * 1e6, 1), "best_us": round(best * 1e6, 1),
                       "datagrams_per_s": round(n / med, 1),
                       "us_per_datagram": round(med * 1e6 / n, 4),
                       "host_single_us": round(m1 * 1e6, 1),
                       "dev_mc_us": round(m2 * 1e6, 1),
                       "parity": "bit-exact vs the device-resident sequence"}
                line = json.dumps(row)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
            del data, res, iv, oseq, ofl, wire, oplen, d, d_sealed
    if out:
        out.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=",".join(map(str, SIZES)))
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="append to --out")
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--conns", type=int, default=0,
                    help="K > 0: the multi-connection host calls over K connections")
    ap.add_argument("--cipher", action="store_true",
                    help="with --conns: the payload cipher too")
    ap.add_argument("--zc-ab", action="store_true",
                    help="with --conns --cipher: copy-then-HBM against mapped reads")
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]
    if args.conns > 0:
        return main_mc(args, sizes)
    L = _lib.lib()
    O = oracle.lib()
    p = lambda a: a.ctypes.data  # noqa: E731
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    sz, u32 = ctypes.c_size_t, ctypes.c_uint32
    out = open(args.out, "a" if args.append else "w") if args.out else None
    nmax = max(sizes)
    rng = np.random.default_rng(11)
    lens_all = rng.choice(np.array([136, 584, 1500], dtype=np.uint32), nmax)
    kb = ctypes.create_string_buffer(KEY, 64)
    keys = _lib.BurstRxKeys(ALG, ctypes.cast(kb, ctypes.c_void_p), 64, 1, None, 0, 0, 0, 0)
    cpu16 = min(16, len(os.sched_getaffinity(0)))
    for memory in ("pinned", "pageable"):
        pin = memory == "pinned"
        for n in sizes:
            lens = lens_all[:n].copy()
            offs = np.zeros(n, dtype=np.uint64)
            offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
            total = int(lens.sum())
            data = host((total,), np.uint8, pin)
            data[:] = rng.integers(0, 256, total, dtype=np.uint8)
            seq = np.arange(n, dtype=np.uint32)
            flags = np.full(n, 3, dtype=np.uint32)
            res = host((n,), np.uint8, pin)
            iv = host((n, IVLEN), np.uint8, pin)
            oseq, ofl = host((n,), np.uint32, pin), host((n,), np.uint32, pin)

            def tx():
                _lib.check(L.net2_packet_encode_burst_host(
                    ALG, KEY, 64, 1, p(seq), p(flags), p(data), p(offs), p(lens), n,
                    p(res), 1), "encode_burst_host")

            def rx():
                _lib.check(L.net2_packet_decode_burst_host(
                    ctypes.byref(keys), IVLEN, p(data), p(offs), p(lens), n, p(res),
                    p(iv), p(oseq), p(ofl), 1), "decode_burst_host")
            # parity once per size: TX against the oracle, then RX
            o_res, o_sealed = oracle.packet_encode_batch(ALG, KEY, True, seq, flags, data,
                                                         offs, lens, nthreads=cpu16)
            tx()
            assert np.array_equal(res, o_res) and np.array_equal(data, o_sealed), (memory, n)
            want = oracle.packet_decode_batch(ALG, KEY, True, IVLEN, data, offs, lens,
                                              nthreads=cpu16)
            rx()
            assert np.array_equal(res, want[0]) and (res == 0).all(), (memory, n)
            assert np.array_equal(iv, want[1]) and np.array_equal(oseq, want[2]), (memory, n)
            reps = reps_for(n)
            for kind, fn in (("rx", rx), ("tx", tx)):
                med, best, k = timed(fn, reps)
                row = {"kind": kind, "memory": memory, "n": n, "bytes": total,
                       "reps": k, "median_us": round(med * 1e6, 1),
                       "best_us": round(best * 1e6, 1),
                       "datagrams_per_s": round(n / med, 1),
                       "us_per_datagram": round(med * 1e6 / n, 4),
                       "parity": "bit-exact vs oracle"}
                if pin and not args.no_oracle:
                    # the CPU restatement of the same call, same buffers
                    o_res = np.empty(n, dtype=np.uint8)
                    o_iv = np.empty((n, IVLEN), dtype=np.uint8)
                    o_sq = np.empty(n, dtype=np.uint32)
                    o_fl = np.empty(n, dtype=np.uint32)
                    scratch = np.array(data, copy=True)
                    for t in (1, cpu16):
                        if kind == "rx":
                            f = lambda t=t: O.oracle_packet_decode_batch(  # noqa: E731
                                ALG, KEY, sz(64), None, sz(0), 0, u32(0), u32(0), 1,
                                sz(IVLEN), vp(data), vp(offs), vp(lens), sz(n), vp(o_res),
                                vp(o_iv), vp(o_sq), vp(o_fl), t)
                        else:
                            f = lambda t=t: O.oracle_packet_encode_batch(  # noqa: E731
                                ALG, KEY, sz(64), 1, vp(seq), vp(flags), vp(scratch),
                                vp(offs), vp(lens), sz(n), vp(o_res), t)
                        m, _, _ = timed(f, max(5, min(reps, (1 << 18) // n)), budget_s=4.0)
                        row[f"oracle_{t}t_us"] = round(m * 1e6, 1)
                        row[f"oracle_{t}t_datagrams_per_s"] = round(n / m, 1)
                line = json.dumps(row)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
            del data, res, iv, oseq, ofl
    if out:
        out.close()


if __name__ == "__main__":
    main()
