#!/usr/bin/env python3
"""The burst payload cipher under per-connection keys beside the
single-connection call.

1 M wire datagrams of {136, 584, 1496} B in HBM under HMAC-SHA512's layout
(8-byte header, 64-byte hash field, an AES-256-CBC payload of {64, 512, 1424}
B), every one PH_SIGNED | PH_ENCRYPTED, as tools/aes_burst_rates.py has them.
For a cipher table of K = 1, 1,024 and 65,536 connections, datagram i on slot
conn[i] drawn uniformly, the _mc call and the single-connection call alternate
in one process on the same datagrams, timed with device events in rounds of
`--reps` after a warm-up.  Every slot holds the same key, so the two calls
must agree bit for bit -- checked before anything is timed -- while each lane
still fetches its round keys from its own slot's entry.  One JSON object per
row (the median of the rounds, min-max beside it):

  rx_single / rx_mc   net2_packet_decrypt_burst / _mc (out of place)
  tx_single / tx_mc   net2_packet_encrypt_burst / _mc

and per K a summary row with the ratios mc / single and the single-connection
call's own spread (max / min of its rounds), the margin for calling a
difference real.

  python tools/aes_burst_mc_rates.py [--n N] [--conns 1,1024,65536]
                                     [--variant TEXT] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ilias_net2_amd import _lib, cipher_burst  # noqa: E402

ALG, HL, IVLEN, PO = 6, 64, 16, 72
EKEY = bytes(range(100, 132))
WIRE = [136, 584, 1496]


def timed_rounds(fns, reps, rounds):
    ms = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b) / reps)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--conns", default="1,1024,65536")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--variant", default=None,
                    help="a note on the build measured, copied into every row")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("aes_burst_mc_rates: no GPU (nothing is measured without one)")
    L = _lib.lib()
    dev = torch.device("cuda:0")
    n = args.n
    out_f = open(args.out, "w") if args.out else None
    g = torch.Generator(device=dev)
    g.manual_seed(29)
    lens64 = torch.tensor(WIRE, dtype=torch.int64, device=dev)[
        torch.randint(0, 3, (n,), device=dev, generator=g)]
    offs = torch.zeros(n, dtype=torch.int64, device=dev)
    offs[1:] = torch.cumsum(lens64, 0)[:-1]
    lens = lens64.to(torch.int32)
    plen = (lens64 - PO - 1).to(torch.int32)
    total = int(lens64.sum())
    payload = total - PO * n
    clear = torch.randint(0, 256, (total,), dtype=torch.uint8, device=dev, generator=g)
    seq = torch.arange(n, dtype=torch.int32, device=dev)
    flags = torch.full((n,), 3, dtype=torch.int32, device=dev)
    iv = torch.zeros((n, IVLEN), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    kb = ctypes.create_string_buffer(EKEY, 32)
    ck = _lib.BurstCipherKeys(_lib.ENC_AES256, ctypes.cast(kb, ctypes.c_void_p), 32,
                              None, 0)
    rk = _lib.BurstRxKeys(ALG, None, 0, 1, None, 0, 0, 0, 0)
    info = {"n": n, "bytes": total, "payload_bytes": payload, "hash": "HMAC-SHA512",
            "cipher": "AES-256-CBC", "build_id": L.net2_sha2_build_id().decode(),
            "device": torch.cuda.get_device_name(0), "reps": args.reps,
            "rounds": args.rounds}
    if args.variant:
        info["variant"] = args.variant
    _lib.check(L.net2_ph_to_iv_dev(seq.data_ptr(), flags.data_ptr(), n, IVLEN,
                                   iv.data_ptr(), st), "ph_to_iv_dev")

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if out_f:
            out_f.write(line + "\n")
            out_f.flush()

    def buffers():
        return (clear.clone(), torch.full((n,), 9, dtype=torch.uint8, device=dev),
                torch.zeros(n, dtype=torch.int32, device=dev))

    for K in [int(k) for k in args.conns.split(",") if k]:
        conn = torch.randint(0, K, (n,), device=dev, generator=g).to(torch.int32)
        with cipher_burst.CipherTable(K) as tab:
            for slot in range(K):
                tab.set_rx(slot, EKEY, hash_alg=ALG)
                tab.set_tx(slot, EKEY)
            tp = tab.ptr
            work_s, e_res_s, wire_s = buffers()
            work_m, e_res_m, wire_m = buffers()
            _, d_res_s, d_plen_s = buffers()
            _, d_res_m, d_plen_m = buffers()
            d_res_s.zero_()         # every datagram arrives OK
            d_res_m.zero_()
            plain_s, plain_m = torch.zeros_like(clear), torch.zeros_like(clear)

            def tx_single():
                _lib.check(L.net2_packet_encrypt_burst(
                    ctypes.byref(ck), HL, flags.data_ptr(), iv.data_ptr(),
                    work_s.data_ptr(), offs.data_ptr(), lens.data_ptr(), plen.data_ptr(),
                    n, e_res_s.data_ptr(), wire_s.data_ptr(), st), "encrypt_burst")

            def tx_mc():
                _lib.check(L.net2_packet_encrypt_burst_mc(
                    tp, conn.data_ptr(), HL, flags.data_ptr(), iv.data_ptr(),
                    work_m.data_ptr(), offs.data_ptr(), lens.data_ptr(), plen.data_ptr(),
                    n, e_res_m.data_ptr(), wire_m.data_ptr(), st), "encrypt_burst_mc")

            # once through, checked: both TX calls make the same burst ...
            tx_single()
            tx_mc()
            assert int((e_res_s != 0).sum()) == 0 and torch.equal(e_res_s, e_res_m), "tx"
            assert torch.equal(wire_s, lens) and torch.equal(wire_m, lens), "tx: wire"
            assert torch.equal(work_s, work_m), "tx: _mc and single differ"
            sealed = work_s.clone()

            def rx_single():
                _lib.check(L.net2_packet_decrypt_burst(
                    ctypes.byref(rk), ctypes.byref(ck), sealed.data_ptr(),
                    offs.data_ptr(), lens.data_ptr(), n, seq.data_ptr(), flags.data_ptr(),
                    iv.data_ptr(), d_res_s.data_ptr(), plain_s.data_ptr(),
                    d_plen_s.data_ptr(), st), "decrypt_burst")

            def rx_mc():
                _lib.check(L.net2_packet_decrypt_burst_mc(
                    tp, conn.data_ptr(), HL, sealed.data_ptr(), offs.data_ptr(),
                    lens.data_ptr(), n, seq.data_ptr(), flags.data_ptr(), iv.data_ptr(),
                    d_res_m.data_ptr(), plain_m.data_ptr(), d_plen_m.data_ptr(), st),
                    "decrypt_burst_mc")

            # ... and both RX calls bring the plaintext back
            rx_single()
            rx_mc()
            assert int((d_res_s != 0).sum()) == 0 and int((d_res_m != 0).sum()) == 0, "rx"
            assert torch.equal(d_plen_s, plen) and torch.equal(d_plen_m, plen), "rx: plen"
            assert torch.equal(plain_s, plain_m), "rx: _mc and single differ"
            m = min(n, 4096)
            end = int(offs[m - 1]) + int(lens[m - 1])
            h_plain, h_clear = plain_m[:end].cpu().numpy(), clear[:end].cpu().numpy()
            for i, (o, pl) in enumerate(zip(offs[:m].tolist(), plen[:m].tolist())):
                assert (h_plain[o + PO:o + PO + pl] == h_clear[o + PO:o + PO + pl]).all(), i

            fns = {"rx_single": rx_single, "rx_mc": rx_mc,
                   "tx_single": tx_single, "tx_mc": tx_mc}
            for fn in fns.values():
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            med, spread = {}, {}
            for name, v in timed_rounds(fns, args.reps, args.rounds).items():
                med[name] = statistics.median(v)
                spread[name] = max(v) / min(v)
                emit(dict(info, conns=K, kind=name, ms=round(med[name], 4),
                          ms_min_max=[round(min(v), 4), round(max(v), 4)],
                          datagrams_per_s=round(n / (med[name] * 1e-3), 1),
                          payload_gb_per_s=round(payload / (med[name] * 1e-3) / 1e9, 2)))
            emit(dict(info, conns=K, kind="summary",
                      rx_mc_over_single=round(med["rx_mc"] / med["rx_single"], 3),
                      tx_mc_over_single=round(med["tx_mc"] / med["tx_single"], 3),
                      rx_single_spread=round(spread["rx_single"], 3),
                      tx_single_spread=round(spread["tx_single"], 3)))
            torch.cuda.synchronize()
    if out_f:
        out_f.close()


if __name__ == "__main__":
    main()
