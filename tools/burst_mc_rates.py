#!/usr/bin/env python3
"""Multi-connection packet bursts against the single-connection calls.

net2_packet_decode_burst_mc / _encode_burst_mc (per-lane keys from the device
key table) at K in {1, 1,024, 65,536} connections with uniformly random
conn[i], beside net2_packet_decode_burst / _encode_burst (one key for the
launch) on the same datagrams: 1 M wire datagrams of {136, 584, 1500} B in
HBM (8-byte header, 64-byte HMAC-SHA512 field, {64, 512, 1428} B payload),
every one PH_SIGNED | PH_ENCRYPTED, 16-byte IVs.  The two calls alternate in
one process, each round of `--reps` calls timed with device events after a
warm-up; one JSON object per point (kind, K) with both rates, their ratio,
net2_sha2_build_id and the device.  Every datagram verifies in both forms,
and at K = 1 the two forms' outputs are compared.

  python tools/burst_mc_rates.py [--n N] [--conns 1,1024,65536] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ilias_net2_amd import _lib, conn_burst  # noqa: E402

ALG, HL, IVLEN = 6, 64, 16
KEY = bytes(range(HL))


def timed_rounds(fns, reps, rounds):
    """fns: name -> callable enqueueing one call.  Rounds alternate between
    them; per name the per-call milliseconds of every round."""
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("burst_mc_rates: no GPU (nothing is measured without one)")
    L = _lib.lib()
    dev = torch.device("cuda:0")
    n = args.n
    out = open(args.out, "w") if args.out else None
    g = torch.Generator(device=dev)
    g.manual_seed(17)
    choice = torch.tensor([136, 584, 1500], dtype=torch.int64, device=dev)
    lens64 = choice[torch.randint(0, 3, (n,), device=dev, generator=g)]
    offs = torch.zeros(n, dtype=torch.int64, device=dev)
    offs[1:] = torch.cumsum(lens64, 0)[:-1]
    lens = lens64.to(torch.int32)
    total = int(lens64.sum())
    plain = torch.randint(0, 256, (total,), dtype=torch.uint8, device=dev, generator=g)
    seq = torch.arange(n, dtype=torch.int32, device=dev)
    flags = torch.full((n,), 3, dtype=torch.int32, device=dev)
    ws = conn_burst.burst_workspace(n, dev)
    st = torch.cuda.current_stream().cuda_stream
    info = {"n": n, "bytes": total, "hash": "HMAC-SHA512", "ivlen": IVLEN,
            "build_id": L.net2_sha2_build_id().decode(),
            "device": torch.cuda.get_device_name(0), "reps": args.reps,
            "rounds": args.rounds}

    def outputs():
        return (torch.full((n,), 9, dtype=torch.uint8, device=dev),
                torch.zeros((n, IVLEN), dtype=torch.uint8, device=dev),
                torch.zeros(n, dtype=torch.int32, device=dev),
                torch.zeros(n, dtype=torch.int32, device=dev))

    # the single-connection burst: one key
    one = plain.clone()
    r1, iv1, sq1, fl1 = outputs()

    def tx_one():
        _lib.check(L.net2_packet_encode_burst(
            ALG, KEY, HL, 1, seq.data_ptr(), flags.data_ptr(), one.data_ptr(),
            offs.data_ptr(), lens.data_ptr(), n, r1.data_ptr(), ws.data_ptr(),
            ws.numel(), st), "encode_burst")

    def rx_one():
        _lib.check(L.net2_packet_decode_burst(
            ALG, KEY, HL, 1, IVLEN, one.data_ptr(), offs.data_ptr(), lens.data_ptr(),
            n, r1.data_ptr(), iv1.data_ptr(), sq1.data_ptr(), fl1.data_ptr(),
            ws.data_ptr(), ws.numel(), st), "decode_burst")
    tx_one()
    assert int((r1 != 0).sum()) == 0
    rx_one()
    assert int((r1 != 0).sum()) == 0

    rng = np.random.default_rng(23)
    for K in [int(k) for k in args.conns.split(",")]:
        tab = conn_burst.KeyTable(ALG, K)
        for k in range(K):
            key = KEY if k == 0 else rng.integers(0, 256, HL, dtype=np.uint8).tobytes()
            tab.set_rx(k, key, enc_set=True)
            tab.set_tx(k, key, enc_set=True)
        conn = torch.randint(0, K, (n,), dtype=torch.int32, device=dev, generator=g)
        many = plain.clone()
        rk, ivk, sqk, flk = outputs()

        def tx_mc():
            _lib.check(L.net2_packet_encode_burst_mc(
                tab.ptr, conn.data_ptr(), seq.data_ptr(), flags.data_ptr(),
                many.data_ptr(), offs.data_ptr(), lens.data_ptr(), n, rk.data_ptr(),
                ws.data_ptr(), ws.numel(), st), "encode_burst_mc")

        def rx_mc():
            _lib.check(L.net2_packet_decode_burst_mc(
                tab.ptr, conn.data_ptr(), IVLEN, many.data_ptr(), offs.data_ptr(),
                lens.data_ptr(), n, rk.data_ptr(), ivk.data_ptr(), sqk.data_ptr(),
                flk.data_ptr(), ws.data_ptr(), ws.numel(), st), "decode_burst_mc")
        tx_mc()
        assert int((rk != 0).sum()) == 0, "mc tx"
        rx_mc()
        assert int((rk != 0).sum()) == 0, "mc rx: a datagram did not verify"
        assert torch.equal(ivk, iv1) and torch.equal(sqk, sq1) and torch.equal(flk, fl1)
        if K == 1:
            assert torch.equal(many, one), "K = 1: sealed bytes differ"
        for kind, fns in (("rx", {"single": rx_one, "mc": rx_mc}),
                          ("tx", {"single": tx_one, "mc": tx_mc})):
            for fn in fns.values():
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            ms = timed_rounds(fns, args.reps, args.rounds)
            row = dict(info, kind=kind, conns=K, table_bytes=K * 400)
            for name, v in ms.items():
                med = statistics.median(v)
                row[f"{name}_ms"] = round(med, 4)
                row[f"{name}_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
                row[f"{name}_datagrams_per_s"] = round(n / (med * 1e-3), 1)
            row["mc_over_single"] = round(row["mc_datagrams_per_s"] /
                                          row["single_datagrams_per_s"], 4)
            line = json.dumps(row)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
        torch.cuda.synchronize()
        tab.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
