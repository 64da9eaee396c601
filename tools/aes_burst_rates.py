#!/usr/bin/env python3
"""The burst payload cipher beside the hash bursts and beside the CPU.

1 M wire datagrams of {136, 584, 1496} B in HBM: 8-byte header, 64-byte
HMAC-SHA512 field, then an AES-256-CBC payload of {64, 512, 1424} B (the
PKCS#7-padded form of {63, 511, 1423} plaintext bytes), every one
PH_SIGNED | PH_ENCRYPTED.  Timed with device events, the calls alternating in
rounds of `--reps` after a warm-up, one JSON object per row:

  rx_hash    net2_packet_decode_burst alone (HMAC verify + IVs)
  rx_aes     net2_packet_decrypt_burst alone (out of place)
  rx_chain   decode_burst, then decrypt_burst on the same stream
  tx_hash    net2_packet_encode_burst alone
  tx_aes     net2_packet_encrypt_burst alone
  tx_chain   encrypt_burst, then encode_burst on the same stream
  cpu_dec_T / cpu_enc_T   EVP AES-256-CBC over the same payloads in host
             memory on T threads (tools/evp_cbc_batch.c through ctypes)

and a summary row with the ratios chain / hash alone and device / CPU.
Before anything is timed the burst goes through TX and RX once: every code
is OK, the plaintext lengths come back, and the first datagrams' ciphertexts
and plaintexts are compared with EVP's.

  python tools/aes_burst_rates.py [--n N] [--threads 1,16] [--out FILE]
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

from ilias_net2_amd import _lib, conn_burst  # noqa: E402

ALG, HL, IVLEN, PO = 6, 64, 16, 72
HKEY = bytes(range(HL))
EKEY = bytes(range(100, 132))
WIRE = [136, 584, 1496]


def evp_lib():
    path = os.path.join(ROOT, "tools", "libevp_cbc_batch.so")
    if not os.path.exists(path):
        sys.exit(f"aes_burst_rates: {path} is missing (make -C tools)")
    E = ctypes.CDLL(path)
    E.evp_cbc_batch.restype = ctypes.c_int64
    E.evp_cbc_batch.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 8 + [
        ctypes.c_uint64, ctypes.c_int]
    return E


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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threads", default="1,16")
    ap.add_argument("--check", type=int, default=4096,
                    help="datagrams compared with EVP before timing")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("aes_burst_rates: no GPU (nothing is measured without one)")
    L, E = _lib.lib(), evp_lib()
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
    ws = conn_burst.burst_workspace(n, dev)
    st = torch.cuda.current_stream().cuda_stream
    kb = ctypes.create_string_buffer(EKEY, 32)
    ck = _lib.BurstCipherKeys(_lib.ENC_AES256, ctypes.cast(kb, ctypes.c_void_p), 32,
                              None, 0)
    rk = _lib.BurstRxKeys(ALG, None, 0, 1, None, 0, 0, 0, 0)
    info = {"n": n, "bytes": total, "payload_bytes": payload, "hash": "HMAC-SHA512",
            "cipher": "AES-256-CBC", "build_id": L.net2_sha2_build_id().decode(),
            "device": torch.cuda.get_device_name(0), "reps": args.reps,
            "rounds": args.rounds}

    def u8(fill=9):
        return torch.full((n,), fill, dtype=torch.uint8, device=dev)

    def i32():
        return torch.zeros(n, dtype=torch.int32, device=dev)
    tx_iv = torch.zeros((n, IVLEN), dtype=torch.uint8, device=dev)
    work, e_res, wire, s_res = clear.clone(), u8(), i32(), u8()
    r_res, r_iv, r_seq, r_fl = u8(), torch.zeros_like(tx_iv), i32(), i32()
    d_res, plain, d_plen = u8(0), torch.zeros_like(clear), i32()

    def tx_aes():
        _lib.check(L.net2_packet_encrypt_burst(
            ctypes.byref(ck), HL, flags.data_ptr(), tx_iv.data_ptr(), work.data_ptr(),
            offs.data_ptr(), lens.data_ptr(), plen.data_ptr(), n, e_res.data_ptr(),
            wire.data_ptr(), st), "encrypt_burst")

    def tx_hash():
        _lib.check(L.net2_packet_encode_burst(
            ALG, HKEY, HL, 1, seq.data_ptr(), flags.data_ptr(), work.data_ptr(),
            offs.data_ptr(), lens.data_ptr(), n, s_res.data_ptr(), ws.data_ptr(),
            ws.numel(), st), "encode_burst")

    def tx_chain():
        tx_aes()
        tx_hash()

    def rx_hash():
        _lib.check(L.net2_packet_decode_burst(
            ALG, HKEY, HL, 1, IVLEN, sealed.data_ptr(), offs.data_ptr(),
            lens.data_ptr(), n, r_res.data_ptr(), r_iv.data_ptr(), r_seq.data_ptr(),
            r_fl.data_ptr(), ws.data_ptr(), ws.numel(), st), "decode_burst")

    def rx_aes(res=None):
        _lib.check(L.net2_packet_decrypt_burst(
            ctypes.byref(rk), ctypes.byref(ck), sealed.data_ptr(), offs.data_ptr(),
            lens.data_ptr(), n, r_seq.data_ptr(), r_fl.data_ptr(), r_iv.data_ptr(),
            (d_res if res is None else res).data_ptr(), plain.data_ptr(),
            d_plen.data_ptr(), st), "decrypt_burst")

    def rx_chain():
        rx_hash()
        rx_aes(r_res)

    # once through, checked: TX of the clear burst, RX of what it made
    _lib.check(L.net2_ph_to_iv_dev(seq.data_ptr(), flags.data_ptr(), n, IVLEN,
                                   tx_iv.data_ptr(), st), "ph_to_iv_dev")
    tx_chain()
    assert int((e_res != 0).sum()) == 0 and int((s_res != 0).sum()) == 0, "tx"
    assert torch.equal(wire, lens), "tx: wire lengths"
    sealed = work.clone()
    rx_chain()
    assert int((r_res != 0).sum()) == 0, "rx: a datagram did not verify or decrypt"
    assert torch.equal(d_plen, plen) and torch.equal(r_iv, tx_iv), "rx"
    m = min(n, args.check)
    end = int(offs[m - 1]) + int(lens[m - 1])
    h_off = offs[:m].cpu().numpy().astype(np.uint64) + np.uint64(PO)
    h_plen = plen[:m].cpu().numpy().astype(np.uint32)
    h_clear, h_sealed = clear[:end].cpu().numpy(), sealed[:end].cpu().numpy()
    h_plain, h_iv = plain[:end].cpu().numpy(), tx_iv[:m].cpu().numpy()
    want = np.zeros(end + 16, dtype=np.uint8)
    wlen = np.zeros(m, dtype=np.uint32)
    p = lambda a: a.ctypes.data  # noqa: E731
    assert E.evp_cbc_batch(1, EKEY, p(h_iv), p(h_clear), p(h_off), p(h_plen), p(want),
                           p(h_off), p(wlen), m, 1) == 0
    for i in range(m):
        a = int(h_off[i])
        assert np.array_equal(h_sealed[a:a + int(wlen[i])], want[a:a + int(wlen[i])]), i
        assert np.array_equal(h_plain[a:a + int(h_plen[i])],
                              h_clear[a:a + int(h_plen[i])]), i

    rows = {}

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if out_f:
            out_f.write(line + "\n")
            out_f.flush()

    fns = {"rx_hash": rx_hash, "rx_aes": rx_aes, "rx_chain": rx_chain,
           "tx_hash": tx_hash, "tx_aes": tx_aes, "tx_chain": tx_chain}
    for fn in fns.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    for name, v in timed_rounds(fns, args.reps, args.rounds).items():
        med = statistics.median(v)
        rows[name] = med
        emit(dict(info, kind=name, ms=round(med, 4),
                  ms_min_max=[round(min(v), 4), round(max(v), 4)],
                  datagrams_per_s=round(n / (med * 1e-3), 1),
                  payload_gb_per_s=round(payload / (med * 1e-3) / 1e9, 2)))

    # the CPU: the same payloads in host memory, EVP on T threads
    h_sealed = sealed.cpu().numpy()
    h_clear = clear.cpu().numpy()
    h_off = offs.cpu().numpy().astype(np.uint64) + np.uint64(PO)
    h_clen = (lens.cpu().numpy() - PO).astype(np.uint32)
    h_plen = plen.cpu().numpy().astype(np.uint32)
    h_iv = tx_iv.cpu().numpy()
    h_out = np.zeros(total + 16, dtype=np.uint8)
    h_len = np.zeros(n, dtype=np.uint32)
    for T in [int(t) for t in args.threads.split(",") if t]:
        for enc, src, ln, name in ((0, h_sealed, h_clen, "cpu_dec"),
                                   (1, h_clear, h_plen, "cpu_enc")):
            v = []
            for _ in range(3):
                t0 = time.perf_counter()
                bad = E.evp_cbc_batch(enc, EKEY, p(h_iv), p(src), p(h_off), p(ln),
                                      p(h_out), p(h_off), p(h_len), n, T)
                v.append((time.perf_counter() - t0) * 1e3)
                assert bad == 0, (name, bad)
            med = statistics.median(v)
            rows[f"{name}_{T}"] = med
            emit(dict(info, kind=f"{name}_{T}", threads=T, ms=round(med, 3),
                      ms_min_max=[round(min(v), 3), round(max(v), 3)],
                      datagrams_per_s=round(n / (med * 1e-3), 1),
                      payload_gb_per_s=round(payload / (med * 1e-3) / 1e9, 2)))
    summary = dict(info, kind="summary",
                   rx_chain_over_hash=round(rows["rx_chain"] / rows["rx_hash"], 3),
                   tx_chain_over_hash=round(rows["tx_chain"] / rows["tx_hash"], 3))
    for k, v in rows.items():
        if k.startswith("cpu_dec_"):
            summary[f"rx_aes_speedup_over_{k}"] = round(v / rows["rx_aes"], 2)
        if k.startswith("cpu_enc_"):
            summary[f"tx_aes_speedup_over_{k}"] = round(v / rows["tx_aes"], 2)
    emit(summary)
    if out_f:
        out_f.close()


if __name__ == "__main__":
    main()
