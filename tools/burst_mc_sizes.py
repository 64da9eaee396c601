#!/usr/bin/env python3
"""Multi-connection keyed bursts by burst size, in both forms.

net2_packet_decode_burst_mc / _encode_burst_mc over n device-resident wire
datagrams, n in {64, 256, 1,024, 4,096, 16,384, 65,536}: HMAC-SHA512, 16-byte
IVs, datagrams of {136, 584, 1500} B (8-byte header, 64-byte hash field,
{64, 512, 1428} B payload), every one PH_SIGNED | PH_ENCRYPTED, conn[i]
uniformly random over 1,024 connections of the device key table.  In this
process the lane form (net2_sha2_burst_limits wave_max 0: hmac_mc_kernel, one
datagram per lane, plus the fold launch on RX) and the wave form (2^30:
burst_wave_mc_kernel, one launch) alternate, five rounds of ten calls each
between device events after a warm-up, with the single-connection calls
(net2_packet_decode_burst / _encode_burst, one key) under the same setting
beside them; net2_sha2_burst_stats confirms the form of every timed round.
The baseline is another build of the library -- the parent commit's,
--baseline, default tools/ab/parent.so -- measured the same way in a process
of its own (NET2_SHA2_LIB, NET2_SHA2_LIB_ALLOW_OLD_ABI=1); its _mc calls have
the lane form only.

"chain_mc" is what a receive loop pays: decode_burst_mc followed on the same
stream by net2_packet_decrypt_burst_mc (the cipher-key table of the same 1,024
connections, the decrypt form at its own default), on datagrams that were
encrypted and sealed by the TX calls -- their 1,500-byte slots carry 1,496
wire bytes, 89 whole AES blocks.

Before anything is timed every call runs once per form: every code OK, the
chain's plaintext lengths as encrypted, and the two forms' outputs identical.

One JSON object per (n, call, form) with the median, minimum and maximum of
the rounds, then per n a "verdict" row -- for rx_mc and tx_mc: the wave form
against the baseline's lane form and that form's own max - min spread; the
forced lane form of this build against the baseline's; the wave form's ratio
to the single-connection wave call -- and a "default" row: the largest n such
that the wave form wins both calls there and at every smaller n (0 if none),
never above the device's 16 datagrams per SIMD.

  python tools/burst_mc_sizes.py [--sizes 64,256,...] [--baseline LIB]
                                 [--out profiles/burst_mc_wave/sizes.jsonl]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [64, 256, 1024, 4096, 16384, 65536]
DGRAM = [136, 584, 1500]
ALG, HL, IVLEN = 6, 64, 16
CONNS = 1024
ROUNDS, REPS, WARMUP = 5, 10, 3
CALLS = ("rx_mc", "tx_mc", "chain_mc", "rx_one", "tx_one")


def hkey(k):
    return bytes((29 * k + 7 * j + 3) & 0xff for j in range(HL))


def ckey(k):
    return bytes((37 * k + 11 * j + 5) & 0xff for j in range(32))


def measure(sizes, baseline):
    """The rows of this process's library.  baseline: the parent's build --
    no limits are set and no form is confirmed (it has no burst stats); its
    _mc calls are the lane form."""
    import torch
    from ilias_net2_amd import _lib, cipher_burst, conn_burst
    if not torch.cuda.is_available():
        sys.exit("burst_mc_sizes: no GPU (nothing is measured without one)")
    L = _lib.lib()
    dev = torch.device("cuda:0")
    forms = [("parent", None)] if baseline else [("lane", 0), ("wave", 1 << 30)]
    calls = CALLS[:3] if baseline else CALLS
    st = torch.cuda.current_stream().cuda_stream
    tab, ctab = conn_burst.KeyTable(ALG, CONNS), cipher_burst.CipherTable(CONNS)
    for k in range(CONNS):
        tab.set_rx(k, hkey(k), enc_set=True)
        tab.set_tx(k, hkey(k), enc_set=True)
        ctab.set_rx(k, ckey(k), hash_alg=ALG)
        ctab.set_tx(k, ckey(k))

    def counts():
        a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
        L.net2_sha2_burst_stats(ctypes.byref(a), ctypes.byref(b))
        return {"lane": a.value, "wave": b.value}

    rows = []
    for n in sizes:
        g = torch.Generator(device=dev)
        g.manual_seed(41 + n)
        lens64 = torch.tensor(DGRAM, dtype=torch.int64, device=dev)[
            torch.randint(0, 3, (n,), device=dev, generator=g)]
        offs = torch.zeros(n, dtype=torch.int64, device=dev)
        offs[1:] = torch.cumsum(lens64, 0)[:-1]
        lens = lens64.to(torch.int32)
        total = int(lens64.sum())
        plain = torch.randint(0, 256, (total,), dtype=torch.uint8, device=dev, generator=g)
        seq = torch.arange(n, dtype=torch.int32, device=dev)
        flags = torch.full((n,), 3, dtype=torch.int32, device=dev)
        conn = torch.randint(0, CONNS, (n,), dtype=torch.int32, device=dev, generator=g)
        ws = conn_burst.burst_workspace(n, dev)
        W = (ws.data_ptr(), ws.numel(), st)
        many, one, chain = plain.clone(), plain.clone(), plain.clone()
        res = torch.full((n,), 9, dtype=torch.uint8, device=dev)
        iv = torch.zeros((n, IVLEN), dtype=torch.uint8, device=dev)
        oseq = torch.zeros(n, dtype=torch.int32, device=dev)
        ofl = torch.zeros(n, dtype=torch.int32, device=dev)
        # the chain's datagrams: encrypted under the IV of their header, then
        # sealed; plaintext one byte short of whole blocks
        ct = ((lens64 - 8 - HL) // 16) * 16
        plen = (ct - 1).to(torch.int32)
        tiv = torch.zeros((n, IVLEN), dtype=torch.uint8, device=dev)
        _lib.check(L.net2_ph_to_iv_dev(seq.data_ptr(), flags.data_ptr(), n, IVLEN,
                                       tiv.data_ptr(), st), "ph_to_iv")
        eres, wire = cipher_burst.encrypt_burst_mc(ctab, conn, HL, flags, tiv, chain, offs,
                                                   lens, plen)
        assert int(eres.sum()) == 0 and torch.equal(wire.to(torch.int64), ct + 8 + HL)
        dec = torch.empty_like(chain)
        got = torch.zeros(n, dtype=torch.int32, device=dev)
        head = (tab.ptr, conn.data_ptr())
        tx_in = (seq.data_ptr(), flags.data_ptr())
        geo = (offs.data_ptr(), lens.data_ptr(), n)
        outs = (res.data_ptr(), iv.data_ptr(), oseq.data_ptr(), ofl.data_ptr())
        # the C entry points themselves, arguments made once: the host's share
        # of a call stays below the shortest burst's device time
        argv = {
            "rx_mc": (L.net2_packet_decode_burst_mc,
                      head + (IVLEN, many.data_ptr()) + geo + outs + W),
            "tx_mc": (L.net2_packet_encode_burst_mc,
                      head + tx_in + (many.data_ptr(),) + geo + (res.data_ptr(),) + W),
            "rx_one": (L.net2_packet_decode_burst,
                       (ALG, hkey(0), HL, 1, IVLEN, one.data_ptr()) + geo + outs + W),
            "tx_one": (L.net2_packet_encode_burst,
                       (ALG, hkey(0), HL, 1) + tx_in + (one.data_ptr(),) + geo +
                       (res.data_ptr(),) + W),
            "chain_rx": (L.net2_packet_decode_burst_mc,
                         head + (IVLEN, chain.data_ptr(), offs.data_ptr(), wire.data_ptr(),
                                 n) + outs + W),
            "chain_tx": (L.net2_packet_encode_burst_mc,
                         head + tx_in + (chain.data_ptr(), offs.data_ptr(), wire.data_ptr(),
                                         n, res.data_ptr()) + W),
            "chain_dec": (L.net2_packet_decrypt_burst_mc,
                          (ctab.ptr, conn.data_ptr(), HL, chain.data_ptr(), offs.data_ptr(),
                           wire.data_ptr(), n, oseq.data_ptr(), ofl.data_ptr(),
                           iv.data_ptr(), res.data_ptr(), dec.data_ptr(), got.data_ptr(),
                           st)),
        }

        def run(name):
            fn, a = argv[name]
            rc = fn(*a)
            if rc != 0:
                _lib.check(rc, name)

        def call(name):
            if name == "chain_mc":
                run("chain_rx")
                run("chain_dec")
            else:
                run(name)

        # once per form, checked, and the forms against each other
        seen = []
        for form, limit in forms:
            if limit is not None:
                L.net2_sha2_burst_limits(limit, -1)
            many.copy_(plain)
            one.copy_(plain)
            state = []
            for name in ("tx_mc", "rx_mc", "tx_one", "rx_one", "chain_tx", "chain_mc"):
                if name.endswith("_one") and baseline:
                    continue
                res.fill_(9)
                for t in (iv, oseq, ofl):
                    t.zero_()
                call(name)
                torch.cuda.synchronize()
                assert int(res.sum()) == 0, (n, name, form, "a datagram was refused")
                state += [iv.clone(), oseq.clone(), ofl.clone()]
            assert torch.equal(got, plen), (n, form, "plaintext lengths")
            seen.append(state + [many.clone(), one.clone(), chain.clone()])
            for name in calls:
                for _ in range(WARMUP):
                    call(name)
        for other in seen[1:]:
            assert all(torch.equal(a, b) for a, b in zip(seen[0], other)), (n, "forms differ")
        del seen
        torch.cuda.synchronize()
        us = {(name, form): [] for name in calls for form, _ in forms}
        for _ in range(ROUNDS):
            for form, limit in forms:
                if limit is not None:
                    L.net2_sha2_burst_limits(limit, -1)
                for name in calls:
                    before = None if baseline else counts()
                    t0 = torch.cuda.Event(enable_timing=True)
                    t1 = torch.cuda.Event(enable_timing=True)
                    t0.record()
                    for _ in range(REPS):
                        call(name)
                    t1.record()
                    t1.synchronize()
                    us[name, form].append(t0.elapsed_time(t1) * 1e3 / REPS)
                    if before is not None:
                        after = counts()
                        took = {k: after[k] - before[k] for k in after}
                        assert took == {form: REPS, "wave" if form == "lane" else "lane": 0}, \
                            (n, name, form, took)
        for name in calls:
            for form, _ in forms:
                v = us[name, form]
                rows.append({"kind": "time", "n": n, "call": name,
                             "form": "parent_lane" if baseline else form,
                             "median_us": round(statistics.median(v), 2),
                             "min_us": round(min(v), 2), "max_us": round(max(v), 2),
                             "rounds_us": [round(x, 2) for x in v], "reps": REPS,
                             "bytes": total, "conns": CONNS, "hash": "HMAC-SHA512",
                             "device": torch.cuda.get_device_name(0),
                             "build_id": L.net2_sha2_build_id().decode()})
                print(json.dumps(rows[-1]), flush=True)
        del many, one, chain, plain, dec
    if not baseline:
        L.net2_sha2_burst_limits(-1, -1)
        simds = 4 * torch.cuda.get_device_properties(0).multi_processor_count
        rows.append({"kind": "device", "simds": simds, "wave_max_single": 16 * simds})
    tab.close()
    ctab.close()
    return rows


def verdicts(rows, sizes):
    """Per n: does the wave form beat the baseline's lane form by more than
    that form's own spread, for RX and TX; and the default that follows."""
    at = {(r["n"], r["call"], r["form"]): r for r in rows if r["kind"] == "time"}
    cap = next((r["wave_max_single"] for r in rows if r["kind"] == "device"), None)
    out, default, unbroken = [], 0, True
    for n in sorted(sizes):
        v = {"kind": "verdict", "n": n}
        wins = True
        for call in ("rx_mc", "tx_mc", "chain_mc"):
            p, w, ln = (at.get((n, call, f)) for f in ("parent_lane", "wave", "lane"))
            if p is None or w is None or ln is None:
                return out + [{"kind": "default", "mc_wave_max": None,
                               "note": "no baseline measured: no default follows"}]
            spread = p["max_us"] - p["min_us"]
            gain = p["median_us"] - w["median_us"]
            v[call] = {"parent_lane_us": p["median_us"], "parent_spread_us": round(spread, 2),
                       "wave_us": w["median_us"], "wave_gain_us": round(gain, 2),
                       "wave_wins": gain > spread, "lane_us": ln["median_us"],
                       "lane_minus_parent_us": round(ln["median_us"] - p["median_us"], 2),
                       "lane_within_parent_spread":
                           abs(ln["median_us"] - p["median_us"]) <= spread}
            single = at.get((n, call.replace("_mc", "_one"), "wave"))
            if single is not None:
                v[call]["single_wave_us"] = single["median_us"]
                v[call]["wave_over_single_wave"] = round(w["median_us"] /
                                                         single["median_us"], 3)
            if call != "chain_mc":          # the chain is reported, not decided on
                wins = wins and gain > spread
        v["wave_wins_rx_and_tx"] = wins
        unbroken = unbroken and wins
        if unbroken:
            default = n
        out.append(v)
    capped = default if cap is None else min(default, cap)
    out.append({"kind": "default", "largest_n_wave_ahead": default, "device_wave_max": cap,
                "mc_wave_max": capped,
                "note": "the wave form up to the largest measured n with it ahead there "
                        "and at every smaller measured n, never above the device's 16 "
                        "datagrams per SIMD" if default else
                        "the wave form is not ahead at the smallest size: never taken"})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=",".join(map(str, SIZES)))
    ap.add_argument("--baseline", default=os.path.join(ROOT, "tools", "ab", "parent.so"),
                    help="the parent commit's libnet2_sha2.so")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "burst_mc_wave",
                                                  "sizes.jsonl"))
    ap.add_argument("--role", default="main", choices=["main", "baseline"])
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]
    if args.role == "baseline":
        measure(sizes, True)
        return
    rows = []
    if os.path.exists(args.baseline):
        # a process of its own: one library per process
        env = dict(os.environ, NET2_SHA2_LIB=os.path.abspath(args.baseline),
                   NET2_SHA2_LIB_ALLOW_OLD_ABI="1")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--role",
                            "baseline", "--sizes", args.sizes], env=env, text=True,
                           stdout=subprocess.PIPE, timeout=900)
        if r.returncode != 0:
            sys.exit(f"burst_mc_sizes: the baseline run failed ({r.returncode})")
        rows = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
        for row in rows:
            print(json.dumps(row), flush=True)
    else:
        print(f"burst_mc_sizes: {args.baseline} is missing: no baseline, no default",
              file=sys.stderr)
    rows += measure(sizes, False)
    tail = verdicts(rows, sizes)
    for row in tail:
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows + tail:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
