#!/usr/bin/env python3
"""RX decrypt bursts by burst size, in both forms.

net2_packet_decrypt_burst (one key) and net2_packet_decrypt_burst_mc (1,024
connections' keys from the cipher-key table) over n device-resident
datagrams, n in {64, 256, 1,024, 4,096, 16,384, 65,536, 262,144, 1 M}:
unsigned wire datagrams with an AES-256-CBC payload of {64, 512, 1424} B (the
mix of DESIGN.md 5.5.3), out of place.  In this process the lane form
(net2_aes_burst_limits(0): one lane per datagram) and the wave form (2^30: one
wave per datagram) alternate, five rounds of ten calls each between device
events after a warm-up; net2_aes_burst_stats confirms the form of every
round.  The baseline is another build of the library -- the parent commit's,
--baseline, default tools/ab/parent.so -- measured the same way in a process
of its own (NET2_SHA2_LIB); it has the lane form only.

Before anything is timed the burst is decrypted once per form: every code OK,
every length as encrypted, and the two forms' outputs identical.

One JSON object per (n, call, form) with the median, minimum and maximum of
the rounds, then per n a "verdict" row -- the wave form beats the baseline's
lane form by more than that form's own max - min spread, for both calls; the
forced lane form of this build against the baseline's -- and a "default" row:
the largest n such that the verdict holds there and at every smaller n (0 if
none).  That n is net2_dgram.cpp's AES_WAVE_MAX_DEFAULT.

  python tools/aes_burst_sizes.py [--sizes 64,256,...] [--baseline LIB]
                                  [--out profiles/aes_burst_wave/sizes.jsonl]
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

SIZES = [64, 256, 1024, 4096, 16384, 65536, 262144, 1 << 20]
CLEN = [64, 512, 1424]          # ciphertext bytes: 4, 32 and 89 blocks
PO = 8                          # unsigned: the payload follows the header
CONNS = 1024
ROUNDS, REPS, WARMUP = 5, 10, 3
ENC = 1


def key_of(k):
    return bytes((37 * k + 11 * j + 5) & 0xff for j in range(32))


def measure(sizes, baseline):
    """The rows of this process's library.  baseline: it has no limits call
    (the parent's build); only its one form is timed."""
    import torch
    from ilias_net2_amd import _lib, cipher_burst
    if not torch.cuda.is_available():
        sys.exit("aes_burst_sizes: no GPU (nothing is measured without one)")
    L = _lib.lib()
    dev = torch.device("cuda:0")
    forms = [("parent_lane", None)] if baseline else [("lane", 0), ("wave", 1 << 30)]
    st = torch.cuda.current_stream().cuda_stream
    kb = ctypes.create_string_buffer(key_of(0), 32)
    ck = _lib.BurstCipherKeys(_lib.ENC_AES256, ctypes.cast(kb, ctypes.c_void_p), 32,
                              None, 0)
    rk = _lib.BurstRxKeys(0, None, 0, 1, None, 0, 0, 0, 0)
    tab = cipher_burst.CipherTable(CONNS)
    for k in range(CONNS):
        tab.set_tx(k, key_of(k))
        tab.set_rx(k, key_of(k))
    rows = []
    for n in sizes:
        g = torch.Generator(device=dev)
        g.manual_seed(31 + n)
        clen = torch.tensor(CLEN, dtype=torch.int64, device=dev)[
            torch.randint(0, 3, (n,), device=dev, generator=g)]
        lens64 = clen + PO
        offs = torch.zeros(n, dtype=torch.int64, device=dev)
        offs[1:] = torch.cumsum(lens64, 0)[:-1]
        lens = lens64.to(torch.int32)
        plen = (clen - 1).to(torch.int32)       # one byte of padding
        total = int(lens64.sum())
        clear = torch.randint(0, 256, (total,), dtype=torch.uint8, device=dev, generator=g)
        flags = torch.full((n,), ENC, dtype=torch.int32, device=dev)
        seq = torch.arange(n, dtype=torch.int32, device=dev)
        conn = torch.randint(0, CONNS, (n,), dtype=torch.int32, device=dev, generator=g)
        iv = torch.randint(0, 256, (n, 16), dtype=torch.uint8, device=dev, generator=g)
        out = torch.empty_like(clear)
        for call in ("one", "mc"):
            sealed = clear.clone()
            if call == "one":
                res, wire = cipher_burst.encrypt_burst(key_of(0), 0, flags, iv, sealed,
                                                       offs, lens, plen)
            else:
                res, wire = cipher_burst.encrypt_burst_mc(tab, conn, 0, flags, iv, sealed,
                                                          offs, lens, plen)
            assert int(res.sum()) == 0 and torch.equal(wire, lens), (n, call, "tx")
            d_res = torch.zeros(n, dtype=torch.uint8, device=dev)
            got = torch.zeros(n, dtype=torch.int32, device=dev)
            # the C entry points themselves, arguments made once: the host's
            # share of a call stays below the shortest burst's device time
            ptrs = [t.data_ptr() for t in (sealed, offs, lens)] + [n] + [
                t.data_ptr() for t in (seq, flags, iv, d_res, out, got)] + [st]
            if call == "one":
                fn, head = L.net2_packet_decrypt_burst, [ctypes.byref(rk), ctypes.byref(ck)]
            else:
                fn, head = L.net2_packet_decrypt_burst_mc, [tab.ptr, conn.data_ptr(), 0]
            argv = head + ptrs

            def rx():
                rc = fn(*argv)
                if rc != 0:
                    _lib.check(rc, fn.__name__)
                return None, None, got

            def counts():
                a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
                L.net2_aes_burst_stats(ctypes.byref(a), ctypes.byref(b))
                return {"lane": a.value, "wave": b.value}

            # once per form, checked, and the forms against each other
            outs = []
            for form, limit in forms:
                if limit is not None:
                    L.net2_aes_burst_limits(limit)
                out.fill_(0xA5)
                _, _, got = rx()
                torch.cuda.synchronize()
                assert int(d_res.sum()) == 0 and torch.equal(got, plen), (n, call, form)
                outs.append(out.clone())
                for _ in range(WARMUP):
                    rx()
            assert all(torch.equal(outs[0], o) for o in outs[1:]), (n, call, "forms differ")
            a = int(offs[n - 1]) + PO
            assert torch.equal(outs[0][a:a + int(plen[n - 1])],
                               clear[a:a + int(plen[n - 1])]), (n, call, "plaintext")
            del outs
            torch.cuda.synchronize()
            us = {form: [] for form, _ in forms}
            for _ in range(ROUNDS):
                for form, limit in forms:
                    if limit is not None:
                        L.net2_aes_burst_limits(limit)
                        before = counts()
                    t0 = torch.cuda.Event(enable_timing=True)
                    t1 = torch.cuda.Event(enable_timing=True)
                    t0.record()
                    for _ in range(REPS):
                        rx()
                    t1.record()
                    t1.synchronize()
                    us[form].append(t0.elapsed_time(t1) * 1e3 / REPS)
                    if limit is not None:
                        after = counts()
                        assert after[form] - before[form] == REPS, (form, before, after)
            for form, _ in forms:
                v = us[form]
                rows.append({"kind": "time", "n": n, "call": call, "form": form,
                             "median_us": round(statistics.median(v), 2),
                             "min_us": round(min(v), 2), "max_us": round(max(v), 2),
                             "rounds_us": [round(x, 2) for x in v], "reps": REPS,
                             "payload_bytes": int(clen.sum()),
                             "device": torch.cuda.get_device_name(0),
                             "build_id": L.net2_sha2_build_id().decode()})
                print(json.dumps(rows[-1]), flush=True)
            del sealed
        del clear, out
    if not baseline:
        L.net2_aes_burst_limits(-1)
    tab.close()
    return rows


def verdicts(rows, sizes):
    """Per n: does the wave form win by more than the baseline's spread, for
    both calls; and the default that follows."""
    at = {(r["n"], r["call"], r["form"]): r for r in rows if r["kind"] == "time"}
    out, default, unbroken = [], 0, True
    for n in sorted(sizes):
        v = {"kind": "verdict", "n": n}
        wins = True
        for call in ("one", "mc"):
            p, w, ln = (at.get((n, call, f)) for f in ("parent_lane", "wave", "lane"))
            if p is None or w is None or ln is None:
                return out + [{"kind": "default", "wave_max": None,
                               "note": "no baseline measured: no default follows"}]
            spread = p["max_us"] - p["min_us"]
            gain = p["median_us"] - w["median_us"]
            v[call] = {"parent_lane_us": p["median_us"], "parent_spread_us": round(spread, 2),
                       "wave_us": w["median_us"], "wave_gain_us": round(gain, 2),
                       "wave_wins": gain > spread, "lane_us": ln["median_us"],
                       "lane_minus_parent_us": round(ln["median_us"] - p["median_us"], 2),
                       "lane_within_parent_spread":
                           abs(ln["median_us"] - p["median_us"]) <= spread}
            wins = wins and gain > spread
        v["wave_wins_both_calls"] = wins
        unbroken = unbroken and wins
        if unbroken:
            default = n
        out.append(v)
    out.append({"kind": "default", "wave_max": default,
                "note": "largest measured n with the wave form ahead at it and at "
                        "every smaller measured n" if default else
                        "the wave form is not ahead at the smallest size: never taken"})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=",".join(map(str, SIZES)))
    ap.add_argument("--baseline", default=os.path.join(ROOT, "tools", "ab", "parent.so"),
                    help="the parent commit's libnet2_sha2.so")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aes_burst_wave",
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
            sys.exit(f"aes_burst_sizes: the baseline run failed ({r.returncode})")
        rows = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
        for row in rows:
            print(json.dumps(row), flush=True)
    else:
        print(f"aes_burst_sizes: {args.baseline} is missing: no baseline, no default",
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
