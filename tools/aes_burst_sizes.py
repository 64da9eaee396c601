#!/usr/bin/env python3
"""Cipher bursts by burst size, in both forms of a direction (DESIGN.md 5.5.5
RX, 5.5.7 TX).

--direction rx (the default): net2_packet_decrypt_burst (one key) and
net2_packet_decrypt_burst_mc (1,024 connections' keys from the cipher-key
table) over n device-resident datagrams, n in {64, 256, 1,024, 4,096, 16,384,
65,536, 262,144, 1 M}: unsigned wire datagrams with an AES-256-CBC payload of
{64, 512, 1424} B (the mix of DESIGN.md 5.5.3), out of place.  In this process
the lane form (net2_aes_burst_limits(0): one lane per datagram) and the wave
form (2^30: one wave per datagram) alternate, five rounds of ten calls each
between device events after a warm-up; net2_aes_burst_stats confirms the form
of every round.

--direction tx: net2_packet_encrypt_burst and net2_packet_encrypt_burst_mc
over the same slots, in place (what a timed call encrypts is the call
before's ciphertext: the same lengths, the same work), the lane form
(net2_aes_encrypt_limits(0)) and the quad form (2^30: four lanes per
datagram) alternating the same way, net2_aes_encrypt_stats the witness.

The baseline is another build of the library -- the parent commit's,
--baseline, default tools/ab/parent.so -- measured the same way in a process
of its own (NET2_SHA2_LIB); it has the lane form only.

Before anything is timed the burst goes through each form once: every code
OK, every length as expected, the forms' outputs identical, and the last
datagram's plaintext back after the other direction.

One JSON object per (n, call, form) with the median, minimum and maximum of
the rounds, then per n a "verdict" row -- the wave / quad form beats the
baseline's lane form by more than that form's own max - min spread, for both
calls; the forced lane form of this build against the baseline's -- and a
"default" row: the largest n such that the verdict holds there and at every
smaller n (0 if none).  That n is net2_dgram.cpp's AES_WAVE_MAX_DEFAULT (rx)
or AES_QUAD_MAX_DEFAULT (tx).

  python tools/aes_burst_sizes.py [--direction rx|tx] [--sizes 64,256,...]
                                  [--baseline LIB] [--out FILE]
  (--out defaults to profiles/aes_burst_wave/sizes.jsonl for rx and
  profiles/aes_burst_quad/sizes.jsonl for tx)
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
# per direction: the second form's name, the limits and stats calls, the
# default --out directory
DIRECTIONS = {
    "rx": ("wave", "net2_aes_burst_limits", "net2_aes_burst_stats", "aes_burst_wave"),
    "tx": ("quad", "net2_aes_encrypt_limits", "net2_aes_encrypt_stats", "aes_burst_quad"),
}


def key_of(k):
    return bytes((37 * k + 11 * j + 5) & 0xff for j in range(32))


def measure(sizes, baseline, direction):
    """The rows of this process's library.  baseline: it has no limits call
    for this direction (the parent's build); only its one form is timed."""
    import torch
    from ilias_net2_amd import _lib, cipher_burst
    if not torch.cuda.is_available():
        sys.exit("aes_burst_sizes: no GPU (nothing is measured without one)")
    L = _lib.lib()
    dev = torch.device("cuda:0")
    alt, limits_name, stats_name, _ = DIRECTIONS[direction]
    forms = [("parent_lane", None)] if baseline else [("lane", 0), (alt, 1 << 30)]
    set_limit = None if baseline else getattr(L, limits_name)
    st = torch.cuda.current_stream().cuda_stream
    kb = ctypes.create_string_buffer(key_of(0), 32)
    ck = _lib.BurstCipherKeys(_lib.ENC_AES256, ctypes.cast(kb, ctypes.c_void_p), 32,
                              None, 0)
    rk = _lib.BurstRxKeys(0, None, 0, 1, None, 0, 0, 0, 0)
    tab = cipher_burst.CipherTable(CONNS)
    for k in range(CONNS):
        tab.set_tx(k, key_of(k))
        tab.set_rx(k, key_of(k))

    def counts():
        a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
        getattr(L, stats_name)(ctypes.byref(a), ctypes.byref(b))
        return {"lane": a.value, alt: b.value}

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
        a = int(offs[n - 1]) + PO
        last = slice(a, a + int(plen[n - 1]))
        for call in ("one", "mc"):
            d_res = torch.zeros(n, dtype=torch.uint8, device=dev)
            got = torch.zeros(n, dtype=torch.int32, device=dev)
            sealed = clear.clone()
            # the C entry points themselves, arguments made once: the host's
            # share of a call stays below the shortest burst's device time
            if direction == "rx":
                if call == "one":
                    res, wire = cipher_burst.encrypt_burst(key_of(0), 0, flags, iv, sealed,
                                                           offs, lens, plen)
                else:
                    res, wire = cipher_burst.encrypt_burst_mc(tab, conn, 0, flags, iv,
                                                              sealed, offs, lens, plen)
                assert int(res.sum()) == 0 and torch.equal(wire, lens), (n, call, "tx")
                ptrs = [t.data_ptr() for t in (sealed, offs, lens)] + [n] + [
                    t.data_ptr() for t in (seq, flags, iv, d_res, out, got)] + [st]
                if call == "one":
                    fn, head = L.net2_packet_decrypt_burst, [ctypes.byref(rk),
                                                             ctypes.byref(ck)]
                else:
                    fn, head = L.net2_packet_decrypt_burst_mc, [tab.ptr, conn.data_ptr(), 0]
                want_got, result = plen, out
            else:
                ptrs = [t.data_ptr() for t in (flags, iv, sealed, offs, lens, plen)] + [n] + [
                    d_res.data_ptr(), got.data_ptr(), st]
                if call == "one":
                    fn, head = L.net2_packet_encrypt_burst, [ctypes.byref(ck), 0]
                else:
                    fn, head = L.net2_packet_encrypt_burst_mc, [tab.ptr, conn.data_ptr(), 0]
                want_got, result = lens, sealed
            argv = head + ptrs

            def run():
                rc = fn(*argv)
                if rc != 0:
                    _lib.check(rc, fn.__name__)

            # once per form, checked, and the forms against each other
            outs = []
            for form, limit in forms:
                if limit is not None:
                    set_limit(limit)
                if direction == "rx":
                    out.fill_(0xA5)
                else:
                    sealed.copy_(clear)
                run()
                torch.cuda.synchronize()
                assert int(d_res.sum()) == 0 and torch.equal(got, want_got), (n, call, form)
                outs.append(result.clone())
                for _ in range(WARMUP):
                    run()
            assert all(torch.equal(outs[0], o) for o in outs[1:]), (n, call, "forms differ")
            if direction == "tx":
                # back through the decrypt burst: the last slot's plaintext
                zero = torch.zeros(n, dtype=torch.uint8, device=dev)
                if call == "one":
                    r = cipher_burst.decrypt_burst(0, key_of(0), outs[0], offs, lens, seq,
                                                   flags, iv, zero)
                else:
                    r = cipher_burst.decrypt_burst_mc(tab, conn, 0, outs[0], offs, lens,
                                                      seq, flags, iv, zero)
                assert int(r[0].sum()) == 0 and torch.equal(r[2], plen), (n, call, "rx")
                outs[0] = r[1]
            assert torch.equal(outs[0][last], clear[last]), (n, call, "plaintext")
            del outs
            torch.cuda.synchronize()
            us = {form: [] for form, _ in forms}
            for _ in range(ROUNDS):
                for form, limit in forms:
                    if limit is not None:
                        set_limit(limit)
                        before = counts()
                    t0 = torch.cuda.Event(enable_timing=True)
                    t1 = torch.cuda.Event(enable_timing=True)
                    t0.record()
                    for _ in range(REPS):
                        run()
                    t1.record()
                    t1.synchronize()
                    us[form].append(t0.elapsed_time(t1) * 1e3 / REPS)
                    if limit is not None:
                        after = counts()
                        assert after[form] - before[form] == REPS, (form, before, after)
            for form, _ in forms:
                v = us[form]
                rows.append({"kind": "time", "direction": direction, "n": n, "call": call,
                             "form": form,
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
        set_limit(-1)
    tab.close()
    return rows


def verdicts(rows, sizes, alt):
    """Per n: does the `alt` form (wave or quad) win by more than the
    baseline's spread, for both calls; and the default that follows."""
    at = {(r["n"], r["call"], r["form"]): r for r in rows if r["kind"] == "time"}
    out, default, unbroken = [], 0, True
    for n in sorted(sizes):
        v = {"kind": "verdict", "n": n}
        wins = True
        for call in ("one", "mc"):
            p, w, ln = (at.get((n, call, f)) for f in ("parent_lane", alt, "lane"))
            if p is None or w is None or ln is None:
                return out + [{"kind": "default", f"{alt}_max": None,
                               "note": "no baseline measured: no default follows"}]
            spread = p["max_us"] - p["min_us"]
            gain = p["median_us"] - w["median_us"]
            v[call] = {"parent_lane_us": p["median_us"], "parent_spread_us": round(spread, 2),
                       f"{alt}_us": w["median_us"], f"{alt}_gain_us": round(gain, 2),
                       f"{alt}_wins": gain > spread, "lane_us": ln["median_us"],
                       "lane_minus_parent_us": round(ln["median_us"] - p["median_us"], 2),
                       "lane_within_parent_spread":
                           abs(ln["median_us"] - p["median_us"]) <= spread}
            wins = wins and gain > spread
        v[f"{alt}_wins_both_calls"] = wins
        unbroken = unbroken and wins
        if unbroken:
            default = n
        out.append(v)
    out.append({"kind": "default", f"{alt}_max": default,
                "note": f"largest measured n with the {alt} form ahead at it and at "
                        "every smaller measured n" if default else
                        f"the {alt} form is not ahead at the smallest size: never taken"})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--direction", default="rx", choices=sorted(DIRECTIONS))
    ap.add_argument("--sizes", default=",".join(map(str, SIZES)))
    ap.add_argument("--baseline", default=os.path.join(ROOT, "tools", "ab", "parent.so"),
                    help="the parent commit's libnet2_sha2.so")
    ap.add_argument("--out", default=None)
    ap.add_argument("--role", default="main", choices=["main", "baseline"])
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]
    alt, _, _, out_dir = DIRECTIONS[args.direction]
    out_path = args.out or os.path.join(ROOT, "profiles", out_dir, "sizes.jsonl")
    if args.role == "baseline":
        measure(sizes, True, args.direction)
        return
    rows = []
    if os.path.exists(args.baseline):
        # a process of its own: one library per process
        env = dict(os.environ, NET2_SHA2_LIB=os.path.abspath(args.baseline),
                   NET2_SHA2_LIB_ALLOW_OLD_ABI="1")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--role",
                            "baseline", "--direction", args.direction, "--sizes",
                            args.sizes], env=env, text=True,
                           stdout=subprocess.PIPE, timeout=900)
        if r.returncode != 0:
            sys.exit(f"aes_burst_sizes: the baseline run failed ({r.returncode})")
        rows = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
        for row in rows:
            print(json.dumps(row), flush=True)
    else:
        print(f"aes_burst_sizes: {args.baseline} is missing: no baseline, no default",
              file=sys.stderr)
    rows += measure(sizes, False, args.direction)
    tail = verdicts(rows, sizes, alt)
    for row in tail:
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        for row in rows + tail:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
