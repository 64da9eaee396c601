#!/usr/bin/env python3
"""ECDSA P-521 verification from prepared key tables beside the bit-by-bit
kernel and the host threads (net2/ecdsa_key.h; the method of ecdsa_rates.py).

For each n: SHA-512 digests and valid signatures (pools of OpenSSL-signed
messages tiled to n), under one key and under 1,024 keys picked at random per
signature.  One JSON object per row:

  keytab_1key / keytab_1024keys    net2_ecdsa_p521_verify_keytab_dev, device events
  bitwise_1key / bitwise_1024keys  net2_ecdsa_p521_verify_dev on the same
                                   inputs (one shared key; the keys gathered per
                                   signature): the comparison, unchanged code
  sig_batch_dev / sig_batch_dev_prepared
                                   net2x_signature_validate_batch_dev over n signed
                                   1 KiB payloads, before and after
                                   net2x_signctx_prepare_dev, wall time
  cpu_16                           net2x_signature_validate_batch on 16 host
                                   threads (GPU hash, OpenSSL verification)
  prepare_K                        net2_ecdsa_p521_keytab_prepare_dev for K keys
                                   (n = K), device events

Every row is the median of `--rounds` rounds with min and max; within a round
the calls run in an order that rotates from round to round.  Before anything
is timed every verdict is checked (all 1, and 0 for a corrupted copy).  The
last row compares: per n the ratio keytab / bitwise, whether the gain exceeds
the spread of the bit-by-bit kernel's own rounds, how many calls (and, at the
largest n, how many signatures) under a key repay its prepare, and the
smallest n at which each device call beat the 16-thread host call.

  python tools/ecdsa_keytab_rates.py [--sizes 64,1024,...] [--rounds 5] [--out FILE]
"""
import argparse
import ctypes
import hashlib
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ecdsa_ref  # noqa: E402
from ilias_net2_amd import _lib, ecdsa, ecdsa_key  # noqa: E402

POOL = 256
MANY = 1024
vp = ctypes.c_void_p


class Signature(ctypes.Structure):
    _fields_ = [("sign_alg", vp), ("hash_alg", vp), ("data", vp),
                ("datalen", ctypes.c_size_t)]


def sign_lib():
    _lib.lib()
    S = ctypes.CDLL(os.path.join(ROOT, "ilias_net2_amd", "libnet2_sign.so"))
    for name in ("net2x_signctx_pubnew", "net2x_signctx_privnew"):
        getattr(S, name).restype = vp
        getattr(S, name).argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
    S.net2x_signctx_prepare_dev.argtypes = [vp]
    S.net2x_signature_create_batch.argtypes = [
        ctypes.POINTER(Signature), vp, vp, vp, ctypes.c_size_t, ctypes.c_int, vp,
        ctypes.c_int]
    S.net2x_signature_validate_batch.argtypes = [
        ctypes.POINTER(Signature), vp, vp, vp, ctypes.c_size_t, vp, vp, ctypes.c_int]
    S.net2x_signature_validate_batch_dev.argtypes = [
        ctypes.POINTER(Signature), vp, vp, vp, ctypes.c_size_t, vp, vp]
    return S


def pool(nkeys: int, count: int):
    """count valid signatures over SHA-512 digests, signature i under key
    i % nkeys: (keys (nkeys x 132), rs, digests, key index)."""
    rng = random.Random(nkeys)
    ds = [rng.randrange(1, ecdsa_ref.order()) for _ in range(nkeys)]
    cases = []
    for i in range(count):
        dig = hashlib.sha512(b"rate %d/%d" % (nkeys, i)).digest()
        r, s = ecdsa_ref.sign(ds[i % nkeys], dig)
        cases.append((ecdsa_ref.public_key(ds[i % nkeys]), r, s, dig, 1))
    _, rs, dig, _, _ = ecdsa_ref.pack(cases, 64)
    keys = np.stack([np.frombuffer(ecdsa_ref.public_key(d), dtype=np.uint8) for d in ds])
    return keys, rs, dig, np.arange(count, dtype=np.int32) % nkeys


def timed(fn):
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def rounds_of(fns, rounds):
    names = list(fns)
    for name in names:              # warm-up, once each
        fns[name]()
    ms = {name: [] for name in names}
    for rnd in range(rounds):
        k = rnd % len(names)
        for name in names[k:] + names[:k]:
            ms[name].append(fns[name]())
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,1024,4096,16384,65536,262144")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sizes = [int(x) for x in args.sizes.split(",")]
    dev = torch.device("cuda:0")
    S = sign_lib()
    with open(os.path.join(ROOT, "tests/golden/keys/ecdsa_p521_priv.pem"), "rb") as f:
        pem = f.read()
    priv = S.net2x_signctx_privnew(0, pem, len(pem))
    with open(os.path.join(ROOT, "tests/golden/keys/ecdsa_p521_pub.pem"), "rb") as f:
        pem = f.read()
    pub = S.net2x_signctx_pubnew(0, pem, len(pem))
    pub_prep = S.net2x_signctx_pubnew(0, pem, len(pem))
    assert priv and pub and pub_prep
    assert S.net2x_signctx_prepare_dev(pub_prep) == 0
    pools = {1: pool(1, POOL), MANY: pool(MANY, MANY)}
    plen = 1024
    pdata = np.random.default_rng(3).integers(0, 256, POOL * plen, dtype=np.uint8)
    poffs = (np.arange(POOL, dtype=np.uint64) * plen)
    plens = np.full(POOL, plen, dtype=np.uint32)
    psigs = (Signature * POOL)()
    p = lambda a: a.ctypes.data  # noqa: E731
    assert S.net2x_signature_create_batch(psigs, p(pdata), p(poffs), p(plens), POOL, 3,
                                          priv, 16) == 0
    meta = {"curve": "secp521r1", "digest": "SHA512", "pool": POOL,
            "build_id": _lib.lib().net2_sha2_build_id().decode(),
            "device": torch.cuda.get_device_name(0), "rounds": args.rounds}
    out = open(args.out, "w") if args.out else None
    medians, spreads = {}, {}

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def rows(ms, n):
        for name, v in ms.items():
            med = statistics.median(v)
            medians[(name, n)], spreads[(name, n)] = med, max(v) - min(v)
            emit({**meta, "n": n, "kind": name, "ms": round(med, 4),
                  "ms_min_max": [round(min(v), 4), round(max(v), 4)],
                  "per_s": round(n / med * 1e3, 1)})

    # the prepare, for 1, 64 and 1,024 keys: tables checked against each other
    t_keys = torch.from_numpy(pools[MANY][0]).to(dev)
    keytabs, fns = {}, {}
    for k in (1, 64, MANY):
        keytabs[k] = torch.zeros(ecdsa_key.keytab_bytes(k), dtype=torch.uint8, device=dev)
        ok = torch.zeros(k, dtype=torch.uint8, device=dev)
        fns[k] = lambda k=k, ok=ok: timed(lambda: ecdsa_key.prepare_p521(
            t_keys[:k], keytab=keytabs[k], ok=ok))
        fns[k]()
        assert bool(ok.all())
    T = ecdsa_key.TABLE_BYTES
    assert torch.equal(keytabs[1], keytabs[MANY][:2 * T])
    assert torch.equal(keytabs[64], keytabs[MANY][:65 * T])
    for k, v in rounds_of({f"prepare_{k}": fns[k] for k in fns}, args.rounds).items():
        rows({k: v}, int(k.split("_")[1]))
    one_tab, _ = ecdsa_key.prepare_p521(torch.from_numpy(pools[1][0]).to(dev))

    for n in sizes:
        fns = {}
        rng = np.random.default_rng(n)
        for nkeys in (1, MANY):
            keys, rs, dig, kix = pools[nkeys]
            pick = rng.integers(0, len(rs), n) if nkeys > 1 else np.arange(n) % len(rs)
            t_rs = torch.from_numpy(np.ascontiguousarray(rs[pick])).to(dev)
            t_dig = torch.from_numpy(np.ascontiguousarray(dig[pick])).to(dev)
            t_idx = torch.from_numpy(np.ascontiguousarray(kix[pick])).to(dev)
            t_pub = (torch.from_numpy(keys[0].copy()).to(dev) if nkeys == 1 else
                     t_keys[t_idx.long()].contiguous())
            tab = one_tab if nkeys == 1 else keytabs[MANY]
            idx = None if nkeys == 1 else t_idx
            o1 = torch.zeros(n, dtype=torch.uint8, device=dev)
            o2 = torch.zeros(n, dtype=torch.uint8, device=dev)
            # verdicts first: all valid, and a corrupted copy all invalid, both ways
            assert bool(ecdsa_key.verify_p521_keytab(tab, nkeys, t_rs, t_dig, kidx=idx,
                                                     out=o1).all())
            assert bool(ecdsa.verify_p521(t_pub, t_rs, t_dig, out=o2).all())
            bad = t_dig.clone()
            bad[:, 0] ^= 1
            assert not bool(ecdsa_key.verify_p521_keytab(tab, nkeys, t_rs, bad,
                                                         kidx=idx).any())
            tag = f"{nkeys}key" + ("s" if nkeys > 1 else "")
            fns["keytab_" + tag] = lambda a=tab, k=nkeys, b=t_rs, c=t_dig, i=idx, o=o1: \
                timed(lambda: ecdsa_key.verify_p521_keytab(a, k, b, c, kidx=i, out=o))
            fns["bitwise_" + tag] = lambda a=t_pub, b=t_rs, c=t_dig, o=o2: \
                timed(lambda: ecdsa.verify_p521(a, b, c, out=o))
        reps = (n + POOL - 1) // POOL
        data = np.tile(pdata, reps)[:n * plen]
        offs = np.arange(n, dtype=np.uint64) * plen
        lens = np.full(n, plen, dtype=np.uint32)
        sigs = (Signature * n)()
        for i in range(n):
            sigs[i] = psigs[i % POOL]
        valid = np.zeros(n, dtype=np.int32)

        def wall(call):
            t0 = time.perf_counter()
            rc = call()
            dt = (time.perf_counter() - t0) * 1e3
            assert rc == 0 and valid.all()
            return dt
        fns["sig_batch_dev"] = lambda: wall(lambda: S.net2x_signature_validate_batch_dev(
            sigs, p(data), p(offs), p(lens), n, pub, p(valid)))
        fns["sig_batch_dev_prepared"] = lambda: wall(
            lambda: S.net2x_signature_validate_batch_dev(
                sigs, p(data), p(offs), p(lens), n, pub_prep, p(valid)))
        fns["cpu_16"] = lambda: wall(lambda: S.net2x_signature_validate_batch(
            sigs, p(data), p(offs), p(lens), n, pub, p(valid), 16))
        rows(rounds_of(fns, args.rounds), n)

    compare = []
    for n in sizes:
        for tag in ("1key", f"{MANY}keys"):
            kt, bw = medians[("keytab_" + tag, n)], medians[("bitwise_" + tag, n)]
            compare.append({
                "n": n, "keys": tag, "keytab_ms": round(kt, 4), "bitwise_ms": round(bw, 4),
                "ratio": round(kt / bw, 4),
                "bitwise_spread_ms": round(spreads[("bitwise_" + tag, n)], 4),
                "faster_by_more_than_spread": bw - kt > spreads[("bitwise_" + tag, n)]})
    big = max(sizes)
    per_sig = (medians[("bitwise_1key", big)] - medians[("keytab_1key", big)]) / big
    per_key = medians[(f"prepare_{MANY}", MANY)] / MANY
    repay = {
        "prepare_1_ms": round(medians[("prepare_1", 1)], 4),
        "prepare_per_key_of_1024_ms": round(per_key, 4),
        "calls_to_repay_one_prepare": {
            str(n): round(medians[("prepare_1", 1)] /
                          (medians[("bitwise_1key", n)] - medians[("keytab_1key", n)]), 2)
            for n in sizes if medians[("bitwise_1key", n)] > medians[("keytab_1key", n)]},
        "signatures_to_repay_a_key_at_n_max": {
            "prepared_alone": round(medians[("prepare_1", 1)] / per_sig) if per_sig > 0
            else None,
            "prepared_among_1024": round(per_key / per_sig) if per_sig > 0 else None}}
    cross = {}
    for kind in ("keytab_1key", f"keytab_{MANY}keys", "bitwise_1key", "sig_batch_dev",
                 "sig_batch_dev_prepared"):
        wins = [n for n in sizes if medians[(kind, n)] < medians[("cpu_16", n)]]
        cross[kind] = min(wins) if wins else None
    emit({**meta, "kind": "summary", "compare": compare, "repay": repay,
          "reference": "cpu_16", "smallest_n_faster_than_reference": cross})
    if out:
        out.close()


if __name__ == "__main__":
    main()
