#!/usr/bin/env python3
"""Batched ECDSA P-521 verification on the device beside the host threads.

For each n: SHA-512 digests, valid signatures (a pool of OpenSSL-signed
messages tiled to n -- the kernel's time does not depend on which valid
signature a lane holds), one shared key and per-signature keys.  One JSON
object per row:

  dev_shared / dev_perkey    net2_ecdsa_p521_verify_dev, device events
  host_shared / host_perkey  net2_ecdsa_p521_verify from host memory, wall time
  sig_batch_dev              net2x_signature_validate_batch_dev over n signed
                             1 KiB payloads (GPU hash, DER on the host, GPU
                             verification), wall time
  cpu_T                      net2x_signature_validate_batch on T host threads
                             (GPU hash, OpenSSL verification): the reference

Every row is the median of `--rounds` rounds with min and max; within a round
the calls run in an order that rotates from round to round.  Before anything
is timed every verdict is checked (all 1, and 0 for a corrupted copy).  The
last row gives the smallest n at which each device call beat the 16-thread
host call.

  python tools/ecdsa_rates.py [--sizes 64,1024,...] [--rounds 5] [--out FILE]
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
from ilias_net2_amd import _lib, ecdsa  # noqa: E402

POOL = 256
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
    S.net2x_signature_create_batch.argtypes = [
        ctypes.POINTER(Signature), vp, vp, vp, ctypes.c_size_t, ctypes.c_int, vp,
        ctypes.c_int]
    S.net2x_signature_validate_batch.argtypes = [
        ctypes.POINTER(Signature), vp, vp, vp, ctypes.c_size_t, vp, vp, ctypes.c_int]
    S.net2x_signature_validate_batch_dev.argtypes = [
        ctypes.POINTER(Signature), vp, vp, vp, ctypes.c_size_t, vp, vp]
    return S


def pool(shared: bool):
    """POOL valid signatures over SHA-512 digests as packed arrays."""
    rng = random.Random(1 if shared else 2)
    d0 = rng.randrange(1, ecdsa_ref.order())
    cases = []
    for i in range(POOL):
        d = d0 if shared else rng.randrange(1, ecdsa_ref.order())
        dig = hashlib.sha512(b"rate %d" % i).digest()
        r, s = ecdsa_ref.sign(d, dig)
        cases.append((ecdsa_ref.public_key(d), r, s, dig, 1))
    return ecdsa_ref.pack(cases, 64)


def tile(a, n):
    return np.ascontiguousarray(np.tile(a, ((n + len(a) - 1) // len(a), 1))[:n])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,1024,4096,16384,65536,262144")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threads", default="1,16")
    ap.add_argument("--cpu1-max", type=int, default=4096,
                    help="largest n the 1-thread host call is timed at")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sizes = [int(x) for x in args.sizes.split(",")]
    threads = [int(x) for x in args.threads.split(",")]
    dev = torch.device("cuda:0")
    S = sign_lib()
    with open(os.path.join(ROOT, "tests/golden/keys/ecdsa_p521_priv.pem"), "rb") as f:
        pem = f.read()
    priv = S.net2x_signctx_privnew(0, pem, len(pem))
    with open(os.path.join(ROOT, "tests/golden/keys/ecdsa_p521_pub.pem"), "rb") as f:
        pem = f.read()
    pub = S.net2x_signctx_pubnew(0, pem, len(pem))
    assert priv and pub
    pools = {True: pool(True), False: pool(False)}
    # the sign layer's pool: POOL signed 1 KiB payloads (C1's shape)
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

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    medians = {}
    for n in sizes:
        fns, checks = {}, []
        for shared in (True, False):
            name = "shared" if shared else "perkey"
            pk, rs, dig, _, _ = pools[shared]
            h_pub = pk[0].copy() if shared else tile(pk, n)
            h_rs, h_dig = tile(rs, n), tile(dig, n)
            t_pub, t_rs, t_dig = (torch.from_numpy(a).to(dev) for a in (h_pub, h_rs, h_dig))
            t_out = torch.zeros(n, dtype=torch.uint8, device=dev)
            # verdicts first: all valid, and a corrupted copy all invalid
            assert bool(ecdsa.verify_p521(t_pub, t_rs, t_dig, out=t_out).all())
            bad = t_dig.clone()
            bad[:, 0] ^= 1
            assert not bool(ecdsa.verify_p521(t_pub, t_rs, bad).any())
            assert ecdsa.verify_p521_host(h_pub, h_rs, h_dig).all()

            def dev_call(a=t_pub, b=t_rs, c=t_dig, o=t_out):
                e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
                e0.record()
                ecdsa.verify_p521(a, b, c, out=o)
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1)

            def host_call(a=h_pub, b=h_rs, c=h_dig):
                t0 = time.perf_counter()
                ecdsa.verify_p521_host(a, b, c)
                return (time.perf_counter() - t0) * 1e3
            fns["dev_" + name], fns["host_" + name] = dev_call, host_call
        # the sign layer over n payloads: the pool's, tiled
        reps = (n + POOL - 1) // POOL
        data = np.tile(pdata, reps)[:n * plen]
        offs = np.arange(n, dtype=np.uint64) * plen
        lens = np.full(n, plen, dtype=np.uint32)
        sigs = (Signature * n)()
        for i in range(n):
            sigs[i] = psigs[i % POOL]
        valid = np.zeros(n, dtype=np.int32)

        def sig_dev():
            t0 = time.perf_counter()
            rc = S.net2x_signature_validate_batch_dev(sigs, p(data), p(offs), p(lens), n,
                                                      pub, p(valid))
            dt = (time.perf_counter() - t0) * 1e3
            assert rc == 0 and valid.all()
            return dt
        fns["sig_batch_dev"] = sig_dev
        for t in threads:
            if t == 1 and n > args.cpu1_max:
                continue

            def cpu(t=t):
                t0 = time.perf_counter()
                rc = S.net2x_signature_validate_batch(sigs, p(data), p(offs), p(lens), n,
                                                      pub, p(valid), t)
                dt = (time.perf_counter() - t0) * 1e3
                assert rc == 0 and valid.all()
                return dt
            fns[f"cpu_{t}"] = cpu
        names = list(fns)
        for name in names:              # warm-up, once each
            fns[name]()
        ms = {name: [] for name in names}
        for rnd in range(args.rounds):
            k = rnd % len(names)
            for name in names[k:] + names[:k]:
                ms[name].append(fns[name]())
        for name in names:
            med = statistics.median(ms[name])
            medians[(name, n)] = med
            emit({**meta, "n": n, "kind": name, "ms": round(med, 4),
                  "ms_min_max": [round(min(ms[name]), 4), round(max(ms[name]), 4)],
                  "verifications_per_s": round(n / med * 1e3, 1)})
    ref = f"cpu_{max(threads)}"
    cross = {}
    for kind in ("dev_shared", "dev_perkey", "host_shared", "host_perkey",
                 "sig_batch_dev"):
        wins = [n for n in sizes if (ref, n) in medians and
                medians[(kind, n)] < medians[(ref, n)]]
        cross[kind] = min(wins) if wins else None
    emit({**meta, "kind": "summary", "reference": ref,
          "smallest_n_faster_than_reference": cross})
    if out:
        out.close()


if __name__ == "__main__":
    main()
