"""GPU: batched ECDSA P-521 verification (net2/ecdsa.h, ilias_net2_amd.ecdsa)
against OpenSSL's ECDSA_do_verify (tests/ecdsa_ref.py), verdict for verdict.

Signed messages over every batch-size class (one lane, a wave less one, a
wave, a wave and one, several waves), digest lengths on both sides of the
66-byte cut, shared and per-signature keys, wide strides and odd byte offsets;
the construction lattice, whose valid signatures drive the point addition
through its exceptional cases; every bit of one signature flipped; the edge
values of r and s; the host-memory call; a captured graph replayed on other
bytes.  A wave is one serial verification long, so every launch here costs
about the same few tens of milliseconds whatever its size.
"""
import hashlib
import random

import numpy as np
import pytest

import ecdsa_ref
from ilias_net2_amd import ecdsa

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N = ecdsa_ref.order()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a GPU (HIP device not visible)")
    return torch.device("cuda:0")


def _signed(rng, count, dlens, shared_d=None, corrupt=True):
    """count cases (pub, r, s, digest, verdict) signed by OpenSSL, the digest
    lengths cycling through dlens; with corrupt, every third one is damaged
    in r, s, the digest or the key, and every verdict is OpenSSL's."""
    out = []
    for i in range(count):
        d = shared_d if shared_d is not None else rng.randrange(1, N)
        dlen = dlens[i % len(dlens)]
        dig = hashlib.shake_256(b"%d/%d" % (rng.getrandbits(64), i)).digest(dlen)
        r, s = ecdsa_ref.sign(d, dig)
        pub = ecdsa_ref.public_key(d)
        if corrupt and i % 3 == 1:
            kind = (i // 3) % 4
            if kind == 0:
                r ^= 1 << rng.randrange(521)
            elif kind == 1:
                s ^= 1 << rng.randrange(521)
            elif kind == 2 and dlen:
                b = bytearray(dig)
                b[rng.randrange(dlen)] ^= 1 << rng.randrange(8)
                dig = bytes(b)
            elif shared_d is None:
                pub = ecdsa_ref.public_key(rng.randrange(1, N))
            else:
                s = N - s if i % 2 else (s + 1) % N or 1
        out.append((pub, r, s, dig, ecdsa_ref.verify(pub, r, s, dig)))
    return out


@pytest.fixture(scope="module")
def pools():
    """The signed cases the batch tests slice: 200 under per-signature keys
    with mixed digest lengths, 200 under one key for each of 32, 48, 64."""
    rng = random.Random(521)
    shared_d = rng.randrange(1, N)
    return {"multi": _signed(rng, 200, (32, 48, 64)),
            **{dl: _signed(rng, 200, (dl,), shared_d) for dl in (32, 48, 64)}}


def _at_offset(dev, a, off):
    """The 2-D uint8 array on the device, its first byte `off` bytes into an
    allocation."""
    flat = torch.zeros(a.size + off, dtype=torch.uint8, device=dev)
    flat[off:] = torch.from_numpy(np.ascontiguousarray(a)).to(dev).reshape(-1)
    return flat[off:].view(a.shape)


def _run(dev, cases, shared=False, uniform=None, pub_stride=132, dig_stride=None,
         off=0):
    """One device launch over the cases; returns (got, want) as arrays."""
    width = max([len(c[3]) for c in cases] + [1])
    pub, rs, dig, dlens, want = ecdsa_ref.pack(cases, dig_stride or width)
    if pub_stride > 132:
        pub = np.concatenate(
            [pub, np.full((len(cases), pub_stride - 132), 0xee, np.uint8)], axis=1)
    t_pub = _at_offset(dev, pub, off)
    if shared:
        assert all(c[0] == cases[0][0] for c in cases)
        t_pub = t_pub[0, :132]
    t_rs, t_dig = _at_offset(dev, rs, off), _at_offset(dev, dig, off)
    if uniform is not None:
        assert all(len(c[3]) == uniform for c in cases)
        lens = uniform
    else:
        lens = torch.from_numpy(dlens.astype(np.int32)).to(dev)
    out = torch.full((len(cases),), 7, dtype=torch.uint8, device=dev)
    got = ecdsa.verify_p521(t_pub, t_rs, t_dig, lens, out=out)
    assert got is out
    return got.cpu().numpy(), want


def _same(got, want):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"lanes {bad[:10].tolist()}: got {got[bad[:10]].tolist()}, " \
                          f"OpenSSL {want[bad[:10]].tolist()}"


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_batch_sizes(dev, pools, n):
    # per-signature keys, per-item lengths, wide strides, off by one byte
    cases = pools["multi"][:n]
    got, want = _run(dev, cases, pub_stride=150, dig_stride=77, off=1)
    _same(got, want)
    # ... dense, aligned
    got, want = _run(dev, cases)
    _same(got, want)
    assert n < 3 or (0 < want.sum() < n)
    # one key for all, one length for all, off by three bytes
    for dl in (32, 48, 64):
        cases = pools[dl][200 - n:]
        got, want = _run(dev, cases, shared=True, uniform=dl, dig_stride=dl + 5, off=3)
        _same(got, want)
        assert n < 3 or (0 < want.sum() < n)
    # the same through per-item lengths and per-item copies of the key
    got, want = _run(dev, pools[64][:n], off=3)
    _same(got, want)


def test_digest_lengths(dev):
    """Lengths on both sides of the 66-byte cut, signed by OpenSSL over the
    same bytes: uniform, and all in one batch through the length array."""
    rng = random.Random(66)
    every = []
    for dl in (0, 1, 65, 66, 67, 100):
        cases = _signed(rng, 6, (dl,), corrupt=False)
        # beyond 66 bytes the tail is not part of e: a flip there changes nothing
        if dl > 66:
            pub, r, s, dig, _ = cases[0]
            dig = dig[:-1] + bytes([dig[-1] ^ 0x80])
            cases.append((pub, r, s, dig, ecdsa_ref.verify(pub, r, s, dig)))
            assert cases[-1][4] == 1
        if dl >= 66:
            # ... and of byte 65 only the top bit is
            pub, r, s, dig, _ = cases[1]
            for bit in (0x40, 0x80):
                d2 = dig[:65] + bytes([dig[65] ^ bit]) + dig[66:]
                cases.append((pub, r, s, d2, ecdsa_ref.verify(pub, r, s, d2)))
        got, want = _run(dev, cases, uniform=dl)
        _same(got, want)
        assert want.sum() >= 6
        every += cases
    rng.shuffle(every)
    got, want = _run(dev, every, dig_stride=100, off=1)
    _same(got, want)


@pytest.fixture(scope="module")
def lattice():
    return ecdsa_ref.lattice()


def test_construction_lattice(dev, lattice):
    """Every (d, u1, u2) of the lattice in one launch: valid signatures whose
    running point meets G, Q, their negatives and infinity on the way."""
    u1s, u2s = ecdsa_ref.lattice_scalars()
    assert len(lattice) > 7 * len(u1s) * len(u2s) - 100
    got, want = _run(dev, lattice)
    _same(got, want)
    assert want.sum() >= len(lattice) - 20 - 30 and (want == 0).sum() >= 20


def test_bit_flips(dev):
    """One lane per bit of r || s of one valid signature, then a bit in each
    digest byte and in each byte of Qx and of Qy."""
    rng = random.Random(1056)
    d = rng.randrange(1, N)
    dig = hashlib.sha512(b"bit flips").digest()
    r, s = ecdsa_ref.sign(d, dig)
    pub = ecdsa_ref.public_key(d)
    cases = [(pub, r, s, dig, ecdsa_ref.verify(pub, r, s, dig))]
    assert cases[0][4] == 1
    for bit in range(528):
        cases.append((pub, r ^ 1 << bit, s, dig))
    for bit in range(528):
        cases.append((pub, r, s ^ 1 << bit, dig))
    for i in range(64):
        b = bytearray(dig)
        b[i] ^= 1 << rng.randrange(8)
        cases.append((pub, r, s, bytes(b)))
    for i in range(132):
        b = bytearray(pub)
        b[i] ^= 1 << (rng.randrange(8) if i % 66 else 0)
        cases.append((bytes(b), r, s, dig))
    cases = [c if len(c) == 5 else c + (ecdsa_ref.verify(*c),) for c in cases]
    assert len(cases) == 1 + 1056 + 64 + 132
    got, want = _run(dev, cases, uniform=64)
    _same(got, want)
    assert want.sum() == 1


def test_edge_scalars(dev):
    """r and s from the edges of their ranges, each with a valid partner."""
    rng = random.Random(3)
    d = rng.randrange(1, N)
    dig = hashlib.sha512(b"edges").digest()
    r, s = ecdsa_ref.sign(d, dig)
    pub = ecdsa_ref.public_key(d)
    edges = [0, 1, N - 1, N, N + 1, ecdsa_ref.P, 2 ** 521 - 1, 2 ** 528 - 1]
    cases = [(pub, e, s, dig) for e in edges] + [(pub, r, e, dig) for e in edges]
    cases += [(pub, a, b, dig) for a in edges for b in edges]
    cases.append((pub, r, s, dig))
    cases = [c + (ecdsa_ref.verify(*c),) for c in cases]
    got, want = _run(dev, cases, uniform=64)
    _same(got, want)
    assert want[-1] == 1 and want[:-1].sum() == 0


def test_key_coordinates_out_of_range(dev):
    """Qx or Qy at p and beyond: rejected, as is a point off the curve."""
    rng = random.Random(4)
    d = rng.randrange(1, N)
    dig = hashlib.sha384(b"keys").digest()
    r, s = ecdsa_ref.sign(d, dig)
    pub = ecdsa_ref.public_key(d)
    x, y = int.from_bytes(pub[:66], "big"), int.from_bytes(pub[66:], "big")
    be = ecdsa_ref.be66
    keys = [pub, be(x) + be(ecdsa_ref.P - y),           # -Q: on the curve, wrong
            be(x + ecdsa_ref.P) + be(y), be(x) + be(y + ecdsa_ref.P),
            be(ecdsa_ref.P) + be(y), be(x) + be(ecdsa_ref.P),
            be(2 ** 528 - 1) + be(y), be(0) + be(0), be(x) + be(y ^ 1)]
    cases = [(k, r, s, dig, ecdsa_ref.verify(k, r, s, dig)) for k in keys]
    got, want = _run(dev, cases, uniform=48)
    _same(got, want)
    assert want.tolist() == [1] + [0] * (len(keys) - 1)


def test_mixed_verdicts(dev, pools):
    """Valid and invalid lanes interleaved within the waves."""
    good = [c for c in pools["multi"] if c[4] == 1][:70]
    bad = [c for c in pools["multi"] if c[4] == 0][:60]
    cases = [c for pair in zip(good, bad) for c in pair] + good[60:]
    got, want = _run(dev, cases)
    _same(got, want)
    assert want[:120].tolist() == [1, 0] * 60


def test_length_beyond_the_slot_is_a_zero_verdict(dev, pools):
    """With per-item lengths, a length above dig_stride cannot be refused by
    the host: that lane gets 0 and its neighbours their own verdicts."""
    cases = pools[32][:8]
    pub, rs, dig, dlens, want = ecdsa_ref.pack(cases, 32)
    lens = dlens.astype(np.int32)
    lens[3] = 33
    out = ecdsa.verify_p521(torch.from_numpy(pub).to(dev), torch.from_numpy(rs).to(dev),
                            torch.from_numpy(dig).to(dev), torch.from_numpy(lens).to(dev))
    want = want.copy()
    want[3] = 0
    _same(out.cpu().numpy(), want)


def test_host_memory_call(dev, pools, lattice):
    for cases, shared in ((pools["multi"][:65], False), (pools[48][:200], True),
                          (lattice[::40], False)):
        width = max(len(c[3]) for c in cases)
        pub, rs, dig, dlens, want = ecdsa_ref.pack(cases, width)
        got = ecdsa.verify_p521_host(cases[0][0] if shared else pub, rs, dig, dlens)
        _same(got, want)
    # one uniform length
    pub, rs, dig, dlens, want = ecdsa_ref.pack(pools[64][:10], 64)
    _same(ecdsa.verify_p521_host(pub, rs, dig), want)
    assert ecdsa.verify_p521_host(pub[:0], rs[:0], dig[:0]).shape == (0,)


def test_graph_replay(dev, pools):
    """verify_p521 captured into a graph, replayed on other bytes in the same
    buffers; the call allocates nothing when given its output."""
    n = 65
    first, second = pools["multi"][:n], pools["multi"][100:100 + n]
    pub, rs, dig, dlens, want1 = ecdsa_ref.pack(first, 64)
    t = [torch.from_numpy(a).to(dev) for a in (pub, rs, dig, dlens.astype(np.int32))]
    out = torch.full((n,), 9, dtype=torch.uint8, device=dev)
    ecdsa.verify_p521(*t, out=out)          # warm up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    count = lambda: torch.cuda.memory_stats(dev)["allocation.all.allocated"]  # noqa: E731
    with torch.cuda.graph(g):
        before = count()        # (entering the capture allocates on its own)
        ecdsa.verify_p521(*t, out=out)
        assert count() == before
    out.fill_(9)
    g.replay()
    _same(out.cpu().numpy(), want1)
    pub, rs, dig, dlens, want2 = ecdsa_ref.pack(second, 64)
    for dst, src in zip(t, (pub, rs, dig, dlens.astype(np.int32))):
        dst.copy_(torch.from_numpy(src))
    out.fill_(9)
    g.replay()
    _same(out.cpu().numpy(), want2)
    assert not np.array_equal(want1, want2)


# ---- the sign layer ------------------------------------------------------------

import ctypes  # noqa: E402
import os  # noqa: E402

from ilias_net2_amd import _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp = ctypes.c_void_p


class Signature(ctypes.Structure):
    """struct net2x_signature (include/net2/signature.h)."""
    _fields_ = [("sign_alg", vp), ("hash_alg", vp), ("data", vp),
                ("datalen", ctypes.c_size_t)]


class IOVec(ctypes.Structure):
    _fields_ = [("iov_base", vp), ("iov_len", ctypes.c_size_t)]


class ValidateReq(ctypes.Structure):
    """struct net2_sc_validate_req (include/net2/signed_carver.h)."""
    _fields_ = [("payload", ctypes.POINTER(IOVec)), ("iovcnt", ctypes.c_size_t),
                ("sig", ctypes.POINTER(Signature)), ("sctx", vp),
                ("result", ctypes.c_int)]


@pytest.fixture(scope="module")
def sign_lib(dev):
    _lib.lib()
    S = ctypes.CDLL(os.path.join(ROOT, "ilias_net2_amd", "libnet2_sign.so"))
    for name in ("net2x_signctx_pubnew", "net2x_signctx_privnew"):
        getattr(S, name).restype = vp
        getattr(S, name).argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
    S.net2x_signctx_free.argtypes = [vp]
    S.net2x_signature_create_batch.argtypes = [
        ctypes.POINTER(Signature), vp, vp, vp, ctypes.c_size_t, ctypes.c_int, vp,
        ctypes.c_int]
    S.net2x_signature_validate_batch.argtypes = [
        ctypes.POINTER(Signature), vp, vp, vp, ctypes.c_size_t, vp, vp, ctypes.c_int]
    S.net2x_signature_validate_batch_dev.argtypes = [
        ctypes.POINTER(Signature), vp, vp, vp, ctypes.c_size_t, vp, vp]
    S.net2x_signature_deinit.argtypes = [ctypes.POINTER(Signature)]
    for name in ("net2_signed_combiner_validate_tick",
                 "net2_signed_combiner_validate_tick_dev"):
        getattr(S, name).argtypes = [ctypes.POINTER(ValidateReq), ctypes.c_size_t,
                                     ctypes.c_int]
    return S


def _golden_pems():
    keys = os.path.join(ROOT, "tests", "golden", "keys")
    with open(os.path.join(keys, "ecdsa_p521_priv.pem"), "rb") as f:
        priv = f.read()
    with open(os.path.join(keys, "ecdsa_p521_pub.pem"), "rb") as f:
        return priv, f.read()


def _flip(addr, at):
    b = (ctypes.c_ubyte * 1).from_address(addr + at)
    b[0] ^= 0x10


def test_signature_validate_batch_dev(sign_lib):
    """300 signed payloads, three hash algorithms, some signatures and some
    payloads corrupted: valid[] of the device form is the host form's."""
    S = sign_lib
    priv_pem, pub_pem = _golden_pems()
    priv = S.net2x_signctx_privnew(0, priv_pem, len(priv_pem))
    pub = S.net2x_signctx_pubnew(0, pub_pem, len(pub_pem))
    assert priv and pub
    n, rng = 300, np.random.default_rng(300)
    lens = rng.integers(1, 700, n).astype(np.uint32)
    offs = np.zeros(n, dtype=np.uint64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    data = rng.integers(0, 256, int(lens.sum()), dtype=np.uint8)
    sigs = (Signature * n)()
    p = lambda a: a.ctypes.data  # noqa: E731
    try:
        for k, alg in enumerate((1, 2, 3)):          # 100 signatures a hash
            lo = 100 * k
            assert S.net2x_signature_create_batch(
                ctypes.cast(ctypes.byref(sigs, lo * ctypes.sizeof(Signature)),
                            ctypes.POINTER(Signature)),
                p(data), p(offs[lo:]), p(lens[lo:]), 100, alg, priv, 4) == 0
        for i in range(0, n, 7):                    # payloads
            data[int(offs[i]) + int(lens[i]) // 2] ^= 1
        for i in range(3, n, 11):                   # signatures: DER and value bytes
            _flip(sigs[i].data, (i * 5) % sigs[i].datalen)
        for i in range(5, n, 50):                   # ... and their lengths
            sigs[i].datalen -= 1
        want = np.full(n, 7, dtype=np.int32)
        got = np.full(n, 7, dtype=np.int32)
        assert S.net2x_signature_validate_batch(sigs, p(data), p(offs), p(lens), n, pub,
                                                p(want), 4) == 0
        assert S.net2x_signature_validate_batch_dev(sigs, p(data), p(offs), p(lens), n,
                                                    pub, p(got)) == 0
        assert np.array_equal(got, want)
        assert 200 < want.sum() < 260 and set(want.tolist()) == {0, 1}
    finally:
        for i in range(n):
            S.net2x_signature_deinit(ctypes.byref(sigs[i]))
        S.net2x_signctx_free(priv)
        S.net2x_signctx_free(pub)


def test_combiner_tick_dev(sign_lib):
    """The combiner's tick over three contexts -- two on P-521, whose checks
    go to the device in one batch, one on P-256, whose checks stay on the host
    threads: result[] is the host tick's."""
    S = sign_lib
    pems = [_golden_pems(), ecdsa_ref.pem_keypair(),
            ecdsa_ref.pem_keypair(ecdsa_ref.NID_P256)]
    privs = [S.net2x_signctx_privnew(0, a, len(a)) for a, _ in pems]
    pubs = [S.net2x_signctx_pubnew(0, b, len(b)) for _, b in pems]
    assert all(privs) and all(pubs)
    n, rng = 90, np.random.default_rng(90)
    payloads = [rng.integers(0, 256, int(rng.integers(1, 400)), dtype=np.uint8)
                for _ in range(n)]
    iovs = (IOVec * n)(*[IOVec(a.ctypes.data, a.size) for a in payloads])
    sigs = (Signature * n)()
    reqs = (ValidateReq * n)()
    off, ln = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint32)
    bogus = ctypes.create_string_buffer(b"SHA999")
    try:
        for i in range(n):
            ln[0] = payloads[i].size
            assert S.net2x_signature_create_batch(
                ctypes.byref(sigs[i]), payloads[i].ctypes.data, off.ctypes.data,
                ln.ctypes.data, 1, 1 + i % 3, privs[i % 3], 1) == 0
            reqs[i] = ValidateReq(ctypes.pointer(iovs[i]), 1, ctypes.pointer(sigs[i]),
                                  pubs[i % 3], 77)
        for i in range(0, n, 4):                    # payloads of every context
            payloads[i][payloads[i].size // 2] ^= 4
        for i in range(1, n, 9):                    # signatures
            _flip(sigs[i].data, sigs[i].datalen - 2)
        for i in (2, 30, 61):                       # the wrong context's key
            reqs[i].sctx = pubs[(i + 1) % 3]
        keep = sigs[44].hash_alg                    # an unknown hash: EIO
        sigs[44].hash_alg = ctypes.addressof(bogus)
        assert S.net2_signed_combiner_validate_tick(reqs, n, 4) == 0
        want = [r.result for r in reqs]
        for r in reqs:
            r.result = 77
        assert S.net2_signed_combiner_validate_tick_dev(reqs, n, 4) == 0
        got = [r.result for r in reqs]
        sigs[44].hash_alg = keep
        assert got == want
        assert set(want) == {0, 22, 5} and want.count(0) > n // 2   # 0, EINVAL, EIO
    finally:
        for i in range(n):
            S.net2x_signature_deinit(ctypes.byref(sigs[i]))
        for c in privs + pubs:
            S.net2x_signctx_free(c)
