"""The payload cipher of the packet bursts on the GPU:
net2_packet_decrypt_burst / net2_packet_encrypt_burst against the system
libcrypto's EVP_aes_256_cbc (tests/aes_ref.py: the calls src/enc.c makes),
IVs from oracle.ph_to_iv_batch.

Every expected code, length and byte comes from the helper: a datagram is
NET2_PDECODE_BAD exactly where EVP_DecryptFinal_ex fails.  One thing is
checked more strictly than the header promises callers: a datagram that ends
BAD is not written at all, so the "untouched" checks cover it as well.
"""
import ctypes
import functools
import json
import os
import struct
import types

import numpy as np
import pytest

import aes_ref
import test_gpu_packet as P

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

OK, RESOURCE, BAD, UNSAFE = 0, 1, 2, 3
ENC, SIGNED, ALTKEY = P.PH_ENCRYPTED, P.PH_SIGNED, P.PH_ALTKEY
HL = P.HL
SENTINEL = 0xA5
# plaintext lengths on both sides of every block edge up to three blocks,
# then the mix's sizes and the longest payload of a 1,500-byte datagram
PLENS = [0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 100, 255, 256,
         511, 512, 1000, 1471, 1472]
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a GPU (HIP device not visible)")
    from ilias_net2_amd import _lib
    assert _lib.device_count() >= 1
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def lane_form():
    """Every decrypt burst of this module's tests -- and of
    test_gpu_aes_burst_mc.py's, which imports this fixture -- in the lane
    form: at the default limit all but the largest would take the wave form,
    which test_gpu_aes_burst_wave.py runs them in (it calls the test
    functions as plain functions, so this fixture does not reach it).  Every
    decrypt launch counts in exactly one of net2_aes_burst_stats' two
    counters: none in the wave form means each took the lane form."""
    from ilias_net2_amd import cipher_burst
    cipher_burst.limits(0)
    before = cipher_burst.stats()
    try:
        yield
        after = cipher_burst.stats()
    finally:
        cipher_burst.limits(-1)
    assert after["wave_launches"] == before["wave_launches"]


# net2_sha2_burst_limits' arguments for each form of the keyed hash bursts
# (tests/test_gpu_burst_lattice.py): hmac_kernel in submission order, the same
# in the length-binned order, burst_wave_kernel
HASH_FORMS = {"lane": (0, -1), "binned": (0, 1), "wave": (1 << 30, -1)}


@pytest.fixture
def hash_form():
    """net2_sha2_burst_limits for one test, the defaults restored after."""
    from ilias_net2_amd import _lib
    L = _lib.lib()

    def set_form(form):
        assert L.net2_sha2_burst_limits(*HASH_FORMS[form]) == 0
    yield set_form
    L.net2_sha2_burst_limits(-1, -1)


def _dev(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)


def _place(lens, rng):
    """Offsets for datagrams of `lens` bytes, stray bytes between
    them; datagram i starts at residue i mod 16."""
    offs = np.zeros(len(lens), dtype=np.uint64)
    cur = int(rng.integers(1, 16))
    for i, ln in enumerate(lens):
        cur += (i - cur) % 16
        offs[i] = cur
        cur += int(ln) + int(rng.integers(1, 9))
    return offs, cur + 16


def _keys(rng):
    return (rng.integers(0, 256, 32, dtype=np.uint8).tobytes(),
            rng.integers(0, 256, 32, dtype=np.uint8).tobytes())


KINDS = ("ragged", "empty", "pad00", "pad11", "padrun", "fullpad", "inbad",
         "noenc")


@functools.lru_cache(maxsize=None)
def rx_case(oracle_mod, hash_alg, n=333, no_cutoff=False):
    """One received burst under rx key state with (hash_alg != 0) or without
    an alternate key, and what EVP makes of every datagram.  Each kind in
    KINDS is 1/16 of the burst, spread over every wave; the other half are
    plain valid datagrams.  no_cutoff (NET2_CK_F_NO_RX_CUTOFF): only PH_ALTKEY
    picks the alternate key, a seq past the cutoff does not.  Built once per
    row; the tests leave it unchanged."""
    rng = np.random.default_rng(4100 + hash_alg + 50 * no_cutoff)
    hl = HL[hash_alg]
    has_alt = hash_alg != 0
    key, alt_key = _keys(rng)
    rx_start = 0xfffff000                       # the window start wraps
    cutoff = (rx_start + 150) & 0xffffffff      # later datagrams: alternate key
    seq = ((rx_start + np.arange(n)) & 0xffffffff).astype(np.uint32)
    kind_of = rng.permutation(n) % 16
    kinds = [KINDS[k] if k < len(KINDS) else "ok" for k in kind_of]
    flags = np.full(n, ENC, dtype=np.uint32)
    if hash_alg:
        flags[rng.random(n) < 0.6] |= SIGNED    # po 8 and 8 + hl in every wave
        flags[rng.random(n) < 0.25] |= ALTKEY
    for i, k in enumerate(kinds):
        if k == "noenc":
            flags[i] &= ~np.uint32(ENC)
    iv = oracle_mod.ph_to_iv_batch(seq, flags, 16)
    picks = np.array([P.ref_rx_key(int(seq[i]), int(flags[i]), has_alt, no_cutoff,
                                   cutoff, rx_start) for i in range(n)])
    res_in = np.zeros(n, dtype=np.uint8)
    dgs, cts = [], []
    for i, k in enumerate(kinds):
        kk = alt_key if picks[i] else key
        ivb = iv[i].tobytes()
        pl = PLENS[i % len(PLENS)]
        if k == "fullpad":
            pl = (0, 16, 32, 48, 1472)[i % 5]
        plain = rng.integers(0, 256, pl, dtype=np.uint8).tobytes()
        if k in ("pad00", "pad11", "padrun"):
            tail = {"pad00": b"\x00", "pad11": b"\x11", "padrun": b"\x03\x02\x03"}[k]
            body = plain + bytes(-(len(plain) + len(tail)) % 16) + tail
            ct = aes_ref.encrypt(kk, ivb, body, pad=False)
        else:
            ct = aes_ref.encrypt(kk, ivb, plain)
        if k == "ragged":
            extra = int(rng.integers(1, 16))
            ct = (ct + rng.integers(0, 256, extra, dtype=np.uint8).tobytes()
                  if i % 2 else ct[:len(ct) - extra])
        elif k == "empty":
            ct = b""
        elif k == "inbad":
            res_in[i] = (BAD, UNSAFE)[i % 2]
        field = (rng.integers(0, 256, hl, dtype=np.uint8).tobytes()
                 if flags[i] & SIGNED else b"")
        dgs.append(struct.pack(">II", int(seq[i]), int(flags[i])) + field + ct)
        cts.append(ct)
    lens = np.array([len(d) for d in dgs], dtype=np.uint32)
    offs, total = _place(lens, rng)
    data = rng.integers(0, 256, total, dtype=np.uint8)
    for i, d in enumerate(dgs):
        data[int(offs[i]):int(offs[i]) + len(d)] = np.frombuffer(d, dtype=np.uint8)
    # what the reference's decryption step makes of each datagram
    want_res = res_in.copy()
    want_plen = np.zeros(n, dtype=np.uint32)
    want_plain = [b""] * n
    written = np.zeros(total, dtype=bool)       # payloads of decrypted datagrams
    for i in range(n):
        if res_in[i] != OK or not flags[i] & ENC:
            continue
        got = aes_ref.decrypt(alt_key if picks[i] else key, iv[i].tobytes(), cts[i])
        if got is None:
            want_res[i] = BAD
            continue
        want_plen[i], want_plain[i] = len(got), got
        po = 8 + (hl if flags[i] & SIGNED else 0)
        written[int(offs[i]) + po:int(offs[i]) + int(lens[i])] = True
    # the case holds what it is meant to hold
    count = {k: kinds.count(k) for k in KINDS}
    assert all(c >= 0.05 * n for c in count.values()), count
    assert len(set(int(o) % 16 for o in offs)) == 16
    decrypted = {len(want_plain[i]) for i in range(n)
                 if res_in[i] == OK and flags[i] & ENC and want_res[i] == OK}
    assert {0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 1472} <= decrypted
    assert int(want_plen.max()) == 1472
    if has_alt:
        alt_by_flag = picks & ((flags & ALTKEY) != 0) & (np.arange(n) < 150)
        alt_by_cutoff = picks & ((flags & ALTKEY) == 0)
        assert alt_by_flag.sum() > 10 and (~picks).sum() > 10
        if no_cutoff:
            # past the cutoff without PH_ALTKEY: the active key, and they
            # decrypt -- under the alternate key they would not
            past = (np.arange(n) >= 150) & ((flags & ALTKEY) == 0)
            assert not (picks & past).any() and alt_by_cutoff.sum() == 0
            assert (past & (res_in == OK) & ((flags & ENC) != 0) &
                    (want_res == OK)).sum() > 10
            assert (picks & ((flags & ALTKEY) != 0)).sum() > 10
        else:
            assert alt_by_cutoff.sum() > 10
    for k in ("pad00", "pad11", "padrun", "ragged", "empty"):
        assert all(want_res[i] == BAD for i in range(n) if kinds[i] == k), k
    assert all(want_res[i] == OK and want_plen[i] % 16 == 0
               for i in range(n) if kinds[i] == "fullpad")
    for a in (data, offs, lens, seq, flags, iv, res_in, want_res, want_plen, written):
        a.setflags(write=False)
    return types.SimpleNamespace(
        n=n, hash_alg=hash_alg, hl=hl, key=key, alt_key=alt_key if has_alt else None,
        no_cutoff=no_cutoff, rx_start=rx_start, cutoff=cutoff, seq=seq, flags=flags, iv=iv, kinds=kinds,
        data=data, offs=offs, lens=lens, res_in=res_in, want_res=want_res,
        want_plen=want_plen, want_plain=want_plain, written=written, total=total)


def _decrypt(c, dev, in_place):
    from ilias_net2_amd import cipher_burst
    d = _dev(c.data, dev)
    out = d if in_place else torch.full((c.total,), SENTINEL, dtype=torch.uint8,
                                        device=dev)
    res, plain, plen = cipher_burst.decrypt_burst(
        c.hash_alg, c.key, d, _dev(c.offs.astype(np.int64), dev),
        _dev(_i32(c.lens), dev), _dev(_i32(c.seq), dev), _dev(_i32(c.flags), dev),
        _dev(c.iv, dev), _dev(c.res_in, dev), alt_key=c.alt_key,
        alt_no_cutoff=c.no_cutoff, alt_cutoff=c.cutoff, rx_start=c.rx_start, out=out)
    torch.cuda.synchronize()
    assert plain is out
    return res.cpu().numpy(), plain.cpu().numpy(), plen.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("hash_alg,no_cutoff", [
    pytest.param(4, False, id="4"), pytest.param(6, False, id="6"),
    pytest.param(0, False, id="0"), pytest.param(5, False, id="5"),
    pytest.param(6, True, id="6-no_cutoff"), pytest.param(4, True, id="4-no_cutoff")])
def test_rx_burst(dev, oracle_mod, hash_alg, no_cutoff, in_place):
    """n = 333: two workgroups, a ragged last wave; rows 4, 5 (payloads at 8
    mod 16) and 6 with an alternate key (by PH_ALTKEY and by the cutoff, or
    with no_cutoff by PH_ALTKEY alone), and no keyed hash -- the instance
    without an alternate key."""
    c = rx_case(oracle_mod, hash_alg, no_cutoff=no_cutoff)
    res, out, plen = _decrypt(c, dev, in_place)
    bad = np.nonzero(res != c.want_res)[0]
    assert len(bad) == 0, [(int(i), c.kinds[i], int(res[i])) for i in bad[:8]]
    bad = np.nonzero(plen != c.want_plen)[0]
    assert len(bad) == 0, [(int(i), c.kinds[i], int(plen[i])) for i in bad[:8]]
    for i in range(c.n):
        if c.want_plen[i]:
            po = 8 + (c.hl if c.flags[i] & SIGNED else 0)
            a = int(c.offs[i]) + po
            assert out[a:a + int(plen[i])].tobytes() == c.want_plain[i], (i, c.kinds[i])
    # nothing outside the payloads of the decrypted datagrams is written
    untouched = ~c.written
    if in_place:
        assert np.array_equal(out[untouched], c.data[untouched])
    else:
        assert (out[untouched] == SENTINEL).all()


@functools.lru_cache(maxsize=None)
def tx_case(hash_alg, n=333):
    """Slots to encrypt: the same lengths; exactly enough room, a byte short,
    or room to spare; with and without PH_ENCRYPTED and PH_SIGNED."""
    rng = np.random.default_rng(4200 + hash_alg)
    hl = HL[hash_alg]
    key, _ = _keys(rng)
    seq = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    flags = np.zeros(n, dtype=np.uint32)
    flags[rng.random(n) < 0.75] |= ENC
    if hash_alg:
        flags[rng.random(n) < 0.6] |= SIGNED
    iv = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    plen = np.array([PLENS[i % len(PLENS)] for i in range(n)], dtype=np.uint32)
    room = rng.permutation(n) % 8              # 0: a byte short; 1..4: exact
    lens = np.zeros(n, dtype=np.uint32)
    po = np.zeros(n, dtype=np.uint32)
    for i in range(n):
        po[i] = 8 + (hl if flags[i] & SIGNED else 0)
        need = po[i] + (16 * (plen[i] // 16 + 1) if flags[i] & ENC else plen[i])
        lens[i] = need - 1 if room[i] == 0 else need + (0 if room[i] <= 4 else
                                                        int(rng.integers(1, 40)))
    offs, total = _place(lens, rng)
    data = rng.integers(0, 256, total, dtype=np.uint8)
    want = data.copy()
    want_res = np.zeros(n, dtype=np.uint8)
    want_wire = np.zeros(n, dtype=np.uint32)
    for i in range(n):
        a = int(offs[i]) + int(po[i])
        if not flags[i] & ENC:
            want_wire[i] = po[i] + plen[i]
            want_res[i] = RESOURCE if want_wire[i] > lens[i] else OK
            continue
        ct = aes_ref.encrypt(key, iv[i].tobytes(), data[a:a + int(plen[i])].tobytes())
        if po[i] + len(ct) > lens[i]:
            want_res[i] = RESOURCE
            continue
        want[a:a + len(ct)] = np.frombuffer(ct, dtype=np.uint8)
        want_wire[i] = po[i] + len(ct)
    short = (room == 0)
    assert (short & ((flags & ENC) != 0)).sum() >= 0.05 * n
    assert (want_res[short] == RESOURCE).all() and (want_res[~short] == OK).all()
    assert ((room >= 1) & (room <= 4) & ((flags & ENC) != 0)).sum() > 50
    for a in (data, offs, lens, flags, iv, plen, want, want_res, want_wire):
        a.setflags(write=False)
    return types.SimpleNamespace(n=n, hl=hl, key=key, seq=seq, flags=flags, iv=iv,
                                 plen=plen, lens=lens, offs=offs, data=data, want=want,
                                 want_res=want_res, want_wire=want_wire)


@pytest.mark.parametrize("hash_alg", [4, 6, 0, 5])
def test_tx_burst(dev, hash_alg):
    from ilias_net2_amd import cipher_burst
    c = tx_case(hash_alg)
    d = _dev(c.data, dev)
    res, wire = cipher_burst.encrypt_burst(
        c.key, c.hl, _dev(_i32(c.flags), dev), _dev(c.iv, dev), d,
        _dev(c.offs.astype(np.int64), dev), _dev(_i32(c.lens), dev),
        _dev(_i32(c.plen), dev))
    torch.cuda.synchronize()
    assert np.array_equal(res.cpu().numpy(), c.want_res)
    assert np.array_equal(wire.cpu().numpy().view(np.uint32), c.want_wire)
    got = d.cpu().numpy()
    bad = np.nonzero(got != c.want)[0]
    assert len(bad) == 0, bad[:8]


def _one_burst(payloads, slack=0):
    """Unsigned datagrams (8-byte header, then the payload) packed back to
    back from offset 3: (data, offsets, lens) host arrays."""
    lens = np.array([8 + len(p) + slack for p in payloads], dtype=np.uint32)
    offs = (3 + np.concatenate(([0], np.cumsum(lens[:-1])))).astype(np.uint64)
    data = np.zeros(3 + int(lens.sum()) + 5, dtype=np.uint8)
    for o, p in zip(offs, payloads):
        data[int(o) + 8:int(o) + 8 + len(p)] = np.frombuffer(p, dtype=np.uint8)
    return data, offs, lens


def _round_trip(dev, key, ivs, plains):
    """encrypt_burst then decrypt_burst over unsigned datagrams, no keyed
    hash; returns (ciphertexts, plaintexts) as the device produced them."""
    from ilias_net2_amd import cipher_burst
    n = len(plains)
    data, offs, lens = _one_burst(plains, slack=16)
    flags = _dev(np.full(n, ENC, dtype=np.int32), dev)
    d, o, ln = _dev(data, dev), _dev(offs.astype(np.int64), dev), _dev(_i32(lens), dev)
    iv = _dev(np.frombuffer(b"".join(ivs), dtype=np.uint8).reshape(n, 16), dev)
    plen = _dev(np.array([len(p) for p in plains], dtype=np.int32), dev)
    res, wire = cipher_burst.encrypt_burst(key, 0, flags, iv, d, o, ln, plen)
    sealed = d.clone()
    seq = torch.zeros(n, dtype=torch.int32, device=dev)
    res2, out, plen2 = cipher_burst.decrypt_burst(0, key, d, o, wire, seq, flags, iv,
                                                  torch.zeros_like(res), out=d)
    torch.cuda.synchronize()
    assert (res.cpu().numpy() == OK).all() and (res2.cpu().numpy() == OK).all()
    w, s, g, pl = (wire.cpu().numpy(), sealed.cpu().numpy(), out.cpu().numpy(),
                   plen2.cpu().numpy())
    cts = [s[int(offs[i]) + 8:int(offs[i]) + int(w[i])].tobytes() for i in range(n)]
    pts = [g[int(offs[i]) + 8:int(offs[i]) + 8 + int(pl[i])].tobytes() for i in range(n)]
    return cts, pts


def test_known_answer(dev):
    """SP 800-38A F.2.5 / F.2.6 as one datagram, both ways."""
    with open(os.path.join(HERE, "golden", "aes256_cbc_kat.json")) as f:
        k = {n: bytes.fromhex(v) for n, v in json.load(f).items()
             if n in ("key", "iv", "plaintext", "ciphertext_padded")}
    cts, pts = _round_trip(dev, k["key"], [k["iv"]], [k["plaintext"]])
    assert cts == [k["ciphertext_padded"]]
    assert pts == [k["plaintext"]]


def test_divergent_lengths(dev):
    """One 1,472-byte datagram among 64 empty ones: a wave whose lanes leave
    the block loop 92 iterations apart, and a second wave of one lane."""
    rng = np.random.default_rng(4300)
    key, _ = _keys(rng)
    for at in (0, 37, 64):
        plains = [b""] * 65
        plains[at] = rng.integers(0, 256, 1472, dtype=np.uint8).tobytes()
        ivs = [rng.integers(0, 256, 16, dtype=np.uint8).tobytes() for _ in range(65)]
        cts, pts = _round_trip(dev, key, ivs, plains)
        assert cts == [aes_ref.encrypt(key, ivs[i], plains[i]) for i in range(65)]
        assert pts == plains


def test_chain_on_one_stream(dev, oracle_mod):
    """IVs, encrypt, seal, verify under a key state with an alternate key
    installed, decrypt: one stream, no synchronisation in between.  The
    transmitter seals each datagram with the key set the receiver will pick
    (net2_ck_tx_key), so TX is one call sequence per key set."""
    _chain_on_one_stream(dev, oracle_mod, False)


def test_chain_on_one_stream_no_cutoff(dev, oracle_mod):
    """The same chain with NET2_CK_F_NO_RX_CUTOFF set in the one key state
    both RX steps run under: seq runs past alt_cutoff, and the datagrams there
    without PH_ALTKEY are sealed, verified and decrypted with the active key.
    A hash step and a cipher step that disagree on a datagram make it BAD."""
    _chain_on_one_stream(dev, oracle_mod, True)


def _chain_on_one_stream(dev, oracle_mod, no_cutoff):
    c = chain_case(no_cutoff)
    t = chain_device(dev, c)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()                        # inputs are in place
    with torch.cuda.stream(s):
        o = chain_body(dev, c, t, s)
    s.synchronize()
    chain_check(oracle_mod, c, o)


@functools.lru_cache(maxsize=None)
def chain_case(no_cutoff, fresh=False):
    """The chain's burst on the host: n = 200 under row 6 with an alternate
    key installed, a tenth of the datagrams tampered with after sealing.
    fresh: the same geometry, keys and headers over other plaintext bytes.
    Built once; the tests leave it unchanged."""
    rng = np.random.default_rng(4400)
    n, hash_alg, hl = 200, 6, 64
    hkey, halt = (rng.integers(0, 256, hl, dtype=np.uint8).tobytes() for _ in range(2))
    ekey, ealt = _keys(rng)
    rx_start, cutoff = 1000, 1120
    seq = (rx_start + np.arange(n)).astype(np.uint32)
    flags = np.full(n, ENC | SIGNED, dtype=np.uint32)
    flags[rng.random(n) < 0.3] |= ALTKEY
    picks = np.array([P.ref_rx_key(int(seq[i]), int(flags[i]), True, no_cutoff, cutoff,
                                   rx_start) for i in range(n)])
    assert 20 < picks.sum() < n - 20
    past = (seq >= cutoff) & ((flags & ALTKEY) == 0)
    # past the cutoff without PH_ALTKEY: the alternate key, unless no_cutoff
    assert past.sum() > 20 and (picks[past] == (not no_cutoff)).all()
    plen = np.array([PLENS[i % len(PLENS)] for i in range(n)], dtype=np.uint32)
    po = 8 + hl
    lens = (po + 16 * (plen // 16 + 1)).astype(np.uint32)
    offs, total = _place(lens, rng)
    data = rng.integers(0, 256, total, dtype=np.uint8)
    flip = np.nonzero(rng.random(n) < 0.1)[0]       # tampered after sealing
    flip_at = np.array([int(offs[i]) + po + int(rng.integers(0, lens[i] - po))
                        for i in flip], dtype=np.int64)
    if fresh:
        data = rng.integers(0, 256, total, dtype=np.uint8)
    plains = [data[int(offs[i]) + po:int(offs[i]) + po + int(plen[i])].tobytes()
              for i in range(n)]
    for a in (seq, flags, picks, plen, lens, offs, data, flip, flip_at):
        a.setflags(write=False)
    return types.SimpleNamespace(
        n=n, hash_alg=hash_alg, hl=hl, po=po, hkey=hkey, halt=halt, ekey=ekey, ealt=ealt,
        no_cutoff=no_cutoff, rx_start=rx_start, cutoff=cutoff, seq=seq, flags=flags,
        picks=picks, plen=plen, lens=lens, offs=offs, total=total, data=data,
        plains=plains, flip=flip, flip_at=flip_at)


def chain_device(dev, c):
    """The chain's inputs on the device; `d` is the buffer it works in."""
    groups = []
    for alt in (False, True):
        idx = np.nonzero(c.picks == alt)[0]
        groups.append((idx, _dev(idx.astype(np.int64), dev), c.halt if alt else c.hkey,
                       c.ealt if alt else c.ekey))
    return types.SimpleNamespace(
        d=_dev(c.data, dev), d_flip=_dev(c.flip_at, dev), d_seq=_dev(_i32(c.seq), dev),
        d_fl=_dev(_i32(c.flags), dev), d_off=_dev(c.offs.astype(np.int64), dev),
        d_len=_dev(_i32(c.lens), dev), d_plen=_dev(_i32(c.plen), dev), groups=groups)


def chain_body(dev, c, t, s):
    """Every call of the chain on stream s, nothing synchronised: TX per key
    set, the tamper step, RX.  Returns the outputs, and the host buffers of
    the RX hash keys."""
    from ilias_net2_amd import _lib, cipher_burst
    L = _lib.lib()
    n, hash_alg, hl, total = c.n, c.hash_alg, c.hl, c.total
    hkey, halt, ekey, ealt = c.hkey, c.halt, c.ekey, c.ealt
    no_cutoff, cutoff, rx_start = c.no_cutoff, c.cutoff, c.rx_start
    d, d_flip, d_seq, d_fl = t.d, t.d_flip, t.d_seq, t.d_fl
    d_off, d_len, d_plen = t.d_off, t.d_len, t.d_plen
    tx_out = []
    for idx, d_idx, hk, ek in t.groups:
        m = len(idx)
        g_seq, g_fl = d_seq[d_idx].contiguous(), d_fl[d_idx].contiguous()
        g_off, g_len = d_off[d_idx].contiguous(), d_len[d_idx].contiguous()
        g_plen = d_plen[d_idx].contiguous()
        iv = torch.empty((m, 16), dtype=torch.uint8, device=dev)
        _lib.check(L.net2_ph_to_iv_dev(g_seq.data_ptr(), g_fl.data_ptr(), m, 16,
                                       iv.data_ptr(), s.cuda_stream))
        eres, wire = cipher_burst.encrypt_burst(ek, hl, g_fl, iv, d, g_off, g_len,
                                                g_plen, stream=s)
        ws = torch.empty(L.net2_packet_burst_workspace(m), dtype=torch.uint8,
                         device=dev)
        sres = torch.empty(m, dtype=torch.uint8, device=dev)
        _lib.check(L.net2_packet_encode_burst(
            hash_alg, hk, hl, 1, g_seq.data_ptr(), g_fl.data_ptr(), d.data_ptr(),
            g_off.data_ptr(), wire.data_ptr(), m, sres.data_ptr(), ws.data_ptr(),
            ws.numel(), s.cuda_stream))
        tx_out.append((eres, wire, sres, ws, (g_seq, g_fl, g_off, g_len, g_plen, iv)))
    sealed = d.clone()
    d[d_flip] ^= 0x40
    # RX
    res = torch.full((n,), 9, dtype=torch.uint8, device=dev)
    iv = torch.zeros((n, 16), dtype=torch.uint8, device=dev)
    r_seq = torch.empty(n, dtype=torch.int32, device=dev)
    r_fl = torch.empty(n, dtype=torch.int32, device=dev)
    ws = torch.empty(L.net2_packet_burst_workspace(n), dtype=torch.uint8, device=dev)
    kb, ab = ctypes.create_string_buffer(hkey, hl), ctypes.create_string_buffer(halt, hl)
    ks = _lib.BurstRxKeys(hash_alg, ctypes.cast(kb, ctypes.c_void_p), hl, 1,
                          ctypes.cast(ab, ctypes.c_void_p), hl, int(no_cutoff), cutoff,
                          rx_start)
    _lib.check(L.net2_packet_decode_burst_ck(
        ctypes.byref(ks), 16, d.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n,
        res.data_ptr(), iv.data_ptr(), r_seq.data_ptr(), r_fl.data_ptr(),
        ws.data_ptr(), ws.numel(), s.cuda_stream))
    out = torch.full((total,), SENTINEL, dtype=torch.uint8, device=dev)
    res, out, got_plen = cipher_burst.decrypt_burst(
        hash_alg, ekey, d, d_off, d_len, r_seq, r_fl, iv, res, alt_key=ealt,
        alt_no_cutoff=no_cutoff, alt_cutoff=cutoff, rx_start=rx_start, out=out, stream=s)
    return types.SimpleNamespace(groups=t.groups, tx_out=tx_out, sealed=sealed, res=res,
                                 out=out, got_plen=got_plen, keys=(kb, ab),
                                 keep=(iv, r_seq, r_fl, ws))


def chain_check(oracle_mod, c, o):
    """What the chain left, against EVP and the oracle (the outputs are read
    after the stream has finished)."""
    n, hash_alg, po, total = c.n, c.hash_alg, c.po, c.total
    ekey, ealt, seq, flags, picks = c.ekey, c.ealt, c.seq, c.flags, c.picks
    plen, lens, offs, data, plains, flip = c.plen, c.lens, c.offs, c.data, c.plains, c.flip
    groups, tx_out, sealed = o.groups, o.tx_out, o.sealed
    res, out, got_plen = o.res, o.out, o.got_plen
    # the sealed datagrams are the oracle's over the helper-encrypted payloads
    ivs = oracle_mod.ph_to_iv_batch(seq, flags, 16)
    want = data.copy()
    for i in range(n):
        ct = aes_ref.encrypt(ealt if picks[i] else ekey, ivs[i].tobytes(), plains[i])
        a = int(offs[i]) + po
        want[a:a + len(ct)] = np.frombuffer(ct, dtype=np.uint8)
    for (idx, _, hk, _), (eres, wire, sres, _, _) in zip(groups, tx_out):
        assert (eres.cpu().numpy() == OK).all() and (sres.cpu().numpy() == OK).all()
        assert np.array_equal(wire.cpu().numpy().view(np.uint32), lens[idx])
        r, sealed_ref = oracle_mod.packet_encode_batch(hash_alg, hk, True, seq[idx],
                                                       flags[idx], want, offs[idx],
                                                       lens[idx])
        assert (r == OK).all()
        for i in idx:
            a, b = int(offs[i]), int(offs[i]) + int(lens[i])
            want[a:b] = sealed_ref[a:b]
    assert np.array_equal(sealed.cpu().numpy(), want)
    # the plaintexts come back; a tampered datagram is BAD and never decrypted
    res, out, got_plen = res.cpu().numpy(), out.cpu().numpy(), got_plen.cpu().numpy()
    tampered = np.zeros(n, dtype=bool)
    tampered[flip] = True
    assert len(flip) > 5
    assert np.array_equal(res, np.where(tampered, BAD, OK))
    assert np.array_equal(got_plen.view(np.uint32), np.where(tampered, 0, plen))
    written = np.zeros(total, dtype=bool)
    for i in range(n):
        if tampered[i]:
            continue
        a = int(offs[i]) + po
        assert out[a:a + int(plen[i])].tobytes() == plains[i], i
        written[a:int(offs[i]) + int(lens[i])] = True
    assert (out[~written] == SENTINEL).all()


def test_keys_need_not_outlive_the_call(dev, oracle_mod):
    """The key buffers are overwritten as soon as each call returns; the
    round keys travelled in the launch's arguments."""
    from ilias_net2_amd import _lib
    L = _lib.lib()
    c = rx_case(oracle_mod, 6)
    vp = ctypes.c_void_p
    kb = ctypes.create_string_buffer(c.key, 32)
    ab = ctypes.create_string_buffer(c.alt_key, 32)
    hb = ctypes.create_string_buffer(64)
    ck = _lib.BurstCipherKeys(_lib.ENC_AES256, ctypes.cast(kb, vp), 32,
                              ctypes.cast(ab, vp), 32)
    rk = _lib.BurstRxKeys(6, ctypes.cast(hb, vp), 64, 1, ctypes.cast(hb, vp), 64, 0,
                          c.cutoff, c.rx_start)
    d = _dev(c.data, dev)
    o, ln = _dev(c.offs.astype(np.int64), dev), _dev(_i32(c.lens), dev)
    sq, fl = _dev(_i32(c.seq), dev), _dev(_i32(c.flags), dev)
    iv, res = _dev(c.iv, dev), _dev(c.res_in, dev)
    plen = torch.zeros(c.n, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    rc = L.net2_packet_decrypt_burst(
        ctypes.byref(rk), ctypes.byref(ck), d.data_ptr(), o.data_ptr(), ln.data_ptr(),
        c.n, sq.data_ptr(), fl.data_ptr(), iv.data_ptr(), res.data_ptr(), d.data_ptr(),
        plen.data_ptr(), st)
    ctypes.memset(kb, 0xEE, 32)
    ctypes.memset(ab, 0xEE, 32)
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(res.cpu().numpy(), c.want_res)
    assert np.array_equal(plen.cpu().numpy().view(np.uint32), c.want_plen)
    # TX
    t = tx_case(6)
    kb = ctypes.create_string_buffer(t.key, 32)
    ck = _lib.BurstCipherKeys(_lib.ENC_AES256, ctypes.cast(kb, vp), 32, None, 0)
    d = _dev(t.data, dev)
    o, ln = _dev(t.offs.astype(np.int64), dev), _dev(_i32(t.lens), dev)
    fl, iv, pl = _dev(_i32(t.flags), dev), _dev(t.iv, dev), _dev(_i32(t.plen), dev)
    res = torch.full((t.n,), 9, dtype=torch.uint8, device=dev)
    wire = torch.zeros(t.n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    rc = L.net2_packet_encrypt_burst(
        ctypes.byref(ck), t.hl, fl.data_ptr(), iv.data_ptr(), d.data_ptr(),
        o.data_ptr(), ln.data_ptr(), pl.data_ptr(), t.n, res.data_ptr(),
        wire.data_ptr(), st)
    ctypes.memset(kb, 0xEE, 32)
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(res.cpu().numpy(), t.want_res)
    assert np.array_equal(d.cpu().numpy(), t.want)


# ---- paths of the kernels that the bursts above do not reach ------------------
#
# The tests below go through the C entry points with d_plen / d_wire_len
# pre-filled, so a datagram that no lane processed shows as a stale length.

STALE = 0x5A5A5A5A          # never a length the cipher can produce here
HASH6, HL6, PO6 = 6, 64, 72


def _bytes(rng, n):
    return rng.integers(0, 256, int(n), dtype=np.uint8).tobytes()


def _pack(lens, rng, lead=128, tail=128):
    """Offsets with `lead` bytes before the first datagram and `tail` after
    the last, 1..8 stray bytes between them; the total size."""
    offs = np.zeros(len(lens), dtype=np.uint64)
    cur = lead + int(rng.integers(0, 16))
    for i, ln in enumerate(lens):
        offs[i] = cur
        cur += int(ln) + int(rng.integers(1, 9))
    return offs, cur + tail


def _rx_datagrams(rng, hl, seq, flags, iv, plens, key_of):
    """Datagram i: header, a random hash field with PH_SIGNED, then the EVP
    ciphertext of plens[i] random bytes under key_of[i] and iv[i].  Returns
    (datagrams, plaintexts as EVP decrypts them again)."""
    dgs, plains = [], []
    for i in range(len(plens)):
        plain = _bytes(rng, plens[i])
        ct = aes_ref.encrypt(key_of[i], iv[i].tobytes(), plain)
        assert aes_ref.decrypt(key_of[i], iv[i].tobytes(), ct) == plain
        field = _bytes(rng, hl) if flags[i] & SIGNED else b""
        dgs.append(struct.pack(">II", int(seq[i]), int(flags[i])) + field + ct)
        plains.append(plain)
    return dgs, plains


def _fill(data, offs, dgs):
    for o, d in zip(offs, dgs):
        data[int(o):int(o) + len(d)] = np.frombuffer(d, dtype=np.uint8)


def _c_decrypt(dev, hash_alg, key, alt_key, no_cutoff, cutoff, rx_start, d, out,
               offs, lens, seq, flags, d_iv, res_in):
    """net2_packet_decrypt_burst itself, d_plen pre-filled with STALE.
    d, out, d_iv: device tensors; the rest host arrays.  Returns host
    (result, plen)."""
    from ilias_net2_amd import _lib
    L = _lib.lib()
    vp = ctypes.c_void_p
    n = len(offs)
    kb = ctypes.create_string_buffer(key, 32)
    ab = ctypes.create_string_buffer(alt_key, 32) if alt_key is not None else None
    hb = ctypes.create_string_buffer(64)
    ck = _lib.BurstCipherKeys(_lib.ENC_AES256, ctypes.cast(kb, vp), 32,
                              None if ab is None else ctypes.cast(ab, vp),
                              0 if ab is None else 32)
    rk = _lib.BurstRxKeys(hash_alg, ctypes.cast(hb, vp), HL[hash_alg], 1,
                          None if ab is None else ctypes.cast(hb, vp),
                          0 if ab is None else HL[hash_alg],
                          int(no_cutoff), cutoff, rx_start)
    o, ln = _dev(offs.astype(np.int64), dev), _dev(_i32(lens), dev)
    sq, fl = _dev(_i32(seq), dev), _dev(_i32(flags), dev)
    res = _dev(res_in, dev)
    plen = torch.full((n,), STALE, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    rc = L.net2_packet_decrypt_burst(
        ctypes.byref(rk), ctypes.byref(ck), d.data_ptr(), o.data_ptr(), ln.data_ptr(),
        n, sq.data_ptr(), fl.data_ptr(), d_iv.data_ptr(), res.data_ptr(),
        out.data_ptr(), plen.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return res.cpu().numpy(), plen.cpu().numpy().view(np.uint32)


def _c_encrypt(dev, key, hl, d, offs, lens, flags, d_iv, plen):
    """net2_packet_encrypt_burst itself, d_result pre-filled with 9 and
    d_wire_len with STALE.  Returns host (result, wire_len)."""
    from ilias_net2_amd import _lib
    L = _lib.lib()
    n = len(offs)
    kb = ctypes.create_string_buffer(key, 32)
    ck = _lib.BurstCipherKeys(_lib.ENC_AES256, ctypes.cast(kb, ctypes.c_void_p), 32,
                              None, 0)
    o, ln = _dev(offs.astype(np.int64), dev), _dev(_i32(lens), dev)
    fl, pl = _dev(_i32(flags), dev), _dev(_i32(plen), dev)
    res = torch.full((n,), 9, dtype=torch.uint8, device=dev)
    wire = torch.full((n,), STALE, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    rc = L.net2_packet_encrypt_burst(
        ctypes.byref(ck), hl, fl.data_ptr(), d_iv.data_ptr(), d.data_ptr(),
        o.data_ptr(), ln.data_ptr(), pl.data_ptr(), n, res.data_ptr(),
        wire.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return res.cpu().numpy(), wire.cpu().numpy().view(np.uint32)


def _po(flags, hl):
    return np.where((flags & SIGNED) != 0, 8 + hl, 8).astype(np.int64)


def _check_rx(got_res, got_plen, got, before, offs, lens, po, want_res, want_plen,
              plains):
    """Every code and length; every plaintext byte; and every other byte of
    the output as it was (`before`), but for the padding a decrypted datagram
    leaves behind its plaintext, which the header leaves unspecified."""
    bad = np.nonzero(got_res != want_res)[0]
    assert len(bad) == 0, [(int(i), int(got_res[i]), int(want_res[i])) for i in bad[:8]]
    bad = np.nonzero(got_plen != want_plen)[0]
    assert len(bad) == 0, [(int(i), hex(got_plen[i]), int(want_plen[i])) for i in bad[:8]]
    want = before.copy()
    care = np.ones(len(before), dtype=bool)
    for i in np.nonzero((want_res == OK) & (lens > po))[0]:
        if plains[i] is None:
            continue
        a = int(offs[i]) + int(po[i])
        want[a:a + len(plains[i])] = np.frombuffer(plains[i], dtype=np.uint8)
        care[a + len(plains[i]):int(offs[i]) + int(lens[i])] = False
    bad = np.nonzero((got != want) & care)[0]
    assert len(bad) == 0, bad[:8]


def _sized_plens(n, pattern):
    i = np.arange(n)
    if pattern == "ties":           # three blocks each: every rank is a tie
        return np.full(n, 40, dtype=np.uint32)
    if pattern == "descending":     # 93 blocks down to 1, then again
        return (16 * (92 - i % 93) + i % 16).astype(np.uint32)
    return np.array([PLENS[k % len(PLENS)] for k in i], dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def sized_case(n, pattern):
    """n datagrams under row 6 with an alternate key, an IV of its own each;
    about 1 in 8 has no cipher work (RX: not PH_ENCRYPTED, or arrives BAD;
    TX: not PH_ENCRYPTED, or a byte short of room)."""
    rng = np.random.default_rng([4500, n, len(pattern)])
    key, alt_key = _keys(rng)
    rx_start, cutoff = 0xffffff80, 0x00000040       # the window wraps
    seq = ((rx_start + np.arange(n)) & 0xffffffff).astype(np.uint32)
    flags = np.full(n, ENC | SIGNED, dtype=np.uint32)
    flags[rng.random(n) < 0.25] |= ALTKEY
    flags[rng.random(n) < 0.2] &= ~np.uint32(SIGNED)
    idle = np.where(rng.random(n) < 0.125, 1 + np.arange(n) % 2, 0)
    flags[idle == 1] &= ~np.uint32(ENC)
    iv = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    plens = _sized_plens(n, pattern)
    nblk = plens // 16 + 1
    if pattern == "ties":
        assert len(set(nblk)) == 1
    elif pattern == "descending":
        assert n < 2 or (np.diff(nblk.astype(np.int64))[np.arange(1, n) % 93 != 0] == -1).all()
    picks = np.array([P.ref_rx_key(int(seq[i]), int(flags[i]), True, False, cutoff,
                                   rx_start) for i in range(n)])
    po = _po(flags, HL6)
    # RX
    dgs, plains = _rx_datagrams(rng, HL6, seq, flags, iv, plens,
                                [alt_key if p else key for p in picks])
    rx_lens = np.array([len(d) for d in dgs], dtype=np.uint32)
    rx_offs, total = _pack(rx_lens, rng)
    rx_data = rng.integers(0, 256, total, dtype=np.uint8)
    _fill(rx_data, rx_offs, dgs)
    res_in = np.where(idle == 2, BAD, OK).astype(np.uint8)
    live = (idle == 0)
    rx_plen = np.where(live, plens, 0).astype(np.uint32)
    rx_plains = [plains[i] if live[i] else None for i in range(n)]
    # TX: the same plaintexts in slots with exactly the room, or a byte short
    tx_lens = (po + 16 * nblk - (idle == 2)).astype(np.uint32)
    tx_offs, total = _pack(tx_lens, rng)
    tx_data = rng.integers(0, 256, total, dtype=np.uint8)
    tx_want = None
    for fill_ct in (False, True):
        for i in range(n):
            a = int(tx_offs[i]) + int(po[i])
            if not fill_ct:
                tx_data[a:a + len(plains[i])] = np.frombuffer(plains[i], dtype=np.uint8)
            elif live[i]:
                ct = aes_ref.encrypt(key, iv[i].tobytes(), plains[i])
                tx_want[a:a + len(ct)] = np.frombuffer(ct, dtype=np.uint8)
        if not fill_ct:
            tx_want = tx_data.copy()
    tx_res = np.where(idle == 2, RESOURCE, OK).astype(np.uint8)
    tx_wire = np.where(live, po + 16 * nblk, np.where(idle == 1, po + plens, 0)
                       ).astype(np.uint32)
    for a in (seq, flags, iv, plens, rx_lens, rx_offs, rx_data, res_in, rx_plen,
              tx_lens, tx_offs, tx_data, tx_want, tx_res, tx_wire):
        a.setflags(write=False)
    return types.SimpleNamespace(
        n=n, key=key, alt_key=alt_key, rx_start=rx_start, cutoff=cutoff, seq=seq,
        flags=flags, iv=iv, plens=plens, po=po, picks=picks, rx_lens=rx_lens,
        rx_offs=rx_offs, rx_data=rx_data, res_in=res_in, rx_plen=rx_plen,
        rx_plains=rx_plains, tx_lens=tx_lens, tx_offs=tx_offs, tx_data=tx_data,
        tx_want=tx_want, tx_res=tx_res, tx_wire=tx_wire)


@pytest.mark.parametrize("pattern", ["ties", "descending", "cycle"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513])
def test_burst_sizes_and_rank_ties(dev, n, pattern):
    """lanes_by_work hands each lane the datagram of its rank among the
    workgroup's 256: bursts that end on, one short of and one past a wave and
    a workgroup, with block counts that all tie, that reverse the lanes, and
    the usual mix -- idle lanes among them.  A rank that collides or skips
    leaves a datagram with its stale length."""
    c = sized_case(n, pattern)
    d = _dev(c.rx_data, dev)
    res, plen = _c_decrypt(dev, HASH6, c.key, c.alt_key, False, c.cutoff, c.rx_start,
                           d, d, c.rx_offs, c.rx_lens, c.seq, c.flags,
                           _dev(c.iv, dev), c.res_in)
    _check_rx(res, plen, d.cpu().numpy(), c.rx_data, c.rx_offs, c.rx_lens, c.po,
              c.res_in, c.rx_plen, c.rx_plains)
    d = _dev(c.tx_data, dev)
    res, wire = _c_encrypt(dev, c.key, HL6, d, c.tx_offs, c.tx_lens, c.flags,
                           _dev(c.iv, dev), c.plens)
    assert np.array_equal(res, c.tx_res)
    bad = np.nonzero(wire != c.tx_wire)[0]
    assert len(bad) == 0, [(int(i), hex(wire[i]), int(c.tx_wire[i])) for i in bad[:8]]
    bad = np.nonzero(d.cpu().numpy() != c.tx_want)[0]
    assert len(bad) == 0, bad[:8]


def _plain_rx(rng, n, flags, plens=None):
    """n valid datagrams under row 6, one key, no alternate: host arrays."""
    key, _ = _keys(rng)
    seq = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    iv = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    if plens is None:
        plens = np.array([PLENS[i % len(PLENS)] for i in range(n)], dtype=np.uint32)
    dgs, plains = _rx_datagrams(rng, HL6, seq, flags, iv, plens, [key] * n)
    return key, seq, iv, plens, dgs, plains


@pytest.mark.parametrize("in_place", [False, True])
def test_rx_incoming_codes_are_kept(dev, in_place):
    """A datagram that arrives with any code but OK -- RESOURCE (1), WINDOW
    (4), NET2_PBURST_NOCONN (5), and one no header names (255) -- keeps it,
    gets plen 0 and is not written, however valid its ciphertext."""
    rng = np.random.default_rng(4600)
    n = 70
    flags = np.full(n, ENC | SIGNED, dtype=np.uint32)
    flags[rng.random(n) < 0.3] &= ~np.uint32(SIGNED)
    key, seq, iv, plens, dgs, plains = _plain_rx(rng, n, flags)
    res_in = np.array([(OK, 1, 4, 5, 255)[i % 5] for i in range(n)], dtype=np.uint8)
    lens = np.array([len(d) for d in dgs], dtype=np.uint32)
    offs, total = _pack(lens, rng)
    data = rng.integers(0, 256, total, dtype=np.uint8)
    _fill(data, offs, dgs)
    d = _dev(data, dev)
    out = d if in_place else torch.full((total,), SENTINEL, dtype=torch.uint8, device=dev)
    res, plen = _c_decrypt(dev, HASH6, key, None, False, 0, 0, d, out, offs, lens, seq,
                           flags, _dev(iv, dev), res_in)
    kept = res_in != OK
    assert (plens[kept] > 0).sum() > 40
    before = data if in_place else np.full(total, SENTINEL, dtype=np.uint8)
    _check_rx(res, plen, out.cpu().numpy(), before, offs, lens, _po(flags, HL6), res_in,
              np.where(kept, 0, plens).astype(np.uint32),
              [None if kept[i] else plains[i] for i in range(n)])
    assert np.array_equal(d.cpu().numpy(), data) or in_place


@pytest.mark.parametrize("in_place", [False, True])
def test_rx_shorter_than_payload_offset(dev, in_place):
    """An OK, PH_ENCRYPTED datagram that ends before (or where) its payload
    starts has no ciphertext: BAD, plen 0, nothing written.  128 bytes of
    slack at both ends of the buffer."""
    rng = np.random.default_rng(4700)
    short = [(ENC | SIGNED, ln) for ln in (0, 5, 8, 9, 71, 72)] + \
            [(ENC, ln) for ln in (0, 7, 8)]
    n = 4 * len(short)
    flags = np.full(n, ENC | SIGNED, dtype=np.uint32)
    flags[2::4] = ENC
    key, seq, iv, plens, dgs, plains = _plain_rx(rng, n, flags)
    is_short = np.zeros(n, dtype=bool)
    for k, (fl, ln) in enumerate(short):
        i = 4 * k + 1 + k % 3               # not every fourth lane
        flags[i], is_short[i], plains[i] = fl, True, None
        dgs[i] = _bytes(rng, ln)
    lens = np.array([len(d) for d in dgs], dtype=np.uint32)
    assert sorted((int(flags[i]), int(lens[i])) for i in np.nonzero(is_short)[0]) == \
        sorted(short)
    offs, total = _pack(lens, rng, lead=128, tail=128)
    assert int(offs.min()) >= 128 and int((offs + lens).max()) + 128 <= total
    data = rng.integers(0, 256, total, dtype=np.uint8)
    _fill(data, offs, dgs)
    d = _dev(data, dev)
    out = d if in_place else torch.full((total,), SENTINEL, dtype=torch.uint8, device=dev)
    res, plen = _c_decrypt(dev, HASH6, key, None, False, 0, 0, d, out, offs, lens, seq,
                           flags, _dev(iv, dev), np.zeros(n, dtype=np.uint8))
    before = data if in_place else np.full(total, SENTINEL, dtype=np.uint8)
    _check_rx(res, plen, out.cpu().numpy(), before, offs, lens, _po(flags, HL6),
              np.where(is_short, BAD, OK).astype(np.uint8),
              np.where(is_short, 0, plens).astype(np.uint32), plains)


def test_tx_length_extremes(dev):
    """d_plen near 2^32 in a slot of ordinary size: the ciphertext length
    does not fit 32 bits, so the room check must be made in 64: RESOURCE,
    wire_len 0, the slot untouched; without PH_ENCRYPTED RESOURCE and
    untouched (wire_len unspecified).  The slots around them as EVP says."""
    rng = np.random.default_rng(4800)
    huge = [0xFFFFFFFF, 0xFFFFFFF0, 0xFFFFFFEF, 0x80000000]
    n = 64
    key, _ = _keys(rng)
    flags = np.full(n, ENC | SIGNED, dtype=np.uint32)
    flags[rng.random(n) < 0.3] &= ~np.uint32(SIGNED)
    iv = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    plen = np.array([PLENS[i % len(PLENS)] for i in range(n)], dtype=np.uint32)
    at = {}
    for k, (pl, fl) in enumerate((p, f) for p in huge
                                 for f in (ENC | SIGNED, ENC, SIGNED, 0)):
        i = 3 * k + 2
        plen[i], flags[i] = pl, fl
        at[i] = (pl, fl)
    assert len(at) == 16 and max(at) < n
    po = _po(flags, HL6)
    lens = np.array([int(rng.integers(100, 1501)) if i in at else
                     po[i] + 16 * (int(plen[i]) // 16 + 1) for i in range(n)],
                    dtype=np.uint32)
    offs, total = _pack(lens, rng)
    data = rng.integers(0, 256, total, dtype=np.uint8)
    want = data.copy()
    want_res = np.zeros(n, dtype=np.uint8)
    want_wire = np.zeros(n, dtype=np.uint32)
    for i in range(n):
        if i in at:
            want_res[i] = RESOURCE
            continue
        a = int(offs[i]) + int(po[i])
        ct = aes_ref.encrypt(key, iv[i].tobytes(), data[a:a + int(plen[i])].tobytes())
        want[a:a + len(ct)] = np.frombuffer(ct, dtype=np.uint8)
        want_wire[i] = po[i] + len(ct)
    d = _dev(data, dev)
    res, wire = _c_encrypt(dev, key, HL6, d, offs, lens, flags, _dev(iv, dev), plen)
    assert np.array_equal(res, want_res), res
    stated = np.array([i not in at or bool(flags[i] & ENC) for i in range(n)])
    assert np.array_equal(wire[stated], want_wire[stated])
    bad = np.nonzero(d.cpu().numpy() != want)[0]
    assert len(bad) == 0, bad[:8]


@pytest.mark.parametrize("iv_at", [1, 3, 8])
def test_unaligned_iv_array(dev, iv_at):
    """d_iv is 16 bytes per datagram at any address: a contiguous slice that
    starts 1, 3 or 8 bytes into its allocation, RX and TX."""
    c = sized_case(65, "cycle")
    room = torch.full((iv_at + 16 * c.n + 16,), SENTINEL, dtype=torch.uint8, device=dev)
    d_iv = room[iv_at:iv_at + 16 * c.n]
    d_iv.copy_(_dev(c.iv, dev).reshape(-1))
    assert d_iv.is_contiguous() and d_iv.data_ptr() % 16 == iv_at
    d = _dev(c.rx_data, dev)
    res, plen = _c_decrypt(dev, HASH6, c.key, c.alt_key, False, c.cutoff, c.rx_start,
                           d, d, c.rx_offs, c.rx_lens, c.seq, c.flags, d_iv, c.res_in)
    _check_rx(res, plen, d.cpu().numpy(), c.rx_data, c.rx_offs, c.rx_lens, c.po,
              c.res_in, c.rx_plen, c.rx_plains)
    d = _dev(c.tx_data, dev)
    res, wire = _c_encrypt(dev, c.key, HL6, d, c.tx_offs, c.tx_lens, c.flags, d_iv,
                           c.plens)
    assert np.array_equal(res, c.tx_res) and np.array_equal(wire, c.tx_wire)
    assert np.array_equal(d.cpu().numpy(), c.tx_want)
    got = room.cpu().numpy()
    assert (got[:iv_at] == SENTINEL).all() and (got[iv_at + 16 * c.n:] == SENTINEL).all()
    assert np.array_equal(got[iv_at:iv_at + 16 * c.n], c.iv.reshape(-1))


def above_4gib_case():
    """130 datagrams of the PLENS cycle under row 6 with an alternate key, in
    three groups of a buffer of 2^32 + 2^16 bytes, and a compact host copy of
    the windows of that buffer that the test uses (see test_chain_above_4gib)."""
    G4 = 1 << 32
    size = G4 + (1 << 16)
    rng = np.random.default_rng(4900)
    n, hash_alg, hl, po = 130, HASH6, HL6, PO6
    hkey, halt = _bytes(rng, hl), _bytes(rng, hl)
    ekey, ealt = _keys(rng)
    rx_start, cutoff = 5000, 5090
    seq = (rx_start + np.arange(n)).astype(np.uint32)
    flags = np.full(n, ENC | SIGNED, dtype=np.uint32)
    flags[rng.random(n) < 0.3] |= ALTKEY
    picks = np.array([P.ref_rx_key(int(seq[i]), int(flags[i]), True, False, cutoff,
                                   rx_start) for i in range(n)])
    assert 20 < picks.sum() < n - 20
    plen = np.array([PLENS[i % len(PLENS)] for i in range(n)], dtype=np.uint32)
    lens = (po + 16 * (plen // 16 + 1)).astype(np.uint32)
    # group i % 3 holds datagram i, so every wave works in all three regions
    group = np.arange(n) % 3
    starts = [64, G4 - 700, G4 + 5 + (1 << 15)]
    offs = np.zeros(n, dtype=np.uint64)
    wins = []                               # [lo, hi) of each group's window
    for g in range(3):
        cur = starts[g]
        for i in np.nonzero(group == g)[0]:
            offs[i] = cur
            cur += int(lens[i]) + int(rng.integers(1, 9))
        wins.append((max(starts[g] - 4096, 0), cur + 4096))
    wins[0] = (0, max(wins[0][1], 1 << 16))  # the first 64 KiB, all of it
    assert wins[0][1] <= wins[1][0] and wins[1][1] <= wins[2][0] and wins[2][1] <= size
    ends = offs + lens
    assert ((offs < G4) & (ends > G4)).sum() == 1           # one straddles
    assert (offs >= G4).sum() > 40 and (offs[group == 2] % 16 != 0).any()
    # a compact host copy: the three windows one after the other
    base = np.cumsum([0] + [hi - lo for lo, hi in wins])
    c_offs = np.array([int(offs[i]) - wins[group[i]][0] + int(base[group[i]])
                       for i in range(n)], dtype=np.uint64)
    data = rng.integers(0, 256, int(base[3]), dtype=np.uint8)
    plains = [data[int(c_offs[i]) + po:int(c_offs[i]) + po + int(plen[i])].tobytes()
              for i in range(n)]
    return types.SimpleNamespace(
        n=n, size=size, hkey=hkey, halt=halt, ekey=ekey, ealt=ealt, rx_start=rx_start,
        cutoff=cutoff, seq=seq, flags=flags, picks=picks, plen=plen, lens=lens,
        offs=offs, wins=wins, base=base, c_offs=c_offs, data=data, plains=plains)


@pytest.mark.parametrize("form", list(HASH_FORMS))
def test_chain_above_4gib(dev, oracle_mod, hash_form, form):
    """The whole chain (IVs, encrypt, seal, verify, decrypt) in place on one
    stream over a buffer of 2^32 + 2^16 bytes: a group of datagrams near
    offset 64, one packed from 2^32 - 700 on so that a datagram straddles
    2^32, and one above 2^32 at odd offsets (from 2^32 + 5 + 32 KiB: the
    straddling group ends past 2^32 + 5).  Every kernel takes 64-bit offsets;
    an offset cut to 32 bits would land in the first 64 KiB, which is
    compared as well, with 4 KiB on either side of every group.  Only the
    windows used are ever written or read.  The hash bursts in each of their
    forms (at the default limits 130 datagrams take the wave form alone):
    hmac_kernel's burst modes, burst_prep_kernel and burst_final_kernel see
    these offsets in the lane and binned forms, on prepared workspaces."""
    from ilias_net2_amd import _lib, cipher_burst
    L = _lib.lib()
    hash_form(form)
    free, _ = torch.cuda.mem_get_info(dev)
    if free < (8 << 30):
        pytest.skip("needs 8 GiB of free device memory")
    c = above_4gib_case()
    n, hash_alg, hl, po = c.n, HASH6, HL6, PO6
    hkey, halt, ekey, ealt = c.hkey, c.halt, c.ekey, c.ealt
    rx_start, cutoff, seq, flags, picks = c.rx_start, c.cutoff, c.seq, c.flags, c.picks
    plen, lens, offs, wins, base, c_offs = c.plen, c.lens, c.offs, c.wins, c.base, c.c_offs
    data, plains, size = c.data, c.plains, c.size

    def windows(t):
        return np.concatenate([t[lo:hi].cpu().numpy() for lo, hi in wins])

    big = torch.empty(size, dtype=torch.uint8, device=dev)
    for k, (lo, hi) in enumerate(wins):
        big[lo:hi].copy_(_dev(data[int(base[k]):int(base[k + 1])], dev))
    s = torch.cuda.Stream(device=dev)
    d_seq, d_fl = _dev(_i32(seq), dev), _dev(_i32(flags), dev)
    d_off, d_len = _dev(offs.astype(np.int64), dev), _dev(_i32(lens), dev)
    d_plen = _dev(_i32(plen), dev)
    sets = []
    for alt in (False, True):
        idx = np.nonzero(picks == alt)[0]
        sets.append((idx, _dev(idx.astype(np.int64), dev), halt if alt else hkey,
                     ealt if alt else ekey))
    torch.cuda.synchronize()
    tx_out = []
    with torch.cuda.stream(s):
        for idx, d_idx, hk, ek in sets:
            m = len(idx)
            g_seq, g_fl = d_seq[d_idx].contiguous(), d_fl[d_idx].contiguous()
            g_off, g_len = d_off[d_idx].contiguous(), d_len[d_idx].contiguous()
            g_plen = d_plen[d_idx].contiguous()
            iv = torch.empty((m, 16), dtype=torch.uint8, device=dev)
            _lib.check(L.net2_ph_to_iv_dev(g_seq.data_ptr(), g_fl.data_ptr(), m, 16,
                                           iv.data_ptr(), s.cuda_stream))
            eres, wire = cipher_burst.encrypt_burst(ek, hl, g_fl, iv, big, g_off, g_len,
                                                    g_plen, stream=s)
            ws = torch.empty(L.net2_packet_burst_workspace(m), dtype=torch.uint8,
                             device=dev)
            _lib.check(L.net2_sha2_workspace_init(ws.data_ptr(), ws.numel(),
                                                  s.cuda_stream))
            sres = torch.empty(m, dtype=torch.uint8, device=dev)
            _lib.check(L.net2_packet_encode_burst(
                hash_alg, hk, hl, 1, g_seq.data_ptr(), g_fl.data_ptr(), big.data_ptr(),
                g_off.data_ptr(), wire.data_ptr(), m, sres.data_ptr(), ws.data_ptr(),
                ws.numel(), s.cuda_stream))
            tx_out.append((eres, wire, sres, ws, iv))
        sealed = [big[lo:hi].clone() for lo, hi in wins]
        res = torch.full((n,), 9, dtype=torch.uint8, device=dev)
        iv = torch.zeros((n, 16), dtype=torch.uint8, device=dev)
        r_seq = torch.empty(n, dtype=torch.int32, device=dev)
        r_fl = torch.empty(n, dtype=torch.int32, device=dev)
        ws = torch.empty(L.net2_packet_burst_workspace(n), dtype=torch.uint8, device=dev)
        _lib.check(L.net2_sha2_workspace_init(ws.data_ptr(), ws.numel(), s.cuda_stream))
        kb, ab = ctypes.create_string_buffer(hkey, hl), ctypes.create_string_buffer(halt, hl)
        ks = _lib.BurstRxKeys(hash_alg, ctypes.cast(kb, ctypes.c_void_p), hl, 1,
                              ctypes.cast(ab, ctypes.c_void_p), hl, 0, cutoff, rx_start)
        _lib.check(L.net2_packet_decode_burst_ck(
            ctypes.byref(ks), 16, big.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n,
            res.data_ptr(), iv.data_ptr(), r_seq.data_ptr(), r_fl.data_ptr(),
            ws.data_ptr(), ws.numel(), s.cuda_stream))
        res, out, got_plen = cipher_burst.decrypt_burst(
            hash_alg, ekey, big, d_off, d_len, r_seq, r_fl, iv, res, alt_key=ealt,
            alt_cutoff=cutoff, rx_start=rx_start, out=big, stream=s)
    s.synchronize()
    assert out is big

    # sealed: EVP ciphertexts, then the oracle's header and HMAC, per key set
    ivs = oracle_mod.ph_to_iv_batch(seq, flags, 16)
    want = data.copy()
    for i in range(n):
        ct = aes_ref.encrypt(ealt if picks[i] else ekey, ivs[i].tobytes(), plains[i])
        a = int(c_offs[i]) + po
        assert len(ct) == int(lens[i]) - po
        want[a:a + len(ct)] = np.frombuffer(ct, dtype=np.uint8)
    for (idx, _, hk, _), (eres, wire, sres, _, _) in zip(sets, tx_out):
        assert (eres.cpu().numpy() == OK).all() and (sres.cpu().numpy() == OK).all()
        assert np.array_equal(wire.cpu().numpy().view(np.uint32), lens[idx])
        r, sealed_ref = oracle_mod.packet_encode_batch(hash_alg, hk, True, seq[idx],
                                                       flags[idx], want, c_offs[idx],
                                                       lens[idx])
        assert (r == OK).all()
        for i in idx:
            a, b = int(c_offs[i]), int(c_offs[i]) + int(lens[i])
            want[a:b] = sealed_ref[a:b]
    got = np.concatenate([t.cpu().numpy() for t in sealed])
    for k in range(3):                      # window by window
        a, b = int(base[k]), int(base[k + 1])
        bad = np.nonzero(got[a:b] != want[a:b])[0]
        assert len(bad) == 0, (k, bad[:8] + wins[k][0])
    # RX: every datagram verifies and decrypts to its plaintext, in place
    assert np.array_equal(r_seq.cpu().numpy().view(np.uint32), seq)
    assert np.array_equal(r_fl.cpu().numpy().view(np.uint32), flags)
    assert np.array_equal(iv.cpu().numpy(), ivs)
    _check_rx(res.cpu().numpy(), got_plen.cpu().numpy().view(np.uint32), windows(big),
              want, c_offs, lens, np.full(n, po, dtype=np.int64),
              np.zeros(n, dtype=np.uint8), plen, plains)
    del big, sealed
    torch.cuda.empty_cache()
