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
def rx_case(oracle_mod, hash_alg, n=333):
    """One received burst under rx key state with (hash_alg != 0) or without
    an alternate key, and what EVP makes of every datagram.  Each kind in
    KINDS is 1/16 of the burst, spread over every wave; the other half are
    plain valid datagrams.  Built once per row; the tests leave it unchanged."""
    rng = np.random.default_rng(4100 + hash_alg)
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
    picks = np.array([P.ref_rx_key(int(seq[i]), int(flags[i]), has_alt, False,
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
        assert alt_by_flag.sum() > 10 and alt_by_cutoff.sum() > 10
        assert (~picks).sum() > 10
    for k in ("pad00", "pad11", "padrun", "ragged", "empty"):
        assert all(want_res[i] == BAD for i in range(n) if kinds[i] == k), k
    assert all(want_res[i] == OK and want_plen[i] % 16 == 0
               for i in range(n) if kinds[i] == "fullpad")
    for a in (data, offs, lens, seq, flags, iv, res_in, want_res, want_plen, written):
        a.setflags(write=False)
    return types.SimpleNamespace(
        n=n, hash_alg=hash_alg, hl=hl, key=key, alt_key=alt_key if has_alt else None,
        rx_start=rx_start, cutoff=cutoff, seq=seq, flags=flags, iv=iv, kinds=kinds,
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
        alt_cutoff=c.cutoff, rx_start=c.rx_start, out=out)
    torch.cuda.synchronize()
    assert plain is out
    return res.cpu().numpy(), plain.cpu().numpy(), plen.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("hash_alg", [4, 6, 0])
def test_rx_burst(dev, oracle_mod, hash_alg, in_place):
    """n = 333: two workgroups, a ragged last wave; rows 4 and 6 with an
    alternate key (by PH_ALTKEY and by the cutoff), and no keyed hash -- the
    instance without an alternate key."""
    c = rx_case(oracle_mod, hash_alg)
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


@pytest.mark.parametrize("hash_alg", [4, 6, 0])
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
    from ilias_net2_amd import _lib, cipher_burst
    L = _lib.lib()
    rng = np.random.default_rng(4400)
    n, hash_alg, hl = 200, 6, 64
    hkey, halt = (rng.integers(0, 256, hl, dtype=np.uint8).tobytes() for _ in range(2))
    ekey, ealt = _keys(rng)
    rx_start, cutoff = 1000, 1120
    seq = (rx_start + np.arange(n)).astype(np.uint32)
    flags = np.full(n, ENC | SIGNED, dtype=np.uint32)
    flags[rng.random(n) < 0.3] |= ALTKEY
    picks = np.array([P.ref_rx_key(int(seq[i]), int(flags[i]), True, False, cutoff,
                                   rx_start) for i in range(n)])
    assert 20 < picks.sum() < n - 20
    plen = np.array([PLENS[i % len(PLENS)] for i in range(n)], dtype=np.uint32)
    po = 8 + hl
    lens = (po + 16 * (plen // 16 + 1)).astype(np.uint32)
    offs, total = _place(lens, rng)
    data = rng.integers(0, 256, total, dtype=np.uint8)
    plains = [data[int(offs[i]) + po:int(offs[i]) + po + int(plen[i])].tobytes()
              for i in range(n)]
    flip = np.nonzero(rng.random(n) < 0.1)[0]       # tampered after sealing
    flip_at = np.array([int(offs[i]) + po + int(rng.integers(0, lens[i] - po))
                        for i in flip], dtype=np.int64)

    s = torch.cuda.Stream(device=dev)
    d = _dev(data, dev)
    d_flip = _dev(flip_at, dev)
    d_seq, d_fl = _dev(_i32(seq), dev), _dev(_i32(flags), dev)
    d_off, d_len = _dev(offs.astype(np.int64), dev), _dev(_i32(lens), dev)
    d_plen = _dev(_i32(plen), dev)
    groups = []
    for alt in (False, True):
        idx = np.nonzero(picks == alt)[0]
        groups.append((idx, _dev(idx.astype(np.int64), dev), halt if alt else hkey,
                       ealt if alt else ekey))
    torch.cuda.synchronize()                        # inputs are in place
    tx_out = []
    with torch.cuda.stream(s):
        for idx, d_idx, hk, ek in groups:
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
            tx_out.append((eres, wire, sres, ws))
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
                              ctypes.cast(ab, ctypes.c_void_p), hl, 0, cutoff, rx_start)
        _lib.check(L.net2_packet_decode_burst_ck(
            ctypes.byref(ks), 16, d.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n,
            res.data_ptr(), iv.data_ptr(), r_seq.data_ptr(), r_fl.data_ptr(),
            ws.data_ptr(), ws.numel(), s.cuda_stream))
        out = torch.full((total,), SENTINEL, dtype=torch.uint8, device=dev)
        res, out, got_plen = cipher_burst.decrypt_burst(
            hash_alg, ekey, d, d_off, d_len, r_seq, r_fl, iv, res, alt_key=ealt,
            alt_cutoff=cutoff, rx_start=rx_start, out=out, stream=s)
    s.synchronize()

    # the sealed datagrams are the oracle's over the helper-encrypted payloads
    ivs = oracle_mod.ph_to_iv_batch(seq, flags, 16)
    want = data.copy()
    for i in range(n):
        ct = aes_ref.encrypt(ealt if picks[i] else ekey, ivs[i].tobytes(), plains[i])
        a = int(offs[i]) + po
        want[a:a + len(ct)] = np.frombuffer(ct, dtype=np.uint8)
    for (idx, _, hk, _), (eres, wire, sres, _) in zip(groups, tx_out):
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
