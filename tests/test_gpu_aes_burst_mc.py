"""The payload cipher under per-connection keys on the GPU:
net2_burst_ciphertab_* and net2_packet_{decrypt,encrypt}_burst_mc against the
system libcrypto's EVP_aes_256_cbc (tests/aes_ref.py), per datagram under that
datagram's own connection's key -- a corrupted ciphertext expects whatever EVP
says of it.

Shapes: n in {1, 255, 256, 257, 513} (the workgroup edge and the ranking
across it), K in {1, 2, 5, 257} connections with the slots dealt out so that
every wave mixes keys, ciphertexts of 1, 2 and 89 blocks mixed, ties included.
As in test_gpu_aes_burst.py one thing is checked more strictly than the header
promises: a datagram that ends BAD, NOCONN or RESOURCE is not written at all.
"""
import ctypes
import functools
import struct
import types

import numpy as np
import pytest

import aes_ref
import test_gpu_packet as P
from test_gpu_aes_burst import lane_form  # noqa: F401  (autouse: the lane form)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

OK, RESOURCE, BAD, UNSAFE, NOCONN = 0, 1, 2, 3, 5
ENC, SIGNED, ALTKEY = P.PH_ENCRYPTED, P.PH_SIGNED, P.PH_ALTKEY
HL = P.HL
SENTINEL = 0xA5
STALE = 0x5A5A5A5A          # never a length the cipher can produce here
NBLK = (1, 2, 89)           # 89 blocks: the payload of a 1,500-byte datagram
vp = ctypes.c_void_p


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


def _bytes(rng, n):
    return rng.integers(0, 256, int(n), dtype=np.uint8).tobytes()


def _pack(lens, rng):
    """Offsets at every alignment, 1..8 stray bytes between the datagrams,
    64 bytes of slack at both ends; the total size."""
    offs = np.zeros(len(lens), dtype=np.uint64)
    cur = 64 + int(rng.integers(0, 16))
    for i, ln in enumerate(lens):
        offs[i] = cur
        cur += int(ln) + int(rng.integers(1, 9))
    return offs, cur + 64


def _po(flags, hl):
    return np.where((flags & SIGNED) != 0, 8 + hl, 8).astype(np.int64)


def _nblk(n, rng):
    """1, 2 and 89 blocks mixed: runs of equal counts (ties) and every count
    in every wave."""
    nb = np.array([NBLK[(i // 2 + i // 7) % 3] for i in range(n)])
    if n >= 3:
        assert set(nb) == set(NBLK) and (nb[:-1] == nb[1:]).any()
    return nb


def _connections(K, hash_alg, rng):
    """K connections' cipher key state.  With a keyed hash, by k mod 4: no
    alternate key; an alternate key whose window start lies within 16 of
    2^32; one without a cutoff; one with a cutoff in mid-range."""
    slots = K + 3
    slot_of = rng.permutation(slots)[:K]
    conns = []
    for k in range(K):
        kind = k % 4 if hash_alg else 0
        rx_start = (0, 0xfffffff8, 5000, 0x40000000 + 977 * k)[kind]
        conns.append(types.SimpleNamespace(
            slot=int(slot_of[k]), key=_bytes(rng, 32), tx_key=_bytes(rng, 32),
            alt_key=_bytes(rng, 32) if kind else None, no_cutoff=kind == 2,
            rx_start=rx_start, cutoff=(rx_start + 40) & 0xffffffff))
    unset = [int(s) for s in sorted(set(range(slots)) - set(int(s) for s in slot_of))]
    return conns, slots, unset


def _deal(n, K):
    """Connection of datagram i: neighbours differ, so a wave mixes keys."""
    return np.array([(5 * i + i // 3) % K for i in range(n)])


def _picks(c_of, conns, seq, flags):
    return np.array([P.ref_rx_key(int(seq[i]), int(flags[i]),
                                  conns[k].alt_key is not None, conns[k].no_cutoff,
                                  conns[k].cutoff, conns[k].rx_start)
                     for i, k in enumerate(c_of)], dtype=bool)


@functools.lru_cache(maxsize=None)
def rx_case(n, K, hash_alg):
    """One received burst of n datagrams over K connections and what EVP makes
    of every datagram under its own connection's key.  About 1 in 12 each:
    a damaged last block, a ragged ciphertext, no PH_ENCRYPTED, an incoming
    code that is not OK, a connection the table does not have.  Built once;
    the tests leave it unchanged."""
    rng = np.random.default_rng([5100, n, K, hash_alg])
    hl = HL[hash_alg]
    conns, slots, unset = _connections(K, hash_alg, rng)
    c_of = _deal(n, K)
    nb = _nblk(n, rng)
    kind = rng.permutation(n) % 12 if n > 1 else np.array([11])
    # seq on both sides of the connection's cutoff (40 past its window start)
    seq = np.array([(conns[k].rx_start + int(rng.integers(0, 80))) & 0xffffffff
                    for k in c_of], dtype=np.uint32)
    flags = np.full(n, ENC, dtype=np.uint32)
    if hash_alg:
        flags[rng.random(n) < 0.6] |= SIGNED
        flags[rng.random(n) < 0.25] |= ALTKEY
    flags[kind == 2] &= ~np.uint32(ENC)
    res_in = np.where(kind == 3, np.array([BAD, UNSAFE, NOCONN, 4])[np.arange(n) % 4],
                      OK).astype(np.uint8)
    conn = np.array([conns[k].slot for k in c_of], dtype=np.uint32)
    missing = [slots, 0xffffffff, slots + 7] + unset
    for j, i in enumerate(np.nonzero(kind == 4)[0]):
        conn[i] = missing[j % len(missing)]
    iv = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    picks = _picks(c_of, conns, seq, flags)
    key_of = [conns[k].alt_key if picks[i] else conns[k].key for i, k in enumerate(c_of)]
    dgs, cts = [], []
    for i in range(n):
        plain = _bytes(rng, 16 * (nb[i] - 1) + (5 * i) % 16)
        ct = aes_ref.encrypt(key_of[i], iv[i].tobytes(), plain)
        assert len(ct) == 16 * nb[i]
        if kind[i] == 0:                    # a damaged last block: EVP decides
            b = bytearray(ct)
            b[len(b) - 1 - i % 16] ^= 1 << (i % 8)
            ct = bytes(b)
        elif kind[i] == 1:
            ct = ct + _bytes(rng, 1 + i % 15) if i % 2 else ct[:len(ct) - 1 - i % 15]
        field = _bytes(rng, hl) if flags[i] & SIGNED else b""
        dgs.append(struct.pack(">II", int(seq[i]), int(flags[i])) + field + ct)
        cts.append(ct)
    lens = np.array([len(d) for d in dgs], dtype=np.uint32)
    offs, total = _pack(lens, rng)
    data = rng.integers(0, 256, total, dtype=np.uint8)
    for o, d in zip(offs, dgs):
        data[int(o):int(o) + len(d)] = np.frombuffer(d, dtype=np.uint8)
    po = _po(flags, hl)
    want_res = res_in.copy()
    want_plen = np.zeros(n, dtype=np.uint32)
    want_plain = [None] * n
    written = np.zeros(total, dtype=bool)       # payloads of decrypted datagrams
    for i in range(n):
        if res_in[i] != OK or not flags[i] & ENC:
            continue
        if kind[i] == 4:
            want_res[i] = NOCONN
            continue
        got = aes_ref.decrypt(key_of[i], iv[i].tobytes(), cts[i])
        if got is None:
            want_res[i] = BAD
            continue
        want_plen[i], want_plain[i] = len(got), got
        written[int(offs[i]) + int(po[i]):int(offs[i]) + int(lens[i])] = True
    if n >= 255:
        assert (want_res[kind == 0] == BAD).sum() > 5 and (want_res[kind == 1] == BAD).all()
        assert (want_res == NOCONN).sum() - (res_in == NOCONN).sum() > 5
        assert len(set(int(o) % 16 for o in offs)) == 16
        if hash_alg and K >= 2:
            assert 10 < picks.sum() < n - 10
    for a in (data, offs, lens, seq, flags, iv, res_in, conn, want_res, want_plen, written):
        a.setflags(write=False)
    return types.SimpleNamespace(
        n=n, K=K, hash_alg=hash_alg, hl=hl, conns=conns, slots=slots, c_of=c_of,
        picks=picks, kind=kind, conn=conn, seq=seq, flags=flags, iv=iv, data=data,
        offs=offs, lens=lens, po=po, res_in=res_in, want_res=want_res,
        want_plen=want_plen, want_plain=want_plain, written=written, total=total)


def _table(c, hash_alg, rx=True, tx=True):
    from ilias_net2_amd import cipher_burst
    tab = cipher_burst.CipherTable(c.slots)
    for k in c.conns:
        if rx:
            tab.set_rx(k.slot, k.key, hash_alg=hash_alg, alt_key=k.alt_key,
                       alt_no_cutoff=k.no_cutoff, alt_cutoff=k.cutoff,
                       rx_start=k.rx_start)
        if tx:
            tab.set_tx(k.slot, k.tx_key)
    return tab


def _decrypt_mc(dev, c, tab, in_place, conn=None):
    """net2_packet_decrypt_burst_mc itself, d_plen pre-filled with STALE."""
    from ilias_net2_amd import _lib
    d = _dev(c.data, dev)
    out = d if in_place else torch.full((c.total,), SENTINEL, dtype=torch.uint8,
                                        device=dev)
    o, ln = _dev(c.offs.astype(np.int64), dev), _dev(_i32(c.lens), dev)
    sq, fl = _dev(_i32(c.seq), dev), _dev(_i32(c.flags), dev)
    cn = _dev(_i32(c.conn if conn is None else conn), dev)
    iv, res = _dev(c.iv, dev), _dev(c.res_in, dev)
    plen = torch.full((c.n,), STALE, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    _lib.check(_lib.lib().net2_packet_decrypt_burst_mc(
        tab.ptr, cn.data_ptr(), c.hl, d.data_ptr(), o.data_ptr(), ln.data_ptr(), c.n,
        sq.data_ptr(), fl.data_ptr(), iv.data_ptr(), res.data_ptr(), out.data_ptr(),
        plen.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return res.cpu().numpy(), out.cpu().numpy(), plen.cpu().numpy().view(np.uint32)


def _check_rx(c, res, out, plen, in_place):
    bad = np.nonzero(res != c.want_res)[0]
    assert len(bad) == 0, [(int(i), int(c.kind[i]), int(res[i]), int(c.want_res[i]))
                           for i in bad[:8]]
    bad = np.nonzero(plen != c.want_plen)[0]
    assert len(bad) == 0, [(int(i), int(c.kind[i]), hex(plen[i])) for i in bad[:8]]
    for i in range(c.n):
        if c.want_plain[i] is not None:
            a = int(c.offs[i]) + int(c.po[i])
            assert out[a:a + int(plen[i])].tobytes() == c.want_plain[i], (i, c.kind[i])
    # nothing outside the payloads of the decrypted datagrams is written: BAD,
    # NOCONN and kept-code datagrams in full, and every byte between datagrams
    untouched = ~c.written
    if in_place:
        assert np.array_equal(out[untouched], c.data[untouched])
    else:
        assert (out[untouched] == SENTINEL).all()


# (n, K, hash_alg): every n, K and digest length; K = 257 > 256 lanes
SHAPES = [(1, 1, 0), (255, 2, 4), (256, 5, 5), (257, 257, 6), (513, 5, 6),
          (513, 257, 0), (513, 1, 4), (513, 2, 5)]


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("n,K,hash_alg", SHAPES)
def test_rx_mixed_keys(dev, n, K, hash_alg, in_place):
    c = rx_case(n, K, hash_alg)
    with _table(c, hash_alg, tx=False) as tab:
        res, out, plen = _decrypt_mc(dev, c, tab, in_place)
    _check_rx(c, res, out, plen, in_place)


@functools.lru_cache(maxsize=None)
def tx_case(n, K, hash_alg):
    """Slots to encrypt under each connection's tx key: exactly the room, a
    byte short, room to spare; with and without PH_ENCRYPTED and PH_SIGNED;
    about 1 in 12 with a connection the table does not have -- among them
    slots a byte short (RESOURCE wins) and slots without PH_ENCRYPTED
    (processed whatever their conn)."""
    rng = np.random.default_rng([5200, n, K, hash_alg])
    hl = HL[hash_alg]
    conns, slots, unset = _connections(K, hash_alg, rng)
    c_of = _deal(n, K)
    nb = _nblk(n, rng)
    flags = np.full(n, ENC, dtype=np.uint32)
    flags[rng.random(n) < 0.2] &= ~np.uint32(ENC)
    if hash_alg:
        flags[rng.random(n) < 0.6] |= SIGNED
    iv = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    plen = np.array([16 * (nb[i] - 1) + (5 * i) % 16 for i in range(n)], dtype=np.uint32)
    room = rng.permutation(n) % 8 if n > 1 else np.array([1])      # 0: a byte short
    po = _po(flags, hl)
    lens = np.zeros(n, dtype=np.uint32)
    for i in range(n):
        need = int(po[i]) + (16 * nb[i] if flags[i] & ENC else int(plen[i]))
        lens[i] = need - 1 if room[i] == 0 else need + (0 if room[i] <= 4 else
                                                        int(rng.integers(1, 40)))
    conn = np.array([conns[k].slot for k in c_of], dtype=np.uint32)
    missing = [slots, 0xffffffff, slots + 7] + unset
    lost = (rng.permutation(n) % 12 == 0) if n > 1 else np.array([False])
    enc = (flags & ENC) != 0
    for sel in (enc & (room == 0), ~enc & (room != 0)):     # two of each for certain
        lost[np.nonzero(sel)[0][:2]] = True
    for j, i in enumerate(np.nonzero(lost)[0]):
        conn[i] = missing[j % len(missing)]
    offs, total = _pack(lens, rng)
    data = rng.integers(0, 256, total, dtype=np.uint8)
    want = data.copy()
    want_res = np.zeros(n, dtype=np.uint8)
    want_wire = np.zeros(n, dtype=np.uint32)
    stated = np.ones(n, dtype=bool)             # wire_len is specified
    for i in range(n):
        a = int(offs[i]) + int(po[i])
        if not flags[i] & ENC:
            want_wire[i] = po[i] + plen[i]
            want_res[i] = RESOURCE if want_wire[i] > lens[i] else OK
            stated[i] = want_res[i] == OK
        elif po[i] + 16 * nb[i] > lens[i]:
            want_res[i] = RESOURCE
        elif lost[i]:
            want_res[i] = NOCONN
        else:
            ct = aes_ref.encrypt(conns[c_of[i]].tx_key, iv[i].tobytes(),
                                 data[a:a + int(plen[i])].tobytes())
            want[a:a + len(ct)] = np.frombuffer(ct, dtype=np.uint8)
            want_wire[i] = po[i] + len(ct)
    if n >= 255:
        assert (want_res == NOCONN).sum() > 5
        assert (lost & enc & (want_res == RESOURCE)).sum() >= 1
        assert (lost & ~enc & (want_res == OK)).sum() >= 1
        assert (enc & (want_res == OK) & (room >= 1) & (room <= 4)).sum() > 50
    for a in (data, offs, lens, flags, iv, plen, conn, want, want_res, want_wire):
        a.setflags(write=False)
    return types.SimpleNamespace(
        n=n, K=K, hl=hl, conns=conns, slots=slots, c_of=c_of, conn=conn, flags=flags,
        iv=iv, plen=plen, lens=lens, offs=offs, data=data, want=want,
        want_res=want_res, want_wire=want_wire, stated=stated)


def _encrypt_mc(dev, c, tab, conn=None):
    """net2_packet_encrypt_burst_mc itself, d_result pre-filled with 9 and
    d_wire_len with STALE."""
    from ilias_net2_amd import _lib
    d = _dev(c.data, dev)
    o, ln = _dev(c.offs.astype(np.int64), dev), _dev(_i32(c.lens), dev)
    fl, pl, iv = _dev(_i32(c.flags), dev), _dev(_i32(c.plen), dev), _dev(c.iv, dev)
    cn = _dev(_i32(c.conn if conn is None else conn), dev)
    res = torch.full((c.n,), 9, dtype=torch.uint8, device=dev)
    wire = torch.full((c.n,), STALE, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    _lib.check(_lib.lib().net2_packet_encrypt_burst_mc(
        tab.ptr, cn.data_ptr(), c.hl, fl.data_ptr(), iv.data_ptr(), d.data_ptr(),
        o.data_ptr(), ln.data_ptr(), pl.data_ptr(), c.n, res.data_ptr(),
        wire.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return res.cpu().numpy(), wire.cpu().numpy().view(np.uint32), d.cpu().numpy()


@pytest.mark.parametrize("n,K,hash_alg", SHAPES)
def test_tx_mixed_keys(dev, n, K, hash_alg):
    c = tx_case(n, K, hash_alg)
    with _table(c, hash_alg, rx=False) as tab:
        res, wire, got = _encrypt_mc(dev, c, tab)
    bad = np.nonzero(res != c.want_res)[0]
    assert len(bad) == 0, [(int(i), int(res[i]), int(c.want_res[i])) for i in bad[:8]]
    bad = np.nonzero((wire != c.want_wire) & c.stated)[0]
    assert len(bad) == 0, [(int(i), hex(wire[i]), int(c.want_wire[i])) for i in bad[:8]]
    # every ciphertext byte; every other byte -- RESOURCE and NOCONN slots in
    # full -- as it was
    bad = np.nonzero(got != c.want)[0]
    assert len(bad) == 0, bad[:8]


@pytest.mark.parametrize("alt", [False, True])
def test_one_connection_equals_the_single_connection_calls(dev, alt):
    """The same bursts through decrypt_burst / encrypt_burst and through a
    one-slot table: codes, lengths and every byte of the buffers identical."""
    from ilias_net2_amd import cipher_burst
    hash_alg = 6 if alt else 4
    c = rx_case(513, 1, hash_alg)
    k = c.conns[0]
    if alt:         # K = 1 has no alternate key of its own: install one
        k = types.SimpleNamespace(**{**vars(k), "alt_key": bytes(range(7, 39)),
                                     "cutoff": (int(c.seq.min()) + 60) & 0xffffffff,
                                     "rx_start": int(c.seq.min())})
        assert 50 < sum(P.ref_rx_key(int(s), int(f), True, False, k.cutoff, k.rx_start)
                        for s, f in zip(c.seq, c.flags)) < c.n - 50
    conn = np.zeros(c.n, dtype=np.uint32)
    args = lambda: (_dev(c.offs.astype(np.int64), dev), _dev(_i32(c.lens), dev),  # noqa: E731
                    _dev(_i32(c.seq), dev), _dev(_i32(c.flags), dev), _dev(c.iv, dev),
                    _dev(c.res_in, dev))
    outs = []
    with cipher_burst.CipherTable(1) as tab:
        tab.set_rx(0, k.key, hash_alg=hash_alg, alt_key=k.alt_key,
                   alt_cutoff=k.cutoff, rx_start=k.rx_start)
        tab.set_tx(0, k.tx_key)
        for mc in (False, True):
            d = _dev(c.data, dev)
            out = torch.full((c.total,), SENTINEL, dtype=torch.uint8, device=dev)
            if mc:
                r = cipher_burst.decrypt_burst_mc(tab, _dev(_i32(conn), dev), c.hl, d,
                                                  *args(), out=out)
            else:
                r = cipher_burst.decrypt_burst(hash_alg, k.key, d, *args(),
                                               alt_key=k.alt_key, alt_cutoff=k.cutoff,
                                               rx_start=k.rx_start, out=out)
            torch.cuda.synchronize()
            outs.append([x.cpu().numpy() for x in r])
        for a, b in zip(*outs):
            assert np.array_equal(a, b)
        assert (outs[0][0] == OK).sum() > 100 and (outs[0][0] == BAD).sum() > 20
        # TX
        t = tx_case(513, 1, hash_alg)
        conn = _dev(_i32(np.zeros(t.n, dtype=np.uint32)), dev)
        outs = []
        for mc in (False, True):
            d = _dev(t.data, dev)
            a = (_dev(_i32(t.flags), dev), _dev(t.iv, dev), d,
                 _dev(t.offs.astype(np.int64), dev), _dev(_i32(t.lens), dev),
                 _dev(_i32(t.plen), dev))
            r = (cipher_burst.encrypt_burst_mc(tab, conn, t.hl, *a) if mc else
                 cipher_burst.encrypt_burst(k.tx_key, t.hl, *a))
            torch.cuda.synchronize()
            outs.append([x.cpu().numpy() for x in r] + [d.cpu().numpy()])
        for a, b in zip(*outs):
            assert np.array_equal(a, b)
        assert (outs[0][0] == OK).sum() > 300 and (outs[0][0] == RESOURCE).sum() > 20


def test_alternate_keys_per_connection(dev):
    """Five connections: two without an alternate key, one whose window
    starts within 16 of 2^32, one without a cutoff, one with a cutoff in
    mid-range; datagrams on both sides of each cutoff, with and without
    PH_ALTKEY.  A wrong choice decrypts under the wrong key: BAD where EVP
    says OK."""
    c = rx_case(513, 5, 6)
    live = (c.res_in == OK) & ((c.flags & ENC) != 0) & (c.kind > 4)
    for k, cn in enumerate(c.conns):
        mine = live & (c.c_of == k)
        flag = (c.flags & ALTKEY) != 0
        past = ((c.seq.astype(np.int64) - cn.rx_start) & 0xffffffff) >= 40
        for f in (False, True):
            for p in (False, True):
                sel = mine & (flag == f) & (past == p)
                assert sel.sum() >= 2, (k, f, p)
                want = cn.alt_key is not None and (f or (p and not cn.no_cutoff))
                assert (c.picks[sel] == want).all(), (k, f, p)
        assert (c.want_res[mine] == OK).all()
    assert c.conns[1].rx_start >= 2**32 - 16 and c.conns[2].no_cutoff
    wrapped = live & (c.c_of == 1) & (c.seq < 0x1000)
    assert wrapped.sum() >= 5
    with _table(c, 6, tx=False) as tab:
        res, out, plen = _decrypt_mc(dev, c, tab, False)
    _check_rx(c, res, out, plen, False)


def test_missing_connections(dev):
    """conn = slots, conn = 0xffffffff, a slot never set, a slot with only the
    other side set, a cleared slot: NOCONN and untouched.  Incoming codes
    that are not OK are kept (5 included), and a slot without PH_ENCRYPTED is
    processed whatever its conn."""
    from ilias_net2_amd import cipher_burst
    c = rx_case(257, 5, 6)
    t = tx_case(257, 5, 6)
    assert c.slots == t.slots == 8
    # each direction's table: connection 0 with only the rx side set, 1 with
    # only the tx side, 2 set whole and cleared again, 3 and 4 whole
    for case, run in ((c, "rx"), (t, "tx")):
        with cipher_burst.CipherTable(case.slots) as tab:
            for k, cn in enumerate(case.conns):
                if k != 1:
                    tab.set_rx(cn.slot, cn.key, hash_alg=6, alt_key=cn.alt_key,
                               alt_no_cutoff=cn.no_cutoff, alt_cutoff=cn.cutoff,
                               rx_start=cn.rx_start)
                if k != 0:
                    tab.set_tx(cn.slot, cn.tx_key)
            tab.clear(case.conns[2].slot)
            if run == "rx":
                res, out, plen = _decrypt_mc(dev, c, tab, False)
            else:
                tres, twire, tgot = _encrypt_mc(dev, t, tab)
    rx_has = {c.conns[k].slot for k in (0, 3, 4)}
    tx_has = {t.conns[k].slot for k in (1, 3, 4)}
    # RX
    want_res, want_plen = c.want_res.copy(), c.want_plen.copy()
    written = c.written.copy()
    gone = np.array([int(s) not in rx_has for s in c.conn])
    hit = gone & (c.res_in == OK) & ((c.flags & ENC) != 0)
    want_res[hit], want_plen[hit] = NOCONN, 0
    for i in np.nonzero(hit)[0]:
        written[int(c.offs[i]):int(c.offs[i]) + int(c.lens[i])] = False
    assert hit.sum() > 60 and (want_res == OK).sum() > 40
    assert np.array_equal(res, want_res)
    assert np.array_equal(plen, want_plen)
    kept = c.res_in != OK
    assert set(c.res_in[kept]) == {BAD, UNSAFE, NOCONN, 4}
    assert np.array_equal(res[kept], c.res_in[kept]) and (plen[kept] == 0).all()
    for i in np.nonzero(want_plen)[0]:
        a = int(c.offs[i]) + int(c.po[i])
        assert out[a:a + int(plen[i])].tobytes() == c.want_plain[i], i
    assert (out[~written] == SENTINEL).all()
    # TX
    gone = np.array([int(s) not in tx_has for s in t.conn])
    hit = gone & ((t.flags & ENC) != 0) & (t.want_res != RESOURCE)
    want_res, want_wire, want = t.want_res.copy(), t.want_wire.copy(), t.want.copy()
    want_res[hit], want_wire[hit] = NOCONN, 0
    for i in np.nonzero(hit)[0]:
        a, b = int(t.offs[i]), int(t.offs[i]) + int(t.lens[i])
        want[a:b] = t.data[a:b]
    assert hit.sum() > 60 and ((t.flags & ENC) != 0)[want_res == OK].sum() > 40
    plainslots = gone & ((t.flags & ENC) == 0)
    assert plainslots.sum() > 10 and set(want_res[plainslots]) == {OK, RESOURCE}
    assert np.array_equal(tres, want_res)
    assert np.array_equal(twire[t.stated], want_wire[t.stated])
    assert np.array_equal(tgot, want)


def _ck(key):
    from ilias_net2_amd import _lib
    kb = ctypes.create_string_buffer(key, 32)
    return _lib.BurstCipherKeys(_lib.ENC_AES256, ctypes.cast(kb, vp), 32, None, 0), kb


def test_updates_are_stream_ordered(dev):
    """set A, bursts, set B, bursts ... on one side stream with no
    synchronisation; each host key buffer is overwritten as soon as its call
    returns.  Every burst sees the keys set before it on the stream; a slot
    set twice in a row ends with the second; set_rx leaves the tx side alone
    and set_tx the rx side."""
    from ilias_net2_amd import _lib, cipher_burst
    L = _lib.lib()
    rng = np.random.default_rng(5300)
    n, slot = 64, 2
    A, B, C, D = (_bytes(rng, 32) for _ in range(4))
    flags = np.full(n, ENC, dtype=np.uint32)
    iv = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    plen = np.array([(1, 17, 40)[i % 3] + i % 5 for i in range(n)], dtype=np.uint32)
    lens = (8 + 16 * (plen // 16 + 1)).astype(np.uint32)
    offs, total = _pack(lens, rng)
    plain = rng.integers(0, 256, total, dtype=np.uint8)

    def sealed(key):
        d = plain.copy()
        for i in range(n):
            a = int(offs[i]) + 8
            ct = aes_ref.encrypt(key, iv[i].tobytes(), plain[a:a + int(plen[i])].tobytes())
            d[a:a + len(ct)] = np.frombuffer(ct, dtype=np.uint8)
        return d

    want = {k: sealed(k) for k in (A, B, C, D)}
    s = torch.cuda.Stream(device=dev)
    o, ln = _dev(offs.astype(np.int64), dev), _dev(_i32(lens), dev)
    fl, d_iv, pl = _dev(_i32(flags), dev), _dev(iv, dev), _dev(_i32(plen), dev)
    conn = torch.full((n,), slot, dtype=torch.int32, device=dev)
    seq = torch.zeros(n, dtype=torch.int32, device=dev)
    d_plain = _dev(plain, dev)
    d_sealed = {k: _dev(want[k], dev) for k in want}
    torch.cuda.synchronize()
    rk = _lib.BurstRxKeys(0, None, 0, 1, None, 0, 0, 0, 0)
    got_tx, got_rx = [], []

    with cipher_burst.CipherTable(4) as tab:
        def set_rx(key):
            ck, kb = _ck(key)
            rc = L.net2_burst_ciphertab_set_rx(tab.ptr, slot, ctypes.byref(rk),
                                               ctypes.byref(ck), s.cuda_stream)
            ctypes.memset(kb, 0xEE, 32)
            assert rc == 0

        def set_tx(key):
            ck, kb = _ck(key)
            rc = L.net2_burst_ciphertab_set_tx(tab.ptr, slot, ctypes.byref(ck),
                                               s.cuda_stream)
            ctypes.memset(kb, 0xEE, 32)
            assert rc == 0

        def rx(key):
            """A burst sealed under `key`, decrypted with what the slot holds."""
            with torch.cuda.stream(s):
                d = d_sealed[key].clone()
                res = torch.zeros(n, dtype=torch.uint8, device=dev)
            got_rx.append(cipher_burst.decrypt_burst_mc(tab, conn, 0, d, o, ln, seq, fl,
                                                        d_iv, res, out=d, stream=s))

        def tx():
            with torch.cuda.stream(s):
                d = d_plain.clone()
            got_tx.append((d,) + cipher_burst.encrypt_burst_mc(tab, conn, 0, fl, d_iv, d,
                                                               o, ln, pl, stream=s))

        for step, key in ((set_rx, A), (set_tx, A), (rx, A), (tx, None),    # under A
                          (set_rx, B), (tx, None), (rx, B),     # tx still A, rx now B
                          (set_tx, B), (set_tx, C), (rx, B), (tx, None),    # rx still B, tx ends C
                          (set_rx, C), (set_rx, D), (rx, D),    # rx ends D
                          (rx, A)):                             # ... and no longer A
            step(*(() if key is None else (key,)))
        s.synchronize()
        for (d, res, wire), key in zip(got_tx, (A, A, C)):
            assert (res.cpu().numpy() == OK).all()
            assert np.array_equal(wire.cpu().numpy().view(np.uint32), lens)
            assert np.array_equal(d.cpu().numpy(), want[key])
        for j, (res, out, got_plen) in enumerate(got_rx[:4]):
            assert (res.cpu().numpy() == OK).all(), j
            assert np.array_equal(got_plen.cpu().numpy().view(np.uint32), plen), j
            g = out.cpu().numpy()
            for i in range(n):
                a = int(offs[i]) + 8
                assert np.array_equal(g[a:a + int(plen[i])], plain[a:a + int(plen[i])]), (j, i)
        # under the wrong key EVP's padding check fails for nearly every one
        assert (got_rx[4][0].cpu().numpy() == BAD).sum() > n - 8


def test_chain_on_one_stream(dev):
    """TX: ph_to_iv, encrypt_burst_mc, encode_burst_mc; RX: decode_burst_mc,
    decrypt_burst_mc -- a KeyTable and a CipherTable over the same conn, one
    stream, no synchronisation between the calls, n = 513, K = 5.  Plaintext
    out equals plaintext in; a datagram tampered with after sealing is BAD,
    one without a connection NOCONN in both steps."""
    from ilias_net2_amd import _lib, cipher_burst, conn_burst
    L = _lib.lib()
    rng = np.random.default_rng(5400)
    n, K, hash_alg, hl = 513, 5, 6, 64
    slots = K + 2
    hkeys = [_bytes(rng, hl) for _ in range(K)]
    ekeys = [_bytes(rng, 32) for _ in range(K)]
    c_of = _deal(n, K)
    conn = c_of.astype(np.uint32) + 1               # slots 1..K; 0 and K + 1 unset
    lost = np.arange(n) % 41 == 7
    conn[lost] = np.where(np.arange(n)[lost] % 2, 0, 0xffffffff)
    seq = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    flags = np.full(n, ENC | SIGNED, dtype=np.uint32)
    nb = _nblk(n, rng)
    plen = np.array([16 * (nb[i] - 1) + (5 * i) % 16 for i in range(n)], dtype=np.uint32)
    po = 8 + hl
    lens = (po + 16 * nb).astype(np.uint32)
    offs, total = _pack(lens, rng)
    data = rng.integers(0, 256, total, dtype=np.uint8)
    flip = np.nonzero((np.arange(n) % 29 == 3) & ~lost)[0]
    flip_at = np.array([int(offs[i]) + po + int(rng.integers(0, lens[i] - po))
                        for i in flip], dtype=np.int64)

    s = torch.cuda.Stream(device=dev)
    d = _dev(data, dev)
    d_conn, d_seq, d_fl = _dev(_i32(conn), dev), _dev(_i32(seq), dev), _dev(_i32(flags), dev)
    d_off, d_len = _dev(offs.astype(np.int64), dev), _dev(_i32(lens), dev)
    d_plen, d_flip = _dev(_i32(plen), dev), _dev(flip_at, dev)
    torch.cuda.synchronize()
    with conn_burst.KeyTable(hash_alg, slots) as ktab, \
            cipher_burst.CipherTable(slots) as ctab:
        with torch.cuda.stream(s):
            for k in range(K):
                ktab.set_rx(k + 1, hkeys[k], enc_set=True, stream=s)
                ktab.set_tx(k + 1, hkeys[k], enc_set=True, stream=s)
                ctab.set_rx(k + 1, ekeys[k], hash_alg=hash_alg, stream=s)
                ctab.set_tx(k + 1, ekeys[k], stream=s)
            iv = torch.empty((n, 16), dtype=torch.uint8, device=dev)
            _lib.check(L.net2_ph_to_iv_dev(d_seq.data_ptr(), d_fl.data_ptr(), n, 16,
                                           iv.data_ptr(), s.cuda_stream))
            eres, wire = cipher_burst.encrypt_burst_mc(ctab, d_conn, hl, d_fl, iv, d,
                                                       d_off, d_len, d_plen, stream=s)
            # a slot the cipher left out keeps its full length for the seal
            sres = conn_burst.encode_burst_mc(ktab, d_conn, d_seq, d_fl, d, d_off,
                                              torch.where(wire > 0, wire, d_len), stream=s)
            sealed = d.clone()
            d[d_flip] ^= 0x40
            res, r_iv, r_seq, r_fl = conn_burst.decode_burst_mc(ktab, d_conn, d, d_off,
                                                                d_len, ivlen=16, stream=s)
            out = torch.full((total,), SENTINEL, dtype=torch.uint8, device=dev)
            res, out, got_plen = cipher_burst.decrypt_burst_mc(
                ctab, d_conn, hl, d, d_off, d_len, r_seq, r_fl, r_iv, res, out=out,
                stream=s)
        s.synchronize()
    tampered = np.zeros(n, dtype=bool)
    tampered[flip] = True
    assert tampered.sum() > 10 and lost.sum() > 10
    want_tx = np.where(lost, NOCONN, OK)
    assert np.array_equal(eres.cpu().numpy(), want_tx)
    assert np.array_equal(sres.cpu().numpy(), want_tx)
    assert np.array_equal(wire.cpu().numpy().view(np.uint32), np.where(lost, 0, lens))
    # the ciphertexts on the wire are EVP's under each connection's key
    ivs = iv.cpu().numpy()
    sealed = sealed.cpu().numpy()
    for i in np.nonzero(~lost)[0][::7]:
        a = int(offs[i]) + po
        ct = aes_ref.encrypt(ekeys[c_of[i]], ivs[i].tobytes(),
                             data[a:a + int(plen[i])].tobytes())
        assert sealed[a:a + len(ct)].tobytes() == ct, i
    res, out, got_plen = res.cpu().numpy(), out.cpu().numpy(), got_plen.cpu().numpy()
    assert np.array_equal(res, np.where(lost, NOCONN, np.where(tampered, BAD, OK)))
    assert np.array_equal(got_plen.view(np.uint32), np.where(lost | tampered, 0, plen))
    written = np.zeros(total, dtype=bool)
    for i in np.nonzero(~(lost | tampered))[0]:
        a = int(offs[i]) + po
        assert np.array_equal(out[a:a + int(plen[i])], data[a:a + int(plen[i])]), i
        written[a:int(offs[i]) + int(lens[i])] = True
    assert (out[~written] == SENTINEL).all()
