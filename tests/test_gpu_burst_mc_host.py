"""Host bursts over many connections, with the payload cipher
(net2_packet_{decode,encode}_burst_mc_host, include/net2/packet.h): datagrams
in host memory, of many connections, encrypted, in one synchronous call.

The contract is a composition, and so is the reference: the device-resident
_mc sequence on the same bytes -- RX decode_burst_mc then decrypt_burst_mc, TX
ph_to_iv_dev, encrypt_burst_mc, then encode_burst_mc over wire_len -- which
every host call must equal bit for bit.  Each case's device-resident reference
is built once, shared and left unchanged, and when it is built it is itself
checked against an independent one: the oracle's packet_{decode,encode}_batch
per connection plus EVP's AES-256-CBC (tests/aes_ref.py).  Each case asserts on
that reference's own codes that more than half its datagrams are OK and that
the codes it is about are there.
"""
import ctypes
import errno
import os
import threading
import types

import numpy as np
import pytest

import aes_ref
import synth
import test_gpu_packet as P

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

OK, RESOURCE, BAD, UNSAFE, NOCONN = 0, 1, 2, 3, 5
ENC, SIGNED, ALTKEY = P.PH_ENCRYPTED, P.PH_SIGNED, P.PH_ALTKEY
HL = P.HL
SENT = 0xA5
STALE = 0x5A5A5A5A          # never a length the cipher can produce here
NBLK = (1, 2, 3, 4, 5, 8, 9, 92, 93)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FI_LIB = os.path.join(ROOT, "tests", "libnet2_sha2_fi.so")
FI_H2D, FI_KERNEL, FI_RECORD = 1, 2, 3
CPU_THREADS = min(16, len(os.sched_getaffinity(0)))
ns = types.SimpleNamespace


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a GPU (HIP device not visible)")
    from ilias_net2_amd import _lib
    assert _lib.device_count() >= 1
    return torch.device("cuda:0")


def _p(a):
    return None if a is None else a.ctypes.data


def _dev(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)


def _bytes(rng, n):
    return rng.integers(0, 256, int(n), dtype=np.uint8).tobytes()


def pinned(shape, dtype=np.uint8):
    """A page-locked host array (torch pin_memory), as a numpy view."""
    t = torch.empty(shape, dtype={np.uint8: torch.uint8, np.uint32: torch.int32,
                                  np.uint64: torch.int64}[dtype], pin_memory=True)
    return t.numpy().view(dtype)


def alloc(pin, shape, dtype=np.uint8, fill=SENT):
    a = pinned(shape, dtype) if pin else np.empty(shape, dtype=dtype)
    a.view(np.uint8)[...] = fill
    return a


# ---- connections and their tables ---------------------------------------------

def connections(K, hash_alg, rng, roll=()):
    """K connections, each with a slot of its own in both tables.  Those in
    `roll` are mid-rollover: their rx side holds an alternate HMAC key and an
    alternate cipher key, and a second slot's tx side seals with that pair (the
    transmitter picks the key set before it builds a datagram).  roll[0] has no
    cutoff (PH_ALTKEY alone selects), roll[1:] a cutoff 1,000 past the window
    start.  Besides: a slot never set, and one with an HMAC key in the key
    table but nothing in the cipher table."""
    hl = HL[hash_alg]
    slots = 2 * K + 4
    perm = [int(s) for s in rng.permutation(slots)]
    conns = []
    for k in range(K):
        rx_start = (0, 0xfffffc00, 5000, 0x40000000 + 977 * k)[k % 4]
        alt = None
        if k in roll:
            alt = ns(slot=perm[K + k], hkey=_bytes(rng, hl), ekey=_bytes(rng, 32),
                     no_cutoff=k == roll[0], cutoff=(rx_start + 1000) & 0xffffffff)
        conns.append(ns(slot=perm[k], hkey=_bytes(rng, hl), ekey=_bytes(rng, 32),
                        alt=alt, rx_start=rx_start))
    nocipher = ns(slot=perm[2 * K], hkey=_bytes(rng, hl), ekey=None, alt=None,
                  rx_start=0)
    unset = perm[2 * K + 1]
    # slot -> the keys its tx side seals with / the connection of its rx side
    tx, rx = {}, {}
    for c in conns + [nocipher]:
        tx[c.slot] = ns(hkey=c.hkey, ekey=c.ekey)
        rx[c.slot] = c
        if c.alt is not None:
            tx[c.alt.slot] = ns(hkey=c.alt.hkey, ekey=c.alt.ekey)
    return ns(K=K, hash_alg=hash_alg, hl=hl, slots=slots, conns=conns,
              nocipher=nocipher, unset=unset, tx=tx, rx=rx)


class Tables:
    """The key table and the cipher table of a set of connections."""

    def __init__(self, C, stream=None):
        from ilias_net2_amd import cipher_burst, conn_burst
        self.kt = conn_burst.KeyTable(C.hash_alg, C.slots)
        self.ct = cipher_burst.CipherTable(C.slots)
        for c in C.conns + [C.nocipher]:
            a = c.alt
            alt = dict(alt_no_cutoff=a.no_cutoff, alt_cutoff=a.cutoff) if a else {}
            self.kt.set_rx(c.slot, c.hkey, enc_set=True, rx_start=c.rx_start,
                           alt_key=a.hkey if a else None, stream=stream, **alt)
            self.kt.set_tx(c.slot, c.hkey, enc_set=True, stream=stream)
            if c.ekey is not None:
                self.ct.set_rx(c.slot, c.ekey, hash_alg=C.hash_alg, rx_start=c.rx_start,
                               alt_key=a.ekey if a else None, stream=stream, **alt)
                self.ct.set_tx(c.slot, c.ekey, stream=stream)
            if a is not None:
                self.kt.set_tx(a.slot, a.hkey, enc_set=True, stream=stream)
                self.ct.set_tx(a.slot, a.ekey, stream=stream)
        torch.cuda.synchronize()

    def close(self):
        self.kt.close()
        self.ct.close()


# ---- the bursts ------------------------------------------------------------------

TX_FAULTS = ("unset", "range", "nocipher", "noroom", "noenc", "nosigned")
RX_FAULTS = ("payload", "field", "runt", "ragged", "badpad", "noenc", "nosigned")


def tx_burst(C, n, seed, nblk=NBLK, faults=True):
    """n slots to send over C's connections, neighbours on different ones,
    byte-aligned with 3-byte gaps.  One slot in five is a fault (TX_FAULTS in
    turn): a connection the tables do not have -- never set, out of range, an
    HMAC key without a cipher key -- a slot a byte short, PH_ENCRYPTED or
    PH_SIGNED cleared.  Connections mid-rollover send every other datagram
    under their alternate keys."""
    rng = np.random.default_rng([7100, n, C.K, C.hash_alg, seed])
    hl = C.hl
    c_of = np.array([(5 * i + i // 3) % C.K for i in range(n)])
    kind = np.array([TX_FAULTS[(i // 5) % len(TX_FAULTS)] if faults and i % 5 == 4
                     else "" for i in range(n)])
    conn = np.zeros(n, dtype=np.uint32)     # the slot that seals
    rx_conn = np.zeros(n, dtype=np.uint32)  # the slot that receives
    seq = np.zeros(n, dtype=np.uint32)
    flags = np.full(n, ENC | SIGNED, dtype=np.uint32)
    for i in range(n):
        c = C.conns[c_of[i]]
        conn[i] = rx_conn[i] = c.slot
        seq[i] = (c.rx_start + int(rng.integers(0, 900))) & 0xffffffff
        if c.alt is not None and (i // C.K) % 2:
            conn[i] = c.alt.slot
            if c.alt.no_cutoff:
                flags[i] |= ALTKEY
            else:
                seq[i] = (c.alt.cutoff + int(rng.integers(0, 900))) & 0xffffffff
    for name, slot in (("unset", C.unset), ("nocipher", C.nocipher.slot)):
        conn[kind == name] = rx_conn[kind == name] = slot
    far = np.nonzero(kind == "range")[0]
    conn[far] = rx_conn[far] = np.where(far % 2, C.slots, 0xffffffff)
    flags[kind == "noenc"] &= ~np.uint32(ENC)
    flags[kind == "nosigned"] &= ~np.uint32(SIGNED)
    nb = np.array([nblk[(i + i // 11) % len(nblk)] for i in range(n)])
    plen = (16 * (nb - 1) + (5 * np.arange(n)) % 16).astype(np.uint32)
    po = np.where(flags & SIGNED, 8 + hl, 8)
    need = po + np.where(flags & ENC, 16 * nb, plen)
    lens = (need + np.where(np.arange(n) % 4 == 0, rng.integers(0, 24, n), 0))
    lens[kind == "noroom"] = need[kind == "noroom"] - 1
    lens = lens.astype(np.uint32)
    data, offs = synth.packed(7200 + seed, lens, align=1, gap=3)
    offs = offs.astype(np.uint64)
    for a in (conn, rx_conn, seq, flags, plen, lens, offs, data):
        a.setflags(write=False)
    return ns(C=C, n=n, kind=kind, conn=conn, rx_conn=rx_conn, seq=seq, flags=flags,
              plen=plen, lens=lens, offs=offs, data=data, po=po)


def dev_tx(dev, T, tabs, cipher, lens=None, data=None):
    """The device-resident TX sequence over T's bytes on one stream."""
    from ilias_net2_amd import _lib, conn_burst
    L = _lib.lib()
    n = T.n
    d = _dev(T.data if data is None else data, dev)
    o, ln = _dev(_i64(T.offs), dev), _dev(_i32(T.lens if lens is None else lens), dev)
    cn, sq, fl = _dev(_i32(T.conn), dev), _dev(_i32(T.seq), dev), _dev(_i32(T.flags), dev)
    ws = conn_burst.burst_workspace(n, dev)
    s = torch.cuda.current_stream().cuda_stream
    res = torch.full((n,), 9, dtype=torch.uint8, device=dev)
    if not cipher:
        _lib.check(L.net2_packet_encode_burst_mc(
            tabs.kt.ptr, cn.data_ptr(), sq.data_ptr(), fl.data_ptr(), d.data_ptr(),
            o.data_ptr(), ln.data_ptr(), n, res.data_ptr(), ws.data_ptr(), ws.numel(), s))
        torch.cuda.synchronize()
        return ns(res=res.cpu().numpy(), data=d.cpu().numpy())
    pl = _dev(_i32(T.plen), dev)
    iv = torch.zeros((n, 16), dtype=torch.uint8, device=dev)
    eres = torch.full((n,), 9, dtype=torch.uint8, device=dev)
    wire = torch.full((n,), STALE, dtype=torch.int32, device=dev)
    _lib.check(L.net2_ph_to_iv_dev(sq.data_ptr(), fl.data_ptr(), n, 16, iv.data_ptr(), s))
    _lib.check(L.net2_packet_encrypt_burst_mc(
        tabs.ct.ptr, cn.data_ptr(), T.C.hl, fl.data_ptr(), iv.data_ptr(), d.data_ptr(),
        o.data_ptr(), ln.data_ptr(), pl.data_ptr(), n, eres.data_ptr(), wire.data_ptr(), s))
    _lib.check(L.net2_packet_encode_burst_mc(
        tabs.kt.ptr, cn.data_ptr(), sq.data_ptr(), fl.data_ptr(), d.data_ptr(),
        o.data_ptr(), wire.data_ptr(), n, res.data_ptr(), ws.data_ptr(), ws.numel(), s))
    torch.cuda.synchronize()
    e, r = eres.cpu().numpy(), res.cpu().numpy()
    return ns(res=np.where(e != OK, e, r), wire=wire.cpu().numpy().view(np.uint32),
              data=d.cpu().numpy())


def host_tx(L, T, tabs, cipher, pin, outpin, lens=None, data=None, stream=None, rc=0):
    """net2_packet_encode_burst_mc_host over a copy of T's bytes."""
    src = T.data if data is None else data
    buf = alloc(pin, src.shape)
    buf[:] = src
    res = alloc(outpin, (T.n,))
    wire = alloc(outpin, (T.n,), np.uint32)
    got = L.net2_packet_encode_burst_mc_host(
        tabs.kt.ptr, tabs.ct.ptr if cipher else None, _p(T.conn), _p(T.seq), _p(T.flags),
        _p(buf), _p(T.offs), _p(T.lens if lens is None else lens),
        _p(T.plen) if cipher else None, T.n, _p(res), _p(wire) if cipher else None,
        stream)
    assert got == rc, got
    return ns(res=res, wire=wire, data=buf)


def indep_tx(T, idx, oracle_mod):
    """The TX sequence of datagrams idx restated: EVP under the sealing slot's
    cipher key, then the oracle's packet_encode under its HMAC key.  Returns
    codes, wire lengths and each slot's bytes."""
    C, hl = T.C, T.C.hl
    ivs = oracle_mod.ph_to_iv_batch(T.seq[idx], T.flags[idx], 16, nthreads=1)
    codes, wires, slots = [], [], []
    for j, i in enumerate(idx):
        f, ln, pl = int(T.flags[i]), int(T.lens[i]), int(T.plen[i])
        po = 8 + (hl if f & SIGNED else 0)
        a = int(T.offs[i])
        b = bytearray(T.data[a:a + ln].tobytes())
        tk = C.tx.get(int(T.conn[i]))
        if not f & ENC:
            wire = po + pl
            code = RESOURCE if wire > ln else OK
            assert code == OK       # (no such slot here: see tx_burst)
        elif po + 16 * (pl // 16 + 1) > ln:
            code, wire = RESOURCE, 0
        elif tk is None or tk.ekey is None:
            code, wire = NOCONN, 0
        else:
            ct = aes_ref.encrypt(tk.ekey, bytes(ivs[j]), bytes(b[po:po + pl]))
            b[po:po + len(ct)] = ct
            code, wire = OK, po + len(ct)
        if code == OK:
            if tk is None:
                code = NOCONN
            else:
                r, sealed = oracle_mod.packet_encode_batch(
                    C.hash_alg, tk.hkey, True, T.seq[i:i + 1], T.flags[i:i + 1],
                    np.frombuffer(bytes(b), dtype=np.uint8), np.zeros(1, np.uint64),
                    np.array([wire], np.uint32), nthreads=1)
                code, b = int(r[0]), bytearray(sealed.tobytes())
        codes.append(code)
        wires.append(wire)
        slots.append(bytes(b))
    return np.array(codes, dtype=np.uint8), np.array(wires, dtype=np.uint32), slots


def check_tx_ref(T, ref, idx, oracle_mod):
    codes, wires, slots = indep_tx(T, idx, oracle_mod)
    assert np.array_equal(ref.res[idx], codes), \
        [(int(i), T.kind[i], int(ref.res[i]), int(c)) for i, c in zip(idx, codes)
         if ref.res[i] != c][:8]
    assert np.array_equal(ref.wire[idx], wires)
    for i, b in zip(idx, slots):
        a = int(T.offs[i])
        assert ref.data[a:a + len(b)].tobytes() == b, (int(i), T.kind[i])


def rx_burst(T, tx, seed, oracle_mod, faults=True):
    """What T's sealed slots look like off the wire: lengths are the wire
    lengths, and one datagram in five is damaged (RX_FAULTS in turn): a
    payload or hash-field byte flipped, cut to a runt, a ragged ciphertext or
    one with bad padding under a valid HMAC, PH_ENCRYPTED or PH_SIGNED cleared
    in the header.  A slot the cipher step left out keeps its length; those of
    the connection with an HMAC key but no cipher key are sealed here, so that
    they reach the cipher step."""
    C, hl = T.C, T.C.hl
    rng = np.random.default_rng([7300, T.n, seed])
    data = tx.data.copy()
    lens = np.where(tx.wire > 0, tx.wire, T.lens).astype(np.uint32)

    def seal(i, b, newlen):
        r, sealed = oracle_mod.packet_encode_batch(
            C.hash_alg, C.tx[int(T.conn[i])].hkey, True, T.seq[i:i + 1], T.flags[i:i + 1],
            np.frombuffer(bytes(b), dtype=np.uint8), np.zeros(1, np.uint64),
            np.array([newlen], np.uint32), nthreads=1)
        assert r[0] == OK
        data[int(T.offs[i]):int(T.offs[i]) + len(b)] = sealed
        lens[i] = newlen

    for i in np.nonzero(T.kind == "nocipher")[0]:
        a = int(T.offs[i])
        seal(i, data[a:a + int(lens[i])].tobytes(), int(lens[i]))
    kind = np.array([RX_FAULTS[(i // 5) % len(RX_FAULTS)]
                     if faults and i % 5 == 3 and tx.res[i] == OK else ""
                     for i in range(T.n)])
    for i in np.nonzero(kind != "")[0]:
        a, k = int(T.offs[i]), kind[i]
        f, po = int(T.flags[i]), int(T.po[i])
        if k == "payload":
            data[a + po + int(rng.integers(0, lens[i] - po))] ^= 1 << (i % 8)
        elif k == "field":
            data[a + 8 + int(rng.integers(0, hl))] ^= 1 << (i % 8)
        elif k == "runt":
            lens[i] = i % 8
        elif k in ("ragged", "badpad"):
            tk = C.tx[int(T.conn[i])]
            clen = int(lens[i]) - po
            b = bytearray(data[a:a + int(lens[i])].tobytes())
            if k == "ragged":
                newlen = int(lens[i]) - 1 - i % 15
            else:
                iv = oracle_mod.ph_to_iv_batch(T.seq[i:i + 1], T.flags[i:i + 1], 16,
                                               nthreads=1)
                plain = _bytes(rng, clen - 1) + bytes([(0, 17, 0xff)[i % 3]])
                b[po:] = aes_ref.encrypt(tk.ekey, bytes(iv[0]), plain, pad=False)
                newlen = int(lens[i])
            seal(i, b, newlen)
        else:
            data[a + 7] &= 0xff ^ (ENC if k == "noenc" else SIGNED)
    for x in (data, lens):
        x.setflags(write=False)
    return ns(C=C, n=T.n, T=T, kind=kind, conn=T.rx_conn, offs=T.offs, lens=lens, data=data)


def dev_rx(dev, R, tabs, cipher, ivlen=16):
    """The device-resident RX sequence over R's bytes on one stream, the cipher
    step in place."""
    from ilias_net2_amd import _lib, conn_burst
    L = _lib.lib()
    n = R.n
    d, o, ln = _dev(R.data, dev), _dev(_i64(R.offs), dev), _dev(_i32(R.lens), dev)
    cn = _dev(_i32(R.conn), dev)
    ws = conn_burst.burst_workspace(n, dev)
    s = torch.cuda.current_stream().cuda_stream
    res = torch.full((n,), 9, dtype=torch.uint8, device=dev)
    iv = torch.zeros((n, max(ivlen, 1)), dtype=torch.uint8, device=dev)
    sq = torch.zeros(n, dtype=torch.int32, device=dev)
    fl = torch.zeros(n, dtype=torch.int32, device=dev)
    _lib.check(L.net2_packet_decode_burst_mc(
        tabs.kt.ptr, cn.data_ptr(), ivlen, d.data_ptr(), o.data_ptr(), ln.data_ptr(), n,
        res.data_ptr(), iv.data_ptr() if ivlen else None, sq.data_ptr(), fl.data_ptr(),
        ws.data_ptr(), ws.numel(), s))
    torch.cuda.synchronize()
    ref = ns(hres=res.cpu().numpy(), iv=iv.cpu().numpy(),
             seq=sq.cpu().numpy().view(np.uint32), fl=fl.cpu().numpy().view(np.uint32))
    ref.res = ref.hres
    # an IV is due where the hash step's code is OK and PH_ENCRYPTED is set
    # (every connection with an rx side here has a cipher key set)
    ref.iv_due = (ref.hres == OK) & ((ref.fl & ENC) != 0)
    if cipher:
        plen = torch.full((n,), STALE, dtype=torch.int32, device=dev)
        _lib.check(L.net2_packet_decrypt_burst_mc(
            tabs.ct.ptr, cn.data_ptr(), R.C.hl, d.data_ptr(), o.data_ptr(), ln.data_ptr(),
            n, sq.data_ptr(), fl.data_ptr(), iv.data_ptr(), res.data_ptr(), d.data_ptr(),
            plen.data_ptr(), s))
        torch.cuda.synchronize()
        ref.res = res.cpu().numpy()
        ref.plen = plen.cpu().numpy().view(np.uint32)
        ref.out = d.cpu().numpy()
        # the plaintexts, and what follows each inside its datagram
        ref.plain = np.zeros(len(R.data), dtype=bool)
        ref.tail = np.zeros(len(R.data), dtype=bool)
        po = np.where(ref.fl & SIGNED, 8 + R.C.hl, 8)
        for i in np.nonzero((ref.res == OK) & ref.iv_due)[0]:
            a = int(R.offs[i]) + int(po[i])
            ref.plain[a:a + int(ref.plen[i])] = True
            ref.tail[a + int(ref.plen[i]):int(R.offs[i]) + int(R.lens[i])] = True
    return ref


def host_rx(L, R, tabs, cipher, pin, outpin, in_place=True, ivlen=16, stream=None,
            rc=0, hdr=True):
    """net2_packet_decode_burst_mc_host over a copy of R's bytes."""
    n = R.n
    buf = alloc(pin, R.data.shape)
    buf[:] = R.data
    g = ns(res=alloc(outpin, (n,)), iv=alloc(outpin, (n, max(ivlen, 1))),
           seq=alloc(outpin, (n,), np.uint32) if hdr else None,
           fl=alloc(outpin, (n,), np.uint32) if hdr else None,
           plen=alloc(outpin, (n,), np.uint32), data=buf)
    g.out = buf if in_place else alloc(pin, R.data.shape)
    got = L.net2_packet_decode_burst_mc_host(
        tabs.kt.ptr, tabs.ct.ptr if cipher else None, _p(R.conn), ivlen, _p(buf),
        _p(R.offs), _p(R.lens), n, _p(g.res), _p(g.iv) if ivlen else None, _p(g.seq),
        _p(g.fl), _p(g.out) if cipher else None, _p(g.plen) if cipher else None, stream)
    assert got == rc, got
    return g


def check_rx(R, g, ref, cipher, in_place, upto=None):
    """Every output of a host RX call against the device-resident sequence
    (of the first `upto` datagrams)."""
    m = slice(0, upto)
    bad = np.nonzero(g.res[m] != ref.res[m])[0]
    assert len(bad) == 0, [(int(i), R.kind[i], int(g.res[i]), int(ref.res[i]))
                           for i in bad[:8]]
    if g.seq is not None:
        assert np.array_equal(g.seq[m], ref.seq[m]) and np.array_equal(g.fl[m], ref.fl[m])
    due = ref.iv_due[m]
    assert np.array_equal(g.iv[m][due], ref.iv[m][due])
    if not cipher:
        assert np.array_equal(g.data, R.data)
        return
    assert np.array_equal(g.plen[m], ref.plen[m])
    end = len(R.data) if upto is None else int(R.offs[upto - 1] + R.lens[upto - 1])
    plain, free = ref.plain[:end], ref.tail[:end]
    assert np.array_equal(g.out[:end][plain], ref.out[:end][plain])
    rest = ~(plain | free)
    if in_place:
        assert np.array_equal(g.out[:end][rest], R.data[:end][rest])
    else:
        assert (g.out[:end][rest] == SENT).all()
        assert np.array_equal(g.data, R.data)


def indep_rx(R, idx, oracle_mod):
    """The RX sequence of datagrams idx restated: the oracle's packet_decode
    under the receiving slot's key state, then EVP under the cipher key that
    net2_ck_rx_key's rule picks.  Returns codes after the hash step, final
    codes, headers, IVs and plaintexts (None: not decrypted)."""
    C, hl = R.C, R.C.hl
    m = len(idx)
    hres = np.zeros(m, dtype=np.uint8)
    seq, fl = np.zeros(m, dtype=np.uint32), np.zeros(m, dtype=np.uint32)
    iv = np.zeros((m, 16), dtype=np.uint8)
    slot_of = R.conn[idx]
    for slot in np.unique(slot_of):
        sel = np.nonzero(slot_of == slot)[0]
        c = C.rx.get(int(slot))
        if c is None:
            for j in sel:
                a, ln = int(R.offs[idx[j]]), int(R.lens[idx[j]])
                hres[j] = BAD if ln < 8 else NOCONN
                if ln >= 8:
                    seq[j] = int.from_bytes(R.data[a:a + 4].tobytes(), "big")
                    fl[j] = int.from_bytes(R.data[a + 4:a + 8].tobytes(), "big")
            continue
        a = c.alt
        r = oracle_mod.packet_decode_batch(
            C.hash_alg, c.hkey, True, 16, R.data, R.offs[idx[sel]], R.lens[idx[sel]],
            alt_key=a.hkey if a else None, alt_no_cutoff=bool(a and a.no_cutoff),
            alt_cutoff=a.cutoff if a else 0, rx_start=c.rx_start, nthreads=CPU_THREADS)
        hres[sel], iv[sel], seq[sel], fl[sel] = r
    res, plain = hres.copy(), [None] * m
    for j, i in enumerate(idx):
        if hres[j] != OK or not fl[j] & ENC:
            continue
        c = C.rx[int(slot_of[j])]
        if c.ekey is None:
            res[j] = NOCONN
            continue
        a = c.alt
        alt = P.ref_rx_key(int(seq[j]), int(fl[j]), a is not None,
                           bool(a and a.no_cutoff), a.cutoff if a else 0, c.rx_start)
        po = 8 + (hl if fl[j] & SIGNED else 0)
        at = int(R.offs[i])
        got = aes_ref.decrypt(a.ekey if alt else c.ekey, iv[j].tobytes(),
                              R.data[at + po:at + int(R.lens[i])].tobytes())
        if got is None:
            res[j] = BAD
        else:
            plain[j] = got
    return ns(hres=hres, res=res, seq=seq, fl=fl, iv=iv, plain=plain)


def check_rx_ref(R, ref, idx, oracle_mod):
    w = indep_rx(R, idx, oracle_mod)
    bad = np.nonzero(ref.hres[idx] != w.hres)[0]
    assert len(bad) == 0, [(int(idx[j]), R.kind[idx[j]], int(ref.hres[idx[j]]),
                            int(w.hres[j])) for j in bad[:8]]
    bad = np.nonzero(ref.res[idx] != w.res)[0]
    assert len(bad) == 0, [(int(idx[j]), R.kind[idx[j]], int(ref.res[idx[j]]),
                            int(w.res[j])) for j in bad[:8]]
    assert np.array_equal(ref.seq[idx], w.seq) and np.array_equal(ref.fl[idx], w.fl)
    due = ref.iv_due[idx]
    assert np.array_equal(ref.iv[idx][due], w.iv[due])
    for j, i in enumerate(idx):
        if w.plain[j] is None:
            assert ref.plen[i] == 0
            continue
        a = int(R.offs[i]) + 8 + (R.C.hl if w.fl[j] & SIGNED else 0)
        assert ref.plen[i] == len(w.plain[j])
        assert ref.out[a:a + len(w.plain[j])].tobytes() == w.plain[j], int(i)


def gives_back_plaintext(R, ref):
    """What TX sealed and nothing damaged afterwards decrypts to what was in
    the slot."""
    T = R.T
    whole = np.nonzero((R.kind == "") & (ref.res == OK) & ((T.flags & ENC) != 0))[0]
    assert len(whole) > R.n // 2
    for i in whole:
        a = int(T.offs[i]) + int(T.po[i])
        assert ref.plen[i] == T.plen[i]
        assert np.array_equal(ref.out[a:a + int(T.plen[i])], T.data[a:a + int(T.plen[i])])


_CASES = {}


def case(dev, oracle_mod, name, K, hash_alg, n, roll=(), nblk=NBLK, faults=True,
         check=None):
    """A burst with its tables and its device-resident references, TX with
    and without the cipher and RX of what TX sealed, built and checked against
    the independent reference once (`check`: the datagrams to check; default
    all)."""
    key = (name, K, hash_alg, n)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng([7000, K, hash_alg, n])
    C = connections(K, hash_alg, rng, roll)
    tabs = Tables(C)
    T = tx_burst(C, n, 1000 * hash_alg + K, nblk, faults)
    tx = dev_tx(dev, T, tabs, True)
    idx = np.arange(n) if check is None else check(T)
    check_tx_ref(T, tx, idx, oracle_mod)
    assert (tx.res == OK).sum() > n // 2
    R = rx_burst(T, tx, 1000 * hash_alg + K, oracle_mod, faults)
    rx = dev_rx(dev, R, tabs, True)
    check_rx_ref(R, rx, idx, oracle_mod)
    assert (rx.res == OK).sum() > n // 2
    gives_back_plaintext(R, rx)
    c = ns(C=C, tabs=tabs, T=T, tx=tx, R=R, rx=rx)
    _CASES[key] = c
    return c


def hash_only(dev, c):
    """The same bursts for the calls without a cipher table: TX seals the
    slots the cipher step left (lengths: the wire lengths), RX is the hash step
    alone."""
    if not hasattr(c, "tx0"):
        from ilias_net2_amd import _lib
        L = _lib.lib()
        T, n = c.T, c.T.n
        d = _dev(T.data, dev)
        cn, fl = _dev(_i32(T.conn), dev), _dev(_i32(T.flags), dev)
        sq, pl = _dev(_i32(T.seq), dev), _dev(_i32(T.plen), dev)
        o, ln = _dev(_i64(T.offs), dev), _dev(_i32(T.lens), dev)
        iv = torch.zeros((n, 16), dtype=torch.uint8, device=dev)
        er = torch.zeros(n, dtype=torch.uint8, device=dev)
        wire = torch.zeros(n, dtype=torch.int32, device=dev)
        s = torch.cuda.current_stream().cuda_stream
        _lib.check(L.net2_ph_to_iv_dev(sq.data_ptr(), fl.data_ptr(), n, 16, iv.data_ptr(), s))
        _lib.check(L.net2_packet_encrypt_burst_mc(
            c.tabs.ct.ptr, cn.data_ptr(), c.C.hl, fl.data_ptr(), iv.data_ptr(),
            d.data_ptr(), o.data_ptr(), ln.data_ptr(), pl.data_ptr(), n, er.data_ptr(),
            wire.data_ptr(), s))
        torch.cuda.synchronize()
        c.enc_data = d.cpu().numpy()
        assert np.array_equal(wire.cpu().numpy().view(np.uint32), c.tx.wire)
        c.tx0 = dev_tx(dev, T, c.tabs, False, lens=c.tx.wire, data=c.enc_data)
        # the hash step's codes of the cipher's OK slots are the sequence's,
        # and it leaves the same bytes
        ok = er.cpu().numpy() == OK
        assert np.array_equal(c.tx0.res[ok], c.tx.res[ok])
        assert np.array_equal(c.tx0.data, c.tx.data)
        c.rx0 = dev_rx(dev, c.R, c.tabs, False)
        assert np.array_equal(c.rx0.hres, c.rx.hres)
    return c


# ---- the forms ---------------------------------------------------------------

def _pair(fn):
    a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
    assert fn(ctypes.byref(a), ctypes.byref(b)) == 0
    return a.value, b.value


def launches(L):
    """(hash lane, hash wave, decrypt lane, decrypt wave, encrypt lane,
    encrypt quad) launches of library L so far."""
    return np.array(_pair(L.net2_sha2_burst_stats) + _pair(L.net2_aes_burst_stats) +
                    _pair(L.net2_aes_encrypt_stats), dtype=np.int64)


@pytest.fixture
def forms():
    """forms(small): the default forms, or every small-burst form switched
    off; the defaults again afterwards."""
    from ilias_net2_amd import _lib
    L = _lib.lib()

    def set_forms(small):
        v = -1 if small else 0
        assert L.net2_sha2_burst_limits(v, -1) == 0
        assert L.net2_aes_burst_limits(v) == 0
        assert L.net2_aes_encrypt_limits(v) == 0
    yield set_forms
    set_forms(True)


# ---- the mix ------------------------------------------------------------------

def mix(dev, oracle_mod, hash_alg):
    c = case(dev, oracle_mod, "mix", 7, hash_alg, 3001, roll=(1, 4))
    T, R = c.T, c.R
    if not hasattr(c, "covered"):
        # what this case is about, on the references' own codes
        assert set(T.kind) == set(TX_FAULTS) | {""} and set(R.kind) == set(RX_FAULTS) | {""}
        assert {OK, RESOURCE, UNSAFE, NOCONN} <= set(c.tx.res)
        assert (c.tx.res[T.kind == "noroom"] == RESOURCE).all()
        for k in ("unset", "range", "nocipher"):
            assert (c.tx.res[T.kind == k] == NOCONN).all(), k
            assert (c.rx.res[T.kind == k] == NOCONN).all(), k
        # an HMAC key but no cipher key: OK after the hash step
        assert (c.rx.hres[T.kind == "nocipher"] == OK).all()
        assert (c.rx.hres[T.kind == "unset"] == NOCONN).all()
        assert {OK, BAD, UNSAFE, NOCONN} <= set(c.rx.res)
        for k in ("payload", "field", "runt", "ragged", "badpad"):
            assert (c.rx.res[R.kind == k] == BAD).all(), k
        # ragged and badly padded ciphertexts pass the hash step
        for k in ("ragged", "badpad"):
            assert (c.rx.hres[R.kind == k] == OK).all(), k
        for k in ("noenc", "nosigned"):
            assert (c.rx.res[R.kind == k] == UNSAFE).all(), k
        # both key sets of both rollovers decrypt
        for k in (1, 4):
            cn = c.C.conns[k]
            mine = (R.kind == "") & (c.rx.res == OK)
            assert (mine & (T.conn == cn.slot)).sum() > 20
            assert (mine & (T.conn == cn.alt.slot)).sum() > 20
        nb = (c.rx.plen[(R.kind == "") & (c.rx.res == OK)] // 16 + 1)
        assert set(nb) == set(NBLK)
        c.covered = True
    return c


@pytest.mark.parametrize("small", [True, False], ids=["default-forms", "lane-forms"])
@pytest.mark.parametrize("cipher", [True, False], ids=["cipher", "hash-only"])
@pytest.mark.parametrize("outpin", [True, False], ids=["out-pinned", "out-pageable"])
@pytest.mark.parametrize("pin", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("hash_alg", [4, 6])
def test_mix(dev, oracle_mod, forms, hash_alg, pin, outpin, cipher, small):
    """n = 3,001 over K = 7, two connections mid-rollover, every fault of
    TX_FAULTS and RX_FAULTS, ciphertexts of 1 to 93 blocks: TX, then RX of what
    TX sealed in place and into a separate `out`, from pageable or one dense
    page-locked buffer, into page-locked or pageable arrays, with and without
    the cipher table, in the default forms and with every small-burst form
    switched off -- the *_stats deltas say which ran."""
    from ilias_net2_amd import _lib
    L = _lib.lib()
    c = mix(dev, oracle_mod, hash_alg)
    if not cipher:
        hash_only(dev, c)
    T, R = c.T, c.R
    forms(small)
    lane = 0 if small else 1
    # TX
    before = launches(L)
    if cipher:
        g = host_tx(L, T, c.tabs, True, pin, outpin)
        want = c.tx
        assert np.array_equal(g.wire, want.wire)
    else:
        g = host_tx(L, T, c.tabs, False, pin, outpin, lens=c.tx.wire, data=c.enc_data)
        want = c.tx0
        assert (g.wire.view(np.uint8) == SENT).all()
    delta = launches(L) - before
    want_delta = np.zeros(6, dtype=np.int64)
    want_delta[1 - lane] = 1
    if cipher:
        want_delta[5 - lane] = 1
    assert np.array_equal(delta, want_delta), (delta, want_delta)
    bad = np.nonzero(g.res != want.res)[0]
    assert len(bad) == 0, [(int(i), T.kind[i], int(g.res[i]), int(want.res[i]))
                           for i in bad[:8]]
    assert np.array_equal(g.data, want.data)        # every byte, gaps included
    # RX
    for in_place in ((True, False) if cipher else (True,)):
        before = launches(L)
        g = host_rx(L, R, c.tabs, cipher, pin, outpin, in_place)
        delta = launches(L) - before
        want_delta = np.zeros(6, dtype=np.int64)
        want_delta[1 - lane] = 1
        if cipher:
            want_delta[3 - lane] = 1
        assert np.array_equal(delta, want_delta), (delta, want_delta)
        check_rx(R, g, c.rx if cipher else c.rx0, cipher, in_place)
        if not cipher:
            assert (g.plen.view(np.uint8) == SENT).all()


@pytest.mark.parametrize("pin", [False, True], ids=["pageable", "pinned"])
def test_mix_mapped_reads(dev, oracle_mod, monkeypatch, pin):
    """The variant of the cipher chunks that reads and writes the datagrams
    through their host mapping (NET2_BURST_MC_ZC_MAX, read per chunk): the
    same results, in place and into a separate `out`."""
    from ilias_net2_amd import _lib
    L = _lib.lib()
    c = mix(dev, oracle_mod, 6)
    monkeypatch.setenv("NET2_BURST_MC_ZC_MAX", str(1 << 20))
    g = host_tx(L, c.T, c.tabs, True, pin, not pin)
    assert np.array_equal(g.res, c.tx.res) and np.array_equal(g.wire, c.tx.wire)
    assert np.array_equal(g.data, c.tx.data)
    for in_place in (True, False):
        g = host_rx(L, c.R, c.tabs, True, pin, not pin, in_place)
        check_rx(c.R, g, c.rx, True, in_place)


def test_mix_optional_outputs(dev, oracle_mod):
    """No iv and no header arrays asked for: the cipher step still gets them."""
    from ilias_net2_amd import _lib
    L = _lib.lib()
    c = mix(dev, oracle_mod, 6)
    R, n = c.R, c.R.n
    buf = R.data.copy()
    res, plen = alloc(False, (n,)), alloc(True, (n,), np.uint32)
    assert L.net2_packet_decode_burst_mc_host(
        c.tabs.kt.ptr, c.tabs.ct.ptr, _p(R.conn), 16, _p(buf), _p(R.offs), _p(R.lens), n,
        _p(res), None, None, None, _p(buf), _p(plen), None) == 0
    assert np.array_equal(res, c.rx.res) and np.array_equal(plen, c.rx.plen)
    assert np.array_equal(buf[c.rx.plain], c.rx.out[c.rx.plain])


def test_hash_only_iv_lengths(dev, oracle_mod):
    """Without the cipher table the call is the host form of
    decode_burst_mc: any IV length up to 64."""
    from ilias_net2_amd import _lib
    L = _lib.lib()
    c = mix(dev, oracle_mod, 6)
    for ivlen in (0, 8, 64):
        ref = dev_rx(dev, c.R, c.tabs, False, ivlen)
        for pin in (False, True):
            g = host_rx(L, c.R, c.tabs, False, pin, pin, ivlen=ivlen)
            assert np.array_equal(g.res, ref.res)
            assert np.array_equal(g.seq, ref.seq) and np.array_equal(g.fl, ref.fl)
            if ivlen:
                assert np.array_equal(g.iv[ref.iv_due], ref.iv[ref.iv_due])


# ---- sizes: the wave, workgroup and grid edges of the forms ---------------------

@pytest.mark.parametrize("mapped", [True, False], ids=["default", "copies"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1024, 1025])
def test_sizes(dev, oracle_mod, monkeypatch, n, mapped):
    """K = 3 with the cipher, RX and TX, at the wave, workgroup and grid edges
    of the forms and on either side of 1,024 datagrams, up to which an RX
    chunk is read through the host mapping by default; `copies` switches that
    off, so both paths run at every size."""
    from ilias_net2_amd import _lib
    L = _lib.lib()
    if not mapped:
        monkeypatch.setenv("NET2_BURST_MC_ZC_MAX", "0")
    c = case(dev, oracle_mod, "sizes", 3, 6, n, roll=(1,), nblk=(1, 2, 5, 93))
    for pin in (False, True):
        g = host_tx(L, c.T, c.tabs, True, pin, not pin)
        assert np.array_equal(g.res, c.tx.res) and np.array_equal(g.wire, c.tx.wire)
        assert np.array_equal(g.data, c.tx.data)
        g = host_rx(L, c.R, c.tabs, True, pin, not pin, in_place=pin)
        check_rx(c.R, g, c.rx, True, pin)


# ---- two chunks -----------------------------------------------------------------

def _two_chunk_lens():
    return np.concatenate([np.full(30000, 136), np.full(60000, 1560)]).astype(np.uint32)


def chunk_cut(lens):
    """Where the 64 MiB chunking cuts: 64 MiB over the mean padded length."""
    padded = int(((lens.astype(np.uint64) + 15) & ~np.uint64(15)).sum())
    return (64 << 20) // max(padded // len(lens), 16)


def two_chunks(dev, oracle_mod):
    """30,000 datagrams of 136 B, then 60,000 of 1,560 B (HMAC-SHA512, 4 and
    93 cipher blocks), back to back: ~98 MB, cut once, all the short ones in
    the first chunk.  Every 97th datagram gets a flipped bit on the way.  The
    independent reference checks 2,000 datagrams, the 64 on either side of the
    cut among them."""
    key = ("two", 5, 6, 90000)
    if key in _CASES:
        return _CASES[key]
    n = 90000
    rng = np.random.default_rng(7400)
    C = connections(5, 6, rng, roll=(2,))
    tabs = Tables(C)
    lens = _two_chunk_lens()
    cut = chunk_cut(lens)
    assert 30000 < cut < n < 2 * cut
    c_of = np.arange(n) % 5
    conn = np.array([C.conns[k].slot for k in c_of], dtype=np.uint32)
    seq = np.array([C.conns[k].rx_start for k in c_of], dtype=np.uint32) + \
        rng.integers(0, 900, n).astype(np.uint32)
    flags = np.full(n, ENC | SIGNED, dtype=np.uint32)
    plen = (lens - 72 - 16 + np.arange(n) % 16).astype(np.uint32)
    offs = np.zeros(n, dtype=np.uint64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    data = rng.integers(0, 256, int(lens.sum()), dtype=np.uint8)
    T = ns(C=C, n=n, kind=np.full(n, ""), conn=conn, rx_conn=conn, seq=seq, flags=flags,
           plen=plen, lens=lens, offs=offs, data=data, po=np.full(n, 72))
    tx = dev_tx(dev, T, tabs, True)
    idx = np.unique(np.concatenate([np.arange(cut - 64, cut + 64),
                                    rng.choice(n, 1872, replace=False)]))
    check_tx_ref(T, tx, idx, oracle_mod)
    assert (tx.res == OK).all() and np.array_equal(tx.wire, lens)
    rdata = tx.data.copy()
    hit = np.arange(n) % 97 == 5
    rdata[(offs[hit] + 8 + (lens[hit] - 9) // 2).astype(np.int64)] ^= 0x10
    R = ns(C=C, n=n, T=T, kind=np.where(hit, "payload", ""), conn=conn, offs=offs,
           lens=lens, data=rdata)
    rx = dev_rx(dev, R, tabs, True)
    check_rx_ref(R, rx, idx, oracle_mod)
    assert np.array_equal(rx.res, np.where(hit, BAD, OK))
    assert np.array_equal(rx.plen, np.where(hit, 0, plen))
    ok = ~hit
    a = (offs[ok] + 72).astype(np.int64)
    assert np.array_equal(rx.out[a], data[a])       # (first plaintext bytes)
    c = ns(C=C, tabs=tabs, T=T, tx=tx, R=R, rx=rx, cut=cut)
    _CASES[key] = c
    return c


@pytest.mark.parametrize("pin", [False, True], ids=["pageable", "pinned"])
def test_two_chunks(dev, oracle_mod, pin):
    from ilias_net2_amd import _lib
    L = _lib.lib()
    c = two_chunks(dev, oracle_mod)
    g = host_tx(L, c.T, c.tabs, True, pin, pin)
    assert np.array_equal(g.res, c.tx.res) and np.array_equal(g.wire, c.tx.wire)
    assert np.array_equal(g.data, c.tx.data)
    for in_place in (True, False):
        g = host_rx(L, c.R, c.tabs, True, pin, pin, in_place)
        check_rx(c.R, g, c.rx, True, in_place)


# ---- table updates ordered in table_stream ---------------------------------------

def test_table_stream_orders_updates(dev, oracle_mod):
    """set_rx / ciphertab_set_rx of a new key on stream X with no
    synchronisation, then the host call with table_stream = X: datagrams under
    the new key are OK, those under the old one BAD; after clear on X they are
    NOCONN."""
    from ilias_net2_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(7500)
    n, hl = 512, 64
    old = ns(hkey=_bytes(rng, hl), ekey=_bytes(rng, 32))
    new = ns(hkey=_bytes(rng, hl), ekey=_bytes(rng, 32))
    # slot 1 seals under the old keys, slot 2 under the new; slot 0 receives
    C = ns(K=1, hash_alg=6, hl=hl, slots=3, tx={1: old, 2: new})
    under_new = np.arange(n) % 3 == 0
    conn = np.where(under_new, 2, 1).astype(np.uint32)
    seq = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    flags = np.full(n, ENC | SIGNED, dtype=np.uint32)
    plen = (np.arange(n) % 50).astype(np.uint32)
    lens = (72 + 16 * (plen // 16 + 1)).astype(np.uint32)
    data, offs = synth.packed(7501, lens, align=1, gap=3)
    T = ns(C=C, n=n, kind=np.full(n, ""), conn=conn, seq=seq, flags=flags, plen=plen,
           lens=lens, offs=offs.astype(np.uint64), data=data)
    codes, wires, slots = indep_tx(T, np.arange(n), oracle_mod)
    assert (codes == OK).all()
    sealed = data.copy()
    for i, b in enumerate(slots):
        sealed[int(offs[i]):int(offs[i]) + len(b)] = np.frombuffer(b, dtype=np.uint8)
    from ilias_net2_amd import cipher_burst, conn_burst
    X = torch.cuda.Stream(device=dev)
    rx_conn = np.zeros(n, dtype=np.uint32)
    R = ns(C=C, n=n, kind=np.full(n, ""), conn=rx_conn, offs=T.offs, lens=lens, data=sealed)
    tabs = ns(kt=conn_burst.KeyTable(6, 3), ct=cipher_burst.CipherTable(3))
    try:
        tabs.kt.set_rx(0, old.hkey, enc_set=True)
        tabs.ct.set_rx(0, old.ekey, hash_alg=6)
        torch.cuda.synchronize()
        g = host_rx(L, R, tabs, True, False, False)
        assert np.array_equal(g.res, np.where(under_new, BAD, OK))
        # the new keys, queued behind work that keeps X busy for a while
        busy = torch.empty(1 << 26, dtype=torch.uint8, device=dev)
        with torch.cuda.stream(X):
            for _ in range(8):
                busy.add_(1)
        tabs.kt.set_rx(0, new.hkey, enc_set=True, stream=X)
        tabs.ct.set_rx(0, new.ekey, hash_alg=6, stream=X)
        g = host_rx(L, R, tabs, True, False, False, stream=X.cuda_stream)
        assert np.array_equal(g.res, np.where(under_new, OK, BAD))
        assert np.array_equal(g.plen, np.where(under_new, plen, 0))
        for i in np.nonzero(under_new)[0]:
            a = int(offs[i]) + 72
            assert np.array_equal(g.out[a:a + int(plen[i])], data[a:a + int(plen[i])])
        with torch.cuda.stream(X):
            for _ in range(8):
                busy.add_(1)
        tabs.kt.clear(0, stream=X)
        tabs.ct.clear(0, stream=X)
        g = host_rx(L, R, tabs, True, True, True, stream=X.cuda_stream)
        assert (g.res == NOCONN).all() and (g.plen == 0).all()
        assert np.array_equal(g.data, sealed)
        X.synchronize()
    finally:
        tabs.kt.close()
        tabs.ct.close()


# ---- with the single-connection host burst on the same device -------------------

def test_concurrent_with_the_single_connection_host_burst(dev, oracle_mod):
    """One thread runs the new RX call, another net2_packet_decode_burst_host
    on the same device (they share the device's two burst slots under one
    lock), eight times each: all results exact."""
    from ilias_net2_amd import _lib
    import test_gpu_burst_host as H
    L = _lib.lib()
    c = mix(dev, oracle_mod, 6)
    m, key = 20000, bytes(range(64))
    data, offs, lens, seq, flags = H._mtu_burst(m, 7600)
    _, sealed = oracle_mod.packet_encode_batch(6, key, True, seq, flags, data, offs, lens,
                                               nthreads=CPU_THREADS)
    want = oracle_mod.packet_decode_batch(6, key, True, 16, sealed, offs, lens,
                                          nthreads=CPU_THREADS)
    assert (want[0] == OK).all()
    keys = H.rx_keys(6, key, True)
    errs = []

    def new_call():
        torch.cuda.set_device(dev)
        for r in range(8):
            try:
                g = host_rx(L, c.R, c.tabs, True, bool(r % 2), bool(r % 2), bool(r % 4 < 2))
                check_rx(c.R, g, c.rx, True, bool(r % 4 < 2))
            except AssertionError as e:
                errs.append(("mc", r, str(e)[:300]))

    def old_call():
        torch.cuda.set_device(dev)
        for r in range(8):
            try:
                H.check_decode(H.decode_host(L, keys, 16, sealed, offs, lens), want, 16)
            except AssertionError as e:
                errs.append(("host", r, str(e)[:300]))
    th = [threading.Thread(target=new_call), threading.Thread(target=old_call)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs


# ---- injected host failures ----------------------------------------------------------

@pytest.fixture(scope="module")
def fi(dev):
    """The fault-injection build, bound like the shipped library
    (tests/test_gpu_failures.py)."""
    from ilias_net2_amd import _lib
    _lib.lib()          # torch's HIP runtime first, as _lib does
    lib = _lib.bind(ctypes.CDLL(FI_LIB))
    lib.net2_fault_inject.argtypes = [ctypes.c_int, ctypes.c_int]
    lib.net2_fault_inject.restype = ctypes.c_int
    yield lib
    lib.net2_fault_inject(0, 0)


def _settled(*arrays):
    """The arrays as they are at the call's return; after the device went idle
    they must still be that."""
    at_return = [a.copy() for a in arrays]
    torch.cuda.synchronize()
    for a, b in zip(at_return, arrays):
        assert np.array_equal(a, b), "output changed after the call returned"


@pytest.mark.parametrize("site", [FI_H2D, FI_KERNEL, FI_RECORD])
@pytest.mark.parametrize("pin", [False, True], ids=["pageable", "pinned"])
def test_failure_in_the_second_chunk(dev, oracle_mod, fi, pin, site):
    """An error return injected into the host code of the second chunk (after
    its input copy is queued, after its hash kernel is launched, at its event
    record): EIO, the first chunk's outputs delivered and exact, nothing
    changing after the return, and the next call exact."""
    c = two_chunks(dev, oracle_mod)
    T, R, cut = c.T, c.R, c.cut
    end = int(T.offs[cut])
    # RX
    assert fi.net2_fault_inject(site, 2) == 0
    g = host_rx(fi, R, c.tabs, True, pin, pin, in_place=False, rc=errno.EIO)
    assert fi.net2_sha2_last_hip_error() != 0
    _settled(g.res, g.iv, g.seq, g.fl, g.plen, g.out, g.data)
    check_rx(R, g, c.rx, True, False, upto=cut)
    assert fi.net2_fault_inject(0, 0) == 0
    g = host_rx(fi, R, c.tabs, True, pin, pin, in_place=False)
    check_rx(R, g, c.rx, True, False)
    # TX
    assert fi.net2_fault_inject(site, 2) == 0
    g = host_tx(fi, T, c.tabs, True, pin, pin, rc=errno.EIO)
    _settled(g.res, g.wire, g.data)
    assert np.array_equal(g.res[:cut], c.tx.res[:cut])
    assert np.array_equal(g.wire[:cut], c.tx.wire[:cut])
    assert np.array_equal(g.data[:end], c.tx.data[:end])
    assert fi.net2_fault_inject(0, 0) == 0
    g = host_tx(fi, T, c.tabs, True, pin, pin)
    assert np.array_equal(g.res, c.tx.res) and np.array_equal(g.wire, c.tx.wire)
    assert np.array_equal(g.data, c.tx.data)
