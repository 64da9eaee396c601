"""Directed bursts for the keyed packet kernels: datagrams at chosen start
alignments, lengths and wave positions (plain numpy, no GPU).

hmac_kernel picks its load path per wave of 64 consecutive lanes from the
address p at which each lane's message starts (sha2_kernels.hip, hmac_item):
every p a multiple of 16 -> A16, else every p a multiple of 4 -> A4, else
A1 (HMAC-SHA256; SHA-384/512 have one path).  In the burst modes

    an OK lane (RX and TX)                      p = off + 8 + hl
    RX, header fine but no room for the field   p = off + 8
    any other refused lane (runt, UNSAFE, TX
    slot without room)                          p = off
    a dead lane of the tail wave                p = base

and 8 + hl is 8 (mod 16) for all three hashes, so datagrams at offsets of
residue 8 (mod 16) make A16 waves, the other multiples of 4 make A4 waves.
Offsets here are relative to a buffer whose base is 16-byte aligned.  In the
header-less datagram modes (HMAC_SIGN / VERIFY) p = off + hl: residue 0 is
A16.  lane_p() / wave_modes() restate that rule; tests/test_burst_cases.py
holds every case to the geometry it claims, on the CPU.

Every case is a Case(data, offs, lens, seq, flags, expect): the unsealed
slots (header || hash field || payload, random content), and in `expect`
what the test needs beyond the oracle's answers -- the RX edits made after
sealing (bit flips, headers of the slots TX refused, RX lengths), the codes
known by construction (-1: the oracle decides) and the claimed wave modes.
answers() runs the oracle (packet_encode_batch, the edits,
packet_decode_batch) once per case and caches the result; nothing returned
here may be modified.
"""
from __future__ import annotations

import functools
import types
from typing import NamedTuple

import numpy as np

import synth

PH_ENCRYPTED, PH_SIGNED, PH_ALTKEY = 0x1, 0x2, 0x80000000
OK, RESOURCE, BAD, UNSAFE = 0, 1, 2, 3
HL = {4: 32, 5: 48, 6: 64}
BLOCK = {4: 64, 5: 128, 6: 128}
WAVE = 64
WANT = PH_SIGNED | PH_ENCRYPTED     # the flags the keys call for (cipher set)
IVLEN = 16
# IV lengths on both sides of one hash round (<= 32) against two, whole
# 16-byte pieces against not, rows alternating between 0 and 8 (mod 16) in an
# aligned array (24), and both ends of the range the C ABI accepts
IVLENS = (0, 1, 8, 15, 16, 17, 24, 31, 32, 33, 47, 48, 63, 64)
A16, A4, A1 = "A16", "A4", "A1"
ALGS = (4, 5, 6)


class Case(NamedTuple):
    data: np.ndarray
    offs: np.ndarray
    lens: np.ndarray
    seq: np.ndarray
    flags: np.ndarray
    expect: types.SimpleNamespace


def mode_of(residue_p: int) -> str:
    return A16 if residue_p % 16 == 0 else A4 if residue_p % 4 == 0 else A1


def place(lens, residue):
    """Offsets, in order and without overlap, each the first one at or past
    the previous datagram's end with its residue (mod 16) -> (offs, total)."""
    offs = np.zeros(len(lens), dtype=np.uint64)
    at = 0
    for i, (ln, r) in enumerate(zip(lens, residue)):
        at += (int(r) - at) % 16
        offs[i] = at
        at += int(ln)
    return offs, at


def _freeze(c: Case) -> Case:
    for a in list(c[:5]) + [v for v in vars(c.expect).values()
                            if isinstance(v, np.ndarray)]:
        a.setflags(write=False)
    return c


def build(name, alg, plen, residue, seed, slot_len=None, flags=None, rx_lens=None,
          flips=(), kinds=None, hdr=True, **claims) -> Case:
    """One burst.  plen / residue: per datagram; slot_len: the slot's length
    where it is not header + field + payload (runts, slots without room);
    flips: (datagram, byte within it, mask) applied to the sealed bytes.
    hdr=False: the header-less datagram shape (field || payload)."""
    hl, h8 = HL[alg], 8 if hdr else 0
    plen = np.asarray(plen, dtype=np.int64)
    n = len(plen)
    residue = np.broadcast_to(np.asarray(residue, dtype=np.int64), (n,)).copy()
    lens = (h8 + hl + plen) if slot_len is None else np.asarray(slot_len, dtype=np.int64)
    offs, total = place(lens, residue)
    data = synth.random_bytes(seed, max(total, 1))
    seq = (synth.splitmix64(seed + 1, n) >> np.uint64(7)).astype(np.uint32)
    flags = (np.full(n, WANT, dtype=np.uint32) if flags is None
             else np.asarray(flags, dtype=np.uint32))
    rx_lens = lens.copy() if rx_lens is None else np.asarray(rx_lens, dtype=np.int64)
    # what the codes are by construction (packet.n2t:364-370, :196-258)
    unsafe = (flags & WANT) != WANT
    tx = np.where(unsafe, UNSAFE, np.where(lens < h8 + hl, RESOURCE, OK)).astype(np.int8)
    rx = np.where(rx_lens < 8, BAD, np.where(unsafe, UNSAFE,
                  np.where(rx_lens < 8 + hl, BAD, OK))).astype(np.int8)
    fpos = np.zeros(len(flips), dtype=np.int64)
    fmask = np.zeros(len(flips), dtype=np.uint8)
    for k, (i, b, m) in enumerate(flips):
        assert tx[i] == OK and 0 <= b < lens[i] and 0 < m < 256
        fpos[k], fmask[k] = int(offs[i]) + b, m
        rx[i] = -1 if b < h8 else BAD
    assert len(np.unique(fpos)) == len(fpos)
    e = types.SimpleNamespace(
        name=name, alg=alg, hdr=hdr, n=n, plen=plen, residue=residue,
        rx_lens=rx_lens.astype(np.uint32), flip_pos=fpos, flip_mask=fmask,
        tx_codes=tx, rx_codes=rx,
        kinds=np.zeros(n, dtype=np.int8) if kinds is None else np.asarray(kinds, np.int8),
        **claims)
    return _freeze(Case(data, offs, lens.astype(np.uint32), seq, flags, e))


def rx_buffer(c: Case, sealed: np.ndarray) -> np.ndarray:
    """The received bytes: what TX sealed, the slots TX refused given a
    header of their own (seq, flags -- as much of it as the slot holds), then
    the bit flips."""
    rx = np.array(sealed, copy=True)
    e = c.expect
    if e.hdr:
        for i in np.nonzero(e.tx_codes != OK)[0]:
            h = np.frombuffer(int(c.seq[i]).to_bytes(4, "big") +
                              int(c.flags[i]).to_bytes(4, "big"), dtype=np.uint8)
            k = min(8, int(c.lens[i]))
            rx[int(c.offs[i]):int(c.offs[i]) + k] = h[:k]
    rx[e.flip_pos] ^= e.flip_mask
    return rx


def lane_p(c: Case, side: str, rx_flags=None) -> np.ndarray:
    """The message start p (offset from the base) of every datagram's lane
    in hmac_kernel, side "rx" or "tx" (module docstring).  rx_flags: the
    flags of the received headers where bit flips changed them."""
    e = c.expect
    hl = HL[e.alg]
    off = c.offs.astype(np.int64)
    if not e.hdr:
        ln = c.lens.astype(np.int64)
        return np.where(ln < hl, off, off + hl)
    if side == "tx":
        return np.where(e.tx_codes == OK, off + 8 + hl, off)
    ln = e.rx_lens.astype(np.int64)
    fl = c.flags if rx_flags is None else np.asarray(rx_flags, dtype=np.uint32)
    hdr_ok = (ln >= 8) & ((fl & WANT) == WANT)
    return np.where(hdr_ok, np.where(ln >= 8 + hl, off + 8 + hl, off + 8), off)


def wave_modes(p: np.ndarray, order=None) -> list:
    """The address mode of every wave of 64 lanes visiting the datagrams in
    `order` (default: submission order); dead lanes of the tail wave have
    p = base, residue 0."""
    p = p if order is None else p[order]
    out = []
    for w in range(0, len(p), WAVE):
        r = p[w:w + WAVE] % 16
        out.append(A16 if (r == 0).all() else A4 if (r % 4 == 0).all() else A1)
    return out


def bin_key(alg: int, wire_len) -> np.ndarray:
    """The length-binning key (bin_of): compressions the datagram would take
    as a plain message, padding included; bins are visited longest first."""
    blk, lb = (64, 8) if alg == 4 else (128, 16)
    return (np.asarray(wire_len, dtype=np.int64) + lb + 1 + blk - 1) // blk


# ---- L1: residue x length lattice ------------------------------------------

@functools.lru_cache(maxsize=None)
def L1(alg: int, r: int, order: str = "asc", hdr: bool = True,
       altkey: bool = False) -> Case:
    """One datagram per payload length 0 .. 4 * BLOCK + 1, every offset of
    residue r; order "asc" or "perm" (one fixed seeded permutation).
    altkey: odd datagrams carry PH_ALTKEY."""
    plen = np.arange(4 * BLOCK[alg] + 2)
    if order == "perm":
        plen = plen[np.random.default_rng(1234).permutation(len(plen))]
    flags = np.full(len(plen), WANT, dtype=np.uint32)
    if altkey:
        flags[1::2] |= PH_ALTKEY
    m = mode_of(r + (8 if hdr else 0) + HL[alg])
    nw = -(-len(plen) // WAVE)
    return build(f"L1-{alg}-r{r}-{order}{'' if hdr else '-nohdr'}{'-alt' if altkey else ''}",
                 alg, plen, r, 11000 + 100 * alg + r, flags=flags, hdr=hdr,
                 modes_rx=[m] * nw, modes_tx=[m] * nw)


# ---- L2: pad-table waves ---------------------------------------------------

L2_N = (64, 65, 129)
L2_PLEN = (0, 64, 128, 192, 1408)
L2_VARIANTS = ("same", "lane0", "lane63", "tail")


@functools.lru_cache(maxsize=None)
def L2(alg: int, r: int, n: int, plen: int, variant: str, hdr: bool = True):
    """n datagrams of one payload length (inner length a whole number of
    SHA-256 blocks, so a wave of them reads its pad schedule from the pad
    table) at residue r; variant: one datagram one byte longer at lane 0 or
    63 of the first wave, or as the lone live lane of the tail wave ("tail";
    None for n = 64, which has no tail wave)."""
    at = {"same": None, "lane0": 0, "lane63": 63, "tail": n - 1}[variant]
    if variant == "tail" and n % WAVE != 1:
        return None
    pl = np.full(n, plen)
    if at is not None:
        pl[at] += 1
    nw = -(-n // WAVE)
    uniform = [at is None or not (w * WAVE <= at < (w + 1) * WAVE) for w in range(nw)]
    m = mode_of(r + (8 if hdr else 0) + HL[alg])
    return build(f"L2-{alg}-r{r}-n{n}-p{plen}-{variant}{'' if hdr else '-nohdr'}", alg,
                 pl, r, 12000 + 1000 * alg + 17 * r + n + plen, hdr=hdr,
                 modes_rx=[m] * nw, modes_tx=[m] * nw, uniform=uniform)


def L2_all(alg: int, residues=(8, 4, 1), hdr: bool = True) -> list:
    out = [L2(alg, r, n, p, v, hdr) for r in residues for n in L2_N for p in L2_PLEN
           for v in L2_VARIANTS]
    return [c for c in out if c is not None]


# ---- L3: the wave's vote ---------------------------------------------------

L3_N = (1, 63, 64, 65, 257)
# kind -> (the odd datagram's residue, RX mode of its wave, TX mode)
L3_KINDS = {
    "r12": (12, A4, A4), "r9": (9, A1, A1),
    # refused lanes keep p at the datagram start: residue 0 leaves the
    # wave A16, residue 8 drops it to A4
    "runt@0": (0, A16, A16), "runt@8": (8, A4, A4),
    "unsigned@0": (0, A16, A16), "unsigned@8": (8, A4, A4),
    # 8 + hl - 1 bytes: TX refuses the slot (p = off); RX decodes the header
    # and then finds no room for the field (p = off + 8), the other way round
    "noroom@0": (0, A4, A16), "noroom@8": (8, A16, A4),
}


def L3_places(n: int) -> list:
    """Lane 0, lane 63 of the first wave, and the last lane of a tail wave."""
    at = [0]
    if n > 63:
        at.append(63)
    if n > WAVE and n % WAVE:
        at.append(n - 1)
    return at


@functools.lru_cache(maxsize=None)
def L3(alg: int, n: int, kind: str, at: int) -> Case:
    """Every datagram at residue 8 and OK (A16 waves) but the one at `at`."""
    hl = HL[alg]
    odd_r, m_rx, m_tx = L3_KINDS[kind]
    plen = (np.arange(n) * 37) % 300
    res = np.full(n, 8)
    res[at] = odd_r
    slot = 8 + hl + plen
    rx_lens = slot.copy()
    flags = np.full(n, WANT, dtype=np.uint32)
    if kind.startswith("runt"):
        slot[at] = rx_lens[at] = 5
    elif kind.startswith("unsigned"):
        flags[at] = PH_ENCRYPTED
    elif kind.startswith("noroom"):
        slot[at] = rx_lens[at] = 8 + hl - 1
    nw = -(-n // WAVE)
    w = at // WAVE
    return build(f"L3-{alg}-n{n}-{kind}-at{at}", alg, plen, res,
                 13000 + 1000 * alg + n + 7 * at + len(kind), slot_len=slot, flags=flags,
                 rx_lens=rx_lens,
                 modes_rx=[m_rx if k == w else A16 for k in range(nw)],
                 modes_tx=[m_tx if k == w else A16 for k in range(nw)])


def L3_all(alg: int) -> list:
    return [L3(alg, n, kind, at) for n in L3_N for kind in L3_KINDS
            for at in L3_places(n)]


# ---- L4: uniform only after binning ----------------------------------------

@functools.lru_cache(maxsize=None)
def L4(alg: int) -> Case:
    """Three block-count classes of 64 datagrams each, one residue per class
    (8, 4, 1), submitted round-robin: every submission-order wave mixes the
    residues (A1), every length-binned wave is one class -- A16 with mixed
    lengths, A4 on the pad table (inner length two blocks), A1 on it."""
    blk = BLOCK[alg]
    k = np.arange(3 * WAVE)
    cls = k % 3
    plen = np.where(cls == 0, (k // 3) % 16, cls * blk)
    res = np.array([8, 4, 1])[cls]
    # binned: longest first; the order inside a bin is the kernel's own
    return build(f"L4-{alg}", alg, plen, res, 14000 + alg, modes_rx=[A1] * 3,
                 modes_tx=[A1] * 3, cls=cls, binned_modes=[A1, A4, A16])


# ---- B1: every bit of the hash field ---------------------------------------

FIELD, PAY_FIRST, PAY_LAST, HEADER, CONTROL = 1, 2, 3, 4, 5
# SIGNED, ENCRYPTED and ALTKEY among the header bits flipped (bit h: byte
# h // 8 of the header, bit h % 8 of it)
_HDR_MUST = (7 * 8 + 1, 7 * 8 + 0, 4 * 8 + 7)


def header_bits() -> list:
    rest = [h for h in np.random.default_rng(77).permutation(64) if h not in _HDR_MUST]
    return sorted(list(_HDR_MUST) + [int(h) for h in rest[:32 - len(_HDR_MUST)]])


@functools.lru_cache(maxsize=None)
def B1(alg: int, r: int, plen: int, hdr: bool = True, altkey: bool = False,
       lead: bool = False) -> Case:
    """Datagram j < 8 * hl has bit j of its hash field flipped after sealing;
    then 8 with bit k of the first payload byte and 8 with bit k of the last
    one flipped (payload length 0 has neither), then 32 with one header bit
    flipped (burst shape only).  An intact control follows every 7 of them
    and more close the burst: at least 64, some in every wave.  altkey: odd
    datagrams carry PH_ALTKEY (sealed under the alternate key).  lead (r = 8):
    the first datagram alone lies at residue 0, at the buffer's first byte,
    which takes its wave from A16 to A4 -- a burst that keeps its residues
    when a host path rebases the offsets to the first datagram."""
    hl, h8 = HL[alg], 8 if hdr else 0
    edits = [(FIELD, h8 + j // 8, 1 << (j % 8)) for j in range(8 * hl)]
    if plen:
        edits += [(PAY_FIRST, h8 + hl, 1 << k) for k in range(8)]
        edits += [(PAY_LAST, h8 + hl + plen - 1, 1 << k) for k in range(8)]
    if hdr:
        edits += [(HEADER, h // 8, 1 << (h % 8)) for h in header_bits()]
    kinds, flips = [], []
    for kind, byte, mask in edits:
        if kind == HEADER and HEADER not in kinds:
            # a flipped flag bit can refuse the datagram and move its lane's
            # p: the header flips start a wave of their own
            kinds += [CONTROL] * (-len(kinds) % WAVE)
        flips.append((len(kinds), byte, mask))
        kinds.append(kind)
        if len(kinds) % 8 == 7:
            kinds.append(CONTROL)
    kinds += [CONTROL] * max(1, 64 - kinds.count(CONTROL))
    n = len(kinds)
    flags = np.full(n, WANT, dtype=np.uint32)
    if altkey:
        flags[1::2] |= PH_ALTKEY
    m = mode_of(r + h8 + hl)
    nw = -(-n // WAVE)
    kinds = np.array(kinds, dtype=np.int8)
    # RX: claimed for the waves before the header flips (None: not claimed)
    clean = int(np.argmax(kinds == HEADER)) // WAVE if hdr else nw
    counts = {k: int((kinds == k).sum()) for k in (FIELD, PAY_FIRST, PAY_LAST, HEADER,
                                                   CONTROL)}
    res = np.full(n, r)
    modes_rx, modes_tx = [m] * clean + [None] * (nw - clean), [m] * nw
    if lead:
        assert r == 8 and hdr
        res[0], modes_rx[0], modes_tx[0] = 0, A4, A4
    return build(f"B1-{alg}-r{r}-p{plen}{'' if hdr else '-nohdr'}{'-alt' if altkey else ''}"
                 f"{'-lead' if lead else ''}",
                 alg, np.full(n, plen), res, 15000 + 100 * alg + r + plen, flags=flags,
                 flips=flips, kinds=kinds, hdr=hdr, modes_rx=modes_rx, modes_tx=modes_tx,
                 counts=counts)


# ---- the oracle's answers ---------------------------------------------------

def keys_for(alg: int, k: int = 0) -> bytes:
    """Key k of a hash row (0: the active key, 1: the alternate key, 2..:
    further connections)."""
    return bytes(synth.random_bytes(900 + 10 * alg + k, HL[alg]))


_answers = {}


def answers(oracle_mod, c: Case, nconn: int = 1):
    """What the oracle makes of the case, computed once: TX codes and sealed
    bytes, the received bytes (rx_buffer), RX codes / IVs / headers.  A case
    with PH_ALTKEY datagrams is sealed under the alternate key there and
    decoded with it (no cutoff).  nconn > 1: datagram i belongs to
    connection i % nconn, each with a key of its own (keys_for(alg, 2 + k))."""
    e = c.expect
    tag = (e.name, nconn)
    if tag in _answers:
        return _answers[tag]
    alg, n = e.alg, e.n
    alt = bool((c.flags & PH_ALTKEY).any())
    assert not (alt and nconn > 1)
    if nconn > 1:
        group = np.arange(n) % nconn
        gkeys = [keys_for(alg, 2 + k) for k in range(nconn)]
    else:
        group = ((c.flags & PH_ALTKEY) != 0).astype(np.int64)
        gkeys = [keys_for(alg, 0), keys_for(alg, 1)]
    tx_res = np.full(n, 9, dtype=np.uint8)
    sealed = np.array(c.data, copy=True)
    for g in np.unique(group):
        idx = np.nonzero(group == g)[0]
        r, out = oracle_mod.packet_encode_batch(alg, gkeys[g], True, c.seq[idx],
                                                c.flags[idx], sealed, c.offs[idx],
                                                c.lens[idx], nthreads=1)
        tx_res[idx] = r
        sealed = out        # the groups' slots are disjoint
    rx = rx_buffer(c, sealed)
    rx_res = np.full(n, 9, dtype=np.uint8)
    rx_iv = np.zeros((n, IVLEN), dtype=np.uint8)
    rx_seq, rx_fl = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    if nconn > 1:
        for g in range(nconn):
            idx = np.nonzero(group == g)[0]
            if len(idx) == 0:
                continue
            rx_res[idx], rx_iv[idx], rx_seq[idx], rx_fl[idx] = \
                oracle_mod.packet_decode_batch(alg, gkeys[g], True, IVLEN, rx,
                                               c.offs[idx], e.rx_lens[idx], nthreads=1)
    else:
        rx_res, rx_iv, rx_seq, rx_fl = oracle_mod.packet_decode_batch(
            alg, gkeys[0], True, IVLEN, rx, c.offs, e.rx_lens,
            alt_key=gkeys[1] if alt else None, alt_no_cutoff=True, nthreads=1)
        rx_iv = np.array(rx_iv)
    a = types.SimpleNamespace(tx_res=tx_res, sealed=sealed, rx=rx, rx_res=rx_res,
                              rx_iv=rx_iv, rx_seq=rx_seq, rx_fl=rx_fl, group=group,
                              keys=gkeys, alt=alt)
    for v in vars(a).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _answers[tag] = a
    return a


_dgram_answers = {}


def dgram_answers(oracle_mod, c: Case):
    """The header-less shape (field || message): the signed bytes, the
    received bytes and the verdicts (0 equal, 1 not, 2 shorter than the
    field), from the oracle's HMAC of every message."""
    e = c.expect
    if e.name in _dgram_answers:
        return _dgram_answers[e.name]
    assert not e.hdr
    hl, key = HL[e.alg], keys_for(e.alg, 0)
    assert (c.lens >= hl).all()
    moff, mlen = c.offs + np.uint64(hl), c.lens - np.uint32(hl)
    cols = c.offs.astype(np.int64)[:, None] + np.arange(hl)[None, :]
    signed = np.array(c.data, copy=True)
    signed[cols] = oracle_mod.hmac_batch(e.alg, key, c.data, offsets=moff, lens=mlen,
                                         nthreads=1)
    rx = rx_buffer(c, signed)
    calc = oracle_mod.hmac_batch(e.alg, key, rx, offsets=moff, lens=mlen, nthreads=1)
    verdict = (rx[cols] != calc).any(axis=1).astype(np.uint8)
    a = types.SimpleNamespace(signed=signed, rx=rx, verdict=verdict, key=key)
    for v in (signed, rx, verdict):
        v.setflags(write=False)
    _dgram_answers[e.name] = a
    return a
