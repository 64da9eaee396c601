"""The directed bursts of tests/burst_cases.py on the CPU: every case has the
geometry it claims (residues, one datagram per length, no overlaps, the
address mode of every wave), and the oracle alone -- encode, the case's
edits, decode -- produces exactly the codes the case states, so what
tests/test_gpu_burst_lattice.py demands of the kernels is what the reference
does with these inputs.  The oracle's HMAC at every lattice length is held
against Python's hmac / hashlib, and so are its IV rows at every IV length
the GPU tests use.
"""
import hashlib
import hmac as pyhmac

import numpy as np
import pytest

import burst_cases as B

ALGS = B.ALGS
PYHASH = {4: hashlib.sha256, 5: hashlib.sha384, 6: hashlib.sha512}


def geometry(c, rx_flags=None):
    """What every case claims: a 16-byte header/field/payload layout at the
    stated residues, ascending without overlaps inside the buffer, and the
    stated address mode in every wave, RX and TX."""
    e = c.expect
    offs, lens = c.offs.astype(np.int64), c.lens.astype(np.int64)
    assert len(offs) == len(lens) == len(c.seq) == len(c.flags) == e.n > 0
    assert np.array_equal(offs % 16, e.residue)
    assert (offs[1:] >= offs[:-1] + lens[:-1]).all()          # no overlaps
    assert offs[-1] + lens[-1] <= len(c.data)
    assert (offs[1:] - (offs[:-1] + lens[:-1]) < 16).all()    # and dense
    assert (e.rx_lens <= c.lens).all()
    got_rx = B.wave_modes(B.lane_p(c, "rx", rx_flags))
    got_tx = B.wave_modes(B.lane_p(c, "tx"))
    assert len(got_rx) == len(e.modes_rx) == len(got_tx) == len(e.modes_tx)
    assert [g for g, m in zip(got_rx, e.modes_rx) if m is not None] == \
        [m for m in e.modes_rx if m is not None], e.name
    assert got_tx == e.modes_tx, e.name


def oracle_codes(oracle_mod, c):
    """Encode -> the case's edits -> decode on the oracle alone: the codes
    the case states by construction, headers and IVs of the OK datagrams."""
    e = c.expect
    a = B.answers(oracle_mod, c)
    assert np.array_equal(a.tx_res, e.tx_codes), e.name
    known = e.rx_codes >= 0
    assert np.array_equal(a.rx_res[known], e.rx_codes[known]), e.name
    ok = a.rx_res == B.OK
    assert a.rx_iv[ok].any(axis=1).all() and not a.rx_iv[~ok].any()
    # bytes outside the header and field of the OK slots are untouched
    same = np.ones(len(c.data), dtype=bool)
    for i in np.nonzero(e.tx_codes == B.OK)[0]:
        same[int(c.offs[i]):int(c.offs[i]) + 8 + B.HL[e.alg]] = False
    assert np.array_equal(a.sealed[same], c.data[same])
    return a


@pytest.mark.parametrize("order", ["asc", "perm"])
@pytest.mark.parametrize("alg", ALGS)
def test_L1_lattice(oracle_mod, alg, order):
    """16 residues x payload lengths 0 .. 4 * BLOCK + 1, each length once;
    residue 8 is A16, 0 / 4 / 12 are A4, the rest A1; all accepted."""
    for r in range(16):
        c = B.L1(alg, r, order)
        geometry(c)
        assert sorted(c.expect.plen) == list(range(4 * B.BLOCK[alg] + 2))
        assert (c.expect.plen[1:] > c.expect.plen[:-1]).all() == (order == "asc")
        want = B.A16 if r == 8 else B.A4 if r % 4 == 0 else B.A1
        assert set(c.expect.modes_rx) == {want}
        a = oracle_codes(oracle_mod, c)
        assert (a.tx_res == B.OK).all() and (a.rx_res == B.OK).all()
        assert np.array_equal(a.rx_seq, c.seq) and np.array_equal(a.rx_fl, c.flags)


@pytest.mark.parametrize("alg", ALGS)
def test_oracle_hmac_at_every_lattice_length(oracle_mod, alg):
    """The fields the oracle seals over the lattice, and oracle.hmac itself,
    against hmac / hashlib."""
    c = B.L1(alg, 3)
    a = B.answers(oracle_mod, c)
    hl, key = B.HL[alg], B.keys_for(alg, 0)
    for i in range(c.expect.n):
        o, ln = int(c.offs[i]), int(c.lens[i])
        msg = c.data[o + 8 + hl:o + ln].tobytes()
        assert len(msg) == c.expect.plen[i]
        want = pyhmac.new(key, msg, PYHASH[alg]).digest()
        assert a.sealed[o + 8:o + 8 + hl].tobytes() == want, i
        assert oracle_mod.hmac(alg, key, msg) == want, i
        assert a.sealed[o:o + 8].tobytes() == (int(c.seq[i]).to_bytes(4, "big") +
                                               int(c.flags[i]).to_bytes(4, "big"))


@pytest.mark.parametrize("hdr", [True, False])
@pytest.mark.parametrize("alg", ALGS)
def test_L2_pad_table_waves(oracle_mod, alg, hdr):
    """Every wave of one whole-block inner length is marked uniform, the
    wave holding the longer datagram is not; n = 64 has no tail variant."""
    residues = (8, 4, 1) if hdr else (0, 4, 1)
    cases = B.L2_all(alg, residues, hdr)
    assert len(cases) == 3 * 5 * (3 + 4 + 4)
    want = [B.A16, B.A4, B.A1]
    for c in cases:
        e = c.expect
        geometry(c)
        assert set(e.modes_rx) == {want[residues.index(int(e.residue[0]))]}
        inner = e.plen + B.BLOCK[4]          # SHA-256: key block + payload
        for w, u in enumerate(e.uniform):
            pl = inner[w * B.WAVE:(w + 1) * B.WAVE]
            assert u == (len(set(pl)) == 1 and pl[0] % 64 == 0), e.name
        assert sum(not u for u in e.uniform) == (0 if "same" in e.name else 1)
        if e.name.endswith("tail") or "-tail-" in e.name:
            assert e.n % B.WAVE == 1 and not e.uniform[-1]
        if hdr:
            a = oracle_codes(oracle_mod, c)
            assert (a.rx_res == B.OK).all()
        else:
            assert not B.dgram_answers(oracle_mod, c).verdict.any()


@pytest.mark.parametrize("alg", ALGS)
def test_L3_vote(oracle_mod, alg):
    """One odd datagram among A16 lanes: its wave takes the stated mode on
    each side, the others stay A16; it alone is refused."""
    cases = B.L3_all(alg)
    assert len(cases) == len(B.L3_KINDS) * (1 + 1 + 2 + 3 + 3)
    for c in cases:
        e = c.expect
        geometry(c)
        odd = np.nonzero(e.residue != 8)[0] if "@8" not in e.name else \
            np.nonzero(c.lens != 8 + B.HL[alg] + e.plen)[0] if "unsigned" not in e.name \
            else np.nonzero(c.flags != B.WANT)[0]
        assert len(odd) == 1
        at = int(odd[0])
        assert at % B.WAVE in (0, 63) or at == e.n - 1
        assert [m for k, m in enumerate(e.modes_rx) if k != at // B.WAVE] == \
            [B.A16] * (len(e.modes_rx) - 1)
        a = oracle_codes(oracle_mod, c)
        refused = "-r12-" not in e.name and "-r9-" not in e.name
        want_rx = np.zeros(e.n, dtype=np.uint8)
        want_tx = np.zeros(e.n, dtype=np.uint8)
        if refused:
            want_rx[at] = B.UNSAFE if "unsigned" in e.name else B.BAD
            want_tx[at] = B.UNSAFE if "unsigned" in e.name else B.RESOURCE
        assert np.array_equal(a.rx_res, want_rx) and np.array_equal(a.tx_res, want_tx)
    # every mode is reached on both sides by some odd lane
    for side in ("modes_rx", "modes_tx"):
        assert {m for c in cases for m in getattr(c.expect, side)} == {B.A16, B.A4, B.A1}


@pytest.mark.parametrize("alg", ALGS)
def test_L4_uniform_only_after_binning(oracle_mod, alg):
    """Submission-order waves mix the three residues; in the binned order
    (longest bin first, any order inside a bin) every wave is one class."""
    c = B.L4(alg)
    e = c.expect
    geometry(c)
    assert e.modes_rx == [B.A1] * 3
    for w in range(3):
        assert set(e.residue[w * B.WAVE:(w + 1) * B.WAVE]) == {8, 4, 1}
    key = B.bin_key(alg, c.lens)
    assert [set(key[e.cls == k]) for k in range(3)] == [{1}, {2}, {3}]
    rng = np.random.default_rng(5)
    order = np.concatenate([rng.permutation(np.nonzero(e.cls == k)[0]) for k in (2, 1, 0)])
    assert (np.diff(key[order]) <= 0).all()
    assert B.wave_modes(B.lane_p(c, "rx"), order) == e.binned_modes == \
        B.wave_modes(B.lane_p(c, "tx"), order)
    # the two longer classes are pad-table waves once binned
    assert set(e.plen[e.cls == 1]) == {B.BLOCK[alg]}
    assert set(e.plen[e.cls == 2]) == {2 * B.BLOCK[alg]}
    a = oracle_codes(oracle_mod, c)
    assert (a.rx_res == B.OK).all()


def hashlib_iv(seq, flags, ivlen):
    """net2_ph_to_iv restated: the first ivlen bytes of D0 || D1, D0 =
    SHA-256(ph), D1 = SHA-256(ph || D0), ph = be32(seq) || be32(flags)."""
    out = np.zeros((len(seq), ivlen), dtype=np.uint8)
    for i, (s, f) in enumerate(zip(seq, flags)):
        ph = int(s).to_bytes(4, "big") + int(f).to_bytes(4, "big")
        d0 = hashlib.sha256(ph).digest()
        iv = (d0 + hashlib.sha256(ph + d0).digest())[:ivlen]
        out[i] = np.frombuffer(iv, dtype=np.uint8)
    return out


@pytest.mark.parametrize("ivlen", B.IVLENS)
def test_iv_reference_at_every_length(oracle_mod, ivlen):
    """The IV rows that the GPU tests expect at every length of B.IVLENS:
    packet_decode_batch's rows of the OK datagrams are ph_to_iv_batch's, on
    the every-bit case and on 500 random headers, and both are the first
    ivlen bytes of the two SHA-256 rounds as hashlib computes them -- so no
    length rests on the oracle's own loop alone."""
    c = B.B1(6, 8, 100)
    a = B.answers(oracle_mod, c)
    res, iv, seq, fl = oracle_mod.packet_decode_batch(
        6, a.keys[0], True, ivlen, a.rx, c.offs, c.expect.rx_lens, nthreads=1)
    assert np.array_equal(res, a.rx_res) and iv.shape == (c.expect.n, ivlen)
    assert np.array_equal(seq, a.rx_seq) and np.array_equal(fl, a.rx_fl)
    ok = res == B.OK
    assert 64 <= ok.sum() < c.expect.n
    rows = oracle_mod.ph_to_iv_batch(seq, fl, ivlen, nthreads=1)
    assert np.array_equal(iv[ok], rows[ok])
    assert not iv[~ok].any()
    assert np.array_equal(rows, hashlib_iv(seq, fl, ivlen))
    if ivlen == B.IVLEN:
        assert np.array_equal(iv, a.rx_iv)
    rng = np.random.default_rng(616)
    seq = rng.integers(0, 2**32, 500, dtype=np.uint64).astype(np.uint32)
    fl = rng.integers(0, 2**32, 500, dtype=np.uint64).astype(np.uint32)
    rows = oracle_mod.ph_to_iv_batch(seq, fl, ivlen, nthreads=1)
    assert rows.shape == (500, ivlen)
    assert np.array_equal(rows, hashlib_iv(seq, fl, ivlen))


@pytest.mark.parametrize("plen", [100, 0])
@pytest.mark.parametrize("alg", ALGS)
def test_B1_every_bit(oracle_mod, alg, plen):
    """Bit j of the field flipped in datagram j: every one of the 8 * hl
    bits once, the exact counts, and the oracle refusing each."""
    hl = B.HL[alg]
    for r in (8, 4, 1):
        for altkey, lead in ((False, False), (True, False), (False, True)):
            if lead and r != 8:
                continue
            c = B.B1(alg, r, plen, altkey=altkey, lead=lead)
            assert c.offs[0] == (0 if lead else r)
            e = c.expect
            a = oracle_codes(oracle_mod, c)
            geometry(c, a.rx_fl)
            assert e.counts == {B.FIELD: 8 * hl, B.PAY_FIRST: 8 if plen else 0,
                                B.PAY_LAST: 8 if plen else 0, B.HEADER: 32,
                                B.CONTROL: (e.kinds == B.CONTROL).sum()}
            assert e.counts[B.CONTROL] >= 64
            for w in range(0, e.n, B.WAVE):          # controls in every wave
                assert (e.kinds[w:w + B.WAVE] == B.CONTROL).any()
            # field flips: one per bit of the field, in order
            fi = np.nonzero(e.kinds == B.FIELD)[0]
            rel = e.flip_pos[:8 * hl] - c.offs[fi].astype(np.int64) - 8
            bit = rel * 8 + np.log2(e.flip_mask[:8 * hl]).astype(np.int64)
            assert np.array_equal(bit, np.arange(8 * hl))
            diff = a.rx != a.sealed
            assert diff.sum() == len(e.flip_pos)
            assert np.array_equal(np.nonzero(diff)[0], np.sort(e.flip_pos))
            for k in (B.FIELD, B.PAY_FIRST, B.PAY_LAST):
                assert (a.rx_res[e.kinds == k] == B.BAD).all()
            assert (a.rx_res[e.kinds == B.CONTROL] == B.OK).all()
            # header flips: SIGNED and ENCRYPTED refuse, PH_ALTKEY picks the
            # other key where there is one, the rest changes the header only
            hd = a.rx_res[e.kinds == B.HEADER]
            assert (hd == B.UNSAFE).sum() == 2
            assert (hd == B.BAD).sum() == (1 if altkey else 0)
            assert (hd == B.OK).sum() == 32 - 2 - (1 if altkey else 0)
            assert (a.rx_res == B.BAD).sum() == 8 * hl + (16 if plen else 0) + \
                (1 if altkey else 0)
            if altkey:
                assert ((c.flags & B.PH_ALTKEY) != 0).sum() == e.n // 2
    # the header-less shape: field and payload flips only
    for r in (0, 4, 1):
        c = B.B1(alg, r, plen, hdr=False)
        geometry(c)
        a = B.dgram_answers(oracle_mod, c)
        assert c.expect.counts[B.HEADER] == 0
        assert np.array_equal(a.verdict, (c.expect.kinds != B.CONTROL).astype(np.uint8))
        assert a.verdict.sum() == 8 * hl + (16 if plen else 0)
