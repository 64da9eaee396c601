"""The keyed packet bursts on the directed cases of tests/burst_cases.py:
wave-uniform start alignments (the A16 / A4 / A1 load and compare paths of
hmac_kernel's burst modes), every bit of the hash field, and payload lengths
0 .. 4 * BLOCK + 1 at all 16 start residues.

Every sealed byte, code, decoded header and IV is compared with the oracle
(packet_encode_batch / packet_decode_batch / hmac_batch), bit for bit.  The
cases and the oracle's answers are computed once (burst_cases.answers) and
shared; tests/test_burst_cases.py shows on the CPU that the cases have the
geometry they claim and that the oracle refuses every flipped bit.

The forms (net2_sha2_burst_limits): "lane" -- hmac_kernel, one lane per
datagram in submission order; "binned" -- the same, visited in the
length-binned order; "wave" -- burst_wave_kernel.

The second half is the IV output (ph_iv_one): every IV length of B.IVLENS
through the three RX entry points in every form, the IV array at unaligned
addresses with guard bytes around it, d_iv = NULL, and net2_ph_to_iv_dev row
by row.
"""
import ctypes
import types

import numpy as np
import pytest

import burst_cases as B
import test_gpu_burst_host as H

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FORMS = {"lane": (0, -1), "binned": (0, 1), "wave": (1 << 30, -1)}
SENTINEL = 0xA5
IVLEN = B.IVLEN


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a GPU (HIP device not visible)")
    from ilias_net2_amd import _lib
    assert _lib.device_count() >= 1
    return torch.device("cuda:0")


@pytest.fixture
def limits():
    """net2_sha2_burst_limits for one test, the defaults restored after."""
    from ilias_net2_amd import _lib
    L = _lib.lib()

    def set_form(form):
        assert L.net2_sha2_burst_limits(*FORMS[form]) == 0
    yield set_form
    L.net2_sha2_burst_limits(-1, -1)


def _dev(a, dev):
    """A device copy through a writable host copy (the shared cases are
    read-only); the kernels' address modes assume a 16-byte aligned base."""
    t = torch.from_numpy(np.array(a, order="C")).to(dev)
    assert t.data_ptr() % 16 == 0
    return t


def family(name, alg):
    """The cases of one family for one hash row."""
    if name == "L1":
        return [B.L1(alg, r, order) for r in range(16) for order in ("asc", "perm")]
    if name == "L2":
        return B.L2_all(alg)
    if name == "L3":
        return B.L3_all(alg)
    if name == "L4":
        return [B.L4(alg)]
    return [B.B1(alg, r, plen) for r in (8, 4, 1) for plen in (100, 0)]


def workspace(L, n, dev):
    """A burst workspace prepared so that its first binning bins."""
    ws = torch.empty(L.net2_packet_burst_workspace(n), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    assert L.net2_sha2_workspace_init(ws.data_ptr(), ws.numel(), st) == 0
    return ws


def check_rx(c, a, res, iv, seq, fl, sentinel, rows=None, due=None):
    """Codes, headers, the IVs of the OK rows, and every other IV row left
    as it was.  rows: the expected IV rows at an IV length other than IVLEN
    (default: the answers' own, a.rx_iv); due: the rows an IV is due to where
    that is not every OK row (a connection without a cipher key)."""
    e = c.expect
    assert np.array_equal(res, a.rx_res), (e.name, np.nonzero(res != a.rx_res)[0][:8])
    known = e.rx_codes >= 0
    assert np.array_equal(res[known], e.rx_codes[known]), e.name
    assert np.array_equal(seq, a.rx_seq) and np.array_equal(fl, a.rx_fl), e.name
    ok = a.rx_res == B.OK if due is None else due
    rows = a.rx_iv if rows is None else rows
    assert iv.shape == rows.shape, (e.name, iv.shape, rows.shape)
    assert np.array_equal(iv[ok], rows[ok]), e.name
    if sentinel is not None:
        assert (iv[~ok] == sentinel).all(), e.name


def device_tx_rx(dev, oracle_mod, c):
    """net2_packet_encode_burst of the case's slots, then
    net2_packet_decode_burst of the received bytes the oracle's TX leads to."""
    from ilias_net2_amd import _lib
    L = _lib.lib()
    e = c.expect
    a = B.answers(oracle_mod, c)
    n, alg, hl = e.n, e.alg, B.HL[e.alg]
    key = a.keys[0]
    st = torch.cuda.current_stream().cuda_stream
    ws = workspace(L, n, dev)
    d, o = _dev(c.data, dev), _dev(c.offs.view(np.int64), dev)
    ln = _dev(c.lens.view(np.int32), dev)
    ds, df = _dev(c.seq.view(np.int32), dev), _dev(c.flags.view(np.int32), dev)
    res = torch.full((n,), 9, dtype=torch.uint8, device=dev)
    assert L.net2_packet_encode_burst(alg, key, hl, 1, ds.data_ptr(), df.data_ptr(),
                                      d.data_ptr(), o.data_ptr(), ln.data_ptr(), n,
                                      res.data_ptr(), ws.data_ptr(), ws.numel(), st) == 0
    got = res.cpu().numpy()
    assert np.array_equal(got, a.tx_res), (e.name, np.nonzero(got != a.tx_res)[0][:8])
    assert np.array_equal(got, e.tx_codes.astype(np.uint8)), e.name
    sealed = d.cpu().numpy()
    assert np.array_equal(sealed, a.sealed), (e.name, np.nonzero(sealed != a.sealed)[0][:8])
    d2, ln2 = _dev(a.rx, dev), _dev(e.rx_lens.view(np.int32), dev)
    res.fill_(9)
    iv = torch.full((n, IVLEN), SENTINEL, dtype=torch.uint8, device=dev)
    oseq = torch.full((n,), 7, dtype=torch.int32, device=dev)
    ofl = torch.full((n,), 7, dtype=torch.int32, device=dev)
    assert L.net2_packet_decode_burst(alg, key, hl, 1, IVLEN, d2.data_ptr(), o.data_ptr(),
                                      ln2.data_ptr(), n, res.data_ptr(), iv.data_ptr(),
                                      oseq.data_ptr(), ofl.data_ptr(), ws.data_ptr(),
                                      ws.numel(), st) == 0
    check_rx(c, a, res.cpu().numpy(), iv.cpu().numpy(), oseq.cpu().numpy().view(np.uint32),
             ofl.cpu().numpy().view(np.uint32), SENTINEL)
    return _lib.workspace_stats(ws.data_ptr(), ws.numel())


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("alg", B.ALGS)
@pytest.mark.parametrize("fam", ["L1", "L2", "L3", "L4", "B1"])
def test_device_bursts(dev, oracle_mod, limits, fam, alg, form):
    """Encode then decode in each form: the residue x length lattice, the
    pad-table waves, the wave's vote with one odd lane, the burst that is
    uniform only once binned, and every bit of the hash field flipped."""
    limits(form)
    for c in family(fam, alg):
        stats = device_tx_rx(dev, oracle_mod, c)
        if form == "binned":
            # both launches did bin (L4: the binned waves are the uniform ones)
            assert stats["binned"] >= 1 and stats["aborts"] == 0, (c.expect.name, stats)
            assert stats["mismatches"] == 0, stats
        else:
            assert stats["binned"] == 0, (c.expect.name, stats)
    if fam == "B1":
        e = c.expect
        assert e.counts[B.FIELD] == 8 * B.HL[alg] and e.counts[B.CONTROL] >= 64
        a = B.answers(oracle_mod, c)
        assert (a.rx_res[e.kinds == B.FIELD] == B.BAD).all()


@pytest.mark.parametrize("form", ["lane", "wave"])
@pytest.mark.parametrize("alg", B.ALGS)
def test_alternate_key(dev, oracle_mod, limits, alg, form):
    """net2_packet_decode_burst_ck during a key rollover: the odd datagrams
    carry PH_ALTKEY and were sealed under the alternate key.  Every field bit
    under either key, the lattice at residues 8, 4 and 1; the datagram whose
    flipped header bit is PH_ALTKEY is checked against the other key and
    refused."""
    from ilias_net2_amd import _lib
    L = _lib.lib()
    limits(form)
    hl = B.HL[alg]
    st = torch.cuda.current_stream().cuda_stream
    cases = [B.B1(alg, r, plen, altkey=True) for r in (8, 4, 1) for plen in (100, 0)]
    cases += [B.L1(alg, r, "perm", altkey=True) for r in (8, 4, 1)]
    for c in cases:
        e = c.expect
        a = B.answers(oracle_mod, c)
        assert a.alt and 0 < (a.group == 1).sum() < e.n
        n = e.n
        kb = ctypes.create_string_buffer(a.keys[0], hl)
        ab = ctypes.create_string_buffer(a.keys[1], hl)
        ks = _lib.BurstRxKeys(alg, ctypes.cast(kb, ctypes.c_void_p), hl, 1,
                              ctypes.cast(ab, ctypes.c_void_p), hl, 1, 0, 0)
        ws = workspace(L, n, dev)
        d, o = _dev(a.rx, dev), _dev(c.offs.view(np.int64), dev)
        ln = _dev(e.rx_lens.view(np.int32), dev)
        res = torch.full((n,), 9, dtype=torch.uint8, device=dev)
        iv = torch.full((n, IVLEN), SENTINEL, dtype=torch.uint8, device=dev)
        oseq = torch.full((n,), 7, dtype=torch.int32, device=dev)
        ofl = torch.full((n,), 7, dtype=torch.int32, device=dev)
        assert L.net2_packet_decode_burst_ck(ctypes.byref(ks), IVLEN, d.data_ptr(),
                                             o.data_ptr(), ln.data_ptr(), n, res.data_ptr(),
                                             iv.data_ptr(), oseq.data_ptr(), ofl.data_ptr(),
                                             ws.data_ptr(), ws.numel(), st) == 0
        check_rx(c, a, res.cpu().numpy(), iv.cpu().numpy(),
                 oseq.cpu().numpy().view(np.uint32), ofl.cpu().numpy().view(np.uint32),
                 SENTINEL)
        if e.name.startswith("B1"):
            hd = a.rx_res[e.kinds == B.HEADER]
            assert (hd == B.BAD).sum() == 1 and (hd == B.UNSAFE).sum() == 2


@pytest.mark.parametrize("order", ["lane", "binned"])
@pytest.mark.parametrize("alg", B.ALGS)
def test_many_connections(dev, oracle_mod, limits, alg, order):
    """net2_packet_{encode,decode}_burst_mc, datagram i on connection i % 3
    (three keys in every wave): every field bit, the lattice at residues 8, 4
    and 1, the pad-table waves."""
    from ilias_net2_amd import conn_burst
    limits(order)
    K = 3
    cases = [B.B1(alg, r, plen) for r in (8, 4, 1) for plen in (100, 0)]
    cases += [B.L1(alg, r, "perm") for r in (8, 4, 1)] + B.L2_all(alg)
    with conn_burst.KeyTable(alg, K) as tab:
        for k in range(K):
            tab.set_rx(k, B.keys_for(alg, 2 + k), enc_set=True)
            tab.set_tx(k, B.keys_for(alg, 2 + k), enc_set=True)
        for c in cases:
            e = c.expect
            a = B.answers(oracle_mod, c, nconn=K)
            conn = _dev((np.arange(e.n) % K).astype(np.int32), dev)
            ws = conn_burst.burst_workspace(e.n, dev)
            d, o = _dev(c.data, dev), _dev(c.offs.view(np.int64), dev)
            res = conn_burst.encode_burst_mc(
                tab, conn, _dev(c.seq.view(np.int32), dev),
                _dev(c.flags.view(np.int32), dev), d, o, _dev(c.lens.view(np.int32), dev),
                workspace=ws)
            assert np.array_equal(res.cpu().numpy(), a.tx_res), e.name
            assert np.array_equal(d.cpu().numpy(), a.sealed), e.name
            r, iv, sq, fl = conn_burst.decode_burst_mc(
                tab, conn, _dev(a.rx, dev), o, _dev(e.rx_lens.view(np.int32), dev),
                ivlen=IVLEN, workspace=ws)
            check_rx(c, a, r.cpu().numpy(), iv.cpu().numpy(),
                     sq.cpu().numpy().view(np.uint32), fl.cpu().numpy().view(np.uint32), 0)


def host_cases(alg):
    out = [B.B1(alg, r, plen) for r in (8, 1) for plen in (100, 0)]
    out += [B.B1(alg, 8, plen, lead=True) for plen in (100, 0)]
    out += [B.L1(alg, r, "perm") for r in (8, 1)]
    return out + [B.L3(alg, 65, "unsigned@0", 0), B.L3(alg, 257, "runt@0", 0), B.L4(alg)]


@pytest.mark.parametrize("form", ["lane", "wave"])
@pytest.mark.parametrize("memory", ["pinned", "pageable"])
@pytest.mark.parametrize("alg", B.ALGS)
def test_host_bursts(dev, oracle_mod, limits, alg, memory, form):
    """net2_packet_{encode,decode}_burst_host from a page-locked arena and
    from pageable memory.

    The start alignment the kernel sees is not the caller's.  Packed form
    (pageable memory, or page-locked but sparse): pack_fill copies every
    datagram to a 16-byte aligned staging offset, so every lane has offset
    residue 0 and p = 8 (mod 16): HMAC-SHA256 runs A4 whatever the caller's
    layout.  Direct form (datagrams dense in one page-locked allocation, as
    all of these are): the range from the first datagram's first byte is
    copied as it lies and the offsets are rebased to it, so the kernel sees
    (offset - first offset) mod 16 -- again residue 0 for the cases at one
    residue (B1, L1 at 8 and at 1: A4), the true residues where the first
    datagram lies at residue 0 (B1 with a lead datagram: every field bit on
    the A16 compare; the two L3 cases: A16 waves with a refused lane at
    residue 0), and residues 0 / 12 / 9 mixed in every wave for L4 (A1)."""
    from ilias_net2_amd import _lib
    L = _lib.lib()
    limits(form)
    for c in host_cases(alg):
        e = c.expect
        a = B.answers(oracle_mod, c)
        key = a.keys[0]
        if memory == "pinned":
            buf = H.pinned(c.data.shape, np.uint8)
            assert buf.ctypes.data % 16 == 0
        else:
            buf = np.empty_like(c.data)
        buf[:] = c.data
        seq, flags = np.array(c.seq), np.array(c.flags)
        offs, lens = np.array(c.offs), np.array(c.lens)
        res = H.encode_host(L, alg, key, True, seq, flags, buf, offs, lens)
        assert np.array_equal(res, a.tx_res), e.name
        assert np.array_equal(buf, a.sealed), e.name
        buf[:] = a.rx
        got = H.decode_host(L, H.rx_keys(alg, key, True), IVLEN, buf, offs,
                            np.array(e.rx_lens))
        check_rx(c, a, got["res"], got["iv"], got["seq"], got["fl"], None)


@pytest.mark.parametrize("binned", [False, True])
@pytest.mark.parametrize("alg", B.ALGS)
def test_datagram_sign_verify(dev, oracle_mod, alg, binned):
    """batch.hmac_sign_dev / hmac_verify_dev on the header-less shape (field
    at the datagram start; residue 0 is A16, 4 is A4, 1 is A1): every field
    bit, and the pad-table waves."""
    from ilias_net2_amd import batch
    cases = [B.B1(alg, r, plen, hdr=False) for r in (0, 4, 1) for plen in (100, 0)]
    cases += B.L2_all(alg, (0, 4, 1), hdr=False)
    for c in cases:
        e = c.expect
        a = B.dgram_answers(oracle_mod, c)
        d, o = _dev(c.data, dev), _dev(c.offs.view(np.int64), dev)
        ln = _dev(c.lens.view(np.int32), dev)
        batch.hmac_sign_dev(alg, a.key, d, o, ln, binned=binned)
        assert np.array_equal(d.cpu().numpy(), a.signed), e.name
        got = batch.hmac_verify_dev(alg, a.key, _dev(a.rx, dev), o, ln,
                                    binned=binned).cpu().numpy()
        assert np.array_equal(got, a.verdict), (e.name, np.nonzero(got != a.verdict)[0][:8])
        if e.name.startswith("B1"):
            assert np.array_equal(got, (e.kinds != B.CONTROL).astype(np.uint8))


# ---- the IV output: every length, every placement ----------------------------
#
# ph_iv_one (sha2_burst.h) takes a second SHA-256 round only above 32 bytes,
# stores 16 bytes at a time only when the length is a multiple of 16 *and* the
# row's address is 16-byte aligned (decided per lane), and otherwise runs a
# byte loop; the wave forms derive the rows into LDS and copy them out
# (bw_store_iv).  The expected rows are oracle.ph_to_iv_batch's, which
# tests/test_burst_cases.py holds against hashlib at every length of B.IVLENS.

GUARD = 64                  # sentinel bytes after (and `start` before) the rows
CK_IVLENS = (1, 24, 33, 48, 64)


def iv_rows(oracle_mod, seq, fl, ivlen):
    return np.array(oracle_mod.ph_to_iv_batch(seq, fl, ivlen, nthreads=1)
                    ).reshape(len(seq), ivlen)


def head(c, a, m):
    """The first m datagrams of a case and of its answers, for check_rx (the
    datagrams of a burst are decoded independently of each other)."""
    e = c.expect
    c2 = c._replace(expect=types.SimpleNamespace(name=f"{e.name}[:{m}]", n=m,
                                                 rx_codes=e.rx_codes[:m]))
    a2 = types.SimpleNamespace(rx_res=a.rx_res[:m], rx_seq=a.rx_seq[:m],
                               rx_fl=a.rx_fl[:m], rx_iv=a.rx_iv[:m])
    return c2, a2


def decode_rows(dev, c, a, ivlen, call, start=0, tail=GUARD, m=None, null_iv=False):
    """One RX burst over the first m (default: all) datagrams of the case's
    received bytes through `call(L, ivlen, d, o, ln, m, res, iv, seq, fl, ws,
    ws_bytes, stream)` -- the C entry point, given device addresses -- with
    the IV rows a slice of m * ivlen bytes that starts `start` bytes into an
    allocation of SENTINEL bytes and ends `tail` bytes before its end.
    Returns the host outputs, the whole allocation and the workspace's
    binning statistics."""
    from ilias_net2_amd import _lib
    L = _lib.lib()
    e = c.expect
    m = e.n if m is None else m
    st = torch.cuda.current_stream().cuda_stream
    ws = workspace(L, m, dev)
    d, o = _dev(a.rx, dev), _dev(c.offs[:m].view(np.int64), dev)
    ln = _dev(e.rx_lens[:m].view(np.int32), dev)
    res = torch.full((m,), 9, dtype=torch.uint8, device=dev)
    room = torch.full((max(start + m * ivlen + tail, 1),), SENTINEL, dtype=torch.uint8,
                      device=dev)
    assert room.data_ptr() % 16 == 0
    oseq = torch.full((m,), 7, dtype=torch.int32, device=dev)
    ofl = torch.full((m,), 7, dtype=torch.int32, device=dev)
    # (an empty slice has no address of its own: the array's address is given)
    rc = call(L, ivlen, d.data_ptr(), o.data_ptr(), ln.data_ptr(), m, res.data_ptr(),
              None if null_iv else room.data_ptr() + start, oseq.data_ptr(),
              ofl.data_ptr(), ws.data_ptr(), ws.numel(), st)
    assert rc == 0, (e.name, rc)
    torch.cuda.synchronize()
    got = room.cpu().numpy()
    return types.SimpleNamespace(
        res=res.cpu().numpy(), room=got,
        iv=got[start:start + m * ivlen].reshape(m, ivlen),
        before=got[:start], after=got[start + m * ivlen:],
        seq=oseq.cpu().numpy().view(np.uint32), fl=ofl.cpu().numpy().view(np.uint32),
        stats=_lib.workspace_stats(ws.data_ptr(), ws.numel()))


def plain_call(alg, key):
    """net2_packet_decode_burst under one key, the cipher set."""
    def call(L, ivlen, d, o, ln, m, res, iv, seq, fl, ws, wsb, st):
        return L.net2_packet_decode_burst(alg, key, B.HL[alg], 1, ivlen, d, o, ln, m,
                                          res, iv, seq, fl, ws, wsb, st)
    return call


def ck_call(alg, key, alt):
    """net2_packet_decode_burst_ck with an alternate key installed."""
    from ilias_net2_amd import _lib
    hl = B.HL[alg]

    def call(L, ivlen, d, o, ln, m, res, iv, seq, fl, ws, wsb, st):
        kb, ab = ctypes.create_string_buffer(key, hl), ctypes.create_string_buffer(alt, hl)
        ks = _lib.BurstRxKeys(alg, ctypes.cast(kb, ctypes.c_void_p), hl, 1,
                              ctypes.cast(ab, ctypes.c_void_p), hl, 1, 0, 0)
        return L.net2_packet_decode_burst_ck(ctypes.byref(ks), ivlen, d, o, ln, m, res,
                                             iv, seq, fl, ws, wsb, st)
    return call


def check_rows(c, a, g, rows, form, due=None):
    """check_rx on decode_rows' outputs, the guard bytes around the rows, and
    the form's binning statistics."""
    check_rx(c, a, g.res, g.iv, g.seq, g.fl, SENTINEL, rows=rows, due=due)
    assert (g.before == SENTINEL).all() and (g.after == SENTINEL).all(), c.expect.name
    if form == "binned":
        assert g.stats["binned"] >= 1 and g.stats["aborts"] == 0, g.stats
        assert g.stats["mismatches"] == 0, g.stats
    else:
        assert g.stats["binned"] == 0, g.stats


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("alg", B.ALGS)
@pytest.mark.parametrize("ivlen", B.IVLENS)
def test_iv_lengths(dev, oracle_mod, limits, ivlen, alg, form):
    """net2_packet_decode_burst at every IV length of B.IVLENS on the
    every-bit case (OK, BAD, UNSAFE and header-flipped rows in every wave):
    the OK rows are the oracle's, every other row and the bytes around the
    array keep the sentinel; ivlen 0 with an array given writes no byte."""
    limits(form)
    c = B.B1(alg, 8, 100)
    a = B.answers(oracle_mod, c)
    g = decode_rows(dev, c, a, ivlen, plain_call(alg, a.keys[0]))
    check_rows(c, a, g, iv_rows(oracle_mod, a.rx_seq, a.rx_fl, ivlen), form)
    ok = a.rx_res == B.OK
    assert ok.any() and (a.rx_res == B.BAD).any() and (a.rx_res == B.UNSAFE).any()
    if ivlen == 0:
        assert (g.room == SENTINEL).all()


@pytest.mark.parametrize("form", ["lane", "wave"])
@pytest.mark.parametrize("alg", B.ALGS)
@pytest.mark.parametrize("ivlen", CK_IVLENS)
def test_iv_lengths_alternate_key(dev, oracle_mod, limits, ivlen, alg, form):
    """The same through net2_packet_decode_burst_ck during a key rollover
    (odd datagrams under the alternate key)."""
    limits(form)
    c = B.B1(alg, 8, 100, altkey=True)
    a = B.answers(oracle_mod, c)
    assert a.alt
    g = decode_rows(dev, c, a, ivlen, ck_call(alg, a.keys[0], a.keys[1]))
    check_rows(c, a, g, iv_rows(oracle_mod, a.rx_seq, a.rx_fl, ivlen), form)


_mc_answers = {}


def mc_answers(oracle_mod, c, ivlen, K=3, plain=1):
    """The oracle's decode of the case's received bytes with datagram i on
    connection i % K; connection `plain` has no cipher set (enc_set false:
    PH_ENCRYPTED is not demanded and no IV is due)."""
    e = c.expect
    tag = (e.name, ivlen, K, plain)
    if tag in _mc_answers:
        return _mc_answers[tag]
    a = B.answers(oracle_mod, c, nconn=K)
    res = np.full(e.n, 9, dtype=np.uint8)
    iv = np.zeros((e.n, ivlen), dtype=np.uint8)
    seq, fl = np.zeros(e.n, dtype=np.uint32), np.zeros(e.n, dtype=np.uint32)
    due = np.zeros(e.n, dtype=bool)
    for k in range(K):
        idx = np.nonzero(a.group == k)[0]
        r, v, s, f = oracle_mod.packet_decode_batch(
            e.alg, a.keys[k], k != plain, ivlen, a.rx, c.offs[idx], e.rx_lens[idx],
            nthreads=1)
        res[idx], seq[idx], fl[idx] = r, s, f
        iv[idx] = np.array(v).reshape(len(idx), ivlen)
        due[idx] = (r == B.OK) & (k != plain) & ((f & B.PH_ENCRYPTED) != 0)
    rows = iv_rows(oracle_mod, seq, fl, ivlen)
    # the oracle's decode derives exactly the rows that are due
    assert np.array_equal(iv[due], rows[due]) and not iv[~due].any()
    out = types.SimpleNamespace(rx=a.rx, keys=a.keys, rx_res=res, rx_seq=seq, rx_fl=fl, rx_iv=rows,
                   due=due, group=a.group)
    _mc_answers[tag] = out
    return out


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("alg", B.ALGS)
@pytest.mark.parametrize("ivlen", B.IVLENS)
def test_iv_lengths_many_connections(dev, oracle_mod, limits, ivlen, alg, form):
    """net2_packet_decode_burst_mc, datagram i on connection i % 3, at every
    IV length: connection 1 has no cipher set, so its OK rows keep the
    sentinel like the refused rows of the other two."""
    from ilias_net2_amd import conn_burst
    limits(form)
    K = 3
    c = B.B1(alg, 8, 100)
    a = mc_answers(oracle_mod, c, ivlen, K)
    plain_ok = (a.rx_res == B.OK) & (a.group == 1)
    assert plain_ok.sum() > 20 and not a.due[plain_ok].any() and a.due.sum() > 40
    with conn_burst.KeyTable(alg, K) as tab:
        for k in range(K):
            tab.set_rx(k, a.keys[k], enc_set=(k != 1))
        conn = _dev((np.arange(c.expect.n) % K).astype(np.int32), dev)

        def call(L, ivlen, d, o, ln, m, res, iv, seq, fl, ws, wsb, st):
            return L.net2_packet_decode_burst_mc(tab.ptr, conn.data_ptr(), ivlen, d, o, ln,
                                                 m, res, iv, seq, fl, ws, wsb, st)
        g = decode_rows(dev, c, a, ivlen, call)
    check_rows(c, a, g, a.rx_iv, form, due=a.due)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("alg", [4, 6])
@pytest.mark.parametrize("ivlen", [16, 32, 48, 17])
@pytest.mark.parametrize("start", [1, 4, 8])
def test_iv_placement(dev, oracle_mod, limits, start, ivlen, alg, form):
    """The IV array is a contiguous slice that starts 1, 4 or 8 bytes into
    its allocation: no row (start 8 with ivlen 16: none at all) is 16-byte
    aligned, so the 16-byte stores must not be taken, and the bytes before
    and after the slice keep the sentinel."""
    limits(form)
    c = B.B1(alg, 8, 100)
    a = B.answers(oracle_mod, c)
    g = decode_rows(dev, c, a, ivlen, plain_call(alg, a.keys[0]), start=start)
    assert len(g.before) == start and len(g.after) == GUARD
    check_rows(c, a, g, iv_rows(oracle_mod, a.rx_seq, a.rx_fl, ivlen), form)


@pytest.mark.parametrize("form", list(FORMS))
def test_iv_array_ends_with_its_allocation(dev, oracle_mod, limits, form):
    """ivlen 16 at start 0, the burst cut to a whole number of 512-byte
    allocation units: the last row's last byte is the tensor's last."""
    limits(form)
    c = B.B1(6, 8, 100)
    a = B.answers(oracle_mod, c)
    m = c.expect.n - c.expect.n % 32
    assert m > 512 and (m * IVLEN) % 512 == 0
    c2, a2 = head(c, a, m)
    g = decode_rows(dev, c, a, IVLEN, plain_call(6, a.keys[0]), tail=0, m=m)
    assert len(g.room) == m * IVLEN
    check_rows(c2, a2, g, None, form)


@pytest.mark.parametrize("form", ["lane", "binned"])
@pytest.mark.parametrize("alg", B.ALGS)
def test_null_iv_array(dev, oracle_mod, limits, alg, form):
    """d_iv = NULL with ivlen 16 in the single-connection lane and binned
    forms: codes and headers are the full call's, no IV is derived."""
    limits(form)
    c = B.B1(alg, 8, 100)
    a = B.answers(oracle_mod, c)
    g = decode_rows(dev, c, a, IVLEN, plain_call(alg, a.keys[0]), null_iv=True)
    assert np.array_equal(g.res, a.rx_res)
    assert np.array_equal(g.seq, a.rx_seq) and np.array_equal(g.fl, a.rx_fl)
    assert (g.room == SENTINEL).all()


@pytest.fixture(scope="module")
def iv_headers(dev):
    rng = np.random.default_rng(1717)
    n = 1001
    seq = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    fl = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    return seq, fl, _dev(seq.view(np.int32), dev), _dev(fl.view(np.int32), dev)


@pytest.mark.parametrize("start", [0, 1, 8])
@pytest.mark.parametrize("ivlen", B.IVLENS)
def test_ph_to_iv_dev_rows(dev, oracle_mod, iv_headers, ivlen, start):
    """net2_ph_to_iv_dev over 1,001 random headers (four workgroups, the last
    ragged): every row at every IV length, the output a slice at byte 0, 1
    and 8 of its allocation with guard bytes around it; ivlen 0 writes
    nothing; above 64 it is EINVAL."""
    import errno
    from ilias_net2_amd import _lib
    L = _lib.lib()
    seq, fl, ds, df = iv_headers
    n = len(seq)
    room = torch.full((start + n * ivlen + GUARD,), SENTINEL, dtype=torch.uint8,
                      device=dev)
    assert room.data_ptr() % 16 == 0
    st = torch.cuda.current_stream().cuda_stream
    assert L.net2_ph_to_iv_dev(ds.data_ptr(), df.data_ptr(), n, ivlen,
                               room.data_ptr() + start, st) == 0
    torch.cuda.synchronize()
    got = room.cpu().numpy()
    want = iv_rows(oracle_mod, seq, fl, ivlen)
    rows = got[start:start + n * ivlen].reshape(n, ivlen)
    assert np.array_equal(rows, want), np.nonzero((rows != want).any(axis=1))[0][:8]
    assert (got[:start] == SENTINEL).all() and (got[start + n * ivlen:] == SENTINEL).all()
    assert L.net2_ph_to_iv_dev(ds.data_ptr(), df.data_ptr(), n, 65,
                               room.data_ptr() + start, st) == errno.EINVAL
