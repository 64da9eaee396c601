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
"""
import ctypes

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


def check_rx(c, a, res, iv, seq, fl, sentinel):
    """Codes, headers, the IVs of the OK rows, and every other IV row left
    as it was."""
    e = c.expect
    assert np.array_equal(res, a.rx_res), (e.name, np.nonzero(res != a.rx_res)[0][:8])
    known = e.rx_codes >= 0
    assert np.array_equal(res[known], e.rx_codes[known]), e.name
    assert np.array_equal(seq, a.rx_seq) and np.array_equal(fl, a.rx_fl), e.name
    ok = a.rx_res == B.OK
    assert np.array_equal(iv[ok], a.rx_iv[ok]), e.name
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
