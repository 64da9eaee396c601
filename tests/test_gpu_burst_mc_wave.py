"""The wave form of the keyed bursts over many connections
(burst_wave_mc_kernel: 1 to 16 datagrams per workgroup, every datagram's keys
read from slot conn[i] of the device key table, codes / headers / IVs / sealed
fields stored by the one launch), which net2_packet_{decode,encode}_burst_mc
take for bursts of at most net2_sha2_burst_limits' wave_max datagrams.

The bursts, the key tables and the expected values are
tests/test_gpu_burst_mc.py's: the unchanged oracle called once per connection.
Every comparison is bit for bit, and net2_sha2_burst_stats tells which form
each call took.  The sizes are chosen for the datagrams per workgroup, G =
ceil(n / SIMDs) <= 16, on a 256-CU device (1,024 SIMDs): 1, 63, 65 (G = 1),
1,025 (G = 2, the last workgroup half empty), 3,001 (G = 3, 64 % G != 0) and
16,385 (forced: G capped at 16, more workgroups than SIMDs).
"""
import ctypes

import numpy as np
import pytest

import burst_cases as B
import test_gpu_burst_lattice as LT
import test_gpu_burst_mc as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

OK, NOCONN = M.OK, M.NOCONN
IVLEN = M.IVLEN
WAVE, LANE = 1 << 30, 0
SENTINEL = 0xA5


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
    yield L.net2_sha2_burst_limits
    L.net2_sha2_burst_limits(-1, -1)


@pytest.fixture
def wave(limits):
    """Every keyed burst of the test in the wave form."""
    assert limits(WAVE, -1) == 0


@pytest.fixture
def set_form(limits):
    """test_gpu_burst_lattice's `limits`: a form by name."""
    def set_form(form):
        assert limits(*LT.FORMS[form]) == 0
    return set_form


def stats():
    from ilias_net2_amd import conn_burst
    return np.array(conn_burst.burst_stats(), dtype=np.int64)       # (lane, wave)


# ---- 1. oracle parity in the wave form

SIZES = [(h, K, n) for h in (4, 5, 6) for K in (1, 5, 257) for n in (1, 63, 65, 1025, 3001)]
SIZES.append((6, 257, 16385))


@pytest.mark.parametrize("hash_alg,K,n", SIZES)
def test_oracle_parity_wave_form(dev, oracle_mod, wave, hash_alg, K, n):
    """TX, then RX of the sealed datagrams with tampered bytes and runts:
    every TX code, sealed byte, RX code, header and IV against the
    per-connection oracle, in exactly two wave launches."""
    c = M.case(oracle_mod, hash_alg, K, n)
    tab = M.make_table(c)
    try:
        before = stats()
        got = M.run_tx_rx(dev, c, tab)
        took = stats() - before
    finally:
        tab.close()
    M.check_against(got, c)
    assert took.tolist() == [0, 2], took


# ---- 2. the two forms against each other, untouched rows included

def _c_abi_tx_rx(dev, c, tab, ws, d_seq=True, d_iv=True):
    """Both _mc calls through the C ABI, every output pre-filled with a
    sentinel; everything back on the host.  d_seq / d_iv False: NULL."""
    from ilias_net2_amd import _lib
    L = _lib.lib()
    n = c.n
    st = torch.cuda.current_stream().cuda_stream
    o = M._dev(c.offs.view(np.int64), dev)
    d = M._dev(c.data, dev)
    tx_res = torch.full((n,), 9, dtype=torch.uint8, device=dev)
    assert L.net2_packet_encode_burst_mc(
        tab.ptr, M._dev(c.txconn.view(np.int32), dev).data_ptr(),
        M._dev(c.seq.view(np.int32), dev).data_ptr(),
        M._dev(c.flags.view(np.int32), dev).data_ptr(), d.data_ptr(), o.data_ptr(),
        M._dev(c.slot.view(np.int32), dev).data_ptr(), n, tx_res.data_ptr(), ws.data_ptr(),
        ws.numel(), st) == 0
    rx_res = torch.full((n,), 9, dtype=torch.uint8, device=dev)
    iv = torch.full((n, IVLEN), SENTINEL, dtype=torch.uint8, device=dev)
    oseq = torch.full((n,), 7, dtype=torch.int32, device=dev)
    ofl = torch.full((n,), 7, dtype=torch.int32, device=dev)
    assert L.net2_packet_decode_burst_mc(
        tab.ptr, M._dev(c.conn.view(np.int32), dev).data_ptr(), IVLEN,
        M._dev(c.rx, dev).data_ptr(), o.data_ptr(),
        M._dev(c.lens.view(np.int32), dev).data_ptr(), n, rx_res.data_ptr(),
        iv.data_ptr() if d_iv else None, oseq.data_ptr() if d_seq else None,
        ofl.data_ptr() if d_seq else None, ws.data_ptr(), ws.numel(), st) == 0
    torch.cuda.synchronize()
    return dict(tx_res=tx_res.cpu().numpy(), sealed=d.cpu().numpy(),
                rx_res=rx_res.cpu().numpy(), rx_iv=iv.cpu().numpy(),
                rx_seq=oseq.cpu().numpy().view(np.uint32),
                rx_fl=ofl.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("hash_alg", [4, 6])
def test_forms_agree(dev, oracle_mod, limits, hash_alg):
    """n = 3,001 over 257 connections under wave_max 0 and 2^30: every output
    array and the sealed buffer identical, the rows neither form writes (IVs
    that are not due) still the sentinel in both."""
    from ilias_net2_amd import conn_burst
    c = M.case(oracle_mod, hash_alg, 257, 3001)
    tab = M.make_table(c)
    outs = []
    try:
        for wave_max, want in ((LANE, [2, 0]), (WAVE, [0, 2])):
            assert limits(wave_max, -1) == 0
            ws = conn_burst.burst_workspace(c.n, dev)
            before = stats()
            outs.append(_c_abi_tx_rx(dev, c, tab, ws))
            assert (stats() - before).tolist() == want
    finally:
        tab.close()
    for name, a in outs[0].items():
        assert np.array_equal(a, outs[1][name]), name
    got = outs[1]
    assert np.array_equal(got["tx_res"], c.tx_res) and np.array_equal(got["sealed"], c.sealed)
    assert np.array_equal(got["rx_res"], c.rx_res)
    ok = c.rx_res == OK
    due = ok & c.enc[c.conn] & ((c.rx_fl & 1) != 0)
    assert due.sum() > 0 and (ok & ~due).sum() > 0
    assert np.array_equal(got["rx_iv"][due], c.rx_iv[due])
    assert (got["rx_iv"][~due] == SENTINEL).all()


# ---- 3. test_gpu_burst_mc's own tests again, in the wave form

def test_missing_connections_wave_form(dev, oracle_mod, wave):
    before = stats()
    M.test_missing_connections(dev, oracle_mod)
    assert (stats() - before).tolist() == [0, 2]


def test_updates_are_stream_ordered_wave_form(dev, oracle_mod, wave):
    before = stats()
    M.test_updates_are_stream_ordered(dev, oracle_mod)
    assert (stats() - before).tolist() == [0, 4]


@pytest.mark.parametrize("hash_alg", [4, 5, 6])
def test_one_connection_equals_the_single_connection_calls_wave_form(dev, oracle_mod, wave,
                                                                     hash_alg):
    """burst_wave_mc_kernel against burst_wave_kernel on the same input."""
    before = stats()
    M.test_one_connection_equals_the_single_connection_calls(dev, oracle_mod, hash_alg)
    assert (stats() - before).tolist() == [0, 4]


# ---- 4. every hash-field bit under three connections

@pytest.mark.parametrize("alg", B.ALGS)
def test_many_connections_wave_form(dev, oracle_mod, set_form, alg):
    """test_gpu_burst_lattice.test_many_connections (B1 at residues 8 / 4 / 1
    with payloads 100 and 0, L1 "perm" at 8 / 4 / 1, every L2 case, datagram i
    on connection i % 3) with every burst in the wave form."""
    ncases = 6 + 3 + len(B.L2_all(alg))
    before = stats()
    LT.test_many_connections(dev, oracle_mod, set_form, alg, "wave")
    assert (stats() - before).tolist() == [0, 2 * ncases]


# ---- 5. NULL outputs

def test_null_outputs(dev, oracle_mod, wave):
    """d_seq = d_flags = NULL, and d_iv = NULL, at n = 1,025: the codes and
    the remaining outputs are the full call's, nothing is stored in place of
    the missing arrays, and the workspace -- checked, not used -- keeps every
    byte."""
    c = M.case(oracle_mod, 6, 5, 1025)
    tab = M.make_table(c)
    try:
        from ilias_net2_amd import _lib
        L = _lib.lib()
        ws = torch.full((L.net2_packet_burst_workspace(c.n),), 0x3C, dtype=torch.uint8,
                        device=dev)
        before = stats()
        full = _c_abi_tx_rx(dev, c, tab, ws)
        no_hdr = _c_abi_tx_rx(dev, c, tab, ws, d_seq=False)
        no_iv = _c_abi_tx_rx(dev, c, tab, ws, d_iv=False)
        assert (stats() - before).tolist() == [0, 6]
        assert bool((ws == 0x3C).all())
    finally:
        tab.close()
    assert np.array_equal(full["rx_res"], c.rx_res) and np.array_equal(full["rx_seq"], c.rx_seq)
    for name in ("tx_res", "sealed", "rx_res", "rx_iv"):
        assert np.array_equal(no_hdr[name], full[name]), name
    assert (no_hdr["rx_seq"] == 7).all() and (no_hdr["rx_fl"] == 7).all()
    for name in ("tx_res", "sealed", "rx_res", "rx_seq", "rx_fl"):
        assert np.array_equal(no_iv[name], full[name]), name
    assert (no_iv["rx_iv"] == SENTINEL).all()
    assert (full["rx_iv"] != SENTINEL).any()


# ---- 6. the threshold

def _decode(dev, c, tab, n):
    """decode_burst_mc of the case's first n datagrams, and the form it took."""
    from ilias_net2_amd import conn_burst
    before = stats()
    r, iv, sq, fl = conn_burst.decode_burst_mc(
        tab, M._dev(c.conn[:n].view(np.int32), dev), M._dev(c.rx, dev),
        M._dev(c.offs[:n].view(np.int64), dev), M._dev(c.lens[:n].view(np.int32), dev),
        ivlen=IVLEN)
    took = (stats() - before).tolist()
    assert took in ([1, 0], [0, 1]), took
    return ("lane" if took[0] else "wave", r.cpu().numpy(), iv.cpu().numpy(),
            sq.cpu().numpy().view(np.uint32), fl.cpu().numpy().view(np.uint32))


def test_threshold(dev, oracle_mod, limits):
    """Default limits: 64 datagrams take the wave form.  wave_max 4,096:
    4,096 datagrams take it, 4,097 the lane form, the results on the shared
    4,096 identical and the oracle's.  wave_max 0: 64 take the lane form."""
    c64 = M.case(oracle_mod, 6, 5, 64)
    c = M.case(oracle_mod, 6, 5, 4097)
    t64, tab = M.make_table(c64), M.make_table(c)
    try:
        assert limits(-1, -1) == 0
        form, r, iv, sq, fl = _decode(dev, c64, t64, 64)
        assert form == "wave" and np.array_equal(r, c64.rx_res)
        assert np.array_equal(iv, c64.rx_iv)
        assert limits(4096, -1) == 0
        at = _decode(dev, c, tab, 4096)
        over = _decode(dev, c, tab, 4097)
        assert at[0] == "wave" and over[0] == "lane"
        for a, b, want in zip(at[1:], over[1:], (c.rx_res, c.rx_iv, c.rx_seq, c.rx_fl)):
            assert np.array_equal(a, b[:4096]) and np.array_equal(b, want)
        assert limits(0, -1) == 0
        form, r, iv, sq, fl = _decode(dev, c64, t64, 64)
        assert form == "lane" and np.array_equal(r, c64.rx_res)
        assert np.array_equal(iv, c64.rx_iv)
    finally:
        t64.close()
        tab.close()
