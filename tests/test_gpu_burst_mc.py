"""Keyed packet bursts over many connections: the device key table
(net2_burst_keytab_*) and net2_packet_{decode,encode}_burst_mc, in which the
lane of datagram i takes its keys from slot conn[i].

The expected values come from the unchanged oracle: the datagrams are
grouped by connection, oracle.packet_decode_batch / packet_encode_batch is
called once per connection with that connection's keys (alternate key,
cutoff, rx_start, enc_set), and the results are scattered back.  What the
oracle does not know is stated here: a datagram whose connection is missing
is NET2_PBURST_NOCONN -- after the header decode, so a runt stays
NET2_PDECODE_BAD -- with its header decoded, no IV, and (TX) its slot
untouched.

The datagrams are test_gpu_burst_wave._burst's: payload lengths on both
sides of the 55/56 and 111/112/119/120/127/128 padding edges, slots without
room, flags that lack PH_SIGNED, PH_ALTKEY on some.
"""
import ctypes
import errno
import functools
import types

import numpy as np
import pytest

import test_gpu_burst_wave as W
import test_gpu_packet as P

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

OK, RESOURCE, BAD, UNSAFE, NOCONN = 0, 1, 2, 3, 5
HL = P.HL
IVLEN = 16
CPU_THREADS = P.CPU_THREADS


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


def _dev(a, dev):
    """A device copy (through a writable host copy: the shared case's arrays
    are read-only)."""
    return torch.from_numpy(np.array(a, order="C")).to(dev)


def _threads(m):
    return CPU_THREADS if m >= 256 else 1


@functools.lru_cache(maxsize=None)
def case(oracle_mod, hash_alg, K, n):
    """One burst of n datagrams over K connections and what the oracle, one
    call per connection, makes of it: TX, then RX of the sealed datagrams
    with tampered bytes and runts.  Computed once per (row, K, n); the tests
    that share it leave it unchanged."""
    seed = 9000 + 1000 * hash_alg + 10 * K + n
    data, offs, slot, seq, flags, rng = W._burst(n, seed, hash_alg, True)
    hl = HL[hash_alg]
    conn = rng.integers(0, K, n).astype(np.uint32)   # mixed within every wave
    keys = [rng.integers(0, 256, hl, dtype=np.uint8).tobytes() for _ in range(K)]
    alt_keys = [rng.integers(0, 256, hl, dtype=np.uint8).tobytes() for _ in range(K)]
    enc = rng.random(K) < 0.5
    has_alt = rng.random(K) < 1 / 3
    enc[0], has_alt[0] = True, True
    if K > 1:
        enc[1], has_alt[1] = False, False
    no_cutoff = rng.random(K) < 0.5
    if K > 1:
        no_cutoff[0] = False
    rx_start = rng.integers(0, 2**32, K, dtype=np.uint64)
    cutoff = (rx_start + rng.integers(2**30, 3 * 2**30, K, dtype=np.uint64)) % 2**32
    # flags as each connection's keys call for, some wrong either way
    flags[~enc[conn]] &= ~np.uint32(P.PH_ENCRYPTED)
    flags[rng.random(n) < 0.06] ^= P.PH_ENCRYPTED
    # the transmitter seals with the key the receiver will pick
    # (net2_ck_tx_key): tx slot k holds connection k's active key, K + k its
    # alternate key
    picks = np.array([P.ref_rx_key(int(seq[i]), int(flags[i]), bool(has_alt[c]),
                                   bool(no_cutoff[c]), int(cutoff[c]), int(rx_start[c]))
                      for i, c in enumerate(conn)])
    txconn = (conn + K * picks).astype(np.uint32)
    tx_res = np.full(n, 9, dtype=np.uint8)
    sealed = data.copy()
    for t in np.unique(txconn):
        idx = np.nonzero(txconn == t)[0]
        k = int(t) % K
        r, out = oracle_mod.packet_encode_batch(
            hash_alg, alt_keys[k] if t >= K else keys[k], bool(enc[k]), seq[idx],
            flags[idx], data, offs[idx], slot[idx], nthreads=_threads(len(idx)))
        tx_res[idx] = r
        for i in idx:
            a, b = int(offs[i]), int(offs[i]) + int(slot[i])
            sealed[a:b] = out[a:b]
    # RX: what TX produced, plus tampered bytes and runts
    rx = sealed.copy()
    lens = slot.copy()
    t = rng.random(n)
    for i in np.nonzero((t < 0.1) & (lens > 8))[0]:
        rx[int(offs[i]) + 8 + int(rng.integers(0, lens[i] - 8))] ^= 0x10
    lens[(t >= 0.1) & (t < 0.13)] = 5
    rx_res = np.full(n, 9, dtype=np.uint8)
    rx_iv = np.zeros((n, IVLEN), dtype=np.uint8)
    rx_seq, rx_fl = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    for k in range(K):
        idx = np.nonzero(conn == k)[0]
        if len(idx) == 0:
            continue
        r, iv, sq, fl = oracle_mod.packet_decode_batch(
            hash_alg, keys[k], bool(enc[k]), IVLEN, rx, offs[idx], lens[idx],
            alt_key=alt_keys[k] if has_alt[k] else None,
            alt_no_cutoff=bool(no_cutoff[k]), alt_cutoff=int(cutoff[k]),
            rx_start=int(rx_start[k]), nthreads=_threads(len(idx)))
        rx_res[idx], rx_iv[idx], rx_seq[idx], rx_fl[idx] = r, iv, sq, fl
    for a in (data, offs, slot, seq, flags, conn, txconn, tx_res, sealed, rx, lens,
              rx_res, rx_iv, rx_seq, rx_fl, picks):
        a.setflags(write=False)
    return types.SimpleNamespace(
        hash_alg=hash_alg, K=K, n=n, hl=hl, data=data, offs=offs, slot=slot, seq=seq,
        flags=flags, conn=conn, keys=keys, alt_keys=alt_keys, enc=enc, has_alt=has_alt,
        no_cutoff=no_cutoff, rx_start=rx_start, cutoff=cutoff, picks=picks,
        txconn=txconn, tx_res=tx_res, sealed=sealed, rx=rx, lens=lens, rx_res=rx_res,
        rx_iv=rx_iv, rx_seq=rx_seq, rx_fl=rx_fl)


def set_rx(tab, c, k, slot=None):
    tab.set_rx(k if slot is None else slot, c.keys[k], enc_set=bool(c.enc[k]),
               alt_key=c.alt_keys[k] if c.has_alt[k] else None,
               alt_no_cutoff=bool(c.no_cutoff[k]), alt_cutoff=int(c.cutoff[k]),
               rx_start=int(c.rx_start[k]))


def make_table(c, extra=0):
    """Slots [0, K): connection k's rx state and its active key as tx key;
    [K, 2K): its alternate key as tx key, where it has one."""
    from ilias_net2_amd import conn_burst
    tab = conn_burst.KeyTable(c.hash_alg, 2 * c.K + extra)
    for k in range(c.K):
        set_rx(tab, c, k)
        tab.set_tx(k, c.keys[k], enc_set=bool(c.enc[k]))
        if c.has_alt[k]:
            tab.set_tx(c.K + k, c.alt_keys[k], enc_set=bool(c.enc[k]))
    return tab


def run_tx_rx(dev, c, tab, ws=None):
    """encode_burst_mc of the case's slots, then decode_burst_mc of its RX
    datagrams; everything back on the host."""
    from ilias_net2_amd import conn_burst
    o = _dev(c.offs.view(np.int64), dev)
    d = _dev(c.data, dev)
    res = conn_burst.encode_burst_mc(
        tab, _dev(c.txconn.view(np.int32), dev), _dev(c.seq.view(np.int32), dev),
        _dev(c.flags.view(np.int32), dev), d, o, _dev(c.slot.view(np.int32), dev),
        workspace=ws)
    got = types.SimpleNamespace(tx_res=res.cpu().numpy(), sealed=d.cpu().numpy())
    r, iv, sq, fl = conn_burst.decode_burst_mc(
        tab, _dev(c.conn.view(np.int32), dev), _dev(c.rx, dev), o,
        _dev(c.lens.view(np.int32), dev), ivlen=IVLEN, workspace=ws)
    got.rx_res, got.rx_iv = r.cpu().numpy(), iv.cpu().numpy()
    got.rx_seq = sq.cpu().numpy().view(np.uint32)
    got.rx_fl = fl.cpu().numpy().view(np.uint32)
    return got


def check_against(got, c):
    """Every code, sealed byte, header and IV."""
    assert np.array_equal(got.tx_res, c.tx_res), np.nonzero(got.tx_res != c.tx_res)[0][:8]
    assert np.array_equal(got.sealed, c.sealed)
    assert np.array_equal(got.rx_res, c.rx_res), np.nonzero(got.rx_res != c.rx_res)[0][:8]
    assert np.array_equal(got.rx_seq, c.rx_seq) and np.array_equal(got.rx_fl, c.rx_fl)
    assert np.array_equal(got.rx_iv, c.rx_iv)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 3001])
@pytest.mark.parametrize("K", [1, 2, 5, 257])
@pytest.mark.parametrize("hash_alg", [4, 5, 6])
def test_mixed_keys_within_a_wave(dev, oracle_mod, hash_alg, K, n):
    c = case(oracle_mod, hash_alg, K, n)
    tab = make_table(c)
    try:
        got = run_tx_rx(dev, c, tab)
    finally:
        tab.close()
    check_against(got, c)
    if n == 3001:
        # every outcome occurred, on both sides
        for code in (OK, BAD, UNSAFE):
            assert (c.rx_res == code).sum() > 0, code
        for code in (OK, RESOURCE, UNSAFE):
            assert (c.tx_res == code).sum() > 0, code
        assert c.rx_iv[c.rx_res == OK].any() and not c.rx_iv[c.rx_res != OK].any()
        ok = c.rx_res == OK
        if K > 1:
            assert len(np.unique(c.conn[ok])) == min(K, 257)
            # both the alternate and the active key verified datagrams
            assert (ok & c.picks).sum() > 0 and (ok & ~c.picks).sum() > 0
            # and connections with and without a cipher key
            assert c.enc[c.conn[ok]].any() and not c.enc[c.conn[ok]].all()


@pytest.mark.parametrize("hash_alg,K", [(6, 257), (4, 5)])
def test_binned_and_submission_order_agree(dev, oracle_mod, limits, hash_alg, K):
    """The n = 3001 burst under net2_sha2_burst_limits(0, 0) (binned by
    datagram length) and (0, 1 << 40) (submission order): identical results,
    and the first workspace's counter shows that it did bin."""
    from ilias_net2_amd import _lib, conn_burst
    c = case(oracle_mod, hash_alg, K, 3001)
    tab = make_table(c)
    try:
        outs, stats = [], []
        for bin_min in (0, 1 << 40):
            assert limits(0, bin_min) == 0
            ws = conn_burst.burst_workspace(c.n, dev)
            outs.append(run_tx_rx(dev, c, tab, ws))
            stats.append(_lib.workspace_stats(ws.data_ptr(), ws.numel()))
    finally:
        tab.close()
    for got in outs:
        check_against(got, c)
    for name in ("tx_res", "sealed", "rx_res", "rx_iv", "rx_seq", "rx_fl"):
        assert np.array_equal(getattr(outs[0], name), getattr(outs[1], name)), name
    assert stats[0]["prepared"] and stats[0]["binned"] > 0, stats[0]
    assert stats[0]["aborts"] == 0 and stats[0]["mismatches"] == 0, stats[0]
    assert stats[1]["binned"] == 0, stats[1]


@pytest.mark.parametrize("hash_alg", [4, 5, 6])
def test_one_connection_equals_the_single_connection_calls(dev, oracle_mod, hash_alg):
    """K = 1, n = 3001: _mc against net2_packet_decode_burst_ck /
    net2_packet_encode_burst on the same input -- result, seq, flags, the
    whole IV array and every sealed byte identical."""
    from ilias_net2_amd import _lib, conn_burst
    L = _lib.lib()
    c = case(oracle_mod, hash_alg, 1, 3001)
    n, hl = c.n, c.hl
    st = torch.cuda.current_stream().cuda_stream
    ws = conn_burst.burst_workspace(n, dev)
    o = _dev(c.offs.view(np.int64), dev)
    zero = torch.zeros(n, dtype=torch.int32, device=dev)
    ds, df = _dev(c.seq.view(np.int32), dev), _dev(c.flags.view(np.int32), dev)
    sl, ln = _dev(c.slot.view(np.int32), dev), _dev(c.lens.view(np.int32), dev)
    tab = make_table(c)
    try:
        # TX under the active key
        d_mc, d_one = _dev(c.data, dev), _dev(c.data, dev)
        r_mc = conn_burst.encode_burst_mc(tab, zero, ds, df, d_mc, o, sl, workspace=ws)
        r_one = torch.full((n,), 9, dtype=torch.uint8, device=dev)
        assert L.net2_packet_encode_burst(hash_alg, c.keys[0], hl, 1, ds.data_ptr(),
                                          df.data_ptr(), d_one.data_ptr(), o.data_ptr(),
                                          sl.data_ptr(), n, r_one.data_ptr(),
                                          ws.data_ptr(), ws.numel(), st) == 0
        assert torch.equal(r_mc, r_one) and torch.equal(d_mc, d_one)
        assert int((r_one == OK).sum()) > n // 2
        # RX under the connection's whole rx key state
        rx = _dev(c.rx, dev)
        m_res, m_iv, m_seq, m_fl = conn_burst.decode_burst_mc(tab, zero, rx, o, ln,
                                                              ivlen=IVLEN, workspace=ws)
        kb = ctypes.create_string_buffer(c.keys[0], hl)
        ab = ctypes.create_string_buffer(c.alt_keys[0], hl)
        ks = _lib.BurstRxKeys(hash_alg, ctypes.cast(kb, ctypes.c_void_p), hl, 1,
                              ctypes.cast(ab, ctypes.c_void_p), hl,
                              int(c.no_cutoff[0]), int(c.cutoff[0]), int(c.rx_start[0]))
        res = torch.full((n,), 9, dtype=torch.uint8, device=dev)
        iv = torch.zeros((n, IVLEN), dtype=torch.uint8, device=dev)
        oseq = torch.full((n,), 7, dtype=torch.int32, device=dev)
        ofl = torch.full((n,), 7, dtype=torch.int32, device=dev)
        assert L.net2_packet_decode_burst_ck(ctypes.byref(ks), IVLEN, rx.data_ptr(),
                                             o.data_ptr(), ln.data_ptr(), n,
                                             res.data_ptr(), iv.data_ptr(),
                                             oseq.data_ptr(), ofl.data_ptr(),
                                             ws.data_ptr(), ws.numel(), st) == 0
        assert torch.equal(m_res, res) and torch.equal(m_iv, iv)
        assert torch.equal(m_seq, oseq) and torch.equal(m_fl, ofl)
        assert np.array_equal(res.cpu().numpy(), c.rx_res)
    finally:
        tab.close()


def test_missing_connections(dev, oracle_mod):
    """RX and TX with connection indices `slots`, 0xffffffff, a slot never
    set, a cleared slot and a slot with only its other side set, among
    datagrams of a live connection: NET2_PBURST_NOCONN except that a runt is
    NET2_PDECODE_BAD; headers decoded, IV rows untouched, TX slots
    byte-identical to their input."""
    from ilias_net2_amd import conn_burst
    c = case(oracle_mod, 6, 1, 3001)
    n, slots = c.n, 8
    rng = np.random.default_rng(77)
    LIVE, NEVER, CLEARED, TX_ONLY, RX_ONLY = 0, 5, 6, 7, 4
    tab = conn_burst.KeyTable(6, slots)
    try:
        set_rx(tab, c, 0, LIVE)
        tab.set_tx(LIVE, c.keys[0], enc_set=True)
        set_rx(tab, c, 0, CLEARED)
        tab.set_tx(CLEARED, c.keys[0], enc_set=True)
        tab.clear(CLEARED)
        tab.set_tx(TX_ONLY, c.keys[0], enc_set=True)
        set_rx(tab, c, 0, RX_ONLY)
        o = _dev(c.offs.view(np.int64), dev)
        # ---- RX
        conn = rng.choice(np.array([LIVE, slots, 0xffffffff, NEVER, CLEARED, TX_ONLY],
                                   dtype=np.uint32), n)
        r, iv, sq, fl = conn_burst.decode_burst_mc(
            tab, _dev(conn.view(np.int32), dev), _dev(c.rx, dev), o,
            _dev(c.lens.view(np.int32), dev), ivlen=IVLEN)
        r, iv = r.cpu().numpy(), iv.cpu().numpy()
        sq, fl = sq.cpu().numpy().view(np.uint32), fl.cpu().numpy().view(np.uint32)
        live, runt = conn == LIVE, c.lens < 8
        want = np.where(live, c.rx_res, np.where(runt, BAD, NOCONN)).astype(np.uint8)
        assert np.array_equal(r, want), np.nonzero(r != want)[0][:8]
        assert (want == NOCONN).sum() > n // 2 and (runt & ~live).sum() > 0
        # the header of every datagram that has one, whatever its connection
        assert np.array_equal(sq, c.rx_seq) and np.array_equal(fl, c.rx_fl)
        assert np.array_equal(iv[live], c.rx_iv[live]) and not iv[~live].any()
        # ---- TX (the case's slots under the active key: connection 0)
        conn = rng.choice(np.array([LIVE, slots, 0xffffffff, NEVER, CLEARED, RX_ONLY],
                                   dtype=np.uint32), n)
        live = conn == LIVE
        w_res, w_sealed = oracle_mod.packet_encode_batch(
            6, c.keys[0], True, c.seq, c.flags, c.data, c.offs, c.slot,
            nthreads=CPU_THREADS)
        d = _dev(c.data, dev)
        res = conn_burst.encode_burst_mc(
            tab, _dev(conn.view(np.int32), dev), _dev(c.seq.view(np.int32), dev),
            _dev(c.flags.view(np.int32), dev), d, o, _dev(c.slot.view(np.int32), dev))
        res, d = res.cpu().numpy(), d.cpu().numpy()
        assert np.array_equal(res, np.where(live, w_res, NOCONN))
        want_d = c.data.copy()
        for i in np.nonzero(live)[0]:
            a, b = int(c.offs[i]), int(c.offs[i]) + int(c.slot[i])
            want_d[a:b] = w_sealed[a:b]
        assert np.array_equal(d, want_d)
    finally:
        tab.close()


def test_updates_are_stream_ordered(dev, oracle_mod):
    """On one stream, no host synchronisation in between: slot 3 set to key
    A, burst decoded; set to B, decoded; set to A and at once to C, decoded;
    set back to A, decoded.  The bursts were sealed under A: OK, BAD, BAD
    (C won), OK.  The key buffers are overwritten as soon as each call
    returns -- an asynchronous copy from them would read the wrong key."""
    from ilias_net2_amd import _lib, conn_burst
    L = _lib.lib()
    n, hash_alg, hl = 300, 6, 64
    rng = np.random.default_rng(55)
    A, B, C = (rng.integers(0, 256, hl, dtype=np.uint8).tobytes() for _ in range(3))
    lens = rng.choice(np.array([136, 584, 1500], dtype=np.uint32), n)
    offs = np.zeros(n, dtype=np.uint64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    data = rng.integers(0, 256, int(lens.sum()), dtype=np.uint8)
    seq = np.arange(n, dtype=np.uint32)
    flags = np.full(n, 3, dtype=np.uint32)
    _, sealed = oracle_mod.packet_encode_batch(hash_alg, A, True, seq, flags, data, offs,
                                               lens, nthreads=CPU_THREADS)
    d, o = _dev(sealed, dev), _dev(offs.view(np.int64), dev)
    ln = _dev(lens.view(np.int32), dev)
    conn = torch.full((n,), 3, dtype=torch.int32, device=dev)
    ws = conn_burst.burst_workspace(n, dev)
    outs = [torch.full((n,), 9, dtype=torch.uint8, device=dev) for _ in range(4)]
    ivs = [torch.zeros((n, IVLEN), dtype=torch.uint8, device=dev) for _ in range(4)]
    kb = ctypes.create_string_buffer(hl)
    ks = _lib.BurstRxKeys(hash_alg, ctypes.cast(kb, ctypes.c_void_p), hl, 1, None, 0, 0,
                          0, 0)
    st = torch.cuda.current_stream().cuda_stream
    tab = conn_burst.KeyTable(hash_alg, 8)

    def set_key(key):
        kb.raw = key
        assert L.net2_burst_keytab_set_rx(tab.ptr, 3, ctypes.byref(ks), st) == 0
        kb.raw = bytes(hl)                  # the caller reuses its buffer

    def decode(k):
        assert L.net2_packet_decode_burst_mc(
            tab.ptr, conn.data_ptr(), IVLEN, d.data_ptr(), o.data_ptr(), ln.data_ptr(),
            n, outs[k].data_ptr(), ivs[k].data_ptr(), None, None, ws.data_ptr(),
            ws.numel(), st) == 0
    try:
        torch.cuda.synchronize()
        set_key(A)
        decode(0)
        set_key(B)
        decode(1)
        set_key(A)
        set_key(C)
        decode(2)
        set_key(A)
        decode(3)
        torch.cuda.synchronize()
    finally:
        tab.close()
    got = [x.cpu().numpy() for x in outs]
    assert (got[0] == OK).all() and (got[3] == OK).all()
    assert (got[1] == BAD).all() and (got[2] == BAD).all()
    want_iv = oracle_mod.ph_to_iv_batch(seq, flags, IVLEN, nthreads=CPU_THREADS)
    assert np.array_equal(ivs[0].cpu().numpy(), want_iv)
    assert not ivs[1].cpu().numpy().any()


def test_argument_errors(dev):
    from ilias_net2_amd import _lib, conn_burst
    L = _lib.lib()
    n = 4
    t = torch.zeros(4096, dtype=torch.uint8, device=dev)
    p = t.data_ptr()
    wsb = L.net2_packet_burst_workspace(n)
    w = torch.zeros(wsb + 16, dtype=torch.uint8, device=dev)
    key = b"k" * 64
    kb = ctypes.create_string_buffer(key, 64)
    kp = ctypes.cast(kb, ctypes.c_void_p)
    tab = conn_burst.KeyTable(6, 4)
    try:
        T = tab.ptr
        # set_rx: another row, a wrong key length, a wrong alternate key
        # length, a slot past the table, NULL keys
        for ks in (_lib.BurstRxKeys(5, kp, 48, 1, None, 0, 0, 0, 0),
                   _lib.BurstRxKeys(6, kp, 63, 1, None, 0, 0, 0, 0),
                   _lib.BurstRxKeys(6, kp, 64, 1, kp, 63, 0, 0, 0),
                   _lib.BurstRxKeys(6, None, 64, 1, None, 0, 0, 0, 0)):
            assert L.net2_burst_keytab_set_rx(T, 0, ctypes.byref(ks), None) == errno.EINVAL
        good = _lib.BurstRxKeys(6, kp, 64, 1, kp, 64, 0, 0, 0)
        assert L.net2_burst_keytab_set_rx(T, 4, ctypes.byref(good), None) == errno.EINVAL
        assert L.net2_burst_keytab_set_rx(T, 0, None, None) == errno.EINVAL
        assert L.net2_burst_keytab_set_rx(T, 3, ctypes.byref(good), None) == 0
        assert L.net2_burst_keytab_set_tx(T, 0, key, 63, 1, None) == errno.EINVAL
        assert L.net2_burst_keytab_set_tx(T, 4, key, 64, 1, None) == errno.EINVAL
        assert L.net2_burst_keytab_set_tx(T, 0, None, 64, 1, None) == errno.EINVAL
        assert L.net2_burst_keytab_clear(T, 4, None) == errno.EINVAL
        # the bursts: ivlen, a workspace one byte short, a misaligned one,
        # d_seq without d_flags, NULL arrays
        # (the one well-formed call of each kind runs: four empty datagrams,
        # every array a region of its own in t)
        r_cn, r_of, r_le, r_rs, r_iv, r_sq, r_fl = (p + 256 * k for k in range(1, 8))

        def dec(T, conn, ivlen, base, offs, lens, n, res, iv, seq, flags, ws, wsb, st):
            return L.net2_packet_decode_burst_mc(
                T, conn and r_cn, ivlen, base, offs and r_of, lens and r_le, n,
                res and r_rs, iv and r_iv, seq and r_sq, flags and r_fl, ws, wsb, st)

        def enc(T, conn, seq, flags, base, offs, lens, n, res, ws, wsb, st):
            return L.net2_packet_encode_burst_mc(
                T, conn and r_cn, seq and r_sq, flags and r_fl, base, offs and r_of,
                lens and r_le, n, res and r_rs, ws, wsb, st)
        assert dec(T, p, 16, p, p, p, n, p, p, p, p, w.data_ptr(), wsb, None) == 0
        assert dec(T, p, 65, p, p, p, n, p, p, p, p, w.data_ptr(), wsb, None) == errno.EINVAL
        assert dec(T, p, 16, p, p, p, n, p, p, p, p, w.data_ptr(), wsb - 1,
                   None) == errno.EINVAL
        assert dec(T, p, 16, p, p, p, n, p, p, p, p, w.data_ptr() + 8, wsb,
                   None) == errno.EINVAL
        assert dec(T, p, 16, p, p, p, n, p, p, p, None, w.data_ptr(), wsb,
                   None) == errno.EINVAL
        assert dec(T, None, 16, p, p, p, n, p, p, p, p, w.data_ptr(), wsb,
                   None) == errno.EINVAL
        assert enc(T, p, p, p, p, p, p, n, p, w.data_ptr(), wsb, None) == 0
        assert enc(T, p, None, p, p, p, p, n, p, w.data_ptr(), wsb, None) == errno.EINVAL
        assert enc(T, p, p, p, p, p, p, n, p, w.data_ptr(), wsb - 1, None) == errno.EINVAL
        assert enc(T, None, p, p, p, p, p, n, p, w.data_ptr(), wsb, None) == errno.EINVAL
        # an empty burst is a no-op
        assert dec(T, None, 16, None, None, None, 0, None, None, None, None, None, 0,
                   None) == 0
        assert enc(T, None, None, None, None, None, None, 0, None, None, 0, None) == 0
        # a calling thread on another device than the table's
        if torch.cuda.device_count() > 1:
            with torch.cuda.device(1):
                assert dec(T, p, 16, p, p, p, n, p, p, p, p, w.data_ptr(), wsb,
                           None) == errno.EINVAL
                assert L.net2_burst_keytab_clear(T, 0, None) == errno.EINVAL
        torch.cuda.synchronize()
    finally:
        tab.close()
    with pytest.raises(ValueError):
        tab.ptr                                   # closed
