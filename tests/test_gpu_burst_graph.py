"""The burst calls captured into a hipGraph and replayed.

INTEGRATION.md promises that nothing in the device launch paths allocates or
synchronises, so every one of them can be captured; DESIGN.md 5.5.2 that the
by-value key-table update can.  A captured burst is not the launched one seen
again: keys and expanded round keys travel in the launch arguments (the
launcher wipes its own copy when the launch returns), a table update carries
its entry by value, the binned form bakes a launch id into two kernels that
the workspace header is compared with on every replay, and the form is read
from a process-wide setting when the call is made.  So every test here

  1. allocates every input, output and workspace, and prepares workspaces;
  2. runs the call sequence once, uncaptured, on a side stream (the
     launchers' one-time device queries happen outside capture);
  3. refills the in-place buffers and fills every output with a sentinel;
  4. captures the sequence on that one stream, as a linear chain;
  5. overwrites every host key buffer with 0xEE;
  6. replays and compares with the oracle (hash: oracle.packet_*_batch;
     cipher: EVP through tests/aes_ref.py), bit for bit;
  7. copies different bytes of the same geometry into the same device
     buffers, resets the outputs, replays and compares with the answers for
     the new bytes -- nothing of the data was frozen at capture;
  8. where the sequence is idempotent replays once more without touching
     anything -- a replay does not depend on what the previous one left;
  9. destroys the graph before any key or cipher table is closed

(replay_protocol).  The calls go through the C entry points with tensors
allocated beforehand; what a torch wrapper allocates during capture belongs
to the graph's pool and is kept for the graph's life.
"""
import ctypes
import types

import numpy as np
import pytest

import aes_ref
import burst_cases as B
import test_gpu_aes_burst as A
import test_gpu_aes_burst_mc as M
import test_gpu_burst_lattice as LT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CODE, BYTE, STALE = 9, 0xA5, 0x5A5A5A5A     # the outputs' sentinels
WIPED = 0xEE
IVLEN = 16
OK, BAD = 0, 2
vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a GPU (HIP device not visible)")
    from ilias_net2_amd import _lib
    assert _lib.device_count() >= 1
    return torch.device("cuda:0")


@pytest.fixture
def limits():
    """net2_sha2_burst_limits and net2_aes_burst_limits for one test, the
    defaults restored after."""
    from ilias_net2_amd import _lib, cipher_burst
    L = _lib.lib()

    def set_form(form=None, aes_wave_max=None):
        if form is not None:
            assert L.net2_sha2_burst_limits(*LT.FORMS[form]) == 0
        if aes_wave_max is not None:
            cipher_burst.limits(aes_wave_max)
    yield set_form
    L.net2_sha2_burst_limits(-1, -1)
    cipher_burst.limits(-1)


def _dev(a, dev):
    t = torch.from_numpy(np.array(a, order="C")).to(dev)
    assert t.data_ptr() % 16 == 0
    return t


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)


def _host(t):
    return t.cpu().numpy()


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def keybuf(key, keep):
    """A host key buffer the test can overwrite; `keep` collects them."""
    b = ctypes.create_string_buffer(bytes(key), len(key))
    keep.append(b)
    return b


def hash_counts():
    from ilias_net2_amd import conn_burst
    return np.array(conn_burst.burst_stats(), dtype=np.int64)      # lane, wave


def aes_counts():
    from ilias_net2_amd import cipher_burst
    st = cipher_burst.stats()
    return np.array([st["lane_launches"], st["wave_launches"]], dtype=np.int64)


def replay_protocol(dev, calls, fill, check, keys, rounds=3, warm=None, took=None,
                    stream=None):
    """Steps 2 to 9 of the module's protocol.  calls(stream handle) makes the
    sequence's C calls, each asserted to return 0; fill(k) copies input set
    k (0 or 1) into the device buffers and resets every output to its
    sentinel; check(k, r) compares after replay r, which ran on input set k;
    keys: the host key buffers, overwritten after capture; warm: the
    uncaptured first run where it differs from `calls`; took(hash, aes): the
    launch counts by form that capture added; stream: the side stream, where
    the caller needs it as a torch stream."""
    s = torch.cuda.Stream(device=dev) if stream is None else stream
    with torch.cuda.stream(s):
        (warm or calls)(s.cuda_stream)
    torch.cuda.synchronize()
    fill(0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    before = hash_counts(), aes_counts()
    with torch.cuda.graph(g, stream=s):
        calls(s.cuda_stream)
    captured = hash_counts(), aes_counts()
    if took is not None:
        took((captured[0] - before[0]).tolist(), (captured[1] - before[1]).tolist())
    for b in keys:
        ctypes.memset(b, WIPED, len(b))
    for r in range(rounds):
        k = min(r, 1)
        if r < 2:
            fill(k)
            torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        check(k, r)
    # the counters moved at capture, not at replay
    after = hash_counts(), aes_counts()
    assert np.array_equal(after[0], captured[0]) and np.array_equal(after[1], captured[1])
    del g


# ---- single-connection hash bursts --------------------------------------------

def rx_want(oracle_mod, c, keys, rx):
    """packet_decode_batch of received bytes under the key state the graphs
    decode with: the alternate key installed, no cutoff."""
    e = c.expect
    res, iv, seq, fl = oracle_mod.packet_decode_batch(
        e.alg, keys[0], True, IVLEN, rx, c.offs, e.rx_lens, alt_key=keys[1],
        alt_no_cutoff=True, nthreads=1)
    return types.SimpleNamespace(res=res, iv=np.array(iv), seq=seq, fl=fl)


def hash_inputs(oracle_mod, c):
    """The two input sets of a case.  TX: the case's slots, then random bytes
    of the same size, each with the oracle's sealing under the active key.
    RX: the case's received bytes, then the oracle's sealed bytes without the
    case's edits -- or, for a case without edits, the second sealing."""
    e = c.expect
    a = B.answers(oracle_mod, c)
    keys = [B.keys_for(e.alg, 0), B.keys_for(e.alg, 1)]
    tx = [np.array(c.data), np.random.default_rng(len(c.data)).integers(
        0, 256, len(c.data), dtype=np.uint8)]
    tx_want = [oracle_mod.packet_encode_batch(e.alg, keys[0], True, c.seq, c.flags, t,
                                              c.offs, c.lens, nthreads=1) for t in tx]
    rx = [np.array(a.rx), np.array(a.sealed if len(e.flip_pos) else tx_want[1][1])]
    assert not np.array_equal(rx[0], rx[1]) and not np.array_equal(tx[0], tx[1])
    want = [rx_want(oracle_mod, c, keys, r) for r in rx]
    assert np.array_equal(want[0].res, a.rx_res) and np.array_equal(want[0].seq, a.rx_seq)
    assert not np.array_equal(want[0].res, want[1].res) or not len(e.flip_pos)
    return types.SimpleNamespace(keys=keys, tx=tx, tx_want=tx_want, rx=rx, rx_want=want)


def hash_graph(dev, oracle_mod, c, ws, warm_ws=None, rounds=3, took=None):
    """net2_packet_encode_burst of the TX buffer, then
    net2_packet_decode_burst_ck of the RX buffer with an alternate key
    installed, as one graph on workspace `ws`."""
    from ilias_net2_amd import _lib
    L = _lib.lib()
    e = c.expect
    n, alg, hl = e.n, e.alg, B.HL[e.alg]
    inp = hash_inputs(oracle_mod, c)
    keep = []
    kb, ab = keybuf(inp.keys[0], keep), keybuf(inp.keys[1], keep)
    ks = _lib.BurstRxKeys(alg, ctypes.cast(kb, vp), hl, 1, ctypes.cast(ab, vp), hl, 1, 0, 0)
    o = _dev(c.offs.view(np.int64), dev)
    ln, rln = _dev(c.lens.view(np.int32), dev), _dev(e.rx_lens.view(np.int32), dev)
    ds, df = _dev(c.seq.view(np.int32), dev), _dev(c.flags.view(np.int32), dev)
    src_tx, src_rx = [_dev(t, dev) for t in inp.tx], [_dev(r, dev) for r in inp.rx]
    d_tx, d_rx = torch.empty_like(src_tx[0]), torch.empty_like(src_rx[0])
    tres = torch.empty((n,), dtype=torch.uint8, device=dev)
    rres = torch.empty((n,), dtype=torch.uint8, device=dev)
    iv = torch.empty((n, IVLEN), dtype=torch.uint8, device=dev)
    oseq = torch.empty((n,), dtype=torch.int32, device=dev)
    ofl = torch.empty((n,), dtype=torch.int32, device=dev)

    def calls_on(w):
        def calls(st):
            assert L.net2_packet_encode_burst(
                alg, kb, hl, 1, ds.data_ptr(), df.data_ptr(), d_tx.data_ptr(),
                o.data_ptr(), ln.data_ptr(), n, tres.data_ptr(), w.data_ptr(), w.numel(),
                st) == 0
            assert L.net2_packet_decode_burst_ck(
                ctypes.byref(ks), IVLEN, d_rx.data_ptr(), o.data_ptr(), rln.data_ptr(), n,
                rres.data_ptr(), iv.data_ptr(), oseq.data_ptr(), ofl.data_ptr(),
                w.data_ptr(), w.numel(), st) == 0
        return calls

    def fill(k):
        d_tx.copy_(src_tx[k])
        d_rx.copy_(src_rx[k])
        tres.fill_(CODE)
        rres.fill_(CODE)
        iv.fill_(BYTE)
        oseq.fill_(STALE)
        ofl.fill_(STALE)

    stats = []

    def check(k, r):
        tag = (e.name, k, r)
        want_res, sealed = inp.tx_want[k]
        assert np.array_equal(_host(tres), want_res), tag
        assert np.array_equal(_host(d_tx), sealed), tag
        w = inp.rx_want[k]
        assert np.array_equal(_host(rres), w.res), (tag, np.nonzero(_host(rres) != w.res)[0][:8])
        assert np.array_equal(_u32(oseq), w.seq) and np.array_equal(_u32(ofl), w.fl), tag
        ok = w.res == OK
        got = _host(iv)
        assert np.array_equal(got[ok], w.iv[ok]) and (got[~ok] == BYTE).all(), tag
        assert np.array_equal(_host(d_rx), inp.rx[k]), tag      # RX reads only
        stats.append(_lib.workspace_stats(ws.data_ptr(), ws.numel()))

    replay_protocol(dev, calls_on(ws), fill, check, keep, rounds=rounds,
                    warm=None if warm_ws is None else calls_on(warm_ws), took=took)
    assert bytes(kb) == bytes([WIPED]) * hl
    return stats


@pytest.mark.parametrize("form", list(LT.FORMS))
@pytest.mark.parametrize("alg", B.ALGS)
def test_hash_bursts(dev, oracle_mod, limits, alg, form):
    """Seal and verify in one graph, in each form: the burst that is uniform
    only once binned, and every field bit flipped under both keys of a
    rollover.  The form is the one the limits chose at capture; in the binned
    form every replayed launch bins -- the ids baked in at capture pass the
    header check again and again."""
    from ilias_net2_amd import _lib
    L = _lib.lib()
    limits(form)
    for c in (B.L4(alg), B.B1(alg, 8, 100, altkey=True)):
        ws = LT.workspace(L, c.expect.n, dev)
        forms = []
        before = _lib.workspace_stats(ws.data_ptr(), ws.numel())
        stats = hash_graph(dev, oracle_mod, c, ws, took=lambda h, a: forms.append((h, a)))
        assert forms == [([0, 2] if form == "wave" else [2, 0], [0, 0])], forms
        # the warm-up's two launches, then two per replay
        want = before["binned"] + 2 if form == "binned" else 0
        for st in stats:
            want += 2 if form == "binned" else 0
            assert st["binned"] == want, (c.expect.name, stats)
            for f in ("aborts", "mismatches", "unprepared"):
                assert st[f] == before[f], (c.expect.name, f, stats)


@pytest.mark.parametrize("alg", [4, 6])
def test_unprepared_workspace(dev, oracle_mod, limits, alg):
    """The binned form on a workspace that nothing prepared (0x3C in every
    byte), captured after a warm-up on another workspace: every replay is the
    oracle's.  (The launch that finds the header unprepared initialises it
    and takes submission order, on every replay: results only.)"""
    from ilias_net2_amd import _lib
    L = _lib.lib()
    limits("binned")
    c = B.L4(alg)
    n = c.expect.n
    ws = torch.full((L.net2_packet_burst_workspace(n),), 0x3C, dtype=torch.uint8,
                    device=dev)
    hash_graph(dev, oracle_mod, c, ws, warm_ws=LT.workspace(L, n, dev))


# ---- many connections, the table updated inside the graph ---------------------

@pytest.mark.parametrize("form", ["lane", "wave"])
@pytest.mark.parametrize("alg", [4, 6])
def test_many_connections_with_updates(dev, oracle_mod, limits, alg, form):
    """set_rx / set_tx of slot 0 (key A), encode_burst_mc, decode_burst_mc,
    set_rx of slot 0 (key B), decode_burst_mc of the same bytes: the first
    decode sees key A on every replay, the second key B -- connection 0's
    datagrams turn BAD.  An update that did not replay, or that read the host
    key when replayed, fails here."""
    from ilias_net2_amd import _lib, conn_burst
    L = _lib.lib()
    limits(form)
    K = 3
    hl = B.HL[alg]
    c = B.B1(alg, 4, 100)
    e = c.expect
    n = e.n
    a = B.answers(oracle_mod, c, nconn=K)
    key_a, key_b = a.keys[0], B.keys_for(alg, 9)

    def decode1(rx, key0=key_a):
        """The oracle's decode, connection k under its key, connection 0
        under key0."""
        res = np.full(n, 9, dtype=np.uint8)
        iv = np.zeros((n, IVLEN), dtype=np.uint8)
        seq, fl = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        for k in range(K):
            idx = np.nonzero(a.group == k)[0]
            res[idx], iv[idx], seq[idx], fl[idx] = oracle_mod.packet_decode_batch(
                alg, a.keys[k] if k else key0, True, IVLEN, rx, c.offs[idx],
                e.rx_lens[idx], nthreads=1)
        return res, iv, seq, fl

    def decode2(rx):
        """Outputs 2: key B for connection 0's datagrams."""
        return decode1(rx, key_b)

    # input set 1: random slots; what TX seals of them is what RX receives
    tx = [np.array(c.data), np.random.default_rng(77 + alg).integers(
        0, 256, len(c.data), dtype=np.uint8)]
    sealed1 = tx[1].copy()
    for k in range(K):
        idx = np.nonzero(a.group == k)[0]
        r, sealed1 = oracle_mod.packet_encode_batch(alg, a.keys[k], True, c.seq[idx],
                                                    c.flags[idx], sealed1, c.offs[idx],
                                                    c.lens[idx], nthreads=1)
        assert np.array_equal(r, a.tx_res[idx])
    tx_want = [np.array(a.sealed), sealed1]
    rx = [a.rx, sealed1]
    out1 = [decode1(r) for r in rx]
    out2 = [decode2(r) for r in rx]
    for got, want in zip(out1[0], (a.rx_res, a.rx_iv, a.rx_seq, a.rx_fl)):
        assert np.array_equal(got, want)        # B.answers(..., nconn=3)
    for k in range(2):
        turned = (out1[k][0] == OK) & (out2[k][0] == BAD)
        assert turned.sum() > 20 and (a.group[turned] == 0).all()
        other = a.group != 0
        assert np.array_equal(out1[k][0][other], out2[k][0][other])

    keep = []
    kb = [keybuf(a.keys[k], keep) for k in range(K)]
    bb = keybuf(key_b, keep)

    def rxkeys(b):
        return _lib.BurstRxKeys(alg, ctypes.cast(b, vp), hl, 1, None, 0, 0, 0, 0)

    conn = _dev((np.arange(n) % K).astype(np.int32), dev)
    o = _dev(c.offs.view(np.int64), dev)
    ln, rln = _dev(c.lens.view(np.int32), dev), _dev(e.rx_lens.view(np.int32), dev)
    ds, df = _dev(c.seq.view(np.int32), dev), _dev(c.flags.view(np.int32), dev)
    src_tx, src_rx = [_dev(t, dev) for t in tx], [_dev(r, dev) for r in rx]
    d_tx, d_rx = torch.empty_like(src_tx[0]), torch.empty_like(src_rx[0])
    ws = LT.workspace(L, n, dev)
    tres = torch.empty((n,), dtype=torch.uint8, device=dev)
    outs = [types.SimpleNamespace(
        res=torch.empty((n,), dtype=torch.uint8, device=dev),
        iv=torch.empty((n, IVLEN), dtype=torch.uint8, device=dev),
        seq=torch.empty((n,), dtype=torch.int32, device=dev),
        fl=torch.empty((n,), dtype=torch.int32, device=dev)) for _ in range(2)]

    with conn_burst.KeyTable(alg, K) as tab:
        for k in (1, 2):
            tab.set_rx(k, a.keys[k], enc_set=True)
            tab.set_tx(k, a.keys[k], enc_set=True)
        torch.cuda.synchronize()

        def decode(st, w):
            assert L.net2_packet_decode_burst_mc(
                tab.ptr, conn.data_ptr(), IVLEN, d_rx.data_ptr(), o.data_ptr(),
                rln.data_ptr(), n, w.res.data_ptr(), w.iv.data_ptr(), w.seq.data_ptr(),
                w.fl.data_ptr(), ws.data_ptr(), ws.numel(), st) == 0

        def calls(st):
            ka, kbb = rxkeys(kb[0]), rxkeys(bb)
            assert L.net2_burst_keytab_set_rx(tab.ptr, 0, ctypes.byref(ka), st) == 0
            assert L.net2_burst_keytab_set_tx(tab.ptr, 0, kb[0], hl, 1, st) == 0
            assert L.net2_packet_encode_burst_mc(
                tab.ptr, conn.data_ptr(), ds.data_ptr(), df.data_ptr(), d_tx.data_ptr(),
                o.data_ptr(), ln.data_ptr(), n, tres.data_ptr(), ws.data_ptr(), ws.numel(),
                st) == 0
            decode(st, outs[0])
            assert L.net2_burst_keytab_set_rx(tab.ptr, 0, ctypes.byref(kbb), st) == 0
            decode(st, outs[1])

        def fill(k):
            d_tx.copy_(src_tx[k])
            d_rx.copy_(src_rx[k])
            tres.fill_(CODE)
            for w in outs:
                w.res.fill_(CODE)
                w.iv.fill_(BYTE)
                w.seq.fill_(STALE)
                w.fl.fill_(STALE)

        def check(k, r):
            tag = (e.name, k, r)
            assert np.array_equal(_host(tres), a.tx_res), tag
            assert np.array_equal(_host(d_tx), tx_want[k]), tag
            for j, (w, want) in enumerate(zip(outs, (out1[k], out2[k]))):
                res, iv, seq, fl = want
                got = _host(w.res)
                assert np.array_equal(got, res), (tag, j, np.nonzero(got != res)[0][:8])
                assert np.array_equal(_u32(w.seq), seq), (tag, j)
                assert np.array_equal(_u32(w.fl), fl), (tag, j)
                ok = res == OK
                got = _host(w.iv)
                assert np.array_equal(got[ok], iv[ok]), (tag, j)
                assert (got[~ok] == BYTE).all(), (tag, j)

        forms = []
        replay_protocol(dev, calls, fill, check, keep,
                        took=lambda h, x: forms.append((h, x)))
        assert forms == [([0, 3] if form == "wave" else [3, 0], [0, 0])], forms


# ---- cipher bursts ---------------------------------------------------------------

AES_FORMS = {"lane": 0, "wave": -1}     # net2_aes_burst_limits' wave_max
NOCONN = 5


def evp_rx(c, po, data, key_of, noconn=None):
    """What EVP makes of every datagram of a received burst in `data` under
    key_of[i]: codes, plaintext lengths, plaintexts, and the bytes of the
    output that a decrypted datagram may write (its payload)."""
    res = np.array(c.res_in)
    plen = np.zeros(c.n, dtype=np.uint32)
    plains = [None] * c.n
    written = np.zeros(c.total, dtype=bool)
    for i in range(c.n):
        if c.res_in[i] != OK or not c.flags[i] & A.ENC:
            continue
        if noconn is not None and noconn[i]:
            res[i] = NOCONN
            continue
        a, b = int(c.offs[i]) + int(po[i]), int(c.offs[i]) + int(c.lens[i])
        got = aes_ref.decrypt(key_of[i], c.iv[i].tobytes(), data[a:max(a, b)].tobytes())
        if got is None:
            res[i] = BAD
            continue
        plen[i], plains[i] = len(got), got
        written[a:b] = True
    return types.SimpleNamespace(res=res, plen=plen, plains=plains, written=written)


def fresh_rx(c, po, key_of, want, seed):
    """Input set 1 of a received burst: every datagram that decrypts holds the
    EVP ciphertext of other plaintext bytes of the same length, in its slot."""
    rng = np.random.default_rng(seed)
    data = np.array(c.data)
    for i in np.nonzero([p is not None for p in want.plains])[0]:
        plain = rng.integers(0, 256, int(want.plen[i]), dtype=np.uint8).tobytes()
        ct = aes_ref.encrypt(key_of[i], c.iv[i].tobytes(), plain)
        a = int(c.offs[i]) + int(po[i])
        assert a + len(ct) == int(c.offs[i]) + int(c.lens[i])
        data[a:a + len(ct)] = np.frombuffer(ct, dtype=np.uint8)
    assert not np.array_equal(data, c.data)
    return data


def check_cipher_rx(tag, c, po, want, res, plen, out):
    """Every code, length and plaintext byte; nothing outside the decrypted
    payloads is written."""
    bad = np.nonzero(res != want.res)[0]
    assert len(bad) == 0, (tag, [(int(i), int(res[i]), int(want.res[i])) for i in bad[:8]])
    bad = np.nonzero(plen != want.plen)[0]
    assert len(bad) == 0, (tag, [(int(i), hex(plen[i]), int(want.plen[i])) for i in bad[:8]])
    for i in range(c.n):
        if want.plains[i] is not None:
            a = int(c.offs[i]) + int(po[i])
            assert out[a:a + int(plen[i])].tobytes() == want.plains[i], (tag, i)
    assert (out[~want.written] == BYTE).all(), tag


@pytest.mark.parametrize("form", list(AES_FORMS))
def test_cipher_rx(dev, oracle_mod, limits, form):
    """net2_packet_decrypt_burst out of place under row 6 with an alternate
    key (n = 333: ragged, bad padding, empty, incoming BAD), in the lane and
    the wave form."""
    from ilias_net2_amd import _lib
    L = _lib.lib()
    limits(aes_wave_max=AES_FORMS[form])
    c = A.rx_case(oracle_mod, 6)
    n, hl = c.n, c.hl
    po = np.where((c.flags & A.SIGNED) != 0, 8 + hl, 8).astype(np.int64)
    picks = [A.P.ref_rx_key(int(c.seq[i]), int(c.flags[i]), True, c.no_cutoff, c.cutoff,
                            c.rx_start) for i in range(n)]
    key_of = [c.alt_key if p else c.key for p in picks]
    want0 = evp_rx(c, po, c.data, key_of)
    assert np.array_equal(want0.res, c.want_res) and np.array_equal(want0.plen, c.want_plen)
    assert np.array_equal(want0.written, c.written)
    data = [np.array(c.data), fresh_rx(c, po, key_of, want0, 6001)]
    want = [want0, evp_rx(c, po, data[1], key_of)]
    assert np.array_equal(want[1].res, want0.res) and want[1].plains != want0.plains

    keep = []
    kb, ab, hb = keybuf(c.key, keep), keybuf(c.alt_key, keep), keybuf(bytes(64), keep)
    ck = _lib.BurstCipherKeys(_lib.ENC_AES256, ctypes.cast(kb, vp), 32,
                              ctypes.cast(ab, vp), 32)
    rk = _lib.BurstRxKeys(6, ctypes.cast(hb, vp), 64, 1, ctypes.cast(hb, vp), 64,
                          int(c.no_cutoff), c.cutoff, c.rx_start)
    src = [_dev(x, dev) for x in data]
    d = torch.empty_like(src[0])
    out = torch.empty((c.total,), dtype=torch.uint8, device=dev)
    o, ln = _dev(c.offs.astype(np.int64), dev), _dev(_i32(c.lens), dev)
    sq, fl, iv = _dev(_i32(c.seq), dev), _dev(_i32(c.flags), dev), _dev(c.iv, dev)
    res_in = _dev(c.res_in, dev)
    res = torch.empty_like(res_in)
    plen = torch.empty((n,), dtype=torch.int32, device=dev)

    def calls(st):
        assert L.net2_packet_decrypt_burst(
            ctypes.byref(rk), ctypes.byref(ck), d.data_ptr(), o.data_ptr(), ln.data_ptr(),
            n, sq.data_ptr(), fl.data_ptr(), iv.data_ptr(), res.data_ptr(), out.data_ptr(),
            plen.data_ptr(), st) == 0

    def fill(k):
        d.copy_(src[k])
        res.copy_(res_in)
        out.fill_(BYTE)
        plen.fill_(STALE)

    def check(k, r):
        check_cipher_rx((form, k, r), c, po, want[k], _host(res), _u32(plen), _host(out))
        assert np.array_equal(_host(d), data[k])

    forms = []
    replay_protocol(dev, calls, fill, check, keep, took=lambda h, x: forms.append((h, x)))
    assert forms == [([0, 0], [0, 1] if form == "wave" else [1, 0])], forms


def test_cipher_tx(dev, limits):
    """net2_packet_encrypt_burst in place (n = 333: exact room, a byte short,
    room to spare); the second replay on other plaintext bytes."""
    from ilias_net2_amd import _lib
    L = _lib.lib()
    c = A.tx_case(6)
    n = c.n
    po = np.where((c.flags & A.SIGNED) != 0, 8 + c.hl, 8).astype(np.int64)
    data = [np.array(c.data), np.random.default_rng(6002).integers(
        0, 256, len(c.data), dtype=np.uint8)]
    want = [np.array(c.want), data[1].copy()]
    for i in np.nonzero(((c.flags & A.ENC) != 0) & (c.want_res == OK))[0]:
        a = int(c.offs[i]) + int(po[i])
        ct = aes_ref.encrypt(c.key, c.iv[i].tobytes(),
                             data[1][a:a + int(c.plen[i])].tobytes())
        assert int(po[i]) + len(ct) == c.want_wire[i]
        want[1][a:a + len(ct)] = np.frombuffer(ct, dtype=np.uint8)
    keep = []
    kb = keybuf(c.key, keep)
    ck = _lib.BurstCipherKeys(_lib.ENC_AES256, ctypes.cast(kb, vp), 32, None, 0)
    src = [_dev(x, dev) for x in data]
    d = torch.empty_like(src[0])
    o, ln = _dev(c.offs.astype(np.int64), dev), _dev(_i32(c.lens), dev)
    fl, iv, pl = _dev(_i32(c.flags), dev), _dev(c.iv, dev), _dev(_i32(c.plen), dev)
    res = torch.empty((n,), dtype=torch.uint8, device=dev)
    wire = torch.empty((n,), dtype=torch.int32, device=dev)

    def calls(st):
        assert L.net2_packet_encrypt_burst(
            ctypes.byref(ck), c.hl, fl.data_ptr(), iv.data_ptr(), d.data_ptr(),
            o.data_ptr(), ln.data_ptr(), pl.data_ptr(), n, res.data_ptr(),
            wire.data_ptr(), st) == 0

    def fill(k):
        d.copy_(src[k])
        res.fill_(CODE)
        wire.fill_(STALE)

    def check(k, r):
        assert np.array_equal(_host(res), c.want_res), (k, r)
        assert np.array_equal(_u32(wire), c.want_wire), (k, r)
        bad = np.nonzero(_host(d) != want[k])[0]
        assert len(bad) == 0, (k, r, bad[:8])

    # encrypting in place is not idempotent: two replays, each on fresh input
    replay_protocol(dev, calls, fill, check, keep, rounds=2)


# ---- the cipher over many connections ---------------------------------------------

@pytest.mark.parametrize("form", list(AES_FORMS))
def test_cipher_many_connections_with_updates(dev, limits, form):
    """CipherTable.set_rx of connection 0's slot with its key, decrypt_burst_mc,
    set_rx of that slot with another key, decrypt_burst_mc of the same bytes
    (n = 513 over 5 connections, row 6): on every replay the first decrypt is
    under the connection's key and the second under the other one, where EVP
    refuses nearly all of connection 0's datagrams."""
    from ilias_net2_amd import _lib
    L = _lib.lib()
    limits(aes_wave_max=AES_FORMS[form])
    n, K, hash_alg = 513, 5, 6
    c = M.rx_case(n, K, hash_alg)
    k0 = c.conns[0]
    assert k0.alt_key is None
    key_b = bytes(range(100, 132))
    noconn = c.kind == 4
    key_a_of = [c.conns[k].alt_key if c.picks[i] else c.conns[k].key
                for i, k in enumerate(c.c_of)]
    on0 = (c.c_of == 0) & ~noconn
    key_b_of = [key_b if on0[i] else key_a_of[i] for i in range(n)]
    want0 = evp_rx(c, c.po, c.data, key_a_of, noconn)
    assert np.array_equal(want0.res, c.want_res) and np.array_equal(want0.plen, c.want_plen)
    assert np.array_equal(want0.written, c.written)
    data = [np.array(c.data), fresh_rx(c, c.po, key_a_of, want0, 6003)]
    want1 = [want0, evp_rx(c, c.po, data[1], key_a_of, noconn)]
    want2 = [evp_rx(c, c.po, x, key_b_of, noconn) for x in data]
    for k in range(2):
        turned = (want1[k].res == OK) & (want2[k].res == BAD)
        assert turned.sum() > 20 and on0[turned].all()
        assert np.array_equal(want1[k].res[~on0], want2[k].res[~on0])

    keep = []
    ka, kbb = keybuf(k0.key, keep), keybuf(key_b, keep)
    cka = _lib.BurstCipherKeys(_lib.ENC_AES256, ctypes.cast(ka, vp), 32, None, 0)
    ckb = _lib.BurstCipherKeys(_lib.ENC_AES256, ctypes.cast(kbb, vp), 32, None, 0)
    rk = _lib.BurstRxKeys(hash_alg, None, 0, _lib.ENC_AES256, None, 0, 0, 0, 0)
    src = [_dev(x, dev) for x in data]
    d = torch.empty_like(src[0])
    o, ln = _dev(c.offs.astype(np.int64), dev), _dev(_i32(c.lens), dev)
    sq, fl, iv = _dev(_i32(c.seq), dev), _dev(_i32(c.flags), dev), _dev(c.iv, dev)
    cn, res_in = _dev(_i32(c.conn), dev), _dev(c.res_in, dev)
    outs = [types.SimpleNamespace(
        res=torch.empty_like(res_in),
        out=torch.empty((c.total,), dtype=torch.uint8, device=dev),
        plen=torch.empty((n,), dtype=torch.int32, device=dev)) for _ in range(2)]

    with M._table(c, hash_alg, tx=False) as tab:
        torch.cuda.synchronize()

        def decrypt(st, w):
            assert L.net2_packet_decrypt_burst_mc(
                tab.ptr, cn.data_ptr(), c.hl, d.data_ptr(), o.data_ptr(), ln.data_ptr(), n,
                sq.data_ptr(), fl.data_ptr(), iv.data_ptr(), w.res.data_ptr(),
                w.out.data_ptr(), w.plen.data_ptr(), st) == 0

        def calls(st):
            assert L.net2_burst_ciphertab_set_rx(tab.ptr, k0.slot, ctypes.byref(rk),
                                                 ctypes.byref(cka), st) == 0
            decrypt(st, outs[0])
            assert L.net2_burst_ciphertab_set_rx(tab.ptr, k0.slot, ctypes.byref(rk),
                                                 ctypes.byref(ckb), st) == 0
            decrypt(st, outs[1])

        def fill(k):
            d.copy_(src[k])
            for w in outs:
                w.res.copy_(res_in)
                w.out.fill_(BYTE)
                w.plen.fill_(STALE)

        def check(k, r):
            for j, (w, want) in enumerate(zip(outs, (want1[k], want2[k]))):
                check_cipher_rx((form, k, r, j), c, c.po, want, _host(w.res), _u32(w.plen),
                                _host(w.out))

        forms = []
        replay_protocol(dev, calls, fill, check, keep,
                        took=lambda h, x: forms.append((h, x)))
        assert forms == [([0, 0], [0, 2] if form == "wave" else [2, 0])], forms


def test_cipher_tx_many_connections(dev, limits):
    """CipherTable.set_tx of one slot, then encrypt_burst_mc in place (n = 513
    over 5 connections): the slot's key is the captured one on both replays,
    whatever the table held before."""
    from ilias_net2_amd import _lib
    L = _lib.lib()
    n, K, hash_alg = 513, 5, 6
    c = M.tx_case(n, K, hash_alg)
    k0 = c.conns[0]
    po = np.where((c.flags & A.SIGNED) != 0, 8 + c.hl, 8).astype(np.int64)
    data = [np.array(c.data), np.random.default_rng(6004).integers(
        0, 256, len(c.data), dtype=np.uint8)]
    want = [np.array(c.want), data[1].copy()]
    done = ((c.flags & A.ENC) != 0) & (c.want_res == OK)
    assert (done & (c.c_of == 0)).sum() > 20
    for i in np.nonzero(done)[0]:
        a = int(c.offs[i]) + int(po[i])
        ct = aes_ref.encrypt(c.conns[c.c_of[i]].tx_key, c.iv[i].tobytes(),
                             data[1][a:a + int(c.plen[i])].tobytes())
        want[1][a:a + len(ct)] = np.frombuffer(ct, dtype=np.uint8)
    keep = []
    kb = keybuf(k0.tx_key, keep)
    ck = _lib.BurstCipherKeys(_lib.ENC_AES256, ctypes.cast(kb, vp), 32, None, 0)
    src = [_dev(x, dev) for x in data]
    d = torch.empty_like(src[0])
    o, ln = _dev(c.offs.astype(np.int64), dev), _dev(_i32(c.lens), dev)
    fl, iv, pl = _dev(_i32(c.flags), dev), _dev(c.iv, dev), _dev(_i32(c.plen), dev)
    cn = _dev(_i32(c.conn), dev)
    res = torch.empty((n,), dtype=torch.uint8, device=dev)
    wire = torch.empty((n,), dtype=torch.int32, device=dev)

    with M._table(c, hash_alg, rx=False) as tab:
        # before the graph runs the slot holds another key
        tab.set_tx(k0.slot, bytes(range(50, 82)))
        torch.cuda.synchronize()

        def calls(st):
            assert L.net2_burst_ciphertab_set_tx(tab.ptr, k0.slot, ctypes.byref(ck), st) == 0
            assert L.net2_packet_encrypt_burst_mc(
                tab.ptr, cn.data_ptr(), c.hl, fl.data_ptr(), iv.data_ptr(), d.data_ptr(),
                o.data_ptr(), ln.data_ptr(), pl.data_ptr(), n, res.data_ptr(),
                wire.data_ptr(), st) == 0

        def fill(k):
            d.copy_(src[k])
            res.fill_(CODE)
            wire.fill_(STALE)

        def check(k, r):
            assert np.array_equal(_host(res), c.want_res), (k, r)
            got = _u32(wire)
            assert np.array_equal(got[c.stated], c.want_wire[c.stated]), (k, r)
            bad = np.nonzero(_host(d) != want[k])[0]
            assert len(bad) == 0, (k, r, bad[:8])

        replay_protocol(dev, calls, fill, check, keep, rounds=2)


# ---- the whole chain as one graph ------------------------------------------------

@pytest.mark.parametrize("no_cutoff", [False, True])
def test_chain_as_one_graph(dev, oracle_mod, no_cutoff):
    """The body of test_gpu_aes_burst's one-stream chain -- IVs, encrypt and
    seal per key set, the tamper step, verify, decrypt -- captured as one
    graph and held to the same checks; the second replay starts from other
    plaintext.  The tensors the body allocates belong to the graph's pool:
    its outputs are read there after every replay."""
    cases = [A.chain_case(no_cutoff), A.chain_case(no_cutoff, fresh=True)]
    assert not np.array_equal(cases[0].data, cases[1].data)
    assert np.array_equal(cases[0].offs, cases[1].offs)
    t = A.chain_device(dev, cases[0])
    src = [_dev(c.data, dev) for c in cases]
    s = torch.cuda.Stream(device=dev)
    outs, keep = [], []     # the warm-up's outputs, then the captured run's

    def calls(st):
        assert st == s.cuda_stream
        outs.append(A.chain_body(dev, cases[0], t, s))
        keep.extend(outs[-1].keys)

    def fill(k):
        t.d.copy_(src[k])

    def check(k, r):
        A.chain_check(oracle_mod, cases[k], outs[-1])

    forms = []
    # tampering in place is not idempotent: two replays, each on fresh input
    replay_protocol(dev, calls, fill, check, keep, rounds=2, stream=s,
                    took=lambda h, x: forms.append((sum(h), sum(x))))
    assert forms == [(3, 1)], forms
