"""Bulk updates of the two device tables (net2_burst_keytab_update,
net2_burst_ciphertab_update) and the fingerprints they are compared through.

The yardstick is pinned first: the fingerprints of a table filled by the
per-slot calls are the SHA-256 (hashlib) of entries restated in plain Python
(tests/tab_ref.py, itself checked against hashlib, hmac and FIPS 197 without a
GPU).  After that a bulk-updated table is compared, byte for byte through its
fingerprints, with a twin that got the same ops through the per-slot calls, and
the bursts are run over bulk-filled tables against the oracle and EVP.

Tables have 300 slots (not a multiple of the 64 lanes of a wave, more than one
256-lane workgroup).
"""
import ctypes
import errno
import hashlib
import threading

import numpy as np
import pytest

import tab_ref
import test_gpu_aes_burst_mc as A
import test_gpu_burst_mc as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SLOTS = 300
HL = {4: 32, 5: 48, 6: 64}
KINDS = [4, 5, 6, "aes"]
OK, BAD, NOCONN = 0, 2, 5
vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a GPU (HIP device not visible)")
    from ilias_net2_amd import _lib
    assert _lib.device_count() >= 1
    return torch.device("cuda:0")


@pytest.fixture
def per_launch():
    """net2_burst_tab_limits for one test, the default restored after."""
    from ilias_net2_amd import conn_burst
    yield conn_burst.tab_limits
    conn_burst.tab_limits(-1)


def table(kind, slots=SLOTS):
    from ilias_net2_amd import cipher_burst, conn_burst
    return (cipher_burst.CipherTable(slots) if kind == "aes"
            else conn_burst.KeyTable(kind, slots))


def rand_ops(kind, rng, n, slots):
    """n random ops (conn_burst / cipher_burst op tuples) on `slots` (an
    array to draw from): every key variant, CLEAR the rarer op."""
    from ilias_net2_amd import cipher_burst, conn_burst
    mod = cipher_burst if kind == "aes" else conn_burst
    kl = 32 if kind == "aes" else HL[kind]
    key = lambda: rng.integers(0, 256, kl, dtype=np.uint8).tobytes()  # noqa: E731
    ops = []
    for i in range(n):
        slot = int(slots[i])
        pick = int(rng.integers(0, 8))
        alt = bool(rng.integers(0, 2))
        state = dict(alt_key=key() if alt else None,
                     alt_no_cutoff=bool(rng.integers(0, 2)),
                     alt_cutoff=int(rng.integers(0, 2**32)),
                     rx_start=int(rng.integers(0, 2**32)))
        enc = bool(rng.integers(0, 2))
        if pick == 0:
            ops.append(mod.clear_op(slot))
        elif pick < 5 and kind == "aes":
            ops.append(mod.rx_op(slot, key(), hash_alg=6 if alt else 0, **state))
        elif pick < 5:
            ops.append(mod.rx_op(slot, key(), enc_set=enc, **state))
        elif kind == "aes":
            ops.append(mod.tx_op(slot, key()))
        else:
            ops.append(mod.tx_op(slot, key(), enc_set=enc))
    return ops


def per_slot(tab, ops, stream=None):
    """The ops through the per-slot calls, in order."""
    for kind, slot, kw in ops:
        getattr(tab, ("clear", "set_rx", "set_tx")[kind])(slot, stream=stream, **kw)


def prints(tab, stream=None):
    fp = tab.fingerprints(stream=stream)
    torch.cuda.synchronize()
    return fp.cpu().numpy()


def same(a, b):
    bad = np.nonzero((a != b).any(axis=1))[0]
    assert len(bad) == 0, ("slots that differ", bad[:16].tolist())


# ---- 1. the yardstick ------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_fingerprint_baseline(dev, kind):
    """Per-slot calls, then fingerprint == hashlib.sha256 of the restated
    entries: set and unset slots, both sides, alternate keys, a CLEAR."""
    rng = np.random.default_rng(100 + (7 if kind == "aes" else kind))
    slots = np.concatenate(([0, 299, 64, 255, 256], rng.integers(0, SLOTS, 35)))
    ops = rand_ops(kind, rng, len(slots), slots)
    ents = [tab_ref.CipherEntry() if kind == "aes" else tab_ref.KeyEntry(kind)
            for _ in range(SLOTS)]
    tab_ref.apply_ops(ents, ops)
    want = np.array([np.frombuffer(hashlib.sha256(e.bytes()).digest(), dtype=np.uint8)
                     for e in ents])
    with table(kind) as tab:
        per_slot(tab, ops)
        got = prints(tab)
        # a sub-range lands at the start of the output
        from ilias_net2_amd import _lib
        part = torch.zeros((3, 32), dtype=torch.uint8, device=dev)
        fn = (_lib.lib().net2_burst_ciphertab_fingerprint if kind == "aes"
              else _lib.lib().net2_burst_keytab_fingerprint)
        _lib.check(fn(tab.ptr, 297, 3, part.data_ptr(),
                      torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
    same(got, want)
    assert np.array_equal(part.cpu().numpy(), want[297:])
    assert len({w.tobytes() for w in want}) > 20     # (the slots do differ)


# ---- 2. bulk equals per-slot -------------------------------------------------------

@pytest.mark.parametrize("per", [None, 64])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257])
@pytest.mark.parametrize("kind", KINDS)
def test_bulk_equals_per_slot(dev, per_launch, kind, n, per):
    from ilias_net2_amd import conn_burst
    rng = np.random.default_rng(1000 * n + (7 if kind == "aes" else kind))
    slots = rng.integers(0, SLOTS, n)
    slots[0] = 299
    if n > 1:
        slots[-1] = 0
    # something there before, so that "the other side stays" is looked at
    pre = rand_ops(kind, rng, 40, np.concatenate(([0, 299], rng.integers(0, SLOTS, 38))))
    ops = rand_ops(kind, rng, n, slots)
    if per is not None:
        per_launch(per)
    with table(kind) as bulk, table(kind) as twin:
        per_slot(bulk, pre)
        per_slot(twin, pre)
        s0, b0 = conn_burst.tab_stats()
        bulk.update(ops)
        s1, b1 = conn_burst.tab_stats()
        per_slot(twin, ops)
        s2, b2 = conn_burst.tab_stats()
        same(prints(bulk), prints(twin))
    assert (s1 - s0, b1 - b0) == (0, -(-n // (per or 65536)))
    assert (s2 - s1, b2 - b1) == (n, 0)
    if (n, per) == (257, 64):
        assert b1 - b0 == 5


@pytest.mark.parametrize("per", [None, 7])
@pytest.mark.parametrize("kind", KINDS)
def test_every_order_on_one_slot(dev, per_launch, kind, per):
    """200 ops over 16 slots, slots 0 and 299 among them: RX, TX and CLEAR of
    one slot in every order, many times over."""
    rng = np.random.default_rng(77 + (7 if kind == "aes" else kind))
    pool = np.concatenate(([0, 299], rng.choice(np.arange(1, 299), 14, replace=False)))
    ops = rand_ops(kind, rng, 200, pool[rng.integers(0, 16, 200)])
    kinds_on = {}
    for k, slot, _ in ops:
        kinds_on.setdefault(slot, []).append(k)
    orders = {tuple(v[i:i + 2]) for v in kinds_on.values() for i in range(len(v) - 1)}
    assert len(orders) == 9 and set(kinds_on) >= {0, 299}     # every pair, in order
    if per is not None:
        per_launch(per)
    with table(kind) as bulk, table(kind) as twin:
        bulk.update(ops)
        per_slot(twin, ops)
        same(prints(bulk), prints(twin))


# ---- 3. the bursts over bulk-filled tables ------------------------------------------

@pytest.mark.parametrize("hash_alg", [4, 5, 6])
def test_hash_bursts_over_a_bulk_filled_table(dev, oracle_mod, hash_alg):
    """test_gpu_burst_mc's 7-connection burst (connection 0 in a rollover),
    the table filled by one bulk call; connection 6 gets no tx side."""
    from ilias_net2_amd import conn_burst
    c = M.case(oracle_mod, hash_alg, 7, 65)
    K, gone = c.K, 6
    assert c.has_alt[0]
    ops = []
    for k in range(K):
        ops.append(conn_burst.rx_op(
            k, c.keys[k], enc_set=bool(c.enc[k]),
            alt_key=c.alt_keys[k] if c.has_alt[k] else None,
            alt_no_cutoff=bool(c.no_cutoff[k]), alt_cutoff=int(c.cutoff[k]),
            rx_start=int(c.rx_start[k])))
        if k != gone:
            ops.append(conn_burst.tx_op(k, c.keys[k], enc_set=bool(c.enc[k])))
            if c.has_alt[k]:
                ops.append(conn_burst.tx_op(K + k, c.alt_keys[k], enc_set=bool(c.enc[k])))
    with conn_burst.KeyTable(hash_alg, 2 * K) as tab:
        tab.update(ops)
        got = M.run_tx_rx(dev, c, tab)
    no_tx = c.txconn % K == gone
    assert no_tx.any() and not no_tx.all()
    assert np.array_equal(got.tx_res, np.where(no_tx, NOCONN, c.tx_res))
    want = c.sealed.copy()
    for i in np.nonzero(no_tx)[0]:          # left untouched
        a, b = int(c.offs[i]), int(c.offs[i]) + int(c.slot[i])
        want[a:b] = c.data[a:b]
    assert np.array_equal(got.sealed, want)
    assert np.array_equal(got.rx_res, c.rx_res)
    assert np.array_equal(got.rx_seq, c.rx_seq) and np.array_equal(got.rx_fl, c.rx_fl)
    assert np.array_equal(got.rx_iv, c.rx_iv)


@pytest.mark.parametrize("in_place", [False, True])
def test_cipher_bursts_over_a_bulk_filled_table(dev, in_place):
    """test_gpu_aes_burst_mc's cases over 7 connections (EVP's plaintexts and
    ciphertexts), the cipher table filled by one bulk call."""
    from ilias_net2_amd import cipher_burst

    def fill(c, rx, tx):
        ops = []
        for k in c.conns:
            if rx:
                ops.append(cipher_burst.rx_op(
                    k.slot, k.key, hash_alg=6, alt_key=k.alt_key,
                    alt_no_cutoff=k.no_cutoff, alt_cutoff=k.cutoff, rx_start=k.rx_start))
            if tx:
                ops.append(cipher_burst.tx_op(k.slot, k.tx_key))
        tab = cipher_burst.CipherTable(c.slots)
        tab.update(ops)
        return tab
    c = A.rx_case(65, 7, 6)
    with fill(c, True, False) as tab:
        res, out, plen = A._decrypt_mc(dev, c, tab, in_place)
    A._check_rx(c, res, out, plen, in_place)
    if in_place:
        return
    c = A.tx_case(65, 7, 6)
    with fill(c, False, True) as tab:
        res, wire, got = A._encrypt_mc(dev, c, tab)
    assert np.array_equal(res, c.want_res)
    assert np.array_equal(wire[c.stated], c.want_wire[c.stated])
    assert np.array_equal(got, c.want)


# ---- 4. stream order and key lifetime ------------------------------------------------

def test_stream_order_and_key_lifetime(dev, oracle_mod):
    """On one stream, no host synchronisation: burst, bulk update, burst.  The
    datagrams are sealed under A; slot 3 holds A, the update makes it B, a
    second one A again: OK, BAD, OK.  `ops` and every key buffer are
    overwritten with 0xA5 as soon as each call returns.  Then the same with
    the update queued on table_stream ahead of a host burst."""
    from ilias_net2_amd import _lib, conn_burst
    L = _lib.lib()
    n, hash_alg, hl = 300, 6, 64
    rng = np.random.default_rng(56)
    KA, KB = (rng.integers(0, 256, hl, dtype=np.uint8).tobytes() for _ in range(2))
    lens = rng.choice(np.array([136, 584, 1500], dtype=np.uint32), n)
    offs = np.zeros(n, dtype=np.uint64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    data = rng.integers(0, 256, int(lens.sum()), dtype=np.uint8)
    seq = np.arange(n, dtype=np.uint32)
    flags = np.full(n, 3, dtype=np.uint32)
    _, sealed = oracle_mod.packet_encode_batch(hash_alg, KA, True, seq, flags, data, offs,
                                               lens, nthreads=M.CPU_THREADS)
    S = torch.cuda.Stream(device=dev)
    st = S.cuda_stream
    d, o = M._dev(sealed, dev), M._dev(offs.view(np.int64), dev)
    ln = M._dev(lens.view(np.int32), dev)
    conn = torch.full((n,), 3, dtype=torch.int32, device=dev)
    ws = conn_burst.burst_workspace(n, dev)
    outs = [torch.full((n,), 9, dtype=torch.uint8, device=dev) for _ in range(3)]
    iv = torch.zeros((n, 16), dtype=torch.uint8, device=dev)
    tab = conn_burst.KeyTable(hash_alg, SLOTS)

    def update(key, stream):
        # slot 3 and some neighbours, slot 3 twice: the last one counts
        ops = [conn_burst.rx_op(s, k, enc_set=True)
               for s, k in ((2, KB), (3, KB if key is KA else KA), (299, KA), (3, key))]
        arr, keep = tab.build_ops(ops)
        assert L.net2_burst_keytab_update(tab.ptr, arr, len(ops), stream) == 0
        ctypes.memset(arr, 0xA5, ctypes.sizeof(arr))
        for b in keep:
            if b is not None:
                ctypes.memset(b, 0xA5, ctypes.sizeof(b))

    def decode(k):
        assert L.net2_packet_decode_burst_mc(
            tab.ptr, conn.data_ptr(), 16, d.data_ptr(), o.data_ptr(), ln.data_ptr(), n,
            outs[k].data_ptr(), iv.data_ptr(), None, None, ws.data_ptr(), ws.numel(),
            st) == 0
    try:
        tab.set_rx(3, KA, enc_set=True)
        torch.cuda.synchronize()
        decode(0)
        update(KB, st)
        decode(1)
        update(KA, st)
        decode(2)
        torch.cuda.synchronize()
        got = [x.cpu().numpy() for x in outs]
        assert (got[0] == OK).all() and (got[1] == BAD).all() and (got[2] == OK).all()
        # ... and ahead of a host burst, on its table_stream, behind work that
        # keeps that stream busy for a while
        update(KB, st)
        torch.cuda.synchronize()
        busy = torch.empty(1 << 26, dtype=torch.uint8, device=dev)
        with torch.cuda.stream(S):
            for _ in range(8):
                busy.add_(1)
        update(KA, st)
        res = np.full(n, 9, dtype=np.uint8)
        hconn = np.full(n, 3, dtype=np.uint32)
        p = lambda a: a.ctypes.data  # noqa: E731
        _lib.check(L.net2_packet_decode_burst_mc_host(
            tab.ptr, None, p(hconn), 0, p(sealed), p(offs), p(lens), n, p(res), None,
            None, None, None, None, st))
        assert (res == OK).all()
        S.synchronize()
    finally:
        tab.close()


# ---- 5. all or nothing ----------------------------------------------------------------

@pytest.mark.parametrize("kind", [6, "aes"])
def test_all_or_nothing(dev, kind):
    from ilias_net2_amd import _lib, conn_burst
    rng = np.random.default_rng(5)
    with table(kind) as tab:
        per_slot(tab, rand_ops(kind, rng, 30, rng.integers(0, SLOTS, 30)))
        before = prints(tab)
        ops = rand_ops(kind, rng, 100, rng.integers(0, SLOTS, 100))
        k, slot, kw = ops[57]
        if k == _lib.TAB_CLEAR:
            k, kw = _lib.TAB_TX, dict(key=b"")
            if kind != "aes":
                kw["enc_set"] = False
        ops[57] = (k, slot, dict(kw, key=bytes(31)))      # no row's key length
        stats = conn_burst.tab_stats()
        with pytest.raises(_lib.Net2Error) as e:
            tab.update(ops)
        assert e.value.errno == errno.EINVAL
        assert conn_burst.tab_stats() == stats
        same(prints(tab), before)
        tab.update(ops[:57] + ops[58:])                   # the rest is fine
        assert not np.array_equal(prints(tab), before)


# ---- 6. capture ------------------------------------------------------------------------

def test_capture_is_refused_and_ends_cleanly(dev):
    """The bulk call on a capturing stream is EINVAL and leaves the capture
    intact: the per-slot call captured next to it replays."""
    from ilias_net2_amd import _lib, conn_burst
    key = bytes(range(64))
    with table(6) as tab, table(6) as twin:
        tab.set_rx(1, key)
        twin.set_rx(1, key)
        torch.cuda.synchronize()
        stats = conn_burst.tab_stats()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            tab.set_tx(299, key, enc_set=True)
            with pytest.raises(_lib.Net2Error) as e:
                tab.update([conn_burst.tx_op(5, key)])
            tab.clear(1)
        assert e.value.errno == errno.EINVAL
        assert conn_burst.tab_stats() == (stats[0] + 2, stats[1])
        g.replay()
        torch.cuda.synchronize()
        twin.set_tx(299, key, enc_set=True)
        twin.clear(1)
        same(prints(tab), prints(twin))
        # outside the capture the same call goes through
        tab.update([conn_burst.tx_op(5, key)])
        twin.set_tx(5, key)
        same(prints(tab), prints(twin))


# ---- 7. two threads ---------------------------------------------------------------------

@pytest.mark.parametrize("kind", [5, "aes"])
def test_two_threads_two_streams(dev, kind):
    """Disjoint halves of the slots, 20 updates each, from two threads on two
    streams: the table ends as after the sequential run."""
    rng = np.random.default_rng(70 + (7 if kind == "aes" else kind))
    halves = (np.arange(0, 150), np.arange(150, 300))
    lists = [[rand_ops(kind, rng, 24, h[rng.integers(0, 150, 24)]) for _ in range(20)]
             for h in halves]
    errors = []

    def run(tab, mine, stream):
        try:
            for ops in mine:
                tab.update(ops, stream=stream)
            stream.synchronize()
        except Exception as exc:                     # noqa: BLE001
            errors.append(exc)
    with table(kind) as tab, table(kind) as twin:
        streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
        torch.cuda.synchronize()
        ths = [threading.Thread(target=run, args=(tab, lists[i], streams[i]))
               for i in range(2)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        assert not errors, errors
        for mine in lists:
            for ops in mine:
                twin.update(ops)
        same(prints(tab), prints(twin))
        per = table(kind)
        try:
            for mine in lists:
                for ops in mine:
                    per_slot(per, ops)
            same(prints(per), prints(twin))
        finally:
            per.close()
