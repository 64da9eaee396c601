"""The quad form of the encrypt bursts (aes_cbc_encrypt_quad_kernel: four
adjacent lanes per datagram, one column of the AES state each, the other three
columns fetched from the neighbours by quad_perm moves once a round --
ilias_net2_amd/csrc/aes_quad.h), which net2_packet_encrypt_burst and
net2_packet_encrypt_burst_mc take for bursts of at most
net2_aes_encrypt_limits' quad_max datagrams.

Every TX and chain test of the lane form is run again in both forms, pinned
(net2_aes_encrypt_limits; net2_aes_encrypt_stats tells which form ran): the
bursts of tests/test_gpu_aes_burst.py and tests/test_gpu_aes_burst_mc.py.
Then what only the quad form has: tails that end before, on and after each
column boundary, quads of very different lengths side by side in one wave,
bursts on both sides of the quad, wave and workgroup edges; the two forms
against each other byte for byte; graph replay; and the default threshold
itself.

Expected values come from EVP (tests/aes_ref.py), as in the lane form's tests.
"""
import functools
import types

import numpy as np
import pytest

import aes_ref
import test_gpu_aes_burst as A
import test_gpu_aes_burst_mc as M
import test_gpu_burst_graph as G

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

OK, RESOURCE, NOCONN = 0, 1, 5
ENC, SIGNED = A.ENC, A.SIGNED
HASH6, HL6 = 6, 64
QUADS = 64                  # datagrams per workgroup and step (AES_QUADS)
PER_ABOVE = QUADS * 1280    # a workgroup takes two groups of 64 above this n


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a GPU (HIP device not visible)")
    from ilias_net2_amd import _lib
    assert _lib.device_count() >= 1
    return torch.device("cuda:0")


def _pinned(limit, rose, still):
    from ilias_net2_amd import cipher_burst
    cipher_burst.encrypt_limits(limit)
    before = cipher_burst.encrypt_stats()
    try:
        yield
        after = cipher_burst.encrypt_stats()
    finally:
        cipher_burst.encrypt_limits(-1)
    assert after[rose] > before[rose]
    assert after[still] == before[still]


@pytest.fixture
def quad():
    """Every encrypt burst of the test in the quad form: at least one was
    launched, and none in the lane form."""
    yield from _pinned(1 << 30, "quad_launches", "lane_launches")


@pytest.fixture
def lane():
    """Every encrypt burst of the test in the lane form, whatever the default
    threshold: at least one was launched, and none in the quad form."""
    yield from _pinned(0, "lane_launches", "quad_launches")


@pytest.fixture(params=["quad", "lane"])
def form(request):
    request.getfixturevalue(request.param)
    return request.param


# ---- 1. the lane form's TX and chain tests, in both forms -------------------------

@pytest.mark.parametrize("hash_alg", [4, 6, 0, 5])
def test_tx_burst_both_forms(dev, form, hash_alg):
    A.test_tx_burst(dev, hash_alg)


def test_known_answer_both_forms(dev, form):
    A.test_known_answer(dev)


def test_divergent_lengths_both_forms(dev, form):
    A.test_divergent_lengths(dev)


@pytest.mark.parametrize("pattern", ["ties", "descending", "cycle"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513])
def test_burst_sizes_and_rank_ties_both_forms(dev, form, n, pattern):
    A.test_burst_sizes_and_rank_ties(dev, n, pattern)


def test_tx_length_extremes_both_forms(dev, form):
    A.test_tx_length_extremes(dev)


@pytest.mark.parametrize("iv_at", [1, 3, 8])
def test_unaligned_iv_array_both_forms(dev, form, iv_at):
    A.test_unaligned_iv_array(dev, iv_at)


def test_chain_on_one_stream_both_forms(dev, oracle_mod, form):
    A.test_chain_on_one_stream(dev, oracle_mod)


def test_chain_on_one_stream_no_cutoff_both_forms(dev, oracle_mod, form):
    A.test_chain_on_one_stream_no_cutoff(dev, oracle_mod)


def test_keys_need_not_outlive_the_call_both_forms(dev, oracle_mod, form):
    A.test_keys_need_not_outlive_the_call(dev, oracle_mod)


@pytest.mark.parametrize("n,K,hash_alg", M.SHAPES)
def test_mc_tx_mixed_keys_both_forms(dev, form, n, K, hash_alg):
    M.test_tx_mixed_keys(dev, n, K, hash_alg)


@pytest.mark.parametrize("alt", [False, True])
def test_mc_one_connection_equals_the_single_connection_calls_both_forms(dev, form, alt):
    M.test_one_connection_equals_the_single_connection_calls(dev, alt)


def test_mc_missing_connections_both_forms(dev, form):
    M.test_missing_connections(dev)


def test_mc_updates_are_stream_ordered_both_forms(dev, form):
    M.test_updates_are_stream_ordered(dev)


def test_mc_chain_on_one_stream_both_forms(dev, form):
    M.test_chain_on_one_stream(dev)


# ---- bursts of this module ----------------------------------------------------------

KEYS = [bytes((29 * k + 7 * j + 3) & 0xff for j in range(32)) for k in range(2)]
SLOT_OF = (2, 0)            # connection k's slot of a three-slot table; 1 is unset
IDLE = ("plain", "plain_short", "short", "noconn")


def build_case(seed, specs, mc):
    """One TX burst.  specs: per slot (kind, nb, rem) -- "enc": PH_ENCRYPTED
    with plen = 16 (nb - 1) + rem, room for exactly the nb blocks or up to 9
    bytes to spare; "plain" / "plain_short": no PH_ENCRYPTED, with room and a
    byte short; "short": PH_ENCRYPTED a byte short of its room; "noconn" (as
    "enc" without mc): a connection the table does not have.  Every slot and,
    the payload offset being even, every payload at an odd address.  mc:
    connections 0 and 1 two slots each in turn, else KEYS[0] throughout.  The
    slack -- a slot's bytes from plen to the end of its last block -- comes
    in two fills, data[0] and data[1], alike everywhere else; `want` is the
    one buffer both must end as."""
    rng = np.random.default_rng(seed)
    n = len(specs)
    i_ = np.arange(n)
    kind = np.array([s[0] if mc or s[0] != "noconn" else "enc" for s in specs])
    nb = np.array([s[1] for s in specs], dtype=np.int64)
    plen = (16 * (nb - 1) + np.array([s[2] for s in specs])).astype(np.uint32)
    enc = np.isin(kind, ("enc", "short", "noconn"))
    flags = np.where(enc, ENC, 0).astype(np.uint32)
    flags[i_ % 3 != 1] |= SIGNED
    po = A._po(flags, HL6)
    need = po + np.where(enc, 16 * nb, plen)
    spare = np.where(i_ % 2 == 0, 0, 1 + i_ % 9)
    lens = np.where(np.isin(kind, ("plain_short", "short")), need - 1,
                    need + spare).astype(np.uint32)
    c_of = (i_ // 2) % 2 if mc else np.zeros(n, dtype=np.int64)
    conn = np.array([SLOT_OF[k] for k in c_of], dtype=np.uint32)
    conn[kind == "noconn"] = np.where(i_[kind == "noconn"] % 2, 1, 0xffffffff)
    iv = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    offs = np.zeros(n, dtype=np.uint64)
    cur = 65
    for i in range(n):
        offs[i] = cur
        cur += int(lens[i]) + int(rng.integers(1, 8))
        cur += 1 - cur % 2                      # odd
    total = cur + 64
    assert (offs % 2 == 1).all() and ((offs + po.astype(np.uint64)) % 2 == 1).all()
    data0 = rng.integers(0, 256, total, dtype=np.uint8)
    data1 = data0.copy()
    want = data0.copy()
    want_res = np.zeros(n, dtype=np.uint8)
    want_wire = np.zeros(n, dtype=np.uint32)
    stated = np.ones(n, dtype=bool)             # wire_len is specified
    for i in range(n):
        a = int(offs[i]) + int(po[i])
        if kind[i] == "plain":
            want_wire[i] = po[i] + plen[i]
        elif kind[i] == "plain_short":
            want_res[i], stated[i] = RESOURCE, False
        elif kind[i] == "short":
            want_res[i] = RESOURCE
        elif kind[i] == "noconn":
            want_res[i] = NOCONN
        else:
            pl, end = int(plen[i]), a + 16 * int(nb[i])
            data1[a + pl:end] = ~data0[a + pl:end]
            ct = aes_ref.encrypt(KEYS[c_of[i]], iv[i].tobytes(), data0[a:a + pl].tobytes())
            assert len(ct) == 16 * nb[i] and end <= int(offs[i]) + int(lens[i])
            want[a:end] = np.frombuffer(ct, dtype=np.uint8)
            want_wire[i] = po[i] + len(ct)
    for a in (data0, data1, offs, lens, flags, iv, plen, conn, want, want_res, want_wire):
        a.setflags(write=False)
    return types.SimpleNamespace(
        n=n, mc=mc, hl=HL6, kind=kind, nb=nb, flags=flags, iv=iv, plen=plen, lens=lens,
        offs=offs, conn=conn, c_of=c_of, data=[data0, data1], total=total, want=want,
        want_res=want_res, want_wire=want_wire, stated=stated)


def run_case(dev, c, fill=0, n=None):
    """The first n slots of the burst (default: all) through the C entry
    point of its key source, d_result and d_wire_len pre-filled.  Returns host
    (result, wire_len, buffer)."""
    from ilias_net2_amd import cipher_burst
    n = c.n if n is None else n
    cc = types.SimpleNamespace(
        n=n, hl=c.hl, data=c.data[fill], offs=c.offs[:n], lens=c.lens[:n],
        flags=c.flags[:n], plen=c.plen[:n], iv=c.iv[:n], conn=c.conn[:n])
    if c.mc:
        with cipher_burst.CipherTable(3) as tab:
            for k in range(2):
                tab.set_tx(SLOT_OF[k], KEYS[k])
            tab.set_rx(1, KEYS[0])              # slot 1: the other side only
            return M._encrypt_mc(dev, cc, tab)
    d = A._dev(cc.data, dev)
    res, wire = A._c_encrypt(dev, KEYS[0], cc.hl, d, cc.offs, cc.lens, cc.flags,
                             A._dev(cc.iv, dev), cc.plen)
    return res, wire, d.cpu().numpy()


def check_case(c, got, n=None):
    """Codes, wire_len where the header states one, and the whole buffer:
    every ciphertext byte as EVP's, every other byte as it was -- slots of any
    other code in full, and of the slots from n on everything."""
    n = c.n if n is None else n
    res, wire, buf = got
    bad = np.nonzero(res != c.want_res[:n])[0]
    assert len(bad) == 0, [(int(i), c.kind[i], int(res[i])) for i in bad[:8]]
    bad = np.nonzero((wire != c.want_wire[:n]) & c.stated[:n])[0]
    assert len(bad) == 0, [(int(i), c.kind[i], hex(wire[i])) for i in bad[:8]]
    want = c.want
    if n < c.n:
        want = c.want.copy()
        want[int(c.offs[n]):] = c.data[0][int(c.offs[n]):]
    bad = np.nonzero(buf != want)[0]
    if len(bad):
        i = int(np.searchsorted(c.offs, bad[0], side="right")) - 1
        at = int(bad[0]) - int(c.offs[i])
        pytest.fail(f"slot {i} ({c.kind[i]}, {int(c.nb[i])} blocks, plen {int(c.plen[i])}): "
                    f"byte {at} of the slot differs; {len(bad)} bytes in all")


# ---- 2. what only the quad form can get wrong ---------------------------------------

# a full pad block, and a tail that ends just before, on and after each
# column boundary (4, 8, 12)
REMS = (0, 1, 3, 4, 5, 7, 8, 9, 11, 12, 13, 15)
# neighbours in this order: a 1-block datagram beside a 4,090-block one (64
# passes less six blocks: the longest payload of a 16-bit datagram length)
EDGE_NBS = (1, 4090, 2, 90, 3, 89, 88)


@functools.lru_cache(maxsize=None)
def edge_case(mc):
    """Every EDGE_NBS length with every REMS tail, neighbouring quads of a
    wave differing in length, and after every fourth a slot without cipher
    work: n = 105, no multiple of 4, 16 or 64.  Built once; the tests leave
    it unchanged."""
    specs = []
    for rem in REMS:
        for nb in EDGE_NBS:
            specs.append(("enc", nb, rem))
            if len(specs) % 5 == 4:
                specs.append((IDLE[(len(specs) // 5) % len(IDLE)], 2, 5))
    n = len(specs)
    assert n == 105 and n % 4 and n % 16 and n % 64
    c = build_case([5600, int(mc)], specs, mc)
    assert set(c.kind) == set(IDLE if mc else IDLE[:3]) | {"enc"}
    assert (np.abs(np.diff(c.nb)) > 0).sum() > 80
    return c


@pytest.mark.parametrize("mc", [False, True], ids=["one", "mc"])
def test_column_tails_and_divergent_quads(dev, quad, mc):
    """1, 2, 3, 88, 89, 90 and 4,090 blocks with plen mod 16 on both sides of
    every column boundary, at odd addresses: lane q forms its word of the last
    block from the plaintext bytes below plen and the padding value, the
    quads of a wave leave the block loop up to 4,089 iterations apart, and
    slots without cipher work lie between them (with mc two connections'
    keys, and slots without a connection).  Every ciphertext byte, code and
    wire_len against EVP; every other byte unchanged; the same with the slack
    bytes filled another way."""
    c = edge_case(mc)
    got = [run_case(dev, c, fill) for fill in (0, 1)]
    check_case(c, got[0])
    check_case(c, got[1])
    assert np.array_equal(got[0][2], got[1][2])


# ---- 3. burst sizes --------------------------------------------------------------------

SIZES = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def sized_case(mc):
    """257 slots, 1 to 6 blocks and now and then 89, every tail, about one in
    eight without cipher work: the bursts of SIZES are its prefixes."""
    specs = []
    for i in range(max(SIZES)):
        if i % 8 == 5:
            specs.append((IDLE[(i // 8) % len(IDLE)], 1 + i % 3, i % 16))
        else:
            specs.append(("enc", 89 if i % 23 == 11 else 1 + (i * 7) % 6, (5 * i) % 16))
    return build_case([5700, int(mc)], specs, mc)


@pytest.mark.parametrize("mc", [False, True], ids=["one", "mc"])
@pytest.mark.parametrize("n", SIZES)
def test_burst_sizes(dev, quad, n, mc):
    """Bursts that end one short of, on and one past a quad (of the 16 in a
    wave), a wave and a workgroup: the lanes past the end do nothing, the
    slots past the end stay as they were."""
    c = sized_case(mc)
    check_case(c, run_case(dev, c, 0, n), n)


# ---- 4. the two forms against each other -------------------------------------------------

def _both_forms(run):
    """run() under limit 0 and under limit 2^30; the launch counts say that
    it was the lane form, then the quad form."""
    from ilias_net2_amd import cipher_burst
    outs = []
    try:
        for limit, took in ((0, "lane_launches"), (1 << 30, "quad_launches")):
            cipher_burst.encrypt_limits(limit)
            before = cipher_burst.encrypt_stats()
            outs.append(run())
            after = cipher_burst.encrypt_stats()
            assert {k: after[k] - before[k] for k in after} == {
                "lane_launches": int(took == "lane_launches"),
                "quad_launches": int(took == "quad_launches")}
    finally:
        cipher_burst.encrypt_limits(-1)
    return outs


def _same(outs):
    for a, b in zip(*outs):
        bad = np.nonzero(a != b)[0]
        assert len(bad) == 0, bad[:8]


def test_quad_and_lane_forms_agree(dev):
    """One burst of 1,000 slots, RESOURCE and unencrypted ones included:
    codes, wire_len and the whole buffer of the lane form (limit 0) and of
    the quad form (limit 2^30) identical, and EVP's."""
    c = A.tx_case(HASH6, n=1000)

    def run():
        d = A._dev(c.data, dev)
        res, wire = A._c_encrypt(dev, c.key, c.hl, d, c.offs, c.lens, c.flags,
                                 A._dev(c.iv, dev), c.plen)
        return res, wire, d.cpu().numpy()
    outs = _both_forms(run)
    _same(outs)
    res, wire, got = outs[1]
    assert np.array_equal(res, c.want_res) and np.array_equal(got, c.want)
    assert np.array_equal(wire, c.want_wire)
    assert (res == RESOURCE).sum() > 50 and ((c.flags & ENC) == 0).sum() > 100


def test_quad_and_lane_forms_agree_mc(dev):
    """The same over five connections' keys from the cipher-key table:
    NOCONN slots as well."""
    c = M.tx_case(1000, 5, HASH6)
    with M._table(c, HASH6, rx=False) as tab:
        outs = _both_forms(lambda: M._encrypt_mc(dev, c, tab))
    _same(outs)
    res, wire, got = outs[1]
    assert np.array_equal(res, c.want_res) and np.array_equal(got, c.want)
    assert np.array_equal(wire[c.stated], c.want_wire[c.stated])
    assert {OK, RESOURCE, NOCONN} <= set(res)


@functools.lru_cache(maxsize=None)
def looped_case():
    """81,920 + 333 slots of 1 to 3 blocks, a tenth each unencrypted, a byte
    short and without a connection: the smallest kind of burst at which a
    workgroup of the quad form takes a second group of 64.  No expected
    values: the forms are compared with each other."""
    n = PER_ABOVE + 333
    rng = np.random.default_rng(5800)
    i_ = np.arange(n)
    kind = rng.integers(0, 10, n)
    plen = ((i_ * 7) % 48).astype(np.uint32)
    flags = np.where(kind == 0, 0, ENC).astype(np.uint32)
    flags[i_ % 3 == 0] |= SIGNED
    po = A._po(flags, HL6)
    need = po + np.where(kind == 0, plen, 16 * (plen // 16 + 1))
    lens = (need - (kind == 1)).astype(np.uint32)
    offs = np.concatenate(([3], 3 + np.cumsum(lens[:-1].astype(np.uint64) + 1))
                          ).astype(np.uint64)
    total = int(offs[-1]) + int(lens[-1]) + 16
    conn = np.where(kind == 2, np.where(i_ % 2, 1, 0xffffffff),
                    np.array(SLOT_OF)[i_ % 2]).astype(np.uint32)
    return types.SimpleNamespace(
        n=n, hl=HL6, flags=flags, plen=plen, lens=lens, offs=offs, conn=conn,
        iv=rng.integers(0, 256, (n, 16), dtype=np.uint8),
        data=rng.integers(0, 256, total, dtype=np.uint8))


@pytest.mark.parametrize("mc", [False, True], ids=["one", "mc"])
def test_quad_and_lane_forms_agree_where_a_workgroup_loops(dev, mc):
    from ilias_net2_amd import cipher_burst
    c = looped_case()
    if mc:
        with cipher_burst.CipherTable(3) as tab:
            for k in range(2):
                tab.set_tx(SLOT_OF[k], KEYS[k])
            outs = _both_forms(lambda: M._encrypt_mc(dev, c, tab))
    else:
        def run():
            d = A._dev(c.data, dev)
            res, wire = A._c_encrypt(dev, KEYS[0], c.hl, d, c.offs, c.lens, c.flags,
                                     A._dev(c.iv, dev), c.plen)
            return res, wire, d.cpu().numpy()
        outs = _both_forms(run)
    _same(outs)
    res = outs[1][0]
    assert set(res) == ({OK, RESOURCE, NOCONN} if mc else {OK, RESOURCE})
    assert (res[-333:] == OK).sum() > 200 and (outs[1][2] != c.data).sum() > 16 * c.n


# ---- 5. graph replay -----------------------------------------------------------------------

def test_graph_replay(dev, quad):
    """net2_packet_encrypt_burst in the quad form captured into a graph on
    one stream and replayed, the second time on other plaintext bytes, each
    against EVP (the protocol of tests/test_gpu_burst_graph.py)."""
    G.test_cipher_tx(dev, None)


def test_graph_replay_mc(dev, quad):
    """The same for net2_packet_encrypt_burst_mc behind a table update."""
    G.test_cipher_tx_many_connections(dev, None)


# ---- 6. the default threshold ----------------------------------------------------------------

class _Idle:
    """Bursts of n slots without PH_ENCRYPTED, all at offset 0 of one 16-byte
    buffer: no cipher work, nothing written but codes and wire_len, one
    launch."""

    def __init__(self, dev, cap):
        z = lambda dt, *shape: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        self.data, self.offs = z(torch.uint8, 16), z(torch.int64, cap)
        self.lens = torch.full((cap,), 8, dtype=torch.int32, device=dev)
        self.flags, self.conn, self.plen = (z(torch.int32, cap) for _ in range(3))
        self.iv = z(torch.uint8, cap, 16)

    def form(self, n, tab=None):
        """The form a burst of n takes: 'lane' or 'quad'."""
        from ilias_net2_amd import cipher_burst
        before = cipher_burst.encrypt_stats()
        a = (self.flags[:n], self.iv[:n], self.data, self.offs[:n], self.lens[:n],
             self.plen[:n])
        if tab is None:
            res, wire = cipher_burst.encrypt_burst(bytes(32), 0, *a)
        else:
            res, wire = cipher_burst.encrypt_burst_mc(tab, self.conn[:n], 0, *a)
        torch.cuda.synchronize()
        assert int(res.sum()) == 0 and int((wire != 8).sum()) == 0
        after = cipher_burst.encrypt_stats()
        d = {k: after[k] - before[k] for k in after}
        assert sorted(d.values()) == [0, 1], d
        return "quad" if d["quad_launches"] else "lane"


def test_default_threshold(dev):
    """At the default limit: a burst of exactly the default takes the quad
    form and one slot more the lane form, for both calls, and so does one of
    1 M.  The default is found by bisection over idle bursts
    (net2_aes_encrypt_stats is the only witness)."""
    from ilias_net2_amd import cipher_burst
    cipher_burst.encrypt_limits(-1)
    cap = 1 << 20
    idle = _Idle(dev, cap)
    if idle.form(1) == "lane":
        pytest.skip("the default is 0: the quad form is never taken")
    assert idle.form(cap) == "lane", "the default is 1 M datagrams or more"
    lo, hi = 1, cap                     # form(lo) == quad, form(hi) == lane
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if idle.form(mid) == "quad" else (lo, mid)
    default = lo
    assert idle.form(default) == "quad" and idle.form(default + 1) == "lane"
    with cipher_burst.CipherTable(1) as tab:
        assert idle.form(default, tab) == "quad"
        assert idle.form(default + 1, tab) == "lane"
        assert idle.form(1 << 20, tab) == "lane"
