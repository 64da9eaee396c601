"""The wave form of the decrypt bursts (aes_cbc_decrypt_wave_kernel: one wave
per datagram, the datagram's blocks spread over the wave's 64 lanes, 64 to a
pass, last pass first -- ilias_net2_amd/csrc/aes_wave.h), which
net2_packet_decrypt_burst and net2_packet_decrypt_burst_mc take for bursts of
at most net2_aes_burst_limits' wave_max datagrams.

Every RX parity test of the lane form is run again in the wave form
(net2_aes_burst_limits raises the limit so bursts of any size take it;
net2_aes_burst_stats tells which form ran): the bursts of
tests/test_gpu_aes_burst.py and tests/test_gpu_aes_burst_mc.py.  Then what
only the wave form has: datagrams on both sides of every pass boundary, in
place and out of place, under all three key sources; broken padding at the
same lengths, where nothing may be written; the two forms against each other
byte for byte; and the default threshold itself.

Expected values come from EVP (tests/aes_ref.py), as in the lane form's tests.
"""
import functools
import struct
import types

import numpy as np
import pytest

import aes_ref
import test_gpu_aes_burst as A
from test_gpu_aes_burst import hash_form  # noqa: F401  (the hash bursts' form)
import test_gpu_aes_burst_mc as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

OK, BAD, NOCONN = 0, 2, 5
ENC, SIGNED, ALTKEY = A.ENC, A.SIGNED, A.ALTKEY
SENTINEL = 0xA5
STALE = 0x5A5A5A5A
HASH6, HL6 = 6, 64
# blocks per datagram: one short of, on and one past every pass boundary up
# to three passes (a pass is 64 blocks), the shortest two, and 64 passes less
# six blocks -- the longest payload a 16-bit datagram length leaves room for
NBS = (1, 2, 63, 64, 65, 127, 128, 129, 192, 193, 4090)
WAVES = 4                   # datagrams per workgroup and step (AES_WAVES)
SRCS = ("one", "alt", "tab")    # the kernel's three key sources


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a GPU (HIP device not visible)")
    from ilias_net2_amd import _lib
    assert _lib.device_count() >= 1
    return torch.device("cuda:0")


@pytest.fixture
def wave():
    """Every decrypt burst of the test in the wave form: at least one was
    launched, and none in the lane form."""
    from ilias_net2_amd import cipher_burst
    cipher_burst.limits(1 << 30)
    before = cipher_burst.stats()
    yield
    after = cipher_burst.stats()
    cipher_burst.limits(-1)
    assert after["wave_launches"] > before["wave_launches"]
    assert after["lane_launches"] == before["lane_launches"]


# ---- 1. the lane form's parity tests, in the wave form ---------------------------

@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("hash_alg,no_cutoff", [
    pytest.param(4, False, id="4"), pytest.param(6, False, id="6"),
    pytest.param(0, False, id="0"), pytest.param(5, False, id="5"),
    pytest.param(6, True, id="6-no_cutoff"), pytest.param(4, True, id="4-no_cutoff")])
def test_rx_burst_wave_form(dev, oracle_mod, wave, hash_alg, no_cutoff, in_place):
    A.test_rx_burst(dev, oracle_mod, hash_alg, no_cutoff, in_place)


def test_known_answer_wave_form(dev, wave):
    A.test_known_answer(dev)


def test_divergent_lengths_wave_form(dev, wave):
    A.test_divergent_lengths(dev)


@pytest.mark.parametrize("pattern", ["ties", "descending", "cycle"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513])
def test_burst_sizes_wave_form(dev, wave, n, pattern):
    A.test_burst_sizes_and_rank_ties(dev, n, pattern)


@pytest.mark.parametrize("in_place", [False, True])
def test_rx_incoming_codes_are_kept_wave_form(dev, wave, in_place):
    A.test_rx_incoming_codes_are_kept(dev, in_place)


@pytest.mark.parametrize("in_place", [False, True])
def test_rx_shorter_than_payload_offset_wave_form(dev, wave, in_place):
    A.test_rx_shorter_than_payload_offset(dev, in_place)


@pytest.mark.parametrize("iv_at", [1, 3, 8])
def test_unaligned_iv_array_wave_form(dev, wave, iv_at):
    A.test_unaligned_iv_array(dev, iv_at)


def test_chain_on_one_stream_wave_form(dev, oracle_mod, wave):
    A.test_chain_on_one_stream(dev, oracle_mod)


def test_chain_on_one_stream_no_cutoff_wave_form(dev, oracle_mod, wave):
    A.test_chain_on_one_stream_no_cutoff(dev, oracle_mod)


def test_keys_need_not_outlive_the_call_wave_form(dev, oracle_mod, wave):
    A.test_keys_need_not_outlive_the_call(dev, oracle_mod)


def test_chain_above_4gib_wave_form(dev, oracle_mod, wave, hash_form):
    A.test_chain_above_4gib(dev, oracle_mod, hash_form, "wave")


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("n,K,hash_alg", M.SHAPES)
def test_mc_rx_mixed_keys_wave_form(dev, wave, n, K, hash_alg, in_place):
    M.test_rx_mixed_keys(dev, n, K, hash_alg, in_place)


@pytest.mark.parametrize("alt", [False, True])
def test_mc_one_connection_equals_the_single_connection_calls_wave_form(dev, wave, alt):
    M.test_one_connection_equals_the_single_connection_calls(dev, alt)


def test_mc_alternate_keys_per_connection_wave_form(dev, wave):
    M.test_alternate_keys_per_connection(dev)


def test_mc_missing_connections_wave_form(dev, wave):
    M.test_missing_connections(dev)


def test_mc_updates_are_stream_ordered_wave_form(dev, wave):
    M.test_updates_are_stream_ordered(dev)


def test_mc_chain_on_one_stream_wave_form(dev, wave):
    M.test_chain_on_one_stream(dev)


# ---- 2. and 3.: pass boundaries, valid and with broken padding -------------------

BROKEN = ("pad00", "pad11", "padrun")


@functools.lru_cache(maxsize=None)
def edge_case(src, broken):
    """One burst under key source `src`.  Not broken: every NBS length twice
    and one more datagram, so n = 23 is no multiple of the datagrams per
    workgroup.  Broken: every NBS length with a last byte of 0, a last byte
    of 17 and a run of v whose bytes are not all v, then an empty and a ragged
    ciphertext (n = 35).  Every datagram at an odd offset, its payload 8 or 72
    bytes further (odd again), 1 to 7 stray bytes between datagrams.  With
    "alt" the alternate key on every other datagram (PH_ALTKEY, no cutoff);
    with "tab" two connections two datagrams each in turn, the alternate key
    of each on every other datagram: the waves of a workgroup differ in key.
    Built once; the tests leave it unchanged."""
    rng = np.random.default_rng([5500, SRCS.index(src), int(broken)])
    if broken:
        specs = [(nb, k) for nb in NBS for k in BROKEN] + [(0, "empty"), (3, "ragged")]
    else:
        specs = [(nb, "ok") for nb in NBS] * 2 + [(65, "ok")]
    n = len(specs)
    assert n % WAVES != 0 and n > 2 * WAVES
    keys = [[A._bytes(rng, 32), A._bytes(rng, 32)] for _ in range(2)]  # [conn][alt]
    i_ = np.arange(n)
    alt = (i_ % 2 == 1) if src != "one" else np.zeros(n, dtype=bool)
    c_of = (i_ // 2) % 2 if src == "tab" else np.zeros(n, dtype=np.int64)
    flags = np.where(i_ % 3 != 0, ENC | SIGNED, ENC).astype(np.uint32)
    flags[alt] |= ALTKEY
    seq = (7000 + i_).astype(np.uint32)
    iv = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    po = A._po(flags, HL6)
    dgs, want_plain = [], []
    for i, (nb, kind) in enumerate(specs):
        key, ivb = keys[c_of[i]][int(alt[i])], iv[i].tobytes()
        if kind == "ok":
            plain = A._bytes(rng, 16 * nb - 1 - (i % 16))          # pad 1 .. 16
            ct = aes_ref.encrypt(key, ivb, plain)
        elif kind in BROKEN:
            body = bytearray(A._bytes(rng, 16 * nb))
            tail = {"pad00": b"\x00", "pad11": b"\x11", "padrun": b"\x03\x02\x03"}[kind]
            body[len(body) - len(tail):] = tail
            plain, ct = None, aes_ref.encrypt(key, ivb, bytes(body), pad=False)
        elif kind == "empty":
            plain, ct = None, b""
        else:
            plain = None
            ct = aes_ref.encrypt(key, ivb, A._bytes(rng, 16 * nb - 5))[:16 * nb - 7]
        assert kind in ("empty", "ragged") or len(ct) == 16 * nb
        assert (aes_ref.decrypt(key, ivb, ct) if ct else None) == plain
        field = A._bytes(rng, HL6) if flags[i] & SIGNED else b""
        dgs.append(struct.pack(">II", int(seq[i]), int(flags[i])) + field + ct)
        want_plain.append(plain)
    lens = np.array([len(d) for d in dgs], dtype=np.uint32)
    offs = np.zeros(n, dtype=np.uint64)
    cur = 65
    for i in range(n):
        offs[i] = cur
        cur += int(lens[i]) + int(rng.integers(1, 8))
        cur += 1 - cur % 2                      # odd
    total = cur + 64
    assert (offs % 2 == 1).all() and ((offs + po.astype(np.uint64)) % 2 == 1).all()
    data = rng.integers(0, 256, total, dtype=np.uint8)
    A._fill(data, offs, dgs)
    want_res = np.array([OK if p is not None else BAD for p in want_plain], dtype=np.uint8)
    want_plen = np.array([len(p) if p is not None else 0 for p in want_plain],
                         dtype=np.uint32)
    written = np.zeros(total, dtype=bool)
    for i in np.nonzero(want_res == OK)[0]:
        written[int(offs[i]) + int(po[i]):int(offs[i]) + int(lens[i])] = True
    assert written.any() != broken
    for a in (data, offs, lens, seq, flags, iv, want_res, want_plen, written):
        a.setflags(write=False)
    return types.SimpleNamespace(
        n=n, src=src, keys=keys, c_of=c_of, alt=alt, seq=seq, flags=flags, iv=iv,
        po=po, data=data, offs=offs, lens=lens, total=total, want_res=want_res,
        want_plen=want_plen, want_plain=want_plain, written=written)


def _run_edge(dev, c, in_place):
    """The burst through the call of its key source, d_plen pre-filled with
    STALE.  Returns host (result, out, plen)."""
    from ilias_net2_amd import cipher_burst
    if c.src == "tab":
        tab = cipher_burst.CipherTable(3)
        for k, slot in ((0, 2), (1, 0)):
            tab.set_rx(slot, c.keys[k][0], hash_alg=HASH6, alt_key=c.keys[k][1],
                       alt_no_cutoff=True)
        conn = np.where(c.c_of == 0, 2, 0).astype(np.uint32)
        cc = types.SimpleNamespace(
            data=c.data, total=c.total, offs=c.offs, lens=c.lens, seq=c.seq,
            flags=c.flags, conn=conn, iv=c.iv, n=c.n, hl=HL6,
            res_in=np.zeros(c.n, dtype=np.uint8))
        with tab:
            return M._decrypt_mc(dev, cc, tab, in_place)
    d = A._dev(c.data, dev)
    out = d if in_place else torch.full((c.total,), SENTINEL, dtype=torch.uint8,
                                        device=dev)
    res, plen = A._c_decrypt(dev, HASH6, c.keys[0][0],
                             c.keys[0][1] if c.src == "alt" else None, True, 0, 0, d,
                             out, c.offs, c.lens, c.seq, c.flags, A._dev(c.iv, dev),
                             np.zeros(c.n, dtype=np.uint8))
    return res, out.cpu().numpy(), plen


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("src", SRCS)
def test_pass_boundaries(dev, wave, src, in_place):
    """1, 2, 63 .. 193 and 4,090 blocks: one, two, three, four and 64 passes,
    a last pass of one lane and of all 64, and the pass boundary where lane
    63's block is the prev of the pass above it -- in place that block must
    be read before the pass above is stored.  Every plaintext byte and
    length against EVP; every byte outside the payloads unchanged."""
    c = edge_case(src, False)
    res, out, plen = _run_edge(dev, c, in_place)
    assert np.array_equal(res, c.want_res), res
    assert np.array_equal(plen, c.want_plen), plen
    for i in range(c.n):
        a = int(c.offs[i]) + int(c.po[i])
        got = out[a:a + int(plen[i])].tobytes()
        if got != c.want_plain[i]:
            at = next(k for k in range(len(got)) if got[k] != c.want_plain[i][k])
            pytest.fail(f"datagram {i} ({int(c.lens[i] - c.po[i]) // 16} blocks): "
                        f"plaintext differs from byte {at} (block {at // 16})")
    untouched = ~c.written
    if in_place:
        assert np.array_equal(out[untouched], c.data[untouched])
    else:
        assert (out[untouched] == SENTINEL).all()


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("src", SRCS)
def test_broken_padding_writes_nothing(dev, wave, src, in_place):
    """The same lengths with the three kinds of broken padding, an empty and
    a ragged ciphertext: NET2_PDECODE_BAD, plen 0, and the whole buffer as it
    was before the call (in place) or d_out still all sentinel -- the verdict
    on the last block is known to the wave before any lane stores."""
    c = edge_case(src, True)
    res, out, plen = _run_edge(dev, c, in_place)
    assert (res == BAD).all(), res
    assert (plen == 0).all(), plen
    if in_place:
        assert np.array_equal(out, c.data)
    else:
        assert (out == SENTINEL).all()


# ---- 4. the two forms against each other -----------------------------------------

def _both_forms(run):
    """run() under limit 0 and under limit 2^30; the launch counts say that
    it was the lane form, then the wave form."""
    from ilias_net2_amd import cipher_burst
    outs = []
    try:
        for limit, took in ((0, "lane_launches"), (1 << 30, "wave_launches")):
            cipher_burst.limits(limit)
            before = cipher_burst.stats()
            outs.append(run())
            after = cipher_burst.stats()
            assert {k: after[k] - before[k] for k in after} == {
                "lane_launches": int(took == "lane_launches"),
                "wave_launches": int(took == "wave_launches")}
    finally:
        cipher_burst.limits(-1)
    return outs


def _compare_forms(outs, flags, offs, po, lens):
    """Codes, lengths and every output byte the header specifies: all but
    what follows a plaintext within its decrypted datagram."""
    (l_res, l_out, l_plen), (w_res, w_out, w_plen) = outs
    assert np.array_equal(l_res, w_res)
    assert np.array_equal(l_plen, w_plen)
    care = np.ones(len(l_out), dtype=bool)
    for i in np.nonzero((l_res == OK) & ((flags & ENC) != 0))[0]:
        a = int(offs[i]) + int(po[i])
        care[a + int(l_plen[i]):int(offs[i]) + int(lens[i])] = False
    bad = np.nonzero((l_out != w_out) & care)[0]
    assert len(bad) == 0, bad[:8]
    return l_res


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("n", [1000, 5123])
def test_wave_and_lane_forms_agree(dev, oracle_mod, n, in_place):
    """One burst of 1,000 mixed datagrams, idle and BAD ones included, under
    one key state with an alternate key: codes, lengths and output bytes of
    the lane form (limit 0) and of the wave form (limit 2^30) identical.
    Again with 5,123 datagrams, where a wave takes two datagrams in turn."""
    c = A.rx_case(oracle_mod, HASH6, n=n)
    res = _compare_forms(_both_forms(lambda: A._decrypt(c, dev, in_place)), c.flags,
                         c.offs, A._po(c.flags, c.hl), c.lens)
    assert np.array_equal(res, c.want_res)
    assert (res == BAD).sum() > n // 5 and (c.want_plen > 0).sum() > n // 3
    assert ((c.flags & ENC) == 0).sum() > n // 32


@pytest.mark.parametrize("in_place", [False, True])
def test_wave_and_lane_forms_agree_mc(dev, in_place):
    """The same over five connections' keys from the cipher-key table:
    NOCONN datagrams and kept codes as well."""
    c = M.rx_case(1000, 5, HASH6)
    with M._table(c, HASH6, tx=False) as tab:
        outs = _both_forms(lambda: M._decrypt_mc(dev, c, tab, in_place))
    res = _compare_forms(outs, c.flags, c.offs, c.po, c.lens)
    assert np.array_equal(res, c.want_res)
    assert {OK, BAD, NOCONN} <= set(res)


# ---- 5. the default threshold -----------------------------------------------------

class _Idle:
    """Bursts of n datagrams without PH_ENCRYPTED, all at offset 0 of one
    16-byte buffer: no cipher work, nothing written but plen, one launch."""

    def __init__(self, dev, cap):
        self.dev, self.cap = dev, cap
        z = lambda dt, *shape: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        self.data, self.offs, self.lens = z(torch.uint8, 16), z(torch.int64, cap), \
            torch.full((cap,), 8, dtype=torch.int32, device=dev)
        self.seq, self.flags, self.conn = (z(torch.int32, cap) for _ in range(3))
        self.iv, self.res = z(torch.uint8, cap, 16), z(torch.uint8, cap)

    def form(self, n, tab=None):
        """The form a burst of n takes: 'lane' or 'wave'."""
        from ilias_net2_amd import cipher_burst
        before = cipher_burst.stats()
        a = (self.data, self.offs[:n], self.lens[:n], self.seq[:n], self.flags[:n],
             self.iv[:n], self.res[:n])
        if tab is None:
            _, _, plen = cipher_burst.decrypt_burst(0, bytes(32), *a, out=self.data)
        else:
            _, _, plen = cipher_burst.decrypt_burst_mc(tab, self.conn[:n], 0, *a,
                                                       out=self.data)
        torch.cuda.synchronize()
        assert int(plen.abs().sum()) == 0 and int(self.res[:n].sum()) == 0
        after = cipher_burst.stats()
        d = {k: after[k] - before[k] for k in after}
        assert sorted(d.values()) == [0, 1], d
        return "wave" if d["wave_launches"] else "lane"


def test_default_threshold(dev):
    """At the default limit: a burst of exactly the default takes the wave
    form and one datagram more the lane form, for both calls; a burst of
    65,536 datagrams takes the lane form (of default + 1 where the default
    is not below 65,536: the measured one is 65,536 itself), and so does one
    of 1 M.  The default is found by bisection over idle bursts
    (net2_aes_burst_stats is the only witness)."""
    from ilias_net2_amd import cipher_burst
    cipher_burst.limits(-1)
    cap = 1 << 21
    idle = _Idle(dev, cap)
    if idle.form(1) == "lane":
        pytest.skip("the default is 0: the wave form is never taken")
    assert idle.form(cap) == "lane", "the default exceeds 2 M datagrams"
    lo, hi = 1, cap                     # form(lo) == wave, form(hi) == lane
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if idle.form(mid) == "wave" else (lo, mid)
    default = lo
    assert idle.form(default) == "wave" and idle.form(default + 1) == "lane"
    with cipher_burst.CipherTable(1) as tab:
        assert idle.form(default, tab) == "wave"
        assert idle.form(default + 1, tab) == "lane"
    assert idle.form(max(65536, default + 1)) == "lane"
    assert idle.form(1 << 20) == "lane"
