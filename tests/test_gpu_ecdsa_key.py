"""GPU: prepared keys for the ECDSA P-521 verification (net2/ecdsa_key.h,
ilias_net2_amd.ecdsa_key) against libcrypto (tests/ecdsa_ref.py): the tables'
entries against EC_POINT_mul in the public layout, and the verdicts of the
verification from tables against ECDSA_do_verify and against the bit-by-bit
kernel (ecdsa.verify_p521) on the same arrays.

A launch of either kernel is one wave-time, a few tens of milliseconds
whatever its size, so every test keeps to a handful of launches.
"""
import ctypes
import hashlib
import os
import random

import numpy as np
import pytest

import ecdsa_key_ref as kr
import ecdsa_ref
from ilias_net2_amd import _lib, ecdsa, ecdsa_key

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N = ecdsa_ref.order()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a GPU (HIP device not visible)")
    return torch.device("cuda:0")


def _t(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _pubs(keys):
    return np.stack([np.frombuffer(ecdsa_ref.public_key(d), dtype=np.uint8) for d in keys])


def _prepare(dev, pub):
    """(keytab, ok) of the (nkeys, 132) array of keys, in buffers filled with
    0xee beforehand: what is not written shows."""
    nkeys = pub.shape[0]
    keytab = torch.full((ecdsa_key.keytab_bytes(nkeys),), 0xee, dtype=torch.uint8,
                        device=dev)
    ok = torch.full((nkeys,), 7, dtype=torch.uint8, device=dev)
    kt, o = ecdsa_key.prepare_p521(_t(dev, pub), keytab=keytab, ok=ok)
    assert kt is keytab and o is ok
    return keytab, ok


def _table(keytab, t):
    return keytab[t * kr.TABLE:(t + 1) * kr.TABLE]


def _same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"lanes {bad[:10].tolist()}: got {got[bad[:10]].tolist()}, " \
                          f"expected {want[bad[:10]].tolist()}"


def _verify(dev, keytab, nkeys, cases, kidx=None, dig_stride=None, uniform=None):
    """One launch over cases (pub, r, s, digest, ...); returns the verdicts."""
    width = max([len(c[3]) for c in cases] + [1])
    cases5 = [c[:4] + (0,) for c in cases]
    _, rs, dig, dlens, _ = ecdsa_ref.pack(cases5, dig_stride or width)
    lens = uniform if uniform is not None else _t(dev, dlens.astype(np.int32))
    idx = None if kidx is None else _t(dev, np.asarray(kidx, dtype=np.uint32).view(np.int32))
    out = torch.full((len(cases),), 7, dtype=torch.uint8, device=dev)
    got = ecdsa_key.verify_p521_keytab(keytab, nkeys, _t(dev, rs), _t(dev, dig), lens,
                                       kidx=idx, out=out)
    assert got is out
    return got.cpu().numpy()


# The seven keys of the construction lattice: d = 1, 2, 3, n - 2, n - 1 and two
# random ones.
KEYS7 = ecdsa_ref.lattice_keys()


@pytest.fixture(scope="module")
def tab7(dev):
    pub = _pubs(KEYS7)
    keytab, ok = _prepare(dev, pub)
    assert ok.tolist() == [1] * 7
    return keytab, pub


def _signed(rng, count, keys, dlens=(64,)):
    """count valid signatures (pub, r, s, digest, key index), the keys cycling."""
    out = []
    for i in range(count):
        k = i % len(keys)
        dig = hashlib.shake_256(b"%d/%d" % (rng.getrandbits(64), i)).digest(
            dlens[i % len(dlens)])
        r, s = ecdsa_ref.sign(keys[k], dig)
        out.append((ecdsa_ref.public_key(keys[k]), r, s, dig, k))
    return out


# ---- 1. the tables ---------------------------------------------------------------

def test_tables_against_point_mul(dev, tab7):
    keytab, pub = tab7
    host = keytab.cpu().numpy().tobytes()
    assert len(host) == 8 * kr.TABLE
    tables = [host[t * kr.TABLE:(t + 1) * kr.TABLE] for t in range(8)]
    for t in tables:
        assert kr.head(t) == (kr.MAGIC, 1, bytes(8))
    # G's table and the table of d = 1 hold the same points
    assert tables[0][kr.HEAD:] == tables[1][kr.HEAD:]
    every = [(j, d) for j in range(kr.WINDOWS) for d in range(1, 16)]
    some = [(j, d) for j in (0, 1, 2, 64, 65, 129, 130) for d in range(1, 16)]
    for k in range(7):
        key = pub[k].tobytes()
        for j, d in every if k in (0, 5) else some:
            at = kr.entry_offset(j, d)
            assert tables[k + 1][at:at + kr.ENTRY] == kr.entry(key, j, d), (k, j, d)
    for j, d in some:
        at = kr.entry_offset(j, d)
        assert tables[0][at:at + kr.ENTRY] == kr.entry(None, j, d), ("G", j, d)


# ---- 2. position independence ------------------------------------------------------

def test_a_table_does_not_depend_on_its_place(dev):
    rng = random.Random(70)
    key = rng.randrange(1, N)
    others = _pubs([rng.randrange(1, N) for _ in range(70)])
    mine = _pubs([key])
    alone, ok = _prepare(dev, mine)
    assert ok.tolist() == [1]
    two, ok = _prepare(dev, np.concatenate([others[:1], mine]))
    assert ok.tolist() == [1, 1]
    pub70 = others.copy()
    for at in (0, 36, 69):
        pub70[at] = mine[0]
    many, ok = _prepare(dev, pub70)
    assert ok.tolist() == [1] * 70
    want = _table(alone, 1)
    assert int(want.to(torch.int32).sum()) != 0xee * kr.TABLE
    assert torch.equal(_table(two, 2), want)
    for at in (0, 36, 69):
        assert torch.equal(_table(many, at + 1), want), at
    for kt in (two, many):              # G's table likewise
        assert torch.equal(_table(kt, 0), _table(alone, 0))
    assert not torch.equal(_table(many, 2), want)
    # padded rows of keys at an odd address: the same tables
    wide = np.full((70, 151), 0xee, dtype=np.uint8)
    wide[:, :132] = pub70
    flat = torch.zeros(wide.size + 3, dtype=torch.uint8, device=dev)
    flat[3:] = _t(dev, wide).reshape(-1)
    again, ok = ecdsa_key.prepare_p521(flat[3:].view(70, 151))
    assert ok.tolist() == [1] * 70 and torch.equal(again, many)


# ---- 3. keys a verification refuses -------------------------------------------------

def test_rejected_keys(dev):
    rng = random.Random(3)
    ds = [rng.randrange(1, N) for _ in range(3)]
    good = _pubs(ds)
    x, y = good[1][:66].tobytes(), good[1][66:].tobytes()
    p66 = ecdsa_ref.be66(ecdsa_ref.P)
    rejects = [p66 + y, x + p66, x + y[:-1] + bytes([y[-1] ^ 1]), bytes(132)]
    rej = [np.frombuffer(b, dtype=np.uint8) for b in rejects]
    pub = np.stack([good[0], rej[0], good[1], rej[1], rej[2], good[2], rej[3]])
    keytab, ok = _prepare(dev, pub)
    assert ok.tolist() == [1, 0, 1, 0, 0, 1, 0]
    host = keytab.cpu().numpy().tobytes()
    for k, want in enumerate([1, 1, 0, 1, 0, 0, 1, 0]):
        assert kr.head(host[k * kr.TABLE:(k + 1) * kr.TABLE]) == (kr.MAGIC, want, bytes(8))
    # the neighbours' tables are those built without the rejects
    clean, ok3 = _prepare(dev, good)
    assert ok3.tolist() == [1, 1, 1]
    for t, c in ((0, 0), (1, 1), (3, 2), (6, 3)):
        assert torch.equal(_table(keytab, t), _table(clean, c)), t
    # signatures valid under the good keys: 1 there, 0 under every reject
    cases = _signed(rng, 21, ds)
    at = {0: 0, 1: 2, 2: 5}
    got = _verify(dev, keytab, 7, cases, kidx=[at[c[4]] for c in cases], uniform=64)
    _same(got, [1] * 21)
    kidx = [k for k in (1, 3, 4, 6) for _ in cases]
    _same(_verify(dev, keytab, 7, cases * 4, kidx=kidx, uniform=64), [0] * 84)


# ---- 4. the construction lattice ----------------------------------------------------

@pytest.fixture(scope="module")
def lattice():
    return ecdsa_ref.lattice()


def test_construction_lattice(dev, lattice):
    """Every (d, u1, u2) of the lattice in one launch under one keytab: valid
    signatures whose running sum meets a table entry (R = T), its negative and
    infinity.  The lattice re-rolls its two random keys per case, so the
    keytab holds every distinct key of the cases, the seven lattice keys
    first, and kidx says which."""
    index = {ecdsa_ref.public_key(d): i for i, d in enumerate(KEYS7)}
    for c in lattice:
        index.setdefault(c[0], len(index))
    assert len(index) >= 7
    pub = np.stack([np.frombuffer(k, dtype=np.uint8) for k in index])
    keytab, ok = ecdsa_key.prepare_p521(_t(dev, pub))
    assert ok.cpu().numpy().all()
    kidx = np.array([index[c[0]] for c in lattice], dtype=np.uint32)
    got = _verify(dev, keytab, len(index), lattice, kidx=kidx)
    want = np.array([c[4] for c in lattice], dtype=np.uint8)
    _same(got, want)
    assert want.sum() >= len(lattice) - 50 and (want == 0).sum() >= 20
    p, rs, dig, dlens, _ = ecdsa_ref.pack(lattice, max(len(c[3]) for c in lattice))
    bitwise = ecdsa.verify_p521(_t(dev, p), _t(dev, rs), _t(dev, dig),
                                _t(dev, dlens.astype(np.int32)))
    _same(got, bitwise.cpu().numpy())


# ---- 5. window edges ------------------------------------------------------------------

def test_window_edges(dev, tab7):
    """Scalars with a single digit, 1 or 15, in the first, second, middle and
    last windows, and u1 = 0: sums of one or two entries."""
    keytab, pub = tab7
    one = sorted({a * 16 ** j % N for j in (0, 1, 65, 129, 130) for a in (1, 15)} - {0})
    pairs = [(u1, u2) for u1 in [0] + one for u2 in one]
    which = (0, 2, 5)
    cases = ecdsa_ref.lattice([KEYS7[k] for k in which], pairs)
    assert len(cases) >= 3 * len(pairs) - 10
    pubs = [pub[k].tobytes() for k in which]
    kidx = [which[pubs.index(c[0])] for c in cases]
    got = _verify(dev, keytab, 7, cases, kidx=kidx)
    want = [c[4] for c in cases]
    _same(got, want)
    assert sum(want) >= len(cases) - 20


# ---- 6. every bit of r || s; the edges of their ranges -----------------------------------

def test_bit_flips_and_edge_scalars(dev, tab7):
    keytab, pub = tab7
    key = pub[5].tobytes()
    dig = hashlib.sha512(b"bit flips").digest()
    r, s = ecdsa_ref.sign(KEYS7[5], dig)
    cases = [(key, r, s, dig)]
    cases += [(key, r ^ 1 << bit, s, dig) for bit in range(528)]
    cases += [(key, r, s ^ 1 << bit, dig) for bit in range(528)]
    edges = [0, 1, N - 1, N, 2 ** 528 - 1]
    cases += [(key, e, s, dig) for e in edges] + [(key, r, e, dig) for e in edges]
    cases += [(key, a, b, dig) for a in edges for b in edges]
    assert len(cases) == 1 + 1056 + 35
    want = [ecdsa_ref.verify(*c) for c in cases]
    got = _verify(dev, keytab, 7, cases, kidx=[5] * len(cases), uniform=64)
    _same(got, want)
    assert want[0] == 1 and sum(want) == 1


# ---- 7. a corrupted entry is used -------------------------------------------------------

def test_a_corrupted_entry_is_used(dev, tab7):
    """One bit of entry (5, 7) flipped: exactly the signatures whose scalar has
    digit 7 in window 5 turn 0 -- u2 for the key's table, u1 for G's."""
    keytab, pub = tab7
    rng = random.Random(57)
    cases = _signed(rng, 300, [KEYS7[5]])
    digits = [[kr.digit(u, 5) for u in kr.scalars(c[1], c[2], c[3])] for c in cases]
    for table, which in ((6, 1), (0, 0)):
        hit = [d[which] == 7 for d in digits]
        assert 5 <= sum(hit) < 100
        bad = keytab.clone()
        bad[table * kr.TABLE + kr.entry_offset(5, 7) + 68 * which + 9] ^= 4
        got = _verify(dev, bad, 7, cases, kidx=[5] * 300, uniform=64)
        _same(got, [0 if h else 1 for h in hit])
    _same(_verify(dev, keytab, 7, cases, kidx=[5] * 300, uniform=64), [1] * 300)


# ---- 8. memory that was never prepared -------------------------------------------------

def test_never_prepared_memory_verifies_nothing(dev, tab7):
    keytab, pub = tab7
    rng = random.Random(8)
    cases = _signed(rng, 70, KEYS7)
    kidx = [c[4] for c in cases]
    _same(_verify(dev, keytab, 7, cases, kidx=kidx, uniform=64), [1] * 70)
    _same(_verify(dev, torch.zeros_like(keytab), 7, cases, kidx=kidx, uniform=64), [0] * 70)
    for word in (0, 4):                 # G's magic, G's valid word
        bad = keytab.clone()
        bad[word:word + 4] = 0
        _same(_verify(dev, bad, 7, cases, kidx=kidx, uniform=64), [0] * 70)
    bad = keytab.clone()                # one key's head: that key alone
    bad[3 * kr.TABLE:3 * kr.TABLE + 16] = 0
    _same(_verify(dev, bad, 7, cases, kidx=kidx, uniform=64),
          [0 if k == 2 else 1 for k in kidx])


# ---- 9. key indices and batch sizes --------------------------------------------------------

@pytest.fixture(scope="module")
def pool():
    return _signed(random.Random(9), 200, KEYS7, dlens=(32, 48, 64))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_key_indices_and_batch_sizes(dev, tab7, pool, n):
    keytab, pub = tab7
    cases = pool[200 - n:]
    kidx = np.array([c[4] for c in cases], dtype=np.uint32)
    want = np.ones(n, dtype=np.uint8)
    for i in range(0, n, 5):            # the wrong key, one past the last, the last u32
        kidx[i] = ((kidx[i] + 1) % 7, 7, 2 ** 32 - 1)[(i // 5) % 3]
        want[i] = 0
    _same(_verify(dev, keytab, 7, cases, kidx=kidx), want)
    # no indices: key 0 for all
    key0 = pub[0].tobytes()
    want0 = [ecdsa_ref.verify(key0, c[1], c[2], c[3]) for c in cases]
    _same(_verify(dev, keytab, 7, cases), want0)
    assert n < 8 or sum(want0) >= 1
    # fewer keys than the keytab holds: the rest are out of range
    got = _verify(dev, keytab, 3, cases, kidx=[c[4] for c in cases])
    _same(got, [1 if c[4] < 3 else 0 for c in cases])


# ---- 10. digests ----------------------------------------------------------------------------

def test_digests(dev, tab7):
    keytab, pub = tab7
    rng = random.Random(10)
    every = []
    for dl in (0, 1, 32, 64, 65, 66, 67, 100):
        cases = _signed(rng, 7, KEYS7, dlens=(dl,))
        if dl:                          # a flipped digest bit that counts
            c = cases[0]
            flipped = bytes([c[3][0] ^ 0x80]) + c[3][1:]
            cases.append((c[0], c[1], c[2], flipped, c[4]))
        if dl > 66:                     # ... and one beyond the 66 bytes, which does not
            c = cases[1]
            cases.append((c[0], c[1], c[2], c[3][:-1] + bytes([c[3][-1] ^ 1]), c[4]))
        every += cases
    want = [ecdsa_ref.verify(*c[:4]) for c in every]
    assert 56 <= sum(want) < len(every)
    kidx = [c[4] for c in every]
    # per-item lengths, dense rows
    _same(_verify(dev, keytab, 7, every, kidx=kidx), want)
    # a wide stride, every array at an odd byte offset
    n = len(every)
    _, rs, dig, dlens, _ = ecdsa_ref.pack([c[:4] + (0,) for c in every], 109)

    def odd(a, off):
        flat = torch.zeros(a.size + off, dtype=torch.uint8, device=dev)
        flat[off:] = _t(dev, a).reshape(-1)
        return flat[off:].view(a.shape)
    lens = _t(dev, dlens.astype(np.int32))
    idx = _t(dev, np.array(kidx, dtype=np.int32))
    got = ecdsa_key.verify_p521_keytab(keytab, 7, odd(rs, 1), odd(dig, 3), lens, kidx=idx)
    _same(got.cpu().numpy(), want)
    # a length beyond the slot: that lane alone is 0
    sl = [c for c in every if len(c[3]) == 32]
    _, rs, dig, dlens, _ = ecdsa_ref.pack([c[:4] + (0,) for c in sl], 32)
    lens = dlens.astype(np.int32)
    lens[3] = 33
    got = ecdsa_key.verify_p521_keytab(
        keytab, 7, _t(dev, rs), _t(dev, dig), _t(dev, lens),
        kidx=_t(dev, np.array([c[4] for c in sl], dtype=np.int32)))
    want = [ecdsa_ref.verify(*c[:4]) for c in sl]
    assert want[3] == 1
    want[3] = 0
    _same(got.cpu().numpy(), want)


# ---- 11. a captured graph ---------------------------------------------------------------------

def test_graph_replay(dev):
    """Prepare and verify captured into one graph, replayed after the keys,
    signatures and digests were overwritten: neither call allocates."""
    rng = random.Random(11)
    n, nkeys = 65, 3
    sets = []
    for step in (6, 4):
        ds = [rng.randrange(1, N) for _ in range(nkeys)]
        cases = _signed(rng, n, ds)
        for i in range(0, n, step):     # some of them wrong
            c = cases[i]
            cases[i] = (c[0], c[1], c[2] ^ 2, c[3], c[4])
        _, rs, dig, _, _ = ecdsa_ref.pack([c[:4] + (0,) for c in cases], 64)
        want = [ecdsa_ref.verify(*c[:4]) for c in cases]
        sets.append((_pubs(ds), rs, dig, np.array([c[4] for c in cases], np.int32), want))
    t = [_t(dev, a) for a in sets[0][:4]]
    keytab = torch.zeros((ecdsa_key.keytab_bytes(nkeys),), dtype=torch.uint8, device=dev)
    ok = torch.zeros((nkeys,), dtype=torch.uint8, device=dev)
    out = torch.full((n,), 9, dtype=torch.uint8, device=dev)

    def both():
        ecdsa_key.prepare_p521(t[0], keytab=keytab, ok=ok)
        ecdsa_key.verify_p521_keytab(keytab, nkeys, t[1], t[2], kidx=t[3], out=out)
    both()                              # warm up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    count = lambda: torch.cuda.memory_stats(dev)["allocation.all.allocated"]  # noqa: E731
    with torch.cuda.graph(g):
        before = count()        # (entering the capture allocates on its own)
        both()
        assert count() == before
    for which in (0, 1, 0):
        for dst, src in zip(t, sets[which][:4]):
            dst.copy_(torch.from_numpy(src))
        keytab.zero_()
        ok.zero_()
        out.fill_(9)
        g.replay()
        _same(out.cpu().numpy(), sets[which][4])
        assert ok.tolist() == [1] * nkeys
    assert sets[0][4] != sets[1][4]
    assert 0 < sum(sets[0][4]) < n


# ---- 12. the host-memory object and the sign layer --------------------------------------------

def test_host_memory_object(dev, tab7, pool, monkeypatch):
    keytab, pub = tab7
    cases = pool[:130]
    kidx = np.array([c[4] for c in cases], dtype=np.uint32)
    kidx[::9] = 7                       # out of range
    width = max(len(c[3]) for c in cases)
    _, rs, dig, dlens, _ = ecdsa_ref.pack([c[:4] + (0,) for c in cases], width)
    want = _verify(dev, keytab, 7, cases, kidx=kidx)
    assert 100 < want.sum() < 130
    L = _lib.lib()
    monkeypatch.setenv("NET2_SHA2_VIRTUAL_DEVICES", "3")
    prev, cur = ctypes.c_int(-9), ctypes.c_int(-9)
    assert L.net2_sha2_set_device(2, ctypes.byref(prev)) == 0
    try:
        with ecdsa_key.KeysP521(pub) as keys:
            assert keys.nkeys == 7 and keys.ok.tolist() == [1] * 7
            for sel in (2, 0, 1):       # whatever the thread selects by then
                assert L.net2_sha2_set_device(sel, None) == 0
                _same(keys.verify(rs, dig, dlens, kidx), want)
                assert L.net2_sha2_get_device(ctypes.byref(cur)) == 0 and cur.value == sel
            # one key, one length, no indices
            one = [c for c in pool if c[4] == 0 and len(c[3]) == 64][:9]
            _, rs1, dig1, _, _ = ecdsa_ref.pack([c[:4] + (0,) for c in one], 64)
            _same(keys.verify(rs1, dig1), [1] * len(one))
            assert keys.verify(rs1[:0], dig1[:0]).shape == (0,)
        bad = pub.copy()
        bad[1, 131] ^= 1
        with ecdsa_key.KeysP521(bad) as keys:
            assert keys.ok.tolist() == [1, 0, 1, 1, 1, 1, 1]
    finally:
        assert L.net2_sha2_set_device(prev.value, None) == 0


vp = ctypes.c_void_p


def _golden_pems():
    keys = os.path.join(ROOT, "tests", "golden", "keys")
    with open(os.path.join(keys, "ecdsa_p521_priv.pem"), "rb") as f:
        priv = f.read()
    with open(os.path.join(keys, "ecdsa_p521_pub.pem"), "rb") as f:
        return priv, f.read()


def test_sign_layer_prepared_context(dev):
    """valid[] of net2x_signctx_validate_batch before and after
    net2x_signctx_prepare_dev, and of a clone (which starts unprepared), on
    valid, corrupted and DER-rejected signatures: all the same, and
    ECDSA_verify's."""
    _lib.lib()
    S = ctypes.CDLL(os.path.join(ROOT, "ilias_net2_amd", "libnet2_sign.so"))
    for name in ("net2x_signctx_pubnew", "net2x_signctx_privnew"):
        getattr(S, name).restype = vp
        getattr(S, name).argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
    S.net2x_signctx_clone.restype = vp
    S.net2x_signctx_clone.argtypes = [vp]
    S.net2x_signctx_free.argtypes = [vp]
    S.net2x_signctx_prepare_dev.argtypes = [vp]
    S.net2x_signctx_sign.argtypes = [vp, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p,
                                     ctypes.POINTER(ctypes.c_size_t)]
    S.net2x_signctx_validate.argtypes = [vp, ctypes.c_char_p, ctypes.c_size_t,
                                         ctypes.c_char_p, ctypes.c_size_t]
    S.net2x_signctx_validate_batch.argtypes = [
        vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_size_t),
        ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
        ctypes.POINTER(ctypes.c_int)]
    priv_pem, pub_pem = _golden_pems()
    priv = S.net2x_signctx_privnew(0, priv_pem, len(priv_pem))
    pub = S.net2x_signctx_pubnew(0, pub_pem, len(pub_pem))
    assert priv and pub
    clone = None
    rng = random.Random(12)
    n = 90
    digs = [hashlib.sha512(b"payload %d" % i).digest() for i in range(n)]
    sigs = []
    for i, d in enumerate(digs):
        buf = ctypes.create_string_buffer(200)
        ln = ctypes.c_size_t(200)
        assert S.net2x_signctx_sign(priv, d, 64, buf, ctypes.byref(ln)) == 0
        sig = bytearray(buf.raw[:ln.value])
        if i % 5 == 1:                  # a value byte
            sig[-1 - rng.randrange(60)] ^= 1 << rng.randrange(8)
        elif i % 5 == 3:                # the DER itself
            sig = sig + b"\0" if i % 2 else sig[:-1]
        sigs.append(bytes(sig))
    for i in range(2, n, 10):           # the digests
        digs[i] = bytes([digs[i][0] ^ 1]) + digs[i][1:]

    def batch(ctx):
        ptrs = (ctypes.c_char_p * n)(*sigs)
        lens = (ctypes.c_size_t * n)(*[len(s) for s in sigs])
        valid = (ctypes.c_int * n)(*([7] * n))
        assert S.net2x_signctx_validate_batch(ctx, ptrs, lens, b"".join(digs), 64, 64, n,
                                              valid) == 0
        return list(valid)
    try:
        want = [S.net2x_signctx_validate(pub, s, len(s), d, 64) for s, d in zip(sigs, digs)]
        assert set(want) == {0, 1} and 30 < sum(want) < 70
        assert batch(pub) == want
        assert S.net2x_signctx_prepare_dev(pub) == 0
        assert S.net2x_signctx_prepare_dev(pub) == 0    # again: nothing to do
        assert batch(pub) == want
        clone = S.net2x_signctx_clone(pub)
        assert clone
        assert batch(clone) == want
        assert S.net2x_signctx_prepare_dev(priv) == 0   # a private context has the key too
        assert batch(priv) == want
    finally:
        for c in (priv, pub, clone):
            if c:
                S.net2x_signctx_free(c)
