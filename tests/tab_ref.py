"""The entries of the two device tables (Net2KeyEnt, sha2_launch.h;
Net2CipherEnt, aes_tab.h) restated in plain Python from the standards, for the
table-update tests: FIPS 180-4 compressions for the HMAC ipad / opad midstates
(RFC 2104), the FIPS 197 key expansion and the equivalent inverse cipher's
schedule, and the meta-word rules of the per-slot calls.  Shares no code with
the library; tests/test_tab_ref.py checks it against hashlib, hmac and the
FIPS 197 vectors."""
import struct

M32, M64 = 0xffffffff, 0xffffffffffffffff


def _primes(n):
    out, x = [], 2
    while len(out) < n:
        if all(x % p for p in out):
            out.append(x)
        x += 1
    return out


def _frac_root(p, k, bits):
    """floor(frac(p^(1/k)) * 2^bits), exactly."""
    lo, hi = 0, 1 << (bits + 8)
    target = p << (k * bits)
    while lo < hi:                      # largest r with r^k <= p * 2^(k*bits)
        mid = (lo + hi + 1) >> 1
        if mid ** k <= target:
            lo = mid
        else:
            hi = mid - 1
    return lo & ((1 << bits) - 1)


K256 = [_frac_root(p, 3, 32) for p in _primes(64)]
K512 = [_frac_root(p, 3, 64) for p in _primes(80)]
IV256 = [_frac_root(p, 2, 32) for p in _primes(8)]
IV512 = [_frac_root(p, 2, 64) for p in _primes(8)]
IV384 = [_frac_root(p, 2, 64) for p in _primes(16)[8:]]


def _ror(x, n, bits):
    return ((x >> n) | (x << (bits - n))) & ((1 << bits) - 1)


def compress(st, block, wide):
    """One FIPS 180-4 compression: SHA-256 (64-byte block) or, wide, SHA-512
    (128-byte block).  Returns the new state."""
    bits, mask, rounds = (64, M64, 80) if wide else (32, M32, 64)
    K = K512 if wide else K256
    S0, S1, s0, s1 = (((28, 34, 39), (14, 18, 41), (1, 8, 7), (19, 61, 6)) if wide
                      else ((2, 13, 22), (6, 11, 25), (7, 18, 3), (17, 19, 10)))
    w = list(struct.unpack(">16" + ("Q" if wide else "I"), block))
    for t in range(16, rounds):
        a, b = w[t - 15], w[t - 2]
        w.append((w[t - 16] + (_ror(a, s0[0], bits) ^ _ror(a, s0[1], bits) ^ (a >> s0[2]))
                  + w[t - 7] + (_ror(b, s1[0], bits) ^ _ror(b, s1[1], bits) ^
                                (b >> s1[2]))) & mask)
    a, b, c, d, e, f, g, h = st
    for t in range(rounds):
        t1 = (h + (_ror(e, S1[0], bits) ^ _ror(e, S1[1], bits) ^ _ror(e, S1[2], bits))
              + ((e & f) ^ (~e & mask & g)) + K[t] + w[t]) & mask
        t2 = ((_ror(a, S0[0], bits) ^ _ror(a, S0[1], bits) ^ _ror(a, S0[2], bits))
              + ((a & b) ^ (a & c) ^ (b & c))) & mask
        a, b, c, d, e, f, g, h = (t1 + t2) & mask, a, b, c, (d + t1) & mask, e, f, g
    return [(x + y) & mask for x, y in zip(st, (a, b, c, d, e, f, g, h))]


def row_iv(row):
    """(initial state, wide) of HMAC row 4..6."""
    return {4: (IV256, False), 5: (IV384, True), 6: (IV512, True)}[row]


def midstates(row, key):
    """The ipad and opad chaining values of ``key`` under HMAC row 4..6, each
    as the 64 bytes an entry stores: 16 little-endian uint32 -- SHA-256: the 8
    state words, then zeros; SHA-384/512: hi, lo of each 64-bit word."""
    iv, wide = row_iv(row)
    block = key + bytes((128 if wide else 64) - len(key))
    out = []
    for pad in (0x36, 0x5c):
        st = compress(iv, bytes(b ^ pad for b in block), wide)
        words = ([w for x in st for w in (x >> 32, x & M32)] if wide
                 else st + [0] * 8)
        out.append(struct.pack("<16I", *words))
    return out


KT_RX, KT_TX, KT_RX_ALT, KT_RX_NOCUT, KT_RX_ENC, KT_TX_ENC = 1, 2, 4, 8, 0x10, 0x20
KT_RX_BITS, KT_TX_BITS = 0x1d, 0x22
KEY_ENT_BYTES, CIPHER_ENT_BYTES = 400, 736


class KeyEntry:
    """One slot of a key table: meta[4] | rx[4][16] | tx[2][16] (uint32)."""

    def __init__(self, row):
        self.row, self.meta = row, [0, 0, 0, 0]
        self.rx, self.tx = bytes(256), bytes(128)

    def set_rx(self, key, enc_set=False, alt_key=None, alt_no_cutoff=False,
               alt_cutoff=0, rx_start=0):
        alt = alt_key is not None
        self.rx = b"".join(midstates(self.row, key)) + (
            b"".join(midstates(self.row, alt_key)) if alt else bytes(128))
        bits = (KT_RX | (KT_RX_ENC if enc_set else 0) | (KT_RX_ALT if alt else 0) |
                (KT_RX_NOCUT if alt and alt_no_cutoff else 0))
        self.meta = [(self.meta[0] & KT_TX_BITS) | bits,
                     alt_cutoff & M32 if alt else 0, rx_start & M32 if alt else 0, 0]

    def set_tx(self, key, enc_set=False):
        self.tx = b"".join(midstates(self.row, key))
        self.meta[0] = (self.meta[0] & KT_RX_BITS) | KT_TX | (KT_TX_ENC if enc_set else 0)

    def clear(self):
        self.meta[0] = 0            # the bits alone: the rest stays

    def bytes(self):
        return struct.pack("<4I", *self.meta) + self.rx + self.tx


# ---- AES-256 (FIPS 197) ---------------------------------------------------------

def _xtime(b):
    return ((b << 1) ^ (0x1b if b & 0x80 else 0)) & 0xff


def _gmul(a, b):
    r = 0
    while b:
        if b & 1:
            r ^= a
        a, b = _xtime(a), b >> 1
    return r


def _make_sbox():
    # multiplicative inverse, then the affine map (FIPS 197 5.1.1)
    inv = [0] * 256
    for x in range(1, 256):
        if not inv[x]:
            for y in range(1, 256):
                if _gmul(x, y) == 1:
                    inv[x], inv[y] = y, x
                    break
    box = []
    for x in range(256):
        b = inv[x]
        r = b
        for s in range(1, 5):
            r ^= ((b << s) | (b >> (8 - s))) & 0xff
        box.append(r ^ 0x63)
    return box


SBOX = _make_sbox()


def _sub_word(w):
    return (SBOX[w >> 24] << 24 | SBOX[(w >> 16) & 0xff] << 16 |
            SBOX[(w >> 8) & 0xff] << 8 | SBOX[w & 0xff])


def enc_schedule(key):
    """KeyExpansion for a 32-byte key: 60 big-endian words."""
    w = list(struct.unpack(">8I", key))
    rcon = 1
    for i in range(8, 60):
        t = w[i - 1]
        if i % 8 == 0:
            t = _sub_word(((t << 8) | (t >> 24)) & M32) ^ (rcon << 24)
            rcon = _xtime(rcon)
        elif i % 8 == 4:
            t = _sub_word(t)
        w.append(w[i - 8] ^ t)
    return w


def _inv_mix(w):
    a = [(w >> s) & 0xff for s in (24, 16, 8, 0)]
    m = (0x0e, 0x0b, 0x0d, 0x09)
    out = 0
    for r in range(4):
        b = 0
        for c in range(4):
            b ^= _gmul(a[c], m[(c - r) % 4])
        out = out << 8 | b
    return out


def dec_schedule(key):
    """The equivalent inverse cipher's schedule (FIPS 197 5.3.5): the round
    keys in reverse order, InvMixColumns on all but the first and last."""
    e = enc_schedule(key)
    out = []
    for r in range(15):
        for c in range(4):
            x = e[4 * (14 - r) + c]
            out.append(_inv_mix(x) if 0 < r < 14 else x)
    return out


CT_RX, CT_TX, CT_RX_ALT, CT_RX_NOCUT = 1, 2, 4, 8


class CipherEntry:
    """One slot of a cipher table: meta[4] | dec[2][60] | enc[60] (uint32)."""

    def __init__(self):
        self.clear()

    def set_rx(self, key, hash_alg=0, alt_key=None, alt_no_cutoff=False,
               alt_cutoff=0, rx_start=0):
        alt = alt_key is not None
        self.dec = struct.pack("<60I", *dec_schedule(key)) + (
            struct.pack("<60I", *dec_schedule(alt_key)) if alt else bytes(240))
        self.meta = [(self.meta[0] & CT_TX) | CT_RX | (CT_RX_ALT if alt else 0) |
                     (CT_RX_NOCUT if alt and alt_no_cutoff else 0),
                     alt_cutoff & M32 if alt else 0, rx_start & M32 if alt else 0, 0]

    def set_tx(self, key):
        self.enc = struct.pack("<60I", *enc_schedule(key))
        self.meta[0] = (self.meta[0] & (CT_RX | CT_RX_ALT | CT_RX_NOCUT)) | CT_TX

    def clear(self):
        self.meta, self.dec, self.enc = [0, 0, 0, 0], bytes(480), bytes(240)

    def bytes(self):
        return struct.pack("<4I", *self.meta) + self.dec + self.enc


def apply_ops(entries, ops):
    """conn_burst / cipher_burst ops (kind, slot, kwargs), one by one."""
    for kind, slot, kw in ops:
        getattr(entries[slot], ("clear", "set_rx", "set_tx")[kind])(**kw)
