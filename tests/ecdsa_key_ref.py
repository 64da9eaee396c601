"""What the prepared-key tests (net2/ecdsa_key.h) need beyond ecdsa_ref.py: the
public layout of a key table, its expected entries through EC_POINT_mul, and
the window digits of a signature's two scalars, worked out in Python."""
import ecdsa_ref

WINDOWS, DIGITS = 131, 15
HEAD, ENTRY = 16, 136
TABLE = HEAD + WINDOWS * DIGITS * ENTRY
MAGIC = 0x4b543531


def entry_offset(j: int, d: int) -> int:
    """Byte offset of entry (j, d) within a key table."""
    assert 0 <= j < WINDOWS and 1 <= d <= DIGITS
    return HEAD + (j * DIGITS + d - 1) * ENTRY


def entry(pub, j: int, d: int) -> bytes:
    """d 16^j Q as the table stores it: x then y, 17 little-endian u32 limbs
    each, canonical.  pub None: the base point G."""
    k = d * 16 ** j % ecdsa_ref.order()
    x, y = ecdsa_ref.point_mul2(k) if pub is None else ecdsa_ref.point_mul2(0, pub, k)
    return x.to_bytes(68, "little") + y.to_bytes(68, "little")


def head(table: bytes):
    """(magic, valid, reserved) of a table's first 16 bytes."""
    return (int.from_bytes(table[0:4], "little"), int.from_bytes(table[4:8], "little"),
            table[8:16])


def digest_to_e(digest: bytes) -> int:
    """ECDSA_do_verify's e over P-521: the leftmost 66 bytes, and of 528 bits
    the top 521."""
    e = int.from_bytes(digest[:66], "big")
    return e >> 7 if len(digest) >= 66 else e


def scalars(r: int, s: int, digest: bytes):
    """u1 = e / s, u2 = r / s mod n."""
    n = ecdsa_ref.order()
    w = pow(s, -1, n)
    return digest_to_e(digest) * w % n, r * w % n


def digit(u: int, j: int) -> int:
    return u >> 4 * j & 15
