/*
 * net2/ecdsa_key.h -- prepared keys for the batched ECDSA P-521 verification
 * on the MI355X (net2/ecdsa.h), in libnet2_sha2.so: prepare a public key once,
 * then verify many batches under it.
 *
 * A connection's peer signs every payload with the same one or two keys.
 * net2_ecdsa_p521_verify_dev treats each signature's key as new and walks the
 * 521 bit positions with a doubling each.  A *key table* holds the key's
 * fixed-window multiples, and the verification from it is additions of table
 * entries alone; the verdict is the same, bit for bit.  Verification only,
 * public data only: nothing here is constant-time, and nothing needs to be.
 *
 * Layout (public, so a table can be read, compared and stored).  Windows of 4
 * bits, 131 of them.  A key table is NET2_ECDSA_P521_KEYTAB_TABLE_BYTES:
 *   head, 16 bytes   u32 magic (NET2_ECDSA_P521_KEYTAB_MAGIC), u32 valid
 *                    (1 or 0), 8 reserved zero bytes
 *   entry (j, d)     j = 0..130, d = 1..15, at 16 + (j * 15 + d - 1) * 136:
 *                    the affine point d 16^j Q as x then y, each 17
 *                    little-endian u32 limbs, canonical (fully reduced below
 *                    p), so equal keys give byte-identical tables.  No entry
 *                    is infinity: the group order is prime.
 * A *keytab* for nkeys keys is nkeys + 1 key tables back to back: table 0 is
 * the base point G's, table k + 1 is key k's.  G's table travels inside the
 * keytab, so both device calls are stateless: no lazy initialisation, no
 * lock, no allocation, and both can be captured into a hipGraph.  A keytab
 * must be 8-byte aligned.
 *
 * Returns 0 or an errno, with the rules of net2/ecdsa.h (EINVAL for a NULL
 * array with n > 0, a NULL dig unless every digest is empty, a dig_stride
 * below dlen when dlens is NULL, n above UINT32_MAX; ENODEV without a gfx950
 * device; ENOMEM / EIO from the runtime), plus EINVAL for nkeys == 0, nkeys
 * above NET2_ECDSA_P521_KEYTAB_MAX_KEYS, a NULL or misaligned keytab and a
 * pub_stride below 132.  The argument checks come before the device check.
 * n == 0 returns 0 and launches nothing.  There is no CPU fallback.
 */
#ifndef NET2_ECDSA_KEY_H
#define NET2_ECDSA_KEY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef NET2_ECDSA_STREAM_T
/* hipStream_t where the HIP headers are in scope, else an opaque pointer */
#if defined(HIP_INCLUDE_HIP_HIP_RUNTIME_API_H) || defined(__HIPCC__)
#define NET2_ECDSA_STREAM_T hipStream_t
#else
#define NET2_ECDSA_STREAM_T void *
#endif
#endif

#define NET2_ECDSA_P521_KEYTAB_WINDOWS 131
#define NET2_ECDSA_P521_KEYTAB_DIGITS 15
#define NET2_ECDSA_P521_KEYTAB_HEAD_BYTES 16
#define NET2_ECDSA_P521_KEYTAB_ENTRY_BYTES 136
#define NET2_ECDSA_P521_KEYTAB_TABLE_BYTES 267256	/* 16 + 131 * 15 * 136 */
#define NET2_ECDSA_P521_KEYTAB_MAGIC 0x4b543531u
/* 2^20 keys are 280 GB of tables, more than a device holds */
#define NET2_ECDSA_P521_KEYTAB_MAX_KEYS 1048576

/* Bytes of a keytab for nkeys keys, G's table included; 0 for nkeys == 0 or
 * above NET2_ECDSA_P521_KEYTAB_MAX_KEYS (no such keytab). */
size_t net2_ecdsa_p521_keytab_bytes(size_t nkeys);

/* Device-resident, asynchronous on stream, allocates nothing.  Writes all
 * nkeys + 1 tables.  Key k is d_pub + k * pub_stride (132 bytes x || y, any
 * alignment; pub_stride >= 132).  A key with a coordinate >= p or off the
 * curve gets valid = 0 (its entries unspecified, but written inside its own
 * table only); d_ok, if not NULL, receives nkeys bytes 1 / 0. */
int net2_ecdsa_p521_keytab_prepare_dev(
    const uint8_t *d_pub, size_t pub_stride, size_t nkeys,
    void *d_keytab, uint8_t *d_ok, NET2_ECDSA_STREAM_T stream);

/* Device-resident, asynchronous on stream, allocates nothing.  Item i is
 * verified under key d_kidx[i] (NULL: key 0 for all); signatures, digests and
 * verdicts as in net2/ecdsa.h.  The verdict is what net2_ecdsa_p521_verify_dev
 * gives for that key's bytes, bit for bit; 0 as well for a kidx of nkeys or
 * more, a table whose magic or valid word is not set (G's included:
 * never-prepared memory verifies nothing) and a length beyond dig_stride. */
int net2_ecdsa_p521_verify_keytab_dev(
    const void *d_keytab, size_t nkeys, const uint32_t *d_kidx,
    const uint8_t *d_rs, const uint8_t *d_dig, size_t dig_stride,
    const uint32_t *d_dlens, uint32_t dlen,
    size_t n, uint8_t *d_valid, NET2_ECDSA_STREAM_T stream);

/* Host-memory, synchronous forms: an object that owns a device keytab, made
 * on the calling thread's selected device (net2_sha2_set_device).
 * net2_ecdsa_p521_keys_new prepares the nkeys keys at pub (host memory) and
 * waits; ok, if not NULL, receives nkeys bytes 1 / 0.
 * net2_ecdsa_p521_verify_keys runs on the device the object was made on,
 * whatever device the calling thread has selected by then, and leaves the
 * thread's device as it found it. */
struct net2_ecdsa_p521_keys;

int net2_ecdsa_p521_keys_new(
    const uint8_t *pub, size_t pub_stride, size_t nkeys,
    struct net2_ecdsa_p521_keys **out, uint8_t *ok);

void net2_ecdsa_p521_keys_free(struct net2_ecdsa_p521_keys *keys);

int net2_ecdsa_p521_verify_keys(
    const struct net2_ecdsa_p521_keys *keys, const uint32_t *kidx,
    const uint8_t *rs, const uint8_t *dig, size_t dig_stride,
    const uint32_t *dlens, uint32_t dlen,
    size_t n, uint8_t *valid);

#ifdef __cplusplus
}
#endif
#endif /* NET2_ECDSA_KEY_H */
