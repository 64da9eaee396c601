/*
 * net2/ecdsa.h -- batched ECDSA signature verification over secp521r1
 * (NIST P-521) on the MI355X, in libnet2_sha2.so.
 *
 * The signed-payload path verifies a whole tick of signatures at once
 * (net2/signed_carver.h); its hash step runs on the device, and these calls
 * put the verification there too: one lane per signature, the accept/reject
 * answer that of OpenSSL's ECDSA_do_verify bit for bit.  Verification only:
 * it touches public data.  Signing stays on the host.
 *
 * Item i of a batch:
 *   public key  pub + i * pub_stride   132 bytes, x || y big-endian;
 *                                      pub_stride 0: one key for all
 *   signature   rs + i * 132           r || s, 66-byte big-endian values
 *   digest      dig + i * dig_stride   dlens[i] bytes, or dlen when dlens
 *                                      is NULL; any length, 0 included
 *   verdict     valid[i]               1 or 0
 * No alignment is required of any of them.  The verdict is 0 unless
 * 1 <= r, s <= n - 1, the key's coordinates are below p and on the curve,
 * and x(u1 G + u2 Q) mod n = r with e the digest's leftmost 66 bytes (shifted
 * right by 7 bits when there are 66), as OpenSSL forms it.
 *
 * Returns 0 or an errno: EINVAL for a NULL pub, rs or valid with n > 0, a
 * NULL dig unless every digest is empty (dlens NULL and dlen 0), a
 * dig_stride below dlen (dlens NULL), a pub_stride between 1 and 131, or
 * n above UINT32_MAX; ENODEV without a gfx950 device; ENOMEM / EIO from the
 * runtime (net2_sha2_last_hip_error).  n == 0 returns 0 and launches nothing.
 * With dlens, an item whose length exceeds dig_stride gets verdict 0.  There
 * is no CPU fallback.
 */
#ifndef NET2_ECDSA_H
#define NET2_ECDSA_H

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

#define NET2_ECDSA_P521_PUB_BYTES 132
#define NET2_ECDSA_P521_SIG_BYTES 132

/* Device-resident, asynchronous on `stream`, allocates nothing (capturable
 * into a hipGraph). */
int net2_ecdsa_p521_verify_dev(
    const uint8_t *d_pub, size_t pub_stride,
    const uint8_t *d_rs, const uint8_t *d_dig, size_t dig_stride,
    const uint32_t *d_dlens, uint32_t dlen,
    size_t n, uint8_t *d_valid, NET2_ECDSA_STREAM_T stream);

/* The same from host memory, synchronous, on the calling thread's selected
 * device (net2_sha2_set_device). */
int net2_ecdsa_p521_verify(
    const uint8_t *pub, size_t pub_stride,
    const uint8_t *rs, const uint8_t *dig, size_t dig_stride,
    const uint32_t *dlens, uint32_t dlen,
    size_t n, uint8_t *valid);

#ifdef __cplusplus
}
#endif
#endif /* NET2_ECDSA_H */
