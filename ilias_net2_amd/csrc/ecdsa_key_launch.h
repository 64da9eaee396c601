/*
 * ecdsa_key_launch.h -- internal interface between the host unit of the
 * prepared ECDSA keys (net2_ecdsa_key.cpp) and their kernels
 * (ecdsa_key_kernels.hip).  Not installed; the public surface is
 * include/net2/ecdsa_key.h.
 */
#ifndef NET2_ECDSA_KEY_LAUNCH_H
#define NET2_ECDSA_KEY_LAUNCH_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

/*
 * One launch that writes all nkeys + 1 tables of the keytab (1 <= nkeys <=
 * NET2_ECDSA_P521_KEYTAB_MAX_KEYS), asynchronous on s; allocates nothing.
 * The arguments are net2_ecdsa_p521_keytab_prepare_dev's, already checked.
 */
hipError_t net2_launch_ecdsa_p521_keytab_build(const uint8_t *d_pub,
    size_t pub_stride, uint32_t nkeys, uint32_t *d_keytab, uint8_t *d_ok,
    hipStream_t s);

/*
 * One launch over n signatures (n > 0, at most UINT32_MAX), asynchronous on
 * s; allocates nothing.  The arguments are net2_ecdsa_p521_verify_keytab_dev's,
 * already checked.  A lane whose digest length exceeds dig_stride stores
 * verdict 0 and reads no digest.
 */
hipError_t net2_launch_ecdsa_p521_keytab_verify(const uint32_t *d_keytab,
    uint32_t nkeys, const uint32_t *d_kidx, const uint8_t *d_rs,
    const uint8_t *d_dig, size_t dig_stride, const uint32_t *d_dlens,
    uint32_t dlen, uint32_t n, uint8_t *d_valid, hipStream_t s);

#endif /* NET2_ECDSA_KEY_LAUNCH_H */
