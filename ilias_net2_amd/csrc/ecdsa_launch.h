/*
 * ecdsa_launch.h -- internal interface between the host unit of the batched
 * ECDSA verification (net2_ecdsa.cpp) and its kernel (ecdsa_kernels.hip).
 * Not installed; the public surface is include/net2/ecdsa.h.
 */
#ifndef NET2_ECDSA_LAUNCH_H
#define NET2_ECDSA_LAUNCH_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

/*
 * One launch over n signatures (n > 0, at most UINT32_MAX), asynchronous on
 * s; allocates nothing.  The arguments are net2_ecdsa_p521_verify_dev's
 * (include/net2/ecdsa.h), already checked.  A lane whose digest length
 * exceeds dig_stride stores verdict 0 and reads no digest.
 */
hipError_t net2_launch_ecdsa_p521_verify(const uint8_t *d_pub, size_t pub_stride,
    const uint8_t *d_rs, const uint8_t *d_dig, size_t dig_stride,
    const uint32_t *d_dlens, uint32_t dlen, uint32_t n, uint8_t *d_valid,
    hipStream_t s);

#endif /* NET2_ECDSA_LAUNCH_H */
