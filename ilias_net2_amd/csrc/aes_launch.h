/*
 * aes_launch.h -- internal interface between the host units (net2_dgram.cpp)
 * and the burst cipher kernels (aes_kernels.hip).  Not installed; the public
 * surface is net2_packet_{decrypt,encrypt}_burst in include/net2/packet.h.
 */
#ifndef NET2_AES_LAUNCH_H
#define NET2_AES_LAUNCH_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#define NET2_AES_KEYLEN 32	/* AES-256 (src/enc.c:70-74) */
#define NET2_AES_BLOCK 16	/* block and IV length */

/* The alternate-key choice of net2_ck_rx_key (src/conn_keys.c:447-476) for
 * the decrypt burst; alt_key == NULL: no alternate key is installed. */
struct AesRxAlt {
	const uint8_t *alt_key;
	int no_cutoff;
	uint32_t cutoff, rx_start;
};

/*
 * Both expand the key schedules on the host and pass them by value in the
 * launch's arguments: the keys are consumed before the call returns.  One
 * lane per datagram, asynchronous on s.  Pointers other than key / alt_key
 * are device memory; seq may be NULL without an alternate key.
 */
hipError_t net2_launch_aes_decrypt(const uint8_t *key, const AesRxAlt &alt,
    uint32_t hashlen, const uint8_t *base, const uint64_t *offsets,
    const uint32_t *lens, uint64_t n, const uint32_t *seq,
    const uint32_t *flags, const uint8_t *iv, uint8_t *result, uint8_t *out,
    uint32_t *plen, hipStream_t s);
hipError_t net2_launch_aes_encrypt(const uint8_t *key, uint32_t hashlen,
    const uint32_t *flags, const uint8_t *iv, uint8_t *base,
    const uint64_t *offsets, const uint32_t *lens, const uint32_t *plen,
    uint64_t n, uint8_t *result, uint32_t *wire_len, hipStream_t s);

#endif /* NET2_AES_LAUNCH_H */
