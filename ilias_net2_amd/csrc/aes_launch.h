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

/*
 * The device cipher-key table (struct net2_burst_ciphertab): entries of
 * NET2_AES_TAB_ENT_BYTES each (Net2CipherEnt, aes_tab.h), 16-byte aligned.
 */
struct Net2CipherEnt;
#define NET2_AES_TAB_ENT_BYTES 736
#define NET2_AES_TAB_RX 1u	/* the sides of an update; 0 clears the slot */
#define NET2_AES_TAB_TX 2u

/*
 * One slot's update: the new entry is made on the host (schedules expanded
 * from key / alt_key, 32 bytes each, alt_key NULL without an alternate key)
 * and travels in the launch's arguments, so the keys are consumed before the
 * call returns and the update is ordered with the work on s.  side
 * NET2_AES_TAB_RX: the rx side, the tx side stays; NET2_AES_TAB_TX: the tx side
 * from key, the rx side stays; 0: the whole entry zeroed.
 */
hipError_t net2_launch_aes_tab_set(Net2CipherEnt *ents, uint32_t slot,
    uint32_t side, const uint8_t *key, const uint8_t *alt_key, int no_cutoff,
    uint32_t cutoff, uint32_t rx_start, hipStream_t s);

/* Where the _mc launches find datagram i's keys: slot conn[i] of tab. */
struct AesTabArgs {
	const uint32_t *conn;
	const Net2CipherEnt *tab;
	uint32_t slots;
};

/*
 * net2_launch_aes_decrypt / _encrypt under the keys of each datagram's own
 * slot.  A datagram with cipher work whose slot is out of range or has no
 * rx / tx side gets code 5 (NET2_PBURST_NOCONN) and is left untouched.
 */
hipError_t net2_launch_aes_decrypt_mc(const AesTabArgs &kt, uint32_t hashlen,
    const uint8_t *base, const uint64_t *offsets, const uint32_t *lens,
    uint64_t n, const uint32_t *seq, const uint32_t *flags, const uint8_t *iv,
    uint8_t *result, uint8_t *out, uint32_t *plen, hipStream_t s);
hipError_t net2_launch_aes_encrypt_mc(const AesTabArgs &kt, uint32_t hashlen,
    const uint32_t *flags, const uint8_t *iv, uint8_t *base,
    const uint64_t *offsets, const uint32_t *lens, const uint32_t *plen,
    uint64_t n, uint8_t *result, uint32_t *wire_len, hipStream_t s);

/*
 * The wave form of the two decrypt launches, for small bursts: one wave per
 * datagram, its blocks spread over the lanes (aes_wave.h), in place of one
 * lane per datagram.  Same arguments, same codes, lengths and output bytes;
 * which form a call takes is net2_dgram.cpp's choice (net2_aes_burst_limits).
 */
hipError_t net2_launch_aes_decrypt_wave(const uint8_t *key, const AesRxAlt &alt,
    uint32_t hashlen, const uint8_t *base, const uint64_t *offsets,
    const uint32_t *lens, uint64_t n, const uint32_t *seq,
    const uint32_t *flags, const uint8_t *iv, uint8_t *result, uint8_t *out,
    uint32_t *plen, hipStream_t s);
hipError_t net2_launch_aes_decrypt_mc_wave(const AesTabArgs &kt,
    uint32_t hashlen, const uint8_t *base, const uint64_t *offsets,
    const uint32_t *lens, uint64_t n, const uint32_t *seq,
    const uint32_t *flags, const uint8_t *iv, uint8_t *result, uint8_t *out,
    uint32_t *plen, hipStream_t s);

/*
 * The quad form of the two encrypt launches, for small bursts: four lanes per
 * datagram, one column of the state each (aes_quad.h), in place of one lane
 * per datagram.  Same arguments, same codes, lengths and output bytes; which
 * form a call takes is net2_dgram.cpp's choice (net2_aes_encrypt_limits).
 */
hipError_t net2_launch_aes_encrypt_quad(const uint8_t *key, uint32_t hashlen,
    const uint32_t *flags, const uint8_t *iv, uint8_t *base,
    const uint64_t *offsets, const uint32_t *lens, const uint32_t *plen,
    uint64_t n, uint8_t *result, uint32_t *wire_len, hipStream_t s);
hipError_t net2_launch_aes_encrypt_mc_quad(const AesTabArgs &kt,
    uint32_t hashlen, const uint32_t *flags, const uint8_t *iv, uint8_t *base,
    const uint64_t *offsets, const uint32_t *lens, const uint32_t *plen,
    uint64_t n, uint8_t *result, uint32_t *wire_len, hipStream_t s);

#endif /* NET2_AES_LAUNCH_H */
