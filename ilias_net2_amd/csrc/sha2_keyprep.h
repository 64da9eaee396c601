/*
 * sha2_keyprep.h -- what the launchers of sha2_kernels.hip compute on the host
 * before a launch: the constant pad block's schedule (PadKW) and the HMAC key
 * blocks' midstates (HMid), both passed to the kernels by value.  Host-safe as
 * sha2_consts.h is: no HIP header, no device qualifier, so a plain C++ program
 * includes it (tests/cxx/test_sha2_keyprep_host.cc).  Product code of the
 * launchers, not the test oracle.
 */
#ifndef NET2_SHA2_KEYPREP_H
#define NET2_SHA2_KEYPREP_H

#include "key_wipe.h"
#include "sha2_consts.h"

#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace net2 {
namespace dev {

/* Constant-pad schedule passed by value (kernarg -> SGPRs / LDS). */
template <class W>
struct PadKW {
	W kw[sizeof(W) == 4 ? 64 : 80];
};

struct HMid {
	/* [0] K' ^ ipad, [1] K' ^ opad as digest words (SHA-256: 8 state words;
	 * SHA-384/512: hi, lo of each 64-bit word); [2..3] the same for the
	 * alternate rx key (HMAC_BURST_RX with rx.alt) */
	uint32_t w[4][16];
};

/* ---- host-side constant pad schedule ---------------------------------- */

inline uint32_t h_ror32(uint32_t x, int n)
{
	return (x >> n) | (x << (32 - n));
}
inline uint64_t h_ror64(uint64_t x, int n)
{
	return (x >> n) | (x << (64 - n));
}

/* Pad block of a message whose length is a multiple of the block size. */
inline void pad_kw256(uint64_t bits, PadKW<uint32_t> &p)
{
	uint32_t w[64] = { 0 };
	w[0] = 0x80000000u;
	w[14] = (uint32_t)(bits >> 32);
	w[15] = (uint32_t)bits;
	for (int t = 16; t < 64; t++) {
		uint32_t s0 = h_ror32(w[t - 15], 7) ^ h_ror32(w[t - 15], 18) ^
		    (w[t - 15] >> 3);
		uint32_t s1 = h_ror32(w[t - 2], 17) ^ h_ror32(w[t - 2], 19) ^
		    (w[t - 2] >> 10);
		w[t] = w[t - 16] + s0 + w[t - 7] + s1;
	}
	for (int t = 0; t < 64; t++)
		p.kw[t] = K256[t] + w[t];
}

inline void pad_kw512(uint64_t bits, PadKW<uint64_t> &p)
{
	uint64_t w[80] = { 0 };
	w[0] = 0x8000000000000000ull;
	w[15] = bits;	/* w[14] = high 64 bits of the 128-bit count = 0 */
	for (int t = 16; t < 80; t++) {
		uint64_t s0 = h_ror64(w[t - 15], 1) ^ h_ror64(w[t - 15], 8) ^
		    (w[t - 15] >> 7);
		uint64_t s1 = h_ror64(w[t - 2], 19) ^ h_ror64(w[t - 2], 61) ^
		    (w[t - 2] >> 6);
		w[t] = w[t - 16] + s0 + w[t - 7] + s1;
	}
	for (int t = 0; t < 80; t++)
		p.kw[t] = K512[t] + w[t];
}

/*
 * The HMAC key blocks, once per launch on the host (RFC 2104 / FIPS 198-1:
 * the ipad and opad chaining values after one compression of K' ^ ipad /
 * K' ^ opad from the IV), in the word layout hmac_kernel's LDS copy takes.
 * One SHA-256 / SHA-512 compression each (FIPS 180-4 6.2.2 / 6.4.2, the
 * reference's SHA256Transform / SHA512Transform, src/sha2.c:374-445,
 * :663-734).
 */
inline void h_compress256(uint32_t st[8], const uint32_t m[16])
{
	uint32_t w[64], v[8];
	for (int t = 0; t < 16; t++)
		w[t] = m[t];
	for (int t = 16; t < 64; t++)
		w[t] = w[t - 16] + (h_ror32(w[t - 15], 7) ^ h_ror32(w[t - 15], 18) ^
		    (w[t - 15] >> 3)) + w[t - 7] + (h_ror32(w[t - 2], 17) ^
		    h_ror32(w[t - 2], 19) ^ (w[t - 2] >> 10));
	for (int i = 0; i < 8; i++)
		v[i] = st[i];
	for (int t = 0; t < 64; t++) {
		const uint32_t t1 = v[7] + (h_ror32(v[4], 6) ^ h_ror32(v[4], 11) ^
		    h_ror32(v[4], 25)) + ((v[4] & v[5]) ^ (~v[4] & v[6])) +
		    K256[t] + w[t];
		const uint32_t t2 = (h_ror32(v[0], 2) ^ h_ror32(v[0], 13) ^
		    h_ror32(v[0], 22)) + ((v[0] & v[1]) ^ (v[0] & v[2]) ^
		    (v[1] & v[2]));
		for (int i = 7; i > 0; i--)
			v[i] = v[i - 1];
		v[4] += t1;
		v[0] = t1 + t2;
	}
	for (int i = 0; i < 8; i++)
		st[i] += v[i];
}

inline void h_compress512(uint64_t st[8], const uint64_t m[16])
{
	uint64_t w[80], v[8];
	for (int t = 0; t < 16; t++)
		w[t] = m[t];
	for (int t = 16; t < 80; t++)
		w[t] = w[t - 16] + (h_ror64(w[t - 15], 1) ^ h_ror64(w[t - 15], 8) ^
		    (w[t - 15] >> 7)) + w[t - 7] + (h_ror64(w[t - 2], 19) ^
		    h_ror64(w[t - 2], 61) ^ (w[t - 2] >> 6));
	for (int i = 0; i < 8; i++)
		v[i] = st[i];
	for (int t = 0; t < 80; t++) {
		const uint64_t t1 = v[7] + (h_ror64(v[4], 14) ^ h_ror64(v[4], 18) ^
		    h_ror64(v[4], 41)) + ((v[4] & v[5]) ^ (~v[4] & v[6])) +
		    K512[t] + w[t];
		const uint64_t t2 = (h_ror64(v[0], 28) ^ h_ror64(v[0], 34) ^
		    h_ror64(v[0], 39)) + ((v[0] & v[1]) ^ (v[0] & v[2]) ^
		    (v[1] & v[2]));
		for (int i = 7; i > 0; i--)
			v[i] = v[i - 1];
		v[4] += t1;
		v[0] = t1 + t2;
	}
	for (int i = 0; i < 8; i++)
		st[i] += v[i];
}

/*
 * ipad / opad midstates of key block kb (K' zero-padded to the block, at
 * most 128 bytes) into hm->w[slot], hm->w[slot + 1].  halg: the SHA row
 * (1 SHA-256, 2 SHA-384, 3 SHA-512).
 */
inline void hmac_midstates(int halg, const uint8_t kb[128], HMid *hm,
    int slot)
{
	for (int pass = 0; pass < 2; pass++) {
		const uint8_t x = pass ? 0x5c : 0x36;
		uint32_t *o = hm->w[slot + pass];
		if (halg == 1) {
			uint32_t st[8], m[16];
			for (int i = 0; i < 8; i++)
				st[i] = IV256[i];
			for (int i = 0; i < 16; i++)
				m[i] = (uint32_t)(kb[4 * i] ^ x) << 24 |
				    (uint32_t)(kb[4 * i + 1] ^ x) << 16 |
				    (uint32_t)(kb[4 * i + 2] ^ x) << 8 |
				    (uint32_t)(kb[4 * i + 3] ^ x);
			h_compress256(st, m);
			for (int i = 0; i < 16; i++)
				o[i] = i < 8 ? st[i] : 0u;
		} else {
			uint64_t st[8], m[16];
			for (int i = 0; i < 8; i++)
				st[i] = halg == 2 ? IV384[i] : IV512[i];
			for (int i = 0; i < 16; i++) {
				uint64_t v = 0;
				for (int b = 0; b < 8; b++)
					v = v << 8 | (uint8_t)(kb[8 * i + b] ^ x);
				m[i] = v;
			}
			h_compress512(st, m);
			for (int i = 0; i < 8; i++) {
				o[2 * i] = (uint32_t)(st[i] >> 32);
				o[2 * i + 1] = (uint32_t)st[i];
			}
		}
	}
}

/*
 * A launch's midstates from its key bytes: *hm zeroed, then slots 0/1 from
 * key and -- with an alternate rx key (altkey != NULL, as long as key) --
 * slots 2/3 from altkey, each zero-padded to the block of SHA row halg.  The
 * key blocks are wiped before returning; the caller wipes *hm once its launch
 * has copied it.  False (and *hm all zero) when keylen is more than a block:
 * registry keys are at most one.
 */
inline bool hmac_key_mids(int halg, const uint8_t *key, const uint8_t *altkey,
    size_t keylen, HMid *hm)
{
	*hm = HMid{};
	if (keylen > (size_t)(halg == 1 ? 64 : 128))
		return false;
	uint8_t kb[128] = { 0 };
	memcpy(kb, key, keylen);
	hmac_midstates(halg, kb, hm, 0);
	if (altkey != nullptr) {
		memcpy(kb, altkey, keylen);	/* the same length: the padding stays */
		hmac_midstates(halg, kb, hm, 2);
	}
	key_wipe(kb, sizeof(kb));
	return true;
}

}	/* namespace dev */
}	/* namespace net2 */

#endif /* NET2_SHA2_KEYPREP_H */
