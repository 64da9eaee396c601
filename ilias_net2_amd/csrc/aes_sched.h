/*
 * aes_sched.h -- the host side of the burst cipher (aes_kernels.hip): the
 * S-box tables worked out at compile time and the AES-256 key schedules
 * (FIPS 197 5.2, 5.3.5) that the launches pass to the kernels.
 *
 * Host code only, plain C++17: aes_kernels.hip includes it, and so does the
 * host check of the block code (tests/cxx/test_aes_host.cc), which runs the
 * cipher of aes_device.h under these schedules without a GPU.  Everything
 * has internal linkage (the anonymous namespace the definitions had inside
 * aes_kernels.hip), so each includer gets its own copy.
 */
#ifndef NET2_AES_SCHED_H
#define NET2_AES_SCHED_H

#include "aes_device.h"

namespace {

/* The S-box and (INV) its inverse, worked out at compile time. */
struct Sbox {
	uint8_t v[256];
};
constexpr Sbox make_sbox(bool inv)
{
	constexpr uint8_t s[256] = NET2_AES_SBOX_INIT;
	Sbox r = {};
	for (int x = 0; x < 256; x++)
		r.v[inv ? s[x] : x] = (uint8_t)(inv ? x : s[x]);
	return r;
}
constexpr Sbox h_sbox = make_sbox(false);

struct AesSched {
	uint32_t w[NET2_AES_RKWORDS];
};

/* ---- the key schedules (FIPS 197 5.2, 5.3.5) -------------------------------- */

uint32_t sub_word(uint32_t w)
{
	return (uint32_t)h_sbox.v[w >> 24] << 24 |
	    (uint32_t)h_sbox.v[(w >> 16) & 0xff] << 16 |
	    (uint32_t)h_sbox.v[(w >> 8) & 0xff] << 8 | h_sbox.v[w & 0xff];
}

void aes256_enc_schedule(const uint8_t *key, AesSched *ks)
{
	uint32_t *w = ks->w;
	uint32_t rcon = 1;
	for (int i = 0; i < 8; i++)
		w[i] = (uint32_t)key[4 * i] << 24 | (uint32_t)key[4 * i + 1] << 16 |
		    (uint32_t)key[4 * i + 2] << 8 | key[4 * i + 3];
	for (int i = 8; i < NET2_AES_RKWORDS; i++) {
		uint32_t t = w[i - 1];
		if (i % 8 == 0) {
			t = sub_word(t << 8 | t >> 24) ^ rcon << 24;
			rcon = aes_xtime(rcon);
		} else if (i % 8 == 4) {
			t = sub_word(t);
		}
		w[i] = w[i - 8] ^ t;
	}
}

/* The equivalent inverse cipher's schedule: the rounds' keys in reverse
 * order, InvMixColumns applied to all but the first and last. */
void aes256_dec_schedule(const uint8_t *key, AesSched *ks)
{
	AesSched e;
	aes256_enc_schedule(key, &e);
	for (int r = 0; r <= NET2_AES_ROUNDS; r++) {
		for (int c = 0; c < 4; c++) {
			uint32_t x = e.w[4 * (NET2_AES_ROUNDS - r) + c];
			if (r != 0 && r != NET2_AES_ROUNDS)
				x = aes_td0_word(x >> 24) ^
				    aes_ror(aes_td0_word((x >> 16) & 0xff), 8) ^
				    aes_ror(aes_td0_word((x >> 8) & 0xff), 16) ^
				    aes_ror(aes_td0_word(x & 0xff), 24);
			ks->w[4 * r + c] = x;
		}
	}
	/* the schedule is key material: leave no copy on the stack */
	volatile uint32_t *z = e.w;
	for (int i = 0; i < NET2_AES_RKWORDS; i++)
		z[i] = 0;
}

}	/* namespace */

#endif /* NET2_AES_SCHED_H */
