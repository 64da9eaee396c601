/*
 * aes_keysched.h -- the AES-256 key schedules (FIPS 197 5.2, 5.3.5) as host +
 * device templates over an S-box accessor S (S(x): the S-box byte of x), so
 * the table-update kernels (tab_kernels.hip) expand a connection's keys on the
 * device from an LDS copy of the S-box and the host check
 * (tests/cxx/test_tab_ops_host.cc) runs the very same code over a plain array.
 * The results are those of aes_sched.h's aes256_enc_schedule /
 * aes256_dec_schedule, word for word; that header keeps its own host-only
 * statement, which the burst launchers and their object are built from.
 *
 * Every loop is fully unrolled and every array index a constant after
 * unrolling: a per-lane array indexed at run time would go to scratch.
 */
#ifndef NET2_AES_KEYSCHED_H
#define NET2_AES_KEYSCHED_H

#include "aes_device.h"

/* SubWord (FIPS 197 5.2) through the accessor. */
template <class S>
AES_HD uint32_t aes_sub_word_t(const S &sbox, uint32_t w)
{
	return (uint32_t)sbox(w >> 24) << 24 | (uint32_t)sbox((w >> 16) & 0xffu) << 16 |
	    (uint32_t)sbox((w >> 8) & 0xffu) << 8 | (uint32_t)sbox(w & 0xffu);
}

/*
 * The encryption schedule: w[0..7] hold the key as big-endian words, w[8..59]
 * are filled in.
 */
template <class S>
AES_HD void aes256_expand_t(const S &sbox, uint32_t (&w)[NET2_AES_RKWORDS])
{
	uint32_t rcon = 1;
#pragma unroll
	for (int i = 8; i < NET2_AES_RKWORDS; i++) {
		uint32_t t = w[i - 1];
		if (i % 8 == 0) {
			t = aes_sub_word_t(sbox, t << 8 | t >> 24) ^ rcon << 24;
			rcon = aes_xtime(rcon);
		} else if (i % 8 == 4) {
			t = aes_sub_word_t(sbox, t);
		}
		w[i] = w[i - 8] ^ t;
	}
}

/* InvMixColumns of one column; needs no table (aes_td0_word). */
AES_HD uint32_t aes_inv_mix_word(uint32_t x)
{
	return aes_td0_word(x >> 24) ^ aes_ror(aes_td0_word((x >> 16) & 0xffu), 8) ^
	    aes_ror(aes_td0_word((x >> 8) & 0xffu), 16) ^
	    aes_ror(aes_td0_word(x & 0xffu), 24);
}

/*
 * Round r (0..14) of the equivalent inverse cipher's schedule out of the
 * encryption schedule e: the rounds' keys in reverse order, InvMixColumns
 * applied to all but the first and last.  r is a constant where this is
 * called from an unrolled loop.
 */
AES_HD void aes256_dec_round_t(const uint32_t (&e)[NET2_AES_RKWORDS], int r,
    uint32_t (&o)[4])
{
#pragma unroll
	for (int c = 0; c < 4; c++) {
		const uint32_t x = e[4 * (NET2_AES_ROUNDS - r) + c];
		o[c] = r != 0 && r != NET2_AES_ROUNDS ? aes_inv_mix_word(x) : x;
	}
}

#endif /* NET2_AES_KEYSCHED_H */
