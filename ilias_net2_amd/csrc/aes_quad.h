/*
 * aes_quad.h -- the schedule of the quad form of the burst cipher's TX encrypt
 * (aes_cbc_encrypt_quad_kernel, aes_kernels.hip): four adjacent lanes per
 * datagram, one column of the AES state each.  CBC encryption is serial from
 * block to block, but not inside a block: a T-table round computes four
 * independent columns, column q from one byte each of columns q, q + 1, q + 2
 * and q + 3 of the state before it (aes_block, aes_device.h).  So lane q of a
 * quad keeps column q, fetches the other three from its neighbours once per
 * round, and the serial chain per block is four look-ups a round instead of
 * sixteen.
 *
 * The schedule, for the quad of lanes 4 d .. 4 d + 3 and its datagram:
 *
 *   - lane l holds column q = l mod 4, as one big-endian word: bytes 4 q ..
 *     4 q + 3 of the block, byte 4 q in bits 31..24.
 *   - of the 60-word key schedule lane q owns words 4 r + q, r = 0 .. 14: its
 *     column of every round key, fifteen words that it keeps for all blocks.
 *   - the k-th input of lane q's column (k = 1, 2, 3) is the column of lane
 *     (q + k) mod 4 of the same quad; every lane of the quad takes part in
 *     every exchange, so whatever decides how often a quad exchanges -- its
 *     block count -- is the same in its four lanes.
 *   - block j of the padded plaintext, lane q: dword q of the block, a 4-byte
 *     access at byte alignment; in the last block the plaintext bytes below
 *     plen and the PKCS#7 value 16 - plen mod 16 in every byte from there on
 *     (a full block of 16s when plen is a multiple of 16).  Bytes of the slot
 *     at or past plen are never read.
 *   - one block of the chain: enter (chain ^ word ^ round key 0), rounds 1 ..
 *     13 (exchange, then aes_col), round 14 (exchange, then aes_last); the
 *     result is the lane's ciphertext word, stored as dword q of block j, and
 *     its chain word for block j + 1.  The chain starts as dword q of the IV.
 *
 * No HIP header: the kernel includes it, and so does the host model of a quad
 * (tests/cxx/test_aes_quad_host.cc), which steps four lanes in lockstep over
 * these pieces.  Host and device code, as aes_device.h (AES_HD).
 */
#ifndef NET2_AES_QUAD_H
#define NET2_AES_QUAD_H

#include "aes_device.h"

#define NET2_AES_QUAD_LANES 4u
#define NET2_AES_QUAD_KEYWORDS (NET2_AES_ROUNDS + 1)	/* schedule words a lane owns */

/* The column lane l holds, and its quad among its wave's or workgroup's. */
constexpr uint32_t aes_quad_col(uint32_t l)
{
	return l % NET2_AES_QUAD_LANES;
}
constexpr uint32_t aes_quad_of(uint32_t l)
{
	return l / NET2_AES_QUAD_LANES;
}

/* The schedule word that lane q adds in round r (0: on entry), r = 0 .. 14. */
constexpr int aes_quad_rk(int r, uint32_t q)
{
	return 4 * r + (int)q;
}

/* The lane of the quad whose column is the k-th input of lane q's, k = 0 .. 3. */
constexpr uint32_t aes_quad_src(uint32_t q, uint32_t k)
{
	return (q + k) % NET2_AES_QUAD_LANES;
}

/* Dword q of a 16-byte block at any byte alignment <-> a big-endian word. */
AES_HD uint32_t aes_quad_ld(const uint8_t *blk, uint32_t q)
{
	uint32_t v;
	__builtin_memcpy(&v, blk + 4 * q, 4);
	return __builtin_bswap32(v);
}

AES_HD void aes_quad_st(uint8_t *blk, uint32_t q, uint32_t w)
{
	const uint32_t v = __builtin_bswap32(w);
	__builtin_memcpy(blk + 4 * q, &v, 4);
}

/*
 * The word lane q contributes for block j of the nb-block padded plaintext
 * of plen bytes at p (nb = plen / 16 + 1, j < nb): see the head of this file.
 */
AES_HD uint32_t aes_quad_word(const uint8_t *p, uint32_t plen, uint32_t nb,
    uint32_t j, uint32_t q)
{
	const uint8_t *blk = p + 16 * (uint64_t)j;
	if (j + 1 < nb)
		return aes_quad_ld(blk, q);
	const uint32_t rem = plen & 15u;
	uint32_t w = 0;
#pragma unroll
	for (uint32_t k = 0; k < 4; k++) {
		const uint32_t at = 4 * q + k;
		const uint32_t v = at < rem ? blk[at] : 16u - rem;
		w |= v << (24 - 8 * k);
	}
	return w;
}

/* A block's first step: the chain word, the plaintext word, round key 0. */
AES_HD uint32_t aes_quad_enter(uint32_t chain, uint32_t word, uint32_t k0)
{
	return chain ^ word ^ k0;
}

/*
 * Round r (1 .. 14) of lane q's column: s the lane's own column, s1, s2, s3
 * those of lanes aes_quad_src(q, 1 .. 3), all as they were after round r - 1;
 * k the lane's schedule word aes_quad_rk(r, q).  tab is Te0.
 */
template <class T>
AES_HD uint32_t aes_quad_round(const T &tab, int r, uint32_t s, uint32_t s1,
    uint32_t s2, uint32_t s3, uint32_t k)
{
	return r < NET2_AES_ROUNDS ? aes_col(tab, s, s1, s2, s3, k) :
	    aes_last<false>(tab, s, s1, s2, s3, k);
}

#endif /* NET2_AES_QUAD_H */
