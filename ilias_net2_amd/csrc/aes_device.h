/*
 * aes_device.h -- AES-256 block primitives for the burst cipher kernels
 * (aes_kernels.hip): the cipher of the reference's "aes256" (src/enc.c:70-74,
 * AES-256-CBC), as T-table rounds over one table per direction.
 *
 * Words are big-endian (byte 0 of a block is bits 31..24 of word 0), the
 * tables those of the Rijndael reference code:
 *   Te0[x] = S[x]  . (02, 01, 01, 03)      Te1..3 = Te0 rotated right 8/16/24
 *   Td0[x] = Si[x] . (0e, 09, 0d, 0b)      Td1..3 = Td0 rotated right 8/16/24
 * so one table per direction and three v_alignbit_b32 rotates per column
 * stand in for four tables.  The last round needs the plain S-box: forward,
 * it is byte 1 of Te0[x]; inverse, it is the XOR of the four bytes of Td0[x]
 * (0e ^ 09 ^ 0d ^ 0b = 01 and the multiplication is linear), so neither
 * direction needs a second table.
 *
 * The functions are templates over a table accessor T (T(x): the table word
 * of byte x) and a round-key accessor K (K(i): word i of the 60-word
 * schedule), so the kernels plug in their LDS layout and the host-side check
 * a plain array.  Everything here is host + device code.
 */
#ifndef NET2_AES_DEVICE_H
#define NET2_AES_DEVICE_H

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define AES_HD __host__ __device__ __forceinline__
#else
#define AES_HD static inline
#endif

#define NET2_AES_ROUNDS 14			/* AES-256 */
#define NET2_AES_RKWORDS (4 * (NET2_AES_ROUNDS + 1))

/* The S-box (FIPS 197 figure 7). */
#define NET2_AES_SBOX_INIT { \
	0x63, 0x7c, 0x77, 0x7b, 0xf2, 0x6b, 0x6f, 0xc5, 0x30, 0x01, 0x67, 0x2b, 0xfe, 0xd7, 0xab, 0x76, \
	0xca, 0x82, 0xc9, 0x7d, 0xfa, 0x59, 0x47, 0xf0, 0xad, 0xd4, 0xa2, 0xaf, 0x9c, 0xa4, 0x72, 0xc0, \
	0xb7, 0xfd, 0x93, 0x26, 0x36, 0x3f, 0xf7, 0xcc, 0x34, 0xa5, 0xe5, 0xf1, 0x71, 0xd8, 0x31, 0x15, \
	0x04, 0xc7, 0x23, 0xc3, 0x18, 0x96, 0x05, 0x9a, 0x07, 0x12, 0x80, 0xe2, 0xeb, 0x27, 0xb2, 0x75, \
	0x09, 0x83, 0x2c, 0x1a, 0x1b, 0x6e, 0x5a, 0xa0, 0x52, 0x3b, 0xd6, 0xb3, 0x29, 0xe3, 0x2f, 0x84, \
	0x53, 0xd1, 0x00, 0xed, 0x20, 0xfc, 0xb1, 0x5b, 0x6a, 0xcb, 0xbe, 0x39, 0x4a, 0x4c, 0x58, 0xcf, \
	0xd0, 0xef, 0xaa, 0xfb, 0x43, 0x4d, 0x33, 0x85, 0x45, 0xf9, 0x02, 0x7f, 0x50, 0x3c, 0x9f, 0xa8, \
	0x51, 0xa3, 0x40, 0x8f, 0x92, 0x9d, 0x38, 0xf5, 0xbc, 0xb6, 0xda, 0x21, 0x10, 0xff, 0xf3, 0xd2, \
	0xcd, 0x0c, 0x13, 0xec, 0x5f, 0x97, 0x44, 0x17, 0xc4, 0xa7, 0x7e, 0x3d, 0x64, 0x5d, 0x19, 0x73, \
	0x60, 0x81, 0x4f, 0xdc, 0x22, 0x2a, 0x90, 0x88, 0x46, 0xee, 0xb8, 0x14, 0xde, 0x5e, 0x0b, 0xdb, \
	0xe0, 0x32, 0x3a, 0x0a, 0x49, 0x06, 0x24, 0x5c, 0xc2, 0xd3, 0xac, 0x62, 0x91, 0x95, 0xe4, 0x79, \
	0xe7, 0xc8, 0x37, 0x6d, 0x8d, 0xd5, 0x4e, 0xa9, 0x6c, 0x56, 0xf4, 0xea, 0x65, 0x7a, 0xae, 0x08, \
	0xba, 0x78, 0x25, 0x2e, 0x1c, 0xa6, 0xb4, 0xc6, 0xe8, 0xdd, 0x74, 0x1f, 0x4b, 0xbd, 0x8b, 0x8a, \
	0x70, 0x3e, 0xb5, 0x66, 0x48, 0x03, 0xf6, 0x0e, 0x61, 0x35, 0x57, 0xb9, 0x86, 0xc1, 0x1d, 0x9e, \
	0xe1, 0xf8, 0x98, 0x11, 0x69, 0xd9, 0x8e, 0x94, 0x9b, 0x1e, 0x87, 0xe9, 0xce, 0x55, 0x28, 0xdf, \
	0x8c, 0xa1, 0x89, 0x0d, 0xbf, 0xe6, 0x42, 0x68, 0x41, 0x99, 0x2d, 0x0f, 0xb0, 0x54, 0xbb, 0x16 }

AES_HD uint32_t aes_ror(uint32_t x, int n)
{
	return (x >> n) | (x << (32 - n));	/* one v_alignbit_b32 */
}

/* Multiplication by x in GF(2^8) mod x^8 + x^4 + x^3 + x + 1. */
AES_HD uint32_t aes_xtime(uint32_t b)
{
	return ((b << 1) ^ ((b & 0x80u) ? 0x1bu : 0u)) & 0xffu;
}

/* Te0's entry for the S-box output s. */
AES_HD uint32_t aes_te0_word(uint32_t s)
{
	const uint32_t s2 = aes_xtime(s);
	return (s2 << 24) | (s << 16) | (s << 8) | (s2 ^ s);
}

/* Td0's entry for the inverse S-box output si. */
AES_HD uint32_t aes_td0_word(uint32_t si)
{
	const uint32_t s2 = aes_xtime(si), s4 = aes_xtime(s2), s8 = aes_xtime(s4);
	return ((s8 ^ s4 ^ s2) << 24) | ((s8 ^ si) << 16) |
	    ((s8 ^ s4 ^ si) << 8) | (s8 ^ s2 ^ si);
}

/* One column of a middle round: T0[a] ^ T1[b] ^ T2[c] ^ T3[d] ^ k. */
template <class T>
AES_HD uint32_t aes_col(const T &tab, uint32_t a, uint32_t b, uint32_t c,
    uint32_t d, uint32_t k)
{
	return tab(a >> 24) ^ aes_ror(tab((b >> 16) & 0xffu), 8) ^
	    aes_ror(tab((c >> 8) & 0xffu), 16) ^ aes_ror(tab(d & 0xffu), 24) ^ k;
}

/* S[x] out of Te0[x]; Si[x] out of Td0[x] (see the head of this file). */
AES_HD uint32_t aes_sub_fwd(uint32_t te)
{
	return (te >> 8) & 0xffu;
}
AES_HD uint32_t aes_sub_inv(uint32_t td)
{
	td ^= td >> 16;
	return (td ^ (td >> 8)) & 0xffu;
}

/* One column of the last round: the substituted bytes in place, ^ k. */
template <bool INV, class T>
AES_HD uint32_t aes_last(const T &tab, uint32_t a, uint32_t b, uint32_t c,
    uint32_t d, uint32_t k)
{
	const uint32_t ta = tab(a >> 24), tb = tab((b >> 16) & 0xffu);
	const uint32_t tc = tab((c >> 8) & 0xffu), td = tab(d & 0xffu);
	if (INV)
		return ((aes_sub_inv(ta) << 24) | (aes_sub_inv(tb) << 16) |
		    (aes_sub_inv(tc) << 8) | aes_sub_inv(td)) ^ k;
	return ((aes_sub_fwd(ta) << 24) | (aes_sub_fwd(tb) << 16) |
	    (aes_sub_fwd(tc) << 8) | aes_sub_fwd(td)) ^ k;
}

/*
 * One block through the cipher (INV: the equivalent inverse cipher, under
 * the schedule aes256_dec_schedule makes).  s: the block as four big-endian
 * words, replaced by the result.  tab is Te0 (forward) or Td0 (inverse).
 */
template <bool INV, class T, class K>
AES_HD void aes_block(const T &tab, const K &rk, uint32_t (&s)[4])
{
	uint32_t s0 = s[0] ^ rk(0), s1 = s[1] ^ rk(1);
	uint32_t s2 = s[2] ^ rk(2), s3 = s[3] ^ rk(3);
#pragma unroll
	for (int r = 1; r < NET2_AES_ROUNDS; r++) {
		/* forward: ShiftRows takes column c's bytes from columns c, c+1,
		 * c+2, c+3; inverse: from c, c-1, c-2, c-3 */
		const uint32_t t0 = INV ? aes_col(tab, s0, s3, s2, s1, rk(4 * r)) :
		    aes_col(tab, s0, s1, s2, s3, rk(4 * r));
		const uint32_t t1 = INV ? aes_col(tab, s1, s0, s3, s2, rk(4 * r + 1)) :
		    aes_col(tab, s1, s2, s3, s0, rk(4 * r + 1));
		const uint32_t t2 = INV ? aes_col(tab, s2, s1, s0, s3, rk(4 * r + 2)) :
		    aes_col(tab, s2, s3, s0, s1, rk(4 * r + 2));
		const uint32_t t3 = INV ? aes_col(tab, s3, s2, s1, s0, rk(4 * r + 3)) :
		    aes_col(tab, s3, s0, s1, s2, rk(4 * r + 3));
		s0 = t0;
		s1 = t1;
		s2 = t2;
		s3 = t3;
	}
	constexpr int L = 4 * NET2_AES_ROUNDS;
	s[0] = INV ? aes_last<true>(tab, s0, s3, s2, s1, rk(L)) :
	    aes_last<false>(tab, s0, s1, s2, s3, rk(L));
	s[1] = INV ? aes_last<true>(tab, s1, s0, s3, s2, rk(L + 1)) :
	    aes_last<false>(tab, s1, s2, s3, s0, rk(L + 1));
	s[2] = INV ? aes_last<true>(tab, s2, s1, s0, s3, rk(L + 2)) :
	    aes_last<false>(tab, s2, s3, s0, s1, rk(L + 2));
	s[3] = INV ? aes_last<true>(tab, s3, s2, s1, s0, rk(L + 3)) :
	    aes_last<false>(tab, s3, s0, s1, s2, rk(L + 3));
}

/*
 * EVP's check of a decrypted last block (PKCS#7): the last byte v is 1..16
 * and the last v bytes all equal v.  Returns v, or 0 when the check fails.
 */
AES_HD uint32_t aes_pkcs7_pad(const uint32_t (&p)[4])
{
	const uint32_t v = p[3] & 0xffu;
	bool ok = v >= 1 && v <= 16;
#pragma unroll
	for (uint32_t k = 0; k < 16; k++) {
		const uint32_t b = (p[3 - k / 4] >> (8 * (k % 4))) & 0xffu;
		ok = ok && (k >= v || b == v);
	}
	return ok ? v : 0u;
}

/*
 * net2_ck_rx_key (src/conn_keys.c:447-476) for one datagram: true when it
 * takes the alternate rx key.  installed: an alternate key is there
 * (NET2_CK_RX_ALT); no_cutoff: NET2_CK_F_NO_RX_CUTOFF; fl, seq: the
 * datagram's header; rx_start: the window's cw_rx_start.  32-bit wrap-around
 * arithmetic, as the reference's.
 */
AES_HD bool aes_rx_alt(bool installed, bool no_cutoff, uint32_t fl,
    uint32_t seq, uint32_t cutoff, uint32_t rx_start)
{
	return installed && ((fl & 0x80000000u /* PH_ALTKEY */) != 0 ||
	    (!no_cutoff && seq - rx_start >= cutoff - rx_start));
}

#endif /* NET2_AES_DEVICE_H */
