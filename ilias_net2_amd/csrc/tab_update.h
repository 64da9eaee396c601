/*
 * tab_update.h -- what one lane of the table-update kernels (tab_kernels.hip)
 * does with one record (net2_tab_ops.h): the keys of one connection slot
 * prepared from their raw bytes -- HMAC ipad / opad midstates for the key
 * table, AES-256 schedules for the cipher table -- and stored into the slot's
 * entry exactly as the per-slot kernels (keytab_set_kernel, sha2_hmac.h;
 * aes_tab_set_kernel, aes_kernels.hip) leave it.
 *
 * Host and device code like aes_cbc.h (AES_HD): the kernels plug in the
 * compressions of sha2_device.h and an LDS S-box, the host check
 * (tests/cxx/test_tab_ops_host.cc) h_compress256 / h_compress512 and a plain
 * array.  Needs clang (ext_vector_type); no HIP header.  An entry is handled
 * as 16-byte pieces: piece 0 the meta words, then the prepared keys.
 */
#ifndef NET2_TAB_UPDATE_H
#define NET2_TAB_UPDATE_H

#include "aes_keysched.h"
#include "aes_tab.h"
#include "net2_tab_ops.h"
#include "sha2_consts.h"

typedef uint32_t tab_u32x4 __attribute__((ext_vector_type(4)));

/* Net2KeyEnt (sha2_launch.h) in pieces: meta, rx[0..3] at 1, tx[0..1] at 17;
 * a midstate is four pieces.  tab_kernels.hip asserts the offsets. */
#define NET2_TAB_KT_PIECES 25
#define NET2_TAB_KT_MID 4

/* Zeroes a record once its lane has read it: no raw key stays in the staging. */
template <class R>
AES_HD void tab_rec_zero(R *r)
{
	tab_u32x4 *p = reinterpret_cast<tab_u32x4 *>(r);
	const tab_u32x4 z = { 0, 0, 0, 0 };
#pragma unroll
	for (unsigned i = 0; i < sizeof(R) / 16; i++)
		p[i] = z;
}

/*
 * The ipad / opad midstates of one key (RFC 2104: one compression each of
 * K' ^ ipad and K' ^ opad from the row's IV) in hmac_midstates' word layout
 * (sha2_keyprep.h), stored as eight pieces at dst.  kp: the key zero-padded to
 * 64 bytes (the rest of a 128-byte SHA-512 block is zero as well).  HALG: the
 * SHA row (1 SHA-256, 2 SHA-384, 3 SHA-512).  C::c256 / C::c512: the
 * compression, st += F(st, m) over 16 message words (it may overwrite m).
 */
template <int HALG, class C>
AES_HD void tab_key_mids(const uint8_t *kp, tab_u32x4 *dst)
{
	using namespace net2::dev;
	uint32_t kw[16];
#pragma unroll
	for (int i = 0; i < 4; i++) {
		const tab_u32x4 v = reinterpret_cast<const tab_u32x4 *>(kp)[i];
		kw[4 * i] = __builtin_bswap32(v.x);
		kw[4 * i + 1] = __builtin_bswap32(v.y);
		kw[4 * i + 2] = __builtin_bswap32(v.z);
		kw[4 * i + 3] = __builtin_bswap32(v.w);
	}
#pragma unroll
	for (int pass = 0; pass < 2; pass++) {
		tab_u32x4 *o = dst + NET2_TAB_KT_MID * pass;
		if (HALG == 1) {
			const uint32_t x = pass ? 0x5c5c5c5cu : 0x36363636u;
			uint32_t st[8], m[16];
#pragma unroll
			for (int i = 0; i < 8; i++)
				st[i] = IV256[i];
#pragma unroll
			for (int i = 0; i < 16; i++)
				m[i] = kw[i] ^ x;
			C::c256(st, m);
			o[0] = tab_u32x4{ st[0], st[1], st[2], st[3] };
			o[1] = tab_u32x4{ st[4], st[5], st[6], st[7] };
			o[2] = tab_u32x4{ 0, 0, 0, 0 };
			o[3] = tab_u32x4{ 0, 0, 0, 0 };
		} else {
			const uint64_t x = pass ? 0x5c5c5c5c5c5c5c5cull :
			    0x3636363636363636ull;
			uint64_t st[8], m[16];
#pragma unroll
			for (int i = 0; i < 8; i++)
				st[i] = HALG == 2 ? IV384[i] : IV512[i];
#pragma unroll
			for (int i = 0; i < 8; i++)
				m[i] = ((uint64_t)kw[2 * i] << 32 | kw[2 * i + 1]) ^ x;
#pragma unroll
			for (int i = 8; i < 16; i++)
				m[i] = x;
			C::c512(st, m);
#pragma unroll
			for (int j = 0; j < 4; j++)
				o[j] = tab_u32x4{ (uint32_t)(st[2 * j] >> 32),
				    (uint32_t)st[2 * j], (uint32_t)(st[2 * j + 1] >> 32),
				    (uint32_t)st[2 * j + 1] };
		}
	}
}

/*
 * One key-table record applied to its entry (q: the entry's 25 pieces), then
 * zeroed.  The three keys of a record land on consecutive runs of eight
 * pieces -- rx at 1, alternate rx at 9, tx at 17 -- so one loop prepares them;
 * without an alternate key its midstates are zeroed, as keytab_set_kernel
 * stores the zeroed half of HMid.  Meta: a CLEAR unsets every bit and leaves
 * the rest; an rx op replaces the rx bits, cutoff and rx_start and keeps the
 * tx bits; a tx op replaces the tx bits and keeps the rest.  A dead op (one a
 * later CLEAR of the same list cancelled) writes its bytes and no bit.
 */
template <int HALG, class C>
AES_HD void keytab_apply(tab_u32x4 *q, TabHashRec *r)
{
	const tab_u32x4 *hp = reinterpret_cast<const tab_u32x4 *>(&r->h);
	const tab_u32x4 h0 = hp[0], h1 = hp[1];
	const uint32_t fl = h0.y, rx_bits = h0.z, tx_bits = h0.w;
	const uint32_t cutoff = h1.x, rx_start = h1.y;
	tab_u32x4 mt = q[0];
	if ((fl & NET2_TR_CLEAR) != 0)
		mt.x = 0;
	for (int k = 0; k < 3; k++) {
		const uint32_t side = k == 2 ? NET2_TR_TX : NET2_TR_RX;
		if ((fl & side) == 0)
			continue;
		tab_u32x4 *dst = q + 1 + 2 * NET2_TAB_KT_MID * k;
		if (k == 1 && (fl & NET2_TR_RX_ALT) == 0) {
#pragma unroll
			for (int i = 0; i < 2 * NET2_TAB_KT_MID; i++)
				dst[i] = tab_u32x4{ 0, 0, 0, 0 };
		} else {
			tab_key_mids<HALG, C>(r->key[k], dst);
		}
	}
	if ((fl & NET2_TR_RX) != 0)
		mt = tab_u32x4{ (mt.x & NET2_TR_KT_TX_BITS) |
		    ((fl & NET2_TR_RX_LIVE) != 0 ? rx_bits : 0u), cutoff, rx_start, 0 };
	if ((fl & NET2_TR_TX) != 0)
		mt.x = (mt.x & NET2_TR_KT_RX_BITS) |
		    ((fl & NET2_TR_TX_LIVE) != 0 ? tx_bits : 0u);
	q[0] = mt;
	tab_rec_zero(r);
}

/* ---- the cipher table -------------------------------------------------------- */

/* Net2CipherEnt (aes_tab.h) in pieces: meta, dec[0] at 1, dec[1] at 16, enc at
 * 31; a schedule is fifteen pieces, one per round. */
#define NET2_TAB_CT_SCHED (NET2_AES_ROUNDS + 1)
static_assert(sizeof(Net2CipherEnt) == 16 * (1 + 3 * NET2_TAB_CT_SCHED) &&
    offsetof(Net2CipherEnt, dec) == 16 && offsetof(Net2CipherEnt, enc) ==
    16 * (1 + 2 * NET2_TAB_CT_SCHED), "the entry in pieces");

/* The encryption schedule of the 32-byte key at kp into e. */
template <class S>
AES_HD void tab_aes_expand(const S &sbox, const uint8_t *kp,
    uint32_t (&e)[NET2_AES_RKWORDS])
{
#pragma unroll
	for (int i = 0; i < 2; i++) {
		const tab_u32x4 v = reinterpret_cast<const tab_u32x4 *>(kp)[i];
		e[4 * i] = __builtin_bswap32(v.x);
		e[4 * i + 1] = __builtin_bswap32(v.y);
		e[4 * i + 2] = __builtin_bswap32(v.z);
		e[4 * i + 3] = __builtin_bswap32(v.w);
	}
	aes256_expand_t(sbox, e);
}

/* A key's schedule, fifteen pieces at dst: DEC the equivalent inverse
 * cipher's (aes256_dec_schedule), else the encryption schedule. */
template <bool DEC, class S>
AES_HD void tab_aes_sched(const S &sbox, const uint8_t *kp, tab_u32x4 *dst)
{
	uint32_t e[NET2_AES_RKWORDS];
	tab_aes_expand(sbox, kp, e);
#pragma unroll
	for (int r = 0; r < NET2_TAB_CT_SCHED; r++) {
		if (DEC) {
			uint32_t o[4];
			aes256_dec_round_t(e, r, o);
			dst[r] = tab_u32x4{ o[0], o[1], o[2], o[3] };
		} else {
			dst[r] = tab_u32x4{ e[4 * r], e[4 * r + 1], e[4 * r + 2],
			    e[4 * r + 3] };
		}
	}
	/* the schedule is key material: leave no copy behind (host: the stack) */
#if !defined(__HIP_DEVICE_COMPILE__)
	key_wipe(e, sizeof(e));
#endif
}

AES_HD void tab_zero_pieces(tab_u32x4 *dst, int n)
{
	for (int i = 0; i < n; i++)
		dst[i] = tab_u32x4{ 0, 0, 0, 0 };
}

/*
 * One cipher-table record applied to its entry (q: the entry's 46 pieces),
 * then zeroed: what aes_tab_fill_rx / aes_tab_fill_tx and aes_tab_set_kernel
 * leave.  A CLEAR zeroes the whole entry, so every piece no later op of the
 * record writes is zeroed; there are no dead ops here (tab_reduce drops them).
 */
template <class S>
AES_HD void ciphertab_apply(const S &sbox, tab_u32x4 *q, TabCipherRec *r)
{
	const tab_u32x4 *hp = reinterpret_cast<const tab_u32x4 *>(&r->h);
	const tab_u32x4 h0 = hp[0], h1 = hp[1];
	const uint32_t fl = h0.y;
	const bool clear = (fl & NET2_TR_CLEAR) != 0;
	tab_u32x4 mt = q[0];
	if (clear)
		mt = tab_u32x4{ 0, 0, 0, 0 };
	if ((fl & NET2_TR_RX) != 0) {
		tab_aes_sched<true>(sbox, r->key[0], q + 1);
		if ((fl & NET2_TR_RX_ALT) != 0)
			tab_aes_sched<true>(sbox, r->key[1], q + 1 + NET2_TAB_CT_SCHED);
		else
			tab_zero_pieces(q + 1 + NET2_TAB_CT_SCHED, NET2_TAB_CT_SCHED);
		mt = tab_u32x4{ (mt.x & NET2_CT_TX_BITS) | (h0.z & NET2_CT_RX_BITS),
		    h1.x, h1.y, 0 };
	} else if (clear) {
		tab_zero_pieces(q + 1, 2 * NET2_TAB_CT_SCHED);
	}
	if ((fl & NET2_TR_TX) != 0) {
		tab_aes_sched<false>(sbox, r->key[2], q + 1 + 2 * NET2_TAB_CT_SCHED);
		mt.x = (mt.x & NET2_CT_RX_BITS) | NET2_CT_TX;
	} else if (clear) {
		tab_zero_pieces(q + 1 + 2 * NET2_TAB_CT_SCHED, NET2_TAB_CT_SCHED);
	}
	q[0] = mt;
	tab_rec_zero(r);
}

#endif /* NET2_TAB_UPDATE_H */
