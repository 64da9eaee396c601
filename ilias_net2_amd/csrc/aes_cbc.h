/*
 * aes_cbc.h -- what one lane of the burst cipher does with one datagram
 * (aes_kernels.hip): the arguments of a burst, the prep step that settles
 * what needs no cipher work, and the CBC chain of each direction, stated once
 * for every key source.  The lane kernels call these with their LDS table and
 * their round keys plugged in (the accessors of aes_device.h); the wave form
 * shares the arguments, the prep steps and the key pick.
 *
 * Host and device code like aes_device.h (AES_HD), so the host check
 * (tests/cxx/test_aes_host.cc, test_aes_tab_host.cc) runs these very
 * functions over exact-size heap buffers with a plain table and a plain
 * schedule.  Needs clang (ext_vector_type); everything has internal linkage,
 * as in aes_sched.h.
 */
#ifndef NET2_AES_CBC_H
#define NET2_AES_CBC_H

#include "aes_device.h"
#include "aes_tab.h"

namespace {

constexpr uint32_t PKT_HDR = 8;			/* net2_ph_overhead */
constexpr uint32_t PKT_PH_ENCRYPTED = 0x00000001u;
constexpr uint32_t PKT_PH_SIGNED = 0x00000002u;
constexpr uint8_t PKT_OK = 0, PKT_RESOURCE = 1, PKT_BAD = 2;
constexpr uint8_t PKT_NOCONN = 5;	/* NET2_PBURST_NOCONN */

struct AesBurstArgs {
	const uint8_t *in;	/* decrypt: the burst; encrypt: unused */
	uint8_t *out;		/* decrypt: d_out; encrypt: the burst */
	const uint64_t *offsets;
	const uint32_t *lens;
	const uint32_t *seq;	/* decrypt with an alternate key */
	const uint32_t *flags;
	const uint8_t *iv;	/* 16 bytes per datagram */
	uint8_t *result;
	uint32_t *plen;		/* decrypt: out; encrypt: in */
	uint32_t *wire_len;	/* encrypt */
	uint64_t n;
	uint32_t hashlen;
	uint32_t no_cutoff, cutoff, rx_start;
};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

/* A block at any byte alignment <-> four big-endian words. */
AES_HD void ld16(const uint8_t *p, uint32_t (&w)[4])
{
	u32x4 v;
	__builtin_memcpy(&v, p, 16);
	w[0] = __builtin_bswap32(v.x);
	w[1] = __builtin_bswap32(v.y);
	w[2] = __builtin_bswap32(v.z);
	w[3] = __builtin_bswap32(v.w);
}

AES_HD void st16(uint8_t *p, const uint32_t (&w)[4])
{
	u32x4 v;
	v.x = __builtin_bswap32(w[0]);
	v.y = __builtin_bswap32(w[1]);
	v.z = __builtin_bswap32(w[2]);
	v.w = __builtin_bswap32(w[3]);
	__builtin_memcpy(p, &v, 16);
}

AES_HD uint32_t payload_at(uint32_t fl, uint32_t hashlen)
{
	return PKT_HDR + ((fl & PKT_PH_SIGNED) != 0 ? hashlen : 0u);
}

/*
 * RX.  Only a datagram that arrives OK with PH_ENCRYPTED is decrypted; every
 * other one keeps its code, gets plen 0 and is not touched.  The last block
 * goes first: its padding decides whether the datagram is BAD (as is an empty
 * or ragged ciphertext), and a BAD datagram is not written at all.  Then the
 * blocks in order, the next one's ciphertext loaded before the current one is
 * decrypted; in place, a block is overwritten only after it and its
 * predecessor's ciphertext are in registers.
 */

/* Datagram i's ciphertext blocks; what needs no cipher is settled here. */
AES_HD uint32_t decrypt_prep(const AesBurstArgs &a, uint64_t i)
{
	if (i >= a.n)
		return 0;
	const uint32_t fl = a.flags[i];
	uint32_t nb = 0;
	if (a.result[i] == PKT_OK && (fl & PKT_PH_ENCRYPTED) != 0) {
		const uint32_t po = payload_at(fl, a.hashlen);
		const uint32_t len = a.lens[i];
		const uint32_t clen = len > po ? len - po : 0u;
		if (clen != 0 && (clen & 15u) == 0)
			nb = clen >> 4;
		else
			a.result[i] = PKT_BAD;
	}
	if (nb == 0)
		a.plen[i] = 0;
	return nb;
}

/* Datagram i (flags fl), nb >= 1 blocks as decrypt_prep counted them, under
 * table T (Td0) and round keys rk (aes256_dec_schedule). */
template <class T, class K>
AES_HD void cbc_decrypt_lane(const AesBurstArgs &a, uint64_t i, uint32_t nb,
    uint32_t fl, const T &tab, const K &rk)
{
	const uint64_t off = a.offsets[i] + payload_at(fl, a.hashlen);
	const uint8_t *src = a.in + off;
	uint8_t *dst = a.out + off;
	uint32_t ivw[4], c[4], prev[4];
	uint32_t b = nb - 1, pad = 0;

	ld16(a.iv + 16 * i, ivw);
	ld16(src + 16 * (uint64_t)b, c);
	if (nb > 1) {
		ld16(src + 16 * (uint64_t)(b - 1), prev);
	} else {
#pragma unroll
		for (int k = 0; k < 4; k++)
			prev[k] = ivw[k];
	}
	for (uint32_t j = 0; j < nb; j++) {
		const uint32_t bn = j == 0 ? 0u : b + 1;
		uint32_t cn[4] = { 0, 0, 0, 0 };
		if (j + 1 < nb)
			ld16(src + 16 * (uint64_t)bn, cn);
		uint32_t x[4] = { c[0], c[1], c[2], c[3] };
		aes_block<true>(tab, rk, x);
#pragma unroll
		for (int k = 0; k < 4; k++)
			x[k] ^= prev[k];
		if (j == 0) {
			pad = aes_pkcs7_pad(x);
			if (pad == 0)
				break;
		}
		st16(dst + 16 * (uint64_t)b, x);
#pragma unroll
		for (int k = 0; k < 4; k++) {
			prev[k] = j == 0 ? ivw[k] : c[k];
			c[k] = cn[k];
		}
		b = bn;
	}
	if (pad == 0)
		a.result[i] = PKT_BAD;
	a.plen[i] = pad != 0 ? 16 * nb - pad : 0u;
}

/*
 * TX.  Slot i holds plen[i] plaintext bytes at its payload offset.  With
 * PH_ENCRYPTED they are encrypted in place into 16 * (plen / 16 + 1) bytes
 * (EVP always pads); a slot without the room is RESOURCE and untouched.
 * The next block's plaintext is loaded before the current one goes through
 * the chain; the last, partial block is read bytewise and padded.
 */

/* Slot i's blocks to encrypt; what needs no cipher is settled here. */
AES_HD uint32_t encrypt_prep(const AesBurstArgs &a, uint64_t i)
{
	if (i >= a.n)
		return 0;
	const uint32_t fl = a.flags[i];
	const uint32_t pl = a.plen[i];
	const uint32_t len = a.lens[i];
	const uint32_t po = payload_at(fl, a.hashlen);
	if ((fl & PKT_PH_ENCRYPTED) == 0) {
		const uint64_t wl = (uint64_t)po + pl;
		a.wire_len[i] = (uint32_t)wl;
		a.result[i] = wl > len ? PKT_RESOURCE : PKT_OK;
		return 0;
	}
	const uint64_t clen = 16 * ((uint64_t)pl / 16 + 1);
	const bool room = po + clen <= len;
	a.wire_len[i] = room ? po + (uint32_t)clen : 0u;
	a.result[i] = room ? PKT_OK : PKT_RESOURCE;
	return room ? (uint32_t)(clen >> 4) : 0u;
}

/* Slot i, nb >= 1 blocks as encrypt_prep counted them, under table T (Te0)
 * and round keys rk (aes256_enc_schedule). */
template <class T, class K>
AES_HD void cbc_encrypt_lane(const AesBurstArgs &a, uint64_t i, uint32_t nb,
    const T &tab, const K &rk)
{
	uint8_t *p = a.out + a.offsets[i] + payload_at(a.flags[i], a.hashlen);
	const uint32_t rem = a.plen[i] & 15u;
	uint32_t chain[4], cur[4];

	/* block j of the padded plaintext: whole, or the tail and its padding */
	auto load = [&](uint32_t j, uint32_t (&w)[4]) {
		const uint8_t *q = p + 16 * (uint64_t)j;
		if (j + 1 < nb) {
			ld16(q, w);
			return;
		}
		w[0] = w[1] = w[2] = w[3] = 0;
#pragma unroll
		for (uint32_t k = 0; k < 16; k++) {
			const uint32_t v = k < rem ? q[k] : 16u - rem;
			w[k / 4] |= v << (24 - 8 * (k % 4));
		}
	};

	ld16(a.iv + 16 * i, chain);
	load(0, cur);
	for (uint32_t j = 0; j < nb; j++) {
		uint32_t nx[4] = { 0, 0, 0, 0 };
		if (j + 1 < nb)
			load(j + 1, nx);
#pragma unroll
		for (int k = 0; k < 4; k++)
			chain[k] ^= cur[k];
		aes_block<false>(tab, rk, chain);
		st16(p + 16 * (uint64_t)j, chain);
#pragma unroll
		for (int k = 0; k < 4; k++)
			cur[k] = nx[k];
	}
}

/*
 * The same under the keys of each datagram's own connection
 * (net2_packet_{decrypt,encrypt}_burst_mc): datagram i belongs to slot conn[i]
 * of the device cipher-key table (Net2CipherEnt, aes_tab.h).  What needs no
 * cipher work is settled as above, without a look-up; a datagram with cipher
 * work but without a connection -- conn[i] out of range, or the slot's rx
 * (decrypt) / tx (encrypt) side unset -- is PKT_NOCONN and left untouched:
 * one conn load and one meta load.  An index out of range is clamped to
 * entry 0 before any address is formed from it.
 */
struct AesMcArgs {
	AesBurstArgs b;
	const uint32_t *conn;
	const Net2CipherEnt *tab;
	uint32_t slots;
};

/* The entry of datagram i; *in: its index was in range (else entry 0). */
AES_HD const Net2CipherEnt *ciphertab_ent(const AesMcArgs &m, uint64_t i,
    bool *in)
{
	const uint32_t c = m.conn[i];
	*in = c < m.slots;
	return m.tab + (*in ? c : 0u);
}

/* Whether datagram i's slot has `side` (NET2_CT_RX / NET2_CT_TX) set. */
AES_HD bool ciphertab_has(const AesMcArgs &m, uint64_t i, uint32_t side)
{
	bool in;
	const Net2CipherEnt *e = ciphertab_ent(m, i, &in);
	return in && (e->meta[0] & side) != 0;
}

/* The rx schedule datagram i (flags fl) is decrypted under: its entry's
 * active or alternate one, picked by address (net2_ck_rx_key,
 * src/conn_keys.c:447-476, as the HMAC step chose).  After decrypt_mc_prep
 * found the entry's rx side set. */
AES_HD const uint32_t *ciphertab_rx_key(const AesMcArgs &m, uint64_t i,
    uint32_t fl)
{
	bool in;
	const Net2CipherEnt *e = ciphertab_ent(m, i, &in);
	const u32x4 mt = *reinterpret_cast<const u32x4 *>(e->meta);
	const bool alt = aes_rx_alt((mt.x & NET2_CT_RX_ALT) != 0,
	    (mt.x & NET2_CT_RX_NOCUT) != 0, fl, m.b.seq[i], mt.y, mt.z);
	return e->dec[alt ? 1 : 0];
}

/* decrypt_prep, after the connection check of a datagram that would be
 * decrypted (no look-up for any other). */
AES_HD uint32_t decrypt_mc_prep(const AesMcArgs &m, uint64_t i)
{
	const AesBurstArgs &a = m.b;
	if (i < a.n && a.result[i] == PKT_OK &&
	    (a.flags[i] & PKT_PH_ENCRYPTED) != 0 && !ciphertab_has(m, i, NET2_CT_RX)) {
		a.result[i] = PKT_NOCONN;
		a.plen[i] = 0;
		return 0;
	}
	return decrypt_prep(a, i);
}

/* encrypt_prep, then the connection check of a slot it found room to encrypt
 * (RESOURCE wins over NOCONN; no look-up for any other). */
AES_HD uint32_t encrypt_mc_prep(const AesMcArgs &m, uint64_t i)
{
	const AesBurstArgs &a = m.b;
	const uint32_t nb = encrypt_prep(a, i);
	if (nb != 0 && !ciphertab_has(m, i, NET2_CT_TX)) {
		a.result[i] = PKT_NOCONN;
		a.wire_len[i] = 0;
		return 0;
	}
	return nb;
}

}	/* namespace */

#endif /* NET2_AES_CBC_H */
