/*
 * sha2_burst.h -- packet-header IVs and the lane form's burst prep / final kernels.
 * One of the device headers of sha2_kernels.hip, which includes them in
 * order into one translation unit.
 */
#ifndef NET2_SHA2_BURST_H
#define NET2_SHA2_BURST_H

#include "sha2_hmac.h"

namespace net2 {
namespace dev {

/* ---- packet-header IV derivation (types/packet.n2t:100-158) ---------------- */

/*
 * iv = first ivlen bytes of D0 || D1 with D0 = SHA-256(ph), D1 = SHA-256(ph
 * || D0), ph = be32(seq) || be32(flags) (cp_packet_header,
 * packet.n2t:89-95).  The reference loops until the IV is long enough;
 * ivlen <= 64 covers two rounds, each a single block (8 + 32 bytes < 56).
 */
/* The IV of one header into out[0 .. ivlen) (ivlen <= 64). */
__device__ __forceinline__ void ph_iv_one(uint32_t s, uint32_t f,
    uint32_t ivlen, uint8_t *o)
{
	uint32_t d[16];
	uint32_t st[8], w[16];
#pragma unroll
	for (int r = 0; r < 2; r++) {
		if (r == 1 && ivlen <= 32)
			break;
#pragma unroll
		for (int j = 0; j < 16; j++)
			w[j] = 0;
		w[0] = s;
		w[1] = f;
		if (r == 0) {
			w[2] = 0x80000000u;
			w[15] = 8 * 8;
		} else {
#pragma unroll
			for (int j = 0; j < 8; j++)
				w[2 + j] = d[j];
			w[10] = 0x80000000u;
			w[15] = 40 * 8;
		}
#pragma unroll
		for (int j = 0; j < 8; j++)
			st[j] = IV256[j];
		compress256(st, w);
#pragma unroll
		for (int j = 0; j < 8; j++)
			d[8 * r + j] = st[j];
	}
	/* 16-byte stores when the IV is whole 16-byte pieces at an aligned
	 * address (AES's 16-byte IV in an n x 16 array), bytes otherwise */
	if ((ivlen & 15) == 0 && (reinterpret_cast<uintptr_t>(o) & 15) == 0) {
		uint4 *q = reinterpret_cast<uint4 *>(o);
#pragma unroll
		for (int k = 0; k < 4; k++)
			if (16u * k < ivlen)
				q[k] = make_uint4(bswap32(d[4 * k]),
				    bswap32(d[4 * k + 1]), bswap32(d[4 * k + 2]),
				    bswap32(d[4 * k + 3]));
		return;
	}
	for (uint32_t b = 0; b < ivlen; b++)
		o[b] = (uint8_t)(d[b >> 2] >> (24 - 8 * (b & 3)));
}

__global__ __launch_bounds__(256) void ph_iv_kernel(const uint32_t *__restrict__ seq,
    const uint32_t *__restrict__ flags, uint64_t n, uint32_t ivlen,
    uint8_t *__restrict__ out)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n)
		return;
	ph_iv_one(seq[i], flags[i], ivlen, out + i * ivlen);
}

/* ---- packet bursts: the hash steps of net2_packet_encode / decode ---------- */

/*
 * A datagram on the wire is the packet header (uint32 seq, uint32 flags,
 * big-endian: cp_packet_header, types/packet.n2t:89-97), then -- when
 * PH_SIGNED -- the HMAC of the rest (prepended last by net2_packet_encode,
 * :417-426, removed first by net2_packet_decode, :233-243), then the
 * payload (encrypted when PH_ENCRYPTED).  burst_prep_kernel does the
 * per-datagram bookkeeping of those functions for a whole burst and points
 * the HMAC kernel at each datagram's "hash field || payload" region;
 * burst_final_kernel folds the HMAC verdicts in and derives the IVs.
 *
 * status byte: the NET2_P{EN,DE}CODE_* code, | BURST_VERIFY when the HMAC
 * verdict of the region decides it.
 */
/* (BURST_VERIFY, the PKT_* codes and load_be32_bytes: above hmac_kernel) */

__global__ __launch_bounds__(256) void burst_prep_kernel(uint8_t *__restrict__ base,
    const uint64_t *__restrict__ offsets, const uint32_t *__restrict__ lens,
    uint64_t n, int encode, int hash_set, int enc_set, uint32_t hashlen,
    const uint32_t *__restrict__ seq_in, const uint32_t *__restrict__ flags_in,
    uint32_t *__restrict__ seq_out, uint32_t *__restrict__ flags_out,
    uint64_t *__restrict__ sub_off, uint32_t *__restrict__ sub_len,
    uint8_t *__restrict__ status)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n)
		return;
	const uint64_t off = offsets[i];
	const uint32_t len = lens[i];
	uint8_t *p = base + off;
	uint32_t seq, fl, st = PKT_OK, sl = 0;
	if (encode) {
		seq = seq_in[i];
		fl = flags_in[i];
	} else if (len < 8) {		/* cp_packet_header decode fails, :196-198 */
		seq = fl = 0;
		st = PKT_BAD;
	} else {
		seq = load_be32_bytes(p);
		fl = load_be32_bytes(p + 4);
	}
	const bool do_sign = (fl & PKT_PH_SIGNED) != 0;
	const bool do_cryp = (fl & PKT_PH_ENCRYPTED) != 0;
	if (st == PKT_OK) {
		/* flags against the negotiated keys: decode :217-221, encode
		 * :364-370 (which also refuses a flag without its key) */
		if ((!do_sign && hash_set) || (!do_cryp && enc_set) ||
		    (encode && ((do_sign && !hash_set) || (do_cryp && !enc_set))))
			st = PKT_UNSAFE;
	}
	if (st == PKT_OK && encode) {
		if (len < 8 + (do_sign ? hashlen : 0)) {
			st = PKT_RESOURCE;	/* the slot has no room for them */
		} else {
			for (int b = 0; b < 4; b++) {
				p[b] = (uint8_t)(seq >> (24 - 8 * b));
				p[4 + b] = (uint8_t)(fl >> (24 - 8 * b));
			}
			if (do_sign)
				sl = len - 8;	/* hash field || payload */
		}
	} else if (st == PKT_OK && do_sign && hash_set) {
		sl = len - 8;		/* supplied hash || payload, :233-257 */
		st |= BURST_VERIFY;
	}
	/* an empty region stays inside the datagram (a runt at the end of the
	 * buffer has no bytes at off + 8) */
	sub_off[i] = sl != 0 ? off + 8 : off;
	sub_len[i] = sl;
	status[i] = (uint8_t)st;
	if (seq_out != nullptr) {
		seq_out[i] = seq;
		flags_out[i] = fl;
	}
}

/* MC (the multi-connection RX burst): the cipher key is a property of the
 * datagram's connection, so the HMAC lane marks the status of a datagram
 * whose connection has none with BURST_NOIV, where a single-connection burst
 * is launched with ivlen 0. */
template <bool MC>
__device__ __forceinline__ void burst_final_item(uint64_t i,
    const uint8_t *__restrict__ status, const uint8_t *__restrict__ verdict,
    const uint32_t *__restrict__ seq, const uint32_t *__restrict__ flags,
    uint32_t ivlen, uint8_t *__restrict__ iv, uint8_t *__restrict__ result,
    uint32_t *__restrict__ seq_out, uint32_t *__restrict__ flags_out)
{
	if (seq_out != nullptr) {	/* the decoded header, to the host */
		seq_out[i] = seq[i];
		flags_out[i] = flags[i];
	}
	uint32_t st = status[i];
	const bool noiv = MC && (st & BURST_NOIV) != 0;
	if (MC)
		st &= ~BURST_NOIV;
	if (st & BURST_VERIFY)		/* net2_buffer_cmp, :253-257 */
		st = verdict[i] == 0 ? PKT_OK : PKT_BAD;
	/* an encrypted datagram's IV from its header, :263-279 */
	if (st == PKT_OK && !noiv && iv != nullptr && ivlen > 0 &&
	    (flags[i] & PKT_PH_ENCRYPTED))
		ph_iv_one(seq[i], flags[i], ivlen, iv + i * ivlen);
	result[i] = (uint8_t)st;
}

__global__ __launch_bounds__(256) void burst_final_kernel(uint64_t n,
    const uint8_t *__restrict__ status, const uint8_t *__restrict__ verdict,
    const uint32_t *__restrict__ seq, const uint32_t *__restrict__ flags,
    uint32_t ivlen, uint8_t *__restrict__ iv, uint8_t *__restrict__ result,
    uint32_t *__restrict__ seq_out, uint32_t *__restrict__ flags_out)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n)
		return;
	burst_final_item<false>(i, status, verdict, seq, flags, ivlen, iv, result,
	    seq_out, flags_out);
}

__global__ __launch_bounds__(256) void burst_final_mc_kernel(uint64_t n,
    const uint8_t *__restrict__ status, const uint8_t *__restrict__ verdict,
    const uint32_t *__restrict__ seq, const uint32_t *__restrict__ flags,
    uint32_t ivlen, uint8_t *__restrict__ iv, uint8_t *__restrict__ result)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n)
		return;
	burst_final_item<true>(i, status, verdict, seq, flags, ivlen, iv, result,
	    nullptr, nullptr);
}

} /* namespace dev */
} /* namespace net2 */

#endif /* NET2_SHA2_BURST_H */
