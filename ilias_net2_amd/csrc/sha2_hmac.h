/*
 * sha2_hmac.h -- the HMAC lane, the packet constants, the device key table, the HMAC kernels.
 * One of the device headers of sha2_kernels.hip, which includes them in
 * order into one translation unit.
 */
#ifndef NET2_SHA2_HMAC_H
#define NET2_SHA2_HMAC_H

#include "sha2_digest.h"

namespace net2 {
namespace dev {

/* ---- HMAC (RFC 2104) ------------------------------------------------------ */

/*
 * The keyed rows of the registry (HMAC-SHA256/384/512, key length = digest
 * length, cxx_src/hash-openssl.cc:417-429), i.e. the per-datagram
 * authenticator of net2_packet_encode/decode (types/packet.n2t:246,417),
 * over a whole batch under one connection key:
 *   HMAC(K, m) = H((K' ^ opad) || H((K' ^ ipad) || m)),  K' = K zero-padded.
 * The two key blocks -- the same for every packet of a launch -- are
 * compressed once on the host (hmac_key_mids, sha2_keyprep.h) and arrive as
 * a kernel argument (HMid): the ipad / opad midstates, copied to LDS at
 * kernel entry; every lane hashes its packet from the inner midstate (bit count includes the key
 * block) and finishes with one outer compression over the inner digest.
 * (Until round 4 wave 0 of every workgroup compressed the key blocks while
 * the other waves waited: a second instance of the round code in the kernel,
 * which held the fixed-layout HMAC-SHA512 kernel at 115 VGPRs.)
 */

/*
 * Where a lane's two midstates come from (hmac_lane's MIDS): inner() before
 * the block loop, outer() after it.  LdsMids: the launch's one key, in the
 * workgroup's LDS copy.
 */
struct LdsMids {
	const uint32_t (*mid)[16];
	template <class H>
	__device__ __forceinline__ void inner(typename H::State &st) const
	{
		load_mid<H>(mid, 0, st);
	}
	template <class H>
	__device__ __forceinline__ void outer(typename H::State &st) const
	{
		load_mid<H>(mid, 1, st);
	}
};

/* Inner hash from the ipad midstate, one address mode. */
template <class H, int AMODE, bool PADCONST, class MIDS,
    bool PREFETCH = H::PREFETCH>
__device__ __forceinline__ void hmac_inner(const uint8_t *p, uint32_t len,
    const MIDS &mids, const typename H::word *kw,
    typename H::State &st, bool padtab)
{
	mids.template inner<H>(st);
	absorb<H, AMODE, PREFETCH>(p, len, st);
	if (!PADCONST && padtab)
		finish<H, true>(p, len, 0, kw, st);
	else
		finish<H, PADCONST>(p, len, ((uint64_t)len + H::BLOCK) << 3, kw,
		    st);
}

template <class H, bool PADCONST, class MIDS>
__device__ __forceinline__ void hmac_lane(const uint8_t *p, uint32_t len,
    int is384, int amode, const MIDS &mids,
    const typename H::word *kw, typename H::State &st, bool padtab = false)
{
	constexpr int NW32 = H::NW32;
	/* the midstates stay in LDS (the key table: in global memory) and are
	 * read where they are used, so neither is held in VGPRs across the
	 * block loop */
	if (amode == AMODE_A16)
		hmac_inner<H, AMODE_A16, PADCONST>(p, len, mids, kw, st, padtab);
	else if (amode == AMODE_A4)
		hmac_inner<H, AMODE_A4, PADCONST>(p, len, mids, kw, st, padtab);
	else
		hmac_inner<H, AMODE_A1, PADCONST>(p, len, mids, kw, st, padtab);

	/* outer: one block = inner digest || 0x80 || 0... || bit count */
	uint32_t w[NW32];
#pragma unroll
	for (int i = 0; i < NW32; i++)
		w[i] = 0;
	const int dw = digest_words<H>(st, is384, w);
#pragma unroll
	for (int i = 12; i < 16; i++)		/* SHA-384 keeps 12 words */
		if (i >= dw)
			w[i] = 0;
	w[dw] = 0x80000000u;
	const uint64_t obits = (uint64_t)(H::BLOCK + 4 * dw) << 3;
	w[NW32 - 2] = (uint32_t)(obits >> 32);
	w[NW32 - 1] = (uint32_t)obits;
	mids.template outer<H>(st);
	H::compress(st, w);
}

/*
 * PADCONST: fixed layout with fixed_len % BLOCK == 0, so the inner pad
 * block (bit count = (BLOCK + fixed_len) * 8) is the same for every lane
 * and its K + W schedule comes precomputed in pad, as in fixed_kernel.
 *
 * MODE (variable layout only for SIGN / VERIFY): datagram i is
 * base[offsets[i] .. + lens[i]) = hash field (dlen bytes) || message, the
 * wire order of net2_packet_encode (the hash is prepended,
 * types/packet.n2t:417-427) and net2_packet_decode (it is removed first,
 * :236-244).
 *   HMAC_DIGESTS: digest of the whole packet to out + i * dlen;
 *   HMAC_SIGN:    digest of the message into the datagram's hash field
 *                 (out == base, writable); datagrams shorter than dlen are
 *                 left untouched;
 *   HMAC_VERIFY:  out[i] = 0 if the hash field equals the digest of the
 *                 message (the net2_buffer_cmp of :254), 1 if it does not,
 *                 2 if the datagram is shorter than dlen (:240-244).
 */
enum { HMAC_DIGESTS = 0, HMAC_SIGN = 1, HMAC_VERIFY = 2, HMAC_BURST_RX = 3,
    HMAC_BURST_TX = 4, HMAC_BURST_RX_MC = 5, HMAC_BURST_TX_MC = 6 };

/*
 * Packet-burst codes (the burst kernels below): the status byte is the
 * NET2_P{EN,DE}CODE_* code, | BURST_VERIFY when the HMAC verdict of the
 * datagram's region decides it.
 */
#define BURST_VERIFY 0x80u
/* (HMAC_BURST_RX_MC only) | BURST_NOIV: the datagram's connection has no
 * cipher key, so no IV is due whatever its flags say */
#define BURST_NOIV 0x40u
#define PKT_PH_ENCRYPTED 0x00000001u	/* types/packet.n2t:27 */
#define PKT_PH_SIGNED 0x00000002u	/* types/packet.n2t:28 */
#define PKT_PH_ALTKEY 0x80000000u	/* types/packet.n2t:34 */
#define PKT_OK 0
#define PKT_RESOURCE 1
#define PKT_BAD 2
#define PKT_UNSAFE 3

__device__ __forceinline__ uint32_t load_be32_bytes(const uint8_t *p)
{
	return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) |
	    ((uint32_t)p[2] << 8) | (uint32_t)p[3];
}

/*
 * HMAC_BURST_RX: the per-datagram bookkeeping of net2_packet_decode folded
 * into the VERIFY kernel.  offsets / lens describe whole wire datagrams;
 * each lane decodes its datagram's header (cp_packet_header,
 * types/packet.n2t:196-198), checks the flags against the negotiated keys
 * (:217-221; a hash key is always set on this path), and, when PH_SIGNED,
 * verifies "hash field || payload" after the 8-byte header (:233-257) --
 * exactly burst_prep_kernel's RX branch followed by HMAC_VERIFY, without
 * prep's extra pass over every datagram's first line.  Writes the status
 * (| BURST_VERIFY), seq and flags per datagram and the verdict to out.
 * HMAC_BURST_TX: the same for net2_packet_encode (out == base): the lane
 * takes seq / flags from the caller's arrays, applies the encode-side flag
 * checks (:364-370) and the room check, writes the header (:384-392) and
 * signs the payload into the hash field (:410-427), as burst_prep_kernel's
 * TX branch followed by HMAC_SIGN; status per datagram.
 */
/* (struct BurstArgs: sha2_launch.h) */

/*
 * HMAC_BURST_RX_MC / HMAC_BURST_TX_MC: the same per lane under the keys of
 * the datagram's own connection (net2_packet_{decode,encode}_burst_mc): a
 * shared socket's receive batch interleaves the datagrams of many
 * connections (src/udp_connection.c:81-170), each with its own negotiated
 * key and rollover state.  Datagram i belongs to slot kt.conn[i] of the
 * device key table (Net2KeyEnt, sha2_launch.h); the entry's bits, cutoff and
 * rx_start stand in for BurstArgs' and its midstates for the launch's, read
 * from global memory where they are used.  RX: the header is decoded first
 * (a runt is PKT_BAD whatever its connection, packet.n2t:196-198 precede the
 * key lookup at :210), then a datagram without a connection -- conn[i] out
 * of range or the slot's rx side unset -- is PKT_NOCONN: header stored, no
 * hash, no IV.  TX: a slot without a tx side is PKT_NOCONN and left
 * untouched.  An index out of range is clamped to entry 0 before any
 * address is formed from it.
 */
#define PKT_NOCONN 5			/* NET2_PBURST_NOCONN */

/* The entry of datagram i; *in: its index was in range (else entry 0). */
__device__ __forceinline__ const Net2KeyEnt *keytab_ent(const KeyTabArgs &kt,
    uint64_t i, bool *in)
{
	const uint32_t c = kt.conn[i];
	*in = c < kt.slots;
	return kt.tab + (*in ? c : 0u);
}

/* net2_ck_rx_key (src/conn_keys.c:447-476) over an entry's meta words. */
__device__ __forceinline__ bool keytab_rx_alt(uint32_t bits, uint32_t cutoff,
    uint32_t rx_start, uint32_t seq, uint32_t fl)
{
	return (bits & NET2_KT_RX_ALT) != 0 && ((fl & PKT_PH_ALTKEY) != 0 ||
	    ((bits & NET2_KT_RX_NOCUT) == 0 &&
	    seq - rx_start >= cutoff - rx_start));
}

/* A table midstate (16-byte aligned) into a state: dwordx4 global loads. */
template <class H>
__device__ __forceinline__ void load_mid_tab(const uint32_t *m,
    typename H::State &st)
{
	typedef __attribute__((address_space(1))) const u32x4 gconst_u32x4;
	gconst_u32x4 *q = (gconst_u32x4 *)reinterpret_cast<uintptr_t>(m);
	constexpr int NQ = sizeof(typename H::word) == 4 ? 2 : 4;
	u32x4 v[NQ];
#pragma unroll
	for (int k = 0; k < NQ; k++)
		v[k] = q[k];
#pragma unroll
	for (int k = 0; k < NQ; k++) {
		if (sizeof(typename H::word) == 4) {
			st[4 * k] = v[k].x;
			st[4 * k + 1] = v[k].y;
			st[4 * k + 2] = v[k].z;
			st[4 * k + 3] = v[k].w;
		} else {
			st[2 * k] = mk64(v[k].y, v[k].x);
			st[2 * k + 1] = mk64(v[k].w, v[k].z);
		}
	}
}

/*
 * hmac_lane's midstates from the key table.  in: the inner midstate, chosen
 * by hmac_item before the hash.  The outer one is found again from conn[i]
 * after the block loop -- for RX with the key choice redone from the stored
 * header -- as the hash field is from offsets[i], so no entry address is
 * held in VGPRs across the loop.
 */
template <bool RX>
struct TabMids {
	const KeyTabArgs &kt;
	const BurstArgs &rx;
	uint64_t i;
	const uint32_t *in;
	template <class H>
	__device__ __forceinline__ void inner(typename H::State &st) const
	{
		load_mid_tab<H>(in, st);
	}
	template <class H>
	__device__ __forceinline__ void outer(typename H::State &st) const
	{
		/* an opaque copy of i: these are addresses and loads of their
		 * own, not hmac_item's (&conn[i] would stay live across the hash) */
		uint64_t j = i;
		/* the look-up and its loads stay between the inner digest and the
		 * outer compression: hoisted to hide their latency, the 8 to 16
		 * midstate VGPRs would be live with the outer block's schedule
		 * (the SHA-512 TX instance: 124 VGPRs against 97) */
		__builtin_amdgcn_sched_barrier(0);
		asm volatile("" : "+v"(j));
		bool inr;
		const Net2KeyEnt *e = keytab_ent(kt, j, &inr);
		const uint32_t *m = e->tx[1];
		if (RX) {
			const uint4 mt = *reinterpret_cast<const uint4 *>(e->meta);
			m = e->rx[keytab_rx_alt(mt.x, mt.y, mt.z, rx.seq[j],
			    rx.flags[j]) ? 3 : 1];
		}
		load_mid_tab<H>(m, st);
#pragma unroll
		for (int k = 0; k < 8; k++)
			asm volatile("" : "+v"(st[k]));
		__builtin_amdgcn_sched_barrier(0);
	}
};


/*
 * One datagram / packet of hmac_kernel: binned position g (live: g < n).
 * Shares the workgroup's key midstates (mid) and, for SHA-512, its LDS
 * constant table; calls block_pad512 (a workgroup barrier), so every
 * thread of the workgroup calls it the same number of times.  IS384 and
 * the digest length are compile-time constants of the kernel instance
 * (SHA-384 is its own instance: the outer block's 0x80 word and zero fill
 * fold into its schedule).
 */
template <class H, bool PADCONST, int MODE, bool IS384>
__device__ __forceinline__ void hmac_item(uint64_t g,
    const uint8_t *__restrict__ base, const uint64_t *__restrict__ offsets,
    const uint32_t *__restrict__ lens, const uint32_t *__restrict__ perm,
    uint64_t stride, uint32_t fixed_len, uint64_t n,
    uint8_t *__restrict__ out, const PadKW<typename H::word> &pad,
    const BurstArgs &rx, const uint32_t (*mid)[16],
    const KeyTabArgs &kt = KeyTabArgs{})
{
	constexpr int is384 = IS384;
	constexpr uint32_t dlen = sizeof(typename H::word) == 4 ? 32 :
	    IS384 ? 48 : 64;
	/* the multi-connection modes: keys per lane from the table kt (mid
	 * unused, no rec form) */
	constexpr bool MC = MODE == HMAC_BURST_RX_MC || MODE == HMAC_BURST_TX_MC;
	constexpr bool RXM = MODE == HMAC_BURST_RX || MODE == HMAC_BURST_RX_MC;
	constexpr bool TXM = MODE == HMAC_BURST_TX || MODE == HMAC_BURST_TX_MC;
	const uint32_t (*lmid)[16] = mid;	/* this lane's key */
	const bool live = g < n;
	uint64_t i = g;
	const uint8_t *p;
	uint32_t len;
	if (offsets != nullptr) {
		i = live ? (perm ? (uint64_t)perm[g] : g) : 0;
		if (i >= n)	/* a corrupt workspace: never out of bounds */
			i = g;
		p = base + (live ? offsets[i] : 0);
		len = live ? lens[i] : 0;
	} else {
		p = base + (live ? i * stride : 0);
		len = live ? fixed_len : 0;
	}
	uint32_t rx_st = PKT_OK, rx_seq = 0, rx_fl = 0;
	/* TX with rx.rec (the host path): instead of sealing in place, every
	 * live lane fills the record of its binned position g -- hash field at
	 * +0, then header, datagram index and code -- so a wave's stores cover
	 * one contiguous stretch of (host) memory; the address is formed where
	 * it is used, not held across the hash */
	if (TXM) {
		if (live) {
			rx_seq = rx.seq[i];
			rx_fl = rx.flags[i];
		}
		const bool sg = (rx_fl & PKT_PH_SIGNED) != 0;
		const bool cr = (rx_fl & PKT_PH_ENCRYPTED) != 0;
		uint32_t bits = 0;	/* MC: the connection's entry */
		if (MC) {
			bool inr;
			const Net2KeyEnt *e = keytab_ent(kt, i, &inr);
			bits = inr ? e->meta[0] : 0u;
			lmid = e->tx;
		}
		if (MC && (bits & NET2_KT_TX) == 0)
			rx_st = PKT_NOCONN;	/* the slot has no tx key */
		else if (!sg || cr != (MC ? (bits & NET2_KT_TX_ENC) != 0 :
		    rx.enc_set != 0))
			rx_st = PKT_UNSAFE;
		else if (len < 8 + dlen)
			rx_st = PKT_RESOURCE;	/* no room for header and hash */
		const bool ok = live && rx_st == PKT_OK;
		if (live && !MC && rx.rec != nullptr) {
			*reinterpret_cast<uint4 *>(rx.rec + g * (dlen + 16) + dlen) =
			    make_uint4(ok ? bswap32(rx_seq) : 0u,
			    ok ? bswap32(rx_fl) : 0u, (uint32_t)i, rx_st);
		} else if (ok) {
			uint8_t *h = out + (p - base);
#pragma unroll
			for (int b = 0; b < 4; b++) {
				h[b] = (uint8_t)(rx_seq >> (24 - 8 * b));
				h[4 + b] = (uint8_t)(rx_fl >> (24 - 8 * b));
			}
		}
		if (ok) {
			p += 8;
			len -= 8;
		} else {
			len = 0;
		}
		if (live && (MC || rx.rec == nullptr))
			rx.status[i] = (uint8_t)rx_st;
	}
	if (RXM) {
		if (len < 8) {
			rx_st = PKT_BAD;	/* header decode fails */
		} else {
			rx_seq = load_be32_bytes(p);
			rx_fl = load_be32_bytes(p + 4);
		}
		bool use_alt;
		int enc_set;
		if (MC) {
			/* the connection's entry, looked up once the header is
			 * decoded (packet.n2t:210) */
			bool inr;
			const Net2KeyEnt *e = keytab_ent(kt, i, &inr);
			const uint4 mt = *reinterpret_cast<const uint4 *>(e->meta);
			const uint32_t bits = inr ? mt.x : 0u;
			use_alt = rx_st == PKT_OK &&
			    keytab_rx_alt(bits, mt.y, mt.z, rx_seq, rx_fl);
			lmid = e->rx + (use_alt ? 2 : 0);
			enc_set = (bits & NET2_KT_RX_ENC) != 0;
			if (rx_st == PKT_OK && (bits & NET2_KT_RX) == 0)
				rx_st = PKT_NOCONN;	/* no rx key: nothing hashed */
		} else {
			/* net2_ck_rx_key (src/conn_keys.c:447-476): the alternate
			 * key when the datagram says so or lies past the cutoff */
			use_alt = rx_st == PKT_OK && rx.alt &&
			    ((rx_fl & PKT_PH_ALTKEY) != 0 || (!rx.no_cutoff &&
			    rx_seq - rx.rx_start >= rx.cutoff - rx.rx_start));
			if (use_alt)
				lmid = mid + 2;
			enc_set = use_alt ? rx.alt_enc_set : rx.enc_set;
		}
		if (rx_st == PKT_OK && ((rx_fl & PKT_PH_SIGNED) == 0 ||
		    (enc_set && (rx_fl & PKT_PH_ENCRYPTED) == 0)))
			rx_st = PKT_UNSAFE;
		if (rx_st == PKT_OK) {
			rx_st |= BURST_VERIFY;	/* hash field || payload */
			if (MC && !enc_set)
				rx_st |= BURST_NOIV;
			p += 8;
			len -= 8;
		} else {
			len = 0;
		}
		/* stored now, so none of them is held across the hash */
		if (live) {
			rx.status[i] = (uint8_t)rx_st;
			rx.seq[i] = rx_seq;
			rx.flags[i] = rx_fl;
		}
	}
	const bool short_dgram = MODE != HMAC_DIGESTS && len < dlen;
	if (MODE != HMAC_DIGESTS) {
		p += short_dgram ? 0 : dlen;
		len = short_dgram ? 0 : len - dlen;
	}
	typename H::State st;
	const uintptr_t pa = reinterpret_cast<uintptr_t>(p);
	const int amode = OnePath<H>::value || __all((pa & 15) == 0) ? AMODE_A16 :
	    __all((pa & 3) == 0) ? AMODE_A4 : AMODE_A1;
	/* a variable-layout SHA-256 wave of one whole-block inner length (key
	 * block included) takes its inner pad schedule from g_padtab256 */
	const typename H::word *kw = nullptr;
	bool padtab = false;
	if constexpr (!PADCONST && sizeof(typename H::word) == 4) {
		if (offsets != nullptr)
			kw = uniform_pad_kw<H>(live, (uint64_t)len + H::BLOCK);
		padtab = kw != nullptr;
	}
	/* (SHA-512: no pad table.  The workgroup-uniform g_padtab512 row the
	 * variable-length digest kernel stages costs these kernels 11 VGPRs --
	 * 106-107 against 95-96, four waves per SIMD instead of five -- and
	 * pays only when a whole workgroup's inner lengths are one multiple of
	 * 128 bytes, which no MTU mix has: payload + 128-byte key block of
	 * {64, 512, 1428 / 1500} B.) */
	if constexpr (MC)
		hmac_lane<H, PADCONST>(p, len, is384, amode,
		    TabMids<RXM>{ kt, rx, i, lmid[0] },
		    kw != nullptr ? kw : pad.kw, st, padtab);
	else
		hmac_lane<H, PADCONST>(p, len, is384, amode, LdsMids{ lmid },
		    kw != nullptr ? kw : pad.kw, st, padtab);
	materialize<H>(st);
	if (!live)
		return;
	uint32_t o[16];
	H::out_words(st, o, is384);
	/* SIGN / VERIFY: the hash field, found again from the descriptor
	 * rather than held in two VGPRs across the hash: the datagram's start,
	 * past the header in the burst modes.  Its line has mostly left L2 by
	 * now (burst RX reads ~115 B more per datagram than round 4,
	 * profiles/pmc_burst_rx.json): HBM bytes, no time on this VALU-bound
	 * kernel */
	const uint8_t *field = MODE == HMAC_DIGESTS ? nullptr :
	    base + offsets[i] + (RXM || TXM ? 8 : 0);
	if (MODE == HMAC_VERIFY || RXM) {
		/* o[] holds the digest bytes little-endian per word, the order
		 * store_digest writes them in */
		uint32_t diff = 0;
		constexpr int NO = dlen / 4;
		if (!short_dgram && amode == AMODE_A16) {
			/* field = message start - dlen: 16-byte aligned as well
			 * (SHA-512: the one address path reads it at any alignment);
			 * all loads issued at once (a per-byte loop waited out one
			 * memory latency per byte) */
			const u32x4 *f = reinterpret_cast<const u32x4 *>(field);
#pragma unroll
			for (int k = 0; k < NO / 4; k++) {
				const u32x4 v = f[k];
				diff |= (v.x ^ o[4 * k]) | (v.y ^ o[4 * k + 1]) |
				    (v.z ^ o[4 * k + 2]) | (v.w ^ o[4 * k + 3]);
			}
		} else if (!short_dgram && amode == AMODE_A4) {
			const uint32_t *f = reinterpret_cast<const uint32_t *>(field);
#pragma unroll
			for (int k = 0; k < NO; k++)
				diff |= f[k] ^ o[k];
		} else if (!short_dgram) {
#pragma unroll
			for (int j = 0; j < (int)dlen; j++)
				diff |= field[j] ^
				    ((o[j >> 2] >> (8 * (j & 3))) & 0xffu);
		}
		out[i] = short_dgram ? 2 : diff != 0;
		return;
	}
	constexpr bool SIGNS = MODE == HMAC_SIGN || TXM;
	if (SIGNS && short_dgram)
		return;
	if (MODE == HMAC_BURST_TX && rx.rec != nullptr)
		store_digest<dlen>(rx.rec + g * (dlen + 16), o);
	else
		store_digest<dlen>(SIGNS ? out + (field - base) : out + i * dlen,
		    o);
}

/*
 * ws: the binning workspace of this launch (variable layout; NULL:
 * submission order); hm: the key's midstates (HMid).  No occupancy request:
 * 5 waves asked of the SHA-512 kernels measured +3-4 % on the digests only
 * while they spilled, and -2 to -15 % on the sign / verify / burst modes
 * (round 2, profiles/round2/hmac512_waves_ab.txt); the VGPR count decides.
 */
template <class H, bool PADCONST, int MODE, bool IS384>
__global__ __launch_bounds__(256) void hmac_kernel(const uint8_t *__restrict__ base,
    const uint64_t *__restrict__ offsets, const uint32_t *__restrict__ lens,
    const uint32_t *__restrict__ ws, uint32_t launch, uint64_t stride,
    uint32_t fixed_len, uint64_t n, uint8_t *__restrict__ out, HMid hm,
    PadKW<typename H::word> pad, BurstArgs rx)
{
	/* [0..1]: the key's ipad / opad midstates; [2..3]: the alternate rx
	 * key's (HMAC_BURST_RX with rx.alt) */
	__shared__ uint32_t mid[4][16];
	const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	/* one lane copies them (the by-value argument read with constant
	 * indices only: a dynamic index would copy it to scratch) */
	if (threadIdx.x == 0) {
		constexpr int NK = MODE == HMAC_BURST_RX ? 4 : 2;
		/* whole chaining values (SHA-384's too) */
		constexpr int NWD = sizeof(typename H::word) == 4 ? 8 : 16;
#pragma unroll
		for (int k = 0; k < NK; k++)
#pragma unroll
			for (int j = 0; j < NWD; j++)
				mid[k][j] = hm.w[k][j];
	}
	if (sizeof(typename H::word) == 8) {
		/* (both synchronise the workgroup) */
		if (PADCONST)
			k512_lds_fill_pad(pad);
		else
			k512_lds_fill();
	} else {
		__syncthreads();
	}
	hmac_item<H, PADCONST, MODE, IS384>(g, base, offsets, lens,
	    offsets != nullptr ? bin_perm(ws, launch) : nullptr, stride,
	    fixed_len, n, out, pad, rx, mid);
}

/*
 * hmac_kernel's sibling for the multi-connection burst modes
 * (HMAC_BURST_RX_MC / _TX_MC, variable layout): the same hmac_item, no key
 * in the arguments and none in LDS -- lane by lane from the key table.
 */
template <class H, int MODE, bool IS384>
__global__ __launch_bounds__(256) void hmac_mc_kernel(
    const uint8_t *__restrict__ base, const uint64_t *__restrict__ offsets,
    const uint32_t *__restrict__ lens, const uint32_t *__restrict__ ws,
    uint32_t launch, uint64_t n, uint8_t *__restrict__ out,
    const uint32_t *__restrict__ conn, const Net2KeyEnt *__restrict__ tab,
    uint32_t slots, PadKW<typename H::word> pad, BurstArgs rx)
{
	const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (sizeof(typename H::word) == 8)
		k512_lds_fill();	/* (synchronises the workgroup) */
	const KeyTabArgs kt = { conn, tab, slots };
	hmac_item<H, false, MODE, IS384>(g, base, offsets, lens,
	    bin_perm(ws, launch), 0, 0, n, out, pad, rx, nullptr, kt);
}

/*
 * One slot's update (net2_burst_keytab_set_rx / _set_tx / _clear): the new
 * midstates and meta words arrive by value and one wave stores them, 16
 * bytes per lane (the argument is read with constant indices only and
 * selected per lane: a dynamic index would copy it to scratch).  side
 * NET2_KT_RX writes the rx midstates, cutoff and rx_start and replaces the
 * rx bits; NET2_KT_TX the tx midstates and the tx bits; 0 clears every bit.
 * Stream order is the only synchronisation an entry has.
 */
__global__ __launch_bounds__(64) void keytab_set_kernel(Net2KeyEnt *ent,
    uint32_t side, uint32_t bits, uint32_t cutoff, uint32_t rx_start, HMid hm)
{
	if (blockIdx.x != 0)
		return;
	const unsigned t = threadIdx.x;
	uint4 *q = reinterpret_cast<uint4 *>(ent);
	/* lane t < 16: the t-th 16 bytes of hm (rx: all four midstates, q[1..16];
	 * tx: the first two, q[17..24]) */
	uint4 v = make_uint4(0, 0, 0, 0);
#pragma unroll
	for (int k = 0; k < 16; k++)
		if (t == (unsigned)k)
			v = make_uint4(hm.w[k / 4][4 * (k % 4)],
			    hm.w[k / 4][4 * (k % 4) + 1], hm.w[k / 4][4 * (k % 4) + 2],
			    hm.w[k / 4][4 * (k % 4) + 3]);
	if (side == NET2_KT_RX && t < 16)
		q[1 + t] = v;
	if (side == NET2_KT_TX && t < 8)
		q[17 + t] = v;
	/* lane 63: the meta words, the other side's bits kept */
	if (t == 63) {
		uint4 mt = q[0];
		if (side == NET2_KT_RX)
			mt = make_uint4((mt.x & NET2_KT_TX_BITS) | bits, cutoff,
			    rx_start, 0);
		else if (side == NET2_KT_TX)
			mt.x = (mt.x & NET2_KT_RX_BITS) | bits;
		else
			mt.x = 0;
		q[0] = mt;
	}
}

} /* namespace dev */
} /* namespace net2 */

#endif /* NET2_SHA2_HMAC_H */
