/*
 * sha2_burst_wave.h -- the wave form of the keyed bursts, for small bursts.
 * One of the device headers of sha2_kernels.hip, which includes them in
 * order into one translation unit.
 */
#ifndef NET2_SHA2_BURST_WAVE_H
#define NET2_SHA2_BURST_WAVE_H

#include "sha2_burst.h"
#include "sha2_jobs.h"

namespace net2 {
namespace dev {

/* ---- small bursts: a few datagrams per workgroup ------------------------- */

/*
 * Latency form of the keyed burst modes (HMAC_BURST_RX / HMAC_BURST_TX of
 * hmac_kernel, plus burst_final_kernel's fold and IV), for bursts of at most
 * BW_GMAX datagrams per SIMD.  A burst that small has at most one wave per
 * SIMD in the lane form too, so its time is one datagram's serial chain of
 * compressions, schedule expansion included (~100 us for a 1,500-byte
 * HMAC-SHA512 datagram, profiles/round6/burst_sizes_*.jsonl).  Here a
 * workgroup of two waves takes G datagrams (G <= BW_GMAX, chosen by the
 *   launcher so that the grid is about one workgroup per SIMD):
 *   wave 0 -- lane l runs datagram (l mod G)'s HMAC, so every datagram's
 *     rounds run on 64 / G lanes in lockstep and no lane idles: rounds on
 *     one lane of a wave (an EXEC mask of one) ran 27 % slower per wave and,
 *     with four workgroups per CU, twice as slow (profiles/round6/bwp_*:
 *     89 / 176 us at 64 / 1,024 datagrams against 70 / 74).  Each pass, the
 *     wave's lanes first expand K = BW_ROWS / G blocks of every one of the G
 *     messages at once (row r: datagram r / K, block c0 + r % K, loaded,
 *     padded and expanded into its K + W row in LDS -- a block's schedule
 *     depends only on its own words), then every lane runs the rounds of
 *     its datagram's K blocks from LDS; lane d < G stores datagram d.  A pass costs one row's expansion however many rows
 *     it fills, so the schedule work leaves the serial chain: a 12-block
 *     datagram takes one pass at G <= 4, five at G = 16, against twelve
 *     expansions in the lane form.  Then the outer block, the verdict (RX)
 *     or the hash field (TX), and every store of the datagram;
 *   wave 1 -- RX: lane d derives datagram d's IV from its header (two
 *     SHA-256 compressions, ph_iv_one) into LDS meanwhile, off the chain.
 * Codes, decoded headers, IVs and sealed fields are those of hmac_item +
 * burst_final_kernel (RX) / hmac_item (TX), bit for bit; the datagrams of a
 * workgroup are consecutive (no binning: the burst's time is its longest
 * datagram's either way).
 *
 * rx: RX -- seq / flags receive the decoded header (NULL: not stored);
 * TX -- seq / flags are the inputs, rec as in BurstArgs (the host path) or
 * NULL (header and hash field written into out == base).  result: the final
 * code per datagram (RX; TX without rec).
 */
#define BW_ROWS 48	/* K + W rows of LDS per workgroup (31 KB at SHA-512:
			 * four workgroups per CU; 16 rows measured no faster,
			 * profiles/round6/bw_w2r16_*.jsonl) */
#define BW_GMAX 16	/* datagrams per workgroup at most: at G = 32 a pass
			 * expands one block per datagram, the lane form's cost */

/* Block k of an inner message of mlen bytes at m (nfull whole blocks, rem
 * tail bytes, nb blocks, bit count `bits` incl. the key block) as
 * big-endian words. */
template <class H>
__device__ __forceinline__ void bw_block(const uint8_t *m, uint32_t k,
    uint32_t nfull, uint32_t rem, uint32_t nb, uint64_t bits,
    uint32_t (&w)[H::NW32])
{
	constexpr int NW32 = H::NW32;
	if (k < nfull) {
		const uint8_t *bp = m + (size_t)k * H::BLOCK;
		Raw<NW32> r;
		issue_block<NW32, AMODE_A1>(bp, r);
		finish_block<NW32, AMODE_A1>(bp, r, w);
		return;
	}
	if (k == nfull) {
		tail_block<NW32>(m + (size_t)nfull * H::BLOCK, rem, w);
	} else {
#pragma unroll
		for (int i = 0; i < NW32; i++)
			w[i] = 0;
	}
	if (k == nb - 1) {
		w[NW32 - 2] = (uint32_t)(bits >> 32);
		w[NW32 - 1] = (uint32_t)bits;
	}
}

/* LDS written by some lanes of a wave, read by others of the same wave. */
__device__ __forceinline__ void wave_lds_sync()
{
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

/* One datagram's header, key choice and the region its HMAC covers (ciph and
 * ent: the key-table kernel's; the other reads neither, so pays nothing). */
struct BwDgram {
	uint32_t st, seq, fl;
	bool ok, hashed, alt;
	bool ciph;		/* RX: the connection has a cipher key */
	uint64_t off;		/* datagram start */
	uint32_t mlen;		/* message bytes after header and hash field */
	const Net2KeyEnt *ent;	/* the connection's entry (entry 0 when the
				 * index is out of range: never used then) */
};

/* The pieces the two kernels share, each rule of the packet format stated
 * once.  After the decode they take scalars: with the BwDgram passed by
 * reference the key-table SHA-256 RX instance takes 77 VGPRs, not 76. */

/* RX: the header's two words; a runt fails the header decode. */
__device__ __forceinline__ void bw_rx_header(BwDgram &g, const uint8_t *p,
    uint32_t len)
{
	if (len < 8) {
		g.st = PKT_BAD;
	} else {
		g.seq = load_be32_bytes(p);
		g.fl = load_be32_bytes(p + 4);
	}
}

/* TX: the code of a datagram whose key is there. */
template <uint32_t DLEN>
__device__ __forceinline__ uint32_t bw_tx_code(uint32_t fl, uint32_t len,
    bool enc_set)
{
	const bool sg = (fl & PKT_PH_SIGNED) != 0;
	const bool cr = (fl & PKT_PH_ENCRYPTED) != 0;
	if (!sg || cr != enc_set)
		return PKT_UNSAFE;
	if (len < 8 + DLEN)
		return PKT_RESOURCE;	/* no room for header and hash */
	return PKT_OK;
}

/* The end of a decode: what is hashed, from the code so far and the length. */
template <uint32_t DLEN>
__device__ __forceinline__ void bw_decode_end(BwDgram &g, uint32_t len)
{
	g.ok = g.st == PKT_OK;
	/* after the header: hash field, then message */
	const uint32_t rlen = g.ok ? len - 8 : 0;
	g.hashed = g.ok && rlen >= DLEN;
	g.mlen = g.hashed ? rlen - DLEN : 0;
}

/* Blocks of the inner hash after the key block (message, 0x80, bit count). */
template <class H>
__device__ __forceinline__ uint32_t bw_nblocks(bool hashed, uint32_t mlen)
{
	if (!hashed)
		return 0;
	const uint32_t rem = mlen % H::BLOCK;
	return mlen / H::BLOCK + 1 +
	    (rem >= (uint32_t)(H::BLOCK - H::LENBYTES) ? 1 : 0);
}

/* What the expanding lanes of a pass know of the G datagrams: three LDS
 * arrays of BW_GMAX that each kernel declares (as one struct in LDS the
 * SHA-256 instances allocate one VGPR less; counts are kept as they were). */
struct BwGeo {
	uint64_t *m;		/* message start (offset) */
	uint32_t *len, *nb;
};

/* Lane d < G publishes datagram d's geometry (a slot past n: no blocks);
 * returns the largest block count of the G, wave-uniform. */
template <uint32_t DLEN>
__device__ __forceinline__ uint32_t bw_publish(const BwGeo &geo, uint32_t lane,
    uint32_t G, uint64_t off, uint32_t mlen, uint32_t nb)
{
	if (lane < G) {
		geo.m[lane] = off + 8 + DLEN;
		geo.len[lane] = mlen;
		geo.nb[lane] = nb;
	}
	wave_lds_sync();
	uint32_t nbmax = 0;
	for (uint32_t d = 0; d < G; d++)
		nbmax = max(nbmax, geo.nb[d]);
	return __builtin_amdgcn_readfirstlane(nbmax);
}

/* The passes: K = BW_ROWS / G blocks of every datagram expanded by the
 * wave's lanes at once, then this lane's datagram's rounds over its rows. */
template <class H, int ROW>
__device__ __forceinline__ void bw_passes(typename H::State &s,
    const uint8_t *__restrict__ base, const BwGeo &geo, typename H::word *rows,
    uint32_t G, uint32_t lane, uint32_t nb, uint32_t nbmax)
{
	const uint32_t K = BW_ROWS / G, dl = lane % G;
	for (uint32_t c0 = 0; c0 < nbmax; c0 += K) {
		/* row `lane`: block c0 + lane % K of datagram lane / K */
		const uint32_t d = lane / K, k = c0 + lane % K;
		if (d < G && k < geo.nb[d]) {
			const uint32_t ml = geo.len[d];
			uint32_t w[H::NW32];
			bw_block<H>(base + geo.m[d], k, ml / H::BLOCK, ml % H::BLOCK,
			    geo.nb[d], ((uint64_t)ml + H::BLOCK) << 3, w);
			sched_row<H>(w, rows + lane * ROW);
		}
		wave_lds_sync();
		const uint32_t cnt = min(K, nbmax - c0);
		for (uint32_t b = 0; b < cnt; b++)
			if (c0 + b < nb)
				rounds_row<H>(s, rows + (dl * K + b) * ROW);
		wave_lds_sync();
	}
}

/* The outer hash's one block: inner digest || 0x80 || 0... || bit count. */
template <class H, bool IS384>
__device__ __forceinline__ void bw_outer_block(const typename H::State &s,
    uint32_t (&w)[H::NW32])
{
	constexpr int NW32 = H::NW32;
#pragma unroll
	for (int j = 0; j < NW32; j++)
		w[j] = 0;
	const int dw = digest_words<H>(s, IS384, w);
#pragma unroll
	for (int j = 12; j < 16; j++)		/* SHA-384 keeps 12 words */
		if (j >= dw)
			w[j] = 0;
	w[dw] = 0x80000000u;
	const uint64_t obits = (uint64_t)(H::BLOCK + 4 * dw) << 3;
	w[NW32 - 2] = (uint32_t)(obits >> 32);
	w[NW32 - 1] = (uint32_t)obits;
}

/* RX: the final code -- a refusal stands; otherwise the hash field against
 * the digest words o (net2_buffer_cmp, packet.n2t:253-257). */
template <uint32_t DLEN>
__device__ __forceinline__ uint32_t bw_rx_code(uint32_t st, bool hashed,
    const uint8_t *field, const uint32_t (&o)[16])
{
	if (st != PKT_OK)
		return st;
	uint32_t diff = 0;
	if (hashed) {
#pragma unroll
		for (uint32_t j = 0; j < DLEN; j++)
			diff |= field[j] ^ ((o[j >> 2] >> (8 * (j & 3))) & 0xffu);
	}
	return !hashed || diff != 0 ? PKT_BAD : PKT_OK;
}

/* RX: the IV that wave 1 left in LDS, for a datagram that verified. */
__device__ __forceinline__ void bw_store_iv(uint8_t *dst,
    const uint32_t (&ivw)[16], uint32_t ivlen)
{
	const uint8_t *src = reinterpret_cast<const uint8_t *>(ivw);
	for (uint32_t b = 0; b < ivlen; b++)
		dst[b] = src[b];
}

/* TX: header and hash field of a sealed datagram, at h. */
template <uint32_t DLEN>
__device__ __forceinline__ void bw_seal(uint8_t *h, uint32_t seq, uint32_t fl,
    const uint32_t (&o)[16])
{
#pragma unroll
	for (int b = 0; b < 4; b++) {
		h[b] = (uint8_t)(seq >> (24 - 8 * b));
		h[4 + b] = (uint8_t)(fl >> (24 - 8 * b));
	}
	store_digest<DLEN>(h + 8, o);
}

template <int MODE, uint32_t DLEN>
__device__ __forceinline__ BwDgram bw_decode(const uint8_t *__restrict__ base,
    const uint64_t *__restrict__ offsets, const uint32_t *__restrict__ lens,
    uint64_t i, const BurstArgs &rx)
{
	BwDgram g = {};		/* PKT_OK so far */
	g.off = offsets[i];
	const uint32_t len = lens[i];
	if (MODE == HMAC_BURST_TX) {
		g.seq = rx.seq[i];
		g.fl = rx.flags[i];
		g.st = bw_tx_code<DLEN>(g.fl, len, rx.enc_set != 0);
	} else {
		bw_rx_header(g, base + g.off, len);
		/* net2_ck_rx_key (src/conn_keys.c:447-476) */
		g.alt = g.st == PKT_OK && rx.alt &&
		    ((g.fl & PKT_PH_ALTKEY) != 0 || (!rx.no_cutoff &&
		    g.seq - rx.rx_start >= rx.cutoff - rx.rx_start));
		const int enc_set = g.alt ? rx.alt_enc_set : rx.enc_set;
		if (g.st == PKT_OK && ((g.fl & PKT_PH_SIGNED) == 0 ||
		    (enc_set && (g.fl & PKT_PH_ENCRYPTED) == 0)))
			g.st = PKT_UNSAFE;
	}
	bw_decode_end<DLEN>(g, len);
	return g;
}

template <class H, int MODE, bool IS384>
__global__ __launch_bounds__(128) void burst_wave_kernel(
    const uint8_t *__restrict__ base, const uint64_t *__restrict__ offsets,
    const uint32_t *__restrict__ lens, uint64_t n, uint32_t G, HMid hm,
    BurstArgs rx, uint8_t *__restrict__ result, uint8_t *__restrict__ iv,
    uint32_t ivlen, uint8_t *__restrict__ out)
{
	typedef typename H::word W;
	constexpr int ROW = sizeof(W) == 4 ? NET2_JOB_ROW256 : NET2_JOB_ROW512;
	constexpr uint32_t dlen = sizeof(W) == 4 ? 32 : IS384 ? 48 : 64;
	__shared__ W rows[BW_ROWS * ROW];
	__shared__ uint32_t mid[4][16];
	__shared__ uint32_t ivw[BW_GMAX][16];
	__shared__ uint64_t geo_m[BW_GMAX];
	__shared__ uint32_t geo_len[BW_GMAX], geo_nb[BW_GMAX];
	const BwGeo geo = { geo_m, geo_len, geo_nb };
	if (threadIdx.x == 0) {
		constexpr int NK = MODE == HMAC_BURST_RX ? 4 : 2;
		constexpr int NWD = sizeof(W) == 4 ? 8 : 16;
#pragma unroll
		for (int k = 0; k < NK; k++)
#pragma unroll
			for (int j = 0; j < NWD; j++)
				mid[k][j] = hm.w[k][j];
	}
	if (sizeof(W) == 8)
		k512_lds_fill();	/* (synchronises the workgroup) */
	else
		__syncthreads();
	const uint32_t lane = threadIdx.x & 63;
	const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	/* every lane of a wave works on datagram slot lane % G (the G slots
	 * replicated across the wave: rounds on one lane of a wave run slower
	 * than on all of them); lane d < G owns slot d's stores */
	const uint64_t i = (uint64_t)blockIdx.x * G + lane % G;
	const bool live = i < n;
	const bool mine = lane < G && live;	/* this lane stores datagram i */
	BwDgram g = {};
	if (live)
		g = bw_decode<MODE, dlen>(base, offsets, lens, i, rx);

	/* RX: the IV of an encrypted datagram that may verify */
	const bool wiv = MODE == HMAC_BURST_RX && mine && g.ok && ivlen > 0 &&
	    iv != nullptr && (g.fl & PKT_PH_ENCRYPTED);
	if (wv == 1) {
		if (wiv)
			ph_iv_one(g.seq, g.fl, ivlen,
			    reinterpret_cast<uint8_t *>(ivw[lane]));
		__syncthreads();
		return;
	}

	/* wave 0: HMAC of every owned message from its ipad midstate (a
	 * datagram already refused, or without room for its hash field,
	 * hashes nothing) */
	const uint32_t nb = bw_nblocks<H>(g.hashed, g.mlen);
	const uint32_t nbmax = bw_publish<dlen>(geo, lane, G, g.off, g.mlen, nb);
	const uint32_t (*lmid)[16] = g.alt ? mid + 2 : mid;
	typename H::State s;
	load_mid<H>(lmid, 0, s);
	bw_passes<H, ROW>(s, base, geo, rows, G, lane, nb, nbmax);
	if (g.hashed) {
		uint32_t w[H::NW32];
		bw_outer_block<H, IS384>(s, w);
		load_mid<H>(lmid, 1, s);
		H::compress(s, w);
	}
	materialize<H>(s);
	uint32_t o[16];
	H::out_words(s, o, IS384);
	__syncthreads();		/* wave 1's IVs are in LDS */
	if (!mine)
		return;
	if (MODE == HMAC_BURST_RX) {
		const uint32_t code = bw_rx_code<dlen>(g.st, g.hashed,
		    base + g.off + 8, o);
		if (rx.seq != nullptr) {
			rx.seq[i] = g.seq;
			rx.flags[i] = g.fl;
		}
		if (wiv && code == PKT_OK)
			bw_store_iv(iv + i * ivlen, ivw[lane], ivlen);
		result[i] = (uint8_t)code;
		return;
	}
	/* TX */
	if (rx.rec != nullptr) {
		uint8_t *r = rx.rec + i * (dlen + 16);
		if (g.hashed)
			store_digest<dlen>(r, o);
		*reinterpret_cast<uint4 *>(r + dlen) = make_uint4(
		    g.ok ? bswap32(g.seq) : 0u, g.ok ? bswap32(g.fl) : 0u,
		    (uint32_t)i, g.st);
		return;
	}
	if (g.hashed)
		bw_seal<dlen>(out + g.off, g.seq, g.fl, o);
	result[i] = (uint8_t)g.st;
}

/*
 * burst_wave_kernel's sibling for bursts over many connections
 * (net2_packet_{decode,encode}_burst_mc at most net2_burst_wave_max()
 * datagrams): the same two waves, G datagrams, K + W rows and passes, with
 * the keys of datagram i taken from entry conn[i] of the device key table as
 * hmac_mc_kernel's lanes take them -- no key in the arguments, none in LDS.
 * A kernel of its own, not an instance of a shared template body: the
 * single-connection instances keep their register allocation (DESIGN.md
 * 5.5.6).  What the two differ in is where keys and the NOCONN / UNSAFE
 * decisions come from; everything else is the bw_* pieces above.
 *
 * The 64 / G replica lanes of a datagram read the same conn[i], meta words
 * and midstates (one request per distinct address).  The entry's address is
 * held in two VGPRs across the pass loop: at two waves per SIMD there are
 * registers to spare, so the outer midstate is loaded from it where the outer
 * block needs it, without hmac_item's second look-up.  A lane with i >= n
 * reads neither conn nor the table.  Codes, headers, IVs and sealed fields are
 * those of hmac_item's _MC modes + burst_final_mc_kernel, bit for bit; there
 * is no rec form.
 */
template <int MODE, uint32_t DLEN>
__device__ __forceinline__ BwDgram bw_decode_mc(
    const uint8_t *__restrict__ base, const uint64_t *__restrict__ offsets,
    const uint32_t *__restrict__ lens, uint64_t i,
    const uint32_t *__restrict__ seq, const uint32_t *__restrict__ flags,
    const KeyTabArgs &kt)
{
	BwDgram g = {};		/* PKT_OK so far */
	g.off = offsets[i];
	const uint32_t len = lens[i];
	bool inr;
	g.ent = keytab_ent(kt, i, &inr);
	if (MODE == HMAC_BURST_TX_MC) {
		g.seq = seq[i];
		g.fl = flags[i];
		const uint32_t bits = inr ? g.ent->meta[0] : 0u;
		/* a slot without a tx key: NOCONN before anything else */
		g.st = (bits & NET2_KT_TX) == 0 ? PKT_NOCONN :
		    bw_tx_code<DLEN>(g.fl, len, (bits & NET2_KT_TX_ENC) != 0);
	} else {
		bw_rx_header(g, base + g.off, len);
		/* the connection's entry, looked at once the header is decoded
		 * (packet.n2t:210) */
		const uint4 mt = *reinterpret_cast<const uint4 *>(g.ent->meta);
		const uint32_t bits = inr ? mt.x : 0u;
		g.alt = g.st == PKT_OK &&
		    keytab_rx_alt(bits, mt.y, mt.z, g.seq, g.fl);
		g.ciph = (bits & NET2_KT_RX_ENC) != 0;
		if (g.st == PKT_OK && (bits & NET2_KT_RX) == 0)
			g.st = PKT_NOCONN;	/* no rx key: nothing hashed */
		if (g.st == PKT_OK && ((g.fl & PKT_PH_SIGNED) == 0 ||
		    (g.ciph && (g.fl & PKT_PH_ENCRYPTED) == 0)))
			g.st = PKT_UNSAFE;
	}
	bw_decode_end<DLEN>(g, len);
	return g;
}

template <class H, int MODE, bool IS384>
__global__ __launch_bounds__(128) void burst_wave_mc_kernel(
    const uint8_t *__restrict__ base, const uint64_t *__restrict__ offsets,
    const uint32_t *__restrict__ lens, uint64_t n, uint32_t G,
    const uint32_t *__restrict__ conn, const Net2KeyEnt *__restrict__ tab,
    uint32_t slots, uint32_t *seq, uint32_t *flags,
    uint8_t *__restrict__ result, uint8_t *__restrict__ iv, uint32_t ivlen,
    uint8_t *__restrict__ out)
{
	typedef typename H::word W;
	constexpr int ROW = sizeof(W) == 4 ? NET2_JOB_ROW256 : NET2_JOB_ROW512;
	constexpr uint32_t dlen = sizeof(W) == 4 ? 32 : IS384 ? 48 : 64;
	constexpr bool RX = MODE == HMAC_BURST_RX_MC;
	__shared__ W rows[BW_ROWS * ROW];
	__shared__ uint32_t ivw[BW_GMAX][16];
	__shared__ uint64_t geo_m[BW_GMAX];
	__shared__ uint32_t geo_len[BW_GMAX], geo_nb[BW_GMAX];
	const BwGeo geo = { geo_m, geo_len, geo_nb };
	if (sizeof(W) == 8)
		k512_lds_fill();	/* (synchronises the workgroup) */
	const uint32_t lane = threadIdx.x & 63;
	const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	/* as burst_wave_kernel: slot lane % G, lane d < G owns slot d's stores */
	const uint64_t i = (uint64_t)blockIdx.x * G + lane % G;
	const bool live = i < n;
	const bool mine = lane < G && live;	/* this lane stores datagram i */
	const KeyTabArgs kt = { conn, tab, slots };
	BwDgram g = {};
	if (live)
		g = bw_decode_mc<MODE, dlen>(base, offsets, lens, i, seq, flags, kt);

	/* RX: the IV of an encrypted datagram that may verify, on a connection
	 * with a cipher key */
	const bool wiv = RX && mine && g.ok && g.ciph && ivlen > 0 &&
	    iv != nullptr && (g.fl & PKT_PH_ENCRYPTED);
	if (wv == 1) {
		if (wiv)
			ph_iv_one(g.seq, g.fl, ivlen,
			    reinterpret_cast<uint8_t *>(ivw[lane]));
		__syncthreads();
		return;
	}

	/* wave 0: HMAC of every owned message from its connection's ipad
	 * midstate (a datagram already refused, or without room for its hash
	 * field, hashes nothing and loads no midstate) */
	const uint32_t nb = bw_nblocks<H>(g.hashed, g.mlen);
	const uint32_t nbmax = bw_publish<dlen>(geo, lane, G, g.off, g.mlen, nb);
	typename H::State s;
#pragma unroll
	for (int j = 0; j < 8; j++)
		s[j] = 0;
	if (g.hashed)
		load_mid_tab<H>(RX ? g.ent->rx[g.alt ? 2 : 0] : g.ent->tx[0], s);
	bw_passes<H, ROW>(s, base, geo, rows, G, lane, nb, nbmax);
	/* the outer block from the opad midstate of the key the inner hash ran
	 * under */
	if (g.hashed) {
		uint32_t w[H::NW32];
		bw_outer_block<H, IS384>(s, w);
		load_mid_tab<H>(RX ? g.ent->rx[g.alt ? 3 : 1] : g.ent->tx[1], s);
		H::compress(s, w);
	}
	materialize<H>(s);
	uint32_t o[16];
	H::out_words(s, o, IS384);
	__syncthreads();		/* wave 1's IVs are in LDS */
	if (!mine)
		return;
	if (RX) {
		const uint32_t code = bw_rx_code<dlen>(g.st, g.hashed,
		    base + g.off + 8, o);
		if (seq != nullptr) {
			seq[i] = g.seq;
			flags[i] = g.fl;
		}
		if (wiv && code == PKT_OK)
			bw_store_iv(iv + i * ivlen, ivw[lane], ivlen);
		result[i] = (uint8_t)code;
		return;
	}
	/* TX: a slot that is not sealed (NOCONN included) is left untouched */
	if (g.hashed)
		bw_seal<dlen>(out + g.off, g.seq, g.fl, o);
	result[i] = (uint8_t)g.st;
}

} /* namespace dev */
} /* namespace net2 */

#endif /* NET2_SHA2_BURST_WAVE_H */
