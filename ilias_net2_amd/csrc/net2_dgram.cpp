/*
 * net2_dgram.cpp -- the calls on device-resident datagrams: HMAC sign /
 * verify and header IVs, the packet bursts, the payload cipher, the key tables
 * and the bursts over many connections (include/net2/packet.h).  Argument
 * checks and launches in the caller's stream; nothing is staged here.
 */
#include "net2_host.h"
#include "aes_launch.h"

#include <atomic>
#include <new>

/* Argument checks shared by the datagram sign / verify entry points. */
static int check_dgram_args(int alg, const void *key, size_t keylen,
    const void *d_base, const uint64_t *d_offsets, const uint32_t *d_lens,
    uint64_t n, const void *d_ws, size_t ws_bytes)
{
	if (!hmac_key_ok(alg, key, keylen, false))
		return EINVAL;
	if (n == 0)
		return 0;
	/* (without a workspace, no limit on n: nothing is indexed by it) */
	if (d_base == nullptr || d_offsets == nullptr || d_lens == nullptr ||
	    !bin_ws_ok(d_ws, ws_bytes, n))
		return EINVAL;
	return check_current_device();
}

NET2_EXPORT int net2_hmac_sign_dev(int alg, const void *key, size_t keylen,
    void *d_base, const uint64_t *d_offsets, const uint32_t *d_lens,
    uint64_t n, void *d_ws, size_t ws_bytes, void *stream)
{
	int rc = check_dgram_args(alg, key, keylen, d_base, d_offsets, d_lens,
	    n, d_ws, ws_bytes);
	if (rc != 0 || n == 0)
		return rc;
	HIP_TRY(net2_launch_hmac(alg, (const uint8_t *)key, nullptr, keylen,
	    (const uint8_t *)d_base, d_offsets, d_lens, 0, 0, n,
	    (uint8_t *)d_base, (uint32_t *)d_ws, (hipStream_t)stream,
	    NET2_HMAC_MODE_SIGN));
	return 0;
}

NET2_EXPORT int net2_hmac_verify_dev(int alg, const void *key,
    size_t keylen, const void *d_base, const uint64_t *d_offsets,
    const uint32_t *d_lens, uint64_t n, uint8_t *d_result, void *d_ws,
    size_t ws_bytes, void *stream)
{
	int rc = check_dgram_args(alg, key, keylen, d_base, d_offsets, d_lens,
	    n, d_ws, ws_bytes);
	if (rc != 0 || n == 0)
		return rc;
	if (d_result == nullptr)
		return EINVAL;
	HIP_TRY(net2_launch_hmac(alg, (const uint8_t *)key, nullptr, keylen,
	    (const uint8_t *)d_base, d_offsets, d_lens, 0, 0, n, d_result,
	    (uint32_t *)d_ws, (hipStream_t)stream, NET2_HMAC_MODE_VERIFY));
	return 0;
}

NET2_EXPORT int net2_hmac_dev(int alg, const void *key, size_t keylen,
    const void *d_base, const uint64_t *d_offsets, const uint32_t *d_lens,
    uint64_t stride, uint32_t fixed_len, uint64_t n, void *d_digests,
    void *d_ws, size_t ws_bytes, void *stream)
{
	if (!hmac_key_ok(alg, key, keylen, false))
		return EINVAL;
	if (n == 0)
		return 0;
	if (d_digests == nullptr)
		return EINVAL;
	if (d_offsets != nullptr) {
		if (d_lens == nullptr || !bin_ws_ok(d_ws, ws_bytes, n))
			return EINVAL;
	} else {
		if (d_base == nullptr && fixed_len > 0)
			return EINVAL;
		if (n > 1 && stride < fixed_len)
			return EINVAL;
	}
	if (int rc = check_current_device())
		return rc;
	HIP_TRY(net2_launch_hmac(alg, (const uint8_t *)key, nullptr, keylen,
	    (const uint8_t *)d_base, d_offsets, d_lens, stride, fixed_len, n,
	    (uint8_t *)d_digests, d_offsets ? (uint32_t *)d_ws : nullptr,
	    (hipStream_t)stream));
	return 0;
}

NET2_EXPORT int net2_ph_to_iv_dev(const uint32_t *d_seq,
    const uint32_t *d_flags, uint64_t n, uint32_t ivlen, void *d_iv,
    void *stream)
{
	if (n == 0 || ivlen == 0)
		return 0;
	if (ivlen > 64 || d_seq == nullptr || d_flags == nullptr ||
	    d_iv == nullptr)
		return EINVAL;
	if (int rc = check_current_device())
		return rc;
	HIP_TRY(net2_launch_ph_iv(d_seq, d_flags, n, ivlen, (uint8_t *)d_iv,
	    (hipStream_t)stream));
	return 0;
}

/* ---- packet bursts (include/net2/packet.h) --------------------------------- */

/* Workspace of a burst, carved in this order, every piece 16-byte aligned:
 * the binning scratch first -- its header and histograms at offset 0 for
 * every n, so one workspace serves bursts of any size up to its own and
 * net2_sha2_workspace_init / _stats apply to it -- then region offsets and
 * lengths for the prep kernel, status and verdict bytes, decoded headers. */
struct BurstWs {
	uint64_t *sub_off;
	uint32_t *sub_len;
	uint8_t *status, *verdict;
	uint32_t *seq, *flags;
	uint32_t *bin;
};

size_t burst_layout(uint64_t n, uint8_t *base, BurstWs *w)
{
	size_t at = 0;
	auto take = [&](size_t bytes) {
		uint8_t *p = base ? base + at : nullptr;
		at += a16(bytes);
		return p;
	};
	uint32_t *bn = (uint32_t *)take(((size_t)NET2_BIN_WS_WORDS + n) * 4);
	uint64_t *so = (uint64_t *)take(8 * n);
	uint32_t *sl = (uint32_t *)take(4 * n);
	uint8_t *st = take(n);
	uint8_t *vd = take(n);
	uint32_t *sq = (uint32_t *)take(4 * n);
	uint32_t *fl = (uint32_t *)take(4 * n);
	if (w != nullptr)
		*w = { so, sl, st, vd, sq, fl, bn };
	return at;
}

/* The cipher calls (net2_host.h): aes256 with a 32-byte key, and as long an alternate key
 * or none */
int check_cipher_keys(const struct net2_burst_cipher_keys *ck)
{
	if (ck == nullptr || ck->enc_alg != NET2_ENC_AES256)
		return EINVAL;
	if (ck->enc_key == nullptr || ck->enc_keylen != NET2_AES_KEYLEN)
		return EINVAL;
	if (ck->alt_enc_key != nullptr && ck->alt_enc_keylen != NET2_AES_KEYLEN)
		return EINVAL;
	return 0;
}

namespace {

/* A workspace of an n-datagram burst (n <= UINT32_MAX): there, as large as
 * the layout and 16-byte aligned. */
bool burst_ws_ok(const void *d_ws, size_t ws_bytes, uint64_t n)
{
	return d_ws != nullptr && ws_bytes >= burst_layout(n, nullptr, nullptr) &&
	    ((uintptr_t)d_ws & 15) == 0;
}

/* hash_alg 0 (none) or an HMAC row with its key; ivlen <= 64 */
int check_burst_args(int hash_alg, const void *key, size_t keylen,
    uint32_t ivlen, const void *d_base, const uint64_t *d_offsets,
    const uint32_t *d_lens, uint64_t n, const uint8_t *d_result,
    const void *d_ws, size_t ws_bytes)
{
	if (!hmac_key_ok(hash_alg, key, keylen, true))
		return EINVAL;
	int rc = check_burst_arrays(ivlen, d_base, d_offsets, d_lens, n, d_result);
	if (rc != 0 || n == 0)
		return rc;
	return burst_ws_ok(d_ws, ws_bytes, n) ? check_current_device() : EINVAL;
}

/* net2_sha2_burst_limits' two thresholds, net2_aes_burst_limits' one,
 * net2_aes_encrypt_limits' one */
FormKnob g_burst_wave_max{"NET2_BURST_WAVE_MAX"};
FormKnob g_burst_bin_min{"NET2_BURST_BIN_MIN"};
FormKnob g_aes_wave_max{"NET2_AES_WAVE_MAX"};
FormKnob g_aes_quad_max{"NET2_AES_QUAD_MAX"};

/* net2_sha2_burst_stats' counts (keyed hash-burst launches) and
 * net2_aes_burst_stats' (decrypt launches); net2_aes_encrypt_stats' (encrypt
 * launches: `wave` counts the quad form) */
FormCounts g_burst_launches, g_aes_launches, g_aes_tx_launches;

/*
 * The binning workspace a burst's HMAC kernel is given: below the binning
 * threshold (default 65,536 datagrams: one lane per datagram, one wave per
 * SIMD) none -- every wave then has a SIMD of its own, the burst takes its
 * longest wave's time whatever the order, and the binning launch is pure
 * fixed cost (tools/burst_sizes.py).
 */
uint32_t *burst_bins(uint64_t n, uint32_t *bin)
{
	return n >= g_burst_bin_min.get(65536) ? bin : nullptr;
}

/* After a keyed hash-burst launch: its form counted, then the fault
 * injection point of a chunk's first kernel. */
int burst_launched(bool wave)
{
	g_burst_launches.count(wave);
	FI_POINT(FI_KERNEL);
	return 0;
}

}	/* namespace */

uint64_t net2_burst_wave_max(void)
{
	uint64_t v;
	return g_burst_wave_max.get(&v) ? v : net2_burst_wave_default();
}

/*
 * The hash steps of net2_packet_decode for a device-resident burst.
 * hdr_out: d_seq / d_flags are copies the final kernel makes (the host
 * path: mapped host memory) -- the HMAC kernel keeps the decoded headers in
 * the workspace; otherwise they are where the HMAC kernel decodes to.
 */
int decode_burst(const struct net2_burst_rx_keys *k, uint32_t ivlen,
    const void *d_base, const uint64_t *d_offsets, const uint32_t *d_lens,
    uint64_t n, uint8_t *d_result, void *d_iv, uint32_t *d_seq,
    uint32_t *d_flags, void *d_ws, hipStream_t s, bool hdr_out, bool wave)
{
	const int hash_alg = k->hash_alg;
	const int hash_set = hash_alg != NET2_HASH_NIL;
	const bool alt = hash_set && k->alt_hash_key != nullptr;
	BurstWs w;
	burst_layout(n, (uint8_t *)d_ws, &w);
	uint32_t *seq = d_seq && !hdr_out ? d_seq : w.seq;
	uint32_t *flags = d_flags && !hdr_out ? d_flags : w.flags;
	const int enc_set = k->enc_alg != 0;
	if (hash_set) {
		/* header decode, key choice, flag checks and HMAC verify in one
		 * kernel over the wire datagrams (binned by datagram length) */
		const uint8_t *const key = (const uint8_t *)k->hash_key;
		const uint8_t *const altkey =
		    alt ? (const uint8_t *)k->alt_hash_key : nullptr;
		/* the kernel's inputs from the connection's keys: no key bytes
		 * (the launcher turns those into midstates) */
		BurstArgs rx = {};
		rx.enc_set = enc_set;
		if (alt) {
			rx.alt = 1;
			rx.alt_enc_set = enc_set;
			rx.no_cutoff = k->alt_no_cutoff != 0;
			rx.cutoff = k->alt_cutoff;
			rx.rx_start = k->rx_start;
		}
		if (wave) {
			/* a small burst: 1 to 16 datagrams per workgroup,
			 * codes, headers and IVs stored by that one launch */
			rx.seq = d_seq;
			rx.flags = d_flags;
			HIP_TRY(net2_launch_burst_wave(hash_alg, key, altkey,
			    k->hash_keylen, (const uint8_t *)d_base, d_offsets,
			    d_lens, n, &rx, d_result,
			    enc_set ? (uint8_t *)d_iv : nullptr, enc_set ? ivlen : 0,
			    nullptr, NET2_HMAC_MODE_BURST_RX, s));
			return burst_launched(true);
		}
		rx.seq = seq;
		rx.flags = flags;
		rx.status = w.status;
		HIP_TRY(net2_launch_hmac(hash_alg, key, altkey, k->hash_keylen,
		    (const uint8_t *)d_base, d_offsets, d_lens, 0, 0, n, w.verdict,
		    burst_bins(n, w.bin), s, NET2_HMAC_MODE_BURST_RX, &rx));
		if (int rc = burst_launched(false))
			return rc;
	} else {
		HIP_TRY(net2_launch_burst_prep((uint8_t *)d_base, d_offsets,
		    d_lens, n, 0, 0, enc_set, 0, nullptr, nullptr, seq,
		    flags, w.sub_off, w.sub_len, w.status, s));
		FI_POINT(FI_KERNEL);
	}
	HIP_TRY(net2_launch_burst_final(n, w.status, w.verdict, seq, flags,
	    enc_set ? ivlen : 0, (uint8_t *)d_iv, d_result, s,
	    hdr_out ? d_seq : nullptr, hdr_out ? d_flags : nullptr));
	return 0;
}

/*
 * The hash steps of net2_packet_encode for a device-resident burst.  rec
 * (keyed hash only): header and hash field of every datagram to a record of
 * their own (BurstArgs::rec) instead of into d_base.  bin: length-bin the
 * burst at or above the threshold (burst_bins); the host path passes false
 * where the order of the records matters more than the kernel's time.
 */
int encode_burst(int hash_alg, const void *hash_key, size_t hash_keylen,
    int enc_alg, const uint32_t *d_seq, const uint32_t *d_flags,
    void *d_base, const uint64_t *d_offsets, const uint32_t *d_lens,
    uint64_t n, uint8_t *d_result, void *d_ws, hipStream_t s, bool wave,
    uint8_t *rec, bool bin, uint8_t *seal_to)
{
	/* seal_to (keyed, no rec): headers and hash fields go there, at the
	 * datagrams' offsets, instead of into d_base (the host path: the
	 * caller's page-locked buffer through its device mapping) */
	uint8_t *const out = seal_to != nullptr ? seal_to : (uint8_t *)d_base;
	BurstWs w;
	burst_layout(n, (uint8_t *)d_ws, &w);
	if (hash_alg != NET2_HASH_NIL) {
		/* flag and room checks, header write and HMAC sign in one
		 * kernel over the wire datagrams; the TX code is final (no
		 * verdict to fold in), so the kernel writes it to d_result */
		BurstArgs tx = {};
		tx.seq = const_cast<uint32_t *>(d_seq);
		tx.flags = const_cast<uint32_t *>(d_flags);
		tx.status = d_result;
		tx.enc_set = enc_alg != 0;
		tx.rec = rec;
		if (wave) {
			/* a small burst: 1 to 16 datagrams per workgroup */
			HIP_TRY(net2_launch_burst_wave(hash_alg,
			    (const uint8_t *)hash_key, nullptr, hash_keylen,
			    (const uint8_t *)d_base, d_offsets, d_lens, n, &tx,
			    d_result, nullptr, 0, out, NET2_HMAC_MODE_BURST_TX, s));
			return burst_launched(true);
		}
		HIP_TRY(net2_launch_hmac(hash_alg, (const uint8_t *)hash_key,
		    nullptr, hash_keylen, (const uint8_t *)d_base, d_offsets,
		    d_lens, 0, 0, n, out, bin ? burst_bins(n, w.bin) : nullptr, s,
		    NET2_HMAC_MODE_BURST_TX, &tx));
		return burst_launched(false);
	}
	HIP_TRY(net2_launch_burst_prep((uint8_t *)d_base, d_offsets,
	    d_lens, n, 1, 0, enc_alg != 0, 0, d_seq, d_flags, nullptr,
	    nullptr, w.sub_off, w.sub_len, w.status, s));
	FI_POINT(FI_KERNEL);
	HIP_TRY(net2_launch_burst_final(n, w.status, nullptr, d_seq, d_flags, 0,
	    nullptr, d_result, s));
	return 0;
}

NET2_EXPORT size_t net2_packet_burst_workspace(uint64_t n)
{
	return burst_layout(n, nullptr, nullptr);
}

NET2_EXPORT int net2_sha2_burst_limits(int64_t wave_max, int64_t bin_min)
{
	g_burst_wave_max.set(wave_max);
	g_burst_bin_min.set(bin_min);
	return 0;
}

NET2_EXPORT int net2_sha2_burst_stats(uint64_t *lane_launches,
    uint64_t *wave_launches)
{
	g_burst_launches.read(lane_launches, wave_launches);
	return 0;
}

NET2_EXPORT int net2_packet_decode_burst_ck(const struct net2_burst_rx_keys *k,
    uint32_t ivlen, const void *d_base, const uint64_t *d_offsets,
    const uint32_t *d_lens, uint64_t n, uint8_t *d_result, void *d_iv,
    uint32_t *d_seq, uint32_t *d_flags, void *d_ws, size_t ws_bytes,
    void *stream)
{
	if (k == nullptr)
		return EINVAL;
	int rc = check_burst_args(k->hash_alg, k->hash_key, k->hash_keylen,
	    ivlen, d_base, d_offsets, d_lens, n, d_result, d_ws, ws_bytes);
	if (rc != 0)
		return rc;
	/* an alternate key is new key material under the same algorithms */
	const bool alt = k->hash_alg != NET2_HASH_NIL &&
	    k->alt_hash_key != nullptr;
	if (alt && k->alt_hash_keylen != k->hash_keylen)
		return EINVAL;
	if (n == 0)
		return 0;
	if ((d_seq == nullptr) != (d_flags == nullptr))
		return EINVAL;
	return decode_burst(k, ivlen, d_base, d_offsets, d_lens, n, d_result,
	    d_iv, d_seq, d_flags, d_ws, (hipStream_t)stream, false,
	    n <= net2_burst_wave_max());
}

NET2_EXPORT int net2_packet_decode_burst(int hash_alg, const void *hash_key,
    size_t hash_keylen, int enc_alg, uint32_t ivlen, const void *d_base,
    const uint64_t *d_offsets, const uint32_t *d_lens, uint64_t n,
    uint8_t *d_result, void *d_iv, uint32_t *d_seq, uint32_t *d_flags,
    void *d_ws, size_t ws_bytes, void *stream)
{
	struct net2_burst_rx_keys k = {};
	k.hash_alg = hash_alg;
	k.hash_key = hash_key;
	k.hash_keylen = hash_keylen;
	k.enc_alg = enc_alg;
	return net2_packet_decode_burst_ck(&k, ivlen, d_base, d_offsets, d_lens,
	    n, d_result, d_iv, d_seq, d_flags, d_ws, ws_bytes, stream);
}

NET2_EXPORT int net2_packet_encode_burst(int hash_alg, const void *hash_key,
    size_t hash_keylen, int enc_alg, const uint32_t *d_seq,
    const uint32_t *d_flags, void *d_base, const uint64_t *d_offsets,
    const uint32_t *d_lens, uint64_t n, uint8_t *d_result, void *d_ws,
    size_t ws_bytes, void *stream)
{
	int rc = check_burst_args(hash_alg, hash_key, hash_keylen, 0, d_base,
	    d_offsets, d_lens, n, d_result, d_ws, ws_bytes);
	if (rc != 0 || n == 0)
		return rc;
	if (d_seq == nullptr || d_flags == nullptr)
		return EINVAL;
	return encode_burst(hash_alg, hash_key, hash_keylen, enc_alg, d_seq,
	    d_flags, d_base, d_offsets, d_lens, n, d_result, d_ws,
	    (hipStream_t)stream, n <= net2_burst_wave_max(), nullptr);
}

/* ---- the payload cipher of the bursts (aes_kernels.hip) -------------------- */

namespace {

/*
 * The largest burst decrypted in the wave form (one wave per datagram): the
 * measured crossover of tools/aes_burst_sizes.py (DESIGN.md 5.5.5,
 * profiles/aes_burst_wave/sizes.jsonl): the largest measured size at which,
 * as at every smaller one, the wave form beat the lane form by more than the
 * lane form's own spread (209 against 283 us there; at 262,144 datagrams one
 * lane per datagram fills the device and wins, 493 against 683 us).
 */
constexpr uint64_t AES_WAVE_MAX_DEFAULT = 65536;

}	/* namespace */

/* Whether a decrypt burst of n takes the wave form. */
bool aes_wave_form(uint64_t n)
{
	return n <= g_aes_wave_max.get(AES_WAVE_MAX_DEFAULT);
}

namespace {

/*
 * The largest burst encrypted in the quad form (four lanes per datagram), by
 * the same rule from tools/aes_burst_sizes.py --direction tx (DESIGN.md
 * 5.5.7, profiles/aes_burst_quad/sizes.jsonl): 188 against 275 us there, 97 to
 * 104 against 241 to 258 us up to 16,384 datagrams; at 262,144 one lane per
 * datagram wins, 436 against 696 us.
 */
constexpr uint64_t AES_QUAD_MAX_DEFAULT = 65536;

}	/* namespace */

/* Whether an encrypt burst of n takes the quad form. */
bool aes_quad_form(uint64_t n)
{
	return n <= g_aes_quad_max.get(AES_QUAD_MAX_DEFAULT);
}

NET2_EXPORT int net2_aes_encrypt_limits(int64_t quad_max)
{
	g_aes_quad_max.set(quad_max);
	return 0;
}

NET2_EXPORT int net2_aes_encrypt_stats(uint64_t *lane_launches,
    uint64_t *quad_launches)
{
	g_aes_tx_launches.read(lane_launches, quad_launches);
	return 0;
}

NET2_EXPORT int net2_aes_burst_limits(int64_t wave_max)
{
	g_aes_wave_max.set(wave_max);
	return 0;
}

NET2_EXPORT int net2_aes_burst_stats(uint64_t *lane_launches,
    uint64_t *wave_launches)
{
	g_aes_launches.read(lane_launches, wave_launches);
	return 0;
}

NET2_EXPORT int net2_packet_decrypt_burst(const struct net2_burst_rx_keys *k,
    const struct net2_burst_cipher_keys *ck, const void *d_base,
    const uint64_t *d_offsets, const uint32_t *d_lens, uint64_t n,
    const uint32_t *d_seq, const uint32_t *d_flags, const void *d_iv,
    uint8_t *d_result, void *d_out, uint32_t *d_plen, void *stream)
{
	if (k == nullptr || check_cipher_keys(ck) != 0)
		return EINVAL;
	if (k->hash_alg != NET2_HASH_NIL && !hmac_row(k->hash_alg))
		return EINVAL;
	/* the alternate cipher key goes with the alternate hash key: the HMAC
	 * step's choice of key set is the one made here */
	const bool alt = k->alt_hash_key != nullptr;
	if (alt && (k->hash_alg == NET2_HASH_NIL || ck->alt_enc_key == nullptr))
		return EINVAL;
	if (n == 0)
		return 0;
	if (!dgrams_ok(d_base, d_offsets, d_lens, n) || d_flags == nullptr ||
	    d_iv == nullptr || d_result == nullptr || d_out == nullptr ||
	    d_plen == nullptr || (alt && d_seq == nullptr))
		return EINVAL;
	if (int rc = check_current_device())
		return rc;
	const AesRxAlt ra = { alt ? (const uint8_t *)ck->alt_enc_key : nullptr,
	    k->alt_no_cutoff, k->alt_cutoff, k->rx_start };
	/* a small burst: one wave per datagram (results are the same) */
	const bool wave = aes_wave_form(n);
	HIP_TRY((wave ? net2_launch_aes_decrypt_wave : net2_launch_aes_decrypt)(
	    (const uint8_t *)ck->enc_key, ra,
	    k->hash_alg != NET2_HASH_NIL ? (uint32_t)digest_len(k->hash_alg) : 0,
	    (const uint8_t *)d_base, d_offsets, d_lens, n, d_seq, d_flags,
	    (const uint8_t *)d_iv, d_result, (uint8_t *)d_out, d_plen,
	    (hipStream_t)stream));
	g_aes_launches.count(wave);
	return 0;
}

NET2_EXPORT int net2_packet_encrypt_burst(
    const struct net2_burst_cipher_keys *ck, uint32_t hashlen,
    const uint32_t *d_flags, const void *d_iv, void *d_base,
    const uint64_t *d_offsets, const uint32_t *d_lens, const uint32_t *d_plen,
    uint64_t n, uint8_t *d_result, uint32_t *d_wire_len, void *stream)
{
	if (check_cipher_keys(ck) != 0)
		return EINVAL;
	if (hashlen != 0 && hashlen != 32 && hashlen != 48 && hashlen != 64)
		return EINVAL;
	if (n == 0)
		return 0;
	if (!dgrams_ok(d_base, d_offsets, d_lens, n) || d_flags == nullptr ||
	    d_iv == nullptr || d_plen == nullptr || d_result == nullptr ||
	    d_wire_len == nullptr)
		return EINVAL;
	if (int rc = check_current_device())
		return rc;
	/* a small burst: four lanes per datagram (results are the same) */
	const bool quad = aes_quad_form(n);
	HIP_TRY((quad ? net2_launch_aes_encrypt_quad : net2_launch_aes_encrypt)(
	    (const uint8_t *)ck->enc_key, hashlen, d_flags, (const uint8_t *)d_iv,
	    (uint8_t *)d_base, d_offsets, d_lens, d_plen, n, d_result, d_wire_len,
	    (hipStream_t)stream));
	g_aes_tx_launches.count(quad);
	return 0;
}

/* ---- keyed bursts over many connections: the device key table ------------- */

/* (struct net2_burst_keytab: net2_host.h) */

/* Arguments first (by the caller), then: a usable device, and the table's. */
int check_table_device(int device)
{
	int cur = -1;
	if (int rc = check_current_device())
		return rc;
	if (hipGetDevice(&cur) != hipSuccess)
		return ENODEV;
	return cur == device ? 0 : EINVAL;
}

namespace {

int check_keytab_device(const struct net2_burst_keytab *tab)
{
	return check_table_device(tab->device);
}

/* What the two _mc calls share: net2_packet_*_burst's checks with a table
 * and a connection index per datagram in place of the key. */
int check_burst_mc_args(const struct net2_burst_keytab *tab,
    const uint32_t *d_conn, uint32_t ivlen, const void *d_base,
    const uint64_t *d_offsets, const uint32_t *d_lens, uint64_t n,
    const uint8_t *d_result, const void *d_ws, size_t ws_bytes,
    bool hdr_pair_ok)
{
	if (tab == nullptr)
		return EINVAL;
	int rc = check_burst_arrays(ivlen, d_base, d_offsets, d_lens, n, d_result);
	if (rc != 0 || n == 0)
		return rc;
	if (d_conn == nullptr || !hdr_pair_ok || !burst_ws_ok(d_ws, ws_bytes, n))
		return EINVAL;
	return check_keytab_device(tab);
}

}	/* namespace */

NET2_EXPORT int net2_burst_keytab_create(int hash_alg, uint32_t slots,
    struct net2_burst_keytab **tab)
{
	if (tab == nullptr)
		return EINVAL;
	*tab = nullptr;
	if (!hmac_row(hash_alg) || slots == 0)
		return EINVAL;
	if (int rc = check_current_device())
		return rc;
	std::unique_ptr<net2_burst_keytab> t(new (std::nothrow) net2_burst_keytab());
	if (!t)
		return ENOMEM;
	if (hipGetDevice(&t->device) != hipSuccess)
		return ENODEV;
	t->hash_alg = hash_alg;
	t->slots = slots;
	const size_t bytes = (size_t)slots * sizeof(Net2KeyEnt);
	HIP_TRY(hipMalloc((void **)&t->ents, bytes));
	/* every slot unset before the first call that could read it, whatever
	 * stream that call uses */
	hipError_t e = hipMemset(t->ents, 0, bytes);
	if (e == hipSuccess)
		e = hipDeviceSynchronize();
	if (e != hipSuccess) {
		(void)hipFree(t->ents);
		return hip_fail(e);
	}
	*tab = t.release();
	return 0;
}

NET2_EXPORT void net2_burst_keytab_destroy(struct net2_burst_keytab *tab)
{
	if (tab == nullptr)
		return;
	/* the bulk updates' staging: its launches waited for, wiped, freed */
	tab_stage_destroy(tab->stage);
	/* (hipFree waits for the work that may still read the entries) */
	(void)hipFree(tab->ents);
	delete tab;
}

NET2_EXPORT int net2_burst_keytab_set_rx(struct net2_burst_keytab *tab,
    uint32_t slot, const struct net2_burst_rx_keys *keys, void *stream)
{
	if (tab == nullptr || keys == nullptr || slot >= tab->slots)
		return EINVAL;
	if (keys->hash_alg != tab->hash_alg || keys->hash_key == nullptr ||
	    keys->hash_keylen != (size_t)kRows[tab->hash_alg].keylen)
		return EINVAL;
	const bool alt = keys->alt_hash_key != nullptr;
	if (alt && keys->alt_hash_keylen != keys->hash_keylen)
		return EINVAL;
	if (int rc = check_keytab_device(tab))
		return rc;
	const uint32_t bits = NET2_KT_RX | (keys->enc_alg != 0 ? NET2_KT_RX_ENC : 0) |
	    (alt ? NET2_KT_RX_ALT : 0) |
	    (alt && keys->alt_no_cutoff != 0 ? NET2_KT_RX_NOCUT : 0);
	HIP_TRY(net2_launch_keytab_set(tab->hash_alg, tab->ents + slot, NET2_KT_RX,
	    (const uint8_t *)keys->hash_key, (const uint8_t *)keys->alt_hash_key,
	    keys->hash_keylen, bits, alt ? keys->alt_cutoff : 0,
	    alt ? keys->rx_start : 0, (hipStream_t)stream));
	tab_slot_launched();
	return 0;
}

NET2_EXPORT int net2_burst_keytab_set_tx(struct net2_burst_keytab *tab,
    uint32_t slot, const void *key, size_t keylen, int enc_alg, void *stream)
{
	if (tab == nullptr || key == nullptr || slot >= tab->slots ||
	    keylen != (size_t)kRows[tab->hash_alg].keylen)
		return EINVAL;
	if (int rc = check_keytab_device(tab))
		return rc;
	HIP_TRY(net2_launch_keytab_set(tab->hash_alg, tab->ents + slot, NET2_KT_TX,
	    (const uint8_t *)key, nullptr, keylen,
	    NET2_KT_TX | (enc_alg != 0 ? NET2_KT_TX_ENC : 0), 0, 0,
	    (hipStream_t)stream));
	tab_slot_launched();
	return 0;
}

NET2_EXPORT int net2_burst_keytab_clear(struct net2_burst_keytab *tab,
    uint32_t slot, void *stream)
{
	if (tab == nullptr || slot >= tab->slots)
		return EINVAL;
	if (int rc = check_keytab_device(tab))
		return rc;
	HIP_TRY(net2_launch_keytab_set(tab->hash_alg, tab->ents + slot, 0, nullptr,
	    nullptr, 0, 0, 0, 0, (hipStream_t)stream));
	tab_slot_launched();
	return 0;
}

int keytab_device(const struct net2_burst_keytab *tab)
{
	return tab->device;
}

int keytab_hash_alg(const struct net2_burst_keytab *tab)
{
	return tab->hash_alg;
}

/* net2_packet_decode_burst_mc's launches, the arguments checked. */
int decode_burst_mc(const struct net2_burst_keytab *tab, const uint32_t *d_conn,
    uint32_t ivlen, const void *d_base, const uint64_t *d_offsets,
    const uint32_t *d_lens, uint64_t n, uint8_t *d_result, void *d_iv,
    uint32_t *d_seq, uint32_t *d_flags, void *d_ws, hipStream_t s, bool wave)
{
	const KeyTabArgs kt = { d_conn, tab->ents, tab->slots };
	if (wave) {
		/* a small burst: 1 to 16 datagrams per workgroup; codes, headers
		 * and IVs stored by that one launch, the workspace not touched */
		BurstArgs rx = {};
		rx.seq = d_seq;
		rx.flags = d_flags;
		HIP_TRY(net2_launch_burst_wave_mc(tab->hash_alg, kt,
		    (const uint8_t *)d_base, d_offsets, d_lens, n, rx, d_result,
		    (uint8_t *)d_iv, ivlen, nullptr, NET2_HMAC_MODE_BURST_RX, s));
		return burst_launched(true);
	}
	BurstWs w;
	burst_layout(n, (uint8_t *)d_ws, &w);
	/* as decode_burst's keyed lane form: the HMAC kernel decodes the
	 * headers to where the caller wants them (else the workspace) ... */
	BurstArgs rx = {};
	rx.seq = d_seq != nullptr ? d_seq : w.seq;
	rx.flags = d_flags != nullptr ? d_flags : w.flags;
	rx.status = w.status;
	HIP_TRY(net2_launch_hmac_mc(tab->hash_alg, kt, (const uint8_t *)d_base,
	    d_offsets, d_lens, n, w.verdict, burst_bins(n, w.bin), s,
	    NET2_HMAC_MODE_BURST_RX, rx));
	if (int rc = burst_launched(false))
		return rc;
	/* ... and the final kernel folds the verdicts in and derives the IV
	 * of every OK PH_ENCRYPTED datagram whose connection has a cipher key
	 * (one cipher, so one ivlen) */
	HIP_TRY(net2_launch_burst_final_mc(n, w.status, w.verdict, rx.seq,
	    rx.flags, ivlen, (uint8_t *)d_iv, d_result, s));
	return 0;
}

NET2_EXPORT int net2_packet_decode_burst_mc(const struct net2_burst_keytab *tab,
    const uint32_t *d_conn, uint32_t ivlen, const void *d_base,
    const uint64_t *d_offsets, const uint32_t *d_lens, uint64_t n,
    uint8_t *d_result, void *d_iv, uint32_t *d_seq, uint32_t *d_flags,
    void *d_ws, size_t ws_bytes, void *stream)
{
	int rc = check_burst_mc_args(tab, d_conn, ivlen, d_base, d_offsets,
	    d_lens, n, d_result, d_ws, ws_bytes,
	    (d_seq == nullptr) == (d_flags == nullptr));
	if (rc != 0 || n == 0)
		return rc;
	return decode_burst_mc(tab, d_conn, ivlen, d_base, d_offsets, d_lens, n,
	    d_result, d_iv, d_seq, d_flags, d_ws, (hipStream_t)stream,
	    n <= net2_burst_wave_max());
}

/* net2_packet_encode_burst_mc's launches, the arguments checked.  seal_to:
 * as encode_burst's (null: the datagrams are sealed in d_base). */
int encode_burst_mc(const struct net2_burst_keytab *tab, const uint32_t *d_conn,
    const uint32_t *d_seq, const uint32_t *d_flags, void *d_base,
    const uint64_t *d_offsets, const uint32_t *d_lens, uint64_t n,
    uint8_t *d_result, void *d_ws, hipStream_t stream, bool wave,
    uint8_t *seal_to)
{
	uint8_t *const out = seal_to != nullptr ? seal_to : (uint8_t *)d_base;
	BurstArgs tx = {};
	tx.seq = const_cast<uint32_t *>(d_seq);
	tx.flags = const_cast<uint32_t *>(d_flags);
	tx.status = d_result;		/* the TX code is final in the kernel */
	const KeyTabArgs kt = { d_conn, tab->ents, tab->slots };
	if (wave) {
		/* a small burst: 1 to 16 datagrams per workgroup */
		HIP_TRY(net2_launch_burst_wave_mc(tab->hash_alg, kt,
		    (const uint8_t *)d_base, d_offsets, d_lens, n, tx, d_result,
		    nullptr, 0, out, NET2_HMAC_MODE_BURST_TX, stream));
		return burst_launched(true);
	}
	BurstWs w;
	burst_layout(n, (uint8_t *)d_ws, &w);
	HIP_TRY(net2_launch_hmac_mc(tab->hash_alg, kt, (const uint8_t *)d_base,
	    d_offsets, d_lens, n, out, burst_bins(n, w.bin), stream,
	    NET2_HMAC_MODE_BURST_TX, tx));
	return burst_launched(false);
}

NET2_EXPORT int net2_packet_encode_burst_mc(const struct net2_burst_keytab *tab,
    const uint32_t *d_conn, const uint32_t *d_seq, const uint32_t *d_flags,
    void *d_base, const uint64_t *d_offsets, const uint32_t *d_lens,
    uint64_t n, uint8_t *d_result, void *d_ws, size_t ws_bytes, void *stream)
{
	int rc = check_burst_mc_args(tab, d_conn, 0, d_base, d_offsets, d_lens, n,
	    d_result, d_ws, ws_bytes, d_seq != nullptr && d_flags != nullptr);
	if (rc != 0 || n == 0)
		return rc;
	return encode_burst_mc(tab, d_conn, d_seq, d_flags, d_base, d_offsets,
	    d_lens, n, d_result, d_ws, (hipStream_t)stream,
	    n <= net2_burst_wave_max(), nullptr);
}

/* ---- the cipher under per-connection keys: the device cipher-key table ---- */

/* (struct net2_burst_ciphertab: net2_host.h) */

NET2_EXPORT int net2_burst_ciphertab_create(int enc_alg, uint32_t slots,
    struct net2_burst_ciphertab **tab)
{
	if (tab == nullptr)
		return EINVAL;
	*tab = nullptr;
	if (enc_alg != NET2_ENC_AES256 || slots == 0)
		return EINVAL;
	if (int rc = check_current_device())
		return rc;
	std::unique_ptr<net2_burst_ciphertab> t(
	    new (std::nothrow) net2_burst_ciphertab());
	if (!t)
		return ENOMEM;
	if (hipGetDevice(&t->device) != hipSuccess)
		return ENODEV;
	t->slots = slots;
	const size_t bytes = (size_t)slots * NET2_AES_TAB_ENT_BYTES;
	HIP_TRY(hipMalloc((void **)&t->ents, bytes));
	/* every slot unset before the first call that could read it, whatever
	 * stream that call uses */
	hipError_t e = hipMemset(t->ents, 0, bytes);
	if (e == hipSuccess)
		e = hipDeviceSynchronize();
	if (e != hipSuccess) {
		(void)hipFree(t->ents);
		return hip_fail(e);
	}
	*tab = t.release();
	return 0;
}

NET2_EXPORT void net2_burst_ciphertab_destroy(struct net2_burst_ciphertab *tab)
{
	if (tab == nullptr)
		return;
	/* the entries are cipher keys: none stays in freed device memory.  On
	 * the table's device: wait for the work that may still read them, zero
	 * them, free (hipFree waits for the memset). */
	int prev = -1;
	(void)hipGetDevice(&prev);
	if (prev != tab->device)
		(void)hipSetDevice(tab->device);
	(void)hipDeviceSynchronize();
	tab_stage_destroy(tab->stage);
	(void)hipMemset(tab->ents, 0, (size_t)tab->slots * NET2_AES_TAB_ENT_BYTES);
	(void)hipFree(tab->ents);
	if (prev >= 0 && prev != tab->device)
		(void)hipSetDevice(prev);
	delete tab;
}

NET2_EXPORT int net2_burst_ciphertab_set_rx(struct net2_burst_ciphertab *tab,
    uint32_t slot, const struct net2_burst_rx_keys *keys,
    const struct net2_burst_cipher_keys *ck, void *stream)
{
	if (tab == nullptr || keys == nullptr || slot >= tab->slots ||
	    check_cipher_keys(ck) != 0)
		return EINVAL;
	if (keys->hash_alg != NET2_HASH_NIL && !hmac_row(keys->hash_alg))
		return EINVAL;
	/* as net2_packet_decrypt_burst: the alternate cipher key goes with
	 * the alternate hash key */
	const bool alt = keys->alt_hash_key != nullptr;
	if (alt && (keys->hash_alg == NET2_HASH_NIL || ck->alt_enc_key == nullptr))
		return EINVAL;
	if (int rc = check_table_device(tab->device))
		return rc;
	HIP_TRY(net2_launch_aes_tab_set(tab->ents, slot, NET2_AES_TAB_RX,
	    (const uint8_t *)ck->enc_key,
	    alt ? (const uint8_t *)ck->alt_enc_key : nullptr, keys->alt_no_cutoff,
	    keys->alt_cutoff, keys->rx_start, (hipStream_t)stream));
	tab_slot_launched();
	return 0;
}

NET2_EXPORT int net2_burst_ciphertab_set_tx(struct net2_burst_ciphertab *tab,
    uint32_t slot, const struct net2_burst_cipher_keys *ck, void *stream)
{
	if (tab == nullptr || slot >= tab->slots || check_cipher_keys(ck) != 0)
		return EINVAL;
	if (int rc = check_table_device(tab->device))
		return rc;
	HIP_TRY(net2_launch_aes_tab_set(tab->ents, slot, NET2_AES_TAB_TX,
	    (const uint8_t *)ck->enc_key, nullptr, 0, 0, 0, (hipStream_t)stream));
	tab_slot_launched();
	return 0;
}

NET2_EXPORT int net2_burst_ciphertab_clear(struct net2_burst_ciphertab *tab,
    uint32_t slot, void *stream)
{
	if (tab == nullptr || slot >= tab->slots)
		return EINVAL;
	if (int rc = check_table_device(tab->device))
		return rc;
	HIP_TRY(net2_launch_aes_tab_set(tab->ents, slot, 0, nullptr, nullptr, 0, 0,
	    0, (hipStream_t)stream));
	tab_slot_launched();
	return 0;
}

static bool digest_hashlen(uint32_t hashlen)
{
	return hashlen == 0 || hashlen == 32 || hashlen == 48 || hashlen == 64;
}

int ciphertab_device(const struct net2_burst_ciphertab *tab)
{
	return tab->device;
}

/* net2_packet_decrypt_burst_mc's launch, the arguments checked. */
int decrypt_burst_mc(const struct net2_burst_ciphertab *tab,
    const uint32_t *d_conn, uint32_t hashlen, const void *d_base,
    const uint64_t *d_offsets, const uint32_t *d_lens, uint64_t n,
    const uint32_t *d_seq, const uint32_t *d_flags, const void *d_iv,
    uint8_t *d_result, void *d_out, uint32_t *d_plen, hipStream_t s, bool wave)
{
	const AesTabArgs kt = { d_conn, tab->ents, tab->slots };
	HIP_TRY((wave ? net2_launch_aes_decrypt_mc_wave : net2_launch_aes_decrypt_mc)(
	    kt, hashlen, (const uint8_t *)d_base, d_offsets, d_lens, n, d_seq,
	    d_flags, (const uint8_t *)d_iv, d_result, (uint8_t *)d_out, d_plen, s));
	g_aes_launches.count(wave);
	return 0;
}

/* net2_packet_encrypt_burst_mc's launch, the arguments checked. */
int encrypt_burst_mc(const struct net2_burst_ciphertab *tab,
    const uint32_t *d_conn, uint32_t hashlen, const uint32_t *d_flags,
    const void *d_iv, void *d_base, const uint64_t *d_offsets,
    const uint32_t *d_lens, const uint32_t *d_plen, uint64_t n,
    uint8_t *d_result, uint32_t *d_wire_len, hipStream_t s, bool quad)
{
	const AesTabArgs kt = { d_conn, tab->ents, tab->slots };
	HIP_TRY((quad ? net2_launch_aes_encrypt_mc_quad : net2_launch_aes_encrypt_mc)(
	    kt, hashlen, d_flags, (const uint8_t *)d_iv, (uint8_t *)d_base, d_offsets,
	    d_lens, d_plen, n, d_result, d_wire_len, s));
	g_aes_tx_launches.count(quad);
	return 0;
}

NET2_EXPORT int net2_packet_decrypt_burst_mc(
    const struct net2_burst_ciphertab *tab, const uint32_t *d_conn,
    uint32_t hashlen, const void *d_base, const uint64_t *d_offsets,
    const uint32_t *d_lens, uint64_t n, const uint32_t *d_seq,
    const uint32_t *d_flags, const void *d_iv, uint8_t *d_result, void *d_out,
    uint32_t *d_plen, void *stream)
{
	if (tab == nullptr || !digest_hashlen(hashlen))
		return EINVAL;
	if (n == 0)
		return 0;
	/* any slot may have an alternate key, so d_seq is always needed */
	if (!dgrams_ok(d_base, d_offsets, d_lens, n) || d_conn == nullptr ||
	    d_seq == nullptr || d_flags == nullptr || d_iv == nullptr ||
	    d_result == nullptr || d_out == nullptr || d_plen == nullptr)
		return EINVAL;
	if (int rc = check_table_device(tab->device))
		return rc;
	return decrypt_burst_mc(tab, d_conn, hashlen, d_base, d_offsets, d_lens, n,
	    d_seq, d_flags, d_iv, d_result, d_out, d_plen, (hipStream_t)stream,
	    aes_wave_form(n));
}

NET2_EXPORT int net2_packet_encrypt_burst_mc(
    const struct net2_burst_ciphertab *tab, const uint32_t *d_conn,
    uint32_t hashlen, const uint32_t *d_flags, const void *d_iv, void *d_base,
    const uint64_t *d_offsets, const uint32_t *d_lens, const uint32_t *d_plen,
    uint64_t n, uint8_t *d_result, uint32_t *d_wire_len, void *stream)
{
	if (tab == nullptr || !digest_hashlen(hashlen))
		return EINVAL;
	if (n == 0)
		return 0;
	if (!dgrams_ok(d_base, d_offsets, d_lens, n) || d_conn == nullptr ||
	    d_flags == nullptr || d_iv == nullptr || d_plen == nullptr ||
	    d_result == nullptr || d_wire_len == nullptr)
		return EINVAL;
	if (int rc = check_table_device(tab->device))
		return rc;
	return encrypt_burst_mc(tab, d_conn, hashlen, d_flags, d_iv, d_base,
	    d_offsets, d_lens, d_plen, n, d_result, d_wire_len,
	    (hipStream_t)stream, aes_quad_form(n));
}
