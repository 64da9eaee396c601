/*
 * net2_single.cpp -- the single-message calls of include/net2/hash.h and
 * include/net2/packet.h: net2_hashctx_hashiov (one coalesced request, or the
 * streaming context for a long message) and net2_ph_to_iv_buf over it.
 */
#include "net2_host.h"
#include "sha2_coalesce.h"

#include <sys/uio.h>

int net2_co_run(const net2co::Request &r)
{
	const std::vector<int> dv = batch_devices();
	if (dv.empty())
		return ENODEV;
	const size_t d = small_device(dv);
	int herr = 0;
	const int rc = net2co::submit(d, dv[d], r, &herr);
	if (rc == EIO)
		tl_last_hip_error = herr;
	return rc;
}

/*
 * A message longer than this (NET2_SHA2_STREAM_CHUNK, default 64 MiB) is
 * hashed through the streaming context, whose Update sends it in requests
 * of at most that size: one request would stage the whole message in
 * page-locked memory.
 */
static size_t long_message_bytes()
{
	const char *e = getenv("NET2_SHA2_STREAM_CHUNK");
	return e != nullptr && *e != '\0' ? strtoull(e, nullptr, 10) :
	    (size_t)64 << 20;
}

/* net2_hashctx_hashiov of a long message: SHA*Init / Update per segment /
 * Final, and for HMAC the same over K' ^ ipad || m, then K' ^ opad || inner
 * (RFC 2104, as hash-openssl.cc's HMAC_* calls). */
static int hashiov_streamed(int alg, const void *key, size_t keylen,
    const struct iovec *iov, size_t iovcnt, uint8_t *out)
{
	const bool keyed = !unkeyed_sha2(alg);
	const int halg = keyed ? alg - 3 : alg;
	const size_t B = halg == NET2_HASH_SHA256 ? 64 : 128;
	uint8_t kp[128] = { 0 }, blk[128], inner[64];
	SHA2_CTX c;
	int rc;
	if (keyed) {
		if (keylen > B)
			return EINVAL;
		memcpy(kp, key, keylen);
	}
	if ((rc = net2_sha2_ctx_init(halg, &c)) != 0)
		return rc;
	if (keyed) {
		for (size_t i = 0; i < B; i++)
			blk[i] = kp[i] ^ 0x36;
		if ((rc = net2_sha2_ctx_update(halg, &c, blk, B)) != 0)
			return rc;
	}
	{
		/* many small segments are gathered into requests of up to one
		 * stream chunk (one GPU round trip each, not one per segment);
		 * a segment of a chunk or more with nothing gathered goes as is */
		const size_t chunk = std::max(long_message_bytes(), B);
		std::vector<uint8_t> gbuf;
		size_t have = 0;
		for (size_t i = 0; i < iovcnt; i++) {
			const uint8_t *q = (const uint8_t *)iov[i].iov_base;
			size_t left = iov[i].iov_len;
			if (have == 0 && left >= chunk) {
				if ((rc = net2_sha2_ctx_update(halg, &c, q, left)) != 0)
					return rc;
				continue;
			}
			while (left > 0) {
				if (gbuf.empty())
					gbuf.resize(chunk);
				const size_t take = std::min(left, chunk - have);
				memcpy(gbuf.data() + have, q, take);
				have += take;
				q += take;
				left -= take;
				if (have == chunk) {
					if ((rc = net2_sha2_ctx_update(halg, &c,
					    gbuf.data(), have)) != 0)
						return rc;
					have = 0;
				}
			}
		}
		if (have > 0 && (rc = net2_sha2_ctx_update(halg, &c, gbuf.data(),
		    have)) != 0)
			return rc;
	}
	if ((rc = net2_sha2_ctx_final(halg, keyed ? inner : out, &c)) != 0 ||
	    !keyed)
		return rc;
	for (size_t i = 0; i < B; i++)
		blk[i] = kp[i] ^ 0x5c;
	if ((rc = net2_sha2_ctx_init(halg, &c)) != 0 ||
	    (rc = net2_sha2_ctx_update(halg, &c, blk, B)) != 0 ||
	    (rc = net2_sha2_ctx_update(halg, &c, inner,
	    (size_t)kRows[alg].hashlen)) != 0)
		return rc;
	return net2_sha2_ctx_final(halg, out, &c);
}

NET2_EXPORT int net2_hashctx_hashiov(int alg, const void *key, size_t keylen,
    const struct iovec *iov, size_t iovcnt, void *out, size_t outlen)
{
	if (alg < 0 || alg >= kNumRows)
		return EINVAL;
	if ((size_t)kRows[alg].keylen != keylen ||
	    (keylen > 0 && key == nullptr))
		return EINVAL;
	if (iovcnt > 0 && iov == nullptr)
		return EINVAL;
	if (alg == NET2_HASH_NIL)
		return 0;
	if (out == nullptr || outlen < (size_t)kRows[alg].hashlen)
		return EINVAL;
	size_t total = 0;
	for (size_t i = 0; i < iovcnt; i++)
		total += iov[i].iov_len;
	if (total > long_message_bytes())
		return hashiov_streamed(alg, key, keylen, iov, iovcnt,
		    (uint8_t *)out);
	/* one coalesced request: concurrent callers share a launch */
	net2co::Request r = {};
	r.kind = unkeyed_sha2(alg) ? net2co::DIGEST : net2co::HMAC;
	r.alg = unkeyed_sha2(alg) ? alg : alg - 3;
	r.iov = iov;
	r.iovcnt = iovcnt;
	r.key = (const uint8_t *)key;
	r.keylen = keylen;
	r.out = (uint8_t *)out;
	return net2_co_run(r);
}

NET2_EXPORT int net2_ph_to_iv_buf(const struct net2_packet_header *ph,
    size_t ivlen, void *iv)
{
	uint8_t hdr[8];
	uint8_t *out = (uint8_t *)iv;
	uint8_t d[32];
	size_t have = 0;

	if (ph == nullptr || (iv == nullptr && ivlen > 0))
		return EINVAL;
	for (int i = 0; i < 4; i++) {
		hdr[i] = (uint8_t)(ph->seq >> (24 - 8 * i));
		hdr[4 + i] = (uint8_t)(ph->flags >> (24 - 8 * i));
	}
	while (have < ivlen) {		/* packet.n2t:127-144 */
		struct iovec v[2] = { { hdr, sizeof(hdr) }, { out, have } };
		int rc = net2_hashctx_hashiov(NET2_HASH_SHA256, nullptr, 0, v, 2,
		    d, sizeof(d));
		if (rc != 0)
			return rc;
		size_t take = std::min<size_t>(32, ivlen - have);
		memcpy(out + have, d, take);
		have += take;
	}
	return 0;
}
