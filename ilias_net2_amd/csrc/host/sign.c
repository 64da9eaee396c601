/*
 * sign.c -- ECDSA signature contexts over OpenSSL (host side of the signed
 * payload path).  Behaviour follows the reference's src/sign.c: algorithm
 * table with one "ecdsa" row (:164-169), PEM key loading (:324-420), the
 * digest signed as is with a DER ECDSA-Sig out (:478-516), validation
 * returning 1/0 (:518-563), the public key as an uncompressed point
 * (:580-639) and its SHA-256 fingerprint, cached (:258-320).  The
 * fingerprint's SHA-256 runs on the MI355X (net2_hashctx_hashiov).
 */
#define OPENSSL_SUPPRESS_DEPRECATED	/* EC_KEY point export, as sign.c */
#include "../../../include/net2/sign.h"
#include "../../../include/net2/hash.h"
#include "../../../include/net2/ecdsa_key.h"

#include <errno.h>
#include <pthread.h>
#include <stdlib.h>
#include <string.h>

#include <openssl/bio.h>
#include <openssl/bn.h>
#include <openssl/ec.h>
#include <openssl/evp.h>
#include <openssl/pem.h>

#define NET2_EXPORT __attribute__((visibility("default")))

struct net2x_sign_ctx {
	int		 alg;
	EVP_PKEY	*pkey;
	int		 is_private;
	pthread_mutex_t	 mu;		/* guards the two caches */
	uint8_t		*pub;		/* cached uncompressed point */
	size_t		 publen;
	int		 have_fp;
	uint8_t		 fp[32];	/* cached fingerprint */
	/* the key prepared for the device (net2x_signctx_prepare_dev), or NULL;
	 * set once under mu, freed with the context */
	struct net2_ecdsa_p521_keys *keys;
};

static const char *const sign_names[] = { "ecdsa" };

NET2_EXPORT const int net2x_signmax =
    (int)(sizeof(sign_names) / sizeof(sign_names[0]));

/* The ECDSA row of the registry, by name (src/sign.c:653; test/sign.c:66,69
 * pass it to net2x_signctx_{priv,pub}new). */
NET2_EXPORT const int net2x_sign_ecdsa = 0;

NET2_EXPORT const char *
net2x_sign_getname(int alg)
{
	return alg >= 0 && alg < net2x_signmax ? sign_names[alg] : NULL;
}

NET2_EXPORT int
net2x_sign_findname(const char *name)
{
	if (name == NULL)
		return -1;
	for (int i = 0; i < net2x_signmax; i++)
		if (strcmp(sign_names[i], name) == 0)
			return i;
	return -1;
}

static struct net2x_sign_ctx *
ctx_from_pem(int alg, const void *key, size_t keylen, int priv)
{
	struct net2x_sign_ctx *s;
	EVP_PKEY *pk;
	BIO *bio;

	if (alg < 0 || alg >= net2x_signmax || key == NULL || keylen == 0 ||
	    keylen > INT32_MAX)
		return NULL;
	if ((bio = BIO_new_mem_buf(key, (int)keylen)) == NULL)
		return NULL;
	pk = priv ? PEM_read_bio_PrivateKey(bio, NULL, NULL, NULL)
	    : PEM_read_bio_PUBKEY(bio, NULL, NULL, NULL);
	BIO_free(bio);
	if (pk == NULL)
		return NULL;
	if (EVP_PKEY_get_base_id(pk) != EVP_PKEY_EC) {	/* ECDSA only */
		EVP_PKEY_free(pk);
		return NULL;
	}
	if ((s = calloc(1, sizeof(*s))) == NULL) {
		EVP_PKEY_free(pk);
		return NULL;
	}
	s->alg = alg;
	s->pkey = pk;
	s->is_private = priv;
	pthread_mutex_init(&s->mu, NULL);
	return s;
}

NET2_EXPORT struct net2x_sign_ctx *
net2x_signctx_pubnew(int alg, const void *key, size_t keylen)
{
	return ctx_from_pem(alg, key, keylen, 0);
}

NET2_EXPORT struct net2x_sign_ctx *
net2x_signctx_privnew(int alg, const void *key, size_t keylen)
{
	return ctx_from_pem(alg, key, keylen, 1);
}

NET2_EXPORT void
net2x_signctx_free(struct net2x_sign_ctx *s)
{
	if (s == NULL)
		return;
	EVP_PKEY_free(s->pkey);
	free(s->pub);
	net2_ecdsa_p521_keys_free(s->keys);
	pthread_mutex_destroy(&s->mu);
	free(s);
}

NET2_EXPORT struct net2x_sign_ctx *
net2x_signctx_clone(struct net2x_sign_ctx *o)
{
	struct net2x_sign_ctx *s;

	if (o == NULL || (s = calloc(1, sizeof(*s))) == NULL)
		return NULL;
	if (!EVP_PKEY_up_ref(o->pkey)) {
		free(s);
		return NULL;
	}
	s->alg = o->alg;
	s->pkey = o->pkey;
	s->is_private = o->is_private;
	pthread_mutex_init(&s->mu, NULL);
	pthread_mutex_lock(&o->mu);
	if (o->have_fp) {			/* the fingerprint cache travels */
		memcpy(s->fp, o->fp, sizeof(s->fp));
		s->have_fp = 1;
	}
	pthread_mutex_unlock(&o->mu);
	return s;
}

NET2_EXPORT size_t
net2x_signctx_maxmsglen(struct net2x_sign_ctx *s)
{
	return s == NULL ? 0 : (size_t)EVP_PKEY_get_size(s->pkey);
}

NET2_EXPORT const char *
net2x_signctx_name(struct net2x_sign_ctx *s)
{
	return s == NULL ? NULL : sign_names[s->alg];
}

NET2_EXPORT int
net2x_signctx_sign(struct net2x_sign_ctx *s, const void *in, size_t inlen,
    void *sig, size_t *siglen)
{
	EVP_PKEY_CTX *pc;
	int rc = -1;

	if (s == NULL || in == NULL || sig == NULL || siglen == NULL)
		return EINVAL;
	if (!s->is_private)
		return EINVAL;
	if (*siglen < net2x_signctx_maxmsglen(s))
		return EINVAL;
	if ((pc = EVP_PKEY_CTX_new(s->pkey, NULL)) == NULL)
		return ENOMEM;
	if (EVP_PKEY_sign_init(pc) == 1 &&
	    EVP_PKEY_sign(pc, sig, siglen, in, inlen) == 1)
		rc = 0;
	EVP_PKEY_CTX_free(pc);
	return rc;
}

NET2_EXPORT int
net2x_signctx_validate(struct net2x_sign_ctx *s, const void *sig,
    size_t siglen, const void *in, size_t inlen)
{
	EVP_PKEY_CTX *pc;
	int ok;

	if (s == NULL || in == NULL || sig == NULL)
		return 0;
	if (siglen > net2x_signctx_maxmsglen(s))	/* src/sign.c:527-529 */
		return 0;
	if ((pc = EVP_PKEY_CTX_new(s->pkey, NULL)) == NULL)
		return 0;
	ok = EVP_PKEY_verify_init(pc) == 1 &&
	    EVP_PKEY_verify(pc, sig, siglen, in, inlen) == 1;
	EVP_PKEY_CTX_free(pc);
	return ok;
}

/* Uncompressed EC point of the key, computed once. */
static int
pubkey_cached(struct net2x_sign_ctx *s)
{
	const EC_KEY *ek;
	const EC_GROUP *g;
	const EC_POINT *pt;
	size_t len;

	if (s->pub != NULL)
		return 0;
	if ((ek = EVP_PKEY_get0_EC_KEY(s->pkey)) == NULL ||
	    (g = EC_KEY_get0_group(ek)) == NULL ||
	    (pt = EC_KEY_get0_public_key(ek)) == NULL)
		return EINVAL;
	len = EC_POINT_point2oct(g, pt, POINT_CONVERSION_UNCOMPRESSED, NULL, 0,
	    NULL);
	if (len == 0)
		return EINVAL;
	if ((s->pub = malloc(len)) == NULL)
		return ENOMEM;
	if (EC_POINT_point2oct(g, pt, POINT_CONVERSION_UNCOMPRESSED, s->pub,
	    len, NULL) != len) {
		free(s->pub);
		s->pub = NULL;
		return EINVAL;
	}
	s->publen = len;
	return 0;
}

NET2_EXPORT int
net2x_signctx_pubkey(struct net2x_sign_ctx *s, void *out, size_t *outlen)
{
	int rc;

	if (s == NULL || outlen == NULL)
		return EINVAL;
	pthread_mutex_lock(&s->mu);
	rc = pubkey_cached(s);
	if (rc == 0) {
		if (out == NULL || *outlen < s->publen)
			rc = out == NULL ? 0 : EINVAL;
		else
			memcpy(out, s->pub, s->publen);
		*outlen = s->publen;
	}
	pthread_mutex_unlock(&s->mu);
	return rc;
}

NET2_EXPORT int
net2x_signctx_fingerprint(struct net2x_sign_ctx *s, uint8_t out[32])
{
	struct iovec iov;
	int rc;

	if (s == NULL || out == NULL)
		return EINVAL;
	pthread_mutex_lock(&s->mu);
	rc = 0;
	if (!s->have_fp) {
		rc = pubkey_cached(s);
		if (rc == 0) {
			iov.iov_base = s->pub;
			iov.iov_len = s->publen;
			rc = net2_hashctx_hashiov(NET2_HASH_SHA256, NULL, 0,
			    &iov, 1, s->fp, sizeof(s->fp));
		}
		if (rc == 0)
			s->have_fp = 1;
	}
	if (rc == 0)
		memcpy(out, s->fp, 32);
	pthread_mutex_unlock(&s->mu);
	return rc;
}

/* ---- batched validation on the device (net2/ecdsa.h) ----------------------- */

#include "../../../include/net2/ecdsa.h"
#include "signature_int.h"

#include <openssl/ecdsa.h>
#include <openssl/obj_mac.h>

#define P521_BYTES 66

/* Is the context's key on secp521r1, the curve the device verifies? */
int
signctx_is_p521(struct net2x_sign_ctx *s)
{
	const EC_KEY *ek;
	const EC_GROUP *g;

	return s != NULL && (ek = EVP_PKEY_get0_EC_KEY(s->pkey)) != NULL &&
	    (g = EC_KEY_get0_group(ek)) != NULL &&
	    EC_GROUP_get_curve_name(g) == NID_secp521r1;
}

/*
 * What ECDSA_verify does with a signature before the mathematics
 * (crypto/ec/ecdsa_vrf.c): parse the DER, re-encode it, and refuse anything
 * that is not byte for byte its own canonical encoding -- trailing bytes,
 * non-minimal lengths.  d2i accepts a negative INTEGER, which the
 * verification then refuses; so is it here, as is a value too long for the
 * 66-byte form (both are outside [1, n - 1]).  1 with r || s in rs, else 0.
 */
static int
der_to_rs(const uint8_t *sig, size_t siglen, uint8_t rs[2 * P521_BYTES])
{
	const unsigned char *p = sig;
	unsigned char *der = NULL;
	const BIGNUM *r, *s;
	ECDSA_SIG *es;
	int derlen, ok = 0;

	if (sig == NULL || siglen == 0 || siglen > INT32_MAX ||
	    (es = d2i_ECDSA_SIG(NULL, &p, (long)siglen)) == NULL)
		return 0;
	derlen = i2d_ECDSA_SIG(es, &der);
	if (derlen > 0 && (size_t)derlen == siglen &&
	    memcmp(sig, der, siglen) == 0) {
		ECDSA_SIG_get0(es, &r, &s);
		ok = !BN_is_negative(r) && !BN_is_negative(s) &&
		    BN_num_bytes(r) <= P521_BYTES && BN_num_bytes(s) <= P521_BYTES &&
		    BN_bn2binpad(r, rs, P521_BYTES) == P521_BYTES &&
		    BN_bn2binpad(s, rs + P521_BYTES, P521_BYTES) == P521_BYTES;
	}
	OPENSSL_free(der);
	ECDSA_SIG_free(es);
	return ok;
}

/* x || y of the context's key, from its cached uncompressed point */
static int
signctx_xy(struct net2x_sign_ctx *s, uint8_t xy[2 * P521_BYTES])
{
	int rc;

	pthread_mutex_lock(&s->mu);
	rc = pubkey_cached(s);
	if (rc == 0 && (s->publen != 1 + 2 * P521_BYTES || s->pub[0] != 0x04))
		rc = EINVAL;
	if (rc == 0)
		memcpy(xy, s->pub + 1, 2 * P521_BYTES);
	pthread_mutex_unlock(&s->mu);
	return rc;
}

/*
 * n DER signatures on the device: item i under ctxs[i * ctx_step] (step 0:
 * one context for all), its digest at digests + i * dig_stride, dlens[i]
 * bytes (or dlen where dlens is NULL).  Every context is on P-521 (the
 * callers looked).  The signatures the host part settles never reach the
 * device; the rest go in one net2_ecdsa_p521_verify batch -- or, for one
 * context that was prepared (net2x_signctx_prepare_dev), in one
 * net2_ecdsa_p521_verify_keys batch from its key's table.
 */
int
signctx_validate_batch_dev(struct net2x_sign_ctx *const *ctxs, size_t ctx_step,
    const uint8_t *const *sigs, const size_t *siglens, const uint8_t *digests,
    size_t dig_stride, const uint32_t *dlens, uint32_t dlen, size_t n,
    int *valid)
{
	uint8_t *pub = NULL, *rs = NULL, *dig = NULL, *verdict = NULL;
	uint32_t *lens = NULL;
	size_t *at = NULL, m = 0, width = dlen;
	int rc = 0;

	for (size_t i = 0; i < n; i++) {
		valid[i] = 0;
		if (dlens != NULL && dlens[i] > width)
			width = dlens[i];
	}
	if (width == 0)
		width = 1;
	pub = malloc((ctx_step ? n : 1) * 2 * P521_BYTES);
	rs = malloc(n * 2 * P521_BYTES);
	dig = malloc(n * width);
	lens = malloc(n * sizeof(*lens));
	at = malloc(n * sizeof(*at));
	verdict = calloc(n, 1);
	if (!pub || !rs || !dig || !lens || !at || !verdict) {
		rc = ENOMEM;
		goto out;
	}
	if (ctx_step == 0 && (rc = signctx_xy(ctxs[0], pub)) != 0)
		goto out;
	for (size_t i = 0; i < n; i++) {
		struct net2x_sign_ctx *s = ctxs[i * ctx_step];
		const uint32_t dl = dlens != NULL ? dlens[i] : dlen;

		if (sigs[i] == NULL || siglens[i] > net2x_signctx_maxmsglen(s) ||
		    dl > dig_stride || !der_to_rs(sigs[i], siglens[i],
		    rs + m * 2 * P521_BYTES))
			continue;		/* valid[i] stays 0 */
		if (ctx_step != 0 &&
		    (rc = signctx_xy(s, pub + m * 2 * P521_BYTES)) != 0)
			goto out;
		if (dl > 0)
			memcpy(dig + m * width, digests + i * dig_stride, dl);
		lens[m] = dl;
		at[m++] = i;
	}
	if (m > 0) {
		const struct net2_ecdsa_p521_keys *keys = NULL;

		if (ctx_step == 0) {
			pthread_mutex_lock(&ctxs[0]->mu);
			keys = ctxs[0]->keys;
			pthread_mutex_unlock(&ctxs[0]->mu);
		}
		if (keys != NULL)	/* prepared: through the key's table */
			rc = net2_ecdsa_p521_verify_keys(keys, NULL, rs, dig, width,
			    lens, 0, m, verdict);
		else
			rc = net2_ecdsa_p521_verify(pub, ctx_step ? 2 * P521_BYTES : 0,
			    rs, dig, width, lens, 0, m, verdict);
		for (size_t k = 0; rc == 0 && k < m; k++)
			valid[at[k]] = verdict[k] == 1;
	}
out:
	free(pub);
	free(rs);
	free(dig);
	free(lens);
	free(at);
	free(verdict);
	return rc;
}

NET2_EXPORT int
net2x_signctx_prepare_dev(struct net2x_sign_ctx *s)
{
	uint8_t xy[2 * P521_BYTES], ok = 0;
	struct net2_ecdsa_p521_keys *keys = NULL;
	int rc;

	if (s == NULL)
		return EINVAL;
	if (!signctx_is_p521(s))
		return EOPNOTSUPP;
	if ((rc = signctx_xy(s, xy)) != 0)
		return rc;
	pthread_mutex_lock(&s->mu);
	if (s->keys == NULL) {
		rc = net2_ecdsa_p521_keys_new(xy, sizeof(xy), 1, &keys, &ok);
		if (rc == 0 && ok != 1) {	/* OpenSSL loaded it: cannot be */
			net2_ecdsa_p521_keys_free(keys);
			rc = EINVAL;
		} else if (rc == 0) {
			s->keys = keys;
		}
	}
	pthread_mutex_unlock(&s->mu);
	return rc;
}

NET2_EXPORT int
net2x_signctx_validate_batch(struct net2x_sign_ctx *s,
    const uint8_t *const *sigs, const size_t *siglens, const uint8_t *digests,
    size_t dig_stride, size_t dlen, size_t n, int *valid)
{
	if (n == 0)
		return 0;
	if (s == NULL || sigs == NULL || siglens == NULL || valid == NULL ||
	    (digests == NULL && dlen > 0) || dlen > UINT32_MAX ||
	    (n > 1 && dig_stride < dlen))
		return EINVAL;
	if (!signctx_is_p521(s))
		return EOPNOTSUPP;
	return signctx_validate_batch_dev(&s, 0, sigs, siglens, digests,
	    n > 1 ? dig_stride : dlen, NULL, (uint32_t)dlen, n, valid);
}
