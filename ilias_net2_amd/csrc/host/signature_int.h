/*
 * signature_int.h -- internal to libnet2_sign.so (hidden symbols).
 */
#ifndef NET2_SIGNATURE_INT_H
#define NET2_SIGNATURE_INT_H

#include "../../../include/net2/signature.h"

/* Fill s with the signature of an already computed digest
 * (types/signature.n2t:74-100); 0 or an errno, s left empty on failure. */
int sign_digest(struct net2x_signature *s, const uint8_t *digest, size_t dlen,
    const char *hash_name, struct net2x_sign_ctx *sign);

/* The device-backed validation (sign.c).  signctx_is_p521: is the key on
 * secp521r1?  signctx_validate_batch_dev: n DER signatures, item i under
 * ctxs[i * ctx_step] (every one on P-521; step 0: one context), digest i
 * at digests + i * dig_stride with dlens[i] bytes (dlens NULL: dlen);
 * valid[i] = 1 / 0; returns 0 or the device call's errno. */
int signctx_is_p521(struct net2x_sign_ctx *s);
int signctx_validate_batch_dev(struct net2x_sign_ctx *const *ctxs,
    size_t ctx_step, const uint8_t *const *sigs, const size_t *siglens,
    const uint8_t *digests, size_t dig_stride, const uint32_t *dlens,
    uint32_t dlen, size_t n, int *valid);

#endif /* NET2_SIGNATURE_INT_H */
