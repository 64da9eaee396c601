/*
 * p521_field.h -- arithmetic modulo p = 2^521 - 1, the field of secp521r1,
 * for the batched ECDSA verification (ecdsa_kernels.hip, ecdsa_p521.h).
 *
 * An element is 17 little-endian 32-bit limbs holding a value in
 * [0, 2^521): limb 16 has 9 bits.  That range holds one value twice, p itself
 * being 0, so results are only "weakly" reduced; fe_canon / fe_is_zero /
 * fe_eq settle the difference where a comparison needs it.  Reduction is the
 * Mersenne fold: 2^521 = 1 (mod p), so the bits above 521 are added back in
 * at the bottom.
 *
 * Every limb index is a compile-time constant once the loops are unrolled, so
 * on the device an element lives in 17 VGPRs and a product in 34; the
 * multiply is 289 32x32+64 multiply-adds (v_mad_u64_u32).  Nothing here is
 * constant-time and nothing needs to be: verification sees public data only.
 *
 * Host + device code, as aes_device.h: plain C++17, no HIP header needed on
 * the host (tests/cxx/test_ecdsa_host.cc compiles it there).
 */
#ifndef NET2_P521_FIELD_H
#define NET2_P521_FIELD_H

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define P521_HD __host__ __device__ __forceinline__
#define P521_UNROLL _Pragma("unroll")
#else
#define P521_HD static inline
#define P521_UNROLL
#endif

#define P521_LIMBS 17
#define P521_BYTES 66			/* a big-endian coordinate or scalar */
#define P521_TOP_MASK 0x1ffu		/* limb 16 of p */

struct p521_fe {
	uint32_t l[P521_LIMBS];
};

/* The curve's b and its base point G (SEC 2, secp521r1), as limbs. */
#define P521_B_INIT { \
	0x6b503f00u, 0xef451fd4u, 0x3d2c34f1u, 0x3573df88u, 0x3bb1bf07u, 0x1652c0bdu, \
	0xec7e937bu, 0x56193951u, 0x8ef109e1u, 0xb8b48991u, 0x99b315f3u, 0xa2da725bu, \
	0xb68540eeu, 0x929a21a0u, 0x8e1c9a1fu, 0x953eb961u, 0x00000051u }
#define P521_GX_INIT { \
	0xc2e5bd66u, 0xf97e7e31u, 0x856a429bu, 0x3348b3c1u, 0xa2ffa8deu, 0xfe1dc127u, \
	0xefe75928u, 0xa14b5e77u, 0x6b4d3dbau, 0xf828af60u, 0x053fb521u, 0x9c648139u, \
	0x2395b442u, 0x9e3ecb66u, 0x0404e9cdu, 0x858e06b7u, 0x000000c6u }
#define P521_GY_INIT { \
	0x9fd16650u, 0x88be9476u, 0xa272c240u, 0x353c7086u, 0x3fad0761u, 0xc550b901u, \
	0x5ef42640u, 0x97ee7299u, 0x273e662cu, 0x17afbd17u, 0x579b4468u, 0x98f54449u, \
	0x2c7d1bd9u, 0x5c8a5fb4u, 0x9a3bc004u, 0x39296a78u, 0x00000118u }

P521_HD p521_fe fe_zero()
{
	p521_fe r;
	P521_UNROLL
	for (int i = 0; i < P521_LIMBS; i++)
		r.l[i] = 0;
	return r;
}

P521_HD p521_fe fe_one()
{
	p521_fe r = fe_zero();
	r.l[0] = 1;
	return r;
}

/*
 * 66 big-endian bytes at any alignment (byte loads).  The 528 bits all land
 * in the limbs; *in_field says whether the value is below p, and a value that
 * is not must not be computed with.
 */
P521_HD p521_fe fe_load_be66(const uint8_t *b, bool *in_field)
{
	p521_fe r;
	uint32_t all = 0xffffffffu;
	P521_UNROLL
	for (int i = 0; i < 16; i++) {
		const uint8_t *q = b + P521_BYTES - 4 - 4 * i;
		r.l[i] = (uint32_t)q[0] << 24 | (uint32_t)q[1] << 16 |
		    (uint32_t)q[2] << 8 | q[3];
		all &= r.l[i];
	}
	r.l[16] = (uint32_t)b[0] << 8 | b[1];
	*in_field = r.l[16] < P521_TOP_MASK ||
	    (r.l[16] == P521_TOP_MASK && all != 0xffffffffu);
	return r;
}

/* a value below 2^522 with its bit 521 folded in: below 2^521 again whenever
 * the value was at most 2^522 - 2 (a sum of two elements is) */
P521_HD void fe_fold_top(p521_fe &r)
{
	uint64_t c = r.l[16] >> 9;
	r.l[16] &= P521_TOP_MASK;
	P521_UNROLL
	for (int i = 0; i < P521_LIMBS; i++) {
		c += r.l[i];
		r.l[i] = (uint32_t)c;
		c >>= 32;
	}
}

P521_HD p521_fe fe_add(const p521_fe &a, const p521_fe &b)
{
	p521_fe r;
	uint64_t c = 0;
	P521_UNROLL
	for (int i = 0; i < P521_LIMBS; i++) {
		c += (uint64_t)a.l[i] + b.l[i];
		r.l[i] = (uint32_t)c;
		c >>= 32;
	}
	fe_fold_top(r);
	return r;
}

/* a - b = a + (p - b), and p - b is b with its 521 bits inverted */
P521_HD p521_fe fe_sub(const p521_fe &a, const p521_fe &b)
{
	p521_fe nb;
	P521_UNROLL
	for (int i = 0; i < 16; i++)
		nb.l[i] = ~b.l[i];
	nb.l[16] = b.l[16] ^ P521_TOP_MASK;
	return fe_add(a, nb);
}

/*
 * The 1042-bit product by rows (each step a 32x32 multiply plus two 32-bit
 * addends, which cannot overflow 64 bits), then the fold: low 521 bits plus
 * the bits above them, a sum below 2^522 - 1, and its bit 521 once more.
 */
P521_HD p521_fe fe_mul(const p521_fe &a, const p521_fe &b)
{
	uint32_t t[2 * P521_LIMBS];
	P521_UNROLL
	for (int i = 0; i < 2 * P521_LIMBS; i++)
		t[i] = 0;
	P521_UNROLL
	for (int i = 0; i < P521_LIMBS; i++) {
		uint64_t c = 0;
		P521_UNROLL
		for (int j = 0; j < P521_LIMBS; j++) {
			c += (uint64_t)a.l[i] * b.l[j] + t[i + j];
			t[i + j] = (uint32_t)c;
			c >>= 32;
		}
		t[i + P521_LIMBS] = (uint32_t)c;
	}
	p521_fe r;
	uint64_t c = 0;
	P521_UNROLL
	for (int i = 0; i < P521_LIMBS; i++) {
		const uint32_t lo = i == 16 ? t[16] & P521_TOP_MASK : t[i];
		const uint32_t hi = t[16 + i] >> 9 |
		    (i == 16 ? 0u : t[17 + i] << 23);
		c += (uint64_t)lo + hi;
		r.l[i] = (uint32_t)c;
		c >>= 32;
	}
	fe_fold_top(r);
	return r;
}

P521_HD p521_fe fe_sqr(const p521_fe &a)
{
	return fe_mul(a, a);
}

/* zero, in either of its two forms */
P521_HD bool fe_is_zero(const p521_fe &a)
{
	uint32_t any = 0, all = 0xffffffffu;
	P521_UNROLL
	for (int i = 0; i < 16; i++) {
		any |= a.l[i];
		all &= a.l[i];
	}
	return (any | a.l[16]) == 0 ||
	    (all == 0xffffffffu && a.l[16] == P521_TOP_MASK);
}

/* the representative in [0, p) */
P521_HD p521_fe fe_canon(const p521_fe &a)
{
	return fe_is_zero(a) ? fe_zero() : a;
}

P521_HD bool fe_eq(const p521_fe &a, const p521_fe &b)
{
	return fe_is_zero(fe_sub(a, b));
}

/*
 * 1 / a = a^(p - 2) = a^(2^521 - 3): 519 ones above a low "01".  518 squarings
 * with a multiplication each run the exponent from 1 up to 2^519 - 1, two more
 * squarings and the last multiplication append the "01".  The inverse of zero
 * comes out as zero.  The verification itself never inverts in the field (its
 * last comparison is made projectively); converting a result to affine
 * coordinates does.
 */
P521_HD p521_fe fe_inv(const p521_fe &a)
{
	p521_fe r = a;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
	for (int i = 0; i < 518; i++)
		r = fe_mul(fe_mul(r, r), a);
	r = fe_mul(r, r);
	r = fe_mul(r, r);
	return fe_mul(r, a);
}

#endif /* NET2_P521_FIELD_H */
