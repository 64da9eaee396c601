/*
 * p521_scalar.h -- arithmetic modulo n, the order of secp521r1's group, for
 * the batched ECDSA verification: what turns (r, s, e) into the two scalars
 * of the double-scalar multiplication.
 *
 * n is no Mersenne prime, so multiplication is Montgomery's, word by word
 * (CIOS) with R = 2^544: sc_mont_mul(a, b) = a b / R mod n, fully reduced,
 * for any a below 2^544 and b below n.  Values are 17 little-endian 32-bit
 * limbs, as the field's.  Not constant-time: public data only.
 *
 * Host + device code (see p521_field.h).
 */
#ifndef NET2_P521_SCALAR_H
#define NET2_P521_SCALAR_H

#include "p521_field.h"

struct p521_sc {
	uint32_t l[P521_LIMBS];
};

#define P521_N_INIT { \
	0x91386409u, 0xbb6fb71eu, 0x899c47aeu, 0x3bb5c9b8u, 0xf709a5d0u, 0x7fcc0148u, \
	0xbf2f966bu, 0x51868783u, 0xfffffffau, 0xffffffffu, 0xffffffffu, 0xffffffffu, \
	0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x000001ffu }
/* R^2 mod n, R = 2^544 */
#define P521_N_R2_INIT { \
	0x61c64ca7u, 0x1163115au, 0x4374a642u, 0x18354a56u, 0x0791d9dcu, 0x5d4dd6d3u, \
	0xd3402705u, 0x4fb35b72u, 0xb7756e3au, 0xcff3d142u, 0xa8e567bcu, 0x5bcc6d61u, \
	0x492d0d45u, 0x2d8e03d1u, 0x8c44383du, 0x5b5a3afeu, 0x0000019au }
/* p - n: r + n is below p exactly when r is below this */
#define P521_PMN_INIT { \
	0x6ec79bf6u, 0x449048e1u, 0x7663b851u, 0xc44a3647u, 0x08f65a2fu, 0x8033feb7u, \
	0x40d06994u, 0xae79787cu, 0x00000005u, 0, 0, 0, 0, 0, 0, 0, 0 }
#define P521_N0INV 0x79a995c7u		/* -1 / n mod 2^32 */

/* Namespace-scope constants a loop may index at run time: on the device they
 * sit in constant memory and a wave-uniform index reads them with scalar
 * loads; an array local to a function would go to scratch. */
#if defined(__HIPCC__)
#define P521_CONST static __device__ __constant__ const
#else
#define P521_CONST static const
#endif

/* limb i of n, a compile-time constant once i is */
P521_HD uint32_t sc_n_limb(int i)
{
	constexpr uint32_t n[P521_LIMBS] = P521_N_INIT;
	return n[i];
}

P521_HD p521_sc sc_n()
{
	p521_sc r;
	P521_UNROLL
	for (int i = 0; i < P521_LIMBS; i++)
		r.l[i] = sc_n_limb(i);
	return r;
}

/* 66 big-endian bytes at any alignment: all 528 bits, unreduced */
P521_HD p521_sc sc_load_be66(const uint8_t *b)
{
	bool dummy;
	const p521_fe f = fe_load_be66(b, &dummy);
	p521_sc r;
	P521_UNROLL
	for (int i = 0; i < P521_LIMBS; i++)
		r.l[i] = f.l[i];
	return r;
}

P521_HD bool sc_is_zero(const p521_sc &a)
{
	uint32_t any = 0;
	P521_UNROLL
	for (int i = 0; i < P521_LIMBS; i++)
		any |= a.l[i];
	return any == 0;
}

/* a - b into *d; returns the borrow, that is a < b */
P521_HD bool sc_sub_borrow(p521_sc *d, const p521_sc &a, const p521_sc &b)
{
	uint64_t c = 0;
	P521_UNROLL
	for (int i = 0; i < P521_LIMBS; i++) {
		c = (uint64_t)a.l[i] - b.l[i] - c;
		d->l[i] = (uint32_t)c;
		c = c >> 63;
	}
	return c != 0;
}

P521_HD bool sc_lt(const p521_sc &a, const p521_sc &b)
{
	p521_sc d;
	return sc_sub_borrow(&d, a, b);
}

/* a + n, for a below p - n (no carry out of the limbs) */
P521_HD p521_sc sc_add_n(const p521_sc &a)
{
	p521_sc r;
	uint64_t c = 0;
	P521_UNROLL
	for (int i = 0; i < P521_LIMBS; i++) {
		c += (uint64_t)a.l[i] + sc_n_limb(i);
		r.l[i] = (uint32_t)c;
		c >>= 32;
	}
	return r;
}

/*
 * a b / R mod n.  Each of the 17 rounds adds a.l[i] b and then the multiple
 * of n that clears the low word, and drops that word; with a < R and b < n
 * the running value stays below 2n, so it fits the 17 limbs plus one carry
 * word, and one conditional subtraction reduces it.
 */
P521_HD p521_sc sc_mont_mul(const p521_sc &a, const p521_sc &b)
{
	uint32_t t[P521_LIMBS + 1];
	P521_UNROLL
	for (int i = 0; i <= P521_LIMBS; i++)
		t[i] = 0;
	P521_UNROLL
	for (int i = 0; i < P521_LIMBS; i++) {
		uint64_t c = 0;
		P521_UNROLL
		for (int j = 0; j < P521_LIMBS; j++) {
			c += (uint64_t)a.l[i] * b.l[j] + t[j];
			t[j] = (uint32_t)c;
			c >>= 32;
		}
		c += t[P521_LIMBS];
		t[P521_LIMBS] = (uint32_t)c;
		const uint32_t over = (uint32_t)(c >> 32);
		const uint32_t m = t[0] * P521_N0INV;
		c = ((uint64_t)m * sc_n_limb(0) + t[0]) >> 32;
		P521_UNROLL
		for (int j = 1; j < P521_LIMBS; j++) {
			c += (uint64_t)m * sc_n_limb(j) + t[j];
			t[j - 1] = (uint32_t)c;
			c >>= 32;
		}
		c += t[P521_LIMBS];
		t[P521_LIMBS - 1] = (uint32_t)c;
		t[P521_LIMBS] = over + (uint32_t)(c >> 32);
	}
	p521_sc r, d;
	P521_UNROLL
	for (int i = 0; i < P521_LIMBS; i++)
		r.l[i] = t[i];
	/* t[17] is zero: the value is below 2n < 2^522 */
	const bool below = sc_sub_borrow(&d, r, sc_n());
	return below ? r : d;
}

P521_CONST uint32_t p521_n_minus_2[P521_LIMBS] = {
	0x91386407u, 0xbb6fb71eu, 0x899c47aeu, 0x3bb5c9b8u, 0xf709a5d0u, 0x7fcc0148u,
	0xbf2f966bu, 0x51868783u, 0xfffffffau, 0xffffffffu, 0xffffffffu, 0xffffffffu,
	0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x000001ffu };

/*
 * ECDSA's two scalars, u1 = e / s and u2 = r / s mod n, for s in [1, n - 1],
 * r below n and any e below 2^544.
 *
 * One chain of Montgomery products through a single site, so that the
 * kernel holds one copy of the multiply: s R first (s times R^2), then
 * (s R)^(n - 2) = R / s by square-and-multiply over the bits of n - 2 below
 * its top one (Fermat; n is prime), and e (R / s) / R = e / s, likewise r / s,
 * leave the Montgomery form on their own.  The exponent is a constant, so
 * the branches on its bits are uniform across a wave.
 */
P521_HD void sc_u1_u2(const p521_sc &r, const p521_sc &s, const p521_sc &e,
    p521_sc *u1, p521_sc *u2)
{
	constexpr uint32_t r2[P521_LIMBS] = P521_N_R2_INIT;
	p521_sc acc, sm = s;
	P521_UNROLL
	for (int i = 0; i < P521_LIMBS; i++)
		acc.l[i] = r2[i];
	/* step -1: s R^2 / R.  Steps 2k and 2k + 1: the square and, where bit
	 * 519 - k of n - 2 is set, the multiplication.  Then e and r times the
	 * inverse. */
	const int chain = 2 * 520;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
	for (int step = -1; step < chain + 2; step++) {
		const bool mul = step >= 0 && step < chain && (step & 1) != 0;
		if (mul) {
			const int bit = 519 - (step >> 1);
			if ((p521_n_minus_2[bit >> 5] >> (bit & 31) & 1) == 0)
				continue;
		}
		const p521_sc left = step == -1 ? s : step == chain ? e :
		    step == chain + 1 ? r : acc;
		const p521_sc prod = sc_mont_mul(left, mul ? sm : acc);
		if (step == -1)
			sm = prod;
		if (step < chain)
			acc = prod;
		else if (step == chain)
			*u1 = prod;
		else
			*u2 = prod;
	}
}

#endif /* NET2_P521_SCALAR_H */
