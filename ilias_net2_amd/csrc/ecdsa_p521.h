/*
 * ecdsa_p521.h -- one ECDSA verification over secp521r1 with the meaning of
 * OpenSSL's ECDSA_do_verify, as the lanes of ecdsa_p521_verify_kernel
 * (ecdsa_kernels.hip) run it and as tests/cxx/test_ecdsa_host.cc runs it on
 * the host.
 *
 *   reject unless 1 <= r, s <= n - 1, 0 <= Qx, Qy < p and Q is on the curve;
 *   e = the digest's leftmost 66 bytes, shifted right 7 bits if those are 66;
 *   u1 = e / s, u2 = r / s mod n;  R = u1 G + u2 Q;
 *   accept iff R is not infinity and x(R) mod n = r.
 *
 * R comes from one interleaved pass over the 521 bit positions (Shamir's
 * trick without the G + Q entry: double, add G where u1 has the bit, add Q
 * where u2 has it), 8 + 11 (b1 + b2) field multiplications a bit.  Leaving
 * G + Q out costs a quarter of an addition per bit and saves what making it
 * affine would need: a field inversion per lane and two more registers of
 * the register file, which is what bounds the waves per CU (p521_point.h).
 * There are no tables beyond the lane's own Q and the constant G.
 *
 * ecdsa_p521_engine is the whole schedule as one loop around one p521_run(),
 * so that the kernel holds a single copy of the field multiply; its stage
 * and bit counters are the same in every lane of a wave, the lanes differ
 * in who stores.  The last comparison is made without leaving Jacobian
 * coordinates: x(R) = X / Z^2 lies in [0, p) and p < 2n, so x(R) mod n = r
 * iff X = r Z^2 or (r + n < p and X = (r + n) Z^2).
 *
 * Not constant-time, deliberately: a verification sees public data only.
 * Host + device code (see p521_field.h).
 */
#ifndef NET2_ECDSA_P521_H
#define NET2_ECDSA_P521_H

#include "p521_field.h"
#include "p521_scalar.h"
#include "p521_point.h"

#define ECDSA_P521_PUB_BYTES (2 * P521_BYTES)	/* x || y */
#define ECDSA_P521_SIG_BYTES (2 * P521_BYTES)	/* r || s */

/* ECDSA_do_verify's e (ossl_ecdsa_simple_verify_sig): the digest's leftmost
 * 66 bytes as a big-endian number, and of 528 bits only the top 521. */
P521_HD p521_sc ecdsa_p521_digest_to_e(const uint8_t *dig, uint32_t dlen)
{
	const uint32_t len = dlen < P521_BYTES ? dlen : P521_BYTES;
	p521_sc e;
	P521_UNROLL
	for (int i = 0; i < P521_LIMBS; i++)
		e.l[i] = 0;
	P521_UNROLL
	for (int k = 0; k < P521_BYTES; k++)
		if ((uint32_t)k < len)
			e.l[k >> 2] |= (uint32_t)dig[len - 1 - k] << 8 * (k & 3);
	if (dlen >= P521_BYTES) {
		P521_UNROLL
		for (int i = 0; i < 16; i++)
			e.l[i] = e.l[i] >> 7 | e.l[i + 1] << 25;
		e.l[16] >>= 7;
	}
	return e;
}

/* A scalar below 2^521 with its bit 520 moved to the top of limb 16, where
 * the engine reads the bits off (sc_top_bit, sc_shl1). */
P521_HD p521_sc sc_align_top(const p521_sc &a)
{
	p521_sc r;
	P521_UNROLL
	for (int i = 16; i > 0; i--)
		r.l[i] = a.l[i] << 23 | a.l[i - 1] >> 9;
	r.l[0] = a.l[0] << 23;
	return r;
}

P521_HD bool sc_top_bit(const p521_sc &a)
{
	return (a.l[16] >> 31) != 0;
}

P521_HD void sc_shl1(p521_sc &a)
{
	P521_UNROLL
	for (int i = 16; i > 0; i--)
		a.l[i] = a.l[i] << 1 | a.l[i - 1] >> 31;
	a.l[0] <<= 1;
}

/* Before P521_PROG_FINAL: r into C, r + n into D where that is below p. */
template <class M> P521_HD bool ecdsa_p521_final_setup(M &m, const p521_sc &r)
{
	constexpr uint32_t pmn[P521_LIMBS] = P521_PMN_INIT;
	p521_sc lim;
	P521_UNROLL
	for (int i = 0; i < P521_LIMBS; i++)
		lim.l[i] = pmn[i];
	const bool second = sc_lt(r, lim);
	const p521_sc rn = sc_add_n(r);
	p521_fe c, d;
	P521_UNROLL
	for (int i = 0; i < P521_LIMBS; i++) {
		c.l[i] = r.l[i];
		d.l[i] = second ? rn.l[i] : 0;
	}
	p521_st(m, P521_R_C, c);
	p521_st(m, P521_R_D, d);
	return second;
}

/* After it: does X equal one of the candidates times Z^2? */
template <class M> P521_HD bool ecdsa_p521_final_match(const M &m, bool second)
{
	const p521_fe x = p521_ld(m, P521_R_X);
	return fe_eq(x, p521_ld(m, P521_R_C)) ||
	    (second && fe_eq(x, p521_ld(m, P521_R_D)));
}

enum {
	ECDSA_ST_CURVE,		/* is Q on the curve? */
	ECDSA_ST_DBL,		/* R = 2R */
	ECDSA_ST_ADD1,		/* R + T, part 1; T = G, then Q */
	ECDSA_ST_ADD2,		/* ... part 2, for the lanes without a special case */
	ECDSA_ST_FIX,		/* the doubling of a lane that met R = T */
	ECDSA_ST_FINAL,		/* x(R) mod n = r? */
	ECDSA_ST_DONE
};

/*
 * The schedule, from `stage` on: [CURVE,] then for each of `nbits` bit
 * positions DBL, ADD1/ADD2/FIX with G, ADD1/ADD2/FIX with Q -- the bits read
 * off the tops of u1 and u2 (sc_align_top) -- and FINAL if `finish`.
 * Starting at ECDSA_ST_ADD1 skips the first position's doubling.  The
 * running point is registers X, Y, Z with L.inf; Q is registers QX, QY.
 * *on_curve and *match are written by the stages that decide them.
 */
template <class M>
P521_HD void ecdsa_p521_engine(M &m, p521_lane &L, p521_sc u1, p521_sc u2,
    const p521_sc &r, int stage, int nbits, bool finish, bool *on_curve,
    bool *match)
{
	int which = 0;
	bool want = false, normal = false, second = false;
	while (stage != ECDSA_ST_DONE) {
		int prog = P521_PROG_DBL;
		bool act = true;
		if (stage == ECDSA_ST_CURVE) {
			prog = P521_PROG_CURVE;
		} else if (stage == ECDSA_ST_ADD1) {
			want = sc_top_bit(which == 0 ? u1 : u2);
			prog = which == 0 ? P521_PROG_MADD1_G : P521_PROG_MADD1_Q;
			act = want;
		} else if (stage == ECDSA_ST_ADD2) {
			prog = P521_PROG_MADD2;
			act = normal;
		} else if (stage == ECDSA_ST_FIX) {
			act = L.fix;
		} else if (stage == ECDSA_ST_FINAL) {
			second = ecdsa_p521_final_setup(m, r);
			prog = P521_PROG_FINAL;
		}
		if (m.any(act))
			p521_run(m, prog, act);
		const int after_bits = finish ? ECDSA_ST_FINAL : ECDSA_ST_DONE;
		if (stage == ECDSA_ST_CURVE) {
			*on_curve = fe_is_zero(p521_ld(m, P521_R_A));
			stage = nbits > 0 ? ECDSA_ST_DBL : after_bits;
		} else if (stage == ECDSA_ST_DBL) {
			which = 0;
			stage = ECDSA_ST_ADD1;
		} else if (stage == ECDSA_ST_ADD1) {
			normal = want && p521_madd_cases(m, L, which);
			stage = ECDSA_ST_ADD2;
		} else if (stage == ECDSA_ST_ADD2) {
			stage = ECDSA_ST_FIX;
		} else if (stage == ECDSA_ST_FIX) {
			L.fix = false;
			if (which == 0) {
				which = 1;
				stage = ECDSA_ST_ADD1;
			} else {
				sc_shl1(u1);
				sc_shl1(u2);
				stage = --nbits > 0 ? ECDSA_ST_DBL : after_bits;
			}
		} else {
			*match = !L.inf && ecdsa_p521_final_match(m, second);
			stage = ECDSA_ST_DONE;
		}
	}
}

/*
 * One verification: 1 or 0.  pub is x || y, rs is r || s, each value 66
 * big-endian bytes at any alignment; dig may be null when dlen is 0.  m is
 * the lane's register file (p521_point.h); what it held is overwritten.
 */
template <class M>
P521_HD int ecdsa_p521_verify_one(M &m, const uint8_t *pub, const uint8_t *rs,
    const uint8_t *dig, uint32_t dlen)
{
	bool x_ok, y_ok, on_curve = false, match = false;
	const p521_fe qx = fe_load_be66(pub, &x_ok);
	const p521_fe qy = fe_load_be66(pub + P521_BYTES, &y_ok);
	const p521_sc r = sc_load_be66(rs), s = sc_load_be66(rs + P521_BYTES);
	const p521_sc n = sc_n();
	const bool range_ok = x_ok && y_ok && !sc_is_zero(r) && !sc_is_zero(s) &&
	    sc_lt(r, n) && sc_lt(s, n);
	const p521_sc e = ecdsa_p521_digest_to_e(dig, dlen);
	p521_sc u1, u2;
	/* (a lane out of range computes along on whatever it loaded; nothing
	 * below indexes memory by data) */
	sc_u1_u2(r, s, e, &u1, &u2);
	p521_st(m, P521_R_QX, qx);
	p521_st(m, P521_R_QY, qy);
	p521_st(m, P521_R_X, fe_one());
	p521_st(m, P521_R_Y, fe_one());
	p521_st(m, P521_R_Z, fe_zero());
	p521_lane L = { true, false };
	ecdsa_p521_engine(m, L, sc_align_top(u1), sc_align_top(u2), r,
	    ECDSA_ST_CURVE, 521, true, &on_curve, &match);
	return range_ok && on_curve && match;
}

#endif /* NET2_ECDSA_P521_H */
