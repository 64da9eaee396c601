/*
 * p521_point.h -- secp521r1 points (a = -3, Jacobian coordinates) for the
 * batched ECDSA verification, as straight-line programs over a small file of
 * field registers.
 *
 * Why programs.  A verification is about 10^4 field multiplications and the
 * multiply is some 1,400 instructions long once unrolled, so the kernel must
 * not hold one copy per use.  The formulas are therefore tables of
 * three-address operations (p521_op) and p521_run() is the only place that
 * multiplies: one loop, one fe_mul.  The operands live in a register file M
 * that the caller supplies -- on the device LDS in a lane-strided layout
 * (ecdsa_kernels.hip), on the host a plain array -- because a register file
 * indexed by a program goes to scratch if it is a private array.  The cost is
 * 51 LDS words per operation against the multiply's 289 multiply-adds.
 *
 * A program is the same for every lane of a wave; what differs per lane is
 * `act`, whether the lane stores the results.  The exceptional cases of the
 * addition are settled between programs, per lane (p521_madd_*).
 *
 * Completeness, for this use.  Infinity is Z = 0.
 *  - p521_prog_dbl is dbl-2001-b with Z3 = 2 Y Z; Z = 0 gives Z3 = 0, and the
 *    group has prime order, so no finite point has Y = 0: the doubling needs
 *    no case at all.
 *  - The mixed addition R + T (T affine, never infinity) is split in two.
 *    Part 1 computes H = x_T Z^2 - X and r = y_T Z^3 - Y.  Then, per lane:
 *    R = infinity gives T; H = 0 and r = 0 is R = T, which gives T and asks
 *    for one more doubling (p521_lane::fix); H = 0 alone is R = -T, which
 *    gives infinity; every other lane runs part 2, the ordinary formulas.
 * Nothing is constant-time: every input of a verification is public.
 *
 * A general Jacobian + Jacobian addition is not here because nothing uses
 * it: the double-scalar multiplication adds the affine G and Q one at a time.
 *
 * Host + device code (see p521_field.h).
 */
#ifndef NET2_P521_POINT_H
#define NET2_P521_POINT_H

#include "p521_field.h"
#include "p521_scalar.h"

/* The register file: the running point, the public key, four temporaries.
 * From P521_R_CONST on a register number names a constant. */
enum {
	P521_R_X, P521_R_Y, P521_R_Z, P521_R_QX, P521_R_QY,
	P521_R_A, P521_R_B, P521_R_C, P521_R_D,
	P521_REGS,
	P521_R_CONST = P521_REGS,
	P521_R_GX = P521_R_CONST, P521_R_GY, P521_R_CB
};

enum { P521_OP_END, P521_OP_MUL, P521_OP_ADD, P521_OP_SUB };

struct p521_op {
	uint8_t op, d, a, b;
};

P521_CONST uint32_t p521_consts[3][P521_LIMBS] = {
	P521_GX_INIT, P521_GY_INIT, P521_B_INIT
};

#define P521_MUL(d, a, b) { P521_OP_MUL, P521_R_##d, P521_R_##a, P521_R_##b }
#define P521_ADD(d, a, b) { P521_OP_ADD, P521_R_##d, P521_R_##a, P521_R_##b }
#define P521_SUB(d, a, b) { P521_OP_SUB, P521_R_##d, P521_R_##a, P521_R_##b }
#define P521_END { P521_OP_END, 0, 0, 0 }

/* Program starts within p521_progs. */
enum {
	P521_PROG_CURVE = 0,
	P521_PROG_DBL = 9,
	P521_PROG_MADD1_G = 32,
	P521_PROG_MADD1_Q = 39,
	P521_PROG_MADD2 = 46,
	P521_PROG_FINAL = 59
};

P521_CONST p521_op p521_progs[] = {
	/* P521_PROG_CURVE: A = x^3 - 3x + b - y^2 of the public key */
	P521_MUL(A, QX, QX), P521_MUL(A, A, QX), P521_ADD(B, QX, QX),
	P521_ADD(B, B, QX), P521_SUB(A, A, B), P521_ADD(A, A, CB),
	P521_MUL(B, QY, QY), P521_SUB(A, A, B), P521_END,
	/* P521_PROG_DBL: delta = Z^2, gamma = Y^2, beta = X gamma,
	 * alpha = 3 (X - delta)(X + delta); X3 = alpha^2 - 8 beta, Z3 = 2 Y Z,
	 * Y3 = alpha (4 beta - X3) - 8 gamma^2 */
	P521_MUL(A, Z, Z), P521_MUL(B, Y, Y), P521_MUL(C, X, B),
	P521_SUB(D, X, A), P521_ADD(A, X, A), P521_MUL(D, D, A),
	P521_ADD(A, D, D), P521_ADD(D, A, D),
	P521_MUL(Z, Y, Z), P521_ADD(Z, Z, Z),
	P521_MUL(A, D, D), P521_ADD(C, C, C), P521_ADD(C, C, C),
	P521_SUB(X, A, C), P521_SUB(X, X, C),
	P521_SUB(C, C, X), P521_MUL(C, D, C), P521_MUL(B, B, B),
	P521_ADD(B, B, B), P521_ADD(B, B, B), P521_ADD(B, B, B),
	P521_SUB(Y, C, B), P521_END,
	/* P521_PROG_MADD1_G: B = H = x_T Z^2 - X, A = r = y_T Z^3 - Y, T = G */
	P521_MUL(A, Z, Z), P521_MUL(B, GX, A), P521_MUL(A, Z, A),
	P521_MUL(A, GY, A), P521_SUB(B, B, X), P521_SUB(A, A, Y), P521_END,
	/* P521_PROG_MADD1_Q: the same, T = Q */
	P521_MUL(A, Z, Z), P521_MUL(B, QX, A), P521_MUL(A, Z, A),
	P521_MUL(A, QY, A), P521_SUB(B, B, X), P521_SUB(A, A, Y), P521_END,
	/* P521_PROG_MADD2: V = X H^2; X3 = r^2 - H^3 - 2V, Z3 = Z H,
	 * Y3 = r (V - X3) - Y H^3 */
	P521_MUL(C, B, B), P521_MUL(D, B, C), P521_MUL(C, X, C),
	P521_MUL(Z, Z, B), P521_MUL(X, A, A), P521_SUB(X, X, D),
	P521_SUB(X, X, C), P521_SUB(X, X, C), P521_SUB(C, C, X),
	P521_MUL(C, A, C), P521_MUL(D, Y, D), P521_SUB(Y, C, D), P521_END,
	/* P521_PROG_FINAL: A = Z^2; C and D, holding r and r + n (or 0), times it */
	P521_MUL(A, Z, Z), P521_MUL(C, C, A), P521_MUL(D, D, A), P521_END,
};

#undef P521_MUL
#undef P521_ADD
#undef P521_SUB
#undef P521_END

/* A plain-array register file: the host's, one lane. */
struct p521_host_regs {
	uint32_t w[P521_REGS * P521_LIMBS];
	uint32_t ld(int reg, int limb) const { return w[reg * P521_LIMBS + limb]; }
	void st(int reg, int limb, uint32_t v) { w[reg * P521_LIMBS + limb] = v; }
	/* does any lane of the wave want it?  One lane here. */
	bool any(bool x) const { return x; }
};

template <class M> P521_HD p521_fe p521_ld(const M &m, int reg)
{
	p521_fe r;
	if (reg >= P521_R_CONST) {
		P521_UNROLL
		for (int i = 0; i < P521_LIMBS; i++)
			r.l[i] = p521_consts[reg - P521_R_CONST][i];
	} else {
		P521_UNROLL
		for (int i = 0; i < P521_LIMBS; i++)
			r.l[i] = m.ld(reg, i);
	}
	return r;
}

template <class M> P521_HD void p521_st(M &m, int reg, const p521_fe &v)
{
	P521_UNROLL
	for (int i = 0; i < P521_LIMBS; i++)
		m.st(reg, i, v.l[i]);
}

/* Runs the program at `start`; a lane with !act computes along and stores
 * nothing. */
template <class M> P521_HD void p521_run(M &m, int start, bool act)
{
#if defined(__HIPCC__)
#pragma unroll 1
#endif
	for (int pc = start; p521_progs[pc].op != P521_OP_END; pc++) {
		const p521_op o = p521_progs[pc];
		const p521_fe a = p521_ld(m, o.a), b = p521_ld(m, o.b);
		p521_fe r;
		if (o.op == P521_OP_MUL)
			r = fe_mul(a, b);
		else if (o.op == P521_OP_ADD)
			r = fe_add(a, b);
		else
			r = fe_sub(a, b);
		if (act)
			p521_st(m, o.d, r);
	}
}

/* One lane's state between the programs. */
struct p521_lane {
	bool inf;	/* the running point is infinity */
	bool fix;	/* it was set to T where 2T is due: double once more */
};

/* The affine T of an addition into the running point: G (which = 0) or Q. */
template <class M> P521_HD void p521_set_affine(M &m, int which)
{
	p521_st(m, P521_R_X, p521_ld(m, which == 0 ? P521_R_GX : P521_R_QX));
	p521_st(m, P521_R_Y, p521_ld(m, which == 0 ? P521_R_GY : P521_R_QY));
	p521_st(m, P521_R_Z, fe_one());
}

/*
 * Between the two parts of R + T, for a lane that wants the addition: settles
 * the exceptional cases from part 1's H and r and returns whether the lane
 * runs part 2.
 */
template <class M> P521_HD bool p521_madd_cases(M &m, p521_lane &L, int which)
{
	if (L.inf) {
		p521_set_affine(m, which);
		L.inf = false;
		return false;
	}
	if (!fe_is_zero(p521_ld(m, P521_R_B)))
		return true;
	if (fe_is_zero(p521_ld(m, P521_R_A))) {
		p521_set_affine(m, which);
		L.fix = true;
	} else {
		p521_st(m, P521_R_Z, fe_zero());
		L.inf = true;
	}
	return false;
}

#endif /* NET2_P521_POINT_H */
