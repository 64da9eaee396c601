/*
 * p521_keytab.h -- prepared key tables for the ECDSA P-521 verification
 * (include/net2/ecdsa_key.h): fixed-window multiples of a public key, built
 * once, and the verification that runs from them without a doubling.  The
 * lanes of ecdsa_key_kernels.hip run this code and
 * tests/cxx/test_ecdsa_key_host.cc runs it on the host.
 *
 * A table holds, for each of 131 windows j of 4 bits and each digit d = 1..15,
 * the affine point d 16^j Q in canonical limbs (fully reduced: p never stands
 * for 0), so that tables compare byte for byte.  u1 G + u2 Q is then the sum
 * of at most 131 entries of G's table and 131 of the key's: mixed additions
 * only, 11 field multiplications each, about 2,900 in all against the 9,800 of
 * the bit-by-bit pass (ecdsa_p521.h).  The scalar chain (sc_u1_u2), the range
 * checks and the last comparison are that pass's own, unchanged.
 *
 * Every exceptional case of the mixed addition is kept (p521_madd_cases):
 * small and crafted scalars make the running sum meet an entry, its negative
 * or infinity.  R = T asks for the one doubling this schedule has.
 *
 * Building a table: one lane per (table, window).  The lane doubles Q 4j
 * times, makes 16^j Q affine (first inversion), then walks 2P, 3P .. 15P in
 * Jacobian coordinates.  Z_k+1 = Z_k H_k, so the inverses of all Z_k follow
 * from that of Z_15 alone by multiplying the H_k back in (the product trick,
 * second inversion); the H_k wait in the table's own entries, which are not
 * final yet.  A second walk of the same chain -- 14 additions, nothing
 * against an inversion's 1,040 multiplications -- meets each 1 / Z_k and
 * stores the canonical x, y.  No storage beyond the nine registers and the
 * table itself.
 *
 * Not constant-time, deliberately: keys, signatures and digests are public.
 * Host + device code (see p521_field.h).
 */
#ifndef NET2_P521_KEYTAB_H
#define NET2_P521_KEYTAB_H

#include "ecdsa_p521.h"

#include <stddef.h>

#define P521_KT_WINDOWS 131
#define P521_KT_DIGITS 15
#define P521_KT_ENTRY_WORDS (2 * P521_LIMBS)
#define P521_KT_HEAD_WORDS 4
#define P521_KT_TABLE_WORDS \
	(P521_KT_HEAD_WORDS + P521_KT_WINDOWS * P521_KT_DIGITS * P521_KT_ENTRY_WORDS)
#define P521_KT_MAGIC 0x4b543531u	/* "15TK" */

/*
 * The programs the tables add, in a table of their own: p521_progs keeps its
 * six programs and their places, which the verification kernel and
 * tests/cxx/test_ecdsa_host.cc hold it to.  A program number from
 * P521_KT_PROG on names a start within p521_kt_progs, any other one within
 * p521_progs, and p521_kt_run runs either, so that a kernel still holds a
 * single copy of the field multiply.
 */
enum {
	P521_KT_PROG = 256,
	P521_PROG_INV_STEP = P521_KT_PROG + 0,
	P521_PROG_INV_TAIL = P521_KT_PROG + 3,
	P521_PROG_TOAFF = P521_KT_PROG + 7,
	P521_PROG_INV_BACK = P521_KT_PROG + 12,
	P521_PROG_NORM = P521_KT_PROG + 14
};

#define P521_MUL(d, a, b) { P521_OP_MUL, P521_R_##d, P521_R_##a, P521_R_##b }
#define P521_END { P521_OP_END, 0, 0, 0 }

P521_CONST p521_op p521_kt_progs[] = {
	/* P521_PROG_INV_STEP: one step of A = Z^(2^521 - 3) (fe_inv's loop) */
	P521_MUL(A, A, A), P521_MUL(A, A, Z), P521_END,
	/* P521_PROG_INV_TAIL: ... and the exponent's low "01" */
	P521_MUL(A, A, A), P521_MUL(A, A, A), P521_MUL(A, A, Z), P521_END,
	/* P521_PROG_TOAFF: with A = 1 / Z, the running point into QX, QY */
	P521_MUL(B, A, A), P521_MUL(QX, X, B), P521_MUL(B, B, A),
	P521_MUL(QY, Y, B), P521_END,
	/* P521_PROG_INV_BACK: 1 / Z_k = (1 / Z_k+1) H_k, H_k in B */
	P521_MUL(A, A, B), P521_END,
	/* P521_PROG_NORM: with A = 1 / Z, the running point's x into C, y into D */
	P521_MUL(B, A, A), P521_MUL(C, X, B), P521_MUL(B, B, A),
	P521_MUL(D, Y, B), P521_END,
};

#undef P521_MUL
#undef P521_END

/* p521_run over both tables. */
template <class M> P521_HD void p521_kt_run(M &m, int prog, bool act)
{
	const p521_op *pc = prog >= P521_KT_PROG ?
	    p521_kt_progs + (prog - P521_KT_PROG) : p521_progs + prog;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
	for (; pc->op != P521_OP_END; pc++) {
		const p521_op o = *pc;
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

/* Element `slot` (0: x, 1: y) of digit d's entry within a window's entries. */
P521_HD p521_fe kt_load(const uint32_t *win, int d, int slot)
{
	const uint32_t *e = win + (d - 1) * P521_KT_ENTRY_WORDS + slot * P521_LIMBS;
	p521_fe r;
	P521_UNROLL
	for (int i = 0; i < P521_LIMBS; i++)
		r.l[i] = e[i];
	return r;
}

P521_HD void kt_store(uint32_t *win, int d, int slot, const p521_fe &v)
{
	uint32_t *e = win + (d - 1) * P521_KT_ENTRY_WORDS + slot * P521_LIMBS;
	P521_UNROLL
	for (int i = 0; i < P521_LIMBS; i++)
		e[i] = v.l[i];
}

/* the low four bits off, the rest down */
P521_HD void sc_shr4(p521_sc &a)
{
	P521_UNROLL
	for (int i = 0; i < 16; i++)
		a.l[i] = a.l[i] >> 4 | a.l[i + 1] << 28;
	a.l[16] >>= 4;
}

template <class M> P521_HD void kt_restart(M &m)
{
	p521_st(m, P521_R_X, p521_ld(m, P521_R_QX));
	p521_st(m, P521_R_Y, p521_ld(m, P521_R_QY));
	p521_st(m, P521_R_Z, fe_one());
}

/* ---- building ----------------------------------------------------------- */

enum {
	KT_ST_CURVE,		/* is Q on the curve? */
	KT_ST_DBLS,		/* 4j doublings: 16^j Q */
	KT_ST_INV,		/* A = 1 / Z, the loop ... */
	KT_ST_INV_TAIL,		/* ... and its end */
	KT_ST_TOAFF,		/* P = 16^j Q affine, in QX, QY */
	KT_ST_DBL2,		/* 2P */
	KT_ST_ADD1,		/* (k - 1) P + P, part 1 */
	KT_ST_ADD2,		/* ... part 2 */
	KT_ST_BACK,		/* 1 / Z_k from 1 / Z_k+1 */
	KT_ST_NORM,		/* k P affine */
	KT_ST_DONE
};

/*
 * One window's fifteen entries: d 16^j Q at win (digit d's entry at
 * win + (d - 1) * 34 words) for the Q in registers QX, QY.  Every lane of a
 * wave runs the same stages; `j` may differ (a lane doubles while its 4j are
 * not done and computes along after), and a lane that is not `live` touches
 * no memory.  *on_curve is whether Q satisfies the curve's equation; the
 * entries of a Q that does not are unspecified.  Between the two walks the
 * x halves of entries 2..15 hold H_k, then 1 / Z_k, in weak form.
 */
template <class M>
P521_HD void p521_keytab_build_window(M &m, int j, uint32_t *win, bool live,
    bool *on_curve)
{
	const int ndbl = 4 * j;
	int stage = KT_ST_CURVE, cnt = 0, k = 0, phase = 0;
	while (stage != KT_ST_DONE) {
		int prog = P521_PROG_DBL;
		bool act = true;
		if (stage == KT_ST_CURVE) {
			prog = P521_PROG_CURVE;
		} else if (stage == KT_ST_DBLS) {
			act = cnt < ndbl;
		} else if (stage == KT_ST_INV) {
			prog = P521_PROG_INV_STEP;
		} else if (stage == KT_ST_INV_TAIL) {
			prog = P521_PROG_INV_TAIL;
		} else if (stage == KT_ST_TOAFF) {
			prog = P521_PROG_TOAFF;
		} else if (stage == KT_ST_ADD1) {
			prog = P521_PROG_MADD1_Q;
		} else if (stage == KT_ST_ADD2) {
			prog = P521_PROG_MADD2;
		} else if (stage == KT_ST_BACK) {
			if (live)
				p521_st(m, P521_R_B, kt_load(win, k, 0));
			prog = P521_PROG_INV_BACK;
		} else if (stage == KT_ST_NORM) {
			if (live)
				p521_st(m, P521_R_A, kt_load(win, k, 0));
			prog = P521_PROG_NORM;
		}
		if (m.any(act))
			p521_kt_run(m, prog, act);
		if (stage == KT_ST_CURVE) {
			*on_curve = fe_is_zero(p521_ld(m, P521_R_A));
			kt_restart(m);
			stage = KT_ST_DBLS;
		} else if (stage == KT_ST_DBLS) {
			cnt++;
			if (!m.any(cnt < ndbl)) {
				p521_st(m, P521_R_A, p521_ld(m, P521_R_Z));
				cnt = 0;
				stage = KT_ST_INV;
			}
		} else if (stage == KT_ST_INV) {
			if (++cnt == 518)
				stage = KT_ST_INV_TAIL;
		} else if (stage == KT_ST_INV_TAIL) {
			if (phase == 0) {
				stage = KT_ST_TOAFF;
			} else {
				if (live)
					kt_store(win, P521_KT_DIGITS, 0,
					    p521_ld(m, P521_R_A));
				k = P521_KT_DIGITS - 1;
				stage = KT_ST_BACK;
			}
		} else if (stage == KT_ST_TOAFF) {
			if (live) {
				kt_store(win, 1, 0, fe_canon(p521_ld(m, P521_R_QX)));
				kt_store(win, 1, 1, fe_canon(p521_ld(m, P521_R_QY)));
			}
			kt_restart(m);
			phase = 1;
			stage = KT_ST_DBL2;
		} else if (stage == KT_ST_DBL2) {
			k = 2;
			if (phase == 1) {
				k = 3;
				stage = KT_ST_ADD1;
			} else {
				stage = KT_ST_NORM;
			}
		} else if (stage == KT_ST_ADD1) {
			/* H of (k - 1) P + P: Z_k = Z_k-1 H_k-1 */
			if (phase == 1 && live)
				kt_store(win, k - 1, 0, p521_ld(m, P521_R_B));
			stage = KT_ST_ADD2;
		} else if (stage == KT_ST_ADD2) {
			if (phase == 2) {
				stage = KT_ST_NORM;
			} else if (k == P521_KT_DIGITS) {
				p521_st(m, P521_R_A, p521_ld(m, P521_R_Z));
				cnt = 0;
				stage = KT_ST_INV;
			} else {
				k++;
				stage = KT_ST_ADD1;
			}
		} else if (stage == KT_ST_BACK) {
			if (live)
				kt_store(win, k, 0, p521_ld(m, P521_R_A));
			if (--k < 2) {
				kt_restart(m);
				phase = 2;
				stage = KT_ST_DBL2;
			}
		} else {	/* KT_ST_NORM */
			if (live) {
				kt_store(win, k, 0, fe_canon(p521_ld(m, P521_R_C)));
				kt_store(win, k, 1, fe_canon(p521_ld(m, P521_R_D)));
			}
			if (k == P521_KT_DIGITS) {
				stage = KT_ST_DONE;
			} else {
				k++;
				stage = KT_ST_ADD1;
			}
		}
	}
}

/*
 * Window j of one table: pub is x || y (66 big-endian bytes each, any
 * alignment), or null for the base point G.  Returns whether the key is one a
 * verification accepts: both coordinates below p and the point on the curve.
 * The lane of window 0 writes the table's head.
 */
template <class M>
P521_HD bool p521_keytab_build_one(M &m, const uint8_t *pub, int j,
    uint32_t *table, bool live)
{
	bool x_ok = true, y_ok = true, on_curve = false;
	if (pub != nullptr) {
		p521_st(m, P521_R_QX, fe_load_be66(pub, &x_ok));
		p521_st(m, P521_R_QY, fe_load_be66(pub + P521_BYTES, &y_ok));
	} else {
		p521_st(m, P521_R_QX, p521_ld(m, P521_R_GX));
		p521_st(m, P521_R_QY, p521_ld(m, P521_R_GY));
	}
	p521_keytab_build_window(m, j, table + P521_KT_HEAD_WORDS +
	    j * P521_KT_DIGITS * P521_KT_ENTRY_WORDS, live, &on_curve);
	const bool valid = x_ok && y_ok && on_curve;
	if (live && j == 0) {
		table[0] = P521_KT_MAGIC;
		table[1] = valid ? 1u : 0u;
		table[2] = 0;
		table[3] = 0;
	}
	return valid;
}

/* ---- verifying ---------------------------------------------------------- */

/*
 * R = u1 G + u2 Q from the two tables' entries (gwin, kwin: the first entry
 * of each), then the last comparison against r: for each window the entry of
 * u1's digit from G's table, then that of u2's digit from the key's, each
 * added where the digit is not zero.  The running point starts at infinity.
 */
template <class M>
P521_HD void ecdsa_p521_keytab_engine(M &m, p521_lane &L, p521_sc u1, p521_sc u2,
    const p521_sc &r, const uint32_t *gwin, const uint32_t *kwin, bool *match)
{
	int stage = ECDSA_ST_ADD1, which = 0, j = 0;
	bool want = false, normal = false, second = false;
	while (stage != ECDSA_ST_DONE) {
		int prog = P521_PROG_DBL;
		bool act = true;
		if (stage == ECDSA_ST_ADD1) {
			const uint32_t d = (which == 0 ? u1 : u2).l[0] & 15u;
			want = d != 0;
			if (want) {
				const uint32_t *w = (which == 0 ? gwin : kwin) +
				    j * P521_KT_DIGITS * P521_KT_ENTRY_WORDS;
				p521_st(m, P521_R_QX, kt_load(w, (int)d, 0));
				p521_st(m, P521_R_QY, kt_load(w, (int)d, 1));
			}
			prog = P521_PROG_MADD1_Q;
			act = want;
		} else if (stage == ECDSA_ST_ADD2) {
			prog = P521_PROG_MADD2;
			act = normal;
		} else if (stage == ECDSA_ST_FIX) {
			act = L.fix;
		} else {	/* ECDSA_ST_FINAL */
			second = ecdsa_p521_final_setup(m, r);
			prog = P521_PROG_FINAL;
		}
		if (m.any(act))
			p521_kt_run(m, prog, act);
		if (stage == ECDSA_ST_ADD1) {
			normal = want && p521_madd_cases(m, L, 1);
			stage = ECDSA_ST_ADD2;
		} else if (stage == ECDSA_ST_ADD2) {
			stage = ECDSA_ST_FIX;
		} else if (stage == ECDSA_ST_FIX) {
			L.fix = false;
			stage = ECDSA_ST_ADD1;
			if (which == 0) {
				which = 1;
			} else {
				which = 0;
				sc_shr4(u1);
				sc_shr4(u2);
				if (++j == P521_KT_WINDOWS)
					stage = ECDSA_ST_FINAL;
			}
		} else {
			*match = !L.inf && ecdsa_p521_final_match(m, second);
			stage = ECDSA_ST_DONE;
		}
	}
}

/*
 * One verification under key `kidx` of the keytab (nkeys + 1 tables, G's
 * first): 1 or 0, what ecdsa_p521_verify_one gives for that key's bytes.  0
 * as well for a kidx of nkeys or more and for a table, G's included, whose
 * head does not say magic and valid.  Such a lane computes along on G's
 * table: nothing is read outside the keytab.
 */
template <class M>
P521_HD int ecdsa_p521_keytab_verify_one(M &m, const uint32_t *keytab,
    uint32_t nkeys, uint32_t kidx, const uint8_t *rs, const uint8_t *dig,
    uint32_t dlen)
{
	const bool g_ok = keytab[0] == P521_KT_MAGIC && keytab[1] == 1;
	const bool k_in = kidx < nkeys;
	const uint32_t *ktab = keytab +
	    (k_in ? (size_t)kidx + 1 : 0) * P521_KT_TABLE_WORDS;
	const bool k_ok = k_in && ktab[0] == P521_KT_MAGIC && ktab[1] == 1;
	bool match = false;
	const p521_sc r = sc_load_be66(rs), s = sc_load_be66(rs + P521_BYTES);
	const p521_sc n = sc_n();
	const bool range_ok = !sc_is_zero(r) && !sc_is_zero(s) && sc_lt(r, n) &&
	    sc_lt(s, n);
	const p521_sc e = ecdsa_p521_digest_to_e(dig, dlen);
	p521_sc u1, u2;
	sc_u1_u2(r, s, e, &u1, &u2);
	p521_st(m, P521_R_X, fe_one());
	p521_st(m, P521_R_Y, fe_one());
	p521_st(m, P521_R_Z, fe_zero());
	p521_lane L = { true, false };
	ecdsa_p521_keytab_engine(m, L, u1, u2, r, keytab + P521_KT_HEAD_WORDS,
	    ktab + P521_KT_HEAD_WORDS, &match);
	return g_ok && k_ok && range_ok && match;
}

#endif /* NET2_P521_KEYTAB_H */
