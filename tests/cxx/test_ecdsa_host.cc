/*
 * test_ecdsa_host.cc -- the P-521 verification's arithmetic on the host
 * (tests/test_ecdsa_host.py builds it under ASan + UBSan and runs it).
 *
 * Includes the headers ecdsa_kernels.hip is made of and holds them to
 * libcrypto: the field and scalar operations to BN_mod_*, the point programs
 * to EC_POINT_dbl / EC_POINT_add, the last comparison on crafted (X, Z, r),
 * and ecdsa_p521_verify_one to ECDSA_do_verify over the vectors of argv[1]
 * (records written by the Python side: the construction lattice and
 * OpenSSL-signed messages).  Exits non-zero with a message at the first
 * mismatch.
 */
#include "ecdsa_p521.h"

#include <openssl/bn.h>
#include <openssl/ec.h>
#include <openssl/ecdsa.h>
#include <openssl/obj_mac.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#pragma GCC diagnostic ignored "-Wdeprecated-declarations"

static BN_CTX *ctx;
static BIGNUM *P, *N;
static EC_GROUP *grp;

#define CHECK(c, ...)                                                       \
	do {                                                                \
		if (!(c)) {                                                 \
			fprintf(stderr, "test_ecdsa_host: %s:%d: ", __FILE__, \
			    __LINE__);                                      \
			fprintf(stderr, __VA_ARGS__);                       \
			fprintf(stderr, "\n");                              \
			exit(1);                                            \
		}                                                           \
	} while (0)

/* limbs <-> BIGNUM, without going through the code under test */
static BIGNUM *bn_of(const uint32_t *l)
{
	uint8_t b[68];
	for (int i = 0; i < 17; i++)
		for (int k = 0; k < 4; k++)
			b[67 - 4 * i - k] = (uint8_t)(l[i] >> 8 * k);
	return BN_bin2bn(b, 68, nullptr);
}

static void limbs_of(const BIGNUM *v, uint32_t *l)
{
	uint8_t b[68];
	CHECK(BN_bn2binpad(v, b, 68) == 68, "value too long");
	for (int i = 0; i < 17; i++)
		l[i] = (uint32_t)b[67 - 4 * i] | (uint32_t)b[66 - 4 * i] << 8 |
		    (uint32_t)b[65 - 4 * i] << 16 | (uint32_t)b[64 - 4 * i] << 24;
}

static p521_fe fe_of(const BIGNUM *v)
{
	p521_fe r;
	limbs_of(v, r.l);
	return r;
}

static p521_sc sc_of(const BIGNUM *v)
{
	p521_sc r;
	limbs_of(v, r.l);
	return r;
}

/* does the (weakly reduced) element equal v mod p? */
static bool fe_is(const p521_fe &a, const BIGNUM *v)
{
	CHECK(a.l[16] <= P521_TOP_MASK, "element above 2^521");
	BIGNUM *x = bn_of(fe_canon(a).l), *y = BN_new();
	BN_nnmod(y, v, P, ctx);
	const bool eq = BN_cmp(x, y) == 0;
	BN_free(x);
	BN_free(y);
	return eq;
}

static std::vector<BIGNUM *> field_operands()
{
	std::vector<BIGNUM *> v;
	auto add = [&](BIGNUM *b) { v.push_back(b); };
	BIGNUM *t;
	for (unsigned w : { 0u, 1u, 2u }) {
		t = BN_new();
		BN_set_word(t, w);
		add(t);
	}
	for (unsigned w : { 0u, 1u, 2u }) {	/* p (non-canonical zero), p - 1, p - 2 */
		t = BN_dup(P);
		BN_sub_word(t, w);
		add(t);
	}
	for (int k : { 32, 64, 256, 288, 512, 520 }) {	/* 2^k - 1: all-ones limbs; 2^k */
		t = BN_new();
		BN_set_bit(t, k);
		add(BN_dup(t));
		BN_sub_word(t, 1);
		add(t);
	}
	t = BN_new();			/* limb 16 full, the rest zero */
	BN_set_word(t, 0x1ff);
	BN_lshift(t, t, 512);
	add(t);
	t = BN_new();			/* sqrt-sized: (2^261 - 1)^2 folds with carries */
	BN_set_bit(t, 261);
	BN_sub_word(t, 1);
	add(t);
	for (int i = 0; i < 40; i++) {
		t = BN_new();
		BN_rand_range(t, P);
		add(t);
	}
	return v;
}

static void test_field()
{
	std::vector<BIGNUM *> ops = field_operands();
	BIGNUM *w = BN_new();
	for (size_t i = 0; i < ops.size(); i++) {
		const p521_fe a = fe_of(ops[i]);
		for (size_t j = 0; j < ops.size(); j++) {
			const p521_fe b = fe_of(ops[j]);
			BN_mod_mul(w, ops[i], ops[j], P, ctx);
			CHECK(fe_is(fe_mul(a, b), w), "fe_mul %zu %zu", i, j);
			BN_mod_add(w, ops[i], ops[j], P, ctx);
			CHECK(fe_is(fe_add(a, b), w), "fe_add %zu %zu", i, j);
			BN_mod_sub(w, ops[i], ops[j], P, ctx);
			CHECK(fe_is(fe_sub(a, b), w), "fe_sub %zu %zu", i, j);
			CHECK(fe_eq(a, b) == (BN_cmp(ops[i], ops[j]) == 0 ||
			    (i == 0 && j == 3) || (i == 3 && j == 0)), "fe_eq %zu %zu", i, j);
		}
		BN_mod_sqr(w, ops[i], P, ctx);
		CHECK(fe_is(fe_sqr(a), w), "fe_sqr %zu", i);
		BN_nnmod(w, ops[i], P, ctx);
		CHECK(fe_is_zero(a) == BN_is_zero(w), "fe_is_zero %zu", i);
		if (i < 30) {
			if (BN_is_zero(w))
				CHECK(fe_is_zero(fe_inv(a)), "fe_inv of zero");
			else {
				BN_mod_inverse(w, ops[i], P, ctx);
				CHECK(fe_is(fe_inv(a), w), "fe_inv %zu", i);
			}
		}
	}
	BN_free(w);
	for (BIGNUM *b : ops)
		BN_free(b);
}

static void test_load()
{
	uint8_t buf[72];
	for (int off = 0; off < 4; off++) {
		for (int round = 0; round < 8; round++) {
			BIGNUM *v = BN_new();
			if (round == 0)
				BN_copy(v, P);
			else if (round == 1) {
				BN_copy(v, P);
				BN_sub_word(v, 1);
			} else if (round == 2) {
				BN_zero(v);
				BN_set_bit(v, 527);
			} else if (round == 3) {	/* 2^528 - 1 */
				BN_zero(v);
				BN_set_bit(v, 528);
				BN_sub_word(v, 1);
			} else
				BN_rand_range(v, P);
			memset(buf, 0xa5, sizeof(buf));
			CHECK(BN_bn2binpad(v, buf + off, 66) == 66, "pad");
			bool in;
			const p521_fe f = fe_load_be66(buf + off, &in);
			BIGNUM *g = bn_of(f.l);
			CHECK(BN_cmp(g, v) == 0, "fe_load_be66 off %d round %d", off, round);
			CHECK(in == (BN_cmp(v, P) < 0), "in_field off %d round %d", off, round);
			const p521_sc s = sc_load_be66(buf + off);
			BN_free(g);
			g = bn_of(s.l);
			CHECK(BN_cmp(g, v) == 0, "sc_load_be66 off %d", off);
			BN_free(g);
			BN_free(v);
		}
	}
}

static void test_scalar()
{
	BIGNUM *R = BN_new(), *Rinv = BN_new(), *w = BN_new(), *top = BN_new();
	BN_set_bit(R, 544);
	BN_mod_inverse(Rinv, R, N, ctx);
	BN_copy(top, R);
	BN_sub_word(top, 1);		/* 2^544 - 1: the left operand's limit */
	std::vector<BIGNUM *> ops;
	for (unsigned k : { 0u, 1u, 2u }) {
		BIGNUM *t = BN_new();
		BN_set_word(t, k);
		ops.push_back(t);
		t = BN_dup(N);
		BN_sub_word(t, k + 1);
		ops.push_back(t);
	}
	for (int i = 0; i < 40; i++) {
		BIGNUM *t = BN_new();
		BN_rand_range(t, N);
		ops.push_back(t);
	}
	for (size_t j = 0; j < ops.size(); j++) {
		std::vector<BIGNUM *> left(ops);
		left.push_back(top);
		left.push_back(P);
		for (size_t i = 0; i < left.size(); i++) {
			BN_mod_mul(w, left[i], ops[j], N, ctx);
			BN_mod_mul(w, w, Rinv, N, ctx);
			const p521_sc got = sc_mont_mul(sc_of(left[i]), sc_of(ops[j]));
			BIGNUM *g = bn_of(got.l);
			CHECK(BN_cmp(g, w) == 0, "sc_mont_mul %zu %zu", i, j);
			BN_free(g);
		}
		CHECK(sc_lt(sc_of(ops[j]), sc_n()), "sc_lt below n");
		CHECK(sc_is_zero(sc_of(ops[j])) == BN_is_zero(ops[j]), "sc_is_zero");
	}
	CHECK(!sc_lt(sc_of(N), sc_n()) && !sc_lt(sc_of(P), sc_n()), "sc_lt at n");
	/* u1 = e / s, u2 = r / s, e up to 2^521 - 1 */
	BIGNUM *inv = BN_new();
	for (size_t j = 0; j + 2 < ops.size(); j++) {
		const BIGNUM *s = ops[j], *r = ops[j + 1];
		const BIGNUM *e = j % 5 == 0 ? P : ops[j + 2];
		if (BN_is_zero(s))
			continue;
		p521_sc u1, u2;
		sc_u1_u2(sc_of(r), sc_of(s), sc_of(e), &u1, &u2);
		BN_mod_inverse(inv, s, N, ctx);
		BIGNUM *g = bn_of(u1.l);
		BN_mod_mul(w, e, inv, N, ctx);
		CHECK(BN_cmp(g, w) == 0, "u1 %zu", j);
		BN_free(g);
		g = bn_of(u2.l);
		BN_mod_mul(w, r, inv, N, ctx);
		CHECK(BN_cmp(g, w) == 0, "u2 %zu", j);
		BN_free(g);
	}
	for (BIGNUM *b : ops)
		BN_free(b);
	BN_free(inv);
	BN_free(R);
	BN_free(Rinv);
	BN_free(w);
	BN_free(top);
}

/* ---- points ---------------------------------------------------------------- */

struct Affine {
	BIGNUM *x, *y;
	bool inf;
};

static Affine affine_of(const EC_POINT *pt)
{
	Affine a = { BN_new(), BN_new(), false };
	if (EC_POINT_is_at_infinity(grp, pt))
		a.inf = true;
	else
		CHECK(EC_POINT_get_affine_coordinates(grp, pt, a.x, a.y, ctx) == 1, "affine");
	return a;
}

static void affine_free(Affine &a)
{
	BN_free(a.x);
	BN_free(a.y);
}

/* the running point := pt in Jacobian coordinates with a random Z */
static void set_running(p521_host_regs &m, p521_lane &L, const EC_POINT *pt)
{
	Affine a = affine_of(pt);
	L.inf = a.inf;
	L.fix = false;
	BIGNUM *z = BN_new(), *t = BN_new();
	do
		BN_rand_range(z, P);
	while (BN_is_zero(z));
	if (a.inf) {
		p521_st(m, P521_R_X, fe_of(z));
		p521_st(m, P521_R_Y, fe_of(z));
		p521_st(m, P521_R_Z, fe_zero());
	} else {
		BN_mod_sqr(t, z, P, ctx);
		BN_mod_mul(a.x, a.x, t, P, ctx);
		BN_mod_mul(t, t, z, P, ctx);
		BN_mod_mul(a.y, a.y, t, P, ctx);
		p521_st(m, P521_R_X, fe_of(a.x));
		p521_st(m, P521_R_Y, fe_of(a.y));
		p521_st(m, P521_R_Z, fe_of(z));
	}
	BN_free(z);
	BN_free(t);
	affine_free(a);
}

static void set_key(p521_host_regs &m, const EC_POINT *pt)
{
	Affine a = affine_of(pt);
	CHECK(!a.inf, "key at infinity");
	p521_st(m, P521_R_QX, fe_of(a.x));
	p521_st(m, P521_R_QY, fe_of(a.y));
	affine_free(a);
}

static void expect_running(const p521_host_regs &m, const p521_lane &L,
    const EC_POINT *want, const char *what)
{
	Affine a = affine_of(want);
	const p521_fe z = p521_ld(m, P521_R_Z);
	CHECK(L.inf == fe_is_zero(z), "%s: inf flag and Z disagree", what);
	CHECK(L.inf == a.inf, "%s: infinity %d, want %d", what, L.inf, a.inf);
	CHECK(!L.fix, "%s: fix left set", what);
	if (!a.inf) {
		const p521_fe zi = fe_inv(z), zi2 = fe_sqr(zi);
		CHECK(fe_is(fe_mul(p521_ld(m, P521_R_X), zi2), a.x), "%s: x", what);
		CHECK(fe_is(fe_mul(p521_ld(m, P521_R_Y), fe_mul(zi2, zi)), a.y), "%s: y", what);
	}
	affine_free(a);
}

static p521_sc top_bit(bool set)
{
	p521_sc s;
	memset(&s, 0, sizeof(s));
	s.l[16] = set ? 0x80000000u : 0;
	return s;
}

/* R = 2R (which < 0) or R + T, T = G (0) or Q (1), through the engine */
static void step(p521_host_regs &m, p521_lane &L, int which)
{
	bool a = false, b = false;
	const p521_sc r = top_bit(false);
	ecdsa_p521_engine(m, L, top_bit(which == 0), top_bit(which == 1), r,
	    which < 0 ? ECDSA_ST_DBL : ECDSA_ST_ADD1, 1, false, &a, &b);
}

static void test_points()
{
	p521_host_regs m;
	p521_lane L;
	memset(&m, 0, sizeof(m));
	EC_POINT *p = EC_POINT_new(grp), *q = EC_POINT_new(grp), *w = EC_POINT_new(grp);
	BIGNUM *k = BN_new();
	const EC_POINT *G = EC_GROUP_get0_generator(grp);
	for (int round = 0; round < 24; round++) {
		BN_rand_range(k, N);
		if (round == 0)
			BN_one(k);
		EC_POINT_mul(grp, p, k, nullptr, nullptr, ctx);
		BN_rand_range(k, N);
		if (BN_is_zero(k))
			BN_one(k);
		EC_POINT_mul(grp, q, k, nullptr, nullptr, ctx);
		set_key(m, q);
		/* double */
		set_running(m, L, p);
		step(m, L, -1);
		EC_POINT_dbl(grp, w, p, ctx);
		expect_running(m, L, w, "2P");
		/* P + G, P + Q */
		set_running(m, L, p);
		step(m, L, 0);
		EC_POINT_add(grp, w, p, G, ctx);
		expect_running(m, L, w, "P + G");
		set_running(m, L, p);
		step(m, L, 1);
		EC_POINT_add(grp, w, p, q, ctx);
		expect_running(m, L, w, "P + Q");
		/* Q + Q and G + G: the addition must double */
		set_running(m, L, q);
		step(m, L, 1);
		EC_POINT_dbl(grp, w, q, ctx);
		expect_running(m, L, w, "Q + Q");
		set_running(m, L, G);
		step(m, L, 0);
		EC_POINT_dbl(grp, w, G, ctx);
		expect_running(m, L, w, "G + G");
		/* (-Q) + Q and (-G) + G: infinity */
		EC_POINT_copy(w, q);
		EC_POINT_invert(grp, w, ctx);
		set_running(m, L, w);
		step(m, L, 1);
		EC_POINT_set_to_infinity(grp, w);
		expect_running(m, L, w, "-Q + Q");
		EC_POINT_copy(w, G);
		EC_POINT_invert(grp, w, ctx);
		set_running(m, L, w);
		step(m, L, 0);
		EC_POINT_set_to_infinity(grp, w);
		expect_running(m, L, w, "-G + G");
		/* infinity + Q, infinity + G, 2 infinity */
		set_running(m, L, w);
		step(m, L, 1);
		expect_running(m, L, q, "inf + Q");
		set_running(m, L, w);
		step(m, L, 0);
		expect_running(m, L, G, "inf + G");
		set_running(m, L, w);
		step(m, L, -1);
		expect_running(m, L, w, "2 inf");
	}
	/* the curve check */
	for (int round = 0; round < 8; round++) {
		BN_rand_range(k, N);
		BN_add_word(k, 1);
		EC_POINT_mul(grp, q, k, nullptr, nullptr, ctx);
		set_key(m, q);
		if (round & 1) {	/* off the curve: y + 1 */
			p521_st(m, P521_R_QY, fe_add(p521_ld(m, P521_R_QY), fe_one()));
		}
		bool on = false, b = false;
		ecdsa_p521_engine(m, L, top_bit(false), top_bit(false), top_bit(false),
		    ECDSA_ST_CURVE, 0, false, &on, &b);
		CHECK(on == !(round & 1), "curve check round %d", round);
	}
	EC_POINT_free(p);
	EC_POINT_free(q);
	EC_POINT_free(w);
	BN_free(k);
}

/* X = x Z^2 for a chosen x: does the last comparison say x mod n = r? */
static bool final_says(const BIGNUM *x, const BIGNUM *r, bool inf)
{
	p521_host_regs m;
	memset(&m, 0, sizeof(m));
	p521_lane L = { inf, false };
	BIGNUM *z = BN_new(), *t = BN_new();
	do
		BN_rand_range(z, P);
	while (BN_is_zero(z));
	BN_mod_sqr(t, z, P, ctx);
	BN_mod_mul(t, t, x, P, ctx);
	p521_st(m, P521_R_X, fe_of(t));
	p521_st(m, P521_R_Z, inf ? fe_zero() : fe_of(z));
	bool a = false, match = false;
	ecdsa_p521_engine(m, L, top_bit(false), top_bit(false), sc_of(r),
	    ECDSA_ST_FINAL, 0, true, &a, &match);
	BN_free(z);
	BN_free(t);
	return match;
}

static void test_final()
{
	BIGNUM *r = BN_new(), *x = BN_new(), *pmn = BN_new();
	BN_sub(pmn, P, N);
	for (int round = 0; round < 12; round++) {
		/* r below p - n: both candidates are in the field */
		BN_rand_range(r, pmn);
		if (round == 0 || BN_is_zero(r))
			BN_one(r);
		if (round == 1)
			BN_sub(r, pmn, BN_value_one());
		CHECK(final_says(r, r, false), "x = r");
		CHECK(!final_says(r, r, true), "infinity never matches");
		BN_add(x, r, N);
		CHECK(final_says(x, r, false), "x = r + n");
		BN_add_word(x, 1);
		CHECK(!final_says(x, r, false), "x = r + n + 1");
		BN_sub(x, r, BN_value_one());
		CHECK(!final_says(x, r, false), "x = r - 1");
		/* r from p - n on: r + n is p or more, and x = r + n - p is
		 * another field element whose x mod n is not r */
		BN_rand_range(r, N);
		if (BN_cmp(r, pmn) < 0)
			BN_add(r, r, pmn);
		if (round == 2)
			BN_copy(r, pmn);
		if (round == 3)
			BN_sub(r, N, BN_value_one());
		CHECK(final_says(r, r, false), "x = r, large r");
		BN_add(x, r, N);
		BN_sub(x, x, P);
		CHECK(!final_says(x, r, false), "x = r + n - p");
	}
	BN_free(r);
	BN_free(x);
	BN_free(pmn);
}

static void test_programs()
{
	const int starts[] = { P521_PROG_CURVE, P521_PROG_DBL, P521_PROG_MADD1_G,
		P521_PROG_MADD1_Q, P521_PROG_MADD2, P521_PROG_FINAL };
	const int count = (int)(sizeof(p521_progs) / sizeof(p521_progs[0]));
	int ends = 0;
	for (int s : starts) {
		CHECK(s < count, "program start %d out of the table", s);
		CHECK(s == 0 || p521_progs[s - 1].op == P521_OP_END,
		    "program start %d does not follow an end", s);
		CHECK(p521_progs[s].op != P521_OP_END, "empty program at %d", s);
	}
	for (int i = 0; i < count; i++) {
		ends += p521_progs[i].op == P521_OP_END;
		CHECK(p521_progs[i].d < P521_REGS, "op %d stores to a constant", i);
		CHECK(p521_progs[i].a <= P521_R_CB && p521_progs[i].b <= P521_R_CB,
		    "op %d reads past the constants", i);
	}
	CHECK(ends == 6 && p521_progs[count - 1].op == P521_OP_END, "six programs");
}

/* ---- verify_one against ECDSA_do_verify over the vectors ------------------ */

struct Vec {
	uint8_t pub[132], rs[132];
	uint32_t dlen;
	uint8_t dig[128];
	uint8_t want, pad[3];
};
static_assert(sizeof(Vec) == 400, "the record of tests/test_ecdsa_host.py");

static int openssl_says(const Vec &v)
{
	EC_KEY *key = EC_KEY_new_by_curve_name(NID_secp521r1);
	BIGNUM *x = BN_bin2bn(v.pub, 66, nullptr), *y = BN_bin2bn(v.pub + 66, 66, nullptr);
	int rc = 0;
	if (EC_KEY_set_public_key_affine_coordinates(key, x, y) == 1) {
		ECDSA_SIG *sig = ECDSA_SIG_new();
		ECDSA_SIG_set0(sig, BN_bin2bn(v.rs, 66, nullptr),
		    BN_bin2bn(v.rs + 66, 66, nullptr));
		rc = ECDSA_do_verify(v.dig, (int)v.dlen, sig, key) == 1;
		ECDSA_SIG_free(sig);
	}
	BN_free(x);
	BN_free(y);
	EC_KEY_free(key);
	return rc;
}

static int test_vectors(const char *path)
{
	FILE *f = fopen(path, "rb");
	CHECK(f != nullptr, "cannot open %s", path);
	Vec v;
	int n = 0, valid = 0;
	p521_host_regs m;
	memset(&m, 0, sizeof(m));
	while (fread(&v, sizeof(v), 1, f) == 1) {
		CHECK(v.dlen <= sizeof(v.dig), "record %d: digest length", n);
		/* exact-size heap copies at odd offsets, so a read past an end
		 * is ASan's to see */
		uint8_t *pub = (uint8_t *)malloc(132 + 1), *rs = (uint8_t *)malloc(132 + 3);
		uint8_t *dig = (uint8_t *)malloc(v.dlen + 1);
		memcpy(pub + 1, v.pub, 132);
		memcpy(rs + 3, v.rs, 132);
		memcpy(dig + 1, v.dig, v.dlen);
		const int got = ecdsa_p521_verify_one(m, pub + 1, rs + 3, dig + 1, v.dlen);
		const int want = openssl_says(v);
		CHECK(want == v.want, "record %d: OpenSSL says %d here, %d there", n, want, v.want);
		CHECK(got == want, "record %d: verify_one %d, OpenSSL %d", n, got, want);
		free(pub);
		free(rs);
		free(dig);
		valid += want;
		n++;
	}
	fclose(f);
	printf("test_ecdsa_host: %d vectors, %d valid\n", n, valid);
	return n;
}

int main(int argc, char **argv)
{
	ctx = BN_CTX_new();
	grp = EC_GROUP_new_by_curve_name(NID_secp521r1);
	P = BN_new();
	N = BN_new();
	BIGNUM *a = BN_new(), *b = BN_new();
	CHECK(EC_GROUP_get_curve(grp, P, a, b, ctx) == 1, "curve");
	CHECK(EC_GROUP_get_order(grp, N, ctx) == 1, "order");
	{	/* the constants of the headers are the group's */
		constexpr uint32_t cb[17] = P521_B_INIT;
		BIGNUM *g = bn_of(cb);
		CHECK(BN_cmp(g, b) == 0, "P521_B_INIT");
		BN_free(g);
		g = bn_of(sc_n().l);
		CHECK(BN_cmp(g, N) == 0, "P521_N_INIT");
		BN_free(g);
	}
	test_programs();
	test_load();
	test_field();
	test_scalar();
	test_points();
	test_final();
	if (argc > 1)
		CHECK(test_vectors(argv[1]) > 0, "no vectors");
	BN_free(a);
	BN_free(b);
	BN_free(P);
	BN_free(N);
	EC_GROUP_free(grp);
	BN_CTX_free(ctx);
	printf("test_ecdsa_host: ok\n");
	return 0;
}
