/*
 * test_ecdsa_key_host.cc -- the prepared-key arithmetic of the ECDSA P-521
 * verification (ilias_net2_amd/csrc/p521_keytab.h) on the host, against
 * libcrypto: the code the lanes of ecdsa_key_kernels.hip run, with a plain
 * array as the register file.
 *
 *  - p521_keytab_build_one, window by window, for G and for the keys
 *    d = 1, 2, n - 1 and a random one: every entry (j, d) against
 *    EC_POINT_mul in canonical limbs, the heads, G's table = the table of
 *    d = 1;
 *  - keys a verification refuses (x = p, y = p, y's last bit flipped, (0, 0))
 *    come out valid = 0 and write inside their table only;
 *  - ecdsa_p521_keytab_verify_one over the vectors tests/test_ecdsa_key_host.py
 *    writes, each verdict against ECDSA_do_verify.  A vector's key table is
 *    laid out here from OpenSSL's own points (the builder was just held to
 *    those, entry by entry), G's is the one built above;
 *  - a key index out of range and heads that do not say "prepared".
 *
 * Built by tests/test_ecdsa_key_host.py under AddressSanitizer and UBSan and
 * run as a child process; tables are exact-size heap blocks, so a store or a
 * gather past an end is ASan's to see.
 */
#include "p521_keytab.h"

#include <openssl/bn.h>
#include <openssl/ec.h>
#include <openssl/ecdsa.h>
#include <openssl/obj_mac.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

static BN_CTX *ctx;
static BIGNUM *P, *N;
static EC_GROUP *grp;

#define CHECK(c, ...)                                                       \
	do {                                                                \
		if (!(c)) {                                                 \
			fprintf(stderr, "test_ecdsa_key_host: line %d: ", __LINE__); \
			fprintf(stderr, __VA_ARGS__);                       \
			fprintf(stderr, "\n");                              \
			exit(1);                                            \
		}                                                           \
	} while (0)

static_assert(P521_KT_TABLE_WORDS * 4 == 267256, "the table of net2/ecdsa_key.h");
static_assert(P521_KT_ENTRY_WORDS * 4 == 136, "the entry of net2/ecdsa_key.h");

/* x, y of a finite point as canonical limbs */
static void limbs_of_point(const EC_POINT *pt, uint32_t *xy)
{
	BIGNUM *x = BN_new(), *y = BN_new();
	uint8_t b[68];
	CHECK(EC_POINT_get_affine_coordinates(grp, pt, x, y, ctx) == 1, "affine");
	for (int c = 0; c < 2; c++) {
		CHECK(BN_bn2binpad(c ? y : x, b, 68) == 68, "coordinate too long");
		for (int i = 0; i < 17; i++)
			xy[c * 17 + i] = (uint32_t)b[67 - 4 * i] | (uint32_t)b[66 - 4 * i] << 8 |
			    (uint32_t)b[65 - 4 * i] << 16 | (uint32_t)b[64 - 4 * i] << 24;
	}
	BN_free(x);
	BN_free(y);
}

static void pub_of_point(const EC_POINT *pt, uint8_t pub[132])
{
	BIGNUM *x = BN_new(), *y = BN_new();
	CHECK(EC_POINT_get_affine_coordinates(grp, pt, x, y, ctx) == 1, "affine");
	CHECK(BN_bn2binpad(x, pub, 66) == 66 && BN_bn2binpad(y, pub + 66, 66) == 66, "pad");
	BN_free(x);
	BN_free(y);
}

/* An exact-size heap table, built window by window by the code under test. */
static uint32_t *build_table(const uint8_t *pub, bool *valid, int step = 1)
{
	uint32_t *t = (uint32_t *)calloc(P521_KT_TABLE_WORDS, 4);
	uint8_t *key = nullptr;
	if (pub != nullptr) {		/* at an odd address */
		key = (uint8_t *)malloc(133);
		memcpy(key + 1, pub, 132);
	}
	p521_host_regs m;
	memset(&m, 0, sizeof(m));
	bool all = true, any = false;
	for (int j = 0; j < P521_KT_WINDOWS; j += step) {
		const bool v = p521_keytab_build_one(m, key ? key + 1 : nullptr, j, t, true);
		all = all && v;
		any = any || v;
	}
	CHECK(all == any, "windows disagree about the key");
	*valid = all;
	free(key);
	return t;
}

/* Every entry of a built table against EC_POINT_mul. */
static void check_table(const uint32_t *t, const EC_POINT *q, const char *what)
{
	CHECK(t[0] == P521_KT_MAGIC && t[1] == 1 && t[2] == 0 && t[3] == 0, "%s: head", what);
	BIGNUM *k = BN_new(), *w = BN_new();
	EC_POINT *r = EC_POINT_new(grp);
	uint32_t want[34];
	BN_one(w);
	for (int j = 0; j < P521_KT_WINDOWS; j++) {
		for (int d = 1; d <= P521_KT_DIGITS; d++) {
			BN_copy(k, w);
			BN_mul_word(k, (BN_ULONG)d);
			CHECK(EC_POINT_mul(grp, r, nullptr, q, k, ctx) == 1, "mul");
			limbs_of_point(r, want);
			const uint32_t *e = t + P521_KT_HEAD_WORDS +
			    (j * P521_KT_DIGITS + d - 1) * P521_KT_ENTRY_WORDS;
			CHECK(memcmp(e, want, sizeof(want)) == 0, "%s: entry (%d, %d)", what, j, d);
		}
		BN_lshift(w, w, 4);
	}
	EC_POINT_free(r);
	BN_free(k);
	BN_free(w);
}

/* The same table from OpenSSL's points alone: doublings and additions. */
static uint32_t *openssl_table(const uint8_t pub[132])
{
	uint32_t *t = (uint32_t *)calloc(P521_KT_TABLE_WORDS, 4);
	BIGNUM *x = BN_bin2bn(pub, 66, nullptr), *y = BN_bin2bn(pub + 66, 66, nullptr);
	EC_POINT *p = EC_POINT_new(grp), *r = EC_POINT_new(grp);
	t[0] = P521_KT_MAGIC;
	if (BN_cmp(x, P) < 0 && BN_cmp(y, P) < 0 &&
	    EC_POINT_set_affine_coordinates(grp, p, x, y, ctx) == 1) {
		t[1] = 1;
		for (int j = 0; j < P521_KT_WINDOWS; j++) {
			EC_POINT_copy(r, p);
			for (int d = 1; d <= P521_KT_DIGITS; d++) {
				limbs_of_point(r, t + P521_KT_HEAD_WORDS +
				    (j * P521_KT_DIGITS + d - 1) * P521_KT_ENTRY_WORDS);
				CHECK(EC_POINT_add(grp, r, r, p, ctx) == 1, "add");
			}
			EC_POINT_copy(p, r);	/* 16 P */
		}
	}
	EC_POINT_free(p);
	EC_POINT_free(r);
	BN_free(x);
	BN_free(y);
	return t;
}

static uint32_t *g_table;

static void test_tables()
{
	bool valid = false;
	g_table = build_table(nullptr, &valid);
	CHECK(valid, "G refused");
	check_table(g_table, EC_GROUP_get0_generator(grp), "G");
	BIGNUM *d = BN_new();
	EC_POINT *q = EC_POINT_new(grp);
	for (int which = 0; which < 4; which++) {
		if (which == 0)
			BN_one(d);
		else if (which == 1)
			BN_set_word(d, 2);
		else if (which == 2) {
			BN_copy(d, N);
			BN_sub_word(d, 1);
		} else {
			CHECK(BN_hex2bn(&d, "13b9f5c2a7e6d84091a5c3e7f2b8d6a4c1e9f7053b2d8c6a4e1f9b7d5c3a1e8f6"
			    "b4d2c0a9e7f5d3b1c8a6e4f2d0b9c7a5e3f1d8b6c4a2e0f9d7b5c3a1") != 0, "hex");
		}
		CHECK(EC_POINT_mul(grp, q, d, nullptr, nullptr, ctx) == 1, "key");
		uint8_t pub[132];
		pub_of_point(q, pub);
		uint32_t *t = build_table(pub, &valid);
		char what[32];
		snprintf(what, sizeof(what), "key %d", which);
		CHECK(valid, "%s refused", what);
		check_table(t, q, what);
		if (which == 0)
			CHECK(memcmp(t, g_table, P521_KT_TABLE_WORDS * 4) == 0, "d = 1 is not G's table");
		uint32_t *o = openssl_table(pub);
		CHECK(memcmp(t, o, P521_KT_TABLE_WORDS * 4) == 0, "%s: OpenSSL's chain differs", what);
		free(o);
		free(t);
	}
	/* refused keys: the first and the last window, which is where a store
	 * past the table would go */
	uint8_t good[132], bad[4][132];
	pub_of_point(q, good);
	for (int i = 0; i < 4; i++)
		memcpy(bad[i], good, 132);
	CHECK(BN_bn2binpad(P, bad[0], 66) == 66, "pad");		/* x = p */
	CHECK(BN_bn2binpad(P, bad[1] + 66, 66) == 66, "pad");	/* y = p */
	bad[2][131] ^= 1;					/* off the curve */
	memset(bad[3], 0, 132);					/* (0, 0) */
	for (int i = 0; i < 4; i++) {
		uint32_t *t = build_table(bad[i], &valid, P521_KT_WINDOWS - 1);
		CHECK(!valid, "refused key %d accepted", i);
		CHECK(t[0] == P521_KT_MAGIC && t[1] == 0 && t[2] == 0 && t[3] == 0,
		    "refused key %d: head", i);
		free(t);
	}
	EC_POINT_free(q);
	BN_free(d);
}

/* ---- verify_one from tables against ECDSA_do_verify over the vectors -------- */

struct Vec {
	uint8_t pub[132], rs[132];
	uint32_t dlen;
	uint8_t dig[128];
	uint8_t want, pad[3];
};
static_assert(sizeof(Vec) == 400, "the record of tests/test_ecdsa_key_host.py");

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
	/* one keytab of two tables per distinct key: G's, the key's */
	std::map<std::string, uint32_t *> tabs;
	while (fread(&v, sizeof(v), 1, f) == 1) {
		CHECK(v.dlen <= sizeof(v.dig), "record %d: digest length", n);
		const std::string id((const char *)v.pub, 132);
		uint32_t *&kt = tabs[id];
		if (kt == nullptr) {
			kt = (uint32_t *)malloc(2 * P521_KT_TABLE_WORDS * 4);
			uint32_t *t = openssl_table(v.pub);
			memcpy(kt, g_table, P521_KT_TABLE_WORDS * 4);
			memcpy(kt + P521_KT_TABLE_WORDS, t, P521_KT_TABLE_WORDS * 4);
			free(t);
		}
		uint8_t *rs = (uint8_t *)malloc(132 + 3), *dig = (uint8_t *)malloc(v.dlen + 1);
		memcpy(rs + 3, v.rs, 132);
		memcpy(dig + 1, v.dig, v.dlen);
		const int got = ecdsa_p521_keytab_verify_one(m, kt, 1, 0, rs + 3, dig + 1, v.dlen);
		const int want = openssl_says(v);
		CHECK(want == v.want, "record %d: OpenSSL says %d here, %d there", n, want, v.want);
		CHECK(got == want, "record %d: keytab_verify_one %d, OpenSSL %d", n, got, want);
		if (want && valid < 8) {
			/* an index out of range; heads that do not say "prepared" */
			CHECK(ecdsa_p521_keytab_verify_one(m, kt, 1, 1, rs + 3, dig + 1, v.dlen) == 0,
			    "record %d: key 1 of 1", n);
			CHECK(ecdsa_p521_keytab_verify_one(m, kt, 1, 0xffffffffu, rs + 3, dig + 1,
			    v.dlen) == 0, "record %d: key 2^32 - 1", n);
			for (int h = 0; h < 4; h++) {
				uint32_t *w = kt + (h >> 1) * P521_KT_TABLE_WORDS + (h & 1);
				const uint32_t keep = *w;
				*w = (h & 1) ? 0 : keep ^ 1;
				CHECK(ecdsa_p521_keytab_verify_one(m, kt, 1, 0, rs + 3, dig + 1,
				    v.dlen) == 0, "record %d: head word %d", n, h);
				*w = keep;
			}
			CHECK(ecdsa_p521_keytab_verify_one(m, kt, 1, 0, rs + 3, dig + 1, v.dlen) == 1,
			    "record %d: restored", n);
		}
		free(rs);
		free(dig);
		valid += want;
		n++;
	}
	fclose(f);
	for (auto &kv : tabs)
		free(kv.second);
	printf("test_ecdsa_key_host: %d vectors, %d valid, %zu keys\n", n, valid, tabs.size());
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
	{	/* the new programs: starts follow ends, no store to a constant */
		const int starts[] = { P521_PROG_INV_STEP, P521_PROG_INV_TAIL, P521_PROG_TOAFF,
			P521_PROG_INV_BACK, P521_PROG_NORM };
		const int count = (int)(sizeof(p521_kt_progs) / sizeof(p521_kt_progs[0]));
		int ends = 0;
		for (int s : starts) {
			const int at = s - P521_KT_PROG;
			CHECK(at >= 0 && at < count, "program start %d out of the table", s);
			CHECK(at == 0 || p521_kt_progs[at - 1].op == P521_OP_END,
			    "program start %d does not follow an end", s);
			CHECK(p521_kt_progs[at].op != P521_OP_END, "empty program at %d", s);
		}
		for (int i = 0; i < count; i++) {
			ends += p521_kt_progs[i].op == P521_OP_END;
			CHECK(p521_kt_progs[i].d < P521_REGS, "op %d stores to a constant", i);
			CHECK(p521_kt_progs[i].a <= P521_R_CB && p521_kt_progs[i].b <= P521_R_CB,
			    "op %d reads past the constants", i);
		}
		CHECK(ends == 5 && p521_kt_progs[count - 1].op == P521_OP_END, "five programs");
		CHECK((int)(sizeof(p521_progs) / sizeof(p521_progs[0])) < P521_KT_PROG,
		    "the two tables' program numbers overlap");
	}
	test_tables();
	if (argc > 1)
		CHECK(test_vectors(argv[1]) > 0, "no vectors");
	free(g_table);
	BN_free(a);
	BN_free(b);
	BN_free(P);
	BN_free(N);
	EC_GROUP_free(grp);
	BN_CTX_free(ctx);
	printf("test_ecdsa_key_host: ok\n");
	return 0;
}
