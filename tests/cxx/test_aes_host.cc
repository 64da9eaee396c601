/*
 * test_aes_host.cc -- host check of the burst cipher's block code and key
 * schedules: aes_device.h (the T-table rounds, the last round's S-box
 * recovery, the PKCS#7 check) under the schedules of aes_sched.h, with a
 * plain 256-word array as the table and a plain schedule as the round keys,
 * against libcrypto's EVP and against restatements of FIPS 197 written here.
 * No GPU: this is the arithmetic the kernels of aes_kernels.hip run.  Then
 * the lane kernels' own per-datagram code (aes_cbc.h: the prep steps,
 * cbc_decrypt_lane, cbc_encrypt_lane) over bursts of one datagram in
 * exact-size heap buffers, bit for bit against EVP and the documented codes:
 * every block count up to the rotation's third, in place and out of place,
 * at each payload offset, and what the prep steps settle on their own.
 *
 * Exits non-zero with a message on the first mismatch.
 *   clang++ -std=c++17 -Iilias_net2_amd/csrc tests/cxx/test_aes_host.cc -lcrypto
 */
#include "aes_cbc.h"
#include "aes_device.h"
#include "aes_sched.h"

#include <openssl/evp.h>

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>
#include <vector>

namespace {

[[noreturn]] void fail(const char *fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	fprintf(stderr, "test_aes_host: FAIL: ");
	vfprintf(stderr, fmt, ap);
	fprintf(stderr, "\n");
	va_end(ap);
	exit(1);
}

const char *hex(const uint8_t *p, size_t n)
{
	static char buf[4][2 * 64 + 1];
	static int at;
	char *b = buf[at++ & 3];
	for (size_t i = 0; i < n && i < 64; i++)
		snprintf(b + 2 * i, 3, "%02x", p[i]);
	return b;
}

/* splitmix64: a fixed stream, the same on every run */
uint64_t rng_state = 0x5eed0a35c0ffee01ull;
uint64_t rnd64()
{
	uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
	z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
	z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
	return z ^ (z >> 31);
}
void rnd_bytes(uint8_t *p, size_t n)
{
	for (size_t i = 0; i < n; i++)
		p[i] = (uint8_t)(rnd64() >> 56);
}

/* ---- restatements written here ------------------------------------------- */

/* GF(2^8) multiply mod x^8 + x^4 + x^3 + x + 1, shift and reduce */
uint8_t gmul(uint8_t a, uint8_t b)
{
	unsigned r = 0, aa = a;
	for (int i = 0; i < 8; i++) {
		if (b & (1u << i))
			r ^= aa;
		aa <<= 1;
		if (aa & 0x100)
			aa ^= 0x11b;
	}
	return (uint8_t)r;
}

/* FIPS 197 5.1.1: the multiplicative inverse, then the affine map */
uint8_t sbox_by_definition(uint8_t x)
{
	uint8_t inv = 0;
	for (unsigned y = 1; y < 256 && x != 0; y++)
		if (gmul(x, (uint8_t)y) == 1) {
			inv = (uint8_t)y;
			break;
		}
	uint8_t r = 0x63;
	for (int s = 0; s < 5; s++)
		r ^= (uint8_t)((inv << s) | (inv >> (8 - s)));
	return r;
}

/* FIPS 197 5.2 KeyExpansion, Nk = 8, Nr = 14 */
void expand_by_definition(const uint8_t S[256], const uint8_t key[32],
    uint32_t w[60])
{
	auto subw = [&](uint32_t x) {
		return (uint32_t)S[x >> 24] << 24 | (uint32_t)S[(x >> 16) & 255] << 16 |
		    (uint32_t)S[(x >> 8) & 255] << 8 | (uint32_t)S[x & 255];
	};
	uint8_t rc = 1;
	for (int i = 0; i < 8; i++)
		w[i] = (uint32_t)key[4 * i] << 24 | (uint32_t)key[4 * i + 1] << 16 |
		    (uint32_t)key[4 * i + 2] << 8 | (uint32_t)key[4 * i + 3];
	for (int i = 8; i < 60; i++) {
		uint32_t t = w[i - 1];
		if (i % 8 == 0) {
			t = subw((t << 8) | (t >> 24)) ^ ((uint32_t)rc << 24);
			rc = gmul(rc, 2);
		} else if (i % 8 == 4) {
			t = subw(t);
		}
		w[i] = w[i - 8] ^ t;
	}
}

/* EVP's PKCS#7 check, bytewise: the pad length, 0 when it is wrong */
uint32_t pad_by_definition(const uint8_t b[16])
{
	const uint32_t v = b[15];
	if (v < 1 || v > 16)
		return 0;
	for (uint32_t k = 0; k < v; k++)
		if (b[15 - k] != v)
			return 0;
	return v;
}

/* ---- libcrypto ------------------------------------------------------------- */

/* one EVP run; returns the output length, -1 where EVP fails */
int evp_run(const EVP_CIPHER *ciph, bool enc, const uint8_t *key,
    const uint8_t *iv, bool pad, const uint8_t *in, size_t n, uint8_t *out)
{
	EVP_CIPHER_CTX *ctx = EVP_CIPHER_CTX_new();
	if (ctx == nullptr)
		fail("EVP_CIPHER_CTX_new");
	int n1 = 0, n2 = 0, rc = -1;
	if (EVP_CipherInit_ex(ctx, ciph, nullptr, key, iv, enc ? 1 : 0) == 1) {
		EVP_CIPHER_CTX_set_padding(ctx, pad ? 1 : 0);
		if (EVP_CipherUpdate(ctx, out, &n1, in, (int)n) == 1 &&
		    EVP_CipherFinal_ex(ctx, out + n1, &n2) == 1)
			rc = n1 + n2;
	}
	EVP_CIPHER_CTX_free(ctx);
	return rc;
}

/* ---- the code under test, with plain arrays plugged in -------------------- */

struct Tab {
	const uint32_t *t;
	uint32_t operator()(uint32_t x) const { return t[x]; }
};
struct Rk {
	const uint32_t *w;
	uint32_t operator()(int i) const { return w[i]; }
};

uint32_t Te0[256], Td0[256];
uint8_t S[256], Si[256];

void to_words(const uint8_t *p, uint32_t (&w)[4])
{
	for (int k = 0; k < 4; k++)
		w[k] = (uint32_t)p[4 * k] << 24 | (uint32_t)p[4 * k + 1] << 16 |
		    (uint32_t)p[4 * k + 2] << 8 | (uint32_t)p[4 * k + 3];
}
void to_bytes(const uint32_t (&w)[4], uint8_t *p)
{
	for (int k = 0; k < 16; k++)
		p[k] = (uint8_t)(w[k / 4] >> (24 - 8 * (k % 4)));
}

void block_enc(const AesSched &ks, const uint8_t *in, uint8_t *out)
{
	uint32_t s[4];
	to_words(in, s);
	aes_block<false>(Tab{ Te0 }, Rk{ ks.w }, s);
	to_bytes(s, out);
}
void block_dec(const AesSched &ks, const uint8_t *in, uint8_t *out)
{
	uint32_t s[4];
	to_words(in, s);
	aes_block<true>(Tab{ Td0 }, Rk{ ks.w }, s);
	to_bytes(s, out);
}

/* ---- the checks ------------------------------------------------------------ */

void check_tables()
{
	const Sbox fwd = make_sbox(false), inv = make_sbox(true);
	for (int x = 0; x < 256; x++) {
		S[x] = fwd.v[x];
		Si[x] = inv.v[x];
	}
	for (int x = 0; x < 256; x++) {
		if (S[x] != sbox_by_definition((uint8_t)x))
			fail("S[%02x] = %02x, FIPS 197 5.1.1 gives %02x", x, S[x],
			    sbox_by_definition((uint8_t)x));
		if (Si[S[x]] != x)
			fail("Si[S[%02x]] = %02x", x, Si[S[x]]);
		if (h_sbox.v[x] != S[x])
			fail("h_sbox[%02x]", x);
		Te0[x] = aes_te0_word(S[x]);
		Td0[x] = aes_td0_word(Si[x]);
		const uint8_t s = S[x], i = Si[x];
		const uint32_t te = (uint32_t)gmul(s, 2) << 24 | (uint32_t)s << 16 |
		    (uint32_t)s << 8 | gmul(s, 3);
		const uint32_t td = (uint32_t)gmul(i, 0x0e) << 24 |
		    (uint32_t)gmul(i, 0x09) << 16 | (uint32_t)gmul(i, 0x0d) << 8 |
		    gmul(i, 0x0b);
		if (Te0[x] != te)
			fail("Te0[%02x] = %08x, want %08x", x, Te0[x], te);
		if (Td0[x] != td)
			fail("Td0[%02x] = %08x, want %08x", x, Td0[x], td);
		if (aes_sub_fwd(Te0[x]) != S[x])
			fail("aes_sub_fwd(Te0[%02x]) = %02x, want %02x", x,
			    aes_sub_fwd(Te0[x]), S[x]);
		if (aes_sub_inv(Td0[x]) != Si[x])
			fail("aes_sub_inv(Td0[%02x]) = %02x, want %02x", x,
			    aes_sub_inv(Td0[x]), Si[x]);
		if (aes_xtime((uint32_t)x) != gmul((uint8_t)x, 2))
			fail("aes_xtime(%02x)", x);
	}
}

void unhex(const char *h, uint8_t *out, size_t n)
{
	for (size_t i = 0; i < n; i++) {
		unsigned v;
		if (sscanf(h + 2 * i, "%2x", &v) != 1)
			fail("bad hex %s", h);
		out[i] = (uint8_t)v;
	}
}

/* FIPS 197 C.3, and the key of SP 800-38A F.2.5 */
const char *const C3_KEY =
    "000102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f";
const char *const F25_KEY =
    "603deb1015ca71be2b73aef0857d77811f352c073b6108d72d9810a30914dff4";

void check_known_answer()
{
	uint8_t key[32], pt[16], ct[16], got[16];
	unhex(C3_KEY, key, 32);
	unhex("00112233445566778899aabbccddeeff", pt, 16);
	unhex("8ea2b7ca516745bfeafc49904b496089", ct, 16);
	AesSched e, d;
	aes256_enc_schedule(key, &e);
	aes256_dec_schedule(key, &d);
	block_enc(e, pt, got);
	if (memcmp(got, ct, 16) != 0)
		fail("FIPS 197 C.3 forward: %s, want %s", hex(got, 16), hex(ct, 16));
	block_dec(d, ct, got);
	if (memcmp(got, pt, 16) != 0)
		fail("FIPS 197 C.3 inverse: %s, want %s", hex(got, 16), hex(pt, 16));
}

void check_schedule()
{
	const char *const keys[2] = { C3_KEY, F25_KEY };
	/* the last word of both expansions as FIPS 197 prints it (C.3
	 * round[14].k_sch, A.3 w59): the restatement here is itself held to
	 * the standard */
	const uint32_t w59[2] = { 0x6d68de36u, 0x706c631eu };
	for (int t = 0; t < 2; t++) {
		uint8_t key[32];
		uint32_t want[60];
		AesSched e;
		unhex(keys[t], key, 32);
		expand_by_definition(S, key, want);
		if (want[59] != w59[t])
			fail("expansion written here: key %d w[59] = %08x, FIPS 197 "
			    "prints %08x", t, want[59], w59[t]);
		aes256_enc_schedule(key, &e);
		for (int i = 0; i < 60; i++)
			if (e.w[i] != want[i])
				fail("aes256_enc_schedule key %d: w[%d] = %08x, want %08x",
				    t, i, e.w[i], want[i]);
	}
}

/* blocks through aes_block<false> / <true> against EVP_aes_256_ecb */
void ecb_against_evp(const uint8_t key[32], const uint8_t *blocks, size_t nblk)
{
	std::vector<uint8_t> ct(16 * nblk + 16), got(16);
	AesSched e, d;
	aes256_enc_schedule(key, &e);
	aes256_dec_schedule(key, &d);
	const int n = evp_run(EVP_aes_256_ecb(), true, key, nullptr, false, blocks,
	    16 * nblk, ct.data());
	if (n != (int)(16 * nblk))
		fail("EVP ecb: %d bytes", n);
	for (size_t b = 0; b < nblk; b++) {
		block_enc(e, blocks + 16 * b, got.data());
		if (memcmp(got.data(), &ct[16 * b], 16) != 0)
			fail("aes_block<false> key %s block %s: %s, EVP %s", hex(key, 32),
			    hex(blocks + 16 * b, 16), hex(got.data(), 16),
			    hex(&ct[16 * b], 16));
		block_dec(d, &ct[16 * b], got.data());
		if (memcmp(got.data(), blocks + 16 * b, 16) != 0)
			fail("aes_block<true> key %s block %s: %s, EVP %s", hex(key, 32),
			    hex(&ct[16 * b], 16), hex(got.data(), 16),
			    hex(blocks + 16 * b, 16));
	}
}

void check_block_cipher()
{
	uint8_t key[32], blocks[18 * 16];
	for (int k = 0; k < 4096; k++) {
		rnd_bytes(key, 32);
		rnd_bytes(blocks, 16 * 16);
		memset(blocks + 16 * 16, 0x00, 16);
		memset(blocks + 17 * 16, 0xff, 16);
		ecb_against_evp(key, blocks, 18);
	}
	/* every byte position takes every value */
	std::vector<uint8_t> all(256 * 16);
	for (int j = 0; j < 256; j++)
		for (int p = 0; p < 16; p++)
			all[16 * j + p] = (uint8_t)(j + 16 * p + (p >> 3));
	rnd_bytes(key, 32);
	ecb_against_evp(key, all.data(), 256);
}

/* one block through aes_pkcs7_pad, the restatement and, where asked, EVP */
void pad_one(const uint8_t b[16], bool evp, const uint8_t key[32],
    const uint8_t iv[16])
{
	uint32_t w[4];
	to_words(b, w);
	const uint32_t got = aes_pkcs7_pad(w), want = pad_by_definition(b);
	if (got != want)
		fail("aes_pkcs7_pad(%s) = %u, want %u", hex(b, 16), got, want);
	if (!evp)
		return;
	/* the one-block ciphertext that decrypts to b */
	uint8_t ct[32], out[48];
	if (evp_run(EVP_aes_256_cbc(), true, key, iv, false, b, 16, ct) != 16)
		fail("EVP cbc encrypt");
	const int n = evp_run(EVP_aes_256_cbc(), false, key, iv, true, ct, 16, out);
	if ((n < 0) != (got == 0) || (n >= 0 && n != 16 - (int)got))
		fail("aes_pkcs7_pad(%s) = %u, EVP_DecryptFinal_ex leaves %d bytes",
		    hex(b, 16), got, n);
}

void check_pad()
{
	uint8_t key[32], iv[16], b[16];
	rnd_bytes(key, 32);
	rnd_bytes(iv, 16);
	for (int v = 0; v < 256; v++) {
		const uint8_t other = (uint8_t)(v ^ 0xa5);
		const bool evp = v <= 17;
		/* the last m bytes are v, the ones before are not */
		for (int m = 0; m <= 16; m++) {
			memset(b, other, 16);
			memset(b + 16 - m, v, m);
			pad_one(b, evp, key, iv);
		}
		/* all v but one byte, at each position; and a byte off by one bit */
		for (int q = 0; q < 16; q++) {
			memset(b, v, 16);
			b[q] = other;
			pad_one(b, evp, key, iv);
			b[q] = (uint8_t)(v ^ 1);
			pad_one(b, evp, key, iv);
		}
	}
}

/*
 * One datagram through the lane code of aes_cbc.h, as a burst of one: the
 * datagram sits at the odd offset LEAD of a heap buffer that ends with its
 * last byte, every per-datagram array is a heap array of one element, so
 * AddressSanitizer reports any byte touched outside them.  Bytes that must
 * stay as they are hold a sentinel.
 */
constexpr size_t LEAD = 3;
constexpr uint8_t SENTINEL = 0xc3;
constexpr uint32_t UNSET = 0xdeadbeefu;

struct One {
	std::vector<uint64_t> off;
	std::vector<uint32_t> len, fl, seq, plen, wire;
	std::vector<uint8_t> iv, res;
	AesBurstArgs a;

	One(uint32_t length, uint32_t flags, uint32_t hashlen, const uint8_t *ivp,
	    uint8_t code, uint32_t pl) :
	    off(1, LEAD), len(1, length), fl(1, flags), seq(1, 0), plen(1, pl),
	    wire(1, UNSET), iv(ivp, ivp + 16), res(1, code), a()
	{
		a.offsets = off.data();
		a.lens = len.data();
		a.seq = seq.data();
		a.flags = fl.data();
		a.iv = iv.data();
		a.result = res.data();
		a.plen = plen.data();
		a.wire_len = wire.data();
		a.n = 1;
		a.hashlen = hashlen;
	}
};

/* LEAD sentinel bytes, then the datagram */
std::vector<uint8_t> burst_of(const uint8_t *dg, size_t len)
{
	std::vector<uint8_t> b(LEAD + len, SENTINEL);
	if (len != 0)
		memcpy(b.data() + LEAD, dg, len);
	return b;
}

struct Done {
	uint8_t code;
	uint32_t plen, wire;
	uint32_t nb;			/* what the prep step counted */
	std::vector<uint8_t> bytes;	/* the output burst, LEAD included */
};

/* RX: decrypt_prep + cbc_decrypt_lane; out of place into a burst of sentinel
 * bytes, or in place */
Done rx(const AesSched &d, const uint8_t *iv, uint32_t flags, uint32_t hashlen,
    const uint8_t *dg, uint32_t len, bool in_place, uint8_t code = PKT_OK)
{
	One o(len, flags, hashlen, iv, code, UNSET);
	std::vector<uint8_t> in = burst_of(dg, len);
	std::vector<uint8_t> out(in_place ? 0 : LEAD + len, SENTINEL);
	o.a.in = in.data();
	o.a.out = in_place ? in.data() : out.data();
	const uint32_t nb = decrypt_prep(o.a, 0);
	if (nb != 0)
		cbc_decrypt_lane(o.a, 0, nb, flags, Tab{ Td0 }, Rk{ d.w });
	if (o.wire[0] != UNSET)
		fail("RX wrote wire_len");
	return Done{ o.res[0], o.plen[0], 0, nb, in_place ? in : out };
}

/* TX: encrypt_prep + cbc_encrypt_lane over the slot, in place */
Done tx(const AesSched &e, const uint8_t *iv, uint32_t flags, uint32_t hashlen,
    const uint8_t *slot, uint32_t len, uint32_t plen)
{
	One o(len, flags, hashlen, iv, 9, plen);
	std::vector<uint8_t> b = burst_of(slot, len);
	o.a.out = b.data();
	const uint32_t nb = encrypt_prep(o.a, 0);
	if (nb != 0)
		cbc_encrypt_lane(o.a, 0, nb, Tab{ Te0 }, Rk{ e.w });
	if (o.plen[0] != plen)
		fail("TX wrote plen");
	return Done{ o.res[0], plen, o.wire[0], nb, b };
}

bool all_are(const uint8_t *p, size_t n, uint8_t v)
{
	for (size_t i = 0; i < n; i++)
		if (p[i] != v)
			return false;
	return true;
}

/* where the payload lies: PH_ENCRYPTED alone, and PH_SIGNED under each hash */
struct Layout {
	uint32_t flags, hashlen, po;
};
const Layout layouts[] = {
	{ PKT_PH_ENCRYPTED, 0, 8 },
	{ PKT_PH_ENCRYPTED, 64, 8 },	/* hashlen counts only with PH_SIGNED */
	{ PKT_PH_ENCRYPTED | PKT_PH_SIGNED, 32, 40 },
	{ PKT_PH_ENCRYPTED | PKT_PH_SIGNED, 48, 56 },
	{ PKT_PH_ENCRYPTED | PKT_PH_SIGNED, 64, 72 },
};

/* Both directions, bit for bit against EVP: every length, every layout. */
void check_cbc()
{
	/* 1, 2, 3, 4, 92 and 93 blocks of ciphertext among them */
	const size_t lens[] = { 0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 63, 1456, 1471,
	    1472 };
	bool blocks[94] = {};
	unsigned refused = 0, refused_long = 0;
	uint8_t key[32], iv[16];
	std::vector<uint8_t> pt(1472), want(1472 + 32), back(1472 + 32);
	for (size_t len : lens)
		for (const Layout &l : layouts) {
			rnd_bytes(key, 32);
			rnd_bytes(iv, 16);
			rnd_bytes(pt.data(), len);
			AesSched e, d;
			aes256_enc_schedule(key, &e);
			aes256_dec_schedule(key, &d);
			const int wn = evp_run(EVP_aes_256_cbc(), true, key, iv, true, pt.data(),
			    len, want.data());
			if (wn != (int)(16 * (len / 16 + 1)))
				fail("EVP CBC encrypt, %zu bytes: %d", len, wn);
			const uint32_t n = (uint32_t)wn, po = l.po;
			if (payload_at(l.flags, l.hashlen) != po)
				fail("payload_at(%x, %u) = %u", l.flags, l.hashlen,
				    payload_at(l.flags, l.hashlen));
			blocks[n / 16] = true;

			/* TX: a slot of exactly header + ciphertext, the plaintext in it */
			std::vector<uint8_t> slot(po + n, 0x5a);
			rnd_bytes(slot.data(), po);
			memcpy(slot.data() + po, pt.data(), len);
			const Done t = tx(e, iv, l.flags, l.hashlen, slot.data(), po + n,
			    (uint32_t)len);
			if (t.code != PKT_OK || t.wire != po + n || t.nb != n / 16)
				fail("CBC encrypt, %zu bytes at %u: code %u, wire_len %u, %u blocks",
				    len, po, t.code, t.wire, t.nb);
			if (memcmp(&t.bytes[LEAD + po], want.data(), n) != 0)
				fail("CBC encrypt, %zu bytes at %u: %s..., EVP %s...", len, po,
				    hex(&t.bytes[LEAD + po], 16), hex(want.data(), 16));
			if (!all_are(t.bytes.data(), LEAD, SENTINEL) ||
			    memcmp(&t.bytes[LEAD], slot.data(), po) != 0)
				fail("CBC encrypt, %zu bytes at %u: wrote before the payload", len, po);

			/* RX of that datagram, out of place and in place */
			const uint8_t *dg = &t.bytes[LEAD];
			const Done r = rx(d, iv, l.flags, l.hashlen, dg, po + n, false);
			if (r.code != PKT_OK || r.plen != len || r.nb != n / 16)
				fail("CBC decrypt, %zu bytes at %u: code %u, plen %u, %u blocks", len,
				    po, r.code, r.plen, r.nb);
			if (memcmp(&r.bytes[LEAD + po], pt.data(), len) != 0)
				fail("CBC decrypt, %zu bytes at %u: wrong plaintext", len, po);
			if (!all_are(r.bytes.data(), LEAD + po, SENTINEL))
				fail("CBC decrypt, %zu bytes at %u: wrote before the payload", len, po);
			const Done ri = rx(d, iv, l.flags, l.hashlen, dg, po + n, true);
			if (ri.code != PKT_OK || ri.plen != len ||
			    memcmp(&ri.bytes[LEAD + po], &r.bytes[LEAD + po], n) != 0)
				fail("CBC decrypt in place, %zu bytes at %u: code %u, plen %u, or "
				    "other bytes than out of place", len, po, ri.code, ri.plen);
			if (!all_are(ri.bytes.data(), LEAD, SENTINEL) ||
			    memcmp(&ri.bytes[LEAD], dg, po) != 0)
				fail("CBC decrypt in place, %zu bytes at %u: wrote before the "
				    "payload", len, po);
			/* EVP agrees that this is what the ciphertext holds */
			const int en = evp_run(EVP_aes_256_cbc(), false, key, iv, true,
			    want.data(), n, back.data());
			if (en != (int)len || memcmp(back.data(), pt.data(), len) != 0)
				fail("EVP CBC decrypt, %zu bytes: %d", len, en);

			/* a last block whose padding is wrong: both refuse, and a refused
			 * datagram is BAD, plen 0, not a byte of it written */
			std::vector<uint8_t> bad(dg, dg + po + n);
			bad[po + n - 1] ^= 0x80;
			const int bad_e = evp_run(EVP_aes_256_cbc(), false, key, iv, true,
			    &bad[po], n, back.data());
			for (int in_place = 0; in_place < 2; in_place++) {
				const Done b = rx(d, iv, l.flags, l.hashlen, bad.data(), po + n,
				    in_place != 0);
				if ((b.code == PKT_BAD) != (bad_e < 0) ||
				    (b.code != PKT_BAD && (b.code != PKT_OK || (int)b.plen != bad_e)))
					fail("CBC decrypt of a damaged last block, %zu bytes: code "
					    "%u, plen %u, EVP %d", len, b.code, b.plen, bad_e);
				if (b.code != PKT_BAD)
					continue;
				refused++;
				refused_long += n / 16 >= 3;
				if (b.plen != 0)
					fail("a BAD datagram's plen is %u", b.plen);
				if (in_place ? memcmp(&b.bytes[LEAD], bad.data(), po + n) != 0 :
				    !all_are(b.bytes.data(), LEAD + po + n, SENTINEL))
					fail("a BAD datagram of %zu bytes at %u was written", len, po);
			}
		}
	for (int nb : { 1, 2, 3, 4, 92, 93 })
		if (!blocks[nb])
			fail("no case of %d blocks", nb);
	if (refused == 0 || refused_long == 0)
		fail("no damaged datagram was refused (%u, %u of three blocks and more)",
		    refused, refused_long);
}

/* What RX settles without the cipher (decrypt_prep). */
void check_rx_prep()
{
	uint8_t key[32], iv[16];
	rnd_bytes(key, 32);
	rnd_bytes(iv, 16);
	AesSched d;
	aes256_dec_schedule(key, &d);
	std::vector<uint8_t> dg(72 + 64);
	rnd_bytes(dg.data(), dg.size());

	auto untouched = [](const Done &r, const char *what, uint32_t len) {
		if (r.nb != 0 || r.plen != 0 ||
		    !all_are(r.bytes.data(), r.bytes.size(), SENTINEL))
			fail("%s, %u bytes: %u blocks, plen %u, or bytes written", what, len,
			    r.nb, r.plen);
	};
	for (const Layout &l : layouts) {
		/* empty and ragged ciphertext; a datagram that ends at or before
		 * its payload */
		for (uint32_t len : { l.po + 0, l.po + 15, l.po + 17, l.po + 1, l.po + 31,
		    l.po - 1, 1u, 0u }) {
			const Done r = rx(d, iv, l.flags, l.hashlen, dg.data(), len, false);
			if (r.code != PKT_BAD)
				fail("RX prep, %u bytes at %u: code %u, want BAD", len, l.po, r.code);
			untouched(r, "RX prep", len);
		}
		/* no PH_ENCRYPTED, or not OK on arrival: the code stays */
		const uint32_t len = l.po + 64;
		const Done c = rx(d, iv, l.flags & ~PKT_PH_ENCRYPTED, l.hashlen, dg.data(),
		    len, false);
		if (c.code != PKT_OK)
			fail("RX prep, a clear datagram: code %u", c.code);
		untouched(c, "RX prep, clear", len);
		for (uint8_t code : { PKT_RESOURCE, PKT_BAD, (uint8_t)3, PKT_NOCONN,
		    (uint8_t)255 }) {
			const Done r = rx(d, iv, l.flags, l.hashlen, dg.data(), len, false, code);
			if (r.code != code)
				fail("RX prep, arriving with code %u: code %u", code, r.code);
			untouched(r, "RX prep, not OK", len);
		}
	}
	/* i >= n: nothing read, nothing written (n = 1: the arrays end after
	 * element 0; n = 0: there are none) */
	One o(72 + 64, 3, 64, iv, PKT_OK, UNSET);
	AesBurstArgs none = {};
	if (decrypt_prep(o.a, 1) != 0 || decrypt_prep(o.a, ~(uint64_t)0) != 0 ||
	    decrypt_prep(none, 0) != 0 || o.res[0] != PKT_OK || o.plen[0] != UNSET)
		fail("RX prep past the burst's end");
}

/* What TX settles without the cipher (encrypt_prep). */
void check_tx_prep()
{
	uint8_t key[32], iv[16];
	rnd_bytes(key, 32);
	rnd_bytes(iv, 16);
	AesSched e;
	aes256_enc_schedule(key, &e);
	std::vector<uint8_t> slot(72 + 112);
	rnd_bytes(slot.data(), slot.size());

	auto untouched = [&](const Done &t, const char *what) {
		if (t.nb != 0 || !all_are(t.bytes.data(), LEAD, SENTINEL) ||
		    memcmp(&t.bytes[LEAD], slot.data(), t.bytes.size() - LEAD) != 0)
			fail("%s: %u blocks, or bytes written", what, t.nb);
	};
	for (const Layout &l : layouts)
		for (uint32_t plen : { 0u, 1u, 15u, 16u, 17u, 95u, 96u }) {
			const uint32_t po = l.po, fit = po + 16 * (plen / 16 + 1);
			/* one byte short of the room: RESOURCE; an exact fit: OK */
			const Done s = tx(e, iv, l.flags, l.hashlen, slot.data(), fit - 1, plen);
			if (s.code != PKT_RESOURCE || s.wire != 0)
				fail("TX prep, %u bytes in a slot of %u: code %u, wire_len %u",
				    plen, fit - 1, s.code, s.wire);
			untouched(s, "TX prep, a slot one byte short");
			const Done f = tx(e, iv, l.flags, l.hashlen, slot.data(), fit, plen);
			if (f.code != PKT_OK || f.wire != fit || f.nb != plen / 16 + 1)
				fail("TX prep, %u bytes in a slot of %u: code %u, wire_len %u",
				    plen, fit, f.code, f.wire);
			/* no PH_ENCRYPTED: the length as it is, RESOURCE past the slot */
			const uint32_t clear = l.flags & ~PKT_PH_ENCRYPTED;
			const Done c = tx(e, iv, clear, l.hashlen, slot.data(), po + plen, plen);
			if (c.code != PKT_OK || c.wire != po + plen)
				fail("TX prep, clear, %u bytes: code %u, wire_len %u", plen, c.code,
				    c.wire);
			untouched(c, "TX prep, a clear slot");
			if (plen == 0)
				continue;
			const Done p = tx(e, iv, clear, l.hashlen, slot.data(), po + plen - 1, plen);
			if (p.code != PKT_RESOURCE || p.wire != po + plen)
				fail("TX prep, clear, %u bytes past the slot: code %u, wire_len %u",
				    plen, p.code, p.wire);
			untouched(p, "TX prep, a clear slot too short");
		}
	One o(72 + 64, 3, 64, iv, 9, 17);
	AesBurstArgs none = {};
	if (encrypt_prep(o.a, 1) != 0 || encrypt_prep(o.a, ~(uint64_t)0) != 0 ||
	    encrypt_prep(none, 0) != 0 || o.res[0] != 9 || o.wire[0] != UNSET)
		fail("TX prep past the burst's end");
}

}	/* namespace */

int main()
{
	check_tables();
	check_known_answer();
	check_schedule();
	check_block_cipher();
	check_pad();
	check_cbc();
	check_rx_prep();
	check_tx_prep();
	printf("test_aes_host: ok\n");
	return 0;
}
