/*
 * test_aes_host.cc -- host check of the burst cipher's block code and key
 * schedules: aes_device.h (the T-table rounds, the last round's S-box
 * recovery, the PKCS#7 check) under the schedules of aes_sched.h, with a
 * plain 256-word array as the table and a plain schedule as the round keys,
 * against libcrypto's EVP and against restatements of FIPS 197 written here.
 * No GPU: this is the arithmetic the kernels of aes_kernels.hip run, and the
 * CBC chaining as they do it (RX: last block first; TX: the padded tail).
 *
 * Exits non-zero with a message on the first mismatch.
 *   c++ -std=c++17 -Iilias_net2_amd/csrc tests/cxx/test_aes_host.cc -lcrypto
 */
#include "aes_device.h"
#include "aes_sched.h"

#include <openssl/evp.h>

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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
 * RX as aes_cbc_decrypt_kernel chains it: the last block first (its padding
 * decides), then the blocks in order.  Returns the plaintext length, -1 for
 * what the kernel makes BAD.
 */
int cbc_decrypt_as_kernel(const AesSched &d, const uint8_t iv[16],
    const uint8_t *ct, size_t clen, uint8_t *out)
{
	if (clen == 0 || clen % 16 != 0)
		return -1;
	const size_t nb = clen / 16;
	uint8_t x[16];
	const uint8_t *prev = nb > 1 ? ct + 16 * (nb - 2) : iv;
	block_dec(d, ct + 16 * (nb - 1), x);
	uint32_t w[4];
	for (int k = 0; k < 16; k++)
		x[k] ^= prev[k];
	to_words(x, w);
	const uint32_t pad = aes_pkcs7_pad(w);
	if (pad == 0)
		return -1;
	memcpy(out + 16 * (nb - 1), x, 16);
	for (size_t b = 0; b + 1 < nb; b++) {
		prev = b == 0 ? iv : ct + 16 * (b - 1);
		block_dec(d, ct + 16 * b, x);
		for (int k = 0; k < 16; k++)
			out[16 * b + k] = x[k] ^ prev[k];
	}
	return (int)(16 * nb - pad);
}

/* TX as aes_cbc_encrypt_kernel chains it: whole blocks, then the tail and
 * its padding (a whole block of 16 when the length is a multiple of 16). */
size_t cbc_encrypt_as_kernel(const AesSched &e, const uint8_t iv[16],
    const uint8_t *pt, size_t plen, uint8_t *out)
{
	const size_t nb = plen / 16 + 1, rem = plen % 16;
	uint8_t chain[16], cur[16];
	memcpy(chain, iv, 16);
	for (size_t j = 0; j < nb; j++) {
		for (size_t k = 0; k < 16; k++)
			cur[k] = j + 1 < nb ? pt[16 * j + k] :
			    k < rem ? pt[16 * j + k] : (uint8_t)(16 - rem);
		for (int k = 0; k < 16; k++)
			chain[k] ^= cur[k];
		block_enc(e, chain, chain);
		memcpy(out + 16 * j, chain, 16);
	}
	return 16 * nb;
}

void check_cbc()
{
	const size_t lens[] = { 0, 1, 15, 16, 17, 31, 32, 33, 1472 };
	uint8_t key[32], iv[16];
	std::vector<uint8_t> pt(1472), ct(1472 + 32), want(1472 + 32), back(1472 + 32);
	for (size_t len : lens) {
		rnd_bytes(key, 32);
		rnd_bytes(iv, 16);
		rnd_bytes(pt.data(), len);
		AesSched e, d;
		aes256_enc_schedule(key, &e);
		aes256_dec_schedule(key, &d);
		const int wn = evp_run(EVP_aes_256_cbc(), true, key, iv, true, pt.data(),
		    len, want.data());
		const size_t n = cbc_encrypt_as_kernel(e, iv, pt.data(), len, ct.data());
		if (wn != (int)n || memcmp(ct.data(), want.data(), n) != 0)
			fail("CBC encrypt, %zu bytes: %zu bytes %s..., EVP %d bytes %s...",
			    len, n, hex(ct.data(), 16), wn, hex(want.data(), 16));
		const int pn = cbc_decrypt_as_kernel(d, iv, want.data(), n, back.data());
		if (pn != (int)len || memcmp(back.data(), pt.data(), len) != 0)
			fail("CBC decrypt, %zu bytes: got %d bytes", len, pn);
		/* EVP agrees that this is what the ciphertext holds */
		const int en = evp_run(EVP_aes_256_cbc(), false, key, iv, true,
		    want.data(), n, back.data());
		if (en != (int)len || memcmp(back.data(), pt.data(), len) != 0)
			fail("EVP CBC decrypt, %zu bytes: %d", len, en);
		/* a last block whose padding is wrong: both refuse */
		want[n - 1] ^= 0x80;
		const int bad_k = cbc_decrypt_as_kernel(d, iv, want.data(), n, back.data());
		const int bad_e = evp_run(EVP_aes_256_cbc(), false, key, iv, true,
		    want.data(), n, back.data());
		if ((bad_k < 0) != (bad_e < 0) || (bad_k >= 0 && bad_k != bad_e))
			fail("CBC decrypt of a damaged last block, %zu bytes: %d, EVP %d",
			    len, bad_k, bad_e);
	}
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
	printf("test_aes_host: ok\n");
	return 0;
}
