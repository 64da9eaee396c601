/*
 * test_aes_wave_host.cc -- host model of the wave form of the burst cipher's
 * RX decrypt (aes_cbc_decrypt_wave_kernel, aes_kernels.hip): a wave of 64
 * lanes in lockstep over the schedule of aes_wave.h, with the block code of
 * aes_device.h under the schedules of aes_sched.h, against libcrypto's EVP.
 *
 * The model runs what the kernel runs per datagram: the runs in the header's
 * order; in each run every lane loads its block and its prev into its own
 * registers before any lane stores; the padding verdict in the header's run
 * from the header's lane, before that run's stores.  Buffers are exact-size
 * heap blocks, so a block index off by one is an AddressSanitizer report.
 *
 * Checked, for nb = 1 .. 200 and 4,090 blocks: the plaintext and its length
 * in place and to a separate buffer; every block visited exactly once; with
 * broken padding (last byte 0; last byte 17; the last v bytes not all v) no
 * byte of either buffer changes.
 *
 * Exits non-zero with a message on the first mismatch.
 *   c++ -std=c++17 -Iilias_net2_amd/csrc tests/cxx/test_aes_wave_host.cc -lcrypto
 */
#include "aes_wave.h"
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
	fprintf(stderr, "test_aes_wave_host: FAIL: ");
	vfprintf(stderr, fmt, ap);
	fprintf(stderr, "\n");
	va_end(ap);
	exit(1);
}

/* splitmix64: a fixed stream, the same on every run */
uint64_t rng_state = 0x0a35c0ffee5eed02ull;
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

/* one EVP AES-256-CBC run; the output length, -1 where EVP fails */
int evp_cbc(bool enc, const uint8_t *key, const uint8_t *iv, bool pad,
    const uint8_t *in, size_t n, uint8_t *out)
{
	EVP_CIPHER_CTX *ctx = EVP_CIPHER_CTX_new();
	if (ctx == nullptr)
		fail("EVP_CIPHER_CTX_new");
	int n1 = 0, n2 = 0, rc = -1;
	if (EVP_CipherInit_ex(ctx, EVP_aes_256_cbc(), nullptr, key, iv, enc ? 1 : 0) == 1) {
		EVP_CIPHER_CTX_set_padding(ctx, pad ? 1 : 0);
		if (EVP_CipherUpdate(ctx, out, &n1, in, (int)n) == 1 &&
		    EVP_CipherFinal_ex(ctx, out + n1, &n2) == 1)
			rc = n1 + n2;
	}
	EVP_CIPHER_CTX_free(ctx);
	return rc;
}

/* ---- the wave ---------------------------------------------------------------- */

struct Tab {
	const uint32_t *t;
	uint32_t operator()(uint32_t x) const { return t[x]; }
};
struct Rk {
	const uint32_t *w;
	uint32_t operator()(int i) const { return w[i]; }
};

uint32_t Td0[256];

/* the kernel's ld16 / st16: a block <-> four big-endian words */
void ld16(const uint8_t *p, uint32_t (&w)[4])
{
	for (int k = 0; k < 4; k++)
		w[k] = (uint32_t)p[4 * k] << 24 | (uint32_t)p[4 * k + 1] << 16 |
		    (uint32_t)p[4 * k + 2] << 8 | (uint32_t)p[4 * k + 3];
}
void st16(uint8_t *p, const uint32_t (&w)[4])
{
	for (int k = 0; k < 16; k++)
		p[k] = (uint8_t)(w[k / 4] >> (24 - 8 * (k % 4)));
}

struct Lane {
	bool mine;
	uint32_t b;
	uint32_t x[4], prev[4];
};

/*
 * decrypt_by_wave of aes_kernels.hip for one datagram: src and dst are the
 * nb-block payload (dst == src: in place).  visits[b] counts the stores to
 * block b.  Returns the padding length, 0 for a datagram that ends BAD.
 */
uint32_t decrypt_by_wave(const AesSched &ks, const uint8_t iv[16],
    const uint8_t *src, uint8_t *dst, uint32_t nb, std::vector<uint32_t> &visits)
{
	const uint32_t runs = aes_wave_passes(nb);
	uint32_t pad = 0;
	std::vector<Lane> wave(NET2_AES_WAVE_LANES);

	for (uint32_t r = 0; r < runs; r++) {
		const uint32_t p = aes_wave_pass_of_run(nb, r);
		/* every lane's loads ... */
		for (uint32_t l = 0; l < NET2_AES_WAVE_LANES; l++) {
			Lane &L = wave[l];
			L.b = aes_wave_block(p, l);
			L.mine = L.b < nb;
			memset(L.x, 0, sizeof(L.x));
			memset(L.prev, 0, sizeof(L.prev));
			if (!L.mine)
				continue;
			ld16(src + 16 * (size_t)L.b, L.x);
			if (aes_wave_prev_is_iv(L.b))
				ld16(iv, L.prev);
			else
				ld16(src + 16 * (size_t)aes_wave_prev(L.b), L.prev);
		}
		/* ... the rounds, idle lanes on zeros ... */
		for (uint32_t l = 0; l < NET2_AES_WAVE_LANES; l++) {
			Lane &L = wave[l];
			aes_block<true>(Tab{ Td0 }, Rk{ ks.w }, L.x);
			for (int k = 0; k < 4; k++)
				L.x[k] ^= L.prev[k];
		}
		/* ... the verdict, known to all before anything is stored ... */
		if (r == NET2_AES_WAVE_VERDICT_RUN) {
			const Lane &V = wave[aes_wave_verdict_lane(nb)];
			if (!V.mine || V.b != nb - 1)
				fail("nb %u: the verdict lane holds block %u", nb, V.b);
			pad = aes_pkcs7_pad(V.x);
			if (pad == 0)
				break;
		}
		/* ... then every lane's stores */
		for (uint32_t l = 0; l < NET2_AES_WAVE_LANES; l++) {
			const Lane &L = wave[l];
			if (!L.mine)
				continue;
			st16(dst + 16 * (size_t)L.b, L.x);
			visits[L.b]++;
		}
	}
	return pad;
}

/* ---- the checks ------------------------------------------------------------ */

/* A valid ciphertext of nb blocks: in place and out of place against EVP. */
void check_valid(uint32_t nb)
{
	uint8_t key[32], iv[16];
	rnd_bytes(key, 32);
	rnd_bytes(iv, 16);
	const size_t clen = 16 * (size_t)nb;
	const size_t plen = clen - 1 - (size_t)(rnd64() % 16);	/* pad 1 .. 16 */
	std::vector<uint8_t> pt(plen ? plen : 1), ct(clen + 16), want(clen + 16);
	rnd_bytes(pt.data(), plen);
	if (evp_cbc(true, key, iv, true, pt.data(), plen, ct.data()) != (int)clen)
		fail("nb %u: EVP encrypt", nb);
	const int wn = evp_cbc(false, key, iv, true, ct.data(), clen, want.data());
	if (wn != (int)plen || memcmp(want.data(), pt.data(), plen) != 0)
		fail("nb %u: EVP decrypt: %d", nb, wn);
	AesSched ks;
	aes256_dec_schedule(key, &ks);

	for (int in_place = 0; in_place < 2; in_place++) {
		/* exact-size blocks: one byte past either end is a report */
		std::vector<uint8_t> src(ct.begin(), ct.begin() + clen);
		std::vector<uint8_t> sep(clen, 0xA5);
		uint8_t *dst = in_place ? src.data() : sep.data();
		std::vector<uint32_t> visits(nb, 0);
		const uint32_t pad = decrypt_by_wave(ks, iv, src.data(), dst, nb, visits);
		if (pad == 0 || clen - pad != plen)
			fail("nb %u %s: pad %u, plaintext of %zu bytes", nb,
			    in_place ? "in place" : "separate", pad, plen);
		if (memcmp(dst, pt.data(), plen) != 0) {
			size_t at = 0;
			while (dst[at] == pt[at])
				at++;
			fail("nb %u %s: plaintext differs from EVP's at byte %zu (block %zu)",
			    nb, in_place ? "in place" : "separate", at, at / 16);
		}
		for (uint32_t b = 0; b < nb; b++)
			if (visits[b] != 1)
				fail("nb %u: block %u stored %u times", nb, b, visits[b]);
		if (!in_place && memcmp(src.data(), ct.data(), clen) != 0)
			fail("nb %u: the ciphertext changed", nb);
	}
}

/* The three kinds of broken padding: nothing of either buffer changes. */
void check_broken(uint32_t nb)
{
	uint8_t key[32], iv[16];
	const size_t clen = 16 * (size_t)nb;
	for (int kind = 0; kind < 3; kind++) {
		rnd_bytes(key, 32);
		rnd_bytes(iv, 16);
		std::vector<uint8_t> body(clen), ct(clen + 16), out(clen + 32);
		rnd_bytes(body.data(), clen);
		if (kind == 0) {
			body[clen - 1] = 0;
		} else if (kind == 1) {
			body[clen - 1] = 17;
		} else {
			const uint32_t v = 2 + (uint32_t)(rnd64() % 15);	/* 2 .. 16 */
			memset(&body[clen - v], (int)v, v);
			body[clen - 2 - rnd64() % (v - 1)] ^= 0x01;	/* one of the v - 1 */
		}
		if (evp_cbc(true, key, iv, false, body.data(), clen, ct.data()) != (int)clen)
			fail("nb %u: EVP encrypt", nb);
		if (evp_cbc(false, key, iv, true, ct.data(), clen, out.data()) >= 0)
			fail("nb %u kind %d: EVP accepts the padding", nb, kind);
		AesSched ks;
		aes256_dec_schedule(key, &ks);
		for (int in_place = 0; in_place < 2; in_place++) {
			std::vector<uint8_t> src(ct.begin(), ct.begin() + clen);
			std::vector<uint8_t> sep(clen, 0xA5);
			uint8_t *dst = in_place ? src.data() : sep.data();
			std::vector<uint32_t> visits(nb, 0);
			if (decrypt_by_wave(ks, iv, src.data(), dst, nb, visits) != 0)
				fail("nb %u kind %d: not BAD", nb, kind);
			if (memcmp(src.data(), ct.data(), clen) != 0)
				fail("nb %u kind %d: the ciphertext changed", nb, kind);
			for (size_t i = 0; i < clen; i++)
				if (sep[i] != 0xA5)
					fail("nb %u kind %d: byte %zu of the output written",
					    nb, kind, i);
			for (uint32_t b = 0; b < nb; b++)
				if (visits[b] != 0)
					fail("nb %u kind %d: block %u stored", nb, kind, b);
		}
	}
}

/* The schedule itself: every block in exactly one (run, lane), last pass
 * first, and a run's reads below every earlier run's stores. */
void check_schedule(uint32_t nb)
{
	const uint32_t runs = aes_wave_passes(nb);
	std::vector<uint32_t> seen(nb, 0);
	uint32_t lowest_stored = nb;		/* by the runs so far */
	if (runs != (nb + 63) / 64)
		fail("nb %u: %u passes", nb, runs);
	for (uint32_t r = 0; r < runs; r++) {
		uint32_t lo = nb;
		for (uint32_t l = 0; l < NET2_AES_WAVE_LANES; l++) {
			const uint32_t b = aes_wave_block(aes_wave_pass_of_run(nb, r), l);
			if (b >= nb)
				continue;
			seen[b]++;
			lo = b < lo ? b : lo;
			if (b >= lowest_stored || (!aes_wave_prev_is_iv(b) &&
			    (aes_wave_prev(b) != b - 1 || b - 1 >= lowest_stored)))
				fail("nb %u run %u: block %u or its prev was stored already",
				    nb, r, b);
		}
		if (r == NET2_AES_WAVE_VERDICT_RUN && (lo > nb - 1 || lo + 64 < nb))
			fail("nb %u: the verdict run does not hold the last block", nb);
		lowest_stored = lo;
	}
	for (uint32_t b = 0; b < nb; b++)
		if (seen[b] != 1)
			fail("nb %u: block %u is in %u (run, lane) pairs", nb, b, seen[b]);
}

}	/* namespace */

int main()
{
	const Sbox inv = make_sbox(true);
	for (int x = 0; x < 256; x++)
		Td0[x] = aes_td0_word(inv.v[x]);
	for (uint32_t nb = 1; nb <= 200; nb++) {
		check_schedule(nb);
		check_valid(nb);
		check_broken(nb);
	}
	check_schedule(4090);
	check_valid(4090);
	check_broken(4090);
	printf("test_aes_wave_host: ok\n");
	return 0;
}
