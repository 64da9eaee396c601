/*
 * test_aes_quad_host.cc -- host model of the quad form of the burst cipher's
 * TX encrypt (aes_cbc_encrypt_quad_kernel, aes_kernels.hip): four lanes in
 * lockstep over the schedule of aes_quad.h, one column of the state each, with
 * the column code of aes_device.h under the schedules of aes_sched.h and the
 * prep steps of aes_cbc.h, against libcrypto's EVP.
 *
 * The model runs what the kernel runs per datagram: lane 0's prep step, the
 * block count made known to the other three; each lane's fifteen schedule
 * words (out of the launch's schedule, or out of the datagram's table entry);
 * then per block every lane's load of the next word, every lane's entry, and
 * per round every lane's exchange before any lane's round -- a lane reads its
 * neighbours' columns as they were after the round before.  One-datagram
 * bursts in exact-size heap blocks, so a byte read or written outside the
 * datagram is an AddressSanitizer report.
 *
 * Checked, for 1, 2, 3, 4, 88, 89, 90 and 93 blocks, every plen mod 16, the
 * payload 8, 40, 56 and 72 bytes into a datagram at an odd offset, both key
 * sources: the ciphertext, code and wire_len against EVP; the same with the
 * slot's bytes past plen filled another way; every byte before the payload
 * unchanged.  Then the codes the prep steps settle, where no cipher work may
 * happen: the slot as it was.
 *
 * Exits non-zero with a message on the first mismatch.
 *   clang++ -std=c++17 -Iilias_net2_amd/csrc tests/cxx/test_aes_quad_host.cc -lcrypto
 */
#include "aes_quad.h"
#include "aes_device.h"
#include "aes_sched.h"
#include "aes_cbc.h"

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
	fprintf(stderr, "test_aes_quad_host: FAIL: ");
	vfprintf(stderr, fmt, ap);
	fprintf(stderr, "\n");
	va_end(ap);
	exit(1);
}

/* splitmix64: a fixed stream, the same on every run */
uint64_t rng_state = 0x0a35c0ffee5eed04ull;
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

/* EVP AES-256-CBC encryption with padding; the output length */
size_t evp_encrypt(const uint8_t *key, const uint8_t *iv, const uint8_t *in,
    size_t n, uint8_t *out)
{
	EVP_CIPHER_CTX *ctx = EVP_CIPHER_CTX_new();
	int n1 = 0, n2 = 0;
	if (ctx == nullptr ||
	    EVP_EncryptInit_ex(ctx, EVP_aes_256_cbc(), nullptr, key, iv) != 1 ||
	    EVP_EncryptUpdate(ctx, out, &n1, in, (int)n) != 1 ||
	    EVP_EncryptFinal_ex(ctx, out + n1, &n2) != 1)
		fail("EVP encrypt");
	EVP_CIPHER_CTX_free(ctx);
	return (size_t)(n1 + n2);
}

/* ---- the quad ------------------------------------------------------------------ */

struct Tab {
	const uint32_t *t;
	uint32_t operator()(uint32_t x) const { return t[x]; }
};

uint32_t Te0[256];

struct Lane {
	uint32_t q;
	uint32_t kw[NET2_AES_QUAD_KEYWORDS];
	uint32_t chain, cur, nx, s, in[4];
};

/*
 * encrypt_by_quad of aes_kernels.hip for slot i of burst a: nb >= 1 blocks as
 * the prep step counted them, sched the 60-word schedule the quad's lanes pick
 * their words from.
 */
void encrypt_by_quad(const AesBurstArgs &a, uint64_t i, uint32_t nb,
    const uint32_t *sched)
{
	Lane quad[NET2_AES_QUAD_LANES];
	uint8_t *p = a.out + a.offsets[i] + payload_at(a.flags[i], a.hashlen);
	const uint32_t plen = a.plen[i];
	const Tab T = { Te0 };

	for (uint32_t l = 0; l < NET2_AES_QUAD_LANES; l++) {
		Lane &L = quad[l];
		L.q = aes_quad_col(l);
		if (aes_quad_of(l) != 0)
			fail("lane %u is not of quad 0", l);
		for (int r = 0; r < NET2_AES_QUAD_KEYWORDS; r++)
			L.kw[r] = sched[aes_quad_rk(r, L.q)];
		L.chain = aes_quad_ld(a.iv + 16 * i, L.q);
		L.cur = aes_quad_word(p, plen, nb, 0, L.q);
	}
	for (uint32_t j = 0; j < nb; j++) {
		/* every lane's next word, before anything of block j is stored */
		for (Lane &L : quad)
			L.nx = j + 1 < nb ? aes_quad_word(p, plen, nb, j + 1, L.q) : 0u;
		for (Lane &L : quad)
			L.s = aes_quad_enter(L.chain, L.cur, L.kw[0]);
		for (int r = 1; r <= NET2_AES_ROUNDS; r++) {
			/* every lane's exchange ... */
			for (Lane &L : quad)
				for (uint32_t k = 0; k < 4; k++)
					L.in[k] = quad[aes_quad_src(L.q, k)].s;
			/* ... then every lane's round */
			for (Lane &L : quad) {
				if (L.in[0] != L.s)
					fail("input 0 of lane %u is not its own column", L.q);
				L.s = aes_quad_round(T, r, L.in[0], L.in[1], L.in[2], L.in[3],
				    L.kw[r]);
			}
		}
		for (Lane &L : quad) {
			aes_quad_st(p + 16 * (size_t)j, L.q, L.s);
			L.chain = L.s;
			L.cur = L.nx;
		}
	}
}

/* ---- one-datagram bursts ---------------------------------------------------- */

struct Slot {
	std::vector<uint8_t> iv;
	uint8_t *buf;		/* exactly off + len bytes */
	size_t size;
	uint64_t off;
	uint32_t len, flags, plen, wire, conn;
	uint8_t result;
	AesBurstArgs a;

	Slot(uint64_t off_, uint32_t len_, uint32_t flags_, uint32_t plen_,
	    uint32_t hashlen) :
	    iv(16), size((size_t)off_ + len_), off(off_), len(len_), flags(flags_),
	    plen(plen_), wire(0x5A5A5A5Au), conn(0), result(9)
	{
		buf = (uint8_t *)malloc(size ? size : 1);
		if (buf == nullptr)
			fail("malloc");
		rnd_bytes(buf, size);
		rnd_bytes(iv.data(), 16);
		a = AesBurstArgs{};
		a.out = buf;
		a.offsets = &off;
		a.lens = &len;
		a.flags = &flags;
		a.iv = iv.data();
		a.result = &result;
		a.plen = &plen;
		a.wire_len = &wire;
		a.n = 1;
		a.hashlen = hashlen;
	}
	~Slot() { free(buf); }
	Slot(const Slot &) = delete;
	Slot &operator=(const Slot &) = delete;
};

/* The kernel's body for the one slot: the prep step on lane 0, then the quad. */
void run_one(Slot &s, const AesSched &ks)
{
	const uint32_t nb = encrypt_prep(s.a, 0);
	if (nb != 0)
		encrypt_by_quad(s.a, 0, nb, ks.w);
}

void run_mc(Slot &s, const Net2CipherEnt *tab, uint32_t slots)
{
	AesMcArgs m = {};
	m.b = s.a;
	m.conn = &s.conn;
	m.tab = tab;
	m.slots = slots;
	const uint32_t nb = encrypt_mc_prep(m, 0);
	if (nb != 0) {
		bool in;
		encrypt_by_quad(s.a, 0, nb, ciphertab_ent(m, 0, &in)->enc);
	}
}

const uint32_t HASHLEN[4] = { 0, 32, 48, 64 };	/* payload at 8, 40, 56, 72 */

/* nb blocks, plen = 16 (nb - 1) + rem, payload offset by `at`, key source mc. */
void check_cipher(uint32_t nb, uint32_t rem, int at, bool mc)
{
	const uint32_t hashlen = HASHLEN[at];
	const uint32_t flags = PKT_PH_ENCRYPTED | (hashlen != 0 ? PKT_PH_SIGNED : 0u);
	const uint32_t po = 8 + hashlen;
	const uint32_t plen = 16 * (nb - 1) + rem;
	const uint64_t off = 1 + 2 * (rnd64() % 16);		/* odd */
	uint8_t key[32], other[32];
	rnd_bytes(key, 32);
	rnd_bytes(other, 32);
	AesSched ks;
	aes256_enc_schedule(key, &ks);
	std::vector<Net2CipherEnt> tab(3);
	memset(tab.data(), 0, 3 * sizeof(Net2CipherEnt));
	aes_tab_fill_tx(&tab[0], other);
	aes_tab_fill_tx(&tab[2], key);

	std::vector<uint8_t> want(16 * (size_t)nb), first, iv0;
	for (int fill = 0; fill < 2; fill++) {
		Slot s(off, po + 16 * nb, flags, plen, hashlen);
		s.conn = 2;
		if (fill == 0) {
			first.assign(s.buf, s.buf + s.size);
			iv0 = s.iv;
			if (evp_encrypt(key, iv0.data(), s.buf + off + po, plen,
			    want.data()) != want.size())
				fail("nb %u rem %u: EVP's length", nb, rem);
		} else {
			/* the same plaintext and IV, the slack filled another way */
			memcpy(s.buf, first.data(), off + po + plen);
			memset(s.buf + off + po + plen, 0xEE, 16 * nb - plen);
			memcpy(s.iv.data(), iv0.data(), 16);
		}
		std::vector<uint8_t> before(s.buf, s.buf + s.size);
		if (mc)
			run_mc(s, tab.data(), 3);
		else
			run_one(s, ks);
		if (s.result != PKT_OK || s.wire != po + 16 * nb)
			fail("nb %u rem %u at %u mc %d: code %u wire_len %u", nb, rem, po, mc,
			    s.result, s.wire);
		if (memcmp(s.buf + off + po, want.data(), want.size()) != 0) {
			size_t k = 0;
			while (s.buf[off + po + k] == want[k])
				k++;
			fail("nb %u rem %u at %u mc %d fill %d: ciphertext differs from "
			    "EVP's at byte %zu (block %zu)", nb, rem, po, mc, fill, k, k / 16);
		}
		if (memcmp(s.buf, before.data(), off + po) != 0)
			fail("nb %u rem %u at %u mc %d: bytes before the payload changed",
			    nb, rem, po, mc);
	}
}

/* What the prep steps settle: the code, wire_len, and the slot as it was. */
void check_settled(const char *what, bool mc, uint32_t flags, uint32_t plen,
    uint32_t len, uint32_t conn, uint8_t want_code, uint32_t want_wire)
{
	const uint32_t hashlen = 64;
	uint8_t key[32];
	rnd_bytes(key, 32);
	AesSched ks;
	aes256_enc_schedule(key, &ks);
	std::vector<Net2CipherEnt> tab(2);
	memset(tab.data(), 0, 2 * sizeof(Net2CipherEnt));
	aes_tab_fill_tx(&tab[0], key);
	aes_tab_fill_rx(&tab[1], key, nullptr, false, 0, 0);	/* no tx side */
	Slot s(3, len, flags, plen, hashlen);
	s.conn = conn;
	std::vector<uint8_t> before(s.buf, s.buf + s.size);
	if (mc)
		run_mc(s, tab.data(), 2);
	else
		run_one(s, ks);
	if (s.result != want_code || s.wire != want_wire)
		fail("%s (mc %d): code %u wire_len %u, want %u and %u", what, mc, s.result,
		    s.wire, want_code, want_wire);
	if (memcmp(s.buf, before.data(), s.size) != 0)
		fail("%s (mc %d): the slot changed", what, mc);
}

}	/* namespace */

int main()
{
	const Sbox fwd = make_sbox(false);
	for (int x = 0; x < 256; x++)
		Te0[x] = aes_te0_word(fwd.v[x]);

	const uint32_t NBS[] = { 1, 2, 3, 4, 88, 89, 90, 93 };
	for (uint32_t nb : NBS)
		for (uint32_t rem = 0; rem < 16; rem++)
			for (int at = 0; at < 4; at++)
				for (int mc = 0; mc < 2; mc++)
					check_cipher(nb, rem, at, mc != 0);

	const uint32_t E = PKT_PH_ENCRYPTED, S = PKT_PH_SIGNED;
	for (int mc = 0; mc < 2; mc++) {
		/* not PH_ENCRYPTED: the length as it is, or no room for it */
		check_settled("plain", mc, S, 100, 172, 0, PKT_OK, 172);
		check_settled("plain, unsigned", mc, 0, 100, 108, 0, PKT_OK, 108);
		check_settled("plain, a byte short", mc, S, 100, 171, 0, PKT_RESOURCE, 172);
		/* PH_ENCRYPTED a byte short of the padded length */
		check_settled("short", mc, E | S, 100, 72 + 111, 0, PKT_RESOURCE, 0);
		check_settled("short, full pad", mc, E, 32, 8 + 47, 0, PKT_RESOURCE, 0);
		/* the 64-bit room check: plen near 2^32 */
		check_settled("huge plen", mc, E | S, 0xfffffff0u, 200, 0, PKT_RESOURCE, 0);
	}
	/* without a connection: out of range, or the slot's tx side unset;
	 * RESOURCE wins over NOCONN; no look-up without PH_ENCRYPTED */
	check_settled("conn out of range", true, E | S, 100, 72 + 112, 2, PKT_NOCONN, 0);
	check_settled("conn far out of range", true, E | S, 100, 72 + 112, 0xffffffffu,
	    PKT_NOCONN, 0);
	check_settled("tx side unset", true, E | S, 100, 72 + 112, 1, PKT_NOCONN, 0);
	check_settled("short and no connection", true, E | S, 100, 72 + 111, 1,
	    PKT_RESOURCE, 0);
	check_settled("plain and no connection", true, S, 100, 172, 0xffffffffu, PKT_OK,
	    172);
	printf("test_aes_quad_host: ok\n");
	return 0;
}
