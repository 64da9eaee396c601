/*
 * test_aes_tab_host.cc -- host check of the device cipher-key table's entry
 * (aes_tab.h) and of the rx key choice the _mc decrypt kernel makes per
 * datagram (aes_rx_alt, aes_device.h), without a GPU:
 *   - an entry filled from keys holds exactly the schedules of aes_sched.h at
 *     the documented offsets, and its meta words;
 *   - setting one side leaves the other side's words and bits alone;
 *   - aes_rx_alt against a plain restatement of net2_ck_rx_key
 *     (src/conn_keys.c:447-476) over a grid that wraps around 2^32;
 *   - an entry's schedules run the SP 800-38A F.2.5 / F.2.6 chain through
 *     aes_block;
 *   - the _mc kernels' own connection checks and key pick (aes_cbc.h:
 *     decrypt_mc_prep, encrypt_mc_prep, ciphertab_rx_key) over an exact-size
 *     table of two entries: NOCONN for a slot out of range or with the side
 *     unset, RESOURCE before NOCONN, no look-up where no cipher is needed.
 *
 * Exits non-zero with a message on the first mismatch.
 *   clang++ -std=c++17 -Iilias_net2_amd/csrc tests/cxx/test_aes_tab_host.cc
 */
#include "aes_cbc.h"
#include "aes_device.h"
#include "aes_sched.h"
#include "aes_tab.h"

#include <stdarg.h>
#include <stddef.h>
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
	fprintf(stderr, "test_aes_tab_host: FAIL: ");
	vfprintf(stderr, fmt, ap);
	fprintf(stderr, "\n");
	va_end(ap);
	exit(1);
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

void key_of(int k, uint8_t key[32])
{
	for (int i = 0; i < 32; i++)
		key[i] = (uint8_t)(17 * k + 29 * i + (i >> 2) + 1);
}

/* the entry as the kernels see it: words at byte offsets */
uint32_t word_at(const Net2CipherEnt &e, size_t byte)
{
	uint32_t w;
	memcpy(&w, (const uint8_t *)&e + byte, 4);
	return w;
}

void expect_sched(const Net2CipherEnt &e, size_t byte, const AesSched *ks,
    const char *what)
{
	for (int i = 0; i < NET2_AES_RKWORDS; i++) {
		const uint32_t want = ks != nullptr ? ks->w[i] : 0u;
		if (word_at(e, byte + 4 * (size_t)i) != want)
			fail("%s: word %d at +%zu = %08x, want %08x", what, i,
			    byte + 4 * (size_t)i, word_at(e, byte + 4 * (size_t)i), want);
	}
}

void expect_meta(const Net2CipherEnt &e, uint32_t bits, uint32_t cutoff,
    uint32_t rx_start, const char *what)
{
	if (word_at(e, 0) != bits || word_at(e, 4) != cutoff ||
	    word_at(e, 8) != rx_start || word_at(e, 12) != 0)
		fail("%s: meta %08x %08x %08x %08x, want %08x %08x %08x 0", what,
		    word_at(e, 0), word_at(e, 4), word_at(e, 8), word_at(e, 12), bits,
		    cutoff, rx_start);
}

void check_layout()
{
	if (sizeof(Net2CipherEnt) != 736 || alignof(Net2CipherEnt) != 16)
		fail("entry: %zu bytes, aligned %zu", sizeof(Net2CipherEnt),
		    alignof(Net2CipherEnt));
	if (offsetof(Net2CipherEnt, meta) != 0 || offsetof(Net2CipherEnt, dec) != 16 ||
	    offsetof(Net2CipherEnt, enc) != 496)
		fail("entry offsets");
	if (NET2_CT_RX != 1 || NET2_CT_TX != 2 || NET2_CT_RX_ALT != 4 ||
	    NET2_CT_RX_NOCUT != 8 || (NET2_CT_RX_BITS & NET2_CT_TX_BITS) != 0)
		fail("bit names");
}

void check_fill()
{
	uint8_t k0[32], k1[32], k2[32], k3[32];
	AesSched d0, d1, d3, e2, e3;
	key_of(0, k0);
	key_of(1, k1);
	key_of(2, k2);
	key_of(3, k3);
	aes256_dec_schedule(k0, &d0);
	aes256_dec_schedule(k1, &d1);
	aes256_dec_schedule(k3, &d3);
	aes256_enc_schedule(k2, &e2);
	aes256_enc_schedule(k3, &e3);

	/* rx with an alternate key into an unset entry: the tx side stays zero */
	Net2CipherEnt e = {};
	aes_tab_fill_rx(&e, k0, k1, false, 0x1234u, 0xfffffff0u);
	expect_meta(e, NET2_CT_RX | NET2_CT_RX_ALT, 0x1234u, 0xfffffff0u, "rx+alt");
	expect_sched(e, 16, &d0, "rx+alt active");
	expect_sched(e, 256, &d1, "rx+alt alternate");
	expect_sched(e, 496, nullptr, "rx+alt tx words");

	/* then tx: the rx words, bits, cutoff and rx_start stay */
	aes_tab_fill_tx(&e, k2);
	expect_meta(e, NET2_CT_RX | NET2_CT_RX_ALT | NET2_CT_TX, 0x1234u, 0xfffffff0u,
	    "tx after rx");
	expect_sched(e, 16, &d0, "tx after rx: active");
	expect_sched(e, 256, &d1, "tx after rx: alternate");
	expect_sched(e, 496, &e2, "tx after rx: tx");

	/* rx again, no cutoff: the tx words and bit stay */
	aes_tab_fill_rx(&e, k1, k0, true, 7, 9);
	expect_meta(e, NET2_CT_RX | NET2_CT_RX_ALT | NET2_CT_RX_NOCUT | NET2_CT_TX, 7, 9,
	    "rx no cutoff");
	expect_sched(e, 16, &d1, "rx no cutoff: active");
	expect_sched(e, 256, &d0, "rx no cutoff: alternate");
	expect_sched(e, 496, &e2, "rx no cutoff: tx");

	/* rx without an alternate key: no bits, no cutoff state, no stale schedule */
	aes_tab_fill_rx(&e, k3, nullptr, true, 7, 9);
	expect_meta(e, NET2_CT_RX | NET2_CT_TX, 0, 0, "rx plain");
	expect_sched(e, 16, &d3, "rx plain: active");
	expect_sched(e, 256, nullptr, "rx plain: alternate");
	expect_sched(e, 496, &e2, "rx plain: tx");

	/* tx alone, and tx twice */
	Net2CipherEnt t = {};
	aes_tab_fill_tx(&t, k2);
	aes_tab_fill_tx(&t, k3);
	expect_meta(t, NET2_CT_TX, 0, 0, "tx alone");
	expect_sched(t, 16, nullptr, "tx alone: active");
	expect_sched(t, 256, nullptr, "tx alone: alternate");
	expect_sched(t, 496, &e3, "tx alone: tx");
}

/* net2_ck_rx_key (src/conn_keys.c:447-476), restated plainly: distances from
 * the window start as 64-bit sums reduced mod 2^32 */
bool rx_key_by_definition(bool installed, bool no_cutoff, uint32_t fl,
    uint32_t seq, uint32_t cutoff, uint32_t rx_start)
{
	if (!installed)
		return false;
	if ((fl >> 31) & 1)		/* PH_ALTKEY */
		return true;
	if (no_cutoff)
		return false;
	const uint64_t m = (uint64_t)1 << 32;
	const uint64_t dseq = ((uint64_t)seq + m - rx_start) % m;
	const uint64_t dcut = ((uint64_t)cutoff + m - rx_start) % m;
	return dseq >= dcut;
}

void check_rx_choice()
{
	static const uint32_t starts[] = { 0, 1, 1000, 0x7fffffffu, 0x80000000u,
	    0xfffffff0u, 0xfffffff8u, 0xffffffffu };
	static const uint32_t spans[] = { 0, 1, 2, 15, 16, 17, 150, 0x7fffffffu,
	    0x80000000u, 0xffffffffu };
	static const int32_t steps[] = { -17, -16, -2, -1, 0, 1, 2, 15, 16, 17, 1000 };
	static const uint32_t flags[] = { 0, 1, 3, 0x80000000u, 0x80000003u,
	    0x7fffffffu };
	unsigned long n = 0, alts = 0, wraps = 0;
	for (uint32_t rx_start : starts)
		for (uint32_t span : spans) {
			const uint32_t cutoff = rx_start + span;	/* wraps */
			/* seq on both sides of the window start, of the cutoff and
			 * of the wrap */
			for (uint32_t at : { rx_start, cutoff, 0u, 0x80000000u })
				for (int32_t st : steps) {
					const uint32_t seq = at + (uint32_t)st;
					for (uint32_t fl : flags)
						for (int inst = 0; inst < 2; inst++)
							for (int nc = 0; nc < 2; nc++) {
								const bool got = aes_rx_alt(inst, nc, fl,
								    seq, cutoff, rx_start);
								const bool want = rx_key_by_definition(
								    inst, nc, fl, seq, cutoff, rx_start);
								if (got != want)
									fail("aes_rx_alt(%d, %d, %08x, seq %08x, "
									    "cutoff %08x, rx_start %08x) = %d, want %d",
									    inst, nc, fl, seq, cutoff, rx_start,
									    got, want);
								n++;
								alts += got;
								wraps += seq < rx_start && rx_start >= 0xfffffff0u;
							}
				}
		}
	if (n < 10000 || alts == 0 || alts == n || wraps == 0)
		fail("rx choice grid: %lu cases, %lu alternate, %lu wrapped", n, alts, wraps);
}

struct Tab {
	const uint32_t *t;
	uint32_t operator()(uint32_t x) const { return t[x]; }
};
struct Rk {
	const uint32_t *w;
	uint32_t operator()(int i) const { return w[i]; }
};

void to_words(const uint8_t *p, uint32_t (&w)[4])
{
	for (int k = 0; k < 4; k++)
		w[k] = (uint32_t)p[4 * k] << 24 | (uint32_t)p[4 * k + 1] << 16 |
		    (uint32_t)p[4 * k + 2] << 8 | (uint32_t)p[4 * k + 3];
}

/* SP 800-38A F.2.5 (CBC-AES256.Encrypt) and F.2.6 through one entry: the tx
 * schedule forwards, the active and the alternate rx schedule backwards */
void check_chain()
{
	uint32_t Te0[256], Td0[256];
	const Sbox fwd = make_sbox(false), inv = make_sbox(true);
	for (int x = 0; x < 256; x++) {
		Te0[x] = aes_te0_word(fwd.v[x]);
		Td0[x] = aes_td0_word(inv.v[x]);
	}
	uint8_t key[32], other[32], iv[16], pt[64], ct[64];
	unhex("603deb1015ca71be2b73aef0857d77811f352c073b6108d72d9810a30914dff4", key, 32);
	unhex("000102030405060708090a0b0c0d0e0f", iv, 16);
	unhex("6bc1bee22e409f96e93d7e117393172aae2d8a571e03ac9c9eb76fac45af8e51"
	    "30c81c46a35ce411e5fbc1191a0a52eff69f2445df4f9b17ad2b417be66c3710", pt, 64);
	unhex("f58c4c04d6e5f1ba779eabfb5f7bfbd69cfc4e967edb808d679f777bc6702c7d"
	    "39f23369a9d9bacfa530e26304231461b2eb05e2c39be9fcda6c19078c6a9d1b", ct, 64);
	key_of(5, other);
	for (int alt = 0; alt < 2; alt++) {
		Net2CipherEnt e = {};
		aes_tab_fill_rx(&e, alt ? other : key, alt ? key : nullptr, false, 0, 0);
		aes_tab_fill_tx(&e, key);
		uint32_t chain[4], prev[4];
		to_words(iv, chain);
		to_words(iv, prev);
		for (int b = 0; b < 4; b++) {
			uint32_t p[4], c[4], x[4];
			to_words(pt + 16 * b, p);
			to_words(ct + 16 * b, c);
			for (int k = 0; k < 4; k++)
				chain[k] ^= p[k];
			aes_block<false>(Tab{ Te0 }, Rk{ e.enc }, chain);
			for (int k = 0; k < 4; k++)
				x[k] = c[k];
			aes_block<true>(Tab{ Td0 }, Rk{ e.dec[alt] }, x);
			for (int k = 0; k < 4; k++) {
				if (chain[k] != c[k])
					fail("F.2.5 block %d word %d: %08x, want %08x", b, k,
					    chain[k], c[k]);
				if ((x[k] ^ prev[k]) != p[k])
					fail("F.2.6 (schedule %d) block %d word %d: %08x, want "
					    "%08x", alt, b, k, x[k] ^ prev[k], p[k]);
				prev[k] = c[k];
			}
		}
	}
}

/*
 * The _mc lane and wave kernels' connection checks and key pick (aes_cbc.h)
 * over a burst of one datagram and a table of exactly two entries on the
 * heap, every per-datagram array a heap array of one element: what lies
 * outside them AddressSanitizer reports.
 */
constexpr uint32_t UNSET = 0xdeadbeefu;

struct One {
	std::vector<uint64_t> off;
	std::vector<uint32_t> len, fl, seq, plen, wire, conn;
	std::vector<uint8_t> res;
	AesMcArgs m;

	One(const std::vector<Net2CipherEnt> *tab, uint32_t c, uint32_t length,
	    uint32_t flags, uint8_t code, uint32_t pl) :
	    off(1, 0), len(1, length), fl(1, flags), seq(1, 0), plen(1, pl),
	    wire(1, UNSET), conn(1, c), res(1, code), m()
	{
		m.b.offsets = off.data();
		m.b.lens = len.data();
		m.b.seq = seq.data();
		m.b.flags = fl.data();
		m.b.result = res.data();
		m.b.plen = plen.data();
		m.b.wire_len = wire.data();
		m.b.n = 1;
		m.b.hashlen = 64;
		m.conn = conn.data();
		m.tab = tab != nullptr ? tab->data() : nullptr;
		m.slots = tab != nullptr ? (uint32_t)tab->size() : 0;
	}
};

void check_mc_prep()
{
	uint8_t k0[32], k1[32];
	key_of(0, k0);
	key_of(1, k1);
	/* a: entry 0 with both sides and an alternate rx key, entry 1 rx alone;
	 * b: entry 0 tx alone, entry 1 unset */
	std::vector<Net2CipherEnt> a(2), b(2);
	aes_tab_fill_rx(&a[0], k0, k1, false, 100, 50);
	aes_tab_fill_tx(&a[0], k0);
	aes_tab_fill_rx(&a[1], k1, nullptr, false, 0, 0);
	aes_tab_fill_tx(&b[0], k0);
	const uint32_t ES = PKT_PH_ENCRYPTED | PKT_PH_SIGNED, po = 72;

	struct Case {
		const std::vector<Net2CipherEnt> *tab;
		uint32_t conn;
		bool rx, tx;	/* the datagram has a connection to decrypt / encrypt */
	};
	const Case cases[] = {
		{ &a, 0, true, true }, { &a, 1, true, false }, { &b, 0, false, true },
		{ &b, 1, false, false },
		/* out of range: clamped, nothing read past the table */
		{ &a, 2, false, false }, { &a, 3, false, false },
		{ &a, 0x80000000u, false, false }, { &a, 0xffffffffu, false, false },
	};
	for (const Case &c : cases) {
		/* RX: four blocks of ciphertext */
		One r(c.tab, c.conn, po + 64, ES, PKT_OK, UNSET);
		const uint32_t nb = decrypt_mc_prep(r.m, 0);
		if (c.rx ? (nb != 4 || r.res[0] != PKT_OK || r.plen[0] != UNSET) :
		    (nb != 0 || r.res[0] != PKT_NOCONN || r.plen[0] != 0))
			fail("RX _mc prep, slot %u: %u blocks, code %u, plen %u", c.conn, nb,
			    r.res[0], r.plen[0]);
		/* TX: 17 bytes into an exact fit of two blocks */
		One t(c.tab, c.conn, po + 32, ES, 9, 17);
		const uint32_t tb = encrypt_mc_prep(t.m, 0);
		if (c.tx ? (tb != 2 || t.res[0] != PKT_OK || t.wire[0] != po + 32) :
		    (tb != 0 || t.res[0] != PKT_NOCONN || t.wire[0] != 0))
			fail("TX _mc prep, slot %u: %u blocks, code %u, wire_len %u", c.conn,
			    tb, t.res[0], t.wire[0]);
		/* TX one byte short: RESOURCE, whatever the connection */
		One s(c.tab, c.conn, po + 31, ES, 9, 17);
		if (encrypt_mc_prep(s.m, 0) != 0 || s.res[0] != PKT_RESOURCE ||
		    s.wire[0] != 0)
			fail("TX _mc prep, slot %u, no room: code %u, wire_len %u", c.conn,
			    s.res[0], s.wire[0]);
	}
	/* what needs no cipher does no look-up: no table, a slot out of range */
	for (uint32_t conn : { 0u, 7u, 0xffffffffu }) {
		One clear(nullptr, conn, po + 64, PKT_PH_SIGNED, PKT_OK, UNSET);
		if (decrypt_mc_prep(clear.m, 0) != 0 || clear.res[0] != PKT_OK ||
		    clear.plen[0] != 0)
			fail("RX _mc prep, a clear datagram: code %u", clear.res[0]);
		One late(nullptr, conn, po + 64, ES, PKT_BAD, UNSET);
		if (decrypt_mc_prep(late.m, 0) != 0 || late.res[0] != PKT_BAD ||
		    late.plen[0] != 0)
			fail("RX _mc prep, arriving BAD: code %u", late.res[0]);
		One tclear(nullptr, conn, po + 17, PKT_PH_SIGNED, 9, 17);
		if (encrypt_mc_prep(tclear.m, 0) != 0 || tclear.res[0] != PKT_OK ||
		    tclear.wire[0] != po + 17)
			fail("TX _mc prep, a clear slot: code %u, wire_len %u", tclear.res[0],
			    tclear.wire[0]);
		One tshort(nullptr, conn, po + 31, ES, 9, 17);
		if (encrypt_mc_prep(tshort.m, 0) != 0 || tshort.res[0] != PKT_RESOURCE)
			fail("TX _mc prep, no room and no table: code %u", tshort.res[0]);
		One past(nullptr, conn, po + 64, ES, PKT_OK, UNSET);
		if (decrypt_mc_prep(past.m, 1) != 0 || encrypt_mc_prep(past.m, 1) != 0 ||
		    past.res[0] != PKT_OK || past.plen[0] != UNSET || past.wire[0] != UNSET)
			fail("_mc prep past the burst's end");
	}

	/* the key pick: the alternate schedule exactly when aes_rx_alt says so */
	unsigned picks[2] = { 0, 0 };
	for (uint32_t slot = 0; slot < 2; slot++)
		for (uint32_t fl : { ES, ES | 0x80000000u })
			for (uint32_t seq : { 0u, 49u, 50u, 99u, 100u, 101u, 0xffffffffu }) {
				One r(&a, slot, po + 64, fl, PKT_OK, UNSET);
				r.seq[0] = seq;
				const bool alt = aes_rx_alt(slot == 0, false, fl, seq, 100, 50);
				if (slot == 1 && alt)
					fail("aes_rx_alt without an alternate key");
				if (ciphertab_rx_key(r.m, 0, fl) != a[slot].dec[alt ? 1 : 0])
					fail("ciphertab_rx_key, slot %u, flags %08x, seq %u: not "
					    "schedule %d", slot, fl, seq, alt ? 1 : 0);
				picks[alt ? 1 : 0]++;
			}
	if (picks[0] == 0 || picks[1] == 0)
		fail("key pick: %u active, %u alternate", picks[0], picks[1]);
}

}	/* namespace */

int main()
{
	check_layout();
	check_fill();
	check_rx_choice();
	check_chain();
	check_mc_prep();
	printf("test_aes_tab_host: ok\n");
	return 0;
}
