/*
 * test_tab_ops_host.cc -- host check of the bulk table updates
 * (net2_burst_keytab_update / net2_burst_ciphertab_update) without a GPU:
 *   (a) the reduction of an op list to one record per slot and launch
 *       (net2_tab_ops.h): random lists of 1 to 300 ops over 1 to 16 slots, cut
 *       into launches of several sizes, leave a table byte for byte as the ops
 *       applied one by one do;
 *   (b) the per-record bodies the update kernels run (tab_update.h), here in
 *       their host instantiation -- h_compress256 / h_compress512 and a plain
 *       S-box array plugged in -- against entries built the per-slot way:
 *       hmac_key_mids (sha2_keyprep.h) plus the meta rules of
 *       keytab_set_kernel, and aes_tab_fill_rx / aes_tab_fill_tx (aes_tab.h).
 *       Rows 4, 5 and 6; with and without an alternate key, with and without
 *       cutoff, cipher bits on and off; TX after RX, RX after TX, CLEAR
 *       between them;
 *   - every record is all zero once its body has run;
 *   - aes_keysched.h's templates give aes_sched.h's schedules word for word.
 * The records live in exact-size heap arrays, so a read or write outside one
 * is AddressSanitizer's.
 *
 * Exits non-zero with a message on the first mismatch.
 *   clang++ -std=c++17 -Iilias_net2_amd/csrc -Itests/cxx/hipstub \
 *       tests/cxx/test_tab_ops_host.cc
 */
#include "sha2_keyprep.h"
#include "sha2_launch.h"
#include "tab_update.h"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <random>
#include <vector>

namespace {

[[noreturn]] void fail(const char *fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	fprintf(stderr, "test_tab_ops_host: FAIL: ");
	vfprintf(stderr, fmt, ap);
	fprintf(stderr, "\n");
	va_end(ap);
	exit(1);
}

static_assert(sizeof(Net2KeyEnt) == 16 * NET2_TAB_KT_PIECES &&
    offsetof(Net2KeyEnt, rx) == 16 && offsetof(Net2KeyEnt, tx) == 272,
    "the key-table entry in pieces");
static_assert(NET2_TR_KT_RX_BITS == NET2_KT_RX_BITS &&
    NET2_TR_KT_TX_BITS == NET2_KT_TX_BITS && NET2_TR_KT_RX_ENC == NET2_KT_RX_ENC &&
    NET2_TR_KT_TX_ENC == NET2_KT_TX_ENC, "the records' bits");

/* the host's compressions behind the bodies' C parameter */
struct HostCompress {
	static void c256(uint32_t (&st)[8], uint32_t (&m)[16])
	{
		net2::dev::h_compress256(st, m);
	}
	static void c512(uint64_t (&st)[8], uint64_t (&m)[16])
	{
		net2::dev::h_compress512(st, m);
	}
};

struct HostSbox {
	uint32_t operator()(uint32_t x) const { return h_sbox.v[x]; }
};

/* ---- the per-slot way, restated from the per-slot calls --------------------- */

int row_keylen(int row) { return row == 4 ? 32 : row == 5 ? 48 : 64; }

/* net2_burst_keytab_set_rx / _set_tx / _clear on a host entry:
 * net2_launch_keytab_set's midstates, keytab_set_kernel's stores */
void ref_key_op(Net2KeyEnt *e, int row, const net2_burst_keytab_op &o)
{
	using namespace net2::dev;
	const size_t kl = (size_t)row_keylen(row);
	HMid hm;
	if (o.op == NET2_BURST_TAB_CLEAR) {
		e->meta[0] = 0;
	} else if (o.op == NET2_BURST_TAB_RX) {
		const bool alt = o.rx.alt_hash_key != nullptr;
		if (!hmac_key_mids(row - 3, (const uint8_t *)o.rx.hash_key,
		    (const uint8_t *)o.rx.alt_hash_key, kl, &hm))
			fail("hmac_key_mids");
		memcpy(e->rx, hm.w, sizeof(e->rx));
		const uint32_t bits = NET2_KT_RX |
		    (o.rx.enc_alg != 0 ? NET2_KT_RX_ENC : 0) |
		    (alt ? NET2_KT_RX_ALT : 0) |
		    (alt && o.rx.alt_no_cutoff != 0 ? NET2_KT_RX_NOCUT : 0);
		e->meta[0] = (e->meta[0] & NET2_KT_TX_BITS) | bits;
		e->meta[1] = alt ? o.rx.alt_cutoff : 0;
		e->meta[2] = alt ? o.rx.rx_start : 0;
		e->meta[3] = 0;
	} else {
		if (!hmac_key_mids(row - 3, (const uint8_t *)o.tx_key, nullptr, kl, &hm))
			fail("hmac_key_mids");
		memcpy(e->tx, hm.w, sizeof(e->tx));
		e->meta[0] = (e->meta[0] & NET2_KT_RX_BITS) | NET2_KT_TX |
		    (o.tx_enc_alg != 0 ? NET2_KT_TX_ENC : 0);
	}
}

/* net2_burst_ciphertab_set_rx / _set_tx / _clear on a host entry */
void ref_cipher_op(Net2CipherEnt *e, const net2_burst_ciphertab_op &o)
{
	if (o.op == NET2_BURST_TAB_CLEAR) {
		memset(e, 0, sizeof(*e));
	} else if (o.op == NET2_BURST_TAB_RX) {
		const bool alt = o.rx.alt_hash_key != nullptr;
		aes_tab_fill_rx(e, (const uint8_t *)o.ck.enc_key,
		    alt ? (const uint8_t *)o.ck.alt_enc_key : nullptr,
		    o.rx.alt_no_cutoff != 0, o.rx.alt_cutoff, o.rx.rx_start);
	} else {
		aes_tab_fill_tx(e, (const uint8_t *)o.ck.enc_key);
	}
}

/* ---- the bulk way: reduce, records, bodies ---------------------------------- */

template <class R>
void check_zero(const R *r, const char *what)
{
	const uint8_t *p = (const uint8_t *)r;
	for (size_t i = 0; i < sizeof(R); i++)
		if (p[i] != 0)
			fail("%s: record byte %zu not zeroed", what, i);
}

void bulk_key(std::vector<Net2KeyEnt> &tab, int row,
    const std::vector<net2_burst_keytab_op> &ops, size_t per)
{
	std::vector<TabSlotOps> red;
	for (size_t at = 0; at < ops.size(); at += per) {
		const size_t m = std::min(per, ops.size() - at);
		tab_reduce(ops.data() + at, m, true, red);
		if (red.size() > m)
			fail("more records than ops");
		/* exact size: one record past the end is ASan's */
		std::unique_ptr<TabHashRec[]> recs(new TabHashRec[red.size()]);
		for (size_t i = 0; i < red.size(); i++) {
			for (size_t j = 0; j < i; j++)
				if (red[j].slot == red[i].slot)
					fail("two records of one slot in one launch");
			tab_hash_rec(ops.data() + at, red[i], (size_t)row_keylen(row),
			    &recs[i]);
		}
		for (size_t i = 0; i < red.size(); i++) {
			tab_u32x4 *q = reinterpret_cast<tab_u32x4 *>(&tab[recs[i].h.slot]);
			if (row == 4)
				keytab_apply<1, HostCompress>(q, &recs[i]);
			else if (row == 5)
				keytab_apply<2, HostCompress>(q, &recs[i]);
			else
				keytab_apply<3, HostCompress>(q, &recs[i]);
			check_zero(&recs[i], "key table");
		}
	}
}

void bulk_cipher(std::vector<Net2CipherEnt> &tab,
    const std::vector<net2_burst_ciphertab_op> &ops, size_t per)
{
	std::vector<TabSlotOps> red;
	for (size_t at = 0; at < ops.size(); at += per) {
		const size_t m = std::min(per, ops.size() - at);
		tab_reduce(ops.data() + at, m, false, red);
		std::unique_ptr<TabCipherRec[]> recs(new TabCipherRec[red.size()]);
		for (size_t i = 0; i < red.size(); i++) {
			for (size_t j = 0; j < i; j++)
				if (red[j].slot == red[i].slot)
					fail("two records of one slot in one launch");
			tab_cipher_rec(ops.data() + at, red[i], &recs[i]);
		}
		for (size_t i = 0; i < red.size(); i++) {
			tab_u32x4 *q = reinterpret_cast<tab_u32x4 *>(&tab[recs[i].h.slot]);
			ciphertab_apply(HostSbox{}, q, &recs[i]);
			check_zero(&recs[i], "cipher table");
		}
	}
}

/* ---- op lists ----------------------------------------------------------------- */

/* key material the ops point into; stable addresses (reserved up front) */
struct Keys {
	std::vector<std::vector<uint8_t>> pool;
	std::mt19937 rng;
	explicit Keys(unsigned seed) : rng(seed) { pool.reserve(4096); }
	const uint8_t *make(size_t n)
	{
		if (pool.size() == pool.capacity())
			fail("key pool too small");
		pool.emplace_back(n);	/* exact size: an over-read is ASan's */
		for (auto &b : pool.back())
			b = (uint8_t)rng();
		return pool.back().data();
	}
};

net2_burst_keytab_op key_op(Keys &k, int row, uint32_t slot, uint32_t op,
    bool alt, bool nocut, bool enc)
{
	net2_burst_keytab_op o = {};
	const size_t kl = (size_t)row_keylen(row);
	o.slot = slot;
	o.op = op;
	if (op == NET2_BURST_TAB_RX) {
		o.rx.hash_alg = row;
		o.rx.hash_key = k.make(kl);
		o.rx.hash_keylen = kl;
		o.rx.enc_alg = enc;
		if (alt) {
			o.rx.alt_hash_key = k.make(kl);
			o.rx.alt_hash_keylen = kl;
		}
		/* stored only with an alternate key; set either way */
		o.rx.alt_no_cutoff = nocut;
		o.rx.alt_cutoff = (uint32_t)k.rng();
		o.rx.rx_start = (uint32_t)k.rng();
	} else if (op == NET2_BURST_TAB_TX) {
		o.tx_key = k.make(kl);
		o.tx_keylen = kl;
		o.tx_enc_alg = enc;
	}
	return o;
}

net2_burst_ciphertab_op cipher_op(Keys &k, uint32_t slot, uint32_t op, bool alt,
    bool nocut)
{
	net2_burst_ciphertab_op o = {};
	o.slot = slot;
	o.op = op;
	if (op != NET2_BURST_TAB_CLEAR) {
		o.ck.enc_alg = NET2_ENC_AES256;
		o.ck.enc_key = k.make(32);
		o.ck.enc_keylen = 32;
	}
	if (op == NET2_BURST_TAB_RX) {
		o.rx.hash_alg = alt ? 6 : 0;
		if (alt) {
			o.rx.alt_hash_key = k.make(1);	/* only its presence counts */
			o.rx.alt_hash_keylen = 64;
			o.ck.alt_enc_key = k.make(32);
			o.ck.alt_enc_keylen = 32;
		}
		o.rx.alt_no_cutoff = nocut;
		o.rx.alt_cutoff = (uint32_t)k.rng();
		o.rx.rx_start = (uint32_t)k.rng();
	}
	return o;
}

template <class E>
void same_tables(const std::vector<E> &a, const std::vector<E> &b,
    const char *what, int iter)
{
	for (size_t s = 0; s < a.size(); s++)
		if (memcmp(&a[s], &b[s], sizeof(E)) != 0) {
			const uint8_t *x = (const uint8_t *)&a[s], *y = (const uint8_t *)&b[s];
			size_t at = 0;
			while (x[at] == y[at])
				at++;
			fail("%s, list %d: slot %zu differs at byte %zu (per-slot %02x, "
			    "bulk %02x)", what, iter, s, at, x[at], y[at]);
		}
}

const size_t kPer[] = { 1, 2, 7, 64, 65536 };

/* (b): every order of the sides on one slot, every key variant */
void fixed_cases()
{
	const uint32_t R = NET2_BURST_TAB_RX, T = NET2_BURST_TAB_TX,
	    C = NET2_BURST_TAB_CLEAR;
	const std::vector<std::vector<uint32_t>> orders = {
		{ R }, { T }, { C }, { R, T }, { T, R }, { R, C, T }, { T, C, R },
		{ R, T, C }, { C, R, T }, { R, R }, { T, T }, { R, C }, { T, C },
		{ R, T, C, R }, { R, T, C, T }, { R, C, R, T, C, T, R },
	};
	int iter = 0;
	for (int row = 4; row <= 6; row++)
	for (int variant = 0; variant < 8; variant++)
	for (const auto &ord : orders)
	for (size_t per : kPer) {
		const bool alt = variant & 1, nocut = variant & 2, enc = variant & 4;
		Keys k(1000u + (unsigned)iter);
		std::vector<net2_burst_keytab_op> ops;
		std::vector<net2_burst_ciphertab_op> cops;
		/* a neighbour slot set first: it must stay as it is */
		ops.push_back(key_op(k, row, 0, R, true, false, true));
		ops.push_back(key_op(k, row, 0, T, false, false, false));
		cops.push_back(cipher_op(k, 0, R, true, false));
		cops.push_back(cipher_op(k, 0, T, false, false));
		for (uint32_t op : ord) {
			ops.push_back(key_op(k, row, 1, op, alt, nocut, enc));
			cops.push_back(cipher_op(k, 1, op, alt, nocut));
		}
		std::vector<Net2KeyEnt> a(2), b(2);
		memset(a.data(), 0, 2 * sizeof(Net2KeyEnt));
		memset(b.data(), 0, 2 * sizeof(Net2KeyEnt));
		for (const auto &o : ops)
			ref_key_op(&a[o.slot], row, o);
		bulk_key(b, row, ops, per);
		same_tables(a, b, "key table, fixed", iter);
		if (row == 4) {
			std::vector<Net2CipherEnt> ca(2), cb(2);
			memset(ca.data(), 0, 2 * sizeof(Net2CipherEnt));
			memset(cb.data(), 0, 2 * sizeof(Net2CipherEnt));
			for (const auto &o : cops)
				ref_cipher_op(&ca[o.slot], o);
			bulk_cipher(cb, cops, per);
			same_tables(ca, cb, "cipher table, fixed", iter);
		}
		iter++;
	}
}

/* (a): random lists; the tables carry over from list to list */
void random_lists()
{
	std::mt19937 rng(20240607u);
	for (int row = 4; row <= 6; row++) {
		std::vector<Net2KeyEnt> a(16), b(16);
		std::vector<Net2CipherEnt> ca(16), cb(16);
		memset(a.data(), 0, 16 * sizeof(Net2KeyEnt));
		memset(b.data(), 0, 16 * sizeof(Net2KeyEnt));
		memset(ca.data(), 0, 16 * sizeof(Net2CipherEnt));
		memset(cb.data(), 0, 16 * sizeof(Net2CipherEnt));
		for (int iter = 0; iter < 40; iter++) {
			Keys k((unsigned)rng());
			const size_t n = iter == 0 ? 1 : iter == 1 ? 300 : 1 + rng() % 300;
			const uint32_t slots = iter == 0 ? 1 : iter == 1 ? 16 : 1 + rng() % 16;
			const size_t per = iter < 2 ? 65536 : kPer[rng() % 5];
			std::vector<net2_burst_keytab_op> ops;
			std::vector<net2_burst_ciphertab_op> cops;
			for (size_t i = 0; i < n; i++) {
				const uint32_t slot = rng() % slots;
				/* CLEAR is rarer, so set sides survive to be compared */
				const uint32_t pick = rng() % 8;
				const uint32_t op = pick == 0 ? NET2_BURST_TAB_CLEAR :
				    pick < 5 ? NET2_BURST_TAB_RX : NET2_BURST_TAB_TX;
				const unsigned v = rng();
				ops.push_back(key_op(k, row, slot, op, v & 1, v & 2, v & 4));
				if (row == 4)
					cops.push_back(cipher_op(k, slot, op, v & 1, v & 2));
			}
			for (const auto &o : ops)
				ref_key_op(&a[o.slot], row, o);
			bulk_key(b, row, ops, per);
			same_tables(a, b, "key table, random", iter);
			if (row == 4) {
				for (const auto &o : cops)
					ref_cipher_op(&ca[o.slot], o);
				bulk_cipher(cb, cops, per);
				same_tables(ca, cb, "cipher table, random", iter);
			}
		}
	}
}

/* aes_keysched.h against aes_sched.h, both directions */
void schedules()
{
	Keys k(7);
	for (int t = 0; t < 64; t++) {
		const uint8_t *key = k.make(32);
		AesSched enc, dec;
		aes256_enc_schedule(key, &enc);
		aes256_dec_schedule(key, &dec);
		alignas(16) uint8_t kb[32];
		memcpy(kb, key, 32);
		tab_u32x4 pe[NET2_TAB_CT_SCHED], pd[NET2_TAB_CT_SCHED];
		tab_aes_sched<false>(HostSbox{}, kb, pe);
		tab_aes_sched<true>(HostSbox{}, kb, pd);
		if (memcmp(pe, enc.w, sizeof(enc.w)) != 0)
			fail("encryption schedule, key %d", t);
		if (memcmp(pd, dec.w, sizeof(dec.w)) != 0)
			fail("decryption schedule, key %d", t);
	}
}

}	/* namespace */

int main()
{
	schedules();
	fixed_cases();
	random_lists();
	printf("test_tab_ops_host: ok\n");
	return 0;
}
