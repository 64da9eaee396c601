/*
 * net2_tab_ops.h -- the host half of the bulk table updates
 * (net2_burst_keytab_update / net2_burst_ciphertab_update,
 * include/net2/packet.h): the op list of one launch reduced to at most one
 * record per slot, and the records the update kernels (tab_kernels.hip) read
 * from page-locked staging.
 *
 * Plain C++17, no HIP header, so the reduction and the records are checked as
 * a stand-alone program under sanitizers (tests/cxx/test_tab_ops_host.cc).
 */
#ifndef NET2_TAB_OPS_H
#define NET2_TAB_OPS_H

#include "key_wipe.h"
#include "../../include/net2/packet.h"

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <unordered_map>
#include <vector>

/*
 * What one launch does to one slot.  Two ops of one launch on one slot must
 * not become two lanes writing one entry, so a slot's ops are folded, in
 * array order, into: clear first?, then the rx side from op `rx`, then the tx
 * side from op `tx` (-1: none).  The two sides own disjoint bytes and bits of
 * an entry, so their order does not matter; a CLEAR cancels what came before
 * it and not what follows.
 *
 * keep_dead: a CLEAR of the key table unsets the slot's bits and leaves its
 * other bytes as they are (keytab_set_kernel), so a set_rx / set_tx issued
 * before the last CLEAR still decides those bytes.  Such an op stays in the
 * record as a dead one (rx_live / tx_live false): its bytes are written, its
 * bits are not.  A CLEAR of the cipher table zeroes the whole entry, so there
 * an op before the last CLEAR is dropped.
 */
struct TabSlotOps {
	uint32_t slot;
	bool clear;
	bool rx_live, tx_live;
	long rx, tx;		/* index into the launch's ops, or -1 */
};

/* ops[0..n) -> recs, one per slot in order of first appearance.  Op: any
 * struct with `slot` and `op` (NET2_BURST_TAB_*); every op is a known one. */
template <class Op>
inline void tab_reduce(const Op *ops, size_t n, bool keep_dead,
    std::vector<TabSlotOps> &recs)
{
	std::unordered_map<uint32_t, size_t> at;
	recs.clear();
	for (size_t i = 0; i < n; i++) {
		auto it = at.find(ops[i].slot);
		if (it == at.end()) {
			it = at.emplace(ops[i].slot, recs.size()).first;
			recs.push_back(TabSlotOps{ ops[i].slot, false, false, false,
			    -1, -1 });
		}
		TabSlotOps &s = recs[it->second];
		if (ops[i].op == NET2_BURST_TAB_CLEAR) {
			s.clear = true;
			s.rx_live = s.tx_live = false;
			if (!keep_dead)
				s.rx = s.tx = -1;
		} else if (ops[i].op == NET2_BURST_TAB_RX) {
			s.rx = (long)i;
			s.rx_live = true;
		} else {
			s.tx = (long)i;
			s.tx_live = true;
		}
	}
}

/* ---- the records ----------------------------------------------------------- */

#define NET2_TR_CLEAR 0x01u	/* unset (cipher table: zero) the entry first */
#define NET2_TR_RX 0x02u	/* write the rx side from key[0] (and key[1]) */
#define NET2_TR_RX_LIVE 0x04u	/* ... and set its bits (else: a dead op) */
#define NET2_TR_RX_ALT 0x08u	/* key[1] is the alternate rx key */
#define NET2_TR_TX 0x10u	/* write the tx side from key[2] */
#define NET2_TR_TX_LIVE 0x20u	/* ... and set its bits */

/* The entries' meta bits as the records carry them (NET2_KT_*, sha2_launch.h,
 * and NET2_CT_*, aes_tab.h; net2_tabs.cpp and tab_kernels.hip assert that
 * they agree). */
#define NET2_TR_KT_RX 0x01u
#define NET2_TR_KT_TX 0x02u
#define NET2_TR_KT_RX_ALT 0x04u
#define NET2_TR_KT_RX_NOCUT 0x08u
#define NET2_TR_KT_RX_ENC 0x10u
#define NET2_TR_KT_TX_ENC 0x20u
#define NET2_TR_KT_RX_BITS 0x1du
#define NET2_TR_KT_TX_BITS 0x22u

/*
 * One slot of a launch as the kernel reads it: a 32-byte head, then the raw
 * keys zero-padded to a fixed size -- key[0] the rx key, key[1] the alternate
 * rx key, key[2] the tx key.  rx_bits / tx_bits: the meta bits a live side
 * sets; cutoff and rx_start are already 0 without an alternate key.  16-byte
 * aligned and a multiple of 16 bytes, so a lane reads and zeroes its record
 * in 16-byte pieces.
 */
struct alignas(16) TabRecHead {
	uint32_t slot, flags, rx_bits, tx_bits, cutoff, rx_start, pad[2];
};
struct alignas(16) TabHashRec {
	TabRecHead h;
	uint8_t key[3][64];	/* HMAC keys are 32, 48 or 64 bytes */
};
struct alignas(16) TabCipherRec {
	TabRecHead h;
	uint8_t key[3][32];	/* AES-256 */
};
static_assert(sizeof(TabHashRec) == 224 && sizeof(TabCipherRec) == 128,
    "the records of tab_kernels.hip");

inline uint32_t tab_rec_flags(const TabSlotOps &s, bool alt)
{
	return (s.clear ? NET2_TR_CLEAR : 0u) |
	    (s.rx >= 0 ? NET2_TR_RX : 0u) | (s.rx_live ? NET2_TR_RX_LIVE : 0u) |
	    (s.rx >= 0 && alt ? NET2_TR_RX_ALT : 0u) |
	    (s.tx >= 0 ? NET2_TR_TX : 0u) | (s.tx_live ? NET2_TR_TX_LIVE : 0u);
}

/* The key-table record of one reduced slot; the ops are checked ones, keylen
 * the row's key length.  Every byte of *r is written. */
inline void tab_hash_rec(const struct net2_burst_keytab_op *ops,
    const TabSlotOps &s, size_t keylen, TabHashRec *r)
{
	memset(r, 0, sizeof(*r));
	bool alt = false;
	if (s.rx >= 0) {
		const struct net2_burst_rx_keys &k = ops[s.rx].rx;
		alt = k.alt_hash_key != nullptr;
		memcpy(r->key[0], k.hash_key, keylen);
		if (alt)
			memcpy(r->key[1], k.alt_hash_key, keylen);
		r->h.rx_bits = NET2_TR_KT_RX |
		    (k.enc_alg != 0 ? NET2_TR_KT_RX_ENC : 0u) |
		    (alt ? NET2_TR_KT_RX_ALT : 0u) |
		    (alt && k.alt_no_cutoff != 0 ? NET2_TR_KT_RX_NOCUT : 0u);
		r->h.cutoff = alt ? k.alt_cutoff : 0u;
		r->h.rx_start = alt ? k.rx_start : 0u;
	}
	if (s.tx >= 0) {
		memcpy(r->key[2], ops[s.tx].tx_key, keylen);
		r->h.tx_bits = NET2_TR_KT_TX |
		    (ops[s.tx].tx_enc_alg != 0 ? NET2_TR_KT_TX_ENC : 0u);
	}
	r->h.slot = s.slot;
	r->h.flags = tab_rec_flags(s, alt);
}

/* The cipher-table record of one reduced slot (keys of 32 bytes).  rx_bits:
 * NET2_CT_RX_ALT / _NOCUT (the same values as the key table's). */
inline void tab_cipher_rec(const struct net2_burst_ciphertab_op *ops,
    const TabSlotOps &s, TabCipherRec *r)
{
	memset(r, 0, sizeof(*r));
	bool alt = false;
	if (s.rx >= 0) {
		const struct net2_burst_ciphertab_op &o = ops[s.rx];
		alt = o.rx.alt_hash_key != nullptr;
		memcpy(r->key[0], o.ck.enc_key, 32);
		if (alt)
			memcpy(r->key[1], o.ck.alt_enc_key, 32);
		r->h.rx_bits = NET2_TR_KT_RX | (alt ? NET2_TR_KT_RX_ALT : 0u) |
		    (alt && o.rx.alt_no_cutoff != 0 ? NET2_TR_KT_RX_NOCUT : 0u);
		r->h.cutoff = alt ? o.rx.alt_cutoff : 0u;
		r->h.rx_start = alt ? o.rx.rx_start : 0u;
	}
	if (s.tx >= 0) {
		memcpy(r->key[2], ops[s.tx].ck.enc_key, 32);
		r->h.tx_bits = NET2_TR_KT_TX;
	}
	r->h.slot = s.slot;
	r->h.flags = tab_rec_flags(s, alt);
}

#endif /* NET2_TAB_OPS_H */
