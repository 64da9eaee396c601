/*
 * aes_tab.h -- the entry of the device cipher-key table (struct
 * net2_burst_ciphertab, include/net2/packet.h) and how one is filled from a
 * connection's keys.  The _mc cipher kernels (aes_kernels.hip) read entries
 * from global memory; aes_tab_set_kernel there is the only writer.
 *
 * Host code only, plain C++17, no HIP header: aes_kernels.hip includes it
 * (through aes_cbc.h, which has the kernels' look-ups), and so do the host
 * checks (tests/cxx/test_aes_tab_host.cc).  The functions have internal
 * linkage, as those of aes_sched.h; inline, so an includer that fills no
 * entry gets no warning.
 */
#ifndef NET2_AES_TAB_H
#define NET2_AES_TAB_H

#include "aes_sched.h"

/*
 * One connection, 736 bytes, 16-byte aligned so every piece moves as 16-byte
 * accesses:
 *   +0    meta[0] NET2_CT_* bits, meta[1] cutoff, meta[2] rx_start, meta[3] 0
 *   +16   dec[0]  the active rx key's schedule (aes256_dec_schedule), 60 words
 *   +256  dec[1]  the alternate rx key's (NET2_CT_RX_ALT), else zero
 *   +496  enc     the tx key's schedule (aes256_enc_schedule)
 * The rx side is meta[1..2], the rx bits and dec; the tx side the tx bit and
 * enc.  Setting one side leaves the other as it is.
 */
#define NET2_CT_RX 0x01u		/* the rx side is set */
#define NET2_CT_TX 0x02u		/* the tx side is set */
#define NET2_CT_RX_ALT 0x04u		/* an alternate rx key is installed */
#define NET2_CT_RX_NOCUT 0x08u		/* ... without a cutoff */
#define NET2_CT_RX_BITS (NET2_CT_RX | NET2_CT_RX_ALT | NET2_CT_RX_NOCUT)
#define NET2_CT_TX_BITS NET2_CT_TX
struct alignas(16) Net2CipherEnt {
	uint32_t meta[4];
	uint32_t dec[2][NET2_AES_RKWORDS];
	uint32_t enc[NET2_AES_RKWORDS];
};
static_assert(sizeof(Net2CipherEnt) == 736, "the entry of aes_launch.h");

namespace {

/*
 * The rx side of *e from a connection's rx cipher keys: key (32 bytes), the
 * alternate key or NULL, and with one the choice's state (net2_ck_rx_key,
 * src/conn_keys.c:447-476; without one the three are stored as 0).
 */
inline void aes_tab_fill_rx(Net2CipherEnt *e, const uint8_t *key,
    const uint8_t *alt_key, bool no_cutoff, uint32_t cutoff, uint32_t rx_start)
{
	AesSched ks;
	const bool alt = alt_key != nullptr;
	aes256_dec_schedule(key, &ks);
	for (int i = 0; i < NET2_AES_RKWORDS; i++)
		e->dec[0][i] = ks.w[i];
	if (alt)
		aes256_dec_schedule(alt_key, &ks);
	for (int i = 0; i < NET2_AES_RKWORDS; i++)
		e->dec[1][i] = alt ? ks.w[i] : 0u;
	e->meta[0] = (e->meta[0] & NET2_CT_TX_BITS) | NET2_CT_RX |
	    (alt ? NET2_CT_RX_ALT : 0u) | (alt && no_cutoff ? NET2_CT_RX_NOCUT : 0u);
	e->meta[1] = alt ? cutoff : 0u;
	e->meta[2] = alt ? rx_start : 0u;
	e->meta[3] = 0;
	volatile uint32_t *z = ks.w;
	for (int i = 0; i < NET2_AES_RKWORDS; i++)
		z[i] = 0;
}

/* The tx side of *e: the key the transmitter encrypts with. */
inline void aes_tab_fill_tx(Net2CipherEnt *e, const uint8_t *key)
{
	AesSched ks;
	aes256_enc_schedule(key, &ks);
	for (int i = 0; i < NET2_AES_RKWORDS; i++)
		e->enc[i] = ks.w[i];
	e->meta[0] = (e->meta[0] & NET2_CT_RX_BITS) | NET2_CT_TX;
	volatile uint32_t *z = ks.w;
	for (int i = 0; i < NET2_AES_RKWORDS; i++)
		z[i] = 0;
}

}	/* namespace */

#endif /* NET2_AES_TAB_H */
