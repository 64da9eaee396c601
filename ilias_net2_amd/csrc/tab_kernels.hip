/*
 * tab_kernels.hip -- bulk updates of the two device tables of the bursts over
 * many connections (net2_burst_keytab_update / net2_burst_ciphertab_update,
 * include/net2/packet.h) for gfx950: one lane per connection slot prepares
 * that slot's keys on the device -- HMAC midstates, AES-256 schedules -- from
 * a record of raw keys in page-locked staging (net2_tab_ops.h) and stores the
 * entry as the per-slot kernels would have left it.  The per-record bodies are
 * tab_update.h's; here are the compressions and the S-box they run with, the
 * slot bound and the launchers.
 *
 * A translation unit of its own, as aes_kernels.hip: the SHA-2 kernels'
 * object, and with it net2_sha2_build_id(), does not change.
 */
#include "sha2_device.h"
#include "sha2_launch.h"
#include "tab_launch.h"
#include "tab_update.h"

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

using namespace net2::dev;

static_assert(sizeof(Net2KeyEnt) == 16 * NET2_TAB_KT_PIECES &&
    offsetof(Net2KeyEnt, rx) == 16 && offsetof(Net2KeyEnt, tx) ==
    16 * (1 + 4 * NET2_TAB_KT_MID), "the key-table entry in pieces");
static_assert(NET2_TR_KT_RX == NET2_KT_RX && NET2_TR_KT_TX == NET2_KT_TX &&
    NET2_TR_KT_RX_ALT == NET2_KT_RX_ALT && NET2_TR_KT_RX_NOCUT == NET2_KT_RX_NOCUT &&
    NET2_TR_KT_RX_ENC == NET2_KT_RX_ENC && NET2_TR_KT_TX_ENC == NET2_KT_TX_ENC &&
    NET2_TR_KT_RX_BITS == NET2_KT_RX_BITS && NET2_TR_KT_TX_BITS == NET2_KT_TX_BITS,
    "the records' bits are the key table's");
static_assert(NET2_TR_KT_RX == NET2_CT_RX && NET2_TR_KT_TX == NET2_CT_TX &&
    NET2_TR_KT_RX_ALT == NET2_CT_RX_ALT && NET2_TR_KT_RX_NOCUT == NET2_CT_RX_NOCUT,
    "... and the cipher table's");
static_assert(sizeof(Net2CipherEnt) == NET2_AES_TAB_ENT_BYTES, "aes_launch.h");

namespace {

constexpr unsigned TAB_WG = 256;

/* The compressions of sha2_device.h on registers (SHA-512's round constants
 * from the workgroup's LDS copy: k512_lds_fill at kernel entry). */
struct DevCompress {
	__device__ __forceinline__ static void c256(uint32_t (&st)[8],
	    uint32_t (&m)[16])
	{
		compress256(st, m);
	}
	__device__ __forceinline__ static void c512(uint64_t (&st)[8],
	    uint64_t (&m)[16])
	{
		compress512(st, m);
	}
};

/*
 * The record of lane g and the entry of its slot.  The host has checked the
 * slot; it is checked again here and clamped to entry 0 before an address is
 * formed from it (as keytab_ent does), and a record out of range is zeroed
 * without touching the table.
 */
template <int HALG>
__global__ __launch_bounds__(TAB_WG) void keytab_update_kernel(Net2KeyEnt *tab,
    uint32_t slots, TabHashRec *recs, uint32_t n)
{
	const uint32_t g = blockIdx.x * TAB_WG + threadIdx.x;
	if (HALG != NET2_ALG_SHA256)
		k512_lds_fill();	/* (synchronises the workgroup) */
	if (g >= n)
		return;
	TabHashRec *r = recs + g;
	const uint32_t slot = r->h.slot;
	const bool in = slot < slots;
	tab_u32x4 *q = reinterpret_cast<tab_u32x4 *>(tab + (in ? slot : 0u));
	if (in)
		keytab_apply<HALG, DevCompress>(q, r);
	else
		tab_rec_zero(r);
}

/* The forward S-box, once per workgroup in LDS (the InvMixColumns step of the
 * decryption schedules needs no table). */
__device__ const uint8_t d_sbox[256] = NET2_AES_SBOX_INIT;

struct LdsSbox {
	const uint8_t *p;
	__device__ __forceinline__ uint32_t operator()(uint32_t x) const
	{
		return p[x];
	}
};

__global__ __launch_bounds__(TAB_WG) void ciphertab_update_kernel(
    Net2CipherEnt *tab, uint32_t slots, TabCipherRec *recs, uint32_t n)
{
	__shared__ uint8_t sbox[256];
	const uint32_t g = blockIdx.x * TAB_WG + threadIdx.x;
	for (unsigned i = threadIdx.x; i < 256; i += TAB_WG)
		sbox[i] = d_sbox[i];
	__syncthreads();
	if (g >= n)
		return;
	TabCipherRec *r = recs + g;
	const uint32_t slot = r->h.slot;
	const bool in = slot < slots;
	tab_u32x4 *q = reinterpret_cast<tab_u32x4 *>(tab + (in ? slot : 0u));
	if (in)
		ciphertab_apply(LdsSbox{ sbox }, q, r);
	else
		tab_rec_zero(r);
}

}	/* namespace */

hipError_t net2_launch_keytab_update(int alg, Net2KeyEnt *tab, uint32_t slots,
    void *d_recs, uint32_t n, hipStream_t s)
{
	const int halg = alg - 3;	/* HMAC row -> SHA row */
	if (halg < NET2_ALG_SHA256 || halg > NET2_ALG_SHA512 || tab == nullptr ||
	    d_recs == nullptr)
		return hipErrorInvalidValue;
	if (n == 0)
		return hipSuccess;
	const dim3 grid((n + TAB_WG - 1) / TAB_WG);
	TabHashRec *recs = (TabHashRec *)d_recs;
	if (halg == NET2_ALG_SHA256)
		keytab_update_kernel<NET2_ALG_SHA256><<<grid, TAB_WG, 0, s>>>(tab,
		    slots, recs, n);
	else if (halg == NET2_ALG_SHA384)
		keytab_update_kernel<NET2_ALG_SHA384><<<grid, TAB_WG, 0, s>>>(tab,
		    slots, recs, n);
	else
		keytab_update_kernel<NET2_ALG_SHA512><<<grid, TAB_WG, 0, s>>>(tab,
		    slots, recs, n);
	return hipGetLastError();
}

hipError_t net2_launch_ciphertab_update(Net2CipherEnt *tab, uint32_t slots,
    void *d_recs, uint32_t n, hipStream_t s)
{
	if (tab == nullptr || d_recs == nullptr)
		return hipErrorInvalidValue;
	if (n == 0)
		return hipSuccess;
	ciphertab_update_kernel<<<dim3((n + TAB_WG - 1) / TAB_WG), TAB_WG, 0, s>>>(
	    tab, slots, (TabCipherRec *)d_recs, n);
	return hipGetLastError();
}
