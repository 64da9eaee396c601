/*
 * aes_kernels.hip -- the payload cipher of the packet bursts:
 * net2_packet_decrypt_burst / net2_packet_encrypt_burst (include/net2/packet.h),
 * the reference's "aes256" (AES-256-CBC with PKCS#7 padding, src/enc.c:70-74,
 * :316-413) as packet.n2t applies it to a datagram's payload (:263-292 RX,
 * :375-398 TX).
 *
 * One lane per datagram, as in the hash bursts: on TX the CBC chain is serial
 * within a datagram anyway, and RX takes the same shape so both directions
 * share the block code (aes_device.h) and the tests.  Small RX bursts take
 * the wave form instead (one wave per datagram, further down), small TX
 * bursts the quad form (four lanes per datagram, after it).
 *
 * What a lane does with its datagram -- the burst's arguments, the prep step
 * that settles what needs no cipher, the CBC chain of each direction, the
 * connection checks of the _mc calls -- is aes_cbc.h, host and device code
 * that the host tests run as it stands.  This file keeps what is device-only:
 * the LDS table and the round-key accessors, the ranking, the kernels (each
 * lane kernel: prep, rank, table, one call of its direction's chain under its
 * key source), the wave form of RX, the quad form of TX, the table update and
 * the launchers.
 *
 * LDS layout.  A workgroup is 256 lanes and holds one T-table (Te0 forward,
 * Td0 inverse) replicated 32 times: entry x for lane l is dword
 * x * 32 + (l & 31), 32 KiB.  A ds_read_b32 is served per half-wave of 32
 * lanes over 32 banks, bank = dword index mod 32 = l & 31: whatever bytes
 * the lanes look up, every lane of a half-wave reads its own bank, so no
 * lookup conflicts and the time of a lookup does not depend on the data.
 * The other three tables of a round are rotations of the first
 * (v_alignbit_b32), the last round's S-box comes out of the same entries
 * (aes_device.h).  The table is built at kernel start from the S-box with
 * ds_write_b32 (lane t writes dwords t, t + 256, ...: consecutive banks).
 *
 * Round keys travel in the launch's arguments.  With one key per burst
 * (encrypt; decrypt without an alternate rx key) they are wave-uniform and
 * stay in scalar registers.  With an alternate rx key installed the choice
 * is per datagram, so that instance copies both schedules to LDS (the second
 * 272 bytes after the first: another bank) and each lane reads its own.
 * The _mc kernels (further down) take each datagram's keys from its own
 * connection's entry of a device table instead.
 *
 * Payloads start at 8, 40, 56 or 72 bytes past an arbitrary offset, so blocks
 * are moved with 16-byte global accesses at byte alignment (the unaligned
 * access mode of gfx9+ global memory that the hash kernels rely on as well).
 * A lane touches only bytes of its own datagram's payload.
 */
#include "aes_cbc.h"
#include "aes_device.h"
#include "aes_launch.h"
#include "aes_quad.h"
#include "aes_sched.h"
#include "aes_tab.h"
#include "aes_wave.h"
#include "key_wipe.h"

#include <stddef.h>
#include <string.h>

namespace {

constexpr int AES_WG = 256;		/* lanes per workgroup = table entries */
/* copies of the table: one per bank (-DNET2_AES_REP=1, a power of two: the
 * plain table, for A/B runs) */
#ifndef NET2_AES_REP
#define NET2_AES_REP 32
#endif
constexpr int AES_REP = NET2_AES_REP;
constexpr int AES_RK_STRIDE = 68;	/* words between the two LDS schedules */

/* the S-box and its inverse, for the kernels' tables (aes_sched.h) */
__device__ const Sbox d_sbox[2] = { make_sbox(false), make_sbox(true) };

template <int NK>
struct AesKeys {
	AesSched k[NK];
};

/* ---- device ------------------------------------------------------------------ */

/* The lane's copy of the replicated table: entry x at p[x * 32]. */
struct LdsTab {
	const uint32_t *p;
	__device__ __forceinline__ uint32_t operator()(uint32_t x) const
	{
		return p[x * AES_REP];
	}
};

/* Round keys out of the launch's arguments (wave-uniform) or out of LDS. */
struct RkArgs {
	const AesSched &k;
	__device__ __forceinline__ uint32_t operator()(int i) const
	{
		return k.w[i];
	}
};
struct RkLds {
	const uint32_t *p;
	__device__ __forceinline__ uint32_t operator()(int i) const
	{
		return p[i];
	}
};

/*
 * The workgroup's table (see the head of this file).  Every lane of the
 * workgroup takes part; ends with a barrier.
 */
template <bool INV>
__device__ __forceinline__ void aes_build_table(uint32_t *tab)
{
	for (uint32_t d = threadIdx.x; d < 256 * AES_REP; d += AES_WG) {
		const uint32_t s = d_sbox[INV].v[d / AES_REP];
		tab[d] = INV ? aes_td0_word(s) : aes_te0_word(s);
	}
	__syncthreads();
}

/*
 * With an alternate rx key the choice is per datagram: the launch's two
 * schedules go to LDS (lanes 0..59 the active one, 64..123 the alternate one;
 * published by the table build's barrier) and a datagram's pick is an address
 * there (net2_ck_rx_key, src/conn_keys.c:447-476, as the HMAC step chose).
 */
__device__ __forceinline__ void stage_rx_keys(uint32_t *rks,
    const AesKeys<2> &keys)
{
	const uint32_t t = threadIdx.x;
	if (t < NET2_AES_RKWORDS)
		rks[t] = keys.k[0].w[t];
	else if (t >= 64 && t < 64 + NET2_AES_RKWORDS)
		rks[AES_RK_STRIDE + t - 64] = keys.k[1].w[t - 64];
}

__device__ __forceinline__ const uint32_t *staged_rx_key(const uint32_t *rks,
    const AesBurstArgs &a, uint64_t i, uint32_t fl)
{
	const bool alt = aes_rx_alt(true, a.no_cutoff != 0, fl, a.seq[i], a.cutoff,
	    a.rx_start);
	return rks + (alt ? AES_RK_STRIDE : 0);
}

/*
 * Lanes by work.  A burst mixes short and long datagrams, and a wave runs as
 * long as its longest lane: in arrival order nearly every wave of the
 * {64, 512, 1500}-byte mix holds a long one.  So before the cipher a
 * workgroup ranks its 256 datagrams by block count (a counting rank over LDS,
 * about the instructions of half a block per lane) and lane t takes the
 * datagram of rank t: the workgroup's waves then hold datagrams of like
 * length and the short waves retire early.  nb: the blocks of the calling
 * lane's own datagram (0: no cipher work).  Returns the workgroup-relative
 * index of the datagram this lane is to process and, in *nb_out, its block
 * count.  scratch: 2 * AES_WG words of LDS, free again on return (the table
 * is built over them); every lane of the workgroup takes part.
 */
__device__ __forceinline__ uint32_t lanes_by_work(uint32_t *scratch,
    uint32_t nb, uint32_t *nb_out)
{
	const uint32_t t = threadIdx.x;
	uint32_t rank = 0;

	scratch[t] = nb;
	__syncthreads();
	for (uint32_t u = 0; u < AES_WG; u++) {
		const uint32_t k = scratch[u];
		rank += (k < nb || (k == nb && u < t)) ? 1u : 0u;
	}
	scratch[AES_WG + rank] = t;
	__syncthreads();
	const uint32_t me = scratch[AES_WG + t];
	*nb_out = scratch[me];
	__syncthreads();
	return me;
}

/*
 * The lane kernels.  Each is four steps: the prep of the datagram in the
 * lane's own position (aes_cbc.h: what needs no cipher is settled there), the
 * ranking, the table, then the direction's one chain (cbc_decrypt_lane /
 * cbc_encrypt_lane, aes_cbc.h) for the datagram the lane drew, under the
 * kernel's key source.
 */
template <bool ALT>
__global__ __launch_bounds__(AES_WG) void aes_cbc_decrypt_kernel(
    const AesBurstArgs a, const AesKeys<ALT ? 2 : 1> keys)
{
	__shared__ uint32_t tab[256 * AES_REP > 2 * AES_WG ? 256 * AES_REP :
	    2 * AES_WG];
	__shared__ __attribute__((aligned(16))) uint32_t
	    rks[ALT ? 2 * AES_RK_STRIDE : 4];

	if constexpr (ALT)
		stage_rx_keys(rks, keys);
	const uint64_t first = (uint64_t)blockIdx.x * AES_WG;
	uint32_t nb;
	const uint64_t i = first + lanes_by_work(tab,
	    decrypt_prep(a, first + threadIdx.x), &nb);
	aes_build_table<true>(tab);
	if (nb == 0)
		return;

	const uint32_t fl = a.flags[i];
	const LdsTab T = { tab + (threadIdx.x & (AES_REP - 1)) };
	if constexpr (ALT) {
		const RkLds K = { staged_rx_key(rks, a, i, fl) };
		cbc_decrypt_lane(a, i, nb, fl, T, K);
	} else {
		const RkArgs K = { keys.k[0] };
		cbc_decrypt_lane(a, i, nb, fl, T, K);
	}
}

__global__ __launch_bounds__(AES_WG) void aes_cbc_encrypt_kernel(
    const AesBurstArgs a, const AesKeys<1> keys)
{
	__shared__ uint32_t tab[256 * AES_REP > 2 * AES_WG ? 256 * AES_REP :
	    2 * AES_WG];

	const uint64_t first = (uint64_t)blockIdx.x * AES_WG;
	uint32_t nb;
	const uint64_t i = first + lanes_by_work(tab,
	    encrypt_prep(a, first + threadIdx.x), &nb);
	aes_build_table<false>(tab);
	if (nb == 0)
		return;

	const LdsTab T = { tab + (threadIdx.x & (AES_REP - 1)) };
	const RkArgs K = { keys.k[0] };
	cbc_encrypt_lane(a, i, nb, T, K);
}

/*
 * The _mc kernels (AesMcArgs and the connection checks: aes_cbc.h).  After
 * the ranking lane t looks up the entry of the datagram it owns and takes its
 * schedule from there (RX: ciphertab_rx_key).
 *
 * Round keys: a lane loads the 60 words of its schedule once, as fifteen
 * 16-byte global loads, and holds them in VGPRs for all its blocks (RkRegs;
 * the rounds are unrolled, so every index is a constant).  With
 * -DNET2_AES_MC_REREAD=1 it reads them from the table again in every block
 * instead (RkGlobal): fewer registers, fifteen scattered loads per lane and
 * block.  DESIGN.md 5.5.4 has both forms' numbers.
 */
#ifndef NET2_AES_MC_REREAD
#define NET2_AES_MC_REREAD 0
#endif

/* Round keys out of a table entry's schedule (16-byte aligned): loaded once
 * into the lane's registers, or read from the table at every use. */
struct RkRegs {
	uint32_t w[NET2_AES_RKWORDS];
	__device__ __forceinline__ explicit RkRegs(const uint32_t *p)
	{
		const u32x4 *q = reinterpret_cast<const u32x4 *>(p);
#pragma unroll
		for (int k = 0; k < NET2_AES_RKWORDS / 4; k++) {
			const u32x4 v = q[k];
			w[4 * k] = v.x;
			w[4 * k + 1] = v.y;
			w[4 * k + 2] = v.z;
			w[4 * k + 3] = v.w;
		}
	}
	__device__ __forceinline__ uint32_t operator()(int i) const
	{
		return w[i];
	}
};
struct RkGlobal {
	const uint32_t *p;	/* a schedule in the table, 16-byte aligned */
	__device__ __forceinline__ explicit RkGlobal(const uint32_t *q) :
	    p((const uint32_t *)__builtin_assume_aligned(q, 16)) {}
	__device__ __forceinline__ uint32_t operator()(int i) const
	{
		return p[i];
	}
};
#if NET2_AES_MC_REREAD
typedef RkGlobal RkMc;
#else
typedef RkRegs RkMc;
#endif

__global__ __launch_bounds__(AES_WG) void aes_cbc_decrypt_mc_kernel(
    const AesMcArgs m)
{
	__shared__ uint32_t tab[256 * AES_REP > 2 * AES_WG ? 256 * AES_REP :
	    2 * AES_WG];

	const AesBurstArgs &a = m.b;
	const uint64_t first = (uint64_t)blockIdx.x * AES_WG;
	uint32_t nb;
	const uint64_t i = first + lanes_by_work(tab,
	    decrypt_mc_prep(m, first + threadIdx.x), &nb);
	aes_build_table<true>(tab);
	if (nb == 0)
		return;

	const uint32_t fl = a.flags[i];
	const LdsTab T = { tab + (threadIdx.x & (AES_REP - 1)) };
	const RkMc K(ciphertab_rx_key(m, i, fl));
	cbc_decrypt_lane(a, i, nb, fl, T, K);
}

__global__ __launch_bounds__(AES_WG) void aes_cbc_encrypt_mc_kernel(
    const AesMcArgs m)
{
	__shared__ uint32_t tab[256 * AES_REP > 2 * AES_WG ? 256 * AES_REP :
	    2 * AES_WG];

	const uint64_t first = (uint64_t)blockIdx.x * AES_WG;
	uint32_t nb;
	const uint64_t i = first + lanes_by_work(tab,
	    encrypt_mc_prep(m, first + threadIdx.x), &nb);
	aes_build_table<false>(tab);
	if (nb == 0)
		return;

	const LdsTab T = { tab + (threadIdx.x & (AES_REP - 1)) };
	bool in;
	const RkMc K(ciphertab_ent(m, i, &in)->enc);
	cbc_encrypt_lane(m.b, i, nb, T, K);
}

/*
 * The wave form of RX, for small bursts (net2_aes_burst_limits): one wave per
 * datagram, the lanes taking the datagram's blocks 64 to a pass -- CBC
 * decryption has no serial chain, block b needs ciphertext blocks b and b - 1
 * only.  With one lane per datagram a burst of a few thousand datagrams is
 * at most one wave per SIMD and lasts as long as its longest lane, 89 blocks
 * one after the other for a 1,424-byte ciphertext; here that datagram is two
 * passes.  aes_wave.h has the schedule (which block a lane takes in a pass,
 * the order of the passes, a block's prev, when the padding verdict is taken)
 * and why that order is safe in place; this kernel follows it call by call.
 *
 * A workgroup is AES_WAVES waves and builds the one table the lane form
 * builds, lane l of a wave on bank l & 31: a ds_read_b32 is served per
 * half-wave of 32 lanes over 32 banks and every lane of a half-wave reads its
 * own bank, so here too no lookup conflicts and the time of a lookup does
 * not depend on key or data.  Idle lanes of a pass (blocks past the end) run
 * the rounds on zeros rather than branch around them.  The table build ends
 * in the kernel's only barrier and comes before anything that can end a
 * wave: waves without a datagram or without cipher work reach it like the
 * others.  Wave w of workgroup g takes datagrams (g * per_wave + k) *
 * AES_WAVES + w, k = 0 .. per_wave - 1: the launch raises per_wave with n so
 * that a larger burst builds fewer tables.
 *
 * What is per datagram is per wave, so wave-uniform: the index (readfirstlane
 * of the wave number, which lets the compiler keep offsets, lengths and flags
 * in scalar registers), the prep step (lane 0 runs the lane form's
 * decrypt_prep / decrypt_mc_prep, the block count is broadcast) and the key
 * choice.  The three key sources share the body: one key in the launch's
 * arguments, read from there (KS_ONE); the active and the alternate key in
 * the arguments, both copied to LDS as in the lane form and the wave's pick
 * by aes_rx_alt moved to scalar registers (KS_ALT); the cipher-key table,
 * the datagram's entry looked up as in the _mc lane form and the picked
 * schedule moved to scalar registers (KS_TAB).
 *
 * A lane touches only whole blocks of its datagram's payload, with the
 * lane form's 16-byte accesses at byte alignment and 64-bit offsets.
 */
constexpr int AES_WAVES = AES_WG / 64;	/* datagrams per workgroup and step */
enum { KS_ONE = 0, KS_ALT = 1, KS_TAB = 2 };

template <int KS> struct AesWaveArgs;
template <> struct AesWaveArgs<KS_ONE> {
	AesBurstArgs b;
	AesKeys<1> keys;
	__device__ __forceinline__ const AesBurstArgs &burst() const { return b; }
};
template <> struct AesWaveArgs<KS_ALT> {
	AesBurstArgs b;
	AesKeys<2> keys;
	__device__ __forceinline__ const AesBurstArgs &burst() const { return b; }
};
template <> struct AesWaveArgs<KS_TAB> {
	AesMcArgs m;
	__device__ __forceinline__ const AesBurstArgs &burst() const { return m.b; }
};

/* A schedule every lane of the wave shares, out of LDS or out of a table
 * entry (16-byte aligned either way), held in scalar registers. */
struct RkWave {
	uint32_t w[NET2_AES_RKWORDS];
	__device__ __forceinline__ explicit RkWave(const uint32_t *p)
	{
		const u32x4 *q = reinterpret_cast<const u32x4 *>(p);
#pragma unroll
		for (int k = 0; k < NET2_AES_RKWORDS / 4; k++) {
			const u32x4 v = q[k];
			w[4 * k] = __builtin_amdgcn_readfirstlane(v.x);
			w[4 * k + 1] = __builtin_amdgcn_readfirstlane(v.y);
			w[4 * k + 2] = __builtin_amdgcn_readfirstlane(v.z);
			w[4 * k + 3] = __builtin_amdgcn_readfirstlane(v.w);
		}
	}
	__device__ __forceinline__ uint32_t operator()(int i) const
	{
		return w[i];
	}
};

/*
 * Datagram i, nb >= 1 blocks, by the calling wave (every lane calls; i, nb,
 * fl and the key are wave-uniform).  The passes of aes_wave.h, last pass
 * first.  In every run a lane loads its block and its prev, decrypts, and
 * stores: its store data depends on both loads, and the wave runs in
 * lockstep, so within a run all loads are done before the first store; the
 * runs before it stored to later passes' blocks only.  So in place every
 * ciphertext block is in registers before a store can overwrite it.  The
 * padding verdict falls in the first run, before the datagram's first store:
 * a BAD datagram is never written.
 */
template <class K>
__device__ __forceinline__ void decrypt_by_wave(const AesBurstArgs &a,
    uint64_t i, uint32_t nb, uint32_t fl, const LdsTab &T, const K &rk,
    uint32_t lane)
{
	const uint64_t off = a.offsets[i] + payload_at(fl, a.hashlen);
	const uint8_t *src = a.in + off;
	uint8_t *dst = a.out + off;
	const uint32_t runs = aes_wave_passes(nb);
	uint32_t pad = 0;

	for (uint32_t r = 0; r < runs; r++) {
		const uint32_t b = aes_wave_block(aes_wave_pass_of_run(nb, r), lane);
		const bool mine = b < nb;
		uint32_t x[4] = { 0, 0, 0, 0 }, prev[4] = { 0, 0, 0, 0 };
		if (mine) {
			ld16(src + 16 * (uint64_t)b, x);
			if (aes_wave_prev_is_iv(b))
				ld16(a.iv + NET2_AES_BLOCK * i, prev);
			else
				ld16(src + 16 * (uint64_t)aes_wave_prev(b), prev);
		}
		aes_block<true>(T, rk, x);
#pragma unroll
		for (int k = 0; k < 4; k++)
			x[k] ^= prev[k];
		if (r == NET2_AES_WAVE_VERDICT_RUN) {
			/* the last block's lane tells the wave */
			pad = __builtin_amdgcn_readlane(aes_pkcs7_pad(x),
			    aes_wave_verdict_lane(nb));
			if (pad == 0)
				break;
		}
		if (mine)
			st16(dst + 16 * (uint64_t)b, x);
	}
	if (lane == 0) {
		if (pad == 0)
			a.result[i] = PKT_BAD;
		a.plen[i] = pad != 0 ? 16 * nb - pad : 0u;
	}
}

template <int KS>
__global__ __launch_bounds__(AES_WG) void aes_cbc_decrypt_wave_kernel(
    const AesWaveArgs<KS> w, const uint32_t per_wave)
{
	__shared__ uint32_t tab[256 * AES_REP];
	__shared__ __attribute__((aligned(16))) uint32_t
	    rks[KS == KS_ALT ? 2 * AES_RK_STRIDE : 4];

	const AesBurstArgs &a = w.burst();
	const uint32_t t = threadIdx.x;
	if constexpr (KS == KS_ALT)
		stage_rx_keys(rks, w.keys);
	/* the one barrier (it publishes rks as well): before any wave can end */
	aes_build_table<true>(tab);

	const uint32_t lane = t & 63u;
	const uint32_t wv = __builtin_amdgcn_readfirstlane(t >> 6);
	const LdsTab T = { tab + (t & (AES_REP - 1)) };
	for (uint32_t k = 0; k < per_wave; k++) {
		const uint64_t i = ((uint64_t)blockIdx.x * per_wave + k) * AES_WAVES + wv;
		if (i >= a.n)
			break;
		/* lane 0 settles what needs no cipher, as a lane of the lane form */
		uint32_t nb = 0;
		if (lane == 0) {
			if constexpr (KS == KS_TAB)
				nb = decrypt_mc_prep(w.m, i);
			else
				nb = decrypt_prep(a, i);
		}
		nb = __builtin_amdgcn_readfirstlane(nb);
		if (nb == 0)
			continue;
		const uint32_t fl = a.flags[i];
		if constexpr (KS == KS_ONE) {
			const RkArgs K = { w.keys.k[0] };
			decrypt_by_wave(a, i, nb, fl, T, K, lane);
		} else if constexpr (KS == KS_ALT) {
			const RkWave K(staged_rx_key(rks, a, i, fl));
			decrypt_by_wave(a, i, nb, fl, T, K, lane);
		} else {
			const RkWave K(ciphertab_rx_key(w.m, i, fl));
			decrypt_by_wave(a, i, nb, fl, T, K, lane);
		}
	}
}

/*
 * The quad form of TX, for small bursts (net2_aes_encrypt_limits): four
 * adjacent lanes per datagram, one column of the state each -- 16 datagrams a
 * wave, AES_QUADS a workgroup.  CBC encryption is serial from block to block,
 * so the wave form above does not transfer; inside a block a round's four
 * columns are independent, and with one lane per datagram a small burst lasts
 * as long as 89 blocks of sixteen look-ups a round, one after the other.  Here
 * a lane's chain is four look-ups a round, and the three columns it needs
 * from its neighbours come by three DPP moves (quad_perm; no LDS, no
 * barrier).  aes_quad.h has the schedule -- which column and which schedule
 * words a lane owns, the word it contributes to a block, the steps of a
 * block -- and this kernel follows it call by call.
 *
 * A DPP move reads its neighbours' registers as they are in that instruction,
 * so all four lanes of a quad must be in the same control flow wherever one
 * executes.  Everything that decides a quad's control flow is therefore a
 * function of its datagram alone: the index, hence the end of the burst; the
 * block count, which lane 0 of the quad works out (the lane form's
 * encrypt_prep / encrypt_mc_prep, which settles what needs no cipher) and a
 * quad_perm [0,0,0,0] makes known to the other three.  Quads of one wave
 * differ in length and diverge from each other, never within themselves.
 * What differs between the lanes of a quad is data only: the column, the
 * addresses, the tail bytes below plen.
 *
 * The table is the lane form's, lane l on bank l & 31: a ds_read_b32 is served
 * per half-wave of 32 lanes over 32 banks and every lane of a half-wave reads
 * its own bank, so no lookup conflicts and the time of a lookup does not
 * depend on key or data.  The table build ends in the kernel's only barrier
 * and comes before anything that can end a lane.  Quad d of workgroup g takes
 * datagrams (g * per + k) * AES_QUADS + d, k = 0 .. per - 1: the launch raises
 * per with n as the wave form's does.
 *
 * Keys, two instances of the body.  One key: the schedule sits in the
 * launch's arguments, is copied to LDS once per workgroup (published by the
 * table build's barrier) and lane q picks its fifteen words from there.  _mc:
 * lane q takes its fifteen words from the tx schedule of its datagram's table
 * entry (ciphertab_ent: the index clamped before any address is formed).
 * Either way they stay in VGPRs for all of a datagram's blocks.
 *
 * Lane q moves dword q of each block, a 4-byte access at byte alignment, and
 * touches only bytes of its own datagram's payload: whole blocks below the
 * last, in the last one the plaintext bytes below plen (read) and the whole
 * block (written).
 */
constexpr int AES_QUADS = AES_WG / NET2_AES_QUAD_LANES;	/* datagrams per workgroup and step */

template <bool MC> struct AesQuadArgs;
template <> struct AesQuadArgs<false> {
	AesBurstArgs b;
	AesKeys<1> keys;
	__device__ __forceinline__ const AesBurstArgs &burst() const { return b; }
};
template <> struct AesQuadArgs<true> {
	AesMcArgs m;
	__device__ __forceinline__ const AesBurstArgs &burst() const { return m.b; }
};

/* quad_perm's control word: lane q of every quad reads lane sel(q). */
constexpr int quad_ctrl(uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3)
{
	return (int)(s0 | s1 << 2 | s2 << 4 | s3 << 6);
}
/* ... for the k-th input of a column (aes_quad_src), and for lane 0's value */
constexpr int quad_ctrl_src(uint32_t k)
{
	return quad_ctrl(aes_quad_src(0, k), aes_quad_src(1, k), aes_quad_src(2, k),
	    aes_quad_src(3, k));
}
constexpr int QUAD_FIRST = quad_ctrl(0, 0, 0, 0);

/* v of the lane that CTRL names, within the calling lane's quad.  Every lane
 * of the quad executes it together. */
template <int CTRL>
__device__ __forceinline__ uint32_t quad_perm(uint32_t v)
{
	return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);
}

/* The fifteen schedule words of lane q out of a 60-word schedule. */
struct RkQuad {
	uint32_t w[NET2_AES_QUAD_KEYWORDS];
	__device__ __forceinline__ RkQuad(const uint32_t *p, uint32_t q)
	{
#pragma unroll
		for (int r = 0; r < NET2_AES_QUAD_KEYWORDS; r++)
			w[r] = p[aes_quad_rk(r, q)];
	}
};

/*
 * Slot i, nb >= 1 blocks, by the calling quad (all four lanes call; i and nb
 * are the same in them): the chain of aes_quad.h, the next block's word loaded
 * before the current one goes through the rounds.  q: the lane's column, K:
 * its schedule words.
 */
__device__ __forceinline__ void encrypt_by_quad(const AesBurstArgs &a,
    uint64_t i, uint32_t nb, const LdsTab &T, const RkQuad &K, uint32_t q)
{
	uint8_t *p = a.out + a.offsets[i] + payload_at(a.flags[i], a.hashlen);
	const uint32_t plen = a.plen[i];
	uint32_t chain = aes_quad_ld(a.iv + NET2_AES_BLOCK * i, q);
	uint32_t cur = aes_quad_word(p, plen, nb, 0, q);

	for (uint32_t j = 0; j < nb; j++) {
		uint32_t nx = 0;
		if (j + 1 < nb)
			nx = aes_quad_word(p, plen, nb, j + 1, q);
		uint32_t s = aes_quad_enter(chain, cur, K.w[0]);
#pragma unroll
		for (int r = 1; r <= NET2_AES_ROUNDS; r++) {
			const uint32_t s1 = quad_perm<quad_ctrl_src(1)>(s);
			const uint32_t s2 = quad_perm<quad_ctrl_src(2)>(s);
			const uint32_t s3 = quad_perm<quad_ctrl_src(3)>(s);
			s = aes_quad_round(T, r, s, s1, s2, s3, K.w[r]);
		}
		aes_quad_st(p + 16 * (uint64_t)j, q, s);
		chain = s;
		cur = nx;
	}
}

template <bool MC>
__global__ __launch_bounds__(AES_WG) void aes_cbc_encrypt_quad_kernel(
    const AesQuadArgs<MC> w, const uint32_t per)
{
	__shared__ uint32_t tab[256 * AES_REP];
	__shared__ uint32_t rks[MC ? 4 : 64];

	const AesBurstArgs &a = w.burst();
	const uint32_t t = threadIdx.x;
	if constexpr (!MC) {
		if (t < NET2_AES_RKWORDS)
			rks[t] = w.keys.k[0].w[t];
	}
	/* the one barrier (it publishes rks as well): before any lane can end */
	aes_build_table<false>(tab);

	const uint32_t q = aes_quad_col(t), quad = aes_quad_of(t);
	const LdsTab T = { tab + (t & (AES_REP - 1)) };
	for (uint32_t k = 0; k < per; k++) {
		const uint64_t i = ((uint64_t)blockIdx.x * per + k) * AES_QUADS + quad;
		if (i >= a.n)
			break;
		/* lane 0 settles what needs no cipher, as a lane of the lane form */
		uint32_t nb = 0;
		if (q == 0) {
			if constexpr (MC)
				nb = encrypt_mc_prep(w.m, i);
			else
				nb = encrypt_prep(a, i);
		}
		nb = quad_perm<QUAD_FIRST>(nb);
		if (nb == 0)
			continue;
		if constexpr (MC) {
			bool in;
			const RkQuad K(ciphertab_ent(w.m, i, &in)->enc, q);
			encrypt_by_quad(a, i, nb, T, K, q);
		} else {
			const RkQuad K(rks, q);
			encrypt_by_quad(a, i, nb, T, K, q);
		}
	}
}

/*
 * One slot's update (net2_burst_ciphertab_set_rx / _set_tx / _clear): the new
 * entry arrives by value and one wave stores it, 16 bytes per lane (the
 * argument is read with constant indices only and selected per lane: a
 * dynamic index would copy it to scratch).  Piece 0 is the meta words, 1..30
 * the two rx schedules, 31..45 the tx schedule.  side NET2_AES_TAB_RX stores
 * the rx pieces and replaces the rx bits, cutoff and rx_start;
 * NET2_AES_TAB_TX the tx pieces and the tx bit; 0 zeroes the entry.  Stream
 * order is the only synchronisation an entry has.
 */
constexpr unsigned CT_PIECES = sizeof(Net2CipherEnt) / 16;
constexpr unsigned CT_TX_FIRST = offsetof(Net2CipherEnt, enc) / 16;

__global__ __launch_bounds__(64) void aes_tab_set_kernel(Net2CipherEnt *ent,
    uint32_t side, const Net2CipherEnt nw)
{
	if (blockIdx.x != 0)
		return;
	const unsigned t = threadIdx.x;
	u32x4 *q = reinterpret_cast<u32x4 *>(ent);
	const uint32_t *w = reinterpret_cast<const uint32_t *>(&nw);
	u32x4 v = { 0, 0, 0, 0 };
#pragma unroll
	for (unsigned k = 1; k < CT_PIECES; k++)
		if (t == k) {
			v.x = w[4 * k];
			v.y = w[4 * k + 1];
			v.z = w[4 * k + 2];
			v.w = w[4 * k + 3];
		}
	const bool rx_piece = t >= 1 && t < CT_TX_FIRST;
	const bool tx_piece = t >= CT_TX_FIRST && t < CT_PIECES;
	if ((side == NET2_AES_TAB_RX && rx_piece) ||
	    (side == NET2_AES_TAB_TX && tx_piece) ||
	    (side == 0 && (rx_piece || tx_piece)))
		q[t] = v;
	/* lane 63: the meta words, the other side's bits kept */
	if (t == 63) {
		u32x4 mt = q[0];
		if (side == NET2_AES_TAB_RX) {
			mt.x = (mt.x & NET2_CT_TX_BITS) | (nw.meta[0] & NET2_CT_RX_BITS);
			mt.y = nw.meta[1];
			mt.z = nw.meta[2];
			mt.w = 0;
		} else if (side == NET2_AES_TAB_TX) {
			mt.x = (mt.x & NET2_CT_RX_BITS) | (nw.meta[0] & NET2_CT_TX_BITS);
		} else {
			mt = u32x4{ 0, 0, 0, 0 };
		}
		q[0] = mt;
	}
}

/* ---- what the launchers share -------------------------------------------- */

/* A decrypt burst's arguments; alt: the alternate key's cutoff (the launches
 * under one connection's keys; NULL: the _mc launches, which take it from
 * the table). */
AesBurstArgs decrypt_args(const AesRxAlt *alt, uint32_t hashlen,
    const uint8_t *base, const uint64_t *offsets, const uint32_t *lens,
    uint64_t n, const uint32_t *seq, const uint32_t *flags, const uint8_t *iv,
    uint8_t *result, uint8_t *out, uint32_t *plen)
{
	AesBurstArgs a = {};
	a.in = base;
	a.out = out;
	a.offsets = offsets;
	a.lens = lens;
	a.seq = seq;
	a.flags = flags;
	a.iv = iv;
	a.result = result;
	a.plen = plen;
	a.n = n;
	a.hashlen = hashlen;
	if (alt != nullptr) {
		a.no_cutoff = alt->no_cutoff != 0;
		a.cutoff = alt->cutoff;
		a.rx_start = alt->rx_start;
	}
	return a;
}

AesBurstArgs encrypt_args(uint32_t hashlen, const uint32_t *flags,
    const uint8_t *iv, uint8_t *base, const uint64_t *offsets,
    const uint32_t *lens, const uint32_t *plen, uint64_t n, uint8_t *result,
    uint32_t *wire_len)
{
	AesBurstArgs a = {};
	a.out = base;
	a.offsets = offsets;
	a.lens = lens;
	a.flags = flags;
	a.iv = iv;
	a.result = result;
	a.plen = const_cast<uint32_t *>(plen);
	a.wire_len = wire_len;
	a.n = n;
	a.hashlen = hashlen;
	return a;
}

AesMcArgs mc_args(const AesBurstArgs &b, const AesTabArgs &kt)
{
	AesMcArgs m = {};
	m.b = b;
	m.conn = kt.conn;
	m.tab = kt.tab;
	m.slots = kt.slots;
	return m;
}

/* The lane forms' grid: one lane per datagram. */
dim3 lane_grid(uint64_t n)
{
	return dim3((unsigned)((n + AES_WG - 1) / AES_WG));
}

/*
 * The wave form's datagrams per wave (the kernel's per_wave) and grid for a
 * burst of n: one datagram per wave until the grid would pass AES_WAVE_GRID
 * workgroups (five of them, 32 KiB of table each, are resident per CU of an
 * MI355X's 256), then as many as keep it there, 16 at the most.
 */
constexpr uint64_t AES_WAVE_GRID = 1280;
constexpr uint64_t AES_WAVE_PER_MAX = 16;

uint32_t wave_per(uint64_t n)
{
	const uint64_t per = (n + AES_WAVES * AES_WAVE_GRID - 1) /
	    (AES_WAVES * AES_WAVE_GRID);
	return (uint32_t)(per < 1 ? 1 : per > AES_WAVE_PER_MAX ? AES_WAVE_PER_MAX : per);
}

dim3 wave_grid(uint64_t n, uint32_t per)
{
	const uint64_t step = (uint64_t)AES_WAVES * per;
	return dim3((unsigned)((n + step - 1) / step));
}

/* The quad form's datagrams per quad (the kernel's per) and grid, by the wave
 * form's rule: AES_QUADS datagrams per workgroup and step. */
uint32_t quad_per(uint64_t n)
{
	const uint64_t per = (n + AES_QUADS * AES_WAVE_GRID - 1) /
	    (AES_QUADS * AES_WAVE_GRID);
	return (uint32_t)(per < 1 ? 1 : per > AES_WAVE_PER_MAX ? AES_WAVE_PER_MAX : per);
}

dim3 quad_grid(uint64_t n, uint32_t per)
{
	const uint64_t step = (uint64_t)AES_QUADS * per;
	return dim3((unsigned)((n + step - 1) / step));
}

/*
 * The decrypt launches under one connection's keys, either form: the rx
 * schedules (key, and alt_key when there is one: NK = 2) expanded into k,
 * which is or lies in the launch's arguments; launch(); the schedules wiped,
 * the launch having copied its arguments.
 */
template <int NK, class L>
void launch_rx_keyed(const uint8_t *key, const uint8_t *alt_key, AesKeys<NK> &k,
    L &&launch)
{
	aes256_dec_schedule(key, &k.k[0]);
	if constexpr (NK == 2)
		aes256_dec_schedule(alt_key, &k.k[1]);
	launch();
	key_wipe(&k, sizeof(k));
}

}	/* namespace */

hipError_t net2_launch_aes_decrypt(const uint8_t *key, const AesRxAlt &alt,
    uint32_t hashlen, const uint8_t *base, const uint64_t *offsets,
    const uint32_t *lens, uint64_t n, const uint32_t *seq,
    const uint32_t *flags, const uint8_t *iv, uint8_t *result, uint8_t *out,
    uint32_t *plen, hipStream_t s)
{
	if (n == 0)
		return hipSuccess;
	const AesBurstArgs a = decrypt_args(&alt, hashlen, base, offsets, lens, n,
	    seq, flags, iv, result, out, plen);
	if (alt.alt_key != nullptr) {
		AesKeys<2> k;
		launch_rx_keyed(key, alt.alt_key, k, [&] {
			hipLaunchKernelGGL(aes_cbc_decrypt_kernel<true>, lane_grid(n),
			    dim3(AES_WG), 0, s, a, k);
		});
	} else {
		AesKeys<1> k;
		launch_rx_keyed(key, nullptr, k, [&] {
			hipLaunchKernelGGL(aes_cbc_decrypt_kernel<false>, lane_grid(n),
			    dim3(AES_WG), 0, s, a, k);
		});
	}
	return hipGetLastError();
}

hipError_t net2_launch_aes_encrypt(const uint8_t *key, uint32_t hashlen,
    const uint32_t *flags, const uint8_t *iv, uint8_t *base,
    const uint64_t *offsets, const uint32_t *lens, const uint32_t *plen,
    uint64_t n, uint8_t *result, uint32_t *wire_len, hipStream_t s)
{
	if (n == 0)
		return hipSuccess;
	const AesBurstArgs a = encrypt_args(hashlen, flags, iv, base, offsets,
	    lens, plen, n, result, wire_len);
	AesKeys<1> k;
	aes256_enc_schedule(key, &k.k[0]);
	hipLaunchKernelGGL(aes_cbc_encrypt_kernel, lane_grid(n), dim3(AES_WG), 0, s,
	    a, k);
	key_wipe(&k, sizeof(k));
	return hipGetLastError();
}

hipError_t net2_launch_aes_tab_set(Net2CipherEnt *ents, uint32_t slot,
    uint32_t side, const uint8_t *key, const uint8_t *alt_key, int no_cutoff,
    uint32_t cutoff, uint32_t rx_start, hipStream_t s)
{
	if (ents == nullptr || (side != 0 && key == nullptr))
		return hipErrorInvalidValue;
	Net2CipherEnt nw = {};
	if (side == NET2_AES_TAB_RX)
		aes_tab_fill_rx(&nw, key, alt_key, no_cutoff != 0, cutoff, rx_start);
	else if (side == NET2_AES_TAB_TX)
		aes_tab_fill_tx(&nw, key);
	hipLaunchKernelGGL(aes_tab_set_kernel, dim3(1), dim3(64), 0, s, ents + slot,
	    side, nw);
	key_wipe(&nw, sizeof(nw));
	return hipGetLastError();
}

hipError_t net2_launch_aes_decrypt_mc(const AesTabArgs &kt, uint32_t hashlen,
    const uint8_t *base, const uint64_t *offsets, const uint32_t *lens,
    uint64_t n, const uint32_t *seq, const uint32_t *flags, const uint8_t *iv,
    uint8_t *result, uint8_t *out, uint32_t *plen, hipStream_t s)
{
	if (n == 0)
		return hipSuccess;
	const AesMcArgs m = mc_args(decrypt_args(nullptr, hashlen, base, offsets,
	    lens, n, seq, flags, iv, result, out, plen), kt);
	hipLaunchKernelGGL(aes_cbc_decrypt_mc_kernel, lane_grid(n), dim3(AES_WG), 0,
	    s, m);
	return hipGetLastError();
}

/* ---- the wave form of the decrypt launches ---------------------------------- */

hipError_t net2_launch_aes_decrypt_wave(const uint8_t *key, const AesRxAlt &alt,
    uint32_t hashlen, const uint8_t *base, const uint64_t *offsets,
    const uint32_t *lens, uint64_t n, const uint32_t *seq,
    const uint32_t *flags, const uint8_t *iv, uint8_t *result, uint8_t *out,
    uint32_t *plen, hipStream_t s)
{
	if (n == 0)
		return hipSuccess;
	const AesBurstArgs a = decrypt_args(&alt, hashlen, base, offsets, lens, n,
	    seq, flags, iv, result, out, plen);
	const uint32_t per = wave_per(n);
	if (alt.alt_key != nullptr) {
		AesWaveArgs<KS_ALT> w;
		w.b = a;
		launch_rx_keyed(key, alt.alt_key, w.keys, [&] {
			hipLaunchKernelGGL(aes_cbc_decrypt_wave_kernel<KS_ALT>,
			    wave_grid(n, per), dim3(AES_WG), 0, s, w, per);
		});
	} else {
		AesWaveArgs<KS_ONE> w;
		w.b = a;
		launch_rx_keyed(key, nullptr, w.keys, [&] {
			hipLaunchKernelGGL(aes_cbc_decrypt_wave_kernel<KS_ONE>,
			    wave_grid(n, per), dim3(AES_WG), 0, s, w, per);
		});
	}
	return hipGetLastError();
}

hipError_t net2_launch_aes_decrypt_mc_wave(const AesTabArgs &kt,
    uint32_t hashlen, const uint8_t *base, const uint64_t *offsets,
    const uint32_t *lens, uint64_t n, const uint32_t *seq,
    const uint32_t *flags, const uint8_t *iv, uint8_t *result, uint8_t *out,
    uint32_t *plen, hipStream_t s)
{
	if (n == 0)
		return hipSuccess;
	AesWaveArgs<KS_TAB> w = {};
	w.m = mc_args(decrypt_args(nullptr, hashlen, base, offsets, lens, n, seq,
	    flags, iv, result, out, plen), kt);
	const uint32_t per = wave_per(n);
	hipLaunchKernelGGL(aes_cbc_decrypt_wave_kernel<KS_TAB>, wave_grid(n, per),
	    dim3(AES_WG), 0, s, w, per);
	return hipGetLastError();
}

hipError_t net2_launch_aes_encrypt_mc(const AesTabArgs &kt, uint32_t hashlen,
    const uint32_t *flags, const uint8_t *iv, uint8_t *base,
    const uint64_t *offsets, const uint32_t *lens, const uint32_t *plen,
    uint64_t n, uint8_t *result, uint32_t *wire_len, hipStream_t s)
{
	if (n == 0)
		return hipSuccess;
	const AesMcArgs m = mc_args(encrypt_args(hashlen, flags, iv, base, offsets,
	    lens, plen, n, result, wire_len), kt);
	hipLaunchKernelGGL(aes_cbc_encrypt_mc_kernel, lane_grid(n), dim3(AES_WG), 0,
	    s, m);
	return hipGetLastError();
}

/* ---- the quad form of the encrypt launches ---------------------------------- */

hipError_t net2_launch_aes_encrypt_quad(const uint8_t *key, uint32_t hashlen,
    const uint32_t *flags, const uint8_t *iv, uint8_t *base,
    const uint64_t *offsets, const uint32_t *lens, const uint32_t *plen,
    uint64_t n, uint8_t *result, uint32_t *wire_len, hipStream_t s)
{
	if (n == 0)
		return hipSuccess;
	AesQuadArgs<false> w;
	w.b = encrypt_args(hashlen, flags, iv, base, offsets, lens, plen, n, result,
	    wire_len);
	aes256_enc_schedule(key, &w.keys.k[0]);
	const uint32_t per = quad_per(n);
	hipLaunchKernelGGL(aes_cbc_encrypt_quad_kernel<false>, quad_grid(n, per),
	    dim3(AES_WG), 0, s, w, per);
	key_wipe(&w.keys, sizeof(w.keys));
	return hipGetLastError();
}

hipError_t net2_launch_aes_encrypt_mc_quad(const AesTabArgs &kt,
    uint32_t hashlen, const uint32_t *flags, const uint8_t *iv, uint8_t *base,
    const uint64_t *offsets, const uint32_t *lens, const uint32_t *plen,
    uint64_t n, uint8_t *result, uint32_t *wire_len, hipStream_t s)
{
	if (n == 0)
		return hipSuccess;
	AesQuadArgs<true> w = {};
	w.m = mc_args(encrypt_args(hashlen, flags, iv, base, offsets, lens, plen, n,
	    result, wire_len), kt);
	const uint32_t per = quad_per(n);
	hipLaunchKernelGGL(aes_cbc_encrypt_quad_kernel<true>, quad_grid(n, per),
	    dim3(AES_WG), 0, s, w, per);
	return hipGetLastError();
}
