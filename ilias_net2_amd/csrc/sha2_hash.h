/*
 * sha2_hash.h -- hash shapes, block loads, padding and the per-lane digest.
 * One of the device headers of sha2_kernels.hip, which includes them in
 * order into one translation unit.
 */
#ifndef NET2_SHA2_HASH_H
#define NET2_SHA2_HASH_H

#include "sha2_device.h"
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace net2 {
namespace dev {

/* ---- hash traits ------------------------------------------------------ */

/*
 * Per-kernel code-shape choices (each measured):
 *   ASM: round bodies as ordered asm blocks (round256_asm, sha2_device.h);
 *   U2:  the two-block ping-pong block loop (absorb below);
 *   PAIR: the pair loop -- both 64-byte blocks of a 128-byte line requested
 *         together, one pair ahead (absorb below);
 *   DRAIN: issue priority while the grid drains (prio_remaining);
 *   GLDS: LDS-DMA staging of the next block (absorb);
 *   PREFETCH: block k+1 in flight while block k is compressed.
 * Alternatives that lost their A/B (the evidence stays
 * under profiles/) are removed from the source, not kept behind switches.
 */
template <bool ASM_, bool U2_, bool PAIR_ = false, bool DRAIN_ = false>
struct Sha256T {
	static constexpr bool ASM = ASM_;
	static constexpr bool U2 = U2_;
	static constexpr bool PAIR = PAIR_;
	static constexpr bool DRAIN = DRAIN_;	/* prio_remaining */
	static constexpr bool GLDS = false;	/* absorb: LDS-DMA staging */
	typedef uint32_t word;
	static constexpr int BLOCK = 64;	/* bytes per block */
	static constexpr int NW32 = 16;		/* 32-bit words per block */
	static constexpr int LENBYTES = 8;	/* trailing length field */
	static constexpr int DLEN = 32;
	/* prefetch block k+1 during block k: 16 VGPRs, still 8 waves/SIMD */
	static constexpr bool PREFETCH = true;
	typedef uint32_t State[8];

	__device__ __forceinline__ static void init(State &st, int)
	{
#pragma unroll
		for (int i = 0; i < 8; i++)
			st[i] = IV256[i];
	}
	__device__ __forceinline__ static void compress(State &st,
	    uint32_t (&b)[16])
	{
		compress256<ASM>(st, b);
	}
	/* Store state big-endian (src/sha2.c:553-557) as 32-bit words. */
	__device__ __forceinline__ static void out_words(const State &st,
	    uint32_t (&o)[16], int)
	{
#pragma unroll
		for (int i = 0; i < 8; i++)
			o[i] = bswap32(st[i]);
	}
};
/*
 * Every SHA-256 kernel takes the asm rounds, the two-block loop and the
 * pair loop (fixed kernel: 92 VGPRs; variable-length kernel: 96, C3 +0.7 %
 * with the pair loop, profiles/round1/var_pair_ab.txt; C3 452 against
 * 463 us with the asm rounds, profiles/round2/var_asm_ab.txt); the HMAC
 * kernels in every mode (launch_hmac_var_mode).
 */
typedef Sha256T<true, true, true> Sha256;	/* fixed, variable, HMAC */
typedef Sha256 Sha256V;
typedef Sha256 Sha256H;

struct Sha512 {
	static constexpr bool ASM = false;
	/* no prefetch: a 128-byte block would cost 32 VGPRs and a wave per
	 * SIMD (the two-block ping-pong: -1.4 %, with 5 waves -18 %,
	 * profiles/round2/fixed512_prefetch_ab.txt) */
	static constexpr bool U2 = false;
	static constexpr bool PAIR = false;	/* a 128-byte block is a whole line */
	/* drain priority (prio_remaining): the fixed kernel only, C4 +1.2 %
	 * (profiles/round2/drain_prio_ab.txt) */
	static constexpr bool DRAIN = true;
	static constexpr bool GLDS = false;
	typedef uint64_t word;
	static constexpr int BLOCK = 128;
	static constexpr int NW32 = 32;
	static constexpr int LENBYTES = 16;
	static constexpr int DLEN = 64;		/* 48 for SHA-384 */
	static constexpr bool PREFETCH = false;
	typedef uint64_t State[8];

	__device__ __forceinline__ static void init(State &st, int is384)
	{
#pragma unroll
		for (int i = 0; i < 8; i++)
			st[i] = is384 ? IV384[i] : IV512[i];
	}
	__device__ __forceinline__ static void compress(State &st,
	    uint32_t (&b)[32])
	{
		uint64_t w[16];
#pragma unroll
		for (int i = 0; i < 16; i++)
			w[i] = mk64(b[2 * i + 1], b[2 * i]);
		compress512(st, w);
	}
	__device__ __forceinline__ static void out_words(const State &st,
	    uint32_t (&o)[16], int)
	{
#pragma unroll
		for (int i = 0; i < 8; i++) {
			o[2 * i] = bswap32(hi32(st[i]));
			o[2 * i + 1] = bswap32(lo32(st[i]));
		}
	}
};

/*
 * SHA-512 for the variable-length kernel: no prefetch -- neither the
 * two-block ping-pong (136-140 VGPRs, 3 waves; +1.9 % on c3_512 on one box,
 * -1.3 % on another, -3 to -4 % on the HMAC-SHA512 MTU configs and both
 * bursts) nor LDS-DMA staging (-1.4 to -2.8 %, profiles/round3/glds_*_ab.txt).
 */
struct Sha512V : Sha512 {
	static constexpr bool DRAIN = false;
};
/* ... for the lane-per-job kernel of the coalescer, whose blocks come over
 * PCIe from zero-copy staging: the next block's load is in flight while one
 * is compressed (64 threads of 1 KiB SHA-512 calls: 431 k against 399 k
 * calls/s, profiles/round2/coalesce_job512_prefetch_ab.txt) ... */
struct Sha512J : Sha512 {
	static constexpr bool DRAIN = false;
	static constexpr bool U2 = true;
	static constexpr bool PREFETCH = true;
};
/* ... for the variable-length HMAC kernels (as Sha512V) ... */
struct Sha512H : Sha512 {
	static constexpr bool DRAIN = false;
};
/* ... and for the fixed-layout HMAC-SHA512 kernel: drain priority kept, the
 * next block fetched with LDS-DMA (global_load_lds) into a per-wave LDS slab
 * while the current one is compressed -- a prefetch that costs no VGPRs
 * (absorb below).  96 VGPRs, its ~35 KB of slabs per workgroup hold it at
 * 4 waves per SIMD; without them it runs 5 waves at 95 VGPRs and measured
 * 0.7 % slower (profiles/round5/ab_hostmid_box2.txt) */
struct Sha512HF : Sha512 {
	static constexpr bool GLDS = true;
};

/* ---- message loading ------------------------------------------------- */

/*
 * Address modes.  A16: every packet start in the wave is 16-byte aligned, a
 * block is NW32/4 global_load_dwordx4.  A4: dword-aligned starts (packed
 * packets whose lengths are multiples of 4, e.g. 1,500-byte datagrams), a
 * block is NW32 global_load_dword.  A1: arbitrary byte alignment; the
 * block is read as NW32 + 1 naturally aligned dwords (the extra one only
 * when misaligned, so no dword outside the packet's own bytes is touched)
 * and re-aligned with v_alignbyte_b32.
 */
enum { AMODE_A16 = 0, AMODE_A1 = 1, AMODE_A4 = 2 };
/*
 * One address path for the SHA-512 variable-length and HMAC kernels: they
 * take the A16 block loads (global_load_dwordx4 at the block start) whatever
 * the packet's alignment, relying on the unaligned access mode ROCm sets for
 * gfx9+ global memory (tools/unaligned_probe.hip: every byte offset reads
 * the right bytes on gfx950, profiles/round4/unaligned_probe.json) -- one
 * code path per kernel instead of three chosen per wave.  The tail block
 * keeps its aligned-dword reads (it never touches a byte past the packet).
 * From order-flipped A/Bs on separate boxes (profiles/round4/ab_*.txt): the
 * SHA-512 kernels gain (HMAC-SHA512 verify +2.8 %, burst RX +2 %, c3_512
 * +0.5 to +1.2 %), the SHA-256 kernels keep the three paths (HMAC-SHA256
 * verify 1.5 % and C3 0.45 % faster with them).
 */
template <class H>
struct OnePath {
	static constexpr bool value = sizeof(typename H::word) == 8;
};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
/*
 * Dword loads from an address rebuilt from an integer (the aligned-down
 * start of a byte-aligned packet) go through a global pointer: a plain
 * pointer would be a flat load, which may alias LDS, and in a kernel with
 * LDS-DMA in flight every flat load waits for all outstanding loads first.
 */
typedef __attribute__((address_space(1))) const uint32_t gconst_u32;

template <int NW32>
struct Raw {
	uint32_t d[NW32 + 1];
};

template <int NW32, int AMODE>
__device__ __forceinline__ void issue_block(const uint8_t *p, Raw<NW32> &r)
{
	if (AMODE == AMODE_A16) {
		const u32x4 *q = reinterpret_cast<const u32x4 *>(p);
#pragma unroll
		for (int i = 0; i < NW32 / 4; i++) {
			u32x4 v = q[i];
			r.d[4 * i] = v.x;
			r.d[4 * i + 1] = v.y;
			r.d[4 * i + 2] = v.z;
			r.d[4 * i + 3] = v.w;
		}
	} else if (AMODE == AMODE_A4) {
		const uint32_t *q = reinterpret_cast<const uint32_t *>(p);
#pragma unroll
		for (int i = 0; i < NW32; i++)
			r.d[i] = q[i];
	} else {
		uintptr_t a = reinterpret_cast<uintptr_t>(p);
		const gconst_u32 *q = (const gconst_u32 *)(a & ~(uintptr_t)3);
#pragma unroll
		for (int i = 0; i < NW32; i++)
			r.d[i] = q[i];
		r.d[NW32] = (a & 3) ? q[NW32] : 0u;
	}
}

/* Raw little-endian dwords -> big-endian message words. */
template <int NW32, int AMODE>
__device__ __forceinline__ void finish_block(const uint8_t *p,
    const Raw<NW32> &r, uint32_t (&w)[NW32])
{
	if (AMODE == AMODE_A16 || AMODE == AMODE_A4) {
#pragma unroll
		for (int i = 0; i < NW32; i++)
			w[i] = bswap32(r.d[i]);
	} else {
		uint32_t sh = (uint32_t)reinterpret_cast<uintptr_t>(p) & 3;
#pragma unroll
		for (int i = 0; i < NW32; i++)
			w[i] = bswap32(__builtin_amdgcn_alignbyte(r.d[i + 1],
			    r.d[i], sh));
	}
}

/*
 * LDS-DMA staging (H::GLDS).  A global_load_lds instruction writes the
 * wave's 64 lane chunks to LDS lane-linearly (wave-uniform base + lane x
 * size), with no VGPR destination.  Chunk j (16 bytes) of every lane's
 * block goes to its own 1 KiB row of the wave's slab, so lane l reads its
 * block back from its own column with ds_read_b128 (consecutive lanes,
 * consecutive banks).  All address modes fetch 16-byte chunks: A16 and A4
 * from the block start (a global dwordx4 needs only dword alignment), A1
 * from the naturally aligned dword below it, plus the one dword past the
 * 32nd into a 256-byte row of its own when the start is misaligned -- the
 * bytes issue_block reads, never one outside the packet.  (Dword-wide
 * fetches, 32 per block, measured 35-42 % slower on the variable-length
 * SHA-512 kernels: every instruction touches the wave's 64 lines.)
 * One 8,448-byte slab per wave of a 256-thread workgroup.
 */
typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) void glb_void;
#define NET2_GLDS_WORDS (33 * 64)
__shared__ uint32_t glds_slab[4 * NET2_GLDS_WORDS];

__device__ __forceinline__ uint32_t *glds_wave_slab()
{
	const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	return glds_slab + wv * NET2_GLDS_WORDS;
}

template <int NW32, int AMODE>
__device__ __forceinline__ void glds_issue(const uint8_t *p, uint32_t *slab)
{
	const uintptr_t a = reinterpret_cast<uintptr_t>(p);
	const uint8_t *q = AMODE != AMODE_A1 ? p :
	    reinterpret_cast<const uint8_t *>(a & ~(uintptr_t)3);
#pragma unroll
	for (int j = 0; j < NW32 / 4; j++)
		__builtin_amdgcn_global_load_lds((glb_void *)(q + 16 * j),
		    (lds_void *)(slab + 256 * j), 16, 0, 0);
	if (AMODE == AMODE_A1 && (a & 3))
		__builtin_amdgcn_global_load_lds((glb_void *)(q + 4 * NW32),
		    (lds_void *)(slab + 64 * NW32), 4, 0, 0);
}

/* The lane's staged block back from the slab, as issue_block leaves it. */
template <int NW32, int AMODE>
__device__ __forceinline__ void glds_read(const uint32_t *slab, Raw<NW32> &r)
{
	const uint32_t lane = threadIdx.x & 63;
	const u32x4 *s = reinterpret_cast<const u32x4 *>(slab) + lane;
#pragma unroll
	for (int j = 0; j < NW32 / 4; j++) {
		const u32x4 v = s[64 * j];
		r.d[4 * j] = v.x;
		r.d[4 * j + 1] = v.y;
		r.d[4 * j + 2] = v.z;
		r.d[4 * j + 3] = v.w;
	}
	/* the A1 dword past the 32nd; unused when the start is aligned
	 * (alignbyte by 0) */
	r.d[NW32] = AMODE == AMODE_A1 ? slab[64 * NW32 + lane] : 0u;
}

/*
 * The last data bytes q[0 .. rem) (rem < BLOCK) followed by the 0x80
 * terminator and zero fill, as big-endian words (the buffer SHA256Pad /
 * SHA512Pad build, src/sha2.c:495-526 / :784-812).  Only dwords that hold
 * packet bytes are read.
 */
template <int NW32>
__device__ __forceinline__ void tail_block(const uint8_t *q, uint32_t rem,
    uint32_t (&w)[NW32])
{
	uintptr_t a = reinterpret_cast<uintptr_t>(q);
	uint32_t sh = (uint32_t)a & 3;
	const gconst_u32 *al = (const gconst_u32 *)(a - sh);
	uint32_t d[NW32 + 1];
#pragma unroll
	for (int j = 0; j <= NW32; j++)
		d[j] = (uint32_t)(4 * j) < sh + rem ? al[j] : 0u;
#pragma unroll
	for (int i = 0; i < NW32; i++) {
		uint32_t x = bswap32(__builtin_amdgcn_alignbyte(d[i + 1], d[i],
		    sh));
		int kk = (int)rem - 4 * i;	/* message bytes in this word */
		if (kk < 4) {
			uint32_t keep = kk > 0 ? ~(0xffffffffu >> (8 * kk)) : 0u;
			uint32_t mark = kk >= 0 ? 0x80000000u >> (8 * kk) : 0u;
			x = (x & keep) | mark;
		}
		w[i] = x;
	}
}

/* Digest store: 16-byte vector stores when aligned, bytes otherwise. */
template <int DLEN>
__device__ __forceinline__ void store_digest(uint8_t *o, const uint32_t (&v)[16])
{
	if ((reinterpret_cast<uintptr_t>(o) & 15) == 0) {
		uint4 *q = reinterpret_cast<uint4 *>(o);
#pragma unroll
		for (int i = 0; i < DLEN / 16; i++)
			q[i] = make_uint4(v[4 * i], v[4 * i + 1], v[4 * i + 2],
			    v[4 * i + 3]);
	} else {
#pragma unroll
		for (int i = 0; i < DLEN / 4; i++) {
			uint32_t x = v[i];
			o[4 * i] = (uint8_t)x;
			o[4 * i + 1] = (uint8_t)(x >> 8);
			o[4 * i + 2] = (uint8_t)(x >> 16);
			o[4 * i + 3] = (uint8_t)(x >> 24);
		}
	}
}

/*
 * Pin a finished state before a lane-conditional use (`if (live) store`):
 * otherwise the compiler sinks the last compression into the branch and
 * leaves its LDS constant reads (SHA-512) above it, all live at once.
 */
template <class H>
__device__ __forceinline__ void materialize(const typename H::State &st)
{
#pragma unroll
	for (int i = 0; i < 8; i++)
		asm volatile("" ::"v"(st[i]));
}

/*
 * Issue priority while a grid drains (H::DRAIN: the fixed SHA-512 kernel;
 * not on the byte-aligned load path).
 * The SIMD's VALU arbiter serves the oldest wave first, so when the grid's
 * last generation of waves is dispatched, the youngest waves -- those with
 * the most blocks left -- progress last and finish alone, at one wave's
 * issue rate.  In the workgroups of the grid's last kPrioGen x 256 (two
 * per CU), a wave's priority follows the work it has left (s_setprio 3..0
 * as its remaining blocks fall below 12 / 6 / 2), so the waves of a SIMD
 * end closer together.  C4 +1.0 % (six alternations on two boxes; one or
 * three / four generations: +0.7 % / flat), C2 flat
 * (profiles/round2/drain_prio_ab.txt).  The same priority in every wave of
 * the grid measured slower (C2 -5 %, C4 -6 %, C3 -1 %,
 * profiles/round2/prio_ab.txt): the age order keeps the waves of a SIMD out
 * of phase, so their loads do not all wait at once.
 */
constexpr unsigned kPrioGen = 2;
template <bool DRAIN>
__device__ __forceinline__ void prio_remaining(uint32_t rem_blocks)
{
	if (!DRAIN)
		return;
	if (gridDim.x < 4 * 256 * kPrioGen ||
	    blockIdx.x + 256 * kPrioGen < gridDim.x)
		return;
	const uint32_t r = __builtin_amdgcn_readfirstlane(rem_blocks);
	if (r >= 12)
		__builtin_amdgcn_s_setprio(3);
	else if (r >= 6)
		__builtin_amdgcn_s_setprio(2);
	else if (r >= 2)
		__builtin_amdgcn_s_setprio(1);
	else
		__builtin_amdgcn_s_setprio(0);
}

/*
 * Whole-message digest for one lane.  nfull full blocks stream from p with
 * a one-block prefetch; then the generic tail (data remainder + 0x80 +
 * length, one or two blocks), or -- when the caller knows every message of
 * the launch is a multiple of the block size -- the constant padding block
 * whose K[t] + W[t] schedule the host precomputed (kw).
 */
/*
 * SHA*Update over the len / BLOCK full blocks at p (src/sha2.c:477-485:
 * whole blocks are transformed straight from caller memory).  With
 * PREFETCH, block k+1 is loaded while block k is compressed.
 */
template <class H, int AMODE, bool PREFETCH = H::PREFETCH>
__device__ __forceinline__ void absorb(const uint8_t *p, uint32_t len,
    typename H::State &st)
{
	constexpr int NW32 = H::NW32;
	const uint32_t nfull = len / H::BLOCK;

	if constexpr (H::GLDS) {
		/*
		 * Block k+1 is requested into the wave's LDS slab (no VGPRs)
		 * once block k has been read out of it, so its memory latency
		 * runs under block k's compression.  The waits are explicit:
		 * the slab is complete after vmcnt(0), and free again once the
		 * lane's reads have returned (lgkmcnt(0)).
		 */
		uint32_t *slab = glds_wave_slab();
		if (nfull > 0)
			glds_issue<NW32, AMODE>(p, slab);
		for (uint32_t k = 0; k < nfull; k++) {
			prio_remaining<H::DRAIN && AMODE != AMODE_A1>(nfull - k);
			const uint8_t *bp = p + (size_t)k * H::BLOCK;
			asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
			Raw<NW32> r;
			glds_read<NW32, AMODE>(slab, r);
			asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
			if (k + 1 < nfull)
				glds_issue<NW32, AMODE>(bp + H::BLOCK, slab);
			uint32_t w[NW32];
			finish_block<NW32, AMODE>(bp, r, w);
			H::compress(st, w);
		}
	} else if (PREFETCH && H::PAIR) {
		/*
		 * Pairs of blocks (one 128-byte line of an aligned packet)
		 * requested together, one pair ahead: two pair buffers swap
		 * roles every pair, so a trip covers four blocks.  With the
		 * one-block-ahead prefetch below, a line's second half was
		 * requested one compression (~20 us) after its first, long
		 * enough for ~10 % of the lines to leave the XCD's 4 MB L2 and
		 * be fetched again; here C2 reads exactly the payload, at the
		 * same speed (92 VGPRs, 5 waves/SIMD;
		 * profiles/round1/pairload_fetch.json).
		 */
		const uint32_t npairs = nfull / 2;
		Raw<NW32> a0, a1, b0, b1;
		if (npairs > 0) {
			issue_block<NW32, AMODE>(p, a0);
			issue_block<NW32, AMODE>(p + H::BLOCK, a1);
		}
		uint32_t q = 0;
		for (; q + 2 <= npairs; q += 2) {
			prio_remaining<H::DRAIN && AMODE != AMODE_A1>(nfull - 2 * q);
			const uint8_t *bp = p + (size_t)q * 2 * H::BLOCK;
			/* (requested one compression later instead, so the first
			 * wave generation asks for one line per lane before it
			 * starts: C2 -0.3 %, HMAC-SHA256 -0.9 %,
			 * profiles/round2/pair_late_ab.txt) */
			issue_block<NW32, AMODE>(bp + 2 * H::BLOCK, b0);
			issue_block<NW32, AMODE>(bp + 3 * H::BLOCK, b1);
			uint32_t w[NW32];
			finish_block<NW32, AMODE>(bp, a0, w);
			H::compress(st, w);
			finish_block<NW32, AMODE>(bp + H::BLOCK, a1, w);
			H::compress(st, w);
			/* past the last pair: re-read pair q + 1 (in bounds, L2-hot,
			 * unused) so a0/a1 are always defined here */
			const uint8_t *np = bp + (q + 2 < npairs ? 4 : 2) * H::BLOCK;
			issue_block<NW32, AMODE>(np, a0);
			issue_block<NW32, AMODE>(np + H::BLOCK, a1);
			finish_block<NW32, AMODE>(bp + 2 * H::BLOCK, b0, w);
			H::compress(st, w);
			finish_block<NW32, AMODE>(bp + 3 * H::BLOCK, b1, w);
			H::compress(st, w);
		}
		if (q < npairs) {
			const uint8_t *bp = p + (size_t)q * 2 * H::BLOCK;
			uint32_t w[NW32];
			finish_block<NW32, AMODE>(bp, a0, w);
			H::compress(st, w);
			finish_block<NW32, AMODE>(bp + H::BLOCK, a1, w);
			H::compress(st, w);
		}
		if (nfull & 1) {
			const uint8_t *bp = p + (size_t)(nfull - 1) * H::BLOCK;
			Raw<NW32> r;
			issue_block<NW32, AMODE>(bp, r);
			uint32_t w[NW32];
			finish_block<NW32, AMODE>(bp, r, w);
			H::compress(st, w);
		}
	} else if (PREFETCH && H::U2) {
		/*
		 * Two blocks per trip with the buffers swapping roles, so the
		 * prefetched block is consumed where it landed (a one-block loop
		 * copies it over: 16 v_mov per block).
		 */
		Raw<NW32> ra, rb;
		if (nfull > 0)
			issue_block<NW32, AMODE>(p, ra);
		uint32_t k = 0;
		for (; k + 2 <= nfull; k += 2) {
			prio_remaining<H::DRAIN && AMODE != AMODE_A1>(nfull - k);
			const uint8_t *bp = p + (size_t)k * H::BLOCK;
			issue_block<NW32, AMODE>(bp + H::BLOCK, rb);
			uint32_t w[NW32];
			finish_block<NW32, AMODE>(bp, ra, w);
			H::compress(st, w);
			/*
			 * Unconditional, so ra is always (re)defined here: a
			 * conditional load makes ra a phi and brings the copies
			 * back.  Past the last block it re-reads block k + 1
			 * (in bounds, L2-hot) and the result is unused.
			 */
			issue_block<NW32, AMODE>(bp + (k + 2 < nfull ? 2 : 1) *
			    H::BLOCK, ra);
			uint32_t w2[NW32];
			finish_block<NW32, AMODE>(bp + H::BLOCK, rb, w2);
			H::compress(st, w2);
		}
		if (k < nfull) {
			uint32_t w[NW32];
			finish_block<NW32, AMODE>(p + (size_t)k * H::BLOCK, ra, w);
			H::compress(st, w);
		}
	} else if (PREFETCH) {
		Raw<NW32> cur;
		if (nfull > 0)
			issue_block<NW32, AMODE>(p, cur);
		for (uint32_t k = 0; k < nfull; k++) {
			prio_remaining<H::DRAIN && AMODE != AMODE_A1>(nfull - k);
			const uint8_t *bp = p + (size_t)k * H::BLOCK;
			Raw<NW32> nxt;
			if (k + 1 < nfull)
				issue_block<NW32, AMODE>(bp + H::BLOCK, nxt);
			uint32_t w[NW32];
			finish_block<NW32, AMODE>(bp, cur, w);
			H::compress(st, w);
			cur = nxt;
		}
	} else {
		for (uint32_t k = 0; k < nfull; k++) {
			prio_remaining<H::DRAIN && AMODE != AMODE_A1>(nfull - k);
			const uint8_t *bp = p + (size_t)k * H::BLOCK;
			Raw<NW32> cur;
			issue_block<NW32, AMODE>(bp, cur);
			uint32_t w[NW32];
			finish_block<NW32, AMODE>(bp, cur, w);
			H::compress(st, w);
		}
	}
}

/*
 * SHA*Pad (src/sha2.c:495-543 / :784-832): the len % BLOCK tail bytes, the
 * 0x80 terminator, zero fill and the big-endian bit count `bits` (the whole
 * message, including any prefix hashed before p), in one or two blocks.
 * PADCONST: the caller knows len % BLOCK == 0 for every lane, so the pad
 * block is constant and its K[t] + W[t] schedule comes precomputed in kw.
 */
template <class H, bool PADCONST>
__device__ __forceinline__ void finish(const uint8_t *p, uint32_t len,
    uint64_t bits, const typename H::word *kw, typename H::State &st)
{
	constexpr int NW32 = H::NW32;
	if (PADCONST) {
		if (sizeof(typename H::word) == 4)
			compress256_kw<H::ASM>(*reinterpret_cast<uint32_t(*)[8]>(&st),
			    reinterpret_cast<const uint32_t *>(kw));
		else
			compress512_kw(*reinterpret_cast<uint64_t(*)[8]>(&st),
			    reinterpret_cast<const uint64_t *>(kw));
		return;
	}
	const uint32_t nfull = len / H::BLOCK;
	const uint32_t rem = len % H::BLOCK;
	uint32_t w[NW32];
	tail_block<NW32>(p + (size_t)nfull * H::BLOCK, rem, w);
	if (rem >= (uint32_t)(H::BLOCK - H::LENBYTES)) {
		/* No room for the length: this block, then a zero block. */
		H::compress(st, w);
#pragma unroll
		for (int i = 0; i < NW32; i++)
			w[i] = 0;
	}
	w[NW32 - 2] = (uint32_t)(bits >> 32);
	w[NW32 - 1] = (uint32_t)bits;
	H::compress(st, w);
}

/* Init + Update + Pad of one whole message (Final's store is the caller's). */
template <class H, int AMODE, bool PADCONST, bool PREFETCH = H::PREFETCH>
__device__ __forceinline__ void digest_one(const uint8_t *p, uint32_t len,
    int is384, const typename H::word *kw, typename H::State &st)
{
	H::init(st, is384);
	absorb<H, AMODE, PREFETCH>(p, len, st);
	finish<H, PADCONST>(p, len, (uint64_t)len << 3, kw, st);
}

} /* namespace dev */
} /* namespace net2 */

#endif /* NET2_SHA2_HASH_H */
