/*
 * sha2_digest.h -- the fixed-stride and variable-length digest kernels, their pad tables.
 * One of the device headers of sha2_kernels.hip, which includes them in
 * order into one translation unit.
 */
#ifndef NET2_SHA2_DIGEST_H
#define NET2_SHA2_DIGEST_H

#include "sha2_hash.h"
#include "sha2_keyprep.h"
#include "sha2_launch.h"

namespace net2 {
namespace dev {

/* One lane of the fixed-stride layout: packet i. */
template <class H, int AMODE, bool PADCONST, bool PREFETCH = H::PREFETCH>
__device__ __forceinline__ void fixed_lane(uint64_t i,
    const uint8_t *__restrict__ base, uint64_t stride, uint32_t len,
    uint8_t *__restrict__ out, uint32_t dlen, int is384,
    const typename H::word *kw)
{
	typename H::State st;
	digest_one<H, AMODE, PADCONST, PREFETCH>(base + i * stride, len, is384,
	    kw, st);
	uint32_t o[16];
	H::out_words(st, o, is384);
	if (dlen == 48)
		store_digest<48>(out + i * 48, o);
	else
		store_digest<H::DLEN>(out + i * H::DLEN, o);
}

/* (no occupancy request: 6 waves per SIMD asked of the fixed SHA-512
 * kernel measured -1.4 %, profiles/round2/occupancy_request_ab.txt) */
template <class H, int AMODE, bool PADCONST>
__global__ __launch_bounds__(256) void fixed_kernel(const uint8_t *__restrict__ base,
    uint64_t stride, uint32_t len, uint64_t n, uint8_t *__restrict__ out,
    uint32_t dlen, int is384, PadKW<typename H::word> pad)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (sizeof(typename H::word) == 8) {
		if (PADCONST)
			k512_lds_fill_pad(pad);
		else
			k512_lds_fill();
	}
	if (i >= n)
		return;
	fixed_lane<H, AMODE, PADCONST>(i, base, stride, len, out, dlen, is384,
	    pad.kw);
}

/*
 * K[t] + W[t] of the SHA-256 pad block of every message whose length is a
 * whole number of blocks, 64 * j bytes for j < NET2_PADTAB_N (up to
 * 65,536-byte payloads plus an HMAC key block): 0x80, zero fill, bit count
 * 512 * j (SHA256Pad for usedspace == 0, src/sha2.c:520-526).  Evaluated
 * at compile time into constant memory, so a wave whose lanes all carry the
 * same such length reads its pad schedule with scalar loads instead of
 * expanding it (48 of 64 schedule words, ~480 VALU instructions per lane),
 * as fixed_kernel does with its kernel-argument copy.
 */
#define NET2_PADTAB_N 1026

struct PadTab256 {
	uint32_t kw[NET2_PADTAB_N][64];
};

constexpr uint32_t cx_ror32(uint32_t x, int n)
{
	return (x >> n) | (x << (32 - n));
}

constexpr PadTab256 make_padtab256()
{
	PadTab256 t{};
	for (int j = 0; j < NET2_PADTAB_N; j++) {
		uint32_t w[64] = {};
		const uint64_t bits = (uint64_t)j * 512;
		w[0] = 0x80000000u;
		w[14] = (uint32_t)(bits >> 32);
		w[15] = (uint32_t)bits;
		for (int r = 16; r < 64; r++) {
			const uint32_t s0 = cx_ror32(w[r - 15], 7) ^
			    cx_ror32(w[r - 15], 18) ^ (w[r - 15] >> 3);
			const uint32_t s1 = cx_ror32(w[r - 2], 17) ^
			    cx_ror32(w[r - 2], 19) ^ (w[r - 2] >> 10);
			w[r] = w[r - 16] + s0 + w[r - 7] + s1;
		}
		for (int r = 0; r < 64; r++)
			t.kw[j][r] = K256[r] + w[r];
	}
	return t;
}

__constant__ const PadTab256 g_padtab256 = make_padtab256();

/*
 * The wave-uniform pad schedule for messages of `bytes` total bytes (any
 * prefix included), or nullptr when the wave's live lanes differ in length,
 * the length is not a whole number of blocks or lies past the table.
 */
template <class H>
__device__ __forceinline__ const typename H::word *uniform_pad_kw(bool live,
    uint64_t bytes)
{
	if (sizeof(typename H::word) != 4)
		return nullptr;
	const uint32_t lo = (uint32_t)bytes;
	const uint32_t b0 = __builtin_amdgcn_readfirstlane(lo);
	if (!__all(!live || bytes == b0) || b0 % 64 != 0 ||
	    b0 / 64 >= NET2_PADTAB_N)
		return nullptr;
	return reinterpret_cast<const typename H::word *>(
	    g_padtab256.kw[b0 / 64]);
}

/*
 * The SHA-512 counterpart: K[t] + W[t] of the pad block of a 128 * j byte
 * message (0x80, zeros, 128-bit bit count 1024 * j; SHA512Pad,
 * src/sha2.c:784-832) for j < NET2_PADTAB512_N, 329 KB of constant memory.
 * SHA-512 compressions read their round constants from the workgroup's LDS
 * copy (k512_lds, sha2_device.h), so the table row is staged there, in the
 * [80, 160) half the fixed kernel's constant pad block uses; that makes the
 * choice per workgroup: every live lane of it must share the length.
 */
#define NET2_PADTAB512_N 514

struct PadTab512 {
	uint64_t kw[NET2_PADTAB512_N][80];
};

constexpr uint64_t cx_ror64(uint64_t x, int n)
{
	return (x >> n) | (x << (64 - n));
}

constexpr PadTab512 make_padtab512()
{
	PadTab512 t{};
	for (int j = 0; j < NET2_PADTAB512_N; j++) {
		uint64_t w[80] = {};
		w[0] = 0x8000000000000000ull;
		w[15] = (uint64_t)j * 1024;	/* w[14]: high half of the count */
		for (int r = 16; r < 80; r++) {
			const uint64_t s0 = cx_ror64(w[r - 15], 1) ^
			    cx_ror64(w[r - 15], 8) ^ (w[r - 15] >> 7);
			const uint64_t s1 = cx_ror64(w[r - 2], 19) ^
			    cx_ror64(w[r - 2], 61) ^ (w[r - 2] >> 6);
			w[r] = w[r - 16] + s0 + w[r - 7] + s1;
		}
		for (int r = 0; r < 80; r++)
			t.kw[j][r] = K512[r] + w[r];
	}
	return t;
}

__constant__ const PadTab512 g_padtab512 = make_padtab512();

/*
 * Workgroup-uniform whole-block length for SHA-512: stage its pad schedule
 * in k512_lds[80, 160) and return true.  Called by every thread of the
 * workgroup (it synchronises), after k512_lds_fill().
 */
__device__ __forceinline__ bool block_pad512(bool live, uint64_t bytes)
{
	__shared__ uint64_t b0s;
	if (threadIdx.x == 0)
		b0s = live ? bytes : 1;	/* thread 0 is live if any thread is */
	__syncthreads();
	const uint64_t b0 = b0s;
	const bool same = __syncthreads_and(!live || bytes == b0);
	if (!same || b0 % 128 != 0 || b0 / 128 >= NET2_PADTAB512_N)
		return false;
	for (unsigned t = threadIdx.x; t < 80; t += blockDim.x)
		k512_lds[80 + t] = g_padtab512.kw[b0 / 128][t];
	__syncthreads();
	return true;
}

/* The state as big-endian digest words (SHA*Final's byte order). */
template <class H>
__device__ __forceinline__ int digest_words(const typename H::State &st,
    int is384, uint32_t (&w)[H::NW32])
{
	if (sizeof(typename H::word) == 4) {
#pragma unroll
		for (int i = 0; i < 8; i++)
			w[i] = (uint32_t)st[i];
		return 8;
	}
#pragma unroll
	for (int i = 0; i < 8; i++) {
		w[2 * i] = hi32((uint64_t)st[i]);
		w[2 * i + 1] = lo32((uint64_t)st[i]);
	}
	return is384 ? 12 : 16;
}

/* Midstate `which` (0 inner, 1 outer) from LDS into a state. */
template <class H>
__device__ __forceinline__ void load_mid(const uint32_t (*mid)[16], int which,
    typename H::State &st)
{
	/* opaque zero: keeps the reads where they are written (not hoisted
	 * and shared across the address-mode branches) */
	uint32_t z;
	asm volatile("s_mov_b32 %0, 0" : "=s"(z));
	mid += z;
#pragma unroll
	for (int i = 0; i < 8; i++) {
		if (sizeof(typename H::word) == 4)
			st[i] = mid[which][i];
		else
			st[i] = mk64(mid[which][2 * i + 1], mid[which][2 * i]);
	}
}

/* digest_one for the variable layout: one block loop, and the pad block
 * from the constant table when the wave (SHA-256: kw) or the workgroup
 * (SHA-512: k512_lds) has one. */
template <class H, int AMODE, bool PREFETCH = H::PREFETCH>
__device__ __forceinline__ void var_digest(const uint8_t *p, uint32_t len,
    int is384, const typename H::word *kw, bool padtab, typename H::State &st)
{
	H::init(st, is384);
	absorb<H, AMODE, PREFETCH>(p, len, st);
	if (padtab)
		finish<H, true>(p, len, 0, kw, st);
	else
		finish<H, false>(p, len, (uint64_t)len << 3, nullptr, st);
}

/*
 * The visiting order a launch's binning left in ws (sha2_launch.h): perm,
 * or submission order (nullptr) when ws is NULL or when that binning launch
 * -- the one tagged `launch` -- found its global histogram inconsistent
 * (BinHdr::bad == launch, bin_onepass_kernel): its workgroups may then have
 * written a mix of binned and identity positions.  One scalar load.
 */
__device__ __forceinline__ const uint32_t *bin_perm(
    const uint32_t *__restrict__ ws, uint32_t launch)
{
	if (ws == nullptr || ws[NET2_BIN_W_BAD] == launch)
		return nullptr;
	return ws + NET2_BIN_WS_WORDS;
}

/*
 * Variable-length packets, visited in binned order: lane g hashes packet
 * perm[g] (perm == NULL: identity).  The address mode is chosen per wave:
 * if every lane's packet start is 16-byte aligned the wave takes the vector
 * load path, else the byte-aligned one.  A SHA-256 wave (SHA-512:
 * workgroup) of one whole-block length, e.g. a bin of a batch of fixed
 * sizes, takes its pad schedule from g_padtab256 (g_padtab512).
 * (No occupancy request: 5 waves asked of the variable-length SHA-256
 * kernel measured flat, of the SHA-512 one -2 %,
 * profiles/round2/occupancy_request_ab.txt.)
 */
/* One packet of var_kernel: binned position g (SHA-512: block_pad512 is a
 * workgroup barrier, so every thread calls this equally often). */
template <class H>
__device__ __forceinline__ void var_item(uint64_t g,
    const uint8_t *__restrict__ base, const uint64_t *__restrict__ offsets,
    const uint32_t *__restrict__ lens, const uint32_t *__restrict__ perm,
    uint64_t n, uint8_t *__restrict__ out, uint32_t dlen, int is384)
{
	const bool live = g < n;
	uint64_t i = live ? (perm ? (uint64_t)perm[g] : g) : 0;
	if (i >= n)	/* a corrupt workspace: never read out of bounds */
		i = g;
	const uint8_t *p = base + (live ? offsets[i] : 0);
	const uint32_t len = live ? lens[i] : 0;
	typename H::State st;
	const typename H::word *kw = uniform_pad_kw<H>(live, len);
	bool padtab = kw != nullptr;
	if constexpr (sizeof(typename H::word) == 8)
		padtab = block_pad512(live, len);

	if (OnePath<H>::value ||
	    __all((reinterpret_cast<uintptr_t>(p) & 15) == 0))
		var_digest<H, AMODE_A16>(p, len, is384, kw, padtab, st);
	else if (__all((reinterpret_cast<uintptr_t>(p) & 3) == 0))
		var_digest<H, AMODE_A4>(p, len, is384, kw, padtab, st);
	else
		/* no prefetch on the byte-aligned path: its double buffer
		 * (17 words each) set the kernel's VGPRs (105 against 96, 5
		 * waves); C3 +0.3 %, byte-aligned mix +0.7 % without,
		 * profiles/round2/var_a1_prefetch_ab.txt */
		var_digest<H, AMODE_A1, false>(p, len, is384, kw, padtab, st);
	materialize<H>(st);
	if (!live)
		return;
	uint32_t o[16];
	H::out_words(st, o, is384);
	if (dlen == 48)
		store_digest<48>(out + i * 48, o);
	else
		store_digest<H::DLEN>(out + i * H::DLEN, o);
}

/* ws: the binning workspace of this launch (NULL: submission order). */
template <class H>
__global__ __launch_bounds__(256) void var_kernel(const uint8_t *__restrict__ base,
    const uint64_t *__restrict__ offsets, const uint32_t *__restrict__ lens,
    const uint32_t *__restrict__ ws, uint32_t launch, uint64_t n,
    uint8_t *__restrict__ out, uint32_t dlen, int is384)
{
	if (sizeof(typename H::word) == 8)
		k512_lds_fill();
	var_item<H>((uint64_t)blockIdx.x * blockDim.x + threadIdx.x, base,
	    offsets, lens, bin_perm(ws, launch), n, out, dlen, is384);
}

} /* namespace dev */
} /* namespace net2 */

#endif /* NET2_SHA2_DIGEST_H */
