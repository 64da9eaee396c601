/*
 * sha2_jobs.h -- the coalescer's job kernels and the schedule-row helpers.
 * One of the device headers of sha2_kernels.hip, which includes them in
 * order into one translation unit.
 */
#ifndef NET2_SHA2_JOBS_H
#define NET2_SHA2_JOBS_H

#include "sha2_digest.h"

namespace net2 {
namespace dev {

/* ---- coalesced small jobs (sha2_coalesce.cpp) ------------------------------- */

/*
 * One lane = one request of the single-message entry points
 * (net2_hashctx_hashiov, the SHA2_CTX streaming calls, net2_ph_to_iv), which
 * the reference runs one payload at a time on threadpool workers
 * (types/signature.n2t:92,147, src/sign.c:298-307, types/packet.n2t:134-142).
 * Concurrent requests are gathered by the host into one staging buffer,
 * every message already padded to whole blocks (SHA*Pad's layout, or the
 * K' ^ ipad block ahead of it for HMAC), so a lane only compresses.
 */
template <class H>
__global__ __launch_bounds__(64) void job_kernel(const uint8_t *__restrict__ stage,
    const Net2Job *__restrict__ jobs, uint32_t n, uint8_t *__restrict__ out,
    uint32_t *done, uint32_t chunk)
{
	constexpr int NW32 = H::NW32;
	typedef typename H::word W;
	if (sizeof(W) == 8)
		k512_lds_fill();
	const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= n)
		return;
	const Net2Job jb = jobs[j];
	const int is384 = (jb.flags & 0xffu) == NET2_ALG_SHA384;
	typename H::State st;
	if (jb.flags & NET2_JOB_STATE) {
		const W *s0 = reinterpret_cast<const W *>(stage + jb.aux);
#pragma unroll
		for (int i = 0; i < 8; i++)
			st[i] = s0[i];
	} else {
		H::init(st, is384);
	}
	/* absorb takes a 32-bit length: a job of 4 GiB or more (nblk up to
	 * UINT32_MAX blocks) goes through in chunks of whole blocks (chunk: a
	 * multiple of 128 below 4 GiB, 2 GiB unless a test asks for less) */
	{
		const uint8_t *q = stage + jb.data;
		uint64_t left = (uint64_t)jb.nblk * H::BLOCK;
		while (left > chunk) {
			absorb<H, AMODE_A16>(q, chunk, st);
			q += chunk;
			left -= chunk;
		}
		absorb<H, AMODE_A16>(q, (uint32_t)left, st);
	}
	if (jb.flags & NET2_JOB_HMAC) {
		/* outer hash: IV, K' ^ opad, inner digest || 0x80 || bit count */
		uint32_t w[NW32];
#pragma unroll
		for (int i = 0; i < NW32; i++)
			w[i] = 0;
		const int dw = digest_words<H>(st, is384, w);
#pragma unroll
		for (int i = 12; i < 16; i++)		/* SHA-384 keeps 12 words */
			if (i >= dw)
				w[i] = 0;
		w[dw] = 0x80000000u;
		const uint64_t obits = (uint64_t)(H::BLOCK + 4 * dw) << 3;
		w[NW32 - 2] = (uint32_t)(obits >> 32);
		w[NW32 - 1] = (uint32_t)obits;
		H::init(st, is384);
		Raw<NW32> r;
		issue_block<NW32, AMODE_A16>(stage + jb.aux, r);
		uint32_t kb[NW32];
		finish_block<NW32, AMODE_A16>(stage + jb.aux, r, kb);
		H::compress(st, kb);
		H::compress(st, w);
	}
	W *o = reinterpret_cast<W *>(out + 64 * (size_t)j);
#pragma unroll
	for (int i = 0; i < 8; i++)
		o[i] = st[i];
	/* count the wave in once all of its lanes' results are visible to the
	 * host (the workgroup is one wave; lane 0 is always live) */
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
	if (threadIdx.x == 0)
		__hip_atomic_fetch_add(done, 1u, __ATOMIC_RELEASE,
		    __HIP_MEMORY_SCOPE_SYSTEM);
}

/*
 * Latency form of job_kernel: one wave per job, for batches small enough
 * that the GPU is otherwise idle (a lone caller, a few threads).  A lane of
 * job_kernel runs message expansion and rounds of every block one after the
 * other; here the 64 lanes first expand up to 64 blocks of the job at once
 * (block b's K[t] + W[t] by lane b, into LDS -- the schedule of a block
 * depends only on its message words, not on the chaining state), then the
 * wave runs only the rounds, block after block, reading K + W from LDS.
 * About a third of a compression's instructions leave the serial chain.
 */
#define NET2_JOB_ROW256 65	/* dwords per LDS row: odd, so the 64 lanes'
				 * row writes fall in distinct banks */
#define NET2_JOB_ROW512 81	/* qwords per row */

template <int T>
struct Sched256 {
	__device__ __forceinline__ static void run(uint32_t (&w)[16],
	    uint32_t *row)
	{
		const uint32_t wt = T < 16 ? w[T & 15] : expand256<T, false>(w);
		row[T] = wt + K256[T];
		Sched256<T + 1>::run(w, row);
	}
};
template <>
struct Sched256<64> {
	__device__ __forceinline__ static void run(uint32_t (&)[16], uint32_t *) {}
};

template <int T>
struct Sched512 {
	__device__ __forceinline__ static void run(uint64_t (&w)[16],
	    uint64_t *row, const lds_k64 *kb)
	{
		const uint64_t wt = T < 16 ? w[T & 15] : expand512<T>(w);
		row[T] = addk512<T>(wt, kb);
		Sched512<T + 1>::run(w, row, kb);
	}
};
template <>
struct Sched512<80> {
	__device__ __forceinline__ static void run(uint64_t (&)[16], uint64_t *,
	    const lds_k64 *) {}
};

template <int T>
struct RowRounds512 {
	__device__ __forceinline__ static void run(uint64_t (&s)[8],
	    const uint64_t *row)
	{
		round512<T>(s, row[T]);
		RowRounds512<T + 1>::run(s, row);
	}
};
template <>
struct RowRounds512<80> {
	__device__ __forceinline__ static void run(uint64_t (&)[8],
	    const uint64_t *) {}
};

/* Expand block `blk` (big-endian words) into its K + W row. */
template <class H>
__device__ __forceinline__ void sched_row(uint32_t (&blk)[H::NW32],
    typename H::word *row)
{
	if constexpr (sizeof(typename H::word) == 4) {
		Sched256<0>::run(blk, row);
	} else {
		uint64_t w[16];
#pragma unroll
		for (int i = 0; i < 16; i++)
			w[i] = mk64(blk[2 * i + 1], blk[2 * i]);
		Sched512<0>::run(w, row, k512_base());
	}
}

/* The rounds of one block from its K + W row (all lanes, same state). */
template <class H>
__device__ __forceinline__ void rounds_row(typename H::State &st,
    const typename H::word *row)
{
	if constexpr (sizeof(typename H::word) == 4) {
		compress256_kw<H::ASM>(st, row);
	} else {
		uint64_t s[8];
#pragma unroll
		for (int i = 0; i < 8; i++)
			s[i] = st[i];
		RowRounds512<0>::run(s, row);
#pragma unroll
		for (int i = 0; i < 8; i++)
			st[i] += s[i];
	}
}

template <class H>
__global__ __launch_bounds__(64) void job_wave_kernel(const uint8_t *__restrict__ stage,
    const Net2Job *__restrict__ jobs, uint8_t *__restrict__ out,
    uint32_t *done)
{
	constexpr int NW32 = H::NW32;
	typedef typename H::word W;
	constexpr int ROW = sizeof(W) == 4 ? NET2_JOB_ROW256 : NET2_JOB_ROW512;
	__shared__ W rows[64 * ROW];
	if (sizeof(W) == 8)
		k512_lds_fill();
	const uint32_t lane = threadIdx.x;
	const Net2Job jb = jobs[blockIdx.x];
	const int is384 = (jb.flags & 0xffu) == NET2_ALG_SHA384;
	typename H::State st;
	if (jb.flags & NET2_JOB_STATE) {
		const W *s0 = reinterpret_cast<const W *>(stage + jb.aux);
#pragma unroll
		for (int i = 0; i < 8; i++)
			st[i] = s0[i];
	} else {
		H::init(st, is384);
	}
	const uint8_t *p = stage + jb.data;
	for (uint32_t c0 = 0; c0 < jb.nblk; c0 += 64) {
		const uint32_t nb = min(64u, jb.nblk - c0);
		if (lane < nb) {
			const uint8_t *bp = p + (size_t)(c0 + lane) * H::BLOCK;
			Raw<NW32> r;
			issue_block<NW32, AMODE_A16>(bp, r);
			uint32_t w[NW32];
			finish_block<NW32, AMODE_A16>(bp, r, w);
			sched_row<H>(w, rows + lane * ROW);
		}
		__syncthreads();
		for (uint32_t b = 0; b < nb; b++)
			rounds_row<H>(st, rows + b * ROW);
		__syncthreads();
	}
	if (jb.flags & NET2_JOB_HMAC) {
		uint32_t w[NW32];
#pragma unroll
		for (int i = 0; i < NW32; i++)
			w[i] = 0;
		const int dw = digest_words<H>(st, is384, w);
#pragma unroll
		for (int i = 12; i < 16; i++)
			if (i >= dw)
				w[i] = 0;
		w[dw] = 0x80000000u;
		const uint64_t obits = (uint64_t)(H::BLOCK + 4 * dw) << 3;
		w[NW32 - 2] = (uint32_t)(obits >> 32);
		w[NW32 - 1] = (uint32_t)obits;
		H::init(st, is384);
		Raw<NW32> r;
		issue_block<NW32, AMODE_A16>(stage + jb.aux, r);
		uint32_t kb[NW32];
		finish_block<NW32, AMODE_A16>(stage + jb.aux, r, kb);
		H::compress(st, kb);
		H::compress(st, w);
	}
	if (lane == 0) {
		W *o = reinterpret_cast<W *>(out + 64 * (size_t)blockIdx.x);
#pragma unroll
		for (int i = 0; i < 8; i++)
			o[i] = st[i];
	}
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
	if (lane == 0)
		__hip_atomic_fetch_add(done, 1u, __ATOMIC_RELEASE,
		    __HIP_MEMORY_SCOPE_SYSTEM);
}

} /* namespace dev */
} /* namespace net2 */

#endif /* NET2_SHA2_JOBS_H */
