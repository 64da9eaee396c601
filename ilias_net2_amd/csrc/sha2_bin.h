/*
 * sha2_bin.h -- length binning of variable-length batches.
 * One of the device headers of sha2_kernels.hip, which includes them in
 * order into one translation unit.
 */
#ifndef NET2_SHA2_BIN_H
#define NET2_SHA2_BIN_H

#include "sha2_launch.h"
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace net2 {
namespace dev {

/* ---- length binning (counting sort by block count, longest first) ---- */

__device__ __forceinline__ uint32_t bin_of(uint32_t len, int blk_shift,
    int lenbytes, uint32_t nbins)
{
	/* total compressions the message needs, including padding */
	uint64_t nb = (((uint64_t)len + lenbytes + 1 + (1u << blk_shift) - 1) >>
	    blk_shift);
	uint32_t b = nb >= nbins ? nbins - 1 : (uint32_t)nb;
	return nbins - 1 - b;	/* descending block count */
}

/* Packets per thread in the binning: one workgroup bins a tile of
 * 256 x 16 = 4,096 packets (the whole 256-workgroup grid covers 1 M packets
 * with one tile each).  Every workgroup pays a fixed cost (clearing the
 * 2,048-bin LDS histogram, the histogram scan, its global atomics), so
 * fewer, larger tiles win down to 4,096 packets; 2,048 and 8,192 measured
 * slower (profiles/round1/binning_time_ab.txt, three-launch binning;
 * profiles/round4/bin_probe_items32_tiles8192.txt, this kernel). */
constexpr int kBinItems = 16;
#define NET2_BIN_TILE (256 * kBinItems)
/* A thread's kBinItems lengths, all loads issued before any is used. */
__device__ __forceinline__ void load_lens(const uint32_t *__restrict__ lens,
    uint64_t n, uint64_t i0, uint32_t (&len)[kBinItems])
{
#pragma unroll
	for (int k = 0; k < kBinItems; k++) {
		const uint64_t i = i0 + (uint64_t)k * 256;
		len[k] = i < n ? lens[i] : 0u;
	}
}

/*
 * Binning in one launch (round 4; until round 3 a memset, a count and a
 * scatter launch): the count, the global prefix and the scatter, no memset.
 * A persistent grid of G workgroups -- at most 256, and no more than the
 * device holds at once (the host caps G at the co-resident capacity of this
 * kernel, net2_bin_order) -- each looping over its 4,096-packet tiles:
 *   1. LDS histogram of its tiles, each packet's rank in its bin kept in
 *      registers (the LDS atomic's return value), then one device-scope
 *      fetch-add per touched bin into the global histogram, whose old value
 *      is where the workgroup's packets start inside that bin;
 *   2. a grid barrier in two levels: 16 group counters (workgroup
 *      blockIdx & 15, one XCD each), the last of each group arrives at a top
 *      counter, the last of those flips `state` to GO and bumps the epoch;
 *      everyone polls `state`;
 *   3. every workgroup scans the global histogram (8 KiB) for the bin
 *      bases and writes perm[base + start + rank] -- no claim pass, no
 *      second read of the lengths (a workgroup with several tiles ranks
 *      them again from the same starts).
 * The workspace cleans up after itself: the histogram and the barrier words
 * come in two parities (the epoch selects); each launch zeroes the parity
 * the next launch uses, so nothing waits for the last workgroup to leave.
 *
 * Never a hang, never a wrong order, and every fallback counted in the
 * header (net2_sha2_workspace_stats):
 *   - a barrier that does not complete within the timeout (the grid not
 *     co-resident, e.g. beside long kernels on other streams) is decided
 *     ABORT by one compare-and-swap on `state`, which every workgroup then
 *     follows: all write the identity order (perm[i] = i, hashing in
 *     submission order: correct, only slower), the header is marked for
 *     re-initialisation and NET2_BIN_W_ABORTS counts it;
 *   - a header is valid when its tag holds the magic and the id of a launch
 *     other than this one; otherwise (fresh memory, after an ABORT or a
 *     mismatch -- which leave a re-init mark, so the counters survive -- or
 *     prepared by workgroup 0 of this very launch -- a workgroup dispatched
 *     after workgroup 0 re-tagged it must not join a barrier the early ones
 *     skipped) every workgroup takes the identity order while workgroup 0
 *     initialises the header and both parities, so the next launch bins
 *     (NET2_BIN_W_UNPREP counts it);
 *   - after the barrier every workgroup checks that the global histogram
 *     adds up to n (64-bit sum): anything else -- stale counts, or barrier
 *     words someone else overwrote (a caller reusing the workspace for other
 *     data) -- marks the launch bad (NET2_BIN_W_BAD = its id,
 *     NET2_BIN_W_MISMATCH counts it) and clears the magic.  Workgroups that
 *     read the histogram at different times may then have written a mix of
 *     orders, so the hash kernel of this launch, given the same id, hashes
 *     in submission order instead (bin_perm);
 *   - the hash kernels clamp perm entries to [0, n) (a corrupt workspace
 *     can cost the binning, never an out-of-bounds access).
 * The workspace must not be used by two launches at once (as before).
 *
 * Memory ordering.  What crosses the barrier is the histogram, written and
 * read only by device-scope atomics, each workgroup's adds returned before
 * it arrives; the plain stores (perm, the next parity's zeroes) are read
 * only by later launches.  So the barrier needs no cache maintenance: its
 * atomics are relaxed.  On gfx950 an agent-scope release writes back the
 * XCD's L2 and an acquire invalidates it; with acq_rel arrivals and an
 * acquire fence the launch measured ~15 % longer, with an acquiring load
 * per poll ~3x (profiles/round4/bin_probe_*.txt).
 */
#define BIN_ORD __ATOMIC_RELAXED
constexpr int kBinSpinSleep = 2;
#define NET2_BIN_GROUPS 16
/*
 * Barrier words, per parity, in the workspace after the two histograms
 * (each word on its own 128-byte line): group counters at 32 g, the top counter
 * at 512, the state at 544.  Words 2,048-4,095 of the area hold the probe
 * stamps (NET2_BIN_PROBE=1, tools/bin_probe.py: thread 0 of every
 * workgroup stamps the 100 MHz clock at seven points; a measurement build,
 * never the shipped one).
 */
#define BIN_CTL_PAR 1024
#define BIN_CTL_TOP 512
#define BIN_CTL_STATE 544
#ifndef NET2_BIN_PROBE
#define NET2_BIN_PROBE 0
#endif
#define BIN_STAMP(p) do { if (NET2_BIN_PROBE && threadIdx.x == 0) \
	ctl0[2048 + blockIdx.x * 8 + (p)] = (uint32_t)wall_clock64(); } while (0)
#define NET2_BIN_MAGIC32 0x4e324253u	/* "N2BS" */
/* the tag after an ABORT or a mismatch: re-initialise, counters kept */
#define NET2_BIN_REINIT32 0x4e325249u	/* "N2RI" */
#define NET2_BIN_GRID 256
/* 50 ms of the 100 MHz s_memrealtime clock */
#define NET2_BIN_TIMEOUT 5000000ull
/* the first bin of packets that need at most two compressions */
#define NET2_BIN_SHORT (NET2_SHA2_NBINS - 3)

static_assert(NET2_BIN_CTL + 2048 + NET2_BIN_GRID * 8 <= NET2_BIN_WS_WORDS,
    "probe words");
static_assert(NET2_BIN_HDR + 2 * NET2_SHA2_NBINS <= NET2_BIN_CTL,
    "histograms");
static_assert(NET2_BIN_W_BINNED < NET2_BIN_HDR, "header words");
static_assert(BIN_CTL_STATE < BIN_CTL_PAR && 32 * NET2_BIN_GROUPS <= BIN_CTL_TOP,
    "barrier words");
static_assert(NET2_BIN_SHORT / (NET2_SHA2_NBINS / 256) == 255,
    "the short tail's first bin is the last thread's");
enum { BIN_UNDECIDED = 0, BIN_GO = 1, BIN_ABORT = 2 };

__device__ __forceinline__ uint32_t ld_agent(const uint32_t *p)
{
	return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void add_agent(uint32_t *p, uint32_t v)
{
	(void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED,
	    __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint64_t *bin_tag(uint32_t *ws)
{
	return reinterpret_cast<uint64_t *>(ws + NET2_BIN_W_TAG);
}

/* perm[i] = i for this workgroup's tiles */
__device__ __forceinline__ void bin_identity(uint32_t *perm, uint64_t n,
    uint64_t ntiles)
{
	for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x)
		for (int k = 0; k < kBinItems; k++) {
			const uint64_t i = t * NET2_BIN_TILE + (uint64_t)k * 256 +
			    threadIdx.x;
			if (i < n)
				perm[i] = (uint32_t)i;
		}
}

__global__ __launch_bounds__(256) void bin_onepass_kernel(
    const uint32_t *__restrict__ lens, uint64_t n, int blk_shift,
    int lenbytes, uint32_t *__restrict__ ws, uint64_t timeout,
    uint32_t launch)
{
	__shared__ uint32_t cnt[NET2_SHA2_NBINS];
	__shared__ uint32_t start[NET2_SHA2_NBINS];
	__shared__ uint32_t wsum[4];
	__shared__ uint64_t wtot[4];
	__shared__ uint32_t bc[2];
	uint32_t *hist0 = ws + NET2_BIN_HDR;		/* [2][NBINS] */
	uint32_t *ctl0 = ws + NET2_BIN_CTL;		/* [2][1024] */
	uint32_t *perm = ws + NET2_BIN_WS_WORDS;
	const uint32_t G = gridDim.x;
	const uint64_t ntiles = (n + NET2_BIN_TILE - 1) / NET2_BIN_TILE;
	constexpr uint32_t HW = NET2_SHA2_NBINS;

	/* the first tile's lengths in flight while the header is read */
	uint32_t len[kBinItems];
	load_lens(lens, n, (uint64_t)blockIdx.x * NET2_BIN_TILE + threadIdx.x,
	    len);
	if (threadIdx.x == 0) {
		const uint64_t tag = __hip_atomic_load(bin_tag(ws),
		    __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		bc[0] = (uint32_t)(tag >> 32) == NET2_BIN_MAGIC32 &&
		    (uint32_t)tag != launch;
		bc[1] = ld_agent(&ws[NET2_BIN_W_EPOCH]);
	}
	for (uint32_t b = threadIdx.x; b < NET2_SHA2_NBINS; b += blockDim.x)
		cnt[b] = 0;
	__syncthreads();
	if (!bc[0]) {
		/* not initialised: submission order now, initialise for next */
		bin_identity(perm, n, ntiles);
		if (blockIdx.x == 0) {
			for (uint32_t w = threadIdx.x; w < 2 * HW; w += blockDim.x)
				hist0[w] = 0;
			for (uint32_t w = threadIdx.x; w < 2 * BIN_CTL_PAR;
			    w += blockDim.x)
				ctl0[w] = 0;
			if (threadIdx.x == 0) {
				/* fresh memory (no re-init mark): its counters
				 * are garbage, start them here */
				const uint64_t tag = __hip_atomic_load(bin_tag(ws),
				    __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				if ((uint32_t)(tag >> 32) != NET2_BIN_REINIT32)
					for (int w = NET2_BIN_W_EPOCH + 1;
					    w <= NET2_BIN_W_BINNED; w++)
						ws[w] = 0;
				ws[NET2_BIN_W_EPOCH] = 0;
				add_agent(&ws[NET2_BIN_W_UNPREP], 1u);
			}
			__threadfence();
			__syncthreads();
			if (threadIdx.x == 0)
				__hip_atomic_store(bin_tag(ws),
				    (uint64_t)NET2_BIN_MAGIC32 << 32 | launch,
				    __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
		}
		return;
	}
	BIN_STAMP(0);
	const uint32_t par = bc[1] & 1;
	uint32_t *hist = hist0 + par * HW;
	uint32_t *ctl = ctl0 + par * BIN_CTL_PAR;
	/* the next launch's parity, zeroed: its histogram across the grid, its
	 * barrier words by workgroup 0 */
	for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w < HW;
	    w += G * blockDim.x)
		hist0[(par ^ 1) * HW + w] = 0;
	if (blockIdx.x == 0 && threadIdx.x <= NET2_BIN_GROUPS + 1) {
		const uint32_t w = threadIdx.x < NET2_BIN_GROUPS ? 32 * threadIdx.x :
		    threadIdx.x == NET2_BIN_GROUPS ? BIN_CTL_TOP : BIN_CTL_STATE;
		ctl0[(par ^ 1) * BIN_CTL_PAR + w] = 0;
	}

	/* 1: this workgroup's histogram; the ranks of its first tile's packets
	 * kept in registers */
	uint32_t bin0[kBinItems], rank0[kBinItems];
	for (uint64_t t = blockIdx.x; t < ntiles; t += G) {
		const uint64_t i0 = t * NET2_BIN_TILE + threadIdx.x;
		if (t != blockIdx.x)
			load_lens(lens, n, i0, len);
#pragma unroll
		for (int k = 0; k < kBinItems; k++) {
			const uint32_t bn = bin_of(len[k], blk_shift, lenbytes,
			    NET2_SHA2_NBINS);
			const uint32_t r = i0 + (uint64_t)k * 256 < n ?
			    atomicAdd(&cnt[bn], 1u) : 0u;
			if (t == blockIdx.x) {
				bin0[k] = bn;
				rank0[k] = r;
			}
		}
	}
	__syncthreads();
	BIN_STAMP(1);
	/* into the global histogram: the add's old value is where this
	 * workgroup's packets start inside the bin */
	for (uint32_t b = threadIdx.x; b < NET2_SHA2_NBINS; b += blockDim.x)
		start[b] = cnt[b] != 0 ? __hip_atomic_fetch_add(&hist[b], cnt[b],
		    __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
	__syncthreads();
	BIN_STAMP(2);

	/* 2: grid barrier in two levels, decided GO or ABORT exactly once */
	if (threadIdx.x == 0) {
		const uint32_t ng = G < NET2_BIN_GROUPS ? G : NET2_BIN_GROUPS;
		const uint32_t g = blockIdx.x % NET2_BIN_GROUPS;
		const uint32_t gsize = (G - g + NET2_BIN_GROUPS - 1) /
		    NET2_BIN_GROUPS;
		if (__hip_atomic_fetch_add(&ctl[32 * g], 1u, BIN_ORD,
		    __HIP_MEMORY_SCOPE_AGENT) == gsize - 1 &&
		    __hip_atomic_fetch_add(&ctl[BIN_CTL_TOP], 1u, BIN_ORD,
		    __HIP_MEMORY_SCOPE_AGENT) == ng - 1) {
			/* every workgroup has read the epoch by now */
			__hip_atomic_store(&ws[NET2_BIN_W_EPOCH], bc[1] + 1,
			    __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			uint32_t exp = BIN_UNDECIDED;
			if (__hip_atomic_compare_exchange_strong(
			    &ctl[BIN_CTL_STATE], &exp, (uint32_t)BIN_GO, BIN_ORD,
			    __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
				add_agent(&ws[NET2_BIN_W_BINNED], 1u);
		}
		BIN_STAMP(3);
		const uint64_t t0 = wall_clock64();
		uint32_t st;
		while ((st = ld_agent(&ctl[BIN_CTL_STATE])) == BIN_UNDECIDED) {
			if (wall_clock64() - t0 > timeout) {
				uint32_t exp = BIN_UNDECIDED;
				if (__hip_atomic_compare_exchange_strong(
				    &ctl[BIN_CTL_STATE], &exp,
				    (uint32_t)BIN_ABORT, BIN_ORD, __ATOMIC_RELAXED,
				    __HIP_MEMORY_SCOPE_AGENT))
					add_agent(&ws[NET2_BIN_W_ABORTS], 1u);
			}
			__builtin_amdgcn_s_sleep(kBinSpinSleep);
		}
		BIN_STAMP(4);
		bc[0] = st;
	}
	__syncthreads();
	bool binned = bc[0] == BIN_GO;
	if (binned) {
		/* 3: bin bases from the global histogram (8 bins per thread, a
		 * shuffle scan per wave, the four wave totals) added to the
		 * workgroup's starts, then its packets' places -- once the
		 * histogram is known to add up to n */
		constexpr int PER = NET2_SHA2_NBINS / 256;
		const int lane = (int)__lane_id(), wave = (int)(threadIdx.x / 64);
		/* (The histogram read with coalesced 8-byte loads staged through
		 * LDS, one request per line per workgroup instead of eight:
		 * 0.4 us slower to the bases -- the read is one round trip, not
		 * contention; profiles/round5/bin_probe_coalesced_read.txt.) */
		uint32_t v[PER], sum = 0;
		uint64_t sum64 = 0;
#pragma unroll
		for (int j = 0; j < PER; j++) {
			const uint32_t c = ld_agent(&hist[threadIdx.x * PER + j]);
			v[j] = sum;
			sum += c;
			sum64 += c;
		}
		uint32_t x = sum;
#pragma unroll
		for (int off = 1; off < 64; off <<= 1) {
			const uint32_t y = __shfl_up(x, off);
			if (lane >= off)
				x += y;
			sum64 += __shfl_xor(sum64, off);
		}
		if (lane == 63)
			wsum[wave] = x;
		if (lane == 0)
			wtot[wave] = sum64;
		__syncthreads();
		uint32_t base = x - sum;
		for (int w = 0; w < wave; w++)
			base += wsum[w];
		binned = wtot[0] + wtot[1] + wtot[2] + wtot[3] == n;
		if (binned) {
#pragma unroll
			for (int j = 0; j < PER; j++)
				start[threadIdx.x * PER + j] += base + v[j];
			/* where the packets of at most two compressions start */
			if (blockIdx.x == 0 && threadIdx.x == 255) {
				ws[NET2_BIN_W_TAIL] = base + v[NET2_BIN_SHORT % PER];
				ws[NET2_BIN_W_TAILID] = launch;
			}
		} else if (threadIdx.x == 0) {
			/* the histogram is not this launch's alone: the hash
			 * kernel of this launch ignores the order, and the next
			 * launch re-initialises */
			if (__hip_atomic_exchange(&ws[NET2_BIN_W_BAD], launch,
			    __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != launch)
				add_agent(&ws[NET2_BIN_W_MISMATCH], 1u);
			__hip_atomic_store(bin_tag(ws),
			    (uint64_t)NET2_BIN_REINIT32 << 32, __ATOMIC_RELAXED,
			    __HIP_MEMORY_SCOPE_AGENT);
		}
		__syncthreads();
		BIN_STAMP(5);
	}
	if (binned) {
		if (ntiles <= G) {
			/* one tile: its packets' places from the kept ranks */
			const uint64_t i0 = (uint64_t)blockIdx.x * NET2_BIN_TILE +
			    threadIdx.x;
#pragma unroll
			for (int k = 0; k < kBinItems; k++) {
				const uint64_t i = i0 + (uint64_t)k * 256;
				const uint32_t pos = start[bin0[k]] + rank0[k];
				if (i < n && pos < n)
					perm[pos] = (uint32_t)i;
			}
		} else {
			/* several tiles: rank them again from the starts, one
			 * counter per bin */
			for (uint32_t b = threadIdx.x; b < NET2_SHA2_NBINS;
			    b += blockDim.x)
				cnt[b] = start[b];
			__syncthreads();
			for (uint64_t t = blockIdx.x; t < ntiles; t += G) {
				const uint64_t i0 = t * NET2_BIN_TILE + threadIdx.x;
				load_lens(lens, n, i0, len);
#pragma unroll
				for (int k = 0; k < kBinItems; k++) {
					const uint64_t i = i0 + (uint64_t)k * 256;
					if (i < n) {
						const uint32_t pos = atomicAdd(
						    &cnt[bin_of(len[k], blk_shift,
						    lenbytes, NET2_SHA2_NBINS)], 1u);
						if (pos < n)
							perm[pos] = (uint32_t)i;
					}
				}
			}
		}
		BIN_STAMP(6);
	} else {
		bin_identity(perm, n, ntiles);
		if (bc[0] != BIN_GO && threadIdx.x == 0) {
			/* ABORT: re-initialise at the next launch */
			__hip_atomic_store(bin_tag(ws),
			    (uint64_t)NET2_BIN_REINIT32 << 32, __ATOMIC_RELAXED,
			    __HIP_MEMORY_SCOPE_AGENT);
		}
	}
}

/* Prepares a binning workspace so its first launch bins, its counters
 * zeroed (one workgroup). */
__global__ __launch_bounds__(256) void bin_ws_init_kernel(uint32_t *ws)
{
	for (uint32_t w = threadIdx.x; w < NET2_BIN_WS_WORDS - 2;
	    w += blockDim.x)
		ws[2 + w] = 0;
	__threadfence();
	__syncthreads();
	if (threadIdx.x == 0)
		__hip_atomic_store(bin_tag(ws), (uint64_t)NET2_BIN_MAGIC32 << 32,
		    __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

} /* namespace dev */
} /* namespace net2 */

#endif /* NET2_SHA2_BIN_H */
