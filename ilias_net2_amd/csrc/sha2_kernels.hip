/*
 * sha2_kernels.hip -- batched SHA-256/384/512 digests for gfx950 (MI355X).
 *
 * The reference hashes one payload at a time on a host thread:
 * SHA{256,512}Init -> Update (per iovec) -> Final (src/sha2.c:280-563,
 * :566-919), called from net2_signature_create/validate
 * (types/signature.n2t:92,147) and net2_signctx_fingerprint
 * (src/sign.c:298-307).  Here one wavefront lane owns one packet and runs
 * Init/Update/Pad/Final for it entirely in registers; a launch covers a whole
 * batch of independent packets.
 *
 * Layouts (device memory):
 *   fixed  : packet i = base[i * stride .. i * stride + len)
 *   var    : packet i = base[offsets[i] .. offsets[i] + lens[i])
 *   digests: digest i at out + i * digest_len (32 / 48 / 64 bytes)
 * Variable-length batches are length-binned first (bin_* kernels, sha2_bin.h) so
 * that the lanes of a wave share a block count: an unbinned {64,512,1500} B
 * mix runs every wave at the 24-block worst case, binned at the average.
 *
 * The block loop is VALU-bound (~1,400 integer ops per 64-byte SHA-256
 * block), so the memory side only has to keep loads in flight: each lane
 * prefetches block k+1 while compressing block k.
 */
#include "sha2_device.h"
#include "sha2_keyprep.h"
#include "sha2_launch.h"

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <type_traits>

/* the device code, by kernel family; the order is part of the build id */
#include "sha2_hash.h"
#include "sha2_digest.h"
#include "sha2_hmac.h"
#include "sha2_jobs.h"
#include "sha2_burst.h"
#include "sha2_burst_wave.h"
#include "sha2_bin.h"

/* ---- launch wrappers (C++ linkage, used by the C-ABI shim) ------------ */

using namespace net2::dev;

static inline unsigned grid_for(uint64_t n)
{
	return (unsigned)((n + 255) / 256);
}

hipError_t net2_launch_fixed(int alg, const uint8_t *base, uint64_t stride,
    uint32_t len, uint64_t n, uint8_t *out, hipStream_t s)
{
	const bool a16 = ((reinterpret_cast<uintptr_t>(base) | stride) & 15) == 0;
	const unsigned grid = grid_for(n);
	if (n == 0)
		return hipSuccess;
	if (alg == NET2_ALG_SHA256) {
		PadKW<uint32_t> pad;
		const bool padc = len % 64 == 0;
		if (padc)
			pad_kw256((uint64_t)len << 3, pad);
		if (a16 && padc)
			fixed_kernel<Sha256, AMODE_A16, true><<<grid, 256, 0, s>>>(
			    base, stride, len, n, out, 32, 0, pad);
		else if (a16)
			fixed_kernel<Sha256, AMODE_A16, false><<<grid, 256, 0, s>>>(
			    base, stride, len, n, out, 32, 0, pad);
		else
			fixed_kernel<Sha256, AMODE_A1, false><<<grid, 256, 0, s>>>(
			    base, stride, len, n, out, 32, 0, pad);
	} else {
		const int is384 = alg == NET2_ALG_SHA384;
		const uint32_t dlen = is384 ? 48 : 64;
		PadKW<uint64_t> pad;
		const bool padc = len % 128 == 0;
		if (padc)
			pad_kw512((uint64_t)len << 3, pad);
		if (a16 && padc)
			fixed_kernel<Sha512, AMODE_A16, true><<<grid, 256, 0, s>>>(
			    base, stride, len, n, out, dlen, is384, pad);
		else if (a16)
			fixed_kernel<Sha512, AMODE_A16, false><<<grid, 256, 0, s>>>(
			    base, stride, len, n, out, dlen, is384, pad);
		else
			fixed_kernel<Sha512, AMODE_A1, false><<<grid, 256, 0, s>>>(
			    base, stride, len, n, out, dlen, is384, pad);
	}
	return hipGetLastError();
}

hipError_t net2_bin_ws_init(uint32_t *ws, hipStream_t s)
{
	bin_ws_init_kernel<<<1, 256, 0, s>>>(ws);
	return hipGetLastError();
}

/*
 * Binning limits: the grid cap (0: the device's co-resident capacity) and
 * the barrier timeout in 100 MHz ticks, set by net2_sha2_bin_limits
 * (diagnostics and tests; read once per launch from two atomics, no
 * environment lookups on the launch path).
 */
static std::atomic<uint32_t> g_bin_grid_cap{0};
static std::atomic<uint64_t> g_bin_timeout{NET2_BIN_TIMEOUT};

void net2_bin_set_limits(uint32_t grid_cap, int64_t timeout_us)
{
	g_bin_grid_cap.store(grid_cap, std::memory_order_relaxed);
	g_bin_timeout.store(timeout_us < 0 ? NET2_BIN_TIMEOUT :
	    (uint64_t)timeout_us * 100, std::memory_order_relaxed);
}

/*
 * The persistent grid's size: at most 256 workgroups and no more than the
 * device can hold at once (workgroups per CU x CUs), cached per device --
 * on a partitioned device (a CPX partition has 32 CUs) 256 workgroups need
 * not all be resident, and the barrier would wait out its timeout on
 * every launch.
 */
static uint32_t bin_resident_grid()
{
	static std::atomic<uint32_t> cache[64];
	int dev = 0;
	if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) {
		(void)hipGetLastError();
		return NET2_BIN_GRID;
	}
	uint32_t g = cache[dev].load(std::memory_order_relaxed);
	if (g != 0)
		return g;
	int per_cu = 0, cus = 0;
	if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu,
	    bin_onepass_kernel, 256, 0) != hipSuccess ||
	    hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
	    dev) != hipSuccess || per_cu <= 0 || cus <= 0) {
		(void)hipGetLastError();
		g = 1;		/* one workgroup is always resident */
	} else {
		g = (uint32_t)std::min<int64_t>(NET2_BIN_GRID,
		    (int64_t)per_cu * cus);
	}
	cache[dev].store(g, std::memory_order_relaxed);
	return g;
}

/* A launch id for the binning and the hash kernel that reads its order:
 * never 0 (the id of net2_bin_ws_init). */
static uint32_t next_bin_launch()
{
	static std::atomic<uint32_t> seq{0};
	uint32_t id;
	do
		id = seq.fetch_add(1, std::memory_order_relaxed) + 1;
	while (id == 0);
	return id;
}

/* Length-binned visiting order of a variable-length batch into ws. */
hipError_t net2_bin_order(int alg, const uint32_t *lens, uint64_t n,
    uint32_t *ws, hipStream_t s, uint32_t *launch)
{
	const bool s256 = alg == NET2_ALG_SHA256;
	const int blk_shift = s256 ? 6 : 7;
	const int lenbytes = s256 ? 8 : 16;
	const uint64_t tiles = (n + NET2_BIN_TILE - 1) / NET2_BIN_TILE;
	uint32_t cap = bin_resident_grid();
	const uint32_t forced = g_bin_grid_cap.load(std::memory_order_relaxed);
	if (forced != 0 && forced < cap)
		cap = forced;
	const unsigned g = (unsigned)(tiles < cap ? tiles : cap);
	*launch = next_bin_launch();
	bin_onepass_kernel<<<g, 256, 0, s>>>(lens, n, blk_shift, lenbytes, ws,
	    g_bin_timeout.load(std::memory_order_relaxed), *launch);
	return hipGetLastError();
}

hipError_t net2_launch_var(int alg, const uint8_t *base,
    const uint64_t *offsets, const uint32_t *lens, uint64_t n, uint8_t *out,
    uint32_t *ws, hipStream_t s)
{
	if (n == 0)
		return hipSuccess;
	const bool s256 = alg == NET2_ALG_SHA256;
	const int is384 = alg == NET2_ALG_SHA384;
	const uint32_t dlen = s256 ? 32 : is384 ? 48 : 64;
	uint32_t launch = 0;

	if (ws != nullptr) {
		hipError_t e = net2_bin_order(alg, lens, n, ws, s, &launch);
		if (e != hipSuccess)
			return e;
	}
	if (s256)
		var_kernel<Sha256V><<<grid_for(n), 256, 0, s>>>(base, offsets,
		    lens, ws, launch, n, out, dlen, 0);
	else
		var_kernel<Sha512V><<<grid_for(n), 256, 0, s>>>(base, offsets,
		    lens, ws, launch, n, out, dlen, is384);
	return hipGetLastError();
}

/* ---- the keyed launchers' dispatch -------------------------------------- */

/* The hash of an HMAC row, as the keyed kernels' template arguments. */
template <class H_, bool IS384_>
struct HashSel {
	typedef H_ H;
	static constexpr bool IS384 = IS384_;
};

/* f(HashSel<H, IS384>{}) for SHA row halg (1..3) of an HMAC row.  (The
 * fixed-layout HMAC takes Sha512HF: net2_launch_hmac's own case.) */
template <class F>
static void with_hash(int halg, F &&f)
{
	if (halg == NET2_ALG_SHA256)
		f(HashSel<Sha256H, false>{});
	else if (halg == NET2_ALG_SHA384)
		f(HashSel<Sha512H, true>{});
	else
		f(HashSel<Sha512H, false>{});
}

/* f(std::integral_constant<int, MODE>{}) for burst mode HMAC_BURST_RX / _TX:
 * MODE is the kernel family's RX or TX. */
template <int RX, int TX, class F>
static void with_burst_mode(int mode, F &&f)
{
	if (mode == HMAC_BURST_RX)
		f(std::integral_constant<int, RX>{});
	else
		f(std::integral_constant<int, TX>{});
}

/* What the burst launchers check alike: an HMAC row and a burst mode, the
 * offsets, counts the kernels' 32-bit indices hold, an IV a lane can hold
 * and -- for the launchers over a key table (kt) -- the table. */
static bool burst_launch_ok(int halg, int mode, const uint64_t *offsets,
    uint64_t n, uint32_t ivlen, const KeyTabArgs *kt)
{
	return (mode == HMAC_BURST_RX || mode == HMAC_BURST_TX) &&
	    halg >= NET2_ALG_SHA256 && halg <= NET2_ALG_SHA512 &&
	    offsets != nullptr && n <= 0xffffffffu && ivlen <= 64 &&
	    (kt == nullptr || (kt->conn != nullptr && kt->tab != nullptr &&
	    kt->slots != 0));
}

/* The variable layout under one key.  Every mode takes H's pair loop.  (Until
 * round 5 the SHA-256 VERIFY and BURST_RX kernels dropped it: 1.5 % faster
 * in round 1, when the key pass held their VGPRs at 110.  With the midstates
 * from the host they measured +4.3 to +5.3 % (verify) and +2.9 to +3.3 %
 * (burst RX) with it, profiles/round5/ab_pairall_box*.txt.) */
template <class H, bool IS384>
static void launch_hmac_var_mode(int mode, unsigned grid, hipStream_t s,
    const uint8_t *base, const uint64_t *offsets, const uint32_t *lens,
    const uint32_t *ws, uint32_t launch, uint64_t n, uint8_t *out,
    const HMid &hm, const BurstArgs &rx)
{
	const PadKW<typename H::word> pad = {};
	if (mode == HMAC_SIGN)
		hmac_kernel<H, false, HMAC_SIGN, IS384><<<grid, 256, 0, s>>>(base,
		    offsets, lens, ws, launch, 0, 0, n, out, hm, pad, rx);
	else if (mode == HMAC_VERIFY)
		hmac_kernel<H, false, HMAC_VERIFY, IS384>
		    <<<grid, 256, 0, s>>>(base, offsets, lens, ws, launch, 0, 0, n,
		    out, hm, pad, rx);
	else if (mode == HMAC_BURST_RX)
		hmac_kernel<H, false, HMAC_BURST_RX, IS384>
		    <<<grid, 256, 0, s>>>(base, offsets, lens, ws, launch, 0, 0, n,
		    out, hm, pad, rx);
	else if (mode == HMAC_BURST_TX)
		hmac_kernel<H, false, HMAC_BURST_TX, IS384><<<grid, 256, 0, s>>>(
		    base, offsets, lens, ws, launch, 0, 0, n, out, hm, pad, rx);
	else
		hmac_kernel<H, false, HMAC_DIGESTS, IS384><<<grid, 256, 0, s>>>(
		    base, offsets, lens, ws, launch, 0, 0, n, out, hm, pad, rx);
}

/* The fixed layout (offsets == NULL): digests only. */
template <class H, bool IS384>
static void launch_hmac_fixed(unsigned grid, hipStream_t s, const uint8_t *base,
    uint64_t stride, uint32_t fixed_len, uint64_t n, uint8_t *out,
    const HMid &hm, const BurstArgs &rx)
{
	constexpr uint32_t blk = sizeof(typename H::word) * 16;
	PadKW<typename H::word> pad = {};
	if (fixed_len % blk == 0) {
		const uint64_t ibits = ((uint64_t)fixed_len + blk) << 3;
		if constexpr (sizeof(typename H::word) == 4)
			pad_kw256(ibits, pad);
		else
			pad_kw512(ibits, pad);
		hmac_kernel<H, true, HMAC_DIGESTS, IS384><<<grid, 256, 0, s>>>(
		    base, nullptr, nullptr, nullptr, 0, stride, fixed_len, n, out,
		    hm, pad, rx);
	} else {
		hmac_kernel<H, false, HMAC_DIGESTS, IS384><<<grid, 256, 0, s>>>(
		    base, nullptr, nullptr, nullptr, 0, stride, fixed_len, n, out,
		    hm, pad, rx);
	}
}

hipError_t net2_launch_hmac(int alg, const uint8_t *key, const uint8_t *altkey,
    size_t keylen, const uint8_t *base, const uint64_t *offsets,
    const uint32_t *lens, uint64_t stride, uint32_t fixed_len, uint64_t n,
    uint8_t *out, uint32_t *ws, hipStream_t s, int mode,
    const BurstArgs *burst_args)
{
	if (mode != HMAC_DIGESTS && offsets == nullptr)
		return hipErrorInvalidValue;	/* datagram modes: var layout */
	if ((mode == HMAC_BURST_RX || mode == HMAC_BURST_TX) !=
	    (burst_args != nullptr))
		return hipErrorInvalidValue;
	if (burst_args != nullptr && burst_args->rec != nullptr &&
	    mode != HMAC_BURST_TX)
		return hipErrorInvalidValue;
	const BurstArgs rx = burst_args ? *burst_args : BurstArgs{};
	/* the alternate key's bytes and the kernel's rx.alt go together */
	if ((altkey != nullptr) != (mode == HMAC_BURST_RX && rx.alt != 0))
		return hipErrorInvalidValue;
	if (n == 0)
		return hipSuccess;
	const int halg = alg - 3;	/* HMAC row -> SHA row */
	HMid hm;
	if (!hmac_key_mids(halg, key, altkey, keylen, &hm))
		return hipErrorInvalidValue;	/* registry keys are <= a block */
	hipError_t e = hipSuccess;
	uint32_t launch = 0;
	if (offsets != nullptr && ws != nullptr)
		e = net2_bin_order(halg, lens, n, ws, s, &launch);
	else
		ws = nullptr;
	if (e == hipSuccess) {
		const unsigned grid = grid_for(n);
		/* Sha256H serves both layouts; the fixed layout of the SHA-512
		 * family has a hash shape of its own (Sha512HF).  (The order in
		 * which the instances are first named here is their order in the
		 * device code, and so part of the build id.) */
		if (offsets != nullptr || halg == NET2_ALG_SHA256)
			with_hash(halg, [&](auto h) {
				typedef decltype(h) S;
				if (offsets != nullptr)
					launch_hmac_var_mode<typename S::H, S::IS384>(mode,
					    grid, s, base, offsets, lens, ws, launch, n,
					    out, hm, rx);
				else if constexpr (std::is_same<typename S::H,
				    Sha256H>::value)
					launch_hmac_fixed<Sha256H, false>(grid, s, base,
					    stride, fixed_len, n, out, hm, rx);
			});
		else if (halg == NET2_ALG_SHA384)
			launch_hmac_fixed<Sha512HF, true>(grid, s, base, stride,
			    fixed_len, n, out, hm, rx);
		else
			launch_hmac_fixed<Sha512HF, false>(grid, s, base, stride,
			    fixed_len, n, out, hm, rx);
		e = hipGetLastError();
	}
	key_wipe(&hm, sizeof(hm));
	return e;
}

hipError_t net2_launch_keytab_set(int alg, Net2KeyEnt *ent, uint32_t side,
    const uint8_t *key, const uint8_t *altkey, size_t keylen, uint32_t bits,
    uint32_t cutoff, uint32_t rx_start, hipStream_t s)
{
	const int halg = alg - 3;	/* HMAC row -> SHA row */
	if (halg < NET2_ALG_SHA256 || halg > NET2_ALG_SHA512 || ent == nullptr ||
	    (side != 0 && key == nullptr))
		return hipErrorInvalidValue;
	HMid hm = {};
	if (side != 0 && !hmac_key_mids(halg, key,
	    side == NET2_KT_RX ? altkey : nullptr, keylen, &hm))
		return hipErrorInvalidValue;
	keytab_set_kernel<<<1, 64, 0, s>>>(ent, side, bits, cutoff, rx_start, hm);
	key_wipe(&hm, sizeof(hm));
	return hipGetLastError();
}

hipError_t net2_launch_hmac_mc(int alg, const KeyTabArgs &kt,
    const uint8_t *base, const uint64_t *offsets, const uint32_t *lens,
    uint64_t n, uint8_t *out, uint32_t *ws, hipStream_t s, int mode,
    const BurstArgs &args)
{
	const int halg = alg - 3;	/* HMAC row -> SHA row */
	if (!burst_launch_ok(halg, mode, offsets, n, 0, &kt) || args.rec != nullptr)
		return hipErrorInvalidValue;
	if (n == 0)
		return hipSuccess;
	uint32_t launch = 0;
	if (ws != nullptr) {
		hipError_t e = net2_bin_order(halg, lens, n, ws, s, &launch);
		if (e != hipSuccess)
			return e;
	}
	const unsigned grid = grid_for(n);
	with_hash(halg, [&](auto h) {
		typedef decltype(h) S;
		const PadKW<typename S::H::word> pad = {};
		with_burst_mode<HMAC_BURST_RX_MC, HMAC_BURST_TX_MC>(mode, [&](auto m) {
			hmac_mc_kernel<typename S::H, decltype(m)::value, S::IS384>
			    <<<grid, 256, 0, s>>>(base, offsets, lens, ws, launch, n,
			    out, kt.conn, kt.tab, kt.slots, pad, args);
		});
	});
	return hipGetLastError();
}

/* SIMDs of the current device (0: unknown), cached per ordinal. */
static uint64_t device_simds()
{
	static std::atomic<int> cus[64];
	int dev = 0;
	if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) {
		(void)hipGetLastError();
		return 0;
	}
	int c = cus[dev].load(std::memory_order_relaxed);
	if (c == 0) {
		if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount,
		    dev) != hipSuccess || c <= 0) {
			(void)hipGetLastError();
			return 0;
		}
		cus[dev].store(c, std::memory_order_relaxed);
	}
	return (uint64_t)c * 4;
}

/* Datagrams per workgroup of the wave forms (burst_wave_kernel and
 * burst_wave_mc_kernel) for a burst of n: about one workgroup per SIMD, 1 to
 * BW_GMAX. */
static uint32_t burst_wave_group(uint64_t n)
{
	const uint64_t simds = std::max<uint64_t>(device_simds(), 1);
	return (uint32_t)std::min<uint64_t>(BW_GMAX,
	    std::max<uint64_t>(1, (n + simds - 1) / simds));
}

uint64_t net2_burst_wave_default(void)
{
	/* BW_GMAX datagrams per SIMD: beyond that a pass of the wave form
	 * expands too few blocks per datagram to beat the lane form */
	return device_simds() * BW_GMAX;
}

hipError_t net2_launch_burst_wave(int alg, const uint8_t *key,
    const uint8_t *altkey, size_t keylen, const uint8_t *base,
    const uint64_t *offsets, const uint32_t *lens, uint64_t n,
    const BurstArgs *args, uint8_t *result, uint8_t *iv, uint32_t ivlen,
    uint8_t *out, int mode, hipStream_t s)
{
	const int halg = alg - 3;	/* HMAC row -> SHA row */
	if (!burst_launch_ok(halg, mode, offsets, n, ivlen, nullptr) ||
	    args == nullptr)
		return hipErrorInvalidValue;
	if (mode == HMAC_BURST_RX && args->rec != nullptr)
		return hipErrorInvalidValue;
	/* the alternate key's bytes and the kernel's args->alt go together */
	if ((altkey != nullptr) != (mode == HMAC_BURST_RX && args->alt != 0))
		return hipErrorInvalidValue;
	if (n == 0)
		return hipSuccess;
	HMid hm;
	if (!hmac_key_mids(halg, key, altkey, keylen, &hm))
		return hipErrorInvalidValue;
	const uint32_t G = burst_wave_group(n);
	const unsigned grid = (unsigned)((n + G - 1) / G);
	with_hash(halg, [&](auto h) {
		typedef decltype(h) S;
		with_burst_mode<HMAC_BURST_RX, HMAC_BURST_TX>(mode, [&](auto m) {
			burst_wave_kernel<typename S::H, decltype(m)::value, S::IS384>
			    <<<grid, 128, 0, s>>>(base, offsets, lens, n, G, hm,
			    *args, result, iv, ivlen, out);
		});
	});
	key_wipe(&hm, sizeof(hm));
	return hipGetLastError();
}

hipError_t net2_launch_burst_wave_mc(int alg, const KeyTabArgs &kt,
    const uint8_t *base, const uint64_t *offsets, const uint32_t *lens,
    uint64_t n, const BurstArgs &args, uint8_t *result, uint8_t *iv,
    uint32_t ivlen, uint8_t *out, int mode, hipStream_t s)
{
	const int halg = alg - 3;	/* HMAC row -> SHA row */
	if (!burst_launch_ok(halg, mode, offsets, n, ivlen, &kt) ||
	    args.rec != nullptr || result == nullptr)
		return hipErrorInvalidValue;
	/* RX: the decoded headers to both arrays or to neither; TX: both are
	 * the inputs, and the sealed datagrams need somewhere to go */
	if ((args.seq == nullptr) != (args.flags == nullptr) ||
	    (mode == HMAC_BURST_TX && (args.seq == nullptr || out == nullptr)))
		return hipErrorInvalidValue;
	if (n == 0)
		return hipSuccess;
	const uint32_t G = burst_wave_group(n);
	const unsigned grid = (unsigned)((n + G - 1) / G);
	with_hash(halg, [&](auto h) {
		typedef decltype(h) S;
		with_burst_mode<HMAC_BURST_RX_MC, HMAC_BURST_TX_MC>(mode, [&](auto m) {
			burst_wave_mc_kernel<typename S::H, decltype(m)::value, S::IS384>
			    <<<grid, 128, 0, s>>>(base, offsets, lens, n, G, kt.conn,
			    kt.tab, kt.slots, args.seq, args.flags, result, iv, ivlen,
			    out);
		});
	});
	return hipGetLastError();
}

hipError_t net2_launch_jobs(const uint8_t *stage, const Net2Job *jobs,
    uint32_t n256, uint32_t n512, uint8_t *out, uint32_t *done, int wave,
    hipStream_t s, uint32_t chunk)
{
	if (chunk == 0 || chunk % 128 != 0)
		return hipErrorInvalidValue;
	if (wave) {
		/* one 64-lane workgroup (one wave) per job */
		if (n256 > 0)
			job_wave_kernel<Sha256><<<n256, 64, 0, s>>>(stage, jobs,
			    out, done);
		if (n512 > 0)
			job_wave_kernel<Sha512><<<n512, 64, 0, s>>>(stage,
			    jobs + n256, out + 64 * (size_t)n256, done);
		return hipGetLastError();
	}
	/* 64-lane workgroups: a few jobs spread over as many CUs as waves */
	if (n256 > 0)
		job_kernel<Sha256><<<(n256 + 63) / 64, 64, 0, s>>>(stage, jobs,
		    n256, out, done, chunk);
	if (n512 > 0)
		job_kernel<Sha512J><<<(n512 + 63) / 64, 64, 0, s>>>(stage,
		    jobs + n256, n512, out + 64 * (size_t)n256, done, chunk);
	return hipGetLastError();
}

hipError_t net2_launch_burst_prep(uint8_t *base, const uint64_t *offsets,
    const uint32_t *lens, uint64_t n, int encode, int hash_set, int enc_set,
    uint32_t hashlen, const uint32_t *seq_in, const uint32_t *flags_in,
    uint32_t *seq_out, uint32_t *flags_out, uint64_t *sub_off,
    uint32_t *sub_len, uint8_t *status, hipStream_t s)
{
	burst_prep_kernel<<<grid_for(n), 256, 0, s>>>(base, offsets, lens, n,
	    encode, hash_set, enc_set, hashlen, seq_in, flags_in, seq_out,
	    flags_out, sub_off, sub_len, status);
	return hipGetLastError();
}

hipError_t net2_launch_burst_final(uint64_t n, const uint8_t *status,
    const uint8_t *verdict, const uint32_t *seq, const uint32_t *flags,
    uint32_t ivlen, uint8_t *iv, uint8_t *result, hipStream_t s,
    uint32_t *seq_out, uint32_t *flags_out)
{
	if (ivlen > 64 || (seq_out == nullptr) != (flags_out == nullptr))
		return hipErrorInvalidValue;
	if (n == 0)
		return hipSuccess;
	burst_final_kernel<<<grid_for(n), 256, 0, s>>>(n, status, verdict, seq,
	    flags, ivlen, iv, result, seq_out, flags_out);
	return hipGetLastError();
}

hipError_t net2_launch_burst_final_mc(uint64_t n, const uint8_t *status,
    const uint8_t *verdict, const uint32_t *seq, const uint32_t *flags,
    uint32_t ivlen, uint8_t *iv, uint8_t *result, hipStream_t s)
{
	if (ivlen > 64)
		return hipErrorInvalidValue;
	if (n == 0)
		return hipSuccess;
	burst_final_mc_kernel<<<grid_for(n), 256, 0, s>>>(n, status, verdict, seq,
	    flags, ivlen, iv, result);
	return hipGetLastError();
}

hipError_t net2_launch_ph_iv(const uint32_t *seq, const uint32_t *flags,
    uint64_t n, uint32_t ivlen, uint8_t *out, hipStream_t s)
{
	if (n == 0 || ivlen == 0)
		return hipSuccess;
	if (ivlen > 64)
		return hipErrorInvalidValue;
	ph_iv_kernel<<<grid_for(n), 256, 0, s>>>(seq, flags, n, ivlen, out);
	return hipGetLastError();
}
