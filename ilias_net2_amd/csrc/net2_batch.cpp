/*
 * net2_batch.cpp -- include/net2/sha2_batch.h: host-memory batches (the pack
 * helpers, the chunk pipeline of a device's slice) and the device-resident
 * digest calls with their binning workspace.
 */
#include "net2_host.h"

/*
 * The pack helpers, shared with the host bursts.  Pack n packets into pinned
 * staging with 16-byte aligned starts and write their staged offsets and
 * lengths, split over up to kPackThreads threads: pack_sizes sums each
 * thread's range of padded lengths (the chunk's byte count, and each
 * range's start), pack_fill then writes offsets and copies packets.  A
 * serial scan and gather over MTU-sized datagrams held the host path well
 * below the PCIe rate.
 */
PackPlan pack_sizes(WorkPool &pool, const uint32_t *lens, uint64_t n,
    int per_shift)
{
	PackPlan pl;
	/* one thread per 2^per_shift packets: ~4 K by default (the fill copies
	 * ~MiBs each) */
	pl.nt = std::min<size_t>(kPackThreads, std::max<size_t>(1,
	    n >> per_shift));
	size_t *st = pl.start;
	const size_t nt = pl.nt;
	pool.run(nt, [=](size_t t) {
		size_t sum = 0;
		for (uint64_t i = n * t / nt; i < n * (t + 1) / nt; i++)
			sum += ((size_t)lens[i] + 15) & ~(size_t)15;
		st[t + 1] = sum;
	});
	for (size_t t = 1; t <= nt; t++)
		st[t] += st[t - 1];
	return pl;
}

void pack_fill(WorkPool &pool, const PackPlan &pl, uint8_t *dst, uint64_t *dst_off,
    uint32_t *dst_len, const uint8_t *base, const uint64_t *offsets,
    const uint32_t *lens, uint64_t n)
{
	const size_t nt = pl.nt;
	const size_t *st = pl.start;
	pool.run(nt, [=](size_t t) {
		size_t at = st[t];
		for (uint64_t i = n * t / nt; i < n * (t + 1) / nt; i++) {
			const uint32_t l = lens[i];
			dst_off[i] = at;
			dst_len[i] = l;
			memcpy(dst + at, base + offsets[i], l);
			at += ((size_t)l + 15) & ~(size_t)15;
		}
	});
}

/*
 * The byte range [*rs, *re) (offsets from base) of packets off / ln [0, n)
 * when it can be DMA'd as it lies: within one page-locked allocation
 * (pinned_span) and dense -- at most a
 * quarter more bytes than the packets themselves, as when a receive loop
 * fills one pinned arena back to back.
 */
bool dense_pinned(WorkPool &pool, const uint8_t *base, const uint64_t *off,
    const uint32_t *ln, uint64_t n, uint64_t *rs, uint64_t *re)
{
	const size_t nt = std::min<size_t>(kPackThreads,
	    std::max<size_t>(1, n >> 14));
	uint64_t lo_t[kPackThreads], hi_t[kPackThreads], sum_t[kPackThreads];
	pool.run(nt, [&](size_t t) {
		uint64_t a = UINT64_MAX, b = 0, m = 0;
		for (uint64_t j = n * t / nt; j < n * (t + 1) / nt; j++) {
			a = std::min<uint64_t>(a, off[j]);
			b = std::max<uint64_t>(b, off[j] + ln[j]);
			m += ln[j];
		}
		lo_t[t] = a;
		hi_t[t] = b;
		sum_t[t] = m;
	});
	uint64_t a = UINT64_MAX, b = 0, m = 0;
	for (size_t t = 0; t < nt; t++) {
		a = std::min(a, lo_t[t]);
		b = std::max(b, hi_t[t]);
		m += sum_t[t];
	}
	if (n == 0 || b <= a || b - a > m + m / 4 || !pinned_span(base + a, b - a))
		return false;
	*rs = a;
	*re = b;
	return true;
}

/* Metadata of packets copied as they lie (dense_pinned): offsets from the
 * range's start rs, lengths as they are. */
void rebase_meta(WorkPool &pool, const uint64_t *off, const uint32_t *ln,
    uint64_t n, uint64_t rs, uint64_t *dst_off, uint32_t *dst_len)
{
	const size_t nt = std::min<size_t>(kPackThreads,
	    std::max<size_t>(1, n >> 14));
	pool.run(nt, [=](size_t t) {
		for (uint64_t j = n * t / nt; j < n * (t + 1) / nt; j++) {
			dst_off[j] = off[j] - rs;
			dst_len[j] = ln[j];
		}
	});
}

/* Packets per chunk of a variable-length slice: kChunkBytes of padded payload
 * at the slice's mean packet size.  A chunk of unusually large packets just
 * grows the staging (reserve); the exact byte count comes from pack_sizes. */
uint64_t var_chunk_packets(WorkPool &pool, const uint32_t *lens, uint64_t n)
{
	const PackPlan all = pack_sizes(pool, lens, n);
	const size_t mean = std::max<size_t>(all.start[all.nt] /
	    std::max<uint64_t>(n, 1), 16);
	return std::max<size_t>(kChunkBytes / mean, 1);
}

/* ---- the host batch pipeline ------------------------------------------------ */

void BatchSlot::release()
{
	drop_host(h_in);
	drop_host(h_dig);
	drop_host(h_off);
	drop_dev(d_in);
	drop_dev(d_dig);
	drop_dev(d_off);
	drop_dev(d_ws);
	cap_in = cap_n = 0;
}

/*
 * Grow to hold `in` payload bytes and `n` packets.  host_in == false: the
 * payload is DMA'd straight from the caller's pinned memory, so no pinned
 * input staging is allocated (or kept) for it.
 */
int BatchSlot::reserve(size_t in, size_t n, bool host_in)
{
	bool fits;
	int rc = open(&in, &n, &fits);
	if (rc != 0 || (fits && (!host_in || h_in != nullptr)))
		return rc;
	release();
	if (host_in)
		HIP_TRY(hipHostMalloc((void **)&h_in, in, hipHostMallocDefault));
	HIP_TRY(hipHostMalloc((void **)&h_dig, n * 64, hipHostMallocDefault));
	HIP_TRY(hipHostMalloc((void **)&h_off, n * 12, hipHostMallocDefault));
	HIP_TRY(hipMalloc((void **)&d_in, in));
	HIP_TRY(hipMalloc((void **)&d_dig, n * 64));
	HIP_TRY(hipMalloc((void **)&d_off, n * 12));
	HIP_TRY(hipMalloc((void **)&d_ws,
	    (NET2_BIN_WS_WORDS + n) * sizeof(uint32_t)));
	return grown(d_ws, in, n);
}

namespace {

/* memcpy of a large range split over the pool's threads (staging copies). */
void par_memcpy(WorkPool &pool, uint8_t *dst, const uint8_t *src,
    size_t bytes)
{
	const size_t piece = 8u << 20;
	if (bytes == 0)		/* n empty packets at stride 0 */
		return;
	const size_t nt = std::min<size_t>(8, (bytes + piece - 1) / piece);
	pool.run(nt, [=](size_t t) {
		const size_t a = bytes * t / nt, b = bytes * (t + 1) / nt;
		memcpy(dst + a, src + a, b - a);
	});
}

/*
 * Digests of the host path: the kernel stores them straight into pinned
 * host memory (the caller's buffer when it is pinned, else the slot's
 * staging) through its device mapping, so a chunk costs one H2D copy and no
 * D2H copy.  With a D2H copy per chunk the copies of every slot shared one
 * DMA queue in submission order: chunk k's D2H, waiting for its kernel,
 * held chunk k+1's H2D back, and the path ran at 91 % of the link's copy
 * rate.  NET2_SHA2_D2H_COPY=1 restores the copy (A/B).
 */
bool d2h_copy()
{
	static const bool on = getenv("NET2_SHA2_D2H_COPY") != nullptr &&
	    atoi(getenv("NET2_SHA2_D2H_COPY")) != 0;
	return on;
}

/*
 * One chunk [lo, hi) of the caller's packets into slot s: H2D (straight from
 * the caller's buffer when it is pinned -- for the variable layout when the
 * chunk's packets also lie densely, dense_pinned -- else through the slot's
 * pinned staging, packed with 16-byte aligned packet starts), kernel
 * writing the digests to pinned host memory (the caller's buffer when that
 * is pinned).
 */
int enqueue_chunk_steps(WorkPool &pool, BatchSlot &s, int alg, const uint8_t *base,
    const uint64_t *offsets, const uint32_t *lens, uint64_t stride,
    uint32_t fixed_len, uint64_t lo, uint64_t hi, uint8_t *user_dig,
    bool src_pinned, bool dst_pinned)
{
	const uint64_t n = hi - lo;
	const int dl = digest_len(alg);
	size_t bytes;
	int rc;
	PackPlan plan;

	uint64_t rs = 0, re = 0;
	const bool var_direct = offsets != nullptr && src_pinned &&
	    dense_pinned(pool, base, offsets + lo, lens + lo, n, &rs, &re);
	if (offsets == nullptr) {
		bytes = src_pinned ? (size_t)(n - 1) * stride + fixed_len
		    : (size_t)n * ((fixed_len + 15) & ~15u);
	} else if (var_direct) {
		bytes = re - rs;
	} else {
		plan = pack_sizes(pool, lens + lo, n);
		bytes = plan.start[plan.nt];
	}
	const double tr0 = dbg_now();
	if ((rc = s.reserve(bytes, n, !((offsets == nullptr && src_pinned) ||
	    var_direct))) != 0)
		return rc;
	if (dbg_timing())
		fprintf(stderr, "net2: reserve %.3f ms\n", dbg_now() - tr0);
	/* where the kernel stores the digests (see d2h_copy) */
	uint8_t *const host_dig = dst_pinned ? user_dig : s.h_dig;
	uint8_t *const dig_map = d2h_copy() ? nullptr : mapped(host_dig);
	const bool direct = dig_map != nullptr;
	uint8_t *const kout = direct ? dig_map : s.d_dig;

	if (offsets == nullptr) {
		/* as it lies at the caller's stride, or staged at st */
		const uint8_t *src = base + lo * stride;
		const size_t st = src_pinned ? stride : (fixed_len + 15) & ~15u;
		if (!src_pinned && st == stride) {
			/* contiguous; the caller's buffer ends at the last
			 * packet's last byte, not at a stride boundary */
			par_memcpy(pool, s.h_in, src,
			    (size_t)(n - 1) * stride + fixed_len);
		} else if (!src_pinned) {
			const size_t nt = std::min<size_t>(kPackThreads,
			    std::max<size_t>(1, bytes >> 22));
			uint8_t *dst = s.h_in;
			pool.run(nt, [=](size_t t) {
				for (uint64_t i = n * t / nt; i < n * (t + 1) / nt; i++)
					memcpy(dst + i * st, src + i * stride,
					    fixed_len);
			});
		}
		if (bytes != 0)
			HIP_TRY(hipMemcpyAsync(s.d_in, src_pinned ? src : s.h_in,
			    bytes, hipMemcpyHostToDevice, s.stream));
		FI_POINT(FI_H2D);
		HIP_TRY(net2_launch_fixed(alg, s.d_in, st, fixed_len, n,
		    kout, s.stream));
		FI_POINT(FI_KERNEL);
	} else {
		const double tg0 = dbg_now();
		if (var_direct) {
			/* as they lie (the kernel picks its address mode per wave) */
			rebase_meta(pool, offsets + lo, lens + lo, n, rs, s.h_off,
			    (uint32_t *)(s.h_off + n));
		} else {
			pack_fill(pool, plan, s.h_in, s.h_off,
			    (uint32_t *)(s.h_off + n), base, offsets + lo,
			    lens + lo, n);
		}
		if (dbg_timing())
			fprintf(stderr, "net2: %s %zu B, %llu packets: %.3f ms\n",
			    var_direct ? "direct" : "pack", bytes,
			    (unsigned long long)n, dbg_now() - tg0);
		if (bytes != 0)
			HIP_TRY(hipMemcpyAsync(s.d_in, var_direct ? base + rs :
			    s.h_in, bytes, hipMemcpyHostToDevice, s.stream));
		HIP_TRY(hipMemcpyAsync(s.d_off, s.h_off, n * 12,
		    hipMemcpyHostToDevice, s.stream));
		FI_POINT(FI_H2D);
		HIP_TRY(net2_launch_var(alg, s.d_in, s.d_off,
		    (const uint32_t *)(s.d_off + n), n, kout,
		    n >= 4096 ? s.d_ws : nullptr, s.stream));
		FI_POINT(FI_KERNEL);
	}
	if (!direct)
		HIP_TRY(hipMemcpyAsync(host_dig, s.d_dig, (size_t)n * dl,
		    hipMemcpyDeviceToHost, s.stream));
	FI_POINT(FI_RECORD);
	HIP_TRY(hipEventRecord(s.done, s.stream));
	s.busy = true;
	/* digests staged for a pageable buffer go to the caller at the drain */
	if (!dst_pinned) {
		const uint8_t *const staged = s.h_dig;
		s.finish = [=]() {
			memcpy(user_dig, staged, (size_t)n * dl);
			return 0;
		};
	}
	return 0;
}

/* One device's share of a host-memory batch. */
int run_device_slice(size_t didx, int ordinal, int alg, const uint8_t *base,
    const uint64_t *offsets, const uint32_t *lens, uint64_t stride,
    uint32_t fixed_len, uint64_t lo, uint64_t hi, uint8_t *digests)
{
	/* on the device's node before anything is allocated or touched */
	const NumaPlace &np = numa_place(ordinal);
	NumaBind bind(np);
	DeviceCtx *c = ctx_for(didx);
	std::lock_guard<std::mutex> g(c->mu);
	struct Count {
		DeviceCtx *c;
		const NumaPlace &np;
		~Count()
		{
			const int cpu = sched_getcpu();
			c->slices.fetch_add(1, std::memory_order_relaxed);
			if (np.node >= 0 && cpu >= 0 && CPU_ISSET(cpu, &np.cpus))
				c->slices_on_node.fetch_add(1,
				    std::memory_order_relaxed);
		}
	} count = { c, np };
	const int dl = digest_len(alg);
	int rc = 0, cur = 0;

	HIP_TRY(hipSetDevice(ordinal));
	/* fixed layout: DMA'd as it lies when the slice's whole span is in one
	 * page-locked allocation; variable: when its chunk's packets also lie
	 * densely in one (enqueue_chunk, dense_pinned).  Digests are stored
	 * through the output's mapping only when the slice's whole output range
	 * is in one page-locked allocation (pinned_span). */
	const bool src_pinned = offsets == nullptr ?
	    pinned_span(base + lo * stride, (size_t)(hi - 1 - lo) * stride +
	    fixed_len) : is_pinned(base);
	const bool dst_pinned = pinned_span(digests + lo * dl,
	    (size_t)(hi - lo) * dl);
	uint64_t per_chunk;	/* packets: kChunkBytes of (padded) payload */
	if (offsets == nullptr) {
		/* the direct-DMA path copies whole strides (a chunk spans
		 * (n - 1) * stride + fixed_len bytes), the staged one packs
		 * packets at 16-byte granularity */
		const size_t per = std::max<size_t>(src_pinned ? stride :
		    (fixed_len + 15) & ~15u, 16);
		per_chunk = std::max<size_t>(kChunkBytes / per, 1);
	} else {
		per_chunk = var_chunk_packets(*c->pool, lens + lo, hi - lo);
	}
	for (uint64_t at = lo; at < hi && rc == 0;) {
		const double tc0 = dbg_now();
		const uint64_t end = std::min<uint64_t>(hi, at + per_chunk);
		BatchSlot &s = c->slot[cur];
		if ((rc = s.drain()) != 0)
			break;
		const double te0 = dbg_now();
		rc = enqueue_chunk_steps(*c->pool, s, alg, base, offsets, lens,
		    stride, fixed_len, at, end, digests + at * dl, src_pinned,
		    dst_pinned);
		/* a chunk that failed part-way is waited for before the error
		 * goes back, and its slot stays free */
		if (rc != 0)
			quiesce(s.stream);
		if (dbg_timing())
			fprintf(stderr, "net2: enqueue %.3f ms (+%.3f ms before it)\n",
			    dbg_now() - te0, te0 - tc0);
		at = end;
		cur ^= 1;
	}
	int rc2 = c->slot[0].drain();
	int rc3 = c->slot[1].drain();
	return rc ? rc : rc2 ? rc2 : rc3;
}

}	/* namespace */

NET2_EXPORT int net2_sha2_dev_fixed(int alg, const void *d_base,
    uint64_t stride, uint32_t len, uint64_t n, void *d_digests, void *stream)
{
	if (!unkeyed_sha2(alg))
		return EINVAL;
	if (n == 0)
		return 0;
	if (d_digests == nullptr || (d_base == nullptr && len > 0))
		return EINVAL;
	if (n > 1 && stride < len)
		return EINVAL;
	if (int rc = check_current_device())
		return rc;
	HIP_TRY(net2_launch_fixed(alg, (const uint8_t *)d_base, stride, len, n,
	    (uint8_t *)d_digests, (hipStream_t)stream));
	return 0;
}

NET2_EXPORT size_t net2_sha2_dev_var_workspace(uint64_t n)
{
	return ((size_t)NET2_BIN_WS_WORDS + (size_t)n) * sizeof(uint32_t);
}

NET2_EXPORT int net2_sha2_workspace_init(void *d_ws, size_t ws_bytes,
    void *stream)
{
	if (d_ws == nullptr || ws_bytes < net2_sha2_dev_var_workspace(0) ||
	    ((uintptr_t)d_ws & 3) != 0)
		return EINVAL;
	if (int rc = check_current_device())
		return rc;
	HIP_TRY(net2_bin_ws_init((uint32_t *)d_ws, (hipStream_t)stream));
	return 0;
}

NET2_EXPORT int net2_sha2_bin_limits(uint32_t grid_cap, int64_t timeout_us)
{
	net2_bin_set_limits(grid_cap, timeout_us);
	return 0;
}

NET2_EXPORT int net2_sha2_workspace_stats(const void *d_ws, size_t ws_bytes,
    struct net2_bin_stats *st)
{
	if (d_ws == nullptr || st == nullptr ||
	    ws_bytes < net2_sha2_dev_var_workspace(0) ||
	    ((uintptr_t)d_ws & 7) != 0)
		return EINVAL;
	if (int rc = check_current_device())
		return rc;
	uint32_t h[NET2_BIN_HDR];
	HIP_TRY(hipMemcpy(h, d_ws, sizeof(h), hipMemcpyDeviceToHost));
	const uint64_t tag = (uint64_t)h[NET2_BIN_W_TAG + 1] << 32 |
	    h[NET2_BIN_W_TAG];
	st->prepared = (uint32_t)(tag >> 32) == 0x4e324253u;	/* "N2BS" */
	st->binned = h[NET2_BIN_W_BINNED];
	st->aborts = h[NET2_BIN_W_ABORTS];
	st->mismatches = h[NET2_BIN_W_MISMATCH];
	st->unprepared = h[NET2_BIN_W_UNPREP];
	return 0;
}

NET2_EXPORT int net2_sha2_dev_var(int alg, const void *d_base,
    const uint64_t *d_offsets, const uint32_t *d_lens, uint64_t n,
    void *d_digests, void *d_ws, size_t ws_bytes, void *stream)
{
	if (!unkeyed_sha2(alg))
		return EINVAL;
	if (n == 0)
		return 0;
	if (d_offsets == nullptr || d_lens == nullptr || d_digests == nullptr)
		return EINVAL;
	if (!bin_ws_ok(d_ws, ws_bytes, n))
		return EINVAL;
	if (int rc = check_current_device())
		return rc;
	HIP_TRY(net2_launch_var(alg, (const uint8_t *)d_base, d_offsets, d_lens,
	    n, (uint8_t *)d_digests, (uint32_t *)d_ws, (hipStream_t)stream));
	return 0;
}

NET2_EXPORT int net2_sha2_batch(int alg, const void *base,
    const uint64_t *offsets, const uint32_t *lens, uint64_t stride,
    uint32_t fixed_len, uint64_t n, void *digests, int max_devices)
{
	if (!unkeyed_sha2(alg))
		return EINVAL;
	if (n == 0)
		return 0;
	if (digests == nullptr || (offsets != nullptr && lens == nullptr))
		return EINVAL;
	if (offsets == nullptr && (base == nullptr && fixed_len > 0))
		return EINVAL;
	if (offsets == nullptr && n > 1 && stride < fixed_len)
		return EINVAL;
	return shard_batch(n, offsets != nullptr ? lens : nullptr, fixed_len,
	    max_devices, [&](size_t didx, int ordinal, uint64_t lo,
	    uint64_t hi) {
		return run_device_slice(didx, ordinal, alg,
		    (const uint8_t *)base, offsets, lens, stride, fixed_len,
		    lo, hi, (uint8_t *)digests);
	});
}
