/*
 * net2_burst_host.cpp -- packet bursts from host memory: sharded over the
 * devices, chunked and double-buffered per device as net2_batch.cpp does for
 * digests, over the burst steps of net2_dgram.cpp.
 */
#include "net2_host.h"

void BurstSlot::release()
{
	drop_host(h_in);
	drop_host(h_out);
	drop_host(h_meta);
	drop_dev(d_in);
	drop_dev(d_ws);
	drop_dev(d_meta);
	drop_dev(d_aux);
	cap_in = cap_n = cap_aux = 0;
}

int BurstSlot::reserve(size_t in, size_t n)
{
	bool fits;
	int rc = open(&in, &n, &fits);
	if (rc != 0 || fits)
		return rc;
	release();
	HIP_TRY(hipHostMalloc((void **)&h_in, in, hipHostMallocDefault));
	HIP_TRY(hipHostMalloc((void **)&h_out, out_bytes(n),
	    hipHostMallocDefault));
	HIP_TRY(hipHostMalloc((void **)&h_meta, mc_meta_bytes(n),
	    hipHostMallocDefault));
	HIP_TRY(hipMalloc((void **)&d_in, in));
	HIP_TRY(hipMalloc((void **)&d_meta, mc_meta_bytes(n)));
	HIP_TRY(hipMalloc((void **)&d_ws, burst_layout(n, nullptr, nullptr)));
	return grown(d_ws, in, n);
}

int BurstSlot::reserve_aux(size_t ivlen)
{
	const size_t need = Aux::bytes(cap_n, ivlen);
	if (need <= cap_aux)
		return 0;
	drop_dev(d_aux);
	cap_aux = 0;
	HIP_TRY(hipMalloc((void **)&d_aux, need));
	cap_aux = need;
	return 0;
}

namespace {

/* The pinned state of each caller buffer of a host burst (looked up once). */
struct BurstPins {
	bool result = false, iv = false, seq = false, flags = false;
	bool base = false;	/* the datagram buffer's start is page-locked */
};

/* What a host burst is asked to do; pointers are the caller's. */
struct HostBurst {
	bool tx;
	/* RX */
	const struct net2_burst_rx_keys *keys;
	uint32_t ivlen;
	void *iv;
	uint32_t *seq_out, *flags_out;
	/* TX */
	int hash_alg;
	const void *hash_key;
	size_t hash_keylen;
	int enc_alg;
	const uint32_t *seq_in, *flags_in;
	/* both */
	uint8_t *base;
	const uint64_t *offsets;
	const uint32_t *lens;
	uint8_t *result;
};

/* Chunk [lo, hi) of a host burst into slot s. */
int enqueue_burst_steps(WorkPool &pool, BurstSlot &s, const HostBurst &hb,
    const BurstPins &pins, uint64_t lo, uint64_t hi)
{
	const uint64_t n = hi - lo;
	int rc;
	const double tp0 = dbg_now();
	uint64_t rs = 0, re = 0;
	const bool direct = pins.base && dense_pinned(pool, hb.base,
	    hb.offsets + lo, hb.lens + lo, n, &rs, &re);
	PackPlan plan;
	if (!direct)
		/* RX packs with a thread per ~512 datagrams: 10-12 % faster
		 * decode calls from 4,096 datagrams up than per ~4 K, 1-4 %
		 * faster again than per ~1 K from 1,024 to 4,096; TX measured
		 * 15-18 % slower per ~1 K and keeps ~4 K
		 * (profiles/round6/pack_ab/) */
		plan = pack_sizes(pool, hb.lens + lo, n, hb.tx ? 12 : 9);
	const size_t bytes = direct ? re - rs : plan.start[plan.nt];
	if ((rc = s.reserve(bytes, n)) != 0)
		return rc;
	/*
	 * A small keyed burst (the one-launch form): its kernel reads the
	 * datagrams and their metadata through their host mapping -- the
	 * caller's page-locked buffer or the slot's staging -- instead of
	 * waiting for two copies: 5-13 % faster from 64 to 16,384 datagrams,
	 * RX and TX, pinned and pageable (profiles/round6/zc_ab/, three
	 * alternations in flipped order).
	 */
	const bool keyed = hb.tx ? hb.hash_alg != NET2_HASH_NIL :
	    hb.keys->hash_alg != NET2_HASH_NIL;
	/* read once per chunk: the burst steps launch the form decided here, so
	 * no concurrent net2_sha2_burst_limits sends mapped pointers to lanes */
	const bool wave = keyed && n <= net2_burst_wave_max();
	uint8_t *z_in = nullptr, *z_meta = nullptr;
	if (wave && n <= NET2_BURST_ZC_MAX &&
	    (z_in = mapped(direct ? hb.base + rs : s.h_in)) != nullptr &&
	    (z_meta = mapped(s.h_meta)) == nullptr)
		z_in = nullptr;		/* both, or the copies */
	uint8_t *const d_in = z_in != nullptr ? z_in : s.d_in;
	const BurstSlot::Meta hm(s.h_meta, n),
	    dm(z_meta != nullptr ? z_meta : s.d_meta, n);
	if (direct) {
		/* the chunk's datagrams lie densely in one page-locked
		 * allocation: copied as they lie, no host pack */
		rebase_meta(pool, hb.offsets + lo, hb.lens + lo, n, rs, hm.off,
		    hm.len);
	} else {
		pack_fill(pool, plan, s.h_in, hm.off, hm.len, hb.base,
		    hb.offsets + lo, hb.lens + lo, n);
	}
	if (dbg_timing())
		fprintf(stderr, "net2 burst: %s %zu B: %.3f ms (%zu threads)\n",
		    direct ? "direct" : "pack", bytes, dbg_now() - tp0, plan.nt);
	if (bytes != 0 && z_in == nullptr)
		HIP_TRY(hipMemcpyAsync(s.d_in, direct ? hb.base + rs : s.h_in, bytes,
		    hipMemcpyHostToDevice, s.stream));
	if (hb.tx) {
		memcpy(hm.hdr, hb.seq_in + lo, (size_t)n * 4);
		memcpy(hm.hdr + n, hb.flags_in + lo, (size_t)n * 4);
	}
	/* offsets, lengths (and TX headers): one copy */
	if (z_meta == nullptr)
		HIP_TRY(hipMemcpyAsync(s.d_meta, s.h_meta,
		    BurstSlot::meta_bytes(n, hb.tx), hipMemcpyHostToDevice,
		    s.stream));
	FI_POINT(FI_H2D);

	/* staged results: [code n][IV n x ivlen | records][seq n][flags n] */
	uint8_t *st_res = s.h_out;
	uint8_t *st_b = st_res + a16(n);
	bool c_res, c_iv = false, c_seq = false, c_fl = false;
	uint8_t *k_res = out_ptr(hb.result + lo, pins.result, st_res, &c_res);
	if (k_res == nullptr)
		return EIO;
	std::vector<std::function<void()>> copies;
	bool sealed = false;	/* TX sealed in place by the kernel */
	if (!hb.tx) {
		const uint32_t ivlen = hb.keys->enc_alg != 0 ? hb.ivlen : 0;
		uint8_t *st_iv = st_b;
		uint8_t *st_sq = st_iv + a16((size_t)n * ivlen);
		uint8_t *st_fl = st_sq + a16((size_t)n * 4);
		uint8_t *k_iv = nullptr, *k_sq = nullptr, *k_fl = nullptr;
		if (hb.iv != nullptr && ivlen > 0 &&
		    (k_iv = out_ptr((uint8_t *)hb.iv + lo * ivlen, pins.iv, st_iv,
		    &c_iv)) == nullptr)
			return EIO;
		if (hb.seq_out != nullptr &&
		    ((k_sq = out_ptr(hb.seq_out + lo, pins.seq, st_sq, &c_seq)) ==
		    nullptr || (k_fl = out_ptr(hb.flags_out + lo, pins.flags,
		    st_fl, &c_fl)) == nullptr))
			return EIO;
		if ((rc = decode_burst(hb.keys, hb.ivlen, d_in, dm.off, dm.len,
		    n, k_res, k_iv, (uint32_t *)k_sq, (uint32_t *)k_fl, s.d_ws,
		    s.stream, true, wave)) != 0)
			return rc;
		if (c_iv)
			copies.push_back([=]() { memcpy((uint8_t *)hb.iv +
			    lo * ivlen, st_iv, (size_t)n * ivlen); });
		if (c_seq)
			copies.push_back([=]() { memcpy(hb.seq_out + lo, st_sq,
			    (size_t)n * 4); });
		if (c_fl)
			copies.push_back([=]() { memcpy(hb.flags_out + lo, st_fl,
			    (size_t)n * 4); });
	} else {
		/*
		 * Datagrams copied as they lie from one page-locked allocation:
		 * the kernel seals headers and hash fields straight into the
		 * caller's buffer through its mapping (no records, no host
		 * scatter).  Otherwise it fills one record per datagram in the
		 * slot's mapped staging, scattered by the host when the chunk is
		 * done.
		 */
		uint8_t *const seal = keyed && direct ? mapped(hb.base + rs) : nullptr;
		uint8_t *const recd = keyed && seal == nullptr ? mapped(st_b) : nullptr;
		if (keyed && seal == nullptr && recd == nullptr)
			return EIO;
		/*
		 * Datagrams copied as they lie (page-locked input) are hashed in
		 * arrival order and sealed in place by the kernel: TX from
		 * pinned memory 2-7 % faster from 1,024 to 16,384 datagrams
		 * than records scattered by the host, the same at 1 M
		 * (profiles/round6/seal_*.jsonl).  Before the kernel sealed
		 * them, arrival order already won over the binned order by
		 * letting the host scatter walk the buffer front to back
		 * (txbin*_*.jsonl); the unbinned kernel stays hidden under the
		 * next chunk's copy.  Packed (pageable) input keeps the binning
		 * and the records: there the pack of the next chunk shares the
		 * host threads with the scatter, and with no binning at all it
		 * measured 1.5 % slower (binoff_*.jsonl).
		 */
		if ((rc = encode_burst(hb.hash_alg, hb.hash_key, hb.hash_keylen,
		    hb.enc_alg, dm.hdr, dm.hdr + n, d_in, dm.off, dm.len, n,
		    k_res, s.d_ws, s.stream, wave, recd, !direct, seal)) != 0)
			return rc;
		sealed = seal != nullptr;
	}
	FI_POINT(FI_RECORD);
	HIP_TRY(hipEventRecord(s.done, s.stream));
	s.busy = true;
	const bool tx = hb.tx;
	/* dl != 0: records to scatter (keyed TX, not sealed by the kernel) */
	const int dl = tx && hb.hash_alg != NET2_HASH_NIL && !sealed ?
	    digest_len(hb.hash_alg) : 0;
	WorkPool *pp = &pool;
	s.finish = [=]() {
		if (c_res && !(tx && dl != 0))
			memcpy(hb.result + lo, st_res, (size_t)n);
		for (const std::function<void()> &c : copies)
			c();
		if (!tx || sealed)
			return 0;
		/* TX: the code of every datagram, and the sealed header (and
		 * hash field) of every OK one into the caller's slot
		 * (packet.n2t:384-392, :417-427) */
		const size_t nt = std::min<size_t>(kPackThreads,
		    std::max<size_t>(1, n >> 12));
		pp->run(nt, [=](size_t t) {
			for (uint64_t j = n * t / nt; j < n * (t + 1) / nt; j++) {
				if (dl != 0) {
					/* record of binned position j */
					const uint8_t *r = st_b + j * (dl + 16);
					uint32_t w[4];
					memcpy(w, r + dl, 16);
					const uint64_t i = lo + w[2];
					hb.result[i] = (uint8_t)w[3];
					if (w[3] != NET2_PENCODE_OK)
						continue;
					uint8_t *dg = hb.base + hb.offsets[i];
					memcpy(dg, w, 8);
					memcpy(dg + 8, r, dl);
					continue;
				}
				if (hb.result[lo + j] != NET2_PENCODE_OK)
					continue;
				uint8_t *dg = hb.base + hb.offsets[lo + j];
				const uint32_t sq = hb.seq_in[lo + j];
				const uint32_t fl = hb.flags_in[lo + j];
				for (int b = 0; b < 4; b++) {
					dg[b] = (uint8_t)(sq >> (24 - 8 * b));
					dg[4 + b] = (uint8_t)(fl >> (24 - 8 * b));
				}
			}
		});
		return 0;
	};
	return 0;
}

/* One device's share [lo, hi) of a host burst, chunked and double-buffered. */
int run_burst_slice(size_t didx, int ordinal, const HostBurst &hb,
    uint64_t lo, uint64_t hi)
{
	const NumaPlace &np = numa_place(ordinal);
	NumaBind bind(np);
	DeviceCtx *c = ctx_for(didx);
	BurstSlot *const slot = c->burst_slot;
	std::lock_guard<std::mutex> g(c->burst_mu);
	HIP_TRY(hipSetDevice(ordinal));
	/* outputs are stored through their mapping only when the slice's
	 * whole range of each is in one page-locked allocation */
	const uint64_t m = hi - lo;
	const double tq0 = dbg_now();
	BurstPins pins;
	pins.base = is_pinned(hb.base);
	pins.result = pinned_span(hb.result + lo, m);
	if (!hb.tx) {
		const uint32_t ivl = hb.keys->enc_alg != 0 ? hb.ivlen : 0;
		pins.iv = hb.iv != nullptr && ivl > 0 && pinned_span((uint8_t *)hb.iv +
		    lo * ivl, m * ivl);
		pins.seq = hb.seq_out != nullptr && pinned_span(hb.seq_out + lo,
		    m * 4);
		pins.flags = hb.flags_out != nullptr && pinned_span(hb.flags_out +
		    lo, m * 4);
	}
	if (dbg_timing())
		fprintf(stderr, "net2 burst: page-lock lookups %.3f ms\n",
		    dbg_now() - tq0);
	const uint64_t per_chunk = var_chunk_packets(*c->pool, hb.lens + lo,
	    hi - lo);
	/*
	 * Chunk k is enqueued into its slot first, then chunk k - 1 (the other
	 * slot) is waited for and its results handed over -- the TX scatter
	 * of sealed headers runs while chunk k copies and hashes, and by the
	 * next iteration that slot is free again.  (Draining a slot right
	 * before reusing it put the scatter between two copies: TX 17.6 ms per
	 * 1 M datagrams against RX's 15.2 ms.)
	 */
	int rc = 0, cur = 0;
	for (uint64_t at = lo; at < hi && rc == 0;) {
		const uint64_t end = std::min<uint64_t>(hi, at + per_chunk);
		const double t0 = dbg_now();
		rc = enqueue_burst_steps(*c->pool, slot[cur], hb, pins, at, end);
		/* a chunk that failed part-way is waited for before the error
		 * goes back, and its slot stays free */
		if (rc != 0)
			quiesce(slot[cur].stream);
		const double t1 = dbg_now();
		if (rc == 0)
			rc = slot[cur ^ 1].drain();
		if (dbg_timing())
			fprintf(stderr, "net2 burst: enqueue %.3f ms, drain+finish "
			    "%.3f ms (%llu datagrams)\n", t1 - t0, dbg_now() - t1,
			    (unsigned long long)(end - at));
		at = end;
		cur ^= 1;
	}
	/* both slots drained whatever happened: no kernel may still write
	 * into the caller's memory when the call returns */
	const int rc2 = slot[0].drain();
	const int rc3 = slot[1].drain();
	return rc ? rc : rc2 ? rc2 : rc3;
}

}	/* namespace */

NET2_EXPORT int net2_packet_decode_burst_host(
    const struct net2_burst_rx_keys *k, uint32_t ivlen, const void *base,
    const uint64_t *offsets, const uint32_t *lens, uint64_t n,
    uint8_t *result, void *iv, uint32_t *seq, uint32_t *flags,
    int max_devices)
{
	if (k == nullptr ||
	    !hmac_key_ok(k->hash_alg, k->hash_key, k->hash_keylen, true))
		return EINVAL;
	int rc = check_burst_arrays(ivlen, base, offsets, lens, n, result);
	if (rc != 0 || n == 0)
		return rc;
	if (k->hash_alg != NET2_HASH_NIL && k->alt_hash_key != nullptr &&
	    k->alt_hash_keylen != k->hash_keylen)
		return EINVAL;
	if ((seq == nullptr) != (flags == nullptr))
		return EINVAL;
	HostBurst hb = {};
	hb.tx = false;
	hb.keys = k;
	hb.ivlen = ivlen;
	hb.iv = iv;
	hb.seq_out = seq;
	hb.flags_out = flags;
	hb.base = (uint8_t *)const_cast<void *>(base);
	hb.offsets = offsets;
	hb.lens = lens;
	hb.result = result;
	return shard_batch(n, lens, 0, max_devices, [&](size_t didx,
	    int ordinal, uint64_t lo, uint64_t hi) {
		return run_burst_slice(didx, ordinal, hb, lo, hi);
	});
}

NET2_EXPORT int net2_packet_encode_burst_host(int hash_alg,
    const void *hash_key, size_t hash_keylen, int enc_alg,
    const uint32_t *seq, const uint32_t *flags, void *base,
    const uint64_t *offsets, const uint32_t *lens, uint64_t n,
    uint8_t *result, int max_devices)
{
	if (!hmac_key_ok(hash_alg, hash_key, hash_keylen, true))
		return EINVAL;
	int rc = check_burst_arrays(0, base, offsets, lens, n, result);
	if (rc != 0 || n == 0)
		return rc;
	if (seq == nullptr || flags == nullptr)
		return EINVAL;
	HostBurst hb = {};
	hb.tx = true;
	hb.hash_alg = hash_alg;
	hb.hash_key = hash_key;
	hb.hash_keylen = hash_keylen;
	hb.enc_alg = enc_alg;
	hb.seq_in = seq;
	hb.flags_in = flags;
	hb.base = (uint8_t *)base;
	hb.offsets = offsets;
	hb.lens = lens;
	hb.result = result;
	return shard_batch(n, lens, 0, max_devices, [&](size_t didx,
	    int ordinal, uint64_t lo, uint64_t hi) {
		return run_burst_slice(didx, ordinal, hb, lo, hi);
	});
}
