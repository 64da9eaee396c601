/*
 * net2_burst_mc_host.cpp -- packet bursts from host memory over many
 * connections, with the payload cipher: net2_burst_host.cpp's pipeline (pack
 * or copy as it lies, 64 MiB chunks double-buffered in the device's two burst
 * slots) over the multi-connection steps of net2_dgram.cpp.  One device, the
 * tables'; no kernel of its own.
 */
#include "net2_host.h"

#include <functional>
#include <vector>

namespace {

/* The pinned state of each caller buffer of a call (looked up once). */
struct McPins {
	bool base = false;	/* the datagram buffer's start is page-locked */
	bool result = false, iv = false, seq = false, flags = false;
	bool len = false;	/* RX plen, TX wire_len */
};

/* What a call is asked to do; pointers are the caller's. */
struct McBurst {
	bool tx;
	const struct net2_burst_keytab *tab;
	const struct net2_burst_ciphertab *ctab;	/* null: hash step only */
	const uint32_t *conn;
	uint32_t hashlen;	/* the table's digest length */
	uint32_t ivlen;		/* RX: the caller's; TX: 16 with the cipher */
	hipEvent_t tables;	/* recorded on the caller's table stream */
	/* RX */
	void *iv;
	uint32_t *seq_out, *flags_out;
	uint8_t *out;
	uint32_t *plen_out;
	/* TX */
	const uint32_t *seq_in, *flags_in, *plen_in;
	uint32_t *wire_len;
	/* both */
	uint8_t *base;
	const uint64_t *offsets;
	const uint32_t *lens;
	uint8_t *result;
};

/* One per-datagram output array of a chunk. */
struct SmallOut {
	uint8_t *dev = nullptr;		/* where the kernels store it */
	uint8_t *host = nullptr;	/* where the host finds it once the chunk is done */
	uint8_t *user = nullptr;	/* the caller's, when host is staging to copy from */
	size_t bytes = 0;
};

/* bytes kept free behind a chunk's datagrams in device memory: at least the
 * longest header and hash field (enqueue_mc_steps) */
constexpr size_t kTxSlack = 128;

/*
 * The largest chunk with the cipher whose kernels read (and write) the
 * datagrams through their host mapping instead of a device copy.  Measured
 * with tools/burst_sizes.py --zc-ab (profiles/burst_mc_host/zc_ab.jsonl, the
 * two alternating in one process, four rounds in flipped order, DESIGN.md
 * 9.5.1): RX 11-17 % faster from 64 to 1,024 datagrams, pinned and pageable,
 * where a variant's own rounds spread at most 2 %, and 2-13 % slower from
 * 4,096; TX 8-21 % slower at every size (the CBC chain waits for each block
 * it reads), so TX always copies.  NET2_BURST_MC_ZC_MAX, read per chunk,
 * overrides both (A/B runs and tests).
 */
constexpr uint64_t kMcZcMaxRx = 1024, kMcZcMaxTx = 0;
uint64_t mc_cipher_zc_max(bool tx)
{
	const char *e = getenv("NET2_BURST_MC_ZC_MAX");
	return e != nullptr && *e != '\0' ? strtoull(e, nullptr, 10) :
	    tx ? kMcZcMaxTx : kMcZcMaxRx;
}

inline uint32_t payload_at(uint32_t flags, uint32_t hashlen)
{
	return 8 + ((flags & NET2_PH_SIGNED) != 0 ? hashlen : 0);
}

/* Chunk [lo, hi) of a call into slot s. */
int enqueue_mc_steps(WorkPool &pool, BurstSlot &s, const McBurst &mb,
    const McPins &pins, uint64_t lo, uint64_t hi)
{
	const uint64_t n = hi - lo;
	const bool cipher = mb.ctab != nullptr;
	int rc;
	const double tp0 = dbg_now();
	uint64_t rs = 0, re = 0;
	const bool direct = pins.base && dense_pinned(pool, mb.base,
	    mb.offsets + lo, mb.lens + lo, n, &rs, &re);
	PackPlan plan;
	if (!direct)
		/* a thread per ~512 (RX) / ~4 K (TX) datagrams, as
		 * enqueue_burst_steps measured */
		plan = pack_sizes(pool, mb.lens + lo, n, mb.tx ? 12 : 9);
	const size_t bytes = direct ? re - rs : plan.start[plan.nt];
	/* (kTxSlack: see the plaintext lengths below) */
	if ((rc = s.reserve(bytes + kTxSlack, n)) != 0 ||
	    (rc = s.reserve_aux(mb.ivlen)) != 0)
		return rc;
	/* every form read once per chunk and passed down: the steps launch what
	 * is decided here whatever a concurrent *_limits call sets */
	const bool wave = n <= net2_burst_wave_max();
	const bool cform = cipher && (mb.tx ? aes_quad_form(n) : aes_wave_form(n));
	/*
	 * Hash step only, a small burst in the one-launch form: the kernel reads
	 * datagrams and metadata through their host mapping and stores its
	 * results through the caller's, as the single-connection host bursts do
	 * (enqueue_burst_steps).  Otherwise the chunk is copied to device memory,
	 * the results are left there (BurstSlot::Aux) and copied out behind the
	 * kernels.  With the cipher the results always stay in device memory,
	 * where the second step reads what the first left; a small RX chunk's
	 * datagrams are still read, and decrypted, through the mapping
	 * (mc_cipher_zc_max).
	 */
	/* RX with the cipher: the plaintexts land in the caller's buffer as the
	 * chunk lies there (in place, one page-locked allocation); else they are
	 * copied out of the staging */
	const bool home = cipher && !mb.tx && direct && mb.out == mb.base;
	uint8_t *z_in = nullptr, *z_meta = nullptr, *z_stage = nullptr;
	bool try_zin = cipher ? n <= mc_cipher_zc_max(mb.tx) :
	    wave && n <= NET2_BURST_ZC_MAX;
	/* a TX slot whose hash step would read past it (see the plaintext
	 * lengths below) is not read where it lies: the caller's allocation may
	 * end there */
	for (uint64_t j = lo; try_zin && cipher && mb.tx && direct && j < hi; j++)
		if ((mb.flags_in[j] & NET2_PH_ENCRYPTED) == 0 &&
		    (uint64_t)payload_at(mb.flags_in[j], mb.hashlen) + mb.plen_in[j] >
		    mb.lens[j])
			try_zin = false;
	if (try_zin &&
	    (z_in = mapped(direct ? mb.base + rs : s.h_in)) != nullptr &&
	    ((z_meta = mapped(s.h_meta)) == nullptr ||
	    (cipher && !mb.tx && direct && !home &&
	    (z_stage = mapped(s.h_in)) == nullptr)))
		z_in = nullptr;		/* all of them, or the copies */
	/* zin: datagrams and metadata are read (with the cipher: and written)
	 * through the mapping; zc: the results are stored through it too */
	const bool zin = z_in != nullptr, zc = zin && !cipher;
	uint8_t *const d_in = zin ? z_in : s.d_in;
	const BurstSlot::Meta hm(s.h_meta, n), dm(zin ? z_meta : s.d_meta, n);
	if (direct) {
		/* the chunk's datagrams lie densely in one page-locked
		 * allocation: copied as they lie, no host pack */
		rebase_meta(pool, mb.offsets + lo, mb.lens + lo, n, rs, hm.off,
		    hm.len);
	} else {
		pack_fill(pool, plan, s.h_in, hm.off, hm.len, mb.base,
		    mb.offsets + lo, mb.lens + lo, n);
	}
	memcpy(hm.conn, mb.conn + lo, (size_t)n * 4);
	if (mb.tx) {
		memcpy(hm.hdr, mb.seq_in + lo, (size_t)n * 4);
		memcpy(hm.hdr + n, mb.flags_in + lo, (size_t)n * 4);
		/*
		 * A slot without PH_ENCRYPTED and without room gets the cipher
		 * step's RESOURCE and wire_len = po + plen, which the hash step
		 * then takes for its length: it reads that far.  A plaintext
		 * length is therefore staged as at most the slot's length -- the
		 * code is the same -- so that no read goes more than po <=
		 * kTxSlack bytes past a slot, which the staging has room for.
		 */
		if (cipher)
			for (uint64_t j = 0; j < n; j++)
				hm.plen[j] = std::min(mb.plen_in[lo + j],
				    mb.lens[lo + j]);
	}
	if (dbg_timing())
		fprintf(stderr, "net2 burst mc: %s %zu B: %.3f ms (%zu threads)\n",
		    direct ? "direct" : "pack", bytes, dbg_now() - tp0, plan.nt);
	/* table updates queued on the caller's stream before the call */
	HIP_TRY(hipStreamWaitEvent(s.stream, mb.tables, 0));
	if (!zin) {
		if (bytes != 0)
			HIP_TRY(hipMemcpyAsync(s.d_in, direct ? mb.base + rs : s.h_in,
			    bytes, hipMemcpyHostToDevice, s.stream));
		/* offsets, lengths, headers, slots, plaintext lengths: one copy */
		HIP_TRY(hipMemcpyAsync(s.d_meta, s.h_meta,
		    BurstSlot::mc_meta_bytes(n), hipMemcpyHostToDevice, s.stream));
	}
	FI_POINT(FI_H2D);

	const BurstSlot::Aux st(s.h_out, n), da(s.d_aux, n);
	/* An output array: through the mapping (zc), else in device memory and
	 * copied behind the kernels -- straight into a page-locked caller array,
	 * else into staging for the host to copy from.  user may be null (an
	 * array only the steps or the hand-over need). */
	bool fail = false;
	auto place = [&](void *user, bool pinned, void *stage, void *dev,
	    size_t nbytes) {
		SmallOut o;
		o.bytes = nbytes;
		if (zc) {
			bool copy;
			o.dev = out_ptr(user, pinned, (uint8_t *)stage, &copy);
			o.host = copy ? (uint8_t *)stage : (uint8_t *)user;
			o.user = copy ? (uint8_t *)user : nullptr;
			fail |= o.dev == nullptr;
			return o;
		}
		o.dev = (uint8_t *)dev;
		const bool to_user = user != nullptr && pinned;
		o.host = to_user ? (uint8_t *)user : (uint8_t *)stage;
		o.user = to_user ? nullptr : (uint8_t *)user;
		return o;
	};
	std::vector<SmallOut> outs;
	/* where the chunk's datagrams come back to (null: they do not) */
	uint8_t *back = nullptr;

	SmallOut res, enc, sq, fl, ln;
	if (!mb.tx) {
		const uint32_t ivlen = mb.ivlen;
		res = place(mb.result + lo, pins.result, st.res, da.res, n);
		outs.push_back(res);
		SmallOut iv;
		if (ivlen > 0 && (mb.iv != nullptr || cipher)) {
			iv = place(mb.iv != nullptr ? (uint8_t *)mb.iv + lo * ivlen :
			    nullptr, pins.iv, st.iv, da.iv, (size_t)n * ivlen);
			if (mb.iv != nullptr)
				outs.push_back(iv);
		}
		if (mb.seq_out != nullptr || cipher) {
			sq = place(mb.seq_out != nullptr ? mb.seq_out + lo : nullptr,
			    pins.seq, st.seq, da.seq, (size_t)n * 4);
			fl = place(mb.flags_out != nullptr ? mb.flags_out + lo : nullptr,
			    pins.flags, st.flags, da.flags, (size_t)n * 4);
			if (mb.seq_out != nullptr)
				outs.push_back(sq);
			if (mb.seq_out != nullptr || cipher)
				outs.push_back(fl);	/* the hand-over reads the flags */
		}
		if (fail)
			return EIO;
		if ((rc = decode_burst_mc(mb.tab, dm.conn, ivlen, d_in, dm.off,
		    dm.len, n, res.dev, iv.dev, (uint32_t *)sq.dev,
		    (uint32_t *)fl.dev, s.d_ws, s.stream, wave)) != 0)
			return rc;
		if (cipher) {
			/* in place where the kernels read the chunk, whatever `out`
			 * is -- but never in the caller's buffer when `out` is
			 * another (mapped reads: into the staging then) */
			ln = place(mb.plen_out + lo, pins.len, st.len, da.len,
			    (size_t)n * 4);
			outs.push_back(ln);
			if ((rc = decrypt_burst_mc(mb.ctab, dm.conn, mb.hashlen, d_in,
			    dm.off, dm.len, n, (const uint32_t *)sq.dev,
			    (const uint32_t *)fl.dev, iv.dev, res.dev,
			    z_stage != nullptr ? z_stage : d_in, (uint32_t *)ln.dev,
			    s.stream, cform)) != 0)
				return rc;
			/* the device copy goes straight back where the plaintexts
			 * are at home (every other byte is the byte that came);
			 * else into the staging, of which the host copies the
			 * plaintexts out */
			if (!zin)
				back = home ? mb.base + rs : s.h_in;
		}
	} else if (cipher) {
		/* both steps' codes are staged: the host folds them */
		res = place(nullptr, false, st.res, da.res, n);
		enc = place(nullptr, false, st.enc, da.enc, n);
		ln = place(mb.wire_len + lo, pins.len, st.len, da.len, (size_t)n * 4);
		outs.push_back(res);
		outs.push_back(enc);
		outs.push_back(ln);
		HIP_TRY(net2_launch_ph_iv(dm.hdr, dm.hdr + n, n, 16, da.iv, s.stream));
		if ((rc = encrypt_burst_mc(mb.ctab, dm.conn, mb.hashlen, dm.hdr + n,
		    da.iv, d_in, dm.off, dm.len, dm.plen, n, enc.dev,
		    (uint32_t *)ln.dev, s.stream, cform)) != 0)
			return rc;
		if ((rc = encode_burst_mc(mb.tab, dm.conn, dm.hdr, dm.hdr + n, d_in,
		    dm.off, (const uint32_t *)ln.dev, n, res.dev, s.d_ws, s.stream,
		    wave, nullptr)) != 0)
			return rc;
		if (!zin)
			back = direct ? mb.base + rs : s.h_in;
	} else {
		res = place(mb.result + lo, pins.result, st.res, da.res, n);
		outs.push_back(res);
		if (fail)
			return EIO;
		/*
		 * Datagrams copied as they lie from one page-locked allocation
		 * are sealed straight into the caller's buffer through its
		 * mapping, as enqueue_burst_steps does.  Otherwise they are
		 * sealed where the kernel reads them -- the mapped staging, or
		 * the device copy, which then comes back whole: the table
		 * kernels have no record form -- and the host copies header and
		 * hash field of every OK one into its slot.
		 */
		uint8_t *const seal = direct ? mapped(mb.base + rs) : nullptr;
		if ((rc = encode_burst_mc(mb.tab, dm.conn, dm.hdr, dm.hdr + n, d_in,
		    dm.off, dm.len, n, res.dev, s.d_ws, s.stream, wave,
		    seal != nullptr && seal != d_in ? seal : nullptr)) != 0)
			return rc;
		if (!zc && seal == nullptr)
			back = direct ? mb.base + rs : s.h_in;
	}
	if (!zc)
		for (const SmallOut &o : outs)
			HIP_TRY(hipMemcpyAsync(o.host, o.dev, o.bytes,
			    hipMemcpyDeviceToHost, s.stream));
	if (back != nullptr && bytes != 0)
		HIP_TRY(hipMemcpyAsync(back, s.d_in, bytes, hipMemcpyDeviceToHost,
		    s.stream));
	FI_POINT(FI_RECORD);
	HIP_TRY(hipEventRecord(s.done, s.stream));
	s.busy = true;

	/* the hand-over: staged arrays to the caller's, then what the contract
	 * says changed in the datagram buffer, out of the staging */
	WorkPool *pp = &pool;
	const uint8_t *const stage_in = s.h_in;
	const uint64_t *const st_off = hm.off;
	const bool scatter = !direct;
	const bool from_stage = cipher && !mb.tx && !home;
	s.finish = [=]() {
		for (const SmallOut &o : outs)
			if (o.user != nullptr)
				memcpy(o.user, o.host, o.bytes);
		/* RX plaintexts: a thread per ~512 datagrams, TX per ~4 K, as the
		 * packs (enqueue_burst_steps): per ~4 K one thread copied a whole
		 * 4,096-datagram RX chunk, and per ~512 TX was the slower one */
		const size_t nt = std::min<size_t>(kPackThreads,
		    std::max<size_t>(1, n >> (mb.tx ? 12 : 9)));
		const uint32_t hl = mb.hashlen;
		if (!mb.tx) {
			if (!from_stage)
				return 0;
			/* RX: the plaintext of every decrypted datagram into out */
			const uint32_t *flags = (const uint32_t *)fl.host;
			const uint32_t *plen = (const uint32_t *)ln.host;
			pp->run(nt, [=](size_t t) {
				for (uint64_t j = n * t / nt; j < n * (t + 1) / nt; j++) {
					if (plen[j] == 0)
						continue;
					const uint32_t po = payload_at(flags[j], hl);
					memcpy(mb.out + mb.offsets[lo + j] + po,
					    stage_in + st_off[j] + po, plen[j]);
				}
			});
			return 0;
		}
		const uint8_t *code = res.host, *ecode = enc.host;
		const uint32_t *wire = (const uint32_t *)ln.host;
		if (!cipher && !scatter)
			return 0;
		/* TX: with the cipher the code of every slot (the cipher step's
		 * where that is not OK); of a packed chunk the slots the cipher
		 * step wrote, and header and hash field of every OK one */
		pp->run(nt, [=](size_t t) {
			for (uint64_t j = n * t / nt; j < n * (t + 1) / nt; j++) {
				const uint64_t i = lo + j;
				uint8_t c = code[j];
				if (cipher) {
					if (ecode[j] != NET2_PENCODE_OK)
						c = ecode[j];
					mb.result[i] = c;
				}
				if (!scatter)
					continue;
				const uint32_t f = mb.flags_in[i];
				uint32_t take = 0;
				if (cipher && (f & NET2_PH_ENCRYPTED) != 0 &&
				    ecode[j] == NET2_PENCODE_OK)
					take = wire[j];
				else if (c == NET2_PENCODE_OK)
					take = payload_at(f, hl);
				if (take != 0)
					memcpy(mb.base + mb.offsets[i],
					    stage_in + st_off[j], take);
			}
		});
		return 0;
	};
	return 0;
}

/* The whole call on the tables' device, chunked and double-buffered as
 * run_burst_slice does. */
int run_mc_burst(McBurst &mb, uint64_t n, void *table_stream)
{
	const int ordinal = keytab_device(mb.tab);
	if (int rc = check_table_device(ordinal))
		return rc;
	const std::vector<int> &dv = devices();
	const size_t didx = (size_t)(std::find(dv.begin(), dv.end(), ordinal) -
	    dv.begin());
	const NumaPlace &np = numa_place(ordinal);
	NumaBind bind(np);
	DeviceCtx *c = ctx_for(didx);
	BurstSlot *const slot = c->burst_slot;
	std::lock_guard<std::mutex> g(c->burst_mu);
	/* one event on the caller's table stream, which every chunk's stream
	 * waits for: the updates queued there before the call are seen, with
	 * no host synchronisation */
	if (c->tables_ev == nullptr)
		HIP_TRY(hipEventCreateWithFlags(&c->tables_ev,
		    hipEventDisableTiming));
	HIP_TRY(hipEventRecord(c->tables_ev, (hipStream_t)table_stream));
	mb.tables = c->tables_ev;
	const bool cipher = mb.ctab != nullptr;
	McPins pins;
	pins.base = is_pinned(mb.base);
	pins.result = pinned_span(mb.result, n);
	if (!mb.tx) {
		pins.iv = mb.iv != nullptr && mb.ivlen > 0 &&
		    pinned_span(mb.iv, n * mb.ivlen);
		pins.seq = mb.seq_out != nullptr && pinned_span(mb.seq_out, n * 4);
		pins.flags = mb.flags_out != nullptr &&
		    pinned_span(mb.flags_out, n * 4);
		pins.len = cipher && pinned_span(mb.plen_out, n * 4);
	} else {
		pins.len = cipher && pinned_span(mb.wire_len, n * 4);
	}
	const uint64_t per_chunk = var_chunk_packets(*c->pool, mb.lens, n);
	/* chunk k enqueued, then chunk k - 1 waited for and handed over
	 * (run_burst_slice) */
	int rc = 0, cur = 0;
	for (uint64_t at = 0; at < n && rc == 0;) {
		const uint64_t end = std::min<uint64_t>(n, at + per_chunk);
		const double t0 = dbg_now();
		rc = enqueue_mc_steps(*c->pool, slot[cur], mb, pins, at, end);
		/* a chunk that failed part-way is waited for before the error
		 * goes back, and its slot stays free */
		if (rc != 0)
			quiesce(slot[cur].stream);
		const double t1 = dbg_now();
		if (rc == 0)
			rc = slot[cur ^ 1].drain();
		if (dbg_timing())
			fprintf(stderr, "net2 burst mc: enqueue %.3f ms, drain+finish "
			    "%.3f ms (%llu datagrams)\n", t1 - t0, dbg_now() - t1,
			    (unsigned long long)(end - at));
		at = end;
		cur ^= 1;
	}
	/* both slots drained whatever happened: nothing may still read or
	 * write the caller's memory when the call returns */
	const int rc2 = slot[0].drain();
	const int rc3 = slot[1].drain();
	return rc ? rc : rc2 ? rc2 : rc3;
}

/* What both calls check before any device work, in check_burst_mc_args'
 * order; *go: the burst is not empty. */
int check_mc_host_args(const struct net2_burst_keytab *tab,
    const struct net2_burst_ciphertab *ctab, const uint32_t *conn,
    uint32_t ivlen, const void *base, const uint64_t *offsets,
    const uint32_t *lens, uint64_t n, const uint8_t *result, bool hdr_pair_ok,
    bool cipher_arrays_ok, bool *go)
{
	*go = false;
	if (tab == nullptr)
		return EINVAL;
	int rc = check_burst_arrays(ivlen, base, offsets, lens, n, result);
	if (rc != 0 || n == 0)
		return rc;
	if (conn == nullptr || !hdr_pair_ok)
		return EINVAL;
	if (ctab != nullptr && (ivlen != 16 || !cipher_arrays_ok ||
	    ciphertab_device(ctab) != keytab_device(tab)))
		return EINVAL;
	*go = true;
	return 0;
}

}	/* namespace */

NET2_EXPORT int net2_packet_decode_burst_mc_host(
    const struct net2_burst_keytab *tab,
    const struct net2_burst_ciphertab *ctab, const uint32_t *conn,
    uint32_t ivlen, const void *base, const uint64_t *offsets,
    const uint32_t *lens, uint64_t n, uint8_t *result, void *iv, uint32_t *seq,
    uint32_t *flags, void *out, uint32_t *plen, void *table_stream)
{
	bool go;
	int rc = check_mc_host_args(tab, ctab, conn, ivlen, base, offsets, lens,
	    n, result, (seq == nullptr) == (flags == nullptr),
	    out != nullptr && plen != nullptr, &go);
	if (!go)
		return rc;
	McBurst mb = {};
	mb.tx = false;
	mb.tab = tab;
	mb.ctab = ctab;
	mb.conn = conn;
	mb.hashlen = (uint32_t)digest_len(keytab_hash_alg(tab));
	mb.ivlen = ivlen;
	mb.iv = iv;
	mb.seq_out = seq;
	mb.flags_out = flags;
	mb.out = (uint8_t *)out;
	mb.plen_out = plen;
	mb.base = (uint8_t *)const_cast<void *>(base);
	mb.offsets = offsets;
	mb.lens = lens;
	mb.result = result;
	return run_mc_burst(mb, n, table_stream);
}

NET2_EXPORT int net2_packet_encode_burst_mc_host(
    const struct net2_burst_keytab *tab,
    const struct net2_burst_ciphertab *ctab, const uint32_t *conn,
    const uint32_t *seq, const uint32_t *flags, void *base,
    const uint64_t *offsets, const uint32_t *lens, const uint32_t *plen,
    uint64_t n, uint8_t *result, uint32_t *wire_len, void *table_stream)
{
	bool go;
	int rc = check_mc_host_args(tab, ctab, conn, ctab != nullptr ? 16 : 0, base,
	    offsets, lens, n, result, seq != nullptr && flags != nullptr,
	    plen != nullptr && wire_len != nullptr, &go);
	if (!go)
		return rc;
	McBurst mb = {};
	mb.tx = true;
	mb.tab = tab;
	mb.ctab = ctab;
	mb.conn = conn;
	mb.hashlen = (uint32_t)digest_len(keytab_hash_alg(tab));
	mb.ivlen = ctab != nullptr ? 16 : 0;
	mb.seq_in = seq;
	mb.flags_in = flags;
	mb.plen_in = plen;
	mb.wire_len = wire_len;
	mb.base = (uint8_t *)base;
	mb.offsets = offsets;
	mb.lens = lens;
	mb.result = result;
	return run_mc_burst(mb, n, table_stream);
}
