/*
 * net2_host.h -- internal: what the host units behind the C ABI share
 * (net2_runtime, net2_batch, net2_single, net2_dgram, net2_burst_host,
 * net2_burst_mc_host .cpp).
 * Host orchestration only: argument checks with errno-style returns (the
 * reference maps hash failures to ENOMEM / NET2_P{EN,DE}CODE_RESOURCE,
 * types/signature.n2t:93-95, types/packet.n2t:246-249), device discovery,
 * pinned staging and stream management.  Every digest is computed by the
 * HIP kernels in sha2_kernels.hip; there is deliberately no CPU hashing
 * path, so a missing or unusable GPU is an ENODEV, never a silent fallback.
 */
#ifndef NET2_HOST_H
#define NET2_HOST_H

#include "sha2_launch.h"
#include "net2_pool.h"

#include <hip/hip_runtime.h>

#include <errno.h>
#include <sched.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <memory>

#define NET2_EXPORT extern "C" __attribute__((visibility("default")))

#include "../../include/net2/hash.h"
#include "../../include/net2/packet.h"
#include "../../include/net2/sha2.h"

/* ---- errors and fault injection (net2_runtime.cpp) ------------------------ */

extern thread_local int tl_last_hip_error;	/* net2_sha2_last_hip_error */

int hip_fail(hipError_t e);	/* records e; ENOMEM or EIO */

#define HIP_TRY(expr)                                                        \
	do {                                                                 \
		hipError_t _e = (expr);                                      \
		if (_e != hipSuccess)                                        \
			return hip_fail(_e);                                 \
	} while (0)

/*
 * Test-only fault injection (a -DNET2_FAULT_INJECT=1 build, libnet2_sha2_fi.so;
 * the shipped library compiles it out).  net2_fault_inject(site, k) makes the
 * k-th pass through `site` of a host-pipeline chunk fail as if its HIP call
 * had: FI_H2D once the chunk's input copy is queued, FI_KERNEL once its first
 * kernel is launched, FI_RECORD in place of the chunk's event record.
 * tests/test_gpu_failures.py drives it.
 */
#ifndef NET2_FAULT_INJECT
#define NET2_FAULT_INJECT 0
#endif
enum { FI_H2D = 1, FI_KERNEL = 2, FI_RECORD = 3 };
#if NET2_FAULT_INJECT
bool fi_hit(int site);
#else
constexpr bool fi_hit(int) { return false; }
#endif
#define FI_POINT(site)                                                       \
	do {                                                                 \
		if (fi_hit(site))                                            \
			return hip_fail(hipErrorLaunchFailure);              \
	} while (0)

/* After a chunk failed part-way: wait for what it already queued on st. */
void quiesce(hipStream_t st);

/* NET2_SHA2_DEBUG_TIMING=1: per-chunk host timings on stderr (dbg_now). */
bool dbg_timing();

/* ---- registry (include/net2/hash.h) ------------------------------------ */

struct HashRow {
	const char *name;
	int hashlen;
	int keylen;
};

constexpr HashRow kRows[] = {
	{ "nil", 0, 0 },
	{ "SHA256", 32, 0 },
	{ "SHA384", 48, 0 },
	{ "SHA512", 64, 0 },
	{ "HMAC-SHA256", 32, 32 },
	{ "HMAC-SHA384", 48, 48 },
	{ "HMAC-SHA512", 64, 64 },
};
constexpr int kNumRows = sizeof(kRows) / sizeof(kRows[0]);

inline bool unkeyed_sha2(int alg)
{
	return alg == NET2_HASH_SHA256 || alg == NET2_HASH_SHA384 ||
	    alg == NET2_HASH_SHA512;
}

inline bool hmac_row(int alg)
{
	return alg >= NET2_HASH_HMAC_SHA256 && alg <= NET2_HASH_HMAC_SHA512;
}

inline int digest_len(int alg)
{
	return alg >= 0 && alg < kNumRows ? kRows[alg].hashlen : -1;
}

/* ---- argument predicates, composed by the entry points ------------------- */

/* An HMAC row with a key of the row's length; nil (no key looked at) when
 * nil_ok. */
inline bool hmac_key_ok(int alg, const void *key, size_t keylen, bool nil_ok)
{
	if (alg == NET2_HASH_NIL)
		return nil_ok;
	return hmac_row(alg) && (size_t)kRows[alg].keylen == keylen &&
	    key != nullptr;
}

/* The datagram arrays, and a count the kernels' 32-bit indices hold. */
inline bool dgrams_ok(const void *base, const uint64_t *offsets,
    const uint32_t *lens, uint64_t n)
{
	return base != nullptr && offsets != nullptr && lens != nullptr &&
	    n <= UINT32_MAX;
}

/* No binning workspace, or one of net2_sha2_dev_var_workspace(n) bytes. */
inline bool bin_ws_ok(const void *d_ws, size_t ws_bytes, uint64_t n)
{
	return d_ws == nullptr || (ws_bytes >= net2_sha2_dev_var_workspace(n) &&
	    ((uintptr_t)d_ws & 3) == 0 && n <= UINT32_MAX);
}

/* ---- devices (net2_runtime.cpp) ------------------------------------------ */

const std::vector<int> &devices();	/* HIP ordinals of the gfx950 devices */
std::vector<int> batch_devices();	/* ... as a host-memory call shards */
uint64_t slice_min_bytes();
int check_current_device();	/* 0, or ENODEV: not one we built code for */
size_t small_device(const std::vector<int> &dv);
SliceWorker *slice_worker(size_t idx);

/* NUMA placement of a device's host-side work (numa_place). */
struct NumaPlace {
	int node = -1;
	bool have = false;	/* cpus holds at least one usable CPU */
	cpu_set_t cpus;
};

const NumaPlace &numa_place(int ordinal);
bool numa_enabled();

/* Binds the calling thread to a device's node for its lifetime. */
class NumaBind {
public:
	explicit NumaBind(const NumaPlace &np)
	{
		if (!np.have || !numa_enabled())
			return;
		if (pthread_getaffinity_np(pthread_self(), sizeof(saved_),
		    &saved_) == 0 && pthread_setaffinity_np(pthread_self(),
		    sizeof(np.cpus), &np.cpus) == 0)
			bound_ = true;
	}
	~NumaBind()
	{
		if (bound_)
			(void)pthread_setaffinity_np(pthread_self(),
			    sizeof(saved_), &saved_);
	}
private:
	cpu_set_t saved_;
	bool bound_ = false;
};

/* Page-locked host memory, and a range within one such allocation. */
bool is_pinned(const void *p);
bool pinned_span(const void *p, size_t bytes);

/* The device mapping of page-locked host memory; null without one. */
inline uint8_t *mapped(const void *p)
{
	void *dp = nullptr;
	if (hipHostGetDevicePointer(&dp, const_cast<void *>(p), 0) == hipSuccess)
		return (uint8_t *)dp;
	(void)hipGetLastError();
	return nullptr;
}

/*
 * Where the kernels store a chunk's output of `bytes` bytes bound for the
 * caller's `user` (its chunk slice): straight into it through its device
 * mapping when it is page-locked, else into `stage` (the slot's pinned
 * results, mapped) -- then *copy is set and the caller copies it over once
 * the chunk is done.
 */
inline uint8_t *out_ptr(void *user, bool user_pinned, uint8_t *stage, bool *copy)
{
	uint8_t *dp = user_pinned ? mapped(user) : nullptr;
	*copy = dp == nullptr;
	return dp != nullptr ? dp : mapped(stage);
}

/* ---- per-device staging for the host-memory paths ------------------------ */

template <class T> void drop_host(T *&p) { if (p) (void)hipHostFree(p); p = nullptr; }
template <class T> void drop_dev(T *&p) { if (p) (void)hipFree(p); p = nullptr; }

/* One pipeline slot: a stream, the event of the chunk in flight and what hands
 * that chunk's results over.  Two slots per device and pipeline double-buffer
 * host pack / H2D / kernels / hand-over; the buffers are the pipeline's. */
struct Slot {
	hipStream_t stream = nullptr;
	hipEvent_t done = nullptr;
	bool busy = false;
	size_t cap_in = 0, cap_n = 0;
	/* run once the chunk's kernels are done: results to the caller */
	std::function<int()> finish;

	/* The stream and event at first use.  *fits: `in` payload bytes and `n`
	 * packets are within the capacity; else *in, *n: what to allocate. */
	int open(size_t *in, size_t *n, bool *fits);
	/* after the allocations: bin_ws prepared, so the first chunk bins */
	int grown(void *bin_ws, size_t in, size_t n);
	/* waits for the chunk in flight, if any, and hands it over */
	int drain();
};

/* Host batches: pinned input and digest staging, device input,
 * offsets/lengths and digests, binning workspace. */
struct BatchSlot : Slot {
	uint8_t *h_in = nullptr, *h_dig = nullptr;
	/* a chunk's offsets (8 n bytes) then lengths (4 n): one copy */
	uint64_t *h_off = nullptr;
	uint8_t *d_in = nullptr, *d_dig = nullptr;
	uint64_t *d_off = nullptr;
	uint32_t *d_ws = nullptr;

	void release();
	int reserve(size_t in, size_t n, bool host_in);
};

/* Host bursts: pinned staging for the packed datagrams, their metadata and
 * results bound for pageable memory, device copies, the burst workspace. */
struct BurstSlot : Slot {
	uint8_t *h_in = nullptr, *h_out = nullptr;
	/* a chunk's per-datagram metadata, one block so it is one copy:
	 * offsets (8 n), lengths (4 n), TX headers (8 n); over many connections
	 * also the slots (4 n) and TX plaintext lengths (4 n) -- see Meta */
	uint8_t *h_meta = nullptr;
	uint8_t *d_in = nullptr, *d_ws = nullptr, *d_meta = nullptr;
	/* bursts over many connections: a chunk's per-datagram results in device
	 * memory (Aux), where the cipher step reads what the hash step left;
	 * allocated by the first such burst (reserve_aux) */
	uint8_t *d_aux = nullptr;
	size_t cap_aux = 0;

	/* The metadata arrays of an n-datagram chunk inside a meta block. */
	struct Meta {
		uint64_t *off;
		uint32_t *len, *hdr, *conn, *plen;
		Meta(uint8_t *m, size_t n) : off((uint64_t *)m),
		    len((uint32_t *)(m + 8 * n)), hdr((uint32_t *)(m + 12 * n)),
		    conn((uint32_t *)(m + 20 * n)), plen((uint32_t *)(m + 24 * n)) {}
	};
	static size_t meta_bytes(size_t n, bool tx) { return n * (tx ? 20 : 12); }
	static size_t mc_meta_bytes(size_t n) { return n * 28; }
	/* results staged per datagram: RX code + IV (<= 64) + header; TX code
	 * + record (hash field + header, <= 80); over many connections an Aux */
	static size_t out_bytes(size_t n) { return n * 81 + 256; }

	/* The per-datagram results of an n-datagram chunk over many connections,
	 * every array 16-byte aligned: in d_aux, and staged in h_out (at most
	 * 78 n + 96 bytes, within out_bytes).  len: RX plaintext lengths, TX
	 * wire lengths; enc: the TX cipher step's codes. */
	struct Aux {
		uint8_t *res, *enc;
		uint32_t *seq, *flags, *len;
		uint8_t *iv;
		Aux(uint8_t *b, size_t n) : res(b), enc(b + a16z(n)),
		    seq((uint32_t *)(b + 2 * a16z(n))),
		    flags((uint32_t *)(b + 2 * a16z(n) + a16z(4 * n))),
		    len((uint32_t *)(b + 2 * a16z(n) + 2 * a16z(4 * n))),
		    iv(b + 2 * a16z(n) + 3 * a16z(4 * n)) {}
		static size_t a16z(size_t x) { return (x + 15) & ~(size_t)15; }
		static size_t bytes(size_t n, size_t ivlen)
		{
			return 2 * a16z(n) + 3 * a16z(4 * n) + a16z(n * ivlen);
		}
	};

	void release();
	int reserve(size_t in, size_t n);
	/* after reserve: d_aux for cap_n datagrams with IVs of ivlen bytes */
	int reserve_aux(size_t ivlen);
};

/* A device's host-side state.  The pipelines hold different locks: a batch and
 * a host burst may run at once on one device, sharing only the pack pool. */
struct DeviceCtx {
	WorkPool *pool = new WorkPool();	/* never freed, see WorkPool */
	std::mutex mu;		/* one host-memory batch per device at a time */
	BatchSlot slot[2];
	std::mutex burst_mu;	/* one host burst per device at a time */
	BurstSlot burst_slot[2];
	/* under burst_mu: what a host burst over many connections records on the
	 * caller's table stream and its chunks' streams wait for */
	hipEvent_t tables_ev = nullptr;
	/* net2_sha2_numa_stats: slices run, and those whose thread was on
	 * the device's NUMA node when it finished */
	std::atomic<uint64_t> slices{0}, slices_on_node{0};
};

DeviceCtx *ctx_for(size_t idx);

/* ---- packing chunks into staging (net2_batch.cpp) ------------------------ */

/* Chunk payload target for the host pipelines, and the threads a chunk is
 * packed by: the CPU share of one GPU on an MI355X node. */
constexpr size_t kChunkBytes = 64u << 20;
#ifndef NET2_PACK_THREADS
#define NET2_PACK_THREADS 16
#endif
constexpr size_t kPackThreads = NET2_PACK_THREADS;

struct PackPlan {
	size_t nt = 1;
	size_t start[kPackThreads + 1] = {};	/* start[nt] = total bytes */
};

PackPlan pack_sizes(WorkPool &pool, const uint32_t *lens, uint64_t n,
    int per_shift = 12);
void pack_fill(WorkPool &pool, const PackPlan &pl, uint8_t *dst,
    uint64_t *dst_off, uint32_t *dst_len, const uint8_t *base,
    const uint64_t *offsets, const uint32_t *lens, uint64_t n);
bool dense_pinned(WorkPool &pool, const uint8_t *base, const uint64_t *off,
    const uint32_t *ln, uint64_t n, uint64_t *rs, uint64_t *re);
void rebase_meta(WorkPool &pool, const uint64_t *off, const uint32_t *ln,
    uint64_t n, uint64_t rs, uint64_t *dst_off, uint32_t *dst_len);
uint64_t var_chunk_packets(WorkPool &pool, const uint32_t *lens, uint64_t n);

/* ---- form knobs and launch counters (net2_dgram.cpp) ---------------------- */

/*
 * A size threshold between two forms of a launch: what the C ABI set
 * (set(v); v < 0 clears it), else the environment variable as it was at
 * first use (A/B runs, one process per setting), else the caller's default.
 * Relaxed atomics, no lock: a thread reading while another sets sees the old
 * value or the new one.
 */
struct FormKnob {
	const char *env_name;
	std::atomic<int64_t> setting{-1};	/* -1: none */
	std::atomic<int64_t> env{-2};		/* -2: not read yet; -1: not there */

	void set(int64_t v)
	{
		setting.store(v < 0 ? -1 : v, std::memory_order_relaxed);
	}
	uint64_t get(uint64_t dflt)
	{
		uint64_t v;
		return get(&v) ? v : dflt;
	}
	/* false: neither set nor in the environment -- the default holds, which
	 * a caller whose default costs something works out only then */
	bool get(uint64_t *v)
	{
		int64_t x = setting.load(std::memory_order_relaxed);
		if (x < 0 && (x = env.load(std::memory_order_relaxed)) == -2) {
			const char *e = getenv(env_name);
			x = e != nullptr && *e != '\0' ?
			    (int64_t)(strtoull(e, nullptr, 10) & INT64_MAX) : -1;
			env.store(x, std::memory_order_relaxed);
		}
		if (x < 0)
			return false;
		*v = (uint64_t)x;
		return true;
	}
};

/* Launches by form (the *_stats calls). */
struct FormCounts {
	std::atomic<uint64_t> lane{0}, wave{0};

	void count(bool is_wave)
	{
		(is_wave ? wave : lane).fetch_add(1, std::memory_order_relaxed);
	}
	void read(uint64_t *lanes, uint64_t *waves) const
	{
		if (lanes != nullptr)
			*lanes = lane.load(std::memory_order_relaxed);
		if (waves != nullptr)
			*waves = wave.load(std::memory_order_relaxed);
	}
};

/* The largest keyed hash burst that takes the wave form on the current
 * device: net2_sha2_burst_limits' setting, else NET2_BURST_WAVE_MAX (0:
 * never), else net2_burst_wave_default(). */
uint64_t net2_burst_wave_max(void);

/* keyed host bursts of at most this many datagrams read their datagrams and
 * metadata through the host mapping (enqueue_burst_steps) */
#ifndef NET2_BURST_ZC_MAX
#define NET2_BURST_ZC_MAX 16384
#endif

/* ---- the burst steps (net2_dgram.cpp) ------------------------------------- */

inline size_t a16(size_t x) { return (x + 15) & ~(size_t)15; }

/* The workspace of an n-datagram burst, carved from base into *w (each may be
 * null); its size (net2_packet_burst_workspace). */
struct BurstWs;
size_t burst_layout(uint64_t n, uint8_t *base, BurstWs *w);

/* The hash steps of a burst on device-visible memory.  wave: the small-burst
 * form (keyed bursts only), decided once by the caller from
 * net2_burst_wave_max(). */
int decode_burst(const struct net2_burst_rx_keys *k, uint32_t ivlen,
    const void *d_base, const uint64_t *d_offsets, const uint32_t *d_lens,
    uint64_t n, uint8_t *d_result, void *d_iv, uint32_t *d_seq,
    uint32_t *d_flags, void *d_ws, hipStream_t s, bool hdr_out, bool wave);
int encode_burst(int hash_alg, const void *hash_key, size_t hash_keylen,
    int enc_alg, const uint32_t *d_seq, const uint32_t *d_flags,
    void *d_base, const uint64_t *d_offsets, const uint32_t *d_lens,
    uint64_t n, uint8_t *d_result, void *d_ws, hipStream_t s, bool wave,
    uint8_t *rec, bool bin = true, uint8_t *seal_to = nullptr);

/*
 * The same over many connections: the launches of net2_packet_{decode,encode}_
 * burst_mc and net2_packet_{decrypt,encrypt}_burst_mc on device-visible
 * memory, the arguments already checked.  The form is the caller's, decided
 * once per chunk: wave from net2_burst_wave_max(), the cipher's from
 * aes_wave_form(n) (decrypt) and aes_quad_form(n) (encrypt).  seal_to as
 * encode_burst's.
 */
struct Net2CipherEnt;
struct TabStage;
/*
 * The two tables of include/net2/packet.h: `slots` entries (Net2KeyEnt,
 * sha2_launch.h, all of one HMAC row; Net2CipherEnt, aes_tab.h) in the memory
 * of the device that was current when the table was made.  Entries change
 * only through the set / clear calls (net2_dgram.cpp), each one launch in the
 * caller's stream, and through the bulk updates (net2_tabs.cpp), whose
 * page-locked staging is `stage`, made by the first of them.
 */
struct net2_burst_keytab {
	int device;
	int hash_alg;
	uint32_t slots;
	Net2KeyEnt *ents;
	TabStage *stage;
};
struct net2_burst_ciphertab {
	int device;
	uint32_t slots;
	Net2CipherEnt *ents;
	TabStage *stage;
};
/* Waits for the staging's launches, wipes and frees it (null: nothing). */
void tab_stage_destroy(TabStage *st);
/* net2_burst_tab_stats' count of per-slot launches (net2_tabs.cpp). */
void tab_slot_launched();
/* aes256 with a 32-byte key, and as long an alternate key or none */
int check_cipher_keys(const struct net2_burst_cipher_keys *ck);
int keytab_device(const struct net2_burst_keytab *tab);
int keytab_hash_alg(const struct net2_burst_keytab *tab);
int ciphertab_device(const struct net2_burst_ciphertab *tab);
/* Arguments first (by the caller), then: a usable device, and the table's. */
int check_table_device(int device);
bool aes_wave_form(uint64_t n);
bool aes_quad_form(uint64_t n);
int decode_burst_mc(const struct net2_burst_keytab *tab, const uint32_t *d_conn,
    uint32_t ivlen, const void *d_base, const uint64_t *d_offsets,
    const uint32_t *d_lens, uint64_t n, uint8_t *d_result, void *d_iv,
    uint32_t *d_seq, uint32_t *d_flags, void *d_ws, hipStream_t s, bool wave);
int encode_burst_mc(const struct net2_burst_keytab *tab, const uint32_t *d_conn,
    const uint32_t *d_seq, const uint32_t *d_flags, void *d_base,
    const uint64_t *d_offsets, const uint32_t *d_lens, uint64_t n,
    uint8_t *d_result, void *d_ws, hipStream_t s, bool wave, uint8_t *seal_to);
int decrypt_burst_mc(const struct net2_burst_ciphertab *tab,
    const uint32_t *d_conn, uint32_t hashlen, const void *d_base,
    const uint64_t *d_offsets, const uint32_t *d_lens, uint64_t n,
    const uint32_t *d_seq, const uint32_t *d_flags, const void *d_iv,
    uint8_t *d_result, void *d_out, uint32_t *d_plen, hipStream_t s, bool wave);
int encrypt_burst_mc(const struct net2_burst_ciphertab *tab,
    const uint32_t *d_conn, uint32_t hashlen, const uint32_t *d_flags,
    const void *d_iv, void *d_base, const uint64_t *d_offsets,
    const uint32_t *d_lens, const uint32_t *d_plen, uint64_t n,
    uint8_t *d_result, uint32_t *d_wire_len, hipStream_t s, bool quad);

/* What every burst entry checks once its keys are accepted: the IV length,
 * then -- of a burst that is not empty -- the arrays. */
inline int check_burst_arrays(uint32_t ivlen, const void *base,
    const uint64_t *offsets, const uint32_t *lens, uint64_t n,
    const uint8_t *result)
{
	if (ivlen > 64)
		return EINVAL;
	if (n == 0)
		return 0;
	return dgrams_ok(base, offsets, lens, n) && result != nullptr ? 0 :
	    EINVAL;
}

/*
 * Shards a host-memory batch of n packets over the devices (net2_sha2_batch,
 * the host packet bursts): contiguous slices -- by packet count for the
 * fixed layout (lens == NULL), by bytes otherwise -- no slice under
 * slice_min_bytes() of payload, each extra device's slice on that device's
 * persistent worker (SliceWorker).  The device list starts at the caller's
 * device (small_device), so one process per GPU with max_devices == 1 stays
 * on its own device.  fn(didx, ordinal, lo, hi)
 * runs one slice; the first error is returned.
 */
template <class F>
int shard_batch(uint64_t n, const uint32_t *lens, uint32_t fixed_len,
    int max_devices, const F &fn)
{
	const std::vector<int> dv = batch_devices();
	if (dv.empty())
		return ENODEV;
	size_t nd = dv.size();
	if (max_devices > 0 && (size_t)max_devices < nd)
		nd = (size_t)max_devices;
	if ((uint64_t)nd > n)
		nd = (size_t)n;
	uint64_t total = 0;
	if (lens == nullptr) {
		total = n * (uint64_t)fixed_len;
	} else {
		for (uint64_t i = 0; i < n; i++)
			total += lens[i];
	}
	const uint64_t min_slice = slice_min_bytes();
	if (min_slice > 0 && nd > 1)
		nd = (size_t)std::max<uint64_t>(1, std::min<uint64_t>(nd,
		    total / min_slice));

	/* Contiguous slices: by packet count, or by bytes for var layout. */
	std::vector<uint64_t> cut(nd + 1, 0);
	cut[nd] = n;
	if (lens == nullptr) {
		for (size_t d = 1; d < nd; d++)
			cut[d] = n * d / nd;
	} else {
		uint64_t acc = 0;
		size_t d = 1;
		for (uint64_t i = 0; i < n && d < nd; i++) {
			acc += lens[i];
			while (d < nd && acc * nd >= total * d)
				cut[d++] = i + 1;
		}
		for (; d < nd; d++)
			cut[d] = n;
	}

	int prev = -1;
	(void)hipGetDevice(&prev);
	const size_t first = small_device(dv);
	std::vector<int> rcs(nd, 0);
	struct {
		std::mutex m;
		std::condition_variable cv;
		size_t left;
	} done;
	done.left = nd - 1;
	for (size_t d = 1; d < nd; d++) {
		const size_t e = (first + d) % dv.size();
		slice_worker(e)->post([&, d, e]() {
			rcs[d] = fn(e, dv[e], cut[d], cut[d + 1]);
			std::lock_guard<std::mutex> g(done.m);
			if (--done.left == 0)
				done.cv.notify_all();
		});
	}
	rcs[0] = fn(first, dv[first], cut[0], cut[1]);
	{
		std::unique_lock<std::mutex> lk(done.m);
		done.cv.wait(lk, [&]() { return done.left == 0; });
	}
	if (prev >= 0)
		(void)hipSetDevice(prev);
	for (int r : rcs)
		if (r != 0)
			return r;
	return 0;
}

#endif /* NET2_HOST_H */
