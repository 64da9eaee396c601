/*
 * net2_tabs.cpp -- bulk updates and fingerprints of the two device tables of
 * the bursts over many connections (net2_burst_keytab_update,
 * net2_burst_ciphertab_update, net2_burst_*_fingerprint; include/net2/packet.h).
 * Argument checks, the op list reduced per launch to one record per slot
 * (net2_tab_ops.h), the records staged in page-locked memory the table owns,
 * and the launches of tab_kernels.hip in the caller's stream.
 */
#include "net2_host.h"
#include "net2_tab_ops.h"
#include "tab_launch.h"

#include <mutex>
#include <new>
#include <vector>

static_assert(NET2_TR_KT_RX == NET2_KT_RX && NET2_TR_KT_TX == NET2_KT_TX &&
    NET2_TR_KT_RX_ALT == NET2_KT_RX_ALT && NET2_TR_KT_RX_NOCUT == NET2_KT_RX_NOCUT &&
    NET2_TR_KT_RX_ENC == NET2_KT_RX_ENC && NET2_TR_KT_TX_ENC == NET2_KT_TX_ENC,
    "the records' bits are the key table's");

/*
 * A table's staging: a ring of page-locked areas, each with the event recorded
 * behind the kernel that reads -- and zeroes -- it.  An area is FREE, taken by
 * one call while that call fills it and launches (FILLING), then INFLIGHT
 * until its event is done.  The ring starts with two areas and grows on
 * demand up to kMaxAreas; only when all of those are in flight does a call
 * wait on the host, for the oldest.  mu guards the states; an area's memory
 * belongs to the call that took it.
 */
struct TabArea {
	enum State { FREE, FILLING, INFLIGHT };
	uint8_t *h = nullptr;		/* page-locked */
	uint8_t *d = nullptr;		/* its device pointer */
	size_t cap = 0;
	hipEvent_t done = nullptr;
	State state = FREE;
	uint64_t seq = 0;		/* launch order, for "the oldest" */
};

struct TabStage {
	static constexpr size_t kMinAreas = 2, kMaxAreas = 8;
	std::mutex mu;
	std::vector<TabArea *> areas;
	uint64_t launches = 0;
};

namespace {

FormKnob g_tab_ops_per_launch{"NET2_BURST_TAB_OPS"};
constexpr uint64_t TAB_OPS_DEFAULT = 65536;
std::atomic<uint64_t> g_slot_launches{0}, g_bulk_launches{0};
/* one staging per table, made by the first bulk update of any thread */
std::mutex g_stage_make;

void area_release(TabArea *a)
{
	if (a->h != nullptr) {
		key_wipe(a->h, a->cap);
		(void)hipHostFree(a->h);
	}
	a->h = a->d = nullptr;
	a->cap = 0;
}

/* At least `bytes` of page-locked memory in a (which no launch is reading). */
int area_reserve(TabArea *a, size_t bytes)
{
	if (a->done == nullptr)
		HIP_TRY(hipEventCreateWithFlags(&a->done, hipEventDisableTiming));
	if (a->cap >= bytes)
		return 0;
	area_release(a);
	/* room to spare, so a table that grows op by op does not reallocate
	 * every time */
	const size_t cap = std::max<size_t>(bytes + bytes / 2, 64 * 1024);
	HIP_TRY(hipHostMalloc((void **)&a->h, cap, hipHostMallocDefault));
	a->cap = cap;
	/* never handed out with a stale byte in it */
	memset(a->h, 0, cap);
	a->d = mapped(a->h);
	if (a->d == nullptr) {
		area_release(a);
		return hip_fail(hipErrorInvalidValue);
	}
	return 0;
}

TabStage *stage_of(TabStage **slot)
{
	std::lock_guard<std::mutex> g(g_stage_make);
	if (*slot == nullptr)
		*slot = new (std::nothrow) TabStage();
	return *slot;
}

/* A FILLING area of at least `bytes`; ENOMEM / EIO. */
int stage_take(TabStage *st, size_t bytes, TabArea **out)
{
	TabArea *a = nullptr;
	{
		std::unique_lock<std::mutex> lk(st->mu);
		for (;;) {
			TabArea *oldest = nullptr;
			for (TabArea *c : st->areas) {
				if (c->state == TabArea::INFLIGHT &&
				    hipEventQuery(c->done) == hipSuccess)
					c->state = TabArea::FREE;
				if (c->state == TabArea::FREE && (a == nullptr ||
				    c->cap > a->cap))
					a = c;
				if (c->state == TabArea::INFLIGHT && (oldest == nullptr ||
				    c->seq < oldest->seq))
					oldest = c;
			}
			(void)hipGetLastError();	/* (hipErrorNotReady) */
			if (a != nullptr)
				break;
			if (st->areas.size() < TabStage::kMaxAreas) {
				/* the ring grows: at first use to two areas, later
				 * by the one this call needs */
				const size_t want = std::max(TabStage::kMinAreas,
				    st->areas.size() + 1);
				while (st->areas.size() < want) {
					TabArea *c = new (std::nothrow) TabArea();
					if (c == nullptr)
						return ENOMEM;
					st->areas.push_back(c);
				}
				continue;
			}
			if (oldest == nullptr) {
				/* every area is being filled by other calls: the
				 * ring is as large as it gets, so let them launch */
				lk.unlock();
				sched_yield();
				lk.lock();
				continue;
			}
			/* every area in flight: wait for the oldest launch */
			hipEvent_t ev = oldest->done;
			lk.unlock();
			hipError_t e = hipEventSynchronize(ev);
			lk.lock();
			if (e != hipSuccess)
				return hip_fail(e);
		}
		a->state = TabArea::FILLING;
	}
	if (int rc = area_reserve(a, bytes)) {
		std::lock_guard<std::mutex> g(st->mu);
		a->state = TabArea::FREE;
		return rc;
	}
	*out = a;
	return 0;
}

/* After the launch over a (e: what the launch returned): the event recorded
 * behind it, or -- nothing launched -- the area wiped and free again. */
int stage_launched(TabStage *st, TabArea *a, size_t used, hipError_t e,
    hipStream_t s)
{
	if (e == hipSuccess)
		e = hipEventRecord(a->done, s);
	std::lock_guard<std::mutex> g(st->mu);
	if (e != hipSuccess) {
		/* the kernel may be queued without its event: wait it out before
		 * the area can be handed out again */
		(void)hipStreamSynchronize(s);
		key_wipe(a->h, used);
		a->state = TabArea::FREE;
		return hip_fail(e);
	}
	a->seq = ++st->launches;
	a->state = TabArea::INFLIGHT;
	return 0;
}

uint64_t ops_per_launch()
{
	return std::max<uint64_t>(1, g_tab_ops_per_launch.get(TAB_OPS_DEFAULT));
}

/* EINVAL for a stream that is being captured: a graph cannot own the staging. */
int check_not_capturing(void *stream)
{
	if (stream == nullptr)
		return 0;	/* (the null stream cannot be captured) */
	hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
	if (hipStreamIsCapturing((hipStream_t)stream, &cs) != hipSuccess) {
		(void)hipGetLastError();
		return 0;	/* not a stream we can tell about: the launch will */
	}
	return cs == hipStreamCaptureStatusNone ? 0 : EINVAL;
}

/* net2_burst_keytab_set_rx / _set_tx / _clear's checks of one op. */
int check_keytab_op(const struct net2_burst_keytab *tab,
    const struct net2_burst_keytab_op &o)
{
	const size_t keylen = (size_t)kRows[tab->hash_alg].keylen;
	if (o.slot >= tab->slots)
		return EINVAL;
	switch (o.op) {
	case NET2_BURST_TAB_CLEAR:
		return 0;
	case NET2_BURST_TAB_RX:
		if (o.rx.hash_alg != tab->hash_alg || o.rx.hash_key == nullptr ||
		    o.rx.hash_keylen != keylen)
			return EINVAL;
		if (o.rx.alt_hash_key != nullptr && o.rx.alt_hash_keylen != keylen)
			return EINVAL;
		return 0;
	case NET2_BURST_TAB_TX:
		return o.tx_key != nullptr && o.tx_keylen == keylen ? 0 : EINVAL;
	default:
		return EINVAL;
	}
}

/* net2_burst_ciphertab_set_rx / _set_tx / _clear's checks of one op. */
int check_ciphertab_op(const struct net2_burst_ciphertab *tab,
    const struct net2_burst_ciphertab_op &o)
{
	if (o.slot >= tab->slots)
		return EINVAL;
	switch (o.op) {
	case NET2_BURST_TAB_CLEAR:
		return 0;
	case NET2_BURST_TAB_RX:
		if (check_cipher_keys(&o.ck) != 0)
			return EINVAL;
		if (o.rx.hash_alg != NET2_HASH_NIL && !hmac_row(o.rx.hash_alg))
			return EINVAL;
		if (o.rx.alt_hash_key != nullptr && (o.rx.hash_alg == NET2_HASH_NIL ||
		    o.ck.alt_enc_key == nullptr))
			return EINVAL;
		return 0;
	case NET2_BURST_TAB_TX:
		return check_cipher_keys(&o.ck);
	default:
		return EINVAL;
	}
}

/*
 * The checked list, launch by launch: each at most ops_per_launch() ops,
 * reduced on its own (a slot may appear in several launches; stream order
 * keeps them apart), its records written straight into a staging area.
 * fill(r, i): record i of the launch's reduction r into the area; launch(d,
 * n): the kernel over n records at device pointer d.
 */
template <class Rec, class Op, class Fill, class Launch>
int run_update(TabStage **stage_slot, const Op *ops, size_t n, bool keep_dead,
    hipStream_t s, const Fill &fill, const Launch &launch)
{
	TabStage *st = stage_of(stage_slot);
	if (st == nullptr)
		return ENOMEM;
	const uint64_t per = ops_per_launch();
	std::vector<TabSlotOps> recs;
	for (size_t at = 0; at < n; at += per) {
		const size_t m = (size_t)std::min<uint64_t>(per, n - at);
		tab_reduce(ops + at, m, keep_dead, recs);
		const size_t bytes = recs.size() * sizeof(Rec);
		TabArea *a = nullptr;
		if (int rc = stage_take(st, bytes, &a))
			return rc;
		Rec *h = (Rec *)a->h;
		for (size_t i = 0; i < recs.size(); i++)
			fill(ops + at, recs[i], h + i);
		const hipError_t e = launch(a->d, (uint32_t)recs.size());
		if (int rc = stage_launched(st, a, bytes, e, s))
			return rc;
		g_bulk_launches.fetch_add(1, std::memory_order_relaxed);
	}
	return 0;
}

}	/* namespace */

void tab_stage_destroy(TabStage *st)
{
	if (st == nullptr)
		return;
	for (TabArea *a : st->areas) {
		if (a->state == TabArea::INFLIGHT)
			(void)hipEventSynchronize(a->done);
		area_release(a);
		if (a->done != nullptr)
			(void)hipEventDestroy(a->done);
		delete a;
	}
	delete st;
}

void tab_slot_launched()
{
	g_slot_launches.fetch_add(1, std::memory_order_relaxed);
}

NET2_EXPORT int net2_burst_tab_limits(int64_t ops_per_launch)
{
	g_tab_ops_per_launch.set(ops_per_launch);
	return 0;
}

NET2_EXPORT int net2_burst_tab_stats(uint64_t *slot_launches,
    uint64_t *bulk_launches)
{
	if (slot_launches != nullptr)
		*slot_launches = g_slot_launches.load(std::memory_order_relaxed);
	if (bulk_launches != nullptr)
		*bulk_launches = g_bulk_launches.load(std::memory_order_relaxed);
	return 0;
}

NET2_EXPORT int net2_burst_keytab_update(struct net2_burst_keytab *tab,
    const struct net2_burst_keytab_op *ops, size_t n, void *stream)
{
	if (tab == nullptr || (ops == nullptr && n > 0) || n > UINT32_MAX)
		return EINVAL;
	for (size_t i = 0; i < n; i++)
		if (int rc = check_keytab_op(tab, ops[i]))
			return rc;
	if (n == 0)
		return 0;
	if (int rc = check_not_capturing(stream))
		return rc;
	if (int rc = check_table_device(tab->device))
		return rc;
	const size_t keylen = (size_t)kRows[tab->hash_alg].keylen;
	const hipStream_t s = (hipStream_t)stream;
	/* a key-table CLEAR leaves the entry's other bytes: dead ops are kept */
	return run_update<TabHashRec>(&tab->stage, ops, n, true, s,
	    [&](const struct net2_burst_keytab_op *o, const TabSlotOps &r,
	    TabHashRec *h) { tab_hash_rec(o, r, keylen, h); },
	    [&](uint8_t *d, uint32_t m) {
		return net2_launch_keytab_update(tab->hash_alg, tab->ents, tab->slots,
		    d, m, s);
	    });
}

NET2_EXPORT int net2_burst_ciphertab_update(struct net2_burst_ciphertab *tab,
    const struct net2_burst_ciphertab_op *ops, size_t n, void *stream)
{
	if (tab == nullptr || (ops == nullptr && n > 0) || n > UINT32_MAX)
		return EINVAL;
	for (size_t i = 0; i < n; i++)
		if (int rc = check_ciphertab_op(tab, ops[i]))
			return rc;
	if (n == 0)
		return 0;
	if (int rc = check_not_capturing(stream))
		return rc;
	if (int rc = check_table_device(tab->device))
		return rc;
	const hipStream_t s = (hipStream_t)stream;
	return run_update<TabCipherRec>(&tab->stage, ops, n, false, s,
	    [&](const struct net2_burst_ciphertab_op *o, const TabSlotOps &r,
	    TabCipherRec *h) { tab_cipher_rec(o, r, h); },
	    [&](uint8_t *d, uint32_t m) {
		return net2_launch_ciphertab_update(tab->ents, tab->slots, d, m, s);
	    });
}

/* ---- fingerprints ---------------------------------------------------------- */

/* SHA-256 of each of n entries of ent_bytes from `first`: the fixed-stride
 * digest kernel over the table's own memory. */
static int fingerprint(int device, const void *ents, uint32_t slots,
    size_t ent_bytes, uint32_t first, uint32_t n, void *d_digests, void *stream)
{
	if ((uint64_t)first + n > slots || (d_digests == nullptr && n > 0))
		return EINVAL;
	if (n == 0)
		return 0;
	if (int rc = check_table_device(device))
		return rc;
	HIP_TRY(net2_launch_fixed(NET2_ALG_SHA256,
	    (const uint8_t *)ents + (size_t)first * ent_bytes, ent_bytes,
	    (uint32_t)ent_bytes, n, (uint8_t *)d_digests, (hipStream_t)stream));
	return 0;
}

NET2_EXPORT int net2_burst_keytab_fingerprint(const struct net2_burst_keytab *tab,
    uint32_t first, uint32_t n, void *d_digests, void *stream)
{
	if (tab == nullptr)
		return EINVAL;
	return fingerprint(tab->device, tab->ents, tab->slots, sizeof(Net2KeyEnt),
	    first, n, d_digests, stream);
}

NET2_EXPORT int net2_burst_ciphertab_fingerprint(
    const struct net2_burst_ciphertab *tab, uint32_t first, uint32_t n,
    void *d_digests, void *stream)
{
	if (tab == nullptr)
		return EINVAL;
	return fingerprint(tab->device, tab->ents, tab->slots,
	    NET2_AES_TAB_ENT_BYTES, first, n, d_digests, stream);
}
