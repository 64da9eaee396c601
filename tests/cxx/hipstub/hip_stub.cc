/*
 * hip_stub.cc -- TEST INFRASTRUCTURE ONLY: the host-only runtime declared in
 * hip/hip_runtime.h here, and a stand-in for net2_launch_jobs
 * (csrc/sha2_launch.h) that executes a launch's jobs on the stream's worker
 * thread exactly as the kernels' contract says: nblk blocks from stage +
 * data, from the IV or the raw state at stage + aux, the HMAC outer hash
 * over the K' ^ opad block at stage + aux, the final state as raw words at
 * out + 64 * j, then one release-ordered increment of *done per wave (per
 * job in the wave form, per 64 jobs of a family in the lane form).
 * tests/cxx/jobs_battery.h pins it to the contract the real kernels are
 * held to.
 *
 * Staging is read and results are written here, in instrumented code
 * (memcpy into and out of local buffers), so a missing happens-before edge
 * between a caller's copy and the launch, or between the results and their
 * reader, is a ThreadSanitizer report.  Only the compression arithmetic is
 * the oracle's (oracle/sha2_oracle.c, compiled without instrumentation).
 */
#include <hip/hip_runtime.h>

#include "sha2_launch.h"

#include "../../../oracle/sha2_oracle.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <utility>

namespace {

struct Alloc {
	size_t size;
	bool host;
};

struct Hook {
	unsigned k = 0;
	hipError_t e = hipSuccess;
};

/* allocations, hooks, counters and the launch log */
std::mutex g_mu;
std::map<uintptr_t, Alloc> g_allocs;
Hook g_hook[hipstub::NUM_CALLS];
uint64_t g_calls[hipstub::NUM_CALLS];
std::vector<hipstub::LaunchRec> g_log;
uint64_t g_violations, g_jobs_queued;
size_t g_host_live, g_host_max;

std::mutex g_gate_mu;
std::condition_variable g_gate_cv;
bool g_gate_closed;

thread_local int tl_device = 0;

/* Count the call; the error it is to fail with, or hipSuccess. */
hipError_t enter(hipstub::Call c)
{
	std::lock_guard<std::mutex> g(g_mu);
	g_calls[c]++;
	Hook &h = g_hook[c];
	if (h.k != 0 && --h.k == 0)
		return h.e;
	return hipSuccess;
}

hipError_t alloc(void **p, size_t bytes, bool host, uint8_t fill)
{
	void *q = nullptr;
	if (p == nullptr || bytes == 0)
		return hipErrorInvalidValue;
	if (posix_memalign(&q, 4096, bytes) != 0)
		return hipErrorOutOfMemory;
	memset(q, fill, bytes);		/* fresh memory holds nothing useful */
	std::lock_guard<std::mutex> g(g_mu);
	g_allocs[(uintptr_t)q] = { bytes, host };
	if (host) {
		g_host_live += bytes;
		g_host_max = std::max(g_host_max, bytes);
	}
	*p = q;
	return hipSuccess;
}

hipError_t release(void *p, bool host)
{
	if (p == nullptr)
		return hipSuccess;
	{
		std::lock_guard<std::mutex> g(g_mu);
		auto it = g_allocs.find((uintptr_t)p);
		if (it == g_allocs.end() || it->second.host != host)
			return hipErrorInvalidValue;
		if (host)
			g_host_live -= it->second.size;
		g_allocs.erase(it);
	}
	free(p);
	return hipSuccess;
}

/* The recorded allocation [p, p + len) lies in; false if none. */
bool find_alloc(const void *p, size_t len, uintptr_t *start, Alloc *a)
{
	std::lock_guard<std::mutex> g(g_mu);
	auto it = g_allocs.upper_bound((uintptr_t)p);
	if (it == g_allocs.begin())
		return false;
	--it;
	if ((uintptr_t)p + len > it->first + it->second.size)
		return false;
	*start = it->first;
	*a = it->second;
	return true;
}

struct Task {
	std::function<void()> fn;
	bool launch;
};

}	/* namespace */

struct hipstubStream {
	std::mutex mu;
	std::condition_variable cv;
	std::deque<Task> q;
	bool stop = false;
	std::thread th;

	void run()
	{
		for (;;) {
			Task t;
			{
				std::unique_lock<std::mutex> lk(mu);
				cv.wait(lk, [&]() { return stop || !q.empty(); });
				if (q.empty())
					return;
				t = std::move(q.front());
				q.pop_front();
			}
			if (t.launch) {
				std::unique_lock<std::mutex> lk(g_gate_mu);
				g_gate_cv.wait(lk, []() { return !g_gate_closed; });
			}
			t.fn();
		}
	}
	void push(std::function<void()> fn, bool launch)
	{
		std::lock_guard<std::mutex> g(mu);
		q.push_back({ std::move(fn), launch });
		cv.notify_one();
	}
};

struct hipstubEvent {
	std::mutex mu;
	std::condition_variable cv;
	uint64_t recorded = 0, completed = 0;
};

hipError_t hipGetDevice(int *dev)
{
	*dev = tl_device;
	return hipSuccess;
}

hipError_t hipSetDevice(int dev)
{
	hipError_t e = enter(hipstub::SET_DEVICE);
	if (e != hipSuccess)
		return e;
	tl_device = dev;
	return hipSuccess;
}

hipError_t hipGetLastError(void)
{
	return hipSuccess;
}

const char *hipGetErrorString(hipError_t e)
{
	return e == hipSuccess ? "no error" : "stand-in runtime error";
}

hipError_t hipHostMalloc(void **p, size_t bytes, unsigned)
{
	hipError_t e = enter(hipstub::HOST_MALLOC);
	return e != hipSuccess ? e : alloc(p, bytes, true, 0xCD);
}

hipError_t hipHostFree(void *p)
{
	return release(p, true);
}

hipError_t hipHostGetDevicePointer(void **dev, void *host, unsigned)
{
	hipError_t e = enter(hipstub::HOST_GET_DEVICE_POINTER);
	if (e != hipSuccess)
		return e;
	uintptr_t start;
	Alloc a;
	if (!find_alloc(host, 1, &start, &a) || !a.host)
		return hipErrorInvalidValue;
	*dev = host;
	return hipSuccess;
}

hipError_t hipMalloc(void **p, size_t bytes)
{
	hipError_t e = enter(hipstub::MALLOC);
	return e != hipSuccess ? e : alloc(p, bytes, false, 0xDD);
}

hipError_t hipFree(void *p)
{
	return release(p, false);
}

hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned)
{
	hipError_t e = enter(hipstub::STREAM_CREATE);
	if (e != hipSuccess)
		return e;
	hipstubStream *st = new hipstubStream;
	st->th = std::thread([st]() { st->run(); });
	*s = st;
	return hipSuccess;
}

hipError_t hipStreamDestroy(hipStream_t s)
{
	if (s == nullptr)
		return hipErrorInvalidValue;
	{
		std::lock_guard<std::mutex> g(s->mu);
		s->stop = true;
		s->cv.notify_one();
	}
	s->th.join();		/* after the queued work */
	delete s;
	return hipSuccess;
}

hipError_t hipStreamSynchronize(hipStream_t s)
{
	hipError_t e = enter(hipstub::STREAM_SYNCHRONIZE);
	if (e != hipSuccess)
		return e;
	if (s == nullptr)
		return hipErrorInvalidValue;
	struct Flag {
		std::mutex mu;
		std::condition_variable cv;
		bool set = false;
	};
	auto f = std::make_shared<Flag>();
	s->push([f]() {
		std::lock_guard<std::mutex> g(f->mu);
		f->set = true;
		f->cv.notify_all();
	}, false);
	std::unique_lock<std::mutex> lk(f->mu);
	f->cv.wait(lk, [&]() { return f->set; });
	return hipSuccess;
}

hipError_t hipEventCreateWithFlags(hipEvent_t *ev, unsigned)
{
	hipError_t e = enter(hipstub::EVENT_CREATE);
	if (e != hipSuccess)
		return e;
	*ev = new hipstubEvent;
	return hipSuccess;
}

hipError_t hipEventDestroy(hipEvent_t ev)
{
	delete ev;
	return hipSuccess;
}

hipError_t hipEventRecord(hipEvent_t ev, hipStream_t s)
{
	hipError_t e = enter(hipstub::EVENT_RECORD);
	if (e != hipSuccess)
		return e;
	if (ev == nullptr || s == nullptr)
		return hipErrorInvalidValue;
	uint64_t seq;
	{
		std::lock_guard<std::mutex> g(ev->mu);
		seq = ++ev->recorded;
	}
	s->push([ev, seq]() {
		std::lock_guard<std::mutex> g(ev->mu);
		ev->completed = std::max(ev->completed, seq);
		ev->cv.notify_all();
	}, false);
	return hipSuccess;
}

hipError_t hipEventSynchronize(hipEvent_t ev)
{
	hipError_t e = enter(hipstub::EVENT_SYNCHRONIZE);
	if (e != hipSuccess)
		return e;
	if (ev == nullptr)
		return hipErrorInvalidValue;
	std::unique_lock<std::mutex> lk(ev->mu);
	const uint64_t want = ev->recorded;
	ev->cv.wait(lk, [&]() { return ev->completed >= want; });
	return hipSuccess;
}

hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes,
    hipMemcpyKind, hipStream_t s)
{
	hipError_t e = enter(hipstub::MEMCPY_ASYNC);
	if (e != hipSuccess)
		return e;
	if (s == nullptr)
		return hipErrorInvalidValue;
	uintptr_t start;
	Alloc a;
	if (!find_alloc(dst, bytes, &start, &a) ||
	    !find_alloc(src, bytes, &start, &a))
		return hipErrorInvalidValue;
	s->push([dst, src, bytes]() { memcpy(dst, src, bytes); }, false);
	return hipSuccess;
}

/* ---- the stand-in net2_launch_jobs ---------------------------------------- */

namespace {

union St {
	uint32_t w32[8];
	uint64_t w64[8];
	uint8_t b[64];
};

void iv_of(int alg, St &st)
{
	oracle_sha2_ctx c;
	memset(&st, 0, sizeof(st));
	if (alg == 1) {
		oracle_sha256_init(&c);
		memcpy(st.w32, c.st.w32, 32);
	} else {
		if (alg == 2)
			oracle_sha384_init(&c);
		else
			oracle_sha512_init(&c);
		memcpy(st.w64, c.st.w64, 64);
	}
}

void violation(const char *what, uint32_t j)
{
	fprintf(stderr, "hipstub: net2_launch_jobs: job %u: %s\n", j, what);
	std::lock_guard<std::mutex> g(g_mu);
	g_violations++;
}

struct Range {
	uintptr_t lo, hi;
};

/* Every range of the launch inside the buffer its pointer belongs to,
 * 64-byte aligned, and no two of them overlapping. */
bool validate(const uint8_t *stage, const Net2Job *jobs, uint32_t n,
    const std::vector<Net2Job> &jd, const uint8_t *out, const uint32_t *done)
{
	uintptr_t s0, o0;
	Alloc sa, oa;
	bool ok = true;
	if (!find_alloc(stage, 1, &s0, &sa)) {
		violation("stage is in no allocation", 0);
		return false;
	}
	const uintptr_t s1 = s0 + sa.size;
	std::vector<Range> r;
	const uintptr_t jl = (uintptr_t)jobs, jh = jl + n * sizeof(Net2Job);
	if (jl < s0 || jh > s1 || jl % 8 != 0) {
		violation("the descriptors are outside the staging buffer", 0);
		ok = false;
	}
	r.push_back({ jl, jh });
	for (uint32_t j = 0; j < n; j++) {
		const Net2Job &d = jd[j];
		const unsigned alg = d.flags & 0xffu;
		if (alg < 1 || alg > 3 || (d.flags & ~(0xffu | NET2_JOB_STATE |
		    NET2_JOB_HMAC)) != 0 || ((d.flags & NET2_JOB_STATE) &&
		    (d.flags & NET2_JOB_HMAC))) {
			violation("bad flags", j);
			ok = false;
			continue;
		}
		const size_t blk = alg == 1 ? 64 : 128;
		const size_t auxlen = (d.flags & NET2_JOB_STATE) ?
		    (alg == 1 ? 32 : 64) : (d.flags & NET2_JOB_HMAC) ? blk : 0;
		const Range dr = { (uintptr_t)stage + d.data,
		    (uintptr_t)stage + d.data + (size_t)d.nblk * blk };
		const Range ar = { (uintptr_t)stage + d.aux,
		    (uintptr_t)stage + d.aux + auxlen };
		if (dr.lo < s0 || dr.hi > s1 || dr.hi < dr.lo) {
			violation("data outside the staging buffer", j);
			ok = false;
		}
		if (auxlen != 0 && (ar.lo < s0 || ar.hi > s1)) {
			violation("aux outside the staging buffer", j);
			ok = false;
		}
		if (dr.lo % 64 != 0 || (auxlen != 0 && ar.lo % 64 != 0)) {
			violation("a range is not 64-byte aligned", j);
			ok = false;
		}
		if (dr.hi > dr.lo)
			r.push_back(dr);
		if (auxlen != 0)
			r.push_back(ar);
	}
	std::sort(r.begin(), r.end(), [](const Range &a, const Range &b) {
		return a.lo < b.lo;
	});
	for (size_t i = 1; i < r.size(); i++)
		if (r[i].lo < r[i - 1].hi) {
			violation("two ranges of the launch overlap", (uint32_t)i);
			ok = false;
			break;
		}
	if (!find_alloc(out, 64 * (size_t)n, &o0, &oa) || !oa.host ||
	    (uintptr_t)out % 64 != 0) {
		violation("the result slots are outside their buffer", 0);
		ok = false;
	}
	if (!find_alloc(done, 4, &o0, &oa) || !oa.host) {
		violation("the counter is in no host allocation", 0);
		ok = false;
	}
	return ok;
}

void run_job(const uint8_t *stage, const Net2Job &d, uint8_t *slot,
    std::vector<uint8_t> &buf)
{
	const int alg = (int)(d.flags & 0xffu);
	const size_t blk = alg == 1 ? 64 : 128;
	const size_t dlen = alg == 1 ? 32 : alg == 2 ? 48 : 64;
	St st;
	if (d.flags & NET2_JOB_STATE) {
		memset(&st, 0, sizeof(st));
		memcpy(st.b, stage + d.aux, alg == 1 ? 32 : 64);
	} else {
		iv_of(alg, st);
	}
	const uint8_t *p = stage + d.data;
	uint64_t left = (uint64_t)d.nblk * blk;
	while (left != 0) {
		const size_t take = (size_t)std::min<uint64_t>(left, buf.size());
		memcpy(buf.data(), p, take);
		for (size_t o = 0; o < take; o += blk) {
			if (alg == 1)
				oracle_sha256_transform(st.w32, buf.data() + o);
			else
				oracle_sha512_transform(st.w64, buf.data() + o);
		}
		p += take;
		left -= take;
	}
	if (d.flags & NET2_JOB_HMAC) {
		/* outer hash: IV, K' ^ opad, inner digest || 0x80 || bit count */
		uint8_t kb[128], ob[128];
		memcpy(kb, stage + d.aux, blk);
		memset(ob, 0, sizeof(ob));
		for (size_t i = 0; i < dlen; i++)
			ob[i] = alg == 1 ?
			    (uint8_t)(st.w32[i / 4] >> (24 - 8 * (i % 4))) :
			    (uint8_t)(st.w64[i / 8] >> (56 - 8 * (i % 8)));
		ob[dlen] = 0x80;
		const uint64_t obits = (uint64_t)(blk + dlen) << 3;
		for (int i = 0; i < 8; i++)
			ob[blk - 1 - i] = (uint8_t)(obits >> (8 * i));
		iv_of(alg, st);
		if (alg == 1) {
			oracle_sha256_transform(st.w32, kb);
			oracle_sha256_transform(st.w32, ob);
		} else {
			oracle_sha512_transform(st.w64, kb);
			oracle_sha512_transform(st.w64, ob);
		}
	}
	memcpy(slot, st.b, alg == 1 ? 32 : 64);
}

void run_launch(const uint8_t *stage, const Net2Job *jobs, uint32_t n256,
    uint32_t n512, uint8_t *out, uint32_t *done, int wave)
{
	const uint32_t n = n256 + n512;
	std::vector<Net2Job> jd(n);
	uintptr_t s0;
	Alloc sa;
	/* the descriptors are read only once they are known to be readable */
	if (!find_alloc(jobs, n * sizeof(Net2Job), &s0, &sa)) {
		violation("the descriptors are in no allocation", 0);
		return;
	}
	memcpy(jd.data(), jobs, n * sizeof(Net2Job));
	const bool ok = validate(stage, jobs, n, jd, out, done);
	hipstub::LaunchRec rec;
	rec.wave = wave;
	rec.n256 = n256;
	rec.n512 = n512;
	rec.failed = false;
	for (uint32_t j = 0; j < n; j++) {
		uint64_t tag = 0;
		if (ok && jd[j].nblk != 0)
			memcpy(&tag, stage + jd[j].data, 8);
		rec.nblk.push_back(jd[j].nblk);
		rec.flags.push_back(jd[j].flags);
		rec.tag.push_back(tag);
	}
	{
		std::lock_guard<std::mutex> g(g_mu);
		g_log.push_back(std::move(rec));
	}
	if (!ok)
		return;		/* nothing runs: the caller sees a stalled counter */
	for (uint32_t j = 0; j < n; j++)
		if (((jd[j].flags & 0xffu) == 1) != (j < n256)) {
			violation("a job in the wrong family's run", j);
			return;
		}
	std::vector<uint8_t> buf(64 << 10);
	for (int fam = 0; fam < 2; fam++) {
		const uint32_t lo = fam == 0 ? 0 : n256, hi = fam == 0 ? n256 : n;
		for (uint32_t j = lo; j < hi; j++) {
			run_job(stage, jd[j], out + 64 * (size_t)j, buf);
			/* a wave counts itself in once its results are stored */
			if (wave || (j - lo) % 64 == 63 || j + 1 == hi)
				__atomic_fetch_add(done, 1u, __ATOMIC_RELEASE);
		}
	}
}

}	/* namespace */

hipError_t net2_launch_jobs(const uint8_t *stage, const Net2Job *jobs,
    uint32_t n256, uint32_t n512, uint8_t *out, uint32_t *done, int wave,
    hipStream_t s, uint32_t chunk)
{
	if (chunk == 0 || chunk % 128 != 0)
		return hipErrorInvalidValue;
	hipError_t e = enter(hipstub::LAUNCH);
	const hipError_t e2 = enter(wave ? hipstub::LAUNCH_WAVE :
	    hipstub::LAUNCH_LANE);
	if (e == hipSuccess)
		e = e2;
	if (e != hipSuccess) {
		hipstub::LaunchRec rec;
		rec.wave = wave;
		rec.n256 = n256;
		rec.n512 = n512;
		rec.failed = true;
		std::lock_guard<std::mutex> g(g_mu);
		g_log.push_back(std::move(rec));
		return e;
	}
	if (s == nullptr)
		return hipErrorInvalidValue;
	if (n256 + n512 == 0)
		return hipSuccess;
	{
		std::lock_guard<std::mutex> g(g_mu);
		g_jobs_queued += n256 + n512;
	}
	s->push([=]() { run_launch(stage, jobs, n256, n512, out, done, wave); },
	    true);
	return hipSuccess;
}

namespace hipstub {

void fail_at(Call c, unsigned k, hipError_t e)
{
	std::lock_guard<std::mutex> g(g_mu);
	g_hook[c].k = k;
	g_hook[c].e = e;
}

uint64_t calls(Call c)
{
	std::lock_guard<std::mutex> g(g_mu);
	return g_calls[c];
}

void gate(bool closed)
{
	std::lock_guard<std::mutex> g(g_gate_mu);
	g_gate_closed = closed;
	g_gate_cv.notify_all();
}

std::vector<LaunchRec> launch_log()
{
	std::lock_guard<std::mutex> g(g_mu);
	return g_log;
}

void clear_launch_log()
{
	std::lock_guard<std::mutex> g(g_mu);
	g_log.clear();
}

uint64_t jobs_queued()
{
	std::lock_guard<std::mutex> g(g_mu);
	return g_jobs_queued;
}

uint64_t violations()
{
	std::lock_guard<std::mutex> g(g_mu);
	return g_violations;
}

size_t host_bytes_live()
{
	std::lock_guard<std::mutex> g(g_mu);
	return g_host_live;
}

size_t host_alloc_max()
{
	std::lock_guard<std::mutex> g(g_mu);
	return g_host_max;
}

}	/* namespace hipstub */
