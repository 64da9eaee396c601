/*
 * net2_pool.h -- internal: the library's host threads, WorkPool (packing
 * staged chunks) and SliceWorker (a device's slice of a sharded call).  No
 * HIP header and nothing else of the project: tests/cxx/test_work_pool.cc
 * drives both under ThreadSanitizer on the CPU.
 */
#ifndef NET2_POOL_H
#define NET2_POOL_H

#include <pthread.h>
#include <stdint.h>
#include <time.h>

#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

/* Monotonic milliseconds: the spin windows, NET2_SHA2_DEBUG_TIMING prints. */
inline double dbg_now()
{
	struct timespec ts;
	clock_gettime(CLOCK_MONOTONIC, &ts);
	return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

/*
 * Host worker threads for packing staged chunks, kept alive between chunks
 * and calls: spawning and joining 16 threads twice per 64 MiB chunk cost
 * about a third of the pack itself.  run(nt, f) calls f(0) on the caller and
 * f(1..nt-1) on workers and returns when all are done.  Workers that took
 * part in a job spin for about half a millisecond after it, the others for
 * 50 us after seeing one (a chunk runs a small job and then a full-width
 * one back to back), then sleep on a condition variable: every worker
 * spinning half a millisecond after every job burnt ~6 CPUs during a 1
 * M-datagram host burst (tools/burst_debug_timing.py), none spinning after
 * a job it sat out cost the pageable host bursts 8-40 % (the full-width
 * pack waited for sleeping workers).  This way: ~34 ms of CPU per 1 M
 * datagrams against ~105, call times the same or better
 * (profiles/round6/spin_ab/).  The job word packs the
 * generation with nt, so a worker that wakes late never runs a job it is
 * not counted in.  Pools are never destroyed (their threads are detached
 * and may be parked at process exit).  One job at a time: job_, pending_
 * and word_ describe a single job, so run() is serialised by run_mu_ -- a
 * device's pool is shared by net2_sha2_batch and the host packet bursts,
 * which hold different locks and may run at once on one device.
 */
#ifndef NET2_POOL_SPIN_US
#define NET2_POOL_SPIN_US 500
#endif
#ifndef NET2_POOL_SPIN_IDLE_US
#define NET2_POOL_SPIN_IDLE_US 50
#endif

class WorkPool {
public:
	template <class F>
	void run(size_t nt, const F &f)
	{
		if (nt <= 1) {
			f((size_t)0);
			return;
		}
		std::lock_guard<std::mutex> one(run_mu_);
		grow(nt - 1);
		const std::function<void(size_t)> job = f;
		job_ = &job;
		pending_.store(nt - 1, std::memory_order_relaxed);
		{
			std::lock_guard<std::mutex> g(m_);
			word_.store(((word_.load(std::memory_order_relaxed) >> 8) + 1)
			    << 8 | nt, std::memory_order_release);
		}
		cv_.notify_all();
		f((size_t)0);
		while (pending_.load(std::memory_order_acquire) != 0)
			__builtin_ia32_pause();
	}

private:
	void grow(size_t want)
	{
		/* a new worker starts from the word before this job's bump */
		const uint64_t now = word_.load(std::memory_order_relaxed);
		while (nworkers_ < want) {
			const size_t idx = ++nworkers_;
			std::thread([this, idx, now]() { worker(idx, now); })
			    .detach();
		}
	}

	void worker(size_t idx, uint64_t seen)
	{
		/* named, so per-thread CPU time can be told apart
		 * (/proc/<pid>/task/<tid>/comm, tools/burst_debug_timing.py) */
		pthread_setname_np(pthread_self(), "net2-pack");
		bool ran = false;	/* took part in the last job */
		for (;;) {
			uint64_t w = seen;
			const double t0 = dbg_now();
			const double spin_ms = (ran ? NET2_POOL_SPIN_US :
			    NET2_POOL_SPIN_IDLE_US) * 1e-3;
			for (unsigned i = 1; w == seen; i++) {
				__builtin_ia32_pause();
				w = word_.load(std::memory_order_acquire);
				if ((i & 255) == 0 && dbg_now() - t0 > spin_ms)
					break;
			}
			if (w == seen) {
				std::unique_lock<std::mutex> lk(m_);
				cv_.wait(lk, [&]() {
					return word_.load(std::memory_order_acquire)
					    != seen;
				});
				w = word_.load(std::memory_order_acquire);
			}
			seen = w;
			ran = idx < (w & 0xff);
			if (ran) {
				(*job_)(idx);
				pending_.fetch_sub(1, std::memory_order_release);
			}
		}
	}

	std::atomic<uint64_t> word_{0};	/* generation << 8 | nt */
	std::atomic<size_t> pending_{0};
	const std::function<void(size_t)> *job_ = nullptr;
	size_t nworkers_ = 0;
	std::mutex run_mu_;	/* one run() at a time */
	std::mutex m_;
	std::condition_variable cv_;
};

/*
 * One persistent host thread per device index for the slices of a sharded
 * call (shard_batch): a thread created and joined per call cost ~30-60 us
 * per extra device on every net2_sha2_batch / host burst.  Jobs of
 * concurrent callers queue in order; a slice takes its device's lock anyway.
 * Workers are detached and live as long as the process.
 */
class SliceWorker {
public:
	void post(std::function<void()> f)
	{
		std::lock_guard<std::mutex> g(m_);
		if (!started_) {
			std::thread([this]() { loop(); }).detach();
			started_ = true;
		}
		q_.push_back(std::move(f));
		cv_.notify_one();
	}

private:
	void loop()
	{
		pthread_setname_np(pthread_self(), "net2-slice");
		for (;;) {
			std::function<void()> f;
			{
				std::unique_lock<std::mutex> lk(m_);
				cv_.wait(lk, [&]() { return !q_.empty(); });
				f = std::move(q_.front());
				q_.pop_front();
			}
			f();
		}
	}

	std::mutex m_;
	std::condition_variable cv_;
	std::deque<std::function<void()>> q_;
	bool started_ = false;
};

#endif /* NET2_POOL_H */
