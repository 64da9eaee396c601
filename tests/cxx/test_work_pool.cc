/*
 * The library's host threads under ThreadSanitizer, off the GPU: WorkPool
 * and SliceWorker of ilias_net2_amd/csrc/net2_pool.h, which needs nothing
 * else of the project.  Results are plain (non-atomic) memory written by the
 * pool's threads and read by the caller after the call returns, so a missing
 * happens-before edge is a sanitizer report; a wrong count is a message and
 * exit status 1.  tests/test_work_pool.py builds and runs it.
 */
#include "net2_pool.h"

#include <stdio.h>
#include <stdlib.h>

#include <chrono>

namespace {

constexpr size_t kMaxNt = 16;
std::atomic<int> g_bad{0};

#define CHECK(cond, ...)                                                     \
	do {                                                                 \
		if (!(cond)) {                                               \
			fprintf(stderr, "test_work_pool: " __VA_ARGS__);     \
			fputc('\n', stderr);                                 \
			g_bad.fetch_add(1);                                  \
		}                                                            \
	} while (0)

void pause_us(unsigned us)
{
	if (us != 0)
		std::this_thread::sleep_for(std::chrono::microseconds(us));
}

/* Between jobs: none, inside the idle window (NET2_POOL_SPIN_IDLE_US),
 * between the two windows, past the long one (NET2_POOL_SPIN_US) -- workers
 * are met spinning after a job they ran, spinning after one they sat out,
 * and parked. */
const unsigned kPauses[] = { 0, NET2_POOL_SPIN_IDLE_US / 5, 0,
    NET2_POOL_SPIN_IDLE_US * 3, NET2_POOL_SPIN_IDLE_US / 2, 0,
    NET2_POOL_SPIN_US + 300 };
constexpr size_t kNumPauses = sizeof(kPauses) / sizeof(kPauses[0]);

/* One job of width nt: every index below nt exactly once, none at or above
 * it, and what the workers wrote is there when run() returns. */
void one_job(WorkPool &pool, size_t nt, unsigned tag)
{
	int hits[kMaxNt] = {};
	unsigned val[kMaxNt] = {};
	pool.run(nt, [&](size_t t) {
		if (t >= nt || t >= kMaxNt) {
			g_bad.fetch_add(1);
			return;
		}
		hits[t]++;
		val[t] = tag * 31 + (unsigned)t;
	});
	for (size_t t = 0; t < kMaxNt; t++) {
		CHECK(hits[t] == (t < nt ? 1 : 0), "job %u of width %zu: index %zu "
		    "ran %d times", tag, nt, t, hits[t]);
		CHECK(t >= nt || val[t] == tag * 31 + (unsigned)t, "job %u: value of "
		    "index %zu not seen by the caller", tag, t);
	}
}

void pool_caller(WorkPool &pool, unsigned who, unsigned jobs)
{
	for (unsigned j = 0; j < jobs; j++) {
		/* widths 1 .. 16 in an order of its own per caller: the inline
		 * path (1), growth while the other caller is active, and
		 * narrow jobs followed by wide ones */
		const size_t nt = 1 + (j * (who == 0 ? 7 : 11) + who * 5) % kMaxNt;
		one_job(pool, nt, j * 2 + who);
		pause_us(kPauses[(j + who * 3) % kNumPauses]);
	}
}

void test_work_pool(unsigned jobs)
{
	WorkPool &pool = *new WorkPool();	/* pools are never destroyed */
	/* a worker that sat out a job takes part in the next, whether it is
	 * met in its short spin, between the windows or parked */
	for (unsigned us : kPauses) {
		one_job(pool, kMaxNt, 1000);
		pause_us(us);
		one_job(pool, 2, 1001);
		pause_us(us);
		one_job(pool, kMaxNt, 1002);
	}
	std::thread a([&]() { pool_caller(pool, 0, jobs); });
	std::thread b([&]() { pool_caller(pool, 1, jobs); });
	a.join();
	b.join();
}

/* shard_batch's pattern: slice 0 on the caller, the others posted to their
 * devices' workers, a stack-held countdown they finish under its lock. */
void sharded_call(std::vector<SliceWorker *> &w, size_t first, size_t nd,
    unsigned tag)
{
	std::vector<unsigned> rcs(nd, 0);
	struct {
		std::mutex m;
		std::condition_variable cv;
		size_t left;
	} done;
	done.left = nd - 1;
	auto fn = [&](size_t d) { return tag * 17 + (unsigned)d + 1; };
	for (size_t d = 1; d < nd; d++) {
		w[(first + d) % w.size()]->post([&, d]() {
			rcs[d] = fn(d);
			std::lock_guard<std::mutex> g(done.m);
			if (--done.left == 0)
				done.cv.notify_all();
		});
	}
	rcs[0] = fn(0);
	{
		std::unique_lock<std::mutex> lk(done.m);
		done.cv.wait(lk, [&]() { return done.left == 0; });
	}
	for (size_t d = 0; d < nd; d++)
		CHECK(rcs[d] == fn(d), "sharded call %u: slice %zu of %zu gave %u",
		    tag, d, nd, rcs[d]);
}

/* Jobs one caller posts to one worker run in the order posted. */
void ordered_posts(SliceWorker &w, unsigned count)
{
	unsigned next = 0, out_of_order = 0;	/* the worker's until `last` */
	std::mutex m;
	std::condition_variable cv;
	bool last = false;
	for (unsigned k = 0; k < count; k++) {
		w.post([&, k]() {
			if (next != k)
				out_of_order++;
			next = k + 1;
			if (k + 1 == count) {
				std::lock_guard<std::mutex> g(m);
				last = true;
				cv.notify_all();
			}
		});
	}
	std::unique_lock<std::mutex> lk(m);
	cv.wait(lk, [&]() { return last; });
	CHECK(next == count && out_of_order == 0, "%u of %u posts ran, %u out of "
	    "order", next, count, out_of_order);
}

void test_slice_workers(unsigned callers, unsigned calls)
{
	std::vector<SliceWorker *> w;	/* never freed, as in the library */
	for (int i = 0; i < 4; i++)
		w.push_back(new SliceWorker());
	std::vector<std::thread> th;
	for (unsigned c = 0; c < callers; c++) {
		th.emplace_back([&, c]() {
			for (unsigned i = 0; i < calls; i++) {
				sharded_call(w, (c + i) % w.size(), 1 + (i + c) % 5,
				    c * calls + i);
				if (i % 100 == 0)
					ordered_posts(*w[c % w.size()], 64);
			}
		});
	}
	for (std::thread &t : th)
		t.join();
}

}	/* namespace */

int main(int argc, char **argv)
{
	const unsigned jobs = argc > 1 ? (unsigned)atoi(argv[1]) : 1500;
	const unsigned calls = argc > 2 ? (unsigned)atoi(argv[2]) : 500;
	test_work_pool(jobs);
	test_slice_workers(3, calls);
	if (g_bad.load() != 0) {
		fprintf(stderr, "test_work_pool: %d failures\n", g_bad.load());
		return 1;
	}
	printf("test_work_pool: ok (2 x %u pool jobs, 3 x %u sharded calls)\n",
	    jobs, calls);
	return 0;
}
