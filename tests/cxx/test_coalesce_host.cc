/*
 * The request coalescer (ilias_net2_amd/csrc/sha2_coalesce.cpp) and the
 * streaming contexts (csrc/sha2_stream.cpp), compiled unchanged against the
 * host-only runtime of tests/cxx/hipstub, as a CPU program for
 * ThreadSanitizer and AddressSanitizer + UBSan: the open slot, the leader,
 * `writers`, the futex on Job::done and the error path, with no GPU.
 * tests/test_coalesce_host.py builds it and runs one process per run and
 * setting (the coalescer reads its environment once):
 *
 *   battery  the stand-in net2_launch_jobs against tests/cxx/jobs_battery.h,
 *            the contract the real kernels are held to (test_jobs_gpu.cc)
 *   stress   32 threads x 300 mixed requests against the oracle
 *   sizes    requests up to 400 KB from many threads (a full batch, staging
 *            that grows) and a few of 17-20 MiB (staging past the retained
 *            size, given back by the next small batch)
 *   stream   SHA*Init / Update / Final from 8 threads, the context bytes
 *            against the oracle's after every call
 *   gate     40 requests arriving while a held launch keeps the device busy
 *   fail     every runtime call of a batch failed once: the callers' error,
 *            nobody hangs, the next requests on the slot succeed
 *
 * Exit status 1 and a message on a wrong result; a sanitizer report ends the
 * process (halt_on_error=1); a hang ends at the alarm below.
 */
#include <hip/hip_runtime.h>

#include "jobs_run.h"
#include "sha2_coalesce.h"

#include "../../include/net2/sha2.h"
#include "../../oracle/sha2_oracle.h"

#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <functional>
#include <map>
#include <string>
#include <thread>
#include <vector>

/* What net2_single.cpp does in the library: here always device 0. */
int net2_co_run(const net2co::Request &r)
{
	int err = 0;
	return net2co::submit(0, 0, r, &err);
}

namespace {

using hipstub::Call;

std::atomic<int> g_bad{0};

#define CHECK(cond, ...)                                                     \
	do {                                                                 \
		if (!(cond)) {                                               \
			if (g_bad.fetch_add(1) < 20) {                       \
				fprintf(stderr, "test_coalesce_host: "       \
				    __VA_ARGS__);                            \
				fputc('\n', stderr);                         \
			}                                                    \
		}                                                            \
	} while (0)

static_assert(sizeof(SHA2_CTX) == sizeof(oracle_sha2_ctx) &&
    sizeof(SHA2_CTX) == 208, "the oracle's context mirrors SHA2_CTX");

struct Rng {
	uint64_t s;
	explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 7) {}
	uint64_t next()
	{
		s ^= s << 13;
		s ^= s >> 7;
		s ^= s << 17;
		return s;
	}
	size_t below(size_t n) { return (size_t)(next() % n); }
	void fill(uint8_t *p, size_t n)
	{
		size_t i = 0;
		for (; i + 8 <= n; i += 8) {
			const uint64_t v = next();
			memcpy(p + i, &v, 8);
		}
		for (; i < n; i++)
			p[i] = (uint8_t)(next() >> 24);
	}
};

size_t block_of(int alg) { return alg == 1 ? 64 : 128; }
size_t dlen_of(int alg) { return alg == 1 ? 32 : alg == 2 ? 48 : 64; }

/*
 * One request through coalescer idx, checked against the oracle when it
 * succeeds: kind 0 digest, 1 HMAC, 2 whole blocks from a state; the message
 * of len bytes (rounded down to whole blocks for kind 2) in two segments;
 * tag != 0 becomes the message's first 8 bytes.  Returns submit()'s value.
 */
int one_request(size_t idx, int kind, int alg, size_t len, Rng &rng,
    uint64_t tag = 0)
{
	const size_t blk = block_of(alg), dl = dlen_of(alg);
	if (kind == net2co::BLOCKS)
		len = len / blk * blk;
	std::vector<uint8_t> m(len + 1);
	rng.fill(m.data(), len);
	if (tag != 0 && len >= 8)
		memcpy(m.data(), &tag, 8);
	const size_t cut = rng.below(len + 1);
	const struct iovec iov[2] = { { m.data(), cut }, { m.data() + cut,
	    len - cut } };
	alignas(8) uint8_t key[128], state[64], out[64], want[64];
	net2co::Request r = {};
	size_t outlen = dl;
	r.kind = kind;
	r.alg = alg;
	r.iov = iov;
	r.iovcnt = 2;
	r.out = out;
	memset(out, 0x5A, sizeof(out));
	if (kind == net2co::DIGEST) {
		oracle_sha2_digest(alg, m.data(), len, want);
	} else if (kind == net2co::HMAC) {
		const size_t kls[4] = { dl, blk, 0, 1 + rng.below(blk) };
		r.keylen = kls[rng.below(4)];
		rng.fill(key, sizeof(key));
		r.key = key;
		oracle_hmac_digest(alg + 3, key, r.keylen, m.data(), len, want);
	} else {
		outlen = alg == 1 ? 32 : 64;
		rng.fill(state, sizeof(state));
		r.state = state;
		memcpy(want, state, 64);
		for (size_t o = 0; o < len; o += blk) {
			if (alg == 1)
				oracle_sha256_transform(
				    reinterpret_cast<uint32_t *>(want), m.data() + o);
			else
				oracle_sha512_transform(
				    reinterpret_cast<uint64_t *>(want), m.data() + o);
		}
	}
	int herr = 0;
	const int rc = net2co::submit(idx, 0, r, &herr);
	if (rc == 0)
		CHECK(memcmp(out, want, outlen) == 0, "coalescer %zu: kind %d alg %d "
		    "len %zu: wrong result", idx, kind, alg, len);
	else
		CHECK(rc != EIO || herr != 0, "EIO without a HIP error code");
	return rc;
}

int random_request(size_t idx, Rng &rng, size_t maxlen)
{
	return one_request(idx, (int)rng.below(3), 1 + (int)rng.below(3),
	    rng.below(maxlen + 1), rng);
}

void run_threads(size_t nt, const std::function<void(size_t)> &fn)
{
	std::vector<std::thread> th;
	for (size_t t = 0; t < nt; t++)
		th.emplace_back(fn, t);
	for (std::thread &t : th)
		t.join();
}

/* Poll (1 ms steps, bounded) until cond holds; whether it did. */
bool wait_for(const std::function<bool()> &cond, int ms = 20000)
{
	for (int i = 0; i < ms; i++) {
		if (cond())
			return true;
		std::this_thread::sleep_for(std::chrono::milliseconds(1));
	}
	return cond();
}

void check_stats(size_t idx, uint64_t want_calls)
{
	uint64_t calls = 0, launches = 0;
	net2co::stats(idx, &calls, &launches);
	CHECK(calls == want_calls, "coalescer %zu served %llu requests, %llu were "
	    "made", idx, (unsigned long long)calls, (unsigned long long)want_calls);
	CHECK(launches >= 1 && launches <= calls, "coalescer %zu: %llu launches "
	    "for %llu requests", idx, (unsigned long long)launches,
	    (unsigned long long)calls);
	printf("test_coalesce_host: coalescer %zu: %llu requests in %llu "
	    "batches\n", idx, (unsigned long long)calls,
	    (unsigned long long)launches);
}

/* ---- battery ------------------------------------------------------------- */

void run_battery()
{
	size_t njobs = 0;
	const int bad = jobsrun::run_battery("test_coalesce_host (stand-in)",
	    &njobs);
	CHECK(bad == 0, "the stand-in net2_launch_jobs misses the kernels' "
	    "contract (%d)", bad);
	/* both staging modes of every launch of every case */
	size_t want = 0;
	for (const jobsbat::Case &c : jobsbat::build_cases())
		want += 2 * c.launches.size();
	CHECK(hipstub::launch_log().size() == want, "launch log: %zu records for "
	    "%zu launches", hipstub::launch_log().size(), want);
	CHECK(hipstub::host_bytes_live() == 0, "the runner leaked host memory");
	printf("test_coalesce_host: battery: %zu jobs\n", njobs);
}

/* ---- stress -------------------------------------------------------------- */

void run_stress()
{
	constexpr size_t NT = 32, NR = 300;
	run_threads(NT, [&](size_t t) {
		Rng rng(1000 + t);
		for (size_t i = 0; i < NR; i++) {
			const int rc = random_request(0, rng, 5000);
			CHECK(rc == 0, "thread %zu request %zu: error %d", t, i, rc);
		}
	});
	check_stats(0, NT * NR);
}

/* ---- sizes --------------------------------------------------------------- */

void run_sizes()
{
	constexpr size_t NT = 16, NR = 60;
	constexpr size_t kRetain = 16u << 20;	/* kRetainStage */
	/* a quarter of the threads up to 400 KB: batches fill the 1 MiB
	 * staging ("no room": join the next batch) and lone large requests
	 * grow it; one 17 MiB request among them */
	run_threads(NT + 1, [&](size_t t) {
		Rng rng(2000 + t);
		if (t == NT) {
			const int rc = one_request(0, net2co::DIGEST, 1,
			    (17u << 20) + 5, rng);
			CHECK(rc == 0, "17 MiB request: error %d", rc);
			return;
		}
		for (size_t i = 0; i < NR; i++) {
			const int rc = random_request(0, rng,
			    t % 4 == 0 ? 400000 : 5000);
			CHECK(rc == 0, "thread %zu request %zu: error %d", t, i, rc);
		}
	});
	CHECK(hipstub::host_alloc_max() > (17u << 20), "staging never grew to "
	    "hold the 17 MiB request (%zu)", hipstub::host_alloc_max());
	/* serial: free slots are taken last-in-first-out, so the small request
	 * after a large one runs on the same slot, whose staging -- larger than
	 * the retained 16 MiB -- it gives back */
	Rng rng(2999);
	const struct { int kind, alg; size_t len; } big[3] = {
		{ net2co::HMAC, 2, (18u << 20) + 77 },
		{ net2co::BLOCKS, 3, 19u << 20 },
		{ net2co::DIGEST, 3, (20u << 20) - 1 },
	};
	for (const auto &b : big) {
		const int rc = one_request(0, b.kind, b.alg, b.len, rng);
		CHECK(rc == 0, "%zu-byte request: error %d", b.len, rc);
		const size_t held = hipstub::host_bytes_live();
		CHECK(held > b.len, "a %zu-byte request with %zu bytes page-locked",
		    b.len, held);
		CHECK(random_request(0, rng, 3000) == 0, "small request failed");
		const size_t left = hipstub::host_bytes_live();
		CHECK(held > left && held - left > kRetain, "the small batch after a "
		    "%zu-byte request gave back %zu bytes of staging", b.len,
		    held - left);
	}
	check_stats(0, NT * NR + 1 + 3 * 2);
}

/* ---- streaming contexts -------------------------------------------------- */

typedef void (*init_fn)(SHA2_CTX *);
typedef void (*update_fn)(SHA2_CTX *, const uint8_t *, size_t);
typedef void (*pad_fn)(SHA2_CTX *);
typedef void (*final_fn)(uint8_t *, SHA2_CTX *);
typedef void (*oinit_fn)(oracle_sha2_ctx *);
typedef void (*oupdate_fn)(oracle_sha2_ctx *, const uint8_t *, size_t);
typedef void (*opad_fn)(oracle_sha2_ctx *);
typedef void (*ofinal_fn)(uint8_t *, oracle_sha2_ctx *);

struct Row {
	init_fn init;
	update_fn update;
	pad_fn pad;
	final_fn fin;
	oinit_fn oinit;
	oupdate_fn oupdate;
	opad_fn opad;
	ofinal_fn ofin;
};

const Row kRows[4] = {
	{},
	{ SHA256Init, SHA256Update, SHA256Pad, SHA256Final, oracle_sha256_init,
	    oracle_sha256_update, oracle_sha256_pad, oracle_sha256_final },
	{ SHA384Init, SHA384Update, SHA384Pad, SHA384Final, oracle_sha384_init,
	    oracle_sha384_update, oracle_sha384_pad, oracle_sha384_final },
	{ SHA512Init, SHA512Update, SHA512Pad, SHA512Final, oracle_sha512_init,
	    oracle_sha512_update, oracle_sha512_pad, oracle_sha512_final },
};

bool same_ctx(const SHA2_CTX &c, const oracle_sha2_ctx &oc)
{
	return memcmp(&c, &oc, sizeof(c)) == 0;
}

void run_stream()
{
	/* the lengths and the five random split points of
	 * test_streaming_matches_oracle_call_by_call */
	const size_t lens[] = { 0, 1, 55, 56, 63, 64, 65, 111, 112, 119, 120, 127,
	    128, 129, 1000, 4097 };
	run_threads(8, [&](size_t t) {
		Rng rng(3000 + t);
		for (int alg = 1; alg <= 3; alg++) {
			const Row &R = kRows[alg];
			const size_t dl = dlen_of(alg), B = block_of(alg);
			for (size_t n : lens) {
				std::vector<uint8_t> m(n + 1);
				rng.fill(m.data(), n);
				size_t cuts[7] = { 0, 0, 0, 0, 0, 0, n };
				for (int k = 1; k <= 5; k++)
					cuts[k] = rng.below(n + 1);
				std::sort(cuts, cuts + 7);
				SHA2_CTX c;
				oracle_sha2_ctx oc;
				memset(&c, 0x11, sizeof(c));
				memset(&oc, 0x11, sizeof(oc));
				R.init(&c);
				R.oinit(&oc);
				CHECK(same_ctx(c, oc), "alg %d: Init", alg);
				for (int k = 0; k < 6; k++) {
					R.update(&c, m.data() + cuts[k], cuts[k + 1] - cuts[k]);
					R.oupdate(&oc, m.data() + cuts[k],
					    cuts[k + 1] - cuts[k]);
					CHECK(same_ctx(c, oc), "alg %d len %zu: Update of "
					    "%zu bytes", alg, n, cuts[k + 1] - cuts[k]);
				}
				uint8_t d[64], od[64], want[64];
				R.fin(d, &c);
				R.ofin(od, &oc);
				oracle_sha2_digest(alg, m.data(), n, want);
				CHECK(memcmp(d, od, dl) == 0 && memcmp(d, want, dl) == 0,
				    "alg %d len %zu: Final", alg, n);
				CHECK(same_ctx(c, oc), "alg %d len %zu: context after "
				    "Final", alg, n);
				const uint8_t zero[208] = {};
				CHECK(memcmp(&c, zero, 208) == 0, "alg %d: Final leaves "
				    "the context", alg);
			}
			/* Pad alone, then Final(NULL): SHA-256 / SHA-512 keep the
			 * padded context, SHA-384 zeroes it */
			const size_t pl[] = { 3, B - 9, B - 8, B };
			for (size_t n : pl) {
				std::vector<uint8_t> m(n);
				rng.fill(m.data(), n);
				SHA2_CTX c;
				oracle_sha2_ctx oc;
				R.init(&c);
				R.oinit(&oc);
				R.update(&c, m.data(), n);
				R.oupdate(&oc, m.data(), n);
				R.pad(&c);
				R.opad(&oc);
				CHECK(same_ctx(c, oc), "alg %d len %zu: Pad", alg, n);
				R.fin(nullptr, &c);
				R.ofin(nullptr, &oc);
				CHECK(same_ctx(c, oc), "alg %d len %zu: Final(NULL)", alg,
				    n);
				const uint8_t zero[208] = {};
				CHECK((memcmp(&c, zero, 208) == 0) == (alg == 2),
				    "alg %d: Final(NULL) zeroes only SHA-384", alg);
			}
		}
	});
}

/* ---- gate closed --------------------------------------------------------- */

/* One launch as the coalescer orders it: SHA-256 jobs, then SHA-384/512,
 * longest first within each; in the automatic mode a lane-form launch holds
 * no job of 1,024 blocks (those took a wave each in a launch of their own). */
void check_order(const hipstub::LaunchRec &r, bool automode)
{
	const uint32_t n = r.n256 + r.n512;
	for (uint32_t j = 0; j < n; j++) {
		const unsigned alg = r.flags[j] & 0xffu;
		CHECK((alg == 1) == (j < r.n256), "job %u of a launch (%u,%u) is of "
		    "row %u", j, r.n256, r.n512, alg);
		if (j != 0 && j != r.n256)
			CHECK(r.nblk[j] <= r.nblk[j - 1], "job %u of a launch has %u "
			    "blocks behind one of %u", j, r.nblk[j], r.nblk[j - 1]);
		if (automode && !r.wave)
			CHECK(r.nblk[j] < 1024, "a job of %u blocks on a lane",
			    r.nblk[j]);
	}
}

void run_gate()
{
	constexpr size_t NR = 40;
	const char *jm = getenv("NET2_COALESCE_JOBMODE");
	const bool automode = jm == nullptr || atoi(jm) == 0;
	hipstub::gate(true);
	std::thread holder([]() {
		Rng rng(4000);
		const int rc = one_request(0, net2co::DIGEST, 3, 700, rng, 0xB0000001);
		CHECK(rc == 0, "the held request: error %d", rc);
	});
	CHECK(wait_for([]() { return hipstub::calls(Call::LAUNCH) >= 1; }),
	    "the first request never launched");
	/* the device is busy: 40 requests arrive, two of them long */
	std::atomic<size_t> returned{0};
	std::vector<std::thread> th;
	for (size_t i = 0; i < NR; i++)
		th.emplace_back([i, &returned]() {
			Rng rng(4100 + i);
			const int alg = 1 + (int)(i % 3);
			const size_t len = i == 7 ? 70000 : i == 20 ? 140000 :
			    8 + (i * 137) % 3000;
			const int rc = one_request(0, net2co::DIGEST, alg, len, rng,
			    0xA0000000 + i);
			CHECK(rc == 0, "request %zu behind the held launch: error %d",
			    i, rc);
			returned.fetch_add(1);
		});
	/* until every request has been launched (queued behind the gate) or
	 * waits for a free slot: nothing returns while the gate is closed */
	(void)wait_for([&]() {
		return hipstub::jobs_queued() >= NR + 1;
	}, 3000);
	CHECK(returned.load() == 0, "%zu requests returned while the device was "
	    "held", returned.load());
	hipstub::gate(false);
	holder.join();
	for (std::thread &t : th)
		t.join();
	check_stats(0, NR + 1);
	std::map<uint64_t, int> seen;
	size_t lane = 0;
	for (const hipstub::LaunchRec &r : hipstub::launch_log()) {
		CHECK(!r.failed, "a launch failed");
		check_order(r, automode);
		lane += !r.wave;
		for (uint64_t tag : r.tag)
			seen[tag]++;
	}
	CHECK(seen.size() == NR + 1, "%zu distinct requests launched, %zu made",
	    seen.size(), NR + 1);
	for (const auto &kv : seen)
		CHECK(kv.second == 1 && (kv.first >> 28) >= 0xA, "request %llx ran "
		    "in %d launches", (unsigned long long)kv.first, kv.second);
	printf("test_coalesce_host: gate: %zu launches, %zu in the lane form\n",
	    hipstub::launch_log().size(), lane);
}

/* ---- injected failures --------------------------------------------------- */

/* The next 100 requests on the slot(s) a failure touched all succeed: serial
 * ones reuse the slot freed last, then a few threads use every slot. */
void next_requests_succeed(size_t idx, const char *name, Rng &rng)
{
	for (int i = 0; i < 100; i++) {
		const int rc = random_request(idx, rng, 3000);
		CHECK(rc == 0, "%s: request %d after the failure: error %d", name, i,
		    rc);
		if (rc != 0)
			break;
	}
	run_threads(4, [&](size_t t) {
		Rng r2(5900 + 10 * idx + t);
		for (int i = 0; i < 25; i++) {
			const int rc = random_request(idx, r2, 3000);
			CHECK(rc == 0, "%s: threaded request after the failure: error "
			    "%d", name, rc);
		}
	});
}

/* A lone caller on coalescer idx (fresh unless warm > 0) meets the k-th
 * call of kind c failing with e. */
void fail_alone(size_t idx, const char *name, Call c, unsigned k,
    hipError_t e, int want_rc, int warm)
{
	Rng rng(5000 + idx);
	for (int i = 0; i < warm; i++)
		CHECK(random_request(idx, rng, 3000) == 0, "%s: warm-up", name);
	const uint64_t before = hipstub::calls(c);
	hipstub::fail_at(c, k, e);
	const int rc = random_request(idx, rng, 3000);
	hipstub::fail_at(c, 0, hipSuccess);
	CHECK(hipstub::calls(c) >= before + k, "%s: the call to fail was never "
	    "made", name);
	CHECK(rc == want_rc, "%s: the caller got %d, expected %d", name, rc,
	    want_rc);
	next_requests_succeed(idx, name, rng);
}

/* hipEventSynchronize is reached only once the host's poll has run out: the
 * launch is held at the gate until the failed call has been made (the error
 * path then waits for the stream). */
void fail_event_sync(size_t idx)
{
	const char *name = "hipEventSynchronize";
	Rng rng(5000 + idx);
	for (int i = 0; i < 3; i++)
		CHECK(random_request(idx, rng, 3000) == 0, "%s: warm-up", name);
	const uint64_t syncs = hipstub::calls(Call::STREAM_SYNCHRONIZE);
	hipstub::gate(true);
	hipstub::fail_at(Call::EVENT_SYNCHRONIZE, 1, hipErrorUnknown);
	int rc = -1;
	std::thread th([&]() {
		Rng r2(5500);
		rc = random_request(idx, r2, 3000);
	});
	CHECK(wait_for([&]() {
		return hipstub::calls(Call::STREAM_SYNCHRONIZE) > syncs;
	}), "%s: the error path never waited for the stream", name);
	hipstub::gate(false);
	th.join();
	hipstub::fail_at(Call::EVENT_SYNCHRONIZE, 0, hipSuccess);
	CHECK(rc == EIO, "%s: the caller got %d, expected EIO", name, rc);
	next_requests_succeed(idx, name, rng);
}

/*
 * A lane-form batch with a long job is two launches (the long job a wave of
 * its own, then the rest a lane each).  With two slots and a long window,
 * 21 requests that arrive while a held launch keeps the device busy form
 * one such batch; `which` fails its first (LAUNCH_WAVE) or second
 * (LAUNCH_LANE) launch.  After the second the counter has moved by the
 * first launch's wave: the next batch on the slot needs the resynchronised
 * base.
 */
void fail_pair(size_t idx, Call which)
{
	const char *name = which == Call::LAUNCH_WAVE ?
	    "first launch of a pair" : "second launch of a pair";
	constexpr size_t NR = 21;
	setenv("NET2_COALESCE_SLOTS", "2", 1);
	setenv("NET2_COALESCE_WINDOW_US", "100000", 1);
	Rng rng(5000 + idx);
	for (int i = 0; i < 3; i++)
		CHECK(random_request(idx, rng, 3000) == 0, "%s: warm-up", name);
	unsetenv("NET2_COALESCE_SLOTS");
	unsetenv("NET2_COALESCE_WINDOW_US");
	hipstub::clear_launch_log();
	const uint64_t l0 = hipstub::calls(Call::LAUNCH);
	hipstub::gate(true);
	int hrc = -1;
	std::thread holder([&]() {
		Rng r2(5600);
		hrc = one_request(idx, net2co::DIGEST, 1, 500, r2);
	});
	CHECK(wait_for([&]() { return hipstub::calls(Call::LAUNCH) > l0; }),
	    "%s: the held request never launched", name);
	const uint64_t w0 = hipstub::calls(which);
	hipstub::fail_at(which, 1, hipErrorUnknown);
	int rcs[NR];
	std::vector<std::thread> th;
	for (size_t i = 0; i < NR; i++)
		th.emplace_back([&, i]() {
			Rng r2(5700 + i);
			rcs[i] = one_request(idx, (int)(i % 2), 1 + (int)(i % 3),
			    i == 4 ? 200000 : 50 + 90 * i, r2);
		});
	CHECK(wait_for([&]() { return hipstub::calls(which) > w0; }),
	    "%s: the launch to fail was never made", name);
	hipstub::gate(false);
	holder.join();
	for (std::thread &t : th)
		t.join();
	hipstub::fail_at(which, 0, hipSuccess);
	CHECK(hrc == 0, "%s: the held request got %d", name, hrc);
	size_t nfail = 0;
	for (size_t i = 0; i < NR; i++) {
		CHECK(rcs[i] == 0 || rcs[i] == EIO, "%s: caller %zu got %d", name, i,
		    rcs[i]);
		nfail += rcs[i] != 0;
	}
	/* every caller of the batch, and the batch was all 21 (they had 100 ms
	 * to arrive): more than 16 jobs, so the lane form with its pair */
	CHECK(nfail == NR, "%s: %zu of %zu callers got the error", name, nfail,
	    (size_t)NR);
	bool wave_ran = false, found = false;
	for (const hipstub::LaunchRec &r : hipstub::launch_log()) {
		if (r.failed) {
			found = true;
			CHECK(r.wave == (which == Call::LAUNCH_WAVE), "%s: a launch of "
			    "the other form failed", name);
			CHECK(which == Call::LAUNCH_WAVE ? r.n256 + r.n512 == 1 :
			    r.n256 + r.n512 == NR - 1, "%s: the failed launch held "
			    "%u jobs", name, r.n256 + r.n512);
		} else if (r.wave && r.n256 + r.n512 == 1 && r.nblk[0] >= 1024) {
			wave_ran = true;
		}
	}
	CHECK(found, "%s: no failed launch in the log", name);
	CHECK(wave_ran == (which == Call::LAUNCH_LANE), "%s: the long job's "
	    "launch %s", name, wave_ran ? "ran" : "did not run");
	next_requests_succeed(idx, name, rng);
}

void run_fail()
{
	size_t idx = 0;
	const hipError_t oom = hipErrorOutOfMemory, bad = hipErrorUnknown;
	fail_alone(idx++, "hipStreamCreateWithFlags", Call::STREAM_CREATE, 1, bad,
	    EIO, 0);
	fail_alone(idx++, "hipEventCreateWithFlags", Call::EVENT_CREATE, 1, bad,
	    EIO, 0);
	fail_alone(idx++, "hipHostMalloc of the staging", Call::HOST_MALLOC, 1,
	    oom, ENOMEM, 0);
	fail_alone(idx++, "hipHostMalloc of the counter", Call::HOST_MALLOC, 2,
	    oom, ENOMEM, 0);
	fail_alone(idx++, "hipHostMalloc of the results", Call::HOST_MALLOC, 3,
	    oom, ENOMEM, 0);
	fail_alone(idx++, "hipHostGetDevicePointer of the staging",
	    Call::HOST_GET_DEVICE_POINTER, 1, bad, ENOMEM, 0);
	fail_alone(idx++, "hipHostGetDevicePointer of the results",
	    Call::HOST_GET_DEVICE_POINTER, 2, bad, EIO, 0);
	fail_alone(idx++, "hipHostGetDevicePointer of the counter",
	    Call::HOST_GET_DEVICE_POINTER, 3, bad, EIO, 0);
	fail_alone(idx++, "hipEventRecord", Call::EVENT_RECORD, 1, bad, EIO, 3);
	fail_alone(idx++, "a lone launch", Call::LAUNCH, 1, bad, EIO, 3);
	fail_event_sync(idx++);
	/* the copy mode: device staging and the H2D copy */
	setenv("NET2_COALESCE_ZEROCOPY", "0", 1);
	fail_alone(idx++, "hipMalloc of the staging", Call::MALLOC, 1, oom, ENOMEM,
	    0);
	fail_alone(idx++, "hipMemcpyAsync", Call::MEMCPY_ASYNC, 1, bad, EIO, 3);
	unsetenv("NET2_COALESCE_ZEROCOPY");
	fail_pair(idx++, Call::LAUNCH_WAVE);
	fail_pair(idx++, Call::LAUNCH_LANE);
}

}	/* namespace */

int main(int argc, char **argv)
{
	const std::string run = argc > 1 ? argv[1] : "";
	const auto t0 = std::chrono::steady_clock::now();
	alarm(280);		/* nobody hangs */
	if (run == "battery")
		run_battery();
	else if (run == "stress")
		run_stress();
	else if (run == "sizes")
		run_sizes();
	else if (run == "stream")
		run_stream();
	else if (run == "gate")
		run_gate();
	else if (run == "fail")
		run_fail();
	else {
		fprintf(stderr, "usage: test_coalesce_host battery | stress | sizes "
		    "| stream | gate | fail\n");
		return 2;
	}
	CHECK(hipstub::violations() == 0, "%llu launches broke the kernels' "
	    "contract", (unsigned long long)hipstub::violations());
	const double sec = std::chrono::duration<double>(
	    std::chrono::steady_clock::now() - t0).count();
	if (g_bad.load() != 0) {
		fprintf(stderr, "test_coalesce_host: %s: %d checks failed\n",
		    run.c_str(), g_bad.load());
		return 1;
	}
	printf("test_coalesce_host: %s: ok (%.2f s)\n", run.c_str(), sec);
	return 0;
}
