/*
 * jobs_battery.h -- TEST INFRASTRUCTURE ONLY: hand-built batches for
 * net2_launch_jobs (sha2_launch.h), shared by tests/cxx/test_jobs_gpu.cc (the
 * real job_kernel / job_wave_kernel) and tests/cxx/test_coalesce_host.cc (the
 * host-only stand-in the coalescer runs on under the sanitizers), so both
 * are held to one contract.
 *
 * A case is a staging image laid out as sha2_coalesce.cpp lays a batch out
 * (every job 64-byte aligned, the message already padded, the K' ^ ipad
 * block in front for HMAC, the aux block -- K' ^ opad or a raw state --
 * behind, the descriptors after the last job), one or two launches over it,
 * and the 64-byte result slot expected for every job.  Expected values come
 * from the CPU oracle (oracle/sha2_oracle.h) twice over: its block
 * transforms run over the staged blocks (all eight raw state words, SHA-384
 * included), and, for digests and HMACs, its one-shot calls over the
 * original message, which must equal the digest-length prefix of those
 * words -- so a mistake in the battery's own padding cannot hide.
 *
 * Plain C++: no HIP call, no HIP type beyond what sha2_launch.h declares.
 */
#ifndef NET2_TESTS_JOBS_BATTERY_H
#define NET2_TESTS_JOBS_BATTERY_H

#include "sha2_launch.h"

#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

namespace jobsbat {

/* Result slots past the last job that a runner allocates and checks. */
constexpr size_t kSpareSlots = 8;

/* One net2_launch_jobs call of a case: jobs [first, first + n256 + n512),
 * results at out + 64 * first. */
struct Launch {
	uint32_t first, n256, n512;
	int wave;
	uint32_t chunk;
};

struct Case {
	std::string name;
	std::vector<uint8_t> stage;	/* the image, descriptors included */
	size_t jobs_off;		/* Net2Job[njobs] at stage + jobs_off */
	uint32_t njobs;
	std::vector<int> alg;		/* per job: 1 SHA-256, 2 SHA-384, 3 SHA-512 */
	std::vector<Launch> launches;	/* one stream, one counter, in order */
	std::vector<uint8_t> expect;	/* 64 * njobs: canary where no word goes */
	uint32_t waves;			/* what the launches add to *done */
};

/* What every launch adds to the counter: a wave per job in the wave form, a
 * wave per 64 jobs of each family in the lane form. */
uint32_t launch_waves(const Launch &l);

/* The canary byte of result byte i (of the whole out array). */
uint8_t canary(size_t i);
void fill_canary(uint8_t *out, size_t slots);

/* Every case of the battery; exits the process if the oracle's two ways to
 * an expected value disagree (a bug in the battery itself). */
std::vector<Case> build_cases();

/*
 * After the case's launches and a stream synchronisation: out (njobs +
 * kSpareSlots slots, canary-filled before) against the expected slots --
 * which covers bytes 32-63 of every SHA-256 slot -- the spare slots still
 * canary, and the counter advanced by exactly c.waves.  Prints every
 * mismatch to stderr under `who`; returns their number.
 */
int check_case(const char *who, const Case &c, const uint8_t *out,
    uint32_t done_before, uint32_t done_after);

}	/* namespace jobsbat */

#endif /* NET2_TESTS_JOBS_BATTERY_H */
