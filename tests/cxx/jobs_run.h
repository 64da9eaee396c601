/*
 * jobs_run.h -- TEST INFRASTRUCTURE ONLY: runs the battery of jobs_battery.h
 * through net2_launch_jobs and the HIP runtime it is compiled against -- the
 * real one and the real kernels in tests/cxx/test_jobs_gpu.cc, the host-only
 * stand-ins of tests/cxx/hipstub in tests/cxx/test_coalesce_host.cc.
 *
 * Every case runs twice, in the coalescer's two staging modes: the image
 * copied to device memory on the launch's stream, and read through the
 * mapping of a coherent page-locked buffer.  Results and the completion
 * counter are always in mapped coherent host memory, as in the product,
 * and are read through the host mapping alone after the stream has been
 * synchronised: no copy back, no spin on the counter.
 */
#ifndef NET2_TESTS_JOBS_RUN_H
#define NET2_TESTS_JOBS_RUN_H

#include <hip/hip_runtime.h>

#include "jobs_battery.h"
#include "sha2_launch.h"

#include <stdio.h>
#include <string.h>

namespace jobsrun {

#define JOBSRUN_TRY(expr)                                                    \
	do {                                                                 \
		const hipError_t e_ = (expr);                                \
		if (e_ != hipSuccess) {                                      \
			fprintf(stderr, "%s: %s: %s failed: %s (%d)\n", who, \
			    c.name.c_str(), #expr, hipGetErrorString(e_),    \
			    (int)e_);                                        \
			return -1;                                           \
		}                                                            \
	} while (0)

/* One case in one staging mode; mismatches found, or -1 at the first HIP
 * error. */
inline int run_case(const char *who, const jobsbat::Case &c, bool mapped,
    hipStream_t s, uint32_t *h_done, uint32_t *d_done)
{
	const unsigned coherent = hipHostMallocMapped | hipHostMallocCoherent;
	const size_t slots = c.njobs + jobsbat::kSpareSlots;
	uint8_t *h_stage = nullptr, *d_stage = nullptr;
	uint8_t *h_out = nullptr, *d_out = nullptr;

	JOBSRUN_TRY(hipHostMalloc((void **)&h_out, 64 * slots, coherent));
	JOBSRUN_TRY(hipHostGetDevicePointer((void **)&d_out, h_out, 0));
	jobsbat::fill_canary(h_out, slots);
	JOBSRUN_TRY(hipHostMalloc((void **)&h_stage, c.stage.size(),
	    mapped ? coherent : (unsigned)hipHostMallocDefault));
	memcpy(h_stage, c.stage.data(), c.stage.size());
	if (mapped) {
		JOBSRUN_TRY(hipHostGetDevicePointer((void **)&d_stage, h_stage, 0));
	} else {
		JOBSRUN_TRY(hipMalloc((void **)&d_stage, c.stage.size()));
		JOBSRUN_TRY(hipMemcpyAsync(d_stage, h_stage, c.stage.size(),
		    hipMemcpyHostToDevice, s));
	}
	const uint32_t before = __atomic_load_n(h_done, __ATOMIC_ACQUIRE);
	const Net2Job *jobs =
	    reinterpret_cast<const Net2Job *>(d_stage + c.jobs_off);
	for (const jobsbat::Launch &l : c.launches)
		JOBSRUN_TRY(net2_launch_jobs(d_stage, jobs + l.first, l.n256,
		    l.n512, d_out + 64 * (size_t)l.first, d_done, l.wave, s,
		    l.chunk));
	JOBSRUN_TRY(hipStreamSynchronize(s));
	const uint32_t after = __atomic_load_n(h_done, __ATOMIC_ACQUIRE);
	const std::string who_mode = std::string(who) +
	    (mapped ? " (mapped staging)" : " (copied staging)");
	const int bad = jobsbat::check_case(who_mode.c_str(), c, h_out, before,
	    after);
	if (!mapped)
		JOBSRUN_TRY(hipFree(d_stage));
	JOBSRUN_TRY(hipHostFree(h_stage));
	JOBSRUN_TRY(hipHostFree(h_out));
	return bad;
}

/* The whole battery on one stream and one counter; mismatches found, or -1
 * at the first HIP error.  *njobs: jobs run. */
inline int run_battery(const char *who, size_t *njobs)
{
	const std::vector<jobsbat::Case> cases = jobsbat::build_cases();
	jobsbat::Case c;	/* (names the set-up calls in messages) */
	c.name = "set-up";
	hipStream_t s = nullptr;
	uint32_t *h_done = nullptr, *d_done = nullptr;
	int bad = 0;

	JOBSRUN_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
	JOBSRUN_TRY(hipHostMalloc((void **)&h_done, 64,
	    hipHostMallocMapped | hipHostMallocCoherent));
	JOBSRUN_TRY(hipHostGetDevicePointer((void **)&d_done, h_done, 0));
	__atomic_store_n(h_done, 0u, __ATOMIC_RELEASE);
	*njobs = 0;
	for (const jobsbat::Case &k : cases)
		for (int mapped = 0; mapped < 2; mapped++) {
			const int r = run_case(who, k, mapped != 0, s, h_done, d_done);
			if (r < 0)
				return -1;
			bad += r;
			*njobs += k.njobs;
		}
	JOBSRUN_TRY(hipStreamSynchronize(s));
	JOBSRUN_TRY(hipStreamDestroy(s));
	JOBSRUN_TRY(hipHostFree(h_done));
	return bad;
}

#undef JOBSRUN_TRY

}	/* namespace jobsrun */

#endif /* NET2_TESTS_JOBS_RUN_H */
