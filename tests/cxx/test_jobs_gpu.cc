/*
 * The coalescer's two job kernels (job_kernel, job_wave_kernel of
 * ilias_net2_amd/csrc/sha2_kernels.hip) on hand-built batches: the battery
 * of jobs_battery.h straight through net2_launch_jobs, with no coalescer and
 * no thread timing in between, so the shape of every launch is the test's
 * choice.  Linked against the library's own kernel object; results, canaries
 * and the completion counter are checked after every case (jobs_run.h).
 * tests/test_gpu_jobs.py runs it; it exits non-zero at the first HIP error
 * or after any mismatch.
 */
#include "jobs_run.h"

#include <chrono>

int main()
{
	const auto t0 = std::chrono::steady_clock::now();
	size_t njobs = 0;
	const int bad = jobsrun::run_battery("test_jobs_gpu", &njobs);
	const double sec = std::chrono::duration<double>(
	    std::chrono::steady_clock::now() - t0).count();
	if (bad != 0) {
		fprintf(stderr, "test_jobs_gpu: %s\n", bad < 0 ? "HIP error" :
		    "results differ from the oracle's");
		return 1;
	}
	printf("test_jobs_gpu: %zu jobs in %.2f s\n", njobs, sec);
	printf("test_jobs_gpu: ok\n");
	return 0;
}
