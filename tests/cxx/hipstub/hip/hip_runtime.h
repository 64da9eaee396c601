/*
 * hip/hip_runtime.h -- TEST INFRASTRUCTURE ONLY: a host-only stand-in for the
 * part of the HIP runtime that csrc/sha2_coalesce.cpp and csrc/sha2_launch.h
 * use, so the coalescer compiles unchanged into a CPU program that runs
 * under ThreadSanitizer and AddressSanitizer (tests/test_coalesce_host.py).
 * Put tests/cxx/hipstub first on the include path; hip_stub.cc implements
 * it, together with a stand-in net2_launch_jobs.
 *
 * Streams are worker threads with a FIFO, events mark a position in a
 * stream, every allocation is recorded with its start and size, "device"
 * memory is host memory, and hipHostGetDevicePointer is the identity.
 */
#ifndef NET2_TESTS_HIPSTUB_HIP_RUNTIME_H
#define NET2_TESTS_HIPSTUB_HIP_RUNTIME_H

#include <stddef.h>
#include <stdint.h>

#include <vector>

typedef enum hipError_t {
	hipSuccess = 0,
	hipErrorInvalidValue = 1,
	hipErrorOutOfMemory = 2,
	hipErrorLaunchFailure = 719,
	hipErrorUnknown = 999,
} hipError_t;

typedef struct hipstubStream *hipStream_t;
typedef struct hipstubEvent *hipEvent_t;

enum { hipHostMallocDefault = 0, hipHostMallocMapped = 2, hipHostMallocCoherent = 0x40000000 };
enum { hipStreamNonBlocking = 1 };
enum { hipEventDisableTiming = 2 };
typedef enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 } hipMemcpyKind;

hipError_t hipGetDevice(int *dev);
hipError_t hipSetDevice(int dev);
hipError_t hipGetLastError(void);
const char *hipGetErrorString(hipError_t e);
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned flags);
hipError_t hipHostFree(void *p);
hipError_t hipHostGetDevicePointer(void **dev, void *host, unsigned flags);
hipError_t hipMalloc(void **p, size_t bytes);
hipError_t hipFree(void *p);
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned flags);
hipError_t hipStreamDestroy(hipStream_t s);
hipError_t hipStreamSynchronize(hipStream_t s);
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned flags);
hipError_t hipEventDestroy(hipEvent_t e);
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s);
hipError_t hipEventSynchronize(hipEvent_t e);
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes,
    hipMemcpyKind kind, hipStream_t s);

/* What a test driver sees of the stand-in. */
namespace hipstub {

enum Call {
	SET_DEVICE, HOST_MALLOC, HOST_GET_DEVICE_POINTER, MALLOC, STREAM_CREATE,
	STREAM_SYNCHRONIZE, EVENT_CREATE, EVENT_RECORD, EVENT_SYNCHRONIZE,
	MEMCPY_ASYNC,
	LAUNCH,		/* any net2_launch_jobs */
	LAUNCH_WAVE,	/* ... in the wave form */
	LAUNCH_LANE,	/* ... in the lane form */
	NUM_CALLS
};

/* The k-th call of this kind from now on (k >= 1) fails with e and does
 * nothing else; k == 0 clears the hook. */
void fail_at(Call c, unsigned k, hipError_t e);
/* Calls of this kind made so far, failed ones included. */
uint64_t calls(Call c);

/* While closed, a stream's worker holds every queued launch (and what is
 * queued behind it): the device is "busy". */
void gate(bool closed);

/* One net2_launch_jobs as the stand-in saw it. */
struct LaunchRec {
	int wave;
	uint32_t n256, n512;
	bool failed;			/* by fail_at: nothing ran */
	std::vector<uint32_t> nblk;	/* per job */
	std::vector<uint32_t> flags;
	std::vector<uint64_t> tag;	/* the job's first 8 data bytes (0: none) */
};
/* Launches in the order their stream ran them (failed ones: when called). */
std::vector<LaunchRec> launch_log();
void clear_launch_log();

/* Jobs of all launches accepted so far, queued ones included. */
uint64_t jobs_queued();

/* Contract violations the stand-in found in launches (a range outside its
 * allocation, unaligned, or overlapping another of the launch), each
 * printed to stderr when found. */
uint64_t violations();

/* Page-locked host memory now allocated, and the largest single
 * hipHostMalloc so far. */
size_t host_bytes_live();
size_t host_alloc_max();

}	/* namespace hipstub */

#endif /* NET2_TESTS_HIPSTUB_HIP_RUNTIME_H */
