/*
 * ecdsa_kernels.hip -- batched ECDSA signature verification over secp521r1
 * (net2_ecdsa_p521_verify_dev, include/net2/ecdsa.h) for gfx950: one lane per
 * signature, each running ecdsa_p521_verify_one (ecdsa_p521.h) with OpenSSL's
 * accept/reject meaning.  Verification only -- signing needs secret nonces
 * and constant-time code and stays on the host.
 *
 * Shape.  Workgroups of one wave.  A lane's nine field registers
 * (p521_point.h) live in LDS, lane-strided: word `limb` of register `reg` of
 * lane l is at regs[(reg * 17 + limb) * 64 + l], so the 64 lanes of one
 * access hit 64 consecutive words (no bank conflicts) and the program's
 * register number, uniform across the wave, only moves the base.  That is
 * 9 * 17 * 64 * 4 = 39,168 bytes a workgroup: four workgroups, one wave per
 * SIMD, fit a CU's 160 KiB.  The work is a serial chain per lane with no
 * memory traffic to hide, so one wave per SIMD is all a SIMD can use.
 *
 * A wave takes the same time whatever its EXEC mask, so a batch too small to
 * fill every SIMD with full waves is spread: each workgroup takes `lpw`
 * signatures, lpw = ceil(n / SIMDs) up to 64, and the rest of its lanes idle
 * along on the batch's first signature without storing.
 *
 * A translation unit of its own, as aes_kernels.hip: the SHA-2 kernels'
 * object, and with it net2_sha2_build_id(), does not change.
 */
#include "ecdsa_launch.h"
#include "ecdsa_p521.h"

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace {

constexpr unsigned ECDSA_WG = 64;

/* The lane's view of the workgroup's register file. */
struct LdsRegs {
	uint32_t *w;		/* the workgroup's array + the lane */
	__device__ __forceinline__ uint32_t ld(int reg, int limb) const
	{
		return w[(reg * P521_LIMBS + limb) * ECDSA_WG];
	}
	__device__ __forceinline__ void st(int reg, int limb, uint32_t v)
	{
		w[(reg * P521_LIMBS + limb) * ECDSA_WG] = v;
	}
	__device__ __forceinline__ bool any(bool x) const
	{
		return __any(x) != 0;
	}
};

__global__ __launch_bounds__(ECDSA_WG) void ecdsa_p521_verify_kernel(
    const uint8_t *pub, size_t pub_stride, const uint8_t *rs, const uint8_t *dig,
    size_t dig_stride, const uint32_t *dlens, uint32_t dlen, uint32_t n,
    uint32_t lpw, uint8_t *valid)
{
	__shared__ uint32_t regs[P521_REGS * P521_LIMBS * ECDSA_WG];
	const uint32_t lane = threadIdx.x;
	const uint64_t item = (uint64_t)blockIdx.x * lpw + lane;
	const bool live = lane < lpw && item < n;
	const uint64_t i = live ? item : 0;	/* n > 0: item 0 exists */
	uint32_t len = dlens != nullptr ? dlens[i] : dlen;
	/* a digest longer than its slot would read its neighbour's */
	const bool len_ok = len <= dig_stride;
	if (!len_ok)
		len = 0;
	LdsRegs m = { regs + lane };
	const int ok = ecdsa_p521_verify_one(m, pub + i * pub_stride,
	    rs + i * ECDSA_P521_SIG_BYTES, dig + i * dig_stride, len);
	if (live)
		valid[item] = (uint8_t)(ok != 0 && len_ok);
}

/* SIMDs of the current device (4 a CU), looked up once per device. */
uint32_t simd_count()
{
	static uint32_t cached[64];
	int dev = 0, cus = 0;
	if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64)
		return 1024;
	uint32_t v = __atomic_load_n(&cached[dev], __ATOMIC_RELAXED);
	if (v == 0) {
		if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
		    dev) != hipSuccess || cus <= 0)
			cus = 256;
		v = 4u * (uint32_t)cus;
		__atomic_store_n(&cached[dev], v, __ATOMIC_RELAXED);
	}
	return v;
}

}	/* namespace */

hipError_t net2_launch_ecdsa_p521_verify(const uint8_t *d_pub, size_t pub_stride,
    const uint8_t *d_rs, const uint8_t *d_dig, size_t dig_stride,
    const uint32_t *d_dlens, uint32_t dlen, uint32_t n, uint8_t *d_valid,
    hipStream_t s)
{
	if (n == 0)
		return hipSuccess;
	const uint32_t simds = simd_count();
	uint32_t lpw = (uint32_t)(((uint64_t)n + simds - 1) / simds);
	if (lpw > ECDSA_WG)
		lpw = ECDSA_WG;
	const uint32_t grid = (uint32_t)(((uint64_t)n + lpw - 1) / lpw);
	ecdsa_p521_verify_kernel<<<dim3(grid), ECDSA_WG, 0, s>>>(d_pub, pub_stride,
	    d_rs, d_dig, dig_stride, d_dlens, dlen, n, lpw, d_valid);
	return hipGetLastError();
}
