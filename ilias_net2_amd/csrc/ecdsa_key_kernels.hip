/*
 * ecdsa_key_kernels.hip -- prepared keys for the batched ECDSA P-521
 * verification (include/net2/ecdsa_key.h) for gfx950: the kernel that builds
 * a keytab's tables and the kernel that verifies from them, both running
 * p521_keytab.h.
 *
 * Shape, both kernels: that of ecdsa_kernels.hip.  Workgroups of one wave; a
 * lane's nine field registers live in LDS, lane-strided (word `limb` of
 * register `reg` of lane l at regs[(reg * 17 + limb) * 64 + l]), 39,168 bytes
 * a workgroup, four workgroups a CU, one wave per SIMD.
 *
 * ecdsa_p521_keytab_verify_kernel: one lane per signature, and a batch too
 * small to fill every SIMD with full waves is spread as the bit-by-bit
 * kernel spreads it (`lpw` signatures a workgroup).  A lane's table reads
 * are gathers of one 136-byte entry per addition.
 *
 * ecdsa_p521_keytab_build_kernel: one lane per (table, window), the 131
 * windows of a table on consecutive lanes and the tables back to back, so
 * nkeys keys are (nkeys + 1) * 131 / 64 waves.  A wave lasts as long as its
 * highest window's 4j doublings and two field inversions.
 *
 * A translation unit of its own, as ecdsa_kernels.hip: no existing kernel
 * object changes, nor net2_sha2_build_id().
 */
#include "ecdsa_key_launch.h"
#include "p521_keytab.h"

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

__global__ __launch_bounds__(ECDSA_WG) void ecdsa_p521_keytab_build_kernel(
    const uint8_t *pub, size_t pub_stride, uint32_t nkeys, uint32_t *keytab,
    uint8_t *ok)
{
	__shared__ uint32_t regs[P521_REGS * P521_LIMBS * ECDSA_WG];
	const uint32_t lane = threadIdx.x;
	const uint64_t slot = (uint64_t)blockIdx.x * ECDSA_WG + lane;
	const bool live = slot < ((uint64_t)nkeys + 1) * P521_KT_WINDOWS;
	/* an idle lane computes along on G's window 0 and stores nothing */
	const uint64_t at = live ? slot : 0;
	const uint64_t t = at / P521_KT_WINDOWS;
	const int j = (int)(at % P521_KT_WINDOWS);
	LdsRegs m = { regs + lane };
	const bool valid = p521_keytab_build_one(m,
	    t == 0 ? nullptr : pub + (t - 1) * pub_stride, j,
	    keytab + t * P521_KT_TABLE_WORDS, live);
	if (live && j == 0 && t != 0 && ok != nullptr)
		ok[t - 1] = (uint8_t)valid;
}

__global__ __launch_bounds__(ECDSA_WG) void ecdsa_p521_keytab_verify_kernel(
    const uint32_t *keytab, uint32_t nkeys, const uint32_t *kidx,
    const uint8_t *rs, const uint8_t *dig, size_t dig_stride,
    const uint32_t *dlens, uint32_t dlen, uint32_t n, uint32_t lpw,
    uint8_t *valid)
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
	const int ok = ecdsa_p521_keytab_verify_one(m, keytab, nkeys,
	    kidx != nullptr ? kidx[i] : 0u, rs + i * ECDSA_P521_SIG_BYTES,
	    dig + i * dig_stride, len);
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

hipError_t net2_launch_ecdsa_p521_keytab_build(const uint8_t *d_pub,
    size_t pub_stride, uint32_t nkeys, uint32_t *d_keytab, uint8_t *d_ok,
    hipStream_t s)
{
	const uint64_t lanes = ((uint64_t)nkeys + 1) * P521_KT_WINDOWS;
	const uint32_t grid = (uint32_t)((lanes + ECDSA_WG - 1) / ECDSA_WG);
	ecdsa_p521_keytab_build_kernel<<<dim3(grid), ECDSA_WG, 0, s>>>(d_pub,
	    pub_stride, nkeys, d_keytab, d_ok);
	return hipGetLastError();
}

hipError_t net2_launch_ecdsa_p521_keytab_verify(const uint32_t *d_keytab,
    uint32_t nkeys, const uint32_t *d_kidx, const uint8_t *d_rs,
    const uint8_t *d_dig, size_t dig_stride, const uint32_t *d_dlens,
    uint32_t dlen, uint32_t n, uint8_t *d_valid, hipStream_t s)
{
	if (n == 0)
		return hipSuccess;
	const uint32_t simds = simd_count();
	uint32_t lpw = (uint32_t)(((uint64_t)n + simds - 1) / simds);
	if (lpw > ECDSA_WG)
		lpw = ECDSA_WG;
	const uint32_t grid = (uint32_t)(((uint64_t)n + lpw - 1) / lpw);
	ecdsa_p521_keytab_verify_kernel<<<dim3(grid), ECDSA_WG, 0, s>>>(d_keytab,
	    nkeys, d_kidx, d_rs, d_dig, dig_stride, d_dlens, dlen, n, lpw, d_valid);
	return hipGetLastError();
}
