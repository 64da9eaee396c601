/*
 * net2_ecdsa.cpp -- the C ABI of the batched ECDSA P-521 verification
 * (include/net2/ecdsa.h): argument checks and the launch for device-resident
 * batches, and the synchronous form from host memory around it.  The
 * verification itself is ecdsa_kernels.hip's; there is no CPU path.
 */
#include "net2_host.h"
#include "ecdsa_launch.h"

#include "../../include/net2/ecdsa.h"

namespace {

int check_args(const uint8_t *pub, size_t pub_stride, const uint8_t *rs,
    const uint8_t *dig, size_t dig_stride, const uint32_t *dlens, uint32_t dlen,
    size_t n, const uint8_t *valid)
{
	if (pub == nullptr || rs == nullptr || valid == nullptr || n > UINT32_MAX)
		return EINVAL;
	if (pub_stride != 0 && pub_stride < NET2_ECDSA_P521_PUB_BYTES)
		return EINVAL;
	if (dig == nullptr && (dlens != nullptr || dlen != 0))
		return EINVAL;
	if (dlens == nullptr && dig_stride < dlen)
		return EINVAL;
	return 0;
}

/* A device copy of host bytes, freed with the object. */
struct DevCopy {
	uint8_t *d = nullptr;
	~DevCopy() { drop_dev(d); }
	int fill(const void *src, size_t bytes)
	{
		if (bytes == 0)
			return 0;
		HIP_TRY(hipMalloc((void **)&d, bytes));
		HIP_TRY(hipMemcpy(d, src, bytes, hipMemcpyHostToDevice));
		return 0;
	}
};

}	/* namespace */

NET2_EXPORT int net2_ecdsa_p521_verify_dev(const uint8_t *d_pub, size_t pub_stride,
    const uint8_t *d_rs, const uint8_t *d_dig, size_t dig_stride,
    const uint32_t *d_dlens, uint32_t dlen, size_t n, uint8_t *d_valid,
    hipStream_t stream)
{
	if (n == 0)
		return 0;
	if (int rc = check_args(d_pub, pub_stride, d_rs, d_dig, dig_stride, d_dlens,
	    dlen, n, d_valid))
		return rc;
	if (int rc = check_current_device())
		return rc;
	HIP_TRY(net2_launch_ecdsa_p521_verify(d_pub, pub_stride, d_rs, d_dig,
	    dig_stride, d_dlens, dlen, (uint32_t)n, d_valid, stream));
	return 0;
}

NET2_EXPORT int net2_ecdsa_p521_verify(const uint8_t *pub, size_t pub_stride,
    const uint8_t *rs, const uint8_t *dig, size_t dig_stride,
    const uint32_t *dlens, uint32_t dlen, size_t n, uint8_t *valid)
{
	if (n == 0)
		return 0;
	if (int rc = check_args(pub, pub_stride, rs, dig, dig_stride, dlens, dlen, n,
	    valid))
		return rc;
	const std::vector<int> dv = batch_devices();
	if (dv.empty())
		return ENODEV;
	int prev = -1;
	(void)hipGetDevice(&prev);
	struct Restore {
		int dev;
		~Restore() { if (dev >= 0) (void)hipSetDevice(dev); }
	} restore = { prev };
	HIP_TRY(hipSetDevice(dv[small_device(dv)]));
	/* the strided arrays as they lie, up to the end of the last record; a
	 * last digest longer than its slot is refused on the device, and not
	 * read here */
	const uint32_t last = dlens != nullptr ? dlens[n - 1] : dlen;
	const size_t dig_bytes = dig == nullptr ? 0 :
	    (n - 1) * dig_stride + std::min<size_t>(last, dig_stride);
	DevCopy d_pub, d_rs, d_dig, d_dlens, d_valid;
	if (int rc = d_pub.fill(pub, (n - 1) * pub_stride + NET2_ECDSA_P521_PUB_BYTES))
		return rc;
	if (int rc = d_rs.fill(rs, n * NET2_ECDSA_P521_SIG_BYTES))
		return rc;
	if (int rc = d_dig.fill(dig, dig_bytes))
		return rc;
	if (dlens != nullptr)
		if (int rc = d_dlens.fill(dlens, n * sizeof(uint32_t)))
			return rc;
	HIP_TRY(hipMalloc((void **)&d_valid.d, n));
	/* an empty digest array still needs a pointer the checks accept */
	const uint8_t *dd = d_dig.d != nullptr ? d_dig.d : d_rs.d;
	HIP_TRY(net2_launch_ecdsa_p521_verify(d_pub.d, pub_stride, d_rs.d,
	    dig == nullptr ? nullptr : dd, dig_stride, (const uint32_t *)d_dlens.d, dlen,
	    (uint32_t)n, d_valid.d, nullptr));
	HIP_TRY(hipMemcpy(valid, d_valid.d, n, hipMemcpyDeviceToHost));
	return 0;
}
