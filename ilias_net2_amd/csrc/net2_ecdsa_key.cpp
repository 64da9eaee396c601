/*
 * net2_ecdsa_key.cpp -- the C ABI of the prepared ECDSA P-521 keys
 * (include/net2/ecdsa_key.h): argument checks and launches for device-resident
 * keytabs, and the host-memory object that owns one.  The tables are built
 * and used by ecdsa_key_kernels.hip; there is no CPU path.
 */
#include "net2_host.h"
#include "ecdsa_key_launch.h"

#include "../../include/net2/ecdsa.h"
#include "../../include/net2/ecdsa_key.h"

struct net2_ecdsa_p521_keys {
	int dev = -1;			/* the HIP device the keytab lives on */
	size_t nkeys = 0;
	uint32_t *d_keytab = nullptr;
};

namespace {

int check_keytab(const void *keytab, size_t nkeys)
{
	if (keytab == nullptr || nkeys == 0 ||
	    nkeys > NET2_ECDSA_P521_KEYTAB_MAX_KEYS || ((uintptr_t)keytab & 7) != 0)
		return EINVAL;
	return 0;
}

int check_batch(const uint8_t *rs, const uint8_t *dig, size_t dig_stride,
    const uint32_t *dlens, uint32_t dlen, size_t n, const uint8_t *valid)
{
	if (rs == nullptr || valid == nullptr || n > UINT32_MAX)
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

/* The calling thread's HIP device, put back when the call returns. */
struct Restore {
	int dev = -1;
	Restore() { (void)hipGetDevice(&dev); }
	~Restore() { if (dev >= 0) (void)hipSetDevice(dev); }
};

int keys_fill(net2_ecdsa_p521_keys *k, const uint8_t *pub, size_t pub_stride,
    uint8_t *ok)
{
	DevCopy d_pub, d_ok;
	HIP_TRY(hipMalloc((void **)&k->d_keytab,
	    net2_ecdsa_p521_keytab_bytes(k->nkeys)));
	if (int rc = d_pub.fill(pub,
	    (k->nkeys - 1) * pub_stride + NET2_ECDSA_P521_PUB_BYTES))
		return rc;
	if (ok != nullptr)
		HIP_TRY(hipMalloc((void **)&d_ok.d, k->nkeys));
	HIP_TRY(net2_launch_ecdsa_p521_keytab_build(d_pub.d, pub_stride,
	    (uint32_t)k->nkeys, k->d_keytab, d_ok.d, nullptr));
	if (ok != nullptr)
		HIP_TRY(hipMemcpy(ok, d_ok.d, k->nkeys, hipMemcpyDeviceToHost));
	HIP_TRY(hipStreamSynchronize(nullptr));
	return 0;
}

}	/* namespace */

NET2_EXPORT size_t net2_ecdsa_p521_keytab_bytes(size_t nkeys)
{
	if (nkeys == 0 || nkeys > NET2_ECDSA_P521_KEYTAB_MAX_KEYS)
		return 0;
	return (nkeys + 1) * (size_t)NET2_ECDSA_P521_KEYTAB_TABLE_BYTES;
}

NET2_EXPORT int net2_ecdsa_p521_keytab_prepare_dev(const uint8_t *d_pub,
    size_t pub_stride, size_t nkeys, void *d_keytab, uint8_t *d_ok,
    hipStream_t stream)
{
	if (int rc = check_keytab(d_keytab, nkeys))
		return rc;
	if (d_pub == nullptr || pub_stride < NET2_ECDSA_P521_PUB_BYTES)
		return EINVAL;
	if (int rc = check_current_device())
		return rc;
	HIP_TRY(net2_launch_ecdsa_p521_keytab_build(d_pub, pub_stride,
	    (uint32_t)nkeys, (uint32_t *)d_keytab, d_ok, stream));
	return 0;
}

NET2_EXPORT int net2_ecdsa_p521_verify_keytab_dev(const void *d_keytab,
    size_t nkeys, const uint32_t *d_kidx, const uint8_t *d_rs,
    const uint8_t *d_dig, size_t dig_stride, const uint32_t *d_dlens,
    uint32_t dlen, size_t n, uint8_t *d_valid, hipStream_t stream)
{
	if (n == 0)
		return 0;
	if (int rc = check_keytab(d_keytab, nkeys))
		return rc;
	if (int rc = check_batch(d_rs, d_dig, dig_stride, d_dlens, dlen, n, d_valid))
		return rc;
	if (int rc = check_current_device())
		return rc;
	HIP_TRY(net2_launch_ecdsa_p521_keytab_verify((const uint32_t *)d_keytab,
	    (uint32_t)nkeys, d_kidx, d_rs, d_dig, dig_stride, d_dlens, dlen,
	    (uint32_t)n, d_valid, stream));
	return 0;
}

NET2_EXPORT int net2_ecdsa_p521_keys_new(const uint8_t *pub, size_t pub_stride,
    size_t nkeys, struct net2_ecdsa_p521_keys **out, uint8_t *ok)
{
	if (out == nullptr)
		return EINVAL;
	*out = nullptr;
	if (pub == nullptr || nkeys == 0 ||
	    nkeys > NET2_ECDSA_P521_KEYTAB_MAX_KEYS ||
	    pub_stride < NET2_ECDSA_P521_PUB_BYTES)
		return EINVAL;
	const std::vector<int> dv = batch_devices();
	if (dv.empty())
		return ENODEV;
	Restore restore;
	std::unique_ptr<net2_ecdsa_p521_keys> k(new (std::nothrow) net2_ecdsa_p521_keys);
	if (!k)
		return ENOMEM;
	k->dev = dv[small_device(dv)];
	k->nkeys = nkeys;
	HIP_TRY(hipSetDevice(k->dev));
	const int rc = keys_fill(k.get(), pub, pub_stride, ok);
	if (rc != 0) {
		drop_dev(k->d_keytab);
		return rc;
	}
	*out = k.release();
	return 0;
}

NET2_EXPORT void net2_ecdsa_p521_keys_free(struct net2_ecdsa_p521_keys *keys)
{
	if (keys == nullptr)
		return;
	Restore restore;
	if (hipSetDevice(keys->dev) == hipSuccess)
		drop_dev(keys->d_keytab);
	delete keys;
}

NET2_EXPORT int net2_ecdsa_p521_verify_keys(
    const struct net2_ecdsa_p521_keys *keys, const uint32_t *kidx,
    const uint8_t *rs, const uint8_t *dig, size_t dig_stride,
    const uint32_t *dlens, uint32_t dlen, size_t n, uint8_t *valid)
{
	if (n == 0)
		return 0;
	if (keys == nullptr)
		return EINVAL;
	if (int rc = check_batch(rs, dig, dig_stride, dlens, dlen, n, valid))
		return rc;
	Restore restore;
	HIP_TRY(hipSetDevice(keys->dev));
	/* the strided digests as they lie, up to the end of the last record; a
	 * last digest longer than its slot is refused on the device, and not
	 * read here */
	const uint32_t last = dlens != nullptr ? dlens[n - 1] : dlen;
	const size_t dig_bytes = dig == nullptr ? 0 :
	    (n - 1) * dig_stride + std::min<size_t>(last, dig_stride);
	DevCopy d_kidx, d_rs, d_dig, d_dlens, d_valid;
	if (kidx != nullptr)
		if (int rc = d_kidx.fill(kidx, n * sizeof(uint32_t)))
			return rc;
	if (int rc = d_rs.fill(rs, n * NET2_ECDSA_P521_SIG_BYTES))
		return rc;
	if (int rc = d_dig.fill(dig, dig_bytes))
		return rc;
	if (dlens != nullptr)
		if (int rc = d_dlens.fill(dlens, n * sizeof(uint32_t)))
			return rc;
	HIP_TRY(hipMalloc((void **)&d_valid.d, n));
	/* an empty digest array still needs a pointer the kernel can offset */
	const uint8_t *dd = d_dig.d != nullptr ? d_dig.d : d_rs.d;
	HIP_TRY(net2_launch_ecdsa_p521_keytab_verify(keys->d_keytab,
	    (uint32_t)keys->nkeys, (const uint32_t *)d_kidx.d, d_rs.d,
	    dig == nullptr ? nullptr : dd, dig_stride, (const uint32_t *)d_dlens.d,
	    dlen, (uint32_t)n, d_valid.d, nullptr));
	HIP_TRY(hipMemcpy(valid, d_valid.d, n, hipMemcpyDeviceToHost));
	return 0;
}
