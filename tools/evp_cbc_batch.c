/*
 * evp_cbc_batch.c -- the CPU side of tools/aes_burst_rates.py: OpenSSL's
 * EVP AES-256-CBC (the calls of the reference's src/enc.c) over the payloads
 * of a datagram burst in host memory, on a given number of threads.  Each
 * payload is one EVP_Cipher{Init_ex,Update,Final_ex} sequence under its own
 * IV, PKCS#7 padding on, as net2_encctx_encbuf runs it -- except that a
 * thread fetches the cipher and expands the key once and re-initialises its
 * context with the IV alone per payload: OpenSSL 3 takes library-wide locks
 * when a cipher is fetched, and with a fetch per datagram 16 threads run
 * slower than one.  This is the CPU at its best.  Loaded through ctypes; a
 * measurement tool, not part of the library.
 */
#include <openssl/evp.h>
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>

struct job {
	int enc;
	const uint8_t *key, *iv, *in;
	uint8_t *out;
	const uint64_t *in_off, *out_off;
	const uint32_t *len;
	uint32_t *outlen;
	uint64_t lo, hi;
	uint64_t failed;
};

static void *
run(void *arg)
{
	struct job *j = arg;
	EVP_CIPHER_CTX *ctx = EVP_CIPHER_CTX_new();
	uint64_t i;

	if (ctx == NULL || EVP_CipherInit_ex(ctx, EVP_aes_256_cbc(), NULL, j->key,
	    NULL, j->enc) != 1) {
		EVP_CIPHER_CTX_free(ctx);
		j->failed = j->hi - j->lo;
		return NULL;
	}
	for (i = j->lo; i < j->hi; i++) {
		int n1 = 0, n2 = 0;
		uint8_t *o = j->out + j->out_off[i];

		if (EVP_CipherInit_ex(ctx, NULL, NULL, NULL, j->iv + 16 * i,
		    j->enc) != 1 ||
		    EVP_CipherUpdate(ctx, o, &n1, j->in + j->in_off[i],
		    (int)j->len[i]) != 1 ||
		    EVP_CipherFinal_ex(ctx, o + n1, &n2) != 1) {
			j->failed++;
			j->outlen[i] = 0;
			continue;
		}
		j->outlen[i] = (uint32_t)(n1 + n2);
	}
	EVP_CIPHER_CTX_free(ctx);
	return NULL;
}

/*
 * Payload i: len[i] bytes at in + in_off[i], its result to out + out_off[i]
 * (room for len[i] + 16 bytes when encrypting) and the result's length to
 * outlen[i]; iv: 16 bytes per payload.  Returns the number of payloads EVP
 * failed on, or -1.
 */
int64_t
evp_cbc_batch(int enc, const uint8_t *key, const uint8_t *iv,
    const uint8_t *in, const uint64_t *in_off, const uint32_t *len,
    uint8_t *out, const uint64_t *out_off, uint32_t *outlen, uint64_t n,
    int nthreads)
{
	pthread_t *th;
	struct job *jobs;
	int64_t failed = 0;
	int t, started = 0;

	if (nthreads < 1)
		nthreads = 1;
	th = calloc((size_t)nthreads, sizeof(*th));
	jobs = calloc((size_t)nthreads, sizeof(*jobs));
	if (th == NULL || jobs == NULL) {
		free(th);
		free(jobs);
		return -1;
	}
	for (t = 0; t < nthreads; t++) {
		struct job j = { enc, key, iv, in, out, in_off, out_off, len,
		    outlen, n * (uint64_t)t / (uint64_t)nthreads,
		    n * (uint64_t)(t + 1) / (uint64_t)nthreads, 0 };
		jobs[t] = j;
		if (pthread_create(&th[t], NULL, run, &jobs[t]) != 0)
			break;
		started++;
	}
	for (t = 0; t < started; t++) {
		pthread_join(th[t], NULL);
		failed += (int64_t)jobs[t].failed;
	}
	if (started != nthreads)
		failed = -1;
	free(th);
	free(jobs);
	return failed;
}
