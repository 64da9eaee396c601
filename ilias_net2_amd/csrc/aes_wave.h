/*
 * aes_wave.h -- the pass and block schedule of the wave form of the burst
 * cipher's RX decrypt (aes_cbc_decrypt_wave_kernel, aes_kernels.hip): one
 * wave of 64 lanes per datagram, the lanes taking the datagram's blocks 64 to
 * a pass.  CBC decryption has no serial chain: plaintext block b is
 * D(c[b]) ^ c[b - 1], with the IV standing in for c[-1].
 *
 * The schedule, for a ciphertext of nb >= 1 blocks:
 *
 *   - pass p covers blocks 64 p .. 64 p + 63; lane l takes block 64 p + l and
 *     sits idle when that is >= nb.  There are ceil(nb / 64) passes.
 *   - the passes run from the last to the first: run r (r = 0 runs first) is
 *     pass ceil(nb / 64) - 1 - r.
 *   - a lane loads its own block and its `prev` -- block b - 1 wherever in
 *     the datagram that lies (for lane 0 of pass p > 0 it is block 64 p - 1,
 *     which belongs to pass p - 1), the datagram's IV for block 0 -- then
 *     decrypts, then stores.  Within a run every lane's loads come before any
 *     lane's stores (the wave executes in lockstep, and a lane's store data
 *     depends on both of its loads).
 *   - the padding verdict is taken in run 0, which holds the last block, by
 *     lane (nb - 1) mod 64, after that run's blocks are decrypted and before
 *     the first store of the whole datagram; it is made known to all lanes.
 *     A failed verdict ends the datagram with nothing written.
 *
 * In place (output over the ciphertext) this order needs no staging: a run
 * reads blocks 64 p - 1 .. 64 p + 63 only, and every store made before it
 * belongs to a later pass, so went to blocks >= 64 (p + 1).  What a run
 * reads no earlier run has written, and within the run the loads are done
 * before the stores begin.
 *
 * No HIP header, plain C++14: the kernel includes it, and so does the host
 * model of a wave (tests/cxx/test_aes_wave_host.cc).  constexpr functions are
 * host and device code alike.
 */
#ifndef NET2_AES_WAVE_H
#define NET2_AES_WAVE_H

#include <stdint.h>

#define NET2_AES_WAVE_LANES 64u

/* The run in which the padding verdict is taken (the last block's pass). */
#define NET2_AES_WAVE_VERDICT_RUN 0u

/* Passes of a ciphertext of nb blocks. */
constexpr uint32_t aes_wave_passes(uint32_t nb)
{
	return nb / NET2_AES_WAVE_LANES + (nb % NET2_AES_WAVE_LANES != 0 ? 1u : 0u);
}

/* The pass that run r executes, r < aes_wave_passes(nb): last pass first. */
constexpr uint32_t aes_wave_pass_of_run(uint32_t nb, uint32_t r)
{
	return aes_wave_passes(nb) - 1u - r;
}

/* The block lane l takes in pass p; the lane is idle when it is >= nb.
 * (nb < 2^28, so no wrap-around: a ciphertext's length fits 32 bits.) */
constexpr uint32_t aes_wave_block(uint32_t p, uint32_t l)
{
	return NET2_AES_WAVE_LANES * p + l;
}

/* Block b's prev: the IV, or ciphertext block aes_wave_prev(b). */
constexpr bool aes_wave_prev_is_iv(uint32_t b)
{
	return b == 0;
}
constexpr uint32_t aes_wave_prev(uint32_t b)
{
	return b - 1u;
}

/* The lane whose block in run NET2_AES_WAVE_VERDICT_RUN is the last one. */
constexpr uint32_t aes_wave_verdict_lane(uint32_t nb)
{
	return (nb - 1u) % NET2_AES_WAVE_LANES;
}

#endif /* NET2_AES_WAVE_H */
