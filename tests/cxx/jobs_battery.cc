/*
 * jobs_battery.cc -- TEST INFRASTRUCTURE ONLY: the cases of jobs_battery.h.
 *
 * The shapes are the smallest at which the job kernels' indexing and loops
 * can go wrong: one job, one short of / exactly / one past a wave of 64 per
 * family, a SHA-512 family that starts at a job index that is no multiple
 * of 64, neighbouring lanes that differ in block count, in kind and in
 * SHA-384 against SHA-512, block counts on both sides of absorb's two- and
 * four-block trips and of the wave form's 64-block step, and the
 * coalescer's pair of launches (long jobs a wave each, the rest a lane
 * each) on one stream and one counter.
 */
#include "jobs_battery.h"

#include "../../oracle/sha2_oracle.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

namespace jobsbat {
namespace {

enum { DIGEST = 0, HMAC = 1, STATE = 2 };

struct Spec {
	int alg, kind;
	uint32_t nblk;
};

union St {
	uint32_t w32[8];
	uint64_t w64[8];
	uint8_t b[64];
};

struct Rng {
	uint64_t s;
	uint64_t next()
	{
		s ^= s << 13;
		s ^= s >> 7;
		s ^= s << 17;
		return s;
	}
	void fill(uint8_t *p, size_t n)
	{
		for (size_t i = 0; i < n; i++)
			p[i] = (uint8_t)(next() >> 32);
	}
};

[[noreturn]] void die(const char *what, const Spec &sp)
{
	fprintf(stderr, "jobs_battery: %s (alg %d, kind %d, %u blocks): the "
	    "battery itself is wrong\n", what, sp.alg, sp.kind, sp.nblk);
	exit(2);
}

size_t align64(size_t x)
{
	return (x + 63) & ~(size_t)63;
}

void iv_of(int alg, St &st)
{
	oracle_sha2_ctx c;
	memset(&st, 0, sizeof(st));
	if (alg == 1) {
		oracle_sha256_init(&c);
		memcpy(st.w32, c.st.w32, 32);
	} else {
		if (alg == 2)
			oracle_sha384_init(&c);
		else
			oracle_sha512_init(&c);
		memcpy(st.w64, c.st.w64, 64);
	}
}

void run_blocks(int alg, St &st, const uint8_t *p, uint32_t nblk)
{
	for (uint32_t b = 0; b < nblk; b++) {
		if (alg == 1)
			oracle_sha256_transform(st.w32, p + 64 * (size_t)b);
		else
			oracle_sha512_transform(st.w64, p + 128 * (size_t)b);
	}
}

/* The first dlen bytes of the state as SHA*Final stores them. */
void be_prefix(int alg, const St &st, uint8_t *d, size_t dlen)
{
	for (size_t i = 0; i < dlen; i++)
		d[i] = alg == 1 ? (uint8_t)(st.w32[i / 4] >> (24 - 8 * (i % 4))) :
		    (uint8_t)(st.w64[i / 8] >> (56 - 8 * (i % 8)));
}

/* 0x80, zeros and the big-endian bit count after `len` bytes at p. */
size_t pad_message(uint8_t *p, size_t len, size_t blk)
{
	const size_t lb = blk == 64 ? 8 : 16;
	const size_t total = (len + 1 + lb + blk - 1) / blk * blk;
	const uint64_t bits = (uint64_t)len << 3;
	p[len] = 0x80;
	memset(p + len + 1, 0, total - len - 1);
	for (int i = 0; i < 8; i++)
		p[total - 1 - i] = (uint8_t)(bits >> (8 * i));
	return total;
}

/* A message length whose padded form is exactly nblk blocks: the shortest,
 * the longest (the bit count ends flush behind 0x80) or one in between. */
size_t length_for(uint32_t nblk, size_t blk, Rng &rng)
{
	const size_t lb = blk == 64 ? 8 : 16;
	const size_t hi = (size_t)nblk * blk - lb - 1;
	const size_t lo = (size_t)(nblk - 1) * blk > lb ?
	    (size_t)(nblk - 1) * blk - lb : 0;
	switch (rng.next() % 3) {
	case 0:
		return lo;
	case 1:
		return hi;
	default:
		return lo + rng.next() % (hi - lo + 1);
	}
}

/* Lay job sp out at stage + off; its descriptor and expected slot. */
size_t build_job(const Spec &sp, Rng &rng, std::vector<uint8_t> &stage,
    size_t off, Net2Job *desc, uint8_t *slot)
{
	const int alg = sp.alg;
	const size_t blk = alg == 1 ? 64 : 128;
	const size_t dlen = alg == 1 ? 32 : alg == 2 ? 48 : 64;
	const size_t body = (size_t)sp.nblk * blk;
	const size_t aux = sp.kind == DIGEST ? 0 : sp.kind == HMAC ? blk : 64;
	const size_t need = align64(body + aux);
	if (stage.size() < off + need)
		stage.resize(off + need, 0xEE);
	uint8_t *p = stage.data() + off;
	St st;
	uint8_t want[64], got[64];

	desc->data = off;
	desc->aux = off + body;
	desc->nblk = sp.nblk;
	desc->flags = (uint32_t)alg;
	if (sp.kind == STATE) {
		desc->flags |= NET2_JOB_STATE;
		rng.fill(p, body);
		rng.fill(p + body, alg == 1 ? 32 : 64);
		memset(&st, 0, sizeof(st));
		memcpy(st.b, p + body, alg == 1 ? 32 : 64);
		run_blocks(alg, st, p, sp.nblk);
	} else if (sp.kind == DIGEST) {
		if (sp.nblk < 1)
			die("a digest of no block", sp);
		const size_t len = length_for(sp.nblk, blk, rng);
		rng.fill(p, len);
		if (oracle_sha2_digest(alg, p, len, want) != (int)dlen)
			die("oracle digest", sp);
		if (pad_message(p, len, blk) != body)
			die("padded length", sp);
		iv_of(alg, st);
		run_blocks(alg, st, p, sp.nblk);
		be_prefix(alg, st, got, dlen);
		if (memcmp(got, want, dlen) != 0)
			die("staged blocks against the one-shot digest", sp);
	} else {
		if (sp.nblk < 2)
			die("an HMAC of under two blocks", sp);
		desc->flags |= NET2_JOB_HMAC;
		const size_t kls[3] = { dlen, blk, 5 };
		const size_t keylen = kls[rng.next() % 3];
		uint8_t key[128];
		rng.fill(key, sizeof(key));
		/* K' ^ ipad block || message: at least the block itself */
		const size_t total = length_for(sp.nblk, blk, rng);
		const size_t len = total > blk ? total - blk : 0;
		for (size_t i = 0; i < blk; i++) {
			const uint8_t k = i < keylen ? key[i] : 0;
			p[i] = k ^ 0x36;
			p[body + i] = k ^ 0x5c;
		}
		rng.fill(p + blk, len);
		if (oracle_hmac_digest(alg + 3, key, keylen, p + blk, len, want) < 0)
			die("oracle HMAC", sp);
		if (pad_message(p, blk + len, blk) != body)
			die("padded length", sp);
		St in;
		iv_of(alg, in);
		run_blocks(alg, in, p, sp.nblk);
		/* outer hash: IV, K' ^ opad, inner digest || 0x80 || bit count */
		uint8_t ob[128];
		be_prefix(alg, in, ob, dlen);
		if (pad_message(ob, dlen, blk) != blk)
			die("outer block", sp);
		/* the count covers the K' ^ opad block too */
		const uint64_t obits = (uint64_t)(blk + dlen) << 3;
		for (int i = 0; i < 8; i++)
			ob[blk - 1 - i] = (uint8_t)(obits >> (8 * i));
		iv_of(alg, st);
		run_blocks(alg, st, p + body, 1);
		run_blocks(alg, st, ob, 1);
		be_prefix(alg, st, got, dlen);
		if (memcmp(got, want, dlen) != 0)
			die("staged blocks against the one-shot HMAC", sp);
	}
	memcpy(slot, st.b, alg == 1 ? 32 : 64);
	return need;
}

/* Kinds with period 3, block counts cycling through `counts`; 0 blocks only
 * with NET2_JOB_STATE (the result is then the input state), an HMAC at
 * least two (its K' ^ ipad block and the padding). */
Spec spec_for(uint32_t g, int alg, const uint32_t *counts, size_t ncounts)
{
	Spec sp;
	sp.alg = alg;
	sp.kind = (int)(g % 3);
	sp.nblk = counts[g % ncounts];
	if (sp.kind == DIGEST && sp.nblk < 1)
		sp.nblk = 1;
	if (sp.kind == HMAC && sp.nblk < 2)
		sp.nblk = 2;
	return sp;
}

const uint32_t kLaneCounts[] = { 0, 1, 2, 3, 4, 5, 7, 8, 33, 70 };
const uint32_t kWaveCounts[] = { 0, 1, 63, 64, 65, 128, 129, 1024 };

/* n256 SHA-256 jobs, then n512 of SHA-384 (j % 7 < 3) / SHA-512; g0 shifts
 * the cycles so the cases start at different places. */
void family_specs(std::vector<Spec> &specs, uint32_t n256, uint32_t n512,
    uint32_t g0, const uint32_t *counts, size_t ncounts)
{
	for (uint32_t j = 0; j < n256; j++)
		specs.push_back(spec_for(g0 + (uint32_t)specs.size(), 1, counts,
		    ncounts));
	for (uint32_t j = 0; j < n512; j++)
		specs.push_back(spec_for(g0 + (uint32_t)specs.size(),
		    j % 7 < 3 ? 2 : 3, counts, ncounts));
}

Case make_case(const std::string &name, const std::vector<Spec> &specs,
    const std::vector<Launch> &launches, uint64_t seed)
{
	Case c;
	Rng rng = { seed * 0x9E3779B97F4A7C15ull + 1 };
	const uint32_t n = (uint32_t)specs.size();
	std::vector<Net2Job> descs(n);
	c.name = name;
	c.njobs = n;
	c.launches = launches;
	c.expect.resize(64 * (size_t)n);
	for (size_t i = 0; i < c.expect.size(); i++)
		c.expect[i] = canary(i);
	/* staging in arrival order, not job order (the coalescer sorts the
	 * descriptors after the callers have reserved their ranges): odd job
	 * indices first, then the even ones */
	size_t used = 0;
	for (int pass = 1; pass >= 0; pass--)
		for (uint32_t j = (uint32_t)pass; j < n; j += 2)
			used += build_job(specs[j], rng, c.stage, used, &descs[j],
			    c.expect.data() + 64 * (size_t)j);
	c.jobs_off = align64(used);
	c.stage.resize(align64(c.jobs_off + n * sizeof(Net2Job)), 0xEE);
	memcpy(c.stage.data() + c.jobs_off, descs.data(), n * sizeof(Net2Job));
	c.waves = 0;
	for (const Spec &sp : specs)
		c.alg.push_back(sp.alg);
	for (const Launch &l : launches)
		c.waves += launch_waves(l);
	return c;
}

}	/* namespace */

uint32_t launch_waves(const Launch &l)
{
	return l.wave ? l.n256 + l.n512 : (l.n256 + 63) / 64 + (l.n512 + 63) / 64;
}

uint8_t canary(size_t i)
{
	return (uint8_t)(0xA5 ^ (i * 7));
}

void fill_canary(uint8_t *out, size_t slots)
{
	for (size_t i = 0; i < 64 * slots; i++)
		out[i] = canary(i);
}

std::vector<Case> build_cases()
{
	std::vector<Case> cases;
	char name[96];
	uint64_t seed = 1;

	const uint32_t lane[][2] = { { 1, 0 }, { 0, 1 }, { 63, 0 }, { 64, 0 },
	    { 65, 0 }, { 0, 65 }, { 64, 64 }, { 65, 129 }, { 130, 1 } };
	for (const uint32_t (&s)[2] : lane) {
		/* (65, 129) also in pieces: the lane form then splits a job
		 * while its neighbours go through whole */
		const uint32_t chunks[] = { 0x80000000u, 128, 4096 };
		const size_t nc = s[0] == 65 && s[1] == 129 ? 3 : 1;
		for (size_t k = 0; k < nc; k++) {
			std::vector<Spec> specs;
			family_specs(specs, s[0], s[1], (uint32_t)cases.size(),
			    kLaneCounts, 10);
			snprintf(name, sizeof(name), "lane (%u,%u) chunk %u", s[0],
			    s[1], chunks[k]);
			cases.push_back(make_case(name, specs,
			    { { 0, s[0], s[1], 0, chunks[k] } }, seed++));
		}
	}
	const uint32_t wave[][2] = { { 1, 0 }, { 0, 1 }, { 3, 2 }, { 16, 16 } };
	for (const uint32_t (&s)[2] : wave) {
		std::vector<Spec> specs;
		family_specs(specs, s[0], s[1], (uint32_t)cases.size(), kWaveCounts,
		    8);
		snprintf(name, sizeof(name), "wave (%u,%u)", s[0], s[1]);
		cases.push_back(make_case(name, specs,
		    { { 0, s[0], s[1], 1, 0x80000000u } }, seed++));
	}
	{
		/* the coalescer's mixed pair: two long jobs a wave each, then 70
		 * small ones a lane each, results behind the long jobs' */
		std::vector<Spec> specs;
		specs.push_back({ 1, DIGEST, 1024 });
		specs.push_back({ 2, HMAC, 1030 });
		family_specs(specs, 5, 65, 0, kLaneCounts, 10);
		cases.push_back(make_case("pair (1,1) wave + (5,65) lane", specs,
		    { { 0, 1, 1, 1, 0x80000000u }, { 2, 5, 65, 0, 0x80000000u } },
		    seed++));
	}
	return cases;
}

int check_case(const char *who, const Case &c, const uint8_t *out,
    uint32_t done_before, uint32_t done_after)
{
	int bad = 0;
	for (uint32_t j = 0; j < c.njobs; j++) {
		const uint8_t *g = out + 64 * (size_t)j;
		const uint8_t *w = c.expect.data() + 64 * (size_t)j;
		const size_t words = c.alg[j] == 1 ? 32 : 64;
		if (memcmp(g, w, words) != 0) {
			if (bad++ < 8)
				fprintf(stderr, "%s: %s: job %u (alg %d): wrong "
				    "state words\n", who, c.name.c_str(), j, c.alg[j]);
		} else if (memcmp(g + words, w + words, 64 - words) != 0) {
			if (bad++ < 8)
				fprintf(stderr, "%s: %s: job %u: bytes 32-63 of a "
				    "SHA-256 slot were written\n", who, c.name.c_str(),
				    j);
		}
	}
	for (size_t i = 64 * (size_t)c.njobs;
	    i < 64 * ((size_t)c.njobs + kSpareSlots); i++)
		if (out[i] != canary(i)) {
			if (bad++ < 8)
				fprintf(stderr, "%s: %s: result slot %zu, past the "
				    "last job, was written\n", who, c.name.c_str(),
				    i / 64);
			break;
		}
	if (done_after - done_before != c.waves) {
		bad++;
		fprintf(stderr, "%s: %s: the counter advanced by %u, expected "
		    "%u\n", who, c.name.c_str(), done_after - done_before, c.waves);
	}
	return bad;
}

}	/* namespace jobsbat */
