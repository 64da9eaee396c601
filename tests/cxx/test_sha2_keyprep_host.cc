/*
 * test_sha2_keyprep_host.cc -- host check of what the keyed launchers compute
 * before a launch (sha2_keyprep.h), without a GPU.  The cases come from a
 * file the Python test writes (tests/test_sha2_keyprep_host.py), one per
 * line, every expected value worked out there with hmac / hashlib:
 *   K halg key alt|-        hmac_key_mids of the two keys (hex): accepted, the
 *                           words in HMid's layout, slots 2/3 zero without alt
 *   M msg|- dig altdig|-    under the last K: HMAC(key, msg) completed from
 *                           slots 0/1 (and HMAC(alt, msg) from slots 2/3)
 *   R halg key              a key of more than a block: refused, *hm zero
 *   P 256|512 bits kw...    pad_kw256 / pad_kw512 of a bit count: K[t] + W[t]
 *
 * Exits non-zero with a message on the first mismatch.
 *   c++ -std=c++17 -Iilias_net2_amd/csrc tests/cxx/test_sha2_keyprep_host.cc
 */
#include "sha2_keyprep.h"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

using namespace net2::dev;

namespace {

[[noreturn]] void fail(const char *fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	fprintf(stderr, "test_sha2_keyprep_host: FAIL: ");
	vfprintf(stderr, fmt, ap);
	fprintf(stderr, "\n");
	va_end(ap);
	exit(1);
}

typedef std::vector<uint8_t> Bytes;

/* "-" is the empty string */
Bytes unhex(const std::string &h)
{
	Bytes out;
	if (h == "-")
		return out;
	if (h.size() % 2 != 0)
		fail("odd hex %s", h.c_str());
	for (size_t i = 0; i < h.size(); i += 2) {
		unsigned v;
		if (sscanf(h.c_str() + i, "%2x", &v) != 1)
			fail("bad hex %s", h.c_str());
		out.push_back((uint8_t)v);
	}
	return out;
}

std::vector<std::string> split(const char *line)
{
	std::vector<std::string> f;
	std::string cur;
	for (const char *p = line;; p++) {
		if (*p == ' ' || *p == '\n' || *p == '\0') {
			if (!cur.empty())
				f.push_back(cur);
			cur.clear();
			if (*p == '\0')
				break;
		} else {
			cur.push_back(*p);
		}
	}
	return f;
}

/*
 * One hash from a midstate in HMid's word layout (SHA-256: 8 words, then
 * zeros; SHA-384/512: hi, lo per 64-bit word): `msg` after `before` bytes
 * already absorbed, FIPS 180-4 padding, the first dlen digest bytes.
 */
Bytes finish_from(int halg, const uint32_t mid[16], size_t before,
    const Bytes &msg)
{
	const size_t blk = halg == 1 ? 64 : 128, lenbytes = halg == 1 ? 8 : 16;
	const size_t dlen = halg == 1 ? 32 : halg == 2 ? 48 : 64;
	Bytes m = msg;
	m.push_back(0x80);
	while ((m.size() + lenbytes) % blk != 0)
		m.push_back(0);
	const uint64_t bits = (uint64_t)(before + msg.size()) * 8;
	for (size_t i = 0; i < lenbytes; i++)
		m.push_back(i + 8 < lenbytes ? 0 :
		    (uint8_t)(bits >> (8 * (lenbytes - 1 - i))));
	Bytes out;
	if (halg == 1) {
		uint32_t st[8];
		for (int i = 0; i < 8; i++)
			st[i] = mid[i];
		for (size_t b = 0; b < m.size(); b += 64) {
			uint32_t w[16];
			for (int i = 0; i < 16; i++)
				w[i] = (uint32_t)m[b + 4 * i] << 24 |
				    (uint32_t)m[b + 4 * i + 1] << 16 |
				    (uint32_t)m[b + 4 * i + 2] << 8 | m[b + 4 * i + 3];
			h_compress256(st, w);
		}
		for (int i = 0; i < 8; i++)
			for (int b = 0; b < 4; b++)
				out.push_back((uint8_t)(st[i] >> (24 - 8 * b)));
	} else {
		uint64_t st[8];
		for (int i = 0; i < 8; i++)
			st[i] = (uint64_t)mid[2 * i] << 32 | mid[2 * i + 1];
		for (size_t b = 0; b < m.size(); b += 128) {
			uint64_t w[16];
			for (int i = 0; i < 16; i++) {
				w[i] = 0;
				for (int k = 0; k < 8; k++)
					w[i] = w[i] << 8 | m[b + 8 * i + k];
			}
			h_compress512(st, w);
		}
		for (int i = 0; i < 8; i++)
			for (int b = 0; b < 8; b++)
				out.push_back((uint8_t)(st[i] >> (56 - 8 * b)));
	}
	out.resize(dlen);
	return out;
}

Bytes hmac_from(int halg, const HMid &hm, int slot, const Bytes &msg)
{
	const size_t blk = halg == 1 ? 64 : 128;
	const Bytes inner = finish_from(halg, hm.w[slot], blk, msg);
	return finish_from(halg, hm.w[slot + 1], blk, inner);
}

bool all_zero(const uint32_t *w, size_t n)
{
	for (size_t i = 0; i < n; i++)
		if (w[i] != 0)
			return false;
	return true;
}

}	/* namespace */

int main(int argc, char **argv)
{
	if (argc != 2)
		fail("usage: %s cases-file", argv[0]);
	FILE *f = fopen(argv[1], "r");
	if (f == nullptr)
		fail("cannot open %s", argv[1]);
	static char line[1 << 16];
	int halg = 0, nk = 0, nm = 0, nr = 0, np = 0, lineno = 0;
	bool have_alt = false;
	HMid hm;
	while (fgets(line, sizeof(line), f) != nullptr) {
		lineno++;
		const std::vector<std::string> a = split(line);
		if (a.empty())
			continue;
		if (a[0] == "K" && a.size() == 4) {
			halg = atoi(a[1].c_str());
			const Bytes key = unhex(a[2]), alt = unhex(a[3]);
			have_alt = !alt.empty();
			if (have_alt && alt.size() != key.size())
				fail("line %d: alternate key of another length", lineno);
			memset(&hm, 0xa5, sizeof(hm));	/* every word is written */
			if (!hmac_key_mids(halg, key.data(),
			    have_alt ? alt.data() : nullptr, key.size(), &hm))
				fail("line %d: a key of %zu bytes refused", lineno,
				    key.size());
			for (int s = 0; s < 4; s++) {
				if (s >= 2 && !have_alt) {
					if (!all_zero(hm.w[s], 16))
						fail("line %d: slot %d not zero without an "
						    "alternate key", lineno, s);
				} else if (halg == 1 && !all_zero(hm.w[s] + 8, 8)) {
					fail("line %d: SHA-256 slot %d, words 8..15 not "
					    "zero", lineno, s);
				} else if (all_zero(hm.w[s], 8)) {
					fail("line %d: slot %d empty", lineno, s);
				}
			}
			nk++;
		} else if (a[0] == "M" && a.size() == 4) {
			if (halg == 0)
				fail("line %d: M before K", lineno);
			const Bytes msg = unhex(a[1]);
			if (hmac_from(halg, hm, 0, msg) != unhex(a[2]))
				fail("line %d: HMAC from slots 0/1, halg %d, %zu-byte "
				    "message", lineno, halg, msg.size());
			if (have_alt != (a[3] != "-"))
				fail("line %d: alternate digest without a key", lineno);
			if (have_alt && hmac_from(halg, hm, 2, msg) != unhex(a[3]))
				fail("line %d: HMAC from slots 2/3, halg %d, %zu-byte "
				    "message", lineno, halg, msg.size());
			nm++;
		} else if (a[0] == "R" && a.size() == 3) {
			const Bytes key = unhex(a[2]);
			HMid r;
			memset(&r, 0xa5, sizeof(r));
			if (hmac_key_mids(atoi(a[1].c_str()), key.data(), key.data(),
			    key.size(), &r))
				fail("line %d: a key of %zu bytes accepted", lineno,
				    key.size());
			if (!all_zero(&r.w[0][0], 64))
				fail("line %d: refused, but *hm not zero", lineno);
			nr++;
		} else if (a[0] == "P" && a.size() >= 3) {
			const uint64_t bits = strtoull(a[2].c_str(), nullptr, 10);
			if (a[1] == "256") {
				PadKW<uint32_t> p;
				pad_kw256(bits, p);
				if (a.size() != 3 + 64)
					fail("line %d: want 64 words", lineno);
				for (int t = 0; t < 64; t++)
					if (p.kw[t] != strtoull(a[3 + t].c_str(), nullptr, 16))
						fail("line %d: pad_kw256(%llu) kw[%d]", lineno,
						    (unsigned long long)bits, t);
			} else {
				PadKW<uint64_t> p;
				pad_kw512(bits, p);
				if (a.size() != 3 + 80)
					fail("line %d: want 80 words", lineno);
				for (int t = 0; t < 80; t++)
					if (p.kw[t] != strtoull(a[3 + t].c_str(), nullptr, 16))
						fail("line %d: pad_kw512(%llu) kw[%d]", lineno,
						    (unsigned long long)bits, t);
			}
			np++;
		} else {
			fail("line %d: not a case: %s", lineno, line);
		}
	}
	fclose(f);
	printf("test_sha2_keyprep_host: ok (%d keys, %d messages, %d refusals, "
	    "%d pad schedules)\n", nk, nm, nr, np);
	return 0;
}
