// The bin index, the quantisation and the host conversion of LD decay (csrc/hip/ld_decay_bin.h) played on the host: `make decay-check`
// builds this file with plain g++ and runs it.  Every function goes against a naive restatement that shares no arithmetic with it:
//   the distance      in signed 64-bit integers;
//   the bin           by the distance against the bins' edges in 64-bit integers (k * width <= d < (k + 1) * width, the last bin open);
//   the quantisation  by taking the double apart (frexp) and rounding its 53-bit integer mantissa, shifted, half to even, in integers;
//   the conversion    by rounding the 128-bit integer to 53 bits, half to even, in integers, and scaling with ldexp.
// Covered: d = 0, width - 1, width, the clamp at and beyond range_bp, positions near 2^32, width = 1, n_bins = 1; r2 = 0, 1, one ulp
// beside 1, ties at odd multiples of 2^-33 (both neighbours), and a pseudo-random sweep of all of them.
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../hip/ld_decay_bin.h"

using namespace twk;

namespace {

int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++failures <= 20) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rng() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

uint32_t naive_distance(uint32_t a, uint32_t b) { const int64_t d = (int64_t)a - (int64_t)b; return (uint32_t)(d < 0 ? -d : d); }

uint32_t naive_bin(uint32_t d, uint32_t range_bp, uint32_t n_bins) {
	const uint64_t width = (uint64_t)range_bp / n_bins;
	for (uint64_t k = 0; k + 1 < n_bins; ++k) {
		if ((k + 1) * width > d) return (uint32_t)k;                 // k * width <= d holds: the bins before k were passed
	}
	return n_bins - 1;
}

// value (an integer below 2^127) shifted right by k >= 0 bits, half to even
unsigned __int128 shift_right_half_even(unsigned __int128 v, int k) {
	if (k == 0) return v;
	if (k >= 127) return 0;
	const unsigned __int128 q = v >> k, rem = v - (q << k), half = (unsigned __int128)1 << (k - 1);
	if (rem > half || (rem == half && (q & 1))) return q + 1;
	return q;
}

unsigned long long naive_quantise(double r2) {
	if (r2 == 0.0) return 0;
	int e = 0;
	const double m = frexp(r2, &e);                                  // r2 = m * 2^e, 0.5 <= m < 1
	const unsigned long long mant = (unsigned long long)ldexp(m, 53);      // exact: 53 bits
	const int sh = e - 53 + 32;                                      // r2 * 2^32 = mant * 2^sh
	if (sh >= 0) return (unsigned long long)((unsigned __int128)mant << sh);
	return (unsigned long long)shift_right_half_even(mant, -sh);
}

double naive_sum_to_double(unsigned long long acc_int, unsigned long long acc_frac) {
	unsigned __int128 v = (unsigned __int128)acc_int * 4294967296ull;
	v += acc_frac;
	if (v == 0) return 0.0;
	int bits = 0;
	for (unsigned __int128 x = v; x; x >>= 1) ++bits;
	int sh = bits > 53 ? bits - 53 : 0;
	unsigned __int128 top = shift_right_half_even(v, sh);
	if (top >> 53) { top >>= 1; ++sh; }                              // (the rounding carried into bit 53: a power of two)
	return ldexp((double)(unsigned long long)top, sh - 32);
}

void check_bins(uint32_t range_bp, uint32_t n_bins) {
	const uint32_t width = dk_width(range_bp, n_bins);
	CHECK(width == range_bp / n_bins && width >= 1, "width of %u / %u", range_bp, n_bins);
	std::vector<uint32_t> ds = {0, 1, width - 1, width, width + 1, 2 * width - 1, 2 * width, range_bp - 1, range_bp, range_bp + 1,
	                            width * (n_bins - 1) - 1, width * (n_bins - 1), width * (n_bins - 1) + 1, width * n_bins - 1, width * n_bins,
	                            0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu};
	for (int k = 0; k < 200; ++k) ds.push_back((uint32_t)rng());
	for (int k = 0; k < 200; ++k) ds.push_back((uint32_t)(rng() % ((uint64_t)range_bp + 2 * width + 1)));
	for (const uint32_t d : ds) {
		const uint32_t got = dk_bin(d, width, n_bins), want = naive_bin(d, range_bp, n_bins);
		CHECK(got == want, "bin of d=%u range=%u bins=%u: %u, naive %u", d, range_bp, n_bins, got, want);
		CHECK(got < n_bins, "bin %u of %u", got, n_bins);
	}
	CHECK(dk_bin(0, width, n_bins) == 0, "d = 0");
	CHECK(dk_bin(width - 1, width, n_bins) == 0, "d = width - 1");
	CHECK(dk_bin(width, width, n_bins) == (n_bins > 1 ? 1u : 0u), "d = width");
	CHECK(dk_bin(range_bp, width, n_bins) == n_bins - 1 && dk_bin(0xFFFFFFFFu, width, n_bins) == n_bins - 1, "the clamp");
}

void check_distance() {
	const uint32_t ps[] = {0, 1, 2, 99, 100, 0x7FFFFFFFu, 0x80000000u, 0x80000001u, 0xFFFFFFF0u, 0xFFFFFFFEu, 0xFFFFFFFFu};
	for (const uint32_t a : ps) for (const uint32_t b : ps) {
		CHECK(dk_distance(a, b) == naive_distance(a, b), "distance %u %u", a, b);
		CHECK(dk_distance(a, b) == dk_distance(b, a), "symmetry %u %u", a, b);
	}
	for (int k = 0; k < 1000; ++k) {
		const uint32_t a = (uint32_t)rng(), b = (uint32_t)rng();
		CHECK(dk_distance(a, b) == naive_distance(a, b), "distance %u %u", a, b);
	}
}

void check_quantise() {
	std::vector<double> rs = {0.0, 1.0, nextafter(1.0, 0.0), nextafter(1.0, 2.0), 0.5, 0.25, ldexp(1.0, -32), ldexp(1.0, -33), ldexp(1.0, -34),
	                          nextafter(ldexp(1.0, -33), 0.0), nextafter(ldexp(1.0, -33), 1.0), 5e-324, 1e-300, 0.1, 0.2, 0.8, 1.0 / 3.0};
	// ties: odd multiples of 2^-33 (exact doubles), with both neighbours
	for (const uint64_t k : {0ull, 1ull, 2ull, 3ull, 4ull, 1000ull, 1001ull, 0x7FFFFFFFull, 0x80000000ull, 0xFFFFFFFEull, 0xFFFFFFFFull}) {
		const double tie = ldexp((double)(2 * k + 1), -33);
		rs.push_back(tie); rs.push_back(nextafter(tie, 0.0)); rs.push_back(nextafter(tie, 2.0));
		CHECK(dk_quantise(tie) == ((k & 1) ? k + 1 : k), "tie %" PRIu64 " -> %llu", k, dk_quantise(tie));
	}
	for (int k = 0; k < 20000; ++k) rs.push_back(ldexp((double)(rng() >> 11), -53));            // uniform in [0, 1)
	for (int k = 0; k < 2000; ++k) rs.push_back(ldexp((double)(rng() >> 11), -53 - (int)(rng() % 40)));      // small ones
	for (int k = 0; k < 2000; ++k) rs.push_back(ldexp((double)(2 * (rng() >> 32) + 1), -33));  // random ties
	for (const double r2 : rs) {
		const unsigned long long got = dk_quantise(r2), want = naive_quantise(r2);
		CHECK(got == want, "q of %.17g: %llu, naive %llu", r2, got, want);
		CHECK(fabs((double)got / DECAY_SCALE - r2) <= ldexp(1.0, -33), "q of %.17g is %llu: further than 2^-33", r2, got);
	}
	CHECK(dk_quantise(0.0) == 0 && dk_quantise(1.0) == 1ull << 32, "0 and 1");
	CHECK(dk_quantise(nextafter(1.0, 0.0)) == 1ull << 32 && dk_quantise(nextafter(1.0, 2.0)) == 1ull << 32, "one ulp beside 1");
}

void check_conversion() {
	struct { unsigned long long hi, lo; } cases[] = {{0, 0}, {0, 1}, {0, 0xFFFFFFFFull}, {1, 0}, {0, 1ull << 32}, {0, ~0ull}, {1ull << 20, 0}, {(1ull << 21) - 1, 0xFFFFFFFFull},
	                                                {1ull << 21, 1}, {(1ull << 21) + 1, 0x80000000ull}, {1ull << 40, 0xFFFFFFFFFFull}, {~0ull >> 1, ~0ull}, {~0ull, ~0ull}};
	for (const auto& c : cases) {
		const double got = dk_sum_to_double(c.hi, c.lo), want = naive_sum_to_double(c.hi, c.lo);
		CHECK(got == want, "conversion of %llu, %llu: %.17g, naive %.17g", c.hi, c.lo, got, want);
	}
	for (int k = 0; k < 20000; ++k) {
		const unsigned long long hi = rng() >> (rng() % 64), lo = rng() >> (rng() % 64);
		const double got = dk_sum_to_double(hi, lo), want = naive_sum_to_double(hi, lo);
		CHECK(got == want, "conversion of %llu, %llu: %.17g, naive %.17g", hi, lo, got, want);
	}
	// the split has no carry: any way to cut a sum into blocks gives the same two-word total
	for (int k = 0; k < 200; ++k) {
		unsigned long long hi = 0, lo = 0; unsigned __int128 total = 0;
		for (int b = 0; b < 50; ++b) {
			const unsigned long long S = rng() >> 18;                    // a block's sum: below 2^46
			hi += S >> 32; lo += S & 0xFFFFFFFFull; total += S;
		}
		CHECK((((unsigned __int128)hi << 32) + lo) == total, "split sums");
	}
}

}  // namespace

int main() {
	check_distance();
	const uint32_t shapes[][2] = {{30000, 1}, {30000, 10}, {30000, 300}, {30000, 4096}, {10000000, 1000}, {4096, 4096}, {1, 1}, {7, 3}, {0xFFFFFFFFu, 1},
	                              {0xFFFFFFFFu, 4096}, {0xFFFFFFFFu, 1000}, {5000, 4096}, {8191, 4096}, {8192, 4096}};
	for (const auto& s : shapes) check_bins(s[0], s[1]);
	check_quantise();
	check_conversion();
	if (failures) { fprintf(stderr, "decay_bin_check: %d failures\n", failures); return 1; }
	printf("decay_bin_check: ok\n");
	return 0;
}
