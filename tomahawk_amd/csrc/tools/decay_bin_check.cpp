// The bin index of LD decay (csrc/hip/ld_decay_bin.h) and the exact sums it adds up (csrc/hip/ld_exact_sum.h, through exact_sum_check.h)
// played on the host: `make decay-check` builds this file with plain g++ and runs it.  Every function goes against a naive restatement
// that shares no arithmetic with it:
//   the distance      in signed 64-bit integers;
//   the bin           by the distance against the bins' edges in 64-bit integers (k * width <= d < (k + 1) * width, the last bin open);
//   the sums          exact_sum_check.h: quantisation, split and conversion, for this kind's split width and the aggregate's.
// Covered: d = 0, width - 1, width, the clamp at and beyond range_bp, positions near 2^32, width = 1, n_bins = 1, and a pseudo-random
// sweep of all of them.
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../hip/ld_decay_bin.h"

using namespace twk;

namespace {

uint32_t naive_distance(uint32_t a, uint32_t b) { const int64_t d = (int64_t)a - (int64_t)b; return (uint32_t)(d < 0 ? -d : d); }

uint32_t naive_bin(uint32_t d, uint32_t range_bp, uint32_t n_bins) {
	const uint64_t width = (uint64_t)range_bp / n_bins;
	for (uint64_t k = 0; k + 1 < n_bins; ++k) {
		if ((k + 1) * width > d) return (uint32_t)k;                 // k * width <= d holds: the bins before k were passed
	}
	return n_bins - 1;
}

#include "exact_sum_check.h"      // (with CHECK, failures and rng)

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

}  // namespace

int main() {
	check_distance();
	const uint32_t shapes[][2] = {{30000, 1}, {30000, 10}, {30000, 300}, {30000, 4096}, {10000000, 1000}, {4096, 4096}, {1, 1}, {7, 3}, {0xFFFFFFFFu, 1},
	                              {0xFFFFFFFFu, 4096}, {0xFFFFFFFFu, 1000}, {5000, 4096}, {8191, 4096}, {8192, 4096}};
	for (const auto& s : shapes) check_bins(s[0], s[1]);
	xs_check_all();
	if (failures) { fprintf(stderr, "decay_bin_check: %d failures\n", failures); return 1; }
	printf("decay_bin_check: ok\n");
	return 0;
}
