// The packing of the LD aggregate (csrc/hip/ld_aggregate_bin.h), the exact sums it adds up (csrc/hip/ld_exact_sum.h, through
// exact_sum_check.h) and the landscape of `tomahawk ldaggregate` (csrc/host/twk_aggregate_landscape.h) played on the host:
// `make aggregate-check` builds this file with plain g++ and runs it.  Every function goes against a naive restatement that shares no
// arithmetic with it:
//   the sums          exact_sum_check.h: quantisation, split and conversion, for this kind's split width and decay's;
//   the landscape     by walking the contigs for the offset and the bins' edges for the bin, in 64-bit integers.
// Covered: every pair of valid, last and off bins through the packing; one contig, several contigs with an absent one in between, a
// range above 2^24 where the float rounding bites, the clamp, bins = 1.
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../hip/ld_aggregate_bin.h"
#include "../host/twk_aggregate_landscape.h"

using namespace twk;
using namespace tomahawk;

namespace {

#include "exact_sum_check.h"      // (with CHECK, failures and rng)

// ---- the landscape ----------------------------------------------------------------------------------------------------------------------
uint32_t naive_bases_per_bin(uint64_t range, uint32_t bins) {
	const float q = (float)range / (float)bins;          // the reference's expression is the definition; ceil by counting
	uint32_t c = (uint32_t)q;
	if ((float)c < q) ++c;
	return c;
}
uint32_t naive_bin(uint64_t coord, uint32_t bpb, uint32_t bins) {
	for (uint64_t k = 0; k + 1 < bins; ++k)
		if ((k + 1) * bpb > coord) return (uint32_t)k;
	return bins - 1;
}

void check_landscape(const std::vector<uint32_t>& rid, const std::vector<uint32_t>& pos, const std::vector<int64_t>& bases, uint32_t xb, uint32_t yb,
                     bool want_single, uint64_t want_range, const char* what) {
	twk_aggregate_landscape l;
	std::vector<uint16_t> bx, by;
	const bool ok = agl_build(rid.data(), pos.data(), rid.size(), bases, xb, yb, l, bx, by);
	CHECK(ok, "%s: refused", what);
	if (!ok) return;
	CHECK(l.single == want_single && l.range == want_range, "%s: single %d range %" PRIu64 ", want %d %" PRIu64, what, (int)l.single, l.range, (int)want_single, want_range);
	CHECK(l.bpx == naive_bases_per_bin(want_range, xb) && l.bpy == naive_bases_per_bin(want_range, yb), "%s: bases per bin %u, %u", what, l.bpx, l.bpy);
	CHECK(l.bpx >= 1 && l.bpy >= 1, "%s: an empty bin width", what);
	uint32_t lo = 0xFFFFFFFFu;
	for (const uint32_t p : pos) if (p < lo) lo = p;
	for (size_t v = 0; v < rid.size(); ++v) {
		uint64_t coord;
		if (want_single) coord = pos[v] - lo;
		else {
			coord = pos[v];
			for (uint32_t k = 0; k < rid[v]; ++k) {          // the contigs in front that hold a variant
				bool present = false;
				for (const uint32_t r : rid) present = present || r == k;
				if (present) coord += (uint64_t)bases[k];
			}
		}
		const uint32_t wx = naive_bin(coord, l.bpx, xb), wy = naive_bin(coord, l.bpy, yb);
		CHECK(bx[v] == wx && by[v] == wy, "%s: variant %zu at coordinate %" PRIu64 ": bins (%u, %u), want (%u, %u)", what, v, coord, bx[v], by[v], wx, wy);
		CHECK(bx[v] < xb && by[v] < yb, "%s: variant %zu beyond the last bin", what, v);
	}
}

}  // namespace

int main() {
	// the packing
	for (uint32_t x : {0u, 1u, 4095u, 0xFFFFu}) for (uint32_t y : {0u, 7u, 4095u, 0xFFFFu}) {
		const uint32_t k = ag_pack(x, y);
		CHECK(ag_x(k) == x && ag_y(k) == y, "pack(%u, %u)", x, y);
		CHECK((k == AGG_NO_KEY) == (x == AGG_OFF && y == AGG_OFF), "pack(%u, %u) against the no-key word", x, y);
	}
	// the quantisation, the split, sums of block sums and the conversion
	xs_check_all();
	// the landscape
	{
		const std::vector<int64_t> bases = {1000000, 5000000, 300, 20000000, 70000};
		// one contig (not the first): the data's range
		check_landscape({1, 1, 1, 1, 1}, {1000, 1001, 5000, 30899, 30900}, bases, 5, 13, true, 29901, "one contig");
		check_landscape({0, 0, 0}, {7, 8, 99}, bases, 1000, 4096, true, 93, "only contig 0, more bins than bases");
		check_landscape({3}, {12345}, bases, 5, 5, true, 1, "a single variant");
		// several contigs, an absent one in between
		check_landscape({0, 0, 1, 3, 3, 3}, {0, 999999, 17, 0, 19999999, 5000}, bases, 1000, 7, false, 26000000, "three contigs, contig 2 absent");
		check_landscape({1, 4}, {4999999, 69999}, bases, 64, 64, false, 5070000, "two contigs, the first absent");
		// bins = 1
		check_landscape({0, 1, 3}, {5, 6, 7}, bases, 1, 1, false, 26000000, "one bin");
		check_landscape({1, 1}, {5, 600}, bases, 1, 4096, true, 596, "one bin on x");
		// a range above 2^24 where (float)range rounds downwards: 2^24 + 1 -> 2^24, one bin of 2^24 bases, coordinate 2^24 -> the clamp
		check_landscape({1, 1, 1}, {0, 5, 16777216}, {0, 16777217}, 1, 2, true, 16777217, "the clamp: range 2^24 + 1, one bin");
		CHECK(agl_bases_per_bin(16777217, 1) == 16777216u && 16777216ull / agl_bases_per_bin(16777217, 1) == 1 && agl_bin(16777216, 16777216u, 1) == 0, "the clamp is needed and holds");
		{
			// 4096 bins over 2^32 - 257 bases: every coordinate of the last megabase stays inside
			const uint64_t range = 0xFFFFFEFFull;
			const uint32_t bpb = agl_bases_per_bin(range, 4096);
			CHECK(bpb == naive_bases_per_bin(range, 4096), "bases per bin of a range near 2^32");
			for (uint64_t c = range - 1000000; c < range; c += 997) CHECK(agl_bin(c, bpb, 4096) == naive_bin(c, bpb, 4096) && agl_bin(c, bpb, 4096) < 4096, "bin of %" PRIu64, c);
		}
		std::vector<uint32_t> rid, pos;
		for (int k = 0; k < 3000; ++k) { rid.push_back((uint32_t)(rng() % 2) * 3); pos.push_back((uint32_t)(rng() % (rid.back() ? 20000000 : 1000000))); }
		check_landscape(rid, pos, bases, 1000, 777, false, 21000000, "a random set on two contigs");
		for (auto& r : rid) r = 3;
		uint32_t lo = 0xFFFFFFFFu, hi = 0;
		for (const uint32_t p : pos) { if (p < lo) lo = p; if (p > hi) hi = p; }
		check_landscape(rid, pos, bases, 4096, 33, true, (uint64_t)hi - lo + 1, "a random set on one contig");
		// refusals
		twk_aggregate_landscape l;
		std::vector<uint16_t> bx, by;
		const uint32_t r5 = 5, p0 = 0;
		CHECK(!agl_build(&r5, &p0, 1, bases, 5, 5, l, bx, by), "a contig the header does not have");
		CHECK(!agl_build(&p0, &p0, 1, bases, 0, 5, l, bx, by) && !agl_build(&p0, &p0, 1, bases, 5, 4097, l, bx, by) && !agl_build(&p0, &p0, 0, bases, 5, 5, l, bx, by), "bin counts and an empty set");
	}
	if (failures) { fprintf(stderr, "aggregate_bin_check: %d failure(s)\n", failures); return 1; }
	printf("aggregate_bin_check: ok\n");
	return 0;
}
