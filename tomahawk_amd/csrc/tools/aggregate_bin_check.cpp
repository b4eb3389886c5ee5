// The packing, the quantisation, the split and the host conversion of the LD aggregate (csrc/hip/ld_aggregate_bin.h) and the landscape of
// `tomahawk ldaggregate` (csrc/host/twk_aggregate_landscape.h) played on the host: `make aggregate-check` builds this file with plain g++
// and runs it.  Every function goes against a naive restatement that shares no arithmetic with it:
//   the quantisation  by taking the double apart (frexp) and rounding its 53-bit integer mantissa, shifted, half to even, in integers,
//                     the sign put back afterwards;
//   the split         by a floor division and a non-negative remainder in 128-bit integers;
//   the conversion    by rounding the magnitude of the 128-bit integer to 53 bits, half to even, in integers, and scaling with ldexp;
//   the landscape     by walking the contigs for the offset and the bins' edges for the bin, in 64-bit integers.
// Covered: v = 0, +-1, one ulp beside +-1, +-0.25, ties at odd multiples of 2^-33 (both neighbours, both signs) and a pseudo-random
// sweep; negative block sums through the split and back, and many of them accumulated word by word as the device does; 128-bit sums
// against the hand-rounded conversion; one contig, several contigs with an absent one in between, a range above 2^24 where the float
// rounding bites, the clamp, bins = 1.
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

int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++failures <= 20) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rng() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

// value (an integer below 2^127) shifted right by k >= 0 bits, half to even
unsigned __int128 shift_right_half_even(unsigned __int128 v, int k) {
	if (k == 0) return v;
	if (k >= 127) return 0;
	const unsigned __int128 q = v >> k, rem = v - (q << k), half = (unsigned __int128)1 << (k - 1);
	if (rem > half || (rem == half && (q & 1))) return q + 1;
	return q;
}

// rint(|v| * 2^32), half to even, for 0 <= v
unsigned long long naive_quantise_magnitude(double v) {
	if (v == 0.0) return 0;
	int e = 0;
	const double m = frexp(v, &e);                                   // v = m * 2^e, 0.5 <= m < 1
	const unsigned long long mant = (unsigned long long)ldexp(m, 53);      // exact: 53 bits
	const int sh = e - 53 + 32;                                      // v * 2^32 = mant * 2^sh
	if (sh >= 0) return (unsigned long long)((unsigned __int128)mant << sh);
	return (unsigned long long)shift_right_half_even(mant, -sh);
}
// (half to even is symmetric: the magnitude is rounded, the sign put back)
long long naive_quantise(double v) { return v < 0 ? -(long long)naive_quantise_magnitude(-v) : (long long)naive_quantise_magnitude(v); }

double naive_to_double(__int128 q) {          // q / 2^32, rounded once
	if (q == 0) return 0.0;
	const bool neg = q < 0;
	unsigned __int128 v = neg ? (unsigned __int128)(-q) : (unsigned __int128)q;
	int bits = 0;
	for (unsigned __int128 x = v; x; x >>= 1) ++bits;
	int sh = bits > 53 ? bits - 53 : 0;
	unsigned __int128 top = shift_right_half_even(v, sh);
	if (top >> 53) { top >>= 1; ++sh; }                              // (the rounding carried into bit 53: a power of two)
	const double d = ldexp((double)(unsigned long long)top, sh - 32);
	return neg ? -d : d;
}

void check_value(double v) {
	const long long q = ag_quantise(v), want = naive_quantise(v);
	CHECK(q == want, "quantise(%.17g) = %lld, want %lld", v, q, want);
	CHECK(fabs((double)q / AGG_SCALE - v) <= ldexp(1.0, -33), "quantise(%.17g) is more than 2^-33 away", v);
	const double sq = v * v;
	const unsigned long long q2 = ag_quantise_sq(v), want2 = naive_quantise_magnitude(sq);
	CHECK(q2 == want2, "quantise_sq(%.17g) = %llu, want %llu", v, q2, want2);
	CHECK(ag_quantise_sq(-v) == q2 && ag_quantise(-v) == -q, "quantise(%.17g) is not symmetric", v);
	CHECK(ag_value_to_double(q) == naive_to_double(q), "value_to_double(%lld)", q);
}

void check_split(long long s) {
	const long long hi = ag_split_hi(s);
	const unsigned long long lo = ag_split_lo(s);
	// floor division and a non-negative remainder, in 128 bits
	const __int128 S = s, K = (__int128)1 << AGG_SPLIT;
	__int128 fq = S / K, fr = S % K;
	if (fr < 0) { fr += K; fq -= 1; }
	CHECK((__int128)hi == fq && (__int128)lo == fr, "split(%lld) = (%lld, %llu)", s, hi, lo);
	CHECK(lo < (1ull << AGG_SPLIT), "split(%lld): lo = %llu", s, lo);
	CHECK((__int128)hi * K + (__int128)lo == S, "split(%lld) does not add up", s);
	CHECK(ag_sum_to_double_signed((unsigned long long)hi, lo) == naive_to_double(S), "one block sum %lld through the split and back", s);
	if (s >= 0) {
		CHECK(ag_split_hi_u((unsigned long long)s) == (unsigned long long)hi && ag_split_lo_u((unsigned long long)s) == lo, "unsigned split(%lld)", s);
		CHECK(ag_sum_to_double_unsigned((unsigned long long)hi, lo) == naive_to_double(S), "one unsigned block sum %lld through the split and back", s);
	}
}

// Many partial sums accumulated word by word, as the device's atomics do (wrapping 64-bit adds), against their sum in 128 bits.
void check_accumulation(int count, long long magnitude, int sign_mode) {
	unsigned long long acc_hi = 0, acc_lo = 0, uacc_hi = 0, uacc_lo = 0;
	__int128 total = 0;
	unsigned __int128 utotal = 0;
	for (int k = 0; k < count; ++k) {
		long long s = (long long)(rng() % (unsigned long long)magnitude);
		if (sign_mode == 1 || (sign_mode == 2 && (rng() & 1))) s = -s;
		acc_hi += (unsigned long long)ag_split_hi(s); acc_lo += ag_split_lo(s);
		total += s;
		const unsigned long long u = (unsigned long long)(s < 0 ? -s : s);
		uacc_hi += ag_split_hi_u(u); uacc_lo += ag_split_lo_u(u);
		utotal += u;
	}
	CHECK(ag_sum_to_double_signed(acc_hi, acc_lo) == naive_to_double(total), "%d signed sums below %lld (mode %d)", count, magnitude, sign_mode);
	CHECK(ag_sum_to_double_unsigned(uacc_hi, uacc_lo) == naive_to_double((__int128)utotal), "%d unsigned sums below %lld", count, magnitude);
}

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
	// the quantisation
	const double ulp1 = ldexp(1.0, -52);
	for (double v : {0.0, 1.0, 1.0 - ulp1 / 2, 1.0 + ulp1, 1.0 + 4 * ulp1, 0.25, 0.5, 1e-300, ldexp(1.0, -33), ldexp(1.0, -34), ldexp(3.0, -34)}) check_value(v);      // (check_value plays -v too)
	for (long long k = 1; k < 200; k += 2) {          // ties: odd multiples of 2^-33, and their neighbours
		const double tie = ldexp((double)k, -33);
		check_value(tie); check_value(nextafter(tie, 0.0)); check_value(nextafter(tie, 2.0));
		const double big = ldexp((double)((1ll << 32) - k), -33);
		check_value(big); check_value(nextafter(big, 0.0)); check_value(nextafter(big, 2.0));
	}
	CHECK(ag_quantise(1.0) == (1ll << 32) && ag_quantise(-1.0) == -(1ll << 32) && ag_quantise(0.25) == (1ll << 30) && ag_quantise(-0.25) == -(1ll << 30), "the exact values");
	CHECK(ag_quantise(ldexp(1.0, -33)) == 0 && ag_quantise(ldexp(3.0, -33)) == 2 && ag_quantise(-ldexp(3.0, -33)) == -2 && ag_quantise(ldexp(5.0, -33)) == 2, "ties go to even");
	CHECK(ag_quantise_sq(0.5) == (1ull << 30) && ag_quantise_sq(-1.0) == (1ull << 32), "the exact squares");
	for (int k = 0; k < 200000; ++k) check_value((double)(rng() >> 11) * ldexp(1.0, -53) * (1.0 + ldexp(1.0, -40)));
	// the split
	for (long long s : {0ll, 1ll, -1ll, (1ll << 20) - 1, 1ll << 20, -(1ll << 20), -(1ll << 20) - 1, -(1ll << 20) + 1, (1ll << 46), -(1ll << 46), -(1ll << 46) + 12345, (1ll << 39) - 1, -(1ll << 39) + 1,
	                    -(8192ll << 32), 8192ll << 32, 0x7FFFFFFFFFFFFFFFll, -0x7FFFFFFFFFFFFFFFll - 1})
		check_split(s);
	for (int k = 0; k < 200000; ++k) { const long long s = (long long)(rng() >> (1 + rng() % 40)); check_split(s); check_split(-s); }
	// sums of block sums
	for (int mode = 0; mode < 3; ++mode) {
		check_accumulation(1, 1ll << 46, mode);
		check_accumulation(1000, 1ll << 46, mode);
		check_accumulation(100000, 1ll << 46, mode);
		check_accumulation(100000, 1ll << 39, mode);
		check_accumulation(3000000, 1ll << 33, mode);
	}
	// 128-bit sums against the hand-rounded conversion: beyond 2^64, exactly on and beside a rounding tie
	{
		const unsigned long long his[] = {0ull, 1ull, (1ull << 33) + 1, (1ull << 43) + 1, (1ull << 57) - 1, 1ull << 56};
		const unsigned long long los[] = {0ull, 1ull, (1ull << 20) - 1, 1ull << 20, (1ull << 63) - 1, (1ull << 63) + (1ull << 10), (1ull << 63) + (1ull << 10) + 1};
		for (const unsigned long long hi : his) for (const unsigned long long lo : los) {
			const __int128 pos = (__int128)hi * ((__int128)1 << AGG_SPLIT) + (__int128)lo;
			CHECK(ag_sum_to_double_unsigned(hi, lo) == naive_to_double(pos), "unsigned conversion of (%llu, %llu)", hi, lo);
			CHECK(ag_sum_to_double_signed(hi, lo) == naive_to_double(pos), "signed conversion of (%llu, %llu)", hi, lo);
			const __int128 neg = -(__int128)hi * ((__int128)1 << AGG_SPLIT) + (__int128)lo;
			CHECK(ag_sum_to_double_signed((unsigned long long)(-(long long)hi), lo) == naive_to_double(neg), "signed conversion of (-%llu, %llu)", hi, lo);
		}
	}
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
