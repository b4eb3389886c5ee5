// The partitioned LD score's term, split and block arithmetic (csrc/hip/ld_annot_term.h) played on the host: `make annot-check` builds this
// file with g++ -fsanitize=address,undefined and runs it.  Everything goes against a restatement that shares no arithmetic with it:
//   the term     at_term(at_scale(r2), a) against llrint((r2 * a) * 4294967296.0): r2 in {0, the smallest positive double, 2^-33,
//                0.5 -+ 1 ulp, 1, 1 + 4 ulps} and a few thousand random values, annotations in {0, -0.0, +-1, +-2^-40, +-0.5, +-2^16, random},
//                and products that land exactly on a tie - each checked to be a tie and to round to even;
//   the sums     exact_sum_check.h: quantisation, and split, accumulation and conversion for this kind's split width;
//   the block    every thread's (half, row, category) and the columns it walks, the ballot words and mask bytes the kernel reads them
//                through, the LDS banks a half-wave meets, the accumulator words - and a whole block, slab by slab and side by side as
//                the kernel forms it, against the plain double loop over its pairs.
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <utility>
#include <vector>

#include "../hip/ld_annot_term.h"

using namespace twk;

namespace {

#include "exact_sum_check.h"      // (CHECK, failures, rng and the checks of ld_exact_sum.h)

long long cases = 0;

void check_term(double r2, double a) {
	++cases;
	const long long got = at_term(at_scale(r2), a), want = llrint((r2 * a) * 4294967296.0);
	CHECK(got == want, "term(%.17g, %.17g) = %lld, want %lld", r2, a, got, want);
	CHECK(want == xs_quantise(r2 * a), "the definition: xs_quantise(%.17g * %.17g)", r2, a);
}

double random_unit() { return (double)(rng() >> 11) * ldexp(1.0, -53); }

void check_terms() {
	const double ulp_half = ldexp(1.0, -53), ulp1 = ldexp(1.0, -52);
	std::vector<double> r2s = {0.0, 5e-324, ldexp(1.0, -33), 0.5 - ulp_half / 2, 0.5, 0.5 + ulp_half * 2, nextafter(0.5, 0.0), nextafter(0.5, 1.0), 1.0, 1.0 + 4 * ulp1,
	                           nextafter(1.0, 0.0), ldexp(1.0, -1022), ldexp(1.0, -32), ldexp(3.0, -33), 0.1, 1.0 / 3.0};
	for (int k = 0; k < 4000; ++k) r2s.push_back(random_unit() * (1.0 + ldexp(1.0, -40)));
	for (int k = 0; k < 500; ++k) r2s.push_back(ldexp(random_unit(), -(int)(rng() % 60)));
	std::vector<double> as = {0.0, -0.0, 1.0, -1.0, ldexp(1.0, -40), -ldexp(1.0, -40), 0.5, -0.5, 65536.0, -65536.0, 3.0, 0.3, 65535.999, nextafter(65536.0, 0.0), 5e-324, -5e-324};
	for (int k = 0; k < 40; ++k) {
		as.push_back(random_unit());                                   // U(0, 1)
		as.push_back((random_unit() - 0.5) * 8.0);                     // signed, a few units
		as.push_back((random_unit() - 0.5) * 131072.0);                // the whole range
		as.push_back(ldexp(random_unit(), -40));                       // terms of a few quanta
	}
	for (const double r2 : r2s) for (const double a : as) check_term(r2, a);
	CHECK(at_term(at_scale(1.0), 1.0) == (1ll << 32) && at_term(at_scale(1.0), -65536.0) == -(1ll << 48) && at_term(at_scale(0.25), 0.0) == 0 && at_term(at_scale(0.25), -0.0) == 0, "the exact values");
	CHECK(at_term(0.0, 65536.0) == 0 && at_term(0.0, -1.0) == 0, "a parked 0 adds nothing");
	// exact ties: r2 * a = (2k + 1) * 2^-33, the product exact - r2 = odd * 2^-33 / |a| for a power of two, odd * 2^-33 for a small odd a
	struct Tie { double a; int shift; };
	for (const Tie tie : {Tie{1.0, 0}, Tie{0.5, 1}, Tie{65536.0, -16}, Tie{0.25, 2}, Tie{3.0, 0}, Tie{5.0, 0}, Tie{65535.0, 0}})
		for (int k = 0; k < 3000; ++k) {
			const uint64_t odd = 2 * (k < 64 ? (uint64_t)k : rng() >> (32 + rng() % 20)) + 1;
			const double r2 = ldexp((double)odd, -33 + tie.shift);
			if (r2 > 1.0) continue;
			for (const double a : {tie.a, -tie.a}) {
				const double x = (r2 * a) * 4294967296.0;
				CHECK(fabs(x) - floor(fabs(x)) == 0.5, "%.17g * %.17g is not a tie", r2, a);
				check_term(r2, a);
				const long long got = at_term(at_scale(r2), a);
				CHECK((got & 1) == 0 && fabs((double)got - x) == 0.5, "the tie %.17g * %.17g rounds to %lld", r2, a, got);
			}
		}
	CHECK(!at_valid(NAN) && !at_valid(INFINITY) && !at_valid(-INFINITY) && !at_valid(65537.0) && !at_valid(nextafter(65536.0, 1e9)) && at_valid(65536.0) && at_valid(-65536.0) && at_valid(-0.0), "the accepted range");
}

// ---- the block ----
void check_threads() {
	std::set<std::pair<uint32_t, std::pair<uint32_t, uint32_t>>> seen;
	for (uint32_t t = 0; t < (uint32_t)ANNOT_THREADS; ++t) {
		++cases;
		const uint32_t half = an_half(t), row = an_row(t), cat = an_cat(t);
		CHECK(half < (uint32_t)ANNOT_HALVES && row < (uint32_t)ANNOT_ROWS && cat < (uint32_t)ANNOT_SLAB, "thread %u: (%u, %u, %u)", t, half, row, cat);
		CHECK(seen.insert({half, {row, cat}}).second, "thread %u: (%u, %u, %u) twice", t, half, row, cat);
		CHECK(an_half(t) == an_half(t & ~63u), "thread %u: a wave lies in one half", t);
		// the staging threads of the row annotations: t < 128 is (row, category) with half 0, and lane & 56 is the first bit of its row's byte
		if (t < (uint32_t)(ANNOT_ROWS * ANNOT_SLAB)) CHECK(half == 0 && t / ANNOT_SLAB == row && ((t & 63) & 56) == (row & 7) * 8, "staging thread %u", t);
	}
	// the columns a thread walks: each of its half once, through the ballot word of the wave that staged it
	for (uint32_t half = 0; half < (uint32_t)ANNOT_HALVES; ++half) {
		std::set<uint32_t> cols;
		for (uint32_t word = 0; word < 2; ++word) for (uint32_t bit = 0; bit < 64; ++bit) {
			++cases;
			const uint32_t col = an_col(half, word, bit);
			CHECK(col < (uint32_t)ANNOT_THREADS && col / 64 == half * 2 + word && col % 64 == bit, "column of (%u, %u, %u): %u", half, word, bit, col);
			cols.insert(col);
		}
		CHECK(cols.size() == (size_t)ANNOT_ROW_SIDE_COLS, "half %u walks %zu columns", half, cols.size());
	}
	// banks (ds_read_b64: dword address mod 64, two dwords a lane, conflicts within a half-wave): the row side's reads of one column
	for (uint32_t t0 = 0; t0 < (uint32_t)ANNOT_THREADS; t0 += 32) for (uint32_t col : {0u, 1u, 63u, 127u, 255u}) {
		++cases;
		std::map<uint32_t, uint32_t> stage_bank, annot_bank;      // bank -> address
		for (uint32_t t = t0; t < t0 + 32; ++t) {
			const uint32_t sa = (an_row(t) * ANNOT_STRIDE + col) * 2, aa = (an_cat(t) * ANNOT_STRIDE + col) * 2;
			for (uint32_t d = 0; d < 2; ++d) {
				auto s = stage_bank.emplace((sa + d) % 64, sa + d); CHECK(s.first->second == sa + d, "stage: two addresses on bank %u", (sa + d) % 64);
				auto a = annot_bank.emplace((aa + d) % 64, aa + d); CHECK(a.first->second == aa + d, "annotations: two addresses on bank %u", (aa + d) % 64);
			}
		}
	}
	for (const uint32_t C : {1u, 7u, 8u, 9u, 65u, 256u}) {
		++cases;
		CHECK(an_slabs(C) * ANNOT_SLAB >= C && (an_slabs(C) - 1) * ANNOT_SLAB < C, "slabs of %u", C);
		std::set<uint64_t> words;
		for (uint32_t v = 0; v < 5; ++v) for (uint32_t c = 0; c < C; ++c) {
			const uint64_t w = an_word(v, C, c);
			CHECK(w + 1 < 2ull * 5 * C && words.insert(w).second && words.insert(w + 1).second, "word of (%u, %u) of %u", v, c, C);
		}
	}
	CHECK(an_word(0xFFFFFFFFu, 256, 255) == ((uint64_t)0xFFFFFFFFu * 256 + 255) * 2, "the last word is formed in 64 bits");
}

// One block as the kernel forms it - the stage, the slabs, the masks, both sides, the split into two words - against the double loop.
void check_block(uint32_t rows, uint32_t cols, uint32_t C, double density, double zero_rate) {
	++cases;
	std::vector<double> stage((size_t)ANNOT_ROWS * ANNOT_STRIDE, 0.0);
	for (uint32_t r = 0; r < rows; ++r) for (uint32_t j = 0; j < cols; ++j)
		if (random_unit() < density) stage[(size_t)r * ANNOT_STRIDE + j] = at_scale(random_unit());
	auto annotation = [&] { return random_unit() < zero_rate ? 0.0 : (rng() & 1) ? 1.0 : (random_unit() - 0.5) * 131072.0; };
	std::vector<double> row_annot((size_t)ANNOT_ROWS * C, 0.0), col_annot((size_t)ANNOT_THREADS * C, 0.0);
	for (uint32_t r = 0; r < rows; ++r) for (uint32_t c = 0; c < C; ++c) row_annot[(size_t)r * C + c] = annotation();
	for (uint32_t j = 0; j < cols; ++j) for (uint32_t c = 0; c < C; ++c) col_annot[(size_t)j * C + c] = annotation();
	// variants: rows 0 .. 15, columns 16 .. 271
	const uint32_t V = ANNOT_ROWS + ANNOT_THREADS;
	std::vector<unsigned long long> acc((size_t)V * C * 2, 0ull);
	std::vector<__int128> want((size_t)V * C, 0);
	for (uint32_t r = 0; r < rows; ++r) for (uint32_t j = 0; j < cols; ++j) for (uint32_t c = 0; c < C; ++c) {
		const double r2 = stage[(size_t)r * ANNOT_STRIDE + j] / 4294967296.0;
		want[(size_t)r * C + c] += llrint((r2 * col_annot[(size_t)j * C + c]) * 4294967296.0);
		want[(size_t)(ANNOT_ROWS + j) * C + c] += llrint((r2 * row_annot[(size_t)r * C + c]) * 4294967296.0);
	}
	auto add = [&](uint32_t v, uint32_t c, long long s) {
		CHECK(c < C && v < V, "a flush to (%u, %u)", v, c);
		if (c >= C || v >= V) return;
		acc[an_word(v, C, c)] += (unsigned long long)xs_split_hi<ANNOT_SPLIT>(s);
		acc[an_word(v, C, c) + 1] += xs_split_lo<ANNOT_SPLIT>(s);
	};
	std::vector<double> col_a((size_t)ANNOT_SLAB * ANNOT_STRIDE), row_a((size_t)ANNOT_ROWS * ANNOT_SLAB);
	for (uint32_t slab = 0; slab < an_slabs(C); ++slab) {
		const uint32_t c0 = slab * ANNOT_SLAB;
		uint32_t row_mask[ANNOT_ROWS] = {0};
		unsigned long long col_mask[ANNOT_THREADS / 64] = {0};
		// staging, thread by thread; the ballots wave by wave
		for (uint32_t wave = 0; wave < 2; ++wave) {
			unsigned long long ballot = 0;
			for (uint32_t lane = 0; lane < 64; ++lane) {
				const uint32_t t = wave * 64 + lane, srow = t / ANNOT_SLAB, scat = t % ANNOT_SLAB;
				const double a = c0 + scat < C ? row_annot[(size_t)srow * C + c0 + scat] : 0.0;
				row_a[(size_t)srow * ANNOT_SLAB + scat] = a;
				if (a != 0.0) ballot |= 1ull << lane;
			}
			for (uint32_t lane = 0; lane < 64; lane += ANNOT_SLAB) row_mask[(wave * 64 + lane) / ANNOT_SLAB] = (uint32_t)(ballot >> (lane & 56)) & 0xFFu;
		}
		for (uint32_t t = 0; t < (uint32_t)ANNOT_THREADS; ++t) {
			bool any = false;
			for (uint32_t k = 0; k < (uint32_t)ANNOT_SLAB; ++k) {
				const double a = c0 + k < C ? col_annot[(size_t)t * C + c0 + k] : 0.0;
				col_a[(size_t)k * ANNOT_STRIDE + t] = a;
				any |= a != 0.0;
			}
			if (any) col_mask[t / 64] |= 1ull << (t % 64);
		}
		for (uint32_t t = 0; t < (uint32_t)ANNOT_THREADS; ++t) {
			// column side
			long long csum[ANNOT_SLAB] = {0};
			for (uint32_t r = 0; r < (uint32_t)ANNOT_ROWS; ++r) {
				const uint32_t m = row_mask[r];
				if (!m) continue;
				for (uint32_t k = 0; k < (uint32_t)ANNOT_SLAB; ++k)
					if (m >> k & 1u) csum[k] += at_term(stage[(size_t)r * ANNOT_STRIDE + t], row_a[(size_t)r * ANNOT_SLAB + k]);
			}
			for (uint32_t k = 0; k < (uint32_t)ANNOT_SLAB; ++k) if (csum[k]) add(ANNOT_ROWS + t, c0 + k, csum[k]);
			// row side
			const uint32_t half = an_half(t), row = an_row(t), cat = an_cat(t);
			long long rsum = 0;
			for (uint32_t word = 0; word < 2; ++word) {
				unsigned long long m = col_mask[half * 2 + word];
				while (m) {
					const uint32_t col = an_col(half, word, (uint32_t)__builtin_ffsll((long long)m) - 1u);
					m &= m - 1;
					rsum += at_term(stage[(size_t)row * ANNOT_STRIDE + col], col_a[(size_t)cat * ANNOT_STRIDE + col]);
				}
			}
			if (rsum) add(row, c0 + cat, rsum);
		}
	}
	for (uint32_t v = 0; v < V; ++v) for (uint32_t c = 0; c < C; ++c)
		CHECK(xs_join_signed<ANNOT_SPLIT>(acc[an_word(v, C, c)], acc[an_word(v, C, c) + 1]) == want[(size_t)v * C + c], "block %u x %u, %u categories: the sum of (%u, %u)", rows, cols, C, v, c);
}

}  // namespace

int main() {
	check_terms();
	xs_check_all();
	check_width<ANNOT_SPLIT>();
	check_threads();
	for (const uint32_t C : {1u, 7u, 8u, 9u, 65u}) {
		check_block(ANNOT_ROWS, ANNOT_THREADS, C, 1.0, 0.0);
		check_block(ANNOT_ROWS, ANNOT_THREADS, C, 0.5, 0.9);
		check_block(5, 77, C, 0.7, 0.5);
		check_block(ANNOT_ROWS, 129, C, 0.05, 0.95);
	}
	printf("annot-check: %lld cases, %d bad\n", cases, failures);
	return failures ? 1 : 0;
}
