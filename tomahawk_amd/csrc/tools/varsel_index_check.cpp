// The variant selection's predicate, word counts and gather walk (csrc/hip/ld_varsel_index.h) played on the host: `make varsel-check`
// builds this file with g++ under AddressSanitizer and UBSan and runs it.
// THE PREDICATE against a straightforward restatement (long double free: the same IEEE double product and comparison, written out from
// the header's text in twk_hip.h), over random counts and over constructed rows that sit EXACTLY on a threshold - minor / obs = 1/4 with
// obs a multiple of 4, missing / N = 1/10 with N a multiple of 10, minor = min_mac, hwe = min_hwe - which must be kept, with their
// neighbours one allele or one sample to either side.
// THE COUNTS of a word against a sample-by-sample loop, with and without a mask.
// THE GATHER: per case - output rows, kept rows, row pitch - every block and every lane of k_varsel_rows' walk moves 16-byte pieces
// from a base of random words into an output with a border on either side, against an array of write counts: a case fails unless every
// piece of the output, padding rows included, was written exactly once, nothing was written outside it, no read left the base, the kept
// rows equal a row-by-row copy through the map and the padding rows are zero.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "../hip/ld_varsel_index.h"

using namespace twk;

namespace {

struct Piece { uint32_t w[4]; };
constexpr size_t BORDER = 64;                    // pieces

bool restated(uint32_t N, uint32_t het, uint32_t hom, uint32_t miss, double hwe, const VarselFilter& f) {
	const uint64_t called = (uint64_t)N - miss, obs = 2 * called, alt = (uint64_t)het + 2ull * hom;
	const uint64_t minor = std::min(alt, obs - alt);
	const bool maf_lo = (double)minor >= f.min_maf * (double)obs;
	const bool maf_hi = (double)minor <= f.max_maf * (double)obs;
	const bool mac = minor >= f.min_mac;
	const bool geno = (double)miss <= f.max_missing * (double)N;
	const bool hw = !(hwe < f.min_hwe);
	return maf_lo && maf_hi && mac && geno && hw;
}

long check_predicate(std::mt19937& rng) {
	long bad = 0, n = 0;
	const VarselFilter off{0.0, 0.5, 0u, 1.0, 0.0};
	const double mafs[] = {0.0, 0.01, 0.05, 0.1, 0.2, 0.25, 0.5}, miss_t[] = {0.0, 0.05, 0.1, 0.5, 1.0}, hwes[] = {0.0, 1e-6, 1e-3, 0.5, 1.0};
	const uint32_t macs[] = {0, 1, 2, 5, 40};
	for (int it = 0; it < 200000; ++it) {
		const uint32_t N = 1 + rng() % 400;
		const uint32_t miss = rng() % 4 == 0 ? rng() % (N + 1) : 0;
		const uint32_t called = N - miss;
		const uint32_t hom = called ? rng() % (called + 1) : 0;
		const uint32_t het = called - hom ? rng() % (called - hom + 1) : 0;
		VarselFilter f = off;
		f.min_maf = mafs[rng() % 7]; f.max_maf = mafs[rng() % 7];
		if (f.min_maf > f.max_maf) std::swap(f.min_maf, f.max_maf);
		f.min_mac = macs[rng() % 5]; f.max_missing = miss_t[rng() % 5]; f.min_hwe = hwes[rng() % 5];
		const double hwe = rng() % 8 == 0 ? hwes[rng() % 5] : (double)(rng() % 100000) / 100000.0;
		if (varsel_pass(N, het, hom, miss, hwe, f) != restated(N, het, hom, miss, hwe, f)) ++bad;
		++n;
	}
	// with everything off, everything is kept - a variant without a called sample and a NaN hwe included
	for (uint32_t N : {1u, 7u, 96u}) {
		if (!varsel_pass(N, 0, 0, N, 1.0, off)) ++bad;
		if (!varsel_pass(N, 0, 0, 0, std::numeric_limits<double>::quiet_NaN(), off)) ++bad;
		if (!varsel_pass(N, N, 0, 0, 0.0, off)) ++bad;
	}
	// the equality boundaries: kept at the threshold, dropped one step beyond it
	for (uint32_t called : {2u, 10u, 48u, 96u, 1000u}) {               // obs = 2 called is a multiple of 4
		const uint32_t obs = 2 * called, q = obs / 4;                  // minor = q: minor / obs = 0.25 exactly
		for (int side = 0; side < 2; ++side) {                         // the minor allele is ALT / REF
			auto counts = [&](uint32_t minor, uint32_t& het, uint32_t& hom) {
				const uint32_t alt = side ? obs - minor : minor;
				hom = alt / 2; het = alt - 2 * hom;
			};
			uint32_t het, hom;
			VarselFilter lo = off; lo.min_maf = 0.25;
			VarselFilter hi = off; hi.max_maf = 0.25;
			counts(q, het, hom);
			if (!varsel_pass(called, het, hom, 0, 1.0, lo) || !varsel_pass(called, het, hom, 0, 1.0, hi)) ++bad;
			if (q >= 1) { counts(q - 1, het, hom); if (varsel_pass(called, het, hom, 0, 1.0, lo) || !varsel_pass(called, het, hom, 0, 1.0, hi)) ++bad; }
			counts(q + 1, het, hom);
			if (!varsel_pass(called, het, hom, 0, 1.0, lo) || varsel_pass(called, het, hom, 0, 1.0, hi)) ++bad;
			VarselFilter mac = off; mac.min_mac = q;
			counts(q, het, hom);
			if (!varsel_pass(called, het, hom, 0, 1.0, mac)) ++bad;
			mac.min_mac = q + 1;
			if (varsel_pass(called, het, hom, 0, 1.0, mac)) ++bad;
		}
	}
	for (uint32_t N : {10u, 50u, 1000u}) {                             // missing / N = 0.1 exactly
		VarselFilter g = off; g.max_missing = 0.1;
		if (!varsel_pass(N, 0, 0, N / 10, 1.0, g) || varsel_pass(N, 0, 0, N / 10 + 1, 1.0, g)) ++bad;
		g.max_missing = 0.0;
		if (!varsel_pass(N, 0, 0, 0, 1.0, g) || varsel_pass(N, 0, 0, 1, 1.0, g)) ++bad;
	}
	{
		VarselFilter h = off; h.min_hwe = 1e-3;
		if (!varsel_pass(10, 2, 1, 0, 1e-3, h) || varsel_pass(10, 2, 1, 0, std::nextafter(1e-3, 0.0), h) || !varsel_pass(10, 2, 1, 0, 1.0, h)) ++bad;
	}
	// the range check of the thresholds
	{
		const double nan = std::numeric_limits<double>::quiet_NaN();
		if (varsel_filter_fault(off)) ++bad;
		for (VarselFilter f : {VarselFilter{-0.1, 0.5, 0, 1, 0}, VarselFilter{0, 0.6, 0, 1, 0}, VarselFilter{0.3, 0.2, 0, 1, 0}, VarselFilter{0, 0.5, 0, 1.5, 0},
		                       VarselFilter{0, 0.5, 0, 1, -1e-9}, VarselFilter{nan, 0.5, 0, 1, 0}, VarselFilter{0, nan, 0, 1, 0}, VarselFilter{0, 0.5, 0, nan, 0},
		                       VarselFilter{0, 0.5, 0, 1, nan}})
			if (!varsel_filter_fault(f)) ++bad;
	}
	std::printf("  predicate: %ld random cases and the boundaries, %ld bad\n", n, bad);
	return bad;
}

long check_counts(std::mt19937& rng) {
	long bad = 0;
	for (int it = 0; it < 100000; ++it) {
		const uint32_t x = rng();
		uint32_t m = 0;
		if (it & 1) for (int s = 0; s < 16; ++s) if (rng() % 5 == 0) m |= 3u << (2 * s);      // the layout's mask: both bits of a missing sample
		if (it % 7 == 0) m = rng();                                                           // and whatever else a caller may have uploaded
		uint32_t het = 0, hom = 0, miss = 0, h = 0, q = 0, ms = 0;
		for (int s = 0; s < 16; ++s) {
			const uint32_t a = (x >> (2 * s)) & 3u, mm = (m >> (2 * s)) & 3u;
			if (mm) ++miss; else if (a == 3u) ++hom; else if (a) ++het;
		}
		varsel_word_counts(x, m, h, q, ms);
		if (h != het || q != hom || ms != miss) ++bad;
	}
	std::printf("  word counts: %ld bad\n", bad);
	return bad;
}

struct Case { std::string name; uint32_t rows_base, w4; std::vector<uint32_t> map; };

long play(const Case& cs, std::mt19937& rng) {
	long bad = 0;
	const uint32_t n_kept = (uint32_t)cs.map.size(), w4 = cs.w4;
	const uint32_t rows_out = (n_kept + 127) / 128 * 128 + 128;
	std::vector<Piece> base((size_t)cs.rows_base * w4);
	for (Piece& p : base) for (uint32_t& w : p.w) w = rng() | 1u;                 // never zero: a padding piece cannot pass for a copy
	const VarselGather g = varsel_gather_geometry(rows_out, n_kept, w4);
	if (g.n_slots != (uint64_t)rows_out * w4 || g.n_blocks == 0 || g.n_blocks > VARSEL_MAX_BLOCKS) ++bad;
	if ((uint64_t)g.step_rows * w4 + g.step_cols != (uint64_t)g.n_blocks * VARSEL_BLOCK || g.step_cols >= w4) ++bad;
	std::vector<Piece> out(g.n_slots + 2 * BORDER, Piece{{0xDEADBEEFu, 0xDEADBEEFu, 0xDEADBEEFu, 0xDEADBEEFu}});
	std::vector<uint32_t> writes(g.n_slots + 2 * BORDER, 0);
	long outside_base = 0, outside_out = 0;
	const Piece zero{{0, 0, 0, 0}};
	for (uint32_t b = 0; b < g.n_blocks; ++b)
		for (uint32_t t = 0; t < VARSEL_BLOCK; ++t)
			varsel_gather_lane(g, b, t, cs.map.data(), zero,
			                   [&](uint32_t row, uint32_t col) {
				                   if (row >= cs.rows_base || col >= w4) { ++outside_base; return zero; }
				                   return base[(size_t)row * w4 + col];
			                   },
			                   [&](uint32_t row, uint32_t col, const Piece& x) {
				                   const int64_t at = (int64_t)BORDER + (int64_t)row * w4 + col;
				                   if (col >= w4 || at < 0 || at >= (int64_t)out.size()) { ++outside_out; return; }
				                   ++writes[(size_t)at]; out[(size_t)at] = x;
			                   });
	bad += outside_base + outside_out;
	for (size_t i = 0; i < writes.size(); ++i) {
		const bool inside = i >= BORDER && i < BORDER + g.n_slots;
		if (writes[i] != (inside ? 1u : 0u)) ++bad;
	}
	for (uint32_t r = 0; r < rows_out; ++r)
		for (uint32_t k = 0; k < w4; ++k) {
			const Piece& got = out[BORDER + (size_t)r * w4 + k];
			const Piece& want = r < n_kept ? base[(size_t)cs.map[r] * w4 + k] : zero;
			if (!std::equal(got.w, got.w + 4, want.w)) ++bad;
		}
	if (bad) std::printf("  %s: %ld bad\n", cs.name.c_str(), bad);
	return bad;
}

std::vector<uint32_t> run(uint32_t a, uint32_t b, uint32_t step = 1) { std::vector<uint32_t> v; for (uint32_t s = a; s < b; s += step) v.push_back(s); return v; }

}  // namespace

int main() {
	std::mt19937 rng(20240917u);
	long bad = check_predicate(rng) + check_counts(rng);
	std::vector<Case> cases;
	// w4: 16-byte pieces a row - a multiple of 8, since the pitch is a multiple of 32 words
	for (uint32_t w4 : {8u, 16u, 24u, 40u, 320u})
		for (uint32_t M : {1u, 127u, 128u, 129u, 140u, 161u, 1000u, 5000u}) {
			if ((uint64_t)M * w4 > 400000) continue;
			auto add = [&](const std::string& name, std::vector<uint32_t> map) {
				if (!map.empty() && map.back() < M) cases.push_back(Case{name + " of " + std::to_string(M) + " x " + std::to_string(w4), M, w4, std::move(map)});
			};
			add("everything", run(0, M));
			add("the first", {0});
			add("the last", {M - 1});
			add("every second", run(0, M, 2));
			add("rows 0..127", run(0, 128));
			add("rows 127..129", run(127, 130));
			if (M >= 129) add("the last 129", run(M - 129, M));
			for (double density : {0.01, 0.5, 0.99}) {
				std::vector<uint32_t> v;
				std::uniform_real_distribution<double> u(0.0, 1.0);
				for (uint32_t s = 0; s < M; ++s) if (u(rng) < density) v.push_back(s);
				add("random at " + std::to_string(density).substr(0, 4), v);
			}
		}
	// more slots than one pass of the largest grid covers: the lanes' stride and the unrolled tail
	cases.push_back(Case{"every third of 9000 x 320", 9000, 320, run(0, 9000, 3)});
	cases.push_back(Case{"everything of 70000 x 8", 70000, 8, run(0, 70000)});
	for (const Case& cs : cases) bad += play(cs, rng) ? 1 : 0;
	std::printf("varsel-check: %zu gather cases, %ld bad\n", cases.size(), bad);
	return bad ? 1 : 0;
}
