// The (U, Z) form of the three-product contraction on the host (make uz-check; tests/test_uz_cpu.py): the conversion the screen kernel and this check
// share (csrc/hip/ld_two_screen.h: uz_to_hh_s, uz_prefix_to_hh_s) against the products themselves -
//   * every 3 x 3 genotype table of up to 7 samples: U = popc(H_A | H_B) and Z = popc((Q_A ^ Q_B) & ~(H_A | H_B)) with the margins give the HH and S the
//     products count, and screen3_keeps decides the same on both;
//   * every pair of a prefix table and a suffix table of up to 4 + 4 samples: the prefix's (U, Z) with the totals minus the suffix margins give the prefix's
//     (HH, S), and screen3_prefix_keeps decides the same on both;
//   * bit-plane rows of 1, 31, 32, 33, 1000 and 4097 samples, zero padded to whole chunks of 32 words as the planes are, word by word as the kernel
//     counts them (ld_count_uz.hip.h), over the whole rows and over every prefix of whole words.
// Host code only, under AddressSanitizer and UBSan.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>
#include "../hip/ld_two_screen.h"

using namespace twk;

static long long g_cases = 0, g_bad = 0;
static void check(bool ok, const char* fmt, ...) {
	if (ok) return;
	if (++g_bad <= 20) { va_list ap; va_start(ap, fmt); fprintf(stderr, "uz-check: "); vfprintf(stderr, fmt, ap); fprintf(stderr, "\n"); va_end(ap); }
}

// A 3 x 3 table: n[gA][gB] samples with gA / gB alt alleles (0, 1 = het, 2 = hom-alt) at the row / column variant.
struct Table { uint32_t n[3][3]; };
struct Counts { ScreenMargins m; uint32_t hh, s, u, z; };
static Counts counts_of(const Table& t) {
	Counts c{};
	for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) {
		const uint32_t k = t.n[a][b];
		if (a == 1) c.m.hA += k;
		if (a == 2) c.m.qA += k;
		if (b == 1) c.m.hB += k;
		if (b == 2) c.m.qB += k;
		if (a == 1 && b == 1) c.hh += k;                                  // HH
		if ((a == 2 && b == 1) || (a == 1 && b == 2)) c.s += k;           // QH + HQ
		if (a == 2 && b == 2) c.s += 2 * k;                               // 2 QQ
		if (a == 1 || b == 1) c.u += k;                                   // U: either is het
		if ((a == 2) != (b == 2) && a != 1 && b != 1) c.z += k;           // Z: one is hom-alt, the other hom-ref
	}
	return c;
}
// every table of exactly n samples -> f(table)
template <class F>
static void tables_of(uint32_t n, F f) {
	Table t{};
	uint32_t* cell = &t.n[0][0];
	auto rec = [&](auto&& self, int k, uint32_t left) -> void {
		if (k == 8) { cell[8] = left; f(t); return; }
		for (uint32_t x = 0; x <= left; ++x) { cell[k] = x; self(self, k + 1, left - x); }
	};
	rec(rec, 0, n);
}

static const double CUTS[] = {0.1 * (1.0 - 1e-6), 2e-6 * (1.0 - 1e-6), 0.5 * (1.0 - 1e-6), 1.0 * (1.0 - 1e-6)};

static void check_tables() {
	for (uint32_t n = 0; n <= 7; ++n) tables_of(n, [&](const Table& t) {
		const Counts c = counts_of(t);
		const CountsHS hs = uz_to_hh_s(c.m, c.u, c.z);
		++g_cases;
		check(hs.hh == c.hh && hs.s == c.s, "n = %u: (U, Z) = (%u, %u) with margins %u %u %u %u gives (%u, %u), the products (%u, %u)", n, c.u, c.z, c.m.hA, c.m.qA, c.m.hB, c.m.qB, hs.hh, hs.s, c.hh, c.s);
		for (const double cut : CUTS) for (const uint32_t extra : {0u, 5u})      // (the table inside a larger cohort of hom-ref samples: other test values, same counts)
			check(screen3_keeps(c.m, hs.hh, hs.s, 2.0 * (n + extra), cut) == screen3_keeps(c.m, c.hh, c.s, 2.0 * (n + extra), cut), "n = %u: the screen decides differently on the converted counts", n);
	});
}

static void check_splits() {
	std::vector<Table> small;
	for (uint32_t n = 0; n <= 4; ++n) tables_of(n, [&](const Table& t) { small.push_back(t); });
	for (const Table& pre : small) {
		const Counts p = counts_of(pre);
		for (const Table& suf : small) {
			const Counts x = counts_of(suf);
			const ScreenMargins m{p.m.hA + x.m.hA, p.m.qA + x.m.qA, p.m.hB + x.m.hB, p.m.qB + x.m.qB};      // the whole rows' margins
			const SuffixMargins sx{x.m.hA, x.m.qA, x.m.hB, x.m.qB};
			const CountsHS hs = uz_prefix_to_hh_s(m, sx, p.u, p.z);
			++g_cases;
			check(hs.hh == p.hh && hs.s == p.s, "prefix (U, Z) = (%u, %u): converted (%u, %u), the prefix's products (%u, %u)", p.u, p.z, hs.hh, hs.s, p.hh, p.s);
			uint32_t n = 0;
			for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) n += pre.n[a][b] + suf.n[a][b];
			for (const double cut : CUTS)
				check(screen3_prefix_keeps(m, sx, hs.hh, hs.s, 2.0 * n, cut) == screen3_prefix_keeps(m, sx, p.hh, p.s, 2.0 * n, cut), "the prefix screen decides differently on the converted counts");
			// ... and the whole rows from the two parts' counts added up, as a tile split along K adds them
			const Counts w = counts_of([&] { Table t{}; for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) t.n[a][b] = pre.n[a][b] + suf.n[a][b]; return t; }());
			const CountsHS whole = uz_to_hh_s(m, p.u + x.u, p.z + x.z);
			check(whole.hh == w.hh && whole.s == w.s, "the parts' (U, Z) added up do not give the whole rows' (HH, S)");
		}
	}
}

static void check_rows() {
	std::mt19937 rng(20241);
	for (const uint32_t N : {1u, 31u, 32u, 33u, 1000u, 4097u}) for (int rep = 0; rep < 8; ++rep) {
		const uint32_t W = ((N + 31) / 32 + 31) / 32 * 32;      // whole chunks of 32 words, zero padded
		std::vector<uint32_t> hA(W, 0), qA(W, 0), hB(W, 0), qB(W, 0);
		const uint32_t pA = 1 + rng() % 9, pB = 1 + rng() % 9, copy = rng() % 3;      // genotype frequencies in tenths; copy: B follows A for most samples (correlated rows)
		for (uint32_t i = 0; i < N; ++i) {
			auto draw = [&](uint32_t p) { const uint32_t a = (rng() % 10 < p) + (rng() % 10 < p); return a; };
			const uint32_t gA = draw(pA), gB = (copy && rng() % 8) ? gA : draw(pB);
			if (gA == 1) hA[i / 32] |= 1u << (i % 32);
			if (gA == 2) qA[i / 32] |= 1u << (i % 32);
			if (gB == 1) hB[i / 32] |= 1u << (i % 32);
			if (gB == 2) qB[i / 32] |= 1u << (i % 32);
		}
		ScreenMargins m{};
		for (uint32_t k = 0; k < W; ++k) { m.hA += __builtin_popcount(hA[k]); m.qA += __builtin_popcount(qA[k]); m.hB += __builtin_popcount(hB[k]); m.qB += __builtin_popcount(qB[k]); }
		ScreenMargins pre{};
		uint32_t u = 0, z = 0, hh = 0, s = 0;
		for (uint32_t k = 0; k <= W; ++k) {      // the prefix of k whole words, k = W: the whole rows, padding included
			const SuffixMargins x{m.hA - pre.hA, m.qA - pre.qA, m.hB - pre.hB, m.qB - pre.qB};
			const CountsHS hs = uz_prefix_to_hh_s(m, x, u, z);
			++g_cases;
			check(hs.hh == hh && hs.s == s, "N = %u, %u words: (U, Z) = (%u, %u) converted to (%u, %u), the products (%u, %u)", N, k, u, z, hs.hh, hs.s, hh, s);
			if (k == W) { const CountsHS all = uz_to_hh_s(m, u, z); check(all.hh == hh && all.s == s, "N = %u: the whole rows", N); break; }
			const uint32_t t = hA[k] | hB[k];
			u += __builtin_popcount(t); z += __builtin_popcount((qA[k] ^ qB[k]) & ~t);
			hh += __builtin_popcount(hA[k] & hB[k]); s += __builtin_popcount(qA[k] & (hB[k] | qB[k])) + __builtin_popcount((hA[k] | qA[k]) & qB[k]);
			pre.hA += __builtin_popcount(hA[k]); pre.qA += __builtin_popcount(qA[k]); pre.hB += __builtin_popcount(hB[k]); pre.qB += __builtin_popcount(qB[k]);
		}
	}
}

int main() {
	check_tables();
	printf("uz-check: every 3 x 3 table of up to 7 samples: (U, Z) and the margins give (HH, S), the screen decides the same\n");
	check_splits();
	printf("uz-check: every prefix and suffix table of up to 4 + 4 samples: the prefix's (U, Z), the whole rows' from the parts, the prefix screen\n");
	check_rows();
	printf("uz-check: zero-padded rows of 1, 31, 32, 33, 1000 and 4097 samples, every prefix of whole words\n");
	printf("uz-check: %lld cases, %lld bad\n", g_cases, g_bad);
	return g_bad != 0;
}
