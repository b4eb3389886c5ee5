// `make prefix-check`: the host side of the prefix contraction, on the CPU under AddressSanitizer and UBSan.
//   1. Soundness of the prefix screens (csrc/hip/ld_two_screen.h): every (prefix 3 x 3 genotype table, suffix 3 x 3 genotype table) of up to
//      4 + 4 samples, at the cut-offs 0.1, 0.5, 0.8 and at cut-offs on, one ulp below and one ulp above the values at which the three-product
//      screen's decision on the summed table turns.  Every pair screen3_keeps keeps on the summed table must be kept by
//      screen3_prefix_keeps and by screen2_prefix_keeps on the prefix counts with the suffix margins - and by screen2c_prefix_keeps, the
//      two-product prefix screen of a launch whose row operand is the carrier plane (CH_pre, CQ_pre), which keeps no pair the H form's drops.
//   2. The table builder with per-tile stops (csrc/hip/ld_count_table.h) against a naive restatement: every tile's units partition
//      [0, stop) exactly, every split tile lies in the zeroed range, a unit that holds a stopped tile's whole count says so (UNIT_WHOLE) and
//      no other does, and with no stops - or every stop at the row's end - the packed image is the one built without them.
//   3. The planner (csrc/hip/ld_plan.h) on the headline's law: p evenly spread over (0.05, 0.5), 1,000,000 samples, 50,000 variants in
//      allele-count order, margins and suffix margins at their expectation: the launches of the two-product walk, the stop of every tile
//      of every launch, the mean contracted fraction per launch and overall (two-product pairs at 0.66 of a three-product pair's cost).
//      Then the same walk with the carrier plane as the row operand of its two-product launches (PlanEnv::carrier): a second report, every line
//      under the prefix "carrier form:", with the cut, the steps of the walk and the count work against the first report's.
//   4. The grid of stops (csrc/hip/ld_two_screen.h prefix_stop_chunks) against a naive restatement for every row length of 1 .. 2,000 chunks:
//      the points never decrease, every coarse point is a fine point and the last point is the row's end; the suffix table's walk over segments
//      of unequal length (csrc/hip/ld_prep.hip.h k_row_suffix_popcount, restated on the host) against plain sums; and the screens of 1. on
//      rows of 129, 137 and 977 chunks cut at every fine stop - the prefix table in front of the stop, the suffix table behind it.
//   5. The planner on the headline's law at four settings, carrier form, every line under the prefix "fine grid:": the grid of 32 points with
//      margin 0.95 (the planner before the fine grid, restated here; the reports of 3. are this setting's), 128 points with 0.95, 128 points with
//      0.95 and six standard deviations (the default), 128 points with 0.98 - count work against whole H-plane rows, against the first setting,
//      and the host time of the stops.
//   6. The one-product launches of the carrier form (PlanEnv::one; csrc/hip/ld_plan.h plan_one_tiles), every line under the prefix "one product:":
//      the prefix screen of such a launch (screen1c_prefix_keeps on CC_pre) keeps every pair the carrier prefix screen keeps - part of 1. - and the
//      planner on the headline's law with the rows in front of the cut in blocks of S and of S / 2 variants: launches by form, and the count work
//      with stops against the carrier form's with stops at the default setting (a one-product tile costs what a two-product tile costs and holds
//      twice the pairs).
//   7. The fine walk (option "walk_fine"; PlanEnv::fine, PrefixEnv::fine), every line under the prefix "walk fine:": the carrier prefix screen with
//      QQ_pre <= min(qa_pre, qb_pre, CQ_pre) keeps every pair three products keep on the whole rows and none the carrier prefix screen drops - part
//      of 1. - and the planner on the headline's law, one-product blocks of S / 2, with walk_fine 0 and 1 and six, five and four and a half standard
//      deviations: the cut, two_last, the launches by form, the count work, and the ratio new / parent expected of a step.
//   8. The fine walk's plan on random het / hom tables of 300 .. 3,000 variants with p up to 0.5: every pair of the triangle lies in exactly one
//      launch's listed tiles and on that launch's side of its staircase, both staircases never rise along a block and move in steps of 128 variants,
//      and with PlanEnv::fine off the launches are the parent's - restated here from plan_one_end and plan_matrix_tiles - tile list by tile list.
// usage: prefix_check [--no-planner]
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <vector>
#include "../hip/ld_count_table.h"
#include "../hip/ld_plan.h"
#include "../hip/ld_two_screen.h"

using namespace twk;

namespace {

int g_bad_checks = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_bad_checks < 40) { fprintf(stderr, "    FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } ++g_bad_checks; } } while (0)

// ---- 1. the screens ----------------------------------------------------------------------------------------------------------
constexpr uint32_t MAX_PART = 4;
uint64_t g_tests = 0, g_kept3 = 0, g_kept3p = 0, g_kept2p = 0, g_kept2cp = 0, g_kept1cp = 0, g_kept2cfp = 0, g_violations = 0;
std::vector<std::vector<uint32_t>> g_tables;          // every 3 x 3 table of 0 .. MAX_PART samples: c[3 a + b]

void each_table(uint32_t c[9], int cell, uint32_t left) {
	if (cell == 8) { c[8] = left; g_tables.push_back(std::vector<uint32_t>(c, c + 9)); return; }
	for (uint32_t k = 0; k <= left; ++k) { c[cell] = k; each_table(c, cell + 1, left - k); }
}
void check_pair(const uint32_t* p, const uint32_t* x) {
	uint32_t c[9], n = 0;
	for (int k = 0; k < 9; ++k) { c[k] = p[k] + x[k]; n += c[k]; }
	if (!n) return;
	const ScreenMargins m{c[3] + c[4] + c[5], c[6] + c[7] + c[8], c[1] + c[4] + c[7], c[2] + c[5] + c[8]};
	const SuffixMargins sx{x[3] + x[4] + x[5], x[6] + x[7] + x[8], x[1] + x[4] + x[7], x[2] + x[5] + x[8]};
	const uint32_t hh = c[4], s = c[7] + c[5] + 2 * c[8];
	const uint32_t hh_pre = p[4], hq_pre = p[5], s_pre = p[7] + p[5] + 2 * p[8];
	const double two_n = 2.0 * n;
	// the facts the bound rests on: the suffix's S is >= 0 (unsigned), and its S + HH is at most min(dA', dB')
	const uint32_t s_suf = x[7] + x[5] + 2 * x[8], hh_suf = x[4];
	CHECK((double)(s_suf + hh_suf) <= prefix_slack(sx), "suffix S + HH = %u above min(dA', dB') = %g", s_suf + hh_suf, prefix_slack(sx));
	// the carrier form's interval over the prefix: e_lo is tested at CQ_pre, e_hi at CH_pre + CQ_pre + min(qa_pre, qb_pre) + min(dA', dB') - the true S and
	// T = S + HH of the summed table lie inside
	{
		const uint32_t ch_pre = p[4] + p[7], cq_pre = p[5] + p[8], qa_pre = m.qA - sx.qA, qb_pre = m.qB - sx.qB;
		CHECK(cq_pre <= s && (double)(s + hh) <= (double)ch_pre + (double)cq_pre + (double)std::min(qa_pre, qb_pre) + prefix_slack(sx),
		      "carrier prefix: S = %u, T = %u outside [%u, %u + %u + %u + %g]", s, s + hh, cq_pre, ch_pre, cq_pre, std::min(qa_pre, qb_pre), prefix_slack(sx));
	}
	double cuts[3 + 6]; int n_cuts = 3;
	cuts[0] = 0.1; cuts[1] = 0.5; cuts[2] = 0.8;
	const double da = m.hA + 2.0 * m.qA, ra = two_n - da, db = m.hB + 2.0 * m.qB, rb = two_n - db, denom = da * ra * db * rb;
	if (denom > 0) {
		const double n11 = (ra - db) + s;
		for (const double e : {n11 * two_n - ra * rb, (n11 + hh) * two_n - ra * rb}) {
			const double v = e * e / denom;
			if (v > 1e-6 && v <= 1.0) { cuts[n_cuts++] = std::nextafter(v, 0.0); cuts[n_cuts++] = v; cuts[n_cuts++] = std::nextafter(v, 2.0); }
		}
	}
	for (int k = 0; k < n_cuts; ++k) {
		if (cuts[k] > 1.0) continue;
		const double cut = cuts[k] * (1.0 - 1e-6);
		const bool k3 = screen3_keeps(m, hh, s, two_n, cut);
		const bool k3p = screen3_prefix_keeps(m, sx, hh_pre, s_pre, two_n, cut), k2p = screen2_prefix_keeps(m, sx, hh_pre, hq_pre, two_n, cut);
		if (k3 && !(k3p && k2p)) {
			++g_violations;
			CHECK(false, "prefix %u %u %u / %u %u %u / %u %u %u + suffix %u %u %u / %u %u %u / %u %u %u at r2 >= %.17g: kept by three products on the whole rows, prefix three %d, prefix two %d",
			      p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7], x[8], cuts[k], (int)k3p, (int)k2p);
		}
		// the carrier form over the prefix: CH_pre = HH_pre + QH_pre, CQ_pre = HQ_pre + QQ_pre - between the whole rows' three products and the H form's prefix screen
		const bool k2cp = screen2c_prefix_keeps(m, sx, p[4] + p[7], p[5] + p[8], two_n, cut);
		if ((k3 && !k2cp) || (k2cp && !k2p)) {
			++g_violations;
			CHECK(false, "prefix %u %u %u / %u %u %u / %u %u %u + suffix %u %u %u / %u %u %u / %u %u %u at r2 >= %.17g: three products on the whole rows %d, carrier prefix %d, H prefix %d",
			      p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7], x[8], cuts[k], (int)k3, (int)k2cp, (int)k2p);
		}
		// the fine walk's carrier prefix screen: QQ_pre <= CQ_pre as well - between the whole rows' three products and the carrier prefix screen
		const bool k2cfp = screen2c_prefix_keeps(m, sx, p[4] + p[7], p[5] + p[8], two_n, cut, true);
		if ((k3 && !k2cfp) || (k2cfp && !k2cp)) {
			++g_violations;
			CHECK(false, "prefix %u %u %u / %u %u %u / %u %u %u + suffix %u %u %u / %u %u %u / %u %u %u at r2 >= %.17g: three products on the whole rows %d, fine carrier prefix %d, carrier prefix %d",
			      p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7], x[8], cuts[k], (int)k3, (int)k2cfp, (int)k2cp);
		}
		g_kept2cfp += k2cfp;
		// one product over the prefix: CC_pre = CH_pre + CQ_pre, the lower test at S >= 0 - every pair the carrier prefix screen keeps
		const bool k1cp = screen1c_prefix_keeps(m, sx, p[4] + p[7] + p[5] + p[8], two_n, cut);
		if ((k3 && !k1cp) || (k2cp && !k1cp)) {
			++g_violations;
			CHECK(false, "prefix %u %u %u / %u %u %u / %u %u %u + suffix %u %u %u / %u %u %u / %u %u %u at r2 >= %.17g: three products on the whole rows %d, carrier prefix %d, one-product prefix %d",
			      p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7], x[8], cuts[k], (int)k3, (int)k2cp, (int)k1cp);
		}
		++g_tests; g_kept3 += k3; g_kept3p += k3p; g_kept2p += k2p; g_kept2cp += k2cp; g_kept1cp += k1cp;
	}
}
int check_screens() {
	const int before = g_bad_checks;
	for (uint32_t n = 0; n <= MAX_PART; ++n) { uint32_t c[9]; each_table(c, 0, n); }
	for (const auto& p : g_tables) for (const auto& x : g_tables) check_pair(p.data(), x.data());
	// a stop at the row's end is the screen itself
	for (const auto& p : g_tables) {
		const uint32_t* c = p.data();
		uint32_t n = 0; for (int k = 0; k < 9; ++k) n += c[k];
		if (!n) continue;
		const ScreenMargins m{c[3] + c[4] + c[5], c[6] + c[7] + c[8], c[1] + c[4] + c[7], c[2] + c[5] + c[8]};
		const SuffixMargins none{0, 0, 0, 0};
		for (const double r2 : {0.1, 0.5, 0.8}) {
			const double cut = r2 * (1.0 - 1e-6);
			CHECK(screen3_prefix_keeps(m, none, c[4], c[7] + c[5] + 2 * c[8], 2.0 * n, cut) == screen3_keeps(m, c[4], c[7] + c[5] + 2 * c[8], 2.0 * n, cut), "empty suffix, three");
			CHECK(screen2_prefix_keeps(m, none, c[4], c[5], 2.0 * n, cut) == screen2_keeps(m, c[4], c[5], 2.0 * n, cut), "empty suffix, two");
			CHECK(screen2c_prefix_keeps(m, none, c[4] + c[7], c[5] + c[8], 2.0 * n, cut) == screen2c_keeps(m, c[4] + c[7], c[5] + c[8], 2.0 * n, cut), "empty suffix, carrier");
			CHECK(screen2c_prefix_keeps(m, none, c[4] + c[7], c[5] + c[8], 2.0 * n, cut, true) == screen2c_keeps(m, c[4] + c[7], c[5] + c[8], 2.0 * n, cut, true), "empty suffix, fine carrier");
			CHECK(screen1c_prefix_keeps(m, none, c[4] + c[7] + c[5] + c[8], 2.0 * n, cut) == screen1c_keeps(m, c[4] + c[7] + c[5] + c[8], 2.0 * n, cut), "empty suffix, one product");
		}
	}
	return g_bad_checks != before;
}

// ---- 2. the table builder with stops -----------------------------------------------------------------------------------------
struct Case { uint32_t nA, nB; bool diag; uint32_t nchunks; int PA; CountSettings s; };
struct HashStops {       // a stop per tile from its coordinates: 1 .. nchunks, a fifth of the tiles at the row's end
	uint32_t nchunks;
	uint32_t operator()(uint32_t yx) const {
		uint32_t h = yx * 2654435761u; h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
		return h % 5 == 0 ? nchunks : 1 + h % nchunks;
	}
};
struct FullStops { uint32_t nchunks; uint32_t operator()(uint32_t) const { return nchunks; } };
int check_table_case(const Case& c) {
	const int before = g_bad_checks;
	twk_hip_tile_desc t{};
	t.rowA0 = 384; t.rowB0 = c.diag ? 384 : 1000; t.nA = c.nA; t.nB = c.nB; t.diag = c.diag ? 1 : 0;
	const HashStops hs{c.nchunks};
	std::vector<uint32_t> stops;
	const CountTable tb = build_count_table(t, 2, c.diag, nullptr, c.nchunks, c.s, c.PA, &hs, &stops);
	const CountTable plain = build_count_table(t, 2, c.diag, nullptr, c.nchunks, c.s, c.PA);
	const uint32_t T = tb.n_tiles(), U = tb.n_units();
	CHECK(tb.tiles == plain.tiles && stops.size() == T, "the tile list does not depend on the stops");
	std::vector<std::vector<std::pair<uint32_t, uint32_t>>> of(T);
	std::vector<int> flagged(T, 0);
	for (uint32_t u = 0; u < U; ++u) {
		const CountUnit& cu = tb.units[u];
		const uint32_t tile = cu.tile & ~UNIT_WHOLE;
		CHECK(tile < T && cu.c0 < cu.c1 && cu.c1 <= c.nchunks, "unit %u = tile %u [%u, %u)", u, tile, cu.c0, cu.c1);
		if (tile >= T) continue;
		CHECK(cu.yx == tb.tiles[tile], "unit %u yx", u);
		of[tile].push_back({cu.c0, cu.c1});
		if (cu.tile & UNIT_WHOLE) ++flagged[tile];
	}
	for (uint32_t k = 0; k < T; ++k) {
		const uint32_t stop = hs(tb.tiles[k]);
		CHECK(stops[k] == stop, "tile %u: stop %u recorded as %u", k, stop, stops[k]);
		std::sort(of[k].begin(), of[k].end());
		uint32_t at = 0;
		for (const auto& r : of[k]) { CHECK(r.first == at, "tile %u: [%u, %u) after %u", k, r.first, r.second, at); at = r.second; }
		CHECK(at == stop, "tile %u covered to %u, stop %u of %u", k, at, stop, c.nchunks);
		if (of[k].size() > 1) CHECK(k >= tb.first_split, "tile %u split before first_split %u", k, tb.first_split);
		// the kernel stores a unit's counts when it is flagged or covers [0, nchunks), and adds them otherwise: stored exactly when the unit is the tile's only one
		const bool stored = of[k].size() == 1 && (flagged[k] || of[k][0].second == c.nchunks);
		CHECK(stored == (of[k].size() == 1) && flagged[k] == ((of[k].size() == 1 && stop < c.nchunks) ? 1 : 0), "tile %u: %zu units, stop %u, %d flagged", k, of[k].size(), stop, flagged[k]);
	}
	// every stop at the row's end: the image of the table built without stops
	const FullStops fs{c.nchunks};
	const CountTable full = build_count_table(t, 2, c.diag, nullptr, c.nchunks, c.s, c.PA, &fs);
	std::vector<uint32_t> a(full.words() + 1, 0), b(plain.words() + 1, 0);
	full.pack(a.data()); plain.pack(b.data());
	CHECK(full.words() == plain.words() && a == b && full.first_split == plain.first_split && full.n_queues == plain.n_queues, "stops at the row's end change the table");
	for (int q = 0; q <= 8; ++q) CHECK(full.queue_begin[q] == plain.queue_begin[q], "queue %d", q);
	return g_bad_checks != before;
}
int check_tables(int& n_cases) {
	auto settings = [](uint32_t nb, uint32_t mc, uint32_t pr, uint32_t pc) { CountSettings s; s.n_blocks = nb; s.min_chunks = mc; s.patch_rows = pr; s.patch_cols = pc; return s; };
	static const uint32_t SHAPES[7][2] = {{5, 9}, {100, 30}, {130, 130}, {200, 200}, {256, 256}, {700, 700}, {1100, 2300}};
	int bad = 0;
	for (const int PA : {0, 1}) for (const auto& sh : SHAPES) for (const bool diag : {false, true}) {
		if (diag && sh[1] < sh[0]) continue;
		bad += check_table_case(Case{sh[0], sh[1], diag, 137, PA, settings(512, 8, 8, 8)});      // whole tiles mostly
		bad += check_table_case(Case{sh[0], sh[1], diag, 300, PA, settings(4, 8, 8, 8)});        // a guided tail of K-split units
		bad += check_table_case(Case{sh[0], sh[1], diag, 137, PA, settings(4, 1, 8, 8)});        // ... down to single chunks
		bad += check_table_case(Case{sh[0], sh[1], diag, 17, PA, settings(1, 1, 16, 32)});       // one block: every tile split
		n_cases += 4;
	}
	return bad;
}

// ---- 3. the planner on the headline's law --------------------------------------------------------------------------------------
// carrier: the second report - the walk's two-product launches contract the carrier plane.  Its lines carry a prefix of their own and the word
// "step" where the first report says "launch" (tests/test_prefix_cpu.py reads the first report by its lines).  -> the count work with stops, in
// three-product tile chunks; *two_end: the cut.
// The planner before the fine grid, restated: the 32 coarse points only, each pair walked from its neighbour's answer, one coarse step added.
struct CoarseTileStops {
	const PrefixEnv* e; bool two; uint32_t a0, b0, nA, nB; mutable uint32_t hint[5];
	uint32_t need(uint32_t vA, uint32_t vB, uint32_t h) const {
		uint32_t g = std::min<uint32_t>(std::max<uint32_t>(h, 1), PREFIX_COARSE);
		while (g > 1 && e->dropped(two, vA, vB, (g - 1) * PREFIX_SUB)) --g;
		while (g < PREFIX_COARSE && !e->dropped(two, vA, vB, g * PREFIX_SUB)) ++g;
		return g;
	}
	uint32_t operator()(uint32_t yx) const {
		const uint32_t y = yx >> 16, x = yx & 0xFFFFu, ta = two ? PLAN_TILE : PLAN_TILE / 2, tb = PLAN_TILE / 2;
		if (!(y * ta < nA && x * tb < nB)) return e->nchunks;
		const uint32_t a_lo = a0 + y * ta, a_hi = std::min(a0 + std::min(nA, (y + 1) * ta) - 1, e->n_variants - 1);
		const uint32_t b_lo = b0 + x * tb, b_hi = std::min(b0 + std::min(nB, (x + 1) * tb) - 1, e->n_variants - 1);
		if (a_lo > a_hi || b_lo > b_hi || b_lo <= a_hi) return e->nchunks;
		const uint32_t pa[5] = {a_lo, a_lo, a_hi, a_hi, a_lo + (a_hi - a_lo) / 2}, pb[5] = {b_lo, b_hi, b_lo, b_hi, b_lo + (b_hi - b_lo) / 2};
		uint32_t g = 1;
		for (int k = 0; k < 5; ++k) { hint[k] = need(pa[k], pb[k], hint[k]); g = std::max(g, hint[k]); }
		return prefix_stop_chunks(std::min<uint32_t>(g + 1, PREFIX_COARSE) * PREFIX_SUB, e->nchunks);
	}
};
// fine: the planner of ld_plan.h on the grid of 128; else CoarseTileStops.  quiet: no report, only the work (section 5).
// walk: the fine walk (PlanEnv::fine, PrefixEnv::fine) - section 7.
struct Setting { bool fine; double margin, sigma; bool walk = false; };
constexpr Setting HEAD_SETTING{false, 0.95, 0.0};
double play_planner(bool carrier, uint32_t* two_end, double h_work = 0, uint32_t h_two_end = 0, const Setting& st = HEAD_SETTING, bool quiet = false,
                    double* work_whole = nullptr, double* stops_ms = nullptr, std::vector<double>* fractions = nullptr, int one_rows = -1, uint32_t* launches = nullptr, uint32_t* two_last = nullptr) {
	const char* tag = carrier ? "carrier form: " : "planner: ";
	const uint32_t M = 50000, N = 1000000, nchunks = (N + 1023) / 1024;
	const double minR2 = 0.1, cut = minR2 * (1.0 - 1e-6), two_cost = 0.66;
	std::vector<uint32_t> het(M), hom(M), suffix((size_t)2 * M * PREFIX_GRID);
	for (uint32_t v = 0; v < M; ++v) {
		const double p = 0.05 + 0.45 * (v + 0.5) / M;
		het[v] = (uint32_t)std::llround(2 * p * (1 - p) * N); hom[v] = (uint32_t)std::llround(p * p * N);
		for (uint32_t g = 0; g < PREFIX_GRID; ++g) {
			const double behind = 1.0 - std::min<double>((double)prefix_stop_chunks(g, nchunks) * 1024.0, N) / N;
			suffix[(size_t)(2 * v) * PREFIX_GRID + g] = (uint32_t)std::llround(het[v] * behind);
			suffix[(size_t)(2 * v + 1) * PREFIX_GRID + g] = (uint32_t)std::llround(hom[v] * behind);
		}
	}
	PlanEnv env; env.n_samples = N; env.Pmax = 2; env.nchunks = nchunks; env.minR2 = minR2; env.phased_math = false; env.het = het.data(); env.hom = hom.data(); env.carrier = carrier;
	env.fine = st.walk;
	env.one = carrier && one_rows >= 0; env.one_rows = one_rows > 0 ? (uint32_t)one_rows : 0;      // (section 6: the one-product launches of the carrier form)
	const PlanGeom g{0, M, 0, M, 1, 0, 1, 0, 0, 0};
	RegionPlan plan;
	plan_region(env, g, plan);
	PrefixEnv pe; pe.het = het.data(); pe.hom = hom.data(); pe.suffix = suffix.data(); pe.n_variants = M; pe.n_samples = N; pe.nchunks = nchunks; pe.cut = cut; pe.margin = st.margin; pe.sigma = st.sigma; pe.carrier = carrier; pe.fine = st.walk;
	*two_end = plan.two_end;
	if (two_last) *two_last = plan.two_last;
	StairRanges stairs; stairs.set(plan, g, nullptr);
	if (!quiet) printf("%s%u variants x %u samples, r2 >= %g, rows of %u chunks, grid step %u chunks; two-product cut at sorted row %u (p = %.3f); %zu %s\n",
	       tag, M, N, minR2, nchunks, prefix_step(nchunks), plan.two_end, 0.05 + 0.45 * plan.two_end / M, plan.mine.size(), carrier ? "steps" : "launches");
	CountSettings cs;
	double work_full = 0, work_done = 0, sum2_full = 0, sum2_done = 0, sum3_full = 0, sum3_done = 0, host_ms = 0;
	uint64_t n_tiles = 0;
	for (size_t i = 0; i < plan.mine.size(); ++i) {
		const twk_hip_tile_desc& t = plan.mine[i];
		const bool two = t.rowA0 + t.nA <= plan.two_end || plan.notes[i].behind, diag = t.diag && t.rowA0 == t.rowB0;
		const ColRange* cr = stairs.of(plan, i);
		const bool one = two && t.one != 0;
		const int P = one ? 1 : 2;
		pe.one = one;
		if (launches) { ++launches[0]; launches[1] += one ? 1 : 0; launches[2] += two ? 1 : 0; }
		const Geometry geo = tile_geometry(P, t, two ? 1 : 0);
		std::vector<uint8_t> grid((size_t)geo.gy * geo.gx, (uint8_t)PREFIX_GRID);
		std::vector<uint32_t> stops;
		const PrefixTileStops stop_of{&pe, two, t.rowA0, t.rowB0, t.nA, t.nB, geo.gx, &grid, {PREFIX_GRID, PREFIX_GRID, PREFIX_GRID, PREFIX_GRID, PREFIX_GRID}};
		const CoarseTileStops coarse_of{&pe, two, t.rowA0, t.rowB0, t.nA, t.nB, {PREFIX_COARSE, PREFIX_COARSE, PREFIX_COARSE, PREFIX_COARSE, PREFIX_COARSE}};
		const auto t0 = std::chrono::steady_clock::now();
		const CountTable tb = st.fine ? build_count_table(t, P, diag, cr, nchunks, cs, two ? 1 : 0, &stop_of, &stops)
		                              : build_count_table(t, 2, diag, cr, nchunks, cs, two ? 1 : 0, &coarse_of, &stops);
		const auto t1 = std::chrono::steady_clock::now();
		const CountTable plain = build_count_table(t, P, diag, cr, nchunks, cs, two ? 1 : 0);
		const auto t2 = std::chrono::steady_clock::now();
		host_ms += std::chrono::duration<double, std::milli>(t1 - t0).count() - std::chrono::duration<double, std::milli>(t2 - t1).count();
		uint64_t done = 0; uint32_t lo = nchunks, hi = 0;
		for (const uint32_t s : stops) { done += s; lo = std::min(lo, s); hi = std::max(hi, s); }
		const uint64_t full = (uint64_t)tb.n_tiles() * nchunks;
		n_tiles += tb.n_tiles();
		if (fractions) fractions->push_back(full ? (double)done / (double)full : 0.0);
		if (!quiet) printf(carrier ? "  carrier form: step %2zu  %s  rows %5u+%-5u cols %5u+%-5u  %6u tiles  stops %3u .. %3u chunks  contracted %.4f of the rows\n" :
		       "  launch %2zu  %s  rows %5u+%-5u cols %5u+%-5u  %6u tiles  stops %3u .. %3u chunks  contracted %.4f of the rows\n", i, two ? "two  " : "three", t.rowA0, t.nA, t.rowB0, t.nB,
		       tb.n_tiles(), lo, hi, full ? (double)done / (double)full : 0.0);
		// (a two-product tile holds 128 x 64 variant pairs, a three-product tile 64 x 64: per tile and chunk twice the pairs at two_cost each; a one-product
		// tile holds 128 x 128 and runs the same kernel over the same 128 x 128 rows as a two-product tile: the same cost per tile and chunk)
		const double w = two ? 2.0 * two_cost : 1.0;
		work_full += w * (double)full; work_done += w * (double)done;
		(two ? sum2_full : sum3_full) += (double)full; (two ? sum2_done : sum3_done) += (double)done;
	}
	const double all_full = sum2_full * 2.0 * two_cost + sum3_full, all_pairs = 2.0 * sum2_full + sum3_full;
	if (work_whole) *work_whole = work_full;
	if (stops_ms) *stops_ms = host_ms;
	if (quiet) return work_done;
	printf(carrier ? "carrier form: two-product steps %.1f %% of the pairs (%.1f %% of the whole rows' count work), mean fraction of the row contracted %.4f; three-product steps %.1f %% of the pairs (%.1f %%), mean fraction %.4f\n" :
	       "planner: two-product launches %.1f %% of the pairs (%.1f %% of today's count work), mean fraction of the row contracted %.4f; three-product launches %.1f %% of the pairs (%.1f %%), mean fraction %.4f\n",
	       100.0 * 2.0 * sum2_full / all_pairs, 100.0 * sum2_full * 2.0 * two_cost / all_full, sum2_full ? sum2_done / sum2_full : 0.0,
	       100.0 * sum3_full / all_pairs, 100.0 * sum3_full / all_full, sum3_full ? sum3_done / sum3_full : 0.0);
	if (!carrier)
		printf("planner: count work %.4f of today's (two-product pairs at %.2f of a three-product pair); %" PRIu64 " tiles, the stops cost %.1f ms of host time a call on this machine\n",
		       work_full ? work_done / work_full : 0.0, two_cost, n_tiles, host_ms);
	else
		printf("carrier form: rows in front of the cut %u (H plane: %u); count work with stops %.4f of the H plane's with stops (two-product pairs at %.2f of a three-product pair); %" PRIu64 " tiles\n",
		       plan.two_end, h_two_end, h_work > 0 ? work_done / h_work : 0.0, two_cost, n_tiles);
	return work_done;
}

// ---- 4. the grid of stops ------------------------------------------------------------------------------------------------------
uint32_t naive_stop(uint32_t f, uint32_t nchunks) {       // the definition in words: coarse interval g, sub-step s, clipped at the next coarse point and at the row's end
	if (f >= 128) return nchunks;
	const uint32_t step = (nchunks + 31) / 32, sub = (step + 3) / 4, g = f / 4, s = f % 4;
	uint64_t at = (uint64_t)g * step + s * sub;
	at = std::min<uint64_t>(at, (uint64_t)(g + 1) * step);
	return (uint32_t)std::min<uint64_t>(at, nchunks);
}
int check_grid() {
	const int before = g_bad_checks;
	static_assert(PREFIX_GRID == 128 && PREFIX_COARSE == 32 && PREFIX_SUB == 4, "the grid the checks below restate");
	for (uint32_t n = 1; n <= 2000; ++n) {
		CHECK(prefix_stop_chunks(0, n) == 0 && prefix_stop_chunks(PREFIX_GRID, n) == n && prefix_stop_chunks(PREFIX_GRID + 7, n) == n, "%u chunks: ends", n);
		for (uint32_t f = 0; f < PREFIX_GRID; ++f) {
			const uint32_t at = prefix_stop_chunks(f, n);
			CHECK(at == naive_stop(f, n), "%u chunks: point %u at %u, naive %u", n, f, at, naive_stop(f, n));
			CHECK(at <= prefix_stop_chunks(f + 1, n) && at <= n, "%u chunks: point %u at %u, the next at %u", n, f, at, prefix_stop_chunks(f + 1, n));
		}
		// every coarse point (the grid of 32 before the fine one: min(g step, nchunks)) is the fine point 4 g
		for (uint32_t g = 0; g <= PREFIX_COARSE; ++g)
			CHECK(prefix_stop_chunks(g * PREFIX_SUB, n) == (uint32_t)std::min<uint64_t>((uint64_t)g * ((n + 31) / 32), n), "%u chunks: coarse point %u", n, g);
		// the suffix table's walk (k_row_suffix_popcount: a lane meets the chunks c, c + 8, .. and moves its segment up), one count per chunk:
		// segment sums -> suffix sums against plain sums
		for (uint32_t lane8 = 0; lane8 < 8; lane8 += 7) {
			uint32_t f = 0, next = prefix_stop_chunks(1, n);
			for (uint32_t c = lane8; c < n; c += 8) {
				while (f + 1 < PREFIX_GRID && next <= c) { ++f; next = prefix_stop_chunks(f + 1, n); }
				CHECK(prefix_stop_chunks(f, n) <= c && c < prefix_stop_chunks(f + 1, n), "%u chunks: chunk %u put into segment %u = [%u, %u)", n, c, f, prefix_stop_chunks(f, n), prefix_stop_chunks(f + 1, n));
			}
		}
	}
	// the screens at every fine stop of a row: sparse random genotypes per chunk (one sample a chunk), prefix table in front of the stop, suffix table behind
	uint64_t rng = 12345;
	auto next_u = [&]() { rng = rng * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rng >> 33); };
	const uint64_t tests_before = g_tests;
	for (const uint32_t n : {129u, 137u, 977u}) for (int rep = 0; rep < 6; ++rep) {
		std::vector<uint8_t> cell(n);
		for (uint32_t c = 0; c < n; ++c) {
			const uint32_t r = next_u() % 100;
			const bool linked = rep % 2 == 1 && c >= n / 2;      // (LD that lies in the back half of the row)
			const uint32_t ga = r < 80 ? 0 : r < 95 ? 1 : 2, gb = linked ? ga : (next_u() % 100 < 85 ? 0 : next_u() % 3);
			cell[c] = (uint8_t)(3 * ga + gb);
		}
		for (uint32_t f = 0; f <= PREFIX_GRID; ++f) {
			uint32_t p[9] = {0}, x[9] = {0};
			const uint32_t stop = prefix_stop_chunks(f, n);
			for (uint32_t c = 0; c < n; ++c) ++(c < stop ? p : x)[cell[c]];
			check_pair(p, x);
		}
	}
	printf("prefix-check: grid of stops: rows of 1 .. 2000 chunks against the naive restatement, %" PRIu64 " screen tests at fine stops of rows of 129, 137, 977 chunks\n", g_tests - tests_before);
	return g_bad_checks != before;
}

// ---- 5. the planner at four settings -----------------------------------------------------------------------------------------------
void report_settings() {
	struct Row { const char* name; Setting st; } rows[4] = {
		{"32 points, margin 0.95 (before the fine grid)", {false, 0.95, 0.0}}, {"128 points, margin 0.95", {true, 0.95, 0.0}},
		{"128 points, margin 0.95 or 6 sigma (the default)", {true, 0.95, 6.0}}, {"128 points, margin 0.98", {true, 0.98, 0.0}}};
	double head = 0;
	for (int k = 0; k < 4; ++k) {
		uint32_t h_end = 0, c_end = 0;
		double whole = 0, ms_h = 0, ms_c = 0;
		std::vector<double> frac;
		const double h_work = play_planner(false, &h_end, 0, 0, rows[k].st, true, &whole, &ms_h);
		const double c_work = play_planner(true, &c_end, h_work, h_end, rows[k].st, true, nullptr, &ms_c, &frac);
		if (k == 0) head = c_work;
		printf("fine grid: %-50s H-form work %.4f of whole rows, x carrier form %.4f = %.4f; against the first setting %.4f; stops %.1f ms of host time a call\n",
		       rows[k].name, h_work / whole, c_work / h_work, c_work / whole, c_work / head, ms_c);
		if (k == 2) {
			printf("fine grid: the default's fraction of the rows contracted, walk step by walk step:");
			for (const double f : frac) printf(" %.4f", f);
			printf("\nfine grid: prediction new / before %.4f\n", c_work / head);
		}
		if (k > 0) CHECK(c_work < head, "setting %d: work %g against %g", k, c_work, head);
	}
}

// ---- 6. the one-product launches ---------------------------------------------------------------------------------------------------
void report_one_product() {
	const Setting dflt{true, 0.95, 6.0};
	uint32_t c_end = 0;
	const double c_work = play_planner(true, &c_end, 0, 0, dflt, true);
	double best = 0;
	for (const int rows : {8192, 4096}) {
		uint32_t end = 0, n[3] = {0, 0, 0};
		const double w = play_planner(true, &end, 0, 0, dflt, true, nullptr, nullptr, nullptr, rows, n);
		printf("one product: rows in front of the cut %u in blocks of %d (%s): %u launches, %u of them one-product and %u two-product in front of the cut; count work with stops %.4f of the carrier form's with stops\n",
		       end, rows, rows == 8192 ? "S" : "S / 2", n[0], n[1], n[2] - n[1], w / c_work);
		CHECK(end == c_end && n[1] > 0 && w < c_work, "blocks of %d: cut %u against %u, %u one-product launches, work %g against %g", rows, end, c_end, n[1], w, c_work);
		if (rows == 4096) best = w;
	}
	printf("one product: prediction new / parent %.4f (blocks of S / 2, the default)\n", best / c_work);
}

// ---- 7. the fine walk ----------------------------------------------------------------------------------------------------------------
// The step's time outside the two count kernels (screens, recount, math, sort, delivery: profiles/sample_ladder_ab.txt) and inside them, in ms.
constexpr double STEP_OTHER_MS = 31.0, STEP_COUNT_MS = 2563.0;
void report_walk_fine() {
	struct Row { const char* name; Setting st; } rows[4] = {
		{"walk_fine 0, 6 sigma (the parent's plan)", {true, 0.95, 6.0, false}}, {"walk_fine 1, 6 sigma", {true, 0.95, 6.0, true}},
		{"walk_fine 1, 5 sigma", {true, 0.95, 5.0, true}}, {"walk_fine 1, 4.5 sigma", {true, 0.95, 4.5, true}}};
	double parent = 0;
	for (int k = 0; k < 4; ++k) {
		uint32_t end = 0, last = 0, n[3] = {0, 0, 0};
		double whole = 0;
		const double w = play_planner(true, &end, 0, 0, rows[k].st, true, &whole, nullptr, nullptr, 4096, n, &last);
		if (k == 0) parent = w;
		printf("walk fine: %-42s two_end %u (p = %.4f), two_last %u (p = %.4f); %u launches: %u one-product, %u two-product, %u three-product; count work %.4f of whole rows in these forms, %.4f of the parent's; a step %.4f of the parent's\n",
		       rows[k].name, end, 0.05 + 0.45 * end / 50000.0, last, 0.05 + 0.45 * last / 50000.0, n[0], n[1], n[2] - n[1], n[0] - n[2], w / whole, w / parent,
		       (STEP_COUNT_MS * w / parent + STEP_OTHER_MS) / (STEP_COUNT_MS + STEP_OTHER_MS));
		if (k > 0) CHECK(w < parent, "setting %d: work %g against the parent's %g", k, w, parent);
	}
}

// ---- 8. the fine walk's plan: exact cover ------------------------------------------------------------------------------------------
struct CoverStats { uint64_t plans = 0, pairs = 0, side_launches = 0, behind_launches = 0, stair_steps = 0, parent_equal = 0; };
// The parent's launches of the rows in front of the cut, restated: one border a block, from the block's last row.
void parent_front(const PlanEnv& e, const PlanGeom& g, const RegionPlan& p, uint32_t xa, uint32_t xb, std::vector<twk_hip_tile_desc>& out) {
	const uint32_t H = plan_one_rows(e, p.S), nB = g.nB;
	for (uint32_t x = xa; x < xb; x += H) {
		const uint32_t h = std::min(H, xb - x), last = x + h - 1;
		uint32_t w = 0;
		if (last + 1 < nB && (h < 2 || plan_one_lower_ok(e, g, x, x + 1))) {
			const uint32_t end = plan_one_end(e, g, last);
			if (end >= std::min(x + h, nB) && end > last + 1) w = end >= nB ? nB - x : std::max(h, (end - x) / PLAN_TILE * PLAN_TILE);
		}
		const uint64_t rows = plan_round_up(h, PLAN_TILE);
		const uint32_t w_max = (uint32_t)std::max<uint64_t>(h, std::min<uint64_t>(32768, ((1ull << 27) / rows) / PLAN_TILE * PLAN_TILE));
		uint32_t col = x;
		for (bool diag = true; col < x + w; diag = false) {
			const uint32_t wl = std::min(w_max, x + w - col);
			plan_push_tile(e, g, out, x, h, col, wl, diag ? 1 : 0);
			out.back().one = 1;
			col += wl;
		}
		if (!w) { plan_matrix_tiles(e, g, p, x, x + h, out, h); continue; }
		if (col < nB) {
			const uint32_t rest = nB - col, n_l = (rest + w_max - 1) / w_max, step = plan_round_up((rest + n_l - 1) / n_l, PLAN_TILE / 2);
			for (; col < nB; col += step) plan_push_tile(e, g, out, x, h, col, std::min(step, nB - col), 0);
		}
	}
}
void check_cover_case(uint32_t M, uint32_t N, double p_lo, double minR2, uint32_t one_rows, uint64_t seed, CoverStats& cs) {
	uint64_t rng = seed * 0x9E3779B97F4A7C15ull + 1;
	auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
	std::vector<std::pair<uint64_t, std::pair<uint32_t, uint32_t>>> v(M);
	for (auto& x : v) {
		const double pf = p_lo + (0.5 - p_lo) * (double)(next() % 1000003) / 1000003.0;
		const uint32_t q = (uint32_t)(pf * pf * N * (0.98 + 0.04 * (double)(next() % 1001) / 1000.0)), h = (uint32_t)(2 * pf * (1 - pf) * N * (0.98 + 0.04 * (double)(next() % 1001) / 1000.0));
		x = {(uint64_t)h + 2ull * q, {h, q}};
	}
	std::sort(v.begin(), v.end());
	std::vector<uint32_t> het(M), hom(M);
	for (uint32_t i = 0; i < M; ++i) { het[i] = v[i].second.first; hom[i] = v[i].second.second; }
	PlanEnv env; env.n_samples = N; env.Pmax = 2; env.nchunks = (N + 1023) / 1024; env.minR2 = minR2; env.phased_math = false; env.het = het.data(); env.hom = hom.data();
	env.carrier = true; env.one = true; env.one_rows = one_rows;
	const PlanGeom g{0, M, 0, M, 1, 0, 1, 0, 0, 0};
	// fine off: the parent's launches, tile list by tile list
	{
		RegionPlan p0; env.fine = false; plan_region(env, g, p0);
		std::vector<twk_hip_tile_desc> want;
		const uint32_t cut = std::min(p0.two_end, p0.r1);
		if (cut > p0.r0) parent_front(env, g, p0, p0.r0, cut, want); else plan_matrix_tiles(env, g, p0, p0.r0, cut, want);
		plan_matrix_tiles(env, g, p0, cut, p0.r1, want);
		bool same = want.size() == p0.mine.size() && p0.stair.empty() && p0.two_last == p0.two_end;
		for (size_t i = 0; same && i < want.size(); ++i) {
			same = std::memcmp(&want[i], &p0.mine[i], sizeof(twk_hip_tile_desc)) == 0 && p0.notes[i].side == 0 && p0.notes[i].behind == 0;
			if (same) {
				const bool one = want[i].one != 0, two = want[i].rowA0 + want[i].nA <= p0.two_end, diag = want[i].diag && want[i].rowA0 == want[i].rowB0;
				std::vector<uint32_t> a, b;
				build_tile_list(want[i], one ? 1 : 2, tile_geometry(one ? 1 : 2, want[i], two ? 1 : 0), diag, nullptr, a, nullptr, 8, 8, two ? 1 : 0);
				build_tile_list(p0.mine[i], one ? 1 : 2, tile_geometry(one ? 1 : 2, p0.mine[i], two ? 1 : 0), diag, StairRanges().of(p0, i), b, nullptr, 8, 8, two ? 1 : 0);
				same = a == b;
			}
		}
		CHECK(same, "M %u N %u r2 %g one_rows %u: walk_fine 0 does not reproduce the parent's launches", M, N, minR2, one_rows);
		cs.parent_equal += same;
	}
	RegionPlan p; env.fine = true; plan_region(env, g, p);
	StairRanges stairs; stairs.set(p, g, nullptr);
	CHECK(p.notes.size() == p.mine.size() && p.two_last >= p.two_end && p.two_last <= M, "notes %zu launches %zu two_end %u two_last %u", p.notes.size(), p.mine.size(), p.two_end, p.two_last);
	std::vector<uint8_t> seen((size_t)M * M, 0);
	for (size_t i = 0; i < p.mine.size(); ++i) {
		const twk_hip_tile_desc& t = p.mine[i];
		const LaunchNote nt = p.notes[i];
		const bool one = t.one != 0, two = t.rowA0 + t.nA <= p.two_end || nt.behind, diag = t.diag && t.rowA0 == t.rowB0;
		cs.side_launches += nt.side != 0; cs.behind_launches += nt.behind;
		if (nt.behind) CHECK(nt.side == 1 && diag && t.rowA0 >= p.two_end && t.rowA0 + t.nA <= p.two_last && !one, "launch %zu behind the cut: rows %u+%u, cut %u .. %u", i, t.rowA0, t.nA, p.two_end, p.two_last);
		if (nt.side) CHECK(p.stair.size() == M, "launch %zu has a side and the plan no staircase", i);
		{	// the launch's sample lies inside it and holds pairs of its own - all of the sub-tile's for a launch without a side
			uint64_t sp = 0;
			const twk_hip_tile_desc st = sample_subtile_of(p, g, i, &sp);
			CHECK(st.rowA0 >= t.rowA0 && st.rowA0 + st.nA <= t.rowA0 + t.nA && st.rowB0 >= t.rowB0 && st.rowB0 + st.nB <= t.rowB0 + t.nB && st.nA && st.nB, "launch %zu: sample %u+%u x %u+%u outside it", i, st.rowA0, st.nA, st.rowB0, st.nB);
			uint64_t have = 0; for (uint32_t a = t.rowA0; a < t.rowA0 + t.nA; ++a) { uint32_t lo, hi; p.launch_cols(g, i, a, lo, hi); have += hi - lo; }
			CHECK(sp > 0 || have == 0, "launch %zu side %u: its sample holds none of its %" PRIu64 " pairs", i, nt.side, have);
			if (!nt.side) CHECK(sp == (st.diag ? (uint64_t)st.nA * (st.nA - 1) / 2 + (uint64_t)st.nA * (st.nB - st.nA) : (uint64_t)st.nA * st.nB), "launch %zu: %" PRIu64 " pairs in a sample of %u x %u", i, sp, st.nA, st.nB);
		}
		const int P = one ? 1 : 2, PA = two ? 1 : 0;
		const uint32_t tvA = two ? TILE : TILE / 2, tvB = one ? TILE : TILE / 2;      // variants a tile holds on either axis
		const Geometry geo = tile_geometry(P, t, PA);
		std::vector<uint32_t> tiles;
		build_tile_list(t, P, geo, diag, stairs.of(p, i), tiles, nullptr, 8, 8, PA);
		for (const uint32_t yx : tiles) {
			const uint32_t y = yx >> 16, x = yx & 0xFFFFu;
			bool any = false;
			for (uint32_t a = t.rowA0 + y * tvA; a < std::min(t.rowA0 + t.nA, t.rowA0 + (y + 1) * tvA); ++a) {
				uint32_t lo, hi; p.launch_cols(g, i, a, lo, hi);      // what the screens' threads keep of the row: the rectangle, the diagonal, the launch's side
				for (uint32_t b = std::max(lo, t.rowB0 + x * tvB); b < std::min(hi, t.rowB0 + (x + 1) * tvB); ++b) { ++seen[(size_t)a * M + b]; any = true; }
			}
			// the tile is on the launch's side of the staircase: some pair of it is the launch's (no tile is contracted for nothing but the diagonal's rounding)
			CHECK(any || diag, "launch %zu side %u: tile (%u, %u) holds no pair of the launch", i, nt.side, y, x);
		}
		// every pair the launch is to decide lies in a listed tile
		std::vector<uint8_t> listed((size_t)geo.gy * geo.gx, 0);
		for (const uint32_t yx : tiles) listed[(size_t)(yx >> 16) * geo.gx + (yx & 0xFFFFu)] = 1;
		for (uint32_t a = t.rowA0; a < t.rowA0 + t.nA; ++a) {
			uint32_t lo, hi; p.launch_cols(g, i, a, lo, hi);
			for (uint32_t b = lo; b < hi; b += tvB) CHECK(listed[(size_t)((a - t.rowA0) / tvA) * geo.gx + (b - t.rowB0) / tvB], "launch %zu: pair (%u, %u) in no listed tile", i, a, b);
			if (hi > lo) CHECK(listed[(size_t)((a - t.rowA0) / tvA) * geo.gx + (hi - 1 - t.rowB0) / tvB], "launch %zu: pair (%u, %u) in no listed tile", i, a, hi - 1);
		}
		// the staircase of the launch's rows: constant over a tile row of 128 counted from the block's first row, in steps of 128 from its first column, never rising
		if (nt.side) for (uint32_t a = t.rowA0; a < t.rowA0 + t.nA; ++a) {
			const uint32_t s = p.stair[a];
			CHECK(s > a && s <= M && (s == M || (s - t.rowA0) % PLAN_TILE == 0), "row %u of block %u: border %u", a, t.rowA0, s);
			if (a > t.rowA0) { CHECK(s <= p.stair[a - 1] && ((a - t.rowA0) % PLAN_TILE == 0 || s == p.stair[a - 1]), "row %u: border %u after %u", a, s, p.stair[a - 1]); cs.stair_steps += s != p.stair[a - 1] && i + 1 < p.mine.size() && nt.side == 1 && diag; }
			// the right side of it: in front of the cut the lower test passes for the row against every column in front of the border
			if (one && s > a + 1) CHECK(plan_one_lower_ok(env, g, a, s - 1), "row %u: the lower test fails in front of its border %u", a, s);
			// (behind the cut the border is a guide asked at two rows of a tile row - with noise in the margins the question's answer need not move one way -
			// but every tile row's last row passes against its own first column: no row from two_last on is in such a launch)
			if (nt.behind && ((a + 1 - t.rowA0) % PLAN_TILE == 0 || a + 1 == t.rowA0 + t.nA) && a + 1 < M) CHECK(!plan_two_keeps(env, g, a, a + 1), "row %u, the last of its tile row: the planner's question keeps the pair with its first column", a);
		}
	}
	uint64_t bad = 0;
	for (uint32_t a = 0; a < M; ++a) for (uint32_t b = 0; b < M; ++b) bad += seen[(size_t)a * M + b] != (b > a ? 1 : 0);
	CHECK(bad == 0, "M %u N %u r2 %g one_rows %u: %" PRIu64 " pairs not in exactly one launch", M, N, minR2, one_rows, bad);
	++cs.plans; cs.pairs += (uint64_t)M * (M - 1) / 2;
}
void check_cover() {
	CoverStats cs;
	uint64_t seed = 1;
	for (const uint32_t M : {300u, 777u, 1400u, 3000u}) for (const uint32_t N : {140000u, 262184u, 1000000u}) for (const double minR2 : {0.05, 0.1})
		for (const uint32_t one_rows : {0u, 128u, 384u}) check_cover_case(M, N, M == 777 ? 0.01 : 0.05, minR2, one_rows, seed++, cs);
	printf("walk fine: plan cover: %" PRIu64 " plans, %" PRIu64 " pairs each in exactly one launch and on its side of the staircase; %" PRIu64 " launches with a side, %" PRIu64 " two-product launches behind the cut, %" PRIu64
	       " steps of a staircase; walk_fine 0 equals the parent's launches in %" PRIu64 " plans\n", cs.plans, cs.pairs, cs.side_launches, cs.behind_launches, cs.stair_steps, cs.parent_equal);
	CHECK(cs.side_launches > 0 && cs.behind_launches > 0 && cs.stair_steps > 0 && cs.parent_equal == cs.plans, "the cases hold no staircase");
}

}  // namespace

int main(int argc, char** argv) {
	const bool planner = !(argc > 1 && std::strcmp(argv[1], "--no-planner") == 0);
	const int bad_screen = check_screens();
	printf("prefix-check: screens: %zu tables of up to %u samples, %" PRIu64 " (prefix table, suffix table, cut-off) tests; three products on the whole rows keep %" PRIu64
	       ", the three-product prefix screen %" PRIu64 ", the two-product prefix screen %" PRIu64 "; violations %" PRIu64 "\n",
	       g_tables.size(), MAX_PART, g_tests, g_kept3, g_kept3p, g_kept2p, g_violations);
	int n_cases = 0;
	const int bad_tables = check_tables(n_cases);
	printf("prefix-check: table builder with stops: %d cases, %d bad\n", n_cases, bad_tables);
	printf("prefix-check: the two-product prefix screen on the carrier plane keeps %" PRIu64 " (three products on the whole rows %" PRIu64 " <= it <= the H plane's %" PRIu64 ")\n", g_kept2cp, g_kept3, g_kept2p);
	if (planner) {
		uint32_t h_end = 0, c_end = 0;
		const double h_work = play_planner(false, &h_end);
		const double c_work = play_planner(true, &c_end, h_work, h_end);
		CHECK(c_end > h_end && c_work < h_work, "carrier form: cut %u against %u, work %g against %g", c_end, h_end, c_work, h_work);
	}
	check_grid();
	if (planner) report_settings();
	printf("prefix-check: the one-product prefix screen keeps %" PRIu64 " (the carrier plane's %" PRIu64 " <= it)\n", g_kept1cp, g_kept2cp);
	if (planner) report_one_product();
	printf("prefix-check: the fine carrier prefix screen (QQ_pre <= min(qa_pre, qb_pre, CQ_pre)) keeps %" PRIu64 " (three products on the whole rows %" PRIu64 " <= it <= the carrier plane's %" PRIu64 "), pair by pair\n", g_kept2cfp, g_kept3, g_kept2cp);
	if (planner) report_walk_fine();
	check_cover();
	printf("prefix-check: %s\n", (bad_screen || bad_tables || g_bad_checks) ? "FAILED" : "ok");
	return (bad_screen || bad_tables || g_bad_checks) ? 1 : 0;
}
