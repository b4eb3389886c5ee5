// `make two-check`: the host side of the two-product form, on the CPU under AddressSanitizer and UBSan.
//   1. The screen (csrc/hip/ld_two_screen.h) over every 3 x 3 genotype table of up to MAX_N samples, at fixed cut-offs and at cut-offs on, one
//      ulp below and one ulp above the values at which the three-product screen's own decision turns: the true S lies in [S_lo, S_hi], and
//      the two-product screen keeps every pair the three-product screen keeps.  The carrier form (the row variant's H | Q as the row operand:
//      CH = HH + QH, CQ = HQ + QQ): the true S and T = S + HH lie in [CQ, .] and [., CH + CQ + min(qA, qB)], and
//      kept(three) <= kept(carrier) <= kept(H) pair by pair.  The one-product form (the carrier rows of both variants: CC = CH + CQ, lower test at
//      S >= 0): kept(carrier) <= kept(one) pair by pair, and screen1c_lower_ok is the lower half of screen1c_keeps.  The fine walk's carrier screen
//      (QQ <= min(qA, qB, CQ): screen2c_keeps with fine = true): T still lies under its upper end, and kept(three) <= kept(carrier, fine) <= kept(carrier)
//      pair by pair.
//   1b. plan_one_end (csrc/hip/ld_plan.h) on random sorted margins: the exact boundary of screen1c_lower_ok along a row's columns.
//   2. The work table of a launch whose row axis has one plane row per variant and whose column axis two (build_count_table with PA = 1,
//      csrc/hip/ld_count_table.h): tiles of 128 row variants x 64 column variants against a naive restatement - a tile is wanted when one of
//      its variant pairs is (diagonal super-tiles: a pair above the diagonal) - units that partition every tile's K range, and the recorded
//      order: one FNV-1a-64 per case in tests/golden/count_tables_two.json.
// usage: two_check <count_tables_two.json>        check
//        two_check --record                       print the file for the tables as they are built now
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include "../hip/ld_count_table.h"
#include "../hip/ld_two_screen.h"
#include "../hip/ld_plan.h"

using namespace twk;

namespace {

int g_bad_checks = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_bad_checks < 40) { fprintf(stderr, "    FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } ++g_bad_checks; } } while (0)

// ---- 1. the screen ---------------------------------------------------------------------------------------------------------
// c[3 a + b]: samples with genotype a (0 ref/ref, 1 het, 2 alt/alt) at the row variant and b at the column variant
constexpr int MAX_N = 7;
uint64_t g_tables = 0, g_kept3 = 0, g_kept2 = 0, g_kept2c = 0, g_kept1c = 0, g_kept2cf = 0;

void check_table(const uint32_t c[9], uint32_t n) {
	const ScreenMargins m{c[3] + c[4] + c[5], c[6] + c[7] + c[8], c[1] + c[4] + c[7], c[2] + c[5] + c[8]};
	const uint32_t hh = c[4], hq = c[5], qh = c[7], qq = c[8], s = qh + hq + 2 * qq;
	const double two_n = 2.0 * n;
	CHECK((double)hq <= (double)s && (double)s <= (double)hq + screen2_slack(m), "S = %u outside [%u, %u + %g]", s, hq, hq, screen2_slack(m));
	// the carrier form: e_lo is tested at S_lo = CQ, e_hi at S_hi + CH = CQ + min(qA, qB) + CH - the true S and T = S + HH lie inside, and the interval inside the H form's
	const uint32_t ch = hh + qh, cq = hq + qq;
	CHECK(cq <= s && (double)(s + hh) <= (double)ch + (double)cq + screen2c_slack(m), "carrier: S = %u, T = %u outside [%u, %u + %u + %g]", s, s + hh, cq, ch, cq, screen2c_slack(m));
	CHECK(cq >= hq && (double)ch + (double)cq + screen2c_slack(m) <= (double)hh + (double)hq + screen2_slack(m), "carrier interval outside the H form's");
	// ... and the fine walk's: QQ <= CQ, so T <= CH + CQ + min(qA, qB, CQ), an upper end no higher than the other
	CHECK((double)(s + hh) <= (double)ch + (double)cq + screen2c_slack_cq(m, (double)cq, true) && screen2c_slack_cq(m, (double)cq, true) <= screen2c_slack(m) && screen2c_slack_cq(m, (double)cq, false) == screen2c_slack(m),
	      "fine carrier: T = %u above %u + %u + %g", s + hh, ch, cq, screen2c_slack_cq(m, (double)cq, true));
	// the cut-offs at which the three-product screen's decision on this very table turns: e^2 / (da ra db rb) of its two test values
	// (without eps they are the pair's own extreme r2 values), each with its neighbours, next to fixed ones
	std::vector<double> cuts = {1e-5, 0.01, 0.1, 0.25, 0.5, 0.9, 1.0};
	const double da = m.hA + 2.0 * m.qA, ra = two_n - da, db = m.hB + 2.0 * m.qB, rb = two_n - db, denom = da * ra * db * rb;
	if (denom > 0) {
		const double n11 = (ra - db) + s;
		for (const double e : {n11 * two_n - ra * rb, (n11 + hh) * two_n - ra * rb}) {
			const double x = e * e / denom;
			if (x > 1e-6 && x <= 1.0) { cuts.push_back(std::nextafter(x, 0.0)); cuts.push_back(x); cuts.push_back(std::nextafter(x, 2.0)); }
		}
	}
	for (const double minR2 : cuts) {
		if (minR2 > 1.0) continue;
		const double cut = minR2 * (1.0 - 1e-6);
		const bool k3 = screen3_keeps(m, hh, s, two_n, cut), k2 = screen2_keeps(m, hh, hq, two_n, cut), k2c = screen2c_keeps(m, ch, cq, two_n, cut);
		CHECK((!k3 || k2c) && (!k2c || k2), "n %u table %u %u %u / %u %u %u / %u %u %u at r2 >= %.17g: three %d, carrier %d, H %d", n, c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], minR2, (int)k3, (int)k2c, (int)k2);
		const bool k2cf = screen2c_keeps(m, ch, cq, two_n, cut, true);
		CHECK((!k3 || k2cf) && (!k2cf || k2c), "n %u table %u %u %u / %u %u %u / %u %u %u at r2 >= %.17g: three %d, fine carrier %d, carrier %d", n, c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], minR2, (int)k3, (int)k2cf, (int)k2c);
		g_kept2cf += k2cf;
		CHECK(!k3 || k2, "n %u table %u %u %u / %u %u %u / %u %u %u at r2 >= %.17g: three products keep it, two drop it", n, c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], minR2);
		// one product: CC = CH + CQ and the lower test at S >= 0 - every pair the carrier screen keeps, hence every pair three products keep
		const bool k1c = screen1c_keeps(m, ch + cq, two_n, cut);
		CHECK(!k2c || k1c, "n %u table %u %u %u / %u %u %u / %u %u %u at r2 >= %.17g: carrier keeps it, one product drops it", n, c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], minR2);
		CHECK(!k3 || k1c, "n %u table %u %u %u / %u %u %u / %u %u %u at r2 >= %.17g: three products keep it, one drops it", n, c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], minR2);
		// the lower half alone: where it fails the screen keeps the pair whatever CC; where it holds the upper half decides
		CHECK(screen1c_lower_ok(m, two_n, cut) || k1c, "lower test fails and the pair is dropped");
		CHECK(!screen1c_lower_ok(m, two_n, cut) || k1c == screen_upper_keeps(m, (double)(ch + cq) + screen2c_slack(m), two_n, cut), "upper half disagrees with the screen");
		++g_tables; g_kept3 += k3; g_kept2 += k2; g_kept2c += k2c; g_kept1c += k1c;
	}
}
void each_table(uint32_t c[9], int cell, uint32_t left, uint32_t n) {
	if (cell == 8) { c[8] = left; check_table(c, n); return; }
	for (uint32_t k = 0; k <= left; ++k) { c[cell] = k; each_table(c, cell + 1, left - k, n); }
}
int check_screen() {
	const int before = g_bad_checks;
	for (uint32_t n = 1; n <= (uint32_t)MAX_N; ++n) { uint32_t c[9]; each_table(c, 0, n, n); }
	// ... and margins of the size the engine meets: S anywhere in its interval, the row variant rare or common
	for (const uint32_t n : {40000u, 1000000u})
		for (const double pa : {0.05, 0.15, 0.3}) for (const double pb : {0.05, 0.3, 0.5}) {
			const ScreenMargins m{(uint32_t)(2 * pa * (1 - pa) * n), (uint32_t)(pa * pa * n), (uint32_t)(2 * pb * (1 - pb) * n), (uint32_t)(pb * pb * n)};
			const uint32_t hh = (uint32_t)((double)m.hA * m.hB / n), hq = (uint32_t)((double)m.hA * m.qB / n);
			const uint32_t slack = (uint32_t)screen2_slack(m);
			for (uint32_t k = 0; k <= 8; ++k) for (const double minR2 : {0.001, 0.1, 0.8}) {
				const uint32_t s = hq + (uint32_t)((uint64_t)slack * k / 8);
				const double cut = minR2 * (1.0 - 1e-6);
				CHECK(!screen3_keeps(m, hh, s, 2.0 * n, cut) || screen2_keeps(m, hh, hq, 2.0 * n, cut), "n %u pa %g pb %g S %u at %g", n, pa, pb, s, minR2);
				// the carrier form at the same margins: QH + QQ = k / 8 of qA split evenly, so CH = HH + QH, CQ = HQ + QQ and S = CQ + QH + QQ
				const uint32_t q_part = (uint32_t)((uint64_t)m.qA * k / 8), qq = std::min(q_part / 2, std::min(m.qA, m.qB)), qh = q_part - qq;
				const uint32_t sc = hq + qh + 2 * qq;
				const bool k3c = screen3_keeps(m, hh, sc, 2.0 * n, cut), k2c = screen2c_keeps(m, hh + qh, hq + qq, 2.0 * n, cut), k2h = screen2_keeps(m, hh, hq, 2.0 * n, cut);
				CHECK((!k3c || k2c) && (!k2c || k2h), "carrier: n %u pa %g pb %g S %u at %g: three %d, carrier %d, H %d", n, pa, pb, sc, minR2, (int)k3c, (int)k2c, (int)k2h);
				const bool k2cf = screen2c_keeps(m, hh + qh, hq + qq, 2.0 * n, cut, true);
				CHECK((!k3c || k2cf) && (!k2cf || k2c), "fine carrier: n %u pa %g pb %g S %u at %g: three %d, fine carrier %d, carrier %d", n, pa, pb, sc, minR2, (int)k3c, (int)k2cf, (int)k2c);
			}
		}
	return g_bad_checks != before;
}

// ---- 1b. one_end ---------------------------------------------------------------------------------------------------------------
// Random margins in order of allele count (frequencies from a flat law, Hardy-Weinberg with binomial noise of our own making): plan_one_end of a
// row is the first column behind it at which screen1c_lower_ok fails - every column in front of it passes, for this row and for every row before it.
uint64_t g_one_rows = 0, g_one_pairs = 0;
int check_one_end() {
	const int before = g_bad_checks;
	uint64_t rng = 0x9E3779B97F4A7C15ull;
	auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
	for (const uint32_t n : {140000u, 1000000u}) for (const double minR2 : {0.05, 0.1, 0.3}) for (const double p_lo : {0.01, 0.05}) {
		const uint32_t M = 900;
		std::vector<std::pair<uint64_t, std::pair<uint32_t, uint32_t>>> v(M);
		for (auto& x : v) {
			const double pf = p_lo + (0.5 - p_lo) * (double)(next() % 1000003) / 1000003.0;
			const uint32_t q = (uint32_t)(pf * pf * n * (0.98 + 0.04 * (double)(next() % 1001) / 1000.0)), h = (uint32_t)(2 * pf * (1 - pf) * n * (0.98 + 0.04 * (double)(next() % 1001) / 1000.0));
			x = {(uint64_t)h + 2ull * q, {h, q}};
		}
		std::sort(v.begin(), v.end());
		std::vector<uint32_t> het(M), hom(M);
		for (uint32_t i = 0; i < M; ++i) { het[i] = v[i].second.first; hom[i] = v[i].second.second; }
		PlanEnv e; e.n_samples = n; e.minR2 = minR2; e.het = het.data(); e.hom = hom.data();
		const PlanGeom g{0, M, 0, M, 1, 0, 1, 0, 0, 0};
		for (uint32_t row = 0; row + 1 < M; row += 37) {
			const uint32_t end = plan_one_end(e, g, row);
			CHECK(end > row && end <= M, "row %u: one_end %u", row, end);
			// (a row whose test fails at once has no column in front of its one_end, and says nothing of the rows before it)
			if (end > row + 1) for (uint32_t r = 0; r <= row; r += (row > 16 ? row / 16 : 1)) for (uint32_t col = r + 1; col < end; ++col) { CHECK(plan_one_lower_ok(e, g, r, col), "n %u r2 %g: pair (%u, %u) in front of one_end %u of row %u fails", n, minR2, r, col, end, row); ++g_one_pairs; }
			for (uint32_t col = row + 1; col < end; ++col) CHECK(plan_one_lower_ok(e, g, row, col), "n %u r2 %g: pair (%u, %u) in front of one_end %u fails", n, minR2, row, col, end);
			if (end < M) CHECK(!plan_one_lower_ok(e, g, row, end), "n %u r2 %g: pair (%u, one_end %u) passes", n, minR2, row, end);
			++g_one_rows;
		}
	}
	return g_bad_checks != before;
}

// ---- 2. the work table of 1 : 2 axes ------------------------------------------------------------------------------------------
struct Case {
	uint32_t nA, nB; bool diag; uint32_t nchunks; CountSettings s;
	std::string name() const {
		char b[160];
		snprintf(b, sizeof(b), "A%u B%u %s c%u b%u m%u p%ux%u", nA, nB, diag ? "diag" : "rect", nchunks, s.n_blocks, s.min_chunks, s.patch_rows, s.patch_cols);
		return b;
	}
};
uint64_t fnv1a64(uint64_t h, const void* data, size_t n) {
	const unsigned char* p = static_cast<const unsigned char*>(data);
	for (size_t k = 0; k < n; ++k) { h ^= p[k]; h *= 1099511628211ull; }
	return h;
}
uint64_t check_case(const Case& c) {
	twk_hip_tile_desc t{};
	t.rowA0 = 384; t.rowB0 = c.diag ? 384 : 1000; t.nA = c.nA; t.nB = c.nB; t.diag = c.diag ? 1 : 0;
	const CountTable tb = build_count_table(t, 2, c.diag, nullptr, c.nchunks, c.s, 1);
	const uint32_t gy = (c.nA + TILE - 1) / TILE, gx = (2 * c.nB + TILE - 1) / TILE, T = tb.n_tiles(), U = tb.n_units();
	CHECK(tb.g.gy == gy && tb.g.gx == gx && tb.g.rowsA == gy * TILE && tb.g.ldc == gx * TILE, "grid %u x %u, ldc %u", tb.g.gy, tb.g.gx, tb.g.ldc);
	// naive: the tile (by, bx) holds the pairs of row variants [128 by, 128 by + 128) and column variants [64 bx, 64 bx + 64)
	std::vector<uint8_t> want((size_t)gy * gx, 0), seen((size_t)gy * gx, 0);
	for (uint32_t a = 0; a < c.nA; ++a) for (uint32_t b = 0; b < c.nB; ++b)
		if (!c.diag || b > a) want[(size_t)(a / TILE) * gx + b / (TILE / 2)] = 1;
	for (uint32_t k = 0; k < T; ++k) {
		const uint32_t by = tb.tiles[k] >> 16, bx = tb.tiles[k] & 0xFFFFu;
		CHECK(by < gy && bx < gx, "tile %u = (%u, %u)", k, by, bx);
		if (by < gy && bx < gx) { CHECK(!seen[(size_t)by * gx + bx], "tile (%u, %u) twice", by, bx); seen[(size_t)by * gx + bx] = 1; }
	}
	for (uint32_t by = 0; by < gy; ++by) for (uint32_t bx = 0; bx < gx; ++bx)
		CHECK(seen[(size_t)by * gx + bx] == want[(size_t)by * gx + bx], "tile (%u, %u) listed %d, wanted %d", by, bx, (int)seen[(size_t)by * gx + bx], (int)want[(size_t)by * gx + bx]);
	// units: every tile's K range partitioned, split tiles behind first_split
	std::vector<std::vector<std::pair<uint32_t, uint32_t>>> of(T);
	for (uint32_t u = 0; u < U; ++u) {
		const CountUnit& cu = tb.units[u];
		CHECK(cu.tile < T && cu.c0 < cu.c1 && cu.c1 <= c.nchunks, "unit %u = tile %u [%u, %u)", u, cu.tile, cu.c0, cu.c1);
		if (cu.tile >= T) continue;
		CHECK(cu.yx == tb.tiles[cu.tile], "unit %u yx", u);
		of[cu.tile].push_back({cu.c0, cu.c1});
	}
	bool any_split = false;
	for (uint32_t k = 0; k < T; ++k) {
		std::sort(of[k].begin(), of[k].end());
		uint32_t at = 0;
		for (const auto& r : of[k]) { CHECK(r.first == at, "tile %u: [%u, %u) after %u", k, r.first, r.second, at); at = r.second; }
		CHECK(at == c.nchunks, "tile %u covered to %u of %u", k, at, c.nchunks);
		if (of[k].size() > 1) { any_split = true; CHECK(k >= tb.first_split, "tile %u split before first_split %u", k, tb.first_split); }
	}
	if (c.nchunks >= 2 * c.s.min_chunks && c.s.n_blocks <= 4 && T) CHECK(any_split, "no tile split over %u chunks on %u blocks", c.nchunks, c.s.n_blocks);
	std::vector<uint32_t> img(tb.words() + 4, 0xA5A5A5A5u);
	tb.pack(img.data());
	for (size_t k = tb.words(); k < img.size(); ++k) CHECK(img[k] == 0xA5A5A5A5u, "pack wrote word %zu of %zu", k, tb.words());
	uint64_t h = fnv1a64(14695981039346656037ull, img.data(), tb.words() * 4);
	const uint32_t head[2] = {tb.first_split, tb.n_queues};
	h = fnv1a64(h, head, sizeof(head));
	return fnv1a64(h, tb.queue_begin, (tb.n_queues + 1) * sizeof(uint32_t));
}
std::vector<Case> all_cases() {
	auto settings = [](uint32_t nb, uint32_t mc, uint32_t pr, uint32_t pc) { CountSettings s; s.n_blocks = nb; s.min_chunks = mc; s.patch_rows = pr; s.patch_cols = pc; return s; };
	std::vector<Case> cases;
	// (row variants, column variants): a single partial tile; less than two row tiles; edges that are no tile multiples on both axes; whole tiles; many tiles
	static const uint32_t SHAPES[7][2] = {{5, 9}, {100, 30}, {130, 130}, {200, 200}, {256, 256}, {700, 700}, {1100, 2300}};
	for (const auto& sh : SHAPES) for (const bool diag : {false, true}) {
		if (diag && sh[1] < sh[0]) continue;
		cases.push_back(Case{sh[0], sh[1], diag, 16, settings(512, 8, 8, 8)});        // whole tiles
		cases.push_back(Case{sh[0], sh[1], diag, 300, settings(4, 8, 8, 8)});         // K-split units: a guided tail
		cases.push_back(Case{sh[0], sh[1], diag, 17, settings(1, 1, 16, 32)});        // one block: every tile split
	}
	return cases;
}
bool read_golden(const char* path, std::map<std::string, std::string>& out) {
	FILE* f = fopen(path, "rb");
	if (!f) return false;
	std::string text; char buf[65536]; size_t n;
	while ((n = fread(buf, 1, sizeof(buf), f)) > 0) text.append(buf, n);
	fclose(f);
	std::vector<std::string> strings;
	for (size_t at = 0; (at = text.find('"', at)) != std::string::npos;) {
		const size_t end = text.find('"', at + 1);
		if (end == std::string::npos) return false;
		strings.push_back(text.substr(at + 1, end - at - 1));
		at = end + 1;
	}
	if (strings.size() % 2) return false;
	for (size_t k = 0; k < strings.size(); k += 2) out[strings[k]] = strings[k + 1];
	return true;
}

}  // namespace

int main(int argc, char** argv) {
	const bool record = argc > 1 && std::strcmp(argv[1], "--record") == 0;
	if (argc < 2) { fprintf(stderr, "usage: two_check <count_tables_two.json> | --record\n"); return 2; }
	std::map<std::string, std::string> golden;
	if (!record && !read_golden(argv[1], golden)) { fprintf(stderr, "two-check: cannot read %s\n", argv[1]); return 2; }
	const std::vector<Case> cases = all_cases();
	int bad = 0, n = 0;
	if (record) printf("{\n");
	for (const Case& c : cases) {
		const int before = g_bad_checks;
		const uint64_t h = check_case(c);
		char hex[17]; snprintf(hex, sizeof(hex), "%016" PRIx64, h);
		bool ok = g_bad_checks == before;
		if (record) printf("\"%s\": \"%s\"%s\n", c.name().c_str(), hex, &c == &cases.back() ? "" : ",");
		else {
			const auto it = golden.find(c.name());
			if (it == golden.end()) { printf("  %s: not in the recorded file\n", c.name().c_str()); ok = false; }
			else if (it->second != hex) { printf("  %s: table %s, recorded %s\n", c.name().c_str(), hex, it->second.c_str()); ok = false; }
		}
		if (!ok && record) fprintf(stderr, "  %s: bad\n", c.name().c_str());
		bad += !ok; ++n;
	}
	if (record) printf("}\n");
	if (!record && golden.size() != cases.size()) { printf("  the recorded file holds %zu cases, not %zu\n", golden.size(), cases.size()); ++bad; }
	const int bad_screen = check_screen(); ++n; bad += bad_screen;
	fprintf(record ? stderr : stdout, "two-check: %d cases, %d bad; screen: %" PRIu64 " (table, cut-off) tests, three products kept %" PRIu64 ", two %" PRIu64 "\n",
	        n, bad, g_tables, g_kept3, g_kept2);
	fprintf(record ? stderr : stdout, "two-check: carrier screen kept %" PRIu64 " of the same tests (three products %" PRIu64 " <= carrier <= H plane %" PRIu64 ")\n", g_kept2c, g_kept3, g_kept2);
	if (!(g_kept3 <= g_kept2c && g_kept2c <= g_kept2)) return 1;
	const int bad_one = check_one_end();
	fprintf(record ? stderr : stdout, "two-check: one-product screen kept %" PRIu64 " of the same tests (carrier %" PRIu64 " <= one product); one_end exact on %" PRIu64 " rows, %" PRIu64 " pairs in front of it, %d bad\n",
	        g_kept1c, g_kept2c, g_one_rows, g_one_pairs, bad_one);
	if (g_kept1c < g_kept2c || bad_one) return 1;
	fprintf(record ? stderr : stdout, "two-check: fine carrier screen (QQ <= min(qA, qB, CQ)) kept %" PRIu64 " of the same tests (three products %" PRIu64 " <= fine carrier <= carrier %" PRIu64 "), pair by pair\n", g_kept2cf, g_kept3, g_kept2c);
	if (!(g_kept3 <= g_kept2cf && g_kept2cf <= g_kept2c)) return 1;
	return bad != 0;
}
