// The plan of one region call: which rows this shard owns, which columns every row reaches, the launches that cover them.
// Host-only arithmetic (no HIP): twk_hip.hip's region_impl builds a PlanEnv from the context, calls plan_region() and executes
// the result; twk_hip_plan_region() (include/twk_hip.h) runs the same planner on caller-supplied arrays so that it can be
// tested without a GPU (tests/test_plan.py).  Replaces the reference's chunk partition and block-pair ticker
// (lib/ld/ld_balancing.h:23-80, 176-233) for one GPU's share of the pair space.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "../../../include/twk_hip.h"
#include "ld_two_screen.h"
#include "ld_count_table.h"

namespace twk {

constexpr uint32_t PLAN_TILE = 128;                 // plane rows per block tile edge (ld_count.hip.h TILE)

struct PlanGeom {                                   // the caller's region and shard
	uint32_t a0, nA, b0, nB; int32_t triangle;
	uint32_t part, n_parts, tile_variants;
	int32_t window; uint32_t l_window;
};
struct PlanEnv {                                    // what the planner needs to know of the problem and the engine
	uint32_t n_samples = 0;
	int Pmax = 1;                                   // plane rows per variant of the widest plane set of the mode
	uint32_t nchunks = 1;                           // K chunks of a row of the first plane set
	uint32_t resident_blocks = 512;
	int screen = 0;                                 // 0: none; 1 / 2: r2 band over an allele-count-sorted set (PhasedMath / UnphasedMath)
	double minR2 = 0;
	bool fused = false;                             // launches of this mode run the fused count -> screen form (band launches possible)
	bool phased_math = true;                        // (candidate entries: 3 words, else 6)
	// per position of the region's index space (file order, or a regrouped / sorted set through `ids`)
	const twk_hip_variant_meta* meta = nullptr; const uint32_t* ids = nullptr; const uint32_t* popc = nullptr;
	// the two-product walk (an unscreened UnphasedMath call over the allele-count-sorted set, twk_hip.hip region_dispatch): het / hom = carriers
	// of either kind per position of the index space; the triangle is then cut at RegionPlan::two_end (plan_two_end)
	const uint32_t* het = nullptr; const uint32_t* hom = nullptr; double two_margin = 0.95;
	// ... the form of its launches' row operand: the carrier plane H | Q in the H plane's place (ld_two_screen.h: screen2c_*) - the cut is then asked of
	// the carrier screen and lies further on (r2 >= 0.1: p ~ 0.21 for ~ 0.16)
	bool carrier = false;
	// ... and, in front of the cut, one product a pair where the screen's lower test is decided by the dosages alone (plan_one_tiles): only with `carrier`.
	// one_rows: the height of those rows' blocks in variants (a multiple of 128; 0: the default, plan_one_rows)
	bool one = false; uint32_t one_rows = 0;
	// ... the fine walk (option "walk_fine", twk_hip.hip walk_fine_applies): the carrier screen's upper value with the counted CQ in its min
	// (ld_two_screen.h screen2c_slack_cq) - the cut is asked of that screen - and stops without the spare grid step (plan_prefix_tile_grid)
	bool fine = false;
	// ... and staircase borders inside a row block (plan_one_tiles, plan_two_stairs): only with `fine`, `carrier` and launches through a matrix.
	// stair_behind: also behind the cut (the caller takes it back where it has no carrier rows for those row variants)
	bool stair_behind = true;
	// options
	bool band_launch = true, band_reverse = true; long long band_work_log2 = 19, band_max_launches = 8, band_list_entries = 0;
	const twk_hip_variant_meta& at(uint32_t i) const { return meta[ids ? ids[i] : i]; }
};
struct BandLaunch { uint32_t xa, xb; size_t list_words; size_t tile_index; };
// What the plan says of a launch besides its rectangle.  side: the launch holds, of each of its rows, the columns on one side of the row's staircase
// border RegionPlan::stair - 1: [.., stair), 2: [stair, ..) - and no tile outside it is contracted or screened (0: the whole rectangle).
// behind: a two-product launch over rows behind the cut, from the diagonal to the rows' two_reach (plan_two_stairs).
struct LaunchNote { uint8_t side = 0, behind = 0; };
struct RegionPlan {
	bool windowed = false;
	std::vector<uint32_t> lo, hi;                   // windowed: row a0 + r reaches the columns [b0 + lo[r], b0 + hi[r])
	std::vector<uint64_t> cum;                      // cum[r] = pairs in reach of rows [0, r)
	uint32_t r0 = 0, r1 = 0;                        // the shard's rows
	uint32_t S = 0;                                 // super-tile edge in variants
	std::vector<twk_hip_tile_desc> mine;            // the launches, in order; the first bands.size() of them are band launches
	std::vector<BandLaunch> bands;
	uint64_t pairs = 0;                             // pairs the shard decides
	uint32_t two_end = 0;                           // the two-product walk: launches over rows below it (a multiple of the tile edge) lie wholly in front of r*
	// the fine walk's staircases: the border of row a0 + r is the column b0 + stair[r], the same for the 128 rows of a tile row counted from their
	// block's first row, and never rises along the rows of a block (empty: no launch has a side; 0: a row without one)
	std::vector<uint32_t> stair;
	std::vector<LaunchNote> notes;                  // per launch of `mine`
	uint32_t two_last = 0;                          // ... rows [two_end, two_last) have a two-product launch from the diagonal to their two_reach (two_end: none)
	void note_last(uint8_t side, uint8_t behind) { notes.resize(mine.size()); if (!notes.empty()) { notes.back().side = side; notes.back().behind = behind; } }
	// the columns [lo, hi) (set positions) of launch i that row `row` (a set position inside it) holds
	void launch_cols(const PlanGeom& g, size_t i, uint32_t row, uint32_t& lo, uint32_t& hi) const {
		const twk_hip_tile_desc& t = mine[i];
		lo = t.rowB0; hi = t.rowB0 + t.nB;
		if (t.diag && t.rowA0 == t.rowB0) lo = std::max(lo, row + 1);
		const uint8_t side = i < notes.size() ? notes[i].side : 0;
		if (side == 1) hi = std::min(hi, g.b0 + stair[row - g.a0]);
		if (side == 2) lo = std::max(lo, g.b0 + stair[row - g.a0]);
		if (hi < lo) hi = lo;
	}
};

// The column ranges of a plan's staircase launches as build_tile_list and the screens take them (ld_count_table.h ColRange): in front of the border
// [0, stair), behind it [stair, nB).  d_stair: the device copy of RegionPlan::stair for the screens (null: host only - the planner's tools).
struct StairRanges {
	std::vector<uint32_t> zero, end; ColRange left, right;
	void set(const RegionPlan& p, const PlanGeom& g, const uint32_t* d_stair) {
		if (p.stair.size() != g.nA) return;
		zero.assign(g.nA, 0); end.assign(g.nA, g.nB);
		left.lo = zero.data(); left.hi = p.stair.data(); left.d_hi = d_stair;
		right.lo = p.stair.data(); right.hi = end.data(); right.d_lo = d_stair;
		left.a0 = right.a0 = g.a0; left.b0 = right.b0 = g.b0; left.n_hi = right.n_hi = g.nA; left.falling = right.falling = true;
	}
	const ColRange* of(const RegionPlan& p, size_t i, const ColRange* other = nullptr) const {
		const uint8_t side = i < p.notes.size() ? p.notes[i].side : 0;
		return side == 1 ? &left : side == 2 ? &right : other;
	}
};

inline uint32_t plan_round_up(uint32_t x, uint32_t m) { return (x + m - 1) / m * m; }

// Rows [0, r) of a triangle (or trapezoid: nB >= nA columns, col > row) hold r*nB - r(r+1)/2 pairs; of an nA x nB rectangle r*nB.
inline uint64_t band_pairs_before(uint64_t r, uint64_t nA, uint64_t nB, bool triangle) {
	(void)nA;
	return triangle ? r * nB - r * (r + 1) / 2 : r * nB;      // triangle: row i pairs with cols (i, nB)
}
// First row of shard k: equal-area bands, boundaries on multiples of 64 variants.
inline uint32_t band_boundary(uint32_t k, uint32_t n_parts, uint32_t nA, uint32_t nB, bool triangle) {
	if (k == 0) return 0;
	if (k >= n_parts) return nA;
	const long double target = (long double)band_pairs_before(nA, nA, nB, triangle) * k / n_parts;
	uint32_t lo = 0, hi = nA;
	while (lo < hi) {
		const uint32_t mid = lo + (hi - lo) / 2;
		if ((long double)band_pairs_before(mid, nA, nB, triangle) < target) lo = mid + 1; else hi = mid;
	}
	return std::min(nA, (lo + 32) / 64 * 64);
}

// ---- the columns every row reaches ---------------------------------------------------------------------------------------
// r2 band (screen): with a and b the minor allele frequencies of two variants, a <= b, no 2x2 table with those margins has r2 above
// a(1-b) / ((1-a)b): |D| <= a(1-b), r2 = D^2 / (a(1-a)b(1-b)).  In order of minor allele count the pairs that can reach the cut-off
// are therefore a band above the diagonal: row r needs the columns (r, hi[r]) only, hi non-decreasing.  UnphasedMath estimates the
// haplotype frequency from genotypes and admits roots up to 1e-5 outside [minhap, maxhap] (ld_engine.h:37, ld_engine.cpp:1429-1558),
// so its |D| is bounded by a(1-b) + 1e-5.  The cut-off is lowered by a part in 1e6 against rounding in the reference's formula;
// pairs inside the band still go through that formula, so the survivors are the same.
inline void plan_reach_screen(const PlanEnv& e, const PlanGeom& g, RegionPlan& p) {
	const uint32_t nA = g.nA, nB = g.nB;
	p.lo.resize(nA); p.hi.resize(nA); p.cum.assign((size_t)nA + 1, 0);
	const long double T2 = 2.0L * e.n_samples, cut = (long double)e.minR2 * (1.0L - 1e-6L);
	auto mac = [&](uint32_t i) -> long double {      // minor allele count as the device counts it (twk_hip.hip ensure_popcounts)
		const long double ac = std::min<long double>(e.popc[e.ids ? e.ids[i] : i], T2);
		return std::min(ac, T2 - ac);
	};
	auto reach = [&](long double ma, long double mb) -> bool {        // can a pair with these minor counts (ma <= mb) pass?
		if (ma <= 0 || mb <= 0) return e.screen == 2;                   // a monomorphic site: PhasedMath drops it (D == 0)
		if (e.screen == 1) return ma * (T2 - mb) >= cut * (T2 - ma) * mb;
		const long double a = ma / T2, b = mb / T2, d = a * (1 - b) + 1e-5L;
		return d * d >= cut * a * (1 - a) * b * (1 - b);
	};
	uint32_t h = 0;
	for (uint32_t r = 0; r < nA; ++r) {
		const long double mr = mac(g.a0 + r);
		if (h < r + 1) h = std::min(r + 1, nB);
		while (h < nB && reach(mr, mac(g.b0 + h))) ++h;
		p.lo[r] = std::min(r + 1, nB);
		p.hi[r] = std::max(h, p.lo[r]);
		p.cum[r + 1] = p.cum[r] + (p.hi[r] - p.lo[r]);
	}
}
// Window mode: same contig, |dpos| <= l_window; variants are sorted by (rid, pos) like every .twk, so both ends only move forward.
// The ranges drive the shard boundaries (equal in-window pairs), the tile edge and the column range of every row block; the exact
// test itself stays in the math kernel.
inline void plan_reach_window(const PlanEnv& e, const PlanGeom& g, RegionPlan& p) {
	const uint32_t nA = g.nA, nB = g.nB;
	p.lo.resize(nA); p.hi.resize(nA); p.cum.assign((size_t)nA + 1, 0);
	uint32_t l = 0, h = 0;
	for (uint32_t r = 0; r < nA; ++r) {
		const twk_hip_variant_meta& R = e.at(g.a0 + r);
		auto before = [&](uint32_t j) { const twk_hip_variant_meta& B = e.at(g.b0 + j);
			return B.rid < R.rid || (B.rid == R.rid && (uint64_t)B.pos + g.l_window < R.pos); };
		auto within = [&](uint32_t j) { const twk_hip_variant_meta& B = e.at(g.b0 + j);
			return B.rid < R.rid || (B.rid == R.rid && B.pos <= (uint64_t)R.pos + g.l_window); };
		while (l < nB && before(l)) ++l;
		if (h < l) h = l;
		while (h < nB && within(h)) ++h;
		p.lo[r] = g.triangle ? std::min(std::max(l, r + 1), nB) : l;
		p.hi[r] = std::max(h, p.lo[r]);
		p.cum[r + 1] = p.cum[r] + (p.hi[r] - p.lo[r]);
	}
}

// ---- shard: a contiguous band of rows holding 1/n_parts of the region's pairs --------------------------------------------
// Row i of a triangle has nA-1-i pairs, of a rectangle nB; in window / band mode what the row reaches.  Equal-area bands,
// boundaries on multiples of 64 variants, derived identically (and without communication) by every rank.
inline void plan_shard(const PlanGeom& g, RegionPlan& p) {
	auto window_boundary = [&](uint32_t k) -> uint32_t {
		if (k == 0) return 0;
		if (k >= g.n_parts) return g.nA;
		const long double target = (long double)p.cum[g.nA] * k / g.n_parts;
		const uint32_t r = (uint32_t)(std::lower_bound(p.cum.begin(), p.cum.end(), (uint64_t)target) - p.cum.begin());
		return std::min(g.nA, (r + 32) / 64 * 64);
	};
	p.r0 = p.windowed ? window_boundary(g.part) : band_boundary(g.part, g.n_parts, g.nA, g.nB, g.triangle != 0);
	p.r1 = p.windowed ? window_boundary(g.part + 1) : band_boundary(g.part + 1, g.n_parts, g.nA, g.nB, g.triangle != 0);
}

// The block tiles build_tile_list (ld_count_table.h) will list for rows [x, x + h) over all the columns they reach.
inline uint64_t plan_tiles_of_rows(const PlanEnv& e, const PlanGeom& g, const RegionPlan& p, uint32_t x, uint32_t h) {
	const uint64_t P = (uint64_t)e.Pmax;
	const uint32_t col0 = g.triangle ? x : (p.windowed ? p.lo[x] : 0);
	uint64_t tiles = 0;
	for (uint64_t by = 0, gy = (h * P + PLAN_TILE - 1) / PLAN_TILE; by < gy; ++by) {
		const uint32_t v0 = x + (uint32_t)((by * PLAN_TILE) / P);
		const uint32_t v1 = (uint32_t)std::min<uint64_t>((uint64_t)x + h, (uint64_t)x + ((by + 1) * PLAN_TILE + P - 1) / P);
		if (v0 >= v1) continue;
		const uint32_t reach = p.windowed ? p.hi[v1 - 1] : g.nB;
		if (reach <= col0) continue;
		uint64_t c_lo = (p.windowed && p.lo[v0] > col0) ? ((uint64_t)(p.lo[v0] - col0) * P) / PLAN_TILE : 0;
		if (g.triangle) c_lo = std::max<uint64_t>(c_lo, by);
		const uint64_t c_hi = ((uint64_t)(reach - col0) * P + PLAN_TILE - 1) / PLAN_TILE;
		if (c_hi > c_lo) tiles += c_hi - c_lo;
	}
	return tiles;
}

// ---- super-tile edge -------------------------------------------------------------------------------------------------------
// Edge S in variants (multiple of 128).  Default: ~16384 plane rows per tile edge so that a launch holds >= 16 rounds of resident
// blocks and the partial last round costs < 3 %.  Window mode: a search over the row-block height.  A launch over rows [x, x + h)
// holds, per row of tiles, the tiles from the diagonal (or the first column its rows reach) to the last column they reach and costs
// ceil(tiles / resident blocks) rounds plus about half a round of launch, ramp-up and tail; the sum over the band's row blocks is
// minimised.  The plain path's math kernel visits every pair of the launch's rectangle, so there the block height stays near the
// window width; the fused path (count -> screen in the same kernel) visits the listed tiles only.
inline uint32_t plan_tile_edge(const PlanEnv& e, const PlanGeom& g, const RegionPlan& p) {
	uint32_t S = g.tile_variants ? g.tile_variants : (16384u / (uint32_t)e.Pmax);
	if (p.windowed && !g.tile_variants && p.r1 > p.r0) {
		const uint64_t wv = std::max<uint64_t>(1, (p.cum[p.r1] - p.cum[p.r0]) / (p.r1 - p.r0));   // mean partners per row
		const uint32_t s_hi = e.fused ? S : std::min<uint32_t>(S, std::max<uint32_t>(512u, plan_round_up((uint32_t)std::min<uint64_t>(wv, 1u << 20), 64)));
		const uint32_t s_lo = std::max<uint32_t>(128u, std::min<uint32_t>(s_hi, plan_round_up((uint32_t)std::min<uint64_t>(wv / 8, 1u << 20), 64)));
		const uint64_t R = e.resident_blocks;
		uint32_t best = s_lo; uint64_t best_cost = ~0ull;
		for (uint32_t cand = s_lo; cand <= s_hi; cand += 64) {
			uint64_t cost = 0;                    // in half rounds
			for (uint32_t x = p.r0; x < p.r1; x += cand) {
				const uint64_t tiles = plan_tiles_of_rows(e, g, p, x, std::min(cand, p.r1 - x));
				if (tiles) cost += 2 * ((tiles + R - 1) / R) + 1;
			}
			if (cost < best_cost || (cost == best_cost && cand > best)) { best_cost = cost; best = cand; }
		}
		S = best;
	}
	S = std::max<uint32_t>(PLAN_TILE, std::min<uint32_t>(S / PLAN_TILE * PLAN_TILE, 32768u));
	return std::min(S, plan_round_up(std::max(g.nA, g.nB), PLAN_TILE));
}

// One launch (tile descriptor) of the region, unless window mode proves that none of its pairs is wanted.
inline void plan_push_tile(const PlanEnv& e, const PlanGeom& g, std::vector<twk_hip_tile_desc>& out, uint32_t ra, uint32_t na, uint32_t cb, uint32_t nb_, int diag) {
	twk_hip_tile_desc t{};
	t.rowA0 = g.a0 + ra; t.nA = na; t.rowB0 = g.b0 + cb; t.nB = nb_; t.diag = diag; t.window = g.window; t.l_window = g.l_window;
	if ((g.window & TWK_HIP_OPT_WINDOW) && !diag) {
		// Each axis of a tile is sorted by (rid, pos) (file order, or one group of the regrouped set), but the two axes are in no
		// particular order relative to each other (regrouped rectangle: the rows are the variants with missing data, the columns the
		// rest).  A tile can only be skipped when both of its axes lie on one contig each and either the contigs differ or the
		// position intervals are more than the window apart, in whichever direction (the reference's ticker skips the rest of a row
		// on the same grounds, ld_balancing.h:191).
		const twk_hip_variant_meta& firstA = e.at(t.rowA0);
		const twk_hip_variant_meta& lastA  = e.at(t.rowA0 + t.nA - 1);
		const twk_hip_variant_meta& firstB = e.at(t.rowB0);
		const twk_hip_variant_meta& lastB  = e.at(t.rowB0 + t.nB - 1);
		if (firstA.rid == lastA.rid && firstB.rid == lastB.rid) {
			if (firstA.rid != firstB.rid) return;
			if ((uint64_t)firstB.pos > (uint64_t)lastA.pos + g.l_window) return;      // columns wholly after the rows' reach
			if ((uint64_t)firstA.pos > (uint64_t)lastB.pos + g.l_window) return;      // columns wholly before it
		}
	}
	out.push_back(t);
}

// Super-tiles sized by their count matrix, for the rows [xa, xb) of the band (appended to `out`).  Column step per row block: a
// launch of B blocks takes ceil(B / resident) rounds of (equal length) blocks, so the partial last round is pure loss; with the
// default tiling the column step is chosen, per row block, to minimise the total number of rounds (ties: fewer launches) - it matters
// for the thin bands of a multi-GPU shard.  C stays <= 2 GiB per tile.
// (S_: a super-tile edge of the caller's in the plan's place - plan_one_tiles)
inline void plan_matrix_tiles(const PlanEnv& e, const PlanGeom& g, const RegionPlan& p, uint32_t xa, uint32_t xb, std::vector<twk_hip_tile_desc>& out, uint32_t S_ = 0) {
	const uint32_t S = S_ ? S_ : p.S, nB = g.nB;
	const uint64_t P = (uint64_t)e.Pmax;
	auto rows_of = [&](uint32_t nv) -> uint64_t { return ((uint64_t)nv * P + PLAN_TILE - 1) / PLAN_TILE; };
	auto blocks_of = [&](uint32_t h, uint32_t w, bool diag) -> uint64_t {      // a diagonal tile only runs the blocks on and above its diagonal
		const uint64_t ra = rows_of(h), rb = rows_of(w);
		return diag ? ra * (ra + 1) / 2 + ra * (rb - ra) : ra * rb;
	};
	auto choose_col_step = [&](uint32_t h, uint32_t col0, bool first_is_diag) -> uint32_t {
		if (g.tile_variants || col0 >= nB) return std::max(S, h);
		const uint64_t R = e.resident_blocks, ra = rows_of(h);
		const uint64_t max_rows_b = std::min<uint64_t>(((2ull << 30) / 4) / (ra * PLAN_TILE), 32768ull * P / PLAN_TILE);   // blocks
		// window mode: the column range of a row block is already cut to what it can reach: one launch (or as few as the 2 GiB bound on C allows)
		if (p.windowed) return std::max<uint32_t>(h, (uint32_t)std::min<uint64_t>(32768ull, max_rows_b * PLAN_TILE / P / 64 * 64));
		uint32_t best = std::max(S, h); uint64_t best_cost = ~0ull;
		for (uint32_t sc = plan_round_up(h, 64); sc <= 32768; sc += 64) {
			if (rows_of(sc) > max_rows_b) break;
			if (sc * 4 < S) continue;                               // keep launches reasonably large
			uint64_t cost = 0; bool diag = first_is_diag;
			for (uint32_t col = col0; col < nB; col += sc, diag = false)
				cost += (blocks_of(h, std::min(sc, nB - col), diag) + R - 1) / R;
			if (cost < best_cost || (cost == best_cost && sc > best)) { best_cost = cost; best = sc; }
		}
		return best;
	};
	for (uint32_t x = xa; x < xb; x += S) {
		const uint32_t h = std::min(S, xb - x);
		// triangle: the first tile of the row block starts on the diagonal (rows [x,x+h) x cols [x,x+w), w >= h, only col > row) and
		// continues into the rectangle to its right in the same launch
		uint32_t col = g.triangle ? x : 0, col_end = nB;
		if (p.windowed) {       // only the columns some row of the block can reach
			if (!g.triangle) col = p.lo[x];
			col_end = p.hi[x + h - 1];
			if (col_end <= col) continue;
		}
		const uint32_t sc = choose_col_step(h, col, g.triangle != 0);
		bool diag = g.triangle != 0;
		for (; col < col_end; col += sc, diag = false) {
			uint32_t w = std::min(sc, col_end - col);
			if (diag && w < h) w = std::min(h, nB - col);            // the diagonal tile must span its own rows
			plan_push_tile(e, g, out, x, h, col, w, diag ? 1 : 0);
			if (diag && w > sc) col += w - sc;
		}
	}
}

// Band launches.  A fused launch keeps no count matrix - what it leaves behind is the list of its candidates - so nothing ties its
// extent to the 2 GiB a matrix may take: it is sized by its *work*.  The rows of the band are cut into launches of at least
// ~2^band_work_log2 tile-chunks (19: about 5 ms of contraction), at most band_max_launches per region, every one over all the columns
// its rows reach: one ramp-up and one tail per launch instead of per row block of 16,384 plane rows, and a handful of sorts, copies and
// hand-overs per region on the host instead of dozens.  More than one launch when there is work for it: the host's writer gets its first
// records while the device still counts.  A launch whose candidates or survivors outgrow their buffers is redone as matrix-sized tiles.
// Fills p.mine / p.bands; leaves both empty when the region does not qualify.
inline void plan_band_launches(const PlanEnv& e, const PlanGeom& g, RegionPlan& p) {
	const uint32_t step = PLAN_TILE;                                  // rows are cut on multiples of 128 variants
	const uint64_t P = (uint64_t)e.Pmax;
	auto rb = [&](uint64_t nv) -> uint64_t { return (nv * P + PLAN_TILE - 1) / PLAN_TILE; };
	std::vector<uint64_t> cum_tiles(1, 0);
	for (uint32_t x = p.r0; x < p.r1; x += step) cum_tiles.push_back(cum_tiles.back() + plan_tiles_of_rows(e, g, p, x, std::min(step, p.r1 - x)));
	const uint64_t total = cum_tiles.back();
	const uint64_t n_launch = std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)e.band_max_launches, total * e.nchunks >> e.band_work_log2));
	const uint64_t pairs_per_tile = (uint64_t)(PLAN_TILE / P) * (PLAN_TILE / P);
	const unsigned words_per_entry = e.phased_math ? 3 : 6;
	size_t k0 = 0;
	for (uint64_t l = 0; l < n_launch && k0 + 1 < cum_tiles.size(); ++l) {
		size_t k1 = cum_tiles.size() - 1;
		if (l + 1 < n_launch) {
			const uint64_t target = total * (l + 1) / n_launch;
			k1 = (size_t)(std::lower_bound(cum_tiles.begin() + k0 + 1, cum_tiles.end(), target) - cum_tiles.begin());
			k1 = std::min(k1, cum_tiles.size() - 1);
		}
		if (k1 <= k0) continue;
		const uint32_t xa = p.r0 + (uint32_t)k0 * step, xb = (uint32_t)std::min<uint64_t>(p.r1, (uint64_t)p.r0 + (uint64_t)k1 * step);
		const uint64_t tiles = cum_tiles[k1] - cum_tiles[k0];
		k0 = k1;
		if (!tiles) continue;
		const uint32_t col0 = g.triangle ? xa : (p.windowed ? p.lo[xa] : 0), col_end = p.windowed ? p.hi[xb - 1] : g.nB;
		if (col_end <= col0) continue;
		uint32_t w = col_end - col0;
		if (g.triangle && w < xb - xa) w = std::min(xb - xa, g.nB - col0);
		if (rb(xb - xa) > 0xFFFFu || rb(w) > 0xFFFFu) { p.bands.clear(); p.mine.clear(); return; }      // beyond a tile list's 16-bit coordinates: matrix tiles
		// candidate slots: 1/32 of the launch's pairs (a survivor-rich window run has 2 % candidates), 4 M at least, 256 M at most; the
		// survivor buffer is sized once the candidates are counted (enqueue_band_math)
		uint64_t entries = std::min<uint64_t>(std::max<uint64_t>(tiles * pairs_per_tile / 32, 1ull << 22), 1ull << 28);
		entries = std::min<uint64_t>(entries, std::max<uint64_t>(tiles * pairs_per_tile / 3, 1024));      // (never more than a matrix tile would get)
		if (e.band_list_entries) entries = (uint64_t)e.band_list_entries;      // (test / measurement: exactly this many)
		const BandLaunch b{xa, xb, (size_t)entries * words_per_entry, p.mine.size()};
		const size_t before = p.mine.size();
		plan_push_tile(e, g, p.mine, xa, xb - xa, col0, w, g.triangle ? 1 : 0);
		if (p.mine.size() > before) p.bands.push_back(b);
	}
	if (p.bands.empty()) { p.mine.clear(); return; }
	if (e.screen && e.band_reverse) {
		// Allele-count order: the survivors of a run concentrate in the last bands (common variants).  Last band first, so that the host
		// compresses those while the device counts the poor ones, instead of after it has finished (profiles/r04_band_timeline.txt).
		std::reverse(p.bands.begin(), p.bands.end());
		std::reverse(p.mine.begin(), p.mine.begin() + (ptrdiff_t)p.bands.size());
		for (size_t i = 0; i < p.bands.size(); ++i) p.bands[i].tile_index = i;
	}
}

// ---- the two-product walk's cut -------------------------------------------------------------------------------------------
// r*: the first row of the region at which the two-product screen (ld_two_screen.h), asked at the independence expectation of a pair and
// with the square root of its bound shrunk to two_margin of it, keeps a pair with some column behind the row.  From there on a two-product
// launch would list a large part of its pairs as candidates (in allele-count order: rows with p above ~0.17 at r2 >= 0.1), so launches
// behind r* keep the three-product form; the rows in front of it are cut off at the A tile edge below r*, and which form their launches
// really take is still decided by a sample of each (ld_form.h: decide_wants).  The margin keeps the rows next to the edge -
// where sampling noise decides - out: 0.95 moves the edge from p = 0.172 to 0.160 at r2 >= 0.1.
// Every rank of a sharded run finds the same r*: it is a property of the region, asked from row 0 on whatever the shard.  Each row is asked
// against at most 256 columns spread evenly over those behind it, the last one included (the predicate is no guarantee, only a guide: the
// sample decides, and an overflowing list is redone).
inline uint32_t plan_two_end(const PlanEnv& e, const PlanGeom& g) {
	if (!e.het || !e.hom || !g.triangle || g.nA == 0) return 0;
	const double two_n = 2.0 * (double)e.n_samples, cut = e.minR2 * (1.0 - 1e-6);
	uint32_t r = 0;
	for (; r < g.nA; ++r) {
		const uint32_t first = r + 1, n_behind = g.nB > first ? g.nB - first : 0;
		if (!n_behind) continue;
		const uint32_t n_ask = std::min<uint32_t>(n_behind, 256);
		bool kept = false;
		for (uint32_t k = 0; k < n_ask && !kept; ++k) {
			const uint32_t j = first + (uint32_t)(((uint64_t)(k + 1) * n_behind) / n_ask) - 1;
			const ScreenMargins m{e.het[g.a0 + r], e.hom[g.a0 + r], e.het[g.b0 + j], e.hom[g.b0 + j]};
			kept = e.carrier ? screen2c_expected_keeps(m, (double)e.n_samples, two_n, cut, e.two_margin, e.fine)
			                 : screen2_expected_keeps(m, (double)e.n_samples, two_n, cut, e.two_margin);
		}
		if (kept) break;
	}
	return r / PLAN_TILE * PLAN_TILE;
}

// ---- one-product launches in front of the cut -----------------------------------------------------------------
// The one-product screen (ld_two_screen.h: screen1c_*) tests its lower value at S >= 0, where it is -(dA dB) - eps: a function of the two
// dosages.  In allele-count order it passes for a row against every column up to some boundary and fails from there on (the ratio
// dA dB / (rA rB) rises along the columns), and a row in front passes wherever a later row does - but for pairs of two very rare variants,
// where eps decides.  plan_one_end: the first column (relative to b0, > row) at which the test fails for `row`, nB if there is none - a binary
// search on the real het and hom counts; row + 1 if it fails at once.
inline bool plan_one_lower_ok(const PlanEnv& e, const PlanGeom& g, uint32_t row, uint32_t col) {
	const ScreenMargins m{e.het[g.a0 + row], e.hom[g.a0 + row], e.het[g.b0 + col], e.hom[g.b0 + col]};
	return screen1c_lower_ok(m, 2.0 * (double)e.n_samples, e.minR2 * (1.0 - 1e-6));
}
inline uint32_t plan_one_end(const PlanEnv& e, const PlanGeom& g, uint32_t row) {
	uint32_t lo = std::min(row + 1, g.nB), hi = g.nB;      // [lo, hi): the first failing column lies in [lo, hi]
	while (lo < hi) {
		const uint32_t mid = lo + (hi - lo) / 2;
		if (plan_one_lower_ok(e, g, row, mid)) lo = mid + 1; else hi = mid;
	}
	return lo;
}
// The height of the row blocks in front of the cut: option "one_rows", else half the super-tile edge S - a block's one_end is its last row's, so
// lower blocks reach further.  The planner predicts 0.8685 of the carrier form's count work with S / 2 against 0.8775 with S on the headline, and
// the GPU agrees: 2598 against 2622 ms a step, one more launch a step included (profiles/one_product_ab.txt).  Never lower than 1024 rows by
// default (or S, where that is less): below that a block is a launch of a few hundred tiles, and halving it buys a sample, a ramp-up and a tail more
// for a boundary that moves by a tile or two.
inline uint32_t plan_one_rows(const PlanEnv& e, uint32_t S) {
	const uint32_t h = e.one_rows ? e.one_rows : std::max<uint32_t>(S / 2, std::min<uint32_t>(S, 1024));
	return std::max<uint32_t>(PLAN_TILE, h / PLAN_TILE * PLAN_TILE);
}
// The rows [xa, xb) in front of the cut, block by block: the columns [diagonal, one_end) of a block as one-product launches (twk_hip_tile_desc::one;
// tiles of 128 x 128 variants over the carrier rows of both axes), the columns [one_end, nB) as two-product launches as before.  one_end: the
// block's last row's, rounded down to a whole number of 128 variants from the diagonal and never before the block's own end; a block whose own
// pairs do not all pass the lower test (two very rare variants; a block that straddles the boundary) has no one-product launch.  A launch's
// rectangle is one whose count matrix stays within 2 GiB also when it is redone with four products, as for every other launch.
// The fine walk (PlanEnv::fine): the border is asked once per tile row of 128 variants, at that tile row's last row, and rounded down to 128 variants
// from the block's first column - a staircase that never rises along the block's rows and ends at the block's own border of before.  The one-product
// launches are then the rectangle [diagonal, the first tile row's border) and list, per tile row, the tiles in front of that tile row's border; the
// two-product launches are the rectangle [the last tile row's border, nB) and list the tiles behind it (RegionPlan::stair, LaunchNote::side).  A block
// whose tile rows' answers would rise (two very rare variants) keeps the one border.
inline void plan_block_launches(const PlanEnv& e, const PlanGeom& g, RegionPlan& p, uint32_t x, uint32_t h, uint32_t col_first, uint32_t col_last, bool left_one, uint8_t behind);
inline void plan_one_tiles(const PlanEnv& e, const PlanGeom& g, RegionPlan& p, uint32_t xa, uint32_t xb) {
	std::vector<twk_hip_tile_desc>& out = p.mine;
	const uint32_t H = plan_one_rows(e, p.S), nB = g.nB;
	for (uint32_t x = xa; x < xb; x += H) {
		const uint32_t h = std::min(H, xb - x), last = x + h - 1;
		uint32_t w = 0;      // columns of the block's one-product launches, from the diagonal
		if (last + 1 < nB && (h < 2 || plan_one_lower_ok(e, g, x, x + 1))) {
			const uint32_t end = plan_one_end(e, g, last);
			if (end >= std::min(x + h, nB) && end > last + 1) w = end >= nB ? nB - x : std::max(h, (end - x) / PLAN_TILE * PLAN_TILE);
		}
		if (w && e.fine && !e.fused && h > PLAN_TILE && x + w < nB) {      // (a block of one tile row, or one that reaches the last column, has no staircase)
			const uint32_t n_ty = (h + PLAN_TILE - 1) / PLAN_TILE;
			std::vector<uint32_t> s(n_ty, x + w);
			bool ok = true;
			for (uint32_t ty = 0; ty + 1 < n_ty && ok; ++ty) {
				const uint32_t end = plan_one_end(e, g, x + (ty + 1) * PLAN_TILE - 1);
				s[ty] = end >= nB ? nB : x + (end - x) / PLAN_TILE * PLAN_TILE;
				if (ty) s[ty] = std::min(s[ty], s[ty - 1]);
				ok = s[ty] >= x + w;
			}
			if (ok && s[0] > x + w) {
				p.stair.resize(g.nA, 0);
				for (uint32_t r = 0; r < h; ++r) p.stair[x + r] = s[r / PLAN_TILE];
				plan_block_launches(e, g, p, x, h, s[0], x + w, true, 0);
				continue;
			}
		}
		const uint64_t rows = plan_round_up(h, PLAN_TILE);
		const uint32_t w_max = (uint32_t)std::max<uint64_t>(h, std::min<uint64_t>(32768, ((1ull << 27) / rows) / PLAN_TILE * PLAN_TILE));
		uint32_t col = x;
		for (bool diag = true; col < x + w; diag = false) {
			const uint32_t wl = std::min(w_max, x + w - col);
			const size_t before = out.size();
			plan_push_tile(e, g, out, x, h, col, wl, diag ? 1 : 0);
			if (out.size() > before) out.back().one = 1;
			col += wl;
		}
		if (!w) { plan_matrix_tiles(e, g, p, x, x + h, out, h); continue; }
		// the rest of the block's columns: two products, as few launches of equal width as that bound allows
		if (col < nB) {
			const uint32_t rest = nB - col, n_l = (rest + w_max - 1) / w_max, step = plan_round_up((rest + n_l - 1) / n_l, PLAN_TILE / 2);
			for (; col < nB; col += step) plan_push_tile(e, g, out, x, h, col, std::min(step, nB - col), 0);
		}
	}
}

// The launches of a block of rows [x, x + h) with a staircase (RegionPlan::stair filled for its rows): the rectangle [x, col_first) - col_first the
// first tile row's border, the largest - as launches of side 1, the first of them on the diagonal, and the rectangle [col_last, nB) - col_last the last
// tile row's border - as launches of side 2; each rectangle one whose count matrix stays within 2 GiB also when it is redone with four products.
// left_one: the left launches are planned for one product (in front of the cut); behind: they are the two-product launches behind the cut.
inline void plan_block_launches(const PlanEnv& e, const PlanGeom& g, RegionPlan& p, uint32_t x, uint32_t h, uint32_t col_first, uint32_t col_last, bool left_one, uint8_t behind) {
	const uint32_t nB = g.nB;
	const uint64_t rows = plan_round_up(h, PLAN_TILE);
	const uint32_t w_max = (uint32_t)std::max<uint64_t>(h, std::min<uint64_t>(32768, ((1ull << 27) / rows) / PLAN_TILE * PLAN_TILE));
	uint32_t col = x;
	for (bool diag = true; col < col_first; diag = false) {
		uint32_t wl = std::min(w_max, col_first - col);
		if (diag && wl < h) wl = std::min(h, nB - col);      // (the diagonal launch spans its own rows)
		const size_t before = p.mine.size();
		plan_push_tile(e, g, p.mine, x, h, col, wl, diag ? 1 : 0);
		if (p.mine.size() > before) { p.mine.back().one = left_one ? 1 : 0; p.note_last(1, behind); }
		col += wl;
	}
	if (col_last < nB) {
		const uint32_t rest = nB - col_last, n_l = (rest + w_max - 1) / w_max, step = plan_round_up((rest + n_l - 1) / n_l, PLAN_TILE / 2);
		for (col = col_last; col < nB; col += step) {
			const size_t before = p.mine.size();
			plan_push_tile(e, g, p.mine, x, h, col, std::min(step, nB - col), 0);
			if (p.mine.size() > before) p.note_last(2, 0);
		}
	}
}

// ---- two products behind the cut -------------------------------------------------------------------------------
// Behind two_end a row fails the planner's question against *some* column - the commonest - and still passes against the columns next to it: with
// QQ <= min(qA, qB, CQ) a row at p = 0.25 passes against columns near 0.25 and fails against 0.5.  two_reach(row): the first column behind the row at
// which the carrier screen, asked as plan_two_end asks it, keeps the pair (nB: none; row + 1: at once) - a binary search, the answer moving one way
// along the columns.
inline bool plan_two_keeps(const PlanEnv& e, const PlanGeom& g, uint32_t row, uint32_t col) {
	const ScreenMargins m{e.het[g.a0 + row], e.hom[g.a0 + row], e.het[g.b0 + col], e.hom[g.b0 + col]};
	return screen2c_expected_keeps(m, (double)e.n_samples, 2.0 * (double)e.n_samples, e.minR2 * (1.0 - 1e-6), e.two_margin, e.fine);
}
inline uint32_t plan_two_reach(const PlanEnv& e, const PlanGeom& g, uint32_t row) {
	uint32_t lo = std::min(row + 1, g.nB), hi = g.nB;
	while (lo < hi) {
		const uint32_t mid = lo + (hi - lo) / 2;
		if (!plan_two_keeps(e, g, row, mid)) lo = mid + 1; else hi = mid;
	}
	return lo;
}
// The rows [xa, xb) behind the cut, in blocks of S (option "one_rows" set: of that many rows, 256 at least - the test hook): per tile row of 128 variants the border is the smaller of its first and its last row's two_reach,
// rounded down to 128 variants from the block's first column and never rising along the block.  While every tile row's border lies behind the tile
// row's own columns, and its last row still passes against the column next to it, the block takes a two-product launch over [diagonal, border) - carrier rows as the row operand - and three products behind it; the
// first block in which some tile row's does not ends that: two_last is its first such row, and the rows from there on are planned as before.  A guide like
// the cut itself: every launch is sampled in its form, and a two-product launch that is refused or overflows is redone with three products.
inline uint32_t plan_two_stairs(const PlanEnv& e, const PlanGeom& g, RegionPlan& p, uint32_t xa, uint32_t xb) {
	uint32_t x = xa;
	const uint32_t H = e.one_rows ? plan_round_up(std::max<uint32_t>(e.one_rows, 2 * PLAN_TILE), PLAN_TILE) : p.S, h_min = e.one_rows ? PLAN_TILE : 4 * PLAN_TILE;
	for (; x < xb; x += H) {
		const uint32_t h = std::min(H, xb - x), n_ty = (h + PLAN_TILE - 1) / PLAN_TILE;
		if (x + PLAN_TILE >= g.nB) break;
		std::vector<uint32_t> s(n_ty);
		uint32_t n_ok = 0;      // tile rows whose border lies behind their own columns
		for (uint32_t ty = 0; ty < n_ty; ++ty, ++n_ok) {
			const uint32_t first = x + ty * PLAN_TILE, end_row = std::min(x + h, first + PLAN_TILE);
			const uint32_t reach = std::min(plan_two_reach(e, g, first), plan_two_reach(e, g, end_row - 1));
			s[ty] = reach >= g.nB ? g.nB : x + (reach > x ? (reach - x) / PLAN_TILE * PLAN_TILE : 0);
			if (ty) s[ty] = std::min(s[ty], s[ty - 1]);
			if (s[ty] < first + PLAN_TILE) break;
			// ... and the tile row's last row passes against its own first column: a border that only equals the tile row's end says nothing of the
			// pairs inside its diagonal tile, of which that one is the hardest (two_last: the first row whose own first column fails)
			if (end_row < g.nB && plan_two_keeps(e, g, end_row - 1, end_row)) break;
		}
		// (a block is cut where its tile rows stop reaching: the rows in front keep their staircase, if they are worth a launch of their own)
		const uint32_t h_ok = n_ok == n_ty ? h : n_ok * PLAN_TILE;
		if (h_ok < std::min<uint32_t>(h, h_min) || h_ok == 0) break;
		p.stair.resize(g.nA, 0);
		for (uint32_t r = 0; r < h_ok; ++r) p.stair[x + r] = s[r / PLAN_TILE];
		plan_block_launches(e, g, p, x, h_ok, s[0], s[(h_ok - 1) / PLAN_TILE], false, 1);
		if (h_ok < h) { x += h_ok; break; }
	}
	return std::min(x, xb);
}

// ---- the prefix contraction's stops ---------------------------------------------------------------------------
// A tile of a two- or three-product launch of the two-product walk is contracted over the chunks [0, stop) only; the screen bounds what it did
// not read by the rows' suffix margins (ld_two_screen.h).  The stop of a tile: for a small fixed set of its variant pairs - the four corners
// and the middle - the smallest point of the fine grid (ld_two_screen.h prefix_stop_chunks) at which the pair, at its independence
// expectation, is dropped by either of two questions: the screen with the square root of its bound shrunk to `margin` of it
// (prefix_expected_keeps), or the screen itself with the expected counts moved outwards by `sigma` standard deviations of theirs
// (prefix_sigma_keeps; sigma 0: the first question alone).  The largest of those, plus one fine step (none on the fine walk with sigma > 0).  Expected prefix counts come from the
// real prefix margins and the suffix term from the real suffix margins, so a file whose carriers crowd its last samples gets later stops by
// itself.  A guide and no guarantee: the launch's sample decides whether the stops are taken, and what the wider screen keeps is recounted.
struct PrefixEnv {
	const uint32_t* het = nullptr; const uint32_t* hom = nullptr;      // per position of the sorted set
	const uint32_t* suffix = nullptr;                                  // [2 x position + plane][PREFIX_GRID]: suffix popcounts of the H and Q rows
	uint32_t n_variants = 0, n_samples = 0, nchunks = 0;
	double cut = 0, margin = 0.95, sigma = 6.0;
	uint32_t fixed_grid = 0;                                           // test hooks "prefix_stop", "prefix_substop": this fine index for every tile (0: the planner's)
	bool carrier = false;                                              // a two-product launch's row operand is the carrier plane (PlanEnv::carrier)
	bool one = false;                                                  // ... and the launch contracts one product a pair (LaunchForm::one): the one-product questions
	bool fine = false;                                                 // the fine walk (PlanEnv::fine): the carrier questions with CQ in the min, and no spare step behind a sigma answer
	uint64_t samples_before(uint32_t f) const { return std::min<uint64_t>((uint64_t)prefix_stop_chunks(f, nchunks) * 32u * 32u, n_samples); }
	bool dropped(bool two, uint32_t vA, uint32_t vB, uint32_t f) const {
		if (f >= PREFIX_GRID) return true;       // (whole rows: the screen itself decides)
		const ScreenMargins m{het[vA], hom[vA], het[vB], hom[vB]};
		const SuffixMargins x{suffix[(size_t)(2 * vA) * PREFIX_GRID + f], suffix[(size_t)(2 * vA + 1) * PREFIX_GRID + f],
		                      suffix[(size_t)(2 * vB) * PREFIX_GRID + f], suffix[(size_t)(2 * vB + 1) * PREFIX_GRID + f]};
		const double n_pre = (double)samples_before(f), two_n = 2.0 * (double)n_samples;
		if (two && carrier && one) {
			if (!prefix_expected_keeps_one(m, x, n_pre, two_n, cut, margin)) return true;
			return sigma > 0 && !prefix_sigma_keeps_one(m, x, n_pre, two_n, cut, sigma);
		}
		if (!(two && carrier ? prefix_expected_keeps_carrier(m, x, n_pre, two_n, cut, margin, fine) : prefix_expected_keeps(m, x, two, n_pre, two_n, cut, margin))) return true;
		return sigma > 0 && !prefix_sigma_keeps(m, x, two, two && carrier, n_pre, two_n, cut, sigma, fine);
	}
	// smallest fine index in [1, PREFIX_GRID] at which the pair is dropped, walked from `hint` (the answer of a neighbouring tile: two or
	// three questions instead of a search - both inequalities move one way along the row)
	uint32_t pair_need(bool two, uint32_t vA, uint32_t vB, uint32_t hint) const {
		uint32_t f = std::min<uint32_t>(std::max<uint32_t>(hint, 1), PREFIX_GRID);
		while (f > 1 && dropped(two, vA, vB, f - 1)) --f;
		while (f < PREFIX_GRID && !dropped(two, vA, vB, f)) ++f;
		return f;
	}
};
// Fine index of the stop of the tile over row variants [a_lo, a_hi] x column variants [b_lo, b_hi] (inclusive; a tile that reaches the
// diagonal holds pairs of neighbours in allele-count order and is few: whole rows).  hint[5]: the caller's, carried from tile to tile.
// Only the largest of the five answers is used, so only one pair is walked: the one whose hint is the largest.  Each of the others is asked once,
// at that answer - dropped there, its own answer is no larger - and walked on from it only where it is not.  Six or seven questions a tile for
// the ten of five walks, which is what pays for the finer grid and the second question on the host.
inline uint32_t plan_prefix_tile_grid(const PrefixEnv& e, bool two, uint32_t a_lo, uint32_t a_hi, uint32_t b_lo, uint32_t b_hi, uint32_t* hint) {
	if (e.fixed_grid) return std::min<uint32_t>(e.fixed_grid, PREFIX_GRID);
	if (a_hi >= e.n_variants) a_hi = e.n_variants - 1;
	if (b_hi >= e.n_variants) b_hi = e.n_variants - 1;
	if (a_lo > a_hi || b_lo > b_hi || b_lo <= a_hi) return PREFIX_GRID;
	const uint32_t pa[5] = {a_lo, a_lo, a_hi, a_hi, a_lo + (a_hi - a_lo) / 2}, pb[5] = {b_lo, b_hi, b_lo, b_hi, b_lo + (b_hi - b_lo) / 2};
	int first = 0;
	for (int k = 1; k < 5; ++k) if (hint[k] > hint[first]) first = k;
	uint32_t need = hint[first] = e.pair_need(two, pa[first], pb[first], hint[first]);
	for (int k = 0; k < 5; ++k) {
		if (k == first) continue;
		if (e.dropped(two, pa[k], pb[k], need)) hint[k] = std::min(hint[k], need);      // (an upper bound of its answer: it only picks the pair walked next time)
		else need = hint[k] = e.pair_need(two, pa[k], pb[k], need);
	}
	// The fine walk with the sigma question on: the answer itself.  The spare step dates from the margin question alone; behind six standard deviations
	// it is about five more (1 / 128 of a row of a million samples: ~2,900 counts of S against sigma ~550), and a miss costs one recount.
	if (e.fine && e.sigma > 0) return std::min<uint32_t>(need, PREFIX_GRID);
	// (one fine step of chunks, not of indices: on short rows fine points coincide where a sub-step is clipped)
	uint32_t f = std::min<uint32_t>(need + 1, PREFIX_GRID);
	while (f < PREFIX_GRID && prefix_stop_chunks(f, e.nchunks) == prefix_stop_chunks(need, e.nchunks)) ++f;
	return f;
}

// The stops of a launch's tiles as build_count_table (ld_count_table.h) asks for them: called with a tile's (tile row << 16 | tile column) in
// the order of the list, -> its stop in chunks; the grid index goes into grid[tile row * gx + tile column] for the screen.  A tile holds
// 64 x 64 variants in the three-product form, 128 row variants x 64 column variants in the two-product form and 128 x 128 in the one-product form.
struct PrefixTileStops {
	const PrefixEnv* e; bool two; uint32_t a0, b0, nA, nB, gx; std::vector<uint8_t>* grid; mutable uint32_t hint[5];
	uint32_t tvA() const { return two ? PLAN_TILE : PLAN_TILE / 2; }
	uint32_t tvB() const { return two && e->carrier && e->one ? PLAN_TILE : PLAN_TILE / 2; }
	uint32_t operator()(uint32_t yx) const {
		const uint32_t y = yx >> 16, x = yx & 0xFFFFu, ta = tvA(), tb = tvB();
		uint32_t g = PREFIX_GRID;
		if (y * ta < nA && x * tb < nB)
			g = plan_prefix_tile_grid(*e, two, a0 + y * ta, a0 + std::min(nA, (y + 1) * ta) - 1, b0 + x * tb, b0 + std::min(nB, (x + 1) * tb) - 1, hint);
		(*grid)[(size_t)y * gx + x] = (uint8_t)g;
		return prefix_stop_chunks(g, e->nchunks);
	}
};

// The whole plan of a region call.
inline void plan_region(const PlanEnv& e, const PlanGeom& g, RegionPlan& p) {
	p = RegionPlan();
	p.windowed = (g.window & TWK_HIP_OPT_WINDOW) != 0 || e.screen != 0;      // rows reach a column range only
	if (e.screen) plan_reach_screen(e, g, p);
	else if (p.windowed) plan_reach_window(e, g, p);
	plan_shard(g, p);
	p.S = plan_tile_edge(e, g, p);
	if (!g.tile_variants && e.band_launch && p.r1 > p.r0 && e.fused) plan_band_launches(e, g, p);
	if (e.het && !p.windowed && p.bands.empty()) p.two_end = plan_two_end(e, g);
	if (p.bands.empty()) {       // (the two-product walk: no launch straddles two_end)
		const uint32_t cut = std::min(std::max(p.two_end, p.r0), p.r1);
		if (e.one && e.carrier && e.het && cut > p.r0) plan_one_tiles(e, g, p, p.r0, cut);      // (... and a block's one-product launches end at its one_end)
		else plan_matrix_tiles(e, g, p, p.r0, cut, p.mine);
		// (the fine walk: two products from the diagonal to the rows' two_reach in the blocks behind the cut that have one)
		p.two_last = p.two_end;
		uint32_t behind = cut;
		if (e.fine && e.stair_behind && e.carrier && e.het && !e.fused && !g.tile_variants && g.triangle && p.two_end == cut && cut < p.r1) behind = p.two_last = plan_two_stairs(e, g, p, cut, p.r1);
		plan_matrix_tiles(e, g, p, behind, p.r1, p.mine);
	}
	p.notes.resize(p.mine.size());
	if (e.screen) p.pairs = band_pairs_before(p.r1, g.nA, g.nB, true) - band_pairs_before(p.r0, g.nA, g.nB, true);   // every pair of the band is decided
	else if (p.windowed) p.pairs = p.cum[p.r1] - p.cum[p.r0];       // pairs inside the window: the ones the math evaluates
	else p.pairs = band_pairs_before(p.r1, g.nA, g.nB, g.triangle != 0) - band_pairs_before(p.r0, g.nA, g.nB, g.triangle != 0);
}

// The sub-tile a density sample of launch t runs (ld_form.h: decide_wants): at most 384 x 384 variants from the launch's middle - a diagonal
// launch's from its diagonal, cut to the triangle's extent - through the same kernels (half a millisecond).
inline twk_hip_tile_desc sample_subtile(const twk_hip_tile_desc& t) {
	twk_hip_tile_desc st = t;
	const uint32_t h = std::min<uint32_t>(384, t.nA), row_c = t.rowA0 + (t.nA - h) / 2;
	st.rowA0 = row_c; st.nA = h;
	if (t.diag && t.rowA0 == t.rowB0) { st.rowB0 = row_c; st.nB = std::min<uint32_t>(h, t.rowB0 + t.nB - row_c); st.diag = 1; }
	else { const uint32_t wv = std::min<uint32_t>(384, t.nB); st.rowB0 = t.rowB0 + (t.nB - wv) / 2; st.nB = wv; st.diag = 0; }
	return st;
}

// ... of launch i of a plan: a launch on one side of a staircase (LaunchNote::side) takes its sample where it has pairs - a launch that lies beside the
// diagonal launch may have none in its rectangle's middle rows, whose border lies in front of it: then from its first rows, whose border is the furthest -
// with the columns from the middle of what the sample's middle row holds.  *pairs: the pairs of the sub-tile that are the launch's.
inline twk_hip_tile_desc sample_subtile_of(const RegionPlan& p, const PlanGeom& g, size_t i, uint64_t* pairs) {
	const twk_hip_tile_desc& t = p.mine[i];
	twk_hip_tile_desc st = sample_subtile(t);
	const bool sided = i < p.notes.size() && p.notes[i].side != 0;
	if (sided && !st.diag) {
		uint32_t lo, hi; p.launch_cols(g, i, st.rowA0 + st.nA / 2, lo, hi);
		if (hi <= lo) { st.rowA0 = t.rowA0; p.launch_cols(g, i, st.rowA0 + st.nA / 2, lo, hi); }
		if (hi > lo) { const uint32_t w = std::min<uint32_t>(384, hi - lo); st.rowB0 = lo + (hi - lo - w) / 2; st.nB = w; }
	}
	uint64_t n = 0;
	for (uint32_t r = st.rowA0; r < st.rowA0 + st.nA; ++r) {
		uint32_t lo = st.rowB0, hi = st.rowB0 + st.nB;
		if (sided) { uint32_t l2, h2; p.launch_cols(g, i, r, l2, h2); lo = std::max(lo, l2); hi = std::min(hi, h2); }
		else if (st.diag) lo = std::max(lo, r + 1);
		if (hi > lo) n += hi - lo;
	}
	if (pairs) *pairs = n;
	return st;
}

}  // namespace twk
