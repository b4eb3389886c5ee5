// The work table of a count launch, host side: which 128 x 128 tiles of a super-tile are contracted and in what order (build_tile_list), how
// their K ranges are cut into the units the persistent blocks draw (build_count_units), how the units are dealt to queues, and how tiles and
// units are packed for the device (CountTable).  With it the one statement of the last-chunk rule (count_last_halves).  Plain C++ with no HIP
// in it: ld_count.hip.h includes it (the kernels read the table, count_work / enqueue_count there launch it), so do the engine's host code and
// the dev tools, and csrc/tools/count_table_check.cpp (`make count-check`) plays it on the CPU against a naive restatement and against the
// recorded order of tests/golden/count_tables.json.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../../include/twk_hip.h"

namespace twk {

constexpr int TILE = 128;       // rows per block tile edge
constexpr int KC   = 32;        // 32-bit words of K per chunk (128 B per row)

inline uint32_t round_up(uint32_t x, uint32_t m) { return (x + m - 1) / m * m; }

struct CountUnit { uint32_t tile, c0, c1, yx; };       // chunks [c0, c1) of tiles[tile]; yx = tiles[tile], so that a block learns everything about its
                                                       // next unit from one 16-byte scalar load (fill_unit_tiles) instead of two dependent ones
// Set in CountUnit::tile of a unit that holds the whole count of a tile whose contraction stops short of the row's end (per-tile stops, the
// prefix contraction of DESIGN 3.1c): the kernel's epilogue stores such a unit's counts like those of a unit over [0, nchunks).  Never set
// in a table built without stops.
constexpr uint32_t UNIT_WHOLE = 0x80000000u;

// The unit table of a launch (host side; shared by the engine and the dev tools).  Guided self-scheduling:
// a unit is never longer than 1/share_div of an even share of the work still to be handed out, so whole
// tiles go out only while more than tail_rounds (= share_div) rounds of work remain, and after that
// K-ranges that shrink with the remainder down to `min_chunks` chunks.  The launch then ends within a few
// of the shortest units of perfect balance however unequal the blocks' speeds are (measured: finish
// times of the 512 blocks within 0.14 ms of each other on a 21 ms launch).  Returns the index of the
// first tile that is split (tiles from there on must be zeroed before the launch); n_tiles if none.
// Long rows, segmented walk (seg_chunks != 0, rows of at least two segments, patch_end = the list index where each
// patch of tiles ends): the tiles of a patch - which share their row and column tiles - are not contracted one whole
// tile per block, each block at its own pace, but K segment by K segment: all tiles of the patch over chunks
// [0, seg), then all over [seg, 2 seg), ...  The blocks working on a patch are then always within a segment of each
// other, so a chunk of a row tile fetched for one block is still in the MALL (and often in L2) when the other blocks
// that need it come by: HBM sees every (row tile, segment) about once per patch instead of once per tile.  The price:
// every unit is a part of its tile's K range (counts added with atomics into zeroed tiles - 32 adds per lane per
// segment, nothing next to the segment's 2048 x seg VALU ops).
template <class Vec>
inline uint32_t build_count_units(uint32_t n_tiles, uint32_t nchunks, uint32_t n_blocks, uint32_t min_chunks, Vec& units,
                                  uint32_t share_div = 8, uint32_t tail_rounds = 8,
                                  const uint32_t* patch_end = nullptr, uint32_t n_patches = 0, uint32_t seg_chunks = 0, const uint32_t* stops = nullptr) {
	units.clear();
	// stops (may be null; the segmented walk is not taken with them): tile t of the list is contracted over the chunks [0, stops[t]) only,
	// 1 <= stops[t] <= nchunks - without stops every tile's stop is nchunks.  Whole-tile units cover [0, stop), the guided tail sizes its
	// units by the chunks really left - the sum of the stops - and a split tile's units partition [0, stop).
	auto stop_of = [&](uint32_t t) -> uint32_t { return !stops ? nchunks : stops[t] < 1 ? 1 : (stops[t] > nchunks ? nchunks : stops[t]); };
	auto flag_of = [&](uint32_t stop) -> uint32_t { return stop < nchunks ? UNIT_WHOLE : 0u; };      // (a unit that holds a stopped tile's whole count)
	const uint32_t tail = (uint32_t)(n_tiles < (unsigned long long)tail_rounds * n_blocks ? n_tiles : (unsigned long long)tail_rounds * n_blocks);
	uint32_t first_split = n_tiles - tail;
	if (nchunks < 2 * min_chunks) first_split = n_tiles;             // rows too short to be worth splitting
	const bool segmented = !stops && seg_chunks && patch_end && n_patches && nchunks >= 2 * seg_chunks && nchunks >= 2 * min_chunks;
	if (segmented) {
		const uint32_t nseg = (nchunks + seg_chunks - 1) / seg_chunks;
		uint32_t p0 = 0;
		for (uint32_t p = 0; p < n_patches && p0 < first_split; ++p) {
			const uint32_t p1 = patch_end[p] < first_split ? patch_end[p] : first_split;
			for (uint32_t sgm = 0; sgm < nseg; ++sgm)
				for (uint32_t t = p0; t < p1; ++t)
					units.push_back(CountUnit{t, (uint32_t)((unsigned long long)nchunks * sgm / nseg), (uint32_t)((unsigned long long)nchunks * (sgm + 1) / nseg), 0});
			p0 = p1;
		}
	} else {
		for (uint32_t t = 0; t < first_split; ++t) units.push_back(CountUnit{t | flag_of(stop_of(t)), 0, stop_of(t), 0});
	}
	unsigned long long rem = 0;                                      // chunks left, from the tile at hand on
	for (uint32_t t = first_split; t < n_tiles; ++t) rem += stop_of(t);
	for (uint32_t t = first_split; t < n_tiles; ++t) {
		const uint32_t stop = stop_of(t);
		unsigned long long target = rem / ((unsigned long long)share_div * n_blocks);
		if (target < min_chunks) target = min_chunks;
		if (segmented && target > seg_chunks) target = seg_chunks;
		uint32_t S = (uint32_t)((stop + target - 1) / target);
		if (S < 1) S = 1;
		if (S > stop) S = stop;
		for (uint32_t k = 0; k < S; ++k)
			units.push_back(CountUnit{t | (S == 1 ? flag_of(stop) : 0u), (uint32_t)((unsigned long long)stop * k / S), (uint32_t)((unsigned long long)stop * (k + 1) / S), 0});
		rem -= stop;
	}
	return segmented ? 0 : first_split;
}

template <class Vec>
inline void fill_unit_tiles(Vec& units, const uint32_t* tiles) { for (auto& u : units) u.yx = tiles[u.tile & ~UNIT_WHOLE]; }

// Window mode: row variant a0 + r of a region reaches the columns [b0 + lo[r], b0 + hi[r]).
struct ColRange { const uint32_t* lo = nullptr; const uint32_t* hi = nullptr; uint32_t a0 = 0, b0 = 0;
                  const uint32_t* d_hi = nullptr; uint32_t n_hi = 0;      // d_hi: device copy of hi, n_hi entries (r2 screen: the math kernel skips what was not contracted)
                  const uint32_t* d_lo = nullptr;      // ... of lo, n_hi entries (the fine walk's launches behind a staircase: the screens skip what was not contracted)
                  bool falling = false;                // the ranges fall along the rows of a block (a staircase of the fine walk) instead of rising (window, band)
                  uint32_t list_zone = 0;              // pairs with both set positions below it are intersected as carrier lists (ld_list.hip.h), not contracted
                  uint32_t probe_zone = 0; };          // <= list_zone: every other pair of a row below it is decided by probing the column's row with the row's carriers (k_probe_screen)

struct Geometry { uint32_t rowsA, rowsB, gx, gy, ldc; };
// PA: plane rows a variant takes on the row axis when that differs from the column axis' P (0: the same).  The two-product form of
// UnphasedMath's contraction (ld_two_screen.h) stages one plane row - the H plane - per row variant against the H and Q rows of the
// column variants: PA = 1, P = 2, a tile of 128 row variants x 64 column variants.
inline Geometry tile_geometry(int P, const twk_hip_tile_desc& t, int PA = 0) {
	Geometry g;
	g.rowsA = round_up(t.nA * (PA ? PA : P), TILE); g.rowsB = round_up(t.nB * P, TILE);
	g.gy = g.rowsA / TILE; g.gx = g.rowsB / TILE; g.ldc = g.rowsB;
	return g;
}

// The 128 x 128 tiles of a super-tile that hold wanted pairs, as (tile row << 16 | tile column):
// on or above the diagonal (diag), and in window mode only those some row of the tile can reach.
// Order: 8 x 8 patches of tiles, patch by patch - the blocks pull consecutive tickets, so the ~P tiles in
// flight at any time are a few neighbouring patches (shared row / column tiles meet in L2 and the MALL).
// PA (0: P): plane rows per variant on the row axis (tile_geometry).  A tile row then starts at variant by * TILE / PA, and a tile of the
// diagonal super-tile is wanted when its last column variant lies behind that one: from column tile by * P / PA on.
inline void build_tile_list(const twk_hip_tile_desc& t, int P, const Geometry& g, bool diag, const ColRange* cr,
                     std::vector<uint32_t>& out, std::vector<uint32_t>* patch_end = nullptr, uint32_t PR = 8, uint32_t PC = 8, int PA_ = 0) {
	const int PA = PA_ ? PA_ : P;
	std::vector<uint32_t> x0(g.gy, 0), x1(g.gy, g.gx);
	for (uint32_t by = 0; by < g.gy; ++by) {
		if (diag) x0[by] = std::min<uint32_t>((uint32_t)((uint64_t)by * P / PA), g.gx);
		if (cr && cr->lo) {
			const uint32_t v0 = t.rowA0 + (by * TILE) / PA;
			const uint32_t v1 = std::min<uint64_t>((uint64_t)t.rowA0 + t.nA, (uint64_t)t.rowA0 + ((uint64_t)(by + 1) * TILE + PA - 1) / PA);   // exclusive
			if (v0 >= v1) { x1[by] = x0[by]; continue; }
			// (window and band mode: the ranges rise along the rows.  Down a staircase of the fine walk they fall - ColRange::falling - and a sample or a
			// strip of such a launch starts anywhere in a step: the tile row's last row then holds the smallest lo and its first row the largest hi)
			const uint64_t c_lo = (uint64_t)cr->b0 + cr->lo[(cr->falling ? v1 - 1 : v0) - cr->a0];
			const uint64_t c_hi = (uint64_t)cr->b0 + cr->hi[(cr->falling ? v0 : v1 - 1) - cr->a0];   // variants [c_lo, c_hi)
			const uint64_t lo = std::max<uint64_t>(c_lo, t.rowB0), hi = std::min<uint64_t>(c_hi, (uint64_t)t.rowB0 + t.nB);
			if (hi <= lo) { x1[by] = x0[by]; continue; }
			x0[by] = std::max<uint32_t>(x0[by], (uint32_t)(((lo - t.rowB0) * P) / TILE));
			x1[by] = std::min<uint32_t>(x1[by], (uint32_t)(((hi - t.rowB0) * P + TILE - 1) / TILE));
			if (x1[by] < x0[by]) x1[by] = x0[by];
		}
		if (cr && cr->list_zone) {      // a row of tiles that lies wholly inside the list zone starts at the zone's last column tile
			const uint64_t v1 = std::min<uint64_t>((uint64_t)t.rowA0 + t.nA, (uint64_t)t.rowA0 + ((uint64_t)(by + 1) * TILE + PA - 1) / PA);
			if (v1 <= cr->probe_zone) x1[by] = x0[by];                    // every pair of these rows is a list merge or a probe
			else if (v1 <= cr->list_zone && cr->list_zone > t.rowB0) {
				x0[by] = std::max<uint32_t>(x0[by], (uint32_t)((((uint64_t)cr->list_zone - t.rowB0) * P) / TILE));
				if (x1[by] < x0[by]) x1[by] = x0[by];
			}
		}
	}
	std::vector<uint32_t> seq;
	seq.reserve((size_t)g.gx * g.gy);
	// Patch shape 8 x 8.  Measured (profiles/r03_patch_pmc.txt, FETCH_SIZE = what the L2s ask the fabric for, 16,384 variants
	// at N = 1 M, 1.05 TB of tile-level demand per launch): 8 x 8 patches 258 GB per launch; wider patches are *worse*
	// (16 x 32: 309 GB), and so is walking a patch K segment by K segment (TWK_HIP_SEG=64: 306 GB) - the tiles in flight
	// are spread over eight L2s by the dispatcher, so fewer distinct row tiles in flight buys nothing per L2.  What does
	// help is giving each XCD its own patches (TWK_HIP_XCD_QUEUES=8 with 64-chunk segments: 149 GB, -42 %), at +0.5 % kernel
	// time for the adds into C; since the kernel is VALU-bound and the fabric sees < 10 % of its rate either way, that
	// trade is not taken by default.  (Options "patch_rows" / "patch_cols" / "seg" / "xcd_queues" are the hooks of that measurement.)
	if (patch_end) patch_end->clear();
	for (uint32_t py = 0; py < g.gy; py += PR)
		for (uint32_t px = 0; px < g.gx; px += PC) {
			for (uint32_t y = py; y < std::min(py + PR, g.gy); ++y)
				for (uint32_t x = std::max(px, x0[y]); x < std::min(px + PC, x1[y]); ++x) seq.push_back(y << 16 | x);
			if (patch_end && (patch_end->empty() ? !seq.empty() : seq.size() > patch_end->back())) patch_end->push_back((uint32_t)seq.size());
		}
	out.swap(seq);
}

// Half-slots (8 bytes per row) of a row's last K chunk that are contracted (CountWork::last_halves; 0: all sixteen) for rows of W_live live
// words in a pitch of W = W_live rounded up to KC.  The shortened chunk runs a plain rolled loop (no reads in flight behind the
// contraction): worth it when it drops a quarter of the chunk or more, not for a half-slot or two (2,504 samples phased: 157 live words
// of 160, 15 half-slots of the fifth chunk - there the pipelined loop over all 16 is the faster one).  (Option "skip_pad" = 0, the
// measurement hook that contracts the zero padding too, is the callers': they pass 0 instead of asking.)
inline uint32_t count_last_halves(uint32_t W_live, uint32_t W) {
	if (!W_live || W_live > W || W - W_live >= (uint32_t)KC) return 0;
	const uint32_t live_last = W_live - (W / KC - 1) * KC;      // live words of the last chunk, 1..KC
	const uint32_t halves = (live_last + 1) / 2;
	return halves > 12 ? 0 : halves;
}

// What a launch's table is built with besides its tile: the engine's options of the same names, the blocks the chip holds at once, and
// fused - no tile's K range is split, because a block must hold a pair's whole count to screen it.  (share_div, tail_rounds: the dev tool's knobs.)
struct CountSettings {
	uint32_t patch_rows = 8, patch_cols = 8, min_chunks = 8, seg_chunks = 0, xcd_queues = 0, n_blocks = 512;
	bool fused = false;
	uint32_t share_div = 8, tail_rounds = 8;
};

// The table of one launch.  Packed for the device it is [tiles | pad to 16 bytes | units]: words() 32-bit words with the units at
// units_at(); a caller that sends more behind it (the engine's parameter blocks) starts at words(), which is a multiple of four.
struct CountTable {
	Geometry g;
	std::vector<uint32_t> tiles, patch_end;      // patch_end[p]: the list index where patch p ends
	std::vector<CountUnit> units;                // in the order they are handed out, queue after queue
	uint32_t first_split = 0;                    // tiles[first_split ..) are covered by several units: zeroed before the launch, added to
	uint32_t n_queues = 1, queue_begin[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};      // CountWork's
	uint32_t n_tiles() const { return (uint32_t)tiles.size(); }
	uint32_t n_units() const { return (uint32_t)units.size(); }
	size_t units_at() const { return (tiles.size() + 3) / 4 * 4; }
	size_t words() const { return units_at() + units.size() * (sizeof(CountUnit) / 4); }
	void pack(uint32_t* dst) const {
		if (tiles.empty()) return;
		memcpy(dst, tiles.data(), tiles.size() * 4);
		memset(dst + tiles.size(), 0, (units_at() - tiles.size()) * 4);
		memcpy(dst + units_at(), units.data(), units.size() * sizeof(CountUnit));
	}
};

// The table for the P-plane rows of tile t (diag: only the tiles on or above the diagonal; cr: window mode's column ranges and zones, or
// null) over rows of nchunks K chunks.  One queue in the order of build_count_units, or - the measurement hook "xcd_queues" on rows of at
// least 128 chunks - the patches dealt round robin to one queue per XCD; within a queue patch after patch, each K segment by K segment.
// PA (0: P): plane rows per variant on the row axis, see tile_geometry.
// stop_of (may be empty): the per-tile stop in chunks, asked with a tile's (tile row << 16 | tile column) once the list is known - the prefix
// contraction's planner (ld_plan.h plan_prefix_stop).  Not combined with K segments or XCD queues (the caller asks for neither then).
// chunks_done / chunks_full (may be null): the chunks the table's tiles are contracted over, and what whole rows would have been.
struct NoStops { uint32_t operator()(uint32_t) const { return 0; } };
template <class StopOf = NoStops>
inline CountTable build_count_table(const twk_hip_tile_desc& t, int P, bool diag, const ColRange* cr, uint32_t nchunks, const CountSettings& s, int PA = 0,
                                    const StopOf* stop_of = nullptr, std::vector<uint32_t>* stops_out = nullptr) {
	CountTable tb;
	tb.g = tile_geometry(P, t, PA);
	build_tile_list(t, P, tb.g, diag, cr, tb.tiles, &tb.patch_end, s.patch_rows, s.patch_cols, PA);
	const uint32_t T = tb.n_tiles();
	const uint32_t min_chunks = s.fused ? nchunks + 1 : s.min_chunks, seg_chunks = s.fused ? 0 : s.seg_chunks;
	if (T && stop_of && !s.fused) {
		std::vector<uint32_t> local;
		std::vector<uint32_t>& stops = stops_out ? *stops_out : local;
		stops.resize(T);
		for (uint32_t i = 0; i < T; ++i) { const uint32_t st = (*stop_of)(tb.tiles[i]); stops[i] = st < 1 ? 1 : (st > nchunks ? nchunks : st); }
		tb.first_split = build_count_units(T, nchunks, s.n_blocks, min_chunks, tb.units, s.share_div, s.tail_rounds, nullptr, 0, 0, stops.data());
		for (uint32_t q = 1; q <= 8; ++q) tb.queue_begin[q] = tb.n_units();
	} else if (T && !s.fused && s.xcd_queues > 1 && s.xcd_queues <= 8 && nchunks >= 128 && !tb.patch_end.empty()) {
		const uint32_t nseg = seg_chunks ? (nchunks + seg_chunks - 1) / seg_chunks : 1;
		std::vector<std::vector<CountUnit>> qs(s.xcd_queues);
		uint32_t p0 = 0;
		for (size_t pi = 0; pi < tb.patch_end.size(); ++pi) {
			auto& qv = qs[pi % s.xcd_queues];
			for (uint32_t sgm = 0; sgm < nseg; ++sgm)
				for (uint32_t tl = p0; tl < tb.patch_end[pi]; ++tl)
					qv.push_back(CountUnit{tl, (uint32_t)((unsigned long long)nchunks * sgm / nseg), (uint32_t)((unsigned long long)nchunks * (sgm + 1) / nseg), 0});
			p0 = tb.patch_end[pi];
		}
		tb.n_queues = s.xcd_queues;
		for (uint32_t q = 0; q < tb.n_queues; ++q) { tb.queue_begin[q] = tb.n_units(); tb.units.insert(tb.units.end(), qs[q].begin(), qs[q].end()); }
		for (uint32_t q = tb.n_queues; q <= 8; ++q) tb.queue_begin[q] = tb.n_units();
		tb.first_split = nseg > 1 ? 0 : T;
	} else {
		tb.first_split = T ? build_count_units(T, nchunks, s.n_blocks, min_chunks, tb.units, s.share_div, s.tail_rounds, tb.patch_end.data(), (uint32_t)tb.patch_end.size(), seg_chunks) : 0;
		for (uint32_t q = 1; q <= 8; ++q) tb.queue_begin[q] = tb.n_units();
	}
	fill_unit_tiles(tb.units, tb.tiles.data());
	return tb;
}

}  // namespace twk
