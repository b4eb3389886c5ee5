// The index arithmetic of the LD matrix fill (csrc/hip/ld_matrix_index.h) played on the host: `make matrix-check` builds this file with
// plain g++ and runs it.  Every lane of every block of every launch of a case goes through the kernel's own steps - live lane, dead
// block, guards, direct slot, staging index, transposed write-out, mirrored slot - against an n x n array of write counts.  A case fails
// unless every off-diagonal entry of the slice whose pair the launches hold was written exactly once from each side (the direct store
// above the diagonal, the mirrored one below it) with its own pair's value, the diagonal was never written, and no slot outside the
// n x n array was touched.  The transposed write-out is also checked for what it is for: the 32 lanes of half a wave read 32 different
// LDS banks and store to 32 consecutive floats of one output row.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "../hip/ld_matrix_index.h"

using namespace twk;

namespace {

struct LaunchGeom { uint32_t a0, nA, b0, nB; bool diag; };      // set positions, as a tile descriptor has them

// The launches of a triangle of `n` set positions from `first` on in super-tiles of S variants (ld_plan.h plan_matrix_tiles with
// tile_variants given): per row block the tile on the diagonal, then the rectangles to its right.
std::vector<LaunchGeom> triangle_launches(uint32_t first, uint32_t n, uint32_t S) {
	std::vector<LaunchGeom> out;
	for (uint32_t x = 0; x < n; x += S) {
		const uint32_t h = std::min(S, n - x);
		bool diag = true;
		for (uint32_t col = x; col < n; col += S, diag = false) {
			uint32_t w = std::min(S, n - col);
			if (diag && w < h) w = std::min(h, n - col);
			out.push_back(LaunchGeom{first + x, h, first + col, w, diag});
		}
	}
	return out;
}

struct Case {
	const char* name;
	uint32_t M;                          // variants of the problem (set positions beyond it hold no variant)
	uint32_t slice_a0, n;                // the matrix's slice
	std::vector<LaunchGeom> launches;
	std::vector<uint32_t> ids;           // empty: plain set
	// which pairs of variants (file order ids) pass 1 / pass 2 of the launches evaluate: 0 all in every launch, 1 pairs with both outside `front`
	// in launches [0, split) and the others in launches [split, ..)
	uint32_t split = 0; std::vector<uint8_t> front;
	uint32_t first_ids_launch = 0;       // launches from here on go through ids (the plain pass of the default mode comes first)
};

struct Board {
	uint32_t n; std::vector<uint32_t> writes; std::vector<uint32_t> value; long outside = 0, wrong_value = 0;
	explicit Board(uint32_t n_) : n(n_), writes((size_t)n_ * n_, 0), value((size_t)n_ * n_, 0) {}
	void store(size_t slot, uint32_t v) {
		if (slot >= writes.size()) { ++outside; return; }
		++writes[slot]; value[slot] = v;
	}
};
uint32_t pair_value(uint32_t u, uint32_t v) { if (u > v) std::swap(u, v); return u * 65536u + v + 1; }

long play_launch(const Case& cs, const LaunchGeom& L, bool with_ids, int pass, Board& bd) {
	long bad = 0;
	const uint32_t* ids = with_ids ? cs.ids.data() : nullptr;
	const uint32_t gx = (L.nB + MX_COLS - 1) / MX_COLS, gy = (L.nA + MX_ROWS - 1) / MX_ROWS;
	const bool diag_launch = L.diag && L.a0 == L.b0;
	std::vector<uint32_t> stage(MX_STAGE_WORDS), kept(MX_COLS);
	for (uint32_t by = 0; by < gy; ++by) for (uint32_t bx = 0; bx < gx; ++bx) {
		const uint32_t i0 = by * MX_ROWS;
		if (mx_block_dead(diag_launch, bx, i0)) {
			// nothing of a dead block may hold a pair
			for (uint32_t r = 0; r < MX_ROWS; ++r) for (uint32_t t = 0; t < MX_COLS; ++t)
				if (mx_lane_live(i0 + r, bx * MX_COLS + t, L.nA, L.nB) && L.b0 + bx * MX_COLS + t > L.a0 + i0 + r) ++bad;
			continue;
		}
		std::fill(stage.begin(), stage.end(), 0xDEADu); std::fill(kept.begin(), kept.end(), 0u);
		for (uint32_t tid = 0; tid < MX_COLS; ++tid) for (uint32_t r = 0; r < MX_ROWS; ++r) {
			const uint32_t i = i0 + r, j = bx * MX_COLS + tid;
			if (!mx_lane_live(i, j, L.nA, L.nB)) continue;
			const uint32_t sA = L.a0 + i, sB = L.b0 + j;
			// the pair rules of the math (d_pair): both variants exist, a diagonal launch keeps col > row, the pass selects its pairs
			if (!(sA < cs.M && sB < cs.M) || (diag_launch && !(sB > sA))) continue;
			const uint32_t A = ids ? ids[sA] : sA, B = ids ? ids[sB] : sB;
			if (pass) {
				const bool any_front = cs.front[A] || cs.front[B];
				if ((pass == 1) == any_front) continue;
			}
			if (!ids) {
				const uint32_t row = mx_rel(L.a0, i, cs.slice_a0), col = mx_rel(L.b0, j, cs.slice_a0);
				if (!mx_ok_plain(row, col, cs.n)) continue;
				bd.store(mx_slot(row, col, cs.n), pair_value(row, col));
				stage[mx_stage(r, tid)] = pair_value(row, col); kept[tid] |= 1u << r;
			} else {
				const uint32_t u = A - cs.slice_a0, v = B - cs.slice_a0;
				if (!mx_ok_ids(u, v, cs.n)) continue;
				bd.store(mx_slot(u, v, cs.n), pair_value(u, v));
				bd.store(mx_slot(v, u, cs.n), pair_value(u, v));
			}
		}
		if (ids) continue;
		// the transposed write-out
		std::vector<uint8_t> seen(MX_ROWS * MX_COLS, 0);
		for (uint32_t k = 0; k < MX_TSTEPS; ++k) for (uint32_t half = 0; half < MX_COLS / 32; ++half) {
			uint32_t banks = 0; size_t slot0 = 0; bool have0 = false; uint32_t lane0 = 0;
			for (uint32_t l = 0; l < 32; ++l) {
				const uint32_t tid = half * 32 + l, r = mx_trow(tid), c = mx_tcol(tid, k);
				if (r >= MX_ROWS || c >= MX_COLS) { ++bad; continue; }
				if (seen[r * MX_COLS + c]++) ++bad;
				const uint32_t b = mx_bank(mx_stage(r, c));
				if (banks >> b & 1) ++bad;                       // a bank conflict inside the half
				banks |= 1u << b;
				if (!(kept[c] >> r & 1)) continue;
				const uint32_t orow = mx_rel(L.b0, bx * MX_COLS + c, cs.slice_a0), ocol = mx_rel(L.a0, i0 + r, cs.slice_a0);
				if (!mx_ok_plain(ocol, orow, cs.n)) continue;
				const size_t slot = mx_slot(orow, ocol, cs.n);
				if (!have0) { have0 = true; slot0 = slot; lane0 = l; }
				else if (slot != slot0 + (l - lane0)) ++bad;     // a half's stores are consecutive floats of one output row
				if (stage[mx_stage(r, c)] != pair_value(orow, ocol)) ++bd.wrong_value;
				bd.store(slot, stage[mx_stage(r, c)]);
			}
		}
		for (const uint8_t s : seen) if (s != 1) ++bad;          // every staged word is visited exactly once
	}
	return bad;
}

long run_case(const Case& cs) {
	Board bd(cs.n);
	long bad = 0;
	for (size_t k = 0; k < cs.launches.size(); ++k) {
		const bool with_ids = !cs.ids.empty() && k >= cs.first_ids_launch;
		const int pass = cs.front.empty() ? 0 : (k < cs.split ? 1 : 2);
		bad += play_launch(cs, cs.launches[k], with_ids, pass, bd);
	}
	bad += bd.outside + bd.wrong_value;
	// every off-diagonal entry of the slice exactly once with its pair's value; the diagonal never
	for (uint32_t u = 0; u < cs.n; ++u) for (uint32_t v = 0; v < cs.n; ++v) {
		const size_t s = mx_slot(u, v, cs.n);
		const bool exists = cs.slice_a0 + u < cs.M && cs.slice_a0 + v < cs.M;
		const uint32_t want = (u != v && exists) ? 1u : 0u;
		if (bd.writes[s] != want) ++bad;
		else if (want && bd.value[s] != pair_value(u, v)) ++bad;
	}
	std::printf("  %-58s %3zu launches  %s\n", cs.name, cs.launches.size(), bad ? "BAD" : "ok");
	return bad;
}

std::vector<uint32_t> shuffled(uint32_t n, uint32_t seed) {
	std::vector<uint32_t> p(n);
	std::iota(p.begin(), p.end(), 0u);
	uint64_t s = seed * 2654435761ull + 1;
	for (uint32_t i = n - 1; i > 0; --i) { s = s * 6364136223846793005ull + 1442695040888963407ull; std::swap(p[i], p[(uint32_t)((s >> 33) % (i + 1))]); }
	return p;
}

}  // namespace

int main() {
	std::vector<Case> cases;
	auto plain = [&](const char* name, uint32_t M, uint32_t a0, uint32_t n, uint32_t S) {
		Case c; c.name = name; c.M = M; c.slice_a0 = a0; c.n = n; c.launches = triangle_launches(a0, n, S);
		cases.push_back(c);
	};
	plain("n=203 a0=37 tiles of 128 (M=300)", 300, 37, 203, 128);
	plain("n=203 a0=37 tiles of 128 (slice ends the file)", 240, 37, 203, 128);
	plain("n=300 a0=0 one tile of 384", 300, 0, 300, 384);
	plain("n=64", 64, 0, 64, 128);
	plain("n=65", 65, 0, 65, 128);
	plain("n=1", 1, 0, 1, 128);
	plain("n=1 a0=5 (M=9)", 9, 5, 1, 128);
	plain("n=700 a0=3 tiles of 512 (blocks across the diagonal)", 800, 3, 700, 512);
	plain("n=300 a0=0 tiles of 128 (six launches)", 300, 0, 300, 128);
	{	// the launches overhang the slice: planned for more variants than the matrix holds - the guards must keep them out
		Case c; c.name = "n=203 a0=37, launches planned over 260 variants"; c.M = 300; c.slice_a0 = 37; c.n = 203;
		c.launches = triangle_launches(37, 260, 128);
		cases.push_back(c);
		Case d; d.name = "n=100 a0=64, launches planned from variant 0 on"; d.M = 300; d.slice_a0 = 64; d.n = 100;
		d.launches = triangle_launches(0, 200, 128);
		cases.push_back(d);
	}
	{	// a regrouped set: a permutation of the ids, pairs in either order, one triangle
		Case c; c.name = "regrouped n=140: a permutation, one triangle"; c.M = 140; c.slice_a0 = 0; c.n = 140;
		c.ids = shuffled(140, 7); c.launches = triangle_launches(0, 140, 128);
		cases.push_back(c);
		Case d = c; d.name = "regrouped n=100 a0=10 of a permutation of 140"; d.slice_a0 = 10; d.n = 100;
		cases.push_back(d);
	}
	{	// the default mode with missing data: a plain pass over the pairs without missing data, then the regrouped set's front group
		// against itself (triangle) and against the rest (rectangle)
		Case c; c.name = "regrouped n=140: plain pass + front triangle + front x rest"; c.M = 140; c.slice_a0 = 0; c.n = 140;
		c.front.assign(140, 0);
		for (uint32_t v = 0; v < 140; ++v) c.front[v] = (v * 7 + 3) % 5 < 2;
		for (uint32_t v = 0; v < 140; ++v) if (c.front[v]) c.ids.push_back(v);
		const uint32_t nG = (uint32_t)c.ids.size();
		for (uint32_t v = 0; v < 140; ++v) if (!c.front[v]) c.ids.push_back(v);
		c.launches = triangle_launches(0, 140, 128);
		c.split = c.first_ids_launch = (uint32_t)c.launches.size();
		for (const LaunchGeom& g : triangle_launches(0, nG, 128)) c.launches.push_back(g);
		c.launches.push_back(LaunchGeom{0, nG, nG, 140 - nG, false});
		cases.push_back(c);
	}
	{	// ... and as two passes over the same file-order launches (a slice of the file: plain planes, then the masked ones)
		Case c; c.name = "two passes over one plain set n=203 a0=37"; c.M = 300; c.slice_a0 = 37; c.n = 203;
		c.front.assign(300, 0);
		for (uint32_t v = 0; v < 300; ++v) c.front[v] = v % 3 == 1;
		c.launches = triangle_launches(37, 203, 128);
		c.split = (uint32_t)c.launches.size();
		for (const LaunchGeom& g : triangle_launches(37, 203, 128)) c.launches.push_back(g);
		cases.push_back(c);
	}
	long bad = 0;
	for (const Case& c : cases) bad += run_case(c) ? 1 : 0;
	std::printf("matrix-check: %zu cases, %ld bad\n", cases.size(), bad);
	return bad ? 1 : 0;
}
