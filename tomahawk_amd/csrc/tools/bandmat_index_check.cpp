// The banded LD matrix's layout and index arithmetic (csrc/hip/ld_bandmat_index.h) played on the host: `make bandmat-check` builds this
// file with g++ under AddressSanitizer and UBSan and runs it.  Per case
//   the layout (bm_band_layout over bm_layout: two forward-moving pointers) is checked against its O(n^2) definition - the band of row u is
//   exactly the set of variants on u's contig within the window, a contiguous range that holds u, symmetric, its ends never decreasing,
//   row_ptr its prefix sums, rows[u] == {ptr[u], first[u], ptr[u + 1] - ptr[u]}, cells == ptr[n], widest the longest row;
//   every lane of every block of every launch then goes through the kernel's own steps - live lane, the two dead-block tests, the pair
//   rules, the slice guards, the in-band guard, direct slot, staging index, transposed write-out, mirrored slot - against an array of
//   write counts of row_ptr[n] slots with a border on either side.
// A case fails unless every in-band off-diagonal slot (its pair passes the window test, by the layout check) was written exactly once
// with its own pair's value, the diagonal and everything outside [0, row_ptr[n]) never, every pair that passes the window test was
// in-band, no dead block held an in-band pair, and every half-wave of the write-out read 32 different LDS banks and stored consecutive
// floats of one row segment.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <string>
#include <vector>

#include "../hip/ld_bandmat_index.h"

using namespace twk;

namespace {

struct LaunchGeom { uint32_t a0, nA, b0, nB; bool diag; };      // set positions, as a tile descriptor has them

// The launches of a triangle of `n` set positions from `first` on in super-tiles of S variants (as csrc/tools/matrix_index_check.cpp).
// Every tile is played, also those the planner would skip as outside the window: they must store nothing.
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
	std::string name;
	uint32_t M = 0;                      // variants of the problem
	std::vector<uint32_t> pos, rid;      // [M], sorted by (rid, pos)
	uint32_t w = 0;                      // the window
	uint32_t slice_a0 = 0, n = 0;
	std::vector<LaunchGeom> launches;
	std::vector<uint32_t> ids;           // empty: plain set
	uint32_t split = 0; std::vector<uint8_t> front;      // two passes (matrix_index_check.cpp): pairs without a `front` variant in launches [0, split)
	uint32_t first_ids_launch = 0;
};

constexpr uint64_t BORDER = 4096;
struct Board {
	uint64_t nnz; std::vector<uint32_t> writes, value; long outside = 0, wrong_value = 0;
	explicit Board(uint64_t nnz_) : nnz(nnz_), writes(nnz_ + 2 * BORDER, 0), value(nnz_ + 2 * BORDER, 0) {}
	void store(uint64_t slot, uint32_t v) {
		const uint64_t at = slot + BORDER;                   // (a slot "below 0" wraps back into the front border, or far outside)
		if (at >= writes.size()) { ++outside; return; }
		++writes[at]; value[at] = v;
	}
};
uint32_t pair_value(uint32_t u, uint32_t v) { if (u > v) std::swap(u, v); return u * 65536u + v + 1; }

typedef BandLayout Layout;      // what the engine's calls lay a band out into

bool window_ok(const Case& cs, uint32_t A, uint32_t B) {
	const int64_t d = (int64_t)cs.pos[A] - (int64_t)cs.pos[B];
	return cs.rid[A] == cs.rid[B] && (d < 0 ? -d : d) <= (int64_t)cs.w;
}

// bm_band_layout (bm_layout, and the rows, slot count and longest row made of it) against the definition, in O(n^2)
long check_layout(const Case& cs, Layout& L) {
	long bad = 0;
	const uint32_t n = cs.n;
	const uint32_t* pos = cs.pos.data() + cs.slice_a0; const uint32_t* rid = cs.rid.data() + cs.slice_a0;
	if (!bm_band_layout(n, [&](uint32_t k) { return pos[k]; }, [&](uint32_t k) { return rid[k]; }, cs.w, L)) return 1;
	if (L.first.size() != n || L.ptr.size() != (size_t)n + 1 || L.rows.size() != n) return 1;
	uint64_t at = 0;
	uint32_t longest = 0;
	for (uint32_t u = 0; u < n; ++u) {
		if (L.ptr[u] != at || L.ptr[u + 1] < L.ptr[u]) { ++bad; break; }
		const uint64_t len64 = L.ptr[u + 1] - L.ptr[u];
		if (len64 == 0 || len64 > n) { ++bad; break; }
		const uint32_t first = L.first[u], len = (uint32_t)len64;
		if (L.rows[u].base != L.ptr[u] || L.rows[u].first != first || L.rows[u].len != len) ++bad;      // rows[u] == {ptr[u], first[u], ptr[u + 1] - ptr[u]}
		longest = std::max(longest, len);
		if ((uint64_t)first + len > n || !bm_in_band(u, first, len)) ++bad;
		for (uint32_t v = 0; v < n; ++v) {
			const bool in = bm_in_band(v, first, len);
			if (in != (v >= first && v < first + len)) ++bad;
			if (in != window_ok(cs, cs.slice_a0 + u, cs.slice_a0 + v)) ++bad;
			if (in && bm_slot(L.ptr[u], first, v) != L.ptr[u] + (v - first)) ++bad;
		}
		if (u && (first < L.first[u - 1] || first + len < L.first[u - 1] + (uint32_t)(L.ptr[u] - L.ptr[u - 1]))) ++bad;      // the ends never decrease
		at += len;
	}
	if (L.ptr[n] != at || L.cells != L.ptr[n] || L.widest != longest) ++bad;
	// symmetric
	if (!bad) for (uint32_t u = 0; u < n; ++u) for (uint32_t v = L.first[u]; v < L.first[u] + L.rows[u].len; ++v)
		if (!bm_in_band(u, L.rows[v].first, L.rows[v].len)) ++bad;
	return bad;
}

long play_launch(const Case& cs, const Layout& lay, const LaunchGeom& L, bool with_ids, int pass, Board& bd, long& dead_blocks) {
	long bad = 0;
	const uint32_t* ids = with_ids ? cs.ids.data() : nullptr;
	const uint32_t gx = (L.nB + MX_COLS - 1) / MX_COLS, gy = (L.nA + MX_ROWS - 1) / MX_ROWS;
	const bool diag_launch = L.diag && L.a0 == L.b0;
	const uint32_t n = cs.n;
	std::vector<uint32_t> stage(MX_STAGE_WORDS), kept(MX_COLS), cfirst(MX_COLS), clen(MX_COLS);
	std::vector<uint64_t> cbase(MX_COLS);
	for (uint32_t by = 0; by < gy; ++by) for (uint32_t bx = 0; bx < gx; ++bx) {
		const uint32_t i0 = by * MX_ROWS;
		bool dead = mx_block_dead(diag_launch, bx, i0);
		if (!dead && !ids) {
			const uint32_t ul = bm_block_last_row(L.a0, i0, L.nA, cs.slice_a0, n);
			if (ul >= n) { ++bad; continue; }                 // the kernel would read outside the map
			dead = bm_block_dead(L.b0, bx, cs.slice_a0, lay.rows[ul].first, lay.rows[ul].len);
			if (dead) ++dead_blocks;
		}
		if (dead) {
			// a dead block has no pair the launch would store: none above the diagonal that lies in the band
			for (uint32_t r = 0; r < MX_ROWS; ++r) for (uint32_t t = 0; t < MX_COLS; ++t) {
				if (!mx_lane_live(i0 + r, bx * MX_COLS + t, L.nA, L.nB)) continue;
				const uint32_t sA = L.a0 + i0 + r, sB = L.b0 + bx * MX_COLS + t;
				if (!(sA < cs.M && sB < cs.M) || !(sB > sA)) continue;
				const uint32_t u = sA - cs.slice_a0, v = sB - cs.slice_a0;
				if (u < n && v < n && bm_in_band(v, lay.rows[u].first, lay.rows[u].len)) ++bad;
			}
			continue;
		}
		std::fill(stage.begin(), stage.end(), 0xDEADu); std::fill(kept.begin(), kept.end(), 0u);
		if (!ids) for (uint32_t tid = 0; tid < MX_COLS; ++tid) {
			const uint32_t col = mx_rel(L.b0, bx * MX_COLS + tid, cs.slice_a0);
			BandRow row{0, 0, 0};
			if (col < n) row = lay.rows[col];
			cbase[tid] = row.base; cfirst[tid] = row.first; clen[tid] = row.len;
		}
		for (uint32_t tid = 0; tid < MX_COLS; ++tid) for (uint32_t r = 0; r < MX_ROWS; ++r) {
			const uint32_t i = i0 + r, j = bx * MX_COLS + tid;
			if (!mx_lane_live(i, j, L.nA, L.nB)) continue;
			const uint32_t sA = L.a0 + i, sB = L.b0 + j;
			// the pair rules of the math (d_pair): both variants exist, a diagonal launch keeps col > row, the pass selects its pairs, the window
			if (!(sA < cs.M && sB < cs.M) || (diag_launch && !(sB > sA))) continue;
			const uint32_t A = ids ? ids[sA] : sA, B = ids ? ids[sB] : sB;
			if (pass) {
				const bool any_front = cs.front[A] || cs.front[B];
				if ((pass == 1) == any_front) continue;
			}
			if (!window_ok(cs, A, B)) continue;
			if (!ids) {
				const uint32_t row = mx_rel(L.a0, i, cs.slice_a0), col = mx_rel(L.b0, j, cs.slice_a0);
				if (!mx_ok_plain(row, col, n)) continue;
				const BandRow& ru = lay.rows[row];
				if (!bm_in_band(col, ru.first, ru.len)) { ++bad; continue; }      // a pair that passes the window test is in-band
				bd.store(bm_slot(ru.base, ru.first, col), pair_value(row, col));
				stage[mx_stage(r, tid)] = pair_value(row, col); kept[tid] |= 1u << r;
			} else {
				const uint32_t u = A - cs.slice_a0, v = B - cs.slice_a0;
				if (!mx_ok_ids(u, v, n)) continue;
				const BandRow& ru = lay.rows[u]; const BandRow& rv = lay.rows[v];
				if (!bm_in_band(v, ru.first, ru.len) || !bm_in_band(u, rv.first, rv.len)) { ++bad; continue; }
				bd.store(bm_slot(ru.base, ru.first, v), pair_value(u, v));
				bd.store(bm_slot(rv.base, rv.first, u), pair_value(u, v));
			}
		}
		if (ids) continue;
		// the transposed write-out
		std::vector<uint8_t> seen(MX_ROWS * MX_COLS, 0);
		for (uint32_t k = 0; k < MX_TSTEPS; ++k) for (uint32_t half = 0; half < MX_COLS / 32; ++half) {
			uint32_t banks = 0; uint64_t slot0 = 0; bool have0 = false; uint32_t lane0 = 0, c0 = 0;
			for (uint32_t l = 0; l < 32; ++l) {
				const uint32_t tid = half * 32 + l, r = mx_trow(tid), c = mx_tcol(tid, k);
				if (r >= MX_ROWS || c >= MX_COLS) { ++bad; continue; }
				if (seen[r * MX_COLS + c]++) ++bad;
				if (l == 0) c0 = c; else if (c != c0) ++bad;      // one column a half: its BandRow is read at one LDS address (a broadcast)
				const uint32_t b = mx_bank(mx_stage(r, c));
				if (banks >> b & 1) ++bad;                       // a bank conflict inside the half
				banks |= 1u << b;
				if (!(kept[c] >> r & 1)) continue;
				const uint32_t orow = mx_rel(L.b0, bx * MX_COLS + c, cs.slice_a0), ocol = mx_rel(L.a0, i0 + r, cs.slice_a0);
				if (!mx_ok_plain(ocol, orow, n)) continue;
				if (!bm_in_band(ocol, cfirst[c], clen[c])) { ++bad; continue; }      // the mirror of an in-band pair is in-band
				const uint64_t slot = bm_slot(cbase[c], cfirst[c], ocol);
				if (slot < lay.ptr[orow] || slot >= lay.ptr[orow + 1]) ++bad;       // inside the column variant's row segment
				if (!have0) { have0 = true; slot0 = slot; lane0 = l; }
				else if (slot != slot0 + (l - lane0)) ++bad;     // a half's stores are consecutive floats of that segment
				if (stage[mx_stage(r, c)] != pair_value(orow, ocol)) ++bd.wrong_value;
				bd.store(slot, stage[mx_stage(r, c)]);
			}
		}
		for (const uint8_t s : seen) if (s != 1) ++bad;          // every staged word is visited exactly once
	}
	return bad;
}

long run_case(const Case& cs) {
	Layout lay;
	long bad = check_layout(cs, lay);
	if (bad) { std::printf("  %-66s layout BAD\n", cs.name.c_str()); return bad; }
	const uint64_t nnz = lay.ptr[cs.n];
	Board bd(nnz);
	long dead_blocks = 0;
	for (size_t k = 0; k < cs.launches.size(); ++k) {
		const bool with_ids = !cs.ids.empty() && k >= cs.first_ids_launch;
		const int pass = cs.front.empty() ? 0 : (k < cs.split ? 1 : 2);
		bad += play_launch(cs, lay, cs.launches[k], with_ids, pass, bd, dead_blocks);
	}
	bad += bd.outside + bd.wrong_value;
	// the border on either side of the band was never written
	for (uint64_t k = 0; k < BORDER; ++k) if (bd.writes[k] || bd.writes[BORDER + nnz + k]) ++bad;
	// every in-band off-diagonal slot exactly once with its pair's value; the diagonal never
	uint64_t visited = 0;
	for (uint32_t u = 0; u < cs.n; ++u) for (uint32_t v = lay.first[u]; v < lay.first[u] + lay.rows[u].len; ++v, ++visited) {
		const uint64_t s = BORDER + bm_slot(lay.rows[u].base, lay.rows[u].first, v);
		const uint32_t want = u != v ? 1u : 0u;
		if (bd.writes[s] != want) ++bad;
		else if (want && bd.value[s] != pair_value(u, v)) ++bad;
	}
	if (visited != nnz) ++bad;
	std::printf("  %-66s %3zu launches  nnz %8llu of %8llu  %4ld dead blocks  %s\n", cs.name.c_str(), cs.launches.size(), (unsigned long long)nnz,
	            (unsigned long long)cs.n * cs.n, dead_blocks, bad ? "BAD" : "ok");
	return bad;
}

std::vector<uint32_t> shuffled(uint32_t n, uint32_t seed) {
	std::vector<uint32_t> p(n);
	std::iota(p.begin(), p.end(), 0u);
	uint64_t s = seed * 2654435761ull + 1;
	for (uint32_t i = n - 1; i > 0; --i) { s = s * 6364136223846793005ull + 1442695040888963407ull; std::swap(p[i], p[(uint32_t)((s >> 33) % (i + 1))]); }
	return p;
}

// positions 1000, 1100, ..: one contig
Case even(const char* name, uint32_t M, uint32_t a0, uint32_t n, uint32_t S, uint32_t w) {
	Case c; c.name = name; c.M = M; c.slice_a0 = a0; c.n = n; c.w = w;
	c.pos.resize(M); c.rid.assign(M, 0);
	for (uint32_t v = 0; v < M; ++v) c.pos[v] = 1000 + 100 * v;
	c.launches = triangle_launches(a0, n, S);
	return c;
}

}  // namespace

int main() {
	std::vector<Case> cases;
	cases.push_back(even("n=203 a0=37 tiles of 128 (M=300), window +-20 variants", 300, 37, 203, 128, 2000));
	cases.push_back(even("n=203 a0=37 tiles of 128 (slice ends the file)", 240, 37, 203, 128, 2000));
	cases.push_back(even("n=300 band narrower than a wave (+-20), one tile of 384", 300, 0, 300, 384, 2000));
	cases.push_back(even("n=300 band narrower than a wave (+-20), tiles of 128", 300, 0, 300, 128, 2000));
	cases.push_back(even("n=700 band wider than a column block (+-300), tiles of 128", 700, 0, 700, 128, 30000));
	cases.push_back(even("n=700 a0=3 band wider than a column block (+-300), tiles of 512", 800, 3, 700, 512, 30000));
	cases.push_back(even("window 0: n=300, the diagonal alone", 300, 0, 300, 128, 0));
	cases.push_back(even("window beyond the span: n=300, the band is the dense matrix", 300, 0, 300, 128, 1u << 30));
	cases.push_back(even("n=1", 1, 0, 1, 128, 500));
	cases.push_back(even("n=1 a0=5 (M=9)", 9, 5, 1, 128, 500));
	cases.push_back(even("n=64", 64, 0, 64, 128, 1500));
	cases.push_back(even("n=65", 65, 0, 65, 128, 1500));
	{	// three contigs that change at indices that are no multiples of 32, positions restarting per contig
		Case c = even("three contigs of 97, 105 and 98 variants, tiles of 128", 300, 0, 300, 128, 1500);
		for (uint32_t v = 0; v < 300; ++v) { c.rid[v] = v < 97 ? 0 : v < 202 ? 1 : 2; c.pos[v] = 500 + 100 * (v < 97 ? v : v < 202 ? v - 97 : v - 202); }
		cases.push_back(c);
		Case d = c; d.name = "three contigs, the slice a0=37 n=203 across both borders"; d.slice_a0 = 37; d.n = 203; d.launches = triangle_launches(37, 203, 128);
		cases.push_back(d);
		Case e = c; e.name = "three contigs, a window beyond every contig (blocks of the dense matrix)"; e.w = 1u << 30;
		cases.push_back(e);
	}
	{	// clustered and duplicated positions: runs of equal positions, tight clusters, then a jump
		Case c = even("clustered and duplicated positions n=400", 400, 0, 400, 128, 300);
		uint32_t p = 1000;
		for (uint32_t v = 0; v < 400; ++v) { c.pos[v] = p; p += (v % 7 == 3) ? 0 : (v % 50 == 49) ? 5000 : (v % 5 == 0) ? 1 : 90; }
		cases.push_back(c);
		Case d = c; d.name = "clustered and duplicated positions, window 0 (the duplicates stay)"; d.w = 0;
		cases.push_back(d);
	}
	{	// gaps wider than the window: rows of length 1 between pairs of neighbours
		Case c = even("gaps wider than the window (rows of length 1) n=300", 300, 0, 300, 128, 150);
		uint32_t p = 1000;
		for (uint32_t v = 0; v < 300; ++v) { c.pos[v] = p; p += (v % 3 == 0) ? 100 : 1000; }
		cases.push_back(c);
	}
	{	// the launches overhang the slice: planned for more variants than the band holds - the guards must keep them out
		Case c = even("n=203 a0=37, launches planned over 260 variants", 300, 37, 203, 128, 2000);
		c.launches = triangle_launches(37, 260, 128);
		cases.push_back(c);
		Case d = even("n=100 a0=64, launches planned from variant 0 on", 300, 64, 100, 128, 2000);
		d.launches = triangle_launches(0, 200, 128);
		cases.push_back(d);
		Case e = even("n=100 a0=300 of 700, launches planned from variant 0 on in tiles of 512", 700, 300, 100, 512, 2000);
		e.launches = triangle_launches(0, 700, 512);
		cases.push_back(e);
	}
	{	// a regrouped set: a permutation of the ids, pairs in either order, one triangle
		Case c = even("regrouped n=140: a permutation, one triangle", 140, 0, 140, 128, 1500);
		c.ids = shuffled(140, 7);
		cases.push_back(c);
		Case d = c; d.name = "regrouped n=100 a0=10 of a permutation of 140"; d.slice_a0 = 10; d.n = 100;
		cases.push_back(d);
	}
	{	// the default mode with missing data: a plain pass over the pairs without missing data, then the regrouped set's front group
		// against itself (triangle) and against the rest (rectangle)
		Case c = even("regrouped n=140: plain pass + front triangle + front x rest", 140, 0, 140, 128, 1500);
		c.front.assign(140, 0);
		for (uint32_t v = 0; v < 140; ++v) c.front[v] = (v * 7 + 3) % 5 < 2;
		for (uint32_t v = 0; v < 140; ++v) if (c.front[v]) c.ids.push_back(v);
		const uint32_t nG = (uint32_t)c.ids.size();
		for (uint32_t v = 0; v < 140; ++v) if (!c.front[v]) c.ids.push_back(v);
		c.split = c.first_ids_launch = (uint32_t)c.launches.size();
		for (const LaunchGeom& g : triangle_launches(0, nG, 128)) c.launches.push_back(g);
		c.launches.push_back(LaunchGeom{0, nG, nG, 140 - nG, false});
		cases.push_back(c);
	}
	{	// ... and as two passes over the same file-order launches (a slice of the file: plain planes, then the masked ones)
		Case c = even("two passes over one plain set n=203 a0=37", 300, 37, 203, 128, 2000);
		c.front.assign(300, 0);
		for (uint32_t v = 0; v < 300; ++v) c.front[v] = v % 3 == 1;
		c.split = (uint32_t)c.launches.size();
		for (const LaunchGeom& g : triangle_launches(37, 203, 128)) c.launches.push_back(g);
		cases.push_back(c);
	}
	{	// unsorted positions are refused by the layout
		uint32_t pos[3] = {100, 90, 200}, rid[3] = {0, 0, 0}, first[3]; uint64_t ptr[4];
		const bool sorted = bm_layout(3, [&](uint32_t k) { return pos[k]; }, [&](uint32_t k) { return rid[k]; }, 50, first, ptr);
		uint32_t rid2[3] = {1, 0, 0}, pos2[3] = {1, 2, 3};
		const bool sorted2 = bm_layout(3, [&](uint32_t k) { return pos2[k]; }, [&](uint32_t k) { return rid2[k]; }, 50, first, ptr);
		BandLayout L;
		const bool sorted3 = bm_band_layout(3, [&](uint32_t k) { return pos[k]; }, [&](uint32_t k) { return rid[k]; }, 50, L);
		const bool sorted4 = bm_band_layout(3, [&](uint32_t k) { return pos2[k]; }, [&](uint32_t k) { return rid2[k]; }, 50, L);
		std::printf("  %-66s %s\n", "unsorted positions and contigs are refused", (sorted || sorted2 || sorted3 || sorted4) ? "BAD" : "ok");
		if (sorted || sorted2 || sorted3 || sorted4) { std::printf("bandmat-check: layout accepted unsorted variants\n"); return 1; }
	}
	long bad = 0;
	for (const Case& c : cases) bad += run_case(c) ? 1 : 0;
	std::printf("bandmat-check: %zu cases, %ld bad\n", cases.size(), bad);
	return bad ? 1 : 0;
}
