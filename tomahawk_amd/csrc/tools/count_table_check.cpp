// `make count-check`: the work table of a count launch (csrc/hip/ld_count_table.h) built on the CPU for a grid of small cases and held to a
// naive restatement of what it promises - which tiles, in patch order; units that partition every tile's K range; queues that hold every
// unit once; a packed image that reads back - and to the recorded order: tests/golden/count_tables.json holds one FNV-1a-64 per case of the
// packed table followed by first_split, n_queues and the queues' bounds queue_begin[0 .. n_queues].  The order in which blocks walk the tiles was tuned and no result
// test sees it, so a differing hash is a failure.  Also count_last_halves against the rule spelled out.  Host code only, under
// AddressSanitizer and UBSan.
// usage: count_table_check <count_tables.json>        check
//        count_table_check --record                   print the file for the tables as they are built now (after an intended change of the order)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>
#include "../hip/ld_count_table.h"

using namespace twk;

namespace {

int g_bad_checks = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_bad_checks < 40) { fprintf(stderr, "    FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } ++g_bad_checks; } } while (0)

// Tile kinds: what limits the tiles of the rectangle
enum Kind { RECT = 0, DIAG, RECT_RANGES, DIAG_RANGES, DIAG_RANGES_ZONES, RECT_ZONES, N_KINDS };
const char* const KIND_NAME[N_KINDS] = {"rect", "diag", "rect+cr", "diag+cr", "diag+cr+zones", "rect+zones"};

struct Case {
	uint32_t gy, gx;            // tiles per axis
	int P;                      // planes per variant
	int kind;
	uint32_t nchunks;
	CountSettings s;
	std::string name() const {
		char b[160];
		snprintf(b, sizeof(b), "%ux%u P%d %s p%ux%u c%u b%u m%u s%u q%u f%d", gy, gx, P, KIND_NAME[kind], s.patch_rows, s.patch_cols, nchunks, s.n_blocks,
		         s.min_chunks, s.seg_chunks, s.xcd_queues, s.fused ? 1 : 0);
		return b;
	}
};

// The geometry of a case: variant counts that are no multiple of the tile, a region around the tile for the column ranges (so that they
// are clipped to the tile), a probe zone that ends where the first row of tiles does and a list zone that ends inside the fourth
struct Shape {
	twk_hip_tile_desc t{};
	bool diag = false;
	std::vector<uint32_t> lo, hi;
	ColRange cr;
	bool with_cr = false;
};
uint32_t variants_for(uint32_t tiles, int P) { return (tiles * TILE - 5) / P; }      // P * n rounds up to `tiles` tiles and is no multiple of TILE
// (on the heap: the ranges point into the shape's own vectors)
Shape* make_shape(const Case& c) {
	Shape* sh = new Shape;
	const bool diag = c.kind == DIAG || c.kind == DIAG_RANGES || c.kind == DIAG_RANGES_ZONES;
	const bool ranges = c.kind == RECT_RANGES || c.kind == DIAG_RANGES || c.kind == DIAG_RANGES_ZONES;
	const bool zones = c.kind == DIAG_RANGES_ZONES || c.kind == RECT_ZONES;
	sh->diag = diag;
	sh->t.rowA0 = 1000; sh->t.rowB0 = diag ? 1000 : 1040;
	sh->t.nA = variants_for(c.gy, c.P); sh->t.nB = variants_for(c.gx, c.P);
	sh->t.diag = diag ? 1 : 0;
	if (ranges || zones) {
		sh->with_cr = true;
		sh->cr.a0 = sh->t.rowA0 - 10; sh->cr.b0 = sh->t.rowB0 - 7;
	}
	if (ranges) {
		// a band: row variant v reaches the columns of the 150 variants around its own place (diag: behind itself), monotone and overlapping
		const uint32_t nRA = sh->t.nA + 25, nRB = sh->t.nB + 30, win = 150;
		sh->lo.resize(nRA); sh->hi.resize(nRA);
		for (uint32_t r = 0; r < nRA; ++r) {
			const uint64_t centre = diag ? (uint64_t)r + 4 : (uint64_t)r * nRB / nRA;
			sh->lo[r] = (uint32_t)(diag ? centre : (centre > win ? centre - win : 0));
			sh->hi[r] = (uint32_t)std::min<uint64_t>(nRB, centre + win);
			if (sh->lo[r] > sh->hi[r]) sh->lo[r] = sh->hi[r];
		}
		sh->cr.lo = sh->lo.data(); sh->cr.hi = sh->hi.data();
	}
	if (zones) {
		sh->cr.probe_zone = sh->t.rowA0 + (TILE + c.P - 1) / c.P;      // exactly the end of the first row of tiles
		sh->cr.list_zone = sh->t.rowA0 + (uint32_t)(3.2 * TILE / c.P);
	}
	return sh;
}

// ---- the naive restatement: is tile (by, bx) wanted?
bool tile_wanted(const Shape& sh, int P, uint32_t by, uint32_t bx) {
	const twk_hip_tile_desc& t = sh.t;
	if (sh.diag && bx < by) return false;
	// the variants with a plane row in the tile's rows / columns, as absolute indices
	std::vector<uint64_t> rows, cols;
	for (uint32_t v = 0; v < t.nA; ++v) if ((uint64_t)v * P < (uint64_t)(by + 1) * TILE && (uint64_t)(v + 1) * P > (uint64_t)by * TILE) rows.push_back((uint64_t)t.rowA0 + v);
	if (!sh.with_cr) return true;
	if (sh.cr.lo) {
		bool reached = false;
		for (const uint64_t v : rows) {
			const uint64_t c_lo = (uint64_t)sh.cr.b0 + sh.cr.lo[v - sh.cr.a0], c_hi = (uint64_t)sh.cr.b0 + sh.cr.hi[v - sh.cr.a0];
			for (uint64_t cv = std::max<uint64_t>(c_lo, t.rowB0); cv < c_hi && cv < (uint64_t)t.rowB0 + t.nB && !reached; ++cv) {
				const uint64_t p0 = (cv - t.rowB0) * P, p1 = p0 + P;      // the column variant's plane rows [p0, p1)
				reached = p0 < (uint64_t)(bx + 1) * TILE && p1 > (uint64_t)bx * TILE;
			}
			if (reached) break;
		}
		if (!reached) return false;
	}
	if (sh.cr.list_zone) {
		bool below_probe = true, below_list = true;
		for (const uint64_t v : rows) { below_probe = below_probe && v < sh.cr.probe_zone; below_list = below_list && v < sh.cr.list_zone; }
		if (below_probe) return false;
		// wholly inside the list zone: only from the tile on that holds the first plane row of the first column variant beyond the zone
		if (below_list && sh.cr.list_zone > t.rowB0 && (uint64_t)bx * TILE + (TILE - 1) < ((uint64_t)sh.cr.list_zone - t.rowB0) * P) return false;
	}
	return true;
}

uint64_t fnv1a64(uint64_t h, const void* data, size_t n) {
	const unsigned char* p = static_cast<const unsigned char*>(data);
	for (size_t k = 0; k < n; ++k) { h ^= p[k]; h *= 1099511628211ull; }
	return h;
}

// One case: the invariants (failures counted in g_bad_checks) and the hash of the packed table
uint64_t check_case(const Case& c) {
	Shape* sh = make_shape(c);
	const CountTable tb = build_count_table(sh->t, c.P, sh->diag, sh->with_cr ? &sh->cr : nullptr, c.nchunks, c.s);
	const uint32_t T = tb.n_tiles(), U = tb.n_units();
	CHECK(tb.g.gy == c.gy && tb.g.gx == c.gx && tb.g.ldc == c.gx * TILE, "grid %u x %u", tb.g.gy, tb.g.gx);
	// tiles: exactly the wanted ones, each once, in patch order
	{
		std::vector<uint8_t> seen((size_t)c.gy * c.gx, 0);
		for (uint32_t k = 0; k < T; ++k) {
			const uint32_t by = tb.tiles[k] >> 16, bx = tb.tiles[k] & 0xFFFFu;
			CHECK(by < c.gy && bx < c.gx, "tile %u = (%u, %u)", k, by, bx);
			if (by < c.gy && bx < c.gx) { CHECK(!seen[(size_t)by * c.gx + bx], "tile (%u, %u) twice", by, bx); seen[(size_t)by * c.gx + bx] = 1; }
		}
		for (uint32_t by = 0; by < c.gy; ++by) for (uint32_t bx = 0; bx < c.gx; ++bx)
			CHECK((seen[(size_t)by * c.gx + bx] != 0) == tile_wanted(*sh, c.P, by, bx), "tile (%u, %u) listed %d", by, bx, (int)seen[(size_t)by * c.gx + bx]);
		auto patch_of = [&](uint32_t yx) { return (uint64_t)((yx >> 16) / c.s.patch_rows) << 32 | (yx & 0xFFFFu) / c.s.patch_cols; };
		for (uint32_t k = 1; k < T; ++k) {
			const uint64_t pa = patch_of(tb.tiles[k - 1]), pb = patch_of(tb.tiles[k]);
			CHECK(pa < pb || (pa == pb && tb.tiles[k - 1] < tb.tiles[k]), "tiles %u, %u out of patch order", k - 1, k);
		}
		CHECK(tb.patch_end.empty() == (T == 0) && (T == 0 || tb.patch_end.back() == T), "patch_end ends at %u of %u", tb.patch_end.empty() ? 0 : tb.patch_end.back(), T);
		uint32_t p0 = 0;
		for (size_t p = 0; p < tb.patch_end.size() && tb.patch_end[p] <= T; ++p) {
			const uint32_t p1 = tb.patch_end[p];
			CHECK(p1 > p0, "patch_end[%zu] = %u not ascending", p, p1);
			for (uint32_t k = p0 + 1; k < p1; ++k) CHECK(patch_of(tb.tiles[k]) == patch_of(tb.tiles[p0]), "tile %u in patch %zu", k, p);
			if (p1 < T && p1 > p0) CHECK(patch_of(tb.tiles[p1]) != patch_of(tb.tiles[p0]), "patch %zu ends inside a patch", p);
			p0 = p1;
		}
	}
	// units: every tile's K range partitioned; split tiles behind first_split
	{
		std::vector<std::vector<std::pair<uint32_t, uint32_t>>> of(T);
		for (uint32_t u = 0; u < U; ++u) {
			const CountUnit& cu = tb.units[u];
			CHECK(cu.tile < T && cu.c0 < cu.c1 && cu.c1 <= c.nchunks, "unit %u = tile %u [%u, %u)", u, cu.tile, cu.c0, cu.c1);
			if (cu.tile >= T) continue;
			CHECK(cu.yx == tb.tiles[cu.tile], "unit %u yx", u);
			of[cu.tile].push_back({cu.c0, cu.c1});
		}
		CHECK(tb.first_split <= T, "first_split %u of %u", tb.first_split, T);
		for (uint32_t k = 0; k < T; ++k) {
			std::sort(of[k].begin(), of[k].end());
			uint32_t at = 0;
			for (const auto& r : of[k]) { CHECK(r.first == at, "tile %u: [%u, %u) after %u", k, r.first, r.second, at); at = r.second; }
			CHECK(at == c.nchunks, "tile %u covered to %u of %u", k, at, c.nchunks);
			if (of[k].size() > 1) CHECK(k >= tb.first_split, "tile %u split before first_split %u", k, tb.first_split);
			if (c.s.fused) CHECK(of[k].size() == 1, "fused: tile %u in %zu units", k, of[k].size());
		}
	}
	// queues: [queue_begin[q], queue_begin[q + 1]) of the unit table, together all of it
	CHECK(tb.n_queues >= 1 && tb.n_queues <= 8 && tb.queue_begin[0] == 0, "%u queues from %u", tb.n_queues, tb.queue_begin[0]);
	for (uint32_t q = 0; q < 8; ++q) CHECK(tb.queue_begin[q] <= tb.queue_begin[q + 1], "queue_begin[%u]", q);
	for (uint32_t q = tb.n_queues; q <= 8; ++q) CHECK(tb.queue_begin[q] == U, "queue_begin[%u] = %u of %u units", q, tb.queue_begin[q], U);
	// the packed image
	CHECK(tb.units_at() % 4 == 0 && tb.words() % 4 == 0 && tb.units_at() >= T && tb.words() == tb.units_at() + (size_t)U * 4, "units at %zu of %zu words", tb.units_at(), tb.words());
	std::vector<uint32_t> img(tb.words() + 4, 0xA5A5A5A5u);
	tb.pack(img.data());
	CHECK(T == 0 || std::memcmp(img.data(), tb.tiles.data(), (size_t)T * 4) == 0, "tiles read back");
	CHECK(U == 0 || std::memcmp(img.data() + tb.units_at(), tb.units.data(), (size_t)U * sizeof(CountUnit)) == 0, "units read back");
	for (size_t k = tb.words(); k < img.size(); ++k) CHECK(img[k] == 0xA5A5A5A5u, "pack wrote word %zu of %zu", k, tb.words());
	uint64_t h = fnv1a64(14695981039346656037ull, img.data(), tb.words() * 4);
	const uint32_t head[2] = {tb.first_split, tb.n_queues};
	h = fnv1a64(h, head, sizeof(head));
	h = fnv1a64(h, tb.queue_begin, (tb.n_queues + 1) * sizeof(uint32_t));
	delete sh;
	return h;
}

// The cases, a subset of the cross product chosen to keep the recorded file small.  Every geometry (grids of 1, 2, 9 and 17 tiles an
// axis, square and not; 1, 2, 3 planes; every tile kind) once, the six settings below - which between them take every path of the
// builder - and the two patch shapes dealt round over them.  Then, on two geometries of many tiles, the settings that act together:
// nchunks x n_blocks x min_chunks for the guided tail, seg and xcd_queues on the rows long enough for them and on one that is not, and
// fused with and without the settings it overrides.
std::vector<Case> all_cases() {
	static const uint32_t GRIDS[6][2] = {{1, 1}, {2, 2}, {9, 9}, {17, 17}, {2, 9}, {9, 17}};
	static const uint32_t PATCH[2][2] = {{8, 8}, {16, 32}};
	static const uint32_t NCHUNKS[7] = {1, 3, 15, 16, 17, 128, 300}, NBLOCKS[3] = {1, 4, 512}, MINCH[2] = {1, 8}, SEG[3] = {0, 32, 64}, XQ[3] = {0, 2, 8};
	auto settings = [](const uint32_t* patch, uint32_t nb, uint32_t mc, uint32_t seg, uint32_t xq, bool fused) {
		CountSettings s; s.patch_rows = patch[0]; s.patch_cols = patch[1]; s.n_blocks = nb; s.min_chunks = mc; s.seg_chunks = seg; s.xcd_queues = xq; s.fused = fused; return s;
	};
	std::vector<Case> cases;
	std::set<std::string> names;
	auto add = [&](const Case& c) { if (names.insert(c.name()).second) cases.push_back(c); };
	uint32_t k = 0;
	for (const auto& g : GRIDS) for (int P = 1; P <= 3; ++P) for (int kind = 0; kind < N_KINDS; ++kind, ++k) {
		const uint32_t* p = PATCH[(k / 6) % 2];
		switch ((k + k / 6) % 6) {      // (six kinds, six settings: shifted by one from one (grid, planes) to the next)
		case 0: add(Case{g[0], g[1], P, kind, 16, settings(p, 512, 8, 0, 0, false)}); break;       // the default: whole tiles, a guided tail
		case 1: add(Case{g[0], g[1], P, kind, 300, settings(p, 4, 8, 64, 0, false)}); break;       // segmented walk
		case 2: add(Case{g[0], g[1], P, kind, 128, settings(p, 4, 1, 32, 8, false)}); break;       // a queue per XCD, segmented
		case 3: add(Case{g[0], g[1], P, kind, 300, settings(p, 512, 8, 0, 2, false)}); break;      // two queues of whole tiles
		case 4: add(Case{g[0], g[1], P, kind, 17, settings(p, 1, 1, 0, 0, false)}); break;         // one block: every tile split
		default: add(Case{g[0], g[1], P, kind, 3, settings(p, 512, 8, 32, 8, true)}); break;       // fused: whole tiles whatever else is asked
		}
	}
	static const struct { uint32_t gy, gx; int P, kind, patch; } MANY[2] = {{17, 17, 2, DIAG, 0}, {9, 17, 3, DIAG_RANGES_ZONES, 1}};
	for (const auto& f : MANY) {
		const uint32_t* p = PATCH[f.patch];
		for (const uint32_t nc : NCHUNKS) for (const uint32_t nb : NBLOCKS) for (const uint32_t mc : MINCH) add(Case{f.gy, f.gx, f.P, f.kind, nc, settings(p, nb, mc, 0, 0, false)});
		for (const uint32_t nc : {17u, 128u, 300u}) for (const uint32_t seg : SEG) for (const uint32_t xq : XQ) for (const uint32_t mc : MINCH) add(Case{f.gy, f.gx, f.P, f.kind, nc, settings(p, 4, mc, seg, xq, false)});
		for (const uint32_t nc : {1u, 16u, 300u}) { add(Case{f.gy, f.gx, f.P, f.kind, nc, settings(p, 512, 8, 0, 0, true)}); add(Case{f.gy, f.gx, f.P, f.kind, nc, settings(p, 4, 1, 64, 2, true)}); }
	}
	return cases;
}

// {"<case>": "<16 hex digits>", ...}: every pair of quoted strings of the file
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

// count_last_halves against the rule said in words: of the last chunk's live words, two to a half-slot, rounded up - and all sixteen (0)
// when that would spare less than a quarter of the chunk, when nothing is live or when the padding is a whole chunk or more
int check_last_halves() {
	const int before = g_bad_checks;
	for (uint32_t live = 1; live <= 5 * (uint32_t)KC; ++live) {
		const uint32_t W = (live + KC - 1) / KC * KC;
		uint32_t in_last = live % KC; if (!in_last) in_last = KC;
		uint32_t halves = 0; for (uint32_t w = 0; w < in_last; w += 2) ++halves;
		const uint32_t want = halves >= 13 ? 0 : halves;
		CHECK(count_last_halves(live, W) == want, "count_last_halves(%u, %u) = %u, not %u", live, W, count_last_halves(live, W), want);
		CHECK(count_last_halves(live, W + KC) == 0 && count_last_halves(live, W + 3 * KC) == 0, "count_last_halves(%u, %u + whole chunks)", live, W);
	}
	for (uint32_t W = 0; W <= 5 * (uint32_t)KC; W += KC) CHECK(count_last_halves(0, W) == 0, "count_last_halves(0, %u)", W);
	return g_bad_checks != before;
}

}  // namespace

int main(int argc, char** argv) {
	const bool record = argc > 1 && std::strcmp(argv[1], "--record") == 0;
	if (argc < 2) { fprintf(stderr, "usage: count_table_check <count_tables.json> | --record\n"); return 2; }
	std::map<std::string, std::string> golden;
	if (!record && !read_golden(argv[1], golden)) { fprintf(stderr, "count-check: cannot read %s\n", argv[1]); return 2; }
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
	const int bad_rule = check_last_halves(); ++n; bad += bad_rule;
	fprintf(record ? stderr : stdout, "count-check: %d cases, %d bad\n", n, bad);
	return bad != 0;
}
