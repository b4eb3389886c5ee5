// The sample relationship's index header (csrc/hip/ld_relate_index.h) played on the host: `make relate-check` builds this file with
// g++ -fsanitize=address,undefined and runs it.  Everything goes against a naive restatement that shares no arithmetic with it:
//   the transposition   every lane of every block of k_relate_transpose's grid, through the header's own position, group, staging and
//                       write-out functions, into a plane set whose live rows start as garbage - against bit (sample, plane, position)
//                       set one at a time from the genotypes.  Every word of the live rows is written exactly once, the padding bits and
//                       the padding rows are zero, the list's last partial word is right, no staged word has two writers;
//   the counts          rl_counts on plane products (popcounts of the transposed rows; the two-plane form's margins from the rows'
//                       popcounts) against the six counts taken genotype by genotype;
//   the epilogue        every lane of every block of k_relate_epilogue's grid over a count matrix in which only the tiles the count kernel
//                       contracts hold values and the rest is poison: no poison is read, every entry of the output is stored exactly once,
//                       the mirrored entry carries het_a and het_b swapped.
// Shapes (samples x variants): the smallest that cross each boundary - the 64-lane ballot, the 16-sample raw word, the 1024-variant chunk,
// one tile of 128 plane rows and two - with and without missing genotypes, and a variant list.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../hip/ld_relate_index.h"

using namespace twk;

namespace {

int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures < 20) { fprintf(stderr, "BAD %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } ++failures; } } while (0)

uint64_t rng_state = 0x2545F4914F6CDD1Dull;
uint64_t rng() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

struct Data {
	uint32_t N, M, Wp;
	std::vector<uint8_t> g;             // [M][N]: 0, 1, 2 ALT alleles, 3 missing
	std::vector<uint32_t> raw, mask;    // [M][Wp]
	uint8_t at(uint32_t v, uint32_t s) const { return g[(size_t)v * N + s]; }
};

Data make_data(uint32_t N, uint32_t M, bool missing) {
	Data d; d.N = N; d.M = M;
	d.Wp = ((2 * N + 31) / 32 + 31) / 32 * 32;
	d.g.resize((size_t)M * N); d.raw.assign((size_t)M * d.Wp, 0); d.mask.assign((size_t)M * d.Wp, 0);
	for (uint32_t v = 0; v < M; ++v) {
		const bool vm = missing && (v % 3 == 1);
		for (uint32_t s = 0; s < N; ++s) {
			const uint64_t r = rng();
			uint8_t x = (uint8_t)(r % 3);
			if (vm && (r >> 8) % 7 == 0) x = 3;
			d.g[(size_t)v * N + s] = x;
			const uint32_t w = s / 16, sh = 2 * (s % 16);
			// 1: one ALT allele, on either haplotype (phase is ignored); a missing genotype carries arbitrary allele bits under its mask
			const uint32_t bits = x == 0 ? 0u : x == 1 ? ((r >> 20) & 1 ? 1u : 2u) : x == 2 ? 3u : (uint32_t)((r >> 24) & 3);
			d.raw[(size_t)v * d.Wp + w] |= bits << sh;
			if (x == 3) d.mask[(size_t)v * d.Wp + w] |= 3u << sh;
		}
	}
	return d;
}

// k_relate_transpose, lane by lane
std::vector<uint32_t> play_transpose(const Data& d, const std::vector<uint32_t>& ids, uint32_t P, uint32_t W, uint64_t rows_alloc) {
	const uint32_t L = (uint32_t)ids.size(), live_rows = d.N * P;
	std::vector<uint32_t> rows((size_t)rows_alloc * W, 0);
	std::vector<uint8_t> written((size_t)rows_alloc * W, 0);
	for (size_t k = 0; k < (size_t)live_rows * W; ++k) rows[k] = 0xDEADBEEFu;
	const uint32_t gx = (d.N + RL_BLOCK_SAMPLES - 1) / RL_BLOCK_SAMPLES, n_chunks = W / RL_KC;
	for (uint32_t bx = 0; bx < gx; ++bx) for (uint32_t chunk = 0; chunk < n_chunks; ++chunk) for (uint32_t pass = 0; pass < RL_PASSES; ++pass) {
		std::vector<uint32_t> stage(RL_STAGE_WORDS, 0);
		std::vector<uint8_t> staged(RL_STAGE_WORDS, 0);
		const uint32_t w0 = rl_raw_word(bx, pass);
		CHECK(w0 + 3 < d.Wp, "raw word %u of %u", w0 + 3, d.Wp);
		for (uint32_t wave = 0; wave < 4; ++wave) for (uint32_t k = 0; k < 4; ++k) {
			const uint32_t g = rl_group(wave, k);
			CHECK(g < RL_GROUPS, "group %u", g);
			for (uint32_t i = 0; i < RL_PASS_SAMPLES; ++i) for (uint32_t plane = 0; plane < P; ++plane) {
				uint64_t ballot = 0;
				for (uint32_t lane = 0; lane < 64; ++lane) {
					const uint32_t pos = rl_position(chunk, wave, k, lane);
					if (pos >= L) continue;
					const uint32_t word = d.raw[(size_t)ids[pos] * d.Wp + w0 + i / 16], mword = P == 3 ? d.mask[(size_t)ids[pos] * d.Wp + w0 + i / 16] : 0u;
					ballot |= (uint64_t)rl_plane_bit(plane, P, rl_het(word, i % 16), rl_hom(word, i % 16), rl_miss(mword, i % 16)) << lane;
				}
				for (uint32_t half = 0; half < 2; ++half) {
					const uint32_t st = rl_stage(i, plane, P, 2 * g + half);
					CHECK(st < RL_STAGE_WORDS && !staged[st < RL_STAGE_WORDS ? st : 0], "staged word %u twice or out of range", st);
					if (st < RL_STAGE_WORDS) { stage[st] = (uint32_t)(ballot >> (32 * half)); staged[st] = 1; }
				}
			}
		}
		for (uint32_t item = 0; item < rl_out_items(P); ++item) {
			const uint32_t r = item >> 5, word = item & 31u, i = r / P, plane = r - i * P;
			const uint32_t s = rl_pass_sample(bx, pass, i);
			if (s >= d.N) continue;
			const size_t at = rl_out_index(s, plane, P, W, chunk, word);
			CHECK(at < (size_t)live_rows * W && !written[at < rows.size() ? at : 0], "output word %zu twice or outside the live rows", at);
			if (at < rows.size()) { rows[at] = stage[rl_stage(i, plane, P, word)]; written[at] = 1; }
		}
	}
	for (size_t k = 0; k < (size_t)live_rows * W; ++k) CHECK(written[k], "live word %zu never written", k);
	return rows;
}

RelCounts naive_counts(const Data& d, const std::vector<uint32_t>& ids, uint32_t a, uint32_t b) {
	RelCounts c{0, 0, 0, 0, 0, 0};
	for (const uint32_t v : ids) {
		const uint8_t ga = d.at(v, a), gb = d.at(v, b);
		if (ga == 3 || gb == 3) continue;
		++c.n;
		if ((ga == 0 && gb == 2) || (ga == 2 && gb == 0)) ++c.ibs0;
		if (ga == gb) ++c.ibs2;
		if (ga == 1 && gb == 1) ++c.hethet;
		if (ga == 1) ++c.het_a;
		if (gb == 1) ++c.het_b;
	}
	return c;
}
bool same(const RelCounts& x, const RelCounts& y) { return x.n == y.n && x.ibs0 == y.ibs0 && x.ibs2 == y.ibs2 && x.hethet == y.hethet && x.het_a == y.het_a && x.het_b == y.het_b; }

uint32_t row_and(const std::vector<uint32_t>& rows, uint32_t W, uint64_t r, uint64_t c) {
	uint32_t n = 0;
	for (uint32_t k = 0; k < W; ++k) n += (uint32_t)__builtin_popcount(rows[r * W + k] & rows[c * W + k]);
	return n;
}

int n_cases = 0;

void check_case(uint32_t N, uint32_t M, bool missing, const char* name, uint32_t list_from = 0, uint32_t list_step = 1, uint32_t list_n = 0) {
	const int before = failures;
	const Data d = make_data(N, M, missing);
	std::vector<uint32_t> ids;
	if (list_n) for (uint32_t k = 0; k < list_n; ++k) ids.push_back(list_from + k * list_step);
	else for (uint32_t v = 0; v < M; ++v) ids.push_back(v);
	bool any_missing = false;
	for (const uint32_t v : ids) for (uint32_t s = 0; s < N; ++s) any_missing = any_missing || d.at(v, s) == 3;
	const uint32_t L = (uint32_t)ids.size(), P = rl_planes(any_missing), W = rl_words(L);
	const uint64_t rows_alloc = rl_rows_alloc(N, P);
	CHECK(W % RL_KC == 0 && W >= rl_words_live(L) && W - rl_words_live(L) < RL_KC, "pitch %u for %u positions", W, L);
	CHECK(rows_alloc % RL_TILE == 0 && rows_alloc >= (uint64_t)N * P + RL_TILE, "rows %" PRIu64, rows_alloc);
	const std::vector<uint32_t> rows = play_transpose(d, ids, P, W, rows_alloc);

	// against the naive transposition: one bit at a time
	std::vector<uint32_t> want((size_t)rows_alloc * W, 0);
	for (uint32_t k = 0; k < L; ++k) for (uint32_t s = 0; s < N; ++s) {
		const uint8_t g = d.at(ids[k], s);
		const bool bit[3] = {g == 1, g == 2, g != 3};
		for (uint32_t plane = 0; plane < P; ++plane) if (bit[plane]) want[rl_row(s, plane, P) * W + rl_word(k)] |= 1u << rl_bit(k);
	}
	size_t bad = 0;
	for (size_t k = 0; k < rows.size(); ++k) bad += rows[k] != want[k];
	CHECK(bad == 0, "%zu words differ from the naive transposition", bad);
	// the padding: bits behind the list's last position, words behind its last word, rows behind the last sample
	for (uint64_t r = 0; r < rows_alloc; ++r) for (uint32_t w = 0; w < W; ++w) {
		const uint32_t x = rows[r * W + w];
		if (r >= (uint64_t)N * P || w >= rl_words_live(L)) CHECK(x == 0, "padding word (%" PRIu64 ", %u) = %08x", r, w, x);
		else if (w == rl_words_live(L) - 1 && (L & 31u)) CHECK((x >> (L & 31u)) == 0, "padding bits of the last word of row %" PRIu64 ": %08x", r, x);
	}
	if (L & 31u) {      // the last partial word itself, for the first sample's planes
		for (uint32_t plane = 0; plane < P; ++plane) {
			uint32_t w = 0;
			for (uint32_t k = L & ~31u; k < L; ++k) { const uint8_t g = d.at(ids[k], 0); if (plane == 0 ? g == 1 : plane == 1 ? g == 2 : g != 3) w |= 1u << (k & 31u); }
			CHECK(rows[rl_row(0, plane, P) * W + rl_words_live(L) - 1] == w, "last partial word of plane %u", plane);
		}
	}

	// the epilogue over a square call: one diagonal super-tile (N <= the super-tile's edge here), only the tiles on or above the diagonal hold values
	const uint32_t rows_pad = (N * P + RL_TILE - 1) / RL_TILE * RL_TILE, ldc = rows_pad;
	const uint32_t POISON = 0xFFFFFFFFu;
	std::vector<uint32_t> Cm((size_t)rows_pad * ldc, POISON), pop(rows_alloc, 0);
	const bool full = N <= 64;                  // (the products of every pair for the small shapes, of a sample of the pairs for the others)
	auto fill_pair = [&](uint32_t a, uint32_t b) {
		for (uint32_t i = 0; i < P; ++i) for (uint32_t j = 0; j < P; ++j) {
			const uint32_t r = a * P + i, c = b * P + j;
			if (c / RL_TILE >= r / RL_TILE) Cm[(size_t)r * ldc + c] = row_and(rows, W, r, c);
		}
	};
	std::vector<std::pair<uint32_t, uint32_t>> pairs;
	if (full) { for (uint32_t a = 0; a < N; ++a) for (uint32_t b = a; b < N; ++b) pairs.emplace_back(a, b); }
	else {
		for (uint32_t a = 0; a < N; ++a) pairs.emplace_back(a, a);
		for (int k = 0; k < 400; ++k) { uint32_t a = (uint32_t)(rng() % N), b = (uint32_t)(rng() % N); if (a > b) std::swap(a, b); pairs.emplace_back(a, b); }
	}
	for (const auto& ab : pairs) fill_pair(ab.first, ab.second);
	for (uint64_t r = 0; r < (uint64_t)N * P; ++r) for (uint32_t k = 0; k < W; ++k) pop[r] += (uint32_t)__builtin_popcount(rows[r * W + k]);
	for (const auto& ab : pairs) {
		const uint32_t a = ab.first, b = ab.second;
		int64_t p[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
		bool poison = false;
		for (uint32_t i = 0; i < P; ++i) for (uint32_t j = 0; j < P; ++j) {
			const size_t at = rl_c_index(a, i, b, j, P, ldc, true);
			CHECK(at < Cm.size(), "count index %zu", at);
			poison = poison || Cm[at] == POISON;
			p[i][j] = Cm[at];
		}
		CHECK(!poison, "pair (%u, %u) reads a tile below the diagonal", a, b);
		if (P == 2) { p[0][2] = pop[rl_row(a, 0, 2)]; p[1][2] = pop[rl_row(a, 1, 2)]; p[2][0] = pop[rl_row(b, 0, 2)]; p[2][1] = pop[rl_row(b, 1, 2)]; p[2][2] = L; }
		const RelCounts got = rl_counts(p), wantc = naive_counts(d, ids, a, b);
		CHECK(same(got, wantc), "counts of (%u, %u): n %u/%u ibs0 %u/%u ibs2 %u/%u hethet %u/%u het %u,%u/%u,%u", a, b, got.n, wantc.n, got.ibs0, wantc.ibs0, got.ibs2, wantc.ibs2,
		      got.hethet, wantc.hethet, got.het_a, got.het_b, wantc.het_a, wantc.het_b);
		if (a == b) CHECK(got.ibs2 == got.n && got.ibs0 == 0 && got.hethet == got.het_a && got.het_a == got.het_b, "diagonal (%u, %u)", a, a);
		int64_t num, den;
		rl_fraction(2, got, num, den);
		CHECK(num == (int64_t)wantc.hethet - 2 * (int64_t)wantc.ibs0 && den == (int64_t)wantc.het_a + wantc.het_b, "KING's fraction of (%u, %u)", a, b);
		rl_fraction(0, got, num, den);
		CHECK(num == (int64_t)wantc.n + wantc.ibs2 - wantc.ibs0 && den == 2 * (int64_t)wantc.n && num >= 0, "IBS's fraction of (%u, %u)", a, b);
	}
	// the epilogue's lanes: every entry of the N x N output exactly once, direct or mirrored
	std::vector<uint8_t> hits((size_t)N * N, 0);
	const uint32_t ge = (N + RL_EP - 1) / RL_EP;
	for (uint32_t by = 0; by < ge; ++by) for (uint32_t bx = by; bx < ge; ++bx) {
		std::vector<uint8_t> staged(RL_EP * RL_EP_PITCH, 0);
		for (uint32_t k = 0; k < RL_EP_STEPS; ++k) for (uint32_t tid = 0; tid < RL_THREADS; ++tid) {
			const uint32_t r = rl_ep_row(tid, k), cl = rl_ep_col(tid), a = by * RL_EP + r, b = bx * RL_EP + cl;
			CHECK(r < RL_EP && cl < RL_EP, "epilogue lane (%u, %u)", r, cl);
			if (!rl_ep_live(a, b, N, N, true)) continue;
			++hits[(size_t)a * N + b];
			CHECK(!staged[rl_ep_stage(r, cl)], "staged pair (%u, %u) twice", r, cl);
			staged[rl_ep_stage(r, cl)] = 1;
		}
		for (uint32_t k = 0; k < RL_EP_STEPS; ++k) for (uint32_t tid = 0; tid < RL_THREADS; ++tid) {
			const uint32_t r = rl_ep_col(tid), cl = rl_ep_row(tid, k), a = by * RL_EP + r, b = bx * RL_EP + cl;
			if (!rl_ep_mirrored(a, b, N, N, true)) continue;
			CHECK(staged[rl_ep_stage(r, cl)], "mirrored pair (%u, %u) was not staged", a, b);
			++hits[(size_t)b * N + a];
		}
	}
	size_t not_once = 0;
	for (const uint8_t h : hits) not_once += h != 1;
	CHECK(not_once == 0, "%zu entries of the %u x %u output not stored exactly once", not_once, N, N);

	++n_cases;
	printf("  %-44s P=%u W=%u rows=%" PRIu64 " %s\n", name, P, W, rows_alloc, failures == before ? "ok" : "BAD");
}

}  // namespace

int main() {
	check_case(1, 1, false, "1 x 1");
	check_case(2, 1, false, "2 x 1");
	check_case(3, 63, false, "3 x 63");
	check_case(17, 64, false, "17 x 64");
	check_case(16, 65, false, "16 x 65");
	check_case(43, 1023, true, "43 x 1023 missing");
	check_case(44, 1024, true, "44 x 1024 missing");
	check_case(64, 1024, false, "64 x 1024");
	check_case(129, 1025, false, "129 x 1025");
	check_case(300, 2100, true, "300 x 2100 missing");
	check_case(300, 3100, true, "300 x 1000 of 3100 from 37 by 3 missing", 37, 3, 1000);
	check_case(40, 90, true, "40 x 30 of 90 from 0 by 3: no missing left", 0, 3, 30);
	check_case(257, 33, true, "257 x 33 missing");
	printf("relate-check: %d cases, %d bad\n", n_cases, failures);
	return failures != 0;
}
