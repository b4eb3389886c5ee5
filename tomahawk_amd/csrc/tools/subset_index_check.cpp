// The sample selection's table, compress and split (csrc/hip/ld_subset_index.h) played on the host: `make subset-check` builds this file
// with g++ under AddressSanitizer and UBSan and runs it.  Per case - a source size and a keep list - one row of random 2-bit fields
// goes through the steps of k_subset_rows (ld_subset.hip.h): every block (chunk of output words), every lane of its 256 over the
// chunk's entries, the compress, the scatter into the block's window, the store of the window - against an array of write counts with a
// border on either side, and against a gather that moves one field at a time.
// A case fails unless every word of the output row - padding included - was stored exactly once, nothing was stored outside it, the
// row equals the naive gather's, its padding is zero, every source word read lies inside the source row, the table lists exactly the
// source words with a kept sample, and no piece was ORed outside its block's window.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "../hip/ld_subset_index.h"

using namespace twk;

namespace {

constexpr uint32_t KC = 32;                      // the rows' pitch is a multiple of this many words (ld_count_table.h)
constexpr size_t BORDER = 512;
uint32_t round_up(uint32_t x, uint32_t m) { return (x + m - 1) / m * m; }
uint32_t pitch_of(uint32_t n_samples) { return round_up((uint32_t)((2ull * n_samples + 31) / 32), KC); }

struct Case { std::string name; uint32_t n_source; std::vector<uint32_t> keep; };

long play(const Case& cs, std::mt19937& rng) {
	long bad = 0;
	const uint32_t n_keep = (uint32_t)cs.keep.size();
	const uint32_t w_src = pitch_of(cs.n_source), w_dst = pitch_of(n_keep);
	std::vector<uint32_t> src(w_src, 0);
	for (uint32_t s = 0; s < cs.n_source; ++s) src[s >> 4] |= (uint32_t)(rng() & 3u) << (2 * (s & 15));
	// the definition: one field at a time
	std::vector<uint32_t> want(w_dst, 0);
	for (uint32_t k = 0; k < n_keep; ++k) want[k >> 4] |= ((src[cs.keep[k] >> 4] >> (2 * (cs.keep[k] & 15))) & 3u) << (2 * (k & 15));

	std::vector<SubsetEntry> table; std::vector<SubsetChunk> chunks;
	if (!build_subset_table(cs.keep.data(), n_keep, cs.n_source, w_dst, table, chunks)) { std::printf("  %s: the table was refused\n", cs.name.c_str()); return 1; }
	// the table: exactly the source words with a kept sample, ascending, the offsets the prefix sums
	{
		std::vector<uint8_t> has((size_t)w_src, 0);
		for (uint32_t s : cs.keep) has[s >> 4] = 1;
		size_t n_has = 0; for (uint8_t h : has) n_has += h;
		if (n_has != table.size()) ++bad;
		uint32_t bit = 0;
		for (size_t i = 0; i < table.size(); ++i) {
			const SubsetEntry& e = table[i];
			if (e.src_word >= w_src || !has[e.src_word] || (i && e.src_word <= table[i - 1].src_word)) ++bad;
			if (e.out_bit != bit || e.n_bits != (uint32_t)__builtin_popcount(e.mask) || e.n_bits == 0 || (e.mask & 0x55555555u) != ((e.mask >> 1) & 0x55555555u)) ++bad;
			bit += e.n_bits;
		}
		if (bit != 2 * n_keep) ++bad;
	}
	if (chunks.size() != (w_dst + SUBSET_CHUNK - 1) / SUBSET_CHUNK) ++bad;

	std::vector<uint32_t> writes(w_dst + 2 * BORDER, 0), out(w_dst + 2 * BORDER, 0xDEADBEEFu);
	long outside_window = 0, outside_source = 0;
	for (uint32_t bx = 0; bx < chunks.size(); ++bx) {                       // a block
		const uint32_t j0 = bx * SUBSET_CHUNK;
		const uint32_t n_words = w_dst - j0 < SUBSET_CHUNK ? w_dst - j0 : SUBSET_CHUNK;
		std::vector<uint32_t> win(SUBSET_CHUNK + 2 * BORDER, 0);            // the window, with a border of its own
		const SubsetChunk ch = chunks[bx];
		if (ch.e_begin > ch.e_end || ch.e_end > table.size()) { ++bad; continue; }
		for (uint32_t tid = 0; tid < 256; ++tid)                            // a lane
			for (uint32_t e = ch.e_begin + tid; e < ch.e_end; e += 256) {
				const SubsetEntry d = table[e];
				if (d.src_word >= w_src) { ++outside_source; continue; }
				subset_scatter(subset_compress(src[d.src_word], d), d.out_bit, j0, n_words, [&](uint32_t w, uint32_t bits) {
					if (w >= n_words) ++outside_window;
					win[BORDER + w] |= bits;
				});
			}
		for (size_t i = 0; i < win.size(); ++i) if ((i < BORDER || i >= BORDER + n_words) && win[i]) ++outside_window;
		for (uint32_t tid = 0; tid < 256; ++tid)
			if (tid < n_words) { ++writes[BORDER + j0 + tid]; out[BORDER + j0 + tid] = win[BORDER + tid]; }
		// every entry that is NOT in the chunk's range must have nothing to give to it
		for (uint32_t e = 0; e < table.size(); ++e) {
			if (e >= ch.e_begin && e < ch.e_end) continue;
			subset_scatter(subset_compress(0xFFFFFFFFu, table[e]), table[e].out_bit, j0, n_words, [&](uint32_t, uint32_t) { ++bad; });
		}
	}
	bad += outside_window + outside_source;
	for (size_t i = 0; i < writes.size(); ++i) {
		const bool inside = i >= BORDER && i < BORDER + w_dst;
		if (writes[i] != (inside ? 1u : 0u)) ++bad;
		if (inside && out[i] != want[i - BORDER]) ++bad;
	}
	// the padding: nothing behind the last kept sample
	for (uint64_t b = 2ull * n_keep; b < (uint64_t)w_dst * 32; ++b) if ((out[BORDER + (b >> 5)] >> (b & 31)) & 1u) { ++bad; break; }
	if (bad) std::printf("  %s: %ld bad\n", cs.name.c_str(), bad);
	return bad;
}

void add(std::vector<Case>& cases, const std::string& name, uint32_t n, std::vector<uint32_t> keep) {
	if (keep.empty() || keep.back() >= n) return;                           // the list does not fit this size
	cases.push_back(Case{name + " of " + std::to_string(n), n, std::move(keep)});
}
std::vector<uint32_t> run(uint32_t a, uint32_t b) { std::vector<uint32_t> v; for (uint32_t s = a; s < b; ++s) v.push_back(s); return v; }

}  // namespace

int main() {
	std::mt19937 rng(20240611u);
	std::vector<Case> cases;
	for (uint32_t n : {1u, 15u, 16u, 17u, 31u, 32u, 33u, 140u, 161u, 512u, 513u, 1000u, 5000u}) {
		add(cases, "everything", n, run(0, n));
		add(cases, "the first", n, {0});
		add(cases, "the last", n, {n - 1});
		{ std::vector<uint32_t> v; for (uint32_t s = 0; s < n; s += 2) v.push_back(s); add(cases, "every second", n, v); }
		add(cases, "the first 16", n, run(0, 16));
		if (n >= 17) add(cases, "the last 17", n, run(n - 17, n));
		add(cases, "the run [15, 33)", n, run(15, 33));
		if (n >= 3) add(cases, "3 of the whole", n, {0, n / 2, n - 1});
		for (double density : {0.01, 0.5, 0.99}) {
			std::vector<uint32_t> v;
			std::uniform_real_distribution<double> u(0.0, 1.0);
			for (uint32_t s = 0; s < n; ++s) if (u(rng) < density) v.push_back(s);
			add(cases, "random at " + std::to_string(density).substr(0, 4), n, v);
		}
	}
	long bad = 0;
	for (const Case& cs : cases) bad += play(cs, rng) ? 1 : 0;
	// refusals of the builder: unsorted, a duplicate, an index == n, an empty list
	{
		std::vector<SubsetEntry> t; std::vector<SubsetChunk> c; uint32_t at = 99;
		const uint32_t a[] = {3, 2}, b[] = {1, 1}, d[] = {0, 5, 10};
		if (build_subset_table(a, 2, 10, 32, t, c, &at) || at != 1) ++bad;
		if (build_subset_table(b, 2, 10, 32, t, c, &at) || at != 1) ++bad;
		if (build_subset_table(d, 3, 10, 32, t, c, &at) || at != 2) ++bad;
		if (build_subset_table(d, 0, 10, 32, t, c, &at)) ++bad;
		cases.push_back(Case{"refusals", 0, {}});
	}
	// the move mask of the one-bit step is zero for every mask of whole fields (all 65,536 of them)
	for (uint32_t f = 0; f < 65536; ++f) {
		uint32_t mask = 0, mv0 = 1, mv[4];
		for (int k = 0; k < 16; ++k) if ((f >> k) & 1u) mask |= 3u << (2 * k);
		subset_move_masks(mask, mv0, mv);
		if (mv0) { ++bad; break; }
	}
	std::printf("subset-check: %zu cases, %ld bad\n", cases.size(), bad);
	return bad ? 1 : 0;
}
