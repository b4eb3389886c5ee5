// Sample subsets: the table a selection is compiled into, the compress of one source word and the split of a row by OUTPUT words.
// Plain C++ with no HIP in it, in the manner of ld_bandmat_index.h: k_subset_rows (ld_subset.hip.h) includes it, and so does
// csrc/tools/subset_index_check.cpp (`make subset-check`), which plays every block and lane of the split against a field-by-field gather.
//
// THE LAYOUT is the raw one (twk_hip.h): 2 bits a sample, sample s at bits 2s and 2s + 1 of its row, 16 samples a 32-bit word.  A
// selection keeps the samples keep[0] < keep[1] < ..: sample k of the output row is source sample keep[k].
// THE TABLE holds one SubsetEntry per source word WITH A KEPT SAMPLE, in ascending order, the same for every row: where the word lies,
// which of its fields are kept (mask), the move masks of the parallel-suffix compress (Hacker's Delight 7-4) of that mask, and the bit
// of the output row at which the compressed fields begin, 2 x the kept samples in front of the word.  A field is a PAIR of bits, so the
// compress never moves anything by one bit: its first move mask is always zero (build_subset_table refuses a mask for which it is
// not), and the four steps by 2, 4, 8 and 16 bits are the whole of it.
// THE SPLIT: a block owns the output words [j0, j0 + SUBSET_CHUNK) of a few rows.  SubsetChunk names the entries whose pieces touch them -
// first and last are shared with the neighbouring chunks, which read the same source word again - and a piece, at most 32 bits at any
// bit offset, is ORed into at most two words of the block's window (subset_scatter), the parts outside the window dropped.  Every output
// word belongs to exactly one chunk and is stored once, the padding behind the last kept sample as zeros.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TWK_SUBSET_FN __host__ __device__ inline
#else
#define TWK_SUBSET_FN inline
#endif

namespace twk {

constexpr uint32_t SUBSET_CHUNK = 256;       // output words a block owns: one a thread at the store
constexpr uint32_t SUBSET_ROWS = 8;          // rows a block carries through one pass over its entries (the entry is loaded once for all of them)

struct SubsetEntry {                         // 32 bytes: two 16-byte loads
	uint32_t src_word;                       // the 32-bit word of the source row
	uint32_t out_bit;                        // bit of the output row the compressed fields begin at
	uint32_t mask;                           // the kept fields: both bits of each
	uint32_t mv[4];                          // the compress' move masks of the steps by 2, 4, 8 and 16 bits
	uint32_t n_bits;                         // 2 x the kept samples of the word: the piece's length
};
struct SubsetChunk { uint32_t e_begin, e_end; };      // the entries whose pieces touch the chunk's output words

// The kept fields of x, packed at the low end in their order.
TWK_SUBSET_FN uint32_t subset_compress(uint32_t x, const SubsetEntry& e) {
	x &= e.mask;
	uint32_t t;
	t = x & e.mv[0]; x = (x ^ t) | (t >> 2);
	t = x & e.mv[1]; x = (x ^ t) | (t >> 4);
	t = x & e.mv[2]; x = (x ^ t) | (t >> 8);
	t = x & e.mv[3]; x = (x ^ t) | (t >> 16);
	return x;
}

// A piece that begins at bit out_bit of the row, into the window of the words [j0, j0 + n_words): or(word of the window, bits), for at
// most two words; nothing for the parts outside and nothing for zero bits.  32-bit shifts only.
template <class Or>
TWK_SUBSET_FN void subset_scatter(uint32_t piece, uint32_t out_bit, uint32_t j0, uint32_t n_words, Or&& put) {
	const uint32_t s = out_bit & 31u;
	const uint32_t w = (out_bit >> 5) - j0;                   // (below the window: wraps to a huge number and is refused)
	const uint32_t lo = piece << s, hi = s ? piece >> (32u - s) : 0u;
	if (lo && w < n_words) put(w, lo);
	if (hi && w + 1u < n_words) put(w + 1u, hi);
}

// Move masks of the compress of `mask` -> mv0 (the step by one bit) and mv[4].
inline void subset_move_masks(uint32_t mask, uint32_t& mv0, uint32_t mv[4]) {
	uint32_t m = mask, mk = ~m << 1;
	for (int i = 0; i < 5; ++i) {
		uint32_t mp = mk ^ (mk << 1);
		mp ^= mp << 2; mp ^= mp << 4; mp ^= mp << 8; mp ^= mp << 16;
		const uint32_t v = mp & m;
		m = (m ^ v) | (v >> (1u << i));
		if (i == 0) mv0 = v; else mv[i - 1] = v;
		mk &= ~mp;
	}
}

// The table and the chunks of the strictly ascending list keep[0 .. n_keep) of samples below n_source, for output rows of w_out words
// (>= ceil(2 n_keep / 32): the row's pitch, padding included).  -> false, with nothing promised about the outputs, for an empty list,
// one that is not strictly ascending or reaches n_source, or a pitch too short.  *bad_at (may be NULL): the first offending position.
inline bool build_subset_table(const uint32_t* keep, uint32_t n_keep, uint32_t n_source, uint32_t w_out,
                               std::vector<SubsetEntry>& table, std::vector<SubsetChunk>& chunks, uint32_t* bad_at = nullptr) {
	table.clear(); chunks.clear();
	if (bad_at) *bad_at = 0;
	if (!keep || n_keep == 0 || n_keep > (1u << 30) || (uint64_t)w_out * 32 < 2ull * n_keep) return false;
	for (uint32_t k = 0; k < n_keep; ++k)
		if (keep[k] >= n_source || (k && keep[k] <= keep[k - 1])) { if (bad_at) *bad_at = k; return false; }
	for (uint32_t k = 0; k < n_keep;) {
		SubsetEntry e{};
		e.src_word = keep[k] >> 4;
		e.out_bit = 2u * k;
		for (; k < n_keep && (keep[k] >> 4) == e.src_word; ++k) { e.mask |= 3u << (2u * (keep[k] & 15u)); e.n_bits += 2; }
		uint32_t mv0 = 0;
		subset_move_masks(e.mask, mv0, e.mv);
		if (mv0) return false;                                    // (cannot happen: the fields are pairs of bits)
		table.push_back(e);
	}
	const uint32_t n_chunks = (w_out + SUBSET_CHUNK - 1) / SUBSET_CHUNK;
	chunks.assign(n_chunks, SubsetChunk{0, 0});
	uint32_t b = 0, e = 0;                                        // two pointers that only move forward
	const uint32_t n = (uint32_t)table.size();
	for (uint32_t c = 0; c < n_chunks; ++c) {
		const uint64_t bit0 = (uint64_t)c * SUBSET_CHUNK * 32, bit1 = bit0 + (uint64_t)SUBSET_CHUNK * 32;
		while (b < n && (uint64_t)table[b].out_bit + table[b].n_bits <= bit0) ++b;      // ends in front of the chunk
		if (e < b) e = b;
		while (e < n && table[e].out_bit < bit1) ++e;                                   // begins inside or in front of its end
		chunks[c] = SubsetChunk{b, e};
	}
	return true;
}

}  // namespace twk
