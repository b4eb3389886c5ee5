// Variant subsets: the predicate of one variant, the genotype counts of one raw word and the walk of one lane through the row gather.
// Plain C++ with no HIP in it, in the manner of ld_subset_index.h: the kernels (ld_varsel.hip.h) include it, and so does
// csrc/tools/varsel_index_check.cpp (`make varsel-check`), which plays the predicate against a restatement and every block and lane of
// the gather against a row-by-row copy.
//
// THE PREDICATE (twk_hip.h, variant subsets): N the base's samples, n_het / n_hom / n_miss what twk_hip_get_marginals returns for the
// variant.  called = N - n_miss, obs = 2 called, alt = n_het + 2 n_hom, minor = min(alt, obs - alt); each threshold is one IEEE double
// multiplication and one comparison (the library is built with -ffp-contract=off, and there is nothing to contract here anyway: the
// product is compared, not added to).
// THE COUNTS of a raw word (2 bits a sample, bit 2s / 2s + 1 = first / second allele is ALT; the mask word has both bits of a sample set
// when either allele is missing): a sample is missing when either mask bit is set, heterozygous when its two allele bits differ,
// homozygous ALT when both are set - the latter two only when it is not missing.  This is what k_build_unphased's planes count.
// THE GATHER moves rows of w4 16-byte pieces (w4 = Wp / 4; Wp is a multiple of 32 words, so a row is whole 128-byte lines).  The output
// of one plane is n_slots = rows_out x w4 SLOTS, slot s = piece s % w4 of output row s / w4.  Lane t of block b of a grid of n_blocks
// takes the slots b * VARSEL_BLOCK + t + k * n_blocks * VARSEL_BLOCK, k = 0, 1, ..: consecutive lanes move consecutive pieces, every
// slot belongs to one lane of one block, and the lane finds its (row, piece) with one division at the start and additions after it.
// Output row r < n_kept is base row map[r]; the rows behind are the padding of the count kernel's tiles and are written as zeros.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TWK_VARSEL_FN __host__ __device__ inline
#else
#define TWK_VARSEL_FN inline
#endif

namespace twk {

constexpr uint32_t VARSEL_BLOCK = 256;       // lanes of a gather block
constexpr uint32_t VARSEL_UNROLL = 4;        // slots a lane has in flight: the loads of all of them are issued before the first store
constexpr uint32_t VARSEL_MAX_BLOCKS = 2048; // of one plane: the rest is the lanes' stride

struct VarselFilter {                        // twk_hip_variant_filter without its padding
	double min_maf, max_maf;
	uint32_t min_mac;
	double max_missing, min_hwe;
};

// het / hom-ALT / missing samples among the 16 of one raw word x and its mask word m (0 where the data set has no missing data).
TWK_VARSEL_FN void varsel_word_counts(uint32_t x, uint32_t m, uint32_t& het, uint32_t& hom, uint32_t& miss) {
	const uint32_t E = 0x55555555u;
	const uint32_t x0 = x & E, x1 = (x >> 1) & E;
	const uint32_t ms = (m | (m >> 1)) & E;
	het += (uint32_t)__builtin_popcount((x0 ^ x1) & ~ms);
	hom += (uint32_t)__builtin_popcount((x0 & x1) & ~ms);
	miss += (uint32_t)__builtin_popcount(ms);
}

// Does the variant pass every threshold?  (The list test is the caller's.)
TWK_VARSEL_FN bool varsel_pass(uint32_t n_samples, uint32_t n_het, uint32_t n_hom, uint32_t n_miss, double hwe, const VarselFilter& f) {
	const uint32_t called = n_samples - n_miss;
	const uint32_t obs = 2u * called;
	const uint32_t alt = n_het + 2u * n_hom;
	const uint32_t minor = alt < obs - alt ? alt : obs - alt;
	if (!((double)minor >= f.min_maf * (double)obs)) return false;
	if (!((double)minor <= f.max_maf * (double)obs)) return false;
	if (!(minor >= f.min_mac)) return false;
	if (!((double)n_miss <= f.max_missing * (double)n_samples)) return false;
	if (hwe < f.min_hwe) return false;
	return true;
}

// Are the thresholds ones twk_hip_select_variants takes?  -> NULL, or the name of the first field that is NaN or outside its range.
inline const char* varsel_filter_fault(const VarselFilter& f) {
	if (!(f.min_maf >= 0.0 && f.min_maf <= 0.5)) return "min_maf";
	if (!(f.max_maf >= 0.0 && f.max_maf <= 0.5)) return "max_maf";
	if (!(f.min_maf <= f.max_maf)) return "min_maf > max_maf";
	if (!(f.max_missing >= 0.0 && f.max_missing <= 1.0)) return "max_missing";
	if (!(f.min_hwe >= 0.0 && f.min_hwe <= 1.0)) return "min_hwe";
	return nullptr;
}

struct VarselGather {
	uint64_t n_slots;            // rows_out * w4
	uint32_t w4;                 // 16-byte pieces a row
	uint32_t n_kept;             // output rows that come from the base; the rest, up to rows_out, is zero padding
	uint32_t n_blocks;           // grid.x
	uint32_t step_rows, step_cols;      // n_blocks * VARSEL_BLOCK slots = step_rows whole rows and step_cols pieces
};

inline VarselGather varsel_gather_geometry(uint32_t rows_out, uint32_t n_kept, uint32_t w4) {
	VarselGather g{};
	g.n_slots = (uint64_t)rows_out * w4; g.w4 = w4; g.n_kept = n_kept;
	const uint64_t want = (g.n_slots + VARSEL_BLOCK - 1) / VARSEL_BLOCK;
	g.n_blocks = (uint32_t)(want < VARSEL_MAX_BLOCKS ? (want ? want : 1) : VARSEL_MAX_BLOCKS);
	const uint64_t step = (uint64_t)g.n_blocks * VARSEL_BLOCK;
	g.step_rows = (uint32_t)(step / w4); g.step_cols = (uint32_t)(step % w4);
	return g;
}

// The slots of one lane, VARSEL_UNROLL at a time: x = row < n_kept ? load(map[row], col) : zero for all of them, then store(row, col, x).
template <class V, class Load, class Store>
TWK_VARSEL_FN void varsel_gather_lane(const VarselGather& g, uint32_t block, uint32_t lane, const uint32_t* map, const V& zero, Load&& load, Store&& store) {
	const uint64_t step = (uint64_t)g.n_blocks * VARSEL_BLOCK;
	uint64_t s = (uint64_t)block * VARSEL_BLOCK + lane;
	if (s >= g.n_slots) return;
	uint32_t row = (uint32_t)(s / g.w4), col = (uint32_t)(s % g.w4);
	auto advance = [&g](uint32_t& r, uint32_t& c) {
		r += g.step_rows; c += g.step_cols;
		if (c >= g.w4) { c -= g.w4; ++r; }
	};
	while (s < g.n_slots) {
		// the loads of the batch, then its stores: the second loop walks the same (row, piece) sequence again from the batch's start
		V x0 = zero, x1 = zero, x2 = zero, x3 = zero;
		static_assert(VARSEL_UNROLL == 4, "the batch is written out");
		uint32_t r = row, c = col;
		uint64_t t = s;
		if (t < g.n_slots) { if (r < g.n_kept) x0 = load(map[r], c); advance(r, c); t += step; }
		if (t < g.n_slots) { if (r < g.n_kept) x1 = load(map[r], c); advance(r, c); t += step; }
		if (t < g.n_slots) { if (r < g.n_kept) x2 = load(map[r], c); advance(r, c); t += step; }
		if (t < g.n_slots) { if (r < g.n_kept) x3 = load(map[r], c); }
		if (s < g.n_slots) { store(row, col, x0); advance(row, col); s += step; }
		if (s < g.n_slots) { store(row, col, x1); advance(row, col); s += step; }
		if (s < g.n_slots) { store(row, col, x2); advance(row, col); s += step; }
		if (s < g.n_slots) { store(row, col, x3); advance(row, col); s += step; }
	}
}

}  // namespace twk
