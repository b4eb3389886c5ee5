// Partitioned LD scores: the epilogue of a count matrix that multiplies the pairs' r2 by a matrix of annotations instead of appending
// (twk_hip_ld_score_annot, include/twk_hip.h): for every variant v and category c,  l(v, c) = the sum over v's partners w of
// a[w][c] * r2(v, w) - what stratified LD-score regression reads.
//
// A pair COUNTS when `calc` would report a record for it.  A counting pair (A, B) adds, for every category c, the integer
// t = rint((R2 * a[B][c]) * 2^32) to (A, c) and rint((R2 * a[A][c]) * 2^32) to (B, c) (ld_annot_term.h: one double multiplication, an exact
// scaling, ties to even; formed without llrint), and 1 to n(A) and to n(B).  Annotations and accumulators are indexed by the variant's
// id in file order; the default mode's two passes add into the same accumulators.  A launch runs the count kernel into C like a record
// launch and then
//   k_ld_annot        a block is 256 lanes = 256 columns by ANNOT_ROWS = 16 rows (ld_reduce.hip.h's shape: the parameter block in device
//                     memory, the pair out of line through d_pair<SRC_MATRIX>, blocks below the diagonal skipped, variant ids through
//                     p.tv.ids for a regrouped set).
//     the rows        walked in a loop that is not unrolled, as k_ld_decay walks them.  A pair's scaled r2 (R2 * 2^32, exact) is PARKED in
//                     an LDS stage of 16 x 256 doubles, 0 for a pair with no record - its terms are then 0 for every annotation.  The
//                     lane counts its column's records, the wave's ballot the row's.  A block without a record ends here.
//     the slabs       the categories are taken ANNOT_SLAB = 8 at a time: the slab's annotations of the block's 16 row variants and 256
//                     column variants are staged in LDS (zeros beyond the last category, for a variant without a record in the block, and
//                     beyond the launch), with one bit per row and category, and per column, that says "not zero".
//     column side     lane = column: eight 64-bit integer sums in registers, a loop over the 16 rows.  The row's annotation is the same
//                     in all lanes - an LDS broadcast - and a (row, category) whose annotation is 0 is skipped on the row's mask bits:
//                     the test is uniform over the wave.  Binary annotations are mostly zeros.
//     row side        thread = (half of the columns, row, category): one 64-bit integer sum, a loop over the 128 columns of the half
//                     whose mask bit is set (uniform over the wave: a column whose eight annotations are all 0 is skipped).  NO
//                     reduction over the wave: a 64-bit butterfly per (row, category) would cost several times the pair math.
//     at the end      a partial that is not 0 goes to the two accumulator words of its (variant, category) with 64-bit integer
//                     atomics, split with K = ANNOT_SPLIT = 24 (ld_exact_sum.h): S >> 24 (arithmetic) and S & (2^24 - 1), no carry
//                     between the words; a word that would add 0 is not issued.  The host joins the words in 128 bits and converts once.
// WHY 16 ROWS AND NOT 32.  The stage of 32 rows alone is 64 KiB; with the annotations a block would need 84 KiB and a CU (160 KiB) would
// hold one block - four waves against the pair math's memory latency.  At 16 rows the block's LDS is 50.8 KiB and a CU holds three.
// Both sides then do the same work a slab - 128 terms a thread - and every thread of the block has work on both.
// THE SUMS ARE EXACT AND HAVE NO ORDER.  Integers add up the same in any order: two runs, any tiling, any launch order and any shard
// split return the same bits, and no floating-point atomic is used anywhere.
// HEADROOM.  |t| <= T = 2^48 (1 + 2^-50): R2 <= 1 + a few ulps, |a| <= 2^16 (the entry point refuses anything else).  A column-side
// partial is a sum of at most 16 terms, a row-side partial of at most 128: |S| <= 2^7 T < 2^56, far inside a signed 64-bit integer.
// A partial is flushed only if it is not 0, so every flush to a word of (v, c) carries at least one counting pair of v, and every
// counting pair of v is in exactly one partial per pass and category: at most F = 2 * (2^32 - 1) < 2^33 flushes a word (v has fewer than
// 2^32 partners - variant ids are 32 bits - and the default mode visits a launch twice, each pass selecting its own pairs), whatever
// the tiling or the shard split.  Then
//   lo = S & (2^24 - 1) < 2^24           an unsigned word: below F * 2^24 < 2^57;
//   hi = S >> 24, |hi| <= |S| / 2^24 + 1  a signed word: the |S| of a word's flushes add up to at most F * T, so the word stays below
//                                         F * T / 2^24 + F < 2^57.1 in magnitude.
// Neither word can wrap in any call the engine admits: launch_reduce enforces no work limit for this kind.  n(v) < 2^33 likewise.
// No Fisher test (minP >= 1), no survivor buffer, no sort.  There is no reference counterpart.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ld_math.hip.h"
#include "ld_reduce.hip.h"
#include "ld_annot_term.h"

namespace twk {

constexpr uint32_t ANNOT_NO_VARIANT = 0xFFFFFFFFu;

struct AnnotMap {
	const double* annot;                // [n_variants][n_annot] the annotations, by variant id in file order
	unsigned long long* acc;            // [n_variants][n_annot][2] the sums' words: hi, lo (an_word)
	unsigned long long* acc_n;          // [n_variants] records
	uint32_t n_annot;
};
struct AnnotArgs : ReduceParams<AnnotMap> {};

// One pair of the launch's matrix: its r2 as a number of 2^-32 (exact, not yet rounded) if `calc` would report it, a negative number if
// not.  Out of line, so that the registers of the two maths are the callee's and not held across the row loop (ld_reduce.hip.h).
__device__ __noinline__ double d_annot_pair(const StatsParams* pp, uint32_t i, uint32_t j) {
	const StatsParams& p = *pp;
	twk_hip_record rec;
	return d_pair<SRC_MATRIX>(p, p.tv.a0 + i, p.tv.b0 + j, i, j, 0, &rec) ? at_scale(rec.R2) : -1.0;
}

// The variant at position s of the plane set, ANNOT_NO_VARIANT if the launch has none there.
__device__ __forceinline__ uint32_t d_annot_variant(const StatsParams& p, bool inside, uint32_t s) {
	if (!inside || s >= p.n_variants) return ANNOT_NO_VARIANT;
	return p.tv.ids ? p.tv.ids[s] : s;
}

// A partial sum that is not 0 into the two words of (v, c).
__device__ __forceinline__ void d_annot_add(const AnnotMap& am, uint32_t v, uint32_t c, long long s) {
	unsigned long long* const w = am.acc + an_word(v, am.n_annot, c);
	const unsigned long long hi = (unsigned long long)xs_split_hi<ANNOT_SPLIT>(s), lo = xs_split_lo<ANNOT_SPLIT>(s);      // (two's complement: the hi word is read as signed)
	if (hi) atomicAdd(w, hi);
	if (lo) atomicAdd(w + 1, lo);
}

// A value that is the same in every lane, as the compiler can see it: in scalar registers.
__device__ __forceinline__ uint32_t d_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ unsigned long long d_uniform(unsigned long long v) {
	return (unsigned long long)d_uniform((uint32_t)(v >> 32)) << 32 | d_uniform((uint32_t)v);
}

__global__ __launch_bounds__(ANNOT_THREADS)
void k_ld_annot(const AnnotArgs* __restrict__ args) {
	__shared__ double stage[ANNOT_ROWS][ANNOT_STRIDE];            // the pairs' scaled r2
	__shared__ double col_a[ANNOT_SLAB][ANNOT_STRIDE];            // the slab's annotations of the column variants
	__shared__ double row_a[ANNOT_ROWS][ANNOT_SLAB];              // ... of the row variants
	__shared__ unsigned long long col_mask[ANNOT_THREADS / 64];   // columns with an annotation of the slab that is not 0
	__shared__ uint32_t row_mask[ANNOT_ROWS];                     // per row: the slab's categories whose annotation is not 0
	__shared__ uint32_t row_id[ANNOT_ROWS], row_n[ANNOT_ROWS];    // the row variants and their records in this block
	const AnnotMap am = args->m;
	const uint32_t nA = args->p.nA, nB = args->p.nB, C = am.n_annot;
	const uint32_t t = threadIdx.x;
	const uint32_t j = blockIdx.x * ANNOT_THREADS + t;
	const uint32_t i0 = blockIdx.y * ANNOT_ROWS;
	const int lane = t & 63, wave = t >> 6;
	if (d_block_dead(args->p, blockIdx.x, ANNOT_THREADS, i0)) return;      // (uniform over the block)
	const uint32_t B = d_annot_variant(args->p, j < nB, args->p.tv.b0 + j);
	if (t < ANNOT_ROWS) { row_id[t] = d_annot_variant(args->p, i0 + t < nA, args->p.tv.a0 + i0 + t); row_n[t] = 0u; }
	__syncthreads();
	uint32_t cn = 0;
#pragma unroll 1
	for (uint32_t r = 0; r < ANNOT_ROWS; ++r) {
		const uint32_t i = i0 + r;
		double s = -1.0;
		if (i < nA && j < nB) s = d_annot_pair(&args->p, i, j);
		const bool keep = s >= 0.0;
		stage[r][t] = keep ? s : 0.0;
		cn += keep ? 1u : 0u;
		const unsigned long long ballot = __ballot(keep);
		if (lane == 0 && ballot) atomicAdd(row_n + r, (uint32_t)__popcll(ballot));
	}
	if (!__syncthreads_or(cn != 0)) return;                                // (no record in the block; uniform over it)
	// (a record implies both set positions below n_variants: the ids are there)
	if (cn) atomicAdd(am.acc_n + B, (unsigned long long)cn);
	if (t < ANNOT_ROWS && row_n[t]) atomicAdd(am.acc_n + row_id[t], (unsigned long long)row_n[t]);
	const uint32_t half = an_half(t), row = an_row(t), cat = an_cat(t);
#pragma unroll 1
	for (uint32_t c0 = 0; c0 < C; c0 += ANNOT_SLAB) {
		if (c0) __syncthreads();                                           // (the slab before this one has been read)
		if (t < ANNOT_ROWS * ANNOT_SLAB) {                                 // (waves 0 and 1, whole: eight rows by eight categories each)
			const uint32_t srow = t / ANNOT_SLAB, scat = t % ANNOT_SLAB;
			double a = 0.0;
			if (row_n[srow] && c0 + scat < C) a = am.annot[(size_t)row_id[srow] * C + c0 + scat];
			row_a[srow][scat] = a;
			const unsigned long long not_zero = __ballot(a != 0.0);
			if (scat == 0) row_mask[srow] = (uint32_t)(not_zero >> (lane & 56)) & 0xFFu;
		}
		bool any = false;
#pragma unroll
		for (uint32_t k = 0; k < ANNOT_SLAB; ++k) {
			double a = 0.0;
			if (cn && c0 + k < C) a = am.annot[(size_t)B * C + c0 + k];
			col_a[k][t] = a;
			any |= a != 0.0;
		}
		const unsigned long long cols = __ballot(any);
		if (lane == 0) col_mask[wave] = cols;
		__syncthreads();
		// column side: the terms of this lane's column variant, R2 * a[row variant][category]
		long long csum[ANNOT_SLAB];
#pragma unroll
		for (uint32_t k = 0; k < ANNOT_SLAB; ++k) csum[k] = 0ll;
#pragma unroll 1
		for (uint32_t r = 0; r < ANNOT_ROWS; ++r) {
			const uint32_t m = d_uniform(row_mask[r]);
			if (!m) continue;
			const double s = stage[r][t];
#pragma unroll
			for (uint32_t k = 0; k < ANNOT_SLAB; ++k)
				if (m >> k & 1u) csum[k] += at_term(s, row_a[r][k]);
		}
		if (cn) {
#pragma unroll
			for (uint32_t k = 0; k < ANNOT_SLAB; ++k)
				if (csum[k]) d_annot_add(am, B, c0 + k, csum[k]);          // (not 0: the category exists - beyond the last the staged annotation is 0)
		}
		// row side: the terms of this thread's (row variant, category), R2 * a[column variant][category], over its half of the columns
		long long rsum = 0ll;
#pragma unroll
		for (uint32_t word = 0; word < 2; ++word) {
			unsigned long long m = d_uniform(col_mask[half * 2 + word]);
			while (m) {
				const uint32_t col = an_col(half, word, (uint32_t)__ffsll((long long)m) - 1u);
				m &= m - 1;
				rsum += at_term(stage[row][col], col_a[cat][col]);
			}
		}
		if (rsum && row_n[row]) d_annot_add(am, row_id[row], c0 + cat, rsum);
	}
}

}  // namespace twk
