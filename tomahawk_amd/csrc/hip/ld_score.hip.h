// LD scores: the epilogue of a count matrix that sums instead of appending (twk_hip_ld_score, include/twk_hip.h).
//
// For every variant v of the problem  n(v) = number of records `calc` would report with v at either end and
// sum_r2(v) = the sum of their R2 fields.  A score launch runs the count kernel into C like a record launch and then
//   k_ld_score       one pair per lane through d_pair<SRC_MATRIX> (ld_math.hip.h) with the launch's StatsParams - the pair rules,
//                    the regrouped sets' ids, auto_select, window, option bits are the record path's own code - and only `keep` and
//                    rec.R2 are used: the record's other fields are dead and the compiler drops them.  A block is 256 lanes = 256
//                    columns and walks SCORE_ROWS rows: a lane's column sum stays in its registers (rows in ascending order), a
//                    row's sum is reduced over the wave (butterfly, fixed lane order) and over the block's four waves through LDS
//                    (wave 0 .. 3).  The block writes one partial per row and one per column: no atomics of any kind.
//   k_ld_score_fold  one lane per row (then, in a second launch, per column) of the tile adds the row's partials, block after
//                    block in ascending order, into the per-variant accumulators (double sum, uint64 n; indexed by variant id in
//                    file order: through `ids` for a regrouped plane set).  Every lane of a launch owns a different variant, the
//                    two launches and the launches of a run follow each other on one stream in the plan's order: the order of
//                    every floating-point addition is fixed, so two runs give the same bits.
// No Fisher test (a score run requires minP >= 1: the two-sided P never exceeds 1), no survivor buffer, no sort, nothing copied
// back but the two arrays at the end.  There is no reference counterpart (the reference writes records only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ld_math.hip.h"
#include "ld_reduce.hip.h"

namespace twk {

constexpr int SCORE_THREADS = 256;      // columns of a block
constexpr int SCORE_ROWS = 32;          // rows of a block

struct ScoreParts {
	double* row_sum; uint32_t* row_n;   // [nA][gx]: row i's partial from column block bx at i * gx + bx
	double* col_sum; uint32_t* col_n;   // [gy][nB]: column j's partial from row block by at by * nB + j
	uint32_t gx, gy;
};
struct ScoreArgs : ReduceParams<ScoreParts> {};

// One pair of the launch's matrix: its r2 if `calc` would report it, a negative number if not.  Out of line, so that the registers of
// the two maths are the callee's and not held across the row loop (inlined into it the kernel needs 191 VGPRs: two waves a SIMD).
__device__ __noinline__ double d_score_pair(const StatsParams* pp, uint32_t i, uint32_t j) {
	const StatsParams& p = *pp;
	twk_hip_record rec;
	return d_pair<SRC_MATRIX>(p, p.tv.a0 + i, p.tv.b0 + j, i, j, 0, &rec) ? rec.R2 : -1.0;
}

__global__ __launch_bounds__(SCORE_THREADS)
void k_ld_score(const ScoreArgs* __restrict__ args) {
	__shared__ double wave_sum[SCORE_ROWS][SCORE_THREADS / 64];
	__shared__ uint32_t wave_n[SCORE_ROWS][SCORE_THREADS / 64];
	const ScoreParts sp = args->m;
	const uint32_t nA = args->p.nA, nB = args->p.nB;
	const uint32_t j = blockIdx.x * SCORE_THREADS + threadIdx.x;
	const uint32_t i0 = blockIdx.y * SCORE_ROWS;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const bool dead = d_block_dead(args->p, blockIdx.x, SCORE_THREADS, i0);      // (such a block still writes its partials: zeros)
	double csum = 0.0; uint32_t cn = 0;
#pragma unroll 1
	for (uint32_t r = 0; r < SCORE_ROWS; ++r) {
		const uint32_t i = i0 + r;
		double r2 = -1.0;
		if (!dead && i < nA && j < nB) r2 = d_score_pair(&args->p, i, j);
		const bool keep = r2 >= 0.0;
		if (!keep) r2 = 0.0;
		csum += r2; cn += keep ? 1u : 0u;
		const unsigned long long ballot = __ballot(keep);
		const double ws = ballot ? d_wave_reduce(r2, WaveSum()) : 0.0;      // (uniform over the wave)
		if (lane == 0) { wave_sum[r][wave] = ws; wave_n[r][wave] = (uint32_t)__popcll(ballot); }
	}
	if (j < nB) {
		const size_t at = (size_t)blockIdx.y * nB + j;
		sp.col_sum[at] = csum; sp.col_n[at] = cn;
	}
	__syncthreads();
	if (threadIdx.x < SCORE_ROWS && i0 + threadIdx.x < nA) {
		double s = 0.0; uint32_t n = 0;
#pragma unroll
		for (int w = 0; w < SCORE_THREADS / 64; ++w) { s += wave_sum[threadIdx.x][w]; n += wave_n[threadIdx.x][w]; }
		const size_t at = (size_t)(i0 + threadIdx.x) * sp.gx + blockIdx.x;
		sp.row_sum[at] = s; sp.row_n[at] = n;
	}
}

// Item x of `count` (a row or a column of the tile, set position first + x) has n_parts partials at x * item_stride + k * part_stride,
// k = 0 .. n_parts - 1; their sum, taken in that order, is added to the accumulators of the item's variant.
__global__ __launch_bounds__(256)
void k_ld_score_fold(const double* __restrict__ part_sum, const uint32_t* __restrict__ part_n, uint32_t count, uint32_t n_parts,
                     size_t item_stride, size_t part_stride, uint32_t first, const uint32_t* __restrict__ ids, uint32_t n_variants,
                     double* __restrict__ acc_sum, unsigned long long* __restrict__ acc_n) {
	const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
	if (x >= count || first + x >= n_variants) return;
	double s = 0.0; unsigned long long n = 0;
	for (uint32_t k = 0; k < n_parts; ++k) {
		const size_t at = (size_t)x * item_stride + (size_t)k * part_stride;
		s += part_sum[at]; n += part_n[at];
	}
	if (!n) return;                      // (no record: nothing to add, and r2 is never negative)
	const uint32_t v = ids ? ids[first + x] : first + x;
	acc_sum[v] += s; acc_n[v] += n;
}

}  // namespace twk
