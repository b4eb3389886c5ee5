// LD matrix: the epilogue of a count matrix that stores one statistic per pair into a dense n x n float32 matrix
// (twk_hip_ld_matrix, include/twk_hip.h).
//
// Over a triangle of n variants [a0, a0 + n) in file order the entry (u, v), u != v, is the chosen statistic - signed r, r2, D or D' -
// of the record `calc` would report for the two variants, computed in double and rounded once to float32; where `calc` would report
// none the entry keeps the caller's fill.  A matrix launch runs the count kernel into C like a record launch and then
//   k_ld_matrix_fill  k_ld_prune_mask's shape - one pair per lane through d_pair<SRC_MATRIX> (ld_math.hip.h) with the launch's
//                     StatsParams, out of line, the parameter block in device memory - over MX_ROWS = 32 rows; of the record only `keep`
//                     and the chosen statistic are used.  The device matrix was preset to the fill (a 32-bit pattern set, once per
//                     call): a pair without a record stores NOTHING, so an entry is written by at most one lane of one launch - in
//                     the default mode the two passes select disjoint pairs (auto_select) - by plain stores, without atomics.
//                     A pair with a record stores twice:
//                       direct    at (row, col): a wave's 64 lanes write 64 consecutive floats;
//                       mirrored  at (col, row).  On a plain plane set (ids == null) the lane stages its value in LDS and sets bit r
//                                 of its column's word `kept`; after the row loop the block writes the staged values out transposed -
//                                 half a wave takes the 32 rows of one column: 32 consecutive floats of one output row, read from 32
//                                 different LDS banks (ld_matrix_index.h: pitch 257).  On a regrouped set (the default mode with missing
//                                 data) columns are not consecutive and a pair arrives in either order: every lane stores its two
//                                 entries at the file-order ids.
//                     Every store is guarded against the slice (ld_matrix_index.h, proven on the host by `make matrix-check`).  The
//                     records are counted per wave from the ballots: one 64-bit integer atomic add a wave.
//   k_ld_matrix_diag  behind the call's last launch: the diagonal (1 for r, r2 and D'; the fill for D - no record pins a variance
//                     under missing data, and none is invented).
// n * n * 4 bytes of device memory for the length of the call; no Fisher test (minP >= 1), no survivor buffer, no sort.  There is no
// reference counterpart.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ld_math.hip.h"
#include "ld_reduce.hip.h"
#include "ld_matrix_index.h"

namespace twk {

constexpr int MATRIX_THREADS = (int)MX_COLS;       // columns of a fill block
constexpr int MATRIX_ROWS = (int)MX_ROWS;          // rows of a fill block

struct MatrixMap {
	float* m;                           // [n][n]
	unsigned long long* n_records;
	uint32_t a0, n;                     // the triangle's first variant, its size
	int32_t stat;                       // TWK_HIP_STAT_*
};
struct MatrixArgs : ReduceParams<MatrixMap> {};

// One pair of the launch's matrix: bit 32 set if `calc` would report it, and then its statistic as a float32 in the low word (the
// double rounded once, to nearest).  Out of line, so that the registers of the two maths are the callee's and not held across the
// row loop (the finding noted at d_score_pair); the result travels in two registers, not through memory.
__device__ __noinline__ unsigned long long d_matrix_pair(const MatrixArgs* args, uint32_t i, uint32_t j) {
	const StatsParams& p = args->p;
	twk_hip_record rec;
	if (!d_pair<SRC_MATRIX>(p, p.tv.a0 + i, p.tv.b0 + j, i, j, 0, &rec)) return 0ull;
	return 1ull << 32 | (unsigned long long)__float_as_uint((float)d_stat_value(rec, args->m.stat));
}

__global__ __launch_bounds__(MATRIX_THREADS)
void k_ld_matrix_fill(const MatrixArgs* __restrict__ args) {
	__shared__ float stage[MX_STAGE_WORDS];
	__shared__ uint32_t kept[MX_COLS];
	const MatrixMap mm = args->m;
	const uint32_t nA = args->p.nA, nB = args->p.nB;
	const uint32_t a0 = args->p.tv.a0, b0 = args->p.tv.b0;
	const uint32_t* ids = args->p.tv.ids;
	const uint32_t tid = threadIdx.x;
	const uint32_t j = blockIdx.x * MX_COLS + tid;
	const uint32_t i0 = blockIdx.y * MX_ROWS;
	const int lane = tid & 63;
	// a block that lies wholly on or below the diagonal of a diagonal launch has no pair (uniform over the block)
	if (mx_block_dead(args->p.diag && a0 == b0, blockIdx.x, i0)) return;
	const uint32_t col = mx_rel(b0, j, mm.a0);              // plain sets: this lane's column, relative to the slice
	uint32_t records = 0, mine = 0;                          // mine: bit r = this lane's column has a value in row i0 + r
#pragma unroll 1
	for (uint32_t r = 0; r < MX_ROWS; ++r) {
		const uint32_t i = i0 + r;
		unsigned long long pv = 0;
		if (mx_lane_live(i, j, nA, nB)) pv = d_matrix_pair(args, i, j);
		bool keep = (uint32_t)(pv >> 32) != 0;
		uint32_t u = mx_rel(a0, i, mm.a0), v = col;
		if (ids) {
			if (keep) { u = ids[a0 + i] - mm.a0; v = ids[b0 + j] - mm.a0; }
			keep = keep && mx_ok_ids(u, v, mm.n);
		} else
			keep = keep && mx_ok_plain(u, v, mm.n);
		const unsigned long long ballot = __ballot(keep);
		if (!ballot) continue;                               // (uniform over the wave)
		records += (uint32_t)__popcll(ballot);
		if (!keep) continue;
		const float x = __uint_as_float((uint32_t)pv);
		mm.m[mx_slot(u, v, mm.n)] = x;
		if (ids) mm.m[mx_slot(v, u, mm.n)] = x;
		else { stage[mx_stage(r, tid)] = x; mine |= 1u << r; }
	}
	if (lane == 0 && records) atomicAdd(mm.n_records, (unsigned long long)records);
	if (ids) return;                                         // (uniform over the block)
	// the mirrored entries of a plain set: the block's values transposed - half a wave per column, 32 consecutive floats of its row
	kept[tid] = mine;
	__syncthreads();
	const uint32_t tr = mx_trow(tid);
	const uint32_t ocol = mx_rel(a0, i0 + tr, mm.a0);       // the row variant is the output column
#pragma unroll 4
	for (uint32_t k = 0; k < MX_TSTEPS; ++k) {
		const uint32_t c = mx_tcol(tid, k);
		if (!(kept[c] >> tr & 1)) continue;
		const uint32_t orow = mx_rel(b0, blockIdx.x * MX_COLS + c, mm.a0);
		if (mx_ok_plain(ocol, orow, mm.n)) mm.m[mx_slot(orow, ocol, mm.n)] = stage[mx_stage(tr, c)];
	}
}

// The diagonal of the n x n matrix, behind the call's last launch.
__global__ __launch_bounds__(256)
void k_ld_matrix_diag(float* __restrict__ m, uint32_t n, float value) {
	const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
	if (v < n) m[mx_slot(v, v, n)] = value;
}

}  // namespace twk
