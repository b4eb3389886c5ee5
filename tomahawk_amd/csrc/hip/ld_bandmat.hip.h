// Banded LD matrix: the epilogue of a count matrix that stores one statistic per pair into BAND STORAGE - per row of the slice only the
// columns inside the window (twk_hip_ld_matrix_band, include/twk_hip.h; the layout: ld_bandmat_index.h).
//
// The values are the dense matrix's (ld_matrix.hip.h), bit for bit: the same pair function, the same guards, the same two stores per
// pair with a record, the same preset - only the address differs.  A windowed run over a chromosome then needs row_ptr[n] floats on the
// device and over the link instead of n * n.
//   k_ld_bandmat_fill  k_ld_matrix_fill's shape - 256 lanes are 256 columns, MX_ROWS = 32 rows in a loop that is not unrolled, the pair
//                      out of line through d_pair<SRC_MATRIX> and d_stat_value, the parameter block in device memory.  The band map - per
//                      variant of the slice a BandRow {base, first, len} - sits in device memory.
//                        direct    at (row, col): the row's BandRow is uniform over the block; a wave's 64 lanes store 64 consecutive
//                                  floats of one row segment.
//                        mirrored  at (col, row).  Plain sets: staged in LDS with pitch 257 and written out transposed - half a wave
//                                  takes the 32 rows of one column, 32 consecutive floats of that column variant's row segment.  The 256
//                                  columns' BandRows are loaded once per block into LDS and read from there in the write-out: the address
//                                  is uniform within a half-wave, so there is no bank conflict.  Regrouped sets (ids != null): both
//                                  stores per lane at the file-order ids, each with its own row's BandRow.
//                      Every store passes the dense kernel's slice guard and bm_in_band (proven on the host by `make bandmat-check`).
//                      Plain stores only; the band was preset to the fill, a pair without a record stores nothing; the records are
//                      counted per wave from the ballots.  No 64-bit shift by a variable amount.
//                      A DEAD BLOCK - wholly outside the band: its first column at or beyond the band end of its last row - returns
//                      before it evaluates a pair (uniform over the block).  The dense kernel cannot: it has no band to ask.
//   k_ld_bandmat_diag  behind the call's last launch: the diagonal (1 for r, r2 and D'; for D it keeps the fill and the kernel is not run).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ld_math.hip.h"
#include "ld_reduce.hip.h"
#include "ld_bandmat_index.h"

namespace twk {

constexpr int BANDMAT_THREADS = (int)MX_COLS;
constexpr int BANDMAT_ROWS = (int)MX_ROWS;

struct BandMap {
	float* values;                      // [row_ptr[n]]
	const BandRow* rows;                // [n]: the band of every variant of the slice
	unsigned long long* n_records;
	uint32_t a0, n;                     // the slice's first variant, its size
	int32_t stat;                       // TWK_HIP_STAT_*
};
struct BandArgs : ReduceParams<BandMap> {};

// (d_matrix_pair's twin: the parameter block is another type, the pair and its statistic are the same code)
__device__ __noinline__ unsigned long long d_bandmat_pair(const BandArgs* args, uint32_t i, uint32_t j) {
	const StatsParams& p = args->p;
	twk_hip_record rec;
	if (!d_pair<SRC_MATRIX>(p, p.tv.a0 + i, p.tv.b0 + j, i, j, 0, &rec)) return 0ull;
	return 1ull << 32 | (unsigned long long)__float_as_uint((float)d_stat_value(rec, args->m.stat));
}

__global__ __launch_bounds__(BANDMAT_THREADS)
void k_ld_bandmat_fill(const BandArgs* __restrict__ args) {
	__shared__ float stage[MX_STAGE_WORDS];
	__shared__ uint32_t kept[MX_COLS];
	__shared__ unsigned long long cbase[MX_COLS];
	__shared__ uint32_t cfirst[MX_COLS], clen[MX_COLS];
	const BandMap mm = args->m;
	const uint32_t nA = args->p.nA, nB = args->p.nB;
	const uint32_t a0 = args->p.tv.a0, b0 = args->p.tv.b0;
	const uint32_t* ids = args->p.tv.ids;
	const uint32_t tid = threadIdx.x;
	const uint32_t j = blockIdx.x * MX_COLS + tid;
	const uint32_t i0 = blockIdx.y * MX_ROWS;
	const int lane = tid & 63;
	if (mx_block_dead(args->p.diag && a0 == b0, blockIdx.x, i0)) return;
	const uint32_t col = mx_rel(b0, j, mm.a0);              // plain sets: this lane's column, relative to the slice
	if (!ids) {
		// wholly outside the band (uniform over the block)
		const BandRow last = mm.rows[bm_block_last_row(a0, i0, nA, mm.a0, mm.n)];
		if (bm_block_dead(b0, blockIdx.x, mm.a0, last.first, last.len)) return;
		// the band of this lane's column variant, for the mirrored stores (a column outside the slice: an empty band)
		BandRow mine_row{0, 0, 0};
		if (col < mm.n) mine_row = mm.rows[col];
		cbase[tid] = mine_row.base; cfirst[tid] = mine_row.first; clen[tid] = mine_row.len;
	}
	uint32_t records = 0, mine = 0;                          // mine: bit r = this lane's column has a value in row i0 + r
#pragma unroll 1
	for (uint32_t r = 0; r < MX_ROWS; ++r) {
		const uint32_t i = i0 + r;
		unsigned long long pv = 0;
		if (mx_lane_live(i, j, nA, nB)) pv = d_bandmat_pair(args, i, j);
		bool keep = (uint32_t)(pv >> 32) != 0;
		uint32_t u = mx_rel(a0, i, mm.a0), v = col;
		if (ids) {
			if (keep) { u = ids[a0 + i] - mm.a0; v = ids[b0 + j] - mm.a0; }
			keep = keep && mx_ok_ids(u, v, mm.n);
		} else
			keep = keep && mx_ok_plain(u, v, mm.n);
		BandRow ru{0, 0, 0};
		if (keep) {                                          // (u < n: inside the map; on a plain set u is uniform over the block)
			ru = mm.rows[u];
			keep = bm_in_band(v, ru.first, ru.len);
		}
		const unsigned long long ballot = __ballot(keep);
		if (!ballot) continue;                               // (uniform over the wave)
		records += (uint32_t)__popcll(ballot);
		if (!keep) continue;
		const float x = __uint_as_float((uint32_t)pv);
		mm.values[bm_slot(ru.base, ru.first, v)] = x;
		if (ids) {
			const BandRow rv = mm.rows[v];                   // (v < n: mx_ok_ids)
			if (bm_in_band(u, rv.first, rv.len)) mm.values[bm_slot(rv.base, rv.first, u)] = x;
		} else { stage[mx_stage(r, tid)] = x; mine |= 1u << r; }
	}
	if (lane == 0 && records) atomicAdd(mm.n_records, (unsigned long long)records);
	if (ids) return;                                         // (uniform over the block)
	// the mirrored entries of a plain set: the block's values transposed - half a wave per column, 32 consecutive floats of its row segment
	kept[tid] = mine;
	__syncthreads();
	const uint32_t tr = mx_trow(tid);
	const uint32_t ocol = mx_rel(a0, i0 + tr, mm.a0);       // the row variant is the output column
#pragma unroll 4
	for (uint32_t k = 0; k < MX_TSTEPS; ++k) {
		const uint32_t c = mx_tcol(tid, k);
		if (!(kept[c] >> tr & 1)) continue;
		const uint32_t orow = mx_rel(b0, blockIdx.x * MX_COLS + c, mm.a0);
		const uint32_t f = cfirst[c];
		if (mx_ok_plain(ocol, orow, mm.n) && bm_in_band(ocol, f, clen[c])) mm.values[bm_slot(cbase[c], f, ocol)] = stage[mx_stage(tr, c)];
	}
}

// The diagonal of the band, behind the call's last launch.
__global__ __launch_bounds__(256)
void k_ld_bandmat_diag(float* __restrict__ values, const BandRow* __restrict__ rows, uint32_t n, float value) {
	const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
	if (v >= n) return;
	const BandRow rv = rows[v];
	if (bm_in_band(v, rv.first, rv.len)) values[bm_slot(rv.base, rv.first, v)] = value;
}

}  // namespace twk
