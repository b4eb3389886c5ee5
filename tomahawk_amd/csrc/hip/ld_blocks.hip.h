// Haplotype blocks: the D' confidence bounds of every in-window pair in band storage (twk_hip_ld_dprime_ci_band), and the blocks
// selected from them by the rule of Gabriel et al. (twk_hip_ld_blocks; include/twk_hip.h, the definitions: ld_block_ci.h).
//
//   k_ld_dprime_ci_band  the epilogue of a count matrix: k_ld_bandmat_fill's shape (ld_bandmat.hip.h) - 256 lanes are 256 columns, 32 rows
//                        in a loop that is not unrolled, the parameter block in device memory, the band map {base, first, len} per
//                        variant, the direct store per lane, the mirrored store staged in LDS with pitch 257 and written out transposed
//                        by half-waves (32 consecutive bytes of a column variant's row segment), both stores per lane at the file-order
//                        ids on a regrouped set, every store behind the dense guard and bm_in_band, the dead blocks.  What differs is
//                        the value: behind d_pair<SRC_MATRIX>, out of line in d_ci_pair, the lane scans the likelihood of the record's
//                        2 x 2 table over 101 values of D' (bc_bounds) and stores two bytes, lo and hi, into two arrays.  A slot
//                        without a record keeps the preset 255.  Plain stores only; nothing is counted here (k_blocks_count counts).
//   k_blocks_prefix      one wave per band row y: P[slot(y, x)] = the number of columns x' <= x of the row with (x', y) STRONG at
//                        strong_lo, and the same for RECOMBINANT, by ballots and a carried count.  With both orientations stored, the
//                        column sum over x = i .. j - 1 of class(x, j) is then one subtraction in row j.
//   k_blocks_count       one thread per first variant i walks j upwards through its band and carries s (strong at strong_lo) and r as
//   / k_blocks_emit      running sums: s(i, j) = s(i, j - 1) + column sum of j.  A candidate of up to 4 markers takes its s from its at
//                        most 6 pairs at its own cut.  The first pass counts per i the qualifying candidates, the candidates and the
//                        informative pairs; after an exclusive scan of the first count the second pass, the same walk, writes key, s
//                        and r of every qualifying candidate at its place.  O(nnz) work, no atomics.
//   k_blocks_walk        one block behind the sort, in k_ld_clump_walk's style.  `used` - one bit per variant of the slice - lives in
//                        LDS (beyond BLOCKS_LDS_WORDS words: in global memory).  The sorted candidates are read 64 at a time, one per
//                        lane (every wave reads the same 64), and passed round the wave.  Per candidate (i, j) every lane reads the
//                        bits of i and j:
//                          either set    an end lies in an earlier block: skipped, without a barrier;
//                          both clear    a block: barrier A; the lanes set the bits i .. j in the words they own, store block_of for
//                                        the variants they own, and thread 0 stores the block's last variant, s and r at slot i;
//                                        barrier B.
//                        WHY EVERY LANE DECIDES ALIKE (k_ld_clump_walk's argument, unchanged).  `used` is written only between a
//                        barrier A and the barrier B behind it.  A lane passes A only when all lanes have arrived there, and a lane
//                        arrives at A only after it has read the bits of every candidate up to and including the accepted one - so
//                        nobody writes while anybody still has a bit to read that was to be decided on the state before A.  A lane
//                        passes B only when all writes of that block are done, so every read behind B sees them all.  Between B and the
//                        next A nothing is written: however far ahead a lane runs through skipped candidates, it reads the state every
//                        other lane will read.  All lanes reach the same decision for every candidate, and the barriers match up: two
//                        per block, none per skipped candidate.  Every lane counts the blocks (the same number in each).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ld_math.hip.h"
#include "ld_reduce.hip.h"
#include "ld_bandmat_index.h"
#include "ld_block_ci.h"

namespace twk {

constexpr int CI_THREADS = (int)MX_COLS;
constexpr int CI_ROWS = (int)MX_ROWS;

struct CiMap {
	uint8_t* lo; uint8_t* hi;           // [row_ptr[n]] each
	const BandRow* rows;                // [n]: the band of every variant of the slice
	uint32_t a0, n;                     // the slice's first variant, its size
};
struct CiArgs : ReduceParams<CiMap> {};

// One pair: 0 without a record, else 1 << 16 | hi << 8 | lo.
__device__ __noinline__ uint32_t d_ci_pair(const CiArgs* args, uint32_t i, uint32_t j) {
	const StatsParams& p = args->p;
	twk_hip_record rec;
	if (!d_pair<SRC_MATRIX>(p, p.tv.a0 + i, p.tv.b0 + j, i, j, 0, &rec)) return 0u;
	uint32_t lo, hi;
	bc_bounds(rec.cnt[0], rec.cnt[1], rec.cnt[2], rec.cnt[3], &lo, &hi);
	return 1u << 16 | hi << 8 | lo;
}

__global__ __launch_bounds__(CI_THREADS)
void k_ld_dprime_ci_band(const CiArgs* __restrict__ args) {
	__shared__ uint32_t stage[MX_STAGE_WORDS];
	__shared__ uint32_t kept[MX_COLS];
	__shared__ unsigned long long cbase[MX_COLS];
	__shared__ uint32_t cfirst[MX_COLS], clen[MX_COLS];
	const CiMap mm = args->m;
	const uint32_t nA = args->p.nA, nB = args->p.nB;
	const uint32_t a0 = args->p.tv.a0, b0 = args->p.tv.b0;
	const uint32_t* ids = args->p.tv.ids;
	const uint32_t tid = threadIdx.x;
	const uint32_t j = blockIdx.x * MX_COLS + tid;
	const uint32_t i0 = blockIdx.y * MX_ROWS;
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
	uint32_t mine = 0;                                       // bit r = this lane's column has a value in row i0 + r
#pragma unroll 1
	for (uint32_t r = 0; r < MX_ROWS; ++r) {
		const uint32_t i = i0 + r;
		uint32_t pv = 0;
		if (mx_lane_live(i, j, nA, nB)) pv = d_ci_pair(args, i, j);
		bool keep = pv != 0;
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
		if (!keep) continue;
		const uint8_t lo = (uint8_t)pv, hi = (uint8_t)(pv >> 8);
		const uint64_t at = bm_slot(ru.base, ru.first, v);
		mm.lo[at] = lo; mm.hi[at] = hi;
		if (ids) {
			const BandRow rv = mm.rows[v];                   // (v < n: mx_ok_ids)
			if (bm_in_band(u, rv.first, rv.len)) { const uint64_t m = bm_slot(rv.base, rv.first, u); mm.lo[m] = lo; mm.hi[m] = hi; }
		} else { stage[mx_stage(r, tid)] = pv; mine |= 1u << r; }
	}
	if (ids) return;                                         // (uniform over the block)
	// the mirrored entries of a plain set: the block's values transposed - half a wave per column, 32 consecutive bytes of its row segment
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
		if (mx_ok_plain(ocol, orow, mm.n) && bm_in_band(ocol, f, clen[c])) {
			const uint32_t pv = stage[mx_stage(tr, c)];
			const uint64_t at = bm_slot(cbase[c], f, ocol);
			mm.lo[at] = (uint8_t)pv; mm.hi[at] = (uint8_t)(pv >> 8);
		}
	}
}

// ---- the blocks, over the finished band ----
constexpr int BLOCKS_THREADS = 256;
constexpr int BLOCKS_WALK_THREADS = 1024;
constexpr uint32_t BLOCKS_LDS_WORDS = 8128;          // `used` in LDS: up to 520,192 variants, as clump's `taken`

// Inclusive prefix counts of the two classes along every band row: one wave per row, 64 columns a step.
__global__ __launch_bounds__(BLOCKS_THREADS)
void k_blocks_prefix(BlocksBand b) {
	const uint32_t y = blockIdx.x * (BLOCKS_THREADS / 64) + (threadIdx.x >> 6);
	const uint32_t lane = threadIdx.x & 63;
	if (y >= b.n) return;                                    // (uniform over the wave)
	const BandRow row = b.rows[y];
	uint32_t cs = 0, cr = 0;
	for (uint32_t k0 = 0; k0 < row.len; k0 += 64) {
		const uint32_t k = k0 + lane;
		uint32_t lo = BC_NONE, hi = BC_NONE;
		if (k < row.len) { lo = b.lo[row.base + k]; hi = b.hi[row.base + k]; }
		const unsigned long long bs = __ballot(bc_strong(lo, hi, b.par.strong_lo, b.par.strong_hi));
		const unsigned long long br = __ballot(bc_recomb(lo, hi, b.par.recomb_hi));
		if (k < row.len) {
			b.ps[row.base + k] = cs + bc_prefix_in_ballot(bs, lane);
			b.pr[row.base + k] = cr + bc_prefix_in_ballot(br, lane);
		}
		cs += (uint32_t)__popcll(bs); cr += (uint32_t)__popcll(br);
	}
}

// informative[u] = the columns v > u of band row u that hold a value: one wave per row.
__global__ __launch_bounds__(BLOCKS_THREADS)
void k_ci_informative(const uint8_t* __restrict__ lo, const BandRow* __restrict__ rows, uint32_t n, uint32_t* __restrict__ informative) {
	const uint32_t u = blockIdx.x * (BLOCKS_THREADS / 64) + (threadIdx.x >> 6);
	const uint32_t lane = threadIdx.x & 63;
	if (u >= n) return;                                      // (uniform over the wave)
	const BandRow row = rows[u];
	uint32_t count = 0;
	for (uint32_t k0 = 0; k0 < row.len; k0 += 64) {
		const uint32_t k = k0 + lane;
		count += (uint32_t)__popcll(__ballot(k < row.len && row.first + k > u && bc_informative(lo[row.base + k])));
	}
	if (lane == 0) informative[u] = count;
}

// The walk of first variant i through its band (bc_candidates_of, ld_block_ci.h).  EMIT false: counts[3 * i ..] = qualifying
// candidates, candidates, informative pairs (i, j > i).  EMIT true: key, s and r of its qualifying candidates from slot off[i] on.
template <bool EMIT>
__global__ __launch_bounds__(BLOCKS_THREADS)
void k_blocks_candidates(BlocksBand b, uint32_t* __restrict__ counts, const uint32_t* __restrict__ off, uint32_t capacity,
                         unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals, uint32_t* __restrict__ cs, uint32_t* __restrict__ cr) {
	const uint32_t i = blockIdx.x * BLOCKS_THREADS + threadIdx.x;
	if (i >= b.n) return;
	bc_candidates_of<EMIT>(b, i, EMIT ? nullptr : counts + 3 * (size_t)i, EMIT ? off[i] : 0u, capacity, keys, vals, cs, cr);
}

// counts[3 * i] -> flat[i] (the scan's input).
__global__ __launch_bounds__(BLOCKS_THREADS)
void k_blocks_flatten(const uint32_t* __restrict__ counts, uint32_t n, uint32_t* __restrict__ flat) {
	const uint32_t i = blockIdx.x * BLOCKS_THREADS + threadIdx.x;
	if (i < n) flat[i] = counts[3 * (size_t)i];
}

// The walk over the sorted candidates.  keys[0 .. m) ascending, vals: each one's slot in cs / cr.  used0: [stride] zeroed words, the
// walk's `used` itself with IN_LDS false.  block_of: [n_variants], TWK_HIP_NO_BLOCK everywhere (the caller's fill).  blk: [3 * n],
// slot i = {last variant, s, r} of the block whose first variant is slice variant i.  out[0] = blocks.
template <bool IN_LDS>
__global__ __launch_bounds__(BLOCKS_WALK_THREADS)
void k_blocks_walk(const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ vals, uint32_t m, BlockKey key,
                   const uint32_t* __restrict__ cs, const uint32_t* __restrict__ cr, uint32_t a0, uint32_t n, uint32_t stride,
                   unsigned long long* used0, uint32_t* __restrict__ block_of, uint32_t* __restrict__ blk, unsigned long long* __restrict__ out) {
	__shared__ unsigned long long lds_used[IN_LDS ? BLOCKS_LDS_WORDS : 1];
	unsigned long long* used = IN_LDS ? lds_used : used0;
	const uint32_t tid = threadIdx.x;
	const int lane = tid & 63;
	if (IN_LDS) for (uint32_t w = tid; w < stride; w += BLOCKS_WALK_THREADS) used[w] = 0ull;
	__syncthreads();
	unsigned long long n_blocks = 0;
	for (uint32_t base = 0; base < m; base += 64) {
		const bool have = base + lane < m;
		const unsigned long long mine = have ? keys[base + lane] : 0ull;
		const uint32_t mine_val = have ? vals[base + lane] : 0u;
		const uint32_t cnt = m - base < 64 ? m - base : 64;
		for (uint32_t k = 0; k < cnt; ++k) {
			const uint32_t klo = (uint32_t)__shfl((int)(uint32_t)mine, (int)k), khi = (uint32_t)__shfl((int)(uint32_t)(mine >> 32), (int)k);
			const uint32_t slot = (uint32_t)__shfl((int)mine_val, (int)k);
			const unsigned long long kk = (unsigned long long)khi << 32 | klo;
			const uint32_t i = bc_key_i(key, kk), mm = bc_key_m(key, kk);
			const uint32_t j = i + mm - 1;
			if (mm < 2 || i >= n || j >= n || j < i) continue;   // (the emitter sends none: a bound, not a case)
			if (!bc_ends_free(used, i, j)) continue;      // the same answer in every lane (see above)
			++n_blocks;
			__syncthreads();                                     // A: every lane has read what it decides by
			for (uint32_t w = (i >> 6) + tid; w <= j >> 6; w += BLOCKS_WALK_THREADS) used[w] |= bc_range_bits(w, i, j);
			for (uint32_t v = i + tid; v <= j; v += BLOCKS_WALK_THREADS) block_of[a0 + v] = a0 + i;
			if (tid == 0) { blk[3 * (size_t)i] = a0 + j; blk[3 * (size_t)i + 1] = cs[slot]; blk[3 * (size_t)i + 2] = cr[slot]; }
			__syncthreads();                                     // B: its writes are done
		}
	}
	if (tid == 0) out[0] = n_blocks;
}

}  // namespace twk
