// LD aggregate: the epilogue of a count matrix that rasterises the pairs' LD into x-by-y cells (twk_hip_ld_aggregate, include/twk_hip.h).
//
// Every variant carries two bins, one per axis (0xFFFF: off the landscape on that axis), packed by the host into one 32-bit word
// (ld_aggregate_bin.h).  For every pair (A, B) `calc` would report a record for, the chosen statistic v - signed r, r2, D or D' - is
// added to cell (bin_x[A], bin_y[B]) and to cell (bin_x[B], bin_y[A]), each if both of its bins are valid: the reference's writer emits
// a record in both orientations and its aggregator indexes mat[x(A)][y(B)].  The two cells are the same set whichever of the two
// variants is called A, so the order in which a regrouped set meets a pair does not matter.  Per cell the call returns the number of
// contributions, the sums of v and of v * v and the extremes of v.  An aggregate launch runs the count kernel into C like a record
// launch and then
//   k_ld_aggregate  one pair per lane through d_pair<SRC_MATRIX> (ld_math.hip.h) with the launch's StatsParams - the pair rules, the
//                   regrouped sets' ids, auto_select, window, option bits are the record path's own code - and only `keep` and the
//                   chosen statistic are used.  The shape is ld_reduce.hip.h's: 256 lanes = 256 columns, AGG_ROWS rows in a loop that
//                   is not unrolled, the parameter block in device memory, the pair out of line, blocks below the diagonal skipped.
// THE SUMS ARE EXACT AND HAVE NO ORDER.  A contribution adds the integers q = rint(v * 2^32) and q2 = rint((v * v) * 2^32)
// (ld_exact_sum.h), and takes part in an integer minimum and maximum of q: integers add up and compare the same in any order, so two
// runs, any tiling and any launch order return the same bits, and no floating-point atomic is used anywhere.
//   in the wave  the row's variant is the same in all 64 lanes; lanes whose column variants share a packed key share both cells.
//                The lanes are grouped by key (d_key_groups, ld_reduce.hip.h): per key present their q, q2, minimum and maximum are
//                reduced over the wave (d_wave_reduce over 64-bit integers; a key with one lane skips it), and the first lane adds the
//                result and the ballot's popcount to both cells.  Right for any distribution of keys over the lanes.
//   in the block two dense windows of cells in LDS, one per orientation, AGG_WIN_A bins of the row side by AGG_WIN_B bins of the column
//                side, anchored at the bins of the block's first row and first column.  A contribution inside its window goes to LDS
//                integer atomics (a uint32 count, 64-bit q and q2 sums, 64-bit minimum and maximum per cell); one outside goes straight
//                to the global accumulators.  On a position-sorted set with monotone bins nearly everything is inside; on a regrouped
//                set or a hostile bin assignment nearly everything is outside - the same integers either way.
//   at the end   every touched window cell is flushed like a direct contribution: 64-bit integer atomic adds for the count and the
//                split sums, atomicMin / atomicMax on signed 64-bit for the extremes (preset to INT64_MAX / INT64_MIN by
//                k_ld_aggregate_init in front of the launches).  No branch on the data beyond inside / outside.
// HEADROOM.  Let Q = 2^33 bound |q| and q2 (v is a correlation, a D or a D': |v| <= 1 up to rounding).  A window cell takes at most
// one contribution a pair of the block and orientation, 8192: its count stays below 2^32 and its sums below 2^13 * Q = 2^46 in
// magnitude.  A wave's group holds at most 64 contributions.  Every global add - a flush or a direct one - carries c >= 1
// contributions with a partial sum |S| <= c * Q and adds, with k = AGG_SPLIT = 20 (ld_exact_sum.h's split),
//   lo = S & (2^k - 1) < 2^20           to an unsigned word: after T contributions to the cell at most T adds, less than T * 2^20;
//   hi = S >> k (arithmetic), |hi| <= |S| / 2^k + 1 <= c * (2^13 + 1)
//                                        to a signed word: after T contributions at most T * (2^13 + 1) in magnitude;
// and the count adds c.  With T <= 2^43 the lo word stays below 2^63, the hi word below 2^57 and the count at 2^43: no word wraps,
// whatever the bin layout - all contributions of a call may fall into one cell, every one of them a direct add.  The engine adds up
// the pairs each launch can evaluate (nA * nB; n (n - 1) / 2 for a square launch on the diagonal), two contributions each, and refuses
// the launch that would take the sum past 2^42.  A call of 2^40 pairs stays inside: a launch on the diagonal that is not square
// evaluates at least half its nA * nB, and the default mode's two passes visit every launch twice - at most 4 * 2^40.
// No Fisher test (minP >= 1), no survivor buffer, no sort; 64 bytes per cell on the device.  The reference's counterpart
// (two_reader::Aggregate) reads the records of a .two file; here no record is formed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ld_math.hip.h"
#include "ld_reduce.hip.h"
#include "ld_aggregate_bin.h"

namespace twk {

constexpr int AGG_THREADS = 256;        // columns of a block
constexpr int AGG_ROWS = 32;            // rows of a block
constexpr uint32_t AGG_WIN_A = 4;       // bins of the row side in a window
constexpr uint32_t AGG_WIN_B = 64;      // bins of the column side in a window
constexpr uint32_t AGG_WIN_CELLS = AGG_WIN_A * AGG_WIN_B;
constexpr uint32_t AGG_CELL_WORDS = 8;  // accumulator words a cell: count, q hi, q lo, q2 hi, q2 lo, min, max, one unused (64 bytes: a cell's atomics meet one line)
enum { AGG_W_N = 0, AGG_W_Q_HI, AGG_W_Q_LO, AGG_W_Q2_HI, AGG_W_Q2_LO, AGG_W_MIN, AGG_W_MAX };
constexpr long long AGG_I64_MAX = 0x7FFFFFFFFFFFFFFFll, AGG_I64_MIN = -AGG_I64_MAX - 1;

struct AggMap {
	const uint32_t* key;                // [n_variants] the two bins of every variant, packed (file order)
	unsigned long long* acc;            // [x_bins * y_bins][AGG_CELL_WORDS]
	uint32_t x_bins, y_bins;
	int32_t stat;                       // TWK_HIP_STAT_*
};
struct AggArgs : ReduceParams<AggMap> {};

struct AggPair { long long q; unsigned long long q2; uint32_t key; };

// One pair of the launch's matrix: the packed key of its column variant and its two integers if `calc` would report it and the column
// variant is on the landscape on either axis, AGG_NO_KEY if not.  Out of line, so that the registers of the two maths are the callee's
// and not held across the row loop (ld_reduce.hip.h).
__device__ __noinline__ AggPair d_agg_pair(const AggArgs* args, uint32_t i, uint32_t j) {
	const StatsParams& p = args->p;
	const uint32_t sA = p.tv.a0 + i, sB = p.tv.b0 + j;
	twk_hip_record rec;
	AggPair out{0ll, 0ull, AGG_NO_KEY};
	if (!d_pair<SRC_MATRIX>(p, sA, sB, i, j, 0, &rec)) return out;
	// (keep implies both set positions below n_variants: the id is there)
	const uint32_t B = p.tv.ids ? p.tv.ids[sB] : sB;
	const uint32_t key = args->m.key[B];
	if (key == AGG_NO_KEY) return out;
	const double v = d_stat_value(rec, args->m.stat);
	out.q = xs_quantise(v);
	out.q2 = xs_quantise_sq(v);
	out.key = key;
	return out;
}

// A partial result of n contributions into the global accumulators of `cell` (< x_bins * y_bins: the entry point checked every bin).
__device__ __forceinline__ void d_agg_global(const AggMap& am, uint32_t cell, uint32_t n, long long q, unsigned long long q2, long long mn, long long mx) {
	unsigned long long* const w = am.acc + (size_t)cell * AGG_CELL_WORDS;
	atomicAdd(w + AGG_W_N, (unsigned long long)n);
	atomicAdd(w + AGG_W_Q_HI, (unsigned long long)xs_split_hi<AGG_SPLIT>(q));      // (two's complement: the word is read as signed)
	atomicAdd(w + AGG_W_Q_LO, xs_split_lo<AGG_SPLIT>(q));
	atomicAdd(w + AGG_W_Q2_HI, xs_split_hi_u<AGG_SPLIT>(q2));
	atomicAdd(w + AGG_W_Q2_LO, xs_split_lo_u<AGG_SPLIT>(q2));
	atomicMin(reinterpret_cast<long long*>(w + AGG_W_MIN), mn);
	atomicMax(reinterpret_cast<long long*>(w + AGG_W_MAX), mx);
}

// The LDS windows of a block: [orientation][row-side bin][column-side bin].
struct AggWindows {
	long long q[2 * AGG_WIN_CELLS];
	unsigned long long q2[2 * AGG_WIN_CELLS];
	long long mn[2 * AGG_WIN_CELLS], mx[2 * AGG_WIN_CELLS];
	uint32_t n[2 * AGG_WIN_CELLS];
};

// A wave group's result into the window of orientation o at (a, b) if that lies inside (unsigned: a bin below the anchor wraps to
// outside, and so does any bin against an anchor that is off the landscape), into the global cell if not.
__device__ __forceinline__ void d_agg_add(const AggMap& am, AggWindows& w, uint32_t o, uint32_t a, uint32_t b, uint32_t cell,
                                          uint32_t n, long long q, unsigned long long q2, long long mn, long long mx) {
	if (a < AGG_WIN_A && b < AGG_WIN_B) {
		const uint32_t at = o * AGG_WIN_CELLS + a * AGG_WIN_B + b;
		atomicAdd(w.n + at, n);
		atomicAdd(reinterpret_cast<unsigned long long*>(w.q + at), (unsigned long long)q);
		atomicAdd(w.q2 + at, q2);
		atomicMin(w.mn + at, mn);
		atomicMax(w.mx + at, mx);
	} else
		d_agg_global(am, cell, n, q, q2, mn, mx);
}

// The packed key of the variant at position s of the plane set, AGG_NO_KEY beyond the last variant.
__device__ __forceinline__ uint32_t d_agg_key_at(const AggArgs* args, uint32_t s) {
	if (s >= args->p.n_variants) return AGG_NO_KEY;
	const uint32_t* ids = args->p.tv.ids;
	return args->m.key[ids ? ids[s] : s];
}

__global__ __launch_bounds__(AGG_THREADS)
void k_ld_aggregate(const AggArgs* __restrict__ args) {
	__shared__ AggWindows win;
	const AggMap am = args->m;
	const uint32_t nA = args->p.nA, nB = args->p.nB;
	const uint32_t j = blockIdx.x * AGG_THREADS + threadIdx.x;
	const uint32_t i0 = blockIdx.y * AGG_ROWS;
	const int lane = threadIdx.x & 63;
	if (d_block_dead(args->p, blockIdx.x, AGG_THREADS, i0)) return;      // (uniform over the block)
	// the anchors: the bins of the block's first row and first column (uniform over the block)
	const uint32_t keyA0 = d_agg_key_at(args, args->p.tv.a0 + i0), keyB0 = d_agg_key_at(args, args->p.tv.b0 + blockIdx.x * AGG_THREADS);
	const uint32_t ax0 = ag_x(keyA0), ay0 = ag_y(keyA0), bx0 = ag_x(keyB0), by0 = ag_y(keyB0);
	for (uint32_t c = threadIdx.x; c < 2 * AGG_WIN_CELLS; c += AGG_THREADS) {
		win.n[c] = 0u; win.q[c] = 0ll; win.q2[c] = 0ull; win.mn[c] = AGG_I64_MAX; win.mx[c] = AGG_I64_MIN;
	}
	__syncthreads();
#pragma unroll 1
	for (uint32_t r = 0; r < AGG_ROWS; ++r) {
		const uint32_t i = i0 + r;
		AggPair pr{0ll, 0ull, AGG_NO_KEY};
		if (i < nA && j < nB) pr = d_agg_pair(args, i, j);
		const unsigned long long todo = __ballot(pr.key != AGG_NO_KEY);
		if (!todo) continue;                                         // (uniform over the wave)
		const uint32_t keyA = d_agg_key_at(args, args->p.tv.a0 + i);  // (the row's variant: the same in every lane)
		const uint32_t xa = ag_x(keyA), ya = ag_y(keyA);
		d_key_groups(pr.key, todo, [&](int first, uint32_t kb, bool mine, unsigned long long same) {
			long long q = mine ? pr.q : 0ll, mn = mine ? pr.q : AGG_I64_MAX, mx = mine ? pr.q : AGG_I64_MIN;
			unsigned long long q2 = mine ? pr.q2 : 0ull;
			if (same & (same - 1)) {                                 // (uniform: more than one lane with the key)
				q = d_wave_reduce(q, WaveSum());
				q2 = d_wave_reduce(q2, WaveSum());
				mn = d_wave_reduce(mn, WaveMin());
				mx = d_wave_reduce(mx, WaveMax());
			}
			if (lane == first) {
				const uint32_t n = (uint32_t)__popcll(same), xb = ag_x(kb), yb = ag_y(kb);
				if (xa != AGG_OFF && yb != AGG_OFF) d_agg_add(am, win, 0, xa - ax0, yb - by0, xa * am.y_bins + yb, n, q, q2, mn, mx);
				if (xb != AGG_OFF && ya != AGG_OFF) d_agg_add(am, win, 1, ya - ay0, xb - bx0, xb * am.y_bins + ya, n, q, q2, mn, mx);
			}
		});
	}
	__syncthreads();
	// (a touched window cell was reached from its anchors by valid bins: its cell exists)
	for (uint32_t c = threadIdx.x; c < 2 * AGG_WIN_CELLS; c += AGG_THREADS) {
		const uint32_t n = win.n[c];
		if (!n) continue;
		const uint32_t o = c / AGG_WIN_CELLS, a = c % AGG_WIN_CELLS / AGG_WIN_B, b = c % AGG_WIN_B;
		const uint32_t cell = o == 0 ? (ax0 + a) * am.y_bins + (by0 + b) : (bx0 + b) * am.y_bins + (ay0 + a);
		d_agg_global(am, cell, n, win.q[c], win.q2[c], win.mn[c], win.mx[c]);
	}
}

// In front of a call's launches: every cell's sums and count 0, its minimum INT64_MAX, its maximum INT64_MIN.  One word a thread.
__global__ __launch_bounds__(256)
void k_ld_aggregate_init(unsigned long long* __restrict__ acc, unsigned long long words) {
	const unsigned long long k = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
	if (k >= words) return;
	const uint32_t w = (uint32_t)(k % AGG_CELL_WORDS);
	acc[k] = w == AGG_W_MIN ? (unsigned long long)AGG_I64_MAX : w == AGG_W_MAX ? (unsigned long long)AGG_I64_MIN : 0ull;
}

}  // namespace twk
