// Top-k LD partners: the epilogue of a count matrix that SELECTS instead of summing (twk_hip_ld_topk, include/twk_hip.h): for every
// variant the k partners with the largest |statistic| - signed r, r2, D or D' - among the records `calc` would report with the variant at
// either end.  Proxy lookup: which variants tag this one best?
//
// A candidate is one 64-bit key (ld_topk_key.h) whose unsigned integer order is the list's order - |value| as float32 descending, ties
// to the smaller partner index in file order - and 0 is "empty".  The lists are k slots per variant in device memory, zeroed in front of
// the call's launches, indexed by the variant's id in file order (through p.tv.ids on a regrouped set: neither the lists nor the
// tie-break depend on the default mode's regrouping, and its two passes insert their disjoint pairs into the same lists).
//
// THE SELECTION is a max-cascade (tk_insert, ld_topk_key.h, with the proof): an insertion max-exchanges its key into slot 0 and carries
// the smaller of the two on to slot 1, and so on to slot k - 1.  The lists end as the k largest keys inserted, in order, WHATEVER THE
// INTERLEAVING: any tiling, launch order, shard or repeat returns the same bytes.  Only 64-bit integer atomic maxima are used, no
// floating-point atomic.  A key that is <= a value read from slot[k - 1] - by a plain load, as stale as it likes: slots only grow - is
// not inserted.
//
// A launch runs the count kernel into C like a record launch and then
//   k_ld_topk   ld_reduce.hip.h's shape: 256 lanes = 256 columns, 32 rows in a loop that is not unrolled, the parameter block in device
//               memory, the pair out of line through d_pair<SRC_MATRIX> with d_stat_value inlined into it (it returns the key for the
//               column variant's list, or 0 for no record), blocks below the diagonal return at once.  256 lanes inserting into one
//               row's global list would be 256 * k serialised atomics on k addresses, so the block has TWO LEVELS:
//     thresholds   at block start the global slot[k - 1] of the 32 row variants and the 256 column variants are loaded once.
//     LDS lists    (32 + 256) * k * 8 bytes of dynamic LDS (tk_lds_bytes: 36 KiB at k = 16, 72 KiB at 32).  32 row lists shared by the
//                  four waves: the cascade with LDS 64-bit atomic maxima.  256 column lists, one per lane, lane-interleaved (free of
//                  bank conflicts) and lane-private: the cascade by loads and stores.  A key enters an LDS list only if it beats the
//                  threshold loaded at block start and its own LDS list's last slot as it stands (a column's lane is its list's only writer; a
//                  row's list is read by a plain LDS load while other waves add to it - stale at worst).
//     flush        behind the row loop and one barrier the threads cover the (32 + 256) * k LDS words; each that is not 0 and above a
//                  FRESH read of its variant's global slot[k - 1] goes through the global cascade.  A list's words are walked from
//                  slot 0 on, largest first: the threshold rises as early as it can.
// Whatever a block's thresholds kept out of its LDS lists is below k keys that are, or will be, in the global list; whatever an LDS list
// dropped is below k keys of the same block that are flushed: the two levels change no list (`make topk-check` plays them).
// k * 8 bytes per variant of device memory; no Fisher test (minP >= 1), no survivor buffer, no sort.  There is no reference counterpart.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ld_math.hip.h"
#include "ld_reduce.hip.h"
#include "ld_topk_key.h"

namespace twk {

constexpr int TOPK_THREADS = (int)TOPK_COLS;
constexpr int TOPK_BLOCK_ROWS = (int)TOPK_ROWS;

struct TopkMap {
	unsigned long long* lists;          // [n_variants][k] the slots, by variant id in file order
	uint32_t k;
	int32_t stat;                       // TWK_HIP_STAT_*
};
struct TopkArgs : ReduceParams<TopkMap> {};

// One pair of the launch's matrix: the key of the row variant as a partner of the column variant if `calc` would report the pair, 0 if
// not (the kernel swaps the partner for the other list).  Out of line, so that the registers of the two maths are the callee's and not
// held across the row loop (ld_reduce.hip.h).
__device__ __noinline__ unsigned long long d_topk_pair(const TopkArgs* args, uint32_t i, uint32_t j) {
	const StatsParams& p = args->p;
	const uint32_t sA = p.tv.a0 + i;
	twk_hip_record rec;
	if (!d_pair<SRC_MATRIX>(p, sA, p.tv.b0 + j, i, j, 0, &rec)) return 0ull;
	// (a record implies both set positions below n_variants: the ids are there)
	return tk_pack(d_stat_value(rec, args->m.stat), p.tv.ids ? p.tv.ids[sA] : sA);
}

// The variant at position s of the plane set, TOPK_NO_PARTNER if the launch has none there.
__device__ __forceinline__ uint32_t d_topk_variant(const StatsParams& p, bool inside, uint32_t s) {
	if (!inside || s >= p.n_variants) return TOPK_NO_PARTNER;
	return p.tv.ids ? p.tv.ids[s] : s;
}

// slot[k - 1] of a variant's global list, read past the caches: as fresh as a load can be (any older value would do as well).
__device__ __forceinline__ unsigned long long d_topk_threshold(const TopkMap& tm, uint32_t v) {
	return __atomic_load_n(tm.lists + (size_t)v * tm.k + (tm.k - 1), __ATOMIC_RELAXED);
}

__global__ __launch_bounds__(TOPK_THREADS)
void k_ld_topk(const TopkArgs* __restrict__ args) {
	extern __shared__ __attribute__((aligned(16))) unsigned char topk_lds[];
	__shared__ unsigned long long row_thr[TOPK_ROWS];
	__shared__ uint32_t row_id[TOPK_ROWS], col_id[TOPK_COLS];
	unsigned long long* const lds = reinterpret_cast<unsigned long long*>(topk_lds);
	const TopkMap tm = args->m;
	const uint32_t k = tm.k;
	const uint32_t nA = args->p.nA, nB = args->p.nB;
	const uint32_t t = threadIdx.x;
	const uint32_t j = blockIdx.x * TOPK_COLS + t;
	const uint32_t i0 = blockIdx.y * TOPK_ROWS;
	if (d_block_dead(args->p, blockIdx.x, TOPK_COLS, i0)) return;      // (uniform over the block)
	const uint32_t B = d_topk_variant(args->p, j < nB, args->p.tv.b0 + j);
	col_id[t] = B;
	// (a lane without a variant has no pair: its threshold is never met)
	unsigned long long col_thr = B != TOPK_NO_PARTNER ? d_topk_threshold(tm, B) : ~0ull;
	if (t < TOPK_ROWS) {
		const uint32_t A = d_topk_variant(args->p, i0 + t < nA, args->p.tv.a0 + i0 + t);
		row_id[t] = A;
		row_thr[t] = A != TOPK_NO_PARTNER ? d_topk_threshold(tm, A) : ~0ull;
	}
	const uint32_t words = tk_lds_words(k);
	for (uint32_t e = t; e < words; e += TOPK_COLS) lds[e] = 0ull;
	__syncthreads();
#pragma unroll 1
	for (uint32_t r = 0; r < TOPK_ROWS; ++r) {
		const uint32_t i = i0 + r;
		unsigned long long key = 0ull;
		if (i < nA && j < nB) key = d_topk_pair(args, i, j);
		if (!key) continue;
		// the column variant's list: this lane's own
		if (key > col_thr) {
			tk_insert(k, key, [&](uint32_t s, unsigned long long x) {
				unsigned long long* const w = lds + tk_col_word(k, t, s);
				const unsigned long long old = *w;
				if (x > old) *w = x;
				return old;
			});
			const unsigned long long last = lds[tk_col_word(k, t, k - 1)];
			if (last > col_thr) col_thr = last;
		}
		// the row variant's list: the block's
		const unsigned long long rkey = tk_with_partner(key, B);
		// (... whose own last slot is a threshold too, read as it happens to stand: the waves do not reach a row at the same moment)
		if (rkey > row_thr[r] && rkey > lds[tk_row_word(k, r, k - 1)])
			tk_insert(k, rkey, [&](uint32_t s, unsigned long long x) { return atomicMax(lds + tk_row_word(k, r, s), x); });
	}
	__syncthreads();
#ifndef TWK_TOPK_TIMING_SKIP_FLUSH      // (defined by tests/sweeps/topk_timing.py alone, in a library of its own: wrong lists, the flush's share of the time)
	for (uint32_t e = t; e < words; e += TOPK_COLS) {
		const unsigned long long key = lds[e];
		if (!key) continue;
		bool is_row; uint32_t which;
		tk_word_owner(k, e, &is_row, &which);
		const uint32_t v = is_row ? row_id[which] : col_id[which];      // (a key in the list: the variant exists)
		if (key <= d_topk_threshold(tm, v)) continue;
		unsigned long long* const list = tm.lists + (size_t)v * k;
		tk_insert(k, key, [&](uint32_t s, unsigned long long x) { return atomicMax(list + s, x); });
	}
#endif
}

}  // namespace twk
