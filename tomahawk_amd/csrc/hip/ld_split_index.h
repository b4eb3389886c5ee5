// LD splitting (Prive 2021, "Optimal linkage disequilibrium splitting"): the index arithmetic of the kernels of ld_split.hip.h - which
// slot a lane reads or writes, when a row prefix saturates, which b a layer launch covers, which d a block's windows hold and what a lane
// does with them.  Plain C++ with no HIP in it, in the manner of ld_bandmat_index.h: the kernels include it, and so does
// csrc/tools/split_check.cpp (`make split-check`), which plays every lane of every kernel against a direct evaluation of the definition
// (include/twk_hip.h, twk_hip_ld_split) with bounds-checked arrays.
//
// THE QUANTITIES, all relative to the slice of n variants:
//   q(u, v)   u < v: llrint((double)B[u][v] * 2^32) where v lies in u's band (xs_quantise, ld_exact_sum.h), else 0.
//   Rp[u][j]  j >= 1: q(u, u + 1) + .. + q(u, u + j).  Stored offset-major - slot (j - 1) * n + u - for 1 <= j <= upc[u], where
//             upc[u] = min(upper length of u's band, max_size - 1).  Beyond upc[u] a prefix SATURATES at Rp[u][upc[u]] (q is 0 beyond
//             the band, and no block reaches further than max_size - 1); with upc[u] == 0 it is 0.
//   W[d][b]   within(b - d, b) = W[d - 1][b] + Rp[b - d][d - 1], W[1][b] = 0.  Stored for min_size <= d <= min(max_size, b) at slot
//             (d - min_size) * (n + 1) + b: consecutive b are consecutive slots.
//   G_k(b)    two rolling layers of n + 1 entries, SPLIT_INFEASIBLE where no k-partition of [0, b) exists.  Layer k is written for
//             k * min_size <= b <= min(n, k * max_size) only - no other b can be feasible - and a reader treats every entry outside that
//             range as infeasible without loading it.
//   D_k(b)    the smallest d that attains G_k(b): uint16, slot (k - 1) * (n + 1) + b, written where G_k(b) is feasible or not (0 then).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "ld_exact_sum.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TWK_SP_FN __host__ __device__ inline
#define TWK_SP_UNROLL _Pragma("unroll 8")
#else
#define TWK_SP_FN inline
#define TWK_SP_UNROLL
#endif

namespace twk {

constexpr long long SPLIT_INFEASIBLE = -1;
constexpr uint32_t SPLIT_THREADS = 256;              // a layer block owns 256 consecutive b
constexpr uint32_t SPLIT_WINDOW_D = 768;             // the d a window of the layer kernel holds ...
constexpr uint32_t SPLIT_LDS_G = SPLIT_WINDOW_D + SPLIT_THREADS - 1;      // ... and the entries of G_(k-1) it stages for them: 1023 (8 KB)
constexpr uint32_t SPLIT_MAX_SIZE = 65535;           // D is uint16
constexpr uint32_t SPLIT_MAX_K = 1024;               // one lane of the backtrack block per K
constexpr uint64_t SPLIT_MAX_PAIRS = 1ull << 31;     // in-band pairs u < v of a call: T stays below 2^63

// What twk_hip_ld_split refuses about its three sizes before it looks at anything else.
TWK_SP_FN bool sp_sizes_ok(uint32_t n, uint32_t min_size, uint32_t max_size, uint32_t k_max) {
	return min_size >= 1 && min_size <= max_size && max_size <= SPLIT_MAX_SIZE && k_max >= 1 && k_max <= SPLIT_MAX_K && (uint64_t)n * max_size < (1ull << 32);
}

// ---- row prefixes ----
// The columns v > u of the band row {first, len} of variant u (the band holds its diagonal: first <= u < first + len).
TWK_SP_FN uint32_t sp_upper(uint32_t first, uint32_t len, uint32_t u) { return first + len - 1 - u; }
// ... of which a block of at most max_size variants can hold max_size - 1.
TWK_SP_FN uint32_t sp_upc(uint32_t upper, uint32_t max_size) { return upper < max_size - 1 ? upper : max_size - 1; }
// Slot of Rp[u][j], 1 <= j <= upc[u].
TWK_SP_FN uint64_t sp_rp_slot(uint32_t j, uint32_t u, uint32_t n) { return (uint64_t)(j - 1) * n + u; }
// The saturation rule: the stored offset that holds Rp[u][j] for any j >= 0; 0: the prefix is 0 and nothing is loaded.
TWK_SP_FN uint32_t sp_rp_offset(uint32_t j, uint32_t upc) { return j < upc ? j : upc; }

// ---- block sums ----
TWK_SP_FN uint64_t sp_w_slot(uint32_t d, uint32_t b, uint32_t n, uint32_t min_size) { return (uint64_t)(d - min_size) * ((uint64_t)n + 1) + b; }
// Thread b of the block-sum kernel, 1 <= b <= n: d ascending, the running sum in a register, a store from min_size on.
template <class RpAt, class UpcAt, class Store>
TWK_SP_FN void sp_block_sums_of(uint32_t b, uint32_t min_size, uint32_t max_size, UpcAt upc_at, RpAt rp_at, Store store) {
	const uint32_t d_end = max_size < b ? max_size : b;
	long long w = 0;
	for (uint32_t d = 1; d <= d_end; ++d) {
		const uint32_t u = b - d, j = sp_rp_offset(d - 1, upc_at(u));
		if (j) w += rp_at(j, u);
		if (d >= min_size) store(d, b, w);
	}
}

// ---- layers ----
// The b a layer can make feasible: [lo, hi], empty (lo > hi) where k * min_size > n.  (k <= 1024, sizes <= 65535: 32 bits hold them.)
TWK_SP_FN uint32_t sp_layer_lo(uint32_t k, uint32_t min_size) { return k * min_size; }
TWK_SP_FN uint32_t sp_layer_hi(uint32_t k, uint32_t max_size, uint32_t n) { const uint32_t top = k * max_size; return top < n ? top : n; }
TWK_SP_FN uint64_t sp_d_slot(uint32_t k, uint32_t b, uint32_t n) { return (uint64_t)(k - 1) * ((uint64_t)n + 1) + b; }
// The d of a block's lanes b0 .. b_last that can meet a feasible G_(k-1): b - d inside [p_lo, p_hi] for one of them, inside
// [min_size, max_size].  -> [*d_lo, *d_hi), empty where *d_lo >= *d_hi.
TWK_SP_FN void sp_block_d_range(uint32_t b0, uint32_t b_last, uint32_t p_lo, uint32_t p_hi, uint32_t min_size, uint32_t max_size, uint32_t* d_lo, uint32_t* d_hi) {
	uint32_t lo = b0 > p_hi ? b0 - p_hi : 0, hi = b_last >= p_lo ? b_last - p_lo + 1 : 0;
	if (lo < min_size) lo = min_size;
	if (hi > max_size + 1) hi = max_size + 1;
	*d_lo = lo; *d_hi = hi;
}
// A window [w_lo, w_hi) of d, at most SPLIT_WINDOW_D wide: stage entry i holds G_(k-1)(base + i), base = b0 - (w_hi - 1) (negative near
// the slice's start), for i < count.  Lane b reads entry (b - d) - base = (b - b0) + (w_hi - 1 - d): inside [0, count) for every
// b0 <= b < b0 + SPLIT_THREADS and w_lo <= d < w_hi.
TWK_SP_FN long long sp_stage_base(uint32_t b0, uint32_t w_hi) { return (long long)b0 - (long long)(w_hi - 1); }
TWK_SP_FN uint32_t sp_stage_count(uint32_t w_lo, uint32_t w_hi) { return (w_hi - 1 - w_lo) + SPLIT_THREADS; }
TWK_SP_FN uint32_t sp_stage_entry(uint32_t b, uint32_t b0, uint32_t d, uint32_t w_hi) { return (b - b0) + (w_hi - 1 - d); }
// What entry `at` = base + i of the stage holds: G_(k-1)(at) inside the previous layer's range, infeasible outside it - never loaded there.
template <class GAt>
TWK_SP_FN long long sp_stage_value(long long at, uint32_t p_lo, uint32_t p_hi, GAt g_at) {
	return at >= (long long)p_lo && at <= (long long)p_hi ? g_at((uint32_t)at) : SPLIT_INFEASIBLE;
}
// Lane b through one window, d ascending.  The strict > keeps the smallest d of a maximum; d > b has no G.  W[d][b] is loaded whether or
// not G_(k-1)(b - d) is feasible - the slot exists for every min_size <= d <= min(max_size, b) - so that the loads of several d do not
// wait for one another's comparison (the device unrolls the loop by 8); an infeasible G only keeps its candidate from being taken.
template <class StageAt, class WAt>
TWK_SP_FN void sp_lane_window(uint32_t b, uint32_t b0, uint32_t w_lo, uint32_t w_hi, StageAt stage_at, WAt w_at, long long* best, uint32_t* best_d) {
	const uint32_t end = w_hi <= b ? w_hi : b + 1;
	TWK_SP_UNROLL
	for (uint32_t d = w_lo; d < end; ++d) {
		const long long g = stage_at(sp_stage_entry(b, b0, d, w_hi));
		const long long cand = g + w_at(d, b);
		if (g >= 0 && cand > *best) { *best = cand; *best_d = d; }
	}
}

// ---- backtrack ----
TWK_SP_FN uint64_t sp_cut_slot(uint32_t K, uint32_t i, uint32_t k_max) { return (uint64_t)(K - 1) * (k_max + 1) + i; }
// Lane K walks its chain from (K, n) through D.  -> false where the chain is broken (a d of 0 or beyond b, an end other than 0): never
// with a feasible G_K(n), a bound and not a case.
template <class DAt, class Store>
TWK_SP_FN bool sp_backtrack(uint32_t K, uint32_t n, DAt d_at, Store store) {
	uint32_t b = n;
	for (uint32_t k = K; k >= 1; --k) {
		store(k, b);
		const uint32_t d = d_at(k, b);
		if (d == 0 || d > b) return false;
		b -= d;
	}
	store(0, b);
	return b == 0;
}

}  // namespace twk
