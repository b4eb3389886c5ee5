// What the nine epilogues that reduce a count matrix instead of keeping records share (ld_score.hip.h, ld_prune.hip.h, ld_clump.hip.h,
// ld_matrix.hip.h, ld_decay.hip.h, ld_aggregate.hip.h, ld_score_annot.hip.h, ld_bandmat.hip.h, ld_topk.hip.h; launch_reduce in twk_hip.hip): the shape of a kernel and the toolkit it is built from.
//
// THE SHAPE.  A block is 256 lanes = 256 columns of the launch and walks a fixed number of its rows (32; clump 64; annot 16) in a loop that is not
// unrolled.  A lane's pair goes through d_pair<SRC_MATRIX> (ld_math.hip.h) with the launch's StatsParams - the pair rules, the regrouped
// sets' ids, auto_select, window and option bits are the record path's own code - in a function that is OUT OF LINE: the registers of
// the two maths are then the callee's and are not held across the row loop (inlined, k_ld_score needs 191 VGPRs: two waves a SIMD).
// The PARAMETER BLOCK lives in device memory and the kernel takes a pointer to it: as a kernel argument it is held in ~170 scalar
// registers across the loop and spilled into vector registers (206 VGPRs; the same finding as k_ld_stats_list's).  A block that lies
// wholly on or below the diagonal of a diagonal launch has no pair (the banded matrix also knows the blocks wholly outside its band).  What a kernel does with `keep` - sum, ballot, store, bin, select - is its own.
//
// THE TOOLKIT.  A new kind is one kernel file built from these, plus one entry point:
//   ReduceParams<Map>  the parameter block {p, m}: the launch's StatsParams and the kind's map.  Every kind derives its own, by name.
//   d_reduce_keeps     the pair function of the kinds that only ask "would `calc` report it?" (prune, clump).
//   d_stat_value       signed r, r2, D or D' of a record, by TWK_HIP_STAT_*.
//   d_wave_reduce      one butterfly over the wave's 64 lanes for any value type and operation (WaveSum, WaveMin, WaveMax).
//   d_key_groups       the lanes of a wave grouped by a key, one call per distinct key: the "in the wave" step of the kinds that bin.
//   d_or_bits, d_block_dead
// WHAT STAYS PER KIND.  The pair function: each returns its own small result in registers and the record stays local to the callee (a
// shared one that returned the record would pass 104 bytes through memory), so d_stat_value is inlined INTO those out-of-line bodies.
// The row loop: the nine carry different state across rows (clump's column word, the matrix's and the band's LDS stage, score's partials, annot's parked r2,
// top-k's LDS lists).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ld_math.hip.h"

namespace twk {

// The parameter block of a reduce launch, in device memory (see above): the launch's own parameters and the kind's map - where its results go.
template <class Map>
struct ReduceParams { StatsParams p; Map m; };

// One pair of the launch's matrix: would `calc` report it?  (Prune's and clump's question; score and matrix also want a field of the
// record and keep a function of their own.)
__device__ __noinline__ bool d_reduce_keeps(const StatsParams* pp, uint32_t i, uint32_t j) {
	const StatsParams& p = *pp;
	twk_hip_record rec;
	return d_pair<SRC_MATRIX>(p, p.tv.a0 + i, p.tv.b0 + j, i, j, 0, &rec);
}

// The statistic `stat` (TWK_HIP_STAT_*; the entry points refuse any other value) of a record.  Inlined into the caller's own out-of-line
// pair function.
__device__ __forceinline__ double d_stat_value(const twk_hip_record& rec, int32_t stat) {
	switch (stat) {
	case TWK_HIP_STAT_R:  return copysign(rec.R, rec.D);
	case TWK_HIP_STAT_R2: return rec.R2;
	case TWK_HIP_STAT_D:  return rec.D;
	default:              return rec.Dprime;
	}
}

// x reduced with `op` over the wave's 64 lanes, the same value in every lane: a butterfly whose pairing does not depend on the data
// (masks 32, 16, .. 1), so a floating-point sum adds in one fixed order.
struct WaveSum { template <class T> __device__ T operator()(T a, T b) const { return a + b; } };
struct WaveMin { template <class T> __device__ T operator()(T a, T b) const { return b < a ? b : a; } };
struct WaveMax { template <class T> __device__ T operator()(T a, T b) const { return b > a ? b : a; } };
template <class T, class Op>
__device__ __forceinline__ T d_wave_reduce(T x, Op op) {
#pragma unroll
	for (int m = 32; m >= 1; m >>= 1) x = op(x, __shfl_xor(x, m, 64));
	return x;
}

// The wave's lanes grouped by `key`: group(first, k, mine, same) is called once per distinct key k != no_key present in the wave, in all
// 64 lanes alike - first: the lowest lane that holds k; mine: this lane holds k; same: the ballot of the lanes that do.  Every lane stays
// in the loop (its condition is the wave's) and the lanes of one key leave the remaining set together, so it is right for any
// distribution of keys over the lanes: a regrouped set is not in position order.  A lane that holds no_key (no pair) is in no group.
// (todo: the ballot of the lanes that hold a key, for a caller that has taken it already)
template <class Group>
__device__ __forceinline__ void d_key_groups(uint32_t key, unsigned long long todo, Group&& group) {
	while (todo) {
		const int first = __ffsll((long long)todo) - 1;
		const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)key, first);
		const bool mine = key == k;
		const unsigned long long same = __ballot(mine);
		group(first, k, mine, same);
		todo &= ~same;
	}
}
template <class Group>
__device__ __forceinline__ void d_key_groups(uint32_t key, uint32_t no_key, Group&& group) { d_key_groups(key, __ballot(key != no_key), group); }

// ORs the 64 bits `bits`, the first of them bit `bit0` of the row, into the one or two words of the row they straddle (nothing where
// they are 0, nothing beyond the row).
__device__ __forceinline__ void d_or_bits(unsigned long long* row, uint32_t stride, uint32_t bit0, unsigned long long bits) {
	const uint32_t at = bit0 >> 6, sh = bit0 & 63;
	const unsigned long long lo = bits << sh, hi = sh ? bits >> (64 - sh) : 0ull;
	if (lo && at < stride) atomicOr(row + at, lo);
	if (hi && at + 1 < stride) atomicOr(row + at + 1, hi);
}

// The block of `cols` columns from column block bx on, whose first row is i0, lies wholly on or below the diagonal of a diagonal launch.
// (k_ld_matrix_fill asks mx_block_dead, ld_matrix_index.h: the same test, where the host check can play it.)
__device__ __forceinline__ bool d_block_dead(const StatsParams& p, uint32_t bx, uint32_t cols, uint32_t i0) {
	return p.diag && p.tv.a0 == p.tv.b0 && bx * cols + (cols - 1) <= i0;
}

}  // namespace twk
