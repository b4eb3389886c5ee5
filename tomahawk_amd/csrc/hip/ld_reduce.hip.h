// What the six epilogues that reduce a count matrix instead of keeping records share (ld_score.hip.h, ld_prune.hip.h, ld_clump.hip.h,
// ld_matrix.hip.h, ld_decay.hip.h, ld_aggregate.hip.h; launch_reduce in twk_hip.hip).
//
// THE SHAPE.  A block is 256 lanes = 256 columns of the launch and walks a fixed number of its rows (32; clump 64) in a loop that is not
// unrolled.  A lane's pair goes through d_pair<SRC_MATRIX> (ld_math.hip.h) with the launch's StatsParams - the pair rules, the regrouped
// sets' ids, auto_select, window and option bits are the record path's own code - in a function that is OUT OF LINE: the registers of
// the two maths are then the callee's and are not held across the row loop (inlined, k_ld_score needs 191 VGPRs: two waves a SIMD).
// The PARAMETER BLOCK lives in device memory and the kernel takes a pointer to it: as a kernel argument it is held in ~170 scalar
// registers across the loop and spilled into vector registers (206 VGPRs; the same finding as k_ld_stats_list's).  A block that lies
// wholly on or below the diagonal of a diagonal launch has no pair.  What a kernel does with `keep` - sum, ballot, store, bin - is its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ld_math.hip.h"

namespace twk {

// One pair of the launch's matrix: would `calc` report it?  (Prune's and clump's question; score and matrix also want a field of the
// record and keep a function of their own.)
__device__ __noinline__ bool d_reduce_keeps(const StatsParams* pp, uint32_t i, uint32_t j) {
	const StatsParams& p = *pp;
	twk_hip_record rec;
	return d_pair<SRC_MATRIX>(p, p.tv.a0 + i, p.tv.b0 + j, i, j, 0, &rec);
}

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
