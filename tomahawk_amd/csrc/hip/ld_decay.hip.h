// LD decay: the epilogue of a count matrix that bins instead of appending (twk_hip_ld_decay, include/twk_hip.h).
//
// A pair COUNTS when `calc` would report a record for it, both variants lie on one contig and their positions differ; its distance
// d = |posA - posB| falls into bin min(d / width, n_bins - 1), width = range_bp / n_bins (ld_decay_bin.h: the reference's arithmetic,
// two_reader::Decay).  Per bin the call returns the number of counting pairs and the sum of their R2.  A decay launch runs the count
// kernel into C like a record launch and then
//   k_ld_decay   one pair per lane through d_pair<SRC_MATRIX> (ld_math.hip.h) with the launch's StatsParams - the pair rules, the
//                regrouped sets' ids, auto_select, window, option bits are the record path's own code - and only `keep` and rec.R2 are
//                used; positions and contigs are p.vm.pos / p.vm.rid of the two variant ids, as d_pair resolves them.  The shape is
//                ld_reduce.hip.h's: 256 lanes = 256 columns, DECAY_ROWS rows in a loop that is not unrolled, the parameter block in
//                device memory, the pair out of line, blocks below the diagonal skipped.
// THE SUMS ARE EXACT AND HAVE NO ORDER.  A counting pair adds the integer q = rint(R2 * 2^32) (ld_exact_sum.h: one rounding, at most
// 2^-33 from R2), and integers add up the same in any order: two runs, any tiling and any launch order return the same bits, and no
// floating-point atomic is used anywhere.
//   in the wave  adjacent columns of a row mostly share a bin, so 64 lanes adding to one LDS word would serialise.  The lanes are
//                grouped by bin (d_key_groups, ld_reduce.hip.h): per bin present their q are added up over the wave (d_wave_reduce over
//                64-bit integers; a bin with one lane skips it), and the first lane adds the sum and the ballot's popcount to the
//                block's histogram.  Right for any distribution of bins over the lanes: a regrouped set is not in position order.
//   in the block the histogram lives in dynamic LDS - a uint64 sum and a uint32 count per bin, 12 bytes x n_bins, n_bins <= 4096
//                (48 KiB) - zeroed at block start, added to with LDS integer atomics (the block's four waves share it).
//   at the end   for every bin the block counted a pair in, three global 64-bit integer atomic adds, with K = DECAY_SPLIT = 32
//                (ld_exact_sum.h's split): S >> 32 into acc_int[bin], S & 0xffffffff into acc_frac[bin], the count into acc_n[bin].  No carry between the words and no branch on the data:
//                every path runs on every input.  The host forms (acc_int << 32) + acc_frac in 128 bits and converts once.
// HEADROOM.  A block holds DECAY_THREADS * DECAY_ROWS = 8192 pairs and q <= 2^32 (+ a few ulps of R2), so a block's S < 2^46.
// acc_frac takes less than 2^32 a flush: room for 2^32 flushes a bin; acc_int takes S >> 32 < 2^14 a flush and less than one a
// pair: room for 2^64 pairs.  The engine counts the blocks it launches for a call and refuses the launch that would pass 2^32 - at
// least 2^32 blocks of up to 8192 pairs, far beyond 2^40 pairs a call.
// No Fisher test (minP >= 1), no survivor buffer, no sort; 24 bytes per bin leave the device.  The reference's counterpart reads a
// sorted .two file; here no record is formed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ld_math.hip.h"
#include "ld_reduce.hip.h"
#include "ld_decay_bin.h"

namespace twk {

constexpr int DECAY_THREADS = 256;      // columns of a block
constexpr int DECAY_ROWS = 32;          // rows of a block
constexpr uint32_t DECAY_NO_BIN = 0xFFFFFFFFu;

struct DecayMap {
	unsigned long long* acc_int;        // [n_bins] sums of S >> 32
	unsigned long long* acc_frac;       // [n_bins] sums of S & 0xffffffff
	unsigned long long* acc_n;          // [n_bins] counting pairs
	uint32_t width, n_bins;
};
struct DecayArgs : ReduceParams<DecayMap> {};
// LDS of a block: the sums, then the counts.
inline size_t decay_lds_bytes(uint32_t n_bins) { return (size_t)n_bins * (sizeof(unsigned long long) + sizeof(uint32_t)); }

struct DecayPair { unsigned long long q; uint32_t bin; };

// One pair of the launch's matrix: its bin and its quantised r2 if it counts, DECAY_NO_BIN if not.  Out of line, so that the registers
// of the two maths are the callee's and not held across the row loop (ld_reduce.hip.h).
__device__ __noinline__ DecayPair d_decay_pair(const DecayArgs* args, uint32_t i, uint32_t j) {
	const StatsParams& p = args->p;
	const uint32_t sA = p.tv.a0 + i, sB = p.tv.b0 + j;
	twk_hip_record rec;
	DecayPair out{0ull, DECAY_NO_BIN};
	if (!d_pair<SRC_MATRIX>(p, sA, sB, i, j, 0, &rec)) return out;
	// (keep implies both set positions below n_variants: the ids are there)
	const uint32_t A = p.tv.ids ? p.tv.ids[sA] : sA, B = p.tv.ids ? p.tv.ids[sB] : sB;
	const uint32_t pa = p.vm.pos[A], pb = p.vm.pos[B];
	if (p.vm.rid[A] != p.vm.rid[B] || pa == pb) return out;
	out.bin = dk_bin(dk_distance(pa, pb), args->m.width, args->m.n_bins);
	out.q = (unsigned long long)xs_quantise(rec.R2);
	return out;
}

__global__ __launch_bounds__(DECAY_THREADS)
void k_ld_decay(const DecayArgs* __restrict__ args) {
	extern __shared__ __attribute__((aligned(16))) unsigned char decay_lds[];
	const DecayMap dm = args->m;
	unsigned long long* const h_sum = reinterpret_cast<unsigned long long*>(decay_lds);
	uint32_t* const h_n = reinterpret_cast<uint32_t*>(h_sum + dm.n_bins);
	const uint32_t nA = args->p.nA, nB = args->p.nB;
	const uint32_t j = blockIdx.x * DECAY_THREADS + threadIdx.x;
	const uint32_t i0 = blockIdx.y * DECAY_ROWS;
	const int lane = threadIdx.x & 63;
	if (d_block_dead(args->p, blockIdx.x, DECAY_THREADS, i0)) return;      // (uniform over the block)
	for (uint32_t b = threadIdx.x; b < dm.n_bins; b += DECAY_THREADS) { h_sum[b] = 0ull; h_n[b] = 0u; }
	__syncthreads();
#pragma unroll 1
	for (uint32_t r = 0; r < DECAY_ROWS; ++r) {
		const uint32_t i = i0 + r;
		DecayPair pr{0ull, DECAY_NO_BIN};
		if (i < nA && j < nB) pr = d_decay_pair(args, i, j);
		d_key_groups(pr.bin, DECAY_NO_BIN, [&](int first, uint32_t bin, bool mine, unsigned long long same) {
			unsigned long long s = mine ? pr.q : 0ull;
			if (same & (same - 1)) s = d_wave_reduce(s, WaveSum());      // (uniform: more than one lane in the bin)
			if (lane == first) {
				atomicAdd(h_sum + bin, s);
				atomicAdd(h_n + bin, (uint32_t)__popcll(same));
			}
		});
	}
	__syncthreads();
	for (uint32_t b = threadIdx.x; b < dm.n_bins; b += DECAY_THREADS) {
		const uint32_t n = h_n[b];
		if (!n) continue;
		const unsigned long long s = h_sum[b];
		atomicAdd(dm.acc_int + b, xs_split_hi_u<DECAY_SPLIT>(s));
		atomicAdd(dm.acc_frac + b, xs_split_lo_u<DECAY_SPLIT>(s));
		atomicAdd(dm.acc_n + b, (unsigned long long)n);
	}
}

}  // namespace twk
