// LD splitting (twk_hip_ld_split; include/twk_hip.h has the contract, ld_split_index.h the index arithmetic and the quantities): the
// chromosome cut into K blocks of min_size .. max_size variants so that as little r2 as possible crosses a cut, for every K up to k_max,
// from the banded r2 matrix the bandmat kind filled (ld_bandmat.hip.h) - which stays on the device.  64-bit integers throughout, plain
// stores only, every slot written once: the same bytes for any tiling and on any repeat.
//
//   k_split_prefix   one wave per band row u, 64 columns a step, in k_blocks_prefix's manner: the lane quantises its float on the fly
//                    (xs_quantise), an inclusive wave scan of the 64 integers by six shuffles of both halves, a carried sum.
//                    Rp[u][j] is stored offset-major for j <= upc[u]; the wave walks on to the end of the row's band for the row's
//                    total, which is T's share of the row (T counts every in-band pair, whatever max_size).
//   k_split_sums     one thread per b walks d upwards: W[d][b] = W[d - 1][b] + Rp[b - d][d - 1], the running sum in a register.
//                    Consecutive lanes are consecutive b - consecutive u = b - d of one offset-major row of Rp, consecutive slots of
//                    W[d] - so loads and stores are coalesced, except where a prefix saturates (the lane's own upc decides the row).
//   k_split_layer    one launch per k: G_k and D_k from G_(k-1) and W, a max-plus band product.  A block owns 256 consecutive b of
//                    the layer's range and goes through the d that can meet a feasible G_(k-1) in windows of 768: it stages the 1023
//                    entries of G_(k-1) the window's lanes read in LDS (entries outside the previous layer's range are infeasible and
//                    not loaded), then every lane walks d upwards - G from LDS at consecutive addresses, W[d][b] coalesced - and
//                    keeps the first maximum under a strict >.  Whatever max_size, the stage is 8 KB.
//   k_split_backtrack  one block: all lanes add up the rows' totals (integers: any order), then lane K - 1 reads G_K(n), and where it
//                    is feasible walks its chain through D and stores cost and cuts.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ld_bandmat_index.h"
#include "ld_split_index.h"

namespace twk {

struct SplitSizes { uint32_t n, min_size, max_size, k_max; };

// The 64-bit value of lane (lane - delta), by halves.
__device__ inline long long sp_shfl_up(long long x, unsigned delta) {
	const int lo = __shfl_up((int)(uint32_t)(unsigned long long)x, delta), hi = __shfl_up((int)(uint32_t)((unsigned long long)x >> 32), delta);
	return (long long)((unsigned long long)(uint32_t)hi << 32 | (uint32_t)lo);
}

// ... and of lane src.
__device__ inline long long sp_shfl(long long x, int src) {
	const int lo = __shfl((int)(uint32_t)(unsigned long long)x, src), hi = __shfl((int)(uint32_t)((unsigned long long)x >> 32), src);
	return (long long)((unsigned long long)(uint32_t)hi << 32 | (uint32_t)lo);
}

__global__ __launch_bounds__(SPLIT_THREADS)
void k_split_prefix(const float* __restrict__ band, const BandRow* __restrict__ rows, const uint32_t* __restrict__ upc, uint32_t n,
                    long long* __restrict__ rp, long long* __restrict__ row_total) {
	const uint32_t u = blockIdx.x * (SPLIT_THREADS / 64) + (threadIdx.x >> 6);
	const uint32_t lane = threadIdx.x & 63;
	if (u >= n) return;                                      // (uniform over the wave)
	const BandRow row = rows[u];
	const uint32_t upper = sp_upper(row.first, row.len, u), keep = upc[u];
	const float* mine = band + row.base + (u - row.first);   // mine[j]: the entry (u, u + j)
	long long carry = 0;
	for (uint32_t j0 = 1; j0 <= upper; j0 += 64) {
		const uint32_t j = j0 + lane;
		long long x = j <= upper ? xs_quantise((double)mine[j]) : 0;
#pragma unroll
		for (unsigned delta = 1; delta < 64; delta <<= 1) {
			const long long below = sp_shfl_up(x, delta);
			if (lane >= delta) x += below;
		}
		x += carry;
		if (j <= keep) rp[sp_rp_slot(j, u, n)] = x;
		carry = sp_shfl(x, 63);                              // (inclusive: lane 63 holds the step's sum, the carry included)
	}
	if (lane == 0) row_total[u] = carry;
}

__global__ __launch_bounds__(SPLIT_THREADS)
void k_split_sums(const long long* __restrict__ rp, const uint32_t* __restrict__ upc, SplitSizes s, long long* __restrict__ w) {
	const uint64_t at = (uint64_t)blockIdx.x * SPLIT_THREADS + threadIdx.x + 1;
	if (at > s.n) return;
	const uint32_t b = (uint32_t)at;
	sp_block_sums_of(b, s.min_size, s.max_size,
	                 [&](uint32_t u) { return upc[u]; },
	                 [&](uint32_t j, uint32_t u) { return rp[sp_rp_slot(j, u, s.n)]; },
	                 [&](uint32_t d, uint32_t bb, long long v) { w[sp_w_slot(d, bb, s.n, s.min_size)] = v; });
}

// Layer k over b = lo .. hi (sp_layer_lo / _hi of k), the previous layer's range [p_lo, p_hi] (k = 1: [0, 0], G_0(0) = 0).
// g_n[k] = G_k(n) where n lies in the range (preset to infeasible by the caller).
__global__ __launch_bounds__(SPLIT_THREADS)
void k_split_layer(const long long* __restrict__ g_prev, const long long* __restrict__ w, SplitSizes s, uint32_t k, uint32_t lo, uint32_t hi,
                   uint32_t p_lo, uint32_t p_hi, long long* __restrict__ g_cur, uint16_t* __restrict__ dk, long long* __restrict__ g_n) {
	__shared__ long long stage[SPLIT_LDS_G + 1];
	const uint32_t tid = threadIdx.x;
	const uint32_t b0 = lo + blockIdx.x * SPLIT_THREADS;      // (the grid covers lo .. hi: b0 <= hi)
	const uint32_t b_last = hi - b0 < SPLIT_THREADS - 1 ? hi : b0 + (SPLIT_THREADS - 1);
	const uint32_t b = b0 + tid;
	uint32_t d_lo, d_hi;
	sp_block_d_range(b0, b_last, p_lo, p_hi, s.min_size, s.max_size, &d_lo, &d_hi);
	long long best = SPLIT_INFEASIBLE;
	uint32_t best_d = 0;
	for (uint32_t w_lo = d_lo; w_lo < d_hi; w_lo += SPLIT_WINDOW_D) {      // (uniform over the block)
		const uint32_t w_hi = d_hi - w_lo < SPLIT_WINDOW_D ? d_hi : w_lo + SPLIT_WINDOW_D;
		const long long base = sp_stage_base(b0, w_hi);
		const uint32_t count = sp_stage_count(w_lo, w_hi);
		__syncthreads();                                                    // the previous window's readers are through
		for (uint32_t i = tid; i < count; i += SPLIT_THREADS)
			stage[i] = sp_stage_value(base + i, p_lo, p_hi, [&](uint32_t at) { return g_prev[at]; });
		__syncthreads();
		if (b <= b_last)
			sp_lane_window(b, b0, w_lo, w_hi, [&](uint32_t i) { return stage[i]; },
			               [&](uint32_t d, uint32_t bb) { return w[sp_w_slot(d, bb, s.n, s.min_size)]; }, &best, &best_d);
	}
	if (b > b_last) return;
	g_cur[b] = best;
	dk[sp_d_slot(k, b, s.n)] = (uint16_t)best_d;
	if (b == s.n) g_n[k] = best;
}

// out_total[0] = T; per K = 1 .. k_max: feasible[K - 1], and where it is 1 cost[K - 1] = T - G_K(n) and cuts[sp_cut_slot(K, 0 .. K)].
// broken[0]: the number of feasible K whose chain did not end at 0 (never: the host checks that it is 0).
__global__ __launch_bounds__(SPLIT_MAX_K)
void k_split_backtrack(const long long* __restrict__ row_total, const long long* __restrict__ g_n, const uint16_t* __restrict__ dk, SplitSizes s,
                       unsigned long long* __restrict__ out_total, uint8_t* __restrict__ feasible, unsigned long long* __restrict__ cost,
                       uint32_t* __restrict__ cuts, uint32_t* __restrict__ broken) {
	__shared__ unsigned long long part[SPLIT_MAX_K];
	__shared__ uint32_t bad[SPLIT_MAX_K];
	const uint32_t tid = threadIdx.x;
	unsigned long long sum = 0;
	for (uint32_t u = tid; u < s.n; u += SPLIT_MAX_K) sum += (unsigned long long)row_total[u];
	part[tid] = sum;
	__syncthreads();
	for (uint32_t half = SPLIT_MAX_K / 2; half; half >>= 1) {
		if (tid < half) part[tid] += part[tid + half];
		__syncthreads();
	}
	const unsigned long long total = part[0];
	if (tid == 0) out_total[0] = total;
	uint32_t mine_bad = 0;
	const uint32_t K = tid + 1;
	if (K <= s.k_max) {
		const long long gain = g_n[K];
		feasible[K - 1] = gain >= 0;
		if (gain >= 0) {
			cost[K - 1] = total - (unsigned long long)gain;
			const bool whole = sp_backtrack(K, s.n, [&](uint32_t k, uint32_t b) { return (uint32_t)dk[sp_d_slot(k, b, s.n)]; },
			                                [&](uint32_t i, uint32_t b) { cuts[sp_cut_slot(K, i, s.k_max)] = b; });
			mine_bad = whole ? 0u : 1u;
		}
	}
	bad[tid] = mine_bad;
	__syncthreads();
	for (uint32_t half = SPLIT_MAX_K / 2; half; half >>= 1) {
		if (tid < half) bad[tid] += bad[tid + half];
		__syncthreads();
	}
	if (tid == 0) broken[0] = bad[0];
}

}  // namespace twk
