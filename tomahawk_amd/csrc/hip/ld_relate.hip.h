// Sample relationship: the genotype matrix transposed on the device into sample-major bit planes, and the epilogue that turns the count
// kernel's plane products into per-pair genotype-sharing counts and one statistic (twk_hip_relationship, include/twk_hip.h).
//
// Between the two runs k_count_list_t (ld_count.hip.h) exactly as the variant paths run it: it contracts the rows of any bit-plane
// matrix and knows nothing of what a row is.  Here a row is a plane of a SAMPLE and the contracted axis is the variants in use:
//   k_relate_transpose  raw layout (variant-major, 16 samples a word) -> P rows a sample, one bit per variant of the call's list
//                       (ld_relate_index.h has the layout and every lane's part).  Lane = variant: a ballot over 64 variants is 64
//                       output bits of one sample and plane.  A lane reads its variant's row 16 bytes at a time, four times from the
//                       same 64 bytes, so every 64-byte sector fetched is used whole; the output is staged in LDS and leaves in whole
//                       128-byte lines.  Every word of the N * P live rows is written, padding included - the rows need no preset.
//   k_relate_epilogue   one sample pair per lane: the 4 (P = 2) or 9 (P = 3) products of the pair from the super-tile's count matrix - in
//                       the two-plane form the margins are the rows' popcounts (k_row_popcount) and n is the list's length - through
//                       rl_counts / rl_fraction to the six counts and ONE double division (IEEE: the build has no fast-math).  Plain
//                       stores, every entry by exactly one lane of one launch: out[a][b], and on a square call the mirrored out[b][a]
//                       with het_a and het_b swapped, staged in LDS so that both orientations leave in runs of 32 consecutive
//                       entries.  No atomics, no scratch.  The parameter block lives in device memory (ld_reduce.hip.h on why).
// There is no reference counterpart that could serve as a parity target.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ld_relate_index.h"

namespace twk {

__global__ __launch_bounds__(RL_THREADS)
void k_relate_transpose(const uint32_t* __restrict__ raw, const uint32_t* __restrict__ rawmask, uint32_t Wp,
                        const uint32_t* __restrict__ ids, uint32_t n_use, uint32_t n_samples, uint32_t P,
                        uint32_t* __restrict__ rows, uint32_t W) {
	__shared__ uint32_t stage[RL_STAGE_WORDS];
	const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const uint32_t n_chunks = W / RL_KC;
	const bool masked = P == 3;
	for (uint32_t chunk = blockIdx.y; chunk < n_chunks; chunk += gridDim.y) {
		// the raw rows of this lane's four positions (a position beyond the list has none: all its bits stay zero)
		const uint32_t* src[4]; const uint32_t* msrc[4];
#pragma unroll
		for (uint32_t k = 0; k < 4; ++k) {
			const uint32_t pos = rl_position(chunk, wave, k, lane);
			const bool valid = pos < n_use;
			const size_t v = valid ? (ids ? ids[pos] : pos) : 0;
			src[k] = valid ? raw + v * Wp : nullptr;
			msrc[k] = valid && masked ? rawmask + v * Wp : nullptr;
		}
#pragma unroll 1
		for (uint32_t pass = 0; pass < RL_PASSES; ++pass) {
			const uint32_t w0 = rl_raw_word(blockIdx.x, pass);          // (< Wp: the raw pitch is a multiple of 32 words)
			// (k unrolled: src[k] stays a register, not an indexed array in scratch memory)
#pragma unroll
			for (uint32_t k = 0; k < 4; ++k) {
				uint4 x = make_uint4(0, 0, 0, 0), m = make_uint4(0, 0, 0, 0);
				if (src[k]) x = *reinterpret_cast<const uint4*>(src[k] + w0);
				if (msrc[k]) m = *reinterpret_cast<const uint4*>(msrc[k] + w0);
				const uint32_t valid = src[k] ? 1u : 0u;
				unsigned long long mine_h = 0, mine_q = 0, mine_v = 0;
				// sample i of the pass: the ballot over the wave's 64 positions is its 64 bits of this group, kept by lane i
				auto sample = [&](uint32_t word, uint32_t mword, uint32_t i0) {
#pragma unroll
					for (uint32_t i = 0; i < 16; ++i) {
						const uint32_t het = rl_het(word, i), hom = rl_hom(word, i), miss = rl_miss(mword, i);
						const unsigned long long bh = __ballot(valid & rl_plane_bit(RL_PLANE_H, P, het, hom, miss));
						const unsigned long long bq = __ballot(valid & rl_plane_bit(RL_PLANE_Q, P, het, hom, miss));
						if (lane == i0 + i) { mine_h = bh; mine_q = bq; }
						if (masked) {      // (uniform)
							const unsigned long long bv = __ballot(valid & rl_plane_bit(RL_PLANE_V, P, het, hom, miss));
							if (lane == i0 + i) mine_v = bv;
						}
					}
				};
				sample(x.x, m.x, 0); sample(x.y, m.y, 16); sample(x.z, m.z, 32); sample(x.w, m.w, 48);
				const uint32_t g = rl_group(wave, k);
				stage[rl_stage(lane, RL_PLANE_H, P, 2 * g)] = (uint32_t)mine_h; stage[rl_stage(lane, RL_PLANE_H, P, 2 * g + 1)] = (uint32_t)(mine_h >> 32);
				stage[rl_stage(lane, RL_PLANE_Q, P, 2 * g)] = (uint32_t)mine_q; stage[rl_stage(lane, RL_PLANE_Q, P, 2 * g + 1)] = (uint32_t)(mine_q >> 32);
				if (masked) { stage[rl_stage(lane, RL_PLANE_V, P, 2 * g)] = (uint32_t)mine_v; stage[rl_stage(lane, RL_PLANE_V, P, 2 * g + 1)] = (uint32_t)(mine_v >> 32); }
			}
			__syncthreads();
			for (uint32_t item = tid; item < rl_out_items(P); item += RL_THREADS) {
				const uint32_t r = item >> 5, word = item & 31u, i = r / P, plane = r - i * P;
				const uint32_t s = rl_pass_sample(blockIdx.x, pass, i);
				if (s < n_samples) rows[rl_out_index(s, plane, P, W, chunk, word)] = stage[rl_stage(i, plane, P, word)];
			}
			__syncthreads();
		}
	}
}

// One super-tile's epilogue.  Samples are absolute; a / b below are relative to the super-tile.
struct RelateArgs {
	const uint32_t* C; uint32_t ldc;          // the super-tile's count matrix: row a * P + pa, column b * P + pb
	uint32_t P, n_use;
	const uint32_t* rowpop;                   // popcounts of the plane rows (two-plane form: the margins)
	uint32_t sa, na, sb, nb;                  // the super-tile: samples [sa, sa + na) x [sb, sb + nb)
	uint32_t out_a0, out_b0, out_ld;          // the call's first row and column sample; entries per row of out / counts
	int32_t diag;                             // a super-tile on the diagonal of a square call: sa == sb, only b >= a
	int32_t mirror;                           // a square call: the pair also fills (b, a)
	int32_t stat;
	unsigned long long fill_bits;             // the caller's fill, as its 64 bits
	unsigned long long* out;                  // [.. x out_ld] doubles as bits, or null
	RelCounts* counts;                        // [.. x out_ld], or null
};

__device__ __forceinline__ RelCounts d_relate_counts(const RelateArgs& g, uint32_t a, uint32_t b) {
	int64_t p[3][3];
	const bool diag = g.diag != 0;
	if (g.P == 3) {
#pragma unroll
		for (uint32_t i = 0; i < 3; ++i)
#pragma unroll
			for (uint32_t j = 0; j < 3; ++j) p[i][j] = g.C[rl_c_index(a, i, b, j, 3, g.ldc, diag)];
	} else {
#pragma unroll
		for (uint32_t i = 0; i < 2; ++i)
#pragma unroll
			for (uint32_t j = 0; j < 2; ++j) p[i][j] = g.C[rl_c_index(a, i, b, j, 2, g.ldc, diag)];
		const uint64_t ra = rl_row(g.sa + a, 0, 2), rb = rl_row(g.sb + b, 0, 2);
		p[0][2] = g.rowpop[ra]; p[1][2] = g.rowpop[ra + 1];
		p[2][0] = g.rowpop[rb]; p[2][1] = g.rowpop[rb + 1];
		p[2][2] = g.n_use;
	}
	return rl_counts(p);
}

__device__ __forceinline__ unsigned long long d_relate_stat(const RelateArgs& g, const RelCounts& c) {
	int64_t num, den;
	rl_fraction(g.stat, c, num, den);
	if (den == 0) return g.fill_bits;
	return (unsigned long long)__double_as_longlong((double)num / (double)den);
}

__global__ __launch_bounds__(RL_THREADS)
void k_relate_epilogue(const RelateArgs* __restrict__ args) {
	__shared__ unsigned long long s_val[RL_EP * RL_EP_PITCH];
	__shared__ uint32_t s_cnt[6][RL_EP * RL_EP_PITCH];
	const RelateArgs g = *args;
	const bool diag = g.diag != 0;
	if (diag && blockIdx.x < blockIdx.y) return;          // wholly below the diagonal (uniform over the block)
	const uint32_t tid = threadIdx.x;
	const uint32_t a0 = blockIdx.y * RL_EP, b0 = blockIdx.x * RL_EP;
#pragma unroll 1
	for (uint32_t k = 0; k < RL_EP_STEPS; ++k) {
		const uint32_t r = rl_ep_row(tid, k), cl = rl_ep_col(tid);
		const uint32_t a = a0 + r, b = b0 + cl;
		if (!rl_ep_live(a, b, g.na, g.nb, diag)) continue;
		const RelCounts c = d_relate_counts(g, a, b);
		const unsigned long long v = d_relate_stat(g, c);
		const size_t at = (size_t)(g.sa + a - g.out_a0) * g.out_ld + (g.sb + b - g.out_b0);
		if (g.out) g.out[at] = v;
		if (g.counts) g.counts[at] = c;
		if (g.mirror) {
			const uint32_t st = rl_ep_stage(r, cl);
			s_val[st] = v;
			s_cnt[0][st] = c.n; s_cnt[1][st] = c.ibs0; s_cnt[2][st] = c.ibs2; s_cnt[3][st] = c.hethet; s_cnt[4][st] = c.het_a; s_cnt[5][st] = c.het_b;
		}
	}
	if (!g.mirror) return;                                  // (uniform over the block)
	__syncthreads();
#pragma unroll 1
	for (uint32_t k = 0; k < RL_EP_STEPS; ++k) {
		const uint32_t r = rl_ep_col(tid), cl = rl_ep_row(tid, k);      // the staged pair this lane mirrors: consecutive lanes, consecutive rows a
		const uint32_t a = a0 + r, b = b0 + cl;
		if (!rl_ep_mirrored(a, b, g.na, g.nb, diag)) continue;
		const uint32_t st = rl_ep_stage(r, cl);
		const size_t at = (size_t)(g.sb + b - g.out_b0) * g.out_ld + (g.sa + a - g.out_a0);
		if (g.out) g.out[at] = s_val[st];
		if (g.counts) {
			RelCounts c;
			c.n = s_cnt[0][st]; c.ibs0 = s_cnt[1][st]; c.ibs2 = s_cnt[2][st]; c.hethet = s_cnt[3][st]; c.het_a = s_cnt[5][st]; c.het_b = s_cnt[4][st];
			g.counts[at] = c;
		}
	}
}

}  // namespace twk
