// LD pruning: the epilogue of a count matrix that ballots instead of appending, and the greedy walk behind it (twk_hip_ld_prune,
// include/twk_hip.h).
//
// Over a triangle of n variants [a0, a0 + n) in file order a pair (u, v), u < v, is an EDGE if `calc` would report a record for it.
// Walking v upwards, v is KEPT iff no kept u < v has an edge (u, v) (PLINK's --indep-pairwise, greedy in file order).  A prune launch
// runs the count kernel into C like a record launch and then
//   k_ld_prune_mask  one pair per lane through d_pair<SRC_MATRIX> (ld_math.hip.h) with the launch's StatsParams - the pair rules, the
//                    regrouped sets' ids, auto_select, window, option bits are the record path's own code - and only `keep` is used.
//                    A block is 256 lanes = 256 columns and walks PRUNE_ROWS rows.  On a plain plane set (ids == null) a wave's 64
//                    columns are 64 consecutive variants: lane 0 ORs the wave's ballot, shifted, into the one or two words of the
//                    row's bitmap it straddles (nothing when the ballot is 0).  On a regrouped set (default mode with missing
//                    data) columns are not consecutive: every keeping lane ORs its own bit at (min, max) of the file-order ids.
//                    atomicOr on 64-bit words: tiles of different launches share words, and OR has no order - two runs set the
//                    same bits.  Edges are counted per wave (popcount of the ballots, one 64-bit atomic add a wave: an integer).
//   k_ld_prune_walk  one block, behind the call's last launch on the same stream.  `removed` (one bit per variant) lives in LDS
//                    (up to 520,192 variants; beyond that in global memory) and every lane OWNS the words w = lane (mod block size):
//                    no two lanes write one word, nothing is reduced.  The walk goes word by word, 64 variants at a time: the
//                    64 x 64 diagonal block of the adjacency is staged in LDS and every lane resolves it for itself (which of the
//                    64 are kept is a sequential question, but one of 64 LDS reads); then every lane ORs the rows of the kept
//                    ones into the words it owns beyond the diagonal - independent loads, all in flight at once.  Forward OR:
//                    only a kept variant costs a row pass; a dropped one costs nothing.  Two barriers per 64 variants.
// The adjacency bitmap: row u - a0, bit v - a0, only v > u is ever set; the row stride is ceil(n / 64) words, so the bitmap takes
// n * ceil(n / 64) * 8 bytes (0.31 GB at 50 k variants, 35 GB at 531,500) whatever the window: a banded layout for windowed runs is
// not done.  It is zeroed once per call.  No Fisher test (minP >= 1), no survivor buffer, no sort; one byte per variant leaves the
// device.  There is no reference counterpart.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ld_math.hip.h"
#include "ld_reduce.hip.h"

namespace twk {

constexpr int PRUNE_THREADS = 256;      // columns of a mask block
constexpr int PRUNE_ROWS = 32;          // rows of a mask block
constexpr int WALK_THREADS = 1024;
constexpr uint32_t WALK_LDS_WORDS = 8192 - 64;      // `removed` in LDS: 64 KB less the diagonal block's share - up to 520,192 variants

struct PruneMap {
	unsigned long long* adj;            // [n][stride]
	unsigned long long* n_edges;
	uint32_t a0, n, stride;             // the triangle's first variant, its size, words per row
};
struct PruneArgs : ReduceParams<PruneMap> {};

__global__ __launch_bounds__(PRUNE_THREADS)
void k_ld_prune_mask(const PruneArgs* __restrict__ args) {
	const PruneMap pm = args->m;
	const uint32_t nA = args->p.nA, nB = args->p.nB;
	const uint32_t a0 = args->p.tv.a0, b0 = args->p.tv.b0;
	const uint32_t* ids = args->p.tv.ids;
	const uint32_t j = blockIdx.x * PRUNE_THREADS + threadIdx.x;
	const uint32_t i0 = blockIdx.y * PRUNE_ROWS;
	const int lane = threadIdx.x & 63;
	if (d_block_dead(args->p, blockIdx.x, PRUNE_THREADS, i0)) return;
	// the wave's first column as a bit of the bitmap (plain sets: its 64 columns are the bits from there on)
	const uint32_t bit0 = b0 + (j - lane) - pm.a0;
	uint32_t edges = 0;
#pragma unroll 1
	for (uint32_t r = 0; r < PRUNE_ROWS; ++r) {
		const uint32_t i = i0 + r;
		bool keep = false;
		if (i < nA && j < nB) keep = d_reduce_keeps(&args->p, i, j);
		const unsigned long long ballot = __ballot(keep);
		if (!ballot) continue;                               // (uniform over the wave)
		edges += (uint32_t)__popcll(ballot);
		if (!ids) {
			// keep implies column variant > row variant (a triangle's launches lie on or above its diagonal) and both inside it
			const uint32_t row = a0 + i - pm.a0;
			if (lane == 0 && row < pm.n) d_or_bits(pm.adj + (size_t)row * pm.stride, pm.stride, bit0, ballot);
		} else if (keep) {
			uint32_t u = ids[a0 + i] - pm.a0, v = ids[b0 + j] - pm.a0;
			if (u > v) { const uint32_t x = u; u = v; v = x; }
			if (v < pm.n) atomicOr(pm.adj + (size_t)u * pm.stride + (v >> 6), 1ull << (v & 63));
		}
	}
	if (lane == 0 && edges) atomicAdd(pm.n_edges, (unsigned long long)edges);
}

// The greedy walk over the finished bitmap.  keep: [n_variants] bytes, zeroed by the caller; out[0] = variants kept.
// g_removed: the `removed` words when they do not fit LDS (IN_LDS false), zeroed by the caller.
template <bool IN_LDS>
__global__ __launch_bounds__(WALK_THREADS)
void k_ld_prune_walk(const unsigned long long* __restrict__ adj, uint32_t a0, uint32_t n, uint32_t stride, unsigned long long* g_removed,
                     uint8_t* __restrict__ keep, unsigned long long* __restrict__ out) {
	__shared__ unsigned long long lds_removed[IN_LDS ? WALK_LDS_WORDS : 1];
	__shared__ unsigned long long diag[64];
	unsigned long long* removed = IN_LDS ? lds_removed : g_removed;
	const uint32_t tid = threadIdx.x;
	if (IN_LDS) for (uint32_t w = tid; w < stride; w += WALK_THREADS) removed[w] = 0;
	unsigned long long n_kept = 0;
	for (uint32_t wi = 0; wi < stride; ++wi) {
		const uint32_t v0 = wi * 64, live = n - v0 < 64 ? n - v0 : 64;      // variants of this word
		__syncthreads();                                     // the owners' writes of the words before are done (and diag is free)
		if (tid < live) diag[tid] = adj[(size_t)(v0 + tid) * stride + wi];
		__syncthreads();
		// which of the 64 are kept: the same answer in every lane
		unsigned long long gone = removed[wi], km = 0;
		if (live < 64) gone |= ~0ull << live;
		for (uint32_t b = 0; b < live; ++b) {
			if (gone >> b & 1) continue;
			km |= 1ull << b;
			gone |= diag[b];
		}
		if (tid < live) keep[a0 + v0 + tid] = (uint8_t)(km >> tid & 1);
		n_kept += (unsigned long long)__popcll(km);
		if (!km) continue;
		// forward OR of the kept variants' rows into the words this lane owns (w = tid mod WALK_THREADS) beyond the diagonal
		uint32_t w = wi + 1 + (tid + WALK_THREADS - (wi + 1) % WALK_THREADS) % WALK_THREADS;
		for (; w < stride; w += WALK_THREADS) {
			unsigned long long acc = removed[w];
			for (unsigned long long m = km; m; m &= m - 1) acc |= adj[(size_t)(v0 + (uint32_t)__ffsll((long long)m) - 1) * stride + w];
			removed[w] = acc;
		}
	}
	if (tid == 0) out[0] = n_kept;
}

}  // namespace twk
