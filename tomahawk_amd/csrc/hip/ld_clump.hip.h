// LD clumping: the mask epilogue with a symmetric fill, and the walk in P order behind it (twk_hip_ld_clump, include/twk_hip.h).
//
// Over a triangle of n variants [a0, a0 + n) in file order {u, v} is an EDGE if `calc` would report a record with those two - prune's
// edge (ld_prune.hip.h), seen from both ends.  Given one P value per variant and 0 <= p1 <= p2 <= 1, the variants with a P value are
// visited in ascending P (ties in file order) up to p1; a visited variant that belongs to no clump yet becomes an INDEX variant and
// claims every variant with P <= p2 that has an edge to it and belongs to no clump yet (PLINK's --clump).  A clump launch runs the
// count kernel into C like a record launch and then
//   k_ld_clump_mask  k_ld_prune_mask's shape - one pair per lane through d_pair<SRC_MATRIX>, out of line, the parameter block in device
//                    memory - over CLUMP_ROWS = 64 rows, and both bits of an edge.  On a plain plane set lane 0 ORs the wave's ballot
//                    into the row's word(s) as prune does, and every lane also gathers `keep` of its own column over the block's 64
//                    rows into one word: the bits [a0 + i0, a0 + i0 + 64) of the bitmap row of ITS column's variant - the transpose of
//                    the block for one shift-OR per pair.  After the loop a lane ORs that word, shifted, into the one or two words it
//                    straddles (nothing when it is 0): at most two atomics per lane and 64 rows, and no second pass over the bitmap.
//                    On a regrouped set every keeping lane ORs its two bits (u, v) and (v, u) of the file-order ids.  atomicOr on
//                    64-bit words: tiles of different launches share words in both directions, and OR has no order.  Edges are
//                    counted once per pair from the ballots.  Every write is guarded against the slice (row < n, word < stride).
//   k_ld_clump_walk  one block, behind the call's last launch on the same stream.  `taken` (one bit per variant: in a clump, or not
//                    eligible) lives in LDS up to the size prune's `removed` allows, beyond that in global memory, and every lane OWNS
//                    the words w = lane (mod block size).  It starts as the host's `taken0` (bit v set where P[v] is NaN or > p2).
//                    The candidates (P <= p1, in visiting order: the host's stable sort) are read 64 at a time, one per lane, and
//                    passed round the wave.  Per candidate u every lane reads u's bit of `taken`:
//                      set    u was claimed: skipped, without a barrier;
//                      clear  u is an index variant: barrier A; every lane takes new = adj[u][w] & ~taken[w] over its own words,
//                             ORs it into taken[w] and stores index_of = u for the bits of new; the owner of u's word sets u's bit
//                             and index_of[u] = u; barrier B.
//                    WHY EVERY LANE DECIDES ALIKE.  `taken` is written only between a barrier A and the barrier B behind it.  A lane
//                    passes A only when all 1024 have arrived there, and a lane arrives at A only after it has read the bits of every
//                    candidate up to and including the index variant - so nobody writes while anybody still has a bit to read that
//                    was to be decided on the state before A.  A lane passes B only when all writes of that index variant are done,
//                    so every read behind B sees them all.  Between B and the next A nothing is written: however far ahead a lane
//                    runs through skipped candidates, it reads the state every other lane will read.  All lanes therefore reach the
//                    same decision for every candidate, and the barriers match up: two per index variant, none per skipped one.
//                    Counts without atomics: a lane sums popc(new), one block reduction at the end; every lane counts the index
//                    variants (the same number in each) and thread 0 writes it.
// The bitmap is prune's: row u - a0, bit v - a0, row stride ceil(n / 64) words, n * ceil(n / 64) * 8 bytes, zeroed once per call - the
// lower triangle prune leaves empty holds the mirrored bits.  No Fisher test (minP >= 1), no survivor buffer, no sort; four bytes per
// variant leave the device.  There is no reference counterpart.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ld_math.hip.h"
#include "ld_prune.hip.h"

namespace twk {

constexpr int CLUMP_THREADS = 256;      // columns of a mask block
constexpr int CLUMP_ROWS = 64;          // rows of a mask block: one word of a column's mirrored bits
constexpr int CLUMP_WALK_THREADS = 1024;
constexpr uint32_t CLUMP_LDS_WORDS = WALK_LDS_WORDS;      // `taken` in LDS: up to 520,192 variants, as prune's `removed`
constexpr uint32_t CLUMP_NONE = 0xFFFFFFFFu;              // TWK_HIP_NO_CLUMP

struct ClumpArgs : ReduceParams<PruneMap> {};      // (the map is prune's)

__global__ __launch_bounds__(CLUMP_THREADS)
void k_ld_clump_mask(const ClumpArgs* __restrict__ args) {
	const PruneMap pm = args->m;
	const uint32_t nA = args->p.nA, nB = args->p.nB;
	const uint32_t a0 = args->p.tv.a0, b0 = args->p.tv.b0;
	const uint32_t* ids = args->p.tv.ids;
	const uint32_t j = blockIdx.x * CLUMP_THREADS + threadIdx.x;
	const uint32_t i0 = blockIdx.y * CLUMP_ROWS;
	const int lane = threadIdx.x & 63;
	if (d_block_dead(args->p, blockIdx.x, CLUMP_THREADS, i0)) return;
	// the wave's first column as a bit of the bitmap (plain sets: its 64 columns are the bits from there on)
	const uint32_t bit0 = b0 + (j - lane) - pm.a0;
	uint32_t edges = 0;
	unsigned long long col = 0;                              // keep of this lane's column over the block's rows: bit r = row i0 + r
#pragma unroll 1
	for (uint32_t r = 0; r < CLUMP_ROWS; ++r) {
		const uint32_t i = i0 + r;
		bool keep = false;
		if (i < nA && j < nB) keep = d_reduce_keeps(&args->p, i, j);
		const unsigned long long ballot = __ballot(keep);
		if (!ballot) continue;                               // (uniform over the wave)
		edges += (uint32_t)__popcll(ballot);
		if (!ids) {
			// keep implies both variants inside the triangle (its launches lie on or above its diagonal)
			col |= (unsigned long long)keep << r;
			const uint32_t row = a0 + i - pm.a0;
			if (lane == 0 && row < pm.n) d_or_bits(pm.adj + (size_t)row * pm.stride, pm.stride, bit0, ballot);
		} else if (keep) {
			const uint32_t u = ids[a0 + i] - pm.a0, v = ids[b0 + j] - pm.a0;
			if (u < pm.n && v < pm.n) {
				atomicOr(pm.adj + (size_t)u * pm.stride + (v >> 6), 1ull << (v & 63));
				atomicOr(pm.adj + (size_t)v * pm.stride + (u >> 6), 1ull << (u & 63));
			}
		}
	}
	// the mirrored bits: the column's variant is the bitmap row, the block's rows are its bits from a0 + i0 on
	if (col) {
		const uint32_t row = b0 + j - pm.a0;
		if (row < pm.n) d_or_bits(pm.adj + (size_t)row * pm.stride, pm.stride, a0 + i0 - pm.a0, col);
	}
	if (lane == 0 && edges) atomicAdd(pm.n_edges, (unsigned long long)edges);
}

// The walk in P order over the finished bitmap.  order[0 .. m): the candidates as offsets into the slice, in visiting order.  taken0:
// [stride] words, bit v set where slice variant v is not eligible; with IN_LDS false it is the walk's `taken` itself and is written.
// index_of: [n_variants], TWK_HIP_NO_CLUMP everywhere (the caller's fill).  out[0] = index variants, out[1] = claimed members.
template <bool IN_LDS>
__global__ __launch_bounds__(CLUMP_WALK_THREADS)
void k_ld_clump_walk(const unsigned long long* __restrict__ adj, uint32_t a0, uint32_t n, uint32_t stride, const uint32_t* __restrict__ order, uint32_t m,
                     unsigned long long* taken0, uint32_t* __restrict__ index_of, unsigned long long* __restrict__ out) {
	__shared__ unsigned long long lds_taken[IN_LDS ? CLUMP_LDS_WORDS : 1];
	__shared__ unsigned long long part[CLUMP_WALK_THREADS / 64];
	unsigned long long* taken = IN_LDS ? lds_taken : taken0;
	const uint32_t tid = threadIdx.x;
	const int lane = tid & 63;
	if (IN_LDS) for (uint32_t w = tid; w < stride; w += CLUMP_WALK_THREADS) taken[w] = taken0[w];
	__syncthreads();
	unsigned long long n_index = 0, n_claimed = 0;
	for (uint32_t base = 0; base < m; base += 64) {
		// 64 candidates, one per lane (every wave reads the same 64), passed round the wave below
		const uint32_t mine = base + lane < m ? order[base + lane] : 0;
		const uint32_t cnt = m - base < 64 ? m - base : 64;
		for (uint32_t k = 0; k < cnt; ++k) {
			const uint32_t u = (uint32_t)__shfl((int)mine, (int)k);
			if (u >= n) continue;                                // (the host sends none: a bound, not a case)
			if (taken[u >> 6] >> (u & 63) & 1) continue;         // claimed before its turn: the same answer in every lane (see above)
			++n_index;
			__syncthreads();                                     // A: every lane has read what it decides by
			const unsigned long long* row = adj + (size_t)u * stride;
			for (uint32_t w = tid; w < stride; w += CLUMP_WALK_THREADS) {
				unsigned long long t = taken[w];
				unsigned long long fresh = row[w] & ~t;
				if (w == u >> 6) { fresh &= ~(1ull << (u & 63)); t |= 1ull << (u & 63); index_of[a0 + u] = a0 + u; }
				if (w == u >> 6 || fresh) taken[w] = t | fresh;
				n_claimed += (unsigned long long)__popcll(fresh);
				for (; fresh; fresh &= fresh - 1) index_of[a0 + w * 64 + (uint32_t)__ffsll((long long)fresh) - 1] = a0 + u;
			}
			__syncthreads();                                     // B: its writes are done
		}
	}
	// the members: lanes -> waves -> thread 0
	for (int d = 32; d; d >>= 1) n_claimed += __shfl_down(n_claimed, d);
	if (lane == 0) part[tid >> 6] = n_claimed;
	__syncthreads();
	if (tid == 0) {
		unsigned long long s = 0;
		for (int k = 0; k < CLUMP_WALK_THREADS / 64; ++k) s += part[k];
		out[0] = n_index; out[1] = s;
	}
}

}  // namespace twk
