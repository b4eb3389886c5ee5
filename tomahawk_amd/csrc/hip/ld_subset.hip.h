// Sample subsets (twk_hip_select_samples): the raw rows of the source compacted to the kept samples - a bit gather over M x N genotype
// fields, read once, written once.  The table, the compress and the split by output words are ld_subset_index.h's, played on the host
// by `make subset-check`.
//
// A block owns SUBSET_CHUNK output words of SUBSET_ROWS rows (grid x: the chunk, y: groups of rows, strided, z: data rows / mask rows -
// the mask goes through the same table).  A lane takes an entry of the chunk - 32 bytes from a table every block of the launch shares,
// which stays in L2 - loads that source word of its eight rows (consecutive lanes read consecutive kept words: whole lines where the
// list is dense, a word a line where it is sparse, and then nothing in between), compresses each and ORs the piece into the row's window
// in LDS.  The window goes out in plain coalesced stores: no global atomics, every output word written by one block, the padding as
// zeros, the same bytes on every run.
#pragma once
#include <hip/hip_runtime.h>
#include "ld_subset_index.h"

namespace twk {

struct SubsetArgs {
	const uint32_t* src[2];          // source rows: data, mask (mask: null when n_planes == 1)
	uint32_t* dst[2];                // output rows
	const SubsetEntry* table;
	const SubsetChunk* chunks;
	uint32_t w_src, w_dst;           // row pitches in words
	uint32_t n_rows;
};

__global__ __launch_bounds__(256) void k_subset_rows(const SubsetArgs a) {
	__shared__ uint32_t win[SUBSET_ROWS][SUBSET_CHUNK];
	const uint32_t tid = threadIdx.x;
	const uint32_t j0 = blockIdx.x * SUBSET_CHUNK;
	const uint32_t n_words = a.w_dst - j0 < SUBSET_CHUNK ? a.w_dst - j0 : SUBSET_CHUNK;
	const SubsetChunk ch = a.chunks[blockIdx.x];
	const uint32_t* __restrict__ src = a.src[blockIdx.z];
	uint32_t* __restrict__ dst = a.dst[blockIdx.z];
	for (uint32_t v0 = blockIdx.y * SUBSET_ROWS; v0 < a.n_rows; v0 += gridDim.y * SUBSET_ROWS) {
#pragma unroll
		for (uint32_t r = 0; r < SUBSET_ROWS; ++r) win[r][tid] = 0;
		__syncthreads();
		for (uint32_t e = ch.e_begin + tid; e < ch.e_end; e += 256) {
			const SubsetEntry d = a.table[e];
			uint32_t x[SUBSET_ROWS];
#pragma unroll
			for (uint32_t r = 0; r < SUBSET_ROWS; ++r) x[r] = v0 + r < a.n_rows ? src[(size_t)(v0 + r) * a.w_src + d.src_word] : 0u;
#pragma unroll
			for (uint32_t r = 0; r < SUBSET_ROWS; ++r) {
				uint32_t* row = win[r];
				subset_scatter(subset_compress(x[r], d), d.out_bit, j0, n_words, [row](uint32_t w, uint32_t bits) { atomicOr(&row[w], bits); });
			}
		}
		__syncthreads();
		if (tid < n_words) {
#pragma unroll
			for (uint32_t r = 0; r < SUBSET_ROWS; ++r)
				if (v0 + r < a.n_rows) dst[(size_t)(v0 + r) * a.w_dst + j0 + tid] = win[r][tid];
		}
		__syncthreads();
	}
}

}  // namespace twk
