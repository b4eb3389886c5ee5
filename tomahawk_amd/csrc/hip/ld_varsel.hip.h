// Variant subsets (twk_hip_select_variants): which variants of the base pass a list and the MAF / MAC / missingness / HWE thresholds,
// decided on the device from the raw rows, and the rows and the metadata of those that do, gathered into a working set of their own.
// The predicate, the counts of a word and the gather's walk are ld_varsel_index.h's, played on the host by `make varsel-check`.
//
//   k_varsel_list_flags  listed[list[i]] = 1                               (plain stores into a zeroed array; the list is strictly ascending)
//   k_varsel_predicate   one wave per base variant: het / hom / missing samples from its raw row (and mask row) in one pass of 16-byte
//                        loads - the numbers twk_hip_get_marginals returns - then lane 0 applies the list flag, d_hwe and the thresholds
//   (rocprim::exclusive_scan of the flags: the position of every kept variant in the working set)
//   k_varsel_map         map[offset[v]] = v for the kept: working -> base, ascending, so file order is preserved; the count
//   k_varsel_rows        the row gather: data rows and mask rows (blockIdx.z) through the map, 16 bytes a lane, consecutive lanes on
//                        consecutive pieces of a row, so a wave reads and writes whole 128-byte lines; the padding rows as zeros; every
//                        output piece written once by a plain store: two calls give the same bytes
//   k_varsel_meta        the metadata SoA through the map, zeros behind the last kept variant
// No atomics anywhere but inside rocprim's scan.
#pragma once
#include <hip/hip_runtime.h>
#include "ld_varsel_index.h"

namespace twk {

__global__ void k_varsel_list_flags(const uint32_t* __restrict__ list, uint32_t n_list, uint32_t* __restrict__ listed) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n_list) listed[list[i]] = 1u;
}

struct VarselPredArgs {
	const uint32_t* raw;             // [n_variants][Wp]
	const uint32_t* rawmask;         // or null: no variant of the base has missing data
	const uint32_t* listed;          // or null: no list test
	const double* hwe;
	uint32_t* flag;                  // [n_variants] -> 1 kept, 0 not
	uint32_t Wp, n_variants, n_samples;
	uint32_t exclude;                // the list names the variants to drop
	VarselFilter f;
};

__global__ __launch_bounds__(256) void k_varsel_predicate(const VarselPredArgs a) {
	const uint32_t v = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
	if (v >= a.n_variants) return;
	const uint32_t lane = threadIdx.x & 63;
	const uint4* __restrict__ x = reinterpret_cast<const uint4*>(a.raw + (size_t)v * a.Wp);
	const uint4* __restrict__ m = a.rawmask ? reinterpret_cast<const uint4*>(a.rawmask + (size_t)v * a.Wp) : nullptr;
	uint32_t het = 0, hom = 0, miss = 0;
	for (uint32_t k = lane; k < a.Wp / 4; k += 64) {
		const uint4 xv = x[k];
		const uint4 mv = m ? m[k] : make_uint4(0, 0, 0, 0);
		varsel_word_counts(xv.x, mv.x, het, hom, miss);
		varsel_word_counts(xv.y, mv.y, het, hom, miss);
		varsel_word_counts(xv.z, mv.z, het, hom, miss);
		varsel_word_counts(xv.w, mv.w, het, hom, miss);
	}
	for (int o = 32; o > 0; o >>= 1) { het += __shfl_xor(het, o); hom += __shfl_xor(hom, o); miss += __shfl_xor(miss, o); }
	if (lane == 0) {
		bool keep = varsel_pass(a.n_samples, het, hom, miss, a.hwe[v], a.f);
		if (a.listed) keep = keep && ((a.listed[v] != 0u) != (a.exclude != 0u));
		a.flag[v] = keep ? 1u : 0u;
	}
}

__global__ void k_varsel_map(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ offset, uint32_t n_variants,
                             uint32_t* __restrict__ map, uint32_t* __restrict__ n_kept) {
	const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
	if (v >= n_variants) return;
	if (flag[v]) map[offset[v]] = v;
	if (v == n_variants - 1) *n_kept = offset[v] + flag[v];
}

struct VarselRowArgs {
	const uint32_t* src[2];          // base rows: data, mask (mask: unused when the grid has one plane)
	uint32_t* dst[2];                // working rows
	const uint32_t* map;             // [n_kept] working -> base
	VarselGather g;
};

__global__ __launch_bounds__(VARSEL_BLOCK) void k_varsel_rows(const VarselRowArgs a) {
	const uint4* __restrict__ src = reinterpret_cast<const uint4*>(a.src[blockIdx.z]);
	uint4* __restrict__ dst = reinterpret_cast<uint4*>(a.dst[blockIdx.z]);
	const uint32_t w4 = a.g.w4;
	varsel_gather_lane(a.g, blockIdx.x, threadIdx.x, a.map, make_uint4(0, 0, 0, 0),
	                   [src, w4](uint32_t row, uint32_t col) { return src[(size_t)row * w4 + col]; },
	                   [dst, w4](uint32_t row, uint32_t col, const uint4& x) { dst[(size_t)row * w4 + col] = x; });
}

struct VarselMetaArgs {
	const uint32_t* src32[5];        // ac, an, pos, rid, missing of the base
	uint32_t* dst32[5];
	const double* src_hwe;
	double* dst_hwe;
	const uint32_t* map;
	uint32_t n_kept, n_out;          // n_out: the working set's M_alloc
};

__global__ void k_varsel_meta(const VarselMetaArgs a) {
	const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= a.n_out) return;
	const bool live = r < a.n_kept;
	const uint32_t v = live ? a.map[r] : 0u;
#pragma unroll
	for (int k = 0; k < 5; ++k) a.dst32[k][r] = live ? a.src32[k][v] : 0u;
	a.dst_hwe[r] = live ? a.src_hwe[v] : 0.0;
}

}  // namespace twk
