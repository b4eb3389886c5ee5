// Sample relationship: where a bit of the transposed plane set lands, what a lane of the transposition and of the epilogue touches, and how
// the six counts and the statistic of a sample pair follow from plane products (twk_hip_relationship, include/twk_hip.h).  Plain C++ with no
// HIP in it: ld_relate.hip.h includes it, the engine's host code includes it, and so does csrc/tools/relate_index_check.cpp
// (`make relate-check`), which plays the transposition lane by lane against a naive one and the count formulas against counted genotypes.
// The count launches behind the transposition are not this file's: their tiles, units and the rule for a row's last K chunk are
// ld_count_table.h's (build_count_table, count_last_halves), whose chunk and tile RL_KC and RL_TILE name.
//
// The plane set is sample-major: P rows a sample, one bit per variant IN USE, in the order of the call's variant list.
//   P = 2 (no variant in use has missing genotypes): H (heterozygous), Q (homozygous ALT);
//   P = 3 (some has):                                H & V, Q & V, V (the genotype is not missing).
// Row of (sample s, plane p) = s * P + p; position k of the list is bit k & 31 of word k >> 5 of the row.  A row is rl_words(L) words -
// the list's ceil(L / 32) words padded with zeros to a multiple of 32 words (the count kernel's K chunk, KC) - and the set has
// rl_rows_alloc(N, P) rows: the N * P live ones padded with zero rows to a multiple of 128 (the count kernel's tile), plus one tile
// more, because a super-tile may begin at any sample and its last tile then overhangs.
//
// The transposition (k_relate_transpose): a block of 256 lanes takes RL_CHUNK = 1024 positions of the list - 32 words = one 128-byte
// line of every output row - times RL_BLOCK_SAMPLES = 256 samples - 16 words = 64 bytes of every raw row - in RL_PASSES = 4 passes of 64
// samples.  In a pass lane l of wave w holds, for k = 0 .. 3, the 16 bytes (64 samples) of the raw row of position
// rl_position(chunk, w, k, l); the ballot over "sample i of the pass is heterozygous" is the 64 output bits [g * 64, g * 64 + 64) of
// sample i's H row, g = rl_group(w, k), and lane i keeps it; lane i then stages its two words per plane at rl_stage(i, p, P, 2 g + {0, 1})
// and after a barrier the block writes the staged rows out, 32 consecutive lanes one whole 128-byte line.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "ld_count_table.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TWK_RL_FN __host__ __device__ inline
#else
#define TWK_RL_FN inline
#endif

namespace twk {

constexpr uint32_t RL_KC = KC;                       // words of a K chunk of the count kernel
constexpr uint32_t RL_TILE = TILE;                   // rows of a tile of the count kernel
constexpr uint32_t RL_THREADS = 256;                 // lanes of a transposition block: 4 waves
constexpr uint32_t RL_CHUNK = 1024;                  // list positions a block takes: RL_KC words of every output row
constexpr uint32_t RL_PASS_SAMPLES = 64;             // samples of a pass: 4 raw words (16 samples a word), one 16-byte load a lane
constexpr uint32_t RL_PASSES = 4;
constexpr uint32_t RL_BLOCK_SAMPLES = RL_PASS_SAMPLES * RL_PASSES;      // 256 samples = 64 bytes of a raw row
constexpr uint32_t RL_BLOCK_WORDS = RL_BLOCK_SAMPLES / 16;              // raw words of a block
constexpr uint32_t RL_GROUPS = RL_CHUNK / 64;        // 64-position groups of a chunk: 4 a wave
constexpr uint32_t RL_STAGE_PITCH = RL_KC + 1;       // words per staged row: 33, so that the 64 lanes of a wave, P * 33 words apart, spread over the banks
constexpr uint32_t RL_STAGE_WORDS = RL_PASS_SAMPLES * 3 * RL_STAGE_PITCH;      // 25,344 bytes of LDS
constexpr uint32_t RL_SUPER_ROWS = 8192;             // plane rows per axis of a super-tile: a count matrix of at most 256 MiB

enum { RL_PLANE_H = 0, RL_PLANE_Q = 1, RL_PLANE_V = 2 };

TWK_RL_FN uint32_t rl_planes(bool any_missing) { return any_missing ? 3u : 2u; }
TWK_RL_FN uint32_t rl_words_live(uint32_t n_use) { return (n_use + 31u) / 32u; }
TWK_RL_FN uint32_t rl_words(uint32_t n_use) { return (rl_words_live(n_use) + RL_KC - 1) / RL_KC * RL_KC; }
TWK_RL_FN uint64_t rl_rows_alloc(uint32_t n_samples, uint32_t P) { return ((uint64_t)n_samples * P + RL_TILE - 1) / RL_TILE * RL_TILE + RL_TILE; }
TWK_RL_FN uint64_t rl_row(uint32_t sample, uint32_t plane, uint32_t P) { return (uint64_t)sample * P + plane; }
TWK_RL_FN uint32_t rl_word(uint32_t position) { return position >> 5; }
TWK_RL_FN uint32_t rl_bit(uint32_t position) { return position & 31u; }
// Samples per axis of a super-tile.
TWK_RL_FN uint32_t rl_super_samples(uint32_t P) { return RL_SUPER_ROWS / P; }

// ---- the raw layout: raw[v * Wp + w] holds the samples 16 w .. 16 w + 15, two bits each (bit 2 i: first allele is ALT, 2 i + 1: second);
// the mask has both bits of a sample set when its genotype is missing
TWK_RL_FN uint32_t rl_het(uint32_t word, uint32_t i) { return ((word >> (2 * i)) ^ (word >> (2 * i + 1))) & 1u; }
TWK_RL_FN uint32_t rl_hom(uint32_t word, uint32_t i) { return (word >> (2 * i)) & (word >> (2 * i + 1)) & 1u; }
TWK_RL_FN uint32_t rl_miss(uint32_t mword, uint32_t i) { return ((mword >> (2 * i)) | (mword >> (2 * i + 1))) & 1u; }
// The bit of plane p for a genotype of a position that exists (positions beyond the list have no bit in any plane).
TWK_RL_FN uint32_t rl_plane_bit(uint32_t plane, uint32_t P, uint32_t het, uint32_t hom, uint32_t miss) {
	const uint32_t ok = P == 3 ? (miss ^ 1u) : 1u;
	return plane == RL_PLANE_H ? (het & ok) : plane == RL_PLANE_Q ? (hom & ok) : ok;
}

// ---- the transposition's lanes
TWK_RL_FN uint32_t rl_group(uint32_t wave, uint32_t k) { return wave + 4u * k; }                       // 64-position group of the chunk that wave `wave` takes in its step k
TWK_RL_FN uint32_t rl_position(uint32_t chunk, uint32_t wave, uint32_t k, uint32_t lane) { return chunk * RL_CHUNK + rl_group(wave, k) * 64u + lane; }
TWK_RL_FN uint32_t rl_raw_word(uint32_t block_x, uint32_t pass) { return block_x * RL_BLOCK_WORDS + pass * 4u; }      // first of the pass's four raw words
TWK_RL_FN uint32_t rl_pass_sample(uint32_t block_x, uint32_t pass, uint32_t i) { return block_x * RL_BLOCK_SAMPLES + pass * RL_PASS_SAMPLES + i; }
TWK_RL_FN uint32_t rl_stage(uint32_t i, uint32_t plane, uint32_t P, uint32_t word) { return (i * P + plane) * RL_STAGE_PITCH + word; }
// the write-out: item x = 0 .. 64 P * 32 - 1 of a pass is word x & 31 of the staged row x >> 5 = (sample i, plane) = ((x >> 5) / P, (x >> 5) % P)
TWK_RL_FN uint32_t rl_out_items(uint32_t P) { return RL_PASS_SAMPLES * P * RL_KC; }
TWK_RL_FN size_t rl_out_index(uint32_t sample, uint32_t plane, uint32_t P, uint32_t W, uint32_t chunk, uint32_t word) {
	return (size_t)rl_row(sample, plane, P) * W + (size_t)chunk * RL_KC + word;
}

// ---- the epilogue: counts and statistic of a sample pair (a, b)
struct RelCounts { uint32_t n, ibs0, ibs2, hethet, het_a, het_b; };      // twk_hip_rel_counts, field for field

// prod[i][j] = popcount(plane i of a & plane j of b), i, j in H, Q, V.  In the two-plane form V is all ones over the list: the caller puts
// the list's length at [V][V] and the rows' popcounts at [H][V], [Q][V] (a's) and [V][H], [V][Q] (b's).  With R = V & ~H & ~Q (homozygous
// REF) every count is a sum of products: 64-bit signed arithmetic, every result fits 32 bits.
TWK_RL_FN RelCounts rl_counts(const int64_t (&p)[3][3]) {
	const int64_t HH = p[0][0], HQ = p[0][1], HV = p[0][2], QH = p[1][0], QQ = p[1][1], QV = p[1][2], VH = p[2][0], VQ = p[2][1], VV = p[2][2];
	const int64_t RQ = VQ - HQ - QQ, QR = QV - QH - QQ;                                   // R_a Q_b, Q_a R_b
	const int64_t RR = VV - VH - VQ - HV + HH + HQ - QV + QH + QQ;                      // (V - H - Q)_a (V - H - Q)_b
	RelCounts c;
	c.n = (uint32_t)VV; c.ibs0 = (uint32_t)(RQ + QR); c.ibs2 = (uint32_t)(RR + HH + QQ);
	c.hethet = (uint32_t)HH; c.het_a = (uint32_t)HV; c.het_b = (uint32_t)VH;
	return c;
}
// Numerator and denominator of a statistic (TWK_HIP_REL_IBS = 0, _IBS0 = 1, _KING = 2), integers formed in 64 bits.  The statistic is
// ONE double division, (double)num / (double)den, and the caller's fill where den == 0.
TWK_RL_FN void rl_fraction(int32_t stat, const RelCounts& c, int64_t& num, int64_t& den) {
	if (stat == 0) { num = (int64_t)c.n + c.ibs2 - c.ibs0; den = 2 * (int64_t)c.n; }
	else if (stat == 1) { num = c.ibs0; den = c.n; }
	else { num = (int64_t)c.hethet - 2 * (int64_t)c.ibs0; den = (int64_t)c.het_a + c.het_b; }
}
TWK_RL_FN bool rl_valid_stat(int32_t stat) { return stat >= 0 && stat <= 2; }

// An epilogue block is 256 lanes over RL_EP x RL_EP = 32 x 32 sample pairs: in step k = 0 .. 3 lane t has row (t >> 5) + 8 k and column
// t & 31 - a wave stores two runs of 32 consecutive entries.  The mirrored entries are staged at rl_ep_stage(row, column) and written out
// with the roles swapped: lane t then reads rl_ep_stage(t & 31, (t >> 5) + 8 k), the pair (row t & 31, column (t >> 5) + 8 k), and stores
// it at (column, row) - again 32 consecutive entries of one output row.
constexpr uint32_t RL_EP = 32;
constexpr uint32_t RL_EP_PITCH = RL_EP + 1;
constexpr uint32_t RL_EP_STEPS = RL_EP * RL_EP / RL_THREADS;
TWK_RL_FN uint32_t rl_ep_row(uint32_t tid, uint32_t k) { return (tid >> 5) + 8u * k; }
TWK_RL_FN uint32_t rl_ep_col(uint32_t tid) { return tid & 31u; }
TWK_RL_FN uint32_t rl_ep_stage(uint32_t row, uint32_t col) { return row * RL_EP_PITCH + col; }
// A pair of the block is computed: inside the super-tile, and on a diagonal super-tile on or above the diagonal.
TWK_RL_FN bool rl_ep_live(uint32_t a, uint32_t b, uint32_t na, uint32_t nb, bool diag) { return a < na && b < nb && (!diag || b >= a); }
// ... and has a mirrored entry: off the diagonal (pairs of a super-tile beyond the diagonal always are).
TWK_RL_FN bool rl_ep_mirrored(uint32_t a, uint32_t b, uint32_t na, uint32_t nb, bool diag) { return a < na && b < nb && (!diag || b > a); }
// Where the product (plane pa of a, plane pb of b) lies in the super-tile's count matrix.  On a diagonal super-tile only the tiles on or
// above the diagonal were contracted; a product of a sample with itself (or, never, with an earlier one) below it is read at its mirror
// image - AND is symmetric.
TWK_RL_FN size_t rl_c_index(uint32_t a, uint32_t pa, uint32_t b, uint32_t pb, uint32_t P, uint32_t ldc, bool diag) {
	uint32_t r = a * P + pa, c = b * P + pb;
	if (diag && c < r) { const uint32_t t = r; r = c; c = t; }
	return (size_t)r * ldc + c;
}

}  // namespace twk
