// LD matrix: where a lane of k_ld_matrix_fill (ld_matrix.hip.h) stores, and when.  Plain C++ with no HIP in it: the kernel includes
// it, and so does csrc/tools/matrix_index_check.cpp (`make matrix-check`), which plays every lane of every block of a set of launch
// geometries against an n x n array with a border - so the slot arithmetic and the guards are proven without a GPU.
//
// The device matrix is n x n floats, row pitch n, of the variants [slice_a0, slice_a0 + n) in file order.  A fill block is
// MX_COLS = 256 lanes = 256 columns of the launch (set positions b0 + j) and walks MX_ROWS = 32 of its rows (a0 + i).
//   direct store    (row variant, column variant): a wave's 64 lanes write 64 consecutive floats of one row.
//   mirrored store  (column variant, row variant).  Per lane it would be strided by n * 4 bytes - one store per cache line - so on a
//                   plain plane set the block's values are staged in LDS, stage[r][c], and written out transposed after the row loop:
//                   half a wave (32 lanes) takes the 32 rows r of ONE column c, i.e. 32 consecutive floats of output row c.  The two
//                   halves take the columns c and c + 32.  A 4-byte LDS read or write is banked modulo 32 words, and only the 32
//                   lanes of one half of a wave can conflict.  With a pitch of MX_PITCH = 257 words the bank of stage[r][c] is
//                   (r + c) mod 32: 32 different banks for the 32 rows a half reads - no conflict on the transposed read, and the
//                   staging write (a half writes 32 consecutive c of one r) has none either.
//   regrouped set   (ids != null) columns are not consecutive and a pair arrives in either order: both entries per lane, at the ids.
// Every store is guarded: tiles overhang the slice, so a store happens only when both relative indices are below n; on a plain set
// only with column variant > row variant (a triangle's launches lie on or above its diagonal), on a regrouped set only with u != v.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TWK_MX_FN __host__ __device__ inline
#else
#define TWK_MX_FN inline
#endif

namespace twk {

constexpr uint32_t MX_COLS = 256;                    // lanes = columns of a fill block
constexpr uint32_t MX_ROWS = 32;                     // rows of a fill block: the consecutive floats of a mirrored store
constexpr uint32_t MX_PITCH = MX_COLS + 1;           // words per staged row: 257 = 1 (mod 32 banks)
constexpr uint32_t MX_STAGE_WORDS = MX_ROWS * MX_PITCH;          // 32,896 bytes of LDS
constexpr uint32_t MX_TSTEPS = 32;                   // steps of the transposed write-out: a wave's 64 columns, two a step

// A lane has a pair at all: inside the launch's rectangle.
TWK_MX_FN bool mx_lane_live(uint32_t i, uint32_t j, uint32_t nA, uint32_t nB) { return i < nA && j < nB; }
// A block that lies wholly on or below the diagonal of a diagonal launch has no pair (bx, i0: its first column block and first row).
TWK_MX_FN bool mx_block_dead(bool diag_launch, uint32_t bx, uint32_t i0) { return diag_launch && bx * MX_COLS + (MX_COLS - 1) <= i0; }
// Set position -> index relative to the slice (plain set: the position is the variant).  Below the slice it wraps to a huge number,
// which every guard refuses.
TWK_MX_FN uint32_t mx_rel(uint32_t first, uint32_t k, uint32_t slice_a0) { return first + k - slice_a0; }
// Guard of a pair's two stores on a plain set: (row, col) direct, (col, row) mirrored.
TWK_MX_FN bool mx_ok_plain(uint32_t row, uint32_t col, uint32_t n) { return row < n && col < n && row < col; }
// ... and on a regrouped set (u, v in either order).
TWK_MX_FN bool mx_ok_ids(uint32_t u, uint32_t v, uint32_t n) { return u < n && v < n && u != v; }
// Slot of (row, col) in the n x n matrix.
TWK_MX_FN size_t mx_slot(uint32_t row, uint32_t col, uint32_t n) { return (size_t)row * n + col; }
// LDS staging index of the block's row r, column c.
TWK_MX_FN uint32_t mx_stage(uint32_t r, uint32_t c) { return r * MX_PITCH + c; }
// The transposed write-out: in step k = 0 .. MX_TSTEPS - 1 thread tid reads stage[mx_trow(tid)][mx_tcol(tid, k)] and stores it at
// (column variant, row variant).
TWK_MX_FN uint32_t mx_trow(uint32_t tid) { return tid & 31; }
TWK_MX_FN uint32_t mx_tcol(uint32_t tid, uint32_t k) { return (tid & ~63u) + ((tid >> 5) & 1) * 32 + k; }
// LDS bank of a staged word for 4-byte accesses (banked modulo 32 words; the two halves of a wave never conflict with each other).
TWK_MX_FN uint32_t mx_bank(uint32_t word) { return word & 31; }

}  // namespace twk
