// Banded LD matrix: the band's layout, where a lane of k_ld_bandmat_fill (ld_bandmat.hip.h) stores, and when.  Plain C++ with no HIP in
// it, in the manner of ld_matrix_index.h: the kernel includes it, and so does csrc/tools/bandmat_index_check.cpp (`make bandmat-check`),
// which checks the layout against its O(n^2) definition and plays every lane of every block of a set of launch geometries against an
// array of write counts with a border.
//
// THE LAYOUT.  The variants of a slice [a0, a0 + n) are sorted by (rid, pos), as in every .twk.  With a window of w base pairs the band of
// row u is the contiguous column range [first[u], first[u] + len[u]), relative to the slice: the variants v on u's contig with
// |pos[u] - pos[v]| <= w - the rule of the engine's window test (d_pair, ld_math.hip.h).  It is symmetric (v in u's band <=> u in v's),
// holds the diagonal, and is clipped at contig and slice borders; first[] and first[] + len[] never decrease with u.  The rows lie one
// behind the other: row_ptr[u] = len[0] + .. + len[u - 1], row_ptr[n] floats in all, and (u, v) lives at row_ptr[u] + (v - first[u]).
// On the device a row is a BandRow {base = row_ptr[u], first, len}.
//
// THE STORES are the dense fill's (ld_matrix_index.h: the direct store, the mirrored store staged in LDS with pitch 257 and written out
// transposed by half-waves, both per lane at the ids on a regrouped set), the mx_* functions unchanged, with the row pitch n replaced
// by the row's base and first.  Every store passes the dense guards (mx_ok_plain / mx_ok_ids) AND bm_in_band: a pair that passes the
// window test is inside the band by construction, the guard is what keeps a mistake from becoming a store outside the buffer.
// A DEAD BLOCK: on a plain set a launch lies on or above the diagonal, so a block whose first column is at or beyond the band end of
// its last row holds no in-band pair (the band ends never decrease) and returns before it evaluates one.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "ld_matrix_index.h"

namespace twk {

// A row of the band on the device.
struct BandRow {
	uint64_t base;                   // row_ptr[u]: the slot of the row's first stored column
	uint32_t first, len;             // the stored columns [first, first + len), relative to the slice
};

// The layout of n variants, variant k of the slice at pos(k) on contig rid(k), by two pointers that only move forward.  first[n],
// row_ptr[n + 1].  -> false, with nothing promised about the arrays, if the variants are not sorted by (rid, pos): a band would then
// not be a contiguous range.
template <class Pos, class Rid>
inline bool bm_layout(uint32_t n, Pos pos, Rid rid, uint32_t w, uint32_t* first, uint64_t* row_ptr) {
	uint32_t lo = 0, hi = 0;
	uint64_t at = 0;
	for (uint32_t u = 0; u < n; ++u) {
		const uint32_t ru = rid(u);
		const int64_t pu = (int64_t)pos(u);
		if (u && (rid(u - 1) > ru || (rid(u - 1) == ru && (int64_t)pos(u - 1) > pu))) return false;
		while (rid(lo) != ru || pu - (int64_t)pos(lo) > (int64_t)w) ++lo;          // (stops at u at the latest)
		if (hi < u + 1) hi = u + 1;
		while (hi < n && rid(hi) == ru && (int64_t)pos(hi) - pu <= (int64_t)w) ++hi;
		first[u] = lo;
		row_ptr[u] = at;
		at += hi - lo;
	}
	row_ptr[n] = at;
	return true;
}

// ... and everything a call needs of it, on the host: first and row_ptr as the caller gets them, the rows as the device reads them
// (rows[u] == {ptr[u], first[u], ptr[u + 1] - ptr[u]}), the number of slots (ptr[n]) and the longest row.  Filled once, by bm_band_layout.
struct BandLayout {
	std::vector<uint32_t> first;     // [n]
	std::vector<uint64_t> ptr;       // [n + 1]
	std::vector<BandRow> rows;       // [n]
	size_t cells = 0;
	uint32_t widest = 0;
};
template <class Pos, class Rid>
inline bool bm_band_layout(uint32_t n, Pos pos, Rid rid, uint32_t w, BandLayout& b) {
	b.first.assign(n, 0); b.ptr.assign((size_t)n + 1, 0); b.rows.resize(n);
	b.cells = 0; b.widest = 0;
	if (!bm_layout(n, pos, rid, w, b.first.data(), b.ptr.data())) return false;
	for (uint32_t u = 0; u < n; ++u) {
		b.rows[u] = BandRow{b.ptr[u], b.first[u], (uint32_t)(b.ptr[u + 1] - b.ptr[u])};      // (a row holds at most n columns)
		if (b.rows[u].len > b.widest) b.widest = b.rows[u].len;
	}
	b.cells = (size_t)b.ptr[n];
	return true;
}

// Column `col` lies in the band [first, first + len) (a column below `first` wraps to a huge number and is refused).
TWK_MX_FN bool bm_in_band(uint32_t col, uint32_t first, uint32_t len) { return col - first < len; }
// Slot of (row, col) of a row whose band begins at column `first` and at slot `base`.  Only for bm_in_band(col, first, len).
TWK_MX_FN uint64_t bm_slot(uint64_t base, uint32_t first, uint32_t col) { return base + (col - first); }
// The last row of the block whose first row is i0 of a launch of nA rows, as an index into the slice's map: clipped to the launch and
// to the slice (a row outside the slice stores nothing: the clip only has to stay inside the map, and n - 1 has the furthest band end).
TWK_MX_FN uint32_t bm_block_last_row(uint32_t a0, uint32_t i0, uint32_t nA, uint32_t slice_a0, uint32_t n) {
	const uint32_t last = i0 + (MX_ROWS - 1) < nA ? i0 + (MX_ROWS - 1) : nA - 1;
	const uint32_t u = mx_rel(a0, last, slice_a0);
	return u < n ? u : n - 1;
}
// A block of a plain set whose first column (set position b0 + bx * MX_COLS; not below the slice, where the relative index would wrap)
// is at or beyond the band end of its last row has no in-band pair on or above the diagonal, and a plain set has no other.
TWK_MX_FN bool bm_block_dead(uint32_t b0, uint32_t bx, uint32_t slice_a0, uint32_t last_first, uint32_t last_len) {
	const uint32_t s0 = b0 + bx * MX_COLS;
	return s0 >= slice_a0 && s0 - slice_a0 >= last_first + last_len;
}

}  // namespace twk
