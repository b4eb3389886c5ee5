// The landscape of `tomahawk ldaggregate`: which bin of the x axis and of the y axis a variant falls into.  The reference's coordinate
// rule (two_reader::Aggregate, lib/two_reader.cpp; lib/aggregation.h), applied to the variants of the loaded slice instead of to the
// records of a .two file.  Plain C++: twk_ld::Aggregate includes it, and so does csrc/tools/aggregate_bin_check.cpp (`make
// aggregate-check`), which plays it against a naive restatement.
//
//   one contig in the slice    coord = pos - min_pos, range = max_pos - min_pos + 1 (the data's range);
//   several contigs            each contig present spans its whole header length, offsets are cumulative in contig order, absent
//                              contigs take no room: coord = offset[rid] + pos, range = the sum of the present contigs' lengths;
//   bases per bin, per axis    (uint32_t)ceil((float)range / bins) - the reference's expression, float rounding included;
//   bin                        min(coord / bases_per_bin, bins - 1).
// Three departures from the reference.  It skips .two blocks of fewer than 5 records (marked "Todo: bugfix" in its source): nothing is
// skipped here.  It counts contig 0 twice when it decides "one contig or several", so a file with only contig 0 gets the whole-contig
// landscape: here the data range is used.  And the clamp to bins - 1 is ours: (float)range rounds, above 2^24 also downwards, and
// coord / bases_per_bin can then be `bins` - one past the end.
#pragma once
#include <math.h>
#include <stdint.h>
#include <vector>

namespace tomahawk {

struct twk_aggregate_landscape {
	uint64_t range = 0;                  // bases the axes cover
	uint32_t bpx = 0, bpy = 0;           // bases per bin on x and on y
	uint32_t min_pos = 0;                // one contig: what a position is counted from (0 for several)
	bool single = true;                  // one contig in the slice
	std::vector<uint64_t> offset;        // [contigs] several contigs: where the contig begins; absent contigs hold their successor's
	std::vector<uint8_t> present;        // [contigs]
};

// The reference's expression.  range >= 1 and bins >= 1: the result is at least 1.
inline uint32_t agl_bases_per_bin(uint64_t range, uint32_t bins) { return (uint32_t)ceilf((float)range / (float)bins); }
inline uint32_t agl_bin(uint64_t coord, uint32_t bases_per_bin, uint32_t bins) {
	const uint64_t b = coord / bases_per_bin;
	return b < bins - 1 ? (uint32_t)b : bins - 1;
}
inline uint64_t agl_coord(const twk_aggregate_landscape& l, uint32_t rid, uint32_t pos) {
	return l.single ? (uint64_t)(pos - l.min_pos) : l.offset[rid] + pos;
}

// The landscape of M variants (rid, pos) over contigs of these lengths, and every variant's bin on the two axes.  -> false if there
// is no variant, a variant names a contig the header does not have, the range is 0 or beyond 2^32 - 256 bases, or a bin count is
// outside [1, 4096].
inline bool agl_build(const uint32_t* rid, const uint32_t* pos, size_t M, const std::vector<int64_t>& contig_bases, uint32_t x_bins, uint32_t y_bins,
                      twk_aggregate_landscape& l, std::vector<uint16_t>& bin_x, std::vector<uint16_t>& bin_y) {
	if (M == 0 || x_bins < 1 || x_bins > 4096 || y_bins < 1 || y_bins > 4096) return false;
	l = twk_aggregate_landscape();
	l.present.assign(contig_bases.size(), 0);
	l.offset.assign(contig_bases.size(), 0);
	uint32_t lo = 0xFFFFFFFFu, hi = 0;
	for (size_t v = 0; v < M; ++v) {
		if (rid[v] >= contig_bases.size()) return false;
		l.present[rid[v]] = 1;
		if (pos[v] < lo) lo = pos[v];
		if (pos[v] > hi) hi = pos[v];
	}
	size_t n_present = 0;
	for (const uint8_t p : l.present) n_present += p;
	l.single = n_present == 1;
	if (l.single) {
		l.min_pos = lo;
		l.range = (uint64_t)hi - lo + 1;
	} else {
		uint64_t at = 0;
		for (size_t k = 0; k < contig_bases.size(); ++k) {
			l.offset[k] = at;
			if (l.present[k]) at += (uint64_t)(contig_bases[k] > 0 ? contig_bases[k] : 0);
		}
		l.range = at;
		if (l.range == 0) return false;
	}
	if (l.range > 0xFFFFFF00ull) return false;          // (beyond it (float)range / bins need not fit 32 bits)
	l.bpx = agl_bases_per_bin(l.range, x_bins);
	l.bpy = agl_bases_per_bin(l.range, y_bins);
	bin_x.resize(M); bin_y.resize(M);
	for (size_t v = 0; v < M; ++v) {
		const uint64_t coord = agl_coord(l, rid[v], pos[v]);
		bin_x[v] = (uint16_t)agl_bin(coord, l.bpx, x_bins);
		bin_y[v] = (uint16_t)agl_bin(coord, l.bpy, y_bins);
	}
	return true;
}

}  // namespace tomahawk
