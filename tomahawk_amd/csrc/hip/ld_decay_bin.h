// LD decay: which bin a pair's distance falls into, and the width at which its partial sums are split.  Plain C++ with no HIP in it:
// k_ld_decay (ld_decay.hip.h) includes it, and so does csrc/tools/decay_bin_check.cpp (`make decay-check`), which plays every function
// against a naive restatement - so the binning is proven without a GPU, and a host that bins records (the tests, a user's script) can
// restate it from here.  What integer a pair's r2 adds to its bin, and how the host reads the sums back, is ld_exact_sum.h.
//
// The arithmetic is the reference's (two_reader::Decay, lib/two_reader.cpp): width = range_bp / n_bins in integers, bin = d / width,
// and the last bin also takes everything at and beyond the range.
#pragma once
#include <stdint.h>
#include "ld_exact_sum.h"

namespace twk {

constexpr uint32_t DECAY_MAX_BINS = 4096;            // 12 bytes of LDS a bin: 48 KiB
constexpr int DECAY_SPLIT = 32;                      // a block's sum S goes to the accumulators as S >> 32 and S & (2^32 - 1)

// Bases per bin.  (0 when range_bp < n_bins: the entry point refuses that.)
TWK_XS_FN uint32_t dk_width(uint32_t range_bp, uint32_t n_bins) { return range_bp / n_bins; }
// |posA - posB| of two positions on one contig, in either order.
TWK_XS_FN uint32_t dk_distance(uint32_t pos_a, uint32_t pos_b) { return pos_a > pos_b ? pos_a - pos_b : pos_b - pos_a; }
// The bin of distance d: d / width, the last bin for everything beyond it.  width >= 1, n_bins >= 1.
TWK_XS_FN uint32_t dk_bin(uint32_t d, uint32_t width, uint32_t n_bins) {
	const uint32_t b = d / width;
	return b < n_bins - 1 ? b : n_bins - 1;
}

}  // namespace twk
