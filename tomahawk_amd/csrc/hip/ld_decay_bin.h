// LD decay: which bin a pair's distance falls into and what integer its r2 adds there.  Plain C++ with no HIP in it: k_ld_decay
// (ld_decay.hip.h) includes it, and so does csrc/tools/decay_bin_check.cpp (`make decay-check`), which plays every function against a
// naive restatement - so the binning and the quantisation are proven without a GPU, and a host that bins records (the tests, a user's
// script) can restate them from here.
//
// The arithmetic is the reference's (two_reader::Decay, lib/two_reader.cpp): width = range_bp / n_bins in integers, bin = d / width,
// and the last bin also takes everything at and beyond the range.  A pair's r2 is added as q = rint(r2 * 2^32), ties to even: the
// product is exact (a power of two), so q is r2 rounded ONCE to a multiple of 2^-32, |q * 2^-32 - r2| <= 2^-33, and sums of q are sums
// of integers - exact, whatever their order.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TWK_DK_FN __host__ __device__ inline
#else
#define TWK_DK_FN inline
#endif

namespace twk {

constexpr uint32_t DECAY_MAX_BINS = 4096;            // 12 bytes of LDS a bin: 48 KiB
constexpr double DECAY_SCALE = 4294967296.0;         // 2^32: q = rint(r2 * DECAY_SCALE), sum_r2 = sum of q / DECAY_SCALE

// Bases per bin.  (0 when range_bp < n_bins: the entry point refuses that.)
TWK_DK_FN uint32_t dk_width(uint32_t range_bp, uint32_t n_bins) { return range_bp / n_bins; }
// |posA - posB| of two positions on one contig, in either order.
TWK_DK_FN uint32_t dk_distance(uint32_t pos_a, uint32_t pos_b) { return pos_a > pos_b ? pos_a - pos_b : pos_b - pos_a; }
// The bin of distance d: d / width, the last bin for everything beyond it.  width >= 1, n_bins >= 1.
TWK_DK_FN uint32_t dk_bin(uint32_t d, uint32_t width, uint32_t n_bins) {
	const uint32_t b = d / width;
	return b < n_bins - 1 ? b : n_bins - 1;
}
// r2 in [0, 1 + a few ulps] as an integer number of 2^-32: round to nearest, ties to even (the default rounding mode on both sides).
TWK_DK_FN unsigned long long dk_quantise(double r2) { return (unsigned long long)llrint(r2 * DECAY_SCALE); }
// A bin's sum as the host forms it from the two device accumulators (host only): acc_int holds the sums' bits from 32 up, acc_frac the
// bits below - each added to without a carry into the other, so acc_frac may have grown past 2^32.  (acc_int << 32) + acc_frac in 128
// bits is the exact sum of the bin's q; it is converted to double once, to nearest, and the scaling by 2^-32 is exact.
inline double dk_sum_to_double(unsigned long long acc_int, unsigned long long acc_frac) {
	const unsigned __int128 q = ((unsigned __int128)acc_int << 32) + acc_frac;
	return (double)q / DECAY_SCALE;
}

}  // namespace twk
