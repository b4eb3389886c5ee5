// LD aggregate: how a variant's two bins are packed, what integers a pair's statistic adds to a cell, how a partial sum is split over
// two accumulator words and how the host puts them together again.  Plain C++ with no HIP in it: k_ld_aggregate (ld_aggregate.hip.h)
// includes it, and so does csrc/tools/aggregate_bin_check.cpp (`make aggregate-check`), which plays every function against a naive
// restatement - so packing, quantisation, split and conversion are proven without a GPU, and a host that bins records (the tests, a
// user's script) can restate them from here.
//
// A pair's value v (signed r, r2, D or D', |v| <= 1 + a few ulps) is added as q = rint(v * 2^32), ties to even, a signed integer: the
// product is exact (a power of two), so q is v rounded ONCE to a multiple of 2^-32, |q * 2^-32 - v| <= 2^-33.  Its square is added as
// q2 = rint((v * v) * 2^32): one double multiplication (rounded once), then the same exact scaling and rounding.  Sums of q and of q2
// are sums of integers - exact, whatever their order.
//
// THE SPLIT.  A partial sum S (of a wave's lanes or of a block's LDS cell, |S| < 2^47) is added to a cell's accumulators as
// hi = S >> 20 (arithmetic: signed) and lo = S & (2^20 - 1) (not negative), S == hi * 2^20 + lo, without a carry between the words.
// ld_aggregate.hip.h proves that neither word can overflow while a call stays inside the room the engine enforces.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TWK_AG_FN __host__ __device__ inline
#else
#define TWK_AG_FN inline
#endif

namespace twk {

constexpr uint32_t AGG_MAX_BINS = 4096;               // bins per axis
constexpr uint32_t AGG_OFF = 0xFFFFu;                 // a variant that is off the landscape on an axis
constexpr uint32_t AGG_NO_KEY = 0xFFFFFFFFu;          // off on both axes: contributes nothing (and a lane without a pair)
constexpr double AGG_SCALE = 4294967296.0;            // 2^32
constexpr int AGG_SPLIT = 20;                         // a partial sum S goes to the accumulators as S >> 20 and S & (2^20 - 1)
constexpr unsigned long long AGG_SPLIT_MASK = (1ull << AGG_SPLIT) - 1;

// A variant's two bins in one word: x in the low half, y in the high half.
TWK_AG_FN uint32_t ag_pack(uint32_t bin_x, uint32_t bin_y) { return (bin_x & 0xFFFFu) | bin_y << 16; }
TWK_AG_FN uint32_t ag_x(uint32_t key) { return key & 0xFFFFu; }
TWK_AG_FN uint32_t ag_y(uint32_t key) { return key >> 16; }
// v as an integer number of 2^-32: round to nearest, ties to even (the default rounding mode on both sides).
TWK_AG_FN long long ag_quantise(double v) { return llrint(v * AGG_SCALE); }
// v squared likewise: the square is one double multiplication, the scaling is exact.
TWK_AG_FN unsigned long long ag_quantise_sq(double v) { const double sq = v * v; return (unsigned long long)llrint(sq * AGG_SCALE); }
// The two words of a signed partial sum.  (>> of a negative signed integer is arithmetic on every compiler this builds with; the check
// plays it against a floor division.)
TWK_AG_FN long long ag_split_hi(long long s) { return s >> AGG_SPLIT; }
TWK_AG_FN unsigned long long ag_split_lo(long long s) { return (unsigned long long)s & AGG_SPLIT_MASK; }
// ... and of an unsigned one.
TWK_AG_FN unsigned long long ag_split_hi_u(unsigned long long s) { return s >> AGG_SPLIT; }
TWK_AG_FN unsigned long long ag_split_lo_u(unsigned long long s) { return s & AGG_SPLIT_MASK; }
// A cell's sum as the host forms it from its two accumulators (host only): acc_hi holds the sums of the `hi` words (two's complement
// for a signed sum), acc_lo the sums of the `lo` words, which may have grown far past 2^20.  hi * 2^20 + lo in 128 bits is the exact
// sum of the cell's q; it is converted to double once, to nearest, and the scaling by 2^-32 is exact.
inline double ag_sum_to_double_signed(unsigned long long acc_hi, unsigned long long acc_lo) {
	const __int128 q = (__int128)(long long)acc_hi * (__int128)(1ll << AGG_SPLIT) + (__int128)acc_lo;
	return (double)q / AGG_SCALE;
}
inline double ag_sum_to_double_unsigned(unsigned long long acc_hi, unsigned long long acc_lo) {
	const unsigned __int128 q = ((unsigned __int128)acc_hi << AGG_SPLIT) + acc_lo;
	return (double)q / AGG_SCALE;
}
// One quantised value (an extreme of a cell) back as a double: |q| < 2^53, so exact.
inline double ag_value_to_double(long long q) { return (double)q / AGG_SCALE; }

}  // namespace twk
