// Sums that are exact and have no order: what LD decay (ld_decay.hip.h) and the LD aggregate (ld_aggregate.hip.h) add up, and how the host
// reads it back.  Plain C++ with no HIP in it: the two kernels include it, and so does csrc/tools/exact_sum_check.h (`make decay-check`,
// `make aggregate-check`), which plays every function against a naive restatement for both split widths - proven without a GPU.
//
// A value v (r2, signed r, D or D': |v| <= 1 + a few ulps) is added as q = rint(v * 2^32), ties to even, a signed integer: the product is
// exact (a power of two), so q is v rounded ONCE to a multiple of 2^-32, |q * 2^-32 - v| <= 2^-33.  Its square is added as
// q2 = rint((v * v) * 2^32): one double multiplication (rounded once), then the same exact scaling and rounding.  Sums of q and of q2
// are sums of integers - exact, whatever their order.
//
// THE SPLIT.  A partial sum S (of a wave's lanes or of a block's LDS cell) is added to two accumulator words as hi = S >> K (arithmetic
// for a signed S) and lo = S & (2^K - 1) (not negative), S == hi * 2^K + lo, without a carry between the words: lo may grow far past
// 2^K.  The host forms hi * 2^K + lo in 128 bits - the exact sum - and converts it to double once, to nearest; the scaling by 2^-32 is
// exact.  K is the kind's own (decay 32, aggregate 20): the kernel that picks it proves that neither word can overflow while a call
// stays inside the room the engine enforces.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TWK_XS_FN __host__ __device__ inline
#else
#define TWK_XS_FN inline
#endif

namespace twk {

constexpr double XS_SCALE = 4294967296.0;            // 2^32: q = rint(v * XS_SCALE), a sum = the sum of q / XS_SCALE

// v as an integer number of 2^-32: round to nearest, ties to even (the default rounding mode on both sides).
TWK_XS_FN long long xs_quantise(double v) { return llrint(v * XS_SCALE); }
// v squared likewise: the square is one double multiplication, the scaling is exact.
TWK_XS_FN unsigned long long xs_quantise_sq(double v) { const double sq = v * v; return (unsigned long long)llrint(sq * XS_SCALE); }
// The two words of a signed partial sum.  (>> of a negative signed integer is arithmetic on every compiler this builds with; the check
// plays it against a floor division.)
template <int K> TWK_XS_FN long long xs_split_hi(long long s) { return s >> K; }
template <int K> TWK_XS_FN unsigned long long xs_split_lo(long long s) { return (unsigned long long)s & ((1ull << K) - 1); }
// ... and of an unsigned one.
template <int K> TWK_XS_FN unsigned long long xs_split_hi_u(unsigned long long s) { return s >> K; }
template <int K> TWK_XS_FN unsigned long long xs_split_lo_u(unsigned long long s) { return s & ((1ull << K) - 1); }

// Host only from here on.  A sum as the host forms it from its two accumulators: acc_hi holds the sums of the `hi` words (two's
// complement for a signed sum), acc_lo the sums of the `lo` words.
template <int K> inline __int128 xs_join_signed(unsigned long long acc_hi, unsigned long long acc_lo) {
	return (__int128)(long long)acc_hi * ((__int128)1 << K) + (__int128)acc_lo;
}
template <int K> inline unsigned __int128 xs_join_unsigned(unsigned long long acc_hi, unsigned long long acc_lo) {
	return ((unsigned __int128)acc_hi << K) + acc_lo;
}
template <int K> inline double xs_sum_to_double_signed(unsigned long long acc_hi, unsigned long long acc_lo) { return (double)xs_join_signed<K>(acc_hi, acc_lo) / XS_SCALE; }
template <int K> inline double xs_sum_to_double_unsigned(unsigned long long acc_hi, unsigned long long acc_lo) { return (double)xs_join_unsigned<K>(acc_hi, acc_lo) / XS_SCALE; }
// One quantised value (an extreme of a cell) back as a double: |q| < 2^53, so exact.
inline double xs_value_to_double(long long q) { return (double)q / XS_SCALE; }

}  // namespace twk
