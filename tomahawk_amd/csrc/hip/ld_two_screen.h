// The r2 screen of UnphasedMath's contraction over a count matrix, as arithmetic on one pair: what k_screen3_pairs and k_screen2_pairs (ld_three.hip.h: screen_pairs_body) run per
// thread, and what the planner (ld_plan.h) asks of a row before it gives its launches the two-product form.  Plain C++ - the device code and
// the host code include the same functions, and csrc/tools/two_check.cpp (`make two-check`) plays them on the CPU over every small genotype table.
//
// Three products leave HH = popc(H_A & H_B) and S = QH + HQ + 2 QQ of a pair; with the margins that is all the screen reads (screen3_keeps:
// the doubles of ScreenCountsUnphased, ld_count.hip.h, in the same order).
//
// Two products leave HH and HQ = popc(H_A & Q_B) only.  The terms of S that involve the row variant's hom-alt plane are bounded by the
// margins: QH + QQ <= qA and QQ <= min(qA, qB), so
//     S in [S_lo, S_hi],   S_lo = HQ,   S_hi = HQ + qA + min(qA, qB).
// Both of the screen's test values rise with S and e_lo <= e_hi at every S, so e_lo(S_lo) <= e_lo(S) <= e_hi(S) <= e_hi(S_hi): when the two
// outer ones lie inside (-sqrt(bound), sqrt(bound)), so do the two the three-product screen would have tested.  screen2_keeps therefore keeps
// every pair screen3_keeps keeps - and, for a row variant with few hom-alt carriers (qA ~ p^2 N), hardly any other.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TWK_SCREEN_FN __host__ __device__ inline
#else
#define TWK_SCREEN_FN inline
#endif

namespace twk {

struct ScreenMargins { uint32_t hA, qA, hB, qB; };       // het and hom-alt carriers of the row and of the column variant

// The test itself at the sums s_lo <= s_hi (three products: both are S).  two_n = 2N; cut = minR2 (1 - 1e-6).  hh is a double because the
// planner asks at an expected count; the kernels pass the integer they counted, converted as before.  bound_factor scales the bound the two
// test values are held to (1: the screen itself; the planner's margin squared).
TWK_SCREEN_FN bool screen_keeps_between(const ScreenMargins& m, double hh, double s_lo, double s_hi, double two_n, double cut, double bound_factor = 1.0) {
	const double T2n = two_n, eps = 1e-5 * (T2n * T2n);
	const double da = (double)(m.hA + 2u * m.qA), ra = T2n - da, fA = cut * (da * ra);
	const double db = (double)(m.hB + 2u * m.qB), rb = T2n - db, fB = db * rb;
	const double n11_lo = (ra - db) + s_lo, n11_hi = (ra - db) + s_hi;
	const double e_lo = (n11_lo * T2n - ra * rb) - eps;
	const double e_hi = ((n11_hi + hh) * T2n - ra * rb) + eps;
	const double bound = fA * fB * bound_factor;      // (x 1.0 is exact: the screen's own bound is fA fB)
	return !(e_lo * e_lo < bound && e_hi * e_hi < bound);
}
TWK_SCREEN_FN bool screen3_keeps(const ScreenMargins& m, uint32_t hh, uint32_t s_sum, double two_n, double cut) {
	return screen_keeps_between(m, (double)hh, (double)s_sum, (double)s_sum, two_n, cut);
}
TWK_SCREEN_FN double screen2_slack(const ScreenMargins& m) { return (double)m.qA + (double)(m.qA < m.qB ? m.qA : m.qB); }       // S_hi - S_lo
TWK_SCREEN_FN bool screen2_keeps(const ScreenMargins& m, uint32_t hh, uint32_t hq, double two_n, double cut) {
	return screen_keeps_between(m, (double)hh, (double)hq, (double)hq + screen2_slack(m), two_n, cut);
}

// The planner's question (ld_plan.h): would a pair with these margins whose variants are independent - HH = hA hB / N, HQ = hA qB / N -
// be kept by the two-product screen if the cut-off's square root were `margin` (< 1) of what it is?  A row for which the answer is yes
// against some column behind it floods the candidate list of a two-product launch: its launches take three products.
TWK_SCREEN_FN bool screen2_expected_keeps(const ScreenMargins& m, double n_samples, double two_n, double cut, double margin) {
	const double hh = (double)m.hA * (double)m.hB / n_samples, hq = (double)m.hA * (double)m.qB / n_samples;
	return screen_keeps_between(m, hh, hq, hq + screen2_slack(m), two_n, cut, margin * margin);
}

}  // namespace twk
