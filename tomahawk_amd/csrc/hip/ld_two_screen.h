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
// (Further down: the same two products of the row variant's carrier plane H | Q, whose interval is narrower - screen2c_*.)
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

// ---- the carrier plane as the row operand ------------------------------------------------------------------------------
// A two-product launch may contract the row variant's carrier plane C_A = H_A | Q_A in the H plane's place.  It leaves
//     CH = popc(C_A & H_B) = HH + QH,     CQ = popc(C_A & Q_B) = HQ + QQ,
// and with S = QH + HQ + 2 QQ = CQ + popc(Q_A & C_B) and T = S + HH = CH + CQ + QQ (e_lo is tested at S, e_hi at T):
//     S >= CQ,     T <= CH + CQ + min(qA, qB).
// Both ends lie inside the H form's - CQ >= HQ, and CH + CQ + min = HH + HQ + (QH + QQ) + min <= HH + HQ + qA + min - so screen2c_keeps keeps
// every pair screen3_keeps keeps and none that screen2_keeps drops; the gap above T falls from about 2 qA to min(qA, qB).
TWK_SCREEN_FN double screen2c_slack(const ScreenMargins& m) { return (double)(m.qA < m.qB ? m.qA : m.qB); }       // (T's upper end) - CH - CQ
// The launch has counted CQ = HQ + QQ >= QQ itself, so QQ <= min(qA, qB, CQ) costs nothing: the gap above T is never more than CQ (the fine
// walk, option "walk_fine"; `fine` false: the bound by the margins alone).  At a = b = 0.25 under independence the term falls from 0.0625 N to
// 0.027 N, less than the room the screen has above T there.  The one-product form counts no CQ and keeps screen2c_slack.
TWK_SCREEN_FN double screen2c_slack_cq(const ScreenMargins& m, double cq, bool fine) { const double s = screen2c_slack(m); return fine && cq < s ? cq : s; }
TWK_SCREEN_FN bool screen2c_keeps(const ScreenMargins& m, uint32_t ch, uint32_t cq, double two_n, double cut, bool fine = false) {
	return screen_keeps_between(m, (double)ch, (double)cq, (double)cq + screen2c_slack_cq(m, (double)cq, fine), two_n, cut);
}
// The planner's question of the carrier form: under independence CH = cA hB / N and CQ = cA qB / N with cA = hA + qA (fine: the expected CQ in the min).
TWK_SCREEN_FN bool screen2c_expected_keeps(const ScreenMargins& m, double n_samples, double two_n, double cut, double margin, bool fine = false) {
	const double ca = (double)m.hA + (double)m.qA, ch = ca * (double)m.hB / n_samples, cq = ca * (double)m.qB / n_samples;
	return screen_keeps_between(m, ch, cq, cq + screen2c_slack_cq(m, cq, fine), two_n, cut, margin * margin);
}

// ---- one product: the two carrier planes against each other --------------------------------------------------------------
// CH + CQ = popc(C_A & (H_B | Q_B)) = popc(C_A & C_B) = CC: the upper end of the carrier screen, CH + CQ + min(qA, qB), needs only the one product
// of the two variants' carrier rows.  CQ by itself is read by the lower test alone - and there the trivial bound S >= 0 may stand in its place:
//     T = S + HH = CC + QQ <= CC + min(qA, qB),     S >= 0,
// and both test values rise with their argument, so the screen at (hh = CC, s_lo = 0, s_hi = min(qA, qB)) tests the same upper value as
// screen2c_keeps and a lower value no larger than its: it keeps every pair screen2c_keeps keeps, which keeps every pair screen3_keeps keeps.
// The lower value at s_lo = 0 reads no count at all: e_lo(0) = (ra - db) 2N - ra rb - eps = -(da db) - eps, a function of the two dosages - the
// sort key of the sorted set - which lies inside the bound whenever, roughly, ab / ((1 - a)(1 - b)) < minR2 for allele frequencies a, b
// (screen1c_lower_ok: the planner's exact question, ld_plan.h plan_one_end).  For such a pair the one-product screen drops what the carrier
// screen drops wherever the latter's own lower test was not the one that kept the pair.
TWK_SCREEN_FN bool screen1c_keeps(const ScreenMargins& m, uint32_t cc, double two_n, double cut) {
	return screen_keeps_between(m, (double)cc, 0.0, screen2c_slack(m), two_n, cut);
}
// The lower half alone, at s_lo = 0 (the doubles of screen_keeps_between in the same order): true where the one-product screen's lower test
// passes whatever the counts - the upper test then decides alone.
TWK_SCREEN_FN bool screen1c_lower_ok(const ScreenMargins& m, double two_n, double cut) {
	const double T2n = two_n, eps = 1e-5 * (T2n * T2n);
	const double da = (double)(m.hA + 2u * m.qA), ra = T2n - da, fA = cut * (da * ra);
	const double db = (double)(m.hB + 2u * m.qB), rb = T2n - db, fB = db * rb;
	const double n11_lo = (ra - db) + 0.0;
	const double e_lo = (n11_lo * T2n - ra * rb) - eps;
	return e_lo * e_lo < fA * fB;
}
// The upper half alone, at t_hi = s_hi + hh, against the bound scaled by bound_factor.
TWK_SCREEN_FN bool screen_upper_keeps(const ScreenMargins& m, double t_hi, double two_n, double cut, double bound_factor = 1.0) {
	const double T2n = two_n, eps = 1e-5 * (T2n * T2n);
	const double da = (double)(m.hA + 2u * m.qA), ra = T2n - da, fA = cut * (da * ra);
	const double db = (double)(m.hB + 2u * m.qB), rb = T2n - db, fB = db * rb;
	const double e_hi = (((ra - db) + t_hi) * T2n - ra * rb) + eps;
	return !(e_hi * e_hi < fA * fB * bound_factor);
}
// The planner's question of the one-product form: under independence CC = cA cB / N.  The lower test has no count in it - it is asked exactly,
// without the margin, as the plan asked it (plan_one_end) - so the margin shrinks the upper test's bound alone.
TWK_SCREEN_FN bool screen1c_expected_keeps(const ScreenMargins& m, double n_samples, double two_n, double cut, double margin) {
	if (!screen1c_lower_ok(m, two_n, cut)) return true;
	const double cc = ((double)m.hA + (double)m.qA) * ((double)m.hB + (double)m.qB) / n_samples;
	return screen_upper_keeps(m, cc + screen2c_slack(m), two_n, cut, margin * margin);
}

// ---- the prefix contraction ------------------------------------------------------------------------------------------
// A launch may contract only the first K chunks [0, stop) of a tile's rows.  Per sample, with g = 0 / 1 / 2 alt alleles, the contribution to
// S = QH + HQ + 2 QQ is >= 0 and the contribution to S + HH is exactly min(gA, gB); summed over the unread suffix, whose margins are the
// popcounts h', q' of the row suffixes (dosage d' = h' + 2 q'):
//     S_suffix >= 0,     (S + HH)_suffix <= min(dA', dB').
// e_lo is tested at s_lo and e_hi at s_hi + hh, and both rise with their argument, so with the prefix counts in the totals' place and
// min(dA', dB') added to s_hi the two outer values again enclose the ones the full three-product screen would test: a prefix screen keeps
// every pair screen3_keeps keeps on the whole rows.  What it keeps is recounted over the whole rows (k_recount_unphased).
struct SuffixMargins { uint32_t hA, qA, hB, qB; };       // het and hom-alt carriers among the samples behind the stop
TWK_SCREEN_FN double prefix_slack(const SuffixMargins& x) {
	const double da = (double)x.hA + 2.0 * (double)x.qA, db = (double)x.hB + 2.0 * (double)x.qB;
	return da < db ? da : db;
}
// Three products over the prefix: hh = HH_pre, s_sum = S_pre.
TWK_SCREEN_FN bool screen3_prefix_keeps(const ScreenMargins& m, const SuffixMargins& x, uint32_t hh, uint32_t s_sum, double two_n, double cut) {
	return screen_keeps_between(m, (double)hh, (double)s_sum, (double)s_sum + prefix_slack(x), two_n, cut);
}
// ---- the (U, Z) form of the three-product contraction (ld_count_uz.hip.h) ------------------------------------------------------------
// Such a launch leaves U = popc(H_A | H_B) and Z = popc((Q_A ^ Q_B) & ~(H_A | H_B)) where the product form leaves HH and S.  H and Q of a variant
// are disjoint and no genotype is missing, so per sample - and over any range of samples, with the margins counted over the same range -
//     HH = hA + hB - U                                  (inclusion - exclusion),
//     S  = QH + HQ + 2 QQ = qA + qB - Z                 (qA + qB counts the cells 20 21 22 02 12 22; Z the opposite homozygotes 20 and 02).
// In integers and exact: the screens behind it test the numbers the product form would have counted.  m: the margins over the range the
// counts cover - the rows' popcounts, or (uz_prefix_to_hh_s) those minus the suffix margins at the tile's stop.
struct CountsHS { uint32_t hh, s; };
TWK_SCREEN_FN CountsHS uz_to_hh_s(const ScreenMargins& m, uint32_t u, uint32_t z) { return CountsHS{m.hA + m.hB - u, m.qA + m.qB - z}; }
TWK_SCREEN_FN CountsHS uz_prefix_to_hh_s(const ScreenMargins& m, const SuffixMargins& x, uint32_t u, uint32_t z) {
	return uz_to_hh_s(ScreenMargins{m.hA - x.hA, m.qA - x.qA, m.hB - x.hB, m.qB - x.qB}, u, z);
}
// Two products over the prefix: hh = HH_pre, hq = HQ_pre; the prefix's own S is bounded by the prefix margins (total minus suffix).
TWK_SCREEN_FN bool screen2_prefix_keeps(const ScreenMargins& m, const SuffixMargins& x, uint32_t hh, uint32_t hq, double two_n, double cut) {
	const double qa = (double)(m.qA - x.qA), qb = (double)(m.qB - x.qB);
	return screen_keeps_between(m, (double)hh, (double)hq, (double)hq + qa + (qa < qb ? qa : qb) + prefix_slack(x), two_n, cut);
}
// The planner's question for a stop (ld_plan.h plan_prefix_stop): would a pair of independent variants with these margins, n_pre samples in
// front of the stop, be kept by the prefix screen if the cut-off's square root were `margin` of what it is?  The expected prefix counts come
// from the prefix margins themselves (HH_pre = hA_pre hB_pre / n_pre, ...), the suffix term from the suffix margins.
TWK_SCREEN_FN bool prefix_expected_keeps(const ScreenMargins& m, const SuffixMargins& x, bool two, double n_pre, double two_n, double cut, double margin) {
	if (n_pre <= 0) return true;
	const double ha = (double)(m.hA - x.hA), qa = (double)(m.qA - x.qA), hb = (double)(m.hB - x.hB), qb = (double)(m.qB - x.qB);
	const double hh = ha * hb / n_pre, hq = ha * qb / n_pre;
	if (two) return screen_keeps_between(m, hh, hq, hq + qa + (qa < qb ? qa : qb) + prefix_slack(x), two_n, cut, margin * margin);
	const double s = (qa * hb + ha * qb + 2.0 * qa * qb) / n_pre;
	return screen_keeps_between(m, hh, s, s + prefix_slack(x), two_n, cut, margin * margin);
}

// The carrier form over the prefix: ch = CH_pre, cq = CQ_pre.  S_pre >= CQ_pre and T_pre <= CH_pre + CQ_pre + min(qa_pre, qb_pre) as over whole
// rows, with the prefix margins (total minus suffix); the unread suffix adds prefix_slack(x) to the upper end as in the other prefix screens.
// fine: QQ_pre <= CQ_pre too - what the launch counted over the prefix is itself such a bound, so it is sound over a prefix as it stands.
TWK_SCREEN_FN double prefix_slack_cq(double qa, double qb, double cq, bool fine) { const double s = qa < qb ? qa : qb; return fine && cq < s ? cq : s; }
TWK_SCREEN_FN bool screen2c_prefix_keeps(const ScreenMargins& m, const SuffixMargins& x, uint32_t ch, uint32_t cq, double two_n, double cut, bool fine = false) {
	const double qa = (double)(m.qA - x.qA), qb = (double)(m.qB - x.qB);
	return screen_keeps_between(m, (double)ch, (double)cq, (double)cq + prefix_slack_cq(qa, qb, (double)cq, fine) + prefix_slack(x), two_n, cut);
}
// ... and the planner's question for a stop of a carrier launch (prefix_expected_keeps with two = true, in the carrier form).
TWK_SCREEN_FN bool prefix_expected_keeps_carrier(const ScreenMargins& m, const SuffixMargins& x, double n_pre, double two_n, double cut, double margin, bool fine = false) {
	if (n_pre <= 0) return true;
	const double ha = (double)(m.hA - x.hA), qa = (double)(m.qA - x.qA), hb = (double)(m.hB - x.hB), qb = (double)(m.qB - x.qB);
	const double ch = (ha + qa) * hb / n_pre, cq = (ha + qa) * qb / n_pre;
	return screen_keeps_between(m, ch, cq, cq + prefix_slack_cq(qa, qb, cq, fine) + prefix_slack(x), two_n, cut, margin * margin);
}

// The planner's second question for a stop (ld_plan.h PrefixEnv::dropped): the screen's own bound (bound_factor 1), asked at the expected
// prefix counts moved outwards by z standard deviations - s_lo down, s_hi + hh up.  The standard deviations are those of the prefix sums of
// n_pre independent samples whose (gA, gB) follow the prefix margins: P(gA = 1) = ha / n_pre, P(gA = 2) = qa / n_pre, likewise gB.  Per sample
//     S = QH + HQ + 2 QQ     mean a2 b1 + a1 b2 + 2 a2 b2,              second moment a2 b1 + a1 b2 + 4 a2 b2
//     T = S + HH             mean a1 b1 + a1 b2 + a2 b1 + 2 a2 b2,      second moment ... + 4 a2 b2
//     HQ, HH + HQ, CQ, CH + CQ     indicators: of (gA = 1, gB = 2), (gA = 1, gB >= 1), (gA >= 1, gB = 2), (gA >= 1, gB >= 1)
// and a sum's variance is n_pre (second moment - mean^2).  The real counts are sums with both margins fixed, whose spread is smaller, so z
// standard deviations of these are at least z of the real ones.  Where the 5 % of sqrt(bound) of prefix_expected_keeps is many standard
// deviations (long rows) this question drops a pair earlier; where it is few (rows of ~ 140 k samples) the other one does.
// (fine: the carrier form's fixed term with the expected CQ_pre in its min, as the screen of the fine walk has the counted one)
TWK_SCREEN_FN bool prefix_sigma_keeps(const ScreenMargins& m, const SuffixMargins& x, bool two, bool carrier, double n_pre, double two_n, double cut, double z, bool fine = false) {
	if (n_pre <= 0) return true;
	const double ha = (double)(m.hA - x.hA), qa = (double)(m.qA - x.qA), hb = (double)(m.hB - x.hB), qb = (double)(m.qB - x.qB);
	const double a1 = ha / n_pre, a2 = qa / n_pre, b1 = hb / n_pre, b2 = qb / n_pre;
	double mu_lo, m2_lo, mu_hi, m2_hi, hh, fixed;       // s_lo's sum; (s_hi + hh)'s sum; the part of it passed as hh; what the screen adds to s_hi besides
	if (!two) {
		mu_lo = a2 * b1 + a1 * b2 + 2.0 * a2 * b2; m2_lo = mu_lo + 2.0 * a2 * b2;
		mu_hi = mu_lo + a1 * b1; m2_hi = m2_lo + a1 * b1;
		hh = a1 * b1; fixed = prefix_slack(x);
	} else if (!carrier) {
		mu_lo = m2_lo = a1 * b2; mu_hi = m2_hi = a1 * (b1 + b2);
		hh = a1 * b1; fixed = qa + (qa < qb ? qa : qb) + prefix_slack(x);
	} else {
		mu_lo = m2_lo = (a1 + a2) * b2; mu_hi = m2_hi = (a1 + a2) * (b1 + b2);
		hh = (a1 + a2) * b1; fixed = prefix_slack_cq(qa, qb, n_pre * mu_lo, fine) + prefix_slack(x);
	}
	const double v_lo = n_pre * (m2_lo - mu_lo * mu_lo), v_hi = n_pre * (m2_hi - mu_hi * mu_hi);
	const double sd_lo = v_lo > 0 ? __builtin_sqrt(v_lo) : 0.0, sd_hi = v_hi > 0 ? __builtin_sqrt(v_hi) : 0.0;
	const double s_lo = n_pre * mu_lo - z * sd_lo, s_hi = n_pre * (mu_hi - hh) + fixed + z * sd_hi;
	return screen_keeps_between(m, n_pre * hh, s_lo, s_hi, two_n, cut);
}

// The one-product form over the prefix: cc = CC_pre.  T_pre <= CC_pre + min(qa_pre, qb_pre) with the prefix margins, the unread suffix adds
// prefix_slack(x) to the upper end, and S >= 0 as over whole rows.
TWK_SCREEN_FN bool screen1c_prefix_keeps(const ScreenMargins& m, const SuffixMargins& x, uint32_t cc, double two_n, double cut) {
	const double qa = (double)(m.qA - x.qA), qb = (double)(m.qB - x.qB);
	return screen_keeps_between(m, (double)cc, 0.0, (qa < qb ? qa : qb) + prefix_slack(x), two_n, cut);
}
// ... and the planner's two questions for a stop of a one-product launch.  The lower sum is 0 with no spread: the lower test is the exact one,
// outside margin and sigmas.  The upper sum CC_pre is the sum of the indicator (gA >= 1, gB >= 1), as in the carrier branch of prefix_sigma_keeps.
TWK_SCREEN_FN bool prefix_expected_keeps_one(const ScreenMargins& m, const SuffixMargins& x, double n_pre, double two_n, double cut, double margin) {
	if (n_pre <= 0 || !screen1c_lower_ok(m, two_n, cut)) return true;
	const double ha = (double)(m.hA - x.hA), qa = (double)(m.qA - x.qA), hb = (double)(m.hB - x.hB), qb = (double)(m.qB - x.qB);
	const double cc = (ha + qa) * (hb + qb) / n_pre;
	return screen_upper_keeps(m, cc + (qa < qb ? qa : qb) + prefix_slack(x), two_n, cut, margin * margin);
}
TWK_SCREEN_FN bool prefix_sigma_keeps_one(const ScreenMargins& m, const SuffixMargins& x, double n_pre, double two_n, double cut, double z) {
	if (n_pre <= 0 || !screen1c_lower_ok(m, two_n, cut)) return true;
	const double ha = (double)(m.hA - x.hA), qa = (double)(m.qA - x.qA), hb = (double)(m.hB - x.hB), qb = (double)(m.qB - x.qB);
	const double mu = ((ha + qa) / n_pre) * ((hb + qb) / n_pre), v = n_pre * (mu - mu * mu);
	const double sd = v > 0 ? __builtin_sqrt(v) : 0.0;
	return screen_upper_keeps(m, n_pre * mu + (qa < qb ? qa : qb) + prefix_slack(x) + z * sd, two_n, cut);
}

// The grid of stops: PREFIX_COARSE coarse points along a row of nchunks K chunks, prefix_step chunks apart (the option "prefix_stop" counts in
// these), and every coarse interval divided into PREFIX_SUB sub-steps of prefix_substep chunks, clipped at the next coarse point: fine index
// f = PREFIX_SUB g + s stands for the stop min(g step + min(s substep, step), nchunks), and PREFIX_GRID (or any stop of nchunks) for the whole
// row.  The points are not equally spaced (137 chunks: 0, 2, 4, 5, 7, ..: step 5, sub-step 2) and may coincide; they never decrease, and every
// coarse point is one of them.  Stated here once: the screens, the planner, the suffix table (ld_prep.hip.h) and `make prefix-check` all ask this.
constexpr uint32_t PREFIX_COARSE = 32, PREFIX_SUB = 4, PREFIX_GRID = PREFIX_COARSE * PREFIX_SUB;
TWK_SCREEN_FN uint32_t prefix_step(uint32_t nchunks) { return (nchunks + PREFIX_COARSE - 1) / PREFIX_COARSE; }
TWK_SCREEN_FN uint32_t prefix_substep(uint32_t nchunks) { return (prefix_step(nchunks) + PREFIX_SUB - 1) / PREFIX_SUB; }
TWK_SCREEN_FN uint32_t prefix_stop_chunks(uint32_t f, uint32_t nchunks) {
	if (f >= PREFIX_GRID) return nchunks;
	const uint32_t step = prefix_step(nchunks), sub = (f % PREFIX_SUB) * prefix_substep(nchunks);
	const unsigned long long s = (unsigned long long)(f / PREFIX_SUB) * step + (sub < step ? sub : step);
	return s >= nchunks ? nchunks : (uint32_t)s;
}

}  // namespace twk
