// Haplotype blocks (Gabriel et al. 2002): what the kernels of ld_blocks.hip.h and the host check (csrc/tools/blocks_check.cpp,
// `make blocks-check`) share - the confidence bounds of a pair's D', the classes of a pair, the rule by which a candidate qualifies,
// and the sort key of the qualifying candidates.  Plain C++ with no HIP in it.
//
// THE BOUNDS.  Over the record's cnt[0..3] = (n11, nX, nY, n22) - doubles, fractional in unphased mode:
//   neg  = n11*n22 < nX*nY                                  two IEEE products, one comparison
//   (m11, m12, m21, m22) = neg ? (nX, n11, n22, nY) : (n11, nX, nY, n22)      one variant's alleles flipped so that D >= 0
//   T  = (m11 + m22) + (m12 + m21)
//   pA = (m11+m12)/T   qA = (m21+m22)/T   pB = (m11+m21)/T   qB = (m12+m22)/T
//   dmax = min(pA*qB, qA*pB)
//   for i in 0..100:  d = (i / 100.0) * dmax
//       f11 = max(pA*pB + d, 1e-10)   f22 = max(qA*qB + d, 1e-10)   f12 = max(pA*qB - d, 1e-10)   f21 = max(qA*pB - d, 1e-10)
//       L[i] = (m11*log f11 + m22*log f22) + (m12*log f12 + m21*log f21)
//   w[i] = exp(L[i] - max L);  total = w[0] + w[1] + ... in this order;  thr = 0.05 * total
//   lo = max(i_up - 1, 0),     i_up   = the first i from 0 upwards   whose running sum w[0..i]   > thr
//   hi = min(i_down + 1, 100), i_down = the first i from 100 downwards whose running sum w[100..i] > thr
// The grouping of the sums makes the result the same whichever of the two variants is "A": swapping them swaps m12 with m21, pA with
// pB and qA with qB, and every expression above is symmetric under that - a regrouped plane set hands a pair over in either order.
// No case is special: with dmax == 0 every L[i] is the same, every w[i] is 1, thr = 5.05, and the scans give lo = 4, hi = 96.
//
// NO ARRAY.  A lane of the kernel has no room for L[101]: bc_bounds recomputes L[i] where it needs it - one pass for the maximum, one for
// the total, and the two scans, each of which stops at its crossing.  L[i] is a pure function of i and seven doubles, so every pass
// sees the same bits, and the result is the definition's.  The products and sums must stay separate roundings (a fused multiply-add
// would break the symmetry between A and B): the engine builds with -ffp-contract=off and the functions say so themselves.
//
// THE CLASSES of an informative pair, by its two bytes: STRONG at a cut c: lo >= c && hi >= strong_hi; RECOMBINANT: hi < recomb_hi.
// A slot without a record holds BC_NONE in both bytes and is in no class.
//
// A CANDIDATE (i, j), m = j - i + 1 markers, sep = pos[j] - pos[i], with s strong pairs at ITS cut (bc_cut) and r recombinant pairs
// among the informative pairs inside [i, j], qualifies by bc_qualifies.  The qualifying candidates are visited in order of sep
// descending, then m descending, then i ascending: ascending order of bc_key, whose three fields are sized by the call (BlockKey).
#pragma once
#include <math.h>
#include <stdint.h>
#include "ld_bandmat_index.h"

namespace twk {

constexpr uint8_t BC_NONE = 255;                     // both bytes of a slot without a record, and of the diagonal
constexpr int BC_POINTS = 101;                       // the grid of D' values: 0, 0.01, .. 1
constexpr double BC_FLOOR = 1e-10;                   // the smallest haplotype frequency a logarithm is taken of
constexpr double BC_TAIL = 0.05;                     // the mass outside the bounds, each side

// The table with D >= 0 and its margins.
struct BcTable { double m11, m12, m21, m22, pA, qA, pB, qB, dmax; };

TWK_MX_FN BcTable bc_table(double n11, double nX, double nY, double n22) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	BcTable t;
	const double d1 = n11 * n22, d2 = nX * nY;
	const bool neg = d1 < d2;
	t.m11 = neg ? nX : n11; t.m12 = neg ? n11 : nX; t.m21 = neg ? n22 : nY; t.m22 = neg ? nY : n22;
	const double T = (t.m11 + t.m22) + (t.m12 + t.m21);
	t.pA = (t.m11 + t.m12) / T; t.qA = (t.m21 + t.m22) / T; t.pB = (t.m11 + t.m21) / T; t.qB = (t.m12 + t.m22) / T;
	const double x = t.pA * t.qB, y = t.qA * t.pB;
	t.dmax = x < y ? x : y;
	return t;
}

TWK_MX_FN double bc_floor(double f) { return f > BC_FLOOR ? f : BC_FLOOR; }

// L[i]: the log likelihood of the table at D' = i / 100.
TWK_MX_FN double bc_loglik(const BcTable& t, int i) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	const double d = ((double)i / 100.0) * t.dmax;
	const double pp = t.pA * t.pB, qq = t.qA * t.qB, pq = t.pA * t.qB, qp = t.qA * t.pB;
	const double f11 = bc_floor(pp + d), f22 = bc_floor(qq + d), f12 = bc_floor(pq - d), f21 = bc_floor(qp - d);
	const double a = t.m11 * log(f11), b = t.m22 * log(f22), c = t.m12 * log(f12), e = t.m21 * log(f21);
	return (a + b) + (c + e);
}

// lo, hi of the table (0..100 each).
TWK_MX_FN void bc_bounds(double n11, double nX, double nY, double n22, uint32_t* lo, uint32_t* hi) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	const BcTable t = bc_table(n11, nX, nY, n22);
	double top = bc_loglik(t, 0);
	for (int i = 1; i < BC_POINTS; ++i) { const double l = bc_loglik(t, i); top = l > top ? l : top; }
	double total = 0.0;
	for (int i = 0; i < BC_POINTS; ++i) total = total + exp(bc_loglik(t, i) - top);
	const double thr = BC_TAIL * total;
	// (a running sum that never exceeds thr - a NaN in the table - leaves the scans at their far ends: 99 and 1, no store out of range)
	int up = 0; double run = 0.0;
	for (; up < BC_POINTS - 1; ++up) { run = run + exp(bc_loglik(t, up) - top); if (run > thr) break; }
	int down = BC_POINTS - 1; run = 0.0;
	for (; down > 0; --down) { run = run + exp(bc_loglik(t, down) - top); if (run > thr) break; }
	*lo = (uint32_t)(up > 0 ? up - 1 : 0);
	*hi = (uint32_t)(down < BC_POINTS - 1 ? down + 1 : BC_POINTS - 1);
}

// ---- the blocks ----
constexpr uint32_t BLOCK_NONE = 0xFFFFFFFFu;         // TWK_HIP_NO_BLOCK
constexpr uint32_t BLOCK_MAX_BAND = 65535;           // the widest band row a call accepts: s + r < 2^31 and m in 16 bits

struct BlockParams {                                 // twk_hip_block_params, field for field
	uint32_t strong_lo, strong_hi, recomb_hi, strong_lo_2, strong_lo_34, inform_permille, max_span_2, max_span_3;
};
constexpr BlockParams BLOCK_DEFAULTS{70, 98, 90, 80, 50, 950, 20000, 30000};

TWK_MX_FN bool bc_params_ok(const BlockParams& p) {
	return p.strong_lo <= 100 && p.strong_hi <= 100 && p.recomb_hi <= 100 && p.strong_lo_2 <= 100 && p.strong_lo_34 <= 100 &&
	       p.recomb_hi <= p.strong_hi && p.inform_permille <= 1000;
}

TWK_MX_FN bool bc_informative(uint32_t lo) { return lo != BC_NONE; }
TWK_MX_FN bool bc_strong(uint32_t lo, uint32_t hi, uint32_t cut, uint32_t strong_hi) { return lo != BC_NONE && lo >= cut && hi >= strong_hi; }
TWK_MX_FN bool bc_recomb(uint32_t lo, uint32_t hi, uint32_t recomb_hi) { return lo != BC_NONE && hi < recomb_hi; }
// The cut-off of lo for the pairs inside a candidate of m markers.
TWK_MX_FN uint32_t bc_cut(const BlockParams& p, uint32_t m) { return m == 2 ? p.strong_lo_2 : m <= 4 ? p.strong_lo_34 : p.strong_lo; }
// A candidate of m markers spanning sep base pairs with s strong (at its cut) and r recombinant pairs inside it.
TWK_MX_FN bool bc_qualifies(const BlockParams& p, uint32_t m, uint32_t sep, uint32_t s, uint32_t r) {
	if (m == 2 && sep > p.max_span_2) return false;
	if (m == 3 && sep > p.max_span_3) return false;
	const uint32_t need = m == 2 ? 1u : m == 3 ? 3u : 6u;
	if (s + r < need) return false;
	return (uint64_t)s * 1000u > (uint64_t)p.inform_permille * (s + r);
}

// The sort key: (sep_max - sep, m_max - m, i) in bits_sep, bits_m and bits_i bits, the first the most significant.
struct BlockKey { uint32_t sep_max, m_max, bits_m, bits_i; };
TWK_MX_FN uint32_t bc_bits(uint64_t max_value) { uint32_t b = 1; while (b < 64 && (max_value >> b)) ++b; return b; }
// -> false if the three fields do not fit 64 bits.  n: the slice's variants; m_max: its widest band row; sep_max: the window.
TWK_MX_FN bool bc_key_layout(uint32_t n, uint32_t m_max, uint32_t sep_max, BlockKey* k, uint32_t* total_bits) {
	k->sep_max = sep_max; k->m_max = m_max; k->bits_m = bc_bits(m_max); k->bits_i = bc_bits(n ? n - 1 : 0);
	*total_bits = bc_bits(sep_max) + k->bits_m + k->bits_i;
	return *total_bits <= 64;
}
TWK_MX_FN uint64_t bc_key(const BlockKey& k, uint32_t sep, uint32_t m, uint32_t i) {
	return ((uint64_t)(k.sep_max - sep) << k.bits_m | (uint64_t)(k.m_max - m)) << k.bits_i | i;
}
TWK_MX_FN uint32_t bc_key_i(const BlockKey& k, uint64_t key) { return (uint32_t)(key & ((1ull << k.bits_i) - 1)); }
TWK_MX_FN uint32_t bc_key_m(const BlockKey& k, uint64_t key) { return k.m_max - (uint32_t)(key >> k.bits_i & ((1ull << k.bits_m) - 1)); }

// The finished band and what the blocks' kernels derive from it.
struct BlocksBand {
	const uint8_t* lo; const uint8_t* hi;
	const BandRow* rows;
	const uint32_t* pos;                // [n]: the positions of the slice's variants
	uint32_t* ps; uint32_t* pr;         // [row_ptr[n]]: the rows' inclusive prefix counts of STRONG at strong_lo and of RECOMBINANT
	uint32_t n;
	BlockParams par;
	BlockKey key;
};

// k_blocks_prefix, one lane: the set bits of a 64-column ballot up to and including this lane's.
TWK_MX_FN uint32_t bc_prefix_in_ballot(unsigned long long ballot, uint32_t lane) {
	const unsigned long long upto = lane == 63 ? ~0ull : (2ull << lane) - 1;
	return (uint32_t)__builtin_popcountll(ballot & upto);
}

// The bytes of the pair (x, y); 255 / 255 where y is not in x's band.
TWK_MX_FN void bc_pair_bytes(const BlocksBand& b, uint32_t x, uint32_t y, uint32_t* lo, uint32_t* hi) {
	const BandRow rx = b.rows[x];
	*lo = BC_NONE; *hi = BC_NONE;
	if (bm_in_band(y, rx.first, rx.len)) { const uint64_t at = bm_slot(rx.base, rx.first, y); *lo = b.lo[at]; *hi = b.hi[at]; }
}

// k_blocks_candidates, one thread: first variant i walks j upwards through its band and carries s (strong at strong_lo) and r as running
// sums - s(i, j) = s(i, j - 1) + the column sum of j over the rows i .. j - 1, one subtraction of row j's prefix counts.  A candidate
// of up to 4 markers takes its s from its at most 6 pairs at its own cut.  counts (EMIT false): {qualifying candidates, candidates,
// informative pairs (i, j > i)}.  EMIT true: key, slot, s and r of its qualifying candidates from slot `at` on, below `capacity`.
template <bool EMIT>
TWK_MX_FN void bc_candidates_of(const BlocksBand& b, uint32_t i, uint32_t* counts, uint32_t at, uint32_t capacity,
                                unsigned long long* keys, uint32_t* vals, uint32_t* cs, uint32_t* cr) {
	const BandRow ri = b.rows[i];
	const uint32_t end = ri.first + ri.len;                  // (the band holds the diagonal: end > i)
	const uint32_t pi = b.pos[i];
	uint32_t s = 0, r = 0, n_q = 0, n_c = 0, n_inf = 0;
	for (uint32_t j = i + 1; j < end && j < b.n; ++j) {
		// the column sums of j over the rows i .. j - 1 (the diagonal slot is in no class)
		const BandRow rj = b.rows[j];
		if (!bm_in_band(i, rj.first, rj.len)) break;         // (the band is symmetric: a bound, not a case)
		const uint64_t dj = bm_slot(rj.base, rj.first, j);
		uint32_t s_col = b.ps[dj], r_col = b.pr[dj];
		if (i > rj.first) { const uint64_t before = bm_slot(rj.base, rj.first, i - 1); s_col -= b.ps[before]; r_col -= b.pr[before]; }
		s += s_col; r += r_col;
		const uint64_t ij = bm_slot(ri.base, ri.first, j);
		const uint32_t lo = b.lo[ij], hi = b.hi[ij];
		if (!bc_informative(lo)) continue;
		++n_inf;
		if (!bc_strong(lo, hi, b.par.strong_lo, b.par.strong_hi)) continue;
		++n_c;
		const uint32_t m = j - i + 1, sep = b.pos[j] - pi;
		uint32_t s_m = s;
		if (m <= 4) {                                        // its own cut: from its at most 6 pairs
			const uint32_t cut = bc_cut(b.par, m);
			s_m = 0;
			for (uint32_t x = i; x < j; ++x)
				for (uint32_t y = x + 1; y <= j; ++y) {
					uint32_t l2, h2;
					bc_pair_bytes(b, x, y, &l2, &h2);
					s_m += bc_strong(l2, h2, cut, b.par.strong_hi) ? 1u : 0u;
				}
		}
		if (!bc_qualifies(b.par, m, sep, s_m, r)) continue;
		++n_q;
		if (EMIT) {
			if (at < capacity) { keys[at] = bc_key(b.key, sep, m, i); vals[at] = at; cs[at] = s_m; cr[at] = r; }
			++at;
		}
	}
	if (!EMIT) { counts[0] = n_q; counts[1] = n_c; counts[2] = n_inf; }
}

// k_blocks_walk: the bits of the variants i .. j that fall into word w of `used` (i >> 6 <= w <= j >> 6).
TWK_MX_FN unsigned long long bc_range_bits(uint32_t w, uint32_t i, uint32_t j) {
	unsigned long long bits = ~0ull;
	if (w == i >> 6) bits &= ~0ull << (i & 63);
	if (w == j >> 6) bits &= ~0ull >> (63 - (j & 63));
	return bits;
}
// ... and whether a candidate is taken as a block: neither end in an earlier one.
TWK_MX_FN bool bc_ends_free(const unsigned long long* used, uint32_t i, uint32_t j) {
	return !(used[i >> 6] >> (i & 63) & 1) && !(used[j >> 6] >> (j & 63) & 1);
}

}  // namespace twk
