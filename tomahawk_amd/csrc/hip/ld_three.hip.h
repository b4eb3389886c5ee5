// The three-product form of UnphasedMath's contraction (ld_count.hip.h: contract3_half, StoreCounts3, ScreenCountsUnphased<TB, true>)
// leaves (HH, S) per variant pair.  This header holds what follows it:
//   k_screen3_pairs     the r2 screen over an (HH, S) count matrix (long rows, where tiles are split along K), or over the (HH, HQ) matrix
//                       of the two-product form (k_screen2_pairs; rows whose hom-alt carriers are few: ld_two_screen.h)
//   k_recount_unphased  the four products HH, HQ, QH, QQ of the pairs that passed, counted afresh from their plane rows
// The candidates then go through k_ld_stats_list_unphased (ld_math.hip.h) like those of the four-product fused form.
// Reference shape: UnphasedMath reads the 3 x 3 table only through n11, the double hets and the margins before its cubic
// (lib/ld/ld_engine.cpp:1334-1375); PhasedListVector counts one cell and derives the rest (ld_engine.cpp:244-246).
#pragma once
#include "ld_count.hip.h"
#include "ld_math.hip.h"
#include "ld_two_screen.h"

namespace twk {

// ---- the three-product form's screen over a count matrix (long rows: tiles split along K, counts added into C) ----
// One thread per variant pair of the super-tile: (HH, S) from the matrix StoreCounts3 wrote, the row margins, and the test of
// ScreenCountsUnphased (same doubles, same order - but for the column variant's dosage, which is read here as the integer it is and
// there from the prefilter's float term: the same number below 2^24 alleles); a pair that passes becomes a candidate (A, B, HH, S, -, -) in the
// launch's list, appended with one atomic per block.  Structural tests as in the fused epilogue (the list math checks them again).
// TWO: the matrix is that of a two-product launch (k_count_list_t over the row variants' H planes against the column variants' H and Q
// rows: (HH, HQ) where the three-product form leaves (HH, S), same layout), the test screen2_keeps - the same doubles with S_lo = HQ and
// S_hi = HQ + qA + min(qA, qB) in S's place (ld_two_screen.h) - and a candidate is (A, B, HH, HQ, -, -).  ScreenWork::carrier: the row operand was
// the carrier plane H | Q, the matrix holds (CH, CQ) in the same layout and the test is screen2c_keeps; a candidate is (A, B, CH, CQ, -, -).
// ONE (k_screen1_pairs; ScreenWork::carrier == 2): the matrix is that of a one-product launch - k_count_list_t over the carrier rows of both axes, one
// count CC = popc(C_A & C_B) per pair, ldc = columns, a tile 128 x 128 variants - the test screen1c_keeps and a candidate (A, B, CC, 0, stop, -).
// ScreenWork::uz (three products only): the launch ran in the (U, Z) form (ld_count_uz.hip.h) - (HH, S) from (U, Z) and the margins of the range the
// tile was contracted over, in integers, before any test (ld_two_screen.h: uz_to_hh_s); candidates, recount and list math see no difference.
constexpr int SCREEN3_THREADS = 256;
template <bool TWO, bool ONE = false>
__device__ __forceinline__ void screen_pairs_body(const ScreenWork* __restrict__ sp, const StatsParams* __restrict__ pp, const uint32_t* __restrict__ C, uint32_t ldc) {
	const ScreenWork& s = *sp;
	const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
	const uint32_t vA = s.a0 + i, vB = s.b0 + j;
	bool ok = i < s.nA && j < s.nB && vA < s.n_variants && vB < s.n_variants && (!s.diag || vB > vA);
	if (ok && s.col_hi) { const uint32_t k = vA - s.hi_a0; ok = vB < s.hi_b0 + s.col_hi[k < s.hi_n ? k : s.hi_n - 1]; }
	if (ok && s.col_lo) { const uint32_t k = vA - s.hi_a0; ok = vB >= s.hi_b0 + s.col_lo[k < s.hi_n ? k : s.hi_n - 1]; }      // (a launch behind a staircase: nothing in front of it was contracted)
	if (ok && ((vA < s.list_zone && vB < s.list_zone) || vA < s.probe_zone)) ok = false;
	if (ok && (pp->window & TWK_HIP_OPT_WINDOW)) {      // window mode: only the tiles some row can reach were contracted - the exact test of d_pair, so that
		const StatsParams& p = *pp;                     // nothing is read from a tile that holds no counts
		const uint32_t A = p.tv.ids ? p.tv.ids[vA] : vA, B = p.tv.ids ? p.tv.ids[vB] : vB;
		const int64_t d = (int64_t)p.vm.pos[A] - (int64_t)p.vm.pos[B];
		if (p.vm.rid[A] != p.vm.rid[B] || (d < 0 ? -d : d) > (int64_t)p.l_window) ok = false;
	}
	uint32_t hh = 0, s_sum = 0, stop = 0;      // stop: the chunks the pair's counts cover (0: the whole rows)
	if (ok) {
		if (ONE) hh = C[(size_t)i * ldc + j];
		else { const uint2 hs = *reinterpret_cast<const uint2*>(C + (size_t)i * ldc + 2 * j); hh = hs.x; s_sum = hs.y; }
		const ScreenMargins m{s.rowpop[2 * vA], s.rowpop[2 * vA + 1], s.rowpop[2 * vB], s.rowpop[2 * vB + 1]};
		bool uz = !TWO && s.uz != 0;      // the counts read are (U, Z): converted once, below, with the margins of the range they cover
		// a prefix launch: the pair's tile was contracted over the chunks [0, stop) only - the counts are the prefix's, and the
		// unread part of the two rows is bounded by its margins (ld_two_screen.h)
		if (s.pre_stops) {
			const uint32_t g = s.pre_stops[(size_t)(i / s.pre_tvA) * s.pre_gx + j / (ONE ? TILE : TILE / 2)];
			const uint32_t st = prefix_stop_chunks(g, s.pre_nchunks);
			if (st < s.pre_nchunks) {
				stop = st;
				// (grid-major: the row variant's two margins are one address a wave, the column variants' two a lane lie side by side)
				const uint32_t* fG = s.pre_suffix + (size_t)g * s.pre_rows;
				const uint2 xA = *reinterpret_cast<const uint2*>(fG + 2 * (size_t)vA), xB = *reinterpret_cast<const uint2*>(fG + 2 * (size_t)vB);
				const SuffixMargins x{xA.x, xA.y, xB.x, xB.y};
				if (uz) { const CountsHS hs = uz_prefix_to_hh_s(m, x, hh, s_sum); hh = hs.hh; s_sum = hs.s; uz = false; }      // (U, Z) of the prefix -> its (HH, S)
				ok = ONE ? screen1c_prefix_keeps(m, x, hh, s.two_n, s.cut)
				   : TWO ? (s.carrier ? screen2c_prefix_keeps(m, x, hh, s_sum, s.two_n, s.cut, s.fine != 0) : screen2_prefix_keeps(m, x, hh, s_sum, s.two_n, s.cut))
				         : screen3_prefix_keeps(m, x, hh, s_sum, s.two_n, s.cut);
			}
		}
		if (uz) { const CountsHS hs = uz_to_hh_s(m, hh, s_sum); hh = hs.hh; s_sum = hs.s; }      // (U, Z) of the whole rows -> (HH, S)
		if (!stop) ok = ONE ? screen1c_keeps(m, hh, s.two_n, s.cut) : TWO ? (s.carrier ? screen2c_keeps(m, hh, s_sum, s.two_n, s.cut, s.fine != 0) : screen2_keeps(m, hh, s_sum, s.two_n, s.cut)) : screen3_keeps(m, hh, s_sum, s.two_n, s.cut);
	}
	__shared__ uint32_t wave_n[SCREEN3_THREADS / 64];
	__shared__ unsigned long long block_base;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const unsigned long long ballot = __ballot(ok);
	if (lane == 0) wave_n[wave] = (uint32_t)__popcll(ballot);
	__syncthreads();
	if (threadIdx.x == 0) {
		uint32_t total = 0;
		for (int k = 0; k < SCREEN3_THREADS / 64; ++k) total += wave_n[k];
		block_base = total ? atomicAdd(s.n_cand, (unsigned long long)total) : 0ull;
	}
	__syncthreads();
	if (ok) {
		unsigned long long slot = block_base;
		for (int k = 0; k < wave; ++k) slot += wave_n[k];
		slot += (unsigned long long)__popcll(ballot & ((1ull << lane) - 1));
		if (slot < s.cap) {
			uint32_t* e = s.cand + slot * 6;
			e[0] = vA; e[1] = vB; e[2] = hh; e[3] = TWO ? s_sum : 0; e[4] = stop; e[5] = TWO ? 0 : s_sum;
		}
	}
}

__global__ __launch_bounds__(SCREEN3_THREADS)
void k_screen3_pairs(const ScreenWork* __restrict__ sp, const StatsParams* __restrict__ pp, const uint32_t* __restrict__ C, uint32_t ldc) { screen_pairs_body<false>(sp, pp, C, ldc); }
__global__ __launch_bounds__(SCREEN3_THREADS)
void k_screen2_pairs(const ScreenWork* __restrict__ sp, const StatsParams* __restrict__ pp, const uint32_t* __restrict__ C, uint32_t ldc) { screen_pairs_body<true>(sp, pp, C, ldc); }
__global__ __launch_bounds__(SCREEN3_THREADS)
void k_screen1_pairs(const ScreenWork* __restrict__ sp, const StatsParams* __restrict__ pp, const uint32_t* __restrict__ C, uint32_t ldc) { screen_pairs_body<true, true>(sp, pp, C, ldc); }

// ---- the candidates' four products --------------------------------------------------------------------------------------
// The three-product forms hand over (A, B, HH, S); UnphasedMath needs HH, HQ, QH and QQ.  LANES lanes per candidate (64 for
// long rows, 16 - one DPP row - for rows of a few hundred words) stream the four plane rows of the pair with 16-byte loads
// and count all four products afresh - nothing of the three-product contraction is reused, so a record is exactly what
// the four-product form would have made it.  The few candidates of a default run (r2 >= 0.1: pairs in real LD) cost nothing
// next to the contraction; the host stops using the three-product forms when a launch's candidates are too many for that to
// hold (Launch::too_rich -> ld_form.h: CallForms::gave_up).  The recount also proves the contraction, always: a candidate whose (HH, S) disagree with its
// own four products is counted in *mismatches, and the host fails the call on it.  two != 0: the candidates are a two-product launch's,
// (A, B, HH, HQ) - the proof is then that both products equal their recount.  two == 2: the launch's row operand was the carrier plane, the
// candidates are (A, B, CH, CQ), and the proof compares them with HH + QH and HQ + QQ of the recount; the records are the four products' as ever.
// two == 3: a one-product launch's candidates (A, B, CC, 0): the proof compares CC with HH + QH + HQ + QQ over the chunks the contraction read.
template <int LANES>
__global__ __launch_bounds__(256)
void k_recount_unphased(const uint32_t* __restrict__ rows, uint32_t W, uint32_t W_live, uint32_t* __restrict__ cand,
                        const unsigned long long* __restrict__ n_cand, unsigned long long cap, unsigned long long* __restrict__ mismatches, int two, int prefix) {
	static_assert(LANES == 64 || LANES == 16, "a wave or a DPP row per candidate");
	const unsigned long long n = *n_cand;
	if (n > cap) return;                                    // the list overflowed: the host redoes the launch with four products, nothing of this one is kept
	const uint32_t lane = threadIdx.x & (LANES - 1);
	const unsigned long long group = ((unsigned long long)blockIdx.x * blockDim.x + threadIdx.x) / LANES;
	const unsigned long long n_groups = (unsigned long long)gridDim.x * blockDim.x / LANES;
	const uint32_t W4 = (W_live + 3) / 4;                 // 16-byte pieces of a row that carry data (rows are padded with zeros to W, a multiple of 32 words)
	for (unsigned long long k = group; k < n; k += n_groups) {
		uint32_t* e = cand + 6 * k;
		const uint32_t sA = e[0], sB = e[1];
		if (sA == CAND_UNUSED) continue;                    // (uniform over the candidate's lanes)
		const uint4* hA = reinterpret_cast<const uint4*>(rows + (size_t)(2 * sA) * W);
		const uint4* qA = reinterpret_cast<const uint4*>(rows + (size_t)(2 * sA + 1) * W);
		const uint4* hB = reinterpret_cast<const uint4*>(rows + (size_t)(2 * sB) * W);
		const uint4* qB = reinterpret_cast<const uint4*>(rows + (size_t)(2 * sB + 1) * W);
		uint32_t hh = 0, hq = 0, qh = 0, qq = 0;
		// a prefix launch's candidate carries the stop of its tile in e[4] (0: whole rows): the contraction counted the 16-byte pieces [0, pre4) only,
		// and it is their sums the proof below compares - the records come from the totals
		const uint32_t pre4 = (prefix && e[4]) ? (e[4] * (uint32_t)(KC / 4) < W4 ? e[4] * (uint32_t)(KC / 4) : W4) : W4;
		uint32_t p_hh = 0, p_s = 0;             // the prefix's HH, and its S (HQ of a two-product launch)
		for (uint32_t p = lane; p < W4; p += LANES) {
			const uint4 a = hA[p], b = qA[p], x = hB[p], y = qB[p];
			const uint32_t d_hh = __popc(a.x & x.x) + __popc(a.y & x.y) + __popc(a.z & x.z) + __popc(a.w & x.w);
			const uint32_t d_hq = __popc(a.x & y.x) + __popc(a.y & y.y) + __popc(a.z & y.z) + __popc(a.w & y.w);
			const uint32_t d_qh = __popc(b.x & x.x) + __popc(b.y & x.y) + __popc(b.z & x.z) + __popc(b.w & x.w);
			const uint32_t d_qq = __popc(b.x & y.x) + __popc(b.y & y.y) + __popc(b.z & y.z) + __popc(b.w & y.w);
			hh += d_hh; hq += d_hq; qh += d_qh; qq += d_qq;
			if (p < pre4) {
				if (two == 3) p_hh += d_hh + d_qh + d_hq + d_qq;                // the two carrier planes' product: CC = CH + CQ (p_s stays 0, as the candidate's)
				else if (two == 2) { p_hh += d_hh + d_qh; p_s += d_hq + d_qq; }      // the carrier plane's products: CH = HH + QH, CQ = HQ + QQ
				else { p_hh += d_hh; p_s += two ? d_hq : d_qh + d_hq + 2u * d_qq; }
			}
		}
#pragma unroll
		for (int d = 1; d < LANES; d <<= 1) {
			hh += __shfl_xor(hh, d, LANES); hq += __shfl_xor(hq, d, LANES); qh += __shfl_xor(qh, d, LANES); qq += __shfl_xor(qq, d, LANES);
			p_hh += __shfl_xor(p_hh, d, LANES); p_s += __shfl_xor(p_s, d, LANES);
		}
		if (lane == 0) {
			if (mismatches && (e[2] != p_hh || (two ? e[3] != p_s : e[5] != p_s))) atomicAdd(mismatches, 1ull);      // the contraction's (HH, S) - (HH, HQ) - against the recount
			e[2] = hh; e[3] = hq; e[4] = qh; e[5] = qq;
		}
	}
}

}  // namespace twk
