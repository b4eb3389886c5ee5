// LD splitting, the parts that are plain C++ (csrc/hip/ld_split_index.h), played on the host: `make split-check` builds this file with
// g++ under AddressSanitizer and UBSan and runs it.  Per case - a random band over n variants, a triple (min_size, max_size, k_max) -
// every lane of every kernel of ld_split.hip.h goes through its steps with arrays that check their bounds and count their writes:
//   the prefixes   a wave per row, 64 offsets a step, the inclusive scan by six shifted additions and the carry - Rp at sp_rp_slot for
//                  j <= upc and nowhere else, each slot once, and the row's total over its whole band;
//   the sums       sp_block_sums_of per b, the saturation rule deciding which stored prefix a lane loads - W against the sum of q over
//                  the pairs inside [b - d, b), each slot of min_size <= d <= min(max_size, b) once;
//   the layers     per k the blocks of 256 b, sp_block_d_range, the windows of SPLIT_WINDOW_D, the stage (every entry the lanes read
//                  lies inside it; what lies outside the previous layer's range is never loaded), sp_lane_window - G and D against
//                  the recurrence evaluated directly over all d, and a d outside the block's range never meets a feasible G;
//   the backtrack  sp_backtrack per K against the chain of the direct D, and for small n against an enumeration of all partitions.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../hip/ld_split_index.h"

using namespace twk;

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return rng_state >> 17; }

// An array that counts the writes of every slot; at() checks the bounds, ASan the rest.
template <class T>
struct Counted {
	std::vector<T> v; std::vector<uint32_t> writes;
	explicit Counted(size_t items) : v(items), writes(items, 0) {}
	void put(uint64_t at, T x) { v.at(at) = x; ++writes.at(at); }
	T get(uint64_t at, long* bad) const { if (!writes.at(at)) ++*bad; return v.at(at); }      // a read of a slot nobody wrote is bad
};

struct Case {
	uint32_t n, min_size, max_size, k_max;
	std::vector<uint32_t> first, len;             // the band rows (the diagonal inside)
	std::vector<std::vector<float>> row;          // row[u][v - first[u]]
	long long q(uint32_t u, uint32_t v) const { return v - first[u] < len[u] ? xs_quantise((double)row[u][v - first[u]]) : 0; }
};

// A band as a window over sorted positions makes it: first and first + len never decrease, symmetric.  kind 0: random values with many
// ties, 1: all zero, 2: all equal, 3: random floats.
Case make_case(uint32_t n, uint32_t reach, int kind, uint32_t min_size, uint32_t max_size, uint32_t k_max) {
	Case c{n, min_size, max_size, k_max, {}, {}, {}};
	std::vector<uint32_t> pos(n);
	uint32_t p = 0;
	for (uint32_t u = 0; u < n; ++u) { p += 1 + (uint32_t)(rnd() % 5); pos[u] = p; }
	const uint32_t w = reach * 3;
	c.first.resize(n); c.len.resize(n); c.row.resize(n);
	for (uint32_t u = 0; u < n; ++u) {
		uint32_t lo = u, hi = u;
		while (lo > 0 && pos[u] - pos[lo - 1] <= w) --lo;
		while (hi + 1 < n && pos[hi + 1] - pos[u] <= w) ++hi;
		c.first[u] = lo; c.len[u] = hi - lo + 1;
		c.row[u].assign(c.len[u], 0.0f);
	}
	for (uint32_t u = 0; u < n; ++u)
		for (uint32_t v = u; v < c.first[u] + c.len[u]; ++v) {
			float x = 0.0f;
			if (kind == 0) x = (float)(rnd() % 3) * 0.25f;
			else if (kind == 2) x = 0.5f;
			else if (kind == 3) x = (float)((double)(rnd() % (1u << 24)) / (double)(1u << 24));
			if (u == v) x = 1.0f;
			c.row[u][v - c.first[u]] = x;
			c.row[v][u - c.first[v]] = x;
		}
	return c;
}

long play(const Case& c) {
	long bad = 0;
	const uint32_t n = c.n, mn = c.min_size, mx = c.max_size, kmax = c.k_max;
	if (!sp_sizes_ok(n, mn, mx, kmax)) return 1;
	// ---- the definition, directly ----
	std::vector<std::vector<long long>> Q(n, std::vector<long long>(n, 0));
	for (uint32_t u = 0; u < n; ++u) for (uint32_t v = u + 1; v < n; ++v) Q[u][v] = c.q(u, v);
	// within(a, b) for all a <= b by columns: within(a, b + 1) = within(a, b) + sum of Q[u][b] over a <= u < b
	std::vector<std::vector<long long>> within(n + 1, std::vector<long long>(n + 1, 0));
	for (uint32_t b = 0; b < n; ++b) {
		long long col = 0;                                    // Q[a][b] + .. + Q[b - 1][b], a descending
		for (uint32_t a = b + 1; a-- > 0;) {
			if (a < b) col += Q[a][b];
			within[a][b + 1] = within[a][b] + col;
		}
	}
	long long T = within[0][n];
	std::vector<std::vector<long long>> G(kmax + 1, std::vector<long long>(n + 1, SPLIT_INFEASIBLE));
	std::vector<std::vector<uint32_t>> D(kmax + 1, std::vector<uint32_t>(n + 1, 0));
	G[0][0] = 0;
	for (uint32_t k = 1; k <= kmax; ++k)
		for (uint32_t b = 1; b <= n; ++b)
			for (uint32_t d = mn; d <= std::min(mx, b); ++d) {
				if (G[k - 1][b - d] < 0) continue;
				const long long cand = G[k - 1][b - d] + within[b - d][b];
				if (cand > G[k][b]) { G[k][b] = cand; D[k][b] = d; }
			}
	// ---- k_split_prefix ----
	std::vector<uint32_t> upc(n);
	uint32_t widest = 1;
	for (uint32_t u = 0; u < n; ++u) { upc[u] = sp_upc(sp_upper(c.first[u], c.len[u], u), mx); widest = std::max(widest, upc[u]); }
	Counted<long long> rp((size_t)widest * n);
	std::vector<long long> row_total(n, -7);
	for (uint32_t u = 0; u < n; ++u) {
		const uint32_t upper = sp_upper(c.first[u], c.len[u], u), keep = upc[u];
		if (c.first[u] > u || upper >= c.len[u]) { ++bad; continue; }
		long long carry = 0;
		for (uint32_t j0 = 1; j0 <= upper; j0 += 64) {
			long long x[64];
			for (uint32_t lane = 0; lane < 64; ++lane) {
				const uint32_t j = j0 + lane;
				x[lane] = j <= upper ? xs_quantise((double)c.row[u].at((u - c.first[u]) + j)) : 0;
			}
			for (unsigned delta = 1; delta < 64; delta <<= 1) {
				long long below[64];
				for (uint32_t lane = 0; lane < 64; ++lane) below[lane] = lane >= delta ? x[lane - delta] : x[lane];      // (__shfl_up: a lane below delta gets its own)
				for (uint32_t lane = 0; lane < 64; ++lane) if (lane >= delta) x[lane] += below[lane];
			}
			for (uint32_t lane = 0; lane < 64; ++lane) {
				x[lane] += carry;
				const uint32_t j = j0 + lane;
				if (j <= keep) rp.put(sp_rp_slot(j, u, n), x[lane]);
			}
			carry = x[63];
		}
		row_total[u] = carry;
	}
	long long total = 0;
	for (uint32_t u = 0; u < n; ++u) {
		long long run = 0, all = 0;
		for (uint32_t v = u + 1; v < n; ++v) all += Q[u][v];
		if (row_total[u] != all) ++bad;
		total += row_total[u];
		for (uint32_t j = 1; j <= widest; ++j) {
			if (u + j < n) run += Q[u][u + j];
			const uint32_t wr = rp.writes[sp_rp_slot(j, u, n)];
			if (wr != (j <= upc[u] ? 1u : 0u)) ++bad;
			if (j <= upc[u] && rp.v[sp_rp_slot(j, u, n)] != run) ++bad;
		}
		// the saturation rule: any offset a block can ask for
		run = 0;
		for (uint32_t j = 0; j < mx; ++j) {
			if (j && u + j < n) run += Q[u][u + j];
			const uint32_t at = sp_rp_offset(j, upc[u]);
			const long long got = at ? rp.v[sp_rp_slot(at, u, n)] : 0;
			if (at > upc[u] || got != run) ++bad;
		}
	}
	if (total != T) ++bad;
	// ---- k_split_sums ----
	const size_t n1 = (size_t)n + 1;
	Counted<long long> w((size_t)(mx - mn + 1) * n1);
	for (uint32_t b = 1; b <= n; ++b)
		sp_block_sums_of(b, mn, mx, [&](uint32_t u) { return upc.at(u); },
		                 [&](uint32_t j, uint32_t u) { return rp.get(sp_rp_slot(j, u, n), &bad); },
		                 [&](uint32_t d, uint32_t bb, long long v) { w.put(sp_w_slot(d, bb, n, mn), v); });
	for (uint32_t d = mn; d <= mx; ++d)
		for (uint32_t b = 0; b <= n; ++b) {
			const uint64_t at = sp_w_slot(d, b, n, mn);
			if (w.writes[at] != (d <= b ? 1u : 0u)) ++bad;
			if (d <= b && w.v[at] != within[b - d][b]) ++bad;
		}
	// ---- k_split_layer, one launch per k ----
	Counted<uint16_t> dk((size_t)kmax * n1);
	std::vector<long long> g(2 * n1, -99), gn(kmax + 1, SPLIT_INFEASIBLE);
	g[0] = 0;
	for (uint32_t k = 1; k <= kmax; ++k) {
		const uint32_t lo = sp_layer_lo(k, mn), hi = sp_layer_hi(k, mx, n);
		// outside the range nothing is feasible
		for (uint32_t b = 0; b <= n; ++b) if ((b < lo || b > hi) && G[k][b] >= 0) ++bad;
		if (lo > hi) break;
		const uint32_t p_lo = sp_layer_lo(k - 1, mn), p_hi = sp_layer_hi(k - 1, mx, n);
		const long long* g_prev = g.data() + ((k - 1) & 1) * n1;
		long long* g_cur = g.data() + (k & 1) * n1;
		std::vector<uint32_t> written(n1, 0);
		const uint32_t blocks = (hi - lo) / SPLIT_THREADS + 1;
		for (uint32_t bx = 0; bx < blocks; ++bx) {
			const uint32_t b0 = lo + bx * SPLIT_THREADS;
			if (b0 > hi) { ++bad; continue; }
			const uint32_t b_last = hi - b0 < SPLIT_THREADS - 1 ? hi : b0 + (SPLIT_THREADS - 1);
			uint32_t d_lo, d_hi;
			sp_block_d_range(b0, b_last, p_lo, p_hi, mn, mx, &d_lo, &d_hi);
			// a d the block leaves out meets no feasible G_(k-1) in any of its lanes
			for (uint32_t b = b0; b <= b_last; ++b)
				for (uint32_t d = mn; d <= std::min(mx, b); ++d)
					if ((d < d_lo || d >= d_hi) && G[k - 1][b - d] >= 0) ++bad;
			std::vector<long long> best(SPLIT_THREADS, SPLIT_INFEASIBLE);
			std::vector<uint32_t> best_d(SPLIT_THREADS, 0);
			for (uint32_t w_lo = d_lo; w_lo < d_hi; w_lo += SPLIT_WINDOW_D) {
				const uint32_t w_hi = d_hi - w_lo < SPLIT_WINDOW_D ? d_hi : w_lo + SPLIT_WINDOW_D;
				const long long base = sp_stage_base(b0, w_hi);
				const uint32_t count = sp_stage_count(w_lo, w_hi);
				if (count > SPLIT_LDS_G) ++bad;
				std::vector<long long> stage(count);
				for (uint32_t i = 0; i < count; ++i)
					stage[i] = sp_stage_value(base + i, p_lo, p_hi, [&](uint32_t at) { if (at > n) ++bad; return g_prev[at]; });
				for (uint32_t tid = 0; tid < SPLIT_THREADS; ++tid) {
					const uint32_t b = b0 + tid;
					if (b > b_last) continue;
					sp_lane_window(b, b0, w_lo, w_hi,
					               [&](uint32_t i) {
						               return stage.at(i); },
					               [&](uint32_t d, uint32_t bb) { if (bb != b || (long long)bb - (long long)d < 0) ++bad; return w.get(sp_w_slot(d, bb, n, mn), &bad); },
					               &best[tid], &best_d[tid]);
				}
			}
			for (uint32_t tid = 0; tid < SPLIT_THREADS; ++tid) {
				const uint32_t b = b0 + tid;
				if (b > b_last) continue;
				g_cur[b] = best[tid]; ++written.at(b);
				dk.put(sp_d_slot(k, b, n), (uint16_t)best_d[tid]);
				if (b == n) gn[k] = best[tid];
			}
		}
		for (uint32_t b = 0; b <= n; ++b) {
			if (written[b] != (b >= lo && b <= hi ? 1u : 0u)) ++bad;
			if (b >= lo && b <= hi && (g_cur[b] != G[k][b] || dk.v[sp_d_slot(k, b, n)] != D[k][b])) ++bad;
		}
	}
	// ---- k_split_backtrack ----
	for (uint32_t K = 1; K <= kmax; ++K) {
		if (gn[K] != G[K][n]) ++bad;
		if (gn[K] < 0) continue;
		std::vector<uint32_t> cuts((size_t)kmax * (kmax + 1), 0xFFFFFFFFu), want(K + 1);
		const bool whole = sp_backtrack(K, n, [&](uint32_t k, uint32_t b) { return (uint32_t)dk.get(sp_d_slot(k, b, n), &bad); },
		                                [&](uint32_t i, uint32_t b) { cuts.at(sp_cut_slot(K, i, kmax)) = b; });
		if (!whole) ++bad;
		uint32_t b = n;
		for (uint32_t k = K; k >= 1; --k) { want[k] = b; b -= D[k][b]; }
		want[0] = b;
		long long gain = 0;
		for (uint32_t i = 0; i <= K; ++i) {
			if (cuts[sp_cut_slot(K, i, kmax)] != want[i]) ++bad;
			if (i && (want[i] - want[i - 1] < mn || want[i] - want[i - 1] > mx)) ++bad;
			if (i) gain += within[want[i - 1]][want[i]];
		}
		if (want[0] != 0 || gain != G[K][n]) ++bad;
		for (size_t at = 0; at < cuts.size(); ++at)
			if (cuts[at] != 0xFFFFFFFFu && (at < sp_cut_slot(K, 0, kmax) || at > sp_cut_slot(K, K, kmax))) ++bad;
	}
	return bad;
}

// All K-partitions of a tiny case, the last block's size ascending first: the first strict maximum is the contract's partition.
void enumerate(const Case& c, const std::vector<std::vector<long long>>& within, uint32_t k, uint32_t b, long long gain, std::vector<uint32_t>& cuts,
               long long* best, std::vector<uint32_t>* best_cuts) {
	if (k == 0) {
		if (b == 0 && gain > *best) { *best = gain; *best_cuts = cuts; }
		return;
	}
	for (uint32_t d = c.min_size; d <= std::min(c.max_size, b); ++d) {
		cuts[k - 1] = b - d;
		enumerate(c, within, k - 1, b - d, gain + within[b - d][b], cuts, best, best_cuts);
	}
}

long play_tiny(const Case& c) {
	long bad = 0;
	const uint32_t n = c.n;
	std::vector<std::vector<long long>> within(n + 1, std::vector<long long>(n + 1, 0));
	for (uint32_t a = 0; a <= n; ++a)
		for (uint32_t b = a; b <= n; ++b)
			for (uint32_t u = a; u < b; ++u) for (uint32_t v = u + 1; v < b; ++v) within[a][b] += c.q(u, v);
	// the recurrence through the header's lane functions alone, one block, then the backtrack
	std::vector<long long> prev(n + 1, SPLIT_INFEASIBLE), cur(n + 1);
	std::vector<std::vector<uint32_t>> D(c.k_max + 1, std::vector<uint32_t>(n + 1, 0));
	prev[0] = 0;
	for (uint32_t K = 1; K <= c.k_max; ++K) {
		for (uint32_t b = 0; b <= n; ++b) {
			long long best = SPLIT_INFEASIBLE; uint32_t best_d = 0;
			// (b0 = 0, one window over every d: the stage's base is -max_size, its entry i holds G_(k-1)(i - max_size))
			sp_lane_window(b, 0, c.min_size, c.max_size + 1, [&](uint32_t i) { return prev.at(i - c.max_size); },
			               [&](uint32_t d, uint32_t bb) { return within[bb - d][bb]; }, &best, &best_d);
			cur[b] = best; D[K][b] = best_d;
		}
		prev = cur;
		long long want = SPLIT_INFEASIBLE;
		std::vector<uint32_t> cuts(K + 1, 0), want_cuts;
		cuts[K] = n;
		enumerate(c, within, K, n, 0, cuts, &want, &want_cuts);
		if (want != cur[n]) { ++bad; continue; }
		if (want < 0) continue;
		std::vector<uint32_t> got(K + 1, 0xFFFFFFFFu);
		if (!sp_backtrack(K, n, [&](uint32_t k, uint32_t b) { return D[k][b]; }, [&](uint32_t i, uint32_t b) { got.at(i) = b; })) ++bad;
		if (got != want_cuts) ++bad;
	}
	return bad;
}

}  // namespace

int main() {
	long cases = 0, bad = 0;
	// refusals
	bad += sp_sizes_ok(10, 0, 5, 1) || sp_sizes_ok(10, 6, 5, 1) || sp_sizes_ok(10, 1, 65536, 1) || sp_sizes_ok(10, 1, 5, 0) || sp_sizes_ok(10, 1, 5, 1025) ||
	       sp_sizes_ok(65538, 1, 65535, 1) || !sp_sizes_ok(65537, 1, 65535, 1024) || !sp_sizes_ok(1, 1, 1, 1);      // (65537 * 65535 = 2^32 - 1)
	++cases;
	// tiny cases against the enumeration of all partitions
	for (uint32_t n = 1; n <= 9; ++n)
		for (int kind = 0; kind < 4; ++kind)
			for (uint32_t mn = 1; mn <= n; ++mn)
				for (uint32_t mx = mn; mx <= n; ++mx) {
					const Case c = make_case(n, 1 + (uint32_t)(rnd() % n), kind, mn, mx, n);
					bad += play_tiny(c) + play(c);
					++cases;
				}
	// every lane of every kernel: sizes around the block of 256 and the window of 768, bands narrower and wider than max_size
	const struct { uint32_t n, reach, mn, mx, kmax; } shapes[] = {
		{1, 1, 1, 1, 2}, {2, 1, 1, 2, 3}, {63, 5, 3, 9, 30}, {64, 70, 1, 64, 5}, {65, 10, 7, 30, 12}, {255, 40, 10, 60, 30}, {256, 300, 64, 64, 5}, {257, 20, 50, 300, 6},
		{300, 8, 7, 7, 50}, {301, 8, 7, 7, 50}, {600, 60, 50, 300, 8}, {600, 400, 100, 300, 4}, {513, 30, 1, 513, 3}, {700, 0, 30, 90, 20},
		{1000, 30, 100, 900, 4}, {1100, 900, 700, 1000, 3}, {1794, 12, 1, 1793, 2}};
	for (const auto& s : shapes)
		for (int kind = 0; kind < 4; ++kind) {
			if (kind && s.n > 700 && kind != 3) continue;
			bad += play(make_case(s.n, s.reach, kind, s.mn, s.mx, s.kmax));
			++cases;
		}
	std::printf("split-check: %ld cases, %ld bad\n", cases, bad);
	return bad ? 1 : 0;
}
