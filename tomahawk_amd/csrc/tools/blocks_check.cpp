// Haplotype blocks, the parts that are plain C++ (csrc/hip/ld_block_ci.h), played on the host: `make blocks-check` builds this file with
// g++ under AddressSanitizer and UBSan and runs it.
//   the scan      bc_bounds - four passes that recompute the likelihood - against a restatement of the definition in long double with the
//                 101 values kept in arrays: tables with dmax == 0, a zero cell, D exactly 0, fractional counts, random ones; and, bit for
//                 bit, the same likelihood at every grid point when the roles of A and B are swapped.  A table whose running sums come
//                 within 1e-9 of the threshold in long double would not decide the comparison and counts as bad.
//   the slots     every lane of every block of a triangle's launches through the steps of k_ld_dprime_ci_band - the guards, the direct
//                 byte stores, the staged word, the transposed write-out - against arrays of write counts with a border: every in-band
//                 off-diagonal slot of lo and of hi exactly once, with its pair's bytes; the diagonal and the border never.
//   the counts    k_blocks_prefix's ballots and carried counts, lane by lane, against a count of the row's columns; then every thread of
//                 k_blocks_candidates (bc_candidates_of, both passes) against the contract's definition with all pairs inside [i, j]
//                 counted one by one - the running sums, the small-m rules, the spans and the permille test.
//   the key       bc_key's order against the comparator (sep descending, m descending, i ascending), and its two decoders.
//   the walk      k_blocks_walk played with lanes that run ahead of one another in random order: a lane moves on through skipped
//                 candidates by itself and waits at barrier A with the candidate it accepted; `used` is written when all lanes wait.
//                 All lanes must wait with the same candidate, no interior variant of a new block may be used, and block_of must be
//                 the sequential walk's.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../hip/ld_block_ci.h"

using namespace twk;

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return rng_state >> 17; }
double rnd01() { return (double)(rnd() % (1u << 30)) / (double)(1u << 30); }

// ---- the scan ----
// The definition in long double, arrays and all -> lo, hi and the smallest relative distance of a running sum from the threshold.
void ld_bounds(double n11, double nX, double nY, double n22, uint32_t* lo, uint32_t* hi, long double* gap) {
	const bool neg = n11 * n22 < nX * nY;
	const long double m11 = neg ? nX : n11, m12 = neg ? n11 : nX, m21 = neg ? n22 : nY, m22 = neg ? nY : n22;
	const long double T = (m11 + m22) + (m12 + m21);
	const long double pA = (m11 + m12) / T, qA = (m21 + m22) / T, pB = (m11 + m21) / T, qB = (m12 + m22) / T;
	const long double dmax = std::min(pA * qB, qA * pB);
	long double L[BC_POINTS], w[BC_POINTS], top = 0;
	for (int i = 0; i < BC_POINTS; ++i) {
		const long double d = ((long double)i / 100.0L) * dmax;
		const long double f11 = std::max(pA * pB + d, 1e-10L), f22 = std::max(qA * qB + d, 1e-10L), f12 = std::max(pA * qB - d, 1e-10L), f21 = std::max(qA * pB - d, 1e-10L);
		L[i] = (m11 * logl(f11) + m22 * logl(f22)) + (m12 * logl(f12) + m21 * logl(f21));
		if (i == 0 || L[i] > top) top = L[i];
	}
	long double total = 0;
	for (int i = 0; i < BC_POINTS; ++i) { w[i] = expl(L[i] - top); total += w[i]; }
	const long double thr = 0.05L * total;
	*gap = 1;
	int up = -1, down = -1;
	long double run = 0;
	for (int i = 0; i < BC_POINTS; ++i) { run += w[i]; *gap = std::min(*gap, fabsl(run - thr) / thr); if (up < 0 && run > thr) up = i; }
	run = 0;
	for (int i = BC_POINTS - 1; i >= 0; --i) { run += w[i]; *gap = std::min(*gap, fabsl(run - thr) / thr); if (down < 0 && run > thr) down = i; }
	*lo = (uint32_t)std::max(up - 1, 0); *hi = (uint32_t)std::min(down + 1, 100);
}

long check_table(double n11, double nX, double nY, double n22, int want_lo = -1, int want_hi = -1) {
	long bad = 0;
	uint32_t lo, hi, lo2, hi2, wlo, whi; long double gap;
	bc_bounds(n11, nX, nY, n22, &lo, &hi);
	bc_bounds(n11, nY, nX, n22, &lo2, &hi2);                 // the roles of A and B swapped
	ld_bounds(n11, nX, nY, n22, &wlo, &whi, &gap);
	if (gap < 1e-9L) ++bad;
	if (lo != wlo || hi != whi || lo != lo2 || hi != hi2 || lo > hi || hi > 100) ++bad;
	if (want_lo >= 0 && ((int)lo != want_lo || (int)hi != want_hi)) ++bad;
	const BcTable t = bc_table(n11, nX, nY, n22), u = bc_table(n11, nY, nX, n22);
	for (int i = 0; i < BC_POINTS; ++i) {
		const double a = bc_loglik(t, i), b = bc_loglik(u, i);
		if (memcmp(&a, &b, sizeof(a)) != 0) { ++bad; break; }
	}
	if (bad) std::printf("    table (%g, %g, %g, %g): lo %u hi %u, want %u %u, swapped %u %u, gap %Lg\n", n11, nX, nY, n22, lo, hi, wlo, whi, lo2, hi2, gap);
	return bad;
}

long check_scan() {
	long bad = 0, tables = 0;
	auto t = [&](double a, double b, double c, double d, int wl = -1, int wh = -1) { bad += check_table(a, b, c, d, wl, wh) ? 1 : 0; ++tables; };
	t(100, 0, 50, 0, 4, 96); t(0, 37, 0, 12, 4, 96); t(60, 40, 0, 0, 4, 96);          // dmax == 0: a monomorphic variant
	t(50, 0, 0, 50); t(120, 0, 30, 50); t(10, 200, 90, 0); t(0, 100, 100, 300); t(1, 0, 0, 499);      // a zero cell: D' = 1
	t(25, 25, 25, 25); t(40, 60, 20, 30); t(9, 21, 21, 49);                                          // D exactly 0
	t(3, 1, 1, 3); t(1, 3, 3, 1); t(250, 3, 2, 245); t(7, 493, 0, 0 + 0.0); t(2, 2, 1, 495);
	t(101.25, 12.5, 30.75, 55.5); t(0.37, 99.63, 44.1, 55.9); t(311.2, 0.8, 1.3, 186.7); t(63.999, 0.001, 0.001, 63.999);      // fractional counts
	for (int k = 0; k < 1500; ++k) {
		const double N = 20 + (double)(rnd() % 2000);
		double c[4]; double sum = 0;
		for (double& x : c) { x = rnd01(); x = x * x; if (rnd() % 7 == 0) x = 0; sum += x; }
		if (sum == 0) continue;
		const bool frac = k % 3 == 0;
		for (double& x : c) x = frac ? x / sum * N : std::floor(x / sum * N);
		if (c[0] + c[1] + c[2] + c[3] < 2) continue;
		t(c[0], c[1], c[2], c[3]);
	}
	std::printf("  %-66s %5ld tables  %s\n", "the scan against the long double restatement, A and B swapped", tables, bad ? "BAD" : "ok");
	return bad;
}

// ---- a band over positions, with random bytes ----
struct Band {
	uint32_t n = 0; std::vector<uint32_t> pos, first; std::vector<uint64_t> ptr; std::vector<BandRow> rows;
	std::vector<uint8_t> lo, hi; std::vector<uint32_t> ps, pr;
	uint32_t widest = 0;
	uint32_t LO(uint32_t x, uint32_t y) const { return lo[ptr[x] + (y - first[x])]; }
	uint32_t HI(uint32_t x, uint32_t y) const { return hi[ptr[x] + (y - first[x])]; }
};
Band make_band(uint32_t n, uint32_t w, uint32_t max_step, int flavour) {
	Band b; b.n = n; b.pos.resize(n); b.first.resize(n); b.ptr.resize((size_t)n + 1);
	uint32_t p = 1000;
	for (uint32_t v = 0; v < n; ++v) { p += 1 + (uint32_t)(rnd() % max_step); b.pos[v] = p; }
	bm_layout(n, [&](uint32_t k) { return b.pos[k]; }, [&](uint32_t) { return 0u; }, w, b.first.data(), b.ptr.data());
	b.rows.resize(n);
	for (uint32_t u = 0; u < n; ++u) { b.rows[u] = BandRow{b.ptr[u], b.first[u], (uint32_t)(b.ptr[u + 1] - b.ptr[u])}; b.widest = std::max(b.widest, b.rows[u].len); }
	b.lo.assign(b.ptr[n], BC_NONE); b.hi.assign(b.ptr[n], BC_NONE);
	b.ps.assign(b.ptr[n], 0xDEADu); b.pr.assign(b.ptr[n], 0xDEADu);
	for (uint32_t u = 0; u < n; ++u) for (uint32_t v = u + 1; v < b.first[u] + b.rows[u].len; ++v) {
		uint8_t lo = BC_NONE, hi = BC_NONE;
		const uint32_t kind = (uint32_t)(rnd() % 100);
		if (kind >= 8) {                                     // (8 % of the pairs have no record)
			const bool in_run = flavour && (u / 9 == v / 9);      // runs of strong pairs: blocks of many markers
			if (in_run ? kind < 97 : kind < 30) { lo = (uint8_t)(45 + rnd() % 56); hi = (uint8_t)(97 + rnd() % 4); }
			else { hi = (uint8_t)(rnd() % 101); lo = (uint8_t)(rnd() % (hi + 1u)); }
		}
		b.lo[b.ptr[u] + (v - b.first[u])] = lo; b.hi[b.ptr[u] + (v - b.first[u])] = hi;
		b.lo[b.ptr[v] + (u - b.first[v])] = lo; b.hi[b.ptr[v] + (u - b.first[v])] = hi;
	}
	return b;
}

// ---- the slots: k_ld_dprime_ci_band's stores on a plain set ----
long check_slots(uint32_t M, uint32_t a0, uint32_t n, uint32_t S, uint32_t w) {
	constexpr uint64_t BORDER = 1024;
	std::vector<uint32_t> pos(M);
	for (uint32_t v = 0; v < M; ++v) pos[v] = 1000 + 100 * v;
	std::vector<uint32_t> first(n); std::vector<uint64_t> ptr((size_t)n + 1);
	bm_layout(n, [&](uint32_t k) { return pos[a0 + k]; }, [&](uint32_t) { return 0u; }, w, first.data(), ptr.data());
	std::vector<BandRow> rows(n);
	for (uint32_t u = 0; u < n; ++u) rows[u] = BandRow{ptr[u], first[u], (uint32_t)(ptr[u + 1] - ptr[u])};
	const uint64_t nnz = ptr[n];
	std::vector<uint32_t> writes_lo(nnz + 2 * BORDER, 0), writes_hi(nnz + 2 * BORDER, 0);
	std::vector<uint8_t> lo(nnz + 2 * BORDER, BC_NONE), hi(nnz + 2 * BORDER, BC_NONE);
	long bad = 0;
	auto store = [&](uint64_t slot, uint32_t pv) {
		const uint64_t at = slot + BORDER;
		if (at >= lo.size()) { ++bad; return; }
		++writes_lo[at]; ++writes_hi[at]; lo[at] = (uint8_t)pv; hi[at] = (uint8_t)(pv >> 8);
	};
	auto value = [](uint32_t u, uint32_t v) { if (u > v) std::swap(u, v); return 1u << 16 | ((u * 7 + v * 3) % 101) << 8 | ((u + v) % 101); };
	std::vector<uint32_t> stage(MX_STAGE_WORDS), kept(MX_COLS), cfirst(MX_COLS), clen(MX_COLS); std::vector<uint64_t> cbase(MX_COLS);
	for (uint32_t x = 0; x < n; x += S) for (uint32_t c0 = x; c0 < n; c0 += S) {
		const uint32_t la0 = a0 + x, nA = std::min(S, n - x), lb0 = a0 + c0, nB = std::min(S, n - c0);
		const bool diag = c0 == x;
		for (uint32_t by = 0; by < (nA + MX_ROWS - 1) / MX_ROWS; ++by) for (uint32_t bx = 0; bx < (nB + MX_COLS - 1) / MX_COLS; ++bx) {
			const uint32_t i0 = by * MX_ROWS;
			if (mx_block_dead(diag, bx, i0)) continue;
			const BandRow last = rows[bm_block_last_row(la0, i0, nA, a0, n)];
			if (bm_block_dead(lb0, bx, a0, last.first, last.len)) continue;
			std::fill(kept.begin(), kept.end(), 0u);
			for (uint32_t tid = 0; tid < MX_COLS; ++tid) {
				const uint32_t col = mx_rel(lb0, bx * MX_COLS + tid, a0);
				BandRow mine{0, 0, 0};
				if (col < n) mine = rows[col];
				cbase[tid] = mine.base; cfirst[tid] = mine.first; clen[tid] = mine.len;
			}
			for (uint32_t tid = 0; tid < MX_COLS; ++tid) for (uint32_t r = 0; r < MX_ROWS; ++r) {
				const uint32_t i = i0 + r, j = bx * MX_COLS + tid;
				if (!mx_lane_live(i, j, nA, nB)) continue;
				const uint32_t sA = la0 + i, sB = lb0 + j;
				if (!(sA < M && sB < M) || (diag && !(sB > sA)) || pos[sB] - pos[sA] > w) continue;      // the pair rules and the window
				const uint32_t u = mx_rel(la0, i, a0), v = mx_rel(lb0, j, a0);
				if (!mx_ok_plain(u, v, n)) continue;
				const BandRow ru = rows[u];
				if (!bm_in_band(v, ru.first, ru.len)) { ++bad; continue; }
				const uint32_t pv = value(u, v);
				store(bm_slot(ru.base, ru.first, v), pv);
				stage[mx_stage(r, tid)] = pv; kept[tid] |= 1u << r;
			}
			for (uint32_t tid = 0; tid < MX_COLS; ++tid) for (uint32_t k = 0; k < MX_TSTEPS; ++k) {
				const uint32_t tr = mx_trow(tid), c = mx_tcol(tid, k);
				if (!(kept[c] >> tr & 1)) continue;
				const uint32_t ocol = mx_rel(la0, i0 + tr, a0), orow = mx_rel(lb0, bx * MX_COLS + c, a0);
				if (mx_ok_plain(ocol, orow, n) && bm_in_band(ocol, cfirst[c], clen[c])) store(bm_slot(cbase[c], cfirst[c], ocol), stage[mx_stage(tr, c)]);
				else ++bad;
			}
		}
	}
	for (uint64_t k = 0; k < BORDER; ++k) if (writes_lo[k] || writes_lo[BORDER + nnz + k]) ++bad;
	for (uint32_t u = 0; u < n; ++u) for (uint32_t v = first[u]; v < first[u] + rows[u].len; ++v) {
		const uint64_t at = BORDER + bm_slot(rows[u].base, rows[u].first, v);
		if (u == v) { if (writes_lo[at] || writes_hi[at] || lo[at] != BC_NONE || hi[at] != BC_NONE) ++bad; continue; }
		const uint32_t pv = value(u, v);
		if (writes_lo[at] != 1 || writes_hi[at] != 1 || lo[at] != (uint8_t)pv || hi[at] != (uint8_t)(pv >> 8)) ++bad;
	}
	char name[96]; snprintf(name, sizeof(name), "the slots: n=%u a0=%u of %u, tiles of %u, window %u", n, a0, M, S, w);
	std::printf("  %-66s %8llu slots  %s\n", name, (unsigned long long)nnz, bad ? "BAD" : "ok");
	return bad;
}

// ---- the counts ----
struct Cand { uint32_t i, j, s, r; uint64_t key; };

long check_counts(const char* name, Band& b, const BlockParams& par, std::vector<Cand>* out_sorted, BlockKey* out_key) {
	long bad = 0;
	const uint32_t n = b.n;
	// k_blocks_prefix: one wave per row
	for (uint32_t y = 0; y < n; ++y) {
		const BandRow row = b.rows[y];
		uint32_t cs = 0, cr = 0;
		for (uint32_t k0 = 0; k0 < row.len; k0 += 64) {
			unsigned long long bs = 0, br = 0;
			for (uint32_t lane = 0; lane < 64; ++lane) {
				uint32_t lo = BC_NONE, hi = BC_NONE;
				if (k0 + lane < row.len) { lo = b.lo[row.base + k0 + lane]; hi = b.hi[row.base + k0 + lane]; }
				bs |= (unsigned long long)bc_strong(lo, hi, par.strong_lo, par.strong_hi) << lane;
				br |= (unsigned long long)bc_recomb(lo, hi, par.recomb_hi) << lane;
			}
			for (uint32_t lane = 0; lane < 64 && k0 + lane < row.len; ++lane) {
				b.ps[row.base + k0 + lane] = cs + bc_prefix_in_ballot(bs, lane);
				b.pr[row.base + k0 + lane] = cr + bc_prefix_in_ballot(br, lane);
			}
			cs += (uint32_t)__builtin_popcountll(bs); cr += (uint32_t)__builtin_popcountll(br);
		}
		uint32_t ws = 0, wr = 0;
		for (uint32_t k = 0; k < row.len; ++k) {
			const uint32_t x = row.first + k;
			if (x != y) { ws += bc_strong(b.LO(y, x), b.HI(y, x), par.strong_lo, par.strong_hi); wr += bc_recomb(b.LO(y, x), b.HI(y, x), par.recomb_hi); }
			if (b.ps[row.base + k] != ws || b.pr[row.base + k] != wr) ++bad;
		}
	}
	BlockKey key; uint32_t bits = 0;
	const uint32_t sep_max = b.pos[n - 1] - b.pos[0];
	if (!bc_key_layout(n, b.widest, sep_max, &key, &bits)) return bad + 1;
	const BlocksBand view{b.lo.data(), b.hi.data(), b.rows.data(), b.pos.data(), b.ps.data(), b.pr.data(), n, par, key};
	// both passes of k_blocks_candidates
	std::vector<uint32_t> counts((size_t)n * 3), off((size_t)n + 1, 0);
	for (uint32_t i = 0; i < n; ++i) bc_candidates_of<false>(view, i, &counts[3 * (size_t)i], 0, 0, nullptr, nullptr, nullptr, nullptr);
	for (uint32_t i = 0; i < n; ++i) off[i + 1] = off[i] + counts[3 * (size_t)i];
	const uint32_t total = off[n];
	std::vector<unsigned long long> keys((size_t)total + 1, ~0ull); std::vector<uint32_t> vals((size_t)total + 1, 0xDEADu), cs((size_t)total + 1, 0xDEADu), cr((size_t)total + 1, 0xDEADu);
	for (uint32_t i = 0; i < n; ++i) bc_candidates_of<true>(view, i, nullptr, off[i], total, keys.data(), vals.data(), cs.data(), cr.data());
	if (keys[total] != ~0ull || vals[total] != 0xDEADu) ++bad;
	// the definition, every pair inside [i, j] counted one by one
	std::vector<Cand> want;
	uint64_t n_c = 0, n_inf = 0;
	for (uint32_t i = 0; i < n; ++i) for (uint32_t j = i + 1; j < b.first[i] + b.rows[i].len; ++j) {
		if (b.LO(i, j) == BC_NONE) continue;
		++n_inf;
		if (!(b.LO(i, j) >= par.strong_lo && b.HI(i, j) >= par.strong_hi)) continue;
		++n_c;
		const uint32_t m = j - i + 1, sep = b.pos[j] - b.pos[i];
		const uint32_t cut = m == 2 ? par.strong_lo_2 : (m == 3 || m == 4) ? par.strong_lo_34 : par.strong_lo;
		uint32_t s = 0, r = 0;
		for (uint32_t x = i; x < j; ++x) for (uint32_t y = x + 1; y <= j; ++y) {
			if (b.LO(x, y) == BC_NONE) continue;
			if (b.LO(x, y) >= cut && b.HI(x, y) >= par.strong_hi) ++s;
			if (b.HI(x, y) < par.recomb_hi) ++r;
		}
		if (m == 2 && sep > par.max_span_2) continue;
		if (m == 3 && sep > par.max_span_3) continue;
		if (s + r < (m == 2 ? 1u : m == 3 ? 3u : 6u)) continue;
		if (!((uint64_t)s * 1000 > (uint64_t)par.inform_permille * (s + r))) continue;
		want.push_back(Cand{i, j, s, r, 0});
	}
	uint64_t got_c = 0, got_inf = 0;
	for (uint32_t i = 0; i < n; ++i) { got_c += counts[3 * (size_t)i + 1]; got_inf += counts[3 * (size_t)i + 2]; }
	if (got_c != n_c || got_inf != n_inf || want.size() != total) ++bad;
	else for (uint32_t k = 0; k < total; ++k) {               // (both in order of i, then j)
		const Cand& wnt = want[k];
		const uint32_t m = wnt.j - wnt.i + 1;
		if (vals[k] != k || cs[k] != wnt.s || cr[k] != wnt.r || bc_key_i(key, keys[k]) != wnt.i || bc_key_m(key, keys[k]) != m ||
		    keys[k] != bc_key(key, b.pos[wnt.j] - b.pos[wnt.i], m, wnt.i)) { ++bad; break; }
	}
	// the key's order against the comparator
	for (Cand& c : want) c.key = bc_key(key, b.pos[c.j] - b.pos[c.i], c.j - c.i + 1, c.i);
	std::vector<Cand> by_key = want, by_rule = want;
	std::sort(by_key.begin(), by_key.end(), [](const Cand& x, const Cand& y) { return x.key < y.key; });
	std::stable_sort(by_rule.begin(), by_rule.end(), [&](const Cand& x, const Cand& y) {
		const uint32_t sx = b.pos[x.j] - b.pos[x.i], sy = b.pos[y.j] - b.pos[y.i], mx = x.j - x.i, my = y.j - y.i;
		if (sx != sy) return sx > sy;
		if (mx != my) return mx > my;
		return x.i < y.i;
	});
	for (size_t k = 0; k < want.size(); ++k) if (by_key[k].i != by_rule[k].i || by_key[k].j != by_rule[k].j) { ++bad; break; }
	for (size_t k = 1; k < by_key.size(); ++k) if (by_key[k].key == by_key[k - 1].key) { ++bad; break; }      // a key names one candidate
	if (bits > 64) ++bad;
	std::printf("  %-66s %6zu qualify of %6llu  %s\n", name, want.size(), (unsigned long long)n_c, bad ? "BAD" : "ok");
	*out_sorted = by_key; *out_key = key;
	return bad;
}

// ---- the walk, with lanes running ahead ----
long check_walk(const char* name, uint32_t n, const std::vector<Cand>& sorted, const BlockKey& key, uint32_t lanes) {
	long bad = 0;
	const uint32_t stride = (n + 63) / 64, m = (uint32_t)sorted.size();
	// the sequential walk
	std::vector<uint32_t> want_of(n, BLOCK_NONE);
	uint32_t want_blocks = 0;
	for (const Cand& c : sorted) {
		if (want_of[c.i] != BLOCK_NONE || want_of[c.j] != BLOCK_NONE) continue;
		for (uint32_t v = c.i; v <= c.j; ++v) { if (want_of[v] != BLOCK_NONE) ++bad; want_of[v] = c.i; }      // no interior variant in an earlier block
		++want_blocks;
	}
	std::vector<unsigned long long> used(stride, 0ull);
	std::vector<uint32_t> block_of(n, BLOCK_NONE);
	std::vector<uint32_t> at(lanes, 0);          // the candidate a lane looks at next
	std::vector<uint8_t> waiting(lanes, 0);      // ... it stands at barrier A with candidate at[lane]
	uint32_t blocks = 0;
	for (;;) {
		bool all = true;
		for (uint32_t l = 0; l < lanes; ++l) all = all && (waiting[l] || at[l] >= m);
		if (all) {
			bool any = false;
			for (uint32_t l = 0; l < lanes; ++l) any = any || waiting[l];
			if (!any) break;
			const uint32_t k = at[0];
			for (uint32_t l = 0; l < lanes; ++l) if (!waiting[l] || at[l] != k) ++bad;      // every lane decided alike
			if (bad) break;
			const uint32_t i = bc_key_i(key, sorted[k].key), j = i + bc_key_m(key, sorted[k].key) - 1;
			if (i != sorted[k].i || j != sorted[k].j) ++bad;
			// between A and B: the words' owners write
			for (uint32_t w = i >> 6; w <= j >> 6; ++w) {
				const unsigned long long bits = bc_range_bits(w, i, j);
				if (used[w] & bits) ++bad;
				used[w] |= bits;
			}
			for (uint32_t v = i; v <= j; ++v) block_of[v] = i;
			++blocks;
			for (uint32_t l = 0; l < lanes; ++l) { waiting[l] = 0; at[l] = k + 1; }
			continue;
		}
		// one lane that is not waiting runs ahead, a random number of candidates
		uint32_t l = (uint32_t)(rnd() % lanes);
		while (waiting[l] || at[l] >= m) l = (l + 1) % lanes;
		for (uint32_t steps = 1 + (uint32_t)(rnd() % 200); steps && at[l] < m; --steps) {
			const uint32_t i = bc_key_i(key, sorted[at[l]].key), j = i + bc_key_m(key, sorted[at[l]].key) - 1;
			if (bc_ends_free(used.data(), i, j)) { waiting[l] = 1; break; }
			++at[l];
		}
	}
	if (blocks != want_blocks || block_of != want_of) ++bad;
	for (uint32_t v = 0; v < n; ++v) if ((used[v >> 6] >> (v & 63) & 1) != (want_of[v] != BLOCK_NONE)) { ++bad; break; }
	std::printf("  %-66s %6u blocks of %6u  %s\n", name, blocks, m, bad ? "BAD" : "ok");
	return bad;
}

}  // namespace

int main() {
	long bad = 0, cases = 0;
	bad += check_scan() ? 1 : 0; ++cases;
	bad += check_slots(300, 37, 203, 128, 2000) ? 1 : 0; ++cases;
	bad += check_slots(240, 37, 203, 64, 2000) ? 1 : 0; ++cases;
	bad += check_slots(700, 0, 700, 512, 30000) ? 1 : 0; ++cases;
	bad += check_slots(65, 0, 65, 64, 0) ? 1 : 0; ++cases;
	// the parameters must be refused where the contract says so
	{
		long b = 0;
		BlockParams p = BLOCK_DEFAULTS;
		if (!bc_params_ok(p)) ++b;
		for (uint32_t BlockParams::* f : {&BlockParams::strong_lo, &BlockParams::strong_hi, &BlockParams::recomb_hi, &BlockParams::strong_lo_2, &BlockParams::strong_lo_34}) {
			BlockParams q = p; q.*f = 101; if (bc_params_ok(q)) ++b;
		}
		{ BlockParams q = p; q.recomb_hi = 99; if (bc_params_ok(q)) ++b; q.strong_hi = 99; if (!bc_params_ok(q)) ++b; }
		{ BlockParams q = p; q.inform_permille = 1001; if (bc_params_ok(q)) ++b; q.inform_permille = 1000; if (!bc_params_ok(q)) ++b; }
		std::printf("  %-66s %s\n", "the parameters' refusals", b ? "BAD" : "ok");
		bad += b ? 1 : 0; ++cases;
	}
	struct Shape { const char* name; uint32_t n, w, step; int flavour; BlockParams par; };
	const BlockParams tight{70, 98, 90, 80, 50, 950, 150, 400}, loose{60, 97, 80, 60, 45, 700, 20000, 30000};
	const Shape shapes[] = {
		{"n=150, window 3000, steps to 400: random classes", 150, 3000, 400, 0, BLOCK_DEFAULTS},
		{"n=150, runs of strong pairs, the defaults", 150, 3000, 400, 1, BLOCK_DEFAULTS},
		{"n=200, runs of strong pairs, spans that bind", 200, 2500, 300, 1, tight},
		{"n=130, a band wider than a wave, loose thresholds", 130, 1u << 20, 50, 1, loose},
		{"n=70, window 0 steps of 1: rows of length 1", 70, 0, 3, 1, BLOCK_DEFAULTS},
		{"n=2", 2, 1000, 10, 1, loose},
	};
	for (const Shape& s : shapes) {
		Band b = make_band(s.n, s.w, s.step, s.flavour);
		std::vector<Cand> sorted; BlockKey key{};
		bad += check_counts(s.name, b, s.par, &sorted, &key) ? 1 : 0; ++cases;
		for (const uint32_t lanes : {1u, 7u, 64u}) {
			char name[96]; snprintf(name, sizeof(name), "  ... its walk with %u lanes running ahead", lanes);
			bad += check_walk(name, s.n, sorted, key, lanes) ? 1 : 0; ++cases;
		}
	}
	std::printf("blocks-check: %ld cases, %ld bad\n", cases, bad);
	return bad ? 1 : 0;
}
