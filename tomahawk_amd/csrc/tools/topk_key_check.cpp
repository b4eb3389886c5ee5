// The top-k partners' key, cascade and block layout (csrc/hip/ld_topk_key.h) played on the host: `make topk-check` builds this file with
// g++ -fsanitize=address,undefined and runs it.  Everything goes against a restatement that shares no arithmetic with it:
//   the key      pack and unpack round trip, and key order against the comparator of the definition (|value| as float32 descending, ties
//                to the smaller partner) over every pair of candidates made of: 0, -0.0, float32 and double denormals, 1.0 and its float32
//                neighbours, negative values, two doubles that round to the same float32, partners 0, 1 and 2^32 - 2;
//   the cascade  several "threads" insert their keys one max-exchange at a time under a seeded random schedule, each after a threshold
//                read that is as stale as the schedule likes, against a sort: k from 1 to 32, fewer than k keys, duplicates;
//   two levels   blocks that take their thresholds at block start, keep LDS lists (through tk_insert and the kernel's word layout, in an
//                array of exactly tk_lds_words(k) words) and flush them word by word in a random interleaving, in two passes, against a
//                sort of everything.
#include <algorithm>
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>

#include "../hip/ld_topk_key.h"

using namespace twk;

namespace {

int failures = 0;
long long cases = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++failures <= 20) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rng() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

uint32_t bits_of(float x) { uint32_t b; memcpy(&b, &x, sizeof(b)); return b; }

// ---- 1: the key ---------------------------------------------------------------------------------------------------------------------
struct Candidate { double value; uint32_t partner; };
// the definition: a comes before b
bool before(const Candidate& a, const Candidate& b) {
	const float fa = fabsf((float)a.value), fb = fabsf((float)b.value);
	if (fa != fb) return fa > fb;
	return a.partner < b.partner;
}

void check_key() {
	const float one = 1.0f;
	std::vector<double> values = {0.0, -0.0, 5e-324, -5e-324, 1e-45, 1.4e-45, -1.4e-45, 1e-40, -1e-40, 1.17549435e-38, 1.0, -1.0,
	                              (double)nextafterf(one, 0.0f), (double)nextafterf(one, 2.0f), -(double)nextafterf(one, 0.0f),
	                              0.1, 0.1 + 1e-12, -0.1, 0.5, -0.5, 0.25, 0.999999, 1.0 + 1e-12, 1.0 - 1e-12, 3.0e-5, -0.75, 1e-300};
	CHECK(bits_of((float)0.1) == bits_of((float)(0.1 + 1e-12)) && 0.1 != 0.1 + 1e-12, "two doubles that round to one float32");
	for (int n = 0; n < 40; ++n) values.push_back(((double)(rng() >> 11) * ldexp(1.0, -53) - 0.5) * 2.0);
	const std::vector<uint32_t> partners = {0u, 1u, 2u, 0xFFFFFFFEu, 0x80000000u, 0x7FFFFFFFu, 12345u};
	std::vector<Candidate> all;
	for (const double v : values) for (const uint32_t p : partners) all.push_back(Candidate{v, p});
	for (const Candidate& c : all) {
		++cases;
		const uint64_t key = tk_pack(c.value, c.partner);
		uint32_t p; float x;
		tk_unpack(key, &p, &x);
		CHECK(key != 0, "the key of (%.17g, %u) is 0", c.value, c.partner);
		CHECK(p == c.partner && bits_of(x) == bits_of((float)c.value), "round trip of (%.17g, %u): (%.9g, %u)", c.value, c.partner, (double)x, p);
		CHECK((key & 1u) == (bits_of((float)c.value) >> 31), "the sign bit of (%.17g, %u)", c.value, c.partner);
		const uint64_t other = tk_with_partner(key, 77u);
		CHECK(other == tk_pack(c.value, 77u), "tk_with_partner of (%.17g, %u)", c.value, c.partner);
	}
	for (const Candidate& a : all)
		for (const Candidate& b : all) {
			++cases;
			const uint64_t ka = tk_pack(a.value, a.partner), kb = tk_pack(b.value, b.partner);
			const bool same_place = a.partner == b.partner && fabsf((float)a.value) == fabsf((float)b.value);
			if (same_place) { CHECK((ka >> 1) == (kb >> 1), "one place, two keys"); continue; }      // (the same partner twice: never in one list)
			CHECK((ka > kb) == before(a, b) && (kb > ka) == before(b, a), "order of (%.17g, %u) and (%.17g, %u)", a.value, a.partner, b.value, b.partner);
		}
	uint32_t p; float x;
	tk_unpack(0, &p, &x);
	CHECK(p == TOPK_NO_PARTNER && bits_of(x) == 0u, "an empty slot is (NO_PARTNER, +0.0f)");
}

// ---- 2: the cascade, one max-exchange at a time ---------------------------------------------------------------------------------------
std::vector<uint64_t> sorted_top(std::vector<uint64_t> keys, uint32_t k) {
	std::sort(keys.begin(), keys.end(), [](uint64_t a, uint64_t b) { return a > b; });
	keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
	keys.resize(k, 0ull);
	return keys;
}

struct Thread {
	std::vector<uint64_t> queue;
	size_t next = 0;
	uint64_t key = 0;
	uint32_t s = 0;
	bool active = false;
	bool done() const { return !active && next == queue.size(); }
};

// The threads' insertions into list[k] under a random schedule.  history: every value slot[k - 1] has held so far - a stale read takes
// any of them.  (The walk is tk_insert's, cut into its steps.)
void play(std::vector<uint64_t>& list, uint32_t k, std::vector<Thread>& threads, std::vector<uint64_t>& history) {
	for (;;) {
		std::vector<size_t> todo;
		for (size_t t = 0; t < threads.size(); ++t) if (!threads[t].done()) todo.push_back(t);
		if (todo.empty()) return;
		Thread& th = threads[todo[rng() % todo.size()]];
		if (!th.active) {
			const uint64_t key = th.queue[th.next++];
			const uint64_t thr = (rng() & 3) ? history[rng() % history.size()] : list[k - 1];
			if (key <= thr) continue;
			th.key = key; th.s = 0; th.active = true;
			continue;
		}
		const uint64_t old = list[th.s];
		if (th.key > old) list[th.s] = th.key;
		if (th.s == k - 1) history.push_back(list[k - 1]);
		if (old == th.key) { th.active = false; continue; }
		if (old < th.key) th.key = old;
		++th.s;
		if (th.s == k || th.key == 0) th.active = false;
	}
}

uint64_t random_key(uint32_t n_values, uint32_t n_partners) {
	// few distinct values: many ties, decided by the partner
	const double v = (double)(rng() % n_values) / (double)n_values * ((rng() & 1) ? 1.0 : -1.0);
	return tk_pack(v, (uint32_t)(rng() % n_partners));
}

void check_cascade() {
	for (uint32_t k = 1; k <= TOPK_MAX; ++k)
		for (int round = 0; round < 40; ++round) {
			++cases;
			const uint32_t n_keys = round < 8 ? (uint32_t)(rng() % (k + 1)) : (uint32_t)(rng() % 200);      // (fewer than k, none; many)
			const uint32_t n_threads = 1 + (uint32_t)(rng() % 8);
			std::vector<uint64_t> keys;
			std::vector<Thread> threads(n_threads);
			for (uint32_t n = 0; n < n_keys; ++n) {
				const uint64_t key = random_key(round & 1 ? 4 : 1000, 64);
				keys.push_back(key);
				threads[rng() % n_threads].queue.push_back(key);
				if (rng() % 10 == 0) threads[rng() % n_threads].queue.push_back(key);      // the same candidate twice: listed once
			}
			std::vector<uint64_t> list(k, 0ull), history(1, 0ull);
			play(list, k, threads, history);
			CHECK(list == sorted_top(keys, k), "the cascade: k = %u, %u keys, %u threads, round %d", k, n_keys, n_threads, round);
			// ... and tk_insert itself, in one piece
			std::vector<uint64_t> seq(k, 0ull);
			for (const uint64_t key : keys)
				tk_insert(k, key, [&](uint32_t s, uint64_t x) { const uint64_t old = seq.at(s); if (x > old) seq.at(s) = x; return old; });
			CHECK(seq == sorted_top(keys, k), "tk_insert: k = %u, %u keys", k, n_keys);
		}
}

// ---- 3: the block's words, and the two levels ------------------------------------------------------------------------------------------
void check_layout() {
	for (uint32_t k = 1; k <= TOPK_MAX; ++k) {
		++cases;
		const uint32_t words = tk_lds_words(k);
		CHECK(tk_lds_bytes(k) == (size_t)(32 + 256) * k * 8, "LDS bytes at k = %u", k);
		std::vector<int> seen(words, 0);
		for (uint32_t r = 0; r < TOPK_ROWS; ++r)
			for (uint32_t s = 0; s < k; ++s) {
				const uint32_t e = tk_row_word(k, r, s);
				bool is_row; uint32_t which;
				tk_word_owner(k, e, &is_row, &which);
				CHECK(e < words && is_row && which == r, "row word (%u, %u) at k = %u", r, s, k);
				if (e < words) ++seen[e];
			}
		for (uint32_t t = 0; t < TOPK_COLS; ++t)
			for (uint32_t s = 0; s < k; ++s) {
				const uint32_t e = tk_col_word(k, t, s);
				bool is_row; uint32_t which;
				tk_word_owner(k, e, &is_row, &which);
				CHECK(e < words && !is_row && which == t, "column word (%u, %u) at k = %u", t, s, k);
				if (e < words) ++seen[e];
				if (t) CHECK(e == tk_col_word(k, t - 1, s) + 1, "lanes side by side");      // (a wave's 64 lanes: 64 consecutive words)
				if (s) CHECK(e > tk_col_word(k, t, s - 1), "the flush meets a list's slots in order");
			}
		CHECK(std::count(seen.begin(), seen.end(), 1) == (long)words, "every word once at k = %u", k);
	}
	CHECK(tk_lds_bytes(16) == 36864 && tk_lds_bytes(32) == 73728, "36 KiB at k = 16, 72 KiB at k = 32");
}

// A block of the kernel for the lists of V variants (variant v < TOPK_ROWS is the block's row v, the others its columns): the keys of its
// pairs enter the LDS lists above the thresholds taken at block start; -> the flush's queue per variant, in word order.
struct BlockKey { uint32_t variant; uint64_t key; };
void check_two_levels() {
	for (uint32_t k = 1; k <= TOPK_MAX; ++k)
		for (int round = 0; round < 12; ++round) {
			++cases;
			const uint32_t V = 1 + (uint32_t)(rng() % 40);                       // variants
			std::vector<std::vector<uint64_t>> global(V, std::vector<uint64_t>(k, 0ull)), history(V, std::vector<uint64_t>(1, 0ull)), everything(V);
			for (int pass = 0; pass < 2; ++pass) {
				uint32_t n_blocks = 1 + (uint32_t)(rng() % 6);
				while (n_blocks) {
					const uint32_t together = 1 + (uint32_t)(rng() % n_blocks);      // blocks that run at the same time
					n_blocks -= together;
					// per variant: one "thread" per block, its queue the block's LDS list of that variant
					std::vector<std::vector<Thread>> flush(V, std::vector<Thread>(together));
					for (uint32_t b = 0; b < together; ++b) {
						std::vector<uint64_t> lds(tk_lds_words(k), 0ull), thr(V);
						for (uint32_t v = 0; v < V; ++v) thr[v] = (rng() & 1) ? global[v][k - 1] : history[v][rng() % history[v].size()];
						const uint32_t n_keys = (uint32_t)(rng() % (round < 4 ? 2 * k + 1 : 400));
						for (uint32_t n = 0; n < n_keys; ++n) {
							const uint32_t v = (uint32_t)(rng() % V);
							const uint64_t key = random_key(round & 1 ? 3 : 500, 1000);
							everything[v].push_back(key);
							if (key <= thr[v]) continue;
							tk_insert(k, key, [&](uint32_t s, uint64_t x) {
								uint64_t& w = lds.at(v < TOPK_ROWS ? tk_row_word(k, v, s) : tk_col_word(k, v - TOPK_ROWS, s));
								const uint64_t old = w;
								if (x > old) w = x;
								return old;
							});
						}
						for (uint32_t e = 0; e < tk_lds_words(k); ++e) {
							if (!lds[e]) continue;
							bool is_row; uint32_t which;
							tk_word_owner(k, e, &is_row, &which);
							const uint32_t v = is_row ? which : which + TOPK_ROWS;
							CHECK(v < V, "a key in a list nobody owns");
							if (v < V) flush[v][b].queue.push_back(lds[e]);
						}
					}
					for (uint32_t v = 0; v < V; ++v) play(global[v], k, flush[v], history[v]);
				}
			}
			for (uint32_t v = 0; v < V; ++v)
				CHECK(global[v] == sorted_top(everything[v], k), "two levels: k = %u, round %d, variant %u of %u", k, round, v, V);
		}
}

}  // namespace

int main() {
	check_key();
	check_cascade();
	check_layout();
	check_two_levels();
	printf("topk-check: %lld cases, %d bad\n", cases, failures);
	return failures ? 1 : 0;
}
