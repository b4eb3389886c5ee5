// Top-k LD partners: the 64-bit key of a candidate, and where a block of k_ld_topk (ld_topk.hip.h) keeps its lists.  Plain C++ with no
// HIP in it, in the manner of ld_matrix_index.h: the kernel includes it, and so does csrc/tools/topk_key_check.cpp (`make topk-check`),
// which checks the key against the comparator of the definition and plays the cascade under random interleavings against a sort.
//
// THE KEY.  The list of a variant is its partners ordered by |value| descending, compared as float32, ties to the smaller partner index
// in file order (twk_hip_ld_topk, include/twk_hip.h).  One word per candidate, so that UNSIGNED INTEGER ORDER IS LIST ORDER:
//   key = bits(float32 |value|) << 33  |  (~partner & 0xFFFFFFFF) << 1  |  sign
//   - the bits of a non-negative float32 are 31 significant bits and grow with the value (denormals and +0 included);
//   - ~partner: of two candidates with the same |value| the smaller index has the larger key;
//   - the sign rides in bit 0: two different partners differ above it, so it never decides an order;
//   - 0 means EMPTY: a partner index is at most 2^32 - 2 (0xFFFFFFFF is TWK_HIP_NO_PARTNER), so ~partner >= 1 and no key is 0.
// The value is rounded from double to float32 once, here, to nearest: the bits twk_hip_ld_matrix stores for the pair.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TWK_TK_FN __host__ __device__ inline
#else
#define TWK_TK_FN inline
#endif

namespace twk {

constexpr uint32_t TOPK_MAX = 32;                    // slots of a list at most (TWK_HIP_TOPK_MAX)
constexpr uint32_t TOPK_NO_PARTNER = 0xFFFFFFFFu;    // (TWK_HIP_NO_PARTNER)
constexpr uint32_t TOPK_COLS = 256;                  // columns of a block = its lanes
constexpr uint32_t TOPK_ROWS = 32;                   // rows of a block
constexpr uint64_t TOPK_PARTNER_FIELD = 0xFFFFFFFFull << 1;

TWK_TK_FN uint32_t tk_float_bits(float x) { uint32_t b; memcpy(&b, &x, sizeof(b)); return b; }
TWK_TK_FN float tk_bits_float(uint32_t b) { float x; memcpy(&x, &b, sizeof(x)); return x; }

// The key of the candidate `partner` with the statistic `value`.
TWK_TK_FN uint64_t tk_pack(double value, uint32_t partner) {
	const uint32_t bits = tk_float_bits((float)value);
	return (uint64_t)(bits & 0x7FFFFFFFu) << 33 | (uint64_t)(~partner) << 1 | (uint64_t)(bits >> 31);
}
// The same candidate value in the list of another variant: the key with its partner replaced.
TWK_TK_FN uint64_t tk_with_partner(uint64_t key, uint32_t partner) { return (key & ~TOPK_PARTNER_FIELD) | (uint64_t)(~partner) << 1; }
TWK_TK_FN uint32_t tk_partner(uint64_t key) { return ~(uint32_t)(key >> 1); }
TWK_TK_FN float tk_value(uint64_t key) { return tk_bits_float((uint32_t)(key >> 33) | (uint32_t)(key & 1u) << 31); }
// A slot as the caller sees it: an empty one is (TOPK_NO_PARTNER, +0.0f).
TWK_TK_FN void tk_unpack(uint64_t key, uint32_t* partner, float* value) {
	*partner = key ? tk_partner(key) : TOPK_NO_PARTNER;
	*value = key ? tk_value(key) : 0.0f;
}

// THE CASCADE over the k slots of a list that only grow.  An insertion walks s = 0 .. k - 1: old = max-exchange(slot[s], key) - the slot
// becomes max(old, key), atomically - and the smaller of the two is carried to slot s + 1; it ends when the carry is 0 (the slot was
// empty), when the carry met itself (old == key: the candidate is listed already, an insertion is idempotent) or behind slot k - 1.
// `exchange(s, key)` is the list's max-exchange and returns `old`: an atomicMax on a shared list, a load and a store on a private one.
//   PROOF that the lists end as the k largest distinct keys inserted, in order, whatever the interleaving of the insertions.  Slot 0 is
//   only ever changed by max-exchanges with inserted keys, so it ends as their maximum m0.  Every other distinct key x reaches slot 1 at
//   least once: when x met slot 0 the slot held more (x is carried on at once), less (x stays, and since the slot ends as m0 != x a
//   later exchange displaces and carries it) or x itself (the copy in the slot is displaced later, likewise).  Nothing but inserted keys
//   reaches slot 1, and m0 never does (nothing displaces the maximum, and a second copy of it meets itself).  So slot 1 sees exactly
//   the keys below m0, each at least once, by max-exchanges only: by induction slot s ends as the (s + 1)-th largest distinct key.
//   THE THRESHOLD.  A key <= a value once read from slot[k - 1] need not be inserted: slots only grow, so the final slot[k - 1] is at
//   least that value, and the key is not among the k largest (or is slot[k - 1] itself, listed already).  The read may be as stale as
//   it likes - a stale value is a smaller one and costs a needless insertion, never a wrong list.
template <class Exchange>
TWK_TK_FN void tk_insert(uint32_t k, uint64_t key, Exchange&& exchange) {
	for (uint32_t s = 0; s < k && key; ++s) {
		const uint64_t old = exchange(s, key);
		if (old == key) return;
		if (old < key) key = old;
	}
}

// LDS OF A BLOCK, in 64-bit words: TOPK_ROWS row lists of k slots one behind the other (shared by the block's four waves), then the
// TOPK_COLS column lists, one per lane and LANE-INTERLEAVED - slot s of lane t at s * TOPK_COLS + t - so that the 64 lanes of a wave
// that step their lists together read 64 consecutive words: no bank conflict.  (32 + 256) * k * 8 bytes: 36 KiB at k = 16, 72 KiB at 32.
TWK_TK_FN uint32_t tk_lds_words(uint32_t k) { return (TOPK_ROWS + TOPK_COLS) * k; }
TWK_TK_FN size_t tk_lds_bytes(uint32_t k) { return (size_t)tk_lds_words(k) * sizeof(uint64_t); }
TWK_TK_FN uint32_t tk_row_word(uint32_t k, uint32_t row, uint32_t s) { return row * k + s; }
TWK_TK_FN uint32_t tk_col_word(uint32_t k, uint32_t lane, uint32_t s) { return TOPK_ROWS * k + s * TOPK_COLS + lane; }
// The flush walks the words e = 0 .. tk_lds_words(k) - 1: whose list is word e?  Row lists: is_row, which = the row; column lists:
// which = the lane.
TWK_TK_FN void tk_word_owner(uint32_t k, uint32_t e, bool* is_row, uint32_t* which) {
	*is_row = e < TOPK_ROWS * k;
	*which = *is_row ? e / k : (e - TOPK_ROWS * k) % TOPK_COLS;
}

}  // namespace twk
