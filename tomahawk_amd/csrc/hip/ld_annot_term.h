// What the partitioned LD score's kernel (ld_score_annot.hip.h) and its host check (csrc/tools/annot_term_check.cpp, `make annot-check`)
// share: the term a pair adds to a (variant, category), the split width of its sums, and the index arithmetic of the block's two sides.
// Plain C++ with no HIP in it.
//
// THE TERM.  A pair with R2 = r2 adds, to the category c of one of its variants, t = rint((r2 * a) * 2^32), a the other variant's
// annotation: one double multiplication (rounded once), an exact scaling, rounding to nearest with ties to even - xs_quantise(r2 * a)
// (ld_exact_sum.h).  It is formed without llrint (on the device a rounding and a ten-instruction conversion per term):
//   s = r2 * 2^32           once per pair (at_scale): exact, a power of two;
//   x = s * a               one multiplication per category.  x == (r2 * a) * 2^32 bit for bit: scaling by a power of two commutes with
//                           the rounding of a product unless r2 * a is subnormal - then both sides lie below 2^-990 and round to 0;
//   y = x + 1.5 * 2^52      |x| <= 2^48 (1 + 2^-50) (r2 <= 1 + a few ulps, |a| <= 2^16), so y lies in [2^52, 2^53) where doubles are
//                           the integers: the addition rounds x to an integer, to nearest, ties to even - rint(x) - and
//   t = bits(y) - bits(1.5 * 2^52)    is that integer, its sign included: the mantissa field counts up from 1.5 * 2^52 in ones.
// The multiplication and the addition must stay two roundings: fused into one they would round the exact product instead of the
// double x.  The engine builds with -ffp-contract=off, and the function says so itself where the compiler understands it.  -0.0 and 0
// give 0; an r2 of 0 (no record: the kernel parks 0 for such a pair) gives 0 whatever a.  The check plays it against
// llrint((r2 * a) * 4294967296.0) over the corners, random values and exact ties.
//
// THE SPLIT.  ANNOT_SPLIT = 24 (ld_exact_sum.h's split; the kernel's header comment holds the proof that neither word can wrap).
#pragma once
#include <stdint.h>
#include <string.h>
#include "ld_exact_sum.h"

namespace twk {

constexpr int ANNOT_SPLIT = 24;
constexpr uint32_t ANNOT_MAX_CATEGORIES = 256;       // TWK_HIP_ANNOT_MAX_CATEGORIES
constexpr double ANNOT_MAX_ABS = 65536.0;            // TWK_HIP_ANNOT_MAX_ABS: 2^16
constexpr double AT_MAGIC = 6755399441055744.0;      // 1.5 * 2^52
constexpr long long AT_MAGIC_BITS = 0x4338000000000000ll;

// r2 as a number of 2^-32, not yet rounded: exact.
TWK_XS_FN double at_scale(double r2) { return r2 * XS_SCALE; }

// rint(s * a) for |s * a| < 2^51, ties to even: the term of a pair whose scaled r2 is s for an annotation a.
TWK_XS_FN long long at_term(double s, double a) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	const double x = s * a;
	const double y = x + AT_MAGIC;
	long long bits;
	memcpy(&bits, &y, sizeof(bits));
	return bits - AT_MAGIC_BITS;
}

// An annotation the engine accepts: finite and at most 2^16 in magnitude (a NaN fails the comparison).
TWK_XS_FN bool at_valid(double a) { return a >= -ANNOT_MAX_ABS && a <= ANNOT_MAX_ABS; }

// ---- The block: ANNOT_THREADS columns by ANNOT_ROWS rows of a launch, the categories ANNOT_SLAB at a time ----
constexpr int ANNOT_THREADS = 256;                   // columns of a block
constexpr int ANNOT_ROWS = 16;                       // rows of a block
constexpr int ANNOT_SLAB = 8;                        // categories staged at a time
// LDS rows of ANNOT_THREADS doubles are padded by two: with a row stride of 258 doubles = 516 dwords the rows a half-wave reads at one
// column (the row side: four rows of the stage, eight categories of the column annotations) start 4 banks apart - no two on one bank.
constexpr int ANNOT_STRIDE = ANNOT_THREADS + 2;
// The row side: thread = (half of the columns, row, category of the slab); a wave is 8 rows x 8 categories of one half.
constexpr int ANNOT_HALVES = ANNOT_THREADS / (ANNOT_ROWS * ANNOT_SLAB);      // 2
constexpr int ANNOT_ROW_SIDE_COLS = ANNOT_THREADS / ANNOT_HALVES;           // 128: the columns a thread walks, two ballot words of 64
static_assert(ANNOT_HALVES * ANNOT_ROWS * ANNOT_SLAB == ANNOT_THREADS && ANNOT_ROW_SIDE_COLS == 128 && ANNOT_ROWS * ANNOT_SLAB == 128,
              "every thread of the block has one (half, row, category); a half is two waves' columns and two waves' threads");
TWK_XS_FN uint32_t an_half(uint32_t thread) { return thread / (ANNOT_ROWS * ANNOT_SLAB); }
TWK_XS_FN uint32_t an_row(uint32_t thread) { return thread / ANNOT_SLAB % ANNOT_ROWS; }
TWK_XS_FN uint32_t an_cat(uint32_t thread) { return thread % ANNOT_SLAB; }
// Column `bit` of mask word `word` (0, 1) of a half: the block's four waves ballot one 64-bit word of columns each.
TWK_XS_FN uint32_t an_col(uint32_t half, uint32_t word, uint32_t bit) { return half * ANNOT_ROW_SIDE_COLS + word * 64 + bit; }
// Slabs of a call with n_annot categories, and the categories of slab k that exist.
TWK_XS_FN uint32_t an_slabs(uint32_t n_annot) { return (n_annot + ANNOT_SLAB - 1) / ANNOT_SLAB; }
// Where the two accumulator words of (variant, category) lie: hi at the index, lo behind it.
TWK_XS_FN uint64_t an_word(uint32_t variant, uint32_t n_annot, uint32_t category) { return ((uint64_t)variant * n_annot + category) * 2; }

}  // namespace twk
