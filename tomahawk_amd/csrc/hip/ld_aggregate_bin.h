// LD aggregate: how a variant's two bins are packed, and the width at which a cell's partial sums are split.  Plain C++ with no HIP in
// it: k_ld_aggregate (ld_aggregate.hip.h) includes it, and so does csrc/tools/aggregate_bin_check.cpp (`make aggregate-check`), which
// plays the packing against a naive restatement.  What integers a pair's statistic adds to a cell, how a partial sum is split over two
// accumulator words and how the host puts them together again is ld_exact_sum.h; ld_aggregate.hip.h proves that neither word can
// overflow at this width while a call stays inside the room the engine enforces.
#pragma once
#include <stdint.h>
#include "ld_exact_sum.h"

namespace twk {

constexpr uint32_t AGG_MAX_BINS = 4096;               // bins per axis
constexpr uint32_t AGG_OFF = 0xFFFFu;                 // a variant that is off the landscape on an axis
constexpr uint32_t AGG_NO_KEY = 0xFFFFFFFFu;          // off on both axes: contributes nothing (and a lane without a pair)
constexpr int AGG_SPLIT = 20;                         // a partial sum S goes to the accumulators as S >> 20 and S & (2^20 - 1)

// A variant's two bins in one word: x in the low half, y in the high half.
TWK_XS_FN uint32_t ag_pack(uint32_t bin_x, uint32_t bin_y) { return (bin_x & 0xFFFFu) | bin_y << 16; }
TWK_XS_FN uint32_t ag_x(uint32_t key) { return key & 0xFFFFu; }
TWK_XS_FN uint32_t ag_y(uint32_t key) { return key >> 16; }

}  // namespace twk
