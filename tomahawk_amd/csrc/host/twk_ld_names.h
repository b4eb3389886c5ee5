// What the command line (calc_main.cpp) and the commands' methods (twk_ld.cpp) both have to know, stated once: the names of the LD and the
// relationship statistics and of ldaggregate's reductions, each with its engine value, and the host's limits on bins and ranges.
#ifndef TWK_LD_NAMES_H_
#define TWK_LD_NAMES_H_

#include <cstdint>
#include <cstring>
#include <string>

#include "twk_hip.h"
#include "twk_ld.h"

namespace tomahawk {

// A list of names whose positions are the values: name(v) and valid(v) one way, value(name) the other
template <int N>
struct NameTable {
	const char* names[N];
	bool valid(int64_t v) const { return v >= 0 && v < N; }
	const char* name(int64_t v) const { return names[v]; }
	int32_t value(const char* s) const {      // -1: no such name
		for (int32_t v = 0; v < N; ++v) if (strcmp(s, names[v]) == 0) return v;
		return -1;
	}
	std::string list() const {                // "r, r2, D, Dprime": what a message offers
		std::string out;
		for (int v = 0; v < N; ++v) { if (v) out += ", "; out += names[v]; }
		return out;
	}
};

static const NameTable<4> LD_STATS = {{"r", "r2", "D", "Dprime"}};
static_assert(TWK_HIP_STAT_R == 0 && TWK_HIP_STAT_R2 == 1 && TWK_HIP_STAT_D == 2 && TWK_HIP_STAT_DPRIME == 3, "LD_STATS is in the engine's order");
static const NameTable<3> REL_STATS = {{"ibs", "ibs0", "king"}};
static_assert(TWK_HIP_REL_IBS == 0 && TWK_HIP_REL_IBS0 == 1 && TWK_HIP_REL_KING == 2, "REL_STATS is in the engine's order");
static const NameTable<6> AGGREGATE_REDUCTIONS = {{"mean", "count", "min", "max", "sd", "total"}};
static_assert(TWK_AGGREGATE_MEAN == 0 && TWK_AGGREGATE_COUNT == 1 && TWK_AGGREGATE_MIN == 2 && TWK_AGGREGATE_MAX == 3 && TWK_AGGREGATE_SD == 4 && TWK_AGGREGATE_TOTAL == 5,
              "AGGREGATE_REDUCTIONS is in the enum's order");

// The host's limits (the engine keeps its own): bins of lddecay and per axis of ldaggregate; lddecay's range in bases, below 2^32
static const int32_t MAX_BINS = 4096;
static const int64_t MAX_RANGE_BP = 0xFFFFFFFFll;

}  // namespace tomahawk
#endif
