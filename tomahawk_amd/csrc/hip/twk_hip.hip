// C ABI of the MI355X pairwise-LD engine (include/twk_hip.h).
//
// Host-side orchestration of the three device stages
//   prep  (ld_prep.hip.h)  reference bitvectors -> contraction planes
//   count (ld_count.hip.h) LDS-tiled AND+popcount contraction  [dominant kernel]
//   math  (ld_math.hip.h)  cells -> D/D'/r2/Fisher -> filters -> compaction
//   (ld_three.hip.h: screen + recount behind the three-product form of the unphased contraction)
//   score (ld_score.hip.h) cells -> r2 -> per-variant sums, in place of the math stage (twk_hip_ld_score)
//   prune (ld_prune.hip.h) cells -> keep -> adjacency bitmap, in place of the math stage, and the greedy walk over it (twk_hip_ld_prune)
//   clump (ld_clump.hip.h) cells -> keep -> the bitmap's bits (u, v) and (v, u), likewise, and the walk over it in P order (twk_hip_ld_clump)
//   matrix (ld_matrix.hip.h) cells -> one statistic of the pair's record -> the entries (u, v) and (v, u) of a dense float32 matrix (twk_hip_ld_matrix)
//   decay (ld_decay.hip.h) cells -> r2 -> exact integer sums per distance bin, in place of the math stage (twk_hip_ld_decay)
//   aggregate (ld_aggregate.hip.h) cells -> one statistic -> exact integer sums, counts and extremes per cell of an x-by-y landscape, likewise (twk_hip_ld_aggregate)
//   annot (ld_score_annot.hip.h) cells -> r2 -> times the partner's annotations -> exact integer sums per (variant, category), likewise (twk_hip_ld_score_annot)
//   bandmat (ld_bandmat.hip.h) cells -> one statistic of the pair's record -> the entries (u, v) and (v, u) of a banded float32 matrix: per row only the columns inside the window (twk_hip_ld_matrix_band)
//   relate (ld_relate.hip.h) the raw layout transposed into planes of the samples -> count -> genotype-sharing counts and one statistic per sample pair
//                          (twk_hip_relationship: its own launches, beside the variant launch path)
//   topk (ld_topk.hip.h) cells -> one statistic of the pair's record -> a 64-bit key -> the k largest per variant, selected with integer atomic maxima (twk_hip_ld_topk)
//   subset (ld_subset.hip.h) the raw rows compacted to a list of samples: a working copy beside the rows as uploaded (twk_hip_select_samples)
//   varsel (ld_varsel.hip.h) a predicate per variant -> scan -> the rows and the metadata of the kept variants gathered beside the base (twk_hip_select_variants)
//   blocks (ld_blocks.hip.h) cells -> the record's 2 x 2 table -> a likelihood scan over 101 values of D' -> the bounds lo, hi as two bytes per in-window pair in band storage
//                          (twk_hip_ld_dprime_ci_band) -> prefix counts, candidates, sort, walk: haplotype blocks (twk_hip_ld_blocks)
//   split (ld_split.hip.h) the bandmat kind's r2 band, kept on the device -> integer row prefixes -> block sums -> one max-plus layer per k -> backtrack: the optimal
//                          split of a contig into near-independent LD blocks for every K (twk_hip_ld_split: no kind of its own, its kernels run behind the band's launches)
//   (score, prune, clump, matrix, decay, aggregate, annot, bandmat, topk and the bounds of dprime_ci / blocks are the kinds of one reduce path - Reduce, launch_reduce, ReduceCall; ld_reduce.hip.h holds what their kernels share)
// over super-tiles of the variant-pair triangle.  Device memory lives in the
// ctx; nothing here falls back to the CPU.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>
#include <chrono>
#include <string.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rccl/rccl.h>          // types only: the library is opened on first use (twk_hip_gather_records), never linked
#include <dlfcn.h>
#include <map>
#include <type_traits>

#include "../../../include/twk_hip.h"
#include "ld_count.hip.h"
#include "ld_prep.hip.h"
#include "ld_math.hip.h"
#include "ld_list.hip.h"
#include "ld_three.hip.h"
#include "ld_reduce.hip.h"
#include "ld_score.hip.h"
#include "ld_decay.hip.h"
#include "ld_aggregate.hip.h"
#include "ld_score_annot.hip.h"
#include "ld_prune.hip.h"
#include "ld_clump.hip.h"
#include "ld_matrix.hip.h"
#include "ld_bandmat.hip.h"
#include "ld_blocks.hip.h"
#include "ld_split.hip.h"
#include "ld_topk.hip.h"
#include "ld_relate.hip.h"
#include "ld_subset.hip.h"
#include "ld_varsel.hip.h"
#include "ld_plan.h"
#include "ld_form.h"
#include "twk_delivery.h"
#include "twk_buffers.h"

using namespace twk;

namespace {


// Every device and page-locked buffer of the engine is one of these (twk_buffers.h): the runtime's allocator behind the owner types.
struct HipMemOps {
	typedef hipError_t error;
	static constexpr hipError_t ok = hipSuccess, out_of_memory = hipErrorOutOfMemory;
	static hipError_t device_alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
	static void device_free(void* p) { (void)hipFree(p); }
	static hipError_t host_alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
	static void host_free(void* p) { (void)hipHostFree(p); }
};
template <class T> using DevBuf = Buffer<T, HipMemOps>;
template <class T> using PinnedBuf = Buffer<T, HipMemOps, true>;

struct PlaneSet {
	uint32_t* rows = nullptr;     // [rows_alloc][W]: own_rows, or the context's raw layout (which *is* the phased plane)
	DevBuf<uint32_t> own_rows;
	DevBuf<uint32_t> rowpop;      // [rows_alloc]
	uint32_t  W = 0;              // words per row (padded to KC)
	uint32_t  W_live = 0;         // words per row that carry data
	uint32_t  rows_alloc = 0;
	bool      built = false;
	// regrouped set only: position in the set -> variant id (device + host), and how many
	// variants with missing genotypes lead the set
	DevBuf<uint32_t> ids;
	std::vector<uint32_t> h_ids;
	uint32_t  n_front = 0;
	// allele-count-sorted phased set only (ld_list.hip.h): carrier lists of the variants that lead the set with at most
	// list_max carriers of their minor allele - positions [0, n_list), n_list a multiple of the tile edge
	DevBuf<uint32_t> lists, list_mac, list_flip;
	uint32_t  n_list = 0, list_max = 0;
	bool      lists_done = false;  // the lists have been built (or found not worth keeping): ensure_lists
	uint32_t  n_probe = 0;         // <= n_list: the leading variants whose lists are short enough for probing to beat the dense pair (ld_list.hip.h)
	// fused screen kernels: the prefilter's per-variant terms at the cut-off of the run that built them (ScreenWork::terms, k_screen_terms)
	DevBuf<float4> terms; double terms_cut = -1.0;
	// the two-product walk's planner (ld_plan.h plan_two_end): het and hom-alt carriers per position, copied from rowpop when first asked for
	std::vector<uint32_t> h_het, h_hom;
	// the prefix contraction: suffix popcounts of every plane row on the grid of stops, built the first time a call may take the form
	// (ensure_suffix) and kept with the set - on the host for the planner, [rows_alloc][PREFIX_GRID], and on the device for the screens, grid-major:
	// [PREFIX_GRID][rows_alloc]
	DevBuf<uint32_t> suffix; std::vector<uint32_t> h_suffix;
	// the carrier plane: H | Q of the variants [0, carrier_n) of the sorted unphased set, one row of W words each and a zeroed pad of one
	// tile of rows behind them (a tile stages 128 rows from its first) - the row operand of the two-product launches on long rows.  Built the first
	// time a call's cut needs it, grown when a later cut needs more rows (ensure_carrier), kept and dropped with the set.  carrier_rows: its first row,
	// placed inside carrier_buf so that it lies a whole number of rows from `rows` - CountWork addresses every row as rows + row x W, so a count launch
	// reaches both through one base and a row offset (carrier_operand_rows)
	DevBuf<uint32_t> carrier_buf; uint32_t* carrier_rows = nullptr; uint32_t carrier_n = 0;
};

// Plane sets a context can hold: one per PlaneKind in file order, plus the masked unphased planes
// regrouped so that the variants with missing genotypes come first (both groups in file order).
// Default-mode runs (reference: phased math unless either variant has missing data)
// then need the expensive 3-plane products only for the pairs that involve the leading group:
// a triangle over it plus its rectangle against the rest.
// ... and (TWK_HIP_OPT_R2_SCREEN) the plain phased / unphased planes in order of minor allele count, variants with
// missing genotypes last: in that order the pairs whose r2 can reach the cut-off at all - a bound from the two
// allele counts alone - are a band along the diagonal, and whole tiles outside it are never contracted.
enum { PS_GROUPED = 4, PS_SORTED_P = 5, PS_SORTED_U = 6, N_PLANE_SETS = 7 };
inline int set_kind(int set) {
	return set == PS_GROUPED ? (int)PK_UNPHASED_MASKED : set == PS_SORTED_P ? (int)PK_PHASED : set == PS_SORTED_U ? (int)PK_UNPHASED : set;
}
// internal modes of the two stages of such a run
enum { MODE_INT_AUTO_CLEAN = 0x10,     // phased math on the plain planes; pairs without missing data only
       MODE_INT_GROUPED    = 0x11,     // unphased math on the regrouped planes; every pair of the tile
       MODE_INT_SORTED_P   = 0x12,     // phased math on the allele-count-sorted planes (variants without missing data)
       MODE_INT_SORTED_U   = 0x13,     // unphased math on the allele-count-sorted planes
       MODE_INT_SORTED_U_ALL = 0x14 }; // ... without the r2 band, the list zone and the probe zone: every pair is contracted (the two-product walk)

constexpr int N_SLOT_COUNTERS = 16;      // (see Slot::n_out)
// Launches of a region call in flight.  Three, not two: the survivors of launch t are sorted on the copy stream, where they
// wait for a CU until the persistent count kernel of launch t + 1 lets go; with only t + 1 enqueued the device then idled
// until the host had sorted, copied and handed over launch t and come back with launch t + 2 (2,504 x 531,500, all pairs:
// 39 launches of 13 ms took 1.25 s).  With t + 2 already queued the count kernels run back to back.
constexpr int PIPE_SLOTS = 3, SYNC_SLOT = PIPE_SLOTS;
// What the running call of one of them sets, for its length: ~ReduceCall puts a default-constructed one back.
struct ReduceState {
	Reduce kind = Reduce::none;
	struct { PruneMap bits; MatrixMap matrix; DecayMap decay; AggMap agg; AnnotMap annot; BandMap band; TopkMap topk; CiMap ci; } map{};      // where the running kind's launches put their results (prune and clump: bits)
	uint64_t work = 0;                            // what the call's launches used up of the room of the kind's accumulators (launch_reduce holds it to the kind's limit)
};
// What twk_hip_*_last tells of an entry point's last call: the stages it timed on its stream (StageMarks; a stage it did not reach is 0)
// and the device memory it reports.  One per entry point, not per Reduce: that says which epilogue a launch takes, and calls share those.
struct CallReport { double stage_ms[4] = {0, 0, 0, 0}; uint64_t bytes = 0; };
struct LastCalls {
	CallReport prune, clump, matrix, bandmat, topk, blocks, split, relate;
	int32_t relate_planes = 0;      // planes a sample of the last relationship call
};
// What a slot's current launch is.  Every launch begins with a fresh one (begin_launch); after that a field is written only by the
// function that decides it.  (Buffers, capacities, events and counters outlive a launch: they are the Slot's.)
struct Launch {
	LaunchForm form;
	FormGrant given;                              // ... decided under this grant (enqueue_tile): what CallForms::gave_up reads when the launch is through
	bool is_list = false;                         // a carrier-list pass (ld_list.hip.h): C holds its candidate list
	bool is_probe = false;                        // ... of the probe kind (zone rows x columns outside the zone)
	// a band launch (region_impl): its pair math is enqueued once its candidate count is known (enqueue_band_math)
	bool deferred = false;
	bool was_deferred = false;                    // (the launch was one: its math runs between ev_c0b and ev_s1, not right behind the count kernel)
	const ScreenWork* d_screen_dev = nullptr;     // the parameter blocks of a fused or three-product launch on the device (behind the launch's unit table)
	StatsParams* d_stats_dev = nullptr;
	StatsParams stats_host;                       // ... and the host's copy of the second, patched with the survivor buffer before it is sent again
	bool presorted = false;                       // band launches: the survivors are in Slot::sorted, sorted on the compute stream right behind Fisher's test (close_launch)
	uint32_t* cand = nullptr;                     // the candidate list of the launch (in C)
	unsigned long long cand_cap = 0;              // ... of this many entries; n_out[2] counts them
	bool cand_overflow = false;                   // set by finish_tile: the list did not hold them all
	bool too_rich = false;                        // set by finish_tile: a three- or one-product launch with more candidates than the form is worth (ld_form.h: three_too_rich, one_too_rich)
	bool band_too_big = false;                    // a band launch whose candidates need more survivor / sort buffers than it may have (or could get): finish_tile reports
	                                              // it as an overflow and the launch's rows are redone as matrix-sized tiles
	int plane_set = 0;                            // the plane set the launch contracted
	double minP = 1.0;
	uint64_t row_pairs = 0, row_pairs_b = 0;      // plane-row pairs of the tiles its (up to two) count kernels contracted - a prefix launch's in full-row
	                                              // equivalents: x chunks contracted / chunks per row, summed over its tiles and rounded down once
	uint64_t extra_units = 0;                                // units of the (first) count launch beyond one a tile: parts of tiles cut along K, added into the matrix with atomics
	uint64_t prefix_chunks = 0, prefix_chunks_full = 0;      // a prefix launch: chunks its tiles were contracted over, and what whole rows would have been
};
// Room for the parameter block of a reduce launch of any kind (send_reduce_args): never read as a union, only sized and aligned as one.
union ReduceArgs { ScoreArgs score; PruneArgs prune; ClumpArgs clump; MatrixArgs matrix; DecayArgs decay; AggArgs aggregate; AnnotArgs annot; BandArgs bandmat; TopkArgs topk; CiArgs ci; };
struct Slot {                      // one in-flight tile (double buffered)
	Launch l;
	DevBuf<uint32_t> C;
	DevBuf<twk_hip_record> out;                   // survivor buffer (grow-only)
	DevBuf<unsigned long long> keys; DevBuf<uint32_t> vals;              // [capacity()]: sort key and position of every survivor, written where it is appended
	unsigned long long capacity() const { return shared_capacity(out, keys, vals); }
	unsigned long long cap_use = 0;               // ... of which the current launch may use this many (what the caller asked for)
	DevBuf<unsigned long long> n_out;             // device counters: [0] survivors appended, [1] of those dropped by the Fisher cut-off,
	                                              // [2] candidates of the fused count kernel, [3] three-product candidates whose recount disagrees, [4] shader cycles and
	                                              // [5] 100 MHz ticks the count kernel's blocks lived for (summed over the blocks), [6], [7] spare, [8 + x] the 100 MHz
	                                              // tick at which the last block on XCD x finished
	PinnedBuf<unsigned long long> h_n_out;        // pinned host copy of all of them (both live as long as the context)
	hipEvent_t ev_c0 = nullptr, ev_c1 = nullptr, ev_s1 = nullptr, ev_c0b = nullptr, ev_c1b = nullptr;
	DevBuf<twk_hip_record> sorted;                // band launches: the survivors in (idxA, idxB) order (Launch::presorted)
	// work lists of the (up to two) count launches of the tile: pinned host copy + device copy
	PinnedBuf<uint32_t> h_tiles[2]; DevBuf<uint32_t> d_tiles[2];
	// score launches (ld_score.hip.h): the blocks' row and column partials of the launch (grow-only)
	DevBuf<double> sc_sum; DevBuf<uint32_t> sc_n;
	// reduce launches (launch_reduce): the parameter blocks of the (up to two) passes, whatever the kind: pinned host copy + device copy
	PinnedBuf<ReduceArgs> h_args; DevBuf<ReduceArgs> d_args;
};

// Where a finished launch's sorted survivors go (finish_tile): appended to the device sink (!to_host), or to the host - left whole in
// c->h_recs (sink == null: the single-tile entry point), or handed to `sink`.
struct Deliver { bool to_host = true; twk_hip_record_sink sink = nullptr; void* user = nullptr; };

}  // namespace

namespace {
// Measurement and test switches (twk_hip_set_option): what used to be TWK_HIP_* environment variables.  The library
// reads no environment variable; a host that embeds it gets the defaults below unless it says otherwise.
// ONE table - X(key, default, lowest, highest, drops the derived plane sets, meaning): the Options struct, the key table of
// twk_hip_set_option / twk_hip_get_option and - through twk_hip_option_describe - the table of INTEGRATION.md 1 all come from it
// (tests/test_docs_consistency.py holds the document to it).
#define TWK_HIP_OPTIONS(X) \
	X(fused, 1, 0, 2, false, "fused count -> r2 screen kernel (no count matrix; DESIGN 3.2a): 0 never, 1 rows of <= 128 K chunks, 2 always") \
	X(three, 1, 0, 2, false, "UnphasedMath on planes without missing genotypes, r2 cut-off > 1e-6: contract three products a pair (HH and S = QH + HQ + 2 QQ: all the screen reads) and recount the four products of the pairs that pass (DESIGN 3.1a); 0: four products for every pair; 2: keep to three whatever a launch's candidate density (1 samples every launch first)") \
	X(uz, 1, 0, 1, false, "the three-product form through a count matrix (rows too long to fuse): contract U = popc(H_A | H_B) and Z = popc((Q_A ^ Q_B) & ~(H_A | H_B)) - two popcounts a word - in the place of HH and S, which the screen derives from them and the margins in integers (HH = hA + hB - U, S = qA + qB - Z; DESIGN 3.1a); candidates, recount and records are unchanged; 0: the three products themselves") \
	X(two, 1, 0, 2, false, "UnphasedMath, whole triangle without a window, rows too long to fuse, three = 1 and no tile edge given: walk the allele-count-sorted planes and contract two products a pair (HH and HQ of the row variant's H plane; S bounded from the margins) in the launches whose rows have few hom-alt carriers (DESIGN 3.1b); 0: never (the call walks the file order); 2: in every launch of that walk, whatever the predicate and the samples say") \
	X(carrier, 1, 0, 1, false, "the two-product walk on rows of more than 128 K chunks: its two-product launches contract the row variant's carrier plane (H or Q, bit by bit) in the H plane's place (CH = HH + QH and CQ = HQ + QQ: S >= CQ and S + HH <= CH + CQ + min(qA, qB)), which moves the walk's cut from p ~ 0.16 to ~ 0.21 at r2 >= 0.1; one more plane row per row variant in front of the cut, built on first use and kept with the planes (DESIGN 3.1b); 0: always the H plane") \
	X(one, 1, 0, 2, false, "the carrier form of the two-product walk: in front of the walk's cut a row block's columns up to its one_end - where the screen's lower test at S >= 0, a function of the two dosages alone, stops passing - are launches that contract one product a pair, the two variants' carrier rows (CC = CH + CQ: all the upper test reads), with carrier rows for the column variants too; the rest of the block's columns stay two-product launches (DESIGN 3.1b); 0: never; 1: launches whose sample in that form is poor in candidates; 2: every such launch whatever its sample") \
	X(one_rows, 0, 0, 32768, false, "... the height in variants of the row blocks in front of the cut, a multiple of 128 (0: half the super-tile edge, but no less than 1024 or the edge itself; 128: the test hook)") \
	X(cand_cap, 0, 0, 1 << 30, false, "test hook: at most this many entries in the candidate list of a two- or three-product launch through a matrix (0: the list's own size), so that a launch overflows and the ladder below it runs") \
	X(prefix, 1, 0, 2, false, "the two-product walk on rows of more than 128 K chunks: a launch contracts each tile over a prefix of its rows, up to a stop the planner chooses per tile, and its screen bounds the unread samples by the rows' suffix margins; what it keeps is recounted over the whole rows (DESIGN 3.1c); 0: never; 1: launches whose sample with stops is poor in candidates; 2: every eligible launch whatever its sample") \
	X(prefix_margin, 950, 1, 1000, false, "... the planner asks with the square root of the screen's bound shrunk to this many thousandths of it (950 as the two-product planner's two_margin = 0.95)") \
	X(prefix_sigma, 60, 0, 200, false, "... and, beside it, with the screen's own bound and the expected prefix counts moved outwards by this many tenths of their standard deviation under independence; a pair counts as decided at a stop where either question drops it (60: six standard deviations, the tighter of the two on rows of about a million samples; 0: the first question alone)") \
	X(walk_fine, 1, 0, 2, false, "the two-product walk's finer rounding (DESIGN 3.1b, 3.1c): a row block's borders are staircases - a block in front of the cut has its one_end per tile row of 128 variants, its one-product launches listing the tiles in front of it and its two-product launches those behind it, and the blocks behind the cut take a two-product launch from the diagonal to their rows' two_reach, up to two_last, with three products behind it; the carrier screens hold QQ to min(qA, qB, CQ) - the launch counted CQ itself - in the launches, their samples and the planner's questions; and a tile's stop is the planner's answer without the spare grid step wherever prefix_sigma is on; 0: never; 1: rows of at least 256 K chunks; 2: every row length the carrier and prefix forms take (more than 128 chunks: the test hook)") \
	X(walk_fine_sigma, 45, 0, 200, false, "... and where it applies prefix_sigma is this many tenths (45: the smallest of 60, 50 and 45 at which the headline recounts under 1 ms of candidates a step, no sample is refused and no launch redone - profiles/walk_fine_ab.txt; 0: prefix_sigma itself)") \
	X(prefix_stop, 0, 0, 32, false, "test hook: this point of the 32 coarse points of the grid of stops for every tile of a prefix launch (0: the planner's stops)") \
	X(prefix_substop, 0, 0, 3, false, "test hook: ... moved this many of the four sub-steps of a coarse interval further, to a point of the 128-point grid that need not be a coarse one (read only where prefix_stop is set)") \
	X(count_min_chunks, 8, 1, 1 << 20, false, "shortest K range a tile of the count kernel is split into at the end of a launch (test hook: 1 splits short rows too)") \
	X(patch_rows, 8, 1, 4096, false, "rows of a patch of tiles in the count kernel's work order (DESIGN 3.1, profiles/r03_patch_pmc.txt)") \
	X(patch_cols, 8, 1, 4096, false, "... and its columns") \
	X(seg, 0, 0, 1 << 20, false, "walk a patch in K segments of this many chunks (0: whole tiles)") \
	X(xcd_queues, 0, 0, 8, false, "one unit queue per XCD (2..8; 0: one queue): -42 % fabric traffic at +0.5 % kernel time") \
	X(skip_pad, 1, 0, 1, false, "leave the zero padding behind a row's last live 8 bytes uncontracted (0: contract it)") \
	X(cand_chunk, -1, -1, 1 << 20, false, "candidate slots a wave of the fused kernels reserves at a time (-1: sized from the list)") \
	X(lists, 1, 0, 2, true, "carrier lists for the rare head of the allele-count-sorted plane sets (DESIGN 3.5): 0 never, 1 rows of >= 4096 words, 2 always (lists of >= 8 carriers)") \
	X(list_max, 0, 0, 60000, true, "longest carrier list kept (0: row words / 128, / 64 for UnphasedMath)") \
	X(probe, 1, 0, 1, false, "pairs of a listed variant with one that keeps no list: probes of its carriers into the partner's row (0: the dense contraction)") \
	X(probe_zone, 1, 0, 1, false, "rows with a list short enough to probe take every column behind them that way, the list zone's own included (0: pairs inside the zone are merges of two lists)") \
	X(probe_lds, 1, 0, 1, false, "probe kernels: the column rows are staged into LDS segment by segment and the carriers tested there (512 zone rows x 4 columns a block; 2 columns of unphased planes); 0: gathers from L2, one column a block (the twin the LDS form is tested against)") \
	X(band_launch, 1, 0, 1, false, "fused runs: launches sized by their work - a band of rows over all the columns it reaches - instead of by a count matrix; 0: matrix-sized tiles only") \
	X(band_work_log2, 19, 0, 40, false, "... of at least 2^n tile-chunks each (19: about 5 ms of contraction)") \
	X(band_max_launches, 8, 1, 64, false, "... and at most this many a region") \
	X(band_list_entries, 0, 0, 1ll << 32, false, "candidate slots of such a launch (0: 1/32 of its pairs, 4 M .. 256 M); a launch that outgrows them, or its survivor buffer, is redone as matrix-sized tiles") \
	X(band_reverse, 1, 0, 1, false, "allele-count-sorted runs: the last band (commonest variants, most survivors) first") \
	X(fisher_order, 1, 0, 1, false, "Fisher's walks binned by their length (DESIGN 3.2)") \
	X(fisher_lds, 1, 0, 1, false, "log-factorial table in LDS while it fits") \
	X(async_delivery, 1, 0, 1, false, "region calls with a sink: a finished launch's sorted survivors are copied aside on the device and a second thread of the engine takes them to the host and calls the sink - in the launches' order, one call at a time - while the calling thread goes on enqueueing launches (twk_delivery.h); 0: the calling thread does both") \
	X(deliver_buffers, 3, 1, 64, false, "staging buffers that thread may hold at a time: a launch whose survivors find none free waits for one (back-pressure)") \
	X(record_cap, 0, 0, 1ll << 40, false, "test hook: cap on a launch's survivor buffer in records (0: none) - forces the overflow paths: a matrix-sized tile is redone in row strips, a band launch as matrix-sized tiles") \
	X(deliver_fail_alloc_at, 0, 0, 1 << 30, false, "test hook: the n-th staging allocation of a region call fails (the calling thread then delivers that launch itself)") \
	X(deliver_fail_copy_at, 0, 0, 1 << 30, false, "test hook: the n-th copy aside of a region call fails (the call fails)") \
	X(timeline, 0, 0, 1, false, "1: the host's steps through a region's launch pipeline, with times, and the outlier watch's findings on stderr")
struct Options {
#define X(key, dflt, lo, hi, rebuilds, doc) long long key = dflt;
	TWK_HIP_OPTIONS(X)
#undef X
};
struct OptionKey { const char* name; long long Options::* field; long long dflt, lo, hi; bool rebuilds_planes; const char* doc; };
const OptionKey OPTION_KEYS[] = {
#define X(key, dflt, lo, hi, rebuilds, doc) {#key, &Options::key, dflt, lo, hi, rebuilds, doc},
	TWK_HIP_OPTIONS(X)
#undef X
};
}  // namespace

// The delivery thread of a region call (twk_delivery.h): the queue's device operations.
struct twk_hip_ctx;
struct HipDeliveryOps {
	twk_hip_ctx* c = nullptr;
	long long n_alloc = 0, n_copy = 0;       // of the current call (test hooks deliver_fail_alloc_at / deliver_fail_copy_at)
	void* alloc(size_t bytes);
	void release(void* p);
	int copy_aside(void* dst, const void* src, size_t bytes);
	int deliver(const void* recs, uint64_t n, twk_hip_record_sink sink, void* user, char* err, size_t err_len);
	void thread_begin();
};
typedef twk::DeliveryQueue<HipDeliveryOps, twk_hip_record_sink> Delivery;

struct twk_hip_ctx {
	int device = 0;
	Options opt;
	hipStream_t s_compute = nullptr, s_copy = nullptr, s_deliver = nullptr;      // s_deliver: the delivery thread's copies to the host
	HipDeliveryOps dl_ops;
	Delivery dl{sizeof(twk_hip_record)};
	bool deliver_warm = false;       // s_deliver has carried a copy (HipDeliveryOps::thread_begin)
	uint32_t N = 0, M = 0, M_alloc = 0;
	uint32_t Wp = 0, Wu = 0;       // padded words per row: raw (2N bits) / unphased planes (N bits)
	DevBuf<uint32_t> raw;          // [M_alloc][Wp]
	DevBuf<uint32_t> rawmask;      // [M_alloc][Wp] or null
	bool any_missing = false;
	bool has_data = false;         // an upload or a generator has filled rows since twk_hip_set_problem
	// twk_hip_select_samples: while a selection is active the rows and the metadata as uploaded - the source - wait here, and raw, rawmask,
	// N, Wp, Wu, any_missing, the metadata and everything derived from them describe the working set
	struct Source {
		bool active = false;
		uint32_t N = 0, Wp = 0, Wu = 0;
		DevBuf<uint32_t> raw, rawmask;
		std::vector<twk_hip_variant_meta> h_meta;
	} source;
	struct { double ms = 0; uint64_t bytes_read = 0, bytes_written = 0; } select_last;      // of the last selection that ran the kernel
	// twk_hip_select_variants: while a variant selection is active the rows and the metadata it selected from - the base: the data as uploaded,
	// or the working set of an active sample selection - wait here, and raw, rawmask, M, M_alloc, any_missing, the metadata (device SoA and
	// h_meta) and everything derived from them describe the working set.  Nothing is copied when the selection is dropped: the buffers move back.
	struct VarBase {
		bool active = false;
		uint32_t M = 0, M_alloc = 0;
		bool any_missing = false;
		DevBuf<uint32_t> raw, rawmask, d_ac, d_an, d_pos, d_rid, d_missing;
		DevBuf<double> d_hwe;
		std::vector<twk_hip_variant_meta> h_meta;
		std::vector<uint32_t> h_map;       // working -> base
	} varbase;
	struct { double ms = 0; uint64_t bytes_read = 0, bytes_written = 0; } varsel_last;      // of the last variant selection that ran the kernels
	// metadata (device SoA) + host mirror
	DevBuf<uint32_t> d_ac, d_an, d_pos, d_rid, d_missing;
	DevBuf<double> d_hwe;
	DevBuf<double> d_lfact; int lfact_n = 0;       // lgamma(i + 1), i <= 2N: Fisher's log-binomials (ld_math.hip.h)
	DevBuf<uint32_t> d_fisher_bins;                // [2 * FISHER_BINS]: bin sizes and fill cursors of the walk-length order (s_compute only)
	std::vector<twk_hip_variant_meta> h_meta;
	std::vector<uint32_t> h_popc;  // ALT alleles per variant as counted on the device (r2 screen; empty until needed, dropped on upload)
	PlaneSet planes[N_PLANE_SETS];
	Slot slot[PIPE_SLOTS + 1];     // [0 .. PIPE_SLOTS): the pipeline of region calls; [SYNC_SLOT]: synchronous single-tile calls
	PinnedBuf<twk_hip_record> h_recs;   // pinned staging
	// twk_hip_set_device_sink: the survivors of region calls stay on the device, appended here tile by tile
	DevBuf<StatsParams> d_list_stats;             // parameter block of the list pass's math kernel (device copy)
	bool sorted_keeps_no_lists[2] = {false, false};      // [phased, unphased]: the allele-count-sorted set was built once for a run below the band's cut-off and
	                                                     // kept no carrier lists: such runs go the file-order way without building it again (cleared with the planes)
	bool device_sink = false;
	DevBuf<twk_hip_record> d_keep; unsigned long long d_keep_n = 0;
	// the survivors of a tile leave in (idxA, idxB) order: sort keys / permutation (double-buffered), the
	// reordered records, rocprim's scratch (grow-only)
	DevBuf<unsigned long long> d_sort_keys; DevBuf<uint32_t> d_sort_vals; DevBuf<twk_hip_record> d_sorted;      // (one capacity)
	DevBuf<char> d_sort_tmp;
	// the same for the sorts of band launches, which run on the compute stream (one at a time, in stream order) while a sort of
	// the other kind may be running on the copy stream
	DevBuf<unsigned long long> d_band_keys; DevBuf<uint32_t> d_band_vals;      // (one capacity)
	DevBuf<char> d_band_tmp;
	Graveyard<HipMemOps> graveyard;    // buffers outgrown while launches were in flight: freed when the call ends (flush_graveyard)
	twk_hip_timing timing{};
	std::vector<twk_hip_launch_stat> launch_ring; uint64_t launches_seen = 0;      // the outlier watch's log (twk_hip_launch_log): the last LAUNCH_RING count launches
	twk_hip_progress_cb progress_cb = nullptr; void* progress_user = nullptr;
	bool progress_muted = false;       // second stage of a default-mode run: its pairs were already counted
	uint32_t resident_blocks = 512;   // count-kernel blocks the chip holds at once (2 per CU)
	DevBuf<uint32_t> tickets;         // [2 * (PIPE_SLOTS + 1)][8] work tickets of the count launches: one set of queues per (slot, launch)
	// staging of twk_hip_upload_rle (grow-only): run bytes, descriptors, status word
	DevBuf<uint8_t> d_rle, d_rle_desc;
	DevBuf<int> d_status;
	DevBuf<uint32_t> d_col_hi;        // r2 screen: per-row column limit of the current region
	DevBuf<uint32_t> d_stair;         // the fine walk: per-row staircase border of the current region (RegionPlan::stair)
	// twk_hip_ld_score, _prune, _clump, _matrix, _decay, _aggregate, _score_annot, _matrix_band: the launches of the running call reduce their count matrices (launch_reduce) instead of keeping records
	ReduceState reduce;                                                          // which way and where to, for the length of the call (ReduceCall)
	// What the last call of each public entry point with a twk_hip_*_last took: its own report, whichever epilogue its launches ran
	// (ld_split's run bandmat's).  stage_ms - prune, clump: [0] the walk; matrix, bandmat: [0] the copy; topk: [0] copy and unpack;
	// blocks: prefix counts + candidate counts + scan, the emitting pass, the sort, the walk; split: the band's launches, prefixes +
	// block sums, the layers, the backtrack; relationship: [0] the transposition.  bytes: the bitmap, the matrix, the band, the lists,
	// the two bounds' bands, everything the split held, the samples' planes.
	LastCalls last;
	DevBuf<unsigned long long> d_counts;                                        // [3] of the call: [0] edges or records; prune [1] kept; clump [1] clumps [2] members
	// score: sums of r2 per variant (ld_score.hip.h)
	DevBuf<double> d_score_sum; DevBuf<unsigned long long> d_score_n;            // [M] accumulators, variant ids in file order
	// prune and clump: what their walks over the call's adjacency bitmap read and write (ld_prune.hip.h, ld_clump.hip.h; the bitmap is the ReduceCall's)
	DevBuf<unsigned long long> d_walk;                                           // prune's `removed` beyond LDS, clump's taken0 / `taken`
	DevBuf<uint8_t> d_prune_keep;                                                // [M]
	DevBuf<uint32_t> d_clump_order, d_clump_index;                               // the candidates in visiting order; index_of [M]
	// decay: exact sums of quantised r2 and counts per distance bin (ld_decay.hip.h)
	DevBuf<unsigned long long> d_decay;                                          // [3][n_bins] accumulators: acc_int, acc_frac, acc_n
	// aggregate: the two bins of every variant, packed (ld_aggregate.hip.h; the cells' accumulators are the ReduceCall's)
	DevBuf<uint32_t> d_agg_key;                                                  // [M]
	// (relationship: its planes, row lists and outputs live for the length of the call)
	char err[512] = {0};
};

namespace {

struct Events {                    // the events of one call, destroyed on every way out
	std::vector<hipEvent_t> v;
	Events() = default;
	Events(const Events&) = delete;
	~Events() { for (hipEvent_t e : v) if (e) (void)hipEventDestroy(e); }
	hipError_t add(size_t n) {
		for (size_t k = 0; k < n; ++k) { hipEvent_t e = nullptr; const hipError_t rc = hipEventCreate(&e); if (rc != hipSuccess) return rc; v.push_back(e); }
		return hipSuccess;
	}
	hipEvent_t operator[](size_t k) const { return v[k]; }
};
// The stages of one call on its stream: mark(st) records the next event where stage st of the call's report begins - or, NO_STAGE, where
// the stage in front merely ends - and once the stream has been waited for, write() puts the distance from every mark to the next one
// into the stage it begins.  A stage that no mark began keeps what the report held: 0 from the call's start.
struct StageMarks {
	static constexpr int NO_STAGE = -1;
	Events ev; std::vector<int> begins;      // begins[k]: the stage from mark k to mark k + 1
	hipError_t mark(int stage, hipStream_t s) {
		// (events are made eight at a time, in front of the call's first mark: making one between two marks would count as the stage's
		// time where the device has caught up with the host, as it has in split's layers; no call here has more than seven marks)
		hipError_t e = begins.size() < ev.v.size() ? hipSuccess : ev.add(8);
		if (e == hipSuccess) e = hipEventRecord(ev[begins.size()], s);
		if (e == hipSuccess) begins.push_back(stage);
		return e;
	}
	void write(CallReport& r) const {
		for (size_t k = 0; k + 1 < begins.size(); ++k) {
			float ms = 0;
			if (begins[k] != NO_STAGE && hipEventElapsedTime(&ms, ev[k], ev[k + 1]) == hipSuccess) r.stage_ms[begins[k]] = ms;
		}
	}
};

#define HIPCHK(ctx, call)                                                                         \
	do {                                                                                          \
		hipError_t e__ = (call);                                                                  \
		if (e__ != hipSuccess) {                                                                  \
			snprintf((ctx)->err, sizeof((ctx)->err), "%s failed: %s (%s:%d)", #call,              \
			         hipGetErrorString(e__), __FILE__, __LINE__);                                 \
			return e__ == hipErrorOutOfMemory ? TWK_HIP_E_NOMEM : TWK_HIP_E_DEVICE;               \
		}                                                                                         \
	} while (0)

void free_planes(twk_hip_ctx* c) {
	c->h_popc.clear();
	c->sorted_keeps_no_lists[0] = c->sorted_keeps_no_lists[1] = false;
	for (auto& p : c->planes) p = PlaneSet();
}
// (the slots' counters and the work tickets live as long as the context)
void free_slots(twk_hip_ctx* c) {
	for (auto& s : c->slot) {
		s.C.reset(); s.out.reset(); s.keys.reset(); s.vals.reset(); s.sorted.reset();
		s.sc_sum.reset(); s.sc_n.reset(); s.h_args.reset(); s.d_args.reset();
		for (int k = 0; k < 2; ++k) { s.h_tiles[k].reset(); s.d_tiles[k].reset(); }
	}
}
void free_problem(twk_hip_ctx* c) {
	free_planes(c);
	free_slots(c);
	c->raw.reset(); c->rawmask.reset(); c->d_lfact.reset(); c->lfact_n = 0;
	c->d_ac.reset(); c->d_an.reset(); c->d_pos.reset(); c->d_rid.reset(); c->d_missing.reset(); c->d_hwe.reset();
	c->d_score_sum.reset(); c->d_score_n.reset();
	c->d_counts.reset(); c->d_walk.reset(); c->d_prune_keep.reset(); c->d_clump_order.reset(); c->d_clump_index.reset();
	c->d_decay.reset(); c->d_agg_key.reset();
	c->h_meta.clear();
	c->source.raw.reset(); c->source.rawmask.reset(); c->source.h_meta.clear(); c->source.active = false;
	c->varbase = twk_hip_ctx::VarBase();
	c->N = c->M = c->M_alloc = 0; c->any_missing = false; c->has_data = false;
}

int plane_kind_for(const twk_hip_ctx* c, bool phased) {
	if (phased) return c->any_missing ? PK_PHASED_MASKED : PK_PHASED;
	return c->any_missing ? PK_UNPHASED_MASKED : PK_UNPHASED;
}

// The r2 screen's bound is a statement about the margins of the table the kernels count, so it takes the
// allele counts from the bits on the device, not from the `ac` field of the file (a .twk whose header
// disagrees with its genotypes must not lose records to the screen).
int ensure_popcounts(twk_hip_ctx* c) {
	if (c->h_popc.size() == c->M) return TWK_HIP_OK;
	DevBuf<uint32_t> d;
	HIPCHK(c, d.reserve(c->M, c->M, nullptr));
	hipLaunchKernelGGL(k_row_popcount, dim3((c->M + 3) / 4), dim3(256), 0, c->s_compute, c->raw, c->Wp, c->M, d);
	hipError_t e = hipGetLastError();
	c->h_popc.assign(c->M, 0);
	if (e == hipSuccess) e = hipMemcpyAsync(c->h_popc.data(), d, (size_t)c->M * 4, hipMemcpyDeviceToHost, c->s_compute);
	if (e == hipSuccess) e = hipStreamSynchronize(c->s_compute);
	if (e != hipSuccess) c->h_popc.clear();
	HIPCHK(c, e);
	return TWK_HIP_OK;
}

// The carrier lists of a sorted set (ld_list.hip.h), built when a run first wants them (ensure_lists: the r2-screen runs; the two-product walk
// over the same planes uses none and does not pay for them).
int build_lists(twk_hip_ctx* c, int set) {
	PlaneSet& ps = c->planes[set];
	{ const int rc = ensure_popcounts(c); if (rc) return rc; }
	// Carrier lists for the head of the set (ld_list.hip.h): worth it where a dense pair costs more than a merge of
	// two lists, i.e. for long rows only.  list_max = (phased row words) / 128 carriers for PhasedMath (the measured
	// break-even is ~W / 150 merge steps per side, profiles/r03_t2_list_vs_dense.txt) and twice that for UnphasedMath (a
	// dense unphased pair costs twice a phased one, a merge over samples about the same), and not below 32 - rows
	// shorter than 4096 words (N < 65,536) keep no lists.  Option "lists" = 0: never; 2: always, with at least 8 carriers
	// (test hook); "list_max" = n: the limit itself (measurement hook).
	const int lists_env = (int)c->opt.lists;
	uint32_t lmax = c->Wp / (set == PS_SORTED_U ? 64 : 128);      // measured optimum at N = 1 M: 488 / 976 carriers (profiles/r03_list_max_sweep.txt)
	if (lists_env == 2) lmax = std::max<uint32_t>(lmax, 8);
	if (c->opt.list_max >= 8) lmax = (uint32_t)c->opt.list_max;      // measurement hook (<= 60000: the unphased merge counts in 16 bits)
	if (lists_env != 0 && (c->Wp / 128 >= 32 || lists_env == 2)) {
		const uint64_t T2 = 2ull * c->N;
		uint32_t n = 0;                                  // variants of the missing-free head with a minor allele count <= lmax
		while (n < ps.n_front) {
			const uint64_t ac = std::min<uint64_t>(c->h_popc[ps.h_ids[n]], T2);
			if (std::min(ac, T2 - ac) > lmax) break;
			++n;
		}
		n = n / TILE * TILE;                             // whole tiles: a tile is either intersected or contracted
		if (n >= 2 * TILE) {
			ps.n_list = n; ps.list_max = lmax;
			// Probing (k_probe_screen) beats the dense pair up to ~W / 114 carriers in isolation (csrc/tools/probe_vs_dense.hip) and
			// up to about half that in a whole run, where the rows that reach beyond the zone are the ones with the longest lists and
			// the columns are thousands of 250 KB rows (1 M x 50,000: 10-11 ps per carrier against 5; with every list probing, the
			// default-cut-off run was 23 ms slower than without probes): PhasedMath probes lists of up to W / 256 carriers,
			// UnphasedMath - two reads per listed sample, a dense pair of twice the cost - of up to W / 160 entries.
			const uint32_t pmax = set == PS_SORTED_U ? std::max<uint32_t>(c->Wp / 160, 8) : std::max<uint32_t>(c->Wp / 256, 8);
			uint32_t np = 0;
			while (np < n) {
				const uint64_t ac = std::min<uint64_t>(c->h_popc[ps.h_ids[np]], T2);
				if (std::min(ac, T2 - ac) > pmax) break;
				++np;
			}
			ps.n_probe = np / TILE * TILE;
			HIPCHK(c, ps.lists.reserve((size_t)n * (lmax + 1), (size_t)n * (lmax + 1), nullptr));
			HIPCHK(c, ps.list_mac.reserve(n, n, nullptr));
			HIPCHK(c, ps.list_flip.reserve(n, n, nullptr));
			if (set == PS_SORTED_P)
				hipLaunchKernelGGL(k_build_lists, dim3((n + 3) / 4), dim3(256), 0, c->s_compute, (const uint32_t*)ps.rows, ps.W, ps.W_live, (uint64_t)T2,
				                   (const uint32_t*)ps.rowpop, n, lmax + 1, ps.lists, ps.list_mac, ps.list_flip);
			else
				hipLaunchKernelGGL(k_build_lists_unphased, dim3((n + 3) / 4), dim3(256), 0, c->s_compute, (const uint32_t*)ps.rows, ps.W, ps.W_live, c->N,
				                   (const uint32_t*)ps.rowpop, n, lmax + 1, ps.lists, ps.list_mac, ps.list_flip);
			HIPCHK(c, hipGetLastError());
		}
	}
	HIPCHK(c, hipStreamSynchronize(c->s_compute));
	return TWK_HIP_OK;
}

int build_planes(twk_hip_ctx* c, int set) {
	PlaneSet& ps = c->planes[set];
	const int kind = set_kind(set);
	const int P = planes_per_variant(kind);
	const bool wide = (kind == PK_PHASED || kind == PK_PHASED_MASKED);
	ps.W = wide ? c->Wp : c->Wu;
	ps.W_live = wide ? (uint32_t)((2ull * c->N + 31) / 32) : (c->N + 31) / 32;
	// (the sorted unphased set: a tile more - a two-product launch stages every other row of 128 variants, 256 plane rows from its last tile's first)
	ps.rows_alloc = round_up(c->M * P, TILE) + (set == PS_SORTED_U ? 2 * TILE : TILE);
	if ((kind == PK_PHASED_MASKED || kind == PK_UNPHASED_MASKED) && !c->rawmask) return TWK_HIP_E_STATE;
	const bool sorted = set == PS_SORTED_P || set == PS_SORTED_U;
	if (sorted) {
		// order: minor allele count ascending (ties in file order), variants with missing genotypes last (file order)
		const uint64_t T2 = 2ull * c->N;
		{ const int rc = ensure_popcounts(c); if (rc) return rc; }
		ps.h_ids.resize(c->M);
		for (uint32_t v = 0; v < c->M; ++v) ps.h_ids[v] = v;
		auto key = [&](uint32_t v) -> uint64_t {
			const twk_hip_variant_meta& m = c->h_meta[v];
			if (m.missing || m.an) return ~0ull;
			const uint64_t ac = std::min<uint64_t>(c->h_popc[v], T2);
			return std::min(ac, T2 - ac);
		};
		std::stable_sort(ps.h_ids.begin(), ps.h_ids.end(), [&](uint32_t a, uint32_t b) { return key(a) < key(b); });
		ps.n_front = 0;                                 // number of variants without missing genotypes (they lead the set)
		for (uint32_t v = 0; v < c->M; ++v) if (key(ps.h_ids[v]) != ~0ull) ++ps.n_front;
	}
	if (kind == PK_PHASED && !sorted) {
		ps.rows = c->raw;                             // the raw layout *is* the phased plane
	} else {
		const size_t words = (size_t)ps.rows_alloc * ps.W;
		HIPCHK(c, ps.own_rows.reserve(words, words, nullptr));
		ps.rows = ps.own_rows;
		HIPCHK(c, hipMemsetAsync(ps.rows, 0, words * 4, c->s_compute));
		if (sorted) {
			HIPCHK(c, ps.ids.reserve(c->M, c->M, nullptr));
			HIPCHK(c, hipMemcpyAsync(ps.ids, ps.h_ids.data(), (size_t)c->M * 4, hipMemcpyHostToDevice, c->s_compute));
		}
		if (set == PS_GROUPED) {
			ps.h_ids.clear(); ps.h_ids.reserve(c->M);
			for (uint32_t v = 0; v < c->M; ++v) if (c->h_meta[v].an) ps.h_ids.push_back(v);
			ps.n_front = (uint32_t)ps.h_ids.size();
			for (uint32_t v = 0; v < c->M; ++v) if (!c->h_meta[v].an) ps.h_ids.push_back(v);
			HIPCHK(c, ps.ids.reserve(c->M, c->M, nullptr));
			HIPCHK(c, hipMemcpyAsync(ps.ids, ps.h_ids.data(), (size_t)c->M * 4, hipMemcpyHostToDevice, c->s_compute));
		}
		const dim3 blk(256), grd((ps.W + 255) / 256, std::min<uint32_t>(c->M, 65535u));
		if (set == PS_SORTED_P)
			hipLaunchKernelGGL(k_permute_rows, grd, blk, 0, c->s_compute, c->raw, c->Wp, c->M, ps.rows, (const uint32_t*)ps.ids);
		else if (kind == PK_PHASED_MASKED)
			hipLaunchKernelGGL(k_build_phased_masked, grd, blk, 0, c->s_compute, c->raw, c->rawmask, c->Wp, c->M, ps.rows);
		else
			hipLaunchKernelGGL(k_build_unphased, grd, blk, 0, c->s_compute, c->raw,
			                   kind == PK_UNPHASED_MASKED ? c->rawmask : (const uint32_t*)nullptr,
			                   c->Wp, c->N, c->M, ps.rows, ps.W, P, (const uint32_t*)ps.ids);
		HIPCHK(c, hipGetLastError());
	}
	HIPCHK(c, ps.rowpop.reserve(ps.rows_alloc, ps.rows_alloc, nullptr));
	HIPCHK(c, hipMemsetAsync(ps.rowpop, 0, (size_t)ps.rows_alloc * 4, c->s_compute));
	const uint32_t live_rows = c->M * P;
	hipLaunchKernelGGL(k_row_popcount, dim3((live_rows + 3) / 4), dim3(256), 0, c->s_compute, ps.rows, ps.W, live_rows, ps.rowpop);
	HIPCHK(c, hipGetLastError());
	HIPCHK(c, hipStreamSynchronize(c->s_compute));
	ps.h_suffix.clear();
	ps.built = true;
	return TWK_HIP_OK;
}
// (a set whose build failed is left empty, not half-built)
int ensure_planes(twk_hip_ctx* c, int set) {
	if (c->planes[set].built) return TWK_HIP_OK;
	const int rc = build_planes(c, set);
	if (rc) c->planes[set] = PlaneSet();
	return rc;
}
// ... with its carrier lists, where the set keeps any (sorted sets only)
int ensure_lists(twk_hip_ctx* c, int set) {
	int rc = ensure_planes(c, set); if (rc) return rc;
	PlaneSet& ps = c->planes[set];
	if (ps.lists_done || !(set == PS_SORTED_P || set == PS_SORTED_U)) return TWK_HIP_OK;
	rc = build_lists(c, set);
	if (rc) { c->planes[set] = PlaneSet(); return rc; }
	ps.lists_done = true;
	return TWK_HIP_OK;
}

// ... with the suffix popcounts of its rows on the grid of stops (the prefix contraction): one pass over the planes and one copy to the
// host, the first time a call may take the form; kept with the set.  -> TWK_HIP_E_NOMEM leaves the set as it was (the call then takes no stops).
int ensure_suffix(twk_hip_ctx* c, int set) {
	int rc = ensure_planes(c, set); if (rc) return rc;
	PlaneSet& ps = c->planes[set];
	const size_t n = (size_t)ps.rows_alloc * PREFIX_GRID;
	if (ps.h_suffix.size() == n && ps.suffix) return TWK_HIP_OK;
	DevBuf<uint32_t> by_row;      // the kernel's own layout, which the host keeps; the device keeps its transpose
	HIPCHK(c, by_row.reserve(n, n, nullptr));
	HIPCHK(c, ps.suffix.reserve(n, n, nullptr));
	HIPCHK(c, hipMemsetAsync(by_row, 0, n * 4, c->s_compute));
	const uint32_t live_rows = c->M * (uint32_t)planes_per_variant(set_kind(set));
	hipLaunchKernelGGL(k_row_suffix_popcount, dim3((live_rows + 3) / 4), dim3(256), 0, c->s_compute, (const uint32_t*)ps.rows, ps.W, live_rows, by_row.get());
	HIPCHK(c, hipGetLastError());
	hipLaunchKernelGGL(k_suffix_grid_major, dim3((ps.rows_alloc + 31) / 32, PREFIX_GRID / 32), dim3(32, 8), 0, c->s_compute, (const uint32_t*)by_row.get(), ps.rows_alloc, ps.suffix.get());
	HIPCHK(c, hipGetLastError());
	ps.h_suffix.resize(n);
	HIPCHK(c, hipMemcpyAsync(ps.h_suffix.data(), by_row, n * 4, hipMemcpyDeviceToHost, c->s_compute));
	HIPCHK(c, hipStreamSynchronize(c->s_compute));
	return TWK_HIP_OK;
}

// ... with the carrier rows H | Q of its variants [0, n) (the two-product form's row operand on long rows): one streaming pass over those
// variants' planes, the first time a call's cut needs them and again when a later cut needs more; kept with the set.  -> TWK_HIP_E_NOMEM leaves the
// set without carrier rows (the call's two-product launches then contract the H planes as before).
int ensure_carrier(twk_hip_ctx* c, int set, uint32_t n) {
	int rc = ensure_planes(c, set); if (rc) return rc;
	PlaneSet& ps = c->planes[set];
	if (planes_per_variant(set_kind(set)) != 2) return TWK_HIP_E_STATE;
	n = std::min(n, c->M);
	if (ps.carrier_rows && ps.carrier_n >= n) return TWK_HIP_OK;
	HIPCHK(c, hipStreamSynchronize(c->s_compute));      // (nothing reads the rows that are replaced)
	ps.carrier_rows = nullptr; ps.carrier_n = 0;
	// a zeroed pad of one tile of rows behind the last, and one row of slack to place the first row in
	const size_t n_rows = (size_t)round_up(n, TILE) + TILE, words = (n_rows + 1) * ps.W;
	HIPCHK(c, ps.carrier_buf.reserve(words, words, nullptr));
	// the first row: the first address of the buffer that lies a whole number of rows from the set's planes, in front of them or behind (byte
	// distances: a row is W words, a multiple of 128 bytes, so the rows stay aligned like the planes')
	const intptr_t pitch = (intptr_t)ps.W * 4, d = (intptr_t)reinterpret_cast<uintptr_t>(ps.rows) - (intptr_t)reinterpret_cast<uintptr_t>(ps.carrier_buf.get());
	const intptr_t off = ((d % pitch) + pitch) % pitch, dist = (d - off) / pitch;      // rows from the first carrier row to the planes' first (negative: the planes lie in front)
	// (both operands of a launch are addressed from the lower of the two bases in 32-bit row numbers: CountWork::rowA0 / rowB0)
	if ((dist < 0 ? -dist : dist) + (intptr_t)std::max<size_t>(n_rows, ps.rows_alloc) >= (intptr_t)1 << 31) { ps.carrier_buf.reset(); return TWK_HIP_E_NOMEM; }
	uint32_t* first = ps.carrier_buf.get() + off / 4;
	// zeroed: the slack in front of the first row and everything behind row n - the pad; the kernel writes the rows [0, n) whole
	if (off) HIPCHK(c, hipMemsetAsync(ps.carrier_buf.get(), 0, (size_t)off, c->s_compute));
	HIPCHK(c, hipMemsetAsync(first + (size_t)n * ps.W, 0, (words - (size_t)off / 4 - (size_t)n * ps.W) * 4, c->s_compute));
	if (n) {
		hipLaunchKernelGGL(k_build_carrier, dim3((ps.W / 4 + 255) / 256, std::min<uint32_t>(n, 65535u)), dim3(256), 0, c->s_compute, (const uint32_t*)ps.rows, ps.W, n, first);
		HIPCHK(c, hipGetLastError());
	}
	HIPCHK(c, hipStreamSynchronize(c->s_compute));
	ps.carrier_rows = first; ps.carrier_n = n;
	return TWK_HIP_OK;
}
// A buffer a form could use and the call can do without (`rc` of its ensure_*): no room for it - the runtime's error and the context's message
// are cleared, what there is of it is dropped (`reset`) and the call goes on without; any other failure ends the call.
template <class Reset> int or_go_without(twk_hip_ctx* c, int rc, Reset reset) {
	if (rc != TWK_HIP_E_NOMEM) return rc;
	(void)hipGetLastError(); c->err[0] = 0; reset();
	return TWK_HIP_OK;
}
// The two operands of a count launch whose row axis walks the carrier rows from variant rowA0 on and whose column axis the planes from plane row rowB0 on,
// as CountWork addresses them: one base and two row numbers (ensure_carrier placed the carrier rows a whole number of rows from the planes).
struct OperandRows { const uint32_t* base; uint32_t rowA0, rowB0; };
OperandRows carrier_operand_rows(const PlaneSet& ps, uint32_t rowA0, uint32_t rowB0) {
	const intptr_t pitch = (intptr_t)ps.W * 4;
	const intptr_t dist = ((intptr_t)reinterpret_cast<uintptr_t>(ps.carrier_rows) - (intptr_t)reinterpret_cast<uintptr_t>(ps.rows)) / pitch;
	if (dist >= 0) return OperandRows{ps.rows, (uint32_t)dist + rowA0, rowB0};
	return OperandRows{ps.carrier_rows, rowA0, (uint32_t)(-dist) + rowB0};
}

// C_words words of count matrix / candidate list and `capacity` survivors for the slot's next launch.
int ensure_slot(twk_hip_ctx* c, Slot& s, size_t C_words, unsigned long long capacity) {
	HIPCHK(c, s.C.reserve(C_words, C_words, &c->graveyard));
	HIPCHK(c, reserve_together(capacity, capacity, &c->graveyard, s.out, s.keys, s.vals));
	s.cap_use = capacity;
	return TWK_HIP_OK;
}

// (err: where a failure's text goes - c->err on the calling thread, the delivery queue's own buffer on its thread)
#define HIPCHK_E(err, err_len, call)                                                              \
	do {                                                                                          \
		hipError_t e__ = (call);                                                                  \
		if (e__ != hipSuccess) {                                                                  \
			snprintf((err), (err_len), "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__, __LINE__); \
			return e__ == hipErrorOutOfMemory ? TWK_HIP_E_NOMEM : TWK_HIP_E_DEVICE;               \
		}                                                                                         \
	} while (0)

// The fine walk (option "walk_fine"; ld_plan.h PlanEnv::fine, PrefixEnv::fine; ScreenWork::fine) on rows of this many K chunks.  By default from 256
// chunks on: the carrier and prefix forms begin behind 128, and up to 256 the grid of 128 stops coincides with the chunks.
bool walk_fine_applies(const twk_hip_ctx* c, uint32_t row_chunks) {
	return c->opt.walk_fine == 2 ? row_chunks > FUSED_MAX_CHUNKS : c->opt.walk_fine == 1 && row_chunks >= 256;
}

int ensure_host_records(twk_hip_ctx* c, unsigned long long n, char* err = nullptr, size_t err_len = 0) {
	if (!err) { err = c->err; err_len = sizeof(c->err); }
	HIPCHK_E(err, err_len, c->h_recs.reserve(n, std::max<unsigned long long>(n, 1ull << 16), nullptr));      // (freed at once: also called on the delivery thread)
	return TWK_HIP_OK;
}

// Launch the count kernel for one tile on the compute stream (which: first or second launch of the slot - its event pair, ev_c0 / ev_c1
// or ev_c0b / ev_c1b, and its row_pairs field follow from it).
// form.fused: the fused kernels (k_count_screen_t) - no tile's K range is split, and the slot's C buffer holds the candidate list
// instead of counts.  form.three: the three-product form - fused, or k_count3_list_t into an (HH, S) matrix.
// The two parameter blocks of a fused or three-product launch (fa) travel to the device behind the tile list and the unit table (one
// copy per launch): the kernels read them from memory where they need them instead of holding ~60 more scalar registers through the
// contraction loop / the candidate loop.  Where they landed: Launch::d_screen_dev / d_stats_dev (null: no tiles, nothing was launched).
struct FusedArgs { ScreenWork screen; StatsParams stats; int unphased; };
int launch_count(twk_hip_ctx* c, int set, const twk_hip_tile_desc& t, Slot& s, int which, const ColRange* cr, const LaunchForm& form, const FusedArgs* fa) {
	const hipEvent_t e0 = which ? s.ev_c0b : s.ev_c0, e1 = which ? s.ev_c1b : s.ev_c1;
	const bool fuse = form.fused, three = form.three, two = form.two, with_args = fuse || three || two;       // with_args: the parameter blocks go to the device behind the unit table
	if (with_args != (fa != nullptr)) return TWK_HIP_E_STATE;
	const PlaneSet& ps = c->planes[set];
	// two products: one plane row - the H plane, every other row - per row variant, so tiles of 128 row variants x 64 column variants
	// ... or, a carrier launch, consecutive rows of the set's carrier plane (ensure_carrier): same tiles, same table, rows of their own
	// ... or, a one-product launch, such rows on both axes: one row per variant, tiles of 128 x 128 variants, the table geometry of a set with one
	// plane per variant (P = PA = 1 from here on; the planes themselves are not read)
	const int P_set = planes_per_variant(set_kind(set));
	if (two && (P_set != 2 || fuse || which != 0)) return TWK_HIP_E_STATE;
	if ((form.carrier && !two) || (form.one && !form.carrier) || (form.uz && !form.three_plain())) return TWK_HIP_E_STATE;
	const int P = form.one ? 1 : P_set;
	const int PA = two ? 1 : P;
	const uint32_t stepA = form.carrier ? 1u : (uint32_t)(P / PA);
	const Geometry g = tile_geometry(P, t, PA);
	if (form.carrier) {      // every row variant has its carrier row, and a tile's 128 rows end inside the zeroed pad
		if (!ps.carrier_rows || (uint64_t)t.rowA0 + t.nA > ps.carrier_n || (uint64_t)t.rowA0 + g.rowsA > (uint64_t)round_up(ps.carrier_n, TILE) + TILE) return TWK_HIP_E_STATE;
		if (form.one) {      // ... and so has every column variant
			if ((uint64_t)t.rowB0 + t.nB > ps.carrier_n || (uint64_t)t.rowB0 + g.rowsB > (uint64_t)round_up(ps.carrier_n, TILE) + TILE) return TWK_HIP_E_STATE;
		} else if ((uint64_t)t.rowB0 * P + g.rowsB > ps.rows_alloc) return TWK_HIP_E_INVALID;
	} else if (((uint64_t)t.rowA0 * PA + g.rowsA) * stepA > ps.rows_alloc || (uint64_t)t.rowB0 * P + g.rowsB > ps.rows_alloc) return TWK_HIP_E_INVALID;
	if (g.gx > 0xFFFFu || g.gy > 0xFFFFu) return TWK_HIP_E_INVALID;
	const bool diag = t.diag && t.rowA0 == t.rowB0;
	// the tiles and the units of work (ld_count_table.h; "count_min_chunks" is a test hook: 1 splits short rows too; "seg" 0: whole tiles and
	// "xcd_queues": see build_tile_list for the measurement behind them)
	CountSettings cs;
	cs.patch_rows = (uint32_t)c->opt.patch_rows; cs.patch_cols = (uint32_t)c->opt.patch_cols; cs.min_chunks = (uint32_t)c->opt.count_min_chunks;
	cs.seg_chunks = (uint32_t)c->opt.seg; cs.xcd_queues = (uint32_t)c->opt.xcd_queues; cs.n_blocks = c->resident_blocks; cs.fused = fuse;
	// A prefix launch: every tile gets a stop from the planner (ld_plan.h plan_prefix_tile_grid: the tile's variants on both axes,
	// asked in the order of the list, each question starting from its neighbour's answer); the grid indices travel to the device behind the
	// parameter blocks, one byte per tile of the super-tile's grid, for the screen.
	const uint32_t nchunks = ps.W / KC;
	std::vector<uint8_t> pre_grid;
	PrefixEnv pe;
	PrefixTileStops stop_of{&pe, two, t.rowA0, t.rowB0, t.nA, t.nB, g.gx, &pre_grid, {PREFIX_GRID, PREFIX_GRID, PREFIX_GRID, PREFIX_GRID, PREFIX_GRID}};
	if (form.prefix) {
		if (!(two || three) || fuse || which != 0 || P_set != 2 || ps.h_suffix.size() != (size_t)ps.rows_alloc * PREFIX_GRID || ps.h_het.size() != c->M) return TWK_HIP_E_STATE;
		pe.het = ps.h_het.data(); pe.hom = ps.h_hom.data(); pe.suffix = ps.h_suffix.data();
		pe.n_variants = c->M; pe.n_samples = c->N; pe.nchunks = nchunks;
		pe.cut = fa->screen.cut; pe.margin = (double)c->opt.prefix_margin / 1000.0; pe.sigma = (double)c->opt.prefix_sigma / 10.0; pe.carrier = form.carrier; pe.one = form.one;
		pe.fine = walk_fine_applies(c, nchunks);
		if (pe.fine && c->opt.walk_fine_sigma > 0 && c->opt.prefix_sigma > 0) pe.sigma = (double)c->opt.walk_fine_sigma / 10.0;
		pe.fixed_grid = c->opt.prefix_stop ? (uint32_t)c->opt.prefix_stop * PREFIX_SUB + (uint32_t)c->opt.prefix_substop : 0;
		pre_grid.assign((size_t)g.gy * g.gx, (uint8_t)PREFIX_GRID);
	}
	std::vector<uint32_t> stops;
	const CountTable tb = form.prefix ? build_count_table(t, P, diag, cr, nchunks, cs, PA, &stop_of, &stops) : build_count_table(t, P, diag, cr, nchunks, cs, PA);
	const size_t T = tb.n_tiles();
	const size_t words_units = tb.words(), fa_words = (sizeof(FusedArgs) + 15) / 16 * 4, pre_words = (pre_grid.size() + 3) / 4;
	const size_t words = words_units + (with_args ? fa_words : 0) + pre_words;   // [tiles | pad | units | FusedArgs | a prefix launch's stops] for a fused or three-product launch
	// (parked, the pinned one too: the device copy of the previous launch's table may still be travelling)
	HIPCHK(c, reserve_together(words, std::max<size_t>(words, 16384), &c->graveyard, s.h_tiles[which], s.d_tiles[which]));
	if (T) {
		tb.pack(s.h_tiles[which]);
		if (with_args) std::memcpy(s.h_tiles[which] + words_units, fa, sizeof(FusedArgs));
		if (form.prefix) {
			uint32_t* at = s.h_tiles[which] + words_units + fa_words;
			at[pre_words - 1] = 0;
			std::memcpy(at, pre_grid.data(), pre_grid.size());
			ScreenWork& sw = reinterpret_cast<FusedArgs*>(s.h_tiles[which] + words_units)->screen;
			sw.pre_stops = reinterpret_cast<const uint8_t*>(s.d_tiles[which] + words_units + fa_words); sw.pre_suffix = ps.suffix;
			sw.pre_gx = g.gx; sw.pre_tvA = stop_of.tvA(); sw.pre_nchunks = nchunks; sw.pre_rows = ps.rows_alloc;
		}
		HIPCHK(c, hipMemcpyAsync(s.d_tiles[which], s.h_tiles[which], words * 4, hipMemcpyHostToDevice, c->s_compute));
	}
	HIPCHK(c, hipEventRecord(e0, c->s_compute));
	if (T) {
		const uint32_t last_halves = c->opt.skip_pad ? count_last_halves(ps.W_live, ps.W) : 0;      // (measurement hook: 0 = contract the zero padding too)
		const OperandRows op = form.one ? OperandRows{ps.carrier_rows, t.rowA0, t.rowB0}      // (both operands are carrier rows: their own base)
		                     : form.carrier ? carrier_operand_rows(ps, t.rowA0, t.rowB0 * P) : OperandRows{ps.rows, t.rowA0 * PA, t.rowB0 * P};
		const CountWork w = count_work(op.base, ps.W, op.rowA0, op.rowB0, s.d_tiles[which], tb, s.C, g.ldc,
		                               c->tickets + ((&s - c->slot) * 2 + which) * 8, last_halves, s.n_out + 4, stepA);
		HIPCHK(c, hipMemsetAsync(w.ticket, 0, 8 * 4, c->s_compute));
		const FusedArgs* d_fa = reinterpret_cast<const FusedArgs*>(s.d_tiles[which] + words_units);
		if (with_args) { s.l.d_stats_dev = const_cast<StatsParams*>(&d_fa->stats); s.l.d_screen_dev = &d_fa->screen; }
		// one kernel: into the candidate list (fused) or into a matrix; a density sample's runs under a name of its own (LaunchForm::sample)
		void (*k_list)(CountWork, const ScreenWork*) = nullptr;
		void (*k_matrix)(CountWork) = nullptr;
		if (fuse && three) k_list = form.sample ? k_count3_screen_unphased_t<COUNT_NW, 1> : k_count3_screen_unphased_t<COUNT_NW>;
		else if (form.uz) k_matrix = form.sample ? k_count3_uz_list_t<COUNT_NW, 1> : k_count3_uz_list_t<COUNT_NW>;
		else if (three) k_matrix = form.sample ? k_count3_list_t<COUNT_NW, 1> : k_count3_list_t<COUNT_NW>;
		else if (fuse) k_list = form.unphased ? k_count_screen_unphased_t<COUNT_NW> : k_count_screen_t<COUNT_NW>;
		else k_matrix = (two && form.sample) ? k_count_list_t<COUNT_NW, 1> : k_count_list_t<COUNT_NW>;
		const uint32_t tile_rows = three ? TILE / 2 : TILE;
		if (k_list) HIPCHK(c, enqueue_count(c->s_compute, w, tb, cs.n_blocks, tile_rows, nullptr, k_list, &d_fa->screen));
		else HIPCHK(c, enqueue_count(c->s_compute, w, tb, cs.n_blocks, tile_rows, nullptr, k_matrix));
	}
	HIPCHK(c, hipEventRecord(e1, c->s_compute));
	(which ? s.l.row_pairs_b : s.l.row_pairs) = (uint64_t)T * TILE * TILE;
	if (!which) s.l.extra_units = tb.n_units() > T ? tb.n_units() - T : 0;
	if (form.prefix) {      // full-row equivalents: what the launch's time is set against (bench.py's roofline, the outlier watch)
		uint64_t done = 0;
		for (uint32_t st : stops) done += st;
		s.l.prefix_chunks = done; s.l.prefix_chunks_full = (uint64_t)T * nchunks;
		s.l.row_pairs = (uint64_t)TILE * TILE * done / nchunks;
	}
	return TWK_HIP_OK;
}

// Bits of idxB in the sort key idxA << shift | idxB of a survivor.
uint32_t key_shift_for(uint32_t n_variants) { uint32_t b = 1; while (b < 32 && (1ull << b) < n_variants) ++b; return b; }

StatsParams make_stats(twk_hip_ctx* c, int set, const twk_hip_tile_desc& t, const Slot& s, bool phased_math,
                       int auto_select, const twk_hip_filters& f, const ColRange* cr = nullptr) {
	const PlaneSet& ps = c->planes[set];
	const int kind = set_kind(set);
	const int P = planes_per_variant(kind);
	StatsParams p;
	p.tv.C = s.C; p.tv.ldc = tile_geometry(P, t).ldc; p.tv.rowpop = ps.rowpop; p.tv.kind = kind;
	p.tv.n_samples = c->N; p.tv.a0 = t.rowA0; p.tv.b0 = t.rowB0; p.tv.ids = ps.ids;
	p.vm = VariantMeta{c->d_ac, c->d_an, c->d_pos, c->d_rid, c->d_missing, c->d_hwe};
	p.raw = c->raw; p.rawmask = c->rawmask; p.Wp = c->Wp;
	p.col_hi = cr ? cr->d_hi : nullptr; p.hi_a0 = cr ? cr->a0 : 0; p.hi_b0 = cr ? cr->b0 : 0; p.col_lo = cr ? cr->d_lo : nullptr;
	p.list_zone = cr ? cr->list_zone : 0; p.probe_zone = cr ? cr->probe_zone : 0;
	p.nA = t.nA; p.nB = t.nB; p.n_variants = c->M;
	p.diag = (t.diag && t.rowA0 == t.rowB0) ? 1 : 0;
	p.phased_math = phased_math ? 1 : 0; p.auto_select = auto_select;
	p.window = t.window; p.l_window = t.l_window;
	p.filt = f; p.out = s.out; p.capacity = s.cap_use; p.n_out = s.n_out;
	p.keys = s.keys; p.vals = s.vals; p.key_shift = key_shift_for(c->M);
	return p;
}

uint64_t pairs_in_tile(const twk_hip_ctx* c, const twk_hip_tile_desc& t) {
	const uint64_t nA = t.rowA0 >= c->M ? 0 : std::min<uint64_t>(t.nA, c->M - t.rowA0);
	const uint64_t nB = t.rowB0 >= c->M ? 0 : std::min<uint64_t>(t.nB, c->M - t.rowB0);
	if (t.diag && t.rowA0 == t.rowB0) { const uint64_t n = std::min(nA, nB); return n * (n - 1) / 2 + (nB > n ? n * (nB - n) : 0); }
	return nA * nB;
}

// What a mode runs on a tile: one or two (plane set, math, pair selection) passes.
struct TilePlan { int set1, set2; bool phased1; int select1; int Pmax; };
TilePlan plan_for(const twk_hip_ctx* c, int mode) {
	TilePlan p{PK_PHASED, -1, true, 0, 1};
	switch (mode) {
	case TWK_HIP_MODE_PHASED:   p.set1 = plane_kind_for(c, true); break;
	case TWK_HIP_MODE_UNPHASED: p.set1 = plane_kind_for(c, false); p.phased1 = false; break;
	case MODE_INT_AUTO_CLEAN:   p.select1 = 1; break;
	case MODE_INT_GROUPED:      p.set1 = PS_GROUPED; p.phased1 = false; break;
	case MODE_INT_SORTED_P:     p.set1 = PS_SORTED_P; break;
	case MODE_INT_SORTED_U: case MODE_INT_SORTED_U_ALL: p.set1 = PS_SORTED_U; p.phased1 = false; break;
	default:                    // AUTO on one tile: plain phased (pairs without missing) then masked unphased
		if (c->any_missing) { p.select1 = 1; p.set2 = PK_UNPHASED_MASKED; }
		break;
	}
	p.Pmax = planes_per_variant(set_kind(p.set1));
	if (p.set2 >= 0) p.Pmax = std::max(p.Pmax, planes_per_variant(set_kind(p.set2)));
	return p;
}

// Fisher's exact test, one record per lane, on recs[0, min(*n_out, cap)): starting points (k_fisher_prepare), then the
// walks (k_ld_fisher_t) - in the order of their length (k_fisher_scatter) when `scratch` (scratch_words uint32, free at
// this point of the stream) is given; records beyond the scratch keep their place.  ld_math.hip.h.
// Option "fisher_order" = 0: walks in the order the records were appended; "fisher_lds" = 0: log-factorial table read
// from global memory also when it would fit LDS (measurement hooks).
int launch_fisher(twk_hip_ctx* c, twk_hip_record* recs, unsigned long long* n_out, unsigned long long cap, double minP,
                  uint32_t* scratch, size_t scratch_words, unsigned long long* keys = nullptr) {
	const LFact lf{c->d_lfact, c->lfact_n};
	const bool ordered = c->opt.fisher_order != 0, lds_ok = c->opt.fisher_lds != 0;
	const bool lds_table = lds_ok && c->lfact_n <= FISHER_LDS_TABLE_MAX;
	const size_t lds_bytes = lds_table ? (size_t)c->lfact_n * sizeof(double) : 0;
	HIPCHK(c, c->d_fisher_bins.reserve(2 * FISHER_BINS, 2 * FISHER_BINS, nullptr));
	const unsigned long long limit = (ordered && scratch && scratch_words >= 4096) ? std::min<unsigned long long>(scratch_words, 0xFFFFFFFFull) : 0;
	HIPCHK(c, hipMemsetAsync(c->d_fisher_bins, 0, 2 * FISHER_BINS * sizeof(uint32_t), c->s_compute));
	if (lds_table) hipLaunchKernelGGL(k_fisher_prepare<true>, dim3(c->resident_blocks), dim3(1024), lds_bytes, c->s_compute, recs, (const unsigned long long*)n_out, cap, lf, limit, c->d_fisher_bins);
	else hipLaunchKernelGGL(k_fisher_prepare<false>, dim3(c->resident_blocks * 2), dim3(256), 0, c->s_compute, recs, (const unsigned long long*)n_out, cap, lf, limit, c->d_fisher_bins);
	if (limit) {
		const unsigned long long bound = std::min(cap, limit);
		const unsigned blocks = (unsigned)std::max<unsigned long long>(1, std::min<unsigned long long>(c->resident_blocks * 4ull, (bound + 1023) / 1024));
		hipLaunchKernelGGL(k_fisher_scatter, dim3(blocks), dim3(256), 0, c->s_compute, (const twk_hip_record*)recs, (const unsigned long long*)n_out, cap, limit, c->d_fisher_bins, scratch);
	}
	if (lds_table) hipLaunchKernelGGL(k_ld_fisher_t<true>, dim3(c->resident_blocks), dim3(1024), lds_bytes, c->s_compute, recs, n_out, cap, minP, lf,
	                                  (const uint32_t*)(limit ? scratch : nullptr), limit, 1, keys);
	else hipLaunchKernelGGL(k_ld_fisher_t<false>, dim3(c->resident_blocks * 2), dim3(256), 0, c->s_compute, recs, n_out, cap, minP, lf,
	                        (const uint32_t*)(limit ? scratch : nullptr), limit, 1, keys);
	HIPCHK(c, hipGetLastError());
	return TWK_HIP_OK;
}

// The form of the (first) launch of a tile of this plan under the grant of the launch's owner: the facts - the plan, the cut-off, the options "fused",
// "three" and "two", the running reduce kind - gathered for decide_form (ld_form.h), which is the one place that weighs them.  Row lengths are read
// last and only where a launch may fuse, from planes built here if need be (a set that cannot be built: no fused form; enqueue_tile reports why).
LaunchForm launch_form(twk_hip_ctx* c, const TilePlan& pl, const twk_hip_filters& f, const FormGrant& grant) {
	FormFacts x;
	const int k = set_kind(pl.set1);
	x.two_pass = pl.set2 >= 0; x.reduce = c->reduce.kind; x.sorted_u = pl.set1 == PS_SORTED_U;
	x.phased_plain = pl.phased1 && k == PK_PHASED; x.unphased_plain = !pl.phased1 && k == PK_UNPHASED;
	x.cut_screens = f.minR2 > 1e-6 && f.minR2 <= 1.0;
	x.opt_fused = c->opt.fused; x.opt_three = c->opt.three; x.opt_two = c->opt.two; x.opt_prefix = c->opt.prefix; x.opt_carrier = c->opt.carrier; x.opt_one = c->opt.one; x.opt_uz = c->opt.uz;
	if (grant.carrier && c->opt.carrier != 0 && ensure_planes(c, pl.set1) == TWK_HIP_OK && c->planes[pl.set1].carrier_rows) x.carrier_chunks = c->planes[pl.set1].W / KC;
	// (stops are not combined with the measurement hooks that walk a tile's K range their own way)
	if (grant.prefix && c->opt.prefix != 0 && c->opt.seg == 0 && c->opt.xcd_queues == 0 && ensure_planes(c, pl.set1) == TWK_HIP_OK) x.row_chunks = c->planes[pl.set1].W / KC;
	if (may_screen(x, grant) && x.opt_fused != 0) {
		if (ensure_planes(c, pl.set1) == TWK_HIP_OK) x.chunks = c->planes[pl.set1].W / KC;
		else x.opt_fused = 0;
	}
	return decide_form(x, grant);
}
// Would a launch of this mode run the fused count -> screen form and nothing else (one pass), as far as the call still allows it?  For the callers
// that size a launch by it.
bool fused_form_applies(twk_hip_ctx* c, int mode, const twk_hip_filters& f, const CallForms& calls) {
	const LaunchForm lf = launch_form(c, plan_for(c, mode), f, calls.grant(LaunchWants()));
	return lf.fused && !lf.two_pass;
}

// The four products of the candidates of a three-product launch (k_recount_unphased), on the compute stream: a wave per candidate for
// long rows, a DPP row of 16 lanes for rows of up to 1024 words.  The recount also checks the contraction: a candidate whose (HH, S)
// disagrees with its own four products is counted in n_out[3], and finish_tile fails the call on it.
int launch_recount(twk_hip_ctx* c, int set, Slot& s) {
	const PlaneSet& ps = c->planes[set];
	if (ps.W_live <= 1024)
		hipLaunchKernelGGL(k_recount_unphased<16>, dim3(c->resident_blocks * 4), dim3(256), 0, c->s_compute, (const uint32_t*)ps.rows, ps.W, ps.W_live, s.l.cand,
		                   (const unsigned long long*)(s.n_out + 2), s.l.cand_cap, s.n_out + 3, s.l.form.one ? 3 : s.l.form.carrier ? 2 : s.l.form.two ? 1 : 0, s.l.form.prefix ? 1 : 0);
	else
		hipLaunchKernelGGL(k_recount_unphased<64>, dim3(c->resident_blocks * 4), dim3(256), 0, c->s_compute, (const uint32_t*)ps.rows, ps.W, ps.W_live, s.l.cand,
		                   (const unsigned long long*)(s.n_out + 2), s.l.cand_cap, s.n_out + 3, s.l.form.one ? 3 : s.l.form.carrier ? 2 : s.l.form.two ? 1 : 0, s.l.form.prefix ? 1 : 0);
	HIPCHK(c, hipGetLastError());
	return TWK_HIP_OK;
}

// The end of every reduce launch: the parameter block `a` of pass `which` into the slot's pinned block and from there to the device, on the stream of
// `kernel`, which then reads it there while it walks the tile in blocks of cols x rows (with lds_bytes of dynamic LDS a block).
template <class A>
int run_reduce_kernel(twk_hip_ctx* c, const twk_hip_tile_desc& t, Slot& s, int which, void (*kernel)(const A*), uint32_t cols, uint32_t rows, const A& a, size_t lds_bytes = 0) {
	static_assert(sizeof(A) <= sizeof(ReduceArgs) && alignof(A) <= alignof(ReduceArgs) && std::is_trivially_copyable<A>::value, "a parameter block the slot has room for");
	const dim3 grid((t.nB + cols - 1) / cols, (t.nA + rows - 1) / rows);
	if (grid.y > 0xFFFFu) return TWK_HIP_E_INVALID;
	memcpy(s.h_args + which, &a, sizeof(A));      // (the slot's previous launch has been waited for: its copy is done)
	HIPCHK(c, hipMemcpyAsync(s.d_args + which, s.h_args + which, sizeof(A), hipMemcpyHostToDevice, c->s_compute));
	hipLaunchKernelGGL(kernel, grid, dim3(cols), lds_bytes, c->s_compute, reinterpret_cast<const A*>(s.d_args + which));
	HIPCHK(c, hipGetLastError());
	return TWK_HIP_OK;
}

// The epilogue of a reduce launch whose count matrix is in the slot's C, by the launch's kind: what follows the call's last launch - prune's and clump's
// walks, the matrix's and the band's diagonal and copy - is the entry point's (twk_hip_ld_prune, _clump, _matrix, _matrix_band).
int launch_reduce(twk_hip_ctx* c, int set, const twk_hip_tile_desc& t, Slot& s, int which, bool phased_math, int auto_select, const twk_hip_filters& f, const ColRange* cr) {
	StatsParams p = make_stats(c, set, t, s, phased_math, auto_select, f, cr);
	p.out = nullptr; p.capacity = 0; p.n_out = nullptr; p.keys = nullptr; p.vals = nullptr;
	if (!t.nA || !t.nB) return TWK_HIP_OK;
	HIPCHK(c, s.h_args.reserve(2, 2, nullptr));
	HIPCHK(c, s.d_args.reserve(2, 2, nullptr));
	ReduceState& rs = c->reduce;
	// the launch's share of the accumulators' proven room: decay's blocks (ld_decay.hip.h), the pairs an aggregate launch can evaluate (ld_aggregate.hip.h)
	const bool square_diag = t.diag && t.rowA0 == t.rowB0 && t.nA == t.nB;
	uint64_t limit = ~0ull; const char* over = "";
	switch (s.l.form.reduce) {
	case Reduce::decay:
		rs.work += (uint64_t)((t.nB + DECAY_THREADS - 1) / DECAY_THREADS) * ((t.nA + DECAY_ROWS - 1) / DECAY_ROWS);
		limit = 0xFFFFFFFFull; over = "LD decay: more than 2^32 blocks in one call; split it into shards"; break;
	case Reduce::aggregate:
		rs.work += square_diag ? (uint64_t)t.nA * (t.nA - 1) / 2 : (uint64_t)t.nA * t.nB;
		limit = 1ull << 42; over = "LD aggregate: more than 2^42 pairs in one call; split it into shards"; break;
	default: break;
	}
	if (rs.work > limit) { snprintf(c->err, sizeof(c->err), "%s", over); return TWK_HIP_E_INVALID; }
	switch (s.l.form.reduce) {
	case Reduce::prune:     return run_reduce_kernel(c, t, s, which, k_ld_prune_mask, PRUNE_THREADS, PRUNE_ROWS, PruneArgs{{p, rs.map.bits}});
	case Reduce::clump:     return run_reduce_kernel(c, t, s, which, k_ld_clump_mask, CLUMP_THREADS, CLUMP_ROWS, ClumpArgs{{p, rs.map.bits}});
	case Reduce::matrix:    return run_reduce_kernel(c, t, s, which, k_ld_matrix_fill, MATRIX_THREADS, MATRIX_ROWS, MatrixArgs{{p, rs.map.matrix}});
	case Reduce::decay:     return run_reduce_kernel(c, t, s, which, k_ld_decay, DECAY_THREADS, DECAY_ROWS, DecayArgs{{p, rs.map.decay}}, decay_lds_bytes(rs.map.decay.n_bins));
	case Reduce::aggregate: return run_reduce_kernel(c, t, s, which, k_ld_aggregate, AGG_THREADS, AGG_ROWS, AggArgs{{p, rs.map.agg}});
	case Reduce::annot:     return run_reduce_kernel(c, t, s, which, k_ld_annot, ANNOT_THREADS, ANNOT_ROWS, AnnotArgs{{p, rs.map.annot}});      // (no work limit: ld_score_annot.hip.h)
	case Reduce::bandmat:   return run_reduce_kernel(c, t, s, which, k_ld_bandmat_fill, BANDMAT_THREADS, BANDMAT_ROWS, BandArgs{{p, rs.map.band}});
	case Reduce::topk:      return run_reduce_kernel(c, t, s, which, k_ld_topk, TOPK_THREADS, TOPK_BLOCK_ROWS, TopkArgs{{p, rs.map.topk}}, tk_lds_bytes(rs.map.topk.k));      // (no work limit: a selection has no headroom to use up)
	case Reduce::dprime_ci:
	case Reduce::blocks:    return run_reduce_kernel(c, t, s, which, k_ld_dprime_ci_band, CI_THREADS, CI_ROWS, CiArgs{{p, rs.map.ci}});
	case Reduce::score: break;
	case Reduce::none: return TWK_HIP_E_STATE;
	}
	// score: the pairs' r2 summed per row and per column inside the blocks, the blocks' partials folded into the context's per-variant accumulators - rows,
	// then columns, each in a launch of its own, so that a variant that is both a row and a column of a diagonal launch is added to by one lane at a time
	ScoreParts sp{};
	sp.gx = (t.nB + SCORE_THREADS - 1) / SCORE_THREADS; sp.gy = (t.nA + SCORE_ROWS - 1) / SCORE_ROWS;
	if (sp.gy > 0xFFFFu) return TWK_HIP_E_INVALID;
	const size_t n_row = (size_t)t.nA * sp.gx, n_col = (size_t)sp.gy * t.nB, need = n_row + n_col;
	HIPCHK(c, reserve_together(need, need, &c->graveyard, s.sc_sum, s.sc_n));
	sp.row_sum = s.sc_sum; sp.row_n = s.sc_n; sp.col_sum = s.sc_sum + n_row; sp.col_n = s.sc_n + n_row;
	const uint32_t* ids = c->planes[set].ids;
	const int rc = run_reduce_kernel(c, t, s, which, k_ld_score, SCORE_THREADS, SCORE_ROWS, ScoreArgs{{p, sp}}); if (rc) return rc;
	hipLaunchKernelGGL(k_ld_score_fold, dim3((t.nA + 255) / 256), dim3(256), 0, c->s_compute, (const double*)sp.row_sum, (const uint32_t*)sp.row_n, t.nA, sp.gx,
	                   (size_t)sp.gx, (size_t)1, t.rowA0, ids, c->M, c->d_score_sum, c->d_score_n);
	hipLaunchKernelGGL(k_ld_score_fold, dim3((t.nB + 255) / 256), dim3(256), 0, c->s_compute, (const double*)sp.col_sum, (const uint32_t*)sp.col_n, t.nB, sp.gy,
	                   (size_t)1, (size_t)t.nB, t.rowB0, ids, c->M, c->d_score_sum, c->d_score_n);
	HIPCHK(c, hipGetLastError());
	return TWK_HIP_OK;
}

// Survivors are appended with an atomic counter, in no order.  They leave the device in (idxA, idxB) order
// - the order the writer puts them in the file, which makes a one-GPU run's output deterministic - by a key
// sort of (idxA << bits | idxB, position) and a gather.  Key and position are written by the math kernels where the
// record is appended (d_append_survivor); records the Fisher cut-off drops get the all-ones key from the Fisher kernel
// and sort behind the rest.
__global__ void k_gather_records(const twk_hip_record* __restrict__ recs, const uint32_t* __restrict__ order, unsigned long long n,
                                 twk_hip_record* __restrict__ out) {
	constexpr uint32_t W = sizeof(twk_hip_record) / 8;              // 13 eight-byte words per record
	const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n * W) return;
	const unsigned long long r = i / W; const uint32_t w = (uint32_t)(i % W);
	reinterpret_cast<unsigned long long*>(out)[i] = reinterpret_cast<const unsigned long long*>(recs + order[r])[w];
}

// Every launch of a slot begins here: what the previous one left in the slot's per-launch state cannot reach it.
Launch& begin_launch(Slot& s, int plane_set, double minP) {
	s.l = Launch();
	s.l.plane_set = plane_set; s.l.minP = minP;
	return s.l;
}

// The list math over the launch's candidate list (phased or unphased by its form), with the parameter block at d_stats.
int launch_list_math(twk_hip_ctx* c, Slot& s, const StatsParams* d_stats) {
	hipLaunchKernelGGL(s.l.form.unphased ? k_ld_stats_list_unphased : k_ld_stats_list, dim3(c->resident_blocks * 4), dim3(256), 0, c->s_compute, d_stats,
	                   (const uint32_t*)s.l.cand, (const unsigned long long*)(s.n_out + 2), s.l.cand_cap);
	HIPCHK(c, hipGetLastError());
	return TWK_HIP_OK;
}

// The end of every launch, on the compute stream: Fisher's exact test on the compacted survivors (the slot's count / candidate buffer is
// free by now - the math kernels in front are done with it - and holds the walk-length order; a score, prune, clump, matrix, decay or aggregate launch has no survivors, and no
// test to run: minP >= 1 drops nothing), for a band launch the sort of its survivors (Launch::presorted), the counters' copy to the host
// and ev_s1.
// The band launch's sort is over as many slots as there were candidates (unused slots carry the all-ones key, like records the Fisher
// cut-off drops: they sort behind the survivors): it does not need the survivor count, so it need not wait for the host - on the copy
// stream (finish_tile's sort_records) it waited for a CU until the *next* launch's persistent count kernel was through, 60 ms per launch
// of the 2,504 x 531,500 run.
int close_launch(twk_hip_ctx* c, Slot& s) {
	if (!s.l.form.reduces()) { const int rc = launch_fisher(c, s.out, s.n_out, s.cap_use, s.l.minP, s.C, s.C.capacity(), s.keys); if (rc) return rc; }
	if (s.l.presorted) {
		const unsigned long long need = s.cap_use;
		size_t bytes = c->d_band_tmp.capacity();
		HIPCHK(c, rocprim::radix_sort_pairs(c->d_band_tmp.get(), bytes, s.keys.get(), c->d_band_keys.get(), s.vals.get(), c->d_band_vals.get(), (size_t)need, 0u, 64u, c->s_compute));
		const unsigned long long words = need * (sizeof(twk_hip_record) / 8);
		hipLaunchKernelGGL(k_gather_records, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, c->s_compute, (const twk_hip_record*)s.out, (const uint32_t*)c->d_band_vals, need, s.sorted);
		HIPCHK(c, hipGetLastError());
	}
	HIPCHK(c, hipMemcpyAsync(s.h_n_out, s.n_out, N_SLOT_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->s_compute));
	HIPCHK(c, hipEventRecord(s.ev_s1, c->s_compute));
	return TWK_HIP_OK;
}

// Enqueue everything for one tile into slot s (count [+ second pass], math, counter copy), in the form its owner's grant allows (launch_form).
// list_words != 0: a band launch (region_impl) - the fused form with a candidate list of that many words and no count
// matrix at all (its rectangle may be far beyond what a matrix could hold); it is an error if the launch does not fuse.
int enqueue_tile(twk_hip_ctx* c, int mode, const twk_hip_tile_desc& t, const twk_hip_filters& f, const FormGrant& grant, Slot& s,
                 unsigned long long capacity, const ColRange* cr = nullptr, size_t list_words = 0) {
	const TilePlan pl = plan_for(c, mode);
	const int kind1 = pl.set1, kind2 = pl.set2;
	int rc = ensure_planes(c, kind1); if (rc) return rc;
	if (kind2 >= 0) { rc = ensure_planes(c, kind2); if (rc) return rc; }
	const LaunchForm form = launch_form(c, pl, f, grant);
	const Geometry g = tile_geometry(pl.Pmax, t);
	if (form.reduces()) capacity = 1;              // a score, prune, clump, matrix, decay or aggregate launch keeps no survivors (and is never a band launch: always the matrix form)
	if (list_words && !(form.fused && !form.two_pass)) return TWK_HIP_E_STATE;
	const auto tl0 = std::chrono::steady_clock::now();
	auto tl = [&](const char* what) { if (c->opt.timeline) fprintf(stderr, "[timeline]     enqueue_tile: %s at +%.3f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tl0).count()); };
	// (two products: the (HH, HQ) matrix has a row per row variant, whole tiles of 128 of them, and the candidate list lies behind it)
	// (one product: the CC matrix has a row per row variant and a column per column variant, whole tiles of 128 of either)
	const uint32_t ldc_one = round_up(t.nB, TILE);
	const size_t c_two_words = form.one ? (size_t)round_up(t.nA, TILE) * ldc_one : form.two ? (size_t)round_up(t.nA, TILE) * g.rowsB : 0;
	const size_t two_list_words = form.two ? 6 * (size_t)cand_list_entries((unsigned long long)t.nA * t.nB) : 0;
	rc = ensure_slot(c, s, list_words ? list_words : std::max((size_t)g.rowsA * g.rowsB, c_two_words + two_list_words), capacity); if (rc) return rc;
	tl("slot buffers");
	Launch& l = begin_launch(s, kind1, f.minP);
	l.form = form; l.given = grant;
	HIPCHK(c, hipMemsetAsync(s.n_out, 0, N_SLOT_COUNTERS * sizeof(unsigned long long), c->s_compute));
	l.cand = s.C; l.cand_cap = (list_words ? list_words : s.C.capacity()) / (form.unphased ? 6 : 3);
	// The three-product form where the launch does not fuse (long rows: tiles are split along K): the (HH, S) matrix takes the first half of the
	// slot's count buffer and the candidate list the room behind it, as far as the form pays (ld_form.h: cand_list_entries).
	if (form.three_plain() || form.two) {
		const size_t c2_words = form.two ? c_two_words : (size_t)(g.rowsA / 2) * g.rowsB;
		const unsigned long long room = s.C.capacity() > c2_words ? (s.C.capacity() - c2_words) / 6 : 0;
		const unsigned long long pairs = (unsigned long long)t.nA * t.nB;
		l.cand = s.C + c2_words;
		l.cand_cap = std::min<unsigned long long>(room, form.keep_three ? room : cand_list_entries(pairs));
		if (c->opt.cand_cap > 0 && !form.sample) l.cand_cap = std::min<unsigned long long>(l.cand_cap, (unsigned long long)c->opt.cand_cap);      // (test hook: the launches, not their samples)
	}
	FusedArgs fa{};
	const bool with_args = form.fused || form.three || form.two;      // the launch carries the screen's and the list math's parameter blocks
	if (with_args) {
		PlaneSet& ps = c->planes[kind1];
		fa.unphased = form.unphased ? 1 : 0;
		ScreenWork& sw = fa.screen;
		sw.cut = f.minR2 * (1.0 - 1e-6); sw.two_n = 2.0 * (double)c->N;
		if (form.fused && (!ps.terms || ps.terms_cut != sw.cut)) {      // the prefilter's per-variant terms: once per plane set and cut-off, on the stream the kernels follow
			const uint32_t P1 = (uint32_t)planes_per_variant(set_kind(kind1)), n_pos = ps.rows_alloc / P1;
			HIPCHK(c, ps.terms.reserve(n_pos, n_pos, nullptr));
			hipLaunchKernelGGL(k_screen_terms, dim3((n_pos + 255) / 256), dim3(256), 0, c->s_compute, (const uint32_t*)ps.rowpop, n_pos, (int)P1, sw.two_n, sw.cut, ps.terms);
			HIPCHK(c, hipGetLastError());
			ps.terms_cut = sw.cut;
		}
		sw.terms = ps.terms; sw.slack = 0.5f + (float)sw.two_n * (1.0f / 1048576.0f);
		fa.stats = make_stats(c, kind1, t, s, pl.phased1, pl.select1, f, cr);
		sw.rowpop = ps.rowpop; sw.a0 = t.rowA0; sw.b0 = t.rowB0; sw.nA = t.nA; sw.nB = t.nB;
		sw.n_variants = c->M; sw.diag = (t.diag && t.rowA0 == t.rowB0) ? 1 : 0;
		sw.col_hi = cr ? cr->d_hi : nullptr; sw.hi_a0 = cr ? cr->a0 : 0; sw.hi_b0 = cr ? cr->b0 : 0; sw.hi_n = cr ? cr->n_hi : 0; sw.col_lo = cr ? cr->d_lo : nullptr;
		sw.list_zone = cr ? cr->list_zone : 0; sw.probe_zone = cr ? cr->probe_zone : 0;
		sw.cand = l.cand; sw.cap = l.cand_cap; sw.n_cand = s.n_out + 2; sw.carrier = form.one ? 2u : form.carrier ? 1u : 0u;
		sw.fine = form.carrier && !form.one && walk_fine_applies(c, ps.W / KC) ? 1u : 0u;
		sw.uz = form.uz ? 1u : 0u;
		{	// slots a wave reserves at a time: what it cannot use is lost to the list, so at most an eighth of the list's
			// capacity may be tied up in the waves' windows (small tiles: 0, i.e. one atomic per wave and tile)
			const unsigned long long per_wave = l.cand_cap / (8ull * c->resident_blocks * (COUNT_THREADS / 64));
			sw.chunk = c->opt.cand_chunk >= 0 ? (uint32_t)c->opt.cand_chunk      // measurement hook
			                                  : (per_wave >= 64 ? (uint32_t)std::min<unsigned long long>(per_wave, 128) : 0u);
		}
	}
	rc = launch_count(c, kind1, t, s, 0, cr, form, with_args ? &fa : nullptr); if (rc) return rc;
	tl("count kernel enqueued");
	if (list_words) {
		// A band launch stops here for now: how many survivors it can have is how many candidates it found, and only the count
		// kernel knows.  The counters travel to the host behind it; enqueue_band_math sizes the survivor buffer by them and
		// enqueues the rest (sizing it by a guess - 1/32 of the launch's pairs - meant gigabytes of allocation per slot, a
		// tenth of a second each, for launches that then kept a few thousand records).
		l.deferred = true; l.was_deferred = true; l.stats_host = fa.stats;
		HIPCHK(c, hipMemcpyAsync(s.h_n_out, s.n_out, N_SLOT_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->s_compute));
		HIPCHK(c, hipEventRecord(s.ev_c1b, c->s_compute));
		return TWK_HIP_OK;
	}
	if (with_args) {
		if (l.d_stats_dev) {      // (else: no tiles, no launch, no candidates)
			if (form.one) {                // CC matrix -> screen with S >= 0 and S + HH bounded from CC and the margins -> candidates -> their four products -> the list math
				hipLaunchKernelGGL(k_screen1_pairs, dim3((t.nB + SCREEN3_THREADS - 1) / SCREEN3_THREADS, t.nA), dim3(SCREEN3_THREADS), 0, c->s_compute, l.d_screen_dev,
				                   (const StatsParams*)l.d_stats_dev, (const uint32_t*)s.C, ldc_one);
				HIPCHK(c, hipGetLastError());
			} else if (form.two) {         // (HH, HQ) matrix -> screen with S bounded from the margins -> candidates -> their four products -> the list math
				hipLaunchKernelGGL(k_screen2_pairs, dim3((t.nB + SCREEN3_THREADS - 1) / SCREEN3_THREADS, t.nA), dim3(SCREEN3_THREADS), 0, c->s_compute, l.d_screen_dev,
				                   (const StatsParams*)l.d_stats_dev, (const uint32_t*)s.C, g.ldc);
				HIPCHK(c, hipGetLastError());
			}
			if (form.three_plain()) {      // (HH, S) matrix -> screen -> candidates -> their four products -> the list math
				hipLaunchKernelGGL(k_screen3_pairs, dim3((t.nB + SCREEN3_THREADS - 1) / SCREEN3_THREADS, t.nA), dim3(SCREEN3_THREADS), 0, c->s_compute, l.d_screen_dev,
				                   (const StatsParams*)l.d_stats_dev, (const uint32_t*)s.C, g.ldc);
				HIPCHK(c, hipGetLastError());
			}
			if (form.three || form.two) { rc = launch_recount(c, kind1, s); if (rc) return rc; }
			rc = launch_list_math(c, s, l.d_stats_dev); if (rc) return rc;
		}
	} else if (form.reduces()) {
		rc = launch_reduce(c, kind1, t, s, 0, pl.phased1, pl.select1, f, cr); if (rc) return rc;
	} else {
		const StatsParams p = make_stats(c, kind1, t, s, pl.phased1, pl.select1, f, cr);
		hipLaunchKernelGGL(k_ld_stats, dim3((t.nB + 255) / 256, t.nA), dim3(256), 0, c->s_compute, p);
	}
	HIPCHK(c, hipGetLastError());
	if (form.two_pass) {
		rc = launch_count(c, kind2, t, s, 1, cr, LaunchForm(), nullptr); if (rc) return rc;
		if (form.reduces()) { rc = launch_reduce(c, kind2, t, s, 1, false, 2, f, nullptr); if (rc) return rc; }
		else {
			const StatsParams p = make_stats(c, kind2, t, s, false, 2, f);
			hipLaunchKernelGGL(k_ld_stats, dim3((t.nB + 255) / 256, t.nA), dim3(256), 0, c->s_compute, p);
		}
		HIPCHK(c, hipGetLastError());
	}
	return close_launch(c, s);
}

// The second half of a band launch (see enqueue_tile): wait for its count kernel, size the survivor buffers by the candidates it
// found (no pair that was not a candidate can survive), enqueue the list math and the launch's end (close_launch: Fisher's test, the
// sort of the survivors, the counters' copy) - all on the compute stream.
int enqueue_band_math(twk_hip_ctx* c, Slot& s) {
	Launch& l = s.l;
	if (!l.deferred) return TWK_HIP_E_STATE;
	l.deferred = false;
	HIPCHK(c, hipEventSynchronize(s.ev_c1b));
	const unsigned long long cand = s.h_n_out[2];
	// Every candidate may survive: the survivor, key and sort buffers are sized by the candidates (220 bytes each).  Beyond 2^26 of them -
	// 15 GB per slot - or when the device cannot give the memory, the launch is treated like one whose list overflowed: its rows are redone
	// as matrix-sized tiles, which split further on their own overflow (the round-4 code returned E_NOMEM and took the run down).
	constexpr unsigned long long BAND_MAX_SURVIVORS = 1ull << 26;
	bool overflow = cand > l.cand_cap;                       // finish_tile reports it; nothing to compute here
	if (!overflow && cand > BAND_MAX_SURVIVORS) { l.band_too_big = true; overflow = true; }
	unsigned long long need = overflow ? 1 : std::max<unsigned long long>(cand, 1);
	if (c->opt.record_cap > 0) need = std::min<unsigned long long>(need, (unsigned long long)c->opt.record_cap);      // (test hook: forces the overflow path)
	auto grow_all = [&]() -> int {
		const size_t roomy = (size_t)(need + need / 4);      // (with some room: the next launch of the region will be about as rich)
		HIPCHK(c, reserve_together(need, roomy, &c->graveyard, s.out, s.keys, s.vals));
		HIPCHK(c, s.sorted.reserve(need, roomy, &c->graveyard));
		HIPCHK(c, reserve_together(need, roomy, &c->graveyard, c->d_band_keys, c->d_band_vals));
		size_t tmp = 0;
		HIPCHK(c, rocprim::radix_sort_pairs(nullptr, tmp, s.keys.get(), c->d_band_keys.get(), s.vals.get(), c->d_band_vals.get(), (size_t)need, 0u, 64u, c->s_compute));
		tmp = std::max<size_t>(tmp, 4096);                   // (never empty: a null scratch pointer would turn the sort into another size query)
		HIPCHK(c, c->d_band_tmp.reserve(tmp, tmp + tmp / 4, &c->graveyard));
		return TWK_HIP_OK;
	};
	{
		int rc = grow_all();
		if (rc == TWK_HIP_E_NOMEM && !overflow) {            // no room for this many survivors: the fallback's tiles need far less at a time
			(void)hipGetLastError();
			l.band_too_big = true; overflow = true; need = 1;
			rc = grow_all();
		}
		if (rc) return rc;
	}
	s.cap_use = need;
	HIPCHK(c, hipEventRecord(s.ev_c0b, c->s_compute));
	if (!overflow) {
		HIPCHK(c, hipMemsetAsync(s.keys, 0xFF, (size_t)need * sizeof(unsigned long long), c->s_compute));
		HIPCHK(c, hipMemsetAsync(s.vals, 0, (size_t)need * sizeof(uint32_t), c->s_compute));
	}
	if (l.d_stats_dev && !overflow) {
		l.stats_host.out = s.out; l.stats_host.capacity = s.cap_use; l.stats_host.n_out = s.n_out;
		l.stats_host.keys = s.keys; l.stats_host.vals = s.vals;
		HIPCHK(c, hipMemcpyAsync(l.d_stats_dev, &l.stats_host, sizeof(StatsParams), hipMemcpyHostToDevice, c->s_compute));
		if (l.form.three) { const int rc = launch_recount(c, l.plane_set, s); if (rc) return rc; }
		{ const int rc = launch_list_math(c, s, l.d_stats_dev); if (rc) return rc; }
	}
	l.presorted = !overflow;
	return close_launch(c, s);
}

static_assert(sizeof(twk_hip_record) % 8 == 0, "record gather copies 8-byte words");

// recs[0..n) on the device, with their keys and positions -> c->d_sorted in (idxA, idxB) order, on stream st.
int sort_records(twk_hip_ctx* c, const twk_hip_record* recs, unsigned long long* keys_in, uint32_t* vals_in, unsigned long long n, bool any_dropped, hipStream_t st) {
	if (n > 0xFFFFFFFFull) return TWK_HIP_E_INVALID;
	HIPCHK(c, reserve_together(n, std::max<unsigned long long>(n + n / 4, 1ull << 16), &c->graveyard, c->d_sort_keys, c->d_sort_vals, c->d_sorted));
	unsigned long long* keys_out = c->d_sort_keys;
	uint32_t* vals_out = c->d_sort_vals;
	const uint32_t bits_b = key_shift_for(c->M);
	// dropped records (Fisher cut-off) carry the all-ones key: sort every bit when there can be any, else only the
	// 2 * bits_b bits a (idxA, idxB) key uses
	const unsigned end_bit = any_dropped ? 64u : 2u * bits_b;
	size_t tmp = 0;
	HIPCHK(c, rocprim::radix_sort_pairs(nullptr, tmp, keys_in, keys_out, vals_in, vals_out, (size_t)n, 0u, end_bit, st));
	HIPCHK(c, c->d_sort_tmp.reserve(std::max<size_t>(tmp, 1), std::max<size_t>(tmp + tmp / 4, 4096), &c->graveyard));      // (never empty: a null scratch pointer would turn the sort into another size query)
	tmp = c->d_sort_tmp.capacity();
	HIPCHK(c, rocprim::radix_sort_pairs(c->d_sort_tmp.get(), tmp, keys_in, keys_out, vals_in, vals_out, (size_t)n, 0u, end_bit, st));
	const unsigned long long words = n * (sizeof(twk_hip_record) / 8);
	hipLaunchKernelGGL(k_gather_records, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, recs, vals_out, n, c->d_sorted);
	HIPCHK(c, hipGetLastError());
	return TWK_HIP_OK;
}

// Room for n more records behind the ones the device sink holds (grow-only, contents kept).
int ensure_device_keep(twk_hip_ctx* c, unsigned long long n_more) {
	const unsigned long long need = c->d_keep_n + n_more;
	if (need <= c->d_keep.capacity()) return TWK_HIP_OK;
	DevBuf<twk_hip_record> p;
	HIPCHK(c, p.reserve(need, std::max<unsigned long long>(need + need / 2, 1ull << 16), &c->graveyard));      // (the graveyard: for its reclaim - p has nothing to park)
	if (c->d_keep_n) {
		HIPCHK(c, hipMemcpyAsync(p, c->d_keep, (size_t)c->d_keep_n * sizeof(twk_hip_record), hipMemcpyDeviceToDevice, c->s_copy));
		HIPCHK(c, hipStreamSynchronize(c->s_copy));
	}
	c->d_keep = std::move(p);
	return TWK_HIP_OK;
}

// The outlier watch: every count launch goes into a ring with its time per unit of work, and is compared with the median of the launches
// of its own kind and row length before it.  (Round 4 saw the same run take 1.7 x as long now and then, cause unknown; the watch names
// the launch, the clock its blocks ran at and how far apart the XCDs finished.)
constexpr size_t LAUNCH_RING = 4096;
void watch_launch(twk_hip_ctx* c, const Slot& s, float ms, const twk_hip_tile_desc& t) {
	twk_hip_launch_stat st{};
	st.ms = ms; st.row_pairs = s.l.row_pairs; st.candidates = (s.l.form.fused || s.l.form.three || s.l.form.two) ? s.h_n_out[2] : 0;
	st.shader_mhz = s.h_n_out[5] ? (double)s.h_n_out[4] / (double)s.h_n_out[5] * 100.0 : 0.0;
	st.words_per_row = c->planes[s.l.plane_set].W_live;
	st.prefix_chunks = s.l.prefix_chunks; st.prefix_chunks_full = s.l.prefix_chunks_full; st.carrier = s.l.form.carrier ? 1u : 0u; st.one = s.l.form.one ? 1u : 0u; st.uz = s.l.form.uz ? 1u : 0u;
	st.kind = s.l.form.fused ? (s.l.form.three ? 4u : (c->planes[s.l.plane_set].rows && set_kind(s.l.plane_set) == PK_UNPHASED ? 3u : 2u)) : (s.l.form.two ? 5u : s.l.form.three_plain() ? 1u : 0u);
	unsigned long long lo = ~0ull, hi = 0;
	for (int x = 0; x < 8; ++x) if (s.h_n_out[8 + x]) { lo = std::min(lo, s.h_n_out[8 + x]); hi = std::max(hi, s.h_n_out[8 + x]); }
	st.xcd_finish_spread_us = hi ? (double)(hi - lo) / 100.0 : 0.0;
	auto cost = [](const twk_hip_launch_stat& x) { return x.row_pairs ? x.ms / ((double)x.row_pairs * (double)x.words_per_row * (x.uz ? 0.5 : (x.kind == 1 || x.kind == 4) ? 0.75 : 1.0)) : 0.0; };
	if (st.ms >= 0.3 && st.row_pairs) {
		std::vector<double> peers;
		for (const auto& x : c->launch_ring)
			if (x.kind == st.kind && x.uz == st.uz && x.words_per_row == st.words_per_row && x.ms >= 0.3 && !x.outlier) peers.push_back(cost(x));
		if (peers.size() >= 8) {
			std::nth_element(peers.begin(), peers.begin() + peers.size() / 2, peers.end());
			const double med = peers[peers.size() / 2];
			if (cost(st) > 1.4 * med) {
				st.outlier = 1; c->timing.outlier_launches += 1;
				if (c->opt.timeline) fprintf(stderr, "[outlier] count launch #%llu (kind %u, rows %u+%u x cols %u+%u, %llu row pairs of %u words): %.3f ms = %.2f x the median cost of its %zu peers; "
				                             "blocks ran at %.0f MHz; XCDs finished %.1f us apart; %llu candidates\n", (unsigned long long)c->launches_seen, st.kind, t.rowA0, t.nA, t.rowB0, t.nB,
				                             (unsigned long long)st.row_pairs, st.words_per_row, st.ms, cost(st) / med, peers.size(), st.shader_mhz, st.xcd_finish_spread_us, (unsigned long long)st.candidates);
			}
		}
	}
	if (c->launch_ring.size() < LAUNCH_RING) c->launch_ring.push_back(st);
	else c->launch_ring[c->launches_seen % LAUNCH_RING] = st;
	c->launches_seen += 1;
}

// kept sorted records on the device -> the host, through the pinned staging buffer, handed to `sink` in pieces of HOST_CHUNK records, each
// piece while the next is being copied (a launch may hold tens of millions of survivors: page-locking a buffer for all of them would cost
// more than the copy).  Called by the thread that finishes the launch, or by the delivery thread.
constexpr unsigned long long HOST_CHUNK = 1ull << 20;       // records per piece (109 MB)
int deliver_records(twk_hip_ctx* c, const twk_hip_record* sorted, unsigned long long kept, twk_hip_record_sink sink, void* user, hipStream_t st, double tl_wait,
                    char* err = nullptr, size_t err_len = 0) {
	if (!err) { err = c->err; err_len = sizeof(c->err); }
	auto since = [](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); };
	double tl_copy = 0, tl_sink = 0;
	int rc;
	if (kept <= HOST_CHUNK) {
		rc = ensure_host_records(c, kept, err, err_len); if (rc) return rc;
		if (kept) HIPCHK_E(err, err_len, hipMemcpyAsync(c->h_recs, sorted, (size_t)kept * sizeof(twk_hip_record), hipMemcpyDeviceToHost, st));
		HIPCHK_E(err, err_len, hipStreamSynchronize(st));
		if (kept && sink(user, c->h_recs, kept)) { snprintf(err, err_len, "the record sink failed"); return TWK_HIP_E_INVALID; }
		return TWK_HIP_OK;
	}
	rc = ensure_host_records(c, 2 * HOST_CHUNK, err, err_len); if (rc) return rc;
	auto copy_piece = [&](unsigned long long first) -> hipError_t {
		const unsigned long long m = std::min(HOST_CHUNK, kept - first);
		return hipMemcpyAsync(c->h_recs + ((first / HOST_CHUNK) & 1) * HOST_CHUNK, sorted + first, (size_t)m * sizeof(twk_hip_record), hipMemcpyDeviceToHost, st);
	};
	HIPCHK_E(err, err_len, copy_piece(0));
	for (unsigned long long first = 0; first < kept; first += HOST_CHUNK) {
		auto t1 = std::chrono::steady_clock::now();
		HIPCHK_E(err, err_len, hipStreamSynchronize(st));                                          // piece `first` has arrived
		if (first + HOST_CHUNK < kept) HIPCHK_E(err, err_len, copy_piece(first + HOST_CHUNK));     // the next one travels while the sink works (into the other half)
		tl_copy += since(t1); t1 = std::chrono::steady_clock::now();
		if (sink(user, c->h_recs + ((first / HOST_CHUNK) & 1) * HOST_CHUNK, std::min(HOST_CHUNK, kept - first))) {
			(void)hipStreamSynchronize(st);
			snprintf(err, err_len, "the record sink failed");
			return TWK_HIP_E_INVALID;
		}
		tl_sink += since(t1);
	}
	if (c->opt.timeline) fprintf(stderr, "[timeline]   inside: waited %.3f ms for the launch, %.3f ms for copies, %.3f ms in the sink (%llu records)\n", tl_wait, tl_copy, tl_sink, kept);
	return TWK_HIP_OK;
}

// ---- the delivery thread (option async_delivery; the queue itself: twk_delivery.h) -----------------------------------------------
// During a region call with a sink a finished launch's sorted survivors are copied aside on the device (a millisecond a gigabyte) into
// one of at most `deliver_buffers` staging buffers and queued; a second thread takes the queue to the host, in order, through
// deliver_records.  The sink is then called from that thread - one call at a time, in the order of the launches, as before.
int discard_records(void*, const twk_hip_record*, uint64_t);
void delivery_begin(twk_hip_ctx* c, twk_hip_record_sink sink) {
	if (c->dl.active() || !sink || c->device_sink || !c->opt.async_delivery) return;
	c->dl_ops.c = c; c->dl_ops.n_alloc = 0; c->dl_ops.n_copy = 0;
	(void)c->dl.begin(&c->dl_ops, (size_t)c->opt.deliver_buffers);      // (no thread to be had: the caller's thread delivers, as with the option off)
}
// -> the delivery thread's result once everything queued has reached the sink; its error text into c->err
int delivery_end(twk_hip_ctx* c) {
	if (!c->dl.active()) return TWK_HIP_OK;
	const int rc = c->dl.end();
	if (rc && c->dl.error()[0]) snprintf(c->err, sizeof(c->err), "%s", c->dl.error());
	return rc;
}
// everything queued so far has reached its sink (the caller may then hand records over itself, in order: finish_tile does for launches with
// few survivors, which are not worth a staging copy and a thread hand-off)
int delivery_drain(twk_hip_ctx* c) { return c->dl.drain(); }
int stage_for_delivery(twk_hip_ctx* c, const twk_hip_record* sorted, unsigned long long kept, twk_hip_record_sink sink, void* user) {
	if (!kept || sink == discard_records) return TWK_HIP_OK;
	const int rc = c->dl.stage(sorted, kept, sink, user);
	if (rc == Delivery::STAGE_DELIVER_YOURSELF) {
		// no room for a copy on the device: this thread hands the records over itself, behind what is queued (as with the option off)
		(void)hipGetLastError();
		const int drc = delivery_drain(c); if (drc) return drc;
		return deliver_records(c, sorted, kept, sink, user, c->s_copy, 0.0);
	}
	return rc;
}
// The calling thread is out of device memory (the graveyard's reclaim: twk_buffers.h): everything queued goes to the sink, the idle staging
// buffers and what the call has outgrown so far are freed -> true when anything was given back (the allocation is then tried once more).
bool reclaim_device_memory(twk_hip_ctx* c) {
	(void)hipGetLastError();
	size_t bytes = c->dl.active() ? c->dl.reclaim() : 0;
	if (!c->graveyard.empty()) {
		(void)hipDeviceSynchronize();            // (outgrown buffers may still be read by launches in flight)
		c->graveyard.flush();
		++bytes;
	}
	return bytes != 0;
}

// Wait for slot s, account timing, put its records in (idxA, idxB) order and hand them on: appended to the device sink
// (!to_host), or through the pinned staging buffer to the host - left there whole (sink == null: c->h_recs, for the
// single-tile entry point), or handed to `sink` in pieces of HOST_CHUNK records, each piece while the next is being copied
// (a launch may hold tens of millions of survivors: page-locking a buffer for all of them would cost more than the copy).
int finish_tile(twk_hip_ctx* c, Slot& s, const twk_hip_tile_desc& t, unsigned long long* n_out, const Deliver& to) {
	const auto tl0 = std::chrono::steady_clock::now();
	auto since = [](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); };
	HIPCHK(c, hipEventSynchronize(s.ev_s1));
	const double tl_wait = since(tl0);
	struct FinishClock {          // timing.finish_ms: from here to whichever return hands the records on
		twk_hip_ctx* c; std::chrono::steady_clock::time_point t0;
		~FinishClock() { c->timing.finish_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
	} finish_clock{c, std::chrono::steady_clock::now()};
	float ms = 0;
	HIPCHK(c, hipEventElapsedTime(&ms, s.ev_c0, s.ev_c1));
	if (!s.l.is_list) watch_launch(c, s, ms, t);
	if (s.l.is_list && s.l.is_probe) { c->timing.probe_ms += ms; c->timing.probe_launches += 1; c->timing.probe_pairs += s.l.row_pairs; c->timing.candidates += s.h_n_out[2]; }
	else if (s.l.is_list) { c->timing.list_ms += ms; c->timing.list_launches += 1; c->timing.list_pairs += s.l.row_pairs; c->timing.candidates += s.h_n_out[2]; }
	else { c->timing.count_ms += ms; c->timing.count_launches += 1; c->timing.row_pairs += s.l.row_pairs;
	       c->timing.count_shader_cycles += s.h_n_out[4]; c->timing.count_wall_ticks += s.h_n_out[5]; }
	if (s.l.form.fused) { c->timing.fused_launches += 1; c->timing.candidates += s.h_n_out[2]; }
	if (s.l.form.three) {
		c->timing.three_launches += 1; c->timing.three_row_pairs += s.l.row_pairs;
		c->timing.recount_candidates += std::min<unsigned long long>(s.h_n_out[2], s.l.cand_cap);
		if (s.l.form.uz) {
			c->timing.uz_launches += 1;
			c->timing.uz_row_pairs += s.l.row_pairs;
			c->timing.uz_split_units += s.l.extra_units;
		}
		if (s.l.form.three_plain()) c->timing.candidates += s.h_n_out[2];
		if (s.h_n_out[3]) {      // the recount disagrees with the contraction: never to be papered over
			snprintf(c->err, sizeof(c->err), "three-product contraction: %llu candidates whose (HH, S) differ from their recounted products (tile rows %u+%u, cols %u+%u)", s.h_n_out[3], t.rowA0, t.nA, t.rowB0, t.nB);
			return TWK_HIP_E_DEVICE;
		}
		// (ld_form.h on the number; the launch's owner folds it into the call: CallForms::gave_up)
		if (!s.l.form.keep_three && three_too_rich(s.h_n_out[2], s.l.row_pairs)) s.l.too_rich = true;
	}
	if (s.l.form.two) {
		c->timing.two_launches += 1; c->timing.carrier_launches += s.l.form.carrier ? 1 : 0; c->timing.one_launches += s.l.form.one ? 1 : 0; c->timing.recount_candidates += std::min<unsigned long long>(s.h_n_out[2], s.l.cand_cap); c->timing.candidates += s.h_n_out[2];
		if (s.h_n_out[3]) {      // as above: the recount is the contraction's proof
			snprintf(c->err, sizeof(c->err), "two-product contraction: %llu candidates whose %s differ from their recounted products (tile rows %u+%u, cols %u+%u)", s.h_n_out[3], s.l.form.one ? "CC" : s.l.form.carrier ? "(CH, CQ)" : "(HH, HQ)", t.rowA0, t.nA, t.rowB0, t.nB);
			return TWK_HIP_E_DEVICE;
		}
		if (s.l.form.one && c->opt.one != 2 && one_too_rich(s.h_n_out[2], pairs_in_tile(c, t))) s.l.too_rich = true;      // (ld_form.h; its list held, so its records stand)
	}
	float ms_all = 0;
	if (s.l.form.two_pass) {
		HIPCHK(c, hipEventElapsedTime(&ms, s.ev_c0b, s.ev_c1b));
		c->timing.count_ms += ms; c->timing.count_launches += 1; c->timing.row_pairs += s.l.row_pairs_b;
		float m1 = 0, m2 = 0;
		HIPCHK(c, hipEventElapsedTime(&m1, s.ev_c1, s.ev_c0b));
		HIPCHK(c, hipEventElapsedTime(&m2, s.ev_c1b, s.ev_s1));
		ms_all = m1 + m2; c->timing.stats_launches += 2;
	} else {
		HIPCHK(c, hipEventElapsedTime(&ms_all, s.l.was_deferred ? s.ev_c0b : s.ev_c1, s.ev_s1));
		c->timing.stats_launches += 1;
	}
	c->timing.stats_ms += ms_all;
	if (!s.l.is_list) c->timing.variant_pairs += pairs_in_tile(c, t);      // (the dense tiles that cover the list zone count its pairs)
	const unsigned long long n = *s.h_n_out;
	*n_out = n;
	if (s.l.was_deferred && s.l.band_too_big) {          // (enqueue_band_math: more candidates than a band launch may keep survivors for)
		snprintf(c->err, sizeof(c->err), "%llu candidates: beyond the survivor buffers of a band launch (tile rows %u+%u, cols %u+%u)", s.h_n_out[2], t.rowA0, t.nA, t.rowB0, t.nB);
		return TWK_HIP_E_OVERFLOW;
	}
	if ((s.l.form.fused || s.l.is_list || s.l.form.three_plain() || s.l.form.two) && s.h_n_out[2] > s.l.cand_cap) {       // more candidates than the list holds
		s.l.cand_overflow = true;
		snprintf(c->err, sizeof(c->err), "%llu candidates for a list of %llu (tile rows %u+%u, cols %u+%u)", s.h_n_out[2], s.l.cand_cap, t.rowA0, t.nA, t.rowB0, t.nB);
		return TWK_HIP_E_OVERFLOW;
	}
	// (behind the overflow check: a prefix launch whose list flooded is redone over whole rows and has taken no stop that counted; the launch log keeps its entry)
	if (s.l.form.prefix) { c->timing.prefix_launches += 1; c->timing.prefix_chunks += s.l.prefix_chunks; c->timing.prefix_chunks_full += s.l.prefix_chunks_full; }
	if (n > s.cap_use) {
		snprintf(c->err, sizeof(c->err), "%llu survivors for a buffer of %llu (tile rows %u+%u, cols %u+%u%s)", n, s.cap_use, t.rowA0, t.nA, t.rowB0, t.nB, s.l.is_list ? ", list pass" : "");
		return TWK_HIP_E_OVERFLOW;
	}
	if (!n) return TWK_HIP_OK;
	// records that failed the Fisher cut-off were only marked on the device (and counted): they sort behind the rest
	const unsigned long long dropped = std::min(s.h_n_out[1], n), kept = n - dropped;
	int rc = TWK_HIP_OK;
	if (!s.l.presorted) { rc = sort_records(c, s.out, s.keys, s.vals, n, dropped != 0, c->s_copy); if (rc) return rc; }
	const twk_hip_record* sorted = s.l.presorted ? s.sorted : c->d_sorted;      // (a band launch sorted its own behind Fisher's test: enqueue_band_math)
	*n_out = kept;
	if (to.to_host && to.sink && c->dl.active()) {
		// many survivors: the delivery thread takes them to the host (deliver_records) while this thread goes on with the launches; few
		// (a hand-over of a millisecond or two): this thread does, behind whatever is queued
		if (kept >= HOST_CHUNK / 4 || to.sink == discard_records) return stage_for_delivery(c, sorted, kept, to.sink, to.user);
		rc = delivery_drain(c); if (rc) return rc;
	}
	if (!to.to_host) {
		rc = ensure_device_keep(c, kept); if (rc) return rc;
		if (kept) HIPCHK(c, hipMemcpyAsync(c->d_keep + c->d_keep_n, sorted, (size_t)kept * sizeof(twk_hip_record), hipMemcpyDeviceToDevice, c->s_copy));
		c->d_keep_n += kept;
		HIPCHK(c, hipStreamSynchronize(c->s_copy));
		return TWK_HIP_OK;
	}
	if (!to.sink) {
		rc = ensure_host_records(c, kept); if (rc) return rc;
		if (kept) HIPCHK(c, hipMemcpyAsync(c->h_recs, sorted, (size_t)kept * sizeof(twk_hip_record), hipMemcpyDeviceToHost, c->s_copy));
		HIPCHK(c, hipStreamSynchronize(c->s_copy));
		return TWK_HIP_OK;
	}
	return deliver_records(c, sorted, kept, to.sink, to.user, c->s_copy, tl_wait);
}

// What a list block and a probe block begin with, on the spare slot: room for a candidate per pair of the block's rectangle t, a fresh
// launch, the math kernel's parameter block on the device and the ListWork fields the two have in common.
int begin_list_launch(twk_hip_ctx* c, const twk_hip_filters& f, bool unphased, bool probe, const twk_hip_tile_desc& t, uint32_t zone, const ColRange& cr,
                      unsigned long long capacity, ListWork& w) {
	const int set = unphased ? PS_SORTED_U : PS_SORTED_P;
	const PlaneSet& ps = c->planes[set];
	Slot& s = c->slot[SYNC_SLOT];
	const unsigned cand_words = unphased ? 6 : 3;              // (A, B, ALTALT) or (A, B, HH, HQ, QH, QQ)
	int rc = ensure_slot(c, s, (size_t)std::max<uint64_t>(cand_words * (uint64_t)t.nA * t.nB, 1024), capacity); if (rc) return rc;
	HIPCHK(c, c->d_list_stats.reserve(1, 1, nullptr));
	Launch& l = begin_launch(s, set, f.minP);
	l.is_list = true; l.is_probe = probe; l.form.unphased = unphased; l.cand = s.C; l.cand_cap = s.C.capacity() / cand_words;
	const StatsParams sp = make_stats(c, set, t, s, !unphased, 0, f, &cr);
	HIPCHK(c, hipMemsetAsync(s.n_out, 0, N_SLOT_COUNTERS * sizeof(unsigned long long), c->s_compute));
	HIPCHK(c, hipMemcpyAsync(c->d_list_stats, &sp, sizeof(sp), hipMemcpyHostToDevice, c->s_compute));
	w.lists = ps.lists; w.stride = ps.list_max + 1; w.mac = ps.list_mac; w.flip = ps.list_flip; w.rowpop = ps.rowpop;
	w.n_list = zone; w.row0 = t.rowA0; w.n_rows = t.nA;
	w.col_hi = cr.d_hi; w.hi_a0 = cr.a0; w.hi_b0 = cr.b0;
	w.two_n = 2.0 * (double)c->N; w.cut = f.minR2 * (1.0 - 1e-6);
	w.cand = l.cand; w.cap = l.cand_cap; w.n_cand = s.n_out + 2;
	return TWK_HIP_OK;
}
// ... and end with, behind their screen kernel (between ev_c0 and ev_c1): the list math over the candidates (if anything ran), the launch's
// end, and the survivors' delivery like a tile's.
int end_list_launch(twk_hip_ctx* c, const twk_hip_tile_desc& t, bool ran, unsigned long long* n_out, const Deliver& to) {
	Slot& s = c->slot[SYNC_SLOT];
	HIPCHK(c, hipEventRecord(s.ev_c1, c->s_compute));
	if (ran) { const int rc = launch_list_math(c, s, c->d_list_stats); if (rc) return rc; }
	{ const int rc = close_launch(c, s); if (rc) return rc; }
	return finish_tile(c, s, t, n_out, to);
}

// Rows [row0, row0 + n_rows) of the list zone of an allele-count-sorted set, synchronously on the spare slot: every
// pair (i, j), i < j < zone, inside the r2 band, as an intersection of two carrier lists (ld_list.hip.h) -> candidates ->
// the list math kernel -> Fisher -> sorted survivors (delivered like a tile's).
int run_list_block(twk_hip_ctx* c, const twk_hip_filters& f, bool unphased, uint32_t row0, uint32_t n_rows, uint32_t zone, int32_t window, uint32_t l_window,
                   const ColRange& cr, unsigned long long capacity, unsigned long long* n_out, const Deliver& to) {
	twk_hip_tile_desc t{};
	t.rowA0 = row0; t.nA = n_rows; t.rowB0 = row0; t.nB = zone - row0; t.diag = 1; t.window = window; t.l_window = l_window;
	ListWork w{};
	int rc = begin_list_launch(c, f, unphased, false, t, zone, cr, capacity, w); if (rc) return rc;
	Slot& s = c->slot[SYNC_SLOT];
	// the widest row of the block decides the grid; lanes beyond a row's own reach leave at once
	uint32_t width = 0;
	for (uint32_t i = row0; i < row0 + n_rows; ++i) {
		const uint32_t lim = std::min<uint32_t>(zone, cr.hi ? cr.b0 + cr.hi[i - cr.a0] : zone);
		if (lim <= i + 1) continue;
		width = std::max(width, lim - i - 1);
		s.l.row_pairs += lim - i - 1;              // pairs intersected (accounting only)
	}
	HIPCHK(c, hipEventRecord(s.ev_c0, c->s_compute));
	if (width) {
		if (unphased) hipLaunchKernelGGL(k_list_screen_unphased, dim3((width + 255) / 256, n_rows), dim3(256), 0, c->s_compute, w, c->N);
		else hipLaunchKernelGGL(k_list_screen, dim3((width + 255) / 256, n_rows), dim3(256), 0, c->s_compute, w);
		HIPCHK(c, hipGetLastError());
	}
	return end_list_launch(c, t, width != 0, n_out, to);
}

// Zone rows [row0, row0 + n_rows) against the columns [col0, col0 + n_cols) outside the zone (col0 >= zone): every pair inside the
// r2 band as a probe of the row variant's carrier list into the column variant's plane row(s) (k_probe_screen, ld_list.hip.h) ->
// candidates -> the list math kernel -> Fisher -> sorted survivors, like a list block.
int run_probe_block(twk_hip_ctx* c, const twk_hip_filters& f, bool unphased, uint32_t row0, uint32_t n_rows, uint32_t zone, uint32_t col0, uint32_t n_cols,
                    int32_t window, uint32_t l_window, const ColRange& cr, unsigned long long capacity, unsigned long long* n_out, const Deliver& to) {
	twk_hip_tile_desc t{};
	t.rowA0 = row0; t.nA = n_rows; t.rowB0 = col0; t.nB = n_cols; t.diag = 0; t.window = window; t.l_window = l_window;
	ProbeWork p{};
	int rc = begin_list_launch(c, f, unphased, true, t, zone, cr, capacity, p.lw); if (rc) return rc;
	Slot& s = c->slot[SYNC_SLOT];
	const PlaneSet& ps = c->planes[s.l.plane_set];
	// through LDS (k_probe_lds_t: 512 rows x 4 columns a block, 2 columns of unphased planes); option probe_lds = 0: gathers straight from L2, one
	// column a block (the round-4 kernels: kept as the twin the LDS form is tested against)
	const bool via_lds = c->opt.probe_lds != 0;
	p.rows = ps.rows; p.W = ps.W; p.col0 = col0; p.n_cols = n_cols; p.n_row_blocks = via_lds ? (n_rows + PROBE_ROWS - 1) / PROBE_ROWS : (n_rows + 255) / 256;
	for (uint32_t i = row0; i < row0 + n_rows; ++i) {
		const uint32_t lim = std::min<uint64_t>((uint64_t)col0 + n_cols, cr.hi ? (uint64_t)cr.b0 + cr.hi[i - cr.a0] : (uint64_t)col0 + n_cols);
		const uint32_t first = std::max(col0, i + 1);             // (columns inside the zone: those behind the row)
		if (lim > first) s.l.row_pairs += lim - first;              // pairs probed (accounting only)
	}
	constexpr uint32_t LDS_COLS_P = 4, LDS_COLS_U = 2;
	const uint32_t strip_cols = via_lds ? (unphased ? LDS_COLS_U : LDS_COLS_P) : 1;
	const uint64_t n_blocks = (uint64_t)p.n_row_blocks * ((n_cols + strip_cols - 1) / strip_cols);
	if (n_blocks > 0x7FFFFFFFull) return TWK_HIP_E_INVALID;
	HIPCHK(c, hipEventRecord(s.ev_c0, c->s_compute));
	if (s.l.row_pairs) {
		const dim3 grid((uint32_t)n_blocks);
		if (via_lds && unphased) hipLaunchKernelGGL(k_probe_lds_unphased_t<LDS_COLS_U>, grid, dim3(PROBE_ROWS), 0, c->s_compute, p);
		else if (via_lds) hipLaunchKernelGGL(k_probe_lds_t<LDS_COLS_P>, grid, dim3(PROBE_ROWS), 0, c->s_compute, p);
		else if (unphased) hipLaunchKernelGGL(k_probe_screen_unphased_t<4>, grid, dim3(256), 0, c->s_compute, p, c->N);
		else hipLaunchKernelGGL(k_probe_screen, grid, dim3(256), 0, c->s_compute, p);
		HIPCHK(c, hipGetLastError());
	}
	return end_list_launch(c, t, s.l.row_pairs != 0, n_out, to);
}

// One tile, synchronously, on the spare slot; survivors go where `to` says.  `given` is what the caller allows the tile, narrowed here by what the
// call has given up since, and this is the one place that redoes a tile whose candidate list overflowed: down the ladder (step_down: two products ->
// three -> four through the matrix; fused -> the matrix), each launch's outcome folded into the call.  Nothing of an overflowed launch was kept (its
// recount and its list math left at once).
int run_tile_sync(twk_hip_ctx* c, int mode, const twk_hip_tile_desc& t, const twk_hip_filters& f, FormGrant given, CallForms& calls,
                  unsigned long long capacity, unsigned long long* n_out, const Deliver& to, const ColRange* cr = nullptr) {
	Slot& s = c->slot[SYNC_SLOT];
	for (;;) {
		const FormGrant grant = calls.redo_grant(given);
		int rc = enqueue_tile(c, mode, t, f, grant, s, capacity, cr); if (rc) return rc;
		rc = finish_tile(c, s, t, n_out, to);
		calls.gave_up(s.l.form, grant, s.l.cand_overflow, s.l.too_rich);
		if (!(rc == TWK_HIP_E_OVERFLOW && s.l.cand_overflow)) return rc;
		given = step_down(s.l.form, grant);
	}
}

int discard_records(void*, const twk_hip_record*, uint64_t) { return 0; }     // the sink of a caller that passed none

// A tile whose survivors overflowed the device buffer: redo it in row strips
// that cannot overflow (strip_rows * cols <= capacity).
// (cr: the region's column ranges - window, r2 band, list zone - so that a strip decides exactly the pairs its tile would have)
int redo_tile_in_strips(twk_hip_ctx* c, int mode, const twk_hip_tile_desc& t, const twk_hip_filters& f, const FormGrant& given, CallForms& calls,
                        unsigned long long capacity, const Deliver& to, uint64_t* n_recs, const ColRange* cr = nullptr) {
	const uint32_t strip = (uint32_t)std::max<unsigned long long>(1, capacity / std::max<uint32_t>(t.nB, 1));
	const bool diag = t.diag && t.rowA0 == t.rowB0;
	for (uint32_t r0 = 0; r0 < t.nA; r0 += strip) {
		const uint32_t nr = std::min(strip, t.nA - r0);
		twk_hip_tile_desc parts[2]; int np = 0;
		if (diag) {      // rows [r0, r0+nr): the diagonal sub-block, then the rectangle to its right
			twk_hip_tile_desc d = t; d.rowA0 = t.rowA0 + r0; d.nA = nr; d.rowB0 = d.rowA0; d.nB = nr; d.diag = 1;
			parts[np++] = d;
			if (r0 + nr < t.nB) {
				twk_hip_tile_desc r = t; r.rowA0 = t.rowA0 + r0; r.nA = nr; r.rowB0 = t.rowB0 + r0 + nr; r.nB = t.nB - (r0 + nr); r.diag = 0;
				parts[np++] = r;
			}
		} else {
			twk_hip_tile_desc r = t; r.rowA0 = t.rowA0 + r0; r.nA = nr; r.diag = 0;
			parts[np++] = r;
		}
		for (int k = 0; k < np; ++k) {
			unsigned long long n = 0;
			int rc = run_tile_sync(c, mode, parts[k], f, given, calls, (unsigned long long)parts[k].nA * parts[k].nB, &n, to, cr);
			if (rc) return rc;
			*n_recs += n;
		}
	}
	return TWK_HIP_OK;
}

// Per-variant metadata of variants [first, first + count): device SoA + host mirror (synchronous copies).
int upload_meta(twk_hip_ctx* c, uint32_t first, uint32_t count, const twk_hip_variant_meta* meta) {
	std::vector<uint32_t> ac(count), an(count), pos(count), rid(count), miss(count);
	std::vector<double> hwe(count);
	for (uint32_t i = 0; i < count; ++i) {
		ac[i] = meta[i].ac; an[i] = meta[i].an; pos[i] = meta[i].pos; rid[i] = meta[i].rid;
		miss[i] = meta[i].missing ? 1 : 0; hwe[i] = meta[i].hwe;
		c->h_meta[first + i] = meta[i];
		if (meta[i].missing) c->any_missing = true;
	}
	HIPCHK(c, hipMemcpy(c->d_ac + first, ac.data(), (size_t)count * 4, hipMemcpyHostToDevice));
	HIPCHK(c, hipMemcpy(c->d_an + first, an.data(), (size_t)count * 4, hipMemcpyHostToDevice));
	HIPCHK(c, hipMemcpy(c->d_pos + first, pos.data(), (size_t)count * 4, hipMemcpyHostToDevice));
	HIPCHK(c, hipMemcpy(c->d_rid + first, rid.data(), (size_t)count * 4, hipMemcpyHostToDevice));
	HIPCHK(c, hipMemcpy(c->d_missing + first, miss.data(), (size_t)count * 4, hipMemcpyHostToDevice));
	HIPCHK(c, hipMemcpy(c->d_hwe + first, hwe.data(), (size_t)count * 8, hipMemcpyHostToDevice));
	return TWK_HIP_OK;
}

bool valid_mode(int m) { return m == TWK_HIP_MODE_PHASED || m == TWK_HIP_MODE_UNPHASED || m == TWK_HIP_MODE_AUTO; }
bool valid_tile(const twk_hip_ctx* c, const twk_hip_tile_desc* t) {
	if (!t || t->nA == 0 || t->nB == 0 || t->nA > 32768 || t->nB > 32768) return false;
	if ((uint64_t)t->rowA0 + t->nA > c->M || (uint64_t)t->rowB0 + t->nB > c->M) return false;
	if (t->diag && (t->rowA0 != t->rowB0 || t->nB < t->nA)) return false;
	return true;
}

}  // namespace

void* HipDeliveryOps::alloc(size_t bytes) {
	if (c->opt.deliver_fail_alloc_at && ++n_alloc == c->opt.deliver_fail_alloc_at) return nullptr;      // (test hook)
	void* p = nullptr;
	if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
	return p;
}
void HipDeliveryOps::release(void* p) { (void)hipFree(p); }
int HipDeliveryOps::copy_aside(void* dst, const void* src, size_t bytes) {
	if (c->opt.deliver_fail_copy_at && ++n_copy == c->opt.deliver_fail_copy_at) {      // (test hook)
		snprintf(c->err, sizeof(c->err), "staging copy of a launch's survivors failed (option deliver_fail_copy_at)");
		return TWK_HIP_E_DEVICE;
	}
	HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->s_copy));
	HIPCHK(c, hipStreamSynchronize(c->s_copy));
	return TWK_HIP_OK;
}
int HipDeliveryOps::deliver(const void* recs, uint64_t n, twk_hip_record_sink sink, void* user, char* err, size_t err_len) {
	return deliver_records(c, static_cast<const twk_hip_record*>(recs), n, sink, user, c->s_deliver, 0.0, err, err_len);
}
void HipDeliveryOps::thread_begin() {
	(void)hipSetDevice(c->device);
	if (!c->deliver_warm) {          // this thread's and this stream's first copy sets up a queue (tens of milliseconds): now, behind the first launches
		uint32_t x = 0;
		if (c->tickets && hipMemcpyAsync(&x, c->tickets, 4, hipMemcpyDeviceToHost, c->s_deliver) == hipSuccess) (void)hipStreamSynchronize(c->s_deliver);
		c->deliver_warm = true;
	}
}

// ================================ C ABI =======================================================
extern "C" {

int twk_hip_abi_version(void) { return TWK_HIP_ABI_VERSION; }

int twk_hip_device_count(void) {
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) return 0;
	return n;
}

const char* twk_hip_strerror(int code) {
	switch (code) {
	case TWK_HIP_OK: return "ok";
	case TWK_HIP_E_INVALID: return "invalid argument";
	case TWK_HIP_E_NOMEM: return "out of memory";
	case TWK_HIP_E_DEVICE: return "HIP device error";
	case TWK_HIP_E_OVERFLOW: return "record buffer too small";
	case TWK_HIP_E_STATE: return "call sequence error";
	default: return "unknown error";
	}
}

const char* twk_hip_last_error(const twk_hip_ctx* ctx) { return ctx ? ctx->err : ""; }

int twk_hip_ctx_create(int device, twk_hip_ctx** out) {
	if (!out) return TWK_HIP_E_INVALID;
	*out = nullptr;
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return TWK_HIP_E_DEVICE;
	if (device < 0 || device >= n) return TWK_HIP_E_INVALID;
	twk_hip_ctx* c = new (std::nothrow) twk_hip_ctx();
	if (!c) return TWK_HIP_E_NOMEM;
	c->device = device;
	auto fail = [&](int code) { twk_hip_ctx_destroy(c); return code; };
	if (hipSetDevice(device) != hipSuccess) return fail(TWK_HIP_E_DEVICE);
	{
		int cus = 0;
		if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) c->resident_blocks = 2u * (uint32_t)cus;
	}
	if (hipStreamCreateWithFlags(&c->s_compute, hipStreamNonBlocking) != hipSuccess) return fail(TWK_HIP_E_DEVICE);
	{	// The copy stream carries the sort of a launch's survivors and their copy to the host, beside the next launch's persistent
		// count kernel on the compute stream.  At normal priority each of the sort's half-dozen dependent kernels had to wait for
		// the CUs the previous one freed, and lost them to the count kernel's waiting blocks every time - one sort kernel per gap
		// between count launches; at the highest priority its blocks are placed first.
		int lo = 0, hi = 0;
		if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) { lo = hi = 0; }
		if (hipStreamCreateWithPriority(&c->s_copy, hipStreamNonBlocking, hi) != hipSuccess) return fail(TWK_HIP_E_DEVICE);
		if (hipStreamCreateWithPriority(&c->s_deliver, hipStreamNonBlocking, hi) != hipSuccess) return fail(TWK_HIP_E_DEVICE);
	}
	c->graveyard.reclaim = [c] { return reclaim_device_memory(c); };
	if (c->tickets.reserve(2 * (PIPE_SLOTS + 1) * 8, 2 * (PIPE_SLOTS + 1) * 8, nullptr) != hipSuccess) return fail(TWK_HIP_E_NOMEM);
	for (auto& s : c->slot) {
		hipEvent_t* evs[] = {&s.ev_c0, &s.ev_c1, &s.ev_s1, &s.ev_c0b, &s.ev_c1b};
		for (auto* e : evs) if (hipEventCreate(e) != hipSuccess) return fail(TWK_HIP_E_DEVICE);
		if (s.n_out.reserve(N_SLOT_COUNTERS, N_SLOT_COUNTERS, nullptr) != hipSuccess) return fail(TWK_HIP_E_NOMEM);
		if (s.h_n_out.reserve(N_SLOT_COUNTERS, N_SLOT_COUNTERS, nullptr) != hipSuccess) return fail(TWK_HIP_E_NOMEM);
		std::memset(s.h_n_out, 0, N_SLOT_COUNTERS * sizeof(unsigned long long));
	}
	*out = c;
	return TWK_HIP_OK;
}

int twk_hip_ctx_destroy(twk_hip_ctx* c) {
	if (!c) return TWK_HIP_OK;
	(void)hipSetDevice(c->device);
	(void)hipDeviceSynchronize();
	(void)c->dl.end();                       // (before the buffers it may be copying from go)
	for (auto& s : c->slot) {
		hipEvent_t evs[] = {s.ev_c0, s.ev_c1, s.ev_s1, s.ev_c0b, s.ev_c1b};
		for (auto e : evs) if (e) (void)hipEventDestroy(e);
	}
	if (c->s_compute) (void)hipStreamDestroy(c->s_compute);
	if (c->s_copy) (void)hipStreamDestroy(c->s_copy);
	if (c->s_deliver) (void)hipStreamDestroy(c->s_deliver);
	delete c;
	return TWK_HIP_OK;
}

int twk_hip_host_alloc(size_t bytes, void** out) {
	if (!out || bytes == 0) return TWK_HIP_E_INVALID;
	*out = nullptr;
	return hipHostMalloc(out, bytes, hipHostMallocDefault) == hipSuccess ? TWK_HIP_OK : TWK_HIP_E_NOMEM;
}
int twk_hip_host_free(void* p) {
	if (!p) return TWK_HIP_OK;
	return hipHostFree(p) == hipSuccess ? TWK_HIP_OK : TWK_HIP_E_DEVICE;
}

int twk_hip_set_problem(twk_hip_ctx* c, uint32_t n_samples, uint32_t n_variants) {
	if (!c || n_samples == 0 || n_variants == 0) return TWK_HIP_E_INVALID;
	if (n_samples > (1u << 30)) return TWK_HIP_E_INVALID;       // counts are u32 on the device
	HIPCHK(c, hipSetDevice(c->device));
	free_problem(c);
	c->N = n_samples; c->M = n_variants;
	c->M_alloc = round_up(n_variants, TILE) + TILE;
	c->Wp = round_up((uint32_t)((2ull * n_samples + 31) / 32), KC);
	c->Wu = round_up((n_samples + 31) / 32, KC);
	const size_t raw_bytes = (size_t)c->M_alloc * c->Wp * 4;
	HIPCHK(c, c->raw.reserve(raw_bytes / 4, raw_bytes / 4, nullptr));
	HIPCHK(c, hipMemset(c->raw, 0, raw_bytes));
	const size_t m4 = (size_t)c->M_alloc * 4;
	for (DevBuf<uint32_t>* b : {&c->d_ac, &c->d_an, &c->d_pos, &c->d_rid, &c->d_missing}) HIPCHK(c, b->reserve(c->M_alloc, c->M_alloc, nullptr));
	HIPCHK(c, c->d_hwe.reserve(c->M_alloc, c->M_alloc, nullptr));
	HIPCHK(c, hipMemset(c->d_ac, 0, m4)); HIPCHK(c, hipMemset(c->d_an, 0, m4)); HIPCHK(c, hipMemset(c->d_pos, 0, m4));
	HIPCHK(c, hipMemset(c->d_rid, 0, m4)); HIPCHK(c, hipMemset(c->d_missing, 0, m4)); HIPCHK(c, hipMemset(c->d_hwe, 0, (size_t)c->M_alloc * 8));
	c->h_meta.assign(n_variants, twk_hip_variant_meta{});
	c->timing.words_per_row = 0;
	{	// every count Fisher's test sees is <= 2N (+ rounding of the unphased expected counts); beyond 2^26 entries lgamma itself is used
		const unsigned long long want = std::min<unsigned long long>(2ull * n_samples + 16, 1ull << 26);
		HIPCHK(c, c->d_lfact.reserve(want, want, nullptr));
		c->lfact_n = (int)want;
		hipLaunchKernelGGL(k_build_lfact, dim3((unsigned)((want + 255) / 256)), dim3(256), 0, c->s_compute, c->d_lfact, c->lfact_n);
		HIPCHK(c, hipGetLastError());
		HIPCHK(c, hipStreamSynchronize(c->s_compute));
	}
	return TWK_HIP_OK;
}

int twk_hip_upload_bitvectors(twk_hip_ctx* c, uint32_t first, uint32_t count, const uint64_t* data,
                              const uint64_t* mask, size_t stride64, const twk_hip_variant_meta* meta) {
	if (!c || !data || !meta || count == 0) return TWK_HIP_E_INVALID;
	if (c->raw && c->varbase.active) { snprintf(c->err, sizeof(c->err), "%s: a variant selection is active (twk_hip_select_variants(ctx, NULL, NULL, 0, 0, ..) drops it)", "twk_hip_upload_bitvectors"); return TWK_HIP_E_STATE; }
	if (!c->raw || c->source.active) return TWK_HIP_E_STATE;      // (a selection is dropped first: twk_hip_select_samples, twk_hip_select_variants)
	const size_t w64 = ((size_t)2 * c->N + 63) / 64;
	if (stride64 < w64 || (uint64_t)first + count > c->M) return TWK_HIP_E_INVALID;
	// Validate everything before any device or context state changes.  A variant's missing-data
	// flags must agree: the reference picks the pair math from `an` (ld_engine.cpp:2775) and builds
	// the mask from `gt_missing` (core.cpp:356-358); both come from the same genotypes in any .twk
	// its importer writes, and the plane selection here relies on that.
	for (uint32_t i = 0; i < count; ++i) {
		if (meta[i].missing && !mask) return TWK_HIP_E_INVALID;
		if ((meta[i].an != 0) != (meta[i].missing != 0)) return TWK_HIP_E_INVALID;
	}
	HIPCHK(c, hipSetDevice(c->device));
	free_planes(c);                                             // derived planes are stale now
	c->has_data = true;
	HIPCHK(c, hipMemcpy2D(c->raw + (size_t)first * c->Wp, (size_t)c->Wp * 4, data, stride64 * 8, w64 * 8, count, hipMemcpyHostToDevice));
	hipLaunchKernelGGL(k_clear_tail, dim3((c->Wp + 255) / 256, std::min<uint32_t>(count, 65535u)), dim3(256), 0, c->s_compute,
	                   c->raw + (size_t)first * c->Wp, c->Wp, c->N, count);
	HIPCHK(c, hipGetLastError());
	if (mask) {
		if (!c->rawmask) {
			const size_t raw_bytes = (size_t)c->M_alloc * c->Wp * 4;
			HIPCHK(c, c->rawmask.reserve(raw_bytes / 4, raw_bytes / 4, nullptr));
			HIPCHK(c, hipMemset(c->rawmask, 0, raw_bytes));
		}
		HIPCHK(c, hipMemcpy2D(c->rawmask + (size_t)first * c->Wp, (size_t)c->Wp * 4, mask, stride64 * 8, w64 * 8, count, hipMemcpyHostToDevice));
		hipLaunchKernelGGL(k_clear_tail, dim3((c->Wp + 255) / 256, std::min<uint32_t>(count, 65535u)), dim3(256), 0, c->s_compute,
		                   c->rawmask + (size_t)first * c->Wp, c->Wp, c->N, count);
		HIPCHK(c, hipGetLastError());
	}
	int rc = upload_meta(c, first, count, meta); if (rc) return rc;
	HIPCHK(c, hipStreamSynchronize(c->s_compute));
	return TWK_HIP_OK;
}

int twk_hip_upload_rle(twk_hip_ctx* c, uint32_t first, uint32_t count, const void* bytes, size_t n_bytes,
                       const twk_hip_rle_desc* desc, const twk_hip_variant_meta* meta) {
	if (!c || !bytes || !desc || !meta || count == 0) return TWK_HIP_E_INVALID;
	if (c->raw && c->varbase.active) { snprintf(c->err, sizeof(c->err), "twk_hip_upload_rle: a variant selection is active (twk_hip_select_variants(ctx, NULL, NULL, 0, 0, ..) drops it)"); return TWK_HIP_E_STATE; }
	if (!c->raw || c->source.active) return TWK_HIP_E_STATE;
	if ((uint64_t)first + count > c->M) return TWK_HIP_E_INVALID;
	// validate before anything changes (same rules as twk_hip_upload_bitvectors)
	bool any_mask = false;
	std::vector<RleDesc> dd(count);
	std::vector<uint32_t> chunk_base(count + 1);      // one block per chunk of RLE_CHUNK_BYTES run bytes, at least one per variant
	uint64_t n_chunks = 0;
	for (uint32_t i = 0; i < count; ++i) {
		const twk_hip_rle_desc& d = desc[i];
		if (d.width != 1 && d.width != 2 && d.width != 4) return TWK_HIP_E_INVALID;
		if (d.offset > n_bytes || (uint64_t)d.n_runs * d.width > n_bytes - d.offset) return TWK_HIP_E_INVALID;
		if ((meta[i].missing != 0) != (d.missing != 0)) return TWK_HIP_E_INVALID;
		if ((meta[i].an != 0) != (meta[i].missing != 0)) return TWK_HIP_E_INVALID;
		if (d.missing) any_mask = true;
		dd[i].off = d.offset; dd[i].n_runs = d.n_runs; dd[i].width_missing = (uint32_t)d.width | (d.missing ? 256u : 0u);
		chunk_base[i] = (uint32_t)n_chunks;
		n_chunks += std::max<uint64_t>(1, ((uint64_t)d.n_runs * d.width + RLE_CHUNK_BYTES - 1) / RLE_CHUNK_BYTES);
	}
	if (n_chunks > 0x7FFFFFFFull) return TWK_HIP_E_INVALID;
	chunk_base[count] = (uint32_t)n_chunks;
	HIPCHK(c, hipSetDevice(c->device));
	free_planes(c);                                             // derived planes are stale now
	c->has_data = true;
	// descriptors | chunk sums (u64 per block) | first block of every variant
	const size_t desc_bytes = (size_t)count * sizeof(RleDesc) + (size_t)n_chunks * 8 + ((size_t)count + 1) * 4;
	const size_t run_bytes = n_bytes + 32;                                  // the kernel's dword loads run up to 19 bytes past the last run
	HIPCHK(c, c->d_rle.reserve(run_bytes, run_bytes + run_bytes / 4, nullptr));
	HIPCHK(c, c->d_rle_desc.reserve(desc_bytes, desc_bytes + desc_bytes / 4, nullptr));
	HIPCHK(c, c->d_status.reserve(1, 1, nullptr));
	if (any_mask && !c->rawmask) {
		const size_t raw_bytes = (size_t)c->M_alloc * c->Wp * 4;
		HIPCHK(c, c->rawmask.reserve(raw_bytes / 4, raw_bytes / 4, nullptr));
		HIPCHK(c, hipMemsetAsync(c->rawmask, 0, raw_bytes, c->s_compute));
	}
	RleDesc* d_desc = reinterpret_cast<RleDesc*>(c->d_rle_desc.get());
	unsigned long long* d_chunk_sum = reinterpret_cast<unsigned long long*>(c->d_rle_desc + (size_t)count * sizeof(RleDesc));
	uint32_t* d_chunk_base = reinterpret_cast<uint32_t*>(c->d_rle_desc + (size_t)count * sizeof(RleDesc) + (size_t)n_chunks * 8);
	HIPCHK(c, hipMemsetAsync(c->d_status, 0, sizeof(int), c->s_compute));
	HIPCHK(c, hipMemcpyAsync(c->d_rle, bytes, n_bytes, hipMemcpyHostToDevice, c->s_compute));
	HIPCHK(c, hipMemcpyAsync(d_desc, dd.data(), (size_t)count * sizeof(RleDesc), hipMemcpyHostToDevice, c->s_compute));
	// the kernel ORs the ALT / missing runs into rows of zeros
	HIPCHK(c, hipMemsetAsync(c->raw + (size_t)first * c->Wp, 0, (size_t)count * c->Wp * 4, c->s_compute));
	if (c->rawmask) HIPCHK(c, hipMemsetAsync(c->rawmask + (size_t)first * c->Wp, 0, (size_t)count * c->Wp * 4, c->s_compute));
	HIPCHK(c, hipMemcpyAsync(d_chunk_base, chunk_base.data(), ((size_t)count + 1) * 4, hipMemcpyHostToDevice, c->s_compute));
	hipLaunchKernelGGL(k_rle_chunk_sums, dim3((uint32_t)n_chunks), dim3(256), 0, c->s_compute, c->d_rle, d_desc, d_chunk_base, count, d_chunk_sum);
	HIPCHK(c, hipGetLastError());
	hipLaunchKernelGGL(k_inflate_rle, dim3((uint32_t)n_chunks), dim3(256), 0, c->s_compute, c->d_rle, d_desc, d_chunk_base, count, d_chunk_sum,
	                   c->raw, c->rawmask, c->Wp, c->N, first, c->d_status);
	HIPCHK(c, hipGetLastError());
	int status = 0;
	HIPCHK(c, hipMemcpyAsync(&status, c->d_status, sizeof(int), hipMemcpyDeviceToHost, c->s_compute));
	int rc = upload_meta(c, first, count, meta); if (rc) return rc;
	HIPCHK(c, hipStreamSynchronize(c->s_compute));
	if (status) { snprintf(c->err, sizeof(c->err), "run lengths of an uploaded variant do not add up to %u samples", c->N); return TWK_HIP_E_INVALID; }
	return TWK_HIP_OK;
}

int twk_hip_download_bitvectors(twk_hip_ctx* c, uint32_t first, uint32_t count, uint64_t* data, uint64_t* mask, size_t stride64) {
	if (!c || !data || count == 0) return TWK_HIP_E_INVALID;
	if (!c->raw) return TWK_HIP_E_STATE;
	const size_t w64 = ((size_t)2 * c->N + 63) / 64;
	if (stride64 < w64 || (uint64_t)first + count > c->M) return TWK_HIP_E_INVALID;
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->s_compute));
	HIPCHK(c, hipMemcpy2D(data, stride64 * 8, c->raw + (size_t)first * c->Wp, (size_t)c->Wp * 4, w64 * 8, count, hipMemcpyDeviceToHost));
	if (mask) {
		if (c->rawmask) HIPCHK(c, hipMemcpy2D(mask, stride64 * 8, c->rawmask + (size_t)first * c->Wp, (size_t)c->Wp * 4, w64 * 8, count, hipMemcpyDeviceToHost));
		else for (uint32_t i = 0; i < count; ++i) std::memset(mask + (size_t)i * stride64, 0, w64 * 8);
	}
	return TWK_HIP_OK;
}

int twk_hip_generate_synthetic(twk_hip_ctx* c, uint64_t seed) { return twk_hip_generate_synthetic_planted(c, seed, 0, nullptr); }
int twk_hip_generate_synthetic_range(twk_hip_ctx* c, uint64_t seed, uint32_t first_variant) { return twk_hip_generate_synthetic_planted(c, seed, first_variant, nullptr); }

// twk_hip_plant -> the generator's own form (max_eps as a 32-bit fraction); false: out of range
static bool plant_of(const twk_hip_plant* p, SynthPlant& out) {
	out = SynthPlant{0, 0, 1, 0, 0};
	if (!p || p->n_planted == 0) return true;
	if (p->n_planted > p->half || p->mult == 0 || !(p->max_eps >= 0.0 && p->max_eps <= 0.5)) return false;
	out.n_planted = p->n_planted; out.half = p->half; out.mult = p->mult; out.offset = p->offset;
	out.eps_scale = (uint32_t)(p->max_eps * 4294967296.0);
	return true;
}

int twk_hip_generate_synthetic_planted(twk_hip_ctx* c, uint64_t seed, uint32_t first_variant, const twk_hip_plant* plant) {
	if (!c) return TWK_HIP_E_INVALID;
	if ((uint64_t)first_variant + (c ? c->M : 0) > 0xFFFFFFFFull) return TWK_HIP_E_INVALID;
	SynthPlant pl;
	if (!plant_of(plant, pl)) return TWK_HIP_E_INVALID;
	if (c->raw && c->varbase.active) { snprintf(c->err, sizeof(c->err), "twk_hip_generate_synthetic: a variant selection is active (twk_hip_select_variants(ctx, NULL, NULL, 0, 0, ..) drops it)"); return TWK_HIP_E_STATE; }
	if (!c->raw || c->source.active) return TWK_HIP_E_STATE;
	HIPCHK(c, hipSetDevice(c->device));
	free_planes(c);
	c->has_data = true;
	c->rawmask.reset();
	c->any_missing = false;
	hipLaunchKernelGGL(k_synth, dim3((c->Wp + 255) / 256, std::min<uint32_t>(c->M, 65535u)), dim3(256), 0, c->s_compute, c->raw, c->Wp, c->N, c->M, seed, first_variant, pl);
	HIPCHK(c, hipGetLastError());
	// metadata: ac = popcount, pos = 1000 + 100 v, one contig, hwe = 1
	hipLaunchKernelGGL(k_row_popcount, dim3((c->M + 3) / 4), dim3(256), 0, c->s_compute, c->raw, c->Wp, c->M, c->d_ac);
	HIPCHK(c, hipGetLastError());
	std::vector<uint32_t> pos(c->M), zero(c->M, 0), ac(c->M);
	std::vector<double> hwe(c->M, 1.0);
	for (uint32_t v = 0; v < c->M; ++v) pos[v] = 1000u + 100u * (first_variant + v);
	HIPCHK(c, hipMemcpyAsync(c->d_pos, pos.data(), (size_t)c->M * 4, hipMemcpyHostToDevice, c->s_compute));
	HIPCHK(c, hipMemcpyAsync(c->d_an, zero.data(), (size_t)c->M * 4, hipMemcpyHostToDevice, c->s_compute));
	HIPCHK(c, hipMemcpyAsync(c->d_rid, zero.data(), (size_t)c->M * 4, hipMemcpyHostToDevice, c->s_compute));
	HIPCHK(c, hipMemcpyAsync(c->d_missing, zero.data(), (size_t)c->M * 4, hipMemcpyHostToDevice, c->s_compute));
	HIPCHK(c, hipMemcpyAsync(c->d_hwe, hwe.data(), (size_t)c->M * 8, hipMemcpyHostToDevice, c->s_compute));
	HIPCHK(c, hipMemcpyAsync(ac.data(), c->d_ac, (size_t)c->M * 4, hipMemcpyDeviceToHost, c->s_compute));
	HIPCHK(c, hipStreamSynchronize(c->s_compute));
	for (uint32_t v = 0; v < c->M; ++v) {
		twk_hip_variant_meta m{}; m.ac = ac[v]; m.pos = pos[v]; m.hwe = 1.0;
		c->h_meta[v] = m;
	}
	return TWK_HIP_OK;
}

uint32_t twk_synth_bitvector(uint64_t seed, uint32_t n_samples, uint32_t v, uint64_t* out_words) {
	return twk_synth_planted_bitvector(seed, n_samples, v, nullptr, out_words);
}

uint32_t twk_synth_planted_bitvector(uint64_t seed, uint32_t n_samples, uint32_t v, const twk_hip_plant* plant, uint64_t* out_words) {
	const size_t w64 = ((size_t)2 * n_samples + 63) / 64;
	std::memset(out_words, 0, w64 * 8);
	SynthPlant pl;
	if (!plant_of(plant, pl)) return 0;
	uint32_t src = v, eps_thr = 0;
	const bool copy = synth_plant_source(seed, pl, v, src, eps_thr);
	const uint32_t thr = synth_threshold(seed, src);
	uint32_t ac = 0;
	for (uint32_t s = 0; s < n_samples; ++s) {
		const uint64_t bits = synth_sample_bits(seed, src, s, thr) ^ (copy ? synth_flip_bits(seed, v, s, eps_thr) : 0u);
		out_words[(2ull * s) >> 6] |= bits << ((2ull * s) & 63);
		ac += (uint32_t)(bits & 1) + (uint32_t)(bits >> 1);
	}
	return ac;
}

int twk_synth_plant_source(uint64_t seed, const twk_hip_plant* plant, uint32_t v, uint32_t* src, double* eps) {
	SynthPlant pl;
	uint32_t s = v, thr = 0;
	const bool copy = plant_of(plant, pl) && synth_plant_source(seed, pl, v, s, thr);
	if (src) *src = copy ? s : v;
	if (eps) *eps = copy ? (double)thr / 4294967296.0 : 0.0;
	return copy ? 1 : 0;
}

int twk_hip_get_marginals(twk_hip_ctx* c, uint32_t* ac, uint32_t* n_het, uint32_t* n_hom, uint32_t* n_miss) {
	if (!c) return TWK_HIP_E_INVALID;
	if (!c->raw) return TWK_HIP_E_STATE;
	HIPCHK(c, hipSetDevice(c->device));
	if (ac) {
		const int kind = plane_kind_for(c, true);
		int rc = ensure_planes(c, kind); if (rc) return rc;
		const int P = planes_per_variant(kind);
		std::vector<uint32_t> rp((size_t)c->M * P);
		HIPCHK(c, hipMemcpy(rp.data(), c->planes[kind].rowpop, rp.size() * 4, hipMemcpyDeviceToHost));
		for (uint32_t v = 0; v < c->M; ++v) ac[v] = rp[(size_t)v * P];
	}
	if (n_het || n_hom || n_miss) {
		const int kind = plane_kind_for(c, false);
		int rc = ensure_planes(c, kind); if (rc) return rc;
		const int P = planes_per_variant(kind);
		std::vector<uint32_t> rp((size_t)c->M * P);
		HIPCHK(c, hipMemcpy(rp.data(), c->planes[kind].rowpop, rp.size() * 4, hipMemcpyDeviceToHost));
		for (uint32_t v = 0; v < c->M; ++v) {
			if (n_het) n_het[v] = rp[(size_t)v * P];
			if (n_hom) n_hom[v] = rp[(size_t)v * P + 1];
			if (n_miss) n_miss[v] = P == 3 ? rp[(size_t)v * P + 2] : 0;
		}
	}
	return TWK_HIP_OK;
}

extern "C++" {
namespace {
// The selection goes: the rows and the metadata as uploaded are the context's again, bit for bit (nothing is copied but the metadata).
int drop_selection(twk_hip_ctx* c) {
	if (!c->source.active) return TWK_HIP_OK;
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->s_compute));
	free_planes(c);
	c->raw = std::move(c->source.raw); c->rawmask = std::move(c->source.rawmask);
	c->N = c->source.N; c->Wp = c->source.Wp; c->Wu = c->source.Wu;
	c->h_meta = std::move(c->source.h_meta); c->source.h_meta.clear();
	c->source.active = false;
	c->any_missing = false;                                     // (upload_meta sets it from the metadata)
	const std::vector<twk_hip_variant_meta> meta = c->h_meta;
	return upload_meta(c, 0, c->M, meta.data());
}
}  // namespace
}

int twk_hip_select_samples(twk_hip_ctx* c, const uint32_t* keep, uint32_t n_keep) {
	if (!c) return TWK_HIP_E_INVALID;
	if (!keep && n_keep != 0) { snprintf(c->err, sizeof(c->err), "twk_hip_select_samples: no list, but a count of %u", n_keep); return TWK_HIP_E_INVALID; }
	if (!c->raw || !c->has_data) return TWK_HIP_E_STATE;
	if (c->varbase.active) { snprintf(c->err, sizeof(c->err), "twk_hip_select_samples: a variant selection is active (twk_hip_select_variants drops it)"); return TWK_HIP_E_STATE; }
	if (!keep) return drop_selection(c);
	const uint32_t n_src = c->source.active ? c->source.N : c->N, w_src = c->source.active ? c->source.Wp : c->Wp;
	if (n_keep == 0) { snprintf(c->err, sizeof(c->err), "twk_hip_select_samples: an empty list"); return TWK_HIP_E_INVALID; }
	const uint32_t Wp = round_up((uint32_t)((2ull * n_keep + 31) / 32), KC), Wu = round_up((n_keep + 31) / 32, KC);
	std::vector<SubsetEntry> table; std::vector<SubsetChunk> chunks;
	uint32_t bad_at = 0;
	if (n_keep > n_src || !build_subset_table(keep, n_keep, n_src, Wp, table, chunks, &bad_at)) {
		if (n_keep > n_src) snprintf(c->err, sizeof(c->err), "twk_hip_select_samples: %u samples listed, the source has %u", n_keep, n_src);
		else snprintf(c->err, sizeof(c->err), "twk_hip_select_samples: keep[%u] = %u is not above its predecessor and below the source's %u samples", bad_at, keep[bad_at], n_src);
		return TWK_HIP_E_INVALID;
	}
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->s_compute));
	const uint32_t* src_raw = c->source.active ? c->source.raw.get() : c->raw.get();
	const uint32_t* src_mask = c->source.active ? c->source.rawmask.get() : c->rawmask.get();
	const std::vector<twk_hip_variant_meta>& src_meta = c->source.active ? c->source.h_meta : c->h_meta;
	const int n_planes = src_mask ? 2 : 1;
	// everything new is built beside what the context holds, and nothing of the context changes until all of it stands
	const size_t row_words = (size_t)c->M_alloc * Wp;
	DevBuf<uint32_t> rows[2], d_pop[2];
	DevBuf<SubsetEntry> d_table; DevBuf<SubsetChunk> d_chunks;
	{
		hipError_t e = hipSuccess;
		for (int p = 0; p < n_planes && e == hipSuccess; ++p) e = rows[p].reserve(row_words, row_words, nullptr);
		for (int p = 0; p < n_planes && e == hipSuccess; ++p) e = d_pop[p].reserve(c->M, c->M, nullptr);
		if (e == hipSuccess) e = d_table.reserve(table.size(), table.size(), nullptr);
		if (e == hipSuccess) e = d_chunks.reserve(chunks.size(), chunks.size(), nullptr);
		if (e != hipSuccess) {
			(void)hipGetLastError();
			snprintf(c->err, sizeof(c->err), "twk_hip_select_samples: the working copy of %u variants x %u samples needs %llu bytes of device memory beside the source: %s",
			         c->M, n_keep, (unsigned long long)(row_words * 4 * n_planes), hipGetErrorString(e));
			return e == hipErrorOutOfMemory ? TWK_HIP_E_NOMEM : TWK_HIP_E_DEVICE;
		}
	}
	Events ev;
	HIPCHK(c, ev.add(2));
	HIPCHK(c, hipMemcpyAsync(d_table, table.data(), table.size() * sizeof(SubsetEntry), hipMemcpyHostToDevice, c->s_compute));
	HIPCHK(c, hipMemcpyAsync(d_chunks, chunks.data(), chunks.size() * sizeof(SubsetChunk), hipMemcpyHostToDevice, c->s_compute));
	// (the rows behind the last variant are padding of the count kernel's tiles: zeros, as twk_hip_set_problem leaves them)
	for (int p = 0; p < n_planes; ++p) HIPCHK(c, hipMemsetAsync(rows[p] + (size_t)c->M * Wp, 0, (size_t)(c->M_alloc - c->M) * Wp * 4, c->s_compute));
	SubsetArgs a{};
	a.src[0] = src_raw; a.src[1] = src_mask; a.dst[0] = rows[0]; a.dst[1] = rows[1];
	a.table = d_table; a.chunks = d_chunks; a.w_src = w_src; a.w_dst = Wp; a.n_rows = c->M;
	const uint32_t row_groups = (c->M + SUBSET_ROWS - 1) / SUBSET_ROWS;
	HIPCHK(c, hipEventRecord(ev[0], c->s_compute));
	hipLaunchKernelGGL(k_subset_rows, dim3((unsigned)chunks.size(), std::min<uint32_t>(row_groups, 65535u), n_planes), dim3(256), 0, c->s_compute, a);
	HIPCHK(c, hipGetLastError());
	HIPCHK(c, hipEventRecord(ev[1], c->s_compute));
	// ac = ALT alleles of the kept samples, an = two per kept sample with a missing genotype: popcounts of the new rows
	std::vector<uint32_t> pop[2];
	for (int p = 0; p < n_planes; ++p) {
		hipLaunchKernelGGL(k_row_popcount, dim3((c->M + 3) / 4), dim3(256), 0, c->s_compute, (const uint32_t*)rows[p], Wp, c->M, d_pop[p].get());
		HIPCHK(c, hipGetLastError());
		pop[p].resize(c->M);
		HIPCHK(c, hipMemcpyAsync(pop[p].data(), d_pop[p], (size_t)c->M * 4, hipMemcpyDeviceToHost, c->s_compute));
	}
	HIPCHK(c, hipStreamSynchronize(c->s_compute));
	float ms = 0.f;
	HIPCHK(c, hipEventElapsedTime(&ms, ev[0], ev[1]));
	std::vector<twk_hip_variant_meta> meta = src_meta;
	bool any_missing = false;
	for (uint32_t v = 0; v < c->M; ++v) {
		meta[v].ac = pop[0][v];
		meta[v].an = n_planes == 2 ? pop[1][v] : 0;
		meta[v].missing = meta[v].an != 0;
		any_missing = any_missing || meta[v].missing;
	}
	// ... and now the context changes hands
	free_planes(c);
	if (!c->source.active) {
		c->source.raw = std::move(c->raw); c->source.rawmask = std::move(c->rawmask);
		c->source.N = c->N; c->source.Wp = c->Wp; c->source.Wu = c->Wu;
		c->source.h_meta = c->h_meta;
		c->source.active = true;
	}
	c->raw = std::move(rows[0]);
	if (any_missing) c->rawmask = std::move(rows[1]); else c->rawmask.reset();      // the mask rows are kept only while a working variant has missing data
	c->N = n_keep; c->Wp = Wp; c->Wu = Wu;
	c->any_missing = false;                                                         // (upload_meta sets it from the metadata)
	c->select_last.ms = ms;
	c->select_last.bytes_read = (uint64_t)c->M * table.size() * 4 * n_planes;
	c->select_last.bytes_written = (uint64_t)c->M * Wp * 4 * n_planes;
	return upload_meta(c, 0, c->M, meta.data());
}

int twk_hip_selection(const twk_hip_ctx* c, uint32_t* n_source, uint32_t* n_selected) {
	if (!c) return TWK_HIP_E_INVALID;
	if (!c->raw) return TWK_HIP_E_STATE;
	if (n_source) *n_source = c->source.active ? c->source.N : c->N;
	if (n_selected) *n_selected = c->N;
	return TWK_HIP_OK;
}

int twk_hip_get_meta(twk_hip_ctx* c, uint32_t first, uint32_t count, twk_hip_variant_meta* out) {
	if (!c || !out || count == 0) return TWK_HIP_E_INVALID;
	if (!c->raw) return TWK_HIP_E_STATE;
	if ((uint64_t)first + count > c->M) return TWK_HIP_E_INVALID;
	std::copy(c->h_meta.begin() + first, c->h_meta.begin() + first + count, out);
	return TWK_HIP_OK;
}

int twk_hip_set_hwe(twk_hip_ctx* c, uint32_t first, uint32_t count, const double* hwe) {
	if (!c || !hwe || count == 0) return TWK_HIP_E_INVALID;
	if (!c->raw) return TWK_HIP_E_STATE;
	if ((uint64_t)first + count > c->M) return TWK_HIP_E_INVALID;
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->s_compute));
	HIPCHK(c, hipMemcpy(c->d_hwe + first, hwe, (size_t)count * 8, hipMemcpyHostToDevice));
	for (uint32_t i = 0; i < count; ++i) c->h_meta[first + i].hwe = hwe[i];
	return TWK_HIP_OK;
}

int twk_hip_select_last(const twk_hip_ctx* c, double* select_ms, uint64_t* bytes_read, uint64_t* bytes_written) {
	if (!c) return TWK_HIP_E_INVALID;
	if (select_ms) *select_ms = c->select_last.ms;
	if (bytes_read) *bytes_read = c->select_last.bytes_read;
	if (bytes_written) *bytes_written = c->select_last.bytes_written;
	return TWK_HIP_OK;
}

extern "C++" {
namespace {
// The variant selection goes: the base's rows and metadata are the context's again, bit for bit.  Nothing is copied; the buffers move back.
int drop_variant_selection(twk_hip_ctx* c) {
	if (!c->varbase.active) return TWK_HIP_OK;
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->s_compute));
	free_planes(c);
	twk_hip_ctx::VarBase& b = c->varbase;
	c->raw = std::move(b.raw); c->rawmask = std::move(b.rawmask);
	c->d_ac = std::move(b.d_ac); c->d_an = std::move(b.d_an); c->d_pos = std::move(b.d_pos); c->d_rid = std::move(b.d_rid);
	c->d_missing = std::move(b.d_missing); c->d_hwe = std::move(b.d_hwe);
	c->h_meta = std::move(b.h_meta);
	c->M = b.M; c->M_alloc = b.M_alloc; c->any_missing = b.any_missing;
	b = twk_hip_ctx::VarBase();
	return TWK_HIP_OK;
}
}  // namespace
}

int twk_hip_select_variants(twk_hip_ctx* c, const twk_hip_variant_filter* filter, const uint32_t* list, uint32_t n_list, int32_t exclude, uint32_t* n_kept_out) {
	if (!c) return TWK_HIP_E_INVALID;
	if (!list && n_list != 0) { snprintf(c->err, sizeof(c->err), "twk_hip_select_variants: no list, but a count of %u", n_list); return TWK_HIP_E_INVALID; }
	VarselFilter f{0.0, 0.5, 0u, 1.0, 0.0};
	if (filter) {
		f = VarselFilter{filter->min_maf, filter->max_maf, filter->min_mac, filter->max_missing, filter->min_hwe};
		if (const char* fault = varsel_filter_fault(f)) {
			snprintf(c->err, sizeof(c->err), "twk_hip_select_variants: threshold %s is NaN or outside its range (min_maf %g, max_maf %g in [0, 0.5], max_missing %g, min_hwe %g in [0, 1])",
			         fault, f.min_maf, f.max_maf, f.max_missing, f.min_hwe);
			return TWK_HIP_E_INVALID;
		}
	}
	if (!c->raw || !c->has_data) { snprintf(c->err, sizeof(c->err), "twk_hip_select_variants: the context holds no data yet (%s): upload or generate first", c->raw ? "twk_hip_set_problem was called, nothing was uploaded" : "no twk_hip_set_problem"); return TWK_HIP_E_STATE; }
	if (!filter && !list) {
		const int rc = drop_variant_selection(c);
		if (rc == TWK_HIP_OK && n_kept_out) *n_kept_out = c->M;
		return rc;
	}
	twk_hip_ctx::VarBase& vb = c->varbase;
	const bool was = vb.active;
	const uint32_t Mb = was ? vb.M : c->M;
	for (uint32_t k = 0; k < n_list; ++k)
		if (list[k] >= Mb || (k && list[k] <= list[k - 1])) {
			snprintf(c->err, sizeof(c->err), "twk_hip_select_variants: list[%u] = %u is not above its predecessor and below the base's %u variants", k, list[k], Mb);
			return TWK_HIP_E_INVALID;
		}
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->s_compute));
	const uint32_t* b_raw = was ? vb.raw.get() : c->raw.get();
	const bool b_missing = was ? vb.any_missing : c->any_missing;
	const uint32_t* b_mask = b_missing ? (was ? vb.rawmask.get() : c->rawmask.get()) : nullptr;      // (mask rows count only while a variant is flagged missing: plane_kind_for)
	const uint32_t* b32[5] = {was ? vb.d_ac.get() : c->d_ac.get(), was ? vb.d_an.get() : c->d_an.get(), was ? vb.d_pos.get() : c->d_pos.get(),
	                          was ? vb.d_rid.get() : c->d_rid.get(), was ? vb.d_missing.get() : c->d_missing.get()};
	const double* b_hwe = was ? vb.d_hwe.get() : c->d_hwe.get();
	const std::vector<twk_hip_variant_meta>& b_meta = was ? vb.h_meta : c->h_meta;
	const uint32_t Wp = c->Wp;
	auto nomem = [c](hipError_t e, unsigned long long bytes, const char* what) {
		(void)hipGetLastError();
		snprintf(c->err, sizeof(c->err), "twk_hip_select_variants: %s needs %llu bytes of device memory beside the base: %s", what, bytes, hipGetErrorString(e));
		return e == hipErrorOutOfMemory ? TWK_HIP_E_NOMEM : TWK_HIP_E_DEVICE;
	};
	// everything new is built beside what the context holds, and nothing of the context changes until all of it stands
	// (a) the predicate, (b) the scan and the map
	DevBuf<uint32_t> d_listed, d_flag, d_off, d_map, d_n;
	DevBuf<char> d_tmp;
	size_t tmp_bytes = 0;
	HIPCHK(c, rocprim::exclusive_scan(nullptr, tmp_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)Mb, rocprim::plus<uint32_t>(), c->s_compute));
	{
		hipError_t e = hipSuccess;
		if (list) e = d_listed.reserve(Mb, Mb, nullptr);
		for (DevBuf<uint32_t>* b : {&d_flag, &d_off, &d_map}) if (e == hipSuccess) e = b->reserve(Mb, Mb, nullptr);
		if (e == hipSuccess) e = d_n.reserve(1, 1, nullptr);
		if (e == hipSuccess) e = d_tmp.reserve(std::max<size_t>(tmp_bytes, 16), std::max<size_t>(tmp_bytes, 16), nullptr);
		if (e != hipSuccess) return nomem(e, (unsigned long long)Mb * 16 + tmp_bytes, "the flags, the scan and the map");
	}
	Events ev;
	HIPCHK(c, ev.add(4));
	DevBuf<uint32_t> d_list;
	if (list) {
		HIPCHK(c, hipMemsetAsync(d_listed, 0, (size_t)Mb * 4, c->s_compute));
		if (n_list) {
			HIPCHK(c, d_list.reserve(n_list, n_list, nullptr));
			HIPCHK(c, hipMemcpyAsync(d_list, list, (size_t)n_list * 4, hipMemcpyHostToDevice, c->s_compute));
			hipLaunchKernelGGL(k_varsel_list_flags, dim3((n_list + 255) / 256), dim3(256), 0, c->s_compute, (const uint32_t*)d_list, n_list, d_listed.get());
			HIPCHK(c, hipGetLastError());
		}
	}
	VarselPredArgs pa{};
	pa.raw = b_raw; pa.rawmask = b_mask; pa.listed = list ? d_listed.get() : nullptr; pa.hwe = b_hwe; pa.flag = d_flag;
	pa.Wp = Wp; pa.n_variants = Mb; pa.n_samples = c->N; pa.exclude = exclude ? 1u : 0u; pa.f = f;
	HIPCHK(c, hipEventRecord(ev[0], c->s_compute));
	hipLaunchKernelGGL(k_varsel_predicate, dim3((Mb + 3) / 4), dim3(256), 0, c->s_compute, pa);
	HIPCHK(c, hipGetLastError());
	HIPCHK(c, rocprim::exclusive_scan(d_tmp.get(), tmp_bytes, d_flag.get(), d_off.get(), 0u, (size_t)Mb, rocprim::plus<uint32_t>(), c->s_compute));
	hipLaunchKernelGGL(k_varsel_map, dim3((Mb + 255) / 256), dim3(256), 0, c->s_compute, (const uint32_t*)d_flag, (const uint32_t*)d_off, Mb, d_map.get(), d_n.get());
	HIPCHK(c, hipGetLastError());
	HIPCHK(c, hipEventRecord(ev[1], c->s_compute));
	uint32_t n_kept = 0;
	HIPCHK(c, hipMemcpyAsync(&n_kept, d_n, 4, hipMemcpyDeviceToHost, c->s_compute));
	HIPCHK(c, hipStreamSynchronize(c->s_compute));
	if (n_kept == 0 || n_kept > Mb) {
		snprintf(c->err, sizeof(c->err), "twk_hip_select_variants: the selection keeps none of the base's %u variants", Mb);
		return TWK_HIP_E_INVALID;
	}
	// the map comes to the host once: for h_meta and twk_hip_variant_map
	std::vector<uint32_t> h_map(n_kept);
	HIPCHK(c, hipMemcpy(h_map.data(), d_map, (size_t)n_kept * 4, hipMemcpyDeviceToHost));
	std::vector<twk_hip_variant_meta> meta(n_kept);
	bool any_missing = false;
	for (uint32_t r = 0; r < n_kept; ++r) {
		if (h_map[r] >= Mb) { snprintf(c->err, sizeof(c->err), "twk_hip_select_variants: the map's entry %u is %u, beyond the base", r, h_map[r]); return TWK_HIP_E_DEVICE; }
		meta[r] = b_meta[h_map[r]];
		any_missing = any_missing || meta[r].missing;
	}
	// (c) the rows and the metadata SoA through the map
	const uint32_t M_alloc = round_up(n_kept, TILE) + TILE;
	const int n_planes = any_missing && b_mask ? 2 : 1;                // the mask rows are kept only while a working variant has missing data
	const size_t row_words = (size_t)M_alloc * Wp;
	DevBuf<uint32_t> rows[2], n32[5];
	DevBuf<double> n_hwe;
	{
		hipError_t e = hipSuccess;
		for (int p = 0; p < n_planes && e == hipSuccess; ++p) e = rows[p].reserve(row_words, row_words, nullptr);
		for (int k = 0; k < 5 && e == hipSuccess; ++k) e = n32[k].reserve(M_alloc, M_alloc, nullptr);
		if (e == hipSuccess) e = n_hwe.reserve(M_alloc, M_alloc, nullptr);
		if (e != hipSuccess) return nomem(e, (unsigned long long)row_words * 4 * n_planes + (unsigned long long)M_alloc * 28, "the working set");
	}
	VarselRowArgs ra{};
	ra.src[0] = b_raw; ra.src[1] = b_mask; ra.dst[0] = rows[0]; ra.dst[1] = rows[1]; ra.map = d_map;
	ra.g = varsel_gather_geometry(M_alloc, n_kept, Wp / 4);
	VarselMetaArgs ma{};
	for (int k = 0; k < 5; ++k) { ma.src32[k] = b32[k]; ma.dst32[k] = n32[k]; }
	ma.src_hwe = b_hwe; ma.dst_hwe = n_hwe; ma.map = d_map; ma.n_kept = n_kept; ma.n_out = M_alloc;
	HIPCHK(c, hipEventRecord(ev[2], c->s_compute));
	hipLaunchKernelGGL(k_varsel_rows, dim3(ra.g.n_blocks, 1, n_planes), dim3(VARSEL_BLOCK), 0, c->s_compute, ra);
	HIPCHK(c, hipGetLastError());
	hipLaunchKernelGGL(k_varsel_meta, dim3((M_alloc + 255) / 256), dim3(256), 0, c->s_compute, ma);
	HIPCHK(c, hipGetLastError());
	HIPCHK(c, hipEventRecord(ev[3], c->s_compute));
	HIPCHK(c, hipStreamSynchronize(c->s_compute));
	float ms_a = 0.f, ms_c = 0.f;
	HIPCHK(c, hipEventElapsedTime(&ms_a, ev[0], ev[1]));
	HIPCHK(c, hipEventElapsedTime(&ms_c, ev[2], ev[3]));
	// ... and now the context changes hands
	free_planes(c);
	if (!was) {
		vb.raw = std::move(c->raw); vb.rawmask = std::move(c->rawmask);
		vb.d_ac = std::move(c->d_ac); vb.d_an = std::move(c->d_an); vb.d_pos = std::move(c->d_pos); vb.d_rid = std::move(c->d_rid);
		vb.d_missing = std::move(c->d_missing); vb.d_hwe = std::move(c->d_hwe);
		vb.h_meta = std::move(c->h_meta);
		vb.M = c->M; vb.M_alloc = c->M_alloc; vb.any_missing = c->any_missing;
		vb.active = true;
	}
	vb.h_map = std::move(h_map);
	c->raw = std::move(rows[0]);
	if (n_planes == 2) c->rawmask = std::move(rows[1]); else c->rawmask.reset();
	c->d_ac = std::move(n32[0]); c->d_an = std::move(n32[1]); c->d_pos = std::move(n32[2]); c->d_rid = std::move(n32[3]); c->d_missing = std::move(n32[4]);
	c->d_hwe = std::move(n_hwe);
	c->h_meta = std::move(meta);
	c->M = n_kept; c->M_alloc = M_alloc; c->any_missing = any_missing;
	c->varsel_last.ms = (double)ms_a + (double)ms_c;
	c->varsel_last.bytes_read = (uint64_t)Mb * Wp * 4 * (b_mask ? 2 : 1) + (uint64_t)n_kept * Wp * 4 * n_planes;
	c->varsel_last.bytes_written = (uint64_t)M_alloc * Wp * 4 * n_planes;
	if (n_kept_out) *n_kept_out = n_kept;
	return TWK_HIP_OK;
}

int twk_hip_variant_selection(const twk_hip_ctx* c, uint32_t* n_before, uint32_t* n_selected) {
	if (!c) return TWK_HIP_E_INVALID;
	if (!c->raw) return TWK_HIP_E_STATE;
	if (n_before) *n_before = c->varbase.active ? c->varbase.M : c->M;
	if (n_selected) *n_selected = c->M;
	return TWK_HIP_OK;
}

int twk_hip_variant_map(const twk_hip_ctx* c, uint32_t first, uint32_t count, uint32_t* index_before) {
	if (!c || !index_before || count == 0) return TWK_HIP_E_INVALID;
	if (!c->raw) return TWK_HIP_E_STATE;
	if ((uint64_t)first + count > c->M) return TWK_HIP_E_INVALID;
	for (uint32_t i = 0; i < count; ++i) index_before[i] = c->varbase.active ? c->varbase.h_map[first + i] : first + i;
	return TWK_HIP_OK;
}

int twk_hip_select_variants_last(const twk_hip_ctx* c, double* select_ms, uint64_t* bytes_read, uint64_t* bytes_written) {
	if (!c) return TWK_HIP_E_INVALID;
	if (select_ms) *select_ms = c->varsel_last.ms;
	if (bytes_read) *bytes_read = c->varsel_last.bytes_read;
	if (bytes_written) *bytes_written = c->varsel_last.bytes_written;
	return TWK_HIP_OK;
}

// Buffers outgrown during a call: freed once nothing is in flight any more.
static void flush_graveyard(twk_hip_ctx* c) {
	if (c->graveyard.empty()) return;
	(void)hipSetDevice(c->device);
	(void)hipDeviceSynchronize();
	c->graveyard.flush();
}

int twk_hip_count_tile(twk_hip_ctx* c, int mode, const twk_hip_tile_desc* t, uint64_t* out) {
	if (!c || !out || (mode != TWK_HIP_MODE_PHASED && mode != TWK_HIP_MODE_UNPHASED)) return TWK_HIP_E_INVALID;
	if (!c->raw) return TWK_HIP_E_STATE;
	if (!valid_tile(c, t)) return TWK_HIP_E_INVALID;
	HIPCHK(c, hipSetDevice(c->device));
	const bool phased = mode == TWK_HIP_MODE_PHASED;
	const int kind = plane_kind_for(c, phased);
	int rc = ensure_planes(c, kind); if (rc) return rc;
	Slot& s = c->slot[SYNC_SLOT];
	const Geometry g = tile_geometry(planes_per_variant(kind), *t);
	rc = ensure_slot(c, s, (size_t)g.rowsA * g.rowsB, 1); if (rc) return rc;
	begin_launch(s, kind, 1.0);
	rc = launch_count(c, kind, *t, s, 0, nullptr, LaunchForm(), nullptr); if (rc) return rc;
	const int ncell = phased ? 4 : 9;
	const size_t n = (size_t)t->nA * t->nB * ncell;
	DevBuf<unsigned long long> d_cells;
	HIPCHK(c, d_cells.reserve(n, n, nullptr));
	StatsParams p = make_stats(c, kind, *t, s, phased, 0, twk_hip_filters{});
	hipLaunchKernelGGL(k_ld_cells, dim3((t->nB + 255) / 256, t->nA), dim3(256), 0, c->s_compute, p.tv, t->nA, t->nB, c->M, p.diag, phased ? 1 : 0, d_cells);
	hipError_t e = hipGetLastError();
	if (e == hipSuccess) e = hipMemcpyAsync(out, d_cells, n * 8, hipMemcpyDeviceToHost, c->s_compute);
	if (e == hipSuccess) e = hipStreamSynchronize(c->s_compute);
	flush_graveyard(c);
	HIPCHK(c, e);
	return TWK_HIP_OK;
}

int twk_hip_ld_tile(twk_hip_ctx* c, int mode, const twk_hip_tile_desc* t, const twk_hip_filters* f,
                    twk_hip_record* out, uint64_t capacity, uint64_t* n_out, uint64_t* n_pairs) {
	if (!c || !f || !n_out || !valid_mode(mode) || (capacity && !out)) return TWK_HIP_E_INVALID;
	if (!c->raw) return TWK_HIP_E_STATE;
	if (!valid_tile(c, t)) return TWK_HIP_E_INVALID;
	HIPCHK(c, hipSetDevice(c->device));
	CallForms calls;                 // (a call of its own: what a region call gave up does not reach it)
	unsigned long long n = 0;
	int rc = run_tile_sync(c, mode, *t, *f, calls.grant(LaunchWants()), calls, std::max<unsigned long long>(capacity, 1), &n, Deliver());      // (whole, in c->h_recs)
	flush_graveyard(c);
	*n_out = n;
	if (n_pairs) *n_pairs = pairs_in_tile(c, *t);
	if (rc == TWK_HIP_OK && n > capacity) rc = TWK_HIP_E_OVERFLOW;
	if (rc) return rc;
	if (n) std::memcpy(out, c->h_recs, (size_t)n * sizeof(twk_hip_record));
	return TWK_HIP_OK;
}

int twk_hip_ld_all(twk_hip_ctx* c, int mode, const twk_hip_filters* f, uint32_t part, uint32_t n_parts,
                   uint32_t tile_variants, int32_t window, uint32_t l_window, twk_hip_record_sink sink,
                   void* user, uint64_t* n_pairs, uint64_t* n_records) {
	if (!c) return TWK_HIP_E_INVALID;
	return twk_hip_ld_region(c, mode, f, 0, c->M, 0, c->M, 1, part, n_parts, tile_variants, window, l_window,
	                         sink, user, n_pairs, n_records);
}

// ---- one region in one index space ------------------------------------------------------------------------------------------
// (the file order, or - modes MODE_INT_GROUPED / MODE_INT_SORTED_* - the order of a regrouped / sorted plane set; a0 / b0 / nA / nB and
// the tiles are positions in that space).  region_impl asks the planner (ld_plan.h: shard, reach of every row, launches - host-only
// arithmetic, tested without a GPU) and hands the plan to a RegionRun, which executes it: zone passes, the decision between three and
// four products, the launch pipeline with its fallbacks.
namespace {

struct RegionRun {
	twk_hip_ctx* c; int mode; const twk_hip_filters* f;
	const PlanGeom& g; const PlanEnv& env; RegionPlan& plan;
	CallForms& calls;                         // what the call - all its stages - has not yet given up (region_dispatch owns it)
	Deliver to;                               // every launch of the region: the device sink, or the caller's sink (none: records are counted and dropped)
	std::chrono::steady_clock::time_point t_origin = std::chrono::steady_clock::now();
	ColRange col_range;
	// the fine walk's staircases (RegionPlan::stair): the column ranges of the launches in front of a border (LaunchNote::side 1) and behind one (2)
	StairRanges stairs;
	unsigned long long cap_default = 1ull << 24;
	uint64_t tot_pairs = 0, tot_recs = 0;
	std::vector<LaunchWants> wants;           // per launch: the forms its samples allow it (decide_three_by_samples -> ld_form.h: decide_wants)
	uint32_t one_refused = 0;                 // samples in the one-product form that were too rich in candidates (the "timeline" log reports them)
	// the prefix applies to the launches of the two-product walk on rows of more than FUSED_MAX_CHUNKS chunks (ld_form.h decide_form holds the rest)
	bool prefix_eligible() const { return two_walk() && c->opt.prefix != 0 && calls.prefix && c->planes[PS_SORTED_U].W / KC > FUSED_MAX_CHUNKS && !c->planes[PS_SORTED_U].h_suffix.empty(); }
	bool two_walk() const { return mode == MODE_INT_SORTED_U_ALL; }
	// (option two = 2, the test hook: every launch of the walk, whatever the predicate says)
	bool two_eligible(const twk_hip_tile_desc& t) const { return two_walk() && c->opt.two != 0 && (c->opt.two == 2 || t.rowA0 + t.nA <= g.a0 + plan.two_end); }
	bool behind(size_t i) const { return i < plan.notes.size() && plan.notes[i].behind != 0; }
	// ... or a launch the planner gave two products behind the cut, while the call still has them
	bool two_eligible(size_t i) const { return two_eligible(plan.mine[i]) || (behind(i) && calls.two_behind && two_walk() && c->opt.two != 0); }
	const ColRange* cr_of(size_t i) const { return stairs.of(plan, i, cr()); }
	// the pairs launch i decides: its rectangle's, or what lies on its side of the staircase
	uint64_t pairs_of(size_t i) const {
		if (!(i < plan.notes.size() && plan.notes[i].side)) return pairs_in_tile(c, plan.mine[i]);
		const twk_hip_tile_desc& t = plan.mine[i];
		uint64_t n = 0;
		for (uint32_t r = t.rowA0; r < t.rowA0 + t.nA; ++r) { uint32_t lo, hi; plan.launch_cols(g, i, r, lo, hi); n += hi - lo; }
		return n;
	}

	// What launch i of the plan may be: the call's forms, as far as the launch's own samples want them.  A tile redone synchronously is not bound by a
	// sample: it may be whatever the call still allows but two products (redo_grant).
	FormGrant grant_of(size_t i) const {
		return calls.grant(behind(i) ? calls.behind_wants(wants[i]) : wants[i]);
	}
	FormGrant redo_grant() const { return calls.grant(LaunchWants()); }

	RegionRun(twk_hip_ctx* c_, int mode_, const twk_hip_filters* f_, const PlanGeom& g_, const PlanEnv& e_, RegionPlan& p_, CallForms& calls_, twk_hip_record_sink sink_, void* user_)
		: c(c_), mode(mode_), f(f_), g(g_), env(e_), plan(p_), calls(calls_), to{!c_->device_sink, sink_ ? sink_ : discard_records, user_} {}

	void mark(const char* what, size_t i, unsigned long long x = 0) const {       // "timeline" option: where the host's time goes
		if (!c->opt.timeline) return;
		fprintf(stderr, "[timeline] %9.3f ms  %s %zu  %llu\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_origin).count(), what, i, x);
	}
	const ColRange* cr() const { return plan.windowed ? &col_range : nullptr; }

	// Survivor buffer of a launch (worst case every pair of a tile survives: capped, split on overflow) and the reach of the rows on the device.
	int prepare() {
		unsigned long long worst = 0;
		for (const auto& t : plan.mine) worst = std::max<unsigned long long>(worst, (unsigned long long)t.nA * t.nB);
		cap_default = std::min<unsigned long long>(worst ? worst : 1, 1ull << 24);
		if (c->opt.record_cap > 0) cap_default = std::min<unsigned long long>(cap_default, (unsigned long long)c->opt.record_cap);   // test hook: force the overflow / strip path
		if (plan.windowed) { col_range.lo = plan.lo.data(); col_range.hi = plan.hi.data(); col_range.a0 = g.a0; col_range.b0 = g.b0; }
		if (!plan.stair.empty() && plan.stair.size() == g.nA) {      // (rows of no staircase are in no launch that has a side)
			HIPCHK(c, c->d_stair.reserve(g.nA, g.nA, nullptr));
			HIPCHK(c, hipMemcpy(c->d_stair, plan.stair.data(), (size_t)g.nA * 4, hipMemcpyHostToDevice));
			stairs.set(plan, g, c->d_stair);
		}
		if (env.screen && g.nA) {
			HIPCHK(c, c->d_col_hi.reserve(g.nA, g.nA, nullptr));
			HIPCHK(c, hipMemcpy(c->d_col_hi, plan.hi.data(), (size_t)g.nA * 4, hipMemcpyHostToDevice));
			col_range.d_hi = c->d_col_hi; col_range.n_hi = g.nA;
		}
		return TWK_HIP_OK;
	}

	// The list zone of an allele-count-sorted set (long rows only): its pairs are intersected as carrier lists, block of rows after
	// block of rows, and the rows with the shortest lists probe every column behind them, before the tiles that are left are contracted.
	int run_zone_passes() {
		if (!(env.screen && g.a0 == 0 && g.b0 == 0)) return TWK_HIP_OK;
		const bool unphased = env.screen == 2;
		const PlaneSet& ps = c->planes[unphased ? PS_SORTED_U : PS_SORTED_P];
		const uint32_t zone = std::min(ps.n_list, g.nA), r0 = plan.r0, r1 = plan.r1;
		if (!(zone >= 2 && ps.lists)) return TWK_HIP_OK;
		col_range.list_zone = zone;
		// rows whose list is short enough to probe with (the first n_probe of the zone) take every column behind them as probes,
		// the zone's own included ("probe_zone": a probe walks one list and tests bits of the partner's row, a merge walks two
		// lists in step - 0.28 against 1.05 ns a pair on the unphased zone of the 1 M x 50 k cohort run); the merges are left
		// with the zone's last rows
		const uint32_t pz_first = (c->opt.probe && c->opt.probe_zone) ? std::min(ps.n_probe, zone) : 0;
		const uint32_t lr0 = std::min(std::max(r0, pz_first), zone), lr1 = std::min(r1, zone);
		uint32_t rows_per = (uint32_t)std::max<uint64_t>(64, std::min<uint64_t>(32768, (1ull << 25) / zone));
		unsigned long long cap_list = cap_default;
		for (uint32_t row = lr0; row < lr1;) {
			const uint32_t nr = std::min(rows_per, lr1 - row);
			unsigned long long nrec = 0;
			const int rc = run_list_block(c, *f, unphased, row, nr, zone, g.window, g.l_window, col_range, cap_list, &nrec, to);
			if (rc == TWK_HIP_E_OVERFLOW && nr > 1) { rows_per = std::max<uint32_t>(1, nr / 2); continue; }      // more survivors than the buffer holds: fewer rows
			if (rc == TWK_HIP_E_OVERFLOW && cap_list < zone) { cap_list = zone; continue; }                      // one row: it cannot have more than `zone` partners
			if (rc) return rc;
			tot_recs += nrec;
			row += nr;
		}
		mark("carrier-list pass done, zone", zone, tot_recs);
		// ... and the zone's rows against the columns beyond the zone: probes of the row variant's carriers into the column
		// variant's row (K1's asymmetric path, ld_engine.cpp:230-242; measured to win for every list the zone keeps,
		// ld_list.hip.h), so that no tile row inside the zone is contracted at all.
		const uint32_t pzone = c->opt.probe ? std::min(ps.n_probe, zone) : 0;
		const bool zone_cols = c->opt.probe_zone != 0;             // the probes' columns start behind the row, not behind the zone
		if (!(pzone && (zone < g.nB || zone_cols))) return TWK_HIP_OK;
		col_range.probe_zone = pzone;
		unsigned long long cap_probe = cap_default;
		uint32_t rows_cap = 32768;                                   // halved when a block's survivors outgrow the buffer
		const uint32_t pr0 = std::min(r0, pzone), pr1 = std::min(r1, pzone);
		// the columns a block's rows reach (the band limit never decreases along the rows)
		auto reach = [&](uint32_t last_row) -> uint32_t { return (uint32_t)std::min<uint64_t>(g.nB, col_range.hi ? (uint64_t)col_range.b0 + col_range.hi[last_row - col_range.a0] : g.nB); };
		for (uint32_t row = pr0; row < pr1;) {
			uint32_t nr = std::min<uint32_t>(pr1 - row, rows_cap);
			const uint32_t first = zone_cols ? row + 1 : zone;       // first column of the block (a row's own start at row + 1: the kernel's j > i)
			while (nr > 256 && (uint64_t)nr * (reach(row + nr - 1) > first ? reach(row + nr - 1) - first : 0) > (1ull << 25)) nr = std::max<uint32_t>(256, nr / 2);
			const uint32_t lim = reach(row + nr - 1);
			if (lim <= first) { row += nr; continue; }
			unsigned long long nrec = 0;
			const int rc = run_probe_block(c, *f, unphased, row, nr, zone, first, lim - first, g.window, g.l_window, col_range, cap_probe, &nrec, to);
			if (rc == TWK_HIP_E_OVERFLOW && nr > 1) { rows_cap = std::max<uint32_t>(1, nr / 2); continue; }
			if (rc == TWK_HIP_E_OVERFLOW && cap_probe < (unsigned long long)(lim - first)) { cap_probe = lim - first; continue; }
			if (rc) return rc;
			tot_recs += nrec;
			row += nr;
		}
		mark("probe pass done, zone", pzone, tot_recs);
		return TWK_HIP_OK;
	}

	// A density sample is not a launch of the run: what it leaves in the timing and in the launch log is taken back when it is through.
	struct SampleScope {
		twk_hip_ctx* c; const twk_hip_timing keep_timing; const size_t keep_ring; const uint64_t keep_seen;
		explicit SampleScope(twk_hip_ctx* c_) : c(c_), keep_timing(c_->timing), keep_ring(c_->launch_ring.size()), keep_seen(c_->launches_seen) {}
		~SampleScope() {
			c->timing = keep_timing;
			if (c->launch_ring.size() > keep_ring && c->launches_seen == keep_seen + 1 && keep_seen < LAUNCH_RING) c->launch_ring.pop_back();
			c->launches_seen = keep_seen;
		}
	};
	// The sample of launch `pick` in the form `as`: its sub-tile (ld_plan.h: sample_subtile) through the same kernels on the spare slot, its records dropped.
	SampleOutcome run_sample(size_t pick, const LaunchWants& as) {
		uint64_t sided_pairs = 0;
		const twk_hip_tile_desc st = sample_subtile_of(plan, g, pick, &sided_pairs);      // (a launch on one side of a staircase: where it has pairs, and those alone counted)
		SampleOutcome o;
		o.pairs = std::max<uint64_t>(pick < plan.notes.size() && plan.notes[pick].side ? sided_pairs : pairs_in_tile(c, st), 1);
		SampleScope not_a_launch(c);
		Slot& ss = c->slot[SYNC_SLOT];
		unsigned long long nrec = 0;
		o.rc = enqueue_tile(c, mode, st, *f, calls.sample_grant(as), ss, std::max<unsigned long long>((unsigned long long)st.nA * st.nB, 1), cr_of(pick));
		if (o.rc == TWK_HIP_OK) o.rc = finish_tile(c, ss, st, &nrec, Deliver{true, discard_records, nullptr});
		o.cand = ss.h_n_out[2];
		return o;
	}
	// What every launch of the plan may be, decided by samples taken before the pipeline starts: the facts of this region for the ladder of
	// ld_form.h (decide_wants), which says which launch is sampled in which form and what follows from each outcome.
	int decide_three_by_samples() {
		const std::vector<twk_hip_tile_desc>& mine = plan.mine;
		LadderFacts x;
		x.opt_two = c->opt.two; x.opt_three = c->opt.three; x.opt_prefix = c->opt.prefix; x.opt_one = c->opt.one;
		x.one_ok = env.one && env.carrier && c->opt.one != 0 && calls.one;
		x.prefix_ok = prefix_eligible();
		x.three_possible = !mine.empty() && c->opt.three == 1 && launch_form(c, plan_for(c, mode), *f, redo_grant()).three;
		x.fused = env.fused; x.carrier = env.carrier;      // (region_impl holds carrier rows for every row in front of the cut)
		for (size_t i = 0; i < mine.size(); ++i) x.eligible_interleaved = x.eligible_interleaved || behind(i);
		const int rc = decide_wants(mine.size(), x, [&](size_t i) { return two_eligible(i); }, [&](size_t i) { return mine[i].one != 0; },
		                            [&](size_t pick, const LaunchWants& as) { return run_sample(pick, as); },
		                            [&](const char* what, size_t i, unsigned long long n_cand) { mark(what, i, n_cand); }, wants, one_refused);
		// (a two-product launch behind the cut whose sample refused the form: none of them takes it)
		if (rc == TWK_HIP_OK && c->opt.two == 1 && calls.two_behind && behind_refused(wants, [&](size_t i) { return behind(i); })) { mark("two-product sample behind the cut refused: launches behind it", mine.size()); calls.two_behind = false; }
		return rc;
	}

	// What every tile ends with once its launch, or the ladder below it (run_tile_sync), is through with rc: more survivors than the buffer holds -> the
	// tile again in row strips that cannot overflow; its records into the total.
	int strips_if_overflowed(int rc, const twk_hip_tile_desc& t, unsigned long long nrec, const ColRange* range) {
		if (rc == TWK_HIP_E_OVERFLOW) {
			uint64_t nr = 0;
			rc = redo_tile_in_strips(c, mode, t, *f, redo_grant(), calls, cap_default, to, &nr, range);
			nrec = nr;
		}
		if (rc == TWK_HIP_OK) tot_recs += nrec;
		return rc;
	}
	// One matrix-sized tile, synchronously, with its fallbacks.
	int run_tile_with_fallbacks(const twk_hip_tile_desc& t) {
		unsigned long long nrec = 0;
		const int rc = run_tile_sync(c, mode, t, *f, redo_grant(), calls, cap_default, &nrec, to, cr());
		return strips_if_overflowed(rc, t, nrec, cr());
	}
	// a band launch that cannot run (or has overflowed) as the matrix-sized tiles of its rows
	int run_band_as_matrix_tiles(const BandLaunch& b) {
		std::vector<twk_hip_tile_desc> sub;
		plan_matrix_tiles(env, g, plan, b.xa, b.xb, sub);
		for (const auto& t : sub) { const int r = run_tile_with_fallbacks(t); if (r) return r; }
		return TWK_HIP_OK;
	}

	// The second half of band launch i (its pair math: once the count kernel's candidate count is known).
	int band_math(size_t i, const std::vector<char>& skipped) {
		if (i < plan.bands.size() && !skipped[i]) {
			mark("math: wait for count of launch", i);
			const int r = enqueue_band_math(c, c->slot[i % PIPE_SLOTS]);
			mark("math enqueued for launch", i, c->slot[i % PIPE_SLOTS].h_n_out[2]);
			return r;
		}
		return TWK_HIP_OK;
	}

	// Launch `done` has been waited for: deliver its records, or run its fallbacks.
	int finish_launch(size_t done, const std::vector<char>& skipped) {
		const std::vector<twk_hip_tile_desc>& mine = plan.mine;
		Slot& s = c->slot[done % PIPE_SLOTS];
		unsigned long long nrec = 0;
		const BandLaunch* b = done < plan.bands.size() ? &plan.bands[done] : nullptr;
		mark("finish: wait for launch", done);
		int rc;
		if (b) {
			rc = skipped[done] ? TWK_HIP_E_OVERFLOW : finish_tile(c, s, mine[done], &nrec, to);
			// (a band launch's list is the planner's guess for a whole band: its overflow ends no form - the matrix-sized tiles that redo it try theirs)
			if (!skipped[done]) calls.gave_up(s.l.form, s.l.given, false, s.l.too_rich);
			mark("finished (records delivered) launch", done, nrec);
			if (rc == TWK_HIP_E_OVERFLOW) rc = run_band_as_matrix_tiles(*b);      // candidates or survivors beyond the launch's buffers
			else if (rc == TWK_HIP_OK) tot_recs += nrec;
			return rc;
		}
		rc = finish_tile(c, s, mine[done], &nrec, to);
		// (a two-product launch behind the cut whose list overflowed ends those launches, and takes no form from the call: the ladder below is the same)
		const bool behind_overflow = behind(done) && s.l.form.two && s.l.cand_overflow;
		if (!behind_overflow) calls.gave_up(s.l.form, s.l.given, s.l.cand_overflow, s.l.too_rich);      // (the launches not yet enqueued see it; those in flight keep their grant)
		const FormGrant down = behind_overflow ? calls.behind_overflowed(s.l.given) : step_down(s.l.form, s.l.given);      // (ld_form.h: ... redone with three products over whole rows)
		if (rc == TWK_HIP_E_OVERFLOW && s.l.cand_overflow)                        // the candidate list overflowed: this tile again, one step down the ladder
			rc = run_tile_sync(c, mode, mine[done], *f, down, calls, cap_default, &nrec, to, cr_of(done));
		rc = strips_if_overflowed(rc, mine[done], nrec, cr_of(done));
		if (rc == TWK_HIP_OK) mark("finished (records delivered) launch", done, tot_recs);
		return rc;
	}

	// Software pipeline over the launches of this shard, PIPE_SLOTS deep.  The pair math of a band launch follows once its count kernel is
	// done - with the next launch's count kernel already queued behind it, so that the device has work while the host waits for the
	// candidate count.
	int run_pipeline() {
		const std::vector<twk_hip_tile_desc>& mine = plan.mine;
		const size_t n = mine.size();
		std::vector<char> skipped(n, 0);
		size_t issued = 0, done = 0, math_issued = 0;      // band launches [0, math_issued) have had the second half of their work enqueued
		int rc = TWK_HIP_OK;
		auto issue_next = [&]() -> int {
			const BandLaunch* b = issued < plan.bands.size() ? &plan.bands[issued] : nullptr;
			if (b && !calls.fused) skipped[issued] = 1;                 // an earlier launch gave the fused form up: this one goes the matrix way when its turn comes
			else {
				mark("enqueue launch", issued);
				const int r = enqueue_tile(c, mode, mine[issued], *f, grant_of(issued), c->slot[issued % PIPE_SLOTS], b ? 1 : cap_default, cr_of(issued), b ? b->list_words : 0);
				if (r) return r;
				mark("enqueued launch", issued);
			}
			++issued;
			return TWK_HIP_OK;
		};
		while (done < n) {
			while (issued < n && issued < done + PIPE_SLOTS) {
				rc = issue_next(); if (rc) return rc;
				while (math_issued + 1 < issued) { rc = band_math(math_issued, skipped); if (rc) return rc; ++math_issued; }
			}
			while (math_issued <= done && math_issued < issued) { rc = band_math(math_issued, skipped); if (rc) return rc; ++math_issued; }
			rc = finish_launch(done, skipped);
			if (rc) return rc;
			tot_pairs += pairs_of(done);
			++done;
			if (c->progress_cb && !c->progress_muted) c->progress_cb(c->progress_user, tot_pairs, (uint32_t)done, (uint32_t)n);
		}
		return TWK_HIP_OK;
	}
};

// What the planner needs to know of the context for this mode.
int plan_env_for(twk_hip_ctx* c, int mode, const twk_hip_filters* f, const CallForms& calls, PlanEnv& env) {
	env = PlanEnv();
	if (mode == MODE_INT_GROUPED || mode == MODE_INT_SORTED_P || mode == MODE_INT_SORTED_U || mode == MODE_INT_SORTED_U_ALL) {
		const int set = mode == MODE_INT_GROUPED ? PS_GROUPED : mode == MODE_INT_SORTED_P ? PS_SORTED_P : PS_SORTED_U;
		const int rc = mode == MODE_INT_SORTED_U_ALL ? ensure_planes(c, set) : ensure_lists(c, set); if (rc) return rc;      // (the two-product walk keeps no zones)
		env.ids = c->planes[set].h_ids.data();
	}
	if (mode == MODE_INT_SORTED_U_ALL && c->opt.two != 0) {      // the two-product walk: the planner cuts the triangle where the rows' hom-alt carriers become too many
		PlaneSet& ps = c->planes[PS_SORTED_U];
		if (ps.h_het.size() != c->M) {
			std::vector<uint32_t> pop((size_t)2 * c->M);
			HIPCHK(c, hipMemcpy(pop.data(), ps.rowpop, pop.size() * 4, hipMemcpyDeviceToHost));
			ps.h_het.resize(c->M); ps.h_hom.resize(c->M);
			for (uint32_t v = 0; v < c->M; ++v) { ps.h_het[v] = pop[2 * (size_t)v]; ps.h_hom[v] = pop[2 * (size_t)v + 1]; }
		}
		env.het = ps.h_het.data(); env.hom = ps.h_hom.data();
		// the carrier plane as the row operand: asked for here, granted by region_impl once the rows in front of the cut it gives are there
		env.carrier = c->opt.carrier != 0 && ps.W / KC > FUSED_MAX_CHUNKS;
		// ... and one product a pair in front of a row block's one_end: likewise, once carrier rows for those launches' columns are there too
		env.one = env.carrier && c->opt.one != 0 && calls.one && f->minR2 > 1e-6 && f->minR2 <= 1.0; env.one_rows = (uint32_t)c->opt.one_rows;
		env.fine = walk_fine_applies(c, ps.W / KC);
		// the prefix contraction: the rows' suffix margins, the first time a call may take the form (no room for the table: the call takes no stops)
		if (c->opt.prefix != 0 && calls.prefix && f->minR2 > 1e-6 && f->minR2 <= 1.0 && ps.W / KC > FUSED_MAX_CHUNKS) {
			const int rc = or_go_without(c, ensure_suffix(c, PS_SORTED_U), [&] { ps.suffix = DevBuf<uint32_t>(); ps.h_suffix.clear(); });
			if (rc) return rc;
		}
	}
	// r2 screen (TWK_HIP_OPT_R2_SCREEN): the region is a triangle over the leading, missing-free part of an allele-count-sorted set
	env.screen = (mode == MODE_INT_SORTED_P) ? 1 : (mode == MODE_INT_SORTED_U) ? 2 : 0;
	if (env.screen) { const int rc = ensure_popcounts(c); if (rc) return rc; env.popc = c->h_popc.data(); }
	const TilePlan pl = plan_for(c, mode);
	env.n_samples = c->N; env.Pmax = pl.Pmax; env.resident_blocks = c->resident_blocks; env.minR2 = f->minR2; env.phased_math = pl.phased1;
	env.meta = c->h_meta.data();
	env.fused = fused_form_applies(c, mode, *f, calls);
	if (env.fused) env.nchunks = c->planes[pl.set1].W / KC;
	env.band_launch = c->opt.band_launch != 0; env.band_reverse = c->opt.band_reverse != 0;
	env.band_work_log2 = c->opt.band_work_log2; env.band_max_launches = c->opt.band_max_launches; env.band_list_entries = c->opt.band_list_entries;
	return TWK_HIP_OK;
}

}  // namespace

// The arguments of twk_hip_ld_region, as they travel inside the library: region_dispatch edits a copy per stage.
struct RegionArgs {
	int mode; const twk_hip_filters* f; uint32_t a0, nA, b0, nB; int32_t triangle; uint32_t part, n_parts, tile_variants; int32_t window; uint32_t l_window;
	twk_hip_record_sink sink; void* user; uint64_t* n_pairs; uint64_t* n_records;
	RegionArgs stage(int mode_, uint32_t a0_, uint32_t nA_, uint32_t b0_, uint32_t nB_, int32_t triangle_, uint64_t* n_pairs_, uint64_t* n_records_) const {
		RegionArgs r = *this;
		r.mode = mode_; r.a0 = a0_; r.nA = nA_; r.b0 = b0_; r.nB = nB_; r.triangle = triangle_; r.n_pairs = n_pairs_; r.n_records = n_records_;
		return r;
	}
};

static int region_impl(twk_hip_ctx* c, const RegionArgs& a, CallForms& calls) {
	const PlanGeom g{a.a0, a.nA, a.b0, a.nB, a.triangle, a.part, a.n_parts, a.tile_variants, a.window, a.l_window};
	PlanEnv env;
	int rc = plan_env_for(c, a.mode, a.f, calls, env); if (rc) return rc;
	RegionPlan plan;
	plan_region(env, g, plan);
	if (env.carrier) {
		// The carrier form's cut lies behind the H form's: carrier rows for every row variant of this shard's two-product launches (option two = 2: every
		// launch of the walk), built now if they are not there.  No room for them: the plan of the H form, as before.
		PlaneSet& ps = c->planes[PS_SORTED_U];
		auto drop_carrier = [&] { ps.carrier_buf.reset(); ps.carrier_rows = nullptr; ps.carrier_n = 0; };
		auto have_carrier = [&](uint32_t n) { return ps.carrier_rows && ps.carrier_n >= n; };
		// The rows are built once, for the largest need of this plan: the column variants of its one-product launches, or - the fine walk's two-product
		// launches behind the cut - the row variants up to two_last.  No room for the latter: those blocks stay three-product.
		{
			uint32_t largest = plan.two_last > plan.two_end && c->opt.two != 2 ? g.a0 + plan.two_last : 0;
			const uint32_t behind_need = largest;
			for (const auto& t : plan.mine) if (t.one) largest = std::max(largest, t.rowB0 + t.nB);
			if (behind_need && !have_carrier(largest)) { rc = or_go_without(c, ensure_carrier(c, PS_SORTED_U, largest), drop_carrier); if (rc) return rc; }
			if (behind_need && !have_carrier(behind_need)) { rc = or_go_without(c, ensure_carrier(c, PS_SORTED_U, behind_need), drop_carrier); if (rc) return rc; }
			if (behind_need && !have_carrier(behind_need)) { env.stair_behind = false; plan_region(env, g, plan); }
		}
		const uint32_t walk_end = c->opt.two == 2 ? g.nA : std::max(plan.two_end, plan.two_last), need = plan.r0 < std::min(walk_end, plan.r1) ? g.a0 + std::min(walk_end, plan.r1) : 0;
		// ... and for every column variant of this shard's one-product launches (at r2 >= 0.1 on a flat frequency law: nearly every variant of the set, one
		// more plane row each).  No room for those: the plan without one-product launches, and the rows in front of the cut as before.
		uint32_t need_one = 0;
		for (const auto& t : plan.mine) if (t.one) need_one = std::max(need_one, t.rowB0 + t.nB);
		if (need && need_one > need && !(ps.carrier_rows && ps.carrier_n >= need_one)) {
			rc = or_go_without(c, ensure_carrier(c, PS_SORTED_U, need_one), drop_carrier); if (rc) return rc;
		}
		if (env.one && (!need || (need_one > need && !(ps.carrier_rows && ps.carrier_n >= need_one)))) {
			env.one = false;
			plan_region(env, g, plan);
		}
		if (need) {
			rc = or_go_without(c, ensure_carrier(c, PS_SORTED_U, need), drop_carrier); if (rc) return rc;
		}
		if (!carrier_operand(c->opt.carrier, ps.W / KC, ps.carrier_rows ? ps.carrier_n : 0, need)) {
			env.carrier = env.one = false;
			plan_region(env, g, plan);
		}
	}
	RegionRun run(c, a.mode, a.f, g, env, plan, calls, a.sink, a.user);
	run.mark("region: mode", (size_t)a.mode, a.nA);
	rc = run.prepare(); if (rc) return rc;
	rc = run.run_zone_passes(); if (rc) return rc;
	run.mark("tiles listed", plan.mine.size());
	rc = run.decide_three_by_samples(); if (rc) return rc;
	if (env.one) run.mark("one-product samples refused", run.one_refused);
	rc = run.run_pipeline(); if (rc) return rc;
	if (plan.windowed) run.tot_pairs = plan.pairs;      // screen: every pair of the band is decided; window: the pairs inside it, the ones the math evaluates
	if (a.n_pairs) *a.n_pairs = run.tot_pairs;
	if (a.n_records) *a.n_records = run.tot_recs;
	return TWK_HIP_OK;
}

static int region_dispatch(twk_hip_ctx* c, const RegionArgs& a) {
	const int mode = a.mode; const twk_hip_filters* f = a.f;
	if (!c || !f || !valid_mode(mode) || a.n_parts == 0 || a.part >= a.n_parts) return TWK_HIP_E_INVALID;
	if (!c->raw) return TWK_HIP_E_STATE;
	if (a.nA == 0 || a.nB == 0 || (uint64_t)a.a0 + a.nA > c->M || (uint64_t)a.b0 + a.nB > c->M) return TWK_HIP_E_INVALID;
	if (a.triangle && (a.a0 != a.b0 || a.nB < a.nA)) return TWK_HIP_E_INVALID;
	HIPCHK(c, hipSetDevice(c->device));
	CallForms calls;                 // of this call, all its stages: a later stage sees what an earlier one gave up
	calls.fused = calls.three = calls.two = c->reduce.kind == Reduce::none;      // a score, a prune, a clump, a matrix, a decay or an aggregate looks at every pair: no screen in front of the count matrix
	const bool whole = a.triangle && a.a0 == 0 && a.nA == c->M && a.nB == c->M;
	// TWK_HIP_OPT_R2_SCREEN: whole-triangle runs with an r2 cut-off worth the name, outside window mode (which
	// already prunes by position, in an order the allele-count sort would destroy)
	// ... or, at any cut-off above zero, rows long enough to keep carrier lists: the band is then (nearly) everything, but the
	// allele-count order still puts the rare variants in a zone whose pairs are list merges and probes instead of contractions
	const bool lists_pay = f->minR2 > 0 && c->opt.lists != 0 && (c->Wp / 128 >= 32 || c->opt.lists == 2);
	const bool screen = (a.window & TWK_HIP_OPT_R2_SCREEN) && whole && !(a.window & TWK_HIP_OPT_WINDOW) && (f->minR2 >= 1e-3 || lists_pay) && c->M >= 2;
	if (screen && !c->any_missing && (mode == TWK_HIP_MODE_PHASED || mode == TWK_HIP_MODE_AUTO || mode == TWK_HIP_MODE_UNPHASED)) {
		// Below the cut-off that makes a band worth having the sorted order is only taken for its carrier lists: when the set turns out to
		// keep none (too few rare variants), the sorted copy of the planes is dropped again and the run goes the file-order way (it used to
		// run the plain matrix path in sorted order with a band that covers everything: twice the plane memory for nothing).
		const int sset = mode == TWK_HIP_MODE_UNPHASED ? PS_SORTED_U : PS_SORTED_P;
		bool keep_sorted = true;
		bool& known_useless = c->sorted_keeps_no_lists[sset == PS_SORTED_U ? 1 : 0];      // (every region call of a multi-step run used to build and drop the set again)
		if (f->minR2 < 1e-3 && known_useless) keep_sorted = false;
		else if (f->minR2 < 1e-3) {
			const int rc = ensure_lists(c, sset); if (rc) return rc;
			if (c->planes[sset].n_list < 2) {
				keep_sorted = false; known_useless = true;
				HIPCHK(c, hipDeviceSynchronize());
				c->planes[sset] = PlaneSet();
			}
		}
		if (keep_sorted) return region_impl(c, a.stage(mode == TWK_HIP_MODE_UNPHASED ? MODE_INT_SORTED_U : MODE_INT_SORTED_P, 0, c->M, 0, c->M, 1, a.n_pairs, a.n_records), calls);
	}
	// The two-product walk: an unscreened UnphasedMath call over the whole triangle walks the allele-count-sorted set as well - every
	// pair is still contracted (no band, no list or probe zone), but the launches over the rows with few hom-alt carriers take two products a pair.
	// Only where the tile edge is the engine's (an explicit one pins the launch geometry in file order) and option three = 1 (2: three products
	// whatever); rows short enough to fuse, masked planes and a window keep the file order.  part / n_parts shard the sorted triangle.  A second
	// plane set that cannot be allocated: the call runs in file order.
	if (mode == TWK_HIP_MODE_UNPHASED && whole && !(a.window & (TWK_HIP_OPT_WINDOW | TWK_HIP_OPT_R2_SCREEN)) && !c->any_missing && c->reduce.kind == Reduce::none &&
	    a.tile_variants == 0 && c->opt.two != 0 && c->opt.three == 1 && f->minR2 > 1e-6 && f->minR2 <= 1.0 && c->M >= 2 &&
	    (c->opt.fused == 0 || (c->opt.fused == 1 && c->Wu / KC > FUSED_MAX_CHUNKS))) {
		const int prc = ensure_planes(c, PS_SORTED_U);
		if (prc == TWK_HIP_OK) return region_impl(c, a.stage(MODE_INT_SORTED_U_ALL, 0, c->M, 0, c->M, 1, a.n_pairs, a.n_records), calls);
		if (prc != TWK_HIP_E_NOMEM) return prc;
		(void)hipGetLastError(); c->err[0] = 0;
	}
	if (!(mode == TWK_HIP_MODE_AUTO && c->any_missing && whole)) return region_impl(c, a, calls);
	// Default mode over the whole triangle with missing genotypes somewhere: every pair goes through
	// the cheap one-plane phased products, and only the pairs that involve a variant with missing
	// data (the leading group G of the regrouped set) through the 3-plane unphased ones:
	// G x G (triangle) and G x rest (rectangle).  Each stage is sharded on its own.
	int rc = ensure_planes(c, PS_GROUPED); if (rc) return rc;
	const uint32_t nG = c->planes[PS_GROUPED].n_front;
	uint64_t pairs = 0, recs = 0, p2 = 0, r2 = 0;
	if (screen) {
		// the pairs without missing data: a screened triangle over the missing-free head of the sorted set;
		// the stages below then cover every pair that involves a variant with missing data
		rc = ensure_planes(c, PS_SORTED_P); if (rc) return rc;
		const uint32_t nC = c->planes[PS_SORTED_P].n_front;
		if (nC >= 2) rc = region_impl(c, a.stage(MODE_INT_SORTED_P, 0, nC, 0, nC, 1, &pairs, &recs), calls);
	} else
		rc = region_impl(c, a.stage(MODE_INT_AUTO_CLEAN, 0, c->M, 0, c->M, 1, &pairs, &recs), calls);
	struct Mute { twk_hip_ctx* c; ~Mute() { c->progress_muted = false; } } mute{c};
	c->progress_muted = true;
	if (rc == TWK_HIP_OK && nG >= 2) {
		rc = region_impl(c, a.stage(MODE_INT_GROUPED, 0, nG, 0, nG, 1, &p2, &r2), calls);
		recs += r2;
		if (screen) pairs += p2;               // the screened stage only counted the pairs without missing data
	}
	if (rc == TWK_HIP_OK && nG >= 1 && nG < c->M) {
		rc = region_impl(c, a.stage(MODE_INT_GROUPED, 0, nG, nG, c->M - nG, 0, &p2, &r2), calls);
		recs += r2;
		if (screen) pairs += p2;
	}
	if (a.n_pairs) *a.n_pairs = pairs;          // every pair of the shard is evaluated exactly once
	if (a.n_records) *a.n_records = recs;
	return rc;
}

int twk_hip_ld_region(twk_hip_ctx* c, int mode, const twk_hip_filters* f, uint32_t a0, uint32_t nA,
                      uint32_t b0, uint32_t nB, int32_t triangle, uint32_t part, uint32_t n_parts,
                      uint32_t tile_variants, int32_t window, uint32_t l_window, twk_hip_record_sink sink,
                      void* user, uint64_t* n_pairs, uint64_t* n_records) {
	if (c) delivery_begin(c, sink);
	int rc = region_dispatch(c, RegionArgs{mode, f, a0, nA, b0, nB, triangle, part, n_parts, tile_variants, window, l_window, sink, user, n_pairs, n_records});
	if (c) {                                // every record staged so far reaches the sink before the call returns, whatever the call's own result
		(void)hipSetDevice(c->device);
		const int drc = delivery_end(c);
		if (rc == TWK_HIP_OK && drc) rc = drc;            // (its text is in c->err: delivery_end)
	}
	if (c) flush_graveyard(c);               // buffers outgrown during the call: nothing is in flight any more
	return rc;
}

extern "C++" {      // (member templates)
namespace {
// The device memory of one call (CallMemory: a request an allocation, all released with the owner): hold() gives `items` of T, or the call
// has failed with `what` - a format of `lead` (a count, or a name), the bytes wanted and the runtime's reason - as TWK_HIP_E_NOMEM when
// the device cannot give it.  From the first failure on hold() gives null and asks for nothing, so an entry point holds what it needs
// line by line and looks at `failed` once, before it uses any of it.
struct HeldMemory : CallMemory<HipMemOps> {
	twk_hip_ctx* c; int failed = TWK_HIP_OK;
	explicit HeldMemory(twk_hip_ctx* c_) : c(c_) {}
	// again: what an earlier hold gave, now needed with room for `items` (CallMemory::retake; null: a buffer of its own)
	template <class T, class Lead>
	T* hold(size_t items, const char* what, Lead lead, T* again = nullptr) {
		if (failed) return nullptr;
		hipError_t e = hipSuccess;
		T* const p = retake(again, items, &e);
		if (e == hipSuccess) return p;
		(void)hipGetLastError();
		snprintf(c->err, sizeof(c->err), what, lead, items * sizeof(T), hipGetErrorString(e));
		failed = e == hipErrorOutOfMemory ? TWK_HIP_E_NOMEM : TWK_HIP_E_DEVICE;
		return nullptr;
	}
};

// "Preset n floats to this bit pattern": any pattern, NaNs included - never through a float register.
hipError_t preset_floats(float* p, float fill, size_t n, hipStream_t s) {
	uint32_t fill_bits; memcpy(&fill_bits, &fill, sizeof(fill_bits));
	return hipMemsetD32Async((hipDeviceptr_t)p, (int)fill_bits, n, s);
}

// One call of twk_hip_ld_score, _prune, _clump, _matrix, _decay or _aggregate: the region call's planner and launch pipeline with the kind's epilogue in place of
// math, Fisher, sort and delivery (launch_reduce).  Constructed at the top of the entry point, which returns `bad` if the shared checks found
// something; whichever way the entry point then leaves, the destructor puts the context back: no kind, no map, nothing in flight, the
// graveyard flushed - and the memory that lived for the call, a member, is released behind it.
struct ReduceCall {
	twk_hip_ctx* c; const twk_hip_filters* f;
	const Reduce kind;             // the epilogue the call's launches take ...
	CallReport* const report;      // ... and the entry point's report the call writes (its own dummy: the entry point has no twk_hip_*_last)
	CallReport unreported;
	int bad;
	// What lives as long as the call - the bitmap, the n x n matrix, the aggregate's cells, the band and its map, the top-k lists, a later
	// step's arrays: gigabytes that a record run behind this call may need, so they go back when the call ends, whichever way.  Members:
	// released behind the destructor's body, which waits for the device.
	HeldMemory mem;
	StageMarks marks;
	// own_args_ok: the entry point's own pointers and numbers; [a0, a0 + n): the rows of the call (a slice call's variants)
	ReduceCall(twk_hip_ctx* c_, Reduce kind_, CallReport LastCalls::* which, const twk_hip_filters* f_, bool own_args_ok, int mode, uint32_t a0, uint32_t n)
		: c(c_), f(f_), kind(kind_), report(c_ && which ? &(c_->last.*which) : &unreported), bad(check(own_args_ok, mode, a0, n)), mem(c_) {}
	ReduceCall(const ReduceCall&) = delete;
	int check(bool own_args_ok, int mode, uint32_t a0, uint32_t n) {
		if (!c || !f || !own_args_ok || !(f->minP >= 1.0)) return TWK_HIP_E_INVALID;
		if (!c->raw) return TWK_HIP_E_STATE;
		if (!valid_mode(mode) || n == 0 || (uint64_t)a0 + n > c->M) return TWK_HIP_E_INVALID;
		HIPCHK(c, hipSetDevice(c->device));
		return TWK_HIP_OK;
	}
	~ReduceCall() {
		if (bad) return;
		c->reduce = ReduceState();
		(void)hipDeviceSynchronize();
		flush_graveyard(c);                 // buffers outgrown during the call: nothing is in flight any more
	}
	// Memory of the call (HeldMemory::hold): null once a hold has failed - mem.failed is the call's result then.
	template <class T, class Lead>
	T* hold(size_t items, const char* what, Lead lead) { return mem.hold<T>(items, what, lead); }
	// The call's three counters, zeroed.
	int zero_counts() {
		HIPCHK(c, c->d_counts.reserve(3, 3, nullptr));
		HIPCHK(c, hipMemsetAsync(c->d_counts, 0, 3 * sizeof(unsigned long long), c->s_compute));
		return TWK_HIP_OK;
	}
	// prune, clump: the adjacency bitmap of the slice [a0, a0 + n), n * ceil(n / 64) words whatever the window (ld_prune.hip.h), held, cleared
	// and armed.  Where it lies is what the launches were told: c->reduce.map.bits.adj, for the rest of the call.
	int bitmap(uint32_t a0, uint32_t n, const char* what) {
		const uint32_t stride = (n + 63) / 64;
		const size_t words = (size_t)n * stride;
		unsigned long long* const adj = hold<unsigned long long>(words, what, n);
		if (mem.failed) return mem.failed;
		const int rc = zero_counts(); if (rc) return rc;
		HIPCHK(c, hipMemsetAsync(adj, 0, words * sizeof(unsigned long long), c->s_compute));
		c->reduce.map.bits = PruneMap{adj, c->d_counts, a0, n, stride};
		arm(words * sizeof(unsigned long long));
		return TWK_HIP_OK;
	}
	// From here on the call's launches take the kind's epilogue, and its report is this call's.  bytes: what twk_hip_*_last reports of it.
	void arm(uint64_t bytes) { *report = CallReport(); report->bytes = bytes; c->reduce.work = 0; c->reduce.kind = kind; }
	// The region call's geometry.  (The r2 band and the carrier-list zones exist to avoid looking at pairs: never for a reduce call.)
	int dispatch(int mode, uint32_t a0, uint32_t nA, uint32_t b0, uint32_t nB, int32_t triangle, uint32_t part, uint32_t n_parts, uint32_t tile_variants,
	             int32_t window, uint32_t l_window, uint64_t* n_pairs) {
		window &= ~(int32_t)TWK_HIP_OPT_R2_SCREEN;
		return region_dispatch(c, RegionArgs{mode, f, a0, nA, b0, nB, triangle, part, n_parts, tile_variants, window, l_window, nullptr, nullptr, n_pairs, nullptr});
	}
	// ... over the triangle of the slice [a0, a0 + n).  A single variant has no pair.
	int dispatch(int mode, uint32_t a0, uint32_t n, uint32_t tile_variants, int32_t window, uint32_t l_window, uint64_t* n_pairs) {
		if (n < 2) { if (n_pairs) *n_pairs = 0; return TWK_HIP_OK; }
		return dispatch(mode, a0, n, a0, n, 1, 0, 1, tile_variants, window, l_window, n_pairs);
	}
	// Behind the last launch: the device-to-host copies `copies` enqueues and one wait for the stream, or "<what>: <the runtime's reason>".
	template <class Copies>
	int download(const char* what, Copies&& copies) {
		hipError_t e = copies();
		if (e == hipSuccess) e = hipStreamSynchronize(c->s_compute);
		if (e != hipSuccess) { snprintf(c->err, sizeof(c->err), "%s: %s", what, hipGetErrorString(e)); return TWK_HIP_E_DEVICE; }
		return TWK_HIP_OK;
	}
	// ... of `items` items of `words` words each at `d`, a slab of items at a time: each(at, m, w) behind each wait - items [at, at + m), their words at w.
	template <class Each>
	int download_slabs(const char* what, const unsigned long long* d, size_t items, size_t words, size_t slab, Each&& each) {
		std::vector<unsigned long long> w(slab * words);
		for (size_t at = 0; at < items; at += slab) {
			const size_t m = std::min(slab, items - at);
			const int rc = download(what, [&] { return hipMemcpyAsync(w.data(), d + at * words, m * words * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->s_compute); });
			if (rc) return rc;
			each(at, m, (const unsigned long long*)w.data());
		}
		return TWK_HIP_OK;
	}
	// A stage of the call's report begins here on its stream (StageMarks::mark).
	hipError_t mark(int stage) { return marks.mark(stage, c->s_compute); }
	// What follows the call's last launch on its stream: `timed` between two marks - stage `stage` of the call's report, the `ms` of
	// twk_hip_*_last - then `rest`, then one wait for the stream, behind which every stage marked so far is written.  Both enqueue and
	// return the runtime's verdict.
	template <class Timed, class Rest>
	int tail(const char* what, Timed&& timed, Rest&& rest, int stage = 0) {
		hipError_t e = mark(stage);
		if (e == hipSuccess) e = timed();
		if (e == hipSuccess) e = mark(StageMarks::NO_STAGE);
		if (e == hipSuccess) e = rest();
		if (e == hipSuccess) e = hipStreamSynchronize(c->s_compute);
		if (e != hipSuccess) { snprintf(c->err, sizeof(c->err), "%s: %s", what, hipGetErrorString(e)); return TWK_HIP_E_DEVICE; }
		marks.write(*report);
		return TWK_HIP_OK;
	}
};

bool valid_stat(int32_t stat) { return stat == TWK_HIP_STAT_R || stat == TWK_HIP_STAT_R2 || stat == TWK_HIP_STAT_D || stat == TWK_HIP_STAT_DPRIME; }

// twk_hip_*_last: stage k of the entry point's report to ms[k], where the caller asks for it.
int last_of(const twk_hip_ctx* c, CallReport LastCalls::* which, std::initializer_list<double*> ms, uint64_t* bytes) {
	if (!c) return TWK_HIP_E_INVALID;
	const double* stage = (c->last.*which).stage_ms;
	for (double* m : ms) { if (m) *m = *stage; ++stage; }
	if (bytes) *bytes = (c->last.*which).bytes;
	return TWK_HIP_OK;
}

}  // namespace
}  // extern "C++"

// LD scores: per-variant sums over the records of the region (a rectangle or a triangle, a shard of it: the region call's geometry).
int twk_hip_ld_score(twk_hip_ctx* c, int mode, const twk_hip_filters* f, uint32_t a0, uint32_t nA, uint32_t b0, uint32_t nB, int32_t triangle,
                     uint32_t part, uint32_t n_parts, uint32_t tile_variants, int32_t window, uint32_t l_window,
                     uint64_t* n_partners, double* sum_r2, uint64_t* n_pairs) {
	ReduceCall call(c, Reduce::score, nullptr, f, n_partners && sum_r2, mode, a0, nA);
	if (call.bad) return call.bad;
	const size_t M = c->M;
	HIPCHK(c, c->d_score_sum.reserve(M, M, nullptr));
	HIPCHK(c, c->d_score_n.reserve(M, M, nullptr));
	HIPCHK(c, hipMemsetAsync(c->d_score_sum, 0, M * sizeof(double), c->s_compute));
	HIPCHK(c, hipMemsetAsync(c->d_score_n, 0, M * sizeof(unsigned long long), c->s_compute));
	call.arm(0);
	const int rc = call.dispatch(mode, a0, nA, b0, nB, triangle, part, n_parts, tile_variants, window, l_window, n_pairs);
	if (rc) return rc;
	return call.download("score arrays", [&] {
		const hipError_t e = hipMemcpyAsync(sum_r2, c->d_score_sum, M * sizeof(double), hipMemcpyDeviceToHost, c->s_compute);
		return e != hipSuccess ? e : hipMemcpyAsync(n_partners, c->d_score_n, M * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->s_compute);
	});
}

// LD pruning: the greedy walk over the bitmap the launches filled.
int twk_hip_ld_prune(twk_hip_ctx* c, int mode, const twk_hip_filters* f, uint32_t a0, uint32_t n, uint32_t tile_variants,
                     int32_t window, uint32_t l_window, uint8_t* keep, uint64_t* n_kept, uint64_t* n_edges, uint64_t* n_pairs) {
	ReduceCall call(c, Reduce::prune, &LastCalls::prune, f, keep != nullptr, mode, a0, n);
	if (call.bad) return call.bad;
	const size_t M = c->M;
	const uint32_t stride = (n + 63) / 64;
	int rc = call.bitmap(a0, n, "LD pruning of %u variants needs an adjacency bitmap of %zu bytes: %s"); if (rc) return rc;
	const bool in_lds = stride <= WALK_LDS_WORDS;
	HIPCHK(c, c->d_prune_keep.reserve(M, M, nullptr));
	if (!in_lds) HIPCHK(c, c->d_walk.reserve(stride, stride, nullptr));
	HIPCHK(c, hipMemsetAsync(c->d_prune_keep, 0, M, c->s_compute));
	if (!in_lds) HIPCHK(c, hipMemsetAsync(c->d_walk, 0, (size_t)stride * sizeof(unsigned long long), c->s_compute));
	rc = call.dispatch(mode, a0, n, tile_variants, window, l_window, n_pairs); if (rc) return rc;
	unsigned long long counts[2] = {0, 0};
	rc = call.tail("prune walk", [&] {
		hipLaunchKernelGGL(in_lds ? k_ld_prune_walk<true> : k_ld_prune_walk<false>, dim3(1), dim3(WALK_THREADS), 0, c->s_compute, (const unsigned long long*)c->reduce.map.bits.adj,
		                   a0, n, stride, in_lds ? nullptr : c->d_walk.get(), c->d_prune_keep.get(), c->d_counts + 1);
		return hipGetLastError();
	}, [&] {
		const hipError_t e = hipMemcpyAsync(keep, c->d_prune_keep, M, hipMemcpyDeviceToHost, c->s_compute);
		return e != hipSuccess ? e : hipMemcpyAsync(counts, c->d_counts, sizeof(counts), hipMemcpyDeviceToHost, c->s_compute);
	});
	if (rc) return rc;
	if (n_edges) *n_edges = counts[0];
	if (n_kept) *n_kept = counts[1];
	return TWK_HIP_OK;
}

int twk_hip_prune_last(const twk_hip_ctx* c, double* walk_ms, uint64_t* bitmap_bytes) { return last_of(c, &LastCalls::prune, {walk_ms}, bitmap_bytes); }

// LD clumping: the walk in P order over the bitmap the launches filled from both ends of a pair.
int twk_hip_ld_clump(twk_hip_ctx* c, int mode, const twk_hip_filters* f, uint32_t a0, uint32_t n, uint32_t tile_variants,
                     int32_t window, uint32_t l_window, const double* p, double p1, double p2,
                     uint32_t* index_of, uint64_t* n_clumps, uint64_t* n_members, uint64_t* n_edges, uint64_t* n_pairs) {
	ReduceCall call(c, Reduce::clump, &LastCalls::clump, f, p && index_of && p1 >= 0.0 && p1 <= p2 && p2 <= 1.0, mode, a0, n);      // (a NaN fails every comparison)
	if (call.bad) return call.bad;
	const size_t M = c->M;
	const uint32_t stride = (n + 63) / 64;
	// the candidates (P <= p1) in visiting order - ascending P, ties in file order - and the variants that can belong to no clump
	std::vector<uint32_t> order;
	std::vector<unsigned long long> taken0(stride, 0ull);
	if (n & 63) taken0[stride - 1] = ~0ull << (n & 63);                            // (beyond the slice: nobody's)
	for (uint32_t v = 0; v < n; ++v) {
		const double pv = p[a0 + v];
		if (pv != pv) { taken0[v >> 6] |= 1ull << (v & 63); continue; }
		if (!(pv >= 0.0 && pv <= 1.0)) return TWK_HIP_E_INVALID;
		if (pv > p2) taken0[v >> 6] |= 1ull << (v & 63);
		if (pv <= p1) order.push_back(v);
	}
	std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return p[a0 + x] < p[a0 + y]; });
	// (p1 <= p2: every candidate is eligible - an index variant that may not be in a clump cannot arise)
	for (const uint32_t v : order) if (taken0[v >> 6] >> (v & 63) & 1) return TWK_HIP_E_INVALID;
	const uint32_t m = (uint32_t)order.size();
	int rc = call.bitmap(a0, n, "LD clumping of %u variants needs an adjacency bitmap of %zu bytes: %s"); if (rc) return rc;      // (both triangles used)
	const bool in_lds = stride <= CLUMP_LDS_WORDS;
	HIPCHK(c, c->d_clump_index.reserve(M, M, nullptr));
	HIPCHK(c, c->d_walk.reserve(stride, stride, nullptr));
	HIPCHK(c, c->d_clump_order.reserve(m ? m : 1, m ? m : 1, nullptr));
	HIPCHK(c, hipMemsetAsync(c->d_clump_index, 0xFF, M * sizeof(uint32_t), c->s_compute));          // TWK_HIP_NO_CLUMP
	// (from pageable memory: the copies have left `order` and `taken0` when they return; both live to the end of the call anyway)
	HIPCHK(c, hipMemcpyAsync(c->d_walk, taken0.data(), (size_t)stride * sizeof(unsigned long long), hipMemcpyHostToDevice, c->s_compute));
	if (m) HIPCHK(c, hipMemcpyAsync(c->d_clump_order, order.data(), (size_t)m * sizeof(uint32_t), hipMemcpyHostToDevice, c->s_compute));
	rc = call.dispatch(mode, a0, n, tile_variants, window, l_window, n_pairs); if (rc) return rc;
	unsigned long long counts[3] = {0, 0, 0};
	rc = call.tail("clump walk", [&] {
		hipLaunchKernelGGL(in_lds ? k_ld_clump_walk<true> : k_ld_clump_walk<false>, dim3(1), dim3(CLUMP_WALK_THREADS), 0, c->s_compute, (const unsigned long long*)c->reduce.map.bits.adj,
		                   a0, n, stride, (const uint32_t*)c->d_clump_order, m, c->d_walk.get(), c->d_clump_index.get(), c->d_counts + 1);
		return hipGetLastError();
	}, [&] {
		const hipError_t e = hipMemcpyAsync(index_of, c->d_clump_index, M * sizeof(uint32_t), hipMemcpyDeviceToHost, c->s_compute);
		return e != hipSuccess ? e : hipMemcpyAsync(counts, c->d_counts, sizeof(counts), hipMemcpyDeviceToHost, c->s_compute);
	});
	if (rc) return rc;
	if (n_edges) *n_edges = counts[0];
	if (n_clumps) *n_clumps = counts[1];
	if (n_members) *n_members = counts[2];
	return TWK_HIP_OK;
}

int twk_hip_clump_last(const twk_hip_ctx* c, double* walk_ms, uint64_t* bitmap_bytes) { return last_of(c, &LastCalls::clump, {walk_ms}, bitmap_bytes); }

// LD matrix: the matrix is preset to the fill in front of the launches, gets its diagonal behind the last of them and leaves in one 2-D
// copy that honours the caller's row pitch.
int twk_hip_ld_matrix(twk_hip_ctx* c, int mode, const twk_hip_filters* f, uint32_t a0, uint32_t n, uint32_t tile_variants, int32_t window, uint32_t l_window,
                      int32_t stat, float fill, float* out, uint64_t ld, uint64_t* n_records, uint64_t* n_pairs) {
	ReduceCall call(c, Reduce::matrix, &LastCalls::matrix, f, out && valid_stat(stat), mode, a0, n);
	if (call.bad) return call.bad;
	if (ld < n) return TWK_HIP_E_INVALID;
	const size_t cells = (size_t)n * n;
	// the dense matrix: n * n floats, whatever the window
	float* const d_matrix = call.hold<float>(cells, "the LD matrix of %u variants needs %zu bytes of device memory: %s", n);
	if (call.mem.failed) return call.mem.failed;
	int rc = call.zero_counts(); if (rc) return rc;
	HIPCHK(c, preset_floats(d_matrix, fill, cells, c->s_compute));
	c->reduce.map.matrix = MatrixMap{d_matrix, c->d_counts, a0, n, stat};
	call.arm(cells * sizeof(float));
	rc = call.dispatch(mode, a0, n, tile_variants, window, l_window, n_pairs); if (rc) return rc;
	if (stat != TWK_HIP_STAT_D) {      // (D: the diagonal keeps the preset fill - no launch stores on it)
		hipLaunchKernelGGL(k_ld_matrix_diag, dim3((n + 255) / 256), dim3(256), 0, c->s_compute, d_matrix, n, 1.0f);
		HIPCHK(c, hipGetLastError());
	}
	unsigned long long count = 0;
	rc = call.tail("LD matrix", [&] {
		return hipMemcpy2DAsync(out, (size_t)ld * sizeof(float), d_matrix, (size_t)n * sizeof(float), (size_t)n * sizeof(float), n, hipMemcpyDeviceToHost, c->s_compute);
	}, [&] { return hipMemcpyAsync(&count, c->d_counts, sizeof(count), hipMemcpyDeviceToHost, c->s_compute); });
	if (rc) return rc;
	if (n_records) *n_records = count;
	return TWK_HIP_OK;
}

int twk_hip_matrix_last(const twk_hip_ctx* c, double* copy_ms, uint64_t* matrix_bytes) { return last_of(c, &LastCalls::matrix, {copy_ms}, matrix_bytes); }

// The banded kinds (banded matrix, D' bounds, haplotype blocks, LD splitting): the band's layout of the slice [a0, a0 + n) from the uploaded
// metadata (ld_bandmat_index.h), on the host, and what the kinds do with it.
extern "C++" {
namespace {
// (the caller has checked [a0, a0 + n) against M)
int band_layout(twk_hip_ctx* c, uint32_t a0, uint32_t n, uint32_t l_window, BandLayout& b) {
	if (c->h_meta.size() < (size_t)a0 + n) return TWK_HIP_E_INVALID;
	const twk_hip_variant_meta* meta = c->h_meta.data() + a0;
	if (bm_band_layout(n, [&](uint32_t k) { return meta[k].pos; }, [&](uint32_t k) { return meta[k].rid; }, l_window, b)) return TWK_HIP_OK;
	snprintf(c->err, sizeof(c->err), "banded LD matrix: the variants [%u, %u) are not sorted by (contig, position): a row's window is then no contiguous band", a0, a0 + n);
	return TWK_HIP_E_INVALID;
}
// first[n] and row_ptr[n + 1] as the caller of an entry point gets them.
void give_layout(const BandLayout& b, uint32_t* first, uint64_t* row_ptr) {
	memcpy(first, b.first.data(), b.first.size() * sizeof(uint32_t));
	memcpy(row_ptr, b.ptr.data(), b.ptr.size() * sizeof(uint64_t));
}
// The band map on the device, a BandRow per variant: held by the call and uploaded.
int band_rows(ReduceCall& call, const BandLayout& b, const BandRow** d_rows) {
	twk_hip_ctx* c = call.c;
	BandRow* const rows = call.hold<BandRow>(b.rows.size(), "the band map of %u variants needs %zu bytes of device memory: %s", (uint32_t)b.rows.size());
	if (call.mem.failed) return call.mem.failed;
	// (from pageable memory: the copy has left the layout's rows when it returns; they live to the end of the call anyway)
	HIPCHK(c, hipMemcpyAsync(rows, b.rows.data(), b.rows.size() * sizeof(BandRow), hipMemcpyHostToDevice, c->s_compute));
	*d_rows = rows;
	return TWK_HIP_OK;
}
// The band of the slice on the device, row_ptr[n] floats and the band map: preset to the fill in front of the launches, its diagonal behind
// the last of them.  Where it lies is what the launches were told: c->reduce.map.band, for the rest of the call.
int band_fill(ReduceCall& call, int mode, uint32_t a0, uint32_t n, uint32_t tile_variants, int32_t window, uint32_t l_window, int32_t stat, float fill,
              const BandLayout& b, uint64_t* n_pairs) {
	twk_hip_ctx* c = call.c;
	BandMap& d = c->reduce.map.band;
	d = BandMap{call.hold<float>(b.cells, "the banded LD matrix of %u variants needs %zu bytes of device memory: %s", n), nullptr, nullptr, a0, n, stat};
	if (call.mem.failed) return call.mem.failed;
	int rc = call.zero_counts(); if (rc) return rc;
	d.n_records = c->d_counts;
	HIPCHK(c, preset_floats(d.values, fill, b.cells, c->s_compute));
	rc = band_rows(call, b, &d.rows); if (rc) return rc;
	call.arm(b.cells * sizeof(float));
	rc = call.dispatch(mode, a0, n, tile_variants, window, l_window, n_pairs); if (rc) return rc;
	if (stat != TWK_HIP_STAT_D) {      // (D: the diagonal keeps the preset fill - no launch stores on it)
		hipLaunchKernelGGL(k_ld_bandmat_diag, dim3((n + 255) / 256), dim3(256), 0, c->s_compute, d.values, d.rows, n, 1.0f);
		HIPCHK(c, hipGetLastError());
	}
	return TWK_HIP_OK;
}
// The D' bounds of the slice on the device, a byte a slot each, and the band map: the preset 255, the launches.  Where they lie:
// c->reduce.map.ci, for the rest of the call.
int ci_band_fill(ReduceCall& call, int mode, uint32_t a0, uint32_t n, uint32_t tile_variants, uint32_t l_window, const BandLayout& b, uint64_t* n_pairs) {
	twk_hip_ctx* c = call.c;
	CiMap& d = c->reduce.map.ci;
	d = CiMap{nullptr, nullptr, nullptr, a0, n};
	d.hi = call.hold<uint8_t>(b.cells, "the upper D' bounds of %u variants' band need %zu bytes of device memory: %s", n);
	d.lo = call.hold<uint8_t>(b.cells, "the lower D' bounds of %u variants' band need %zu bytes of device memory: %s", n);
	if (call.mem.failed) return call.mem.failed;
	int rc = call.zero_counts(); if (rc) return rc;
	HIPCHK(c, hipMemsetAsync(d.lo, BC_NONE, b.cells, c->s_compute));
	HIPCHK(c, hipMemsetAsync(d.hi, BC_NONE, b.cells, c->s_compute));
	rc = band_rows(call, b, &d.rows); if (rc) return rc;
	call.arm(b.cells * 2);
	return call.dispatch(mode, a0, n, tile_variants, (int32_t)TWK_HIP_OPT_WINDOW, l_window, n_pairs);
}
}  // namespace
}  // extern "C++"

int twk_hip_bandmat_layout(twk_hip_ctx* c, uint32_t a0, uint32_t n, uint32_t l_window, uint32_t* first, uint64_t* row_ptr) {
	if (!c || !first || !row_ptr) return TWK_HIP_E_INVALID;
	if (!c->raw) return TWK_HIP_E_STATE;
	if (n == 0 || (uint64_t)a0 + n > c->M) return TWK_HIP_E_INVALID;
	BandLayout b;
	const int rc = band_layout(c, a0, n, l_window, b); if (rc) return rc;
	give_layout(b, first, row_ptr);
	return TWK_HIP_OK;
}

// ... and the band itself, in one contiguous copy of row_ptr[n] floats; first and row_ptr are the host layout's.
int twk_hip_ld_matrix_band(twk_hip_ctx* c, int mode, const twk_hip_filters* f, uint32_t a0, uint32_t n, uint32_t tile_variants, int32_t window, uint32_t l_window,
                           int32_t stat, float fill, float* values, uint64_t capacity, uint32_t* first, uint64_t* row_ptr, uint64_t* n_records, uint64_t* n_pairs) {
	ReduceCall call(c, Reduce::bandmat, &LastCalls::bandmat, f, values && first && row_ptr && valid_stat(stat) && (window & TWK_HIP_OPT_WINDOW), mode, a0, n);
	if (call.bad) return call.bad;
	BandLayout b;
	int rc = band_layout(c, a0, n, l_window, b); if (rc) return rc;
	if (capacity < b.cells) {
		snprintf(c->err, sizeof(c->err), "banded LD matrix: the band of %u variants holds %zu floats, the caller's array %llu", n, b.cells, (unsigned long long)capacity);
		return TWK_HIP_E_INVALID;
	}
	rc = band_fill(call, mode, a0, n, tile_variants, window, l_window, stat, fill, b, n_pairs); if (rc) return rc;
	const BandMap& d = c->reduce.map.band;
	unsigned long long count = 0;
	rc = call.tail("banded LD matrix", [&] {
		return hipMemcpyAsync(values, d.values, b.cells * sizeof(float), hipMemcpyDeviceToHost, c->s_compute);
	}, [&] { return hipMemcpyAsync(&count, c->d_counts, sizeof(count), hipMemcpyDeviceToHost, c->s_compute); });
	if (rc) return rc;
	give_layout(b, first, row_ptr);
	if (n_records) *n_records = count;
	return TWK_HIP_OK;
}

int twk_hip_bandmat_last(const twk_hip_ctx* c, double* copy_ms, uint64_t* band_bytes) { return last_of(c, &LastCalls::bandmat, {copy_ms}, band_bytes); }

// Haplotype blocks (ld_blocks.hip.h): the D' confidence bounds of the in-window pairs in band storage, and the blocks selected from them.
int twk_hip_ld_dprime_ci_band(twk_hip_ctx* c, int mode, const twk_hip_filters* f, uint32_t a0, uint32_t n, uint32_t tile_variants, uint32_t l_window,
                              uint8_t* lo, uint8_t* hi, uint64_t capacity, uint32_t* first, uint64_t* row_ptr, uint64_t* n_records, uint64_t* n_pairs) {
	ReduceCall call(c, Reduce::dprime_ci, nullptr, f, lo && hi && first && row_ptr && l_window > 0, mode, a0, n);
	if (call.bad) return call.bad;
	BandLayout b;
	int rc = band_layout(c, a0, n, l_window, b); if (rc) return rc;
	if (capacity < b.cells) {
		snprintf(c->err, sizeof(c->err), "D' bounds: the band of %u variants holds %zu slots, the caller's arrays %llu", n, b.cells, (unsigned long long)capacity);
		return TWK_HIP_E_INVALID;
	}
	uint32_t* const d_inf = call.hold<uint32_t>((size_t)n, "the informative counts of %u variants need %zu bytes of device memory: %s", n);
	if (call.mem.failed) return call.mem.failed;
	rc = ci_band_fill(call, mode, a0, n, tile_variants, l_window, b, n_pairs); if (rc) return rc;
	const CiMap& d = c->reduce.map.ci;
	hipLaunchKernelGGL(k_ci_informative, dim3((n + 3) / 4), dim3(BLOCKS_THREADS), 0, c->s_compute, (const uint8_t*)d.lo, d.rows, n, d_inf);
	HIPCHK(c, hipGetLastError());
	std::vector<uint32_t> inf(n);
	rc = call.tail("D' bounds", [&] {
		const hipError_t e = hipMemcpyAsync(lo, d.lo, b.cells, hipMemcpyDeviceToHost, c->s_compute);
		return e != hipSuccess ? e : hipMemcpyAsync(hi, d.hi, b.cells, hipMemcpyDeviceToHost, c->s_compute);
	}, [&] { return hipMemcpyAsync(inf.data(), d_inf, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->s_compute); });
	if (rc) return rc;
	give_layout(b, first, row_ptr);
	if (n_records) { uint64_t sum = 0; for (const uint32_t x : inf) sum += x; *n_records = sum; }
	return TWK_HIP_OK;
}

int twk_hip_ld_blocks(twk_hip_ctx* c, int mode, const twk_hip_filters* f, uint32_t a0, uint32_t n, uint32_t tile_variants, uint32_t l_window,
                      const twk_hip_block_params* params, uint32_t* block_of, uint32_t* first, uint32_t* last, uint32_t* n_strong, uint32_t* n_recomb,
                      uint64_t* n_blocks, uint64_t* n_candidates, uint64_t* n_informative, uint64_t* n_pairs) {
	static_assert(sizeof(twk_hip_block_params) == sizeof(BlockParams), "BlockParams is twk_hip_block_params, field for field");
	BlockParams par = BLOCK_DEFAULTS;
	if (params) memcpy(&par, params, sizeof(par));
	ReduceCall call(c, Reduce::blocks, &LastCalls::blocks, f, block_of && bc_params_ok(par) && l_window > 0, mode, a0, n);
	if (call.bad) return call.bad;
	enum { COUNTS, EMIT, SORT, WALK };      // the stages of the call's report (twk_hip_blocks_stages; twk_hip_blocks_last: the walk)
	BandLayout b;
	int rc = band_layout(c, a0, n, l_window, b); if (rc) return rc;
	BlockKey key; uint32_t key_bits = 0;
	if (b.widest > BLOCK_MAX_BAND || !bc_key_layout(n, b.widest, l_window, &key, &key_bits)) {
		snprintf(c->err, sizeof(c->err), "haplotype blocks: a window of %u base pairs reaches %u variants in a row of %u (at most %u, and a sort key of at most 64 bits)",
		         l_window, b.widest, n, BLOCK_MAX_BAND);
		return TWK_HIP_E_INVALID;
	}
	const size_t M = c->M;
	const uint32_t stride = (n + 63) / 64;
	const bool in_lds = stride <= BLOCKS_LDS_WORDS;
	std::vector<uint32_t> h_pos(n);
	for (uint32_t u = 0; u < n; ++u) h_pos[u] = c->h_meta[a0 + u].pos;
	size_t scan_tmp = 0;
	HIPCHK(c, rocprim::exclusive_scan(nullptr, scan_tmp, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)n, rocprim::plus<uint32_t>(), c->s_compute));
	const char* const band_what = "the prefix counts of %u variants' band need %zu bytes of device memory: %s";
	const char* const variant_what = "the per-variant arrays of %u variants need %zu bytes of device memory: %s";
	uint32_t* const d_ps = call.hold<uint32_t>(b.cells, band_what, n);
	uint32_t* const d_pr = call.hold<uint32_t>(b.cells, band_what, n);
	uint32_t* const d_counts3 = call.hold<uint32_t>((size_t)n * 3, variant_what, n);
	uint32_t* const d_blk = call.hold<uint32_t>((size_t)n * 3, variant_what, n);
	uint32_t *d_pos, *d_flat, *d_off;
	for (uint32_t** x : {&d_pos, &d_flat, &d_off}) *x = call.hold<uint32_t>((size_t)n, variant_what, n);
	uint32_t* const d_block_of = call.hold<uint32_t>(M, variant_what, n);
	unsigned long long* const d_used = call.hold<unsigned long long>((size_t)stride, variant_what, n);
	size_t tmp_bytes = std::max<size_t>(scan_tmp, 16);      // the scan's scratch, then the sort's: one buffer, grown for the sort if that needs more
	char* d_tmp = call.hold<char>(tmp_bytes, "the scan of %u counts needs %zu bytes of device memory: %s", n);
	if (call.mem.failed) return call.mem.failed;
	rc = ci_band_fill(call, mode, a0, n, tile_variants, l_window, b, n_pairs); if (rc) return rc;
	const CiMap& ci = c->reduce.map.ci;
	HIPCHK(c, hipMemcpyAsync(d_pos, h_pos.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, c->s_compute));
	HIPCHK(c, hipMemsetAsync(d_block_of, 0xFF, M * sizeof(uint32_t), c->s_compute));          // TWK_HIP_NO_BLOCK
	HIPCHK(c, hipMemsetAsync(d_blk, 0, (size_t)n * 3 * sizeof(uint32_t), c->s_compute));
	HIPCHK(c, hipMemsetAsync(d_used, 0, (size_t)stride * sizeof(unsigned long long), c->s_compute));
	HIPCHK(c, hipMemsetAsync(c->d_counts, 0, 3 * sizeof(unsigned long long), c->s_compute));
	HIPCHK(c, call.mark(COUNTS));
	const BlocksBand band{ci.lo, ci.hi, ci.rows, d_pos, d_ps, d_pr, n, par, key};
	const dim3 per_row((n + 3) / 4), per_variant((n + BLOCKS_THREADS - 1) / BLOCKS_THREADS), threads(BLOCKS_THREADS);
	hipLaunchKernelGGL(k_blocks_prefix, per_row, threads, 0, c->s_compute, band);
	HIPCHK(c, hipGetLastError());
	hipLaunchKernelGGL(k_blocks_candidates<false>, per_variant, threads, 0, c->s_compute, band, d_counts3, (const uint32_t*)nullptr, 0u,
	                   (unsigned long long*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr);
	HIPCHK(c, hipGetLastError());
	hipLaunchKernelGGL(k_blocks_flatten, per_variant, threads, 0, c->s_compute, (const uint32_t*)d_counts3, n, d_flat);
	HIPCHK(c, hipGetLastError());
	HIPCHK(c, rocprim::exclusive_scan(d_tmp, scan_tmp, d_flat, d_off, 0u, (size_t)n, rocprim::plus<uint32_t>(), c->s_compute));
	HIPCHK(c, call.mark(StageMarks::NO_STAGE));
	std::vector<uint32_t> counts3((size_t)n * 3);
	rc = call.download("haplotype blocks: the candidate counts", [&] {
		return hipMemcpyAsync(counts3.data(), d_counts3, counts3.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->s_compute);
	});
	if (rc) return rc;
	call.marks.write(*call.report);            // (the counts: a call that ends here, or without a candidate, has no other stage)
	uint64_t n_q = 0, n_c = 0, n_inf = 0;
	for (uint32_t u = 0; u < n; ++u) { n_q += counts3[3 * (size_t)u]; n_c += counts3[3 * (size_t)u + 1]; n_inf += counts3[3 * (size_t)u + 2]; }
	if (n_q > 0xFFFFFFFFull) {
		snprintf(c->err, sizeof(c->err), "haplotype blocks: %llu qualifying candidates, more than 2^32 - 1; split the slice", (unsigned long long)n_q);
		return TWK_HIP_E_INVALID;
	}
	std::vector<uint32_t> h_block_of(M, BLOCK_NONE), h_blk;
	unsigned long long walked = 0;
	if (n_q) {
		const size_t q = (size_t)n_q;
		const char* what = "the %u qualifying candidates need %zu bytes of device memory: %s";
		unsigned long long *d_keys, *d_keys_out;
		uint32_t *d_vals, *d_vals_out, *d_cs, *d_cr;
		for (unsigned long long** x : {&d_keys, &d_keys_out}) *x = call.hold<unsigned long long>(q, what, (uint32_t)n_q);
		for (uint32_t** x : {&d_vals, &d_vals_out, &d_cs, &d_cr}) *x = call.hold<uint32_t>(q, what, (uint32_t)n_q);
		if (call.mem.failed) return call.mem.failed;
		HIPCHK(c, hipMemsetAsync(d_keys, 0xFF, q * sizeof(unsigned long long), c->s_compute));      // (a slot the emitter leaves is no candidate: the walk skips it)
		HIPCHK(c, hipMemsetAsync(d_vals, 0, q * sizeof(uint32_t), c->s_compute));
		HIPCHK(c, call.mark(EMIT));
		hipLaunchKernelGGL(k_blocks_candidates<true>, per_variant, threads, 0, c->s_compute, band, (uint32_t*)nullptr, (const uint32_t*)d_off, (uint32_t)n_q,
		                   d_keys, d_vals, d_cs, d_cr);
		HIPCHK(c, hipGetLastError());
		HIPCHK(c, call.mark(SORT));
		size_t sort_tmp = 0;
		HIPCHK(c, rocprim::radix_sort_pairs(nullptr, sort_tmp, d_keys, d_keys_out, d_vals, d_vals_out, q, 0u, key_bits, c->s_compute));
		tmp_bytes = std::max(tmp_bytes, sort_tmp);
		d_tmp = call.mem.hold(tmp_bytes, "the sort of %u candidates needs %zu bytes of device memory: %s", (uint32_t)n_q, d_tmp);
		if (call.mem.failed) return call.mem.failed;
		HIPCHK(c, rocprim::radix_sort_pairs(d_tmp, tmp_bytes, d_keys, d_keys_out, d_vals, d_vals_out, q, 0u, key_bits, c->s_compute));
		HIPCHK(c, call.mark(StageMarks::NO_STAGE));
		h_blk.resize((size_t)n * 3);
		rc = call.tail("haplotype blocks: the walk", [&] {
			hipLaunchKernelGGL(in_lds ? k_blocks_walk<true> : k_blocks_walk<false>, dim3(1), dim3(BLOCKS_WALK_THREADS), 0, c->s_compute,
			                   (const unsigned long long*)d_keys_out, (const uint32_t*)d_vals_out, (uint32_t)n_q, key, (const uint32_t*)d_cs, (const uint32_t*)d_cr,
			                   a0, n, stride, d_used, d_block_of, d_blk, c->d_counts.get());
			return hipGetLastError();
		}, [&] {
			hipError_t e = hipMemcpyAsync(h_block_of.data(), d_block_of, M * sizeof(uint32_t), hipMemcpyDeviceToHost, c->s_compute);
			if (e == hipSuccess) e = hipMemcpyAsync(h_blk.data(), d_blk, h_blk.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->s_compute);
			return e != hipSuccess ? e : hipMemcpyAsync(&walked, c->d_counts, sizeof(walked), hipMemcpyDeviceToHost, c->s_compute);
		}, WALK);
		if (rc) return rc;
	}
	// the blocks in file order: a variant that is its own block_of begins one
	uint64_t nb = 0;
	for (uint32_t u = 0; u < n && n_q; ++u) {
		if (h_block_of[a0 + u] != a0 + u) continue;
		if (nb >= n / 2) { snprintf(c->err, sizeof(c->err), "haplotype blocks: more than %u blocks among %u variants", n / 2, n); return TWK_HIP_E_DEVICE; }
		if (first) first[nb] = a0 + u;
		if (last) last[nb] = h_blk[3 * (size_t)u];
		if (n_strong) n_strong[nb] = h_blk[3 * (size_t)u + 1];
		if (n_recomb) n_recomb[nb] = h_blk[3 * (size_t)u + 2];
		++nb;
	}
	if (nb != walked) { snprintf(c->err, sizeof(c->err), "haplotype blocks: the walk made %llu blocks, block_of holds %llu", walked, (unsigned long long)nb); return TWK_HIP_E_DEVICE; }
	memcpy(block_of, h_block_of.data(), M * sizeof(uint32_t));
	if (n_blocks) *n_blocks = nb;
	if (n_candidates) *n_candidates = n_c;
	if (n_informative) *n_informative = n_inf;
	return TWK_HIP_OK;
}

// (the report's stages: COUNTS, EMIT, SORT, WALK)
int twk_hip_blocks_last(const twk_hip_ctx* c, double* walk_ms, uint64_t* band_bytes) { return last_of(c, &LastCalls::blocks, {nullptr, nullptr, nullptr, walk_ms}, band_bytes); }
int twk_hip_blocks_stages(const twk_hip_ctx* c, double* counts_ms, double* emit_ms, double* sort_ms) { return last_of(c, &LastCalls::blocks, {counts_ms, emit_ms, sort_ms}, nullptr); }

// LD splitting (ld_split.hip.h): the banded r2 matrix of the slice, filled by the bandmat kind and kept on the device, then row prefixes,
// block sums, one layer launch per k and the backtrack - all of it integers.  (The call writes its own report: twk_hip_bandmat_last keeps what the
// last twk_hip_ld_matrix_band call left.)
int twk_hip_ld_split(twk_hip_ctx* c, int mode, const twk_hip_filters* f, uint32_t a0, uint32_t n, uint32_t tile_variants, uint32_t l_window,
                     uint32_t min_size, uint32_t max_size, uint32_t k_max, uint64_t* total, uint8_t* feasible, uint64_t* cost, uint32_t* cuts,
                     uint64_t* n_records, uint64_t* n_pairs) {
	ReduceCall call(c, Reduce::bandmat, &LastCalls::split, f, total && feasible && cost && cuts && l_window > 0 && sp_sizes_ok(n, min_size, max_size, k_max), mode, a0, n);
	if (call.bad) return call.bad;
	enum { BAND, SUMS, LAYERS, BACKTRACK };      // the stages of the call's report (twk_hip_split_last)
	BandLayout b;
	int rc = band_layout(c, a0, n, l_window, b); if (rc) return rc;
	if (c->h_meta[a0].rid != c->h_meta[(size_t)a0 + n - 1].rid) {
		snprintf(c->err, sizeof(c->err), "LD splitting: the variants [%u, %u) lie on more than one contig; split one contig a call", a0, a0 + n);
		return TWK_HIP_E_INVALID;
	}
	if ((b.cells - n) / 2 >= SPLIT_MAX_PAIRS) {
		snprintf(c->err, sizeof(c->err), "LD splitting: the band of %u variants holds %zu pairs, 2^31 or more: their sum may pass 2^63; narrow the window or split the slice", n, (b.cells - n) / 2);
		return TWK_HIP_E_INVALID;
	}
	std::vector<uint32_t> h_upc(n);
	uint32_t widest = 1;                       // the offsets Rp stores: at least one row, so that no buffer is empty
	for (uint32_t u = 0; u < n; ++u) {
		h_upc[u] = sp_upc(sp_upper(b.rows[u].first, b.rows[u].len, u), max_size);
		widest = std::max(widest, h_upc[u]);
	}
	const SplitSizes sizes{n, min_size, max_size, k_max};
	const size_t n1 = (size_t)n + 1, rp_items = (size_t)widest * n, w_items = (size_t)(max_size - min_size + 1) * n1, d_items = (size_t)k_max * n1;
	const size_t cut_items = (size_t)k_max * (k_max + 1);
	const char* const sums_what = "LD splitting: the row prefixes and block sums of %u variants need %zu bytes of device memory: %s";
	const char* const layers_what = "LD splitting: the layers of %u variants need %zu bytes of device memory: %s";
	long long* const d_rp = call.hold<long long>(rp_items, sums_what, n);
	long long* const d_w = call.hold<long long>(w_items, sums_what, n);
	uint16_t* const d_dk = call.hold<uint16_t>(d_items, layers_what, n);
	long long* const d_g = call.hold<long long>(2 * n1, layers_what, n);
	long long* const d_row_total = call.hold<long long>((size_t)n, layers_what, n);
	uint32_t* const d_upc = call.hold<uint32_t>((size_t)n, layers_what, n);
	long long* const d_gn = call.hold<long long>((size_t)k_max + 1, layers_what, n);
	unsigned long long* const d_cost = call.hold<unsigned long long>((size_t)k_max, layers_what, n);
	uint32_t* const d_cuts = call.hold<uint32_t>(cut_items, layers_what, n);
	uint8_t* const d_feasible = call.hold<uint8_t>((size_t)k_max, layers_what, n);
	unsigned long long* const d_total = call.hold<unsigned long long>((size_t)1, layers_what, n);
	uint32_t* const d_broken = call.hold<uint32_t>((size_t)1, layers_what, n);
	if (call.mem.failed) return call.mem.failed;
	HIPCHK(c, call.mark(BAND));
	rc = band_fill(call, mode, a0, n, tile_variants, (int32_t)TWK_HIP_OPT_WINDOW, l_window, TWK_HIP_STAT_R2, 0.0f, b, n_pairs); if (rc) return rc;
	const BandMap& band = c->reduce.map.band;
	call.report->bytes = call.mem.bytes();      // (everything the call holds, not the band alone: nothing is held behind this line)
	HIPCHK(c, call.mark(SUMS));
	// (from pageable memory: the copy has left h_upc when it returns)
	HIPCHK(c, hipMemcpyAsync(d_upc, h_upc.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, c->s_compute));
	HIPCHK(c, hipMemsetAsync(d_gn, 0xFF, ((size_t)k_max + 1) * sizeof(long long), c->s_compute));      // SPLIT_INFEASIBLE
	HIPCHK(c, hipMemsetAsync(d_g, 0, sizeof(long long), c->s_compute));                                // G_0(0) = 0, layer 0's whole range
	const dim3 threads(SPLIT_THREADS);
	hipLaunchKernelGGL(k_split_prefix, dim3((n + 3) / 4), threads, 0, c->s_compute, (const float*)band.values, band.rows, (const uint32_t*)d_upc, n, d_rp, d_row_total);
	HIPCHK(c, hipGetLastError());
	hipLaunchKernelGGL(k_split_sums, dim3((n + SPLIT_THREADS - 1) / SPLIT_THREADS), threads, 0, c->s_compute, (const long long*)d_rp, (const uint32_t*)d_upc, sizes, d_w);
	HIPCHK(c, hipGetLastError());
	HIPCHK(c, call.mark(LAYERS));
	for (uint32_t k = 1; k <= k_max; ++k) {
		const uint32_t lo = sp_layer_lo(k, min_size), hi = sp_layer_hi(k, max_size, n);
		if (lo > hi) break;                    // k * min_size > n: no further layer holds a feasible b
		long long* const g_prev = d_g + ((k - 1) & 1) * n1;
		long long* const g_cur = d_g + (k & 1) * n1;
		hipLaunchKernelGGL(k_split_layer, dim3((hi - lo) / SPLIT_THREADS + 1), threads, 0, c->s_compute, (const long long*)g_prev, (const long long*)d_w, sizes, k, lo, hi,
		                   sp_layer_lo(k - 1, min_size), sp_layer_hi(k - 1, max_size, n), g_cur, d_dk, d_gn);
		HIPCHK(c, hipGetLastError());
	}
	HIPCHK(c, call.mark(BACKTRACK));
	hipLaunchKernelGGL(k_split_backtrack, dim3(1), dim3(SPLIT_MAX_K), 0, c->s_compute, (const long long*)d_row_total, (const long long*)d_gn, (const uint16_t*)d_dk, sizes,
	                   d_total, d_feasible, d_cost, d_cuts, d_broken);
	HIPCHK(c, hipGetLastError());
	HIPCHK(c, call.mark(StageMarks::NO_STAGE));
	std::vector<uint8_t> h_feasible(k_max);
	std::vector<unsigned long long> h_cost(k_max);
	std::vector<uint32_t> h_cuts(cut_items);
	unsigned long long h_total = 0, count = 0;
	uint32_t broken = 0;
	rc = call.download("LD splitting: the partitions", [&] {
		hipError_t e = hipMemcpyAsync(h_feasible.data(), d_feasible, k_max, hipMemcpyDeviceToHost, c->s_compute);
		if (e == hipSuccess) e = hipMemcpyAsync(h_cost.data(), d_cost, (size_t)k_max * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->s_compute);
		if (e == hipSuccess) e = hipMemcpyAsync(h_cuts.data(), d_cuts, cut_items * sizeof(uint32_t), hipMemcpyDeviceToHost, c->s_compute);
		if (e == hipSuccess) e = hipMemcpyAsync(&h_total, d_total, sizeof(h_total), hipMemcpyDeviceToHost, c->s_compute);
		if (e == hipSuccess) e = hipMemcpyAsync(&broken, d_broken, sizeof(broken), hipMemcpyDeviceToHost, c->s_compute);
		return e != hipSuccess ? e : hipMemcpyAsync(&count, c->d_counts, sizeof(count), hipMemcpyDeviceToHost, c->s_compute);
	});
	if (rc) return rc;
	call.marks.write(*call.report);
	if (broken) { snprintf(c->err, sizeof(c->err), "LD splitting: %u of the chains through D do not end at the slice's start", broken); return TWK_HIP_E_DEVICE; }
	*total = h_total;
	for (uint32_t K = 1; K <= k_max; ++K) {
		feasible[K - 1] = h_feasible[K - 1];
		if (!h_feasible[K - 1]) continue;      // (the rows of an infeasible K stay as the caller left them)
		cost[K - 1] = h_cost[K - 1];
		memcpy(cuts + sp_cut_slot(K, 0, k_max), h_cuts.data() + sp_cut_slot(K, 0, k_max), ((size_t)K + 1) * sizeof(uint32_t));
	}
	if (n_records) *n_records = count;
	return TWK_HIP_OK;
}

int twk_hip_split_last(const twk_hip_ctx* c, double* band_ms, double* sums_ms, double* layers_ms, double* backtrack_ms, uint64_t* bytes) {
	return last_of(c, &LastCalls::split, {band_ms, sums_ms, layers_ms, backtrack_ms}, bytes);
}

// Top-k LD partners: the lists' slots are zeroed in front of the launches; behind the last of them the keys are copied out and unpacked
// on the host, a slab of variants at a time - 8 bytes per slot leave the device whoever unpacks.
int twk_hip_ld_topk(twk_hip_ctx* c, int mode, const twk_hip_filters* f, uint32_t a0, uint32_t nA, uint32_t b0, uint32_t nB, int32_t triangle,
                    uint32_t part, uint32_t n_parts, uint32_t tile_variants, int32_t window, uint32_t l_window,
                    int32_t stat, uint32_t k, uint32_t* idx, float* val, uint64_t* n_pairs) {
	ReduceCall call(c, Reduce::topk, &LastCalls::topk, f, idx && val && k >= 1 && k <= TOPK_MAX && valid_stat(stat), mode, a0, nA);
	if (call.bad) return call.bad;
	const size_t M = c->M, slots = M * k;
	unsigned long long* const d_topk = call.hold<unsigned long long>(slots, "the top-k lists of %u variants need %zu bytes of device memory: %s", (uint32_t)M);
	if (call.mem.failed) return call.mem.failed;
	// (beyond 64 KiB of dynamic LDS a kernel has to be told so; k = 32 asks for 72 KiB)
	HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(k_ld_topk), hipFuncAttributeMaxDynamicSharedMemorySize, (int)tk_lds_bytes(TOPK_MAX)));
	HIPCHK(c, hipMemsetAsync(d_topk, 0, slots * sizeof(unsigned long long), c->s_compute));
	c->reduce.map.topk = TopkMap{d_topk, k, stat};
	call.arm(slots * sizeof(unsigned long long));
	if (triangle && nA < 2) { if (n_pairs) *n_pairs = 0; }      // (a single variant has no pair)
	else { const int rc = call.dispatch(mode, a0, nA, b0, nB, triangle, part, n_parts, tile_variants, window, l_window, n_pairs); if (rc) return rc; }
	const auto t0 = std::chrono::steady_clock::now();
	const int rc = call.download_slabs("top-k lists", d_topk, slots, 1, std::min<size_t>(slots, (size_t)1 << 21),      // 16 MiB of keys at a time
		[&](size_t at, size_t m, const unsigned long long* keys) { for (size_t e = 0; e < m; ++e) tk_unpack(keys[e], idx + at + e, val + at + e); });
	if (rc) return rc;
	call.report->stage_ms[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();      // (the host's clock: the unpacking is the host's)
	return TWK_HIP_OK;
}

int twk_hip_topk_last(const twk_hip_ctx* c, double* unpack_ms, uint64_t* list_bytes) { return last_of(c, &LastCalls::topk, {unpack_ms}, list_bytes); }

// LD decay: the bins' integer accumulators are zeroed in front of the launches and converted behind the last of them.
int twk_hip_ld_decay(twk_hip_ctx* c, int mode, const twk_hip_filters* f, uint32_t a0, uint32_t nA, uint32_t b0, uint32_t nB, int32_t triangle,
                     uint32_t part, uint32_t n_parts, uint32_t tile_variants, int32_t window, uint32_t l_window,
                     uint32_t range_bp, uint32_t n_bins, uint64_t* n, double* sum_r2, uint64_t* n_pairs) {
	const bool bins_ok = n_bins >= 1 && n_bins <= DECAY_MAX_BINS && range_bp >= n_bins;      // (range_bp < n_bins: a width of 0)
	ReduceCall call(c, Reduce::decay, nullptr, f, n && sum_r2 && bins_ok, mode, a0, nA);
	if (call.bad) return call.bad;
	const size_t B = n_bins;
	HIPCHK(c, c->d_decay.reserve(3 * B, 3 * B, nullptr));
	HIPCHK(c, hipMemsetAsync(c->d_decay, 0, 3 * B * sizeof(unsigned long long), c->s_compute));
	c->reduce.map.decay = DecayMap{c->d_decay, c->d_decay + B, c->d_decay + 2 * B, dk_width(range_bp, n_bins), n_bins};
	call.arm(3 * B * sizeof(unsigned long long));
	int rc = call.dispatch(mode, a0, nA, b0, nB, triangle, part, n_parts, tile_variants, window, l_window, n_pairs);
	if (rc) return rc;
	std::vector<unsigned long long> acc(3 * B);
	rc = call.download("decay arrays", [&] { return hipMemcpyAsync(acc.data(), c->d_decay, 3 * B * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->s_compute); });
	if (rc) return rc;
	for (size_t b = 0; b < B; ++b) {
		sum_r2[b] = xs_sum_to_double_unsigned<DECAY_SPLIT>(acc[b], acc[B + b]);      // (exact in 128 bits, one conversion: ld_exact_sum.h)
		n[b] = acc[2 * B + b];
	}
	return TWK_HIP_OK;
}

// LD aggregate: the variants' bins are packed and uploaded and the cells' integer accumulators preset in front of the launches, and
// converted behind the last of them, a slab of cells at a time.
int twk_hip_ld_aggregate(twk_hip_ctx* c, int mode, const twk_hip_filters* f, uint32_t a0, uint32_t nA, uint32_t b0, uint32_t nB, int32_t triangle,
                         uint32_t part, uint32_t n_parts, uint32_t tile_variants, int32_t window, uint32_t l_window,
                         int32_t stat, const uint16_t* bin_x, const uint16_t* bin_y, uint32_t x_bins, uint32_t y_bins,
                         uint64_t* n, double* sum, double* sum_sq, double* min, double* max, uint64_t* n_pairs) {
	const bool bins_ok = x_bins >= 1 && x_bins <= AGG_MAX_BINS && y_bins >= 1 && y_bins <= AGG_MAX_BINS;
	ReduceCall call(c, Reduce::aggregate, nullptr, f, bin_x && bin_y && n && sum && sum_sq && min && max && valid_stat(stat) && bins_ok, mode, a0, nA);
	if (call.bad) return call.bad;
	const size_t M = c->M, cells = (size_t)x_bins * y_bins, words = cells * AGG_CELL_WORDS;
	std::vector<uint32_t> key(M);
	for (size_t v = 0; v < M; ++v) {
		if ((bin_x[v] != AGG_OFF && bin_x[v] >= x_bins) || (bin_y[v] != AGG_OFF && bin_y[v] >= y_bins)) return TWK_HIP_E_INVALID;
		key[v] = ag_pack(bin_x[v], bin_y[v]);
	}
	HIPCHK(c, c->d_agg_key.reserve(M, M, nullptr));
	unsigned long long* const d_agg = call.hold<unsigned long long>(words, "the LD aggregate of %u variants needs %zu bytes of device memory: %s", (uint32_t)M);
	if (call.mem.failed) return call.mem.failed;
	int rc = call.zero_counts(); if (rc) return rc;
	// (from pageable memory: the copy has left `key` when it returns)
	HIPCHK(c, hipMemcpyAsync(c->d_agg_key, key.data(), M * sizeof(uint32_t), hipMemcpyHostToDevice, c->s_compute));
	hipLaunchKernelGGL(k_ld_aggregate_init, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, c->s_compute, d_agg, (unsigned long long)words);
	HIPCHK(c, hipGetLastError());
	c->reduce.map.agg = AggMap{c->d_agg_key, d_agg, x_bins, y_bins, stat};
	call.arm(words * sizeof(unsigned long long));
	rc = call.dispatch(mode, a0, nA, b0, nB, triangle, part, n_parts, tile_variants, window, l_window, n_pairs);
	if (rc) return rc;
	return call.download_slabs("aggregate arrays", d_agg, cells, AGG_CELL_WORDS, std::min<size_t>(cells, (size_t)1 << 18),      // 16 MiB of accumulators at a time
		[&](size_t at, size_t m, const unsigned long long* acc) {
			for (size_t k = 0; k < m; ++k) {
				const unsigned long long* w = acc + k * AGG_CELL_WORDS;
				n[at + k] = w[AGG_W_N];
				sum[at + k] = xs_sum_to_double_signed<AGG_SPLIT>(w[AGG_W_Q_HI], w[AGG_W_Q_LO]);      // (exact in 128 bits, one conversion: ld_exact_sum.h)
				sum_sq[at + k] = xs_sum_to_double_unsigned<AGG_SPLIT>(w[AGG_W_Q2_HI], w[AGG_W_Q2_LO]);
				min[at + k] = w[AGG_W_N] ? xs_value_to_double((long long)w[AGG_W_MIN]) : 0.0;
				max[at + k] = w[AGG_W_N] ? xs_value_to_double((long long)w[AGG_W_MAX]) : 0.0;
			}
		});
}

// Partitioned LD scores: the annotations are checked, packed to n_annot columns and uploaded, the integer accumulators of every
// (variant, category) zeroed in front of the launches, and converted behind the last of them, a slab of variants at a time.
int twk_hip_ld_score_annot(twk_hip_ctx* c, int mode, const twk_hip_filters* f, uint32_t a0, uint32_t nA, uint32_t b0, uint32_t nB, int32_t triangle,
                           uint32_t part, uint32_t n_parts, uint32_t tile_variants, int32_t window, uint32_t l_window,
                           const double* annot, uint32_t n_annot, uint64_t ld_annot, uint64_t* n_partners, double* score, uint64_t* n_pairs) {
	const bool shape_ok = n_annot >= 1 && n_annot <= ANNOT_MAX_CATEGORIES && ld_annot >= n_annot;
	ReduceCall call(c, Reduce::annot, nullptr, f, annot && n_partners && score && shape_ok, mode, a0, nA);
	if (call.bad) return call.bad;
	const size_t M = c->M, C = n_annot, cells = M * C;
	std::vector<double> packed(cells);
	for (size_t v = 0; v < M; ++v)
		for (size_t k = 0; k < C; ++k) {
			const double a = annot[v * ld_annot + k];
			if (!at_valid(a)) {
				snprintf(c->err, sizeof(c->err), "partitioned LD scores: the annotation of variant %zu in column %zu is %g: not finite or beyond 65536 in magnitude", v, k, a);
				return TWK_HIP_E_INVALID;
			}
			packed[v * C + k] = a;
		}
	double* const d_annot = call.hold<double>(cells, "the annotations of %u variants need %zu bytes of device memory: %s", (uint32_t)M);
	unsigned long long* const d_annot_acc = call.hold<unsigned long long>(2 * cells, "the partitioned LD scores of %u variants need %zu bytes of device memory: %s", (uint32_t)M);
	if (call.mem.failed) return call.mem.failed;
	HIPCHK(c, c->d_score_n.reserve(M, M, nullptr));
	// (from pageable memory: the copy has left `packed` when it returns)
	HIPCHK(c, hipMemcpyAsync(d_annot, packed.data(), cells * sizeof(double), hipMemcpyHostToDevice, c->s_compute));
	HIPCHK(c, hipMemsetAsync(d_annot_acc, 0, 2 * cells * sizeof(unsigned long long), c->s_compute));
	HIPCHK(c, hipMemsetAsync(c->d_score_n, 0, M * sizeof(unsigned long long), c->s_compute));
	c->reduce.map.annot = AnnotMap{d_annot, d_annot_acc, c->d_score_n, n_annot};
	call.arm(2 * cells * sizeof(unsigned long long));
	int rc = call.dispatch(mode, a0, nA, b0, nB, triangle, part, n_parts, tile_variants, window, l_window, n_pairs);
	if (rc) return rc;
	rc = call.download("partner counts", [&] { return hipMemcpyAsync(n_partners, c->d_score_n, M * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->s_compute); });
	if (rc) return rc;
	return call.download_slabs("partitioned score arrays", d_annot_acc, cells, 2, std::min<size_t>(cells, (size_t)1 << 20),      // 16 MiB of accumulators at a time
		[&](size_t at, size_t m, const unsigned long long* acc) {
			for (size_t k = 0; k < m; ++k) score[at + k] = xs_sum_to_double_signed<ANNOT_SPLIT>(acc[2 * k], acc[2 * k + 1]);      // (exact in 128 bits, one conversion: ld_exact_sum.h)
		});
}

// ---- sample relationship (ld_relate.hip.h): its own plane set, tile lists, count launches and epilogue, beside the variant launch path ----
extern "C++" {
namespace {
static_assert(sizeof(RelCounts) == sizeof(twk_hip_rel_counts) && sizeof(RelCounts) == 24, "the epilogue stores twk_hip_rel_counts");

struct RelateSuper { uint32_t sa, na, sb, nb; bool diag; CountTable table; size_t table_at = 0; };      // table_at: where the packed table lies in the call's one copy
}  // namespace
}  // extern "C++"

int twk_hip_relationship(twk_hip_ctx* c, const uint32_t* variants, uint32_t n_use, uint32_t sA0, uint32_t nSA, uint32_t sB0, uint32_t nSB,
                         int32_t stat, double fill, double* out, uint64_t ld, twk_hip_rel_counts* counts, uint64_t ld_counts, uint64_t* n_sample_pairs) {
	if (!c || (!out && !counts) || !rl_valid_stat(stat)) return TWK_HIP_E_INVALID;
	if (!c->raw) return TWK_HIP_E_STATE;
	if (nSA == 0 || nSB == 0 || (uint64_t)sA0 + nSA > c->N || (uint64_t)sB0 + nSB > c->N) return TWK_HIP_E_INVALID;
	if ((out && ld < nSB) || (counts && ld_counts < nSB)) return TWK_HIP_E_INVALID;
	if (variants) {
		if (n_use == 0) return TWK_HIP_E_INVALID;
		for (uint32_t k = 0; k < n_use; ++k)
			if (variants[k] >= c->M || (k && variants[k] <= variants[k - 1])) return TWK_HIP_E_INVALID;
	} else n_use = c->M;
	bool any_missing = false;
	for (uint32_t k = 0; k < n_use && !any_missing; ++k) any_missing = c->h_meta[variants ? variants[k] : k].missing != 0;
	if (any_missing && !c->rawmask) return TWK_HIP_E_STATE;
	HIPCHK(c, hipSetDevice(c->device));

	// the plane set: P rows a sample over the variants in use (ld_relate_index.h)
	const uint32_t P = rl_planes(any_missing), W = rl_words(n_use), N = c->N;
	const uint64_t rows_alloc = rl_rows_alloc(N, P), live_rows = (uint64_t)N * P;
	// the call's memory: released when the entry point leaves, behind the wait for its stream - or, on a failure's way out, by frees that
	// wait for the device themselves
	HeldMemory mem(c);
	const char* const what = "sample relationship: %s needs %zu bytes of device memory: %s";
	uint32_t* const d_rows = mem.hold<uint32_t>((size_t)rows_alloc * W, what, "the planes of the samples");
	uint32_t* const d_rowpop = mem.hold<uint32_t>((size_t)rows_alloc, what, "the planes' popcounts");
	uint32_t* const d_ids = variants ? mem.hold<uint32_t>(n_use, what, "the variant list") : nullptr;
	if (mem.failed) return mem.failed;
	if (variants) HIPCHK(c, hipMemcpyAsync(d_ids, variants, (size_t)n_use * 4, hipMemcpyHostToDevice, c->s_compute));
	// (the transposition writes every word of the live rows; the zero rows behind them are set here)
	HIPCHK(c, hipMemsetAsync(d_rows + live_rows * W, 0, (size_t)(rows_alloc - live_rows) * W * 4, c->s_compute));
	HIPCHK(c, hipMemsetAsync(d_rowpop, 0, (size_t)rows_alloc * 4, c->s_compute));
	StageMarks marks;
	HIPCHK(c, marks.mark(0, c->s_compute));      // the report's one stage: the transposition
	{
		const dim3 grid((N + RL_BLOCK_SAMPLES - 1) / RL_BLOCK_SAMPLES, std::min<uint32_t>(W / RL_KC, 65535u)), block(RL_THREADS);
		hipLaunchKernelGGL(k_relate_transpose, grid, block, 0, c->s_compute, (const uint32_t*)c->raw, (const uint32_t*)(any_missing ? c->rawmask.get() : nullptr), c->Wp,
		                   (const uint32_t*)d_ids, n_use, N, P, d_rows, W);
		HIPCHK(c, hipGetLastError());
	}
	HIPCHK(c, marks.mark(StageMarks::NO_STAGE, c->s_compute));
	hipLaunchKernelGGL(k_row_popcount, dim3((unsigned)((live_rows + 3) / 4)), dim3(256), 0, c->s_compute, (const uint32_t*)d_rows, W, (uint32_t)live_rows, d_rowpop);
	HIPCHK(c, hipGetLastError());

	// the super-tiles of the sample-pair space, each with its tile list and unit table (one copy to the device for all of them)
	const bool square = sA0 == sB0 && nSA == nSB;
	const uint32_t S = rl_super_samples(P), nchunks = W / KC, n_blocks = c->resident_blocks;
	std::vector<RelateSuper> supers;
	std::vector<uint32_t> blob;               // per super-tile: its packed table (CountTable::pack)
	CountSettings cs;                         // (one queue of whole-tile units and a guided tail: "seg" and "xcd_queues" are the variant path's)
	cs.patch_rows = (uint32_t)c->opt.patch_rows; cs.patch_cols = (uint32_t)c->opt.patch_cols; cs.min_chunks = (uint32_t)c->opt.count_min_chunks; cs.n_blocks = n_blocks;
	size_t c_words = 0;
	for (uint32_t ia = 0; ia < nSA; ia += S)
		for (uint32_t ib = 0; ib < nSB; ib += S) {
			if (square && ib < ia) continue;
			RelateSuper st{sA0 + ia, std::min(S, nSA - ia), sB0 + ib, std::min(S, nSB - ib), square && ia == ib};
			const twk_hip_tile_desc t{st.sa, st.na, st.sb, st.nb, st.diag ? 1 : 0, 0, 0, 0};
			st.table = build_count_table(t, (int)P, st.diag, nullptr, nchunks, cs);
			st.table_at = blob.size();
			blob.resize(blob.size() + st.table.words());
			st.table.pack(blob.data() + st.table_at);
			c_words = std::max(c_words, (size_t)st.table.g.rowsA * st.table.g.rowsB);
			supers.push_back(std::move(st));
		}
	const size_t cells = (size_t)nSA * nSB;
	uint32_t* const d_C = mem.hold<uint32_t>(c_words, what, "the count matrix of a super-tile");
	uint32_t* const d_lists = mem.hold<uint32_t>(blob.size(), what, "the tile lists");
	uint32_t* const d_tickets = mem.hold<uint32_t>(supers.size() * 8, what, "the work tickets");
	RelateArgs* const d_args = mem.hold<RelateArgs>(supers.size(), what, "the epilogue's parameter blocks");
	unsigned long long* const d_out = out ? mem.hold<unsigned long long>(cells, what, "the matrix") : nullptr;
	RelCounts* const d_counts = counts ? mem.hold<RelCounts>(cells, what, "the counts") : nullptr;
	if (mem.failed) return mem.failed;
	unsigned long long fill_bits; memcpy(&fill_bits, &fill, sizeof(fill_bits));          // any pattern, NaNs included
	std::vector<RelateArgs> args(supers.size());
	for (size_t k = 0; k < supers.size(); ++k) {
		const RelateSuper& st = supers[k];
		RelateArgs& a = args[k];
		a.C = d_C; a.ldc = st.table.g.ldc; a.P = P; a.n_use = n_use; a.rowpop = d_rowpop;
		a.sa = st.sa; a.na = st.na; a.sb = st.sb; a.nb = st.nb;
		a.out_a0 = sA0; a.out_b0 = sB0; a.out_ld = nSB;
		a.diag = st.diag ? 1 : 0; a.mirror = square ? 1 : 0; a.stat = stat; a.fill_bits = fill_bits;
		a.out = d_out; a.counts = d_counts;
	}
	// (from pageable memory: the copies have left `blob` and `args` when they return)
	HIPCHK(c, hipMemcpyAsync(d_lists, blob.data(), blob.size() * 4, hipMemcpyHostToDevice, c->s_compute));
	HIPCHK(c, hipMemcpyAsync(d_args, args.data(), args.size() * sizeof(RelateArgs), hipMemcpyHostToDevice, c->s_compute));
	HIPCHK(c, hipMemsetAsync(d_tickets, 0, supers.size() * 8 * 4, c->s_compute));
	Events ev;                                // per super-tile: the count's begin, its end, the epilogue's end
	HIPCHK(c, ev.add(3 * supers.size()));
	const uint32_t last_halves = c->opt.skip_pad ? count_last_halves(rl_words_live(n_use), W) : 0;
	for (size_t k = 0; k < supers.size(); ++k) {
		const RelateSuper& st = supers[k];
		const CountWork w = count_work(d_rows, W, st.sa * P, st.sb * P, d_lists + st.table_at, st.table, d_C, st.table.g.ldc, d_tickets + k * 8, last_halves, nullptr);
		HIPCHK(c, enqueue_count(c->s_compute, w, st.table, n_blocks, (uint32_t)TILE, ev[3 * k], k_count_list_t<COUNT_NW>));      // (the count's time starts behind the zeroing)
		HIPCHK(c, hipEventRecord(ev[3 * k + 1], c->s_compute));
		hipLaunchKernelGGL(k_relate_epilogue, dim3((st.nb + RL_EP - 1) / RL_EP, (st.na + RL_EP - 1) / RL_EP), dim3(RL_THREADS), 0, c->s_compute, (const RelateArgs*)(d_args + k));
		HIPCHK(c, hipGetLastError());
		HIPCHK(c, hipEventRecord(ev[3 * k + 2], c->s_compute));
	}
	if (out) HIPCHK(c, hipMemcpy2DAsync(out, (size_t)ld * sizeof(double), d_out, (size_t)nSB * sizeof(double), (size_t)nSB * sizeof(double), nSA, hipMemcpyDeviceToHost, c->s_compute));
	if (counts) HIPCHK(c, hipMemcpy2DAsync(counts, (size_t)ld_counts * sizeof(RelCounts), d_counts, (size_t)nSB * sizeof(RelCounts), (size_t)nSB * sizeof(RelCounts), nSA, hipMemcpyDeviceToHost, c->s_compute));
	HIPCHK(c, hipStreamSynchronize(c->s_compute));
	c->last.relate = CallReport();
	c->last.relate.bytes = (uint64_t)rows_alloc * W * 4;
	c->last.relate_planes = (int32_t)P;
	marks.write(c->last.relate);
	float ms = 0;
	for (size_t k = 0; k < supers.size(); ++k) {
		if (hipEventElapsedTime(&ms, ev[3 * k], ev[3 * k + 1]) == hipSuccess) c->timing.count_ms += ms;
		if (hipEventElapsedTime(&ms, ev[3 * k + 1], ev[3 * k + 2]) == hipSuccess) c->timing.stats_ms += ms;
		c->timing.count_launches += 1; c->timing.stats_launches += 1;
		c->timing.row_pairs += (uint64_t)supers[k].table.n_tiles() * TILE * TILE;
	}
	if (n_sample_pairs) *n_sample_pairs = square ? (uint64_t)nSA * (nSA + 1) / 2 : (uint64_t)nSA * nSB;
	return TWK_HIP_OK;
}

int twk_hip_relationship_last(const twk_hip_ctx* c, int32_t* planes_per_sample, double* transpose_ms, uint64_t* plane_bytes) {
	if (c && planes_per_sample) *planes_per_sample = c->last.relate_planes;
	return last_of(c, &LastCalls::relate, {transpose_ms}, plane_bytes);
}

int twk_hip_shard_rows(uint32_t n_rows, uint32_t n_cols, int32_t triangle, uint32_t part, uint32_t n_parts,
                       uint32_t* row_begin, uint32_t* row_end, uint64_t* n_pairs) {
	if (n_parts == 0 || part >= n_parts || n_rows == 0 || n_cols == 0 || (triangle && n_rows != n_cols)) return TWK_HIP_E_INVALID;
	const uint32_t r0 = band_boundary(part, n_parts, n_rows, n_cols, triangle != 0);
	const uint32_t r1 = band_boundary(part + 1, n_parts, n_rows, n_cols, triangle != 0);
	if (row_begin) *row_begin = r0;
	if (row_end) *row_end = r1;
	if (n_pairs) *n_pairs = band_pairs_before(r1, n_rows, n_cols, triangle != 0) - band_pairs_before(r0, n_rows, n_cols, triangle != 0);
	return TWK_HIP_OK;
}

int twk_hip_plan_region(const twk_hip_plan_env* pe, const twk_hip_variant_meta* meta, const uint32_t* popc, uint32_t n_variants,
                        uint32_t a0, uint32_t nA, uint32_t b0, uint32_t nB, int32_t triangle, uint32_t part, uint32_t n_parts,
                        uint32_t tile_variants, int32_t window, uint32_t l_window,
                        twk_hip_tile_desc* tiles, uint32_t capacity, uint32_t* n_tiles, uint32_t* n_band_launches,
                        uint32_t* row_begin, uint32_t* row_end, uint64_t* n_pairs, uint32_t* lo, uint32_t* hi) {
	return twk_hip_plan_region_two(pe, meta, popc, nullptr, nullptr, 0.0, n_variants, a0, nA, b0, nB, triangle, part, n_parts, tile_variants, window, l_window,
	                               tiles, capacity, n_tiles, n_band_launches, row_begin, row_end, n_pairs, lo, hi, nullptr);
}
int twk_hip_plan_region_two(const twk_hip_plan_env* pe, const twk_hip_variant_meta* meta, const uint32_t* popc, const uint32_t* het, const uint32_t* hom, double two_margin,
                            uint32_t n_variants, uint32_t a0, uint32_t nA, uint32_t b0, uint32_t nB, int32_t triangle, uint32_t part, uint32_t n_parts,
                            uint32_t tile_variants, int32_t window, uint32_t l_window,
                            twk_hip_tile_desc* tiles, uint32_t capacity, uint32_t* n_tiles, uint32_t* n_band_launches,
                            uint32_t* row_begin, uint32_t* row_end, uint64_t* n_pairs, uint32_t* lo, uint32_t* hi, uint32_t* two_end) {
	return twk_hip_plan_region_two_operand(pe, meta, popc, het, hom, two_margin, 0, n_variants, a0, nA, b0, nB, triangle, part, n_parts, tile_variants, window, l_window,
	                                       tiles, capacity, n_tiles, n_band_launches, row_begin, row_end, n_pairs, lo, hi, two_end);
}
int twk_hip_plan_region_two_operand(const twk_hip_plan_env* pe, const twk_hip_variant_meta* meta, const uint32_t* popc, const uint32_t* het, const uint32_t* hom, double two_margin,
                                    int32_t carrier, uint32_t n_variants, uint32_t a0, uint32_t nA, uint32_t b0, uint32_t nB, int32_t triangle, uint32_t part, uint32_t n_parts,
                                    uint32_t tile_variants, int32_t window, uint32_t l_window,
                                    twk_hip_tile_desc* tiles, uint32_t capacity, uint32_t* n_tiles, uint32_t* n_band_launches,
                                    uint32_t* row_begin, uint32_t* row_end, uint64_t* n_pairs, uint32_t* lo, uint32_t* hi, uint32_t* two_end) {
	return twk_hip_plan_region_two_form(pe, meta, popc, het, hom, two_margin, carrier, 0, 0, n_variants, a0, nA, b0, nB, triangle, part, n_parts, tile_variants, window, l_window,
	                                    tiles, capacity, n_tiles, n_band_launches, row_begin, row_end, n_pairs, lo, hi, two_end);
}
int twk_hip_plan_region_two_form(const twk_hip_plan_env* pe, const twk_hip_variant_meta* meta, const uint32_t* popc, const uint32_t* het, const uint32_t* hom, double two_margin,
                                 int32_t carrier, int32_t one, uint32_t one_rows, uint32_t n_variants, uint32_t a0, uint32_t nA, uint32_t b0, uint32_t nB, int32_t triangle, uint32_t part, uint32_t n_parts,
                                 uint32_t tile_variants, int32_t window, uint32_t l_window,
                                 twk_hip_tile_desc* tiles, uint32_t capacity, uint32_t* n_tiles, uint32_t* n_band_launches,
                                 uint32_t* row_begin, uint32_t* row_end, uint64_t* n_pairs, uint32_t* lo, uint32_t* hi, uint32_t* two_end) {
	return twk_hip_plan_region_walk(pe, meta, popc, het, hom, two_margin, carrier, one, one_rows, 0, n_variants, a0, nA, b0, nB, triangle, part, n_parts, tile_variants, window, l_window,
	                                tiles, capacity, n_tiles, n_band_launches, row_begin, row_end, n_pairs, lo, hi, two_end, nullptr, nullptr, nullptr);
}
int twk_hip_plan_region_walk(const twk_hip_plan_env* pe, const twk_hip_variant_meta* meta, const uint32_t* popc, const uint32_t* het, const uint32_t* hom, double two_margin,
                             int32_t carrier, int32_t one, uint32_t one_rows, int32_t fine, uint32_t n_variants, uint32_t a0, uint32_t nA, uint32_t b0, uint32_t nB, int32_t triangle, uint32_t part, uint32_t n_parts,
                             uint32_t tile_variants, int32_t window, uint32_t l_window,
                             twk_hip_tile_desc* tiles, uint32_t capacity, uint32_t* n_tiles, uint32_t* n_band_launches,
                             uint32_t* row_begin, uint32_t* row_end, uint64_t* n_pairs, uint32_t* lo, uint32_t* hi, uint32_t* two_end,
                             uint32_t* two_last, uint8_t* notes, uint32_t* stair) {
	if ((het != nullptr) != (hom != nullptr)) return TWK_HIP_E_INVALID;
	if (!pe || !meta || !n_tiles || (capacity && !tiles) || n_parts == 0 || part >= n_parts) return TWK_HIP_E_INVALID;
	if (nA == 0 || nB == 0 || (uint64_t)a0 + nA > n_variants || (uint64_t)b0 + nB > n_variants) return TWK_HIP_E_INVALID;
	if (triangle && (a0 != b0 || nB < nA)) return TWK_HIP_E_INVALID;
	if (pe->screen && (!popc || !triangle)) return TWK_HIP_E_INVALID;
	if (pe->planes_per_variant < 1 || pe->planes_per_variant > 3 || pe->n_samples == 0) return TWK_HIP_E_INVALID;
	PlanEnv env;
	env.n_samples = pe->n_samples; env.Pmax = pe->planes_per_variant; env.nchunks = std::max<uint32_t>(pe->k_chunks, 1); env.resident_blocks = std::max<uint32_t>(pe->resident_blocks, 1);
	env.screen = pe->screen; env.minR2 = pe->minR2; env.fused = pe->fused != 0; env.phased_math = pe->phased_math != 0;
	env.meta = meta; env.ids = nullptr; env.popc = popc;
	env.het = het; env.hom = hom; if (two_margin > 0) env.two_margin = two_margin;
	env.carrier = carrier != 0 && het != nullptr;
	env.one = env.carrier && one != 0 && pe->minR2 > 1e-6 && pe->minR2 <= 1.0; env.one_rows = one_rows;
	env.fine = fine != 0 && env.carrier;
	env.band_launch = pe->band_launch != 0; env.band_reverse = pe->band_reverse != 0; env.band_work_log2 = pe->band_work_log2; env.band_max_launches = std::max<long long>(pe->band_max_launches, 1);
	const PlanGeom g{a0, nA, b0, nB, triangle, part, n_parts, tile_variants, window, l_window};
	RegionPlan plan;
	plan_region(env, g, plan);
	*n_tiles = (uint32_t)plan.mine.size();
	if (n_band_launches) *n_band_launches = (uint32_t)plan.bands.size();
	if (row_begin) *row_begin = plan.r0;
	if (row_end) *row_end = plan.r1;
	if (n_pairs) *n_pairs = plan.pairs;
	if (two_end) *two_end = plan.two_end;
	if (two_last) *two_last = plan.two_last;
	if (stair) for (uint32_t r = 0; r < nA; ++r) stair[r] = r < plan.stair.size() ? plan.stair[r] : 0;
	if (notes) for (size_t i = 0; i < plan.mine.size() && i < capacity; ++i) notes[i] = (uint8_t)(plan.notes[i].side | (plan.notes[i].behind ? 4 : 0));
	if (plan.windowed) {
		if (lo) std::copy(plan.lo.begin(), plan.lo.end(), lo);
		if (hi) std::copy(plan.hi.begin(), plan.hi.end(), hi);
	}
	if (plan.mine.size() > capacity) return TWK_HIP_E_OVERFLOW;
	std::copy(plan.mine.begin(), plan.mine.end(), tiles);
	return TWK_HIP_OK;
}

// Fisher's exact test on caller-supplied tables, through the same kernels the pair math uses.
__global__ void k_tables_to_records(const int32_t* __restrict__ t, unsigned long long n, twk_hip_record* __restrict__ r) {
	const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	twk_hip_record x{};
	x.idxA = 0; x.idxB = 1;
	x.cnt[0] = t[4 * i]; x.cnt[2] = t[4 * i + 1]; x.cnt[1] = t[4 * i + 2]; x.cnt[3] = t[4 * i + 3];      // n12 rides in the REFALT slot (ld_engine.cpp:1222-1226)
	r[i] = x;
}
__global__ void k_records_to_p(const twk_hip_record* __restrict__ r, unsigned long long n, double* __restrict__ p) {
	const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) p[i] = r[i].P;
}

int twk_hip_fisher_exact(twk_hip_ctx* c, const int32_t* tables, uint64_t n, double* p_two_sided, int32_t in_given_order, float* kernel_ms) {
	if (!c || !tables || !p_two_sided || n == 0 || n > (1ull << 28)) return TWK_HIP_E_INVALID;
	if (!c->d_lfact) return TWK_HIP_E_STATE;
	HIPCHK(c, hipSetDevice(c->device));
	DevBuf<int32_t> d_t; DevBuf<twk_hip_record> d_r; DevBuf<double> d_p; DevBuf<unsigned long long> d_n;
	Events ev;
	hipError_t e = d_t.reserve((size_t)n * 4, (size_t)n * 4, nullptr);
	if (e == hipSuccess) e = d_r.reserve(n, n, nullptr);
	if (e == hipSuccess) e = d_p.reserve(n, n, nullptr);
	if (e == hipSuccess) e = d_n.reserve(4, 4, nullptr);
	if (e == hipSuccess) e = ev.add(2);
	const unsigned long long counters[4] = {n, 0, 0, 0};
	if (e == hipSuccess) e = hipMemcpyAsync(d_t, tables, (size_t)n * 16, hipMemcpyHostToDevice, c->s_compute);
	if (e == hipSuccess) e = hipMemcpyAsync(d_n, counters, sizeof(counters), hipMemcpyHostToDevice, c->s_compute);
	if (e == hipSuccess) {
		hipLaunchKernelGGL(k_tables_to_records, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->s_compute, d_t, (unsigned long long)n, d_r);
		e = hipEventRecord(ev[0], c->s_compute);
	}
	if (e == hipSuccess) {
		// as the engine runs it (walk-length order; the table buffer is free: the tables are in the records by now), or in the order given
		const int rc = launch_fisher(c, d_r, d_n, (unsigned long long)n, 2.0, in_given_order ? nullptr : (uint32_t*)d_t.get(), (size_t)n * 4);
		if (rc) return rc;
		e = hipEventRecord(ev[1], c->s_compute);
	}
	if (e == hipSuccess) {
		hipLaunchKernelGGL(k_records_to_p, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->s_compute, d_r, (unsigned long long)n, d_p);
		e = hipMemcpyAsync(p_two_sided, d_p, (size_t)n * 8, hipMemcpyDeviceToHost, c->s_compute);
	}
	if (e == hipSuccess) e = hipStreamSynchronize(c->s_compute);
	if (e == hipSuccess) e = hipGetLastError();
	if (e == hipSuccess && kernel_ms) e = hipEventElapsedTime(kernel_ms, ev[0], ev[1]);
	HIPCHK(c, e);
	return TWK_HIP_OK;
}

int twk_hip_set_device_sink(twk_hip_ctx* c, int on) {
	if (!c) return TWK_HIP_E_INVALID;
	c->device_sink = on != 0;
	c->d_keep_n = 0;
	return TWK_HIP_OK;
}

int twk_hip_device_records(twk_hip_ctx* c, const twk_hip_record** records, uint64_t* n) {
	if (!c || !records || !n) return TWK_HIP_E_INVALID;
	if (!c->device_sink) return TWK_HIP_E_STATE;
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->s_copy));
	*records = c->d_keep_n ? c->d_keep : nullptr;
	*n = c->d_keep_n;
	return TWK_HIP_OK;
}

// ---- the gather of a one-process multi-GPU run: device sink -> device sink over RCCL ------------------------------------------------
// (north star: "a final RCCL gather of .two output blocks over xGMI"; the reference's counterpart is every slave's flush of its output
// block into the shared writer, lib/ld/ld_engine.cpp:1742-1802).  librccl is opened when the first gather asks for it - a process that
// never gathers, or a box without RCCL, loses nothing - and one communicator clique per set of devices is kept for the life of the process.
extern "C++" {
namespace {
struct Rccl {
	void* lib = nullptr; bool tried = false; char why[256] = {0}; int version = 0;
	ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
	ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
	ncclResult_t (*GroupStart)() = nullptr;
	ncclResult_t (*GroupEnd)() = nullptr;
	ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
	ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
	ncclResult_t (*GetVersion)(int*) = nullptr;
	const char* (*GetErrorString)(ncclResult_t) = nullptr;
	std::map<std::vector<int>, std::vector<ncclComm_t>> cliques;
	std::mutex mu;
	bool open() {
		if (tried) return lib != nullptr;
		tried = true;
		// RCCL 2.27 prints a banner (its version, HIP's, the host name, its own path) to STDOUT when the first communicator comes up, unless
		// NCCL_DEBUG says NONE: a `tomahawk calc` whose stdout is somebody's pipe must not grow five lines.  Left alone if the caller set it.
		(void)setenv("NCCL_DEBUG", "NONE", 0);
		for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) { lib = dlopen(name, RTLD_NOW | RTLD_LOCAL); if (lib) break; }
		if (!lib) { snprintf(why, sizeof(why), "librccl.so.1 cannot be opened: %s", dlerror()); return false; }
		auto sym = [&](const char* n) { void* p = dlsym(lib, n); if (!p) snprintf(why, sizeof(why), "librccl lacks %s", n); return p; };
		CommInitAll = (decltype(CommInitAll))sym("ncclCommInitAll"); CommDestroy = (decltype(CommDestroy))sym("ncclCommDestroy");
		GroupStart = (decltype(GroupStart))sym("ncclGroupStart"); GroupEnd = (decltype(GroupEnd))sym("ncclGroupEnd");
		Send = (decltype(Send))sym("ncclSend"); Recv = (decltype(Recv))sym("ncclRecv");
		GetVersion = (decltype(GetVersion))sym("ncclGetVersion"); GetErrorString = (decltype(GetErrorString))sym("ncclGetErrorString");
		if (!(CommInitAll && CommDestroy && GroupStart && GroupEnd && Send && Recv && GetVersion && GetErrorString)) { dlclose(lib); lib = nullptr; return false; }
		(void)GetVersion(&version);
		return true;
	}
};
Rccl& rccl() { static Rccl r; return r; }
}  // namespace
}  // extern "C++"

const char* twk_hip_gather_backend(void) {
	Rccl& r = rccl();
	std::lock_guard<std::mutex> lk(r.mu);
	static char text[320];
	if (r.open()) snprintf(text, sizeof(text), "rccl %d", r.version);
	else snprintf(text, sizeof(text), "unavailable (%s)", r.why);
	return text;
}

int twk_hip_gather_records(twk_hip_ctx* const* ctxs, uint32_t n, uint32_t dst, int32_t flags, uint64_t* n_records, double* transfer_ms) {
	if (!ctxs || n == 0 || dst >= n) return TWK_HIP_E_INVALID;
	for (uint32_t r = 0; r < n; ++r) {
		if (!ctxs[r]) return TWK_HIP_E_INVALID;
		if (!ctxs[r]->device_sink) return TWK_HIP_E_STATE;
		for (uint32_t q = 0; q < r; ++q) if (ctxs[q]->device == ctxs[r]->device) return TWK_HIP_E_INVALID;      // one context per GPU: RCCL refuses a device twice
	}
	twk_hip_ctx* d = ctxs[dst];
	const bool loop = n == 1 && (flags & TWK_HIP_GATHER_SELF_LOOP);
	if (n_records) *n_records = d->d_keep_n;
	if (transfer_ms) *transfer_ms = 0.0;
	if (n == 1 && !loop) return TWK_HIP_OK;
	Rccl& rc = rccl();
	std::lock_guard<std::mutex> lk(rc.mu);
	if (!rc.open()) { snprintf(d->err, sizeof(d->err), "RCCL gather: %s", rc.why); return TWK_HIP_E_DEVICE; }
	auto NCHK = [&](ncclResult_t e, const char* what) -> int {
		if (e == ncclSuccess) return TWK_HIP_OK;
		snprintf(d->err, sizeof(d->err), "RCCL gather: %s failed: %s", what, rc.GetErrorString(e));
		return TWK_HIP_E_DEVICE;
	};
	std::vector<int> devs(n);
	for (uint32_t r = 0; r < n; ++r) devs[r] = ctxs[r]->device;
	auto it = rc.cliques.find(devs);
	if (it == rc.cliques.end()) {
		std::vector<ncclComm_t> comms(n);
		if (const int e = NCHK(rc.CommInitAll(comms.data(), (int)n, devs.data()), "ncclCommInitAll")) return e;
		it = rc.cliques.emplace(devs, std::move(comms)).first;
	}
	const std::vector<ncclComm_t>& comm = it->second;
	// every context's survivors are final (their copies ran on the contexts' copy streams): counts on the host, room on the destination
	unsigned long long total = 0;
	std::vector<unsigned long long> cnt(n), off(n);
	for (uint32_t r = 0; r < n; ++r) { HIPCHK(d, hipSetDevice(ctxs[r]->device)); HIPCHK(d, hipStreamSynchronize(ctxs[r]->s_copy)); cnt[r] = ctxs[r]->d_keep_n; }
	off[dst] = 0; total = cnt[dst];
	for (uint32_t r = 0; r < n; ++r) if (r != dst) { off[r] = total; total += cnt[r]; }
	HIPCHK(d, hipSetDevice(d->device));
	DevBuf<twk_hip_record> loop_buf;          // (freed on every way out, unless it became the sink)
	if (loop) {          // one GPU: the same group of ncclSend / ncclRecv, from the sink to itself through a second buffer (what a one-GPU box can show of the path)
		HIPCHK(d, loop_buf.reserve(cnt[0], cnt[0], nullptr));
	} else {
		const unsigned long long own = d->d_keep_n;
		d->d_keep_n = own;
		const int e = ensure_device_keep(d, total - own); if (e) return e;         // (keeps the destination's own records, at the front)
	}
	Events ev;
	HIPCHK(d, ev.add(2));
	HIPCHK(d, hipEventRecord(ev[0], d->s_copy));
	int rcode = NCHK(rc.GroupStart(), "ncclGroupStart");
	for (uint32_t r = 0; r < n && !rcode; ++r) {
		if (!loop && r == dst) continue;
		const size_t bytes = (size_t)cnt[r] * sizeof(twk_hip_record);
		if (!bytes) continue;
		if (hipSetDevice(ctxs[r]->device) != hipSuccess) { rcode = TWK_HIP_E_DEVICE; break; }
		rcode = NCHK(rc.Send(ctxs[r]->d_keep.get(), bytes, ncclUint8, (int)dst, comm[r], ctxs[r]->s_copy), "ncclSend");
		if (rcode) break;
		if (hipSetDevice(d->device) != hipSuccess) { rcode = TWK_HIP_E_DEVICE; break; }
		rcode = NCHK(rc.Recv(loop ? loop_buf.get() : d->d_keep + off[r], bytes, ncclUint8, (int)r, comm[dst], d->s_copy), "ncclRecv");
	}
	{ const int e = NCHK(rc.GroupEnd(), "ncclGroupEnd"); if (!rcode) rcode = e; }
	(void)hipSetDevice(d->device);
	if (!rcode && hipEventRecord(ev[1], d->s_copy) != hipSuccess) rcode = TWK_HIP_E_DEVICE;
	for (uint32_t r = 0; r < n && !rcode; ++r) {
		if (hipSetDevice(ctxs[r]->device) != hipSuccess || hipStreamSynchronize(ctxs[r]->s_copy) != hipSuccess) rcode = TWK_HIP_E_DEVICE;
	}
	(void)hipSetDevice(d->device);
	float ms = 0;
	if (!rcode && hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess && transfer_ms) *transfer_ms = ms;
	if (rcode) { if (!d->err[0]) snprintf(d->err, sizeof(d->err), "RCCL gather: a HIP call failed"); return rcode; }
	if (loop) {
		if (loop_buf) d->d_keep = std::move(loop_buf);        // the records that went round are the sink's content from here on
	} else {
		d->d_keep_n = total;
		for (uint32_t r = 0; r < n; ++r) if (r != dst) ctxs[r]->d_keep_n = 0;
	}
	if (n_records) *n_records = d->d_keep_n;
	return TWK_HIP_OK;
}

int twk_hip_drain_device_sink(twk_hip_ctx* c, twk_hip_record_sink sink, void* user, uint64_t* n_records) {
	if (!c || !sink) return TWK_HIP_E_INVALID;
	if (!c->device_sink) return TWK_HIP_E_STATE;
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->s_copy));
	const unsigned long long n = c->d_keep_n;
	if (n_records) *n_records = n;
	const int rc = n ? deliver_records(c, c->d_keep, n, sink, user, c->s_copy, 0.0) : TWK_HIP_OK;
	c->d_keep_n = 0;
	return rc;
}

int twk_hip_set_option(twk_hip_ctx* c, const char* key, int64_t value) {
	if (!c || !key) return TWK_HIP_E_INVALID;
	for (const OptionKey& k : OPTION_KEYS) {
		if (std::strcmp(k.name, key) != 0) continue;
		if (value < k.lo || value > k.hi) { snprintf(c->err, sizeof(c->err), "option %s: %lld is outside [%lld, %lld]", key, (long long)value, k.lo, k.hi); return TWK_HIP_E_INVALID; }
		if (c->opt.*(k.field) == value) return TWK_HIP_OK;
		c->opt.*(k.field) = value;
		if (k.rebuilds_planes && c->raw) {       // the carrier lists belong to the allele-count-sorted sets: rebuilt on next use
			HIPCHK(c, hipSetDevice(c->device));
			HIPCHK(c, hipDeviceSynchronize());
			free_planes(c);
		}
		return TWK_HIP_OK;
	}
	snprintf(c->err, sizeof(c->err), "unknown option %s", key);
	return TWK_HIP_E_INVALID;
}

int twk_hip_option_describe(uint32_t index, const char** key, int64_t* dflt, int64_t* lo, int64_t* hi, const char** meaning) {
	if (index >= sizeof(OPTION_KEYS) / sizeof(OPTION_KEYS[0])) return TWK_HIP_E_INVALID;
	const OptionKey& k = OPTION_KEYS[index];
	if (key) *key = k.name;
	if (dflt) *dflt = k.dflt;
	if (lo) *lo = k.lo;
	if (hi) *hi = k.hi;
	if (meaning) *meaning = k.doc;
	return TWK_HIP_OK;
}

int twk_hip_get_option(const twk_hip_ctx* c, const char* key, int64_t* value) {
	if (!c || !key || !value) return TWK_HIP_E_INVALID;
	for (const OptionKey& k : OPTION_KEYS)
		if (std::strcmp(k.name, key) == 0) { *value = c->opt.*(k.field); return TWK_HIP_OK; }
	return TWK_HIP_E_INVALID;
}

int twk_hip_set_progress(twk_hip_ctx* c, twk_hip_progress_cb cb, void* user) {
	if (!c) return TWK_HIP_E_INVALID;
	c->progress_cb = cb; c->progress_user = user;
	return TWK_HIP_OK;
}

int twk_hip_launch_log(twk_hip_ctx* c, twk_hip_launch_stat* out, uint32_t capacity, uint32_t* n_copied, uint64_t* n_total) {
	if (!c || (capacity && !out)) return TWK_HIP_E_INVALID;
	const size_t have = c->launch_ring.size(), n = std::min<size_t>(have, capacity);
	// oldest first: the ring's write position is launches_seen % LAUNCH_RING once it has wrapped
	const size_t start = have < LAUNCH_RING ? 0 : (size_t)(c->launches_seen % LAUNCH_RING);
	for (size_t k = 0; k < n; ++k) out[k] = c->launch_ring[(start + (have - n) + k) % have];
	if (n_copied) *n_copied = (uint32_t)n;
	if (n_total) *n_total = c->launches_seen;
	return TWK_HIP_OK;
}

int twk_hip_timing_reset(twk_hip_ctx* c) {
	if (!c) return TWK_HIP_E_INVALID;
	c->launch_ring.clear(); c->launches_seen = 0;
	const uint64_t w = c->timing.words_per_row;
	c->timing = twk_hip_timing{};
	c->timing.words_per_row = w;
	return TWK_HIP_OK;
}

int twk_hip_timing_get(twk_hip_ctx* c, twk_hip_timing* out) {
	if (!c || !out) return TWK_HIP_E_INVALID;
	*out = c->timing;
	// words contracted per row pair: live words of whichever plane set was used last
	for (const auto& p : c->planes) if (p.built) out->words_per_row = p.W_live;
	return TWK_HIP_OK;
}

}  // extern "C"
