// The form of a count launch - which contraction, which math behind it - and who may take which: what a launch is (LaunchForm), what its
// owner allows it (FormGrant), what the plan, the filters and the options fix (FormFacts), what the running call has not yet given up
// (CallForms), what a launch's owner wants for it (LaunchWants), the numbers that call a launch or its sample poor or rich in candidates, and the
// samples that decide the wants of a region's launches (decide_wants).  Host-only, no HIP: twk_hip.hip's launch_form gathers the facts and calls
// decide_form(), its RegionRun gathers the ladder's facts, runs the samples decide_wants() asks for and keeps the wants;
// csrc/tools/form_check.cpp plays every combination on the host (make form-check, tests/test_form_cpu.py).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "../../../include/twk_hip.h"

namespace twk {

// The epilogue that stands in for math, Fisher, sort and delivery while a call of twk_hip_ld_score, _prune, _clump, _matrix, _decay, _aggregate, _score_annot, _matrix_band or _topk runs: it looks at
// every pair of a count matrix and keeps no survivor (ld_reduce.hip.h on what the nine kernels share).
enum class Reduce { none, score, prune, clump, matrix, decay, aggregate, annot, bandmat, topk, dprime_ci, blocks };      // (dprime_ci and blocks: one epilogue, two calls)
constexpr int N_REDUCE = (int)Reduce::blocks + 1;
// The form of a launch, decided once (decide_form) and passed down: which count kernel, which math behind it.
struct LaunchForm {
	bool two_pass = false;         // a default-mode tile with missing data: a second (masked unphased) pass follows; the form describes the first
	bool fused = false;            // the fused count -> screen kernel: no count matrix, C holds the candidate list
	bool unphased = false;         // plain unphased planes with UnphasedMath: the list math, if there is one, is the unphased kernel
	bool three = false;            // the three-product form (HH + S; the candidates' four products are recounted): fused, or ...
	bool three_plain() const { return three && !fused; }      // ... through a count matrix (long rows): C holds the (HH, S) matrix and, behind it, the candidate list
	bool uz = false;               // a three_plain() launch whose matrix holds (U, Z) = (popc(H_A | H_B), popc((Q_A ^ Q_B) & ~(H_A | H_B))) in (HH, S)'s place - two popcounts a
	                               // word for three (ld_count_uz.hip.h); its screen converts (ld_two_screen.h: uz_to_hh_s).  An attribute of three_plain(), never set with `fused`
	bool two = false;              // the two-product form (HH + HQ through a count matrix, S bounded from the margins): never fused, never with `three`
	bool keep_three = false;       // option three = 2: whatever a launch's candidate density
	bool sample = false;           // a density sample (decide_wants below): its count kernel runs under its own name (k_count3_list_t<.., 1>), so that a
	                               // kernel trace's statistics of the real launches are not diluted by half-millisecond ones
	bool carrier = false;          // a two-product launch whose row operand is the carrier plane H | Q (CH + CQ in place of HH + HQ; ld_two_screen.h): an attribute of
	                               // `two`, never set without it
	bool one = false;              // a carrier launch that contracts one product a pair - the carrier rows on both axes, CC = CH + CQ - and whose screen's lower test
	                               // stands at S >= 0 (ld_two_screen.h: screen1c_*): an attribute of `two && carrier`, never set without them
	bool prefix = false;           // a two- or three-product launch through a matrix whose tiles are contracted over a prefix of their rows (per-tile stops)
	Reduce reduce = Reduce::none;  // the epilogue in place of math, Fisher and records (launch_reduce): always through a matrix
	bool reduces() const { return reduce != Reduce::none; }      // ... the launch looks at every pair and keeps no survivor: no screen, no Fisher test, no sort
};
inline bool operator==(const LaunchForm& a, const LaunchForm& b) {
	return a.two_pass == b.two_pass && a.fused == b.fused && a.unphased == b.unphased && a.three == b.three && a.uz == b.uz && a.two == b.two && a.keep_three == b.keep_three &&
	       a.sample == b.sample && a.carrier == b.carrier && a.one == b.one && a.prefix == b.prefix && a.reduce == b.reduce;
}

// Rows of at most this many K chunks (32 words each: N <= 65,536 phased, N <= 131,072 unphased) take the fused
// count -> screen kernel.  Up to 16 chunks a tile is never worth splitting, and the C round trip plus the
// one-thread-per-pair math front end cost as much as the counting itself.  Beyond that a fused launch ends less evenly
// (a block must hold a pair's whole count to screen it, so the last tiles cannot be cut along K: +2..6 % count kernel at
// 40-118 chunks) but still saves several times that in the math kernel (tests/sweeps/fused_mid_n.sh,
// profiles/r03_fused_mid_n.txt: N = 60,000 -p, 4e4 variants: 46 + 15 ms -> 49 + 2.5 ms); the two meet near 220 chunks.
constexpr uint32_t FUSED_MAX_CHUNKS = 128;

// What the owner of a launch allows it: `two` only where the two-product walk's owner says so for this launch (RegionRun, on the sorted set).
// `prefix`: an attribute of such a launch's two- or three-product form, not a form of its own - stops for its tiles, where the owner's sample allows them.
// `carrier`: the owner holds carrier rows for this launch's row variants (carrier_operand below) - the row operand of its two-product form, if it takes it.
// `one`: the walk's owner planned this launch in front of its rows' one_end (ld_plan.h) and holds carrier rows for its column variants too.
struct FormGrant { bool fused = true, three = true, two = false, sample = false, prefix = false, carrier = false, one = false; };
// What the owner of a launch wants for it, before the call has its say (CallForms::grant): three products unless the launch's sample was dense
// in candidates; two products, stops and one product where its sample in that form was poor in them (decide_wants below), or where an option
// forces them; `carrier` where the owner holds carrier rows for the region's two-product launches.
struct LaunchWants { bool three = true, two = false, prefix = false, carrier = false, one = false; };
// What the tile plan, the filters and the options fix, whoever grants what.
struct FormFacts {
	bool two_pass = false;
	bool phased_plain = false, unphased_plain = false;      // PhasedMath on plain phased planes (one count per pair) / UnphasedMath on plain unphased planes
	Reduce reduce = Reduce::none;
	bool cut_screens = false;                               // an r2 cut-off a screen can use: minR2 > 1e-6 && minR2 <= 1
	uint32_t chunks = 0;                                    // K chunks of a row (read only where a launch may fuse)
	bool sorted_u = false;                                  // the set is PS_SORTED_U
	long long opt_fused = 1, opt_three = 1, opt_two = 1, opt_prefix = 1, opt_carrier = 1, opt_one = 1, opt_uz = 1;
	uint32_t row_chunks = 0;                                // K chunks of a row (read only where a launch is granted the prefix)
	uint32_t carrier_chunks = 0;                            // K chunks of a row (read only where a launch is granted the carrier plane)
};
// The row operand of a call's two-product launches: the carrier plane where option "carrier" allows it, the rows are longer than the fused form
// ever takes - shorter ones gain little and the third plane is not worth its memory - and carrier rows for the row variants [0, rows_need) of the
// walk are there.  rows_have < rows_need: they could not be allocated - the H plane as before, and no error.
inline bool carrier_operand(long long opt_carrier, uint32_t row_chunks, uint32_t rows_have, uint32_t rows_need) {
	return opt_carrier != 0 && row_chunks > FUSED_MAX_CHUNKS && rows_need > 0 && rows_have >= rows_need;
}
// A screen in front of the math needs plain phased planes with PhasedMath, or plain unphased planes (four products per pair, gathered in the
// epilogue) with UnphasedMath, and an r2 cut-off the screen can use.  Such a launch fuses when its rows are short enough that no tile's K
// range is split (option fused = 2: never split; 0: never fuse), and takes the three-product form (ld_count.hip.h) on unphased planes - or,
// where it is granted, two products in place of three through a matrix.
inline bool may_screen(const FormFacts& x, const FormGrant& g) { return x.reduce == Reduce::none && g.fused && (x.phased_plain || x.unphased_plain) && x.cut_screens; }
inline LaunchForm decide_form(const FormFacts& x, const FormGrant& g) {
	LaunchForm lf;
	lf.two_pass = x.two_pass; lf.reduce = x.reduce; lf.keep_three = x.opt_three == 2; lf.unphased = x.unphased_plain; lf.sample = g.sample;
	if (!may_screen(x, g)) return lf;
	lf.three = lf.unphased && g.three && x.opt_three != 0;
	lf.fused = x.opt_fused != 0 && (x.opt_fused == 2 || x.chunks <= FUSED_MAX_CHUNKS);
	if (lf.three && !lf.fused && !lf.two_pass && x.sorted_u && g.two && x.opt_two != 0) { lf.two = true; lf.three = false; }
	lf.uz = lf.three_plain() && x.opt_uz != 0;      // (the same launch, samples included: what it costs, not what it keeps)
	lf.carrier = lf.two && g.carrier && x.opt_carrier != 0 && x.carrier_chunks > FUSED_MAX_CHUNKS;
	lf.one = lf.carrier && g.one && x.opt_one != 0;
	// the prefix: only the matrix forms of the sorted walk, and only on rows the fused form never takes by policy - whatever "fused" is set to
	lf.prefix = g.prefix && x.opt_prefix != 0 && (lf.two || lf.three_plain()) && !lf.two_pass && x.sorted_u && x.row_chunks > FUSED_MAX_CHUNKS;
	return lf;
}
// The ladder: what the tile of a launch whose candidate list overflowed may be when it is redone - a two-product launch's with three products
// (if it was granted them), a fused or three-product launch's with four products through a matrix.
// A prefix launch's is redone over whole rows in the same product form; a one-product launch's in the carrier two-product form.
inline FormGrant step_down(const LaunchForm& was, FormGrant given) {
	if (was.prefix) { given.prefix = false; return given; }
	if (was.one) { given.one = false; return given; }
	if (!was.two) given.fused = given.three = false;
	given.two = given.carrier = given.one = false;
	return given;
}

// What the running call has not yet given up: a region call owns one for all its stages, the single-tile entry a fresh one.
struct CallForms {
	bool fused = true, three = true, two = true, prefix = true, one = true;
	bool two_behind = true;      // the two-product launches behind the walk's cut (below: behind_wants, behind_overflowed)
	// ... what a launch behind the cut may still want
	LaunchWants behind_wants(LaunchWants w) const { if (!two_behind) w.two = w.one = false; return w; }
	// ... such a launch, of form `was` under `given`, whose candidate list overflowed: the call gives up those launches and no other form, and the tile is
	// redone with three products over whole rows -> the grant of that
	FormGrant behind_overflowed(FormGrant given) {
		two_behind = false;
		given.two = given.carrier = given.one = given.prefix = false;
		return given;
	}
	// ... and allows a launch, whose owner wants three / two products for it (and stops for its tiles)
	// (the carrier plane is no form of the call's to give up: it goes where the two-product form goes)
	// (one product is: a launch that overflows or is too rich in that form ends it for the call, and nothing else)
	FormGrant grant(const LaunchWants& w) const {
		FormGrant g;
		g.fused = fused; g.three = three && w.three; g.two = two && w.two; g.sample = false; g.prefix = prefix && w.prefix;
		g.carrier = g.two && w.carrier; g.one = one && g.carrier && w.one;
		return g;
	}
	// ... a density sample in the form `w` (decide_wants): three products granted - a sample is only taken where the call allows them; and its own
	// overflow or richness decides its launch, not the call
	FormGrant sample_grant(const LaunchWants& w) const { FormGrant g = grant(w); g.three = true; g.sample = true; return g; }
	// ... a tile that is redone synchronously under `given` (run_tile_sync), narrowed by what the call has given up since: over whole rows - never
	// the prefix - and a two-product tile keeps its row operand, and its one product
	FormGrant redo_grant(const FormGrant& given) const {
		LaunchWants w; w.three = given.three; w.two = given.two; w.carrier = given.carrier; w.one = given.one;
		FormGrant g = grant(w);
		g.fused = g.fused && given.fused; g.sample = given.sample;
		return g;
	}
	// A launch of form `was`, given `given`, is through: a list that overflowed (cand_overflow) or held more candidates than the recount is worth
	// (too_rich) ends the form for the rest of the call - but a form the launch was not given is not taken from the call on its account.
	void gave_up(const LaunchForm& was, const FormGrant& given, bool cand_overflow, bool too_rich) {
		// (a prefix launch's overflow - and its richness in candidates, which the wider screen of its stops makes - is the stops' doing: either ends
		// the prefix for the call, the two-product rule, and no product form: the launches behind it are judged over whole rows again)
		if (was.prefix) { if (cand_overflow || too_rich) prefix = false; return; }
		if (was.one) { if (cand_overflow || too_rich) one = one && !given.one; return; }
		if (cand_overflow && was.two) two = two && !given.two;
		if (cand_overflow && (was.fused || was.three)) { fused = fused && !given.fused; three = three && !given.three; }
		if (too_rich && was.three && !was.keep_three) three = three && !given.three;
	}
};

// ---- the two-product launches behind the walk's cut (the fine walk; ld_plan.h LaunchNote::behind) --------------------------------------------------
// A form of the call's of its own: a refused sample or an overflowing list of such a launch ends them for the rest of the call, and nothing else - the
// launches in front of the cut keep their two products.  CallForms::two_behind holds it; behind(i): launch i is one of them.
// ... after the samples (decide_wants, option two = 1): a launch behind the cut whose own sample did not leave it two products -> true: none of them takes it
template <class Behind>
bool behind_refused(const std::vector<LaunchWants>& wants, Behind behind) {
	for (size_t i = 0; i < wants.size(); ++i) if (behind(i) && !wants[i].two) return true;
	return false;
}

// ---- the numbers that decide a launch's fate, side by side ---------------------------------------------------------------------------------
// A sample is poor in candidates - its launch takes the form the sample ran in - if at most 1 pair in `one_in` of it is a candidate ...
constexpr bool sample_poor(unsigned long long cand, unsigned long long pairs, unsigned long long one_in) { return cand * one_in <= pairs; }
// ... 1 in 256: the two- and one-product samples, the samples with stops and the three-product sample of a launch through a matrix
constexpr unsigned long long SAMPLE_ONE_IN = 256;
// ... 1 in 128: the three-product sample of a fused launch, whose recount reads short rows from L2.  (Fused launches - short rows - keep their
// candidates whatever their number, but past ~1.2 % of the pairs the recount costs more than the third product saves: 2,504 samples, -u -w 1000000,
// 2.9 % candidates: 27.4 + 30.3 ms of count kernel and math with three products in the first of two launches, 30 + 21 ms with four in both.)
constexpr unsigned long long SAMPLE_ONE_IN_THREE_FUSED = 128;
// The candidate list of a two- or three-product launch through a matrix (enqueue_tile): room for at most 1/128 of the tile's pairs - a candidate's
// recount streams its four rows once more, ~25 pairs' worth of contraction, so a launch with more candidates than that is cheaper in the
// four-product form (overflow -> CallForms::gave_up -> redone).
inline unsigned long long cand_list_entries(unsigned long long pairs) { return std::max<unsigned long long>(pairs / 128, 4096); }
// A three-product launch this rich in candidates pays more for their recount than the fourth product costs: the rest of the call in the
// four-product forms (finish_tile -> Launch::too_rich -> CallForms::gave_up).  Measured at 2,504 samples, -u -w 1000000 (2.9 % of the pairs
// candidates): count kernel 32.1 -> 27.3 ms, but 58 M recounts at 0.16 ns each (four 320-byte rows from L2 per candidate: 8 TB/s) add 9.3 ms to the
// math; the two meet near 1.2 %.  (Against the variant pairs of the tiles the launch contracted - four plane-row pairs each - not the launch's
// rectangle: a window launch's rectangle is mostly outside the window.)
inline bool three_too_rich(unsigned long long cand, unsigned long long row_pairs) { return cand > std::max<unsigned long long>(row_pairs / 4 / 128, 4096); }
// A one-product launch with more candidates than its sample was allowed (1 pair in 256): its list held, so its records stand, but the wider screen
// is not paying here - the launches behind it keep two products (CallForms::gave_up takes `one` from the call and nothing else).
inline bool one_too_rich(unsigned long long cand, unsigned long long pairs) { return cand > std::max<unsigned long long>(pairs / 256, 4096); }

// ---- the sample ladder: what the owner of a region's launches wants for each ------------------------------------------------------------------
// The three-product form through a count matrix (long rows) pays only where candidates are few: a launch whose list overflows is redone with four
// products, three-product launches already in flight behind it included (1 M x 50,000 cohort run, calc -u: 977 -> 1,426 ms of count kernel with
// three such launches wasted), and how many pairs are candidates differs from launch to launch - in allele-count order the launches over the common
// variants hold nearly all of them.  So every launch is decided by a sample of its own, taken before the pipeline starts (ld_plan.h:
// sample_subtile), three products unless the sample is dense in candidates.  Regions of more than 64 launches sample every k-th one; the others
// follow their nearest sampled neighbour.
// The two-product walk: a launch in front of the planner's cut is sampled in the two-product form first - two products if that sample is poor in
// candidates - and only if that fails in the three-product form (those launches lead the plan and are sampled one by one: the neighbour across the
// cut says nothing).  A launch the planner marked for one product is sampled in that form first; refused, it is sampled again as any other launch
// in front of the cut.  The prefix: the same samples, first with the stops the launch would use - poor in candidates and the launch takes the form
// with its stops; otherwise the rungs behind decide without them.
struct SampleOutcome { int rc = TWK_HIP_OK; unsigned long long cand = 0, pairs = 1; };      // rc: TWK_HIP_OK, TWK_HIP_E_OVERFLOW (the sample's list), or an error that ends the call
struct LadderFacts {
	long long opt_two = 1, opt_three = 1, opt_prefix = 1, opt_one = 1;
	bool prefix_ok = false;           // the region's launches may take stops (the walk's long rows, their suffix margins there, the call still allows them)
	bool one_ok = false;              // ... and one product (the planner marked launches for it, carrier rows for their columns are there, the call still allows it)
	bool three_possible = false;      // some launch of the region would take three products (none: nothing to sample)
	bool fused = false;               // the region's launches fuse
	bool carrier = false;             // the region's two-product launches contract the carrier plane: wanted for every launch, and for every sample
	// The fine walk's plan (ld_plan.h plan_two_stairs) has two-eligible launches behind the cut, between three-product ones: such a launch is sampled by
	// itself wherever it lies - a step of several launches ends in front of it - so that none is left to follow a neighbour in another form.
	bool eligible_interleaved = false;
};
// two_eligible(i): launch i lies in front of the walk's cut (option two = 2: every launch of the walk); planned_one(i): the planner marked it for one
// product; sample(pick, as) runs launch pick's sample in the form `as` (CallForms::sample_grant) -> SampleOutcome; mark(what, i, x): the timeline log.
// -> TWK_HIP_OK with a LaunchWants per launch in `out`, or the error of the sample that ended the call.
template <class Eligible, class PlannedOne, class Sample, class Mark>
int decide_wants(size_t n, const LadderFacts& x, Eligible two_eligible, PlannedOne planned_one, Sample sample, Mark mark, std::vector<LaunchWants>& out, uint32_t& one_refused) {
	LaunchWants unsampled; unsampled.carrier = x.carrier;
	out.assign(n, unsampled);
	if (x.one_ok) for (size_t i = 0; i < n; ++i) out[i].one = planned_one(i) && two_eligible(i);      // (taken back below where a launch's sample says so)
	if (x.opt_two == 2) for (size_t i = 0; i < n; ++i) out[i].two = two_eligible(i);
	if (x.prefix_ok && x.opt_prefix == 2) for (size_t i = 0; i < n; ++i) out[i].prefix = true;
	if (n == 0 || x.opt_three != 1 || !x.three_possible) return TWK_HIP_OK;
	const unsigned long long dense_one_in = x.fused ? SAMPLE_ONE_IN_THREE_FUSED : SAMPLE_ONE_IN;
	size_t n_front = 0;
	if (x.opt_two == 1) while (n_front < n && two_eligible(n_front)) ++n_front;
	const size_t step_behind = std::max<size_t>(1, (n - n_front + 63) / 64);
	auto own_sample = [&](size_t i) { return x.eligible_interleaved && x.opt_two == 1 && two_eligible(i); };
	for (size_t i0 = 0, step = 1; i0 < n; i0 += step) {
		step = (i0 < n_front || own_sample(i0)) ? 1 : step_behind;
		for (size_t k = i0 + 1; k < i0 + step && k < n; ++k) if (own_sample(k)) { step = k - i0; break; }
		const size_t pick = std::min(n - 1, i0 + step / 2), i1 = std::min(n, i0 + step);
		const bool front = x.opt_two == 1 && two_eligible(pick), try_two = front || (x.opt_two == 2 && out[pick].two);
		LaunchWants as = unsampled; as.one = out[pick].one;
		int err = TWK_HIP_OK;
		// one rung: the sample in the form `as` (with two products and / or stops), its line in the timeline -> poor in candidates?
		auto poor = [&](bool two, bool prefix, const char* what, unsigned long long one_in) -> bool {
			as.two = two; as.prefix = prefix;
			const SampleOutcome o = sample(pick, as);
			if (o.rc != TWK_HIP_OK && o.rc != TWK_HIP_E_OVERFLOW) { err = o.rc; return false; }
			mark(what, pick, o.cand);
			return o.rc == TWK_HIP_OK && sample_poor(o.cand, o.pairs, one_in);
		};
		// the rungs in front of the three-product one: with stops (the whole step follows), then two products (the sampled launch alone)
		auto cheaper_form = [&]() -> bool {
			if (x.prefix_ok && x.opt_prefix == 1) {
				if (poor(try_two, true, as.one ? "one-product prefix sample of launch: candidates" : "prefix sample of launch: candidates", SAMPLE_ONE_IN)) {
					for (size_t i = i0; i < i1; ++i) { out[i].prefix = true; if (try_two && two_eligible(i)) out[i].two = true; }
					return true;
				}
				if (err) return false;
			}
			if (front && poor(true, false, as.one ? "one-product sample of launch: candidates" : "two-product sample of launch: candidates", SAMPLE_ONE_IN)) {
				out[pick].two = true;      // (three products stay wanted: what a launch falls back to)
				return true;
			}
			return false;
		};
		bool decided = cheaper_form();
		if (!decided && !err && as.one && x.opt_one == 1) {      // one product refused: the step's launches without it, and the same rungs again
			as.one = false; ++one_refused;
			for (size_t i = i0; i < i1; ++i) out[i].one = false;
			decided = cheaper_form();
		}
		if (err) return err;
		if (decided) continue;
		// (dense: the sample's own list overflowed, or more than 1 pair in dense_one_in is a candidate)
		const bool dense = !poor(false, false, "three-product sample of launch: candidates", dense_one_in);
		if (err) return err;
		for (size_t i = i0; i < i1; ++i) out[i].three = !dense;
	}
	return TWK_HIP_OK;
}

}  // namespace twk
