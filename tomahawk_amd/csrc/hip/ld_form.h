// The form of a count launch - which contraction, which math behind it - and who may take which: what a launch is (LaunchForm), what its
// owner allows it (FormGrant), what the plan, the filters and the options fix (FormFacts), what the running call has not yet given up
// (CallForms).  Host-only, no HIP: twk_hip.hip's launch_form gathers the facts and calls decide_form(); csrc/tools/form_check.cpp plays every
// combination on the host (make form-check, tests/test_form_cpu.py).
#pragma once
#include <stdint.h>

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
	bool two = false;              // the two-product form (HH + HQ through a count matrix, S bounded from the margins): never fused, never with `three`
	bool keep_three = false;       // option three = 2: whatever a launch's candidate density
	bool sample = false;           // a density sample (RegionRun::decide_three_by_samples): its count kernel runs under its own name (k_count3_list_t<.., 1>), so that a
	                               // kernel trace's statistics of the real launches are not diluted by half-millisecond ones
	bool carrier = false;          // a two-product launch whose row operand is the carrier plane H | Q (CH + CQ in place of HH + HQ; ld_two_screen.h): an attribute of
	                               // `two`, never set without it
	bool one = false;              // a carrier launch that contracts one product a pair - the carrier rows on both axes, CC = CH + CQ - and whose screen's lower test
	                               // stands at S >= 0 (ld_two_screen.h: screen1c_*): an attribute of `two && carrier`, never set without them
	bool prefix = false;           // a two- or three-product launch through a matrix whose tiles are contracted over a prefix of their rows (per-tile stops)
	Reduce reduce = Reduce::none;  // the epilogue in place of math, Fisher and records (launch_reduce): always through a matrix
	bool reduces() const { return reduce != Reduce::none; }      // ... the launch looks at every pair and keeps no survivor: no screen, no Fisher test, no sort
};

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
// What the tile plan, the filters and the options fix, whoever grants what.
struct FormFacts {
	bool two_pass = false;
	bool phased_plain = false, unphased_plain = false;      // PhasedMath on plain phased planes (one count per pair) / UnphasedMath on plain unphased planes
	Reduce reduce = Reduce::none;
	bool cut_screens = false;                               // an r2 cut-off a screen can use: minR2 > 1e-6 && minR2 <= 1
	uint32_t chunks = 0;                                    // K chunks of a row (read only where a launch may fuse)
	bool sorted_u = false;                                  // the set is PS_SORTED_U
	long long opt_fused = 1, opt_three = 1, opt_two = 1, opt_prefix = 1, opt_carrier = 1, opt_one = 1;
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
	// ... and allows a launch, whose owner wants three / two products for it (and stops for its tiles)
	// (the carrier plane is no form of the call's to give up: it goes where the two-product form goes)
	// (one product is: a launch that overflows or is too rich in that form ends it for the call, and nothing else)
	FormGrant grant(bool want_three, bool want_two, bool want_prefix = false, bool want_carrier = false, bool want_one = false) const {
		return FormGrant{fused, three && want_three, two && want_two, false, prefix && want_prefix, two && want_two && want_carrier, one && two && want_two && want_carrier && want_one};
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

}  // namespace twk
