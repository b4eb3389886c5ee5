// `make form-check`: who may take which form of a count launch (csrc/hip/ld_form.h), on the CPU under AddressSanitizer and UBSan.
//   1. decide_form over every combination of FormFacts x FormGrant: no two forms that exclude each other, a reducing launch in no form but
//      four products through a matrix, every form only on the planes, under the grants and with the options it needs, and no grant whose
//      withdrawal adds a form - but grant.two, which turns two products into three.
//   2. CallForms::gave_up: the transitions a launch's outcome makes in what the call still allows, one by one, that a form the launch was not
//      granted is never taken from the call, and that a second telling changes nothing; step_down, the ladder a redone tile descends.
//   3. CallForms::grant, sample_grant and redo_grant against the expressions they replaced; the thresholds at their edges; the samples' sub-tile.
//   4. decide_wants, the sample ladder, under scripted samplers: its invariants over every option, fact, plan length and outcome, and named scripts
//      whose samples and wants are written out.
#include <algorithm>
#include <cstdio>
#include <initializer_list>
#include <string>
#include <vector>
#include "../hip/ld_form.h"
#include "../hip/ld_plan.h"

using namespace twk;

namespace {

int g_bad_checks = 0;
long g_cases = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_bad_checks < 40) { fprintf(stderr, "    FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } ++g_bad_checks; } } while (0)

// (two forms are the same when every field of LaunchForm is: operator== in ld_form.h)
enum { G_FUSED = 1, G_THREE = 2, G_TWO = 4, G_SAMPLE = 8, G_PREFIX = 16, G_CARRIER = 32, G_ONE = 64, G_ALL_BITS = 128 };
FormGrant grant_of(int bits) {
	FormGrant g;
	g.fused = (bits & G_FUSED) != 0; g.three = (bits & G_THREE) != 0; g.two = (bits & G_TWO) != 0; g.sample = (bits & G_SAMPLE) != 0;
	g.prefix = (bits & G_PREFIX) != 0; g.carrier = (bits & G_CARRIER) != 0; g.one = (bits & G_ONE) != 0;
	return g;
}
enum { W_THREE = 1, W_TWO = 2, W_PREFIX = 4, W_CARRIER = 8, W_ONE = 16, W_ALL_BITS = 32 };
LaunchWants wants_of(int bits) {
	LaunchWants w;
	w.three = (bits & W_THREE) != 0; w.two = (bits & W_TWO) != 0; w.prefix = (bits & W_PREFIX) != 0; w.carrier = (bits & W_CARRIER) != 0; w.one = (bits & W_ONE) != 0;
	return w;
}
bool same_grant(const FormGrant& a, const FormGrant& b) {
	return a.fused == b.fused && a.three == b.three && a.two == b.two && a.sample == b.sample && a.prefix == b.prefix && a.carrier == b.carrier && a.one == b.one;
}

std::vector<FormFacts> all_facts() {
	std::vector<FormFacts> out;
	for (int two_pass = 0; two_pass < 2; ++two_pass)
	for (int planes = 0; planes < 3; ++planes)                        // neither, phased math on plain phased planes, unphased math on plain unphased planes
	for (const Reduce reduce : {Reduce::none, Reduce::score, Reduce::annot})
	for (int cut = 0; cut < 2; ++cut)
	for (const uint32_t chunks : {0u, 1u, FUSED_MAX_CHUNKS, FUSED_MAX_CHUNKS + 1, 4000u})
	for (int sorted_u = 0; sorted_u < 2; ++sorted_u)
	for (int f = 0; f < 3; ++f) for (int t3 = 0; t3 < 3; ++t3) for (int t2 = 0; t2 < 3; ++t2) {
		FormFacts x;
		x.two_pass = two_pass != 0; x.phased_plain = planes == 1; x.unphased_plain = planes == 2; x.reduce = reduce; x.cut_screens = cut != 0;
		x.chunks = chunks; x.sorted_u = sorted_u != 0; x.opt_fused = f; x.opt_three = t3; x.opt_two = t2;
		out.push_back(x);
	}
	return out;
}

void check_decide_form() {
	for (const FormFacts& x : all_facts()) for (int gb = 0; gb < 16; ++gb) {
		const FormGrant g = grant_of(gb);
		const LaunchForm lf = decide_form(x, g);
		++g_cases;
		CHECK(!(lf.two && (lf.three || lf.fused || lf.two_pass)), "two products with another form (grant %d)", gb);
		CHECK(!(lf.reduces() && (lf.fused || lf.three || lf.two)), "a reducing launch in a screened form (grant %d)", gb);
		CHECK(lf.reduce == x.reduce && lf.two_pass == x.two_pass && lf.unphased == x.unphased_plain && lf.keep_three == (x.opt_three == 2), "a fact not carried over");
		CHECK(!(lf.three || lf.two) || x.unphased_plain, "three or two products off the plain unphased planes");
		CHECK(!lf.three || (g.three && g.fused && x.opt_three != 0), "three products without their grants or with the option off");
		CHECK(!lf.two || (x.sorted_u && g.two && g.three && g.fused && x.opt_two != 0 && x.opt_three != 0), "two products without the sorted set, their grants or their options");
		CHECK(!lf.fused || (g.fused && x.opt_fused != 0 && (x.opt_fused == 2 || x.chunks <= FUSED_MAX_CHUNKS)), "fused against the option or on rows too long");
		CHECK(!(lf.fused || lf.three || lf.two) || (x.cut_screens && (x.phased_plain || x.unphased_plain)), "a screen without a cut-off or planes it can use");
		CHECK(lf.sample == g.sample, "the sample mark");
		// withdrawing a grant adds no form (two -> three excepted), and grant.sample changes nothing but the mark
		for (int bit = 0; bit < 4; ++bit) {
			if (!(gb & (1 << bit))) continue;
			const LaunchForm less = decide_form(x, grant_of(gb & ~(1 << bit)));
			if (bit == 3) { LaunchForm marked = less; marked.sample = true; CHECK(marked == lf, "grant.sample changed the form"); continue; }
			CHECK(!(less.fused && !lf.fused), "withdrawing grant %d added the fused form", bit);
			CHECK(!(less.two && !lf.two), "withdrawing grant %d added two products", bit);
			if (less.three && !lf.three) CHECK(bit == 2 && lf.two && !less.two, "withdrawing grant %d added three products", bit);
			if (bit == 2 && !(less == lf)) CHECK(lf.two && !less.two && less.three && !lf.three && less.fused == lf.fused, "withdrawing grant.two did more than turn two products into three");
		}
	}
}

LaunchForm form_of(bool fused, bool three, bool two, bool keep_three = false) { LaunchForm lf; lf.unphased = three || two; lf.fused = fused; lf.three = three; lf.two = two; lf.keep_three = keep_three; return lf; }
bool is(const CallForms& c, bool fused, bool three, bool two) { return c.fused == fused && c.three == three && c.two == two; }

void check_gave_up() {
	const FormGrant all = grant_of(G_FUSED | G_THREE | G_TWO);
	const LaunchForm two = form_of(false, false, true), fused4 = form_of(true, false, false), fused3 = form_of(true, true, false), three = form_of(false, true, false),
	                 four = form_of(false, false, false), kept3 = form_of(true, true, false, true);
	{ CallForms c; c.gave_up(two, all, true, false); CHECK(is(c, true, true, false), "a two-product list overflowed"); }
	for (const LaunchForm& lf : {fused4, fused3, three}) { CallForms c; c.gave_up(lf, all, true, false); CHECK(is(c, false, false, true), "a fused or three-product list overflowed"); }
	for (const LaunchForm& lf : {fused3, three}) { CallForms c; c.gave_up(lf, all, false, true); CHECK(is(c, true, false, true), "a launch too rich in candidates"); }
	{ CallForms c; c.gave_up(kept3, all, false, true); CHECK(is(c, true, true, true), "option three = 2 keeps the form"); }
	{ CallForms c; c.gave_up(four, all, false, false); c.gave_up(fused3, all, false, false); c.gave_up(two, all, false, false); CHECK(is(c, true, true, true), "nothing happened"); }
	// every outcome of every form under every grant, from every state of the call: nothing comes back, nothing not granted is taken, twice is once
	for (int fb = 0; fb < 16; ++fb) for (int gb = 0; gb < 8; ++gb) for (int ob = 0; ob < 4; ++ob) for (int cb = 0; cb < 8; ++cb) {
		const LaunchForm lf = form_of((fb & 1) != 0, (fb & 2) != 0, (fb & 4) != 0, (fb & 8) != 0);
		if (lf.two && (lf.three || lf.fused)) continue;
		const FormGrant g = grant_of(gb);
		CallForms before; before.fused = (cb & 1) != 0; before.three = (cb & 2) != 0; before.two = (cb & 4) != 0;
		CallForms c = before;
		c.gave_up(lf, g, (ob & 1) != 0, (ob & 2) != 0);
		++g_cases;
		CHECK((!c.fused || before.fused) && (!c.three || before.three) && (!c.two || before.two), "a form came back");
		CHECK((c.fused == before.fused || g.fused) && (c.three == before.three || g.three) && (c.two == before.two || g.two), "a form that was not granted was taken from the call");
		if (!ob) CHECK(is(c, before.fused, before.three, before.two), "a launch that went well changed the call");
		CallForms again = c;
		again.gave_up(lf, g, (ob & 1) != 0, (ob & 2) != 0);
		CHECK(is(again, c.fused, c.three, c.two), "not idempotent");
		// what the call then grants a launch is no more than it still holds
		const FormGrant next = c.grant(wants_of(W_THREE | W_TWO));
		CHECK(next.fused == c.fused && next.three == c.three && next.two == c.two && !next.sample, "grant");
		CHECK(!c.grant(wants_of(W_TWO)).three && !c.grant(wants_of(W_THREE)).two, "grant beyond what the owner wants");
	}
	// the ladder: two -> three (if granted) -> four through the matrix; fused or three -> four through the matrix
	{ const FormGrant g = step_down(two, all); CHECK(g.fused && g.three && !g.two, "below two products"); }
	for (const LaunchForm& lf : {fused4, fused3, three}) { const FormGrant g = step_down(lf, all); CHECK(!g.fused && !g.three && !g.two, "below a fused or three-product launch"); }
	{ FormGrant s = all; s.sample = true; CHECK(step_down(three, s).sample, "the sample mark stays"); }
	// the prefix: an attribute of a two- or three-product launch through a matrix.  Its overflow ends the prefix for the call and
	// no product form, and the tile is redone over whole rows in the same product form; a launch without it never touches it.
	FormGrant with_prefix = all; with_prefix.prefix = true;
	for (LaunchForm lf : {two, three}) {
		lf.prefix = true;
		{ CallForms c; c.gave_up(lf, with_prefix, true, false); CHECK(is(c, true, true, true) && !c.prefix, "a prefix launch's list overflowed"); }
		{ CallForms c; c.gave_up(lf, with_prefix, false, false); CHECK(is(c, true, true, true) && c.prefix, "a prefix launch went well"); }
		const FormGrant g = step_down(lf, with_prefix);
		CHECK(!g.prefix && g.fused == with_prefix.fused && g.three == with_prefix.three && g.two == with_prefix.two, "below a prefix launch: the same product form over whole rows");
		CallForms gone; gone.prefix = false;
		CHECK(!gone.grant(wants_of(W_THREE | W_TWO | W_PREFIX)).prefix && CallForms().grant(wants_of(W_THREE | W_TWO | W_PREFIX)).prefix && !CallForms().grant(wants_of(W_THREE | W_TWO)).prefix, "prefix grants");
	}
	{ LaunchForm lf = three; lf.prefix = true; CallForms c; c.gave_up(lf, with_prefix, false, true); CHECK(is(c, true, true, true) && !c.prefix, "a three-product prefix launch too rich in candidates: the stops go, the form stays"); }
	{ LaunchForm lf = three; lf.prefix = true; CallForms c; c.gave_up(lf, with_prefix, true, true); CHECK(is(c, true, true, true) && !c.prefix, "a flooded prefix launch is rich by its stops: the form stays"); }
	for (const LaunchForm& lf : {two, fused4, fused3, three, four}) for (int ob = 0; ob < 4; ++ob) { CallForms c; c.gave_up(lf, all, (ob & 1) != 0, (ob & 2) != 0); CHECK(c.prefix, "a launch without stops took the prefix from the call"); }
	// decide_form: only with the grant, the option, the sorted set, a matrix form of two or three products and rows beyond the fused form's policy
	for (const FormFacts& x0 : all_facts()) for (const uint32_t rc : {0u, FUSED_MAX_CHUNKS, FUSED_MAX_CHUNKS + 1}) for (int op = 0; op < 3; ++op) for (int gp = 0; gp < 2; ++gp) for (int gt = 0; gt < 2; ++gt) {
		FormFacts x = x0; x.row_chunks = rc; x.opt_prefix = op;
		FormGrant g; g.two = gt != 0; g.prefix = gp != 0;
		const LaunchForm lf = decide_form(x, g);
		FormGrant g0 = g; g0.prefix = false;
		const LaunchForm base = decide_form(x, g0);
		++g_cases;
		CHECK(lf.fused == base.fused && lf.three == base.three && lf.two == base.two && lf.two_pass == base.two_pass, "the prefix grant changed the product form");
		CHECK(!base.prefix, "a prefix without its grant");
		CHECK(lf.prefix == (gp && op != 0 && rc > FUSED_MAX_CHUNKS && x.sorted_u && !lf.two_pass && (lf.two || lf.three_plain())), "prefix: grant %d option %d chunks %u", gp, op, rc);
	}
}

// The carrier plane as the row operand of a two-product launch: an attribute of `two` - the rung of the ladder where the two-product
// form sits, with rows of its own.
void check_carrier() {
	// decide_form: only with the grant, the option, rows beyond the fused form's policy and a launch that takes two products; it changes nothing else
	for (const FormFacts& x0 : all_facts()) for (const uint32_t cc : {0u, FUSED_MAX_CHUNKS, FUSED_MAX_CHUNKS + 1}) for (int oc = 0; oc < 2; ++oc) for (int gc = 0; gc < 2; ++gc) for (int gt = 0; gt < 2; ++gt)
	for (int gp = 0; gp < 2; ++gp) {
		FormFacts x = x0; x.carrier_chunks = cc; x.row_chunks = cc; x.opt_carrier = oc;
		FormGrant g; g.two = gt != 0; g.carrier = gc != 0; g.prefix = gp != 0;
		const LaunchForm lf = decide_form(x, g);
		FormGrant g0 = g; g0.carrier = false;
		const LaunchForm base = decide_form(x, g0);
		++g_cases;
		// (every field is compared now: the carrier grant changes `carrier`, which is its purpose, and nothing else - the check used to pass because `carrier` was not looked at)
		{ LaunchForm but_carrier = lf; but_carrier.carrier = false; CHECK(but_carrier == base, "the carrier grant changed more than the row operand"); }
		CHECK(!base.carrier, "a carrier launch without its grant");
		CHECK(lf.carrier == (gc && oc != 0 && cc > FUSED_MAX_CHUNKS && lf.two), "carrier: grant %d option %d chunks %u two %d", gc, oc, cc, (int)lf.two);
		CHECK(!lf.carrier || (lf.two && !lf.three && !lf.fused && !lf.two_pass && x.sorted_u), "a carrier launch that is no two-product launch of the sorted walk");
	}
	// the ladder: a carrier launch whose list overflowed is redone with three products, and the call's two-product launches end - as the H form's;
	// a prefix launch on carrier rows is redone over whole rows on the same rows
	FormGrant all = grant_of(G_FUSED | G_THREE | G_TWO | G_CARRIER);
	LaunchForm two; two.unphased = true; two.two = true; two.carrier = true;
	{ const FormGrant g = step_down(two, all); CHECK(g.fused && g.three && !g.two && !g.carrier, "below a carrier launch: three products"); }
	{ CallForms c; c.gave_up(two, all, true, false); CHECK(c.fused && c.three && !c.two && c.prefix, "a carrier launch's list overflowed: no more two-product launches"); CHECK(!c.grant(wants_of(W_THREE | W_TWO | W_CARRIER)).carrier && !c.grant(wants_of(W_THREE | W_TWO | W_CARRIER)).two, "... and none on carrier rows"); }
	{ CallForms c; c.gave_up(two, all, false, false); CHECK(c.two && c.grant(wants_of(W_THREE | W_TWO | W_CARRIER)).carrier, "a carrier launch went well"); }
	{ LaunchForm lf = two; lf.prefix = true; FormGrant wp = all; wp.prefix = true; const FormGrant g = step_down(lf, wp); CHECK(!g.prefix && g.two && g.carrier, "below a carrier prefix launch: whole rows, same operand");
	  CallForms c; c.gave_up(lf, wp, true, false); CHECK(c.two && !c.prefix, "a carrier prefix launch's list overflowed: the stops go"); }
	CHECK(!CallForms().grant(wants_of(W_THREE | W_CARRIER)).carrier && !CallForms().grant(wants_of(W_THREE | W_TWO)).carrier && CallForms().grant(wants_of(W_THREE | W_TWO | W_CARRIER)).carrier, "carrier grants follow the two-product grant");
	g_cases += 6;
	// the row operand of a call (carrier_operand): the option, rows beyond the fused form's, and carrier rows for every row in front of the cut - rows that
	// could not be allocated (have 0 < need) leave the H plane, and a call with nothing in front of its cut asks for none
	// (the answers are written out, not restated: option, chunks of a row, rows held, rows needed -> carrier plane?)
	static const struct { long long opt; uint32_t chunks, have, need; bool carrier; const char* what; } CASES[] = {
		{1, 977, 18304, 18304, true,  "the headline: every row in front of the cut has its carrier row"},
		{1, 977, 50000, 18304, true,  "rows left by an earlier call with a later cut"},
		{1, 129, 128, 128, true,      "the shortest rows that take the form"},
		{1, 977, 0, 18304, false,     "an allocation that failed: the H plane"},
		{1, 977, 12544, 18304, false, "rows for an earlier cut only: the H plane"},
		{1, 977, 18304, 0, false,     "a shard with no row in front of the cut asks for none"},
		{1, 977, 0, 0, false,         "nothing held, nothing needed"},
		{0, 977, 18304, 18304, false, "option carrier = 0"},
		{1, 128, 18304, 18304, false, "rows of 128 chunks keep the H plane"},
		{1, 40, 18304, 18304, false,  "rows of 40 chunks keep the H plane"},
		{1, 1, 128, 128, false,       "rows of one chunk keep the H plane"},
	};
	for (const auto& k : CASES) { ++g_cases; CHECK(carrier_operand(k.opt, k.chunks, k.have, k.need) == k.carrier, "carrier_operand(%lld, %u, %u, %u): %s", k.opt, k.chunks, k.have, k.need, k.what); }
}

// The (U, Z) form: an attribute of a three-product launch through a matrix - what the launch counts, not what it keeps - chosen by option
// "uz" alone: no grant, no sample and no rung of the ladder knows it.
void check_uz() {
	for (const FormFacts& x0 : all_facts()) for (const uint32_t cc : {1u, FUSED_MAX_CHUNKS, FUSED_MAX_CHUNKS + 1}) for (int ou = 0; ou < 2; ++ou) for (int gbits = 0; gbits < 128; ++gbits) {
		FormFacts x = x0; x.chunks = cc; x.carrier_chunks = cc; x.row_chunks = cc; x.opt_uz = ou;
		FormGrant g; g.fused = (gbits & 1) != 0; g.three = (gbits & 2) != 0; g.two = (gbits & 4) != 0; g.sample = (gbits & 8) != 0; g.prefix = (gbits & 16) != 0; g.carrier = (gbits & 32) != 0; g.one = (gbits & 64) != 0;
		const LaunchForm lf = decide_form(x, g);
		FormFacts x_off = x; x_off.opt_uz = 0;
		const LaunchForm base = decide_form(x_off, g);
		++g_cases;
		{ LaunchForm but_uz = lf; but_uz.uz = false; CHECK(but_uz == base, "option uz changed more than what a three-product launch counts"); }
		CHECK(!base.uz, "a (U, Z) launch with option uz = 0");
		CHECK(lf.uz == (ou != 0 && lf.three && !lf.fused), "uz: option %d three %d fused %d", ou, (int)lf.three, (int)lf.fused);
		CHECK(!lf.uz || (lf.three_plain() && lf.unphased && !lf.two && !lf.carrier && !lf.one && !lf.reduces()), "a (U, Z) launch that is no three-product launch through a matrix");
		{ LaunchForm other = lf; other.uz = !other.uz; CHECK(!(other == lf), "operator== does not look at uz"); }
	}
	// the ladder does not know the form: what a flooded or rich (U, Z) launch gives up and steps down to is the three-product launch's
	FormGrant all = grant_of(G_FUSED | G_THREE | G_TWO);
	LaunchForm three; three.unphased = true; three.three = true;
	LaunchForm uz = three; uz.uz = true;
	for (int ob = 0; ob < 4; ++ob) {
		CallForms a, b; a.gave_up(three, all, (ob & 1) != 0, (ob & 2) != 0); b.gave_up(uz, all, (ob & 1) != 0, (ob & 2) != 0);
		CHECK(a.fused == b.fused && a.three == b.three && a.two == b.two && a.prefix == b.prefix && a.one == b.one, "a (U, Z) launch gave up something else than a three-product launch");
		++g_cases;
	}
	printf("form-check: (U, Z) attribute: three-product launches through a matrix only, by option uz alone; the ladder does not know it\n");
	{ const FormGrant a = step_down(three, all), b = step_down(uz, all); CHECK(a.fused == b.fused && a.three == b.three && a.two == b.two && a.prefix == b.prefix, "below a (U, Z) launch: what lies below a three-product launch"); ++g_cases; }
}

// One product a pair: an attribute of a carrier launch - the carrier rows on both axes - granted by the walk's owner launch by launch.
void check_one() {
	// decide_form: only with the grant, the option and a launch that takes the carrier form; it changes nothing else
	for (const FormFacts& x0 : all_facts()) for (const uint32_t cc : {FUSED_MAX_CHUNKS, FUSED_MAX_CHUNKS + 1}) for (int oo = 0; oo < 3; ++oo) for (int go = 0; go < 2; ++go) for (int gc = 0; gc < 2; ++gc)
	for (int gt = 0; gt < 2; ++gt) for (int gp = 0; gp < 2; ++gp) {
		FormFacts x = x0; x.carrier_chunks = cc; x.row_chunks = cc; x.opt_one = oo;
		FormGrant g; g.two = gt != 0; g.carrier = gc != 0; g.prefix = gp != 0; g.one = go != 0;
		const LaunchForm lf = decide_form(x, g);
		FormGrant g0 = g; g0.one = false;
		const LaunchForm base = decide_form(x, g0);
		++g_cases;
		// (likewise: the one-product grant changes `one` and nothing else)
		{ LaunchForm but_one = lf; but_one.one = false; CHECK(but_one == base, "the one-product grant changed more than the one product"); }
		CHECK(!base.one, "a one-product launch without its grant");
		CHECK(lf.one == (go && oo != 0 && lf.carrier), "one: grant %d option %d carrier %d", go, oo, (int)lf.carrier);
		CHECK(!lf.one || (lf.two && lf.carrier && !lf.three && !lf.fused && !lf.two_pass && x.sorted_u), "a one-product launch that is no carrier launch of the sorted walk");
	}
	// the ladder: a one-product launch whose list overflowed, or that was too rich, is redone in the carrier two-product form and the call gives up
	// `one` and nothing else; with stops, the stops go first
	FormGrant all = grant_of(G_FUSED | G_THREE | G_TWO | G_CARRIER | G_ONE);
	LaunchForm one; one.unphased = true; one.two = true; one.carrier = true; one.one = true;
	{ const FormGrant g = step_down(one, all); CHECK(g.fused && g.three && g.two && g.carrier && !g.one, "below a one-product launch: the carrier two-product form"); }
	for (int ob = 1; ob < 4; ++ob) { CallForms c; c.gave_up(one, all, (ob & 1) != 0, (ob & 2) != 0); CHECK(c.fused && c.three && c.two && c.prefix && !c.one, "a one-product launch overflowed or was too rich: the call gives up one product only");
	                                 CHECK(c.grant(wants_of(W_THREE | W_TWO | W_CARRIER | W_ONE)).carrier && !c.grant(wants_of(W_THREE | W_TWO | W_CARRIER | W_ONE)).one, "... and grants the carrier form still"); }
	{ CallForms c; c.gave_up(one, all, false, false); CHECK(c.one && c.grant(wants_of(W_THREE | W_TWO | W_CARRIER | W_ONE)).one, "a one-product launch went well"); }
	{ FormGrant ng = all; ng.one = false; LaunchForm lf = one; CallForms c; c.gave_up(lf, ng, true, false); CHECK(c.one, "one product was not granted: not taken from the call"); }
	{ LaunchForm lf = one; lf.prefix = true; FormGrant wp = all; wp.prefix = true; const FormGrant g = step_down(lf, wp); CHECK(!g.prefix && g.two && g.carrier && g.one, "below a one-product prefix launch: whole rows, same form");
	  CallForms c; c.gave_up(lf, wp, true, false); CHECK(c.two && c.one && !c.prefix, "a one-product prefix launch's list overflowed: the stops go"); }
	{ LaunchForm two = one; two.one = false; FormGrant g2 = all; g2.one = false; const FormGrant g = step_down(two, g2); CHECK(!g.two && !g.carrier && !g.one && g.three, "below a carrier launch: three products, as before");
	  CallForms c; c.gave_up(two, all, true, false); CHECK(!c.two && !c.grant(wants_of(W_THREE | W_TWO | W_CARRIER | W_ONE)).one, "no two-product launches: none with one product either"); }
	CHECK(!CallForms().grant(wants_of(W_THREE | W_TWO | W_ONE)).one && !CallForms().grant(wants_of(W_THREE | W_CARRIER | W_ONE)).one && !CallForms().grant(wants_of(W_THREE | W_TWO | W_CARRIER)).one, "one-product grants follow the carrier grant");
	g_cases += 10;
	printf("form-check: one-product attribute: granted with the carrier form only, given up alone\n");
}

// The three ways a grant is made - for a launch of the plan, for a sample, for a tile that is redone - against the expressions they replaced, which
// are written out here once: every state of the call x every wants (or every grant given).
void check_named_grants() {
	for (int cb = 0; cb < 32; ++cb) {
		CallForms c; c.fused = (cb & 1) != 0; c.three = (cb & 2) != 0; c.two = (cb & 4) != 0; c.prefix = (cb & 8) != 0; c.one = (cb & 16) != 0;
		for (int wb = 0; wb < W_ALL_BITS; ++wb) {
			const LaunchWants w = wants_of(wb);
			FormGrant launch;      // (what the overload of five positional flags gave)
			launch.fused = c.fused; launch.three = c.three && w.three; launch.two = c.two && w.two; launch.sample = false; launch.prefix = c.prefix && w.prefix;
			launch.carrier = c.two && w.two && w.carrier; launch.one = c.one && c.two && w.two && w.carrier && w.one;
			FormGrant sample;      // (the literal of the sample: three products whatever the call holds, the mark, the rest as the launch's)
			sample.fused = c.fused; sample.three = true; sample.two = w.two && c.two; sample.sample = true; sample.prefix = w.prefix && c.prefix;
			sample.carrier = w.two && c.two && w.carrier; sample.one = w.one && w.two && c.two && c.one && w.carrier;
			g_cases += 2;
			CHECK(same_grant(c.grant(w), launch), "grant(LaunchWants): call %d wants %d", cb, wb);
			CHECK(same_grant(c.sample_grant(w), sample), "sample_grant: call %d wants %d", cb, wb);
		}
		for (int gb = 0; gb < G_ALL_BITS; ++gb) {
			const FormGrant given = grant_of(gb);
			FormGrant redo;        // (grant(given.three, given.two, false, given.carrier, given.one), then fused narrowed and the mark carried over)
			redo.fused = c.fused && given.fused; redo.three = c.three && given.three; redo.two = c.two && given.two; redo.sample = given.sample; redo.prefix = false;
			redo.carrier = c.two && given.two && given.carrier; redo.one = c.one && c.two && given.two && given.carrier && given.one;
			++g_cases;
			CHECK(same_grant(c.redo_grant(given), redo), "redo_grant: call %d given %d", cb, gb);
		}
	}
	printf("form-check: grant, sample_grant and redo_grant equal the expressions they replaced\n");
}

// The numbers that call a sample poor and a launch too rich, at their edges.
void check_thresholds() {
	CHECK(SAMPLE_ONE_IN == 256 && SAMPLE_ONE_IN_THREE_FUSED == 128, "the samples' thresholds");
	CHECK(sample_poor(576, 147456, SAMPLE_ONE_IN) && !sample_poor(577, 147456, SAMPLE_ONE_IN), "1 candidate in 256 is poor, one more is not");
	CHECK(sample_poor(1152, 147456, SAMPLE_ONE_IN_THREE_FUSED) && !sample_poor(1153, 147456, SAMPLE_ONE_IN_THREE_FUSED), "1 candidate in 128 is poor for a fused launch, one more is not");
	CHECK(sample_poor(0, 0, SAMPLE_ONE_IN) && !sample_poor(1, 0, SAMPLE_ONE_IN) && sample_poor(0, 1, SAMPLE_ONE_IN), "no pairs: only no candidates are few");
	// three products: row_pairs / 4 / 128 crosses 4096 at row_pairs = 4096 * 512 + 512 = 2,097,664 (below it the floor of 4096 candidates stands)
	CHECK(!three_too_rich(4096, 0) && three_too_rich(4097, 0), "three products, no pairs: the floor");
	CHECK(!three_too_rich(4096, 2097663) && three_too_rich(4097, 2097663), "three products, just below the crossing: the floor still");
	CHECK(!three_too_rich(4097, 2097664) && three_too_rich(4098, 2097664), "three products, just above the crossing: 1 in 512 of the row pairs");
	CHECK(!three_too_rich(4097, 2097667) && !three_too_rich(4097, 2098175) && !three_too_rich(4098, 2098176), "three products: the division in two steps rounds down twice");
	// one product: pairs / 256 crosses 4096 at pairs = 4096 * 256 + 256 = 1,048,832
	CHECK(!one_too_rich(4096, 0) && one_too_rich(4097, 0) && !one_too_rich(4096, 1048831) && one_too_rich(4097, 1048831) && !one_too_rich(4097, 1048832) && one_too_rich(4098, 1048832), "one product: floor and crossing");
	// the candidate list: pairs / 128 crosses 4096 at pairs = 4096 * 128 + 128 = 524,416
	CHECK(cand_list_entries(0) == 4096 && cand_list_entries(524415) == 4096 && cand_list_entries(524416) == 4097 && cand_list_entries(128ull * 128 * 64 * 64) == 524288, "the candidate list's entries");
	g_cases += 9;
}

// The sub-tile a sample runs (ld_plan.h): rows, columns and diagonal flag written out.
void check_sample_subtile() {
	static const struct { uint32_t rowA0, nA, rowB0, nB; int diag; uint32_t s_rowA0, s_nA, s_rowB0, s_nB; int s_diag; const char* what; } CASES[] = {
		{100, 200, 1000, 300, 0,    100, 200, 1000, 300, 0,   "a tile smaller than the sample: itself"},
		{0, 300, 0, 300, 1,         0, 300, 0, 300, 1,        "a diagonal tile smaller than the sample: itself"},
		{1024, 1024, 1024, 4096, 1, 1344, 384, 1344, 384, 1,  "a diagonal tile with more columns than rows: 384 x 384 on the diagonal, from the rows' middle"},
		{0, 1000, 0, 500, 1,        308, 384, 308, 192, 1,    "a diagonal tile whose columns end inside the sample: cut to the triangle's extent"},
		{0, 8192, 8192, 4096, 0,    3904, 384, 10048, 384, 0, "an off-diagonal tile: the middle of both axes"},
		{0, 1000, 512, 2000, 1,     308, 384, 1320, 384, 0,   "a tile marked diagonal whose axes start apart: as an off-diagonal one"},
		{7, 385, 7, 385, 1,         7, 384, 7, 384, 1,        "one row more than the sample: the odd row is left at the end"},
	};
	for (const auto& k : CASES) {
		twk_hip_tile_desc t{}; t.rowA0 = k.rowA0; t.nA = k.nA; t.rowB0 = k.rowB0; t.nB = k.nB; t.diag = k.diag; t.one = 1;
		const twk_hip_tile_desc st = sample_subtile(t);
		++g_cases;
		CHECK(st.rowA0 == k.s_rowA0 && st.nA == k.s_nA && st.rowB0 == k.s_rowB0 && st.nB == k.s_nB && st.diag == k.s_diag && st.one == 1, "sample_subtile: %s: rows %u+%u, cols %u+%u, diag %d", k.what, st.rowA0, st.nA, st.rowB0, st.nB, (int)st.diag);
	}
}

// ---- the sample ladder (decide_wants) under scripted samplers ---------------------------------------------------------------------------------------
// A sample's outcome: P poor (exactly 1 candidate in 256), M middling (exactly 1 in 128), R rich (one more than that), O its list overflowed, E an
// error that ends the call.  A script: the outcome of the rung with stops, of the two-product rung and of the three-product rung, the first two once
// more for samples that run with one product, and one exception at (rung, pick).
SampleOutcome outcome_of(char o) {
	SampleOutcome r; r.pairs = 384 * 384;
	r.rc = o == 'O' ? TWK_HIP_E_OVERFLOW : o == 'E' ? TWK_HIP_E_DEVICE : TWK_HIP_OK;
	r.cand = o == 'P' ? 576 : o == 'M' ? 1152 : o == 'R' ? 1153 : o == 'O' ? 99999 : 7;
	return r;
}
struct Script { char stops = 'R', two = 'R', three = 'P', one_stops = 'R', one_two = 'R'; char but_rung = 0; size_t but_pick = 0; char but = 'P'; };
// A sample as the ladder asked for it: 'p' with stops, 'P' with stops and two products, '2' two products, '3' three; 'Q' and '1': 'P' and '2' with one product
struct Asked { char rung; size_t pick; };
char rung_of(const LaunchWants& as) { const bool one = as.one && as.two; return as.prefix ? (one ? 'Q' : as.two ? 'P' : 'p') : as.two ? (one ? '1' : '2') : '3'; }
SampleOutcome play(const Script& s, char rung, size_t pick) {
	if (s.but_rung == rung && s.but_pick == pick) return outcome_of(s.but);
	return outcome_of(rung == 'p' || rung == 'P' ? s.stops : rung == 'Q' ? s.one_stops : rung == '2' ? s.two : rung == '1' ? s.one_two : s.three);
}
struct Played { int rc = 0; std::vector<LaunchWants> wants; uint32_t one_refused = 0; std::vector<Asked> asked; std::vector<char> outcomes; int marks = 0; bool carrier_kept = true; };
template <class Eligible, class Planned>
Played play_ladder(size_t n, const LadderFacts& x, const Script& s, Eligible eligible, Planned planned) {
	Played p;
	p.rc = decide_wants(n, x, eligible, planned,
		[&](size_t pick, const LaunchWants& as) {
			const char rung = rung_of(as);
			p.asked.push_back(Asked{rung, pick}); p.carrier_kept = p.carrier_kept && as.carrier == x.carrier;
			const SampleOutcome o = play(s, rung, pick);
			p.outcomes.push_back(o.rc == TWK_HIP_OK ? 'k' : o.rc == TWK_HIP_E_OVERFLOW ? 'O' : 'E');
			return o;
		},
		[&](const char*, size_t, unsigned long long) { ++p.marks; }, p.wants, p.one_refused);
	return p;
}

void check_ladder_invariants() {
	static const size_t NS[] = {0, 1, 2, 3, 64, 65, 66, 129, 200};
	static const char OUTCOMES[] = {'P', 'R', 'O', 'E'};
	long scripts = 0;
	for (int o2 = 0; o2 < 3; ++o2) for (int op = 0; op < 3; ++op) for (int oo = 0; oo < 3; ++oo) for (int o3 = 0; o3 < 3; ++o3) for (int fb = 0; fb < 16; ++fb)
	for (const size_t n : NS) for (int fi = 0; fi < 4; ++fi) {
		const size_t n_front = fi == 0 ? 0 : fi == 1 ? 1 : fi == 2 ? n / 2 : n;
		if (n_front > n || (fi == 1 && n_front == 0) || (fi == 2 && n_front <= 1) || (fi == 3 && n_front <= std::max<size_t>(1, n / 2))) continue;      // (each cut once)
		LadderFacts x; x.opt_two = o2; x.opt_prefix = op; x.opt_one = oo; x.opt_three = o3;
		x.prefix_ok = (fb & 1) != 0; x.one_ok = (fb & 2) != 0; x.three_possible = (fb & 4) != 0; x.fused = (fb & 8) != 0; x.carrier = x.one_ok;
		// (as RegionRun's predicate: nothing with option two = 0, every launch with two = 2, the launches in front of the cut otherwise)
		auto eligible = [&](size_t i) { return o2 != 0 && (o2 == 2 || i < n_front); };
		auto planned = [&](size_t i) { return i % 3 != 1; };
		const bool samples = n > 0 && o3 == 1 && x.three_possible;
		for (const char a : OUTCOMES) for (const char b : OUTCOMES) for (const char c3 : OUTCOMES) for (int shift = 0; shift < (samples ? 2 : 1); ++shift) {
			if (!samples && !(a == 'P' && b == 'P' && c3 == 'P')) continue;      // (no sample is taken: one script says it all)
			Script s; s.stops = a; s.two = b; s.three = c3; s.one_stops = shift ? 'R' : a; s.one_two = shift ? 'R' : b;
			const Played p = play_ladder(n, x, s, eligible, planned);
			++scripts; ++g_cases;
			CHECK(p.wants.size() == n, "a launch without its wants, or one too many");
			if (p.wants.size() != n) continue;
			const size_t cut = o2 == 1 ? n_front : 0, step_behind = std::max<size_t>(1, (n - cut + 63) / 64);      // (the launches sampled one by one lead the plan)
			size_t three_behind = 0, errors = 0;
			for (size_t k = 0; k < p.asked.size(); ++k) {
				if (p.asked[k].rung == '3' && p.asked[k].pick >= cut) ++three_behind;
				if (p.outcomes[k] == 'E') { ++errors; CHECK(k + 1 == p.asked.size(), "a sample was taken after one that failed"); }
			}
			CHECK(three_behind <= 64, "%zu three-product samples behind the cut", three_behind);
			CHECK(p.carrier_kept, "a sample without the region's row operand");
			CHECK(errors ? p.rc == TWK_HIP_E_DEVICE : p.rc == TWK_HIP_OK, "the sampler's error is not the ladder's");
			CHECK(p.marks == (int)p.asked.size() - (int)errors, "a sample without its line in the timeline");
			if (!samples) CHECK(p.asked.empty() && p.one_refused == 0, "samples where no launch would take three products");
			for (size_t i = 0; i < n; ++i) {
				const LaunchWants& w = p.wants[i];
				CHECK(!w.one || (x.one_ok && planned(i) && eligible(i)), "one product for a launch the planner did not mark, or behind the cut");
				CHECK(!w.two || eligible(i), "two products behind the cut");
				CHECK(!w.prefix || x.prefix_ok, "stops where the region may take none");
				CHECK(w.carrier == x.carrier, "the region's row operand");
				if (!samples) CHECK(w.three && w.two == (o2 == 2 && eligible(i)) && w.prefix == (x.prefix_ok && op == 2) && w.one == (x.one_ok && planned(i) && eligible(i)), "no sample: the marks made in front of them");
			}
			if (!samples || errors) continue;
			// a launch in front of the cut is sampled itself; one behind it follows the sample of its own step
			std::vector<char> sampled(n, 0);
			for (const Asked& q : p.asked) sampled[q.pick] = 1;
			for (size_t i = 0; i < n; ++i) {
				const size_t pick = i < cut ? i : std::min(n - 1, cut + (i - cut) / step_behind * step_behind + step_behind / 2);
				CHECK(sampled[pick], "launch %zu: the launch it follows (%zu) was not sampled", i, pick);
				CHECK(p.wants[i].three == p.wants[pick].three && p.wants[i].prefix == p.wants[pick].prefix, "launch %zu does not follow its step's sample", i);
			}
			size_t n_sampled = 0; for (const char c : sampled) n_sampled += c;
			CHECK(n_sampled == cut + (n - cut + step_behind - 1) / step_behind, "launches sampled: %zu", n_sampled);
		}
	}
	printf("form-check: the sample ladder: %ld scripted runs keep their invariants\n", scripts);
}

// Named scripts, answers written out by hand from the ladder as RegionRun::decide_three_by_samples had it: the samples in order - runs of
// `count` steps from pick0 on, `stride` apart, each asked the rungs of `rungs` in turn - and the wants launch by launch ('3' three, '2' two, 'p'
// stops, 'c' carrier rows, '1' one product; "a|b": launches in turn).
struct AskedRun { const char* rungs; size_t pick0, stride, count; };
struct WantsRun { const char* wants; size_t count; };
struct LadderCase {
	const char* what; size_t n; unsigned long long eligible_mask, planned_mask;      // (launches of 64 and beyond: as bit 63)
	LadderFacts x; Script s;
	int rc; uint32_t one_refused; std::vector<AskedRun> asked; std::vector<WantsRun> wants;
};
LadderFacts facts(long long two, long long prefix, long long one, bool prefix_ok, bool one_ok, bool fused = false, long long three = 1) {
	LadderFacts x; x.opt_two = two; x.opt_prefix = prefix; x.opt_one = one; x.opt_three = three; x.prefix_ok = prefix_ok; x.one_ok = one_ok; x.carrier = one_ok; x.fused = fused; x.three_possible = true;
	return x;
}
Script script(char stops, char two, char three, char one_stops = 'R', char one_two = 'R', char but_rung = 0, size_t but_pick = 0, char but = 'P') {
	Script s; s.stops = stops; s.two = two; s.three = three; s.one_stops = one_stops; s.one_two = one_two; s.but_rung = but_rung; s.but_pick = but_pick; s.but = but;
	return s;
}
LadderFacts interleaved(LadderFacts x) { x.eligible_interleaved = true; return x; }      // (the fine walk's plan: two-eligible launches behind the cut too)
std::string wants_text(const LaunchWants& w) { return std::string(w.three ? "3" : "") + (w.two ? "2" : "") + (w.prefix ? "p" : "") + (w.carrier ? "c" : "") + (w.one ? "1" : ""); }

void check_ladder_table() {
	const unsigned long long ALL = ~0ull;
	const std::vector<LadderCase> cases = {
		{"one product marked and its sample poor", 2, 0x1, 0x1, facts(1, 1, 1, false, true), script('R', 'R', 'P', 'R', 'P'),
		 TWK_HIP_OK, 0, {{"1", 0, 0, 1}, {"3", 1, 0, 1}}, {{"32c1", 1}, {"3c", 1}}},
		{"one product refused, then two products poor; the launch behind the cut dense", 2, 0x1, 0x1, facts(1, 1, 1, false, true), script('R', 'P', 'R', 'R', 'R'),
		 TWK_HIP_OK, 1, {{"12", 0, 0, 1}, {"3", 1, 0, 1}}, {{"32c", 1}, {"c", 1}}},
		{"one product refused, then two products refused, then three dense", 1, 0x1, 0x1, facts(1, 1, 1, false, true), script('R', 'R', 'R', 'R', 'R'),
		 TWK_HIP_OK, 1, {{"123", 0, 0, 1}}, {{"c", 1}}},
		{"option one = 2: a rich one-product sample takes nothing back, and the launch is left without two products", 1, 0x1, 0x1, facts(1, 1, 2, false, true), script('R', 'R', 'P', 'R', 'R'),
		 TWK_HIP_OK, 0, {{"13", 0, 0, 1}}, {{"3c1", 1}}},
		{"the sample with stops poor on steps of 2 behind the cut: both launches of a step get the stops", 66, 0, 0, facts(1, 1, 1, true, false), script('P', 'R', 'P'),
		 TWK_HIP_OK, 0, {{"p", 1, 2, 33}}, {{"3p", 66}}},
		{"... poor at one step only: its two launches and no other", 66, 0, 0, facts(1, 1, 1, true, false), script('R', 'R', 'P', 'R', 'R', 'p', 5, 'P'),
		 TWK_HIP_OK, 0, {{"p3", 1, 2, 2}, {"p", 5, 0, 1}, {"p3", 7, 2, 30}}, {{"3", 4}, {"3p", 2}, {"3", 60}}},
		{"the two-product sample poor in front of the cut: each launch by its own sample", 3, 0x3, 0, facts(1, 1, 1, false, false), script('R', 'P', 'R', 'R', 'R', '2', 1, 'R'),
		 TWK_HIP_OK, 0, {{"2", 0, 0, 1}, {"23", 1, 0, 1}, {"3", 2, 0, 1}}, {{"32", 1}, {"", 2}}},
		{"the two-product sample poor on steps of 2 (the walk's launches behind one that is not): the sampled launch alone gets two products", 66, ALL & ~1ull, 0, facts(1, 1, 1, false, false), script('R', 'P', 'P'),
		 TWK_HIP_OK, 0, {{"2", 1, 2, 33}}, {{"3|32", 66}}},
		{"the same with stops: the whole step gets them, and two products with them", 66, ALL & ~1ull, 0, facts(1, 1, 1, true, false), script('P', 'P', 'P'),
		 TWK_HIP_OK, 0, {{"P", 1, 2, 33}}, {{"3p", 1}, {"32p", 65}}},
		{"every list overflows, on every rung", 1, 0x1, 0x1, facts(1, 1, 1, true, true), script('O', 'O', 'O', 'O', 'O'),
		 TWK_HIP_OK, 1, {{"Q1P23", 0, 0, 1}}, {{"c", 1}}},
		{"65 launches behind the cut: steps of 2, the last step one launch, dense there alone", 65, 0, 0, facts(1, 1, 1, false, false), script('R', 'R', 'P', 'R', 'R', '3', 64, 'R'),
		 TWK_HIP_OK, 0, {{"3", 1, 2, 32}, {"3", 64, 0, 1}}, {{"3", 64}, {"", 1}}},
		{"option two = 2 with stops: the sample with stops runs with two products; rich, the launch keeps the two products it was marked for", 2, ALL, 0, facts(2, 1, 1, true, false), script('P', 'R', 'P', 'R', 'R', 'P', 1, 'R'),
		 TWK_HIP_OK, 0, {{"P", 0, 0, 1}, {"P3", 1, 0, 1}}, {{"32p", 1}, {"32", 1}}},
		{"an error on the two-product rung ends the call there", 3, 0x7, 0, facts(1, 1, 1, false, false), script('R', 'P', 'P', 'R', 'R', '2', 1, 'E'),
		 TWK_HIP_E_DEVICE, 0, {{"2", 0, 1, 2}}, {{"32", 1}, {"3", 2}}},
		{"option three = 2: no sample, the marks of two = 2, prefix = 2 and the planner's one product stand", 2, ALL, 0x1, facts(2, 2, 1, true, true, false, 2), script('R', 'R', 'R'),
		 TWK_HIP_OK, 0, {}, {{"32pc1", 1}, {"32pc", 1}}},
		{"1 candidate in 128: dense for a launch through a matrix", 1, 0, 0, facts(1, 1, 1, false, false, false), script('R', 'R', 'M'),
		 TWK_HIP_OK, 0, {{"3", 0, 0, 1}}, {{"", 1}}},
		{"two-eligible launches between three-product ones (the fine walk): each sampled by itself, and the steps of 4 end in front of them", 200, 0x223, 0, interleaved(facts(1, 1, 1, false, false)), script('R', 'P', 'P'),
		 TWK_HIP_OK, 0, {{"2", 0, 1, 2}, {"3", 3, 0, 1}, {"2", 5, 0, 1}, {"3", 7, 0, 1}, {"2", 9, 0, 1}, {"3", 12, 4, 47}, {"3", 199, 0, 1}}, {{"32", 2}, {"3", 3}, {"32", 1}, {"3", 3}, {"32", 1}, {"3", 190}}},
		{"... one of them refused: it alone is left without two products by the ladder (the call then ends them all: behind_refused)", 200, 0x223, 0, interleaved(facts(1, 1, 1, false, false)), script('R', 'P', 'P', 'R', 'R', '2', 9, 'R'),
		 TWK_HIP_OK, 0, {{"2", 0, 1, 2}, {"3", 3, 0, 1}, {"2", 5, 0, 1}, {"3", 7, 0, 1}, {"23", 9, 0, 1}, {"3", 12, 4, 47}, {"3", 199, 0, 1}}, {{"32", 2}, {"3", 3}, {"32", 1}, {"3", 3}, {"3", 1}, {"3", 190}}},
		{"... without the fact the same plan is sampled in steps, as before: launch 5 follows launch 4", 200, 0x223, 0, facts(1, 1, 1, false, false), script('R', 'P', 'P'),
		 TWK_HIP_OK, 0, {{"2", 0, 1, 2}, {"3", 4, 4, 49}, {"3", 199, 0, 1}}, {{"32", 2}, {"3", 198}}},
		{"1 candidate in 128: still three products for a fused launch", 1, 0, 0, facts(1, 1, 1, false, false, true), script('R', 'R', 'M'),
		 TWK_HIP_OK, 0, {{"3", 0, 0, 1}}, {{"3", 1}}},
	};
	for (const LadderCase& k : cases) {
		auto bit = [](unsigned long long mask, size_t i) { return ((mask >> std::min<size_t>(i, 63)) & 1) != 0; };
		const Played p = play_ladder(k.n, k.x, k.s, [&](size_t i) { return k.x.opt_two != 0 && bit(k.eligible_mask, i); }, [&](size_t i) { return bit(k.planned_mask, i); });
		++g_cases;
		std::string asked, want_asked, wants, want_wants;
		for (const Asked& q : p.asked) asked += std::string(1, q.rung) + std::to_string(q.pick) + " ";
		for (const AskedRun& r : k.asked) for (size_t j = 0; j < r.count; ++j) for (const char* c = r.rungs; *c; ++c) want_asked += std::string(1, *c) + std::to_string(r.pick0 + j * r.stride) + " ";
		for (const LaunchWants& w : p.wants) wants += wants_text(w) + ",";
		for (const WantsRun& r : k.wants) {
			std::vector<std::string> turn(1);
			for (const char* c = r.wants; *c; ++c) { if (*c == '|') turn.emplace_back(); else turn.back() += *c; }
			for (size_t j = 0; j < r.count; ++j) want_wants += turn[j % turn.size()] + ",";
		}
		CHECK(p.rc == k.rc && p.one_refused == k.one_refused, "%s: rc %d, %u samples refused", k.what, p.rc, p.one_refused);
		CHECK(asked == want_asked, "%s: samples %s, expected %s", k.what, asked.c_str(), want_asked.c_str());
		CHECK(wants == want_wants, "%s: wants %s expected %s", k.what, wants.c_str(), want_wants.c_str());
	}
	printf("form-check: the sample ladder: %zu named scripts as written out\n", cases.size());
}

// ---- the two-product launches behind the walk's cut ----------------------------------------------------------------------------------------------
void check_behind() {
	CallForms c;
	LaunchWants w; w.two = true; w.carrier = true; w.one = true; w.prefix = true;
	++g_cases;
	CHECK(c.two_behind && c.behind_wants(w).two && c.behind_wants(w).one, "a fresh call has the launches behind the cut");
	const FormGrant given = c.grant(w);
	const FormGrant down = c.behind_overflowed(given);
	CHECK(!c.two_behind && c.two && c.three && c.fused && c.prefix && c.one, "an overflowing launch behind the cut takes another form from the call");
	CHECK(!down.two && !down.carrier && !down.one && !down.prefix && down.three == given.three && down.fused == given.fused && down.three, "redone with three products over whole rows");
	CHECK(!c.behind_wants(w).two && !c.behind_wants(w).one && c.behind_wants(w).three && c.behind_wants(w).prefix, "the launches behind the cut keep two products");
	CHECK(c.grant(w).two && c.grant(w).one && c.grant(w).prefix, "the launches in front of the cut lose theirs");
	CHECK(!c.grant(c.behind_wants(w)).two && c.grant(c.behind_wants(w)).three, "the grant of a launch behind the cut");
	std::vector<LaunchWants> wants(5);
	for (size_t i : {0, 1, 3}) wants[i].two = true;
	auto behind = [](size_t i) { return i == 3 || i == 4; };
	++g_cases;
	CHECK(behind_refused(wants, behind), "launch 4 behind the cut was refused two products");
	wants[4].two = true;
	CHECK(!behind_refused(wants, behind), "no launch behind the cut was refused (launch 2 in front of it says nothing)");
	printf("form-check: the launches behind the cut: sampled by themselves, given up alone\n");
}

}  // namespace

int main() {
	check_decide_form();
	check_gave_up();
	check_carrier();
	check_one();
	check_uz();
	check_named_grants();
	check_thresholds();
	check_sample_subtile();
	check_ladder_invariants();
	check_ladder_table();
	check_behind();
	printf("form-check: %ld cases, %d bad\n", g_cases, g_bad_checks);
	return g_bad_checks ? 1 : 0;
}
