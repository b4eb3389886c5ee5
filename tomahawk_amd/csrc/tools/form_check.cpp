// `make form-check`: who may take which form of a count launch (csrc/hip/ld_form.h), on the CPU under AddressSanitizer and UBSan.
//   1. decide_form over every combination of FormFacts x FormGrant: no two forms that exclude each other, a reducing launch in no form but
//      four products through a matrix, every form only on the planes, under the grants and with the options it needs, and no grant whose
//      withdrawal adds a form - but grant.two, which turns two products into three.
//   2. CallForms::gave_up: the transitions a launch's outcome makes in what the call still allows, one by one, that a form the launch was not
//      granted is never taken from the call, and that a second telling changes nothing; step_down, the ladder a redone tile descends.
#include <cstdio>
#include <initializer_list>
#include <vector>
#include "../hip/ld_form.h"

using namespace twk;

namespace {

int g_bad_checks = 0;
long g_cases = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_bad_checks < 40) { fprintf(stderr, "    FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } ++g_bad_checks; } } while (0)

bool same(const LaunchForm& a, const LaunchForm& b) {
	return a.two_pass == b.two_pass && a.fused == b.fused && a.unphased == b.unphased && a.three == b.three && a.two == b.two && a.keep_three == b.keep_three &&
	       a.sample == b.sample && a.reduce == b.reduce;
}
FormGrant grant_of(int bits) { return FormGrant{(bits & 1) != 0, (bits & 2) != 0, (bits & 4) != 0, (bits & 8) != 0}; }

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
			if (bit == 3) { LaunchForm marked = less; marked.sample = true; CHECK(same(marked, lf), "grant.sample changed the form"); continue; }
			CHECK(!(less.fused && !lf.fused), "withdrawing grant %d added the fused form", bit);
			CHECK(!(less.two && !lf.two), "withdrawing grant %d added two products", bit);
			if (less.three && !lf.three) CHECK(bit == 2 && lf.two && !less.two, "withdrawing grant %d added three products", bit);
			if (bit == 2 && !same(less, lf)) CHECK(lf.two && !less.two && less.three && !lf.three && less.fused == lf.fused, "withdrawing grant.two did more than turn two products into three");
		}
	}
}

LaunchForm form_of(bool fused, bool three, bool two, bool keep_three = false) { LaunchForm lf; lf.unphased = three || two; lf.fused = fused; lf.three = three; lf.two = two; lf.keep_three = keep_three; return lf; }
bool is(const CallForms& c, bool fused, bool three, bool two) { return c.fused == fused && c.three == three && c.two == two; }

void check_gave_up() {
	const FormGrant all{true, true, true, false};
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
		const FormGrant next = c.grant(true, true);
		CHECK(next.fused == c.fused && next.three == c.three && next.two == c.two && !next.sample, "grant");
		CHECK(!c.grant(false, true).three && !c.grant(true, false).two, "grant beyond what the owner wants");
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
		CHECK(!gone.grant(true, true, true).prefix && CallForms().grant(true, true, true).prefix && !CallForms().grant(true, true).prefix, "prefix grants");
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
		CHECK(same(lf, base) && lf.prefix == base.prefix, "the carrier grant changed the form");
		CHECK(!base.carrier, "a carrier launch without its grant");
		CHECK(lf.carrier == (gc && oc != 0 && cc > FUSED_MAX_CHUNKS && lf.two), "carrier: grant %d option %d chunks %u two %d", gc, oc, cc, (int)lf.two);
		CHECK(!lf.carrier || (lf.two && !lf.three && !lf.fused && !lf.two_pass && x.sorted_u), "a carrier launch that is no two-product launch of the sorted walk");
	}
	// the ladder: a carrier launch whose list overflowed is redone with three products, and the call's two-product launches end - as the H form's;
	// a prefix launch on carrier rows is redone over whole rows on the same rows
	FormGrant all{true, true, true, false}; all.carrier = true;
	LaunchForm two; two.unphased = true; two.two = true; two.carrier = true;
	{ const FormGrant g = step_down(two, all); CHECK(g.fused && g.three && !g.two && !g.carrier, "below a carrier launch: three products"); }
	{ CallForms c; c.gave_up(two, all, true, false); CHECK(c.fused && c.three && !c.two && c.prefix, "a carrier launch's list overflowed: no more two-product launches"); CHECK(!c.grant(true, true, false, true).carrier && !c.grant(true, true, false, true).two, "... and none on carrier rows"); }
	{ CallForms c; c.gave_up(two, all, false, false); CHECK(c.two && c.grant(true, true, false, true).carrier, "a carrier launch went well"); }
	{ LaunchForm lf = two; lf.prefix = true; FormGrant wp = all; wp.prefix = true; const FormGrant g = step_down(lf, wp); CHECK(!g.prefix && g.two && g.carrier, "below a carrier prefix launch: whole rows, same operand");
	  CallForms c; c.gave_up(lf, wp, true, false); CHECK(c.two && !c.prefix, "a carrier prefix launch's list overflowed: the stops go"); }
	CHECK(!CallForms().grant(true, false, false, true).carrier && !CallForms().grant(true, true).carrier && CallForms().grant(true, true, false, true).carrier, "carrier grants follow the two-product grant");
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
		CHECK(same(lf, base) && lf.prefix == base.prefix && lf.carrier == base.carrier, "the one-product grant changed the form");
		CHECK(!base.one, "a one-product launch without its grant");
		CHECK(lf.one == (go && oo != 0 && lf.carrier), "one: grant %d option %d carrier %d", go, oo, (int)lf.carrier);
		CHECK(!lf.one || (lf.two && lf.carrier && !lf.three && !lf.fused && !lf.two_pass && x.sorted_u), "a one-product launch that is no carrier launch of the sorted walk");
	}
	// the ladder: a one-product launch whose list overflowed, or that was too rich, is redone in the carrier two-product form and the call gives up
	// `one` and nothing else; with stops, the stops go first
	FormGrant all{true, true, true, false}; all.carrier = true; all.one = true;
	LaunchForm one; one.unphased = true; one.two = true; one.carrier = true; one.one = true;
	{ const FormGrant g = step_down(one, all); CHECK(g.fused && g.three && g.two && g.carrier && !g.one, "below a one-product launch: the carrier two-product form"); }
	for (int ob = 1; ob < 4; ++ob) { CallForms c; c.gave_up(one, all, (ob & 1) != 0, (ob & 2) != 0); CHECK(c.fused && c.three && c.two && c.prefix && !c.one, "a one-product launch overflowed or was too rich: the call gives up one product only");
	                                 CHECK(c.grant(true, true, false, true, true).carrier && !c.grant(true, true, false, true, true).one, "... and grants the carrier form still"); }
	{ CallForms c; c.gave_up(one, all, false, false); CHECK(c.one && c.grant(true, true, false, true, true).one, "a one-product launch went well"); }
	{ FormGrant ng = all; ng.one = false; LaunchForm lf = one; CallForms c; c.gave_up(lf, ng, true, false); CHECK(c.one, "one product was not granted: not taken from the call"); }
	{ LaunchForm lf = one; lf.prefix = true; FormGrant wp = all; wp.prefix = true; const FormGrant g = step_down(lf, wp); CHECK(!g.prefix && g.two && g.carrier && g.one, "below a one-product prefix launch: whole rows, same form");
	  CallForms c; c.gave_up(lf, wp, true, false); CHECK(c.two && c.one && !c.prefix, "a one-product prefix launch's list overflowed: the stops go"); }
	{ LaunchForm two = one; two.one = false; FormGrant g2 = all; g2.one = false; const FormGrant g = step_down(two, g2); CHECK(!g.two && !g.carrier && !g.one && g.three, "below a carrier launch: three products, as before");
	  CallForms c; c.gave_up(two, all, true, false); CHECK(!c.two && !c.grant(true, true, false, true, true).one, "no two-product launches: none with one product either"); }
	CHECK(!CallForms().grant(true, true, false, false, true).one && !CallForms().grant(true, false, false, true, true).one && !CallForms().grant(true, true, false, true).one, "one-product grants follow the carrier grant");
	g_cases += 10;
	printf("form-check: one-product attribute: granted with the carrier form only, given up alone\n");
}

}  // namespace

int main() {
	check_decide_form();
	check_gave_up();
	check_carrier();
	check_one();
	printf("form-check: %ld cases, %d bad\n", g_cases, g_bad_checks);
	return g_bad_checks ? 1 : 0;
}
