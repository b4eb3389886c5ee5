// `tomahawk calc` on the MI355X engine: same flags, defaults, messages-on-stderr
// and exit codes as the reference CLI (lib/main.cpp:19-93, lib/calc.h:28-240); the engine's other commands; the reference's host tools.
// An engine command is one row (Command): its usage text, a verbatim literal, is followed by its own options and its row; run_command()
// parses the shared options, and run_main() reads the rows for dispatch, help and the "Illegal command" sentence.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <getopt.h>
#include <iostream>
#include <regex>
#include <string>
#include <vector>
#include <fstream>
#include <ctime>
#include <unistd.h>
#include <sys/wait.h>
#include <malloc.h>

#include "twk_ld.h"
#include "twk_ld_names.h"
#include "twk_format.h"
#include "twk_hip.h"
#include "twk_two_tools.h"
#include "twk_import.h"

namespace tomahawk { std::string LITERAL_COMMAND_LINE; }

static void program_message() {
	std::cerr << "Program:   tomahawk-mi355x (pairwise LD on AMD MI355X; `tomahawk calc` compatible)\n"
	          << "Libraries: tomahawk_amd; ZSTD-" << tomahawk::zstd_version() << "; twk_hip ABI " << twk_hip_abi_version() << "\n"
	          << "----------" << std::endl;
}

static void calc_usage() {
	program_message();
	std::cerr <<
	"About:  Calculate linkage disequilibrium\n"
	"        Force phased -p or unphased -u for faster calculations if\n"
	"        all variant sites are guaranteed to have the given phasing.\n\n"
	"Usage:  tomahawk calc [options] -i <in.twk> -o <output.two>\n\n"
	"Options:\n"
	"  -i FILE   input Tomahawk (required)\n"
	"  -o FILE   output file or file prefix (required)\n"
	"  -t INT    number of CPU threads used to unpack the input (default: maximum available)\n"
	"  -c INT    number of subproblems to split compute into (must be in (c!2 + c))\n"
	"  -C INT    chosen part to compute (0 < -C < -c)\n"
	"  -m, -M    accepted for compatibility (CPU low-memory modes; no effect on the GPU engine)\n"
	"  -b        number of records in a block (accepted; unused by calc, as in the reference)\n"
	"  -w INT    sliding window width in bases\n"
	"  -I STRING filter interval <contig>:pos-pos (see manual)\n"
	"  -p        force computations to use phased math\n"
	"  -u        force computations to use unphased math\n"
	"  -P FLOAT  Fisher's exact test / Chi-squared cutoff P-value (default: 1)\n"
	"  -r FLOAT  Pearson's R-squared minimum cut-off value (default: 0.1)\n"
	"  -k INT    compression level to use (default: 1, max = 22).\n"
	"  --engine-option KEY=INT  a switch of the GPU engine (twk_hip_set_option, include/twk_hip.h; repeatable)\n"
	"Environment: TWK_HIP_DEVICE=<n> selects the GPU (default 0); TWK_HIP_GPUS=<n> uses GPUs 0..n-1, one\n"
	"             driver thread each (equal-area row bands, one shared output file); TWK_HIP_PART=k/n makes\n"
	"             this process compute share k of n of a multi-node run (merge the outputs with concat).\n" << std::endl;
}

static std::string stamp(const char* t) { return std::string("[") + t + "] "; }

static bool fail(const std::string& what) { std::cerr << stamp("ERROR") << what << std::endl; return false; }

// ---- What is parsed more than once, parsed here.  Each -> false after its error message ----
using tomahawk::twk_ld_settings;

static bool thread_option(const char* arg, int32_t& n_threads) {
	n_threads = atoi(arg);
	return n_threads > 0 || fail("Cannot have a non-positive number of worker threads");
}

// A non-negative integer, maybe with an exponent (5000, 1e6)?  (Says nothing: -w answers in the reference's words.)
static bool integer_form(const std::string& arg) {
	static const std::regex form("^(([0-9]+)|([0-9]+[eE]{1}[0-9]+))$");
	return std::regex_match(arg, form);
}
// Such an integer in [lo, hi] -> v.  subject: "range (-d)"; bounds: the words after "must be"
static bool integer_option(const std::string& arg, const char* subject, double lo, double hi, const std::string& bounds, double& v) {
	if (!integer_form(arg)) return fail(std::string("The ") + subject + " must be a non-negative integer: " + arg);
	v = atof(arg.c_str());
	return (v >= lo && v <= hi) || fail(std::string("The ") + subject + " must be " + bounds);
}

// -f: a fill value (nan and inf are numbers here: a fill may be either)
template <typename T>
static bool fill_option(const char* arg, T& fill) {
	char* end = nullptr;
	T v;
	if constexpr (sizeof(T) == sizeof(float)) v = strtof(arg, &end); else v = strtod(arg, &end);
	if (end == arg || *end) return fail(std::string("The fill value (-f) must be a number: ") + arg);
	fill = v;
	return true;
}

// -s: a statistic by its name in `names` (twk_ld_names.h)
template <int N>
static bool stat_option(const char* arg, const tomahawk::NameTable<N>& names, int32_t& stat) {
	const int32_t v = names.value(arg);
	if (v < 0) return fail(std::string("Unknown statistic (-s): ") + arg + " - one of " + names.list());
	stat = v;
	return true;
}

// ---- An engine command is a row: what the one parser and the one tail below need to know about it ----
enum Took { took, failed, declined };
struct Refusal { const char* flags; const char* why; };      // a shared option the command refuses: its letters, and the sentence (%c: the letter met)
struct NoOptions {};
template <class Own>                      // Own: the settings the command's own options fill in; run_command() holds them by value
struct Command {
	const char* name;
	const char* summary;                  // its line of `tomahawk` without arguments
	void (*usage)();
	const char* short_options;            // getopt's string, as the command has always had it
	const struct option* long_options;
	double minR2;                         // the default of -r (every other default is twk_ld_settings' own)
	Refusal refusals[5];
	const char* only_P1;                  // -P below 1 is refused with this sentence; null: calc, which applies -P
	Took (*option)(int c, const char* arg, twk_ld_settings& settings, Own& own);      // the command's own options; null: it has none
	bool (*check)(twk_ld_settings& settings, Own& own);                               // after the options and the input's name; null: nothing more
	bool (*run)(tomahawk::twk_ld& ld, const twk_ld_settings& settings, const Own& own);
};

// --extract FILE / --exclude FILE / --maf X / --max-maf X / --mac N / --geno X / --hwe P (not in the reference): LD over a subset of the
// variants, twk_ld_settings::extract_file.  Long names only, as --keep; one table entry list and one handler for every command that
// takes --keep / --remove.  The ranges are the engine's (twk_hip_select_variants), checked here so that the error names the option.
#define VARIANT_SELECTION_LONG_OPTIONS \
	{"extract", required_argument, 0, 1010}, {"exclude", required_argument, 0, 1011}, {"maf", required_argument, 0, 1012}, {"max-maf", required_argument, 0, 1013}, {"mac", required_argument, 0, 1014}, {"geno", required_argument, 0, 1015}, {"hwe", required_argument, 0, 1016}
static Took variant_selection_option(int c, const char* arg, twk_ld_settings& settings) {
	auto number = [&](const char* name, double lo, double hi, double& out) {
		char* end = nullptr;
		const double x = strtod(arg, &end);
		if (end == arg || *end || !(x >= lo && x <= hi)) { char why[160]; snprintf(why, sizeof(why), "%s wants a number between %g and %g", name, lo, hi); fail(why); return failed; }
		out = x;
		return took;
	};
	switch (c) {
	case 1010: settings.extract_file = arg; return took;
	case 1011: settings.exclude_file = arg; return took;
	case 1012: return number("--maf", 0.0, 0.5, settings.min_maf);
	case 1013: return number("--max-maf", 0.0, 0.5, settings.max_maf);
	case 1014: {      // an unsigned integer, digits only
		const std::string a(arg);
		if (a.empty() || a.size() > 10 || a.find_first_not_of("0123456789") != std::string::npos || strtoull(arg, nullptr, 10) > 4294967295ull) { fail("--mac wants an integer between 0 and 4294967295"); return failed; }
		settings.min_mac = (uint32_t)strtoull(arg, nullptr, 10);
		return took;
	}
	case 1015: return number("--geno", 0.0, 1.0, settings.max_missing);
	case 1016: return number("--hwe", 0.0, 1.0, settings.min_hwe);
	}
	return declined;
}

// The shared options once (-i -o -I -p -u -t -c -C -r -P -w --engine-option, the sample and variant selections), anything else to the command's own handler; then the checks
// after the options, the banner, and the call.
template <class Own>
static int run_command(const Command<Own>& cmd, int argc, char** argv) {
	if (argc < 3) { cmd.usage(); return 1; }
	twk_ld_settings settings;
	settings.minR2 = cmd.minR2;
	Own own{};
	std::vector<std::pair<std::string, long long>> engine_options;
	int c, option_index = 0;
	while ((c = getopt_long(argc, argv, cmd.short_options, cmd.long_options, &option_index)) != -1) {
		for (const Refusal& r : cmd.refusals) {
			if (!r.flags || c <= 0 || c > 127 || !strchr(r.flags, c)) continue;
			char why[256];
			snprintf(why, sizeof(why), r.why, c);
			return !fail(why);
		}
		switch (c) {
		case 'i': settings.in = optarg; break;
		case 'o': settings.out = optarg; break;
		case 'I': settings.ival_strings.push_back(optarg); break;
		case 'p': settings.force_phased = true; settings.forced_unphased = false; break;
		case 'u': settings.forced_unphased = true; settings.force_phased = false; break;
		case 't': if (!thread_option(optarg, settings.n_threads)) return 1; break;
		case 'c':
			settings.n_chunks = atoi(optarg);
			if (settings.n_chunks <= 0) return !fail("Cannot have a negative or zero amount of partitions");
			break;
		case 'C':
			settings.c_chunk = atoi(optarg) - 1;   // 1-based on the command line (calc.h:152-153)
			if (settings.c_chunk < 0) return !fail("Cannot have a non-positive start partition");
			break;
		case 'r':
			settings.minR2 = atof(optarg);
			if (settings.minR2 < 0) return !fail("Cannot have a negative minimum R-squared value");
			if (settings.minR2 > 1) return !fail("Cannot have minimum R-squared value > 1");
			break;
		case 'P':
			settings.minP = atof(optarg);
			if (cmd.only_P1) { if (!(settings.minP >= 1)) return !fail(cmd.only_P1); }
			else if (settings.minP < 0) return !fail("Cannot have a negative cutoff P-value");
			if (settings.minP > 1) return !fail("Cannot have a cutoff P-value > 1");
			break;
		case 'w': {
			settings.window = true;
			const std::string a(optarg);           // (--windowBases without =: no argument, and std::string says so)
			if (!integer_form(a)) { std::cerr << "not an integer" << std::endl; return 1; }
			settings.l_window = a.find_first_of("eE") == std::string::npos ? atoi(optarg) : (int32_t)atof(optarg);
			if (settings.l_window <= 0) return !fail("Cannot have a non-positive window size");
			break;
		}
		case 1006: settings.keep_file = optarg; break;        // --keep FILE / --remove FILE (not in the reference): LD over a subset of the samples,
		case 1007: settings.remove_file = optarg; break;      // twk_ld_settings::keep_file.  Long names only, as --annot: the usage texts answer as they always have
		case 1000: {      // --engine-option key=value (not in the reference): twk_ld::SetEngineOption
			const std::string a(optarg);
			const size_t eq = a.find('=');
			if (eq == std::string::npos || eq == 0 || eq + 1 >= a.size()) return !fail("--engine-option wants key=value");
			engine_options.emplace_back(a.substr(0, eq), atoll(a.c_str() + eq + 1));
			break;
		}
		default:
			if (const Took v = variant_selection_option(c, optarg, settings); v != declined) { if (v == failed) return 1; break; }
			switch (cmd.option ? cmd.option(c, optarg, settings, own) : declined) {
			case took: break;
			case failed: return 1;
			case declined:      // (a long option without a letter - another command's --annot, --self, --band, --top - by its name)
				return !fail(std::string("Unrecognized option: ") + (c > 127 ? std::string("--") + cmd.long_options[option_index].name : std::string(1, (char)c)));
			}
		}
	}
	if (settings.in.empty()) return !fail("No input value specified...");
	if (cmd.check && !cmd.check(settings, own)) return 1;
	program_message();
	std::cerr << stamp("LOG") << "Calling " << cmd.name << "..." << std::endl;
	tomahawk::twk_ld ld;
	for (const auto& kv : engine_options) ld.SetEngineOption(kv.first, kv.second);
	return cmd.run(ld, settings, own) ? 0 : 1;
}

// The long names of `calc` (the reference's), of the six commands that reduce calc's records, and of `relationship`
static const struct option CALC_LONG_OPTIONS[] = {
	{"input", required_argument, 0, 'i'}, {"threads", optional_argument, 0, 't'}, {"output", required_argument, 0, 'o'},
	{"interval", optional_argument, 0, 'I'}, {"parts", optional_argument, 0, 'c'}, {"partStart", optional_argument, 0, 'C'},
	{"low-memory", optional_argument, 0, 'm'}, {"block-size", optional_argument, 0, 'b'}, {"bitmaps", optional_argument, 0, 'M'},
	{"compression-level", optional_argument, 0, 'k'}, {"cross-chr-only", no_argument, 0, 'X'}, {"no-cross-chr", no_argument, 0, 'x'},
	{"minP", optional_argument, 0, 'P'}, {"force-phased", no_argument, 0, 'p'}, {"force-unphased", no_argument, 0, 'u'},
	{"samples", optional_argument, 0, 'S'}, {"minR2", optional_argument, 0, 'r'}, {"detailedProgress", no_argument, 0, 'd'},
	{"silent", no_argument, 0, 's'}, {"windowBases", optional_argument, 0, 'w'},
	{"engine-option", required_argument, 0, 1000}, {"keep", required_argument, 0, 1006}, {"remove", required_argument, 0, 1007}, VARIANT_SELECTION_LONG_OPTIONS, {0, 0, 0, 0}};
static const struct option REDUCE_LONG_OPTIONS[] = {
	{"input", required_argument, 0, 'i'}, {"threads", optional_argument, 0, 't'}, {"output", required_argument, 0, 'o'},
	{"interval", optional_argument, 0, 'I'}, {"parts", optional_argument, 0, 'c'}, {"partStart", optional_argument, 0, 'C'},
	{"minP", optional_argument, 0, 'P'}, {"force-phased", no_argument, 0, 'p'}, {"force-unphased", no_argument, 0, 'u'},
	{"minR2", optional_argument, 0, 'r'}, {"windowBases", optional_argument, 0, 'w'},
	{"engine-option", required_argument, 0, 1000}, {"keep", required_argument, 0, 1006}, {"remove", required_argument, 0, 1007}, VARIANT_SELECTION_LONG_OPTIONS, {"assoc", required_argument, 0, 'a'}, {"annot", required_argument, 0, 1002}, {"self", no_argument, 0, 1001}, {"p1", required_argument, 0, '1'}, {"p2", required_argument, 0, '2'},
	{"stat", required_argument, 0, 's'}, {"fill", required_argument, 0, 'f'}, {"text", no_argument, 0, 'T'}, {"band", no_argument, 0, 1003},
	{"top", required_argument, 0, 1004}, {"top-stat", required_argument, 0, 1005}, {"kept-only", no_argument, 0, 1017},
	{"range", required_argument, 0, 'd'}, {"bins", required_argument, 0, 'b'},
	{"xbins", required_argument, 0, 'x'}, {"ybins", required_argument, 0, 'y'}, {"reduce", required_argument, 0, 'R'}, {"minCount", required_argument, 0, 'm'},
	{0, 0, 0, 0}};
static const struct option RELATIONSHIP_LONG_OPTIONS[] = {
	{"input", required_argument, 0, 'i'}, {"interval", required_argument, 0, 'I'}, {"stat", required_argument, 0, 's'}, {"fill", required_argument, 0, 'f'},
	{"output", required_argument, 0, 'o'}, {"text", no_argument, 0, 'T'}, {"threads", required_argument, 0, 't'}, {"engine-option", required_argument, 0, 1000}, {"keep", required_argument, 0, 1006}, {"remove", required_argument, 0, 1007}, VARIANT_SELECTION_LONG_OPTIONS,
	{"force-phased", no_argument, 0, 'p'}, {"force-unphased", no_argument, 0, 'u'}, {"minR2", required_argument, 0, 'r'}, {"windowBases", required_argument, 0, 'w'},
	{"parts", required_argument, 0, 'c'}, {"partStart", required_argument, 0, 'C'}, {"minP", required_argument, 0, 'P'}, {0, 0, 0, 0}};

// `calc`'s own options: the reference's low-memory modes and block size (accepted, unused here) and the compression level
static Took calc_option(int c, const char* arg, twk_ld_settings& settings, NoOptions&) {
	switch (c) {
	case 'm': settings.low_memory = true; return took;
	case 'M': settings.force_phased = true; settings.low_memory = true; settings.bitmaps = true; return took;
	case 'b':
		settings.bl_size = atoi(arg);
		return settings.bl_size > 0 || fail("Cannot have a non-positive number of entries in a block!") ? took : failed;
	case 'k': settings.c_level = atoi(arg); return took;
	}
	return declined;
}
static const Command<NoOptions> CALC = {
	"calc", "  calc     calculate linkage disequilibrium: tomahawk calc [options] -i <in.twk> -o <output.two>\n", calc_usage,
	"i:o:t:puP:a:A:r:w:S:I:sdc:C:mMb:xXk:?", CALC_LONG_OPTIONS, 0.1, {}, nullptr, calc_option,
	[](twk_ld_settings& settings, NoOptions&) { return !settings.out.empty() || fail("No output value specified..."); },
	[](tomahawk::twk_ld& ld, const twk_ld_settings& settings, const NoOptions&) { return ld.Compute(settings); }};

// `tomahawk ldscore` (not in the reference): per-variant sums of r2 over the records `calc` would write, reduced on the GPU.
static void ldscore_usage() {
	program_message();
	std::cerr <<
	"About:  LD scores: for every variant the number of partners `calc` would report it with\n"
	"        and the sum of their R-squared values, reduced on the GPU (no .two is written).\n"
	"        With -r 0 (default) the sum is the LD score; with -r 0.8 the count is the number\n"
	"        of tagging partners.\n\n"
	"Usage:  tomahawk ldscore [options] -i <in.twk> [-o <out.tsv>]\n\n"
	"Options:\n"
	"  -i FILE   input Tomahawk (required)\n"
	"  -o FILE   output text file (- for stdout; default: -)\n"
	"  -t INT    number of CPU threads used to unpack the input (default: maximum available)\n"
	"  -c INT    number of subproblems to split compute into (must be in (c!2 + c))\n"
	"  -C INT    chosen part to compute (0 < -C < -c)\n"
	"  -w INT    sliding window width in bases\n"
	"  -I STRING filter interval <contig>:pos-pos (see manual)\n"
	"  -p        force computations to use phased math\n"
	"  -u        force computations to use unphased math\n"
	"  -r FLOAT  Pearson's R-squared minimum cut-off value (default: 0)\n"
	"  -P FLOAT  accepted only as 1: a score sums over every record, Fisher's test is not run\n"
	"  --engine-option KEY=INT  a switch of the GPU engine (twk_hip_set_option, include/twk_hip.h; repeatable)\n"
	"Output: '#' header lines, then per variant: contig <TAB> pos <TAB> n_partners <TAB> sum_r2\n"
	"Environment: TWK_HIP_DEVICE=<n> selects the GPU (default 0).\n" << std::endl;
}

// (`ldscore --top K [--top-stat r2|r|D|Dprime]`, likewise long names only and not in the usage text: every variant's K strongest partners,
// INTEGRATION section 1)
// ... and `ldscore --annot FILE [--self]`: the scores partitioned by annotation category.  Long names only, and not in
// the usage text above: `ldscore -a`, `ldscore --assoc` and the usage itself answer as they always have (tests/golden/cli_transcript.json).
static Took ldscore_option(int c, const char* arg, twk_ld_settings&, tomahawk::twk_score_settings& score) {
	if (c == 1002) { score.annot = arg; return took; }
	if (c == 1001) { score.self = true; return took; }
	if (c == 1004) {      // --top K: the K strongest partners of every variant in place of the scores
		char* end = nullptr;
		const long k = strtol(arg, &end, 10);
		if (end == arg || *end || k < 1 || k > TWK_HIP_TOPK_MAX) return fail(std::string("The number of partners to list (--top) must be an integer between 1 and ") + std::to_string(TWK_HIP_TOPK_MAX) + ": " + arg) ? took : failed;
		score.top = (int32_t)k;
		return took;
	}
	if (c == 1005) {      // --top-stat: what the partners are ranked by
		const int32_t v = tomahawk::LD_STATS.value(arg);
		if (v < 0) return fail(std::string("Unknown statistic (--top-stat): ") + arg + " - one of " + tomahawk::LD_STATS.list()) ? took : failed;
		score.top_stat = v;
		return took;
	}
	return declined;
}

static const Command<tomahawk::twk_score_settings> LDSCORE = {
	"ldscore", "  ldscore  per-variant LD scores (sums of r2 over a variant's partners), reduced on the GPU\n", ldscore_usage,
	"i:o:t:puP:r:w:I:c:C:?", REDUCE_LONG_OPTIONS, 0, {},
	"Cannot score with a cutoff P-value below 1: a score sums over every record and Fisher's exact test is not run", ldscore_option,
	[](twk_ld_settings&, tomahawk::twk_score_settings& score) {
		if (score.top_stat >= 0 && !score.top) return fail("--top-stat needs a number of partners to list (--top)");
		if (score.top && !score.annot.empty()) return fail("--top lists partners and takes no annotation file (--annot)");
		return !score.self || !score.annot.empty() || fail("--self needs an annotation file (--annot)");
	},
	[](tomahawk::twk_ld& ld, const twk_ld_settings& settings, const tomahawk::twk_score_settings& score) { return ld.Score(settings, score); }};

// `tomahawk prune` (not in the reference): greedy LD pruning in file order over the records `calc` would write, decided on the GPU.
static void prune_usage() {
	program_message();
	std::cerr <<
	"About:  LD pruning: walking the variants in file order, a variant is kept if and only if no\n"
	"        variant kept before it forms a pair with it that `calc` would report under the same\n"
	"        options (greedy pruning, like PLINK's --indep-pairwise); decided on the GPU (no .two\n"
	"        is written).\n\n"
	"Usage:  tomahawk prune [options] -i <in.twk> [-o <out.tsv>]\n\n"
	"Options:\n"
	"  -i FILE   input Tomahawk (required)\n"
	"  -o FILE   output text file (- for stdout; default: -)\n"
	"  -t INT    number of CPU threads used to unpack the input (default: maximum available)\n"
	"  -w INT    sliding window width in bases\n"
	"  -I STRING filter interval <contig>:pos-pos (see manual)\n"
	"  -p        force computations to use phased math\n"
	"  -u        force computations to use unphased math\n"
	"  -r FLOAT  Pearson's R-squared minimum cut-off value: pairs at or above it are in LD (default: 0.1)\n"
	"  -P FLOAT  accepted only as 1: pruning looks at every record, Fisher's test is not run\n"
	"  --engine-option KEY=INT  a switch of the GPU engine (twk_hip_set_option, include/twk_hip.h; repeatable)\n"
	"  (-c / -C are refused: the walk needs every pair)\n"
	"Output: '#' header lines, then per variant: contig <TAB> pos <TAB> keep (1 kept, 0 pruned)\n"
	"Environment: TWK_HIP_DEVICE=<n> selects the GPU (default 0).\n" << std::endl;
}

// (`prune --kept-only`, long name only and not in the usage text: the kept variants' lines alone, a list that --extract reads back)
static Took prune_option(int c, const char*, twk_ld_settings&, tomahawk::twk_prune_settings& prune) {
	if (c == 1017) { prune.kept_only = true; return took; }
	return declined;
}
static const Command<tomahawk::twk_prune_settings> PRUNE = {      // (-r: calc's default)
	"prune", "  prune    greedy LD pruning in file order (a keep flag per variant), decided on the GPU\n", prune_usage,
	"i:o:t:puP:r:w:I:c:C:?", REDUCE_LONG_OPTIONS, 0.1, {{"cC", "Cannot prune a part of the pair space (-c / -C): the walk needs every pair"}},
	"Cannot prune with a cutoff P-value below 1: pruning looks at every record and Fisher's exact test is not run", prune_option, nullptr,
	[](tomahawk::twk_ld& ld, const twk_ld_settings& settings, const tomahawk::twk_prune_settings& prune) { return ld.Prune(settings, prune); }};

// `tomahawk clump` (not in the reference): LD clumping (PLINK's --clump) over the records `calc` would write, decided on the GPU.
static void clump_usage() {
	program_message();
	std::cerr <<
	"About:  LD clumping: the variants are visited from the smallest association P-value upwards, up\n"
	"        to the index threshold; a visited variant that belongs to no clump yet becomes an index\n"
	"        variant and claims every variant that belongs to no clump, passes the secondary threshold\n"
	"        and forms a pair with it that `calc` would report under the same options (like PLINK's\n"
	"        --clump); decided on the GPU (no .two is written).\n\n"
	"Usage:  tomahawk clump [options] -i <in.twk> -a <assoc.txt> [-o <out.tsv>]\n\n"
	"Options:\n"
	"  -i FILE   input Tomahawk (required)\n"
	"  -a FILE   association file (required): text, split on tabs or spaces, '#' lines ignored;\n"
	"            columns contig, pos (1-based, as `ldscore` / `prune` / `view` print it), P (NA / nan:\n"
	"            none); further columns are ignored.  Every selected variant at a (contig, pos) gets\n"
	"            that P; variants the file does not name get none.  The same (contig, pos) twice or a\n"
	"            P outside [0, 1] is an error\n"
	"  -1 FLOAT  index threshold: a variant with P at or below it may start a clump (default: 1e-4)\n"
	"  -2 FLOAT  secondary threshold: a variant with P at or below it may be claimed (default: 1e-2)\n"
	"  -o FILE   output text file (- for stdout; default: -)\n"
	"  -t INT    number of CPU threads used to unpack the input (default: maximum available)\n"
	"  -w INT    sliding window width in bases\n"
	"  -I STRING filter interval <contig>:pos-pos (see manual)\n"
	"  -p        force computations to use phased math\n"
	"  -u        force computations to use unphased math\n"
	"  -r FLOAT  Pearson's R-squared minimum cut-off value: pairs at or above it are in LD (default: 0.1)\n"
	"  -P FLOAT  accepted only as 1: clumping looks at every record, Fisher's test is not run\n"
	"  --engine-option KEY=INT  a switch of the GPU engine (twk_hip_set_option, include/twk_hip.h; repeatable)\n"
	"  (-c / -C are refused: the walk needs every pair)\n"
	"  (-r and -w keep calc's defaults: the same flags as calc mean the same pairs in LD)\n"
	"Output: '#' header lines, among them ##clumps=<index variants>,members=<claimed>,total=<variants>,edges=<pairs in LD>,\n"
	"        then per variant: contig <TAB> pos <TAB> P <TAB> index_contig <TAB> index_pos\n"
	"        (P: NA where the variant has none; index_contig, index_pos: . where it is in no clump;\n"
	"        an index variant names itself)\n"
	"Environment: TWK_HIP_DEVICE=<n> selects the GPU (default 0).\n" << std::endl;
}

static Took clump_option(int c, const char* arg, twk_ld_settings&, tomahawk::twk_clump_settings& clump) {
	if (c == 'a') { clump.assoc = arg; return took; }
	if (c != '1' && c != '2') return declined;
	char* end = nullptr;
	const double t = strtod(arg, &end);
	if (end == arg || *end || !(t >= 0 && t <= 1)) { fail(std::string("A clumping threshold (-") + (char)c + ") must be a P-value in [0, 1]"); return failed; }
	(c == '1' ? clump.p1 : clump.p2) = t;
	return took;
}
static const Command<tomahawk::twk_clump_settings> CLUMP = {      // (-r, -w: calc's defaults)
	"clump", "  clump    LD clumping by association P-value (an index variant per variant), decided on the GPU\n", clump_usage,
	"i:o:t:puP:r:w:I:c:C:a:1:2:?", REDUCE_LONG_OPTIONS, 0.1, {{"cC", "Cannot clump a part of the pair space (-c / -C): the walk needs every pair"}},
	"Cannot clump with a cutoff P-value below 1: clumping looks at every record and Fisher's exact test is not run", clump_option,
	[](twk_ld_settings&, tomahawk::twk_clump_settings& clump) {
		if (clump.assoc.empty()) return fail("No association file specified (-a)...");
		return !(clump.p1 > clump.p2) || fail("The index threshold (-1) cannot be above the secondary threshold (-2)");
	},
	[](tomahawk::twk_ld& ld, const twk_ld_settings& settings, const tomahawk::twk_clump_settings& clump) { return ld.Clump(settings, clump); }};

// `tomahawk ldmatrix` (not in the reference): the dense LD matrix of a region, filled on the GPU from the records `calc` would write.
static void ldmatrix_usage() {
	program_message();
	std::cerr <<
	"About:  The dense LD matrix of the selected variants - the input of fine-mapping (SuSiE, FINEMAP)\n"
	"        and of Bayesian polygenic scores (LDpred, PRS-CS): entry (u, v) is the chosen statistic of\n"
	"        the pair `calc` would report under the same options, and the fill value where it would\n"
	"        report none; r carries the sign of D.  The diagonal is 1 (for D: the fill value).  Filled\n"
	"        on the GPU (no .two is written); n x n x 4 bytes on the device and on the host.\n\n"
	"Usage:  tomahawk ldmatrix [options] -i <in.twk> -o <PREFIX>\n\n"
	"Options:\n"
	"  -i FILE   input Tomahawk (required)\n"
	"  -o PREFIX output prefix (required)\n"
	"  -s STRING statistic: r, r2, D or Dprime (default: r)\n"
	"  -f FLOAT  fill value of a pair without a record, nan allowed (default: 0)\n"
	"  -T        write PREFIX.ld (text) instead of PREFIX.npy\n"
	"  -t INT    number of CPU threads used to unpack the input (default: maximum available)\n"
	"  -w INT    sliding window width in bases: entries outside it are the fill value\n"
	"  -I STRING filter interval <contig>:pos-pos (see manual)\n"
	"  -p        force computations to use phased math\n"
	"  -u        force computations to use unphased math\n"
	"  -r FLOAT  Pearson's R-squared minimum cut-off value: entries below it are the fill value (default: 0)\n"
	"  -P FLOAT  accepted only as 1: the matrix holds every record, Fisher's test is not run\n"
	"  --engine-option KEY=INT  a switch of the GPU engine (twk_hip_set_option, include/twk_hip.h; repeatable)\n"
	"  (-c / -C are refused: the matrix needs every pair)\n"
	"  (-r defaults to 0, as for ldscore: calc's 0.1 would punch holes into a matrix meant for fine-mapping)\n"
	"Output: PREFIX.npy           the matrix as a NumPy file: float32, C order, shape (n, n); or, with -T,\n"
	"        PREFIX.ld            the matrix as text: one row per line, space-separated, 9 significant digits\n"
	"        PREFIX.variants.tsv  per row of the matrix: contig <TAB> pos\n"
	"Environment: TWK_HIP_DEVICE=<n> selects the GPU (default 0).\n" << std::endl;
}

static Took matrix_option(int c, const char* arg, twk_ld_settings&, tomahawk::twk_matrix_settings& matrix) {
	switch (c) {
	case 's': return stat_option(arg, tomahawk::LD_STATS, matrix.stat) ? took : failed;
	case 'f': return fill_option(arg, matrix.fill) ? took : failed;
	case 'T': matrix.text = true; return took;
	case 1003: matrix.band = true; return took;
	}
	return declined;
}
// (`ldmatrix --band -w INT`: the matrix in band storage, INTEGRATION section 1.  A long name only, and not in the usage text above: the usage and
// every recorded invocation answer as they always have, tests/golden/cli_transcript.json.)
static const Command<tomahawk::twk_matrix_settings> LDMATRIX = {
	"ldmatrix", "  ldmatrix dense LD matrix of a region (signed r, r2, D or D'), filled on the GPU\n", ldmatrix_usage,
	"i:o:t:puP:r:w:I:c:C:s:f:T?", REDUCE_LONG_OPTIONS, 0, {{"cC", "Cannot fill a part of the pair space (-c / -C): the matrix needs every pair"}},
	"Cannot fill a matrix with a cutoff P-value below 1: the matrix holds every record and Fisher's exact test is not run", matrix_option,
	[](twk_ld_settings& settings, tomahawk::twk_matrix_settings& matrix) {
		if (matrix.band && !settings.window) return fail("--band stores the columns inside the window: it needs one (-w)");
		if (matrix.band && matrix.text) return fail("--band has no text form (-T): it writes PREFIX.values.npy, PREFIX.indptr.npy and PREFIX.first.npy");
		return !(settings.out.empty() || settings.out == "-") || fail("No output prefix specified (-o)...");
	},
	[](tomahawk::twk_ld& ld, const twk_ld_settings& settings, const tomahawk::twk_matrix_settings& matrix) { return ld.Matrix(settings, matrix); }};

// `tomahawk blocks` (not in the reference): haplotype blocks by the rule of Gabriel et al., the D' confidence bounds formed and the blocks
// selected on the GPU.
static void blocks_usage() {
	program_message();
	std::cerr <<
	"About:  Haplotype blocks by the rule of Gabriel et al. (2002) - PLINK's --blocks, Haploview's default\n"
	"        view.  For every pair `calc` would report under the same options the 5 % / 95 % confidence\n"
	"        bounds of D' come from a likelihood scan of the pair's 2 x 2 haplotype table; a pair is strong\n"
	"        (lower bound >= 70, upper >= 98) or recombinant (upper < 90); a stretch of variants whose ends\n"
	"        are strong and of whose informative pairs more than 95 % are strong can be a block, and the\n"
	"        longest such stretches are taken first.  Computed and selected on the GPU (no .two is written).\n"
	"        Not PLINK's or Haploview's numbers: they add a LOD filter, their own MAF rule and, unphased, a\n"
	"        double-heterozygote term; here the table is the one `calc` reports.\n\n"
	"Usage:  tomahawk blocks [options] -i <in.twk> [-o <blocks.tsv>]\n\n"
	"Options:\n"
	"  -i FILE   input Tomahawk (required)\n"
	"  -o FILE   output text file (- for stdout; default: -)\n"
	"  -w INT    longest block, and the window of the computation, in bases (default: 200000)\n"
	"  -t INT    number of CPU threads used to unpack the input (default: maximum available)\n"
	"  -I STRING filter interval <contig>:pos-pos (see manual)\n"
	"  -p        force computations to use phased math\n"
	"  -u        force computations to use unphased math\n"
	"  -r FLOAT  Pearson's R-squared minimum cut-off value (default: 0)\n"
	"  -P FLOAT  accepted only as 1: blocks look at every record, Fisher's test is not run\n"
	"  --ci-out PREFIX  also write the bounds in band storage: PREFIX.lo.npy, PREFIX.hi.npy (uint8, 255: no\n"
	"            record), PREFIX.indptr.npy, PREFIX.first.npy and PREFIX.variants.tsv, as ldmatrix --band\n"
	"  --keep / --remove FILE, --extract / --exclude FILE, --maf, --max-maf, --mac, --geno, --hwe: as for calc\n"
	"  --engine-option KEY=INT  a switch of the GPU engine (twk_hip_set_option, include/twk_hip.h; repeatable)\n"
	"  (-c / -C are refused: a block needs every pair inside it)\n"
	"Output: '#' header lines, then per block, in file order:\n"
	"        contig <TAB> first pos <TAB> last pos <TAB> span <TAB> variants <TAB> strong pairs <TAB> recombinant pairs\n"
	"Environment: TWK_HIP_DEVICE=<n> selects the GPU (default 0).\n" << std::endl;
}
static const struct option BLOCKS_LONG_OPTIONS[] = {
	{"input", required_argument, 0, 'i'}, {"threads", optional_argument, 0, 't'}, {"output", required_argument, 0, 'o'},
	{"interval", optional_argument, 0, 'I'}, {"parts", optional_argument, 0, 'c'}, {"partStart", optional_argument, 0, 'C'},
	{"minP", optional_argument, 0, 'P'}, {"force-phased", no_argument, 0, 'p'}, {"force-unphased", no_argument, 0, 'u'},
	{"minR2", optional_argument, 0, 'r'}, {"windowBases", optional_argument, 0, 'w'},
	{"engine-option", required_argument, 0, 1000}, {"keep", required_argument, 0, 1006}, {"remove", required_argument, 0, 1007}, VARIANT_SELECTION_LONG_OPTIONS,
	{"ci-out", required_argument, 0, 1020}, {0, 0, 0, 0}};
static Took blocks_option(int c, const char* arg, twk_ld_settings&, tomahawk::twk_block_settings& blocks) {
	if (c != 1020) return declined;
	blocks.ci_out = arg;
	return !blocks.ci_out.empty() || fail("--ci-out wants a prefix") ? took : failed;
}
// (Reached by its name, but not a row of ENTRIES: the list of `tomahawk` without arguments and the "Illegal command" sentence answer as
// they always have, tests/golden/cli_transcript.json - as `ldmatrix --band` stays out of ldmatrix's usage.)
static const Command<tomahawk::twk_block_settings> BLOCKS = {
	"blocks", "  blocks   haplotype blocks (Gabriel et al.), D' confidence bounds and block walk on the GPU\n", blocks_usage,
	"i:o:t:puP:r:w:I:c:C:?", BLOCKS_LONG_OPTIONS, 0, {{"cC", "Cannot find the blocks of a part of the pair space (-c / -C): a block needs every pair inside it"}},
	"Cannot find blocks with a cutoff P-value below 1: blocks look at every record and Fisher's exact test is not run", blocks_option,
	nullptr,
	[](tomahawk::twk_ld& ld, const twk_ld_settings& settings, const tomahawk::twk_block_settings& blocks) { return ld.Blocks(settings, blocks); }};

// `tomahawk ldsplit` (not in the reference): every contig split into near-independent LD blocks, the dynamic programme solved on the GPU.
static void ldsplit_usage() {
	program_message();
	std::cerr <<
	"About:  Optimal LD splitting (Prive 2021; bigsnpr's snp_ldsplit): where to cut every contig into K blocks\n"
	"        of --min-size to --max-size variants so that as little r2 as possible crosses a cut, for every K\n"
	"        up to --max-blocks.  The r2 is that of every pair `calc` would report under the same options\n"
	"        inside the window; the banded r2 matrix stays on the GPU and the dynamic programme runs there, in\n"
	"        integers of 2^-32 (no .two is written).  Not bigsnpr's max_r2 constraint, not LDetect's rule.\n\n"
	"Usage:  tomahawk ldsplit [options] -i <in.twk> -w <bases> --min-size m --max-size M --max-blocks K -o <PREFIX>\n\n"
	"Options:\n"
	"  -i FILE   input Tomahawk (required)\n"
	"  -o PREFIX output prefix (required): PREFIX.costs.tsv, and with -B PREFIX.blocks.tsv\n"
	"  -w INT    window in bases: pairs further apart count as r2 = 0 (required)\n"
	"  --min-size INT    smallest block in variants (required, >= 1)\n"
	"  --max-size INT    largest block in variants (required, <= 65535)\n"
	"  --max-blocks INT  largest number of blocks a contig is split into (required, <= 1024)\n"
	"  -B INT    also write every contig's partition into this many blocks\n"
	"  -t INT    number of CPU threads used to unpack the input (default: maximum available)\n"
	"  -I STRING filter interval <contig>:pos-pos (see manual)\n"
	"  -p        force computations to use phased math\n"
	"  -u        force computations to use unphased math\n"
	"  -r FLOAT  Pearson's R-squared minimum cut-off value (default: 0)\n"
	"  -P FLOAT  accepted only as 1: a split looks at every record, Fisher's test is not run\n"
	"  --keep / --remove FILE, --extract / --exclude FILE, --maf, --max-maf, --mac, --geno, --hwe: as for calc\n"
	"  --engine-option KEY=INT  a switch of the GPU engine (twk_hip_set_option, include/twk_hip.h; repeatable)\n"
	"  (-c / -C are refused: a block sum needs every pair inside the block)\n"
	"Output: PREFIX.costs.tsv, '#' header lines, then per contig and feasible K:\n"
	"        contig <TAB> K <TAB> cost <TAB> cost / total <TAB> sum of squared block sizes\n"
	"        PREFIX.blocks.tsv (-B): contig <TAB> block <TAB> first pos <TAB> last pos <TAB> variants\n"
	"Environment: TWK_HIP_DEVICE=<n> selects the GPU (default 0).\n" << std::endl;
}
static const struct option LDSPLIT_LONG_OPTIONS[] = {
	{"input", required_argument, 0, 'i'}, {"threads", optional_argument, 0, 't'}, {"output", required_argument, 0, 'o'},
	{"interval", optional_argument, 0, 'I'}, {"parts", optional_argument, 0, 'c'}, {"partStart", optional_argument, 0, 'C'},
	{"minP", optional_argument, 0, 'P'}, {"force-phased", no_argument, 0, 'p'}, {"force-unphased", no_argument, 0, 'u'},
	{"minR2", optional_argument, 0, 'r'}, {"windowBases", optional_argument, 0, 'w'},
	{"engine-option", required_argument, 0, 1000}, {"keep", required_argument, 0, 1006}, {"remove", required_argument, 0, 1007}, VARIANT_SELECTION_LONG_OPTIONS,
	{"min-size", required_argument, 0, 1030}, {"max-size", required_argument, 0, 1031}, {"max-blocks", required_argument, 0, 1032}, {"blocks", required_argument, 0, 'B'}, {0, 0, 0, 0}};
static Took ldsplit_option(int c, const char* arg, twk_ld_settings&, tomahawk::twk_split_settings& split) {
	uint32_t* where = c == 1030 ? &split.min_size : c == 1031 ? &split.max_size : c == 1032 ? &split.max_blocks : c == 'B' ? &split.blocks : nullptr;
	if (!where) return declined;
	const char* name = c == 1030 ? "--min-size" : c == 1031 ? "--max-size" : c == 1032 ? "--max-blocks" : "-B";
	const uint32_t top = c == 1032 || c == 'B' ? 1024 : 65535;
	const std::string a(arg);      // an unsigned integer, digits only
	if (a.empty() || a.size() > 6 || a.find_first_not_of("0123456789") != std::string::npos || strtoul(arg, nullptr, 10) < 1 || strtoul(arg, nullptr, 10) > top) {
		char why[96]; snprintf(why, sizeof(why), "%s wants an integer between 1 and %u", name, top); fail(why); return failed;
	}
	*where = (uint32_t)strtoul(arg, nullptr, 10);
	return took;
}
static bool ldsplit_check(twk_ld_settings& settings, tomahawk::twk_split_settings& split) {
	if (!split.min_size || !split.max_size || !split.max_blocks) return fail("A split needs --min-size, --max-size and --max-blocks");
	if (split.min_size > split.max_size) return fail("Cannot have --min-size above --max-size");
	if (split.blocks > split.max_blocks) return fail("Cannot write a partition of more blocks (-B) than --max-blocks");
	if (!settings.window) return fail("A split needs a window in bases (-w)");
	if (settings.out.empty() || settings.out == "-") return fail("A split writes PREFIX.costs.tsv and PREFIX.blocks.tsv: -o wants a prefix");
	return true;
}
// (Reached by its name, but not a row of ENTRIES, as `blocks`: the list of `tomahawk` without arguments answers as recorded.)
static const Command<tomahawk::twk_split_settings> LDSPLIT = {
	"ldsplit", "  ldsplit  optimal near-independent LD blocks (Prive 2021), the dynamic programme solved on the GPU\n", ldsplit_usage,
	"i:o:t:puP:r:w:I:c:C:B:?", LDSPLIT_LONG_OPTIONS, 0, {{"cC", "Cannot split a part of the pair space (-c / -C): a block sum needs every pair inside the block"}},
	"Cannot split with a cutoff P-value below 1: a split looks at every record and Fisher's exact test is not run", ldsplit_option,
	ldsplit_check,
	[](tomahawk::twk_ld& ld, const twk_ld_settings& settings, const tomahawk::twk_split_settings& split) { return ld.Split(settings, split); }};

// `tomahawk relationship`: the sample-by-sample matrix (IBS, IBS0 or KING kinship), counted on the GPU.  The reference's name and its -i / -I;
// its numbers are not reproduced (include/twk_hip.h, twk_hip_relationship).
static void relationship_usage() {
	program_message();
	std::cerr <<
	"About:  The sample relationship matrix - what a cohort is checked with for duplicates and relatives\n"
	"        before any LD: per pair of samples, over the selected variants at which both are non-missing,\n"
	"        n, IBS0 (opposite homozygotes), IBS2 (same genotype) and the heterozygote counts, exact\n"
	"        integers counted on the GPU, and one statistic of them:\n"
	"          ibs   (n + ibs2 - ibs0) / (2 n)                mean allele sharing\n"
	"          ibs0  ibs0 / n\n"
	"          king  (hethet - 2 ibs0) / (het_a + het_b)      KING-robust kinship (0.5 duplicate, 0.25 first degree)\n"
	"        The reference's `relationship` is not reproduced: it skips the first sample of every run,\n"
	"        scores het/het differently inside and across runs, leaves column 0 empty and divides by the\n"
	"        number of variants whatever is missing.\n\n"
	"Usage:  tomahawk relationship -i <in.twk> [-I interval ...] [-s ibs|ibs0|king] [-f fill] [-o PREFIX [-T]]\n\n"
	"Options:\n"
	"  -i FILE   input Tomahawk (required)\n"
	"  -I STRING filter interval <contig>:pos-pos (repeatable; default: every variant)\n"
	"  -s STRING statistic: ibs, ibs0 or king (default: king)\n"
	"  -f FLOAT  fill value of a pair whose denominator is 0, nan allowed (default: nan)\n"
	"  -o PREFIX output prefix (default: the matrix as text on stdout)\n"
	"  -T        with -o: write PREFIX.tsv (text) instead of PREFIX.npy\n"
	"  -t INT    number of CPU threads used to unpack the input (default: maximum available)\n"
	"  --engine-option KEY=INT  a switch of the GPU engine (twk_hip_set_option, include/twk_hip.h; repeatable)\n"
	"  (-p, -u, -r, -w, -c, -C and -P are refused: samples are compared genotype by genotype over every selected variant)\n"
	"Output: without -o       the matrix on stdout: one row per sample, tab-separated, 17 significant digits\n"
	"        PREFIX.npy          the matrix as a NumPy file: float64, C order, shape (n, n); or, with -T,\n"
	"        PREFIX.tsv          the matrix as text, as on stdout\n"
	"        PREFIX.samples.tsv  one sample name per row of the matrix, from the input's header\n"
	"Environment: TWK_HIP_DEVICE=<n> selects the GPU (default 0).\n" << std::endl;
}

static Took relationship_option(int c, const char* arg, twk_ld_settings&, tomahawk::twk_relationship_settings& rel) {
	switch (c) {
	case 's': return stat_option(arg, tomahawk::REL_STATS, rel.stat) ? took : failed;
	case 'f': return fill_option(arg, rel.fill) ? took : failed;
	case 'T': rel.text = true; return took;
	}
	return declined;
}
static const Command<tomahawk::twk_relationship_settings> RELATIONSHIP = {
	"relationship", "  relationship  sample-by-sample matrix (IBS, IBS0 or KING kinship), counted on the GPU\n", relationship_usage,
	"i:I:s:f:o:Tt:pur:w:c:C:P:?", RELATIONSHIP_LONG_OPTIONS, 0.1,
	{{"pu", "Cannot force a phasing (-%c): samples are compared by genotype, phase is ignored"},
	 {"r", "Cannot apply an R-squared cut-off (-r): no variant pair is formed"},
	 {"w", "Cannot apply a window (-w): samples are compared over every selected variant"},
	 {"cC", "Cannot relate over a part of the pair space (-%c): samples are compared over every selected variant"},
	 {"P", "Cannot apply a cutoff P-value (-P): the matrix is counted, no test is run"}},
	nullptr, relationship_option,
	[](twk_ld_settings& settings, tomahawk::twk_relationship_settings& rel) {
		return !(rel.text && (settings.out.empty() || settings.out == "-")) || fail("-T names the file written for -o PREFIX: without -o the text goes to stdout anyway");
	},
	[](tomahawk::twk_ld& ld, const twk_ld_settings& settings, const tomahawk::twk_relationship_settings& rel) { return ld.Relationship(settings, rel); }};

// `tomahawk lddecay`: mean r2 by the distance between two variants over the records `calc` would write, binned and summed on the GPU.  (The
// reference's `decay` reads a .two file, and its range is -w; here -w keeps calc's meaning, the window of the computation.)
static void lddecay_usage() {
	program_message();
	std::cerr <<
	"About:  LD decay: R-squared as a function of the distance between two variants.  Every pair `calc`\n"
	"        would report under the same options, with both variants on one contig at different\n"
	"        positions, falls into the bin of its distance; per bin the pairs are counted and their\n"
	"        R-squared summed exactly on the GPU (no .two is written).  The last bin also takes every\n"
	"        pair beyond the range.\n\n"
	"Usage:  tomahawk lddecay [options] -i <in.twk> [-o <out.tsv>]\n\n"
	"Options:\n"
	"  -i FILE   input Tomahawk (required)\n"
	"  -o FILE   output text file (- for stdout; default: -)\n"
	"  -d INT    range in bases the bins cover (default: 10000000, or the -w window when only -w is given)\n"
	"  -b INT    number of bins, 1 to 4096 (default: 1000); a bin is -d / -b bases wide\n"
	"  -t INT    number of CPU threads used to unpack the input (default: maximum available)\n"
	"  -c INT    number of subproblems to split compute into (must be in (c!2 + c))\n"
	"  -C INT    chosen part to compute (0 < -C < -c)\n"
	"  -w INT    sliding window width in bases: pairs further apart are not computed\n"
	"  -I STRING filter interval <contig>:pos-pos (see manual)\n"
	"  -p        force computations to use phased math\n"
	"  -u        force computations to use unphased math\n"
	"  -r FLOAT  Pearson's R-squared minimum cut-off value (default: 0)\n"
	"  -P FLOAT  accepted only as 1: a decay curve averages over every record, Fisher's test is not run\n"
	"  --engine-option KEY=INT  a switch of the GPU engine (twk_hip_set_option, include/twk_hip.h; repeatable)\n"
	"Output: '#' header lines, then per bin: From <TAB> To <TAB> Mean <TAB> Frequency <TAB> Sum\n"
	"        (Mean = Sum / Frequency, 0 for an empty bin)\n"
	"Environment: TWK_HIP_DEVICE=<n> selects the GPU (default 0).\n" << std::endl;
}

static const std::string ONE_TO_MAX_BINS = "between 1 and " + std::to_string(tomahawk::MAX_BINS);
struct DecayOptions { tomahawk::twk_decay_settings decay; bool range_given = false; };
static Took decay_option(int c, const char* arg, twk_ld_settings&, DecayOptions& own) {
	double v = 0;
	if (c == 'd') {
		if (!integer_option(arg, "range (-d)", 1, (double)tomahawk::MAX_RANGE_BP, "between 1 and " + std::to_string(tomahawk::MAX_RANGE_BP) + " bases", v)) return failed;
		own.decay.range_bp = (int64_t)v; own.range_given = true;
		return took;
	}
	if (c != 'b') return declined;
	if (!integer_option(arg, "number of bins (-b)", 1, tomahawk::MAX_BINS, ONE_TO_MAX_BINS, v)) return failed;
	own.decay.n_bins = (int32_t)v;
	return took;
}
static const Command<DecayOptions> LDDECAY = {
	"lddecay", "  lddecay  LD decay: R-squared by the distance between two variants, binned and summed on the GPU\n", lddecay_usage,
	"i:o:t:puP:r:w:I:c:C:d:b:?", REDUCE_LONG_OPTIONS, 0, {},
	"Cannot bin with a cutoff P-value below 1: a decay curve averages over every record and Fisher's exact test is not run", decay_option,
	[](twk_ld_settings& settings, DecayOptions& own) {
		tomahawk::twk_decay_settings& d = own.decay;
		if (!own.range_given && settings.window) d.range_bp = settings.l_window;      // (only -w given: no pair lies further apart)
		return d.range_bp >= d.n_bins || fail("The range (-d, or -w without -d: " + std::to_string(d.range_bp) + ") cannot be smaller than the number of bins (-b: " + std::to_string(d.n_bins) + "): a bin would be 0 bases wide");
	},
	[](tomahawk::twk_ld& ld, const twk_ld_settings& settings, const DecayOptions& own) { return ld.Decay(settings, own.decay); }};

// `tomahawk ldaggregate`: the LD of every record `calc` would write rasterised into x-by-y cells, binned and summed on the GPU.  (The
// reference's `aggregate` reads a .two file and writes a binary .twa; its -c, the minimum count, is -m here: -c is the chunk flag.)
static void ldaggregate_usage() {
	program_message();
	std::cerr <<
	"About:  LD aggregate: the pairwise LD of a region rasterised into an x-by-y heat map.  Every pair\n"
	"        `calc` would report under the same options adds its statistic to cell (x(A), y(B)) and to\n"
	"        cell (x(B), y(A)); per cell the contributions are counted and summed exactly on the GPU\n"
	"        (no .two is written).  One contig: the axes span the data's range; several: every contig\n"
	"        present at its whole length, one after the other.\n\n"
	"Usage:  tomahawk ldaggregate [options] -i <in.twk> [-o <out.tsv>]\n\n"
	"Options:\n"
	"  -i FILE   input Tomahawk (required)\n"
	"  -o FILE   output text file (- for stdout; default: -)\n"
	"  -x INT    number of bins on the x axis, 1 to 4096 (default: 1000)\n"
	"  -y INT    number of bins on the y axis, 1 to 4096 (default: 1000)\n"
	"  -s STRING statistic: r2, r (signed), D or Dprime (default: r2)\n"
	"  -R STRING reduction of a cell: mean, count (or n), min, max, sd or total (default: mean)\n"
	"  -m INT    minimum count of a cell: a cell with fewer contributions prints 0 (default: 5)\n"
	"  -t INT    number of CPU threads used to unpack the input (default: maximum available)\n"
	"  -c INT    number of subproblems to split compute into (must be in (c!2 + c))\n"
	"  -C INT    chosen part to compute (0 < -C < -c)\n"
	"  -w INT    sliding window width in bases: pairs further apart are not computed\n"
	"  -I STRING filter interval <contig>:pos-pos (see manual)\n"
	"  -p        force computations to use phased math\n"
	"  -u        force computations to use unphased math\n"
	"  -r FLOAT  Pearson's R-squared minimum cut-off value (default: 0)\n"
	"  -P FLOAT  accepted only as 1: an aggregate takes in every record, Fisher's test is not run\n"
	"  --engine-option KEY=INT  a switch of the GPU engine (twk_hip_set_option, include/twk_hip.h; repeatable)\n"
	"Output: '#' comment lines (x, y, bases per bin, range, each contig's offset), then x rows of y\n"
	"        tab-separated values (mean = sum / n; sd = sqrt(sum_sq / n - mean^2), at least 0)\n"
	"Environment: TWK_HIP_DEVICE=<n> selects the GPU (default 0).\n" << std::endl;
}

static Took aggregate_option(int c, const char* arg, twk_ld_settings&, tomahawk::twk_aggregate_settings& a) {
	double v = 0;
	switch (c) {
	case 'x': case 'y':
		if (!integer_option(arg, c == 'x' ? "number of x bins (-x)" : "number of y bins (-y)", 1, tomahawk::MAX_BINS, ONE_TO_MAX_BINS, v)) return failed;
		(c == 'x' ? a.x_bins : a.y_bins) = (int32_t)v;
		return took;
	case 'm':
		if (!integer_option(arg, "minimum count (-m)", 0, 9007199254740992.0, "at most 2^53", v)) return failed;
		a.min_count = (int64_t)v;
		return took;
	case 'R':
		a.reduce = strcmp(arg, "n") == 0 ? (int32_t)tomahawk::TWK_AGGREGATE_COUNT : tomahawk::AGGREGATE_REDUCTIONS.value(arg);
		if (a.reduce < 0) { fail(std::string("Unknown reduction (-R): ") + arg + " - one of mean, count, n, min, max, sd, total"); return failed; }
		return took;
	case 's': return stat_option(arg, tomahawk::LD_STATS, a.stat) ? took : failed;
	}
	return declined;
}
static const Command<tomahawk::twk_aggregate_settings> LDAGGREGATE = {
	"ldaggregate", "  ldaggregate  LD aggregate: r2, r, D or D' rasterised into x-by-y bins, summed exactly on the GPU\n", ldaggregate_usage,
	"i:o:t:puP:r:w:I:c:C:x:y:s:R:m:?", REDUCE_LONG_OPTIONS, 0, {},
	"Cannot aggregate with a cutoff P-value below 1: an aggregate takes in every record and Fisher's exact test is not run", aggregate_option, nullptr,
	[](tomahawk::twk_ld& ld, const twk_ld_settings& settings, const tomahawk::twk_aggregate_settings& a) { return ld.Aggregate(settings, a); }};

// `tomahawk concat` (lib/concat.h:63-251): copy the compressed blocks of several .two files into one.
static int concat(int argc, char** argv) {
	if (argc < 3) {
		program_message();
		std::cerr << "About:  Concatenate two or more TWO files\n\n"
		             "Usage:  tomahawk concat [options] -i <in.two> -i <in.two> -o <out.two>\n\n"
		             "Options:\n  -i FILE    input TWO file specified 1-or-more times (required)\n"
		             "  -I STRING  input file list (required)\n  -o FILE    output file (- for stdout; default: -)\n" << std::endl;
		return 0;
	}
	std::vector<std::string> in_list, lists;
	std::string out = "-";
	int c;
	while ((c = getopt(argc, argv, "i:I:o:?")) != -1) {
		switch (c) {
		case 'i': in_list.push_back(optarg); break;
		case 'I': lists.push_back(optarg); break;
		case 'o': out = optarg; break;
		default: fprintf(stderr, "%s: option `-%c' is invalid: ignored\n", argv[0], optopt); break;
		}
	}
	for (const auto& l : lists) {
		std::ifstream f(l);
		if (!f.good()) { std::cerr << "faield to open list=" << l << std::endl; return 1; }
		std::string line;
		while (std::getline(f, line)) if (!line.empty()) in_list.push_back(line);
	}
	if (in_list.empty()) { std::cerr << stamp("ERROR") << "No input value specified..." << std::endl; return 1; }
	if (in_list.size() == 1) { std::cerr << stamp("ERROR") << "Only one input file provided..." << std::endl; return 1; }
	if (out != "-") {      // extension forced to .two like calc (concat.h:163-171)
		const size_t sl = out.find_last_of("/\\"), dot = out.rfind('.');
		const std::string ext = (dot == std::string::npos || (sl != std::string::npos && dot < sl)) ? "" : out.substr(dot + 1);
		if (!(ext.size() == 3 && strncasecmp(ext.c_str(), "two", 3) == 0)) out += ".two";
	}
	char date[64]; time_t t = time(nullptr); struct tm now; localtime_r(&t, &now);
	strftime(date, sizeof(date), "%Y-%m-%d %H:%M:%S", &now);
	const std::string note = "\n##tomahawk_concatVersion=mi355x\n##tomahawk_concatCommand=" + tomahawk::LITERAL_COMMAND_LINE + "; Date=" + date;
	std::string err;
	std::cerr << stamp("LOG") << "Concatenating " << in_list.size() << " files into " << out << "..." << std::endl;
	if (!tomahawk::two_concat(in_list, out, note, err)) { std::cerr << stamp("ERROR") << err << std::endl; return 1; }
	return 0;
}

// `tomahawk view` (lib/view.h:28-459): same flags; -h prints the header only and -H drops it,
// as the reference's option switch has them (view.h:367-368).
static void view_usage() {
	program_message();
	std::cerr <<
	"About:  Convert binary TWO->LD/TWO, subset and slice TWO data\n\n"
	"Usage:  tomahawk view [options] -i <in.two>\n\n"
	"Options:\n"
	"  -i FILE   input TWO file (required)\n"
	"  -h/H      (twk/two) header only / no header\n"
	"  -I STRING filter interval <contig>:pos-pos (TWK/TWO) or linked interval <contig>:pos-pos,<contig>:pos-pos\n\n"
	"  -o FILE    output file (- for stdout; default: -)\n"
	"  -O <b|u>   b: compressed TWO, u: uncompressed LD\n\n"
	"Filter parameters:\n"
	"  -r,-R --minR2,--maxR2   FLOAT   Pearson's R-squared min/max cut-off value\n"
	"  -z,-Z --minR,--maxR     FLOAT   Pearson's R min/max cut-off value\n"
	"  -p,-P --minP,--maxP     FLOAT   Min/max P-value (default: [0,1])\n"
	"  -d,-D --minD,--maxD     FLOAT   Min/max D value (default: [-1,1])\n"
	"  -b,-B --minDP,--maxDP   FLOAT   Min/max D' value (default: [0,1])\n"
	"  -1,-5 --minP1,--maxP1   FLOAT   Min/max REF_REF count (default: [0,inf])\n"
	"  -2,-6 --minP2,--maxP2   FLOAT   Min/max REF_ALT count (default: [0,inf])\n"
	"  -3,-7 --minQ1,--maxQ1   FLOAT   Min/max ALT_REF count (default: [0,inf])\n"
	"  -4,-8 --minQ2,--maxQ1   FLOAT   Min/max ALT_ALT count (default: [0,inf])\n"
	"  -a,-A --minMHC,--maxMHC FLOAT   Min/max number of non-major haplotype count (default: [0,inf])\n"
	"  -x,-X --minChi,--maxChi FLOAT   Min/max Chi-squared CV of contingency table (default: [0,inf])\n"
	"  -m,-M --minMCV,--maxMCV FLOAT   Min/max Chi-squared CV of unphased model (default: [0,inf])\n"
	"  -f  INT  include FLAG value\n"
	"  -F  INT  exclude FLAG value\n"
	"  -u       output only the upper triangular values\n"
	"  -l       output only the lower triangular values\n"
	"  -t INT   number of worker threads (default: all; not in the reference)\n";
}

static int view(int argc, char** argv) {
	if (argc < 3) { view_usage(); return 0; }
	static struct option long_options[] = {
		{"input", required_argument, 0, 'i'}, {"output", optional_argument, 0, 'o'}, {"output-type", optional_argument, 0, 'O'},
		{"minP", optional_argument, 0, 'p'}, {"maxP", optional_argument, 0, 'P'}, {"minR", optional_argument, 0, 'z'},
		{"maxR", optional_argument, 0, 'Z'}, {"minR2", optional_argument, 0, 'r'}, {"maxR2", optional_argument, 0, 'R'},
		{"minDP", optional_argument, 0, 'b'}, {"maxDP", optional_argument, 0, 'B'}, {"minD", optional_argument, 0, 'd'},
		{"maxD", optional_argument, 0, 'D'}, {"minP1", optional_argument, 0, '1'}, {"minP2", optional_argument, 0, '2'},
		{"minQ1", optional_argument, 0, '3'}, {"minQ2", optional_argument, 0, '4'}, {"maxP1", optional_argument, 0, '5'},
		{"maxP2", optional_argument, 0, '6'}, {"maxQ1", optional_argument, 0, '7'}, {"maxQ2", optional_argument, 0, '8'},
		{"minMHC", optional_argument, 0, 'a'}, {"maxMHC", optional_argument, 0, 'A'}, {"minChi", optional_argument, 0, 'x'},
		{"maxChi", optional_argument, 0, 'X'}, {"minMCV", optional_argument, 0, 'm'}, {"maxMCV", optional_argument, 0, 'M'},
		{"flagInclude", optional_argument, 0, 'f'}, {"flagExclude", optional_argument, 0, 'F'},
		{"upperTriangular", no_argument, 0, 'u'}, {"lowerTriangular", no_argument, 0, 'l'},
		{"headerOnly", no_argument, 0, 'H'}, {"noHeader", no_argument, 0, 'h'}, {"interval", optional_argument, 0, 'I'},
		{"threads", required_argument, 0, 't'}, {0, 0, 0, 0}};
	static const std::regex re_float("^[-+]?[0-9]*\\.?[0-9]+([eE][-+]?[0-9]+)?$"), re_number("^[0-9]+$");   // tomahawk.h:61-62
	tomahawk::two_view_settings st;
	tomahawk::TwoFilter& f = st.filter;
	using F = tomahawk::TwoFilter;
	int c = 0, long_index = 0;
	while ((c = getopt_long(argc, argv, "i:HhI:o:O:r:R:z:Z:p:P:d:D:b:B:1:2:3:4:5:6:7:8:x:X:a:A:m:M:f:F:ult:", long_options, &long_index)) != -1) {
		double* dst = nullptr; F::Bit bit = F::R2;
		switch (c) {
		case ':': fprintf(stderr, "%s: option `-%c' requires an argument\n", argv[0], optopt); continue;
		case '?': default: fprintf(stderr, "%s: option `-%c' is invalid: ignored\n", argv[0], optopt); continue;
		case 'i': st.in = optarg; continue;
		case 'o': st.out = optarg; continue;
		case 'O': if (std::string(optarg).size() != 1) { std::cerr << "illegal O" << std::endl; return 1; } st.mode = optarg[0]; continue;
		case 'u': f.set(F::UPPER); continue;
		case 'l': f.set(F::LOWER); continue;
		case 'h': st.header_only = true; continue;
		case 'H': st.write_header = false; continue;
		case 'I': st.ivals.push_back(optarg); continue;
		case 't': st.n_threads = atoi(optarg); continue;
		case 'f': case 'F':
			if (!std::regex_match(std::string(optarg), re_number)) { std::cerr << "not a valid number" << std::endl; return 1; }
			(c == 'f' ? f.flag_include : f.flag_exclude) = (uint32_t)atof(optarg); f.set(F::FLAGS); continue;
		case 'p': dst = &f.minP; bit = F::P; break;          case 'P': dst = &f.maxP; bit = F::P; break;
		case 'z': dst = &f.minR; bit = F::R; break;          case 'Z': dst = &f.maxR; bit = F::R; break;
		case 'r': dst = &f.minR2; bit = F::R2; break;        case 'R': dst = &f.maxR2; bit = F::R2; break;
		case 'b': dst = &f.minDprime; bit = F::DPRIME; break; case 'B': dst = &f.maxDprime; bit = F::DPRIME; break;
		case 'd': dst = &f.minD; bit = F::D; break;          case 'D': dst = &f.maxD; bit = F::D; break;
		case '1': dst = &f.hA_min; bit = F::HAPA; break;     case '5': dst = &f.hA_max; bit = F::HAPA; break;
		case '2': dst = &f.hB_min; bit = F::HAPB; break;     case '6': dst = &f.hB_max; bit = F::HAPB; break;
		case '3': dst = &f.hC_min; bit = F::HAPC; break;     case '7': dst = &f.hC_max; bit = F::HAPC; break;
		case '4': dst = &f.hD_min; bit = F::HAPD; break;     case '8': dst = &f.hD_max; bit = F::HAPD; break;
		case 'a': dst = &f.mhc_min; bit = F::MHC; break;     case 'A': dst = &f.mhc_max; bit = F::MHC; break;
		case 'x': dst = &f.minChi; bit = F::CHI; break;      case 'X': dst = &f.maxChi; bit = F::CHI; break;
		case 'm': dst = &f.minChiModel; bit = F::CHIMODEL; break; case 'M': dst = &f.maxChiModel; bit = F::CHIMODEL; break;
		}
		if (!std::regex_match(std::string(optarg), re_float)) { std::cerr << "not a valid float" << std::endl; return 1; }
		*dst = atof(optarg); f.set(bit);
	}
	if (st.in.empty()) { std::cerr << stamp("ERROR") << "No input value specified..." << std::endl; return 1; }
	if (!(st.out.empty() || st.out == "-")) program_message();
	if (st.n_threads <= 0) st.n_threads = 1;
	return tomahawk::two_view(st);
}

// `tomahawk import` (lib/import.h:28-131): VCF text (plain / gzip) -> .twk
static int import_cmd(int argc, char** argv) {
	if (argc < 3) {
		program_message();
		std::cerr << "About:  Convert VCF->TWK\n\nUsage:  tomahawk import [options] -i <in.vcf[.gz]> -o <out.twk>\n\nOptions:\n"
		             "  -i FILE  input VCF (plain or gzip/bgzip text) or BCF2, '-' for stdin (required)\n  -o FILE  output file prefix (required)\n"
		             "  -n FLOAT missingness fraction in range [0,1] (default: 0.9)\n  -H FLOAT Hardy-Weinberg P-value cutoff (default: 0)\n"
		             "  -r       do not filter out univariate sites\n  -f       flip reference and alternative alleles when the major allele is the alternative (no effect, as in the reference)\n"
		             "  -b INT   number of variants per block (default: 500)\n  -L INT   compression level 1-20 (default: 1)\n"
		             "  -t INT   parser threads (default: all; not in the reference)\n\n";
		return 1;
	}
	static struct option long_options[] = {{"input", required_argument, 0, 'i'}, {"output", optional_argument, 0, 'o'},
		{"filter-univariate", optional_argument, 0, 'r'}, {"flip", optional_argument, 0, 'f'}, {"missingness", optional_argument, 0, 'n'},
		{"compression-level", optional_argument, 0, 'L'}, {"block-size", optional_argument, 0, 'b'}, {"hwe", optional_argument, 0, 'H'},
		{"threads", required_argument, 0, 't'}, {0, 0, 0, 0}};
	tomahawk::twk_vimport_settings st;
	int c = 0, option_index = 0;
	while ((c = getopt_long(argc, argv, "i:o:rfn:b:L:H:t:?", long_options, &option_index)) != -1) {
		switch (c) {
		case 'i': st.input = optarg; break;
		case 'o': st.output = optarg; break;
		case 'n':
			st.threshold_miss = (float)atof(optarg);
			if (st.threshold_miss < 0) { std::cerr << stamp("ERROR") << "Cannot set missingness filter to < 0..." << std::endl; return 1; }
			if (st.threshold_miss > 1) { std::cerr << stamp("ERROR") << "Cannot set missingness filter to > 1..." << std::endl; return 1; }
			break;
		case 'H':
			st.hwe = atof(optarg);
			if (st.hwe < 0) { std::cerr << stamp("ERROR") << "Cannot set Hardy-Weinberg filter to < 0..." << std::endl; return 1; }
			if (st.hwe > 1) { std::cerr << stamp("ERROR") << "Cannot set Hardy-Weinberg filter to > 1..." << std::endl; return 1; }
			break;
		case 'r': st.remove_univariate = false; break;
		case 'f': st.flip_major_minor = false; break;          // import.h:92-94
		case 'b': st.block_size = (uint32_t)atoi(optarg); break;
		case 'L': st.c_level = (uint8_t)atoi(optarg); break;
		case 't': st.n_threads = atoi(optarg); break;
		default: std::cerr << stamp("ERROR") << "Unrecognized option: " << (char)c << std::endl; return 1;
		}
	}
	if (st.input.empty()) { std::cerr << stamp("ERROR") << "No input value specified..." << std::endl; return 1; }
	if (st.output.empty()) { std::cerr << stamp("ERROR") << "No output value specified..." << std::endl; return 1; }
	if (st.block_size == 0) { std::cerr << stamp("ERROR") << "Cannot set the block size to 0..." << std::endl; return 1; }
	program_message();
	std::cerr << stamp("LOG") << "Calling import..." << std::endl;
	tomahawk::twk_variant_importer importer;
	if (!importer.Import(st)) { std::cerr << "failed import" << std::endl; return 1; }
	return 0;
}

// `tomahawk sort` (lib/sort.h:28-124)
static int sort_cmd(int argc, char** argv) {
	if (argc < 3) {
		program_message();
		std::cerr << "About:  Sort TWO files\n\nUsage:  tomahawk sort [options] -i <in.two>\n\nOptions:\n"
		             "  -i FILE   input TWO file (required)\n  -o FILE   output file (- for stdout; default: -)\n"
		             "  -m FLOAT  maximum memory usage per thread in GB (default: 0.5)\n"
		             "  -c INT    compression level 1-20 (default: 1)\n  -t INT    number of threads (default: maximum available)\n\n";
		return 0;
	}
	static struct option long_options[] = {{"input", required_argument, 0, 'i'}, {"output", optional_argument, 0, 'o'},
		{"memory-usage", optional_argument, 0, 'm'}, {"compression-level", optional_argument, 0, 'c'},
		{"threads", optional_argument, 0, 't'}, {0, 0, 0, 0}};
	tomahawk::two_sorter_settings st;
	int c = 0, long_index = 0;
	while ((c = getopt_long(argc, argv, "i:o:m:c:t:?", long_options, &long_index)) != -1) {
		switch (c) {
		case 'i': st.in = optarg; break;
		case 'o': st.out = optarg; break;
		case 'm': st.memory_limit = (float)atof(optarg); break;
		case 'c': st.c_level = atoi(optarg); break;
		case 't': st.n_threads = atoi(optarg); break;
		default: fprintf(stderr, "%s: option `-%c' is invalid: ignored\n", argv[0], optopt); break;
		}
	}
	if (st.in.empty()) { std::cerr << stamp("ERROR") << "No input value specified..." << std::endl; return 1; }
	if (st.memory_limit <= 0) { std::cerr << stamp("ERROR") << "Cannot set memory limit <= 0..." << std::endl; return 1; }
	if (st.n_threads <= 0) { std::cerr << stamp("ERROR") << "Cannot set number of threads <= 0..." << std::endl; return 1; }
	if (st.c_level <= 0) { std::cerr << stamp("ERROR") << "Cannot set the compression level <= 0..." << std::endl; return 1; }
	program_message();
	std::cerr << stamp("LOG") << "Calling sort..." << std::endl;
	return tomahawk::two_sort(st) ? 0 : 1;
}

// `tomahawk scalc` (lib/scalc.h:50-194): one site against its neighbourhood.
static int scalc(int argc, char** argv) {
	if (argc < 3) {
		program_message();
		std::cerr << "About:  Calculate linkage disequilibrium for a single site\n"
		             "Usage:  tomahawk scalc [options] -i <in.twk> -I <chr:pos> -o <output.two>\n\n"
		             "Options:\n"
		             "  -i FILE   input Tomahawk (required)\n  -o FILE   output file or file prefix (required)\n"
		             "  -I STRING target site <contig>:pos (required)\n  -w INT    flanking width in bases (default: 500000)\n"
		             "  -t INT    number of CPU threads\n  -P FLOAT  Fisher's exact test cutoff P-value (default: 1)\n"
		             "  -k INT    compression level to use (default: 1)\n" << std::endl;
		return 1;
	}
	tomahawk::twk_ld_settings settings;
	int c;
	static const struct option long_options[] = {{"keep", required_argument, 0, 1006}, {"remove", required_argument, 0, 1007}, VARIANT_SELECTION_LONG_OPTIONS, {0, 0, 0, 0}};
	while ((c = getopt_long(argc, argv, "i:o:t:I:mMb:r:R:P:k:w:?", long_options, nullptr)) != -1) {
		switch (c) {
		case 1006: settings.keep_file = optarg; break;
		case 1007: settings.remove_file = optarg; break;
		case 1010: case 1011: case 1012: case 1013: case 1014: case 1015: case 1016:
			if (variant_selection_option(c, optarg, settings) != took) return 1;
			break;
		case 'i': settings.in = optarg; break;
		case 'o': settings.out = optarg; break;
		case 'I': settings.ival_strings.push_back(optarg); break;
		case 'm': settings.low_memory = true; break;
		case 'M': settings.force_phased = true; settings.low_memory = true; settings.bitmaps = true; break;
		case 't': if (!thread_option(optarg, settings.n_threads)) return 1; break;
		case 'b':
			settings.bl_size = atoi(optarg);
			if (settings.bl_size <= 0) { std::cerr << stamp("ERROR") << "Cannot have a non-positive number of entries in a block!" << std::endl; return 1; }
			break;
		case 'r':
			settings.minR2 = atof(optarg);
			if (settings.minR2 < 0 || settings.minR2 > 1) { std::cerr << stamp("ERROR") << "Cannot have a minimum R-squared value outside [0,1]" << std::endl; return 1; }
			break;
		case 'R':
			settings.maxR2 = atof(optarg);
			if (settings.maxR2 < 0 || settings.maxR2 > 1) { std::cerr << stamp("ERROR") << "Cannot have a maximum R-squared value outside [0,1]" << std::endl; return 1; }
			break;
		case 'P':
			settings.minP = atof(optarg);
			if (settings.minP < 0 || settings.minP > 1) { std::cerr << stamp("ERROR") << "Cannot have a cutoff P-value outside [0,1]" << std::endl; return 1; }
			break;
		case 'k': settings.c_level = atoi(optarg); break;
		case 'w':
			settings.l_surrounding = atoi(optarg);
			if (settings.l_surrounding < 1) { std::cerr << stamp("ERROR") << "Cannot have a non-positive window size" << std::endl; return 1; }
			break;
		default:
			std::cerr << stamp("ERROR") << "Unrecognized option: " << (char)c << std::endl;
			return 1;
		}
	}
	if (settings.in.empty()) { std::cerr << stamp("ERROR") << "No input value specified..." << std::endl; return 1; }
	if (settings.out.empty()) { std::cerr << stamp("ERROR") << "No output value specified..." << std::endl; return 1; }
	program_message();
	std::cerr << stamp("LOG") << "Calling calc..." << std::endl;
	settings.single = true;
	settings.minR2 = 0;           // scalc.h:188-189: -r is parsed, then overwritten
	tomahawk::twk_ld ld;
	return ld.ComputeSingle(settings, true, true) ? 0 : 1;
}

// Every command, in the order `tomahawk` without arguments lists them: an engine command's row, or a host tool that parses for itself
// (the reference's parsers, with the reference's words) with its name, its line of that list and, for two, what else selects it.
struct Entry {
	const char* name; const char* summary;      // summary: its line of `tomahawk` without arguments
	int (*main)(int, char**);
	int said;                                   // its place in the "Illegal command" sentence, which ends with the .two tools in another order
	const char* alias; bool by_prefix;          // what else selects it: another name; any word that begins with its name
};
template <const auto& CMD> static int engine(int argc, char** argv) { return run_command(CMD, argc, argv); }
static const Entry ENTRIES[] = {
	{"import", "  import   convert VCF text (plain / gzip) to .twk\n", import_cmd, 0},
	{CALC.name, CALC.summary, engine<CALC>, 1},
	{"scalc", "  scalc    linkage disequilibrium of one site against its neighbourhood\n", scalc, 2, "calc-single"},
	{RELATIONSHIP.name, RELATIONSHIP.summary, engine<RELATIONSHIP>, 3},
	{LDSCORE.name, LDSCORE.summary, engine<LDSCORE>, 4},
	{PRUNE.name, PRUNE.summary, engine<PRUNE>, 5},
	{CLUMP.name, CLUMP.summary, engine<CLUMP>, 6},
	{LDMATRIX.name, LDMATRIX.summary, engine<LDMATRIX>, 7},
	{LDDECAY.name, LDDECAY.summary, engine<LDDECAY>, 8},
	{LDAGGREGATE.name, LDAGGREGATE.summary, engine<LDAGGREGATE>, 9},
	{"sort", "  sort     sort a .two file\n", sort_cmd, 12},
	{"view", "  view     convert, filter and slice .two files\n", view, 11},
	{"concat", "  concat   concatenate .two files from the same set of samples\n", concat, 10, nullptr, true}};
static const size_t N_ENTRIES = sizeof(ENTRIES) / sizeof(ENTRIES[0]);

static int run_main(int argc, char** argv) {
	if (argc == 1) {           // reference: lib/main.cpp:28-60 lists its commands
		program_message();
		std::cerr << "Usage: tomahawk <command> [options]\n\nCommands:\n";
		for (const Entry& e : ENTRIES) std::cerr << e.summary;
		std::cerr << std::endl;
		return 1;
	}
	// The host tools allocate and free MB-sized block buffers on hundreds of threads; served by
	// mmap/munmap (glibc's default above 128 KiB) that serialises on the address-space lock.
	mallopt(M_MMAP_THRESHOLD, 1 << 30);
	mallopt(M_TRIM_THRESHOLD, 1 << 30);
	tomahawk::LITERAL_COMMAND_LINE = "tomahawk";
	for (int i = 1; i < argc; ++i) tomahawk::LITERAL_COMMAND_LINE += " " + std::string(argv[i]);
	if (strcmp(argv[1], BLOCKS.name) == 0) return engine<BLOCKS>(argc, argv);
	if (strcmp(argv[1], LDSPLIT.name) == 0) return engine<LDSPLIT>(argc, argv);
	for (const Entry& e : ENTRIES)
		if (strcmp(argv[1], e.name) == 0 || (e.alias && strcmp(argv[1], e.alias) == 0) || (e.by_prefix && strncmp(argv[1], e.name, strlen(e.name)) == 0)) return e.main(argc, argv);
	if (strcmp(argv[1], "--version") == 0 || strcmp(argv[1], "version") == 0) { program_message(); return 0; }
	if (strcmp(argv[1], "--help") == 0 || strcmp(argv[1], "help") == 0) { calc_usage(); return 0; }
	program_message();
	const char* said[N_ENTRIES] = {};
	for (const Entry& e : ENTRIES) said[e.said] = e.name;
	std::string names;
	for (size_t k = 0; k < N_ENTRIES; ++k) names += std::string(k == 0 ? "`" : k + 1 < N_ENTRIES ? ", `" : " and `") + said[k] + "`";
	std::cerr << stamp("ERROR") << "Illegal command: only " << names << " are provided by the MI355X engine (aggregate/decay/... are the reference's; `lddecay` bins by distance and `ldaggregate` into x-by-y cells without a .two; `relationship` keeps the reference's name, not its numbers)" << std::endl;
	return 1;
}

int main(int argc, char** argv) {
	try {
		return run_main(argc, argv);
	} catch (const std::bad_alloc&) {
		std::cerr << stamp("ERROR") << "Out of memory (or a corrupt file declaring an absurd size)..." << std::endl;
	} catch (const std::exception& e) {
		std::cerr << stamp("ERROR") << e.what() << std::endl;
	}
	return 1;
}
