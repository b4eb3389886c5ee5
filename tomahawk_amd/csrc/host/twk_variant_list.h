// `--extract FILE` / `--exclude FILE`: a list of positions and the variants a command has loaded -> the ascending list of the variants
// at a listed position.  Pure host code with no device and no .twk in it (exported as twk_resolve_variants, tests/test_varsel_cli.py),
// beside twk_sample_list.h: a command reads its lists right after the header, before any device work, and matches them against the
// positions of the variants it loads.
//
// A line is CONTIG:POS or CONTIG<whitespace>POS; further columns are ignored, so the first two columns of any per-variant output of
// the commands (`ldscore`, `prune`, `clump`, ..) can be fed back.  A line whose second column is a number is read as CONTIG POS, any
// other as CONTIG:POS with the position behind the last colon (contig names may hold colons).  A line that reads both ways - `1:1000 1`,
// CONTIG:POS with a numeric further column, or the contig `1:1000` at position 1 - is settled against the header's contig names when
// the list is matched: CONTIG POS if the whole first column names a contig, else CONTIG:POS if what stands before its last colon does.
// Surrounding blanks and a trailing carriage return are dropped; blank
// lines and lines that start with '#' are skipped.  POS is written as the commands print it: 1-based, the stored position + 1.  EVERY
// variant at a listed position matches (a multi-allelic site split over several records); a position listed twice counts once.  A
// listed position that no loaded variant has - an unknown contig included - is no error: such entries are counted and the command
// reports the count on stderr.  Errors: a file that cannot be read, and a line that does not parse, which is named.
#pragma once
#include <algorithm>
#include <cstdint>
#include <fstream>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

namespace tomahawk {

struct VariantListEntry {
	std::string contig; uint64_t pos;              // pos: as printed, 1-based
	bool has_alt = false;                          // the line also reads as CONTIG:POS followed by a numeric column:
	std::string alt_contig; uint64_t alt_pos = 0;  // that reading, taken when `contig` is no contig of the header and alt_contig is
};

inline bool read_variant_file(const std::string& path, const char* option, std::vector<VariantListEntry>& out, std::string& err) {
	std::ifstream in(path);
	if (!in.good()) { err = std::string("Cannot read the variant list (") + option + "): " + path; return false; }
	std::string line;
	size_t line_no = 0;
	const char* blanks = " \t\r";
	while (std::getline(in, line)) {
		++line_no;
		const size_t b = line.find_first_not_of(blanks);
		if (b == std::string::npos || line[b] == '#') continue;
		auto fail = [&]() {
			err = std::string("Cannot parse line ") + std::to_string(line_no) + " of the variant list (" + option + " " + path + "): \"" + line.substr(b, 60) +
			      "\" is neither CONTIG:POS nor CONTIG<whitespace>POS";
			return false;
		};
		// the first column ends at the first blank; if it holds a ':' the position is what follows the LAST one (contig names may hold colons)
		const size_t e1 = std::min(line.find_first_of(blanks, b), line.size());
		std::string contig = line.substr(b, e1 - b), number;
		const size_t colon = contig.rfind(':');
		const size_t b2 = line.find_first_not_of(blanks, e1);
		bool two_columns = false;
		if (b2 != std::string::npos) {
			const size_t e2 = std::min(line.find_first_of(blanks, b2), line.size());
			const std::string second = line.substr(b2, e2 - b2);
			two_columns = !second.empty() && second.find_first_not_of("0123456789") == std::string::npos;
			if (two_columns) number = second;
		}
		if (!two_columns) {
			if (colon == std::string::npos) return fail();
			number = contig.substr(colon + 1);
			contig.resize(colon);
		}
		if (contig.empty() || number.empty() || number.size() > 18 || number.find_first_not_of("0123456789") != std::string::npos) return fail();
		VariantListEntry e;
		e.contig = contig; e.pos = std::stoull(number);
		if (two_columns && colon != std::string::npos && colon > 0) {
			const std::string behind = contig.substr(colon + 1);
			if (!behind.empty() && behind.size() <= 18 && behind.find_first_not_of("0123456789") == std::string::npos) {
				e.has_alt = true; e.alt_contig = contig.substr(0, colon); e.alt_pos = std::stoull(behind);
			}
		}
		out.push_back(e);
	}
	if (in.bad()) { err = std::string("Cannot read the variant list (") + option + "): " + path; return false; }
	return true;
}

// The variants v < M - contig contigs[rid[v]], printed position pos[v] + 1 - at a position of `entries` -> out, ascending; *n_absent:
// the distinct listed positions that no variant has.
inline void match_variant_list(const std::vector<std::string>& contigs, const uint32_t* rid, const uint32_t* pos, size_t M,
                               const std::vector<VariantListEntry>& entries, std::vector<uint32_t>& out, uint64_t* n_absent) {
	out.clear();
	std::unordered_map<std::string, uint32_t> rid_of;
	for (size_t k = 0; k < contigs.size(); ++k) rid_of.emplace(contigs[k], (uint32_t)k);      // (a name twice in the header: its first contig)
	std::vector<std::pair<uint32_t, uint64_t>> keys;                                           // (rid, printed position), sorted, distinct
	uint64_t unknown = 0;
	{
		std::vector<std::pair<std::string, uint64_t>> strangers;
		for (const VariantListEntry& e : entries) {
			const auto it = rid_of.find(e.contig);
			const auto alt = e.has_alt && it == rid_of.end() ? rid_of.find(e.alt_contig) : rid_of.end();
			if (it != rid_of.end()) keys.emplace_back(it->second, e.pos);
			else if (alt != rid_of.end()) keys.emplace_back(alt->second, e.alt_pos);
			else strangers.emplace_back(e.contig, e.pos);
		}
		std::sort(strangers.begin(), strangers.end());
		unknown = (uint64_t)(std::unique(strangers.begin(), strangers.end()) - strangers.begin());
	}
	std::sort(keys.begin(), keys.end());
	keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
	std::vector<char> hit(keys.size(), 0);
	for (size_t v = 0; v < M; ++v) {
		const std::pair<uint32_t, uint64_t> key(rid[v], (uint64_t)pos[v] + 1);
		const auto it = std::lower_bound(keys.begin(), keys.end(), key);
		if (it != keys.end() && *it == key) { hit[it - keys.begin()] = 1; out.push_back((uint32_t)v); }
	}
	if (n_absent) *n_absent = unknown + (uint64_t)std::count(hit.begin(), hit.end(), 0);
}

// One list file against the loaded variants.  -> false with the message in err.
inline bool resolve_variant_list(const std::vector<std::string>& contigs, const uint32_t* rid, const uint32_t* pos, size_t M, const std::string& path,
                                 const char* option, std::vector<uint32_t>& out, uint64_t* n_absent, std::string& err) {
	err.clear();
	std::vector<VariantListEntry> entries;
	if (!read_variant_file(path, option, entries, err)) return false;
	match_variant_list(contigs, rid, pos, M, entries, out, n_absent);
	return true;
}

}  // namespace tomahawk
