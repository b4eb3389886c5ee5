// `--keep FILE` / `--remove FILE`: the header's sample names and the two files -> the ascending list of kept sample indices, or an
// error.  Pure host code with no device and no .twk in it (exported as twk_resolve_samples, tests/test_subset_cpu.py): a command
// resolves its list right after it has read the header, before any device work.
//
// A file holds one sample name per line; surrounding blanks and a trailing carriage return are dropped, blank lines and lines that
// start with '#' are skipped.  keep: only the named samples stay (no file: all of them); remove: the named samples go; both: keep, then
// remove.  The result is in header order, whatever the files' order.  Errors: a file that cannot be read, a name that is not in the
// header (the first one is named), a name listed twice in one file, a result without a sample.
#pragma once
#include <cstdint>
#include <fstream>
#include <string>
#include <unordered_map>
#include <vector>

namespace tomahawk {

// The names of one list file -> header indices, in the file's order.
inline bool read_sample_file(const std::string& path, const char* option, const std::unordered_map<std::string, uint32_t>& index_of,
                             size_t n_header, std::vector<uint32_t>& out, std::string& err) {
	std::ifstream in(path);
	if (!in.good()) { err = std::string("Cannot read the sample list (") + option + "): " + path; return false; }
	std::vector<char> seen(n_header, 0);
	std::string line;
	size_t line_no = 0;
	while (std::getline(in, line)) {
		++line_no;
		const size_t b = line.find_first_not_of(" \t\r");
		if (b == std::string::npos || line[b] == '#') continue;
		const std::string name = line.substr(b, line.find_last_not_of(" \t\r") - b + 1);
		const auto it = index_of.find(name);
		if (it == index_of.end()) { err = std::string("Sample \"") + name + "\" (" + option + " " + path + ", line " + std::to_string(line_no) + ") is not in the input's header"; return false; }
		if (seen[it->second]) { err = std::string("Sample \"") + name + "\" is listed twice (" + option + " " + path + ", line " + std::to_string(line_no) + ")"; return false; }
		seen[it->second] = 1;
		out.push_back(it->second);
	}
	if (in.bad()) { err = std::string("Cannot read the sample list (") + option + "): " + path; return false; }
	return true;
}

// keep_path / remove_path: empty for "not given".  -> false with the message in err.
inline bool resolve_sample_list(const std::vector<std::string>& header, const std::string& keep_path, const std::string& remove_path,
                                std::vector<uint32_t>& out, std::string& err) {
	out.clear(); err.clear();
	std::unordered_map<std::string, uint32_t> index_of;
	index_of.reserve(header.size() * 2);
	for (size_t s = 0; s < header.size(); ++s) index_of.emplace(header[s], (uint32_t)s);      // (a name twice in the header: its first sample)
	std::vector<char> kept(header.size(), keep_path.empty() ? 1 : 0);
	std::vector<uint32_t> ids;
	if (!keep_path.empty()) {
		if (!read_sample_file(keep_path, "--keep", index_of, header.size(), ids, err)) return false;
		for (uint32_t s : ids) kept[s] = 1;
	}
	if (!remove_path.empty()) {
		ids.clear();
		if (!read_sample_file(remove_path, "--remove", index_of, header.size(), ids, err)) return false;
		for (uint32_t s : ids) kept[s] = 0;
	}
	for (size_t s = 0; s < header.size(); ++s) if (kept[s]) out.push_back((uint32_t)s);
	if (out.empty()) { err = "No sample is left after --keep / --remove"; return false; }
	return true;
}

}  // namespace tomahawk
