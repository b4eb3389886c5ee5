// tomahawk::twk_ld on the MI355X engine.
//
// Host orchestration that the reference does in lib/ld/ld.cpp:477-671 (Compute):
// open the .twk, pick the chunk of the block triangle (-c/-C), unpack the blocks
// to bitvectors on worker threads, hand them to the device through the C ABI
// (include/twk_hip.h), stream the surviving pairs back and write the .two file
// (forward + reverse copies in separate blocks, ld_engine.cpp:1270-1309).
#include "twk_ld.h"

#include <algorithm>
#include <iterator>
#include <memory>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <ctime>
#include <iomanip>
#include <iostream>
#include <limits>
#include <map>
#include <set>
#include <fstream>
#include <regex>
#include <sstream>
#include <thread>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <sys/time.h>
#include <cstdio>

#include <fcntl.h>
#include <unistd.h>

#include "twk_aggregate_landscape.h"
#include "twk_format.h"
#include "twk_hip.h"
#include "twk_import.h"
#include "twk_ld_names.h"
#include "twk_parallel.h"
#include "twk_record_sink.h"
#include "twk_sample_list.h"
#include "twk_variant_list.h"
#include "twk_util.h"

#ifndef TWK_AMD_VERSION
#define TWK_AMD_VERSION "0.7.0-mi355x"
#endif

namespace tomahawk {

using namespace util;

namespace {
// twk_ld_balancer::Build (lib/ld/ld_balancing.h:23-80), including its chunk
// arithmetic (last chunk of a row is `chunk_size` blocks ending at n_blocks).
struct Balancer {
	bool diag = true;
	uint32_t fromL = 0, toL = 0, fromR = 0, toR = 0;
	bool build(uint32_t n_blocks, uint32_t parts, uint32_t chosen) {
		if (chosen >= parts) { std::cerr << stamp("ERROR", "BALANCER") << "Illegal chosen block: " << chosen << " >= " << parts << std::endl; return false; }
		if (parts > n_blocks) { std::cerr << stamp("ERROR", "BALANCER") << "Illegal desired number of blocks! You are asking for more subproblems than there are blocks available (" << parts << ">" << n_blocks << ")..." << std::endl; return false; }
		if (parts == 1) { fromL = 0; toL = n_blocks; fromR = 0; toR = n_blocks; diag = true; return true; }
		uint32_t factor = 0;
		for (uint32_t i = 1; i < parts; ++i) if ((((i * i) - i) / 2) + i == parts) { factor = i; break; }
		if (factor == 0) { std::cerr << stamp("ERROR", "BALANCER") << "Could not partition into " << parts << " number of subproblems. This number is not a function of x!2 + x..." << std::endl; return false; }
		const uint32_t chunk = n_blocks / factor;
		for (uint32_t i = 0, k = 0; i < factor; ++i) {
			for (uint32_t j = i; j < factor; ++j, ++k) {
				if (k != chosen) continue;
				toR = (j + 1 == factor ? n_blocks : chunk * (j + 1)); fromR = toR - chunk;
				toL = (i + 1 == factor ? n_blocks : chunk * (i + 1)); fromL = toL - chunk;
				diag = (i == j);
				return true;
			}
		}
		return true;
	}
};
}  // namespace

// ---- settings (lib/core.cpp:297-332) -----------------------------------------------------
twk_ld_settings::twk_ld_settings()
    : square(true), window(false), low_memory(false), bitmaps(false), single(false), force_phased(false),
      forced_unphased(false), force_cross_intervals(false), c_level(1), bl_size(500), b_size(10000),
      l_window(1000000), n_threads((int32_t)std::thread::hardware_concurrency()), cycle_threshold(0),
      ldd_load_type(TWK_LDD_ALL), l_surrounding(500000), out("-"), minP(1), minR2(0.1), maxR2(100),
      minDprime(0), maxDprime(100), n_chunks(1), c_chunk(0) {}

std::string twk_ld_settings::GetString() const {
	auto tf = [](bool b) { return std::string(b ? "TRUE" : "FALSE"); };
	return "square=" + tf(square) + ",window=" + tf(window) + ",low_memory=" + tf(low_memory) + ",bitmaps=" + tf(bitmaps)
	     + ",single=" + tf(single) + ",force_phased=" + tf(force_phased) + ",force_unphased=" + tf(forced_unphased)
	     + ",compression_level=" + std::to_string(c_level) + ",block_size=" + std::to_string(bl_size)
	     + ",output_block_size=" + std::to_string(b_size) + (window ? ",window_size=" + std::to_string(l_window) : "")
	     + ",l_surrounding=" + std::to_string(l_surrounding) + ",minP=" + std::to_string(minP) + ",minR2=" + std::to_string(minR2)
	     + ",maxR2=" + std::to_string(maxR2) + ",minDprime=" + std::to_string(minDprime) + ",maxDprime=" + std::to_string(maxDprime)
	     + ",n_chunks=" + std::to_string(n_chunks) + ",c_chunk=" + std::to_string(c_chunk) + ",n_threads=" + std::to_string(n_threads)
	     + ",ldd_type=" + std::to_string((int)ldd_load_type) + ",cycle_threshold=" + std::to_string(cycle_threshold);
}

// ---- implementation ---------------------------------------------------------------------------
class twk_ld::twk_ld_impl {
public:
	uint64_t n_pairs = 0, n_records = 0;
	std::vector<std::pair<std::string, int64_t>> engine_options;     // twk_ld::SetEngineOption, in the order given
	int64_t option(const char* key, int64_t dflt) const {
		for (const auto& kv : engine_options) if (kv.first == key) dflt = kv.second;
		return dflt;
	}

	// per-variant (rid,pos) of the uploaded selection
	std::vector<uint32_t> rid, pos;

	// Output: one shared writer, one emitter (pair of open forward / reverse blocks) per GPU driver
	// thread - the reference's per-thread blocks behind one spinlocked writer (twk_record_sink.h).
	TwoOutput out;

	// TWK_REF_COMPAT=1 with -w: what the reference's window mode really keeps, as a filter on the
	// exact window's records.  blk_first[k] = first variant of the k-th loaded block.
	struct CompatWindow {
		bool on = false, forced = false;             // forced: -p / -u (the slave loops test every pair)
		uint32_t w = 0;
		std::vector<uint32_t> blk_first;             // [n_blocks + 1]
		std::vector<uint32_t> blk_of;                // [n_variants]
	} cw;
	// Reference, block pair (bi, bj) of a window run:
	//  * the ticker issues (i, j), j = i, i+1, ..., and gives up the rest of row i at the first j != i with
	//    pos(first of j) - pos(last of i) > w - in uint32 arithmetic and without looking at the contigs
	//    (ld_balancing.h:176-203);
	//  * -p / -u: the slave walks the pairs (p, q) of the block pair in order and leaves the WHOLE block pair at
	//    the first same-contig pair with pos(q) - pos(p) > w (goto end_cycle, ld_engine.cpp:2553-2560, 2582-2588).
	//    Positions ascend, so that happens in the first row or never: of a block pair that is not wholly inside
	//    the window only the first variant's in-window pairs come out;
	//  * default mode has no window loop at all (ld_engine.cpp:1841-1843: Calculate): every pair of every block
	//    pair the ticker issued is computed.
	bool compat_keep(uint32_t A, uint32_t B) const {
		const uint32_t bi = cw.blk_of[A], bj = cw.blk_of[B];
		const uint32_t last_i = cw.blk_first[bi + 1] - 1;
		for (uint32_t j = bi + 1; j <= bj; ++j)
			if ((uint32_t)(pos[cw.blk_first[j]] - pos[last_i]) > cw.w) return false;
		if (!cw.forced) return true;
		const uint32_t first_i = cw.blk_first[bi], last_j = cw.blk_first[bj + 1] - 1;
		if (rid[first_i] != rid[last_j] || (uint32_t)(pos[last_j] - pos[first_i]) <= cw.w) return true;      // wholly inside
		return A == first_i && rid[A] == rid[B] && (uint32_t)(pos[B] - pos[A]) <= cw.w;
	}

	bool run(twk_ld_settings& settings, const Header& hdr, const std::vector<twk_hip_ctx*>& ctxs, uint32_t n_samples, const void* spec);
};

twk_ld::twk_ld() : mImpl(new twk_ld_impl) {}
twk_ld::~twk_ld() { delete mImpl; }
void twk_ld::SetEngineOption(const std::string& key, int64_t value) { mImpl->engine_options.emplace_back(key, value); }
uint64_t twk_ld::n_pairs() const { return mImpl->n_pairs; }
uint64_t twk_ld::n_records() const { return mImpl->n_records; }

bool twk_ld::Compute(const twk_ld_settings& s) { settings = s; return Compute(); }
bool twk_ld::ComputeSingle(const twk_ld_settings& s, bool verbose, bool progress) { settings = s; return ComputeSingle(verbose, progress); }
// (the reference's own default build answers the same way: TWK_SLAVE_DEBUG_MODE is 0, lib/ld/ld_engine.h:20, lib/ld/ld.cpp:878-882)
bool twk_ld::ComputePerformance() {
	std::cerr << stamp("ERROR") << "ComputePerformance is a compile-time debug harness of the CPU reference; not available." << std::endl;
	return false;
}
namespace {
struct DeviceCtxs {          // one engine context per GPU of the run
	std::vector<twk_hip_ctx*> ctx;
	~DeviceCtxs() { for (auto* c : ctx) if (c) twk_hip_ctx_destroy(c); }
};
bool hip_ok(twk_hip_ctx* ctx, int rc, const char* what) {
	if (rc == TWK_HIP_OK) return true;
	std::cerr << stamp("ERROR", "HIP") << what << ": " << twk_hip_strerror(rc);
	if (ctx && twk_hip_last_error(ctx)[0]) std::cerr << " (" << twk_hip_last_error(ctx) << ")";
	std::cerr << std::endl;
	return false;
}
}  // namespace

// ---- interval strings (lib/intervals.cpp:96-139; regexes include/tomahawk.h:57-59) -------------
struct Interval { int32_t rid; uint32_t from, to; };
static bool parse_interval(const std::string& str, const Header& hdr, Interval& out) {
	static const std::regex re_range("^[A-Za-z0-9\\-_]+\\:[0-9]+([\\.]{1}[0-9]+){0,1}([eE]{1}[0-9]{1})?\\-[0-9]+([\\.]{1}[0-9]+){0,1}([eE]{1}[0-9]{1})?$");
	static const std::regex re_pos("^[A-Za-z0-9\\-_]+\\:[0-9]+([\\.]{1}[0-9]+){0,1}([eE]{1}[0-9]{1})?$");
	static const std::regex re_contig("^[A-Za-z0-9\\-_]+$");
	auto contig = [&](const std::string& name) -> int {
		const int id = hdr.contig_id(name);
		if (id < 0) std::cerr << stamp("ERROR", "INTERVAL") << "Contig does not exist in string " << str << std::endl;
		return id;
	};
	if (std::regex_match(str, re_range)) {
		const size_t c = str.find(':'), d = str.find('-', c);
		const int id = contig(str.substr(0, c));
		if (id < 0) return false;
		out = {hdr.contigs[id].idx == (uint32_t)id ? id : (int32_t)hdr.contigs[id].idx,
		       (uint32_t)std::atof(str.substr(c + 1, d - c - 1).c_str()), (uint32_t)std::atof(str.substr(d + 1).c_str())};
		return true;
	}
	if (std::regex_match(str, re_pos)) {
		const size_t c = str.find(':');
		const int id = contig(str.substr(0, c));
		if (id < 0) return false;
		const uint32_t p = (uint32_t)std::atof(str.substr(c + 1).c_str());
		out = {(int32_t)hdr.contigs[id].idx, p, p + 1};
		return true;
	}
	if (std::regex_match(str, re_contig)) {
		const int id = contig(str);
		if (id < 0) return false;
		out = {(int32_t)hdr.contigs[id].idx, 0, (uint32_t)hdr.contigs[id].n_bases};
		return true;
	}
	std::cerr << stamp("ERROR", "INTERVAL") << "Illegal format: " << str << std::endl;
	return false;
}
// Index::FindOverlap (lib/index.cpp:124-133): blocks with rid match and [minpos,maxpos] meeting [from,to].
static void overlapping_blocks(const TwkIndex& idx, const Interval& iv, std::vector<uint32_t>& out) {
	for (size_t i = 0; i < idx.ent.size(); ++i)
		if (idx.ent[i].rid == iv.rid && idx.ent[i].minpos <= iv.to && idx.ent[i].maxpos >= iv.from) out.push_back((uint32_t)i);
}

namespace {
// Everything after the variants are in HBM: output file, compute, final statistics.
struct RunSpec {
	uint32_t nA = 0, nB = 0;     // variants [0,nA) are the row set, [nA,nA+nB) the column set (nB = 0: one set)
	bool triangleA = true;       // all pairs inside the row set
	bool rectAB = false;         // row set x column set
	int options = 0;             // TWK_HIP_OPT_*
	uint32_t l_window = 0;
	// Window mode on several GPUs: GPU g holds only its band of rows plus the halo its window reaches, as
	// local variants [0, n_local) = global [first, first + n_local); rows [0, n_band) are its own.
	struct Slab { uint32_t first = 0, n_band = 0, n_local = 0; };
	std::vector<Slab> slabs;     // empty: every GPU holds everything and takes shard g of n of every region
};
}  // namespace

// What is said before an output file is opened and after it did not open; the same for the input
static void opening(const std::string& path) { std::cerr << stamp("LOG", "WRITER") << "Opening " << path << "..." << std::endl; }
static bool opened(bool ok, const std::string& path) {
	if (!ok) std::cerr << stamp("ERROR", "WRITER") << "Failed to open file: " << path << "..." << std::endl;
	return ok;
}
static bool open_input(TwkReader& reader, const std::string& path, bool announce) {
	if (announce) std::cerr << stamp("LOG", "READER") << "Opening " << path << "..." << std::endl;
	if (reader.open(path)) return true;
	std::cerr << stamp("ERROR") << "Failed to open file: " << path << "... (" << reader.error << ")" << std::endl;
	return false;
}

static bool open_output(twk_ld_settings& settings, const Header& in_hdr, TwoWriter& writer) {   // ld.cpp:583-618
	std::string out = settings.out;
	if (out.empty() || out == "-") {
		std::cerr << stamp("LOG", "WRITER") << "Writing to stdout..." << std::endl;
		out = "-";
	} else {
		const std::string ext = extension(out);
		if (!(ext.size() == 3 && strncasecmp(ext.c_str(), "two", 3) == 0)) {
			const std::string bp = base_path(out);
			out = (bp.size() ? bp + "/" : "") + base_name(out) + ".two";
		}
		opening(out);
	}
	settings.out = out;
	Header hdr = in_hdr;
	hdr.literals += "\n##tomahawk_calcVersion=" + std::string(TWK_AMD_VERSION) + "\n";
	hdr.literals += "##tomahawk_calcCommand=" + command_line() + "; Date=" + datetime() + "\n";
	return opened(writer.open(out, hdr, settings.c_level), out);
}

// ---- input: .twk blocks -> HBM (ld.cpp:370-465, ld_unpacker.h:44-123) ------------------------------------
// The reference's unpack threads decompress every block and expand every variant's run-length genotypes
// into a bitvector in host memory.  Here the host only decompresses: blocks are grouped into batches of
// <= 32 MB (uncompressed), decode threads read (pread) and zstd-decompress a batch each and walk the
// record headers for the per-variant metadata and the place of the run words; the runs are expanded by
// HIP kernels (twk_hip_upload_rle), so PCIe carries the compressed genotypes.  The batches pass through a
// small ring of page-locked slots to one uploader thread per GPU (load_blocks below).
namespace {
bool pread_all(int fd, void* buf, size_t n, uint64_t off) {
	uint8_t* p = static_cast<uint8_t*>(buf);
	while (n) {
		const ssize_t r = pread(fd, p, n, (off_t)off);
		if (r <= 0) return false;
		p += r; n -= (size_t)r; off += (uint64_t)r;
	}
	return true;
}
struct Staging {            // page-locked when the HIP runtime can give it, plain memory otherwise
	uint8_t* p = nullptr; size_t cap = 0; bool pinned = false;
	bool reserve(size_t n) {
		if (cap >= n) return true;
		release();
		void* q = nullptr;
		if (twk_hip_host_alloc(n, &q) == TWK_HIP_OK && q) { p = static_cast<uint8_t*>(q); pinned = true; }
		else { p = static_cast<uint8_t*>(std::malloc(n)); pinned = false; }
		cap = p ? n : 0;
		return p != nullptr;
	}
	void release() { if (p) { if (pinned) twk_hip_host_free(p); else std::free(p); } p = nullptr; cap = 0; }
	~Staging() { release(); }
};
struct LoadBatch {
	size_t k0 = 0, k1 = 0;                      // blocks [k0, k1) of the selection
	uint32_t first = 0, nv = 0;                 // variants [first, first + nv)
	size_t bytes = 0;
	std::vector<size_t> boff;                   // where each block's bytes start in the staging buffer
	std::vector<twk_hip_rle_desc> desc;
	std::vector<twk_hip_variant_meta> meta;
};
// One decompressed block (core.cpp:245-261: u32 n, u32 m, u32 rid, then n records) -> descriptors + metadata
// of its variants; record = 38-byte header (core.cpp:59-73) + n_runs run words.
bool index_block(const uint8_t* base, size_t block_off, size_t block_len, uint32_t n_expected,
                 twk_hip_rle_desc* desc, twk_hip_variant_meta* meta) {
	const uint8_t* p = base + block_off; const uint8_t* end = p + block_len;
	if (block_len < 12) return false;
	uint32_t n; std::memcpy(&n, p, 4);
	if (n != n_expected) return false;
	p += 12;
	for (uint32_t i = 0; i < n; ++i) {
		if ((size_t)(end - p) < 38) return false;
		const uint8_t pack = p[0];
		const uint32_t width = pack >> 3;
		if (width != 1 && width != 2 && width != 4) return false;       // "illegal gt primitive type" core.cpp:95
		twk_hip_variant_meta& m = meta[i];
		std::memcpy(&m.pos, p + 2, 4); std::memcpy(&m.ac, p + 6, 4); std::memcpy(&m.an, p + 10, 4); std::memcpy(&m.rid, p + 14, 4);
		std::memcpy(&m.hwe, p + 26, 8);
		uint32_t n_write; std::memcpy(&n_write, p + 34, 4);
		const uint32_t n_runs = n_write >> 1, missing = n_write & 1;   // the container's own miss bit (= gt_missing in valid files)
		m.missing = missing; m._pad = 0;
		p += 38;
		if ((uint64_t)n_runs * width > (uint64_t)(end - p)) return false;
		desc[i].offset = (uint64_t)(p - base); desc[i].n_runs = n_runs; desc[i].width = (uint8_t)width; desc[i].missing = (uint8_t)missing; desc[i]._pad = 0;
		p += (size_t)n_runs * width;
	}
	return true;
}
}  // namespace

static bool load_blocks(const std::string& path, const TwkReader& reader, const std::vector<uint32_t>& sel,
                        uint32_t T, const std::vector<twk_hip_ctx*>& ctxs, uint32_t n_samples, std::vector<uint32_t>& rid, std::vector<uint32_t>& pos,
                        std::vector<twk_hip_variant_meta>* meta_out = nullptr) {      // meta_out: the caller also wants the variants' allele counts
	using lclock = std::chrono::steady_clock;
	const auto t_begin = lclock::now();
	std::vector<uint32_t> first(sel.size() + 1, 0);
	for (size_t k = 0; k < sel.size(); ++k) first[k + 1] = first[k] + reader.index.ent[sel[k]].n;
	rid.assign(first.back(), 0); pos.assign(first.back(), 0);
	if (meta_out) meta_out->assign(first.back(), twk_hip_variant_meta{});
	if (sel.empty()) {
		for (auto* c : ctxs) if (!hip_ok(c, twk_hip_set_problem(c, n_samples, 0), "twk_hip_set_problem")) return false;
		return true;
	}
	const int fd = ::open(path.c_str(), O_RDONLY);
	if (fd < 0) { std::cerr << stamp("ERROR") << "Failed to open " << path << std::endl; return false; }
	struct Closer { int fd; ~Closer() { ::close(fd); } } closer{fd};
	// Batches of whole blocks, one decode thread each.  A batch holds at least one block and at most 32 MB
	// (the first batch reaches the GPU after ~30 ms); small inputs are cut finer so that every decode thread
	// gets several.
	const uint32_t W = std::max<uint32_t>(1, std::min<uint32_t>(T, 32));           // decode threads
	size_t total_unc = 0, max_block = 0;
	for (uint32_t k : sel) { const size_t u = ((size_t)reader.index.ent[k].b_unc + 15) / 16 * 16; total_unc += u; max_block = std::max(max_block, u); }
	const size_t batch_cap = std::max(max_block, std::min<size_t>((size_t)32 << 20, std::max<size_t>((size_t)2 << 20, total_unc / (4 * (size_t)W))));
	std::vector<LoadBatch> batches;
	for (size_t k = 0; k < sel.size();) {
		LoadBatch b; b.k0 = k; b.first = first[k];
		while (k < sel.size() && (b.bytes == 0 || b.bytes + reader.index.ent[sel[k]].b_unc <= batch_cap)) {
			b.boff.push_back(b.bytes);
			b.bytes += ((size_t)reader.index.ent[sel[k]].b_unc + 15) / 16 * 16;
			++k;
		}
		b.k1 = k; b.nv = first[k] - b.first;
		batches.push_back(std::move(b));
	}
	size_t max_bytes = 0;
	for (const auto& b : batches) max_bytes = std::max(max_bytes, b.bytes);
	const size_t n_batches = batches.size(), n_gpus = ctxs.size();
	const uint32_t n_workers = (uint32_t)std::min<size_t>(W, n_batches);
	// A decode thread takes the next batch in file order, reads and decompresses its blocks into its own buffer
	// and walks the record headers; when its batch's turn comes it copies the bytes into a slot of a small ring of
	// page-locked memory (page-locking costs ~0.2 s per GB here, unlocking ~0.13 s: the ring is 8 slots, not one
	// per thread).  One uploader thread per GPU takes the batches in file order (copy + device inflate); batch b
	// uses slot b mod 8, free again when every GPU has batch b - 8.  The device allocations of the problem are
	// made before the threads start: 10-20 ms for 12.5 GB then, but up to a second next to 32 threads faulting
	// their buffers in.
	const size_t n_slots = std::min<size_t>(n_batches, 8);
	const auto t_alloc0 = lclock::now();
	{
		std::vector<int> rc(n_gpus, TWK_HIP_OK);
		std::vector<std::thread> th;
		for (size_t g = 0; g < n_gpus; ++g) th.emplace_back([&, g] { rc[g] = twk_hip_set_problem(ctxs[g], n_samples, first.back()); });
		for (auto& t : th) t.join();
		for (size_t g = 0; g < n_gpus; ++g) if (!hip_ok(ctxs[g], rc[g], "twk_hip_set_problem")) return false;
	}
	Staging ring;
	if (!ring.reserve(n_slots * max_bytes)) { std::cerr << stamp("ERROR") << "Out of host memory for the upload staging buffers" << std::endl; return false; }
	const double t_alloc = std::chrono::duration<double>(lclock::now() - t_alloc0).count();
	size_t max_cmp = 0;
	for (uint32_t k : sel) max_cmp = std::max<size_t>(max_cmp, reader.index.ent[k].b_cmp);
	std::mutex mu;
	std::condition_variable cv_slot, cv_ready;
	std::vector<char> ready(n_batches, 0);           // under mu: batch is in its slot
	std::vector<uint32_t> pending(n_batches, (uint32_t)n_gpus);
	size_t released = 0;                             // under mu: batches [0, released) have left their slots
	std::atomic<size_t> next_batch(0);
	std::atomic<bool> failed(false);
	std::string fail_msg;                            // under mu, first failure only
	auto fail = [&](const std::string& msg) {
		std::lock_guard<std::mutex> lk(mu);
		if (!failed.exchange(true)) fail_msg = msg;
		cv_slot.notify_all(); cv_ready.notify_all();
	};
	std::vector<double> busy_decode(n_workers, 0.0), busy_upload(n_gpus, 0.0);

	auto decode_batch = [&](LoadBatch& b, uint8_t* buf, std::vector<uint8_t>& z) -> bool {
		b.desc.resize(b.nv); b.meta.resize(b.nv);
		for (size_t k = b.k0; k < b.k1; ++k) {
			const IndexEntry& e = reader.index.ent[sel[k]];
			uint8_t head[9];
			if (!pread_all(fd, head, 9, e.foff)) return false;
			uint32_t unc, cmp; std::memcpy(&unc, head + 1, 4); std::memcpy(&cmp, head + 5, 4);
			if (head[0] != 1 || unc != e.b_unc || cmp != e.b_cmp) return false;      // the header must agree with the index (sizes the buffers)
			z.resize(cmp);
			if (!pread_all(fd, z.data(), cmp, e.foff + 9)) return false;
			if (!zstd_decompress_into(z.data(), cmp, buf + b.boff[k - b.k0], unc)) return false;
			const uint32_t v0 = first[k] - b.first;
			if (!index_block(buf, b.boff[k - b.k0], unc, e.n, &b.desc[v0], &b.meta[v0])) return false;
		}
		for (uint32_t i = 0; i < b.nv; ++i) { rid[b.first + i] = b.meta[i].rid; pos[b.first + i] = b.meta[i].pos; }
		if (meta_out) for (uint32_t i = 0; i < b.nv; ++i) (*meta_out)[b.first + i] = b.meta[i];
		return true;
	};
	auto decoder = [&](uint32_t w) {
		std::vector<uint8_t> z;                          // compressed block, sized once
		z.reserve(max_cmp + 16);
		std::unique_ptr<uint8_t[]> own(new (std::nothrow) uint8_t[max_bytes]);
		if (!own) { fail("Out of host memory for the decode buffers"); return; }
		for (;;) {
			const size_t bi = next_batch++;
			if (bi >= n_batches || failed) return;
			const auto t0 = lclock::now();
			if (!decode_batch(batches[bi], own.get(), z)) {
				fail("Failed to load blocks " + std::to_string(batches[bi].k0) + "-" + std::to_string(batches[bi].k1) + "!");
				return;
			}
			busy_decode[w] += std::chrono::duration<double>(lclock::now() - t0).count();
			{
				std::unique_lock<std::mutex> lk(mu);
				cv_slot.wait(lk, [&] { return failed || bi < released + n_slots; });
				if (failed) return;
			}
			const auto t1 = lclock::now();
			std::memcpy(ring.p + (bi % n_slots) * max_bytes, own.get(), batches[bi].bytes);
			busy_decode[w] += std::chrono::duration<double>(lclock::now() - t1).count();
			{ std::lock_guard<std::mutex> lk(mu); ready[bi] = 1; }
			cv_ready.notify_all();
		}
	};
	auto uploader = [&](size_t g) {
		for (size_t bi = 0; bi < n_batches; ++bi) {
			{
				std::unique_lock<std::mutex> lk(mu);
				cv_ready.wait(lk, [&] { return failed || ready[bi]; });
				if (failed) return;
			}
			const LoadBatch& b = batches[bi];
			const auto t0 = lclock::now();
			const int rc = twk_hip_upload_rle(ctxs[g], b.first, b.nv, ring.p + (bi % n_slots) * max_bytes, b.bytes, b.desc.data(), b.meta.data());
			busy_upload[g] += std::chrono::duration<double>(lclock::now() - t0).count();
			if (rc != TWK_HIP_OK) {
				const char* m = twk_hip_last_error(ctxs[g]);
				fail(std::string("twk_hip_upload_rle: ") + twk_hip_strerror(rc) + (m && m[0] ? std::string(" (") + m + ")" : std::string()));
				return;
			}
			std::lock_guard<std::mutex> lk(mu);
			if (--pending[bi] == 0) {                         // every GPU is in file order, so batches leave in file order too
				while (released < n_batches && pending[released] == 0) ++released;
				cv_slot.notify_all();
			}
		}
	};
	std::vector<std::thread> th;
	for (size_t g = 0; g < n_gpus; ++g) th.emplace_back(uploader, g);
	for (uint32_t w = 0; w < n_workers; ++w) th.emplace_back(decoder, w);
	for (auto& t : th) t.join();
	if (failed) { std::cerr << stamp("ERROR") << fail_msg << std::endl; return false; }
	double dec = 0, up = 0;
	for (double x : busy_decode) dec += x;
	for (double x : busy_upload) up = std::max(up, x);
	std::cerr << stamp("LOG", "UNPACK") << n_batches << " batches, " << total_unc / 1000000 << " MB of run-length genotypes in "
	          << std::chrono::duration<double>(lclock::now() - t_begin).count() << " s: " << n_workers << " decode threads busy " << dec
	          << " s in all (read + decompress + copy to staging), copy + device inflate " << up
	          << " s per GPU, device + staging allocations " << t_alloc << " s, " << n_slots << " staging slots of "
	          << max_bytes / 1000000 << " MB" << (ring.pinned ? "" : " (not page-locked)") << std::endl;
	return true;
}

// TWK_REF_COMPAT=1: reproduce slips of the reference that change output bytes instead of the correct result -
// PhasedVectorized's tail / padding arithmetic (q6/q7; TWK_HIP_OPT_REF_COMPAT, include/twk_hip.h), scalc's dropping
// of the last partial group of 100 neighbours (q15) and, with -w, the reference's window mode as it really
// behaves (q8; twk_ld_impl::compat_keep).  The off-diagonal-chunk slip (q9) is not reproduced.
static bool ref_compat() { const char* e = std::getenv("TWK_REF_COMPAT"); return e && e[0] && e[0] != '0'; }

// The r2 screen (TWK_HIP_OPT_R2_SCREEN) is on unless TWK_HIP_NO_SCREEN=1 (A/B comparisons; the records are the same).
static bool r2_screen() { const char* e = std::getenv("TWK_HIP_NO_SCREEN"); return !(e && e[0] && e[0] != '0'); }

// TWK_HIP_PART=k/n: this process's share of a multi-process run.
static bool part_from_env(uint32_t& part0, uint32_t& n_procs) {
	part0 = 0; n_procs = 1;
	if (const char* e = std::getenv("TWK_HIP_PART")) {
		unsigned k = 0, n = 1;
		if (sscanf(e, "%u/%u", &k, &n) == 2 && n >= 1 && k < n) { part0 = k; n_procs = n; }
		else { std::cerr << stamp("ERROR") << "Bad TWK_HIP_PART (want k/n): " << e << std::endl; return false; }
	}
	return true;
}

static bool create_devices(DeviceCtxs& dc, int n_gpus, const std::vector<std::pair<std::string, int64_t>>& options) {
	int64_t force_device = -1;                                       // option "force_device" (testing): several engine contexts on one GPU
	for (const auto& kv : options) if (kv.first == "force_device") force_device = kv.second;
	const bool force = force_device >= 0;
	const char* dev_env = std::getenv("TWK_HIP_DEVICE");
	if (twk_hip_abi_version() != TWK_HIP_ABI_VERSION) {      // (struct layouts cross this boundary: twk_hip_timing, twk_hip_record)
		std::cerr << stamp("ERROR", "HIP") << "libtwk_hip has ABI version " << twk_hip_abi_version() << ", this library was built against " << TWK_HIP_ABI_VERSION << "." << std::endl;
		return false;
	}
	const int n_dev = twk_hip_device_count();
	if (n_dev <= 0) { std::cerr << stamp("ERROR", "HIP") << "No HIP device available (this build has no CPU path)." << std::endl; return false; }
	if (!force && n_gpus > n_dev) { std::cerr << stamp("ERROR", "HIP") << "TWK_HIP_GPUS=" << n_gpus << " but only " << n_dev << " device(s) are visible." << std::endl; return false; }
	for (int g = 0; g < n_gpus; ++g) {
		const int device = force ? (int)force_device : (n_gpus == 1 && dev_env ? std::atoi(dev_env) : g);
		twk_hip_ctx* c = nullptr;
		if (!hip_ok(nullptr, twk_hip_ctx_create(device, &c), "twk_hip_ctx_create")) return false;
		dc.ctx.push_back(c);
		for (const auto& kv : options) {
			if (kv.first == "force_device" || kv.first == "progress_ms" || kv.first == "map_output" || kv.first == "emit_workers" || kv.first == "emit_backlog_mb" || kv.first == "emit_queue_pieces" || kv.first == "record_codec" || kv.first == "direct_output" || kv.first == "gather") continue;       // this class's own
			if (!hip_ok(c, twk_hip_set_option(c, kv.first.c_str(), kv.second), "twk_hip_set_option")) return false;
		}
	}
	return true;
}
// `--keep` / `--remove`: the context, loaded with every sample of the input, becomes the problem of the kept samples (twk_hip_select_samples:
// selected on the device, ac / an / missing recomputed there), and every variant's Hardy-Weinberg P is recomputed over them - the genotype
// counts from the device's marginals, the importer's exact test on T host threads - so that the context holds what a re-import of the
// subset would have uploaded.  meta_out (may be null): the caller's copy of the metadata follows.
static bool apply_sample_selection(twk_hip_ctx* ctx, const std::vector<uint32_t>& keep, uint32_t M, uint32_t T, std::vector<twk_hip_variant_meta>* meta_out) {
	if (keep.empty() || M == 0) return true;
	if (!hip_ok(ctx, twk_hip_select_samples(ctx, keep.data(), (uint32_t)keep.size()), "twk_hip_select_samples")) return false;
	std::vector<uint32_t> het(M), hom(M), miss(M);
	if (!hip_ok(ctx, twk_hip_get_marginals(ctx, nullptr, het.data(), hom.data(), miss.data()), "twk_hip_get_marginals")) return false;
	std::vector<double> hwe(M);
	const uint64_t n = keep.size();
	const size_t piece = 4096, n_pieces = (M + piece - 1) / piece;
	struct None {};
	const bool ok = par::ordered_parallel<None>(n_pieces, (int)T,
		[&](size_t i, None&) {
			for (size_t v = i * piece; v < std::min<size_t>(M, (i + 1) * piece); ++v)
				hwe[v] = hardy_weinberg_exact(n - het[v] - hom[v] - miss[v], het[v], hom[v]);      // over the complete genotypes, as the importer counts them
			return true;
		},
		[](size_t, None&) { return true; });
	if (!ok) return false;
	if (!hip_ok(ctx, twk_hip_set_hwe(ctx, 0, M, hwe.data()), "twk_hip_set_hwe")) return false;
	if (meta_out) {
		meta_out->resize(M);
		if (!hip_ok(ctx, twk_hip_get_meta(ctx, 0, M, meta_out->data()), "twk_hip_get_meta")) return false;
	}
	return true;
}

// `--extract` / `--exclude` / `--maf` / `--max-maf` / `--mac` / `--geno` / `--hwe`.  The list files are read before any device work
// (read_variant_lists: an unreadable file or a line that does not parse ends the command there); after the upload, the sample selection and
// its Hardy-Weinberg P, the lists are matched against the loaded variants' positions and every context - each holds the same M variants -
// becomes the problem of the kept variants (twk_hip_select_variants: the rule is the engine's).  The host's tables follow the map: rid and
// pos are compacted, nL / nR - the variants of the L range and of the R range of a chunk, or scalc's targets and neighbours - become the
// kept ones among them, and meta_out (may be null) is read back.  Every per-variant side input is matched against rid / pos after this.
namespace {
struct VariantLists { std::vector<VariantListEntry> extract, exclude; };
}
static bool read_variant_lists(const twk_ld_settings& settings, VariantLists& lists) {
	std::string err;
	if (!settings.extract_file.empty() && !read_variant_file(settings.extract_file, "--extract", lists.extract, err)) { std::cerr << stamp("ERROR") << err << "..." << std::endl; return false; }
	if (!settings.exclude_file.empty() && !read_variant_file(settings.exclude_file, "--exclude", lists.exclude, err)) { std::cerr << stamp("ERROR") << err << "..." << std::endl; return false; }
	return true;
}
static bool apply_variant_selection(const std::vector<twk_hip_ctx*>& ctxs, const twk_ld_settings& settings, const VariantLists& lists, const Header& hdr,
                                    std::vector<uint32_t>& rid, std::vector<uint32_t>& pos, uint32_t& nL, uint32_t& nR, std::vector<twk_hip_variant_meta>* meta_out) {
	if (!settings.selects_variants() || ctxs.empty()) return true;
	const uint32_t M = (uint32_t)rid.size();
	std::vector<std::string> contigs;
	for (const auto& c : hdr.contigs) contigs.push_back(c.name);
	std::vector<uint32_t> list;
	bool have_list = false; int32_t exclude = 0;
	if (!settings.extract_file.empty()) {
		uint64_t absent = 0;
		match_variant_list(contigs, rid.data(), pos.data(), M, lists.extract, list, &absent);
		std::cerr << stamp("LOG") << "--extract: " << pretty(list.size()) << " variants at the listed positions" << (absent ? "; " + pretty(absent) + " listed positions are not among the loaded variants" : std::string()) << "..." << std::endl;
		have_list = true;
	}
	if (!settings.exclude_file.empty()) {
		uint64_t absent = 0;
		std::vector<uint32_t> out;
		match_variant_list(contigs, rid.data(), pos.data(), M, lists.exclude, out, &absent);
		std::cerr << stamp("LOG") << "--exclude: " << pretty(out.size()) << " variants at the listed positions" << (absent ? "; " + pretty(absent) + " listed positions are not among the loaded variants" : std::string()) << "..." << std::endl;
		if (have_list) {          // both: extract, then exclude
			std::vector<uint32_t> rest;
			std::set_difference(list.begin(), list.end(), out.begin(), out.end(), std::back_inserter(rest));
			list.swap(rest);
		} else { list.swap(out); exclude = 1; have_list = true; }
	}
	if (have_list && !exclude && list.empty()) { std::cerr << stamp("ERROR") << "No variant is left after --extract / --exclude..." << std::endl; return false; }
	twk_hip_variant_filter f{};
	f.min_maf = settings.min_maf; f.max_maf = settings.max_maf; f.min_mac = settings.min_mac; f.max_missing = settings.max_missing; f.min_hwe = settings.min_hwe;
	const uint32_t none = 0;
	uint32_t n_kept = 0;
	for (twk_hip_ctx* ctx : ctxs) {
		if (!hip_ok(ctx, twk_hip_select_variants(ctx, &f, have_list ? (list.empty() ? &none : list.data()) : nullptr, (uint32_t)list.size(), exclude, &n_kept), "twk_hip_select_variants")) return false;
	}
	std::vector<uint32_t> map(n_kept);
	if (!hip_ok(ctxs[0], twk_hip_variant_map(ctxs[0], 0, n_kept, map.data()), "twk_hip_variant_map")) return false;
	std::cerr << stamp("LOG") << "Keeping " << pretty(n_kept) << " of " << pretty(M) << " variants..." << std::endl;
	uint32_t kL = 0;
	for (uint32_t k = 0; k < n_kept; ++k) {
		if (map[k] < nL) ++kL;
		rid[k] = rid[map[k]]; pos[k] = pos[map[k]];          // (the map ascends: map[k] >= k)
	}
	rid.resize(n_kept); pos.resize(n_kept);
	nR = nR ? n_kept - kL : 0; nL = kL;
	if (meta_out) {
		meta_out->resize(n_kept);
		if (!hip_ok(ctxs[0], twk_hip_get_meta(ctxs[0], 0, n_kept, meta_out->data()), "twk_hip_get_meta")) return false;
	}
	return true;
}

static int gpus_from_env() {
	if (const char* g = std::getenv("TWK_HIP_GPUS")) { const int n = std::atoi(g); if (n >= 1) return std::min(n, 64); }
	return 1;
}

// compute + write + final log lines (ld.cpp:620-668, ld_progress.h:89-96)
bool twk_ld::twk_ld_impl::run(twk_ld_settings& settings, const Header& hdr, const std::vector<twk_hip_ctx*>& ctxs, uint32_t n_samples, const void* spec_) {
	using clock = std::chrono::steady_clock;
	const RunSpec& spec = *static_cast<const RunSpec*>(spec_);
	if (!open_output(settings, hdr, out.writer)) return false;
	// Engine option "map_output" = 1: blocks go into the file through a shared mapping, copied in by the emitter's workers in
	// parallel (twk_format.h).  Built because round 3's single writer thread looked like the bound of survivor-rich runs;
	// measured on the GPU box it is 2-3x *slower* than the stream (66 M records, 4.3 GB: 2.8-3.0 s against 1.0 s,
	// profiles/r04_writer_ab.txt - 32 threads taking page faults in one address space do not scale there), so the stream
	// stays the default and the mapping an option.
	if (option("map_output", 0)) (void)out.writer.map_output();
	// Engine option "direct_output" = 1: the block frames go into the file with one pwritev() each, its space reserved ahead
	// (twk_format.h) - with the record codec the one stream into the file is what a survivor-rich run waits for.
	else if (option("direct_output", 0)) (void)out.writer.direct_output();
	out.b_size = (uint32_t)std::max(2, settings.b_size);
	// The blocks' zstd frames come from the records' own encoder (twk_repcodec.h) instead of libzstd wherever the run asks for the
	// fastest level (-k <= 1, the reference's default, lib/core.cpp:304): what binds a survivor-rich run is libzstd's level 1 itself
	// (2,504 x 531,500 -p -w 4000000, 37 M records: compute + write 0.69 -> 0.42 s for a file 6 % larger).  -k 2 and up asks
	// for ratio and gets libzstd at that level; engine option "record_codec" = 0 / 1 says so either way.
	const bool own_codec = option("record_codec", -1) < 0 ? settings.c_level <= 1 : option("record_codec", -1) != 0;
	out.c_level = own_codec ? (int)RECORD_CODEC_LEVEL + std::max(-999, std::min(settings.c_level, 999)) : settings.c_level;
	out.rid = rid.data(); out.pos = pos.data(); out.n_variants = rid.size(); out.n_records = 0;
	n_records = 0; n_pairs = 0;
	const int n_gpus = (int)ctxs.size();
	// output workers per GPU: 32 at most (beyond that the one placing step and the memory system are the limit)
	// (and never more threads than the process has CPUs - its affinity mask, its container's quota: util::usable_cpus)
	int n_workers = std::max(1, std::min(std::max(1, std::min(settings.n_threads, util::usable_cpus()) / n_gpus), 32));
	if (option("emit_workers", 0) > 0) n_workers = (int)std::min<int64_t>(option("emit_workers", 0), 64);      // (measurement: the emitter's worker threads per GPU)
	const int mode = settings.single ? TWK_HIP_MODE_AUTO
	               : settings.force_phased ? TWK_HIP_MODE_PHASED : (settings.forced_unphased ? TWK_HIP_MODE_UNPHASED : TWK_HIP_MODE_AUTO);
	twk_hip_filters f{settings.minR2, settings.maxR2, settings.minDprime, settings.maxDprime, settings.minP};
	// Shards: GPU g of this process takes part k * n_gpus + g of n * n_gpus of every region, where k/n is
	// this process's share of a multi-node (farm) run: TWK_HIP_PART=k/n (the reference's -c/-C idea,
	// ld_balancing.h:23-80, with equal-area row bands; `concat` merges the processes' outputs).
	uint32_t part0 = 0, n_procs = 1;
	if (!part_from_env(part0, n_procs)) return false;
	const uint32_t n_parts = n_procs * (uint32_t)n_gpus;
	const auto t0 = clock::now();
	// Progress lines like the reference's ticker (ld_progress.h:40-86), every 30 s, driven by the
	// engines' per-tile callbacks instead of a polling thread.
	struct Progress {
		twk_ld_impl* self; clock::time_point t0, last; uint64_t total = 0; uint32_t n_s = 0; bool header = false;
		double every = 30.0;
		std::mutex mu;
		std::vector<uint64_t> done, base;         // per GPU: pairs finished in the current / earlier region calls
		struct PerGpu { Progress* p; int g; };
		static void cb(void* u, uint64_t pairs_done, uint32_t, uint32_t) {
			PerGpu& pg = *static_cast<PerGpu*>(u);
			Progress& p = *pg.p;
			std::lock_guard<std::mutex> lk(p.mu);
			p.done[pg.g] = pairs_done;
			const auto now = clock::now();
			if (std::chrono::duration<double>(now - p.last).count() < p.every) return;
			p.last = now;
			if (!p.header) {
				std::cerr << stamp("PROGRESS") << std::setw(12) << "Time elapsed" << std::setw(15) << "Variants" << std::setw(20) << "Genotypes"
				          << std::setw(15) << "Output" << std::setw(10) << "Progress" << "\tEst. Time left" << std::endl;
				p.header = true;
			}
			const double sec = std::chrono::duration<double>(now - p.t0).count();
			uint64_t done = 0;
			for (size_t g = 0; g < p.done.size(); ++g) done += p.done[g] + p.base[g];
			const double frac = p.total ? (double)done / (double)p.total : 0.0;
			uint64_t n_out;
			{ std::lock_guard<std::mutex> lo(p.self->out.mu); n_out = p.self->out.n_records; }
			std::cerr << stamp("PROGRESS") << std::setw(12) << elapsed_string(sec) << std::setw(15) << pretty(done)
			          << std::setw(20) << pretty(done * p.n_s) << std::setw(15) << pretty(n_out)
			          << std::setw(10) << frac * 100 << "%\t" << (frac > 0 ? elapsed_string(sec * (1 - frac) / frac) : std::string("-")) << std::endl;
		}
	} progress;
	progress.self = this; progress.t0 = progress.last = t0; progress.n_s = n_samples;
	progress.done.assign(n_gpus, 0); progress.base.assign(n_gpus, 0);
	progress.every = (double)option("progress_ms", (int64_t)(progress.every * 1000.0)) / 1000.0;      // (test hook)
	progress.total = (spec.triangleA && spec.nA > 1 ? (uint64_t)spec.nA * (spec.nA - 1) / 2 : 0) + (spec.rectAB ? (uint64_t)spec.nA * spec.nB : 0);
	if (n_procs > 1) progress.total /= n_procs;
	std::vector<Progress::PerGpu> per_gpu(n_gpus);

	// one driver thread per GPU: region calls for its shard, survivors into its own emitter
	struct Driver {
		twk_ld_impl* self;
		std::vector<twk_hip_record> kept;      // declared before the emitter: its workers read it until they are joined
		RecordEmitter emitter; bool write_failed = false; uint64_t pairs = 0; int rc = TWK_HIP_OK;
		RecordHandOff handoff;                 // between the engine's thread (sink below) and the emitter (twk_record_sink.h)
		uint32_t shift = 0;
		Driver(twk_ld_impl* s, int workers, size_t backlog, size_t pieces) : self(s), emitter(s->out, workers, backlog), handoff(emitter, pieces) {}
		bool drain() {
			if (!handoff.drain()) write_failed = true;
			return !write_failed;
		}
		static int sink(void* user, const twk_hip_record* recs, uint64_t n) {
			auto* d = static_cast<Driver*>(user);
			const bool edit = d->shift || d->self->cw.on;
			// slab-local variant indices -> positions in the run's rid / pos arrays; TWK_REF_COMPAT window filter
			auto fix = [d](twk_hip_record& r) -> bool {
				r.idxA += d->shift; r.idxB += d->shift;
				return !d->self->cw.on || d->self->compat_keep(r.idxA, r.idxB);
			};
			if (d->handoff.takes(n)) {
				if (!(edit ? d->handoff.put(recs, n, fix) : d->handoff.put(recs, n))) { d->write_failed = true; return 1; }
				return 0;
			}
			if (!d->drain()) return 1;           // (no queue, or a piece larger than its buffers: in order behind what is queued)
			if (edit) {
				d->kept.clear();
				for (uint64_t i = 0; i < n; ++i) {
					twk_hip_record r = recs[i];
					if (fix(r)) d->kept.push_back(r);
				}
				recs = d->kept.data(); n = d->kept.size();
			}
			if (!d->emitter.emit(recs, n, false, true)) { d->write_failed = true; return 1; }     // (the engine's survivors come sorted)
			return 0;
		}
	};
	std::vector<std::unique_ptr<Driver>> drivers;
	// expanded blocks that may wait in memory for the compressing workers, per GPU (twk_record_sink.h; measurement: none pays)
	const size_t backlog = (size_t)std::max<int64_t>(0, option("emit_backlog_mb", 0)) << 20;
	// buffers of the hand-off between the engine's thread and the emitter, per GPU (Driver above; 0: none, the sink feeds the emitter itself)
	// (8: 2,504 x 531,500 `-p` 1.02 -> 0.86 s, `-u` 1.57 -> 1.42 s of compute + write; 32 and 64 no better; window runs, which wait
	// for the compression whatever the queue holds, within their noise - profiles/r04_band_sort_ab.txt)
	const size_t pieces = (size_t)std::max<int64_t>(0, option("emit_queue_pieces", 8));
	for (int g = 0; g < n_gpus; ++g) drivers.emplace_back(new Driver(this, n_workers, backlog, pieces));
	// Engine option "gather" = 1 (the north star's "final RCCL gather of .two output blocks over xGMI", inside this one process): every GPU keeps
	// its survivors in HBM (twk_hip_set_device_sink), and when all are done they travel GPU to GPU over RCCL into GPU 0's sink
	// (twk_hip_gather_records: one group of exact-size ncclSend / ncclRecv), from where they leave for the host once, into ONE emitter.  Default 0:
	// every GPU's driver thread streams its survivors to the host while it computes (one hop fewer for a file sink, and no bound on the
	// survivors by GPU 0's memory: INTEGRATION 1).  With one GPU the records take the same calls in a loop from the sink to itself.
	const bool gather = option("gather", 0) != 0;
	if (gather) for (int g = 0; g < n_gpus; ++g) if (!hip_ok(ctxs[g], twk_hip_set_device_sink(ctxs[g], 1), "twk_hip_set_device_sink")) return false;
	auto drive = [&](int g) {
		Driver& d = *drivers[g];
		twk_hip_ctx* ctx = ctxs[g];
		const uint32_t part = part0 * (uint32_t)n_gpus + (uint32_t)g;
		per_gpu[g] = Progress::PerGpu{&progress, g};
		twk_hip_set_progress(ctx, &Progress::cb, &per_gpu[g]);
		uint64_t np = 0, nr = 0;
		if (!spec.slabs.empty()) {          // this GPU's own slab: its band of rows against band + halo, nothing to shard
			const RunSpec::Slab& sl = spec.slabs[g];
			d.shift = sl.first;
			if (sl.n_band && sl.n_local > 1)
				d.rc = twk_hip_ld_region(ctx, mode, &f, 0, sl.n_band, 0, sl.n_local, 1, 0, 1, 0, spec.options, spec.l_window, &Driver::sink, &d, &np, &nr);
			d.pairs += np;
		} else
		if (spec.triangleA && spec.nA > 1) {
			d.rc = twk_hip_ld_region(ctx, mode, &f, 0, spec.nA, 0, spec.nA, 1, part, n_parts, 0, spec.options, spec.l_window, &Driver::sink, &d, &np, &nr);
			d.pairs += np;
			std::lock_guard<std::mutex> lk(progress.mu);
			progress.base[g] += np; progress.done[g] = 0;
		}
		if (spec.slabs.empty() && d.rc == TWK_HIP_OK && spec.rectAB && spec.nA && spec.nB) {
			d.rc = twk_hip_ld_region(ctx, mode, &f, 0, spec.nA, spec.nA, spec.nB, 0, part, n_parts, 0, spec.options, spec.l_window, &Driver::sink, &d, &np, &nr);
			d.pairs += np;
		}
		twk_hip_set_progress(ctx, nullptr, nullptr);
		if (gather) return;                 // (the survivors are still in HBM: gathered and written below)
		if (!d.drain()) d.write_failed = true;
		if (d.rc == TWK_HIP_OK && !d.write_failed && !d.emitter.emit(nullptr, 0, true)) d.write_failed = true;     // close the open blocks
	};
	if (n_gpus == 1) drive(0);
	else {
		std::vector<std::thread> th;
		for (int g = 0; g < n_gpus; ++g) th.emplace_back(drive, g);
		for (auto& t : th) t.join();
	}
	if (gather) {
		for (int g = 0; g < n_gpus; ++g) if (!hip_ok(ctxs[g], drivers[g]->rc, "twk_hip_ld_region")) return false;
		// what every GPU holds (its slab's index shift applies to its records wherever they travel), then the gather, then GPU 0 -> host -> emitter 0
		struct Feed {
			Driver* d0; std::vector<uint64_t> end; std::vector<uint32_t> shift; uint64_t seen = 0; std::vector<twk_hip_record> tmp;
			static int sink(void* user, const twk_hip_record* recs, uint64_t n) {
				auto* f = static_cast<Feed*>(user);
				uint64_t i = 0;
				while (i < n) {
					size_t g = 0;
					while (g + 1 < f->end.size() && f->seen >= f->end[g]) ++g;
					const uint64_t m = std::min<uint64_t>(n - i, f->end[g] > f->seen ? f->end[g] - f->seen : n - i);
					f->tmp.clear();
					for (uint64_t k = 0; k < m; ++k) {
						twk_hip_record r = recs[i + k];
						r.idxA += f->shift[g]; r.idxB += f->shift[g];
						if (!f->d0->self->cw.on || f->d0->self->compat_keep(r.idxA, r.idxB)) f->tmp.push_back(r);
					}
					// (a piece of the sink may span launches: each launch's records are in order, the piece need not be - the emitter sorts what is not)
					if (!f->tmp.empty() && !f->d0->emitter.emit(f->tmp.data(), f->tmp.size(), false, false)) { f->d0->write_failed = true; return 1; }
					f->seen += m; i += m;
				}
				return 0;
			}
		} feed;
		feed.d0 = drivers[0].get();
		uint64_t total = 0;
		std::vector<uint64_t> held(n_gpus, 0);
		for (int g = 0; g < n_gpus; ++g) {
			const twk_hip_record* p = nullptr;
			if (!hip_ok(ctxs[g], twk_hip_device_records(ctxs[g], &p, &held[g]), "twk_hip_device_records")) return false;
			total += held[g];
			feed.end.push_back(total); feed.shift.push_back(drivers[g]->shift);
		}
		const auto t_g = clock::now();
		uint64_t got = 0; double xfer_ms = 0;
		int grc = twk_hip_gather_records(ctxs.data(), (uint32_t)n_gpus, 0, n_gpus == 1 ? TWK_HIP_GATHER_SELF_LOOP : 0, &got, &xfer_ms);
		if (grc == TWK_HIP_OK) {
			if (got != total) { std::cerr << stamp("ERROR", "HIP") << "gather: " << got << " records arrived, " << total << " were held." << std::endl; return false; }
			std::cerr << stamp("LOG", "HIP") << "Gathered " << pretty(total) << " records of " << n_gpus << " GPU(s) into GPU 0 over " << twk_hip_gather_backend()
			          << (n_gpus == 1 ? " (one GPU: from its sink to itself)" : "") << ": " << pretty((total - held[0]) * sizeof(twk_hip_record)) << " bytes moved"
			          << (n_gpus == 1 ? " (+ the loop's " + pretty(held[0] * sizeof(twk_hip_record)) + ")" : std::string()) << ", transfers " << xfer_ms << " ms, "
			          << std::chrono::duration<double, std::milli>(clock::now() - t_g).count() << " ms in all." << std::endl;
			uint64_t nd = 0;
			if (!hip_ok(ctxs[0], twk_hip_drain_device_sink(ctxs[0], &Feed::sink, &feed, &nd), "twk_hip_drain_device_sink")) return false;
		} else {
			// no RCCL, or not enough room on GPU 0 for everybody's survivors: every GPU's sink goes to the host by itself, one after the other
			std::cerr << stamp("WARNING", "HIP") << "gather over RCCL not possible (" << twk_hip_last_error(ctxs[0]) << "): the GPUs' survivors go to the host one GPU at a time." << std::endl;
			for (int g = 0; g < n_gpus; ++g) {
				uint64_t nd = 0;
				if (!hip_ok(ctxs[g], twk_hip_drain_device_sink(ctxs[g], &Feed::sink, &feed, &nd), "twk_hip_drain_device_sink")) return false;
			}
		}
		for (int g = 0; g < n_gpus; ++g) (void)twk_hip_set_device_sink(ctxs[g], 0);
		if (!drivers[0]->write_failed && !drivers[0]->emitter.emit(nullptr, 0, true)) drivers[0]->write_failed = true;
	}
	for (int g = 0; g < n_gpus; ++g) {
		if (drivers[g]->write_failed) { std::cerr << stamp("ERROR", "WRITER") << "Failed to write output block!" << std::endl; return false; }
		if (!hip_ok(ctxs[g], drivers[g]->rc, "twk_hip_ld_region")) return false;
		n_pairs += drivers[g]->pairs;
	}
	n_records = out.n_records;
	const double sec = std::chrono::duration<double>(clock::now() - t0).count();
	std::cerr << stamp("PROGRESS") << "Finished in " << elapsed_string(sec) << ". Variants: " << pretty(n_pairs) << ", genotypes: "
	          << pretty(n_pairs * n_samples) << ", output: " << pretty(n_records) << std::endl;
	std::cerr << stamp("PROGRESS") << pretty((uint64_t)(n_pairs / std::max(sec, 1e-9))) << " variants/s and "
	          << pretty((uint64_t)((double)n_pairs * n_samples / std::max(sec, 1e-9))) << " genotypes/s" << std::endl;
	for (int g = 0; g < n_gpus; ++g) {
		twk_hip_timing tm;
		if (twk_hip_timing_get(ctxs[g], &tm) == TWK_HIP_OK)
			std::cerr << stamp("LOG", "HIP") << (n_gpus > 1 ? "GPU " + std::to_string(g) + ": " : std::string()) << "count kernel " << tm.count_ms << " ms in "
			          << tm.count_launches << " launches ("
			          // what the launches issued: one AND+popcount (6 cycles per wave) per word of a plane-row pair - three for every four of them in
			          // the three-product form (v_and / v_bitop3 + v_bcnt: no other instruction since round 6), and two popcounts behind a v_or and a
			          // v_bitop3 - 12 cycles for the 24 of four products - in its (U, Z) form
			          << (tm.count_ms > 0 ? ((double)(tm.row_pairs - tm.three_row_pairs) + (double)(tm.three_row_pairs - tm.uz_row_pairs) * 0.75 + (double)tm.uz_row_pairs * 0.5) * (double)tm.words_per_row / (tm.count_ms * 1e-3) / 2.62e13 * 100.0 : 0.0)
			          << " % of the and+bcnt issue ceiling over the tiles it contracted"
			          << (tm.count_wall_ticks ? "; its blocks ran at " + std::to_string((int)((double)tm.count_shader_cycles / (double)tm.count_wall_ticks * 100.0 + 0.5)) + " MHz" : std::string())
			          << "), math kernels " << tm.stats_ms << " ms"
			          << (tm.fused_launches ? "; " + std::to_string(tm.fused_launches) + " launches fused count -> r2 screen, " + pretty(tm.candidates) + " candidate slots" : std::string())
			          << (tm.three_launches ? "; " + std::to_string(tm.three_launches) + " launches in the three-product form (HH + S), " + pretty(tm.recount_candidates) + " candidates recounted" : std::string())
			          << (tm.uz_launches ? "; " + std::to_string(tm.uz_launches) + " of them counted (U, Z), two popcounts a word" : std::string())
			          << (tm.prefix_launches && tm.prefix_chunks_full ? "; " + std::to_string(tm.prefix_launches) + " launches contracted a prefix of their rows, " +
			              std::to_string((int)(100.0 * (double)tm.prefix_chunks / (double)tm.prefix_chunks_full + 0.5)) + " % of them" : std::string())
			          << (tm.list_launches ? "; carrier-list kernel " + std::to_string(tm.list_ms) + " ms in " + std::to_string(tm.list_launches) + " launches over " + pretty(tm.list_pairs) + " rare pairs" : std::string())
			          << (tm.probe_launches ? "; probe kernel " + std::to_string(tm.probe_ms) + " ms in " + std::to_string(tm.probe_launches) + " launches over " + pretty(tm.probe_pairs) + " rare x common pairs" : std::string())
			          << std::endl;
	}
	{
		double t_sort = 0, t_blocks = 0;
		for (int g = 0; g < n_gpus; ++g) { t_sort = std::max(t_sort, drivers[g]->emitter.t_sort); t_blocks = std::max(t_blocks, drivers[g]->emitter.t_blocks); }
		std::cerr << stamp("LOG", "WRITER") << pretty(out.n_blocks) << " blocks, " << out.bytes_packed / 1000000 << " MB compressed; the producer spent "
		          << t_sort + t_blocks << " s handing its survivors over (the engine's thread " << drivers[0]->handoff.t_copy << " s copying them out of its buffer); workers: expanding " << drivers[0]->emitter.ns_expand.load() * 1e-9 << " s, compressing "
		          << drivers[0]->emitter.ns_pack.load() * 1e-9 << " s in all; writer thread " << drivers[0]->emitter.ns_write.load() * 1e-9 << " s" << (n_gpus > 1 ? " (slowest GPU's emitter)" : "") << std::endl;
	}
	if (!out.writer.close()) { std::cerr << stamp("ERROR", "WRITER") << "Failed to write final block!" << std::endl; return false; }
	return true;
}

// What a run computes on, from the settings: the input file, the blocks the intervals (-I) select, the chunk (-c / -C) of their
// pair space and the blocks of its row and column ranges.  Shared by Compute and Score.  *nothing_to_do: no valid data (the
// caller returns true, like the reference).
namespace {
struct Selection {
	TwkReader reader;
	uint32_t n_samples = 0;          // the samples the run computes over: the header's, or (--keep / --remove) the kept ones - reader.hdr.samples names exactly these
	uint32_t n_source = 0;           // the samples of the input: what is uploaded
	std::vector<uint32_t> keep;      // --keep / --remove: the kept samples' indices in the input, ascending; empty: no selection
	VariantLists lists;              // --extract / --exclude: the files' positions, matched against the loaded variants after the upload
	Balancer bal;
	std::vector<uint32_t> sel;       // the L range's blocks, then (square chunk only) the R range's
	uint32_t nL = 0, nR = 0, M = 0;
};
}  // namespace
// --keep / --remove resolved against the header, before any device work: keep = the kept samples' indices in the input, and the header's
// sample list becomes the kept names, so that whatever writes a sample count or sample names writes the kept ones.  Neither option:
// nothing changes and keep stays empty.
static bool select_samples(const twk_ld_settings& settings, Header& hdr, std::vector<uint32_t>& keep) {
	keep.clear();
	if (settings.keep_file.empty() && settings.remove_file.empty()) return true;
	std::string err;
	if (!resolve_sample_list(hdr.samples, settings.keep_file, settings.remove_file, keep, err)) { std::cerr << stamp("ERROR") << err << "..." << std::endl; return false; }
	std::vector<std::string> names;
	names.reserve(keep.size());
	for (uint32_t s : keep) names.push_back(hdr.samples[s]);
	std::cerr << stamp("LOG") << "Keeping " << pretty(keep.size()) << " of " << pretty(hdr.samples.size()) << " samples..." << std::endl;
	hdr.samples.swap(names);
	return true;
}

static bool select_blocks(twk_ld_settings& settings, Selection& S, bool* nothing_to_do) {
	*nothing_to_do = false;
	TwkReader& reader = S.reader;
	Balancer& bal = S.bal;
	std::vector<uint32_t>& sel = S.sel;
	uint32_t& nL = S.nL; uint32_t& nR = S.nR;
	if (settings.window && settings.n_chunks != 1) { std::cerr << stamp("ERROR") << "Cannot use chunking in window mode!" << std::endl; return false; }
	if (settings.bitmaps || settings.low_memory)
		std::cerr << stamp("LOG") << "Note: -m/-M are CPU memory-saving modes; the GPU engine keeps dense bit-planes in HBM." << std::endl;

	if (!open_input(reader, settings.in, true)) return false;
	S.n_source = (uint32_t)reader.hdr.samples.size();
	if (!select_samples(settings, reader.hdr, S.keep)) return false;
	if (!read_variant_lists(settings, S.lists)) return false;
	const uint32_t n_samples = S.n_samples = (uint32_t)reader.hdr.samples.size();
	std::cerr << stamp("LOG") << "Samples: " << pretty(n_samples) << "..." << std::endl;

	// The universe of blocks: all of them, or (-I) those overlapping the intervals
	// (ld.cpp:523-527, 257-277: whole blocks are loaded, like the reference).
	std::vector<uint32_t> universe;
	if (settings.ival_strings.empty()) {
		for (uint32_t b = 0; b < reader.index.ent.size(); ++b) universe.push_back(b);
	} else {
		for (const auto& str : settings.ival_strings) {
			Interval iv;
			if (!parse_interval(str, reader.hdr, iv)) return false;
			overlapping_blocks(reader.index, iv, universe);
		}
		std::sort(universe.begin(), universe.end());
		universe.erase(std::unique(universe.begin(), universe.end()), universe.end());
		if (universe.empty()) { std::cerr << stamp("ERROR", "INTERVAL") << "Found no blocks overlapping the provided range(s)..." << std::endl; return false; }
	}
	const uint32_t n_blocks = (uint32_t)universe.size();
	if (n_blocks == 0 || n_samples == 0) { std::cerr << stamp("ERROR") << "No valid data available..." << std::endl; *nothing_to_do = true; return true; }

	if (settings.window) settings.c_chunk = 0;
	if (!bal.build(n_blocks, (uint32_t)settings.n_chunks, (uint32_t)settings.c_chunk)) return false;
	std::cerr << stamp("LOG", "BALANCING") << "Using ranges [" << bal.fromL << "-" << bal.toL << "," << bal.fromR << "-" << bal.toR
	          << "] in " << (settings.window ? "window mode" : "square mode") << "..." << std::endl;

	// Selected blocks: the L range, then (square chunk only) the R range.
	for (uint32_t b = bal.fromL; b < bal.toL; ++b) { sel.push_back(universe[b]); nL += reader.index.ent[universe[b]].n; }
	if (!bal.diag) for (uint32_t b = bal.fromR; b < bal.toR; ++b) { sel.push_back(universe[b]); nR += reader.index.ent[universe[b]].n; }
	const uint32_t M = S.M = nL + nR;
	const uint64_t n_cmp = bal.diag ? (uint64_t)M * (M - 1) / 2 : (uint64_t)nL * nR;
	std::cerr << stamp("LOG") << pretty(M) << " variants from " << pretty(sel.size()) << " blocks..." << std::endl;
	std::cerr << stamp("LOG", "PARAMS") << settings.GetString() << std::endl;
	std::cerr << stamp("LOG") << "Performing: " << pretty(n_cmp) << " variant comparisons..." << std::endl;

	return true;
}

bool twk_ld::Compute() {
	using clock = std::chrono::steady_clock;
	mImpl->n_pairs = mImpl->n_records = 0;
	if (settings.in.empty()) { std::cerr << stamp("ERROR") << "No file-name provided..." << std::endl; return false; }
	Selection S;
	bool nothing_to_do = false;
	if (!select_blocks(settings, S, &nothing_to_do)) return false;
	if (nothing_to_do) return true;
	TwkReader& reader = S.reader;
	const Balancer& bal = S.bal;
	const std::vector<uint32_t>& sel = S.sel;
	const uint32_t n_samples = S.n_samples;
	uint32_t nL = S.nL, nR = S.nR, M = S.M;      // (a variant selection shrinks them after the upload)

	const int n_gpus = gpus_from_env();
	uint32_t part0 = 0, n_procs = 1;
	if (!part_from_env(part0, n_procs)) return false;
	const uint32_t n_parts = n_procs * (uint32_t)n_gpus;
	// (window mode on several GPUs or processes: every GPU loads its own band and halo, below)
	const bool slabs = settings.window && bal.diag && n_parts > 1 && !(ref_compat() && !(settings.force_phased || settings.forced_unphased));
	// a variant selection needs one context that holds the command's whole variant set: refused before any device is touched
	if (settings.selects_variants() && (slabs || (ref_compat() && settings.window))) {
		std::cerr << stamp("ERROR") << "--extract / --exclude / --maf / --max-maf / --mac / --geno / --hwe need one context that holds the command's whole variant set: not in window mode over "
		          << "several GPUs or processes (every GPU holds its own band and halo), and not in window mode under TWK_REF_COMPAT (its windows follow the input's blocks)..." << std::endl;
		return false;
	}
	DeviceCtxs dc;
	if (!create_devices(dc, n_gpus, mImpl->engine_options)) return false;
	if (n_gpus > 1) std::cerr << stamp("LOG", "HIP") << "Using " << n_gpus << " GPUs: one driver thread each, equal-area row bands of the pair space..." << std::endl;
	RunSpec spec;
	const auto t_load = clock::now();
	const uint32_t T = (uint32_t)std::max(1, std::min(settings.n_threads, util::usable_cpus()));
	std::cerr << stamp("LOG", "THREAD") << "Unpacking using " << T << " threads..."
	          << (T < (uint32_t)settings.n_threads ? " (of " + std::to_string(settings.n_threads) + " asked for: the process may use " + std::to_string(util::usable_cpus()) + " CPUs)" : std::string()) << std::endl;
	// Window mode on several GPUs (or processes): a GPU needs only the blocks of its band of rows plus the blocks its
	// window reaches beyond it (the reference's ticker prunes block pairs the same way, ld_balancing.h:176-203) -
	// for BASELINE configs[4] that is 75 GB per GPU instead of 500 GB.  Bands are cut at block boundaries with equal
	// estimated in-window pairs, from the index alone (block span and size), identically in every process.
	if (slabs) {
		const uint64_t w = (uint64_t)std::max(0, settings.l_window);
		const size_t nb = sel.size();
		auto ent = [&](size_t k) -> const IndexEntry& { return reader.index.ent[sel[k]]; };
		std::vector<size_t> reach(nb);                       // first block beyond what block k's window can touch
		std::vector<uint64_t> nvar(nb + 1, 0), cost(nb + 1, 0);
		for (size_t k = 0; k < nb; ++k) nvar[k + 1] = nvar[k] + ent(k).n;
		for (size_t k = 0, e = 0; k < nb; ++k) {
			if (e < k + 1) e = k + 1;
			while (e < nb && ent(e).rid == ent(k).rid && (uint64_t)ent(e).minpos <= (uint64_t)ent(k).maxpos + w) ++e;
			reach[k] = e;
			const uint64_t n = ent(k).n;
			cost[k + 1] = cost[k] + n * (n - 1) / 2 + n * (nvar[e] - nvar[k + 1]);
		}
		auto boundary = [&](uint32_t p) -> size_t {
			if (p == 0) return 0;
			if (p >= n_parts) return nb;
			const long double target = (long double)cost[nb] * p / n_parts;
			return (size_t)(std::lower_bound(cost.begin(), cost.end(), (uint64_t)target) - cost.begin());
		};
		std::vector<std::vector<uint32_t>> sel_g(n_gpus);
		for (int g = 0; g < n_gpus; ++g) {
			const uint32_t p = part0 * (uint32_t)n_gpus + (uint32_t)g;
			const size_t B0 = boundary(p), B1 = std::max(B0, boundary(p + 1));
			const size_t H1 = B1 > B0 ? std::max(B1, reach[B1 - 1]) : B1;
			RunSpec::Slab sl;
			sl.first = (uint32_t)nvar[B0]; sl.n_band = (uint32_t)(nvar[B1] - nvar[B0]); sl.n_local = (uint32_t)(nvar[H1] - nvar[B0]);
			spec.slabs.push_back(sl);
			for (size_t k = B0; k < H1; ++k) sel_g[g].push_back(sel[k]);
			std::cerr << stamp("LOG", "BALANCING") << "GPU " << g << ": rows = variants [" << sl.first << ", " << sl.first + sl.n_band << "), + "
			          << sl.n_local - sl.n_band << " halo variants" << std::endl;
		}
		mImpl->rid.assign(M, 0); mImpl->pos.assign(M, 0);
		std::vector<std::vector<uint32_t>> rid_g(n_gpus), pos_g(n_gpus);
		std::vector<char> ok(n_gpus, 1);
		std::vector<std::thread> th;
		for (int g = 0; g < n_gpus; ++g) th.emplace_back([&, g] {
			if (sel_g[g].empty()) return;
			const uint32_t Tg = std::max<uint32_t>(1, T / (uint32_t)n_gpus);
			if (!load_blocks(settings.in, reader, sel_g[g], Tg, {dc.ctx[g]}, S.n_source, rid_g[g], pos_g[g])) ok[g] = 0;
			else if (!apply_sample_selection(dc.ctx[g], S.keep, (uint32_t)rid_g[g].size(), Tg, nullptr)) ok[g] = 0;
		});
		for (auto& t : th) t.join();
		for (int g = 0; g < n_gpus; ++g) {
			if (!ok[g]) return false;
			std::copy(rid_g[g].begin(), rid_g[g].end(), mImpl->rid.begin() + spec.slabs[g].first);
			std::copy(pos_g[g].begin(), pos_g[g].end(), mImpl->pos.begin() + spec.slabs[g].first);
		}
	} else {
		if (!load_blocks(settings.in, reader, sel, T, dc.ctx, S.n_source, mImpl->rid, mImpl->pos)) return false;
		for (twk_hip_ctx* c : dc.ctx) if (!apply_sample_selection(c, S.keep, M, T, nullptr)) return false;
		if (!apply_variant_selection(dc.ctx, settings, S.lists, reader.hdr, mImpl->rid, mImpl->pos, nL, nR, nullptr)) return false;
		if (settings.selects_variants()) M = (uint32_t)mImpl->rid.size();
	}
	std::cerr << stamp("LOG") << "Unpacked and uploaded " << pretty(M) << " variants. "
	          << elapsed_string(std::chrono::duration<double>(clock::now() - t_load).count()) << std::endl;

	spec.nA = bal.diag ? M : nL; spec.nB = bal.diag ? 0 : nR;
	spec.triangleA = bal.diag; spec.rectAB = !bal.diag;
	spec.options = (settings.window ? TWK_HIP_OPT_WINDOW : 0) | (ref_compat() ? TWK_HIP_OPT_REF_COMPAT : 0) | (r2_screen() ? TWK_HIP_OPT_R2_SCREEN : 0);
	spec.l_window = (uint32_t)settings.l_window;
	mImpl->cw = twk_ld_impl::CompatWindow();
	if (ref_compat() && settings.window) {
		auto& cw = mImpl->cw;
		cw.on = true; cw.w = (uint32_t)settings.l_window;
		cw.forced = settings.force_phased || settings.forced_unphased;
		cw.blk_first.assign(1, 0);
		for (uint32_t b : sel) cw.blk_first.push_back(cw.blk_first.back() + reader.index.ent[b].n);
		cw.blk_of.resize(M);
		for (size_t k = 0; k + 1 < cw.blk_first.size(); ++k) for (uint32_t v = cw.blk_first[k]; v < cw.blk_first[k + 1]; ++v) cw.blk_of[v] = (uint32_t)k;
		// default mode: the reference tests no pair against the window, so pairs outside it come out too: compute them all
		if (!cw.forced) spec.options &= ~TWK_HIP_OPT_WINDOW;
	}
	if (!mImpl->run(settings, reader.hdr, dc.ctx, n_samples, &spec)) return false;
	std::cerr << stamp("LOG", "PROGRESS") << "All done..." << elapsed_string(std::chrono::duration<double>(clock::now() - t_load).count()) << "!" << std::endl;
	return true;
}

// What `ldscore`, `prune`, `clump`, `ldmatrix`, `lddecay` and `ldaggregate` share around their one engine call: the checks common to all, the input loaded exactly as
// Compute loads it onto one GPU, the text output with its `##` header, the `contig \t pos` that begins a variant's line, the closing lines.
namespace {
struct ReduceCommand {
	using clock = std::chrono::steady_clock;
	twk_ld_settings& settings;
	std::vector<uint32_t>& rid; std::vector<uint32_t>& pos;      // per variant of the uploaded selection (twk_ld_impl)
	uint64_t& n_pairs; uint64_t& n_records;                      // the object's results (twk_ld_impl)
	const std::vector<std::pair<std::string, int64_t>>& engine_options;
	Selection S;
	DeviceCtxs dc;
	twk_hip_ctx* ctx = nullptr;
	uint32_t M = 0;
	int mode = TWK_HIP_MODE_AUTO, options = 0;
	twk_hip_filters f{};
	clock::time_point t_load;
	std::ofstream file;
	std::vector<twk_hip_variant_meta>* meta = nullptr;           // set before load(): filled with the selection's per-variant metadata (`ldscore --annot`: allele counts)

	// (Impl is twk_ld::twk_ld_impl: private to twk_ld, so a struct out here cannot name it, only take it as a template's argument)
	template <class Impl>
	ReduceCommand(twk_ld_settings& settings_, Impl& impl) : settings(settings_), rid(impl.rid), pos(impl.pos), n_pairs(impl.n_pairs), n_records(impl.n_records), engine_options(impl.engine_options) {}

	// How every method begins: the caller's settings taken, the results zeroed, and the checks common to all - the input's name; the P
	// cut-off (every: why the command cannot have one, "A score sums over every record"); -c / -C (partial: why not, "Cannot prune a part
	// of the pair space: the walk needs every pair"; null: the command takes a part)
	bool begin(const twk_ld_settings& s, const char* every, const char* partial) {
		settings = s;
		n_pairs = n_records = 0;
		if (settings.in.empty()) { std::cerr << stamp("ERROR") << "No file-name provided..." << std::endl; return false; }
		if (!(settings.minP >= 1)) { std::cerr << stamp("ERROR") << every << ": a cutoff P-value below 1 is not supported (Fisher's test is not run)..." << std::endl; return false; }
		if (partial && settings.n_chunks != 1) { std::cerr << stamp("ERROR") << partial << " (no -c / -C)..." << std::endl; return false; }
		return true;
	}
	// Selection, device, upload; mode, filters and options of the engine call.  Unless `ready` the command ends: `empty` - the selection
	// holds nothing, nothing to do - is its success, `failed` an error, reported
	enum Loaded { failed, empty, ready };
	Loaded load() {
		bool nothing_to_do = false;
		if (!select_blocks(settings, S, &nothing_to_do)) return failed;
		if (nothing_to_do) return empty;
		M = S.M;
		if (!create_devices(dc, 1, engine_options)) return failed;
		ctx = dc.ctx[0];
		t_load = clock::now();
		const uint32_t T = (uint32_t)std::max(1, std::min(settings.n_threads, util::usable_cpus()));
		std::cerr << stamp("LOG", "THREAD") << "Unpacking using " << T << " threads..." << std::endl;
		if (!load_blocks(settings.in, S.reader, S.sel, T, dc.ctx, S.n_source, rid, pos, meta)) return failed;
		if (!apply_sample_selection(ctx, S.keep, M, T, meta)) return failed;
		if (settings.selects_variants()) {
			if (!apply_variant_selection(dc.ctx, settings, S.lists, S.reader.hdr, rid, pos, S.nL, S.nR, meta)) return failed;
			M = S.M = (uint32_t)rid.size();
		}
		std::cerr << stamp("LOG") << "Unpacked and uploaded " << pretty(M) << " variants. "
		          << elapsed_string(std::chrono::duration<double>(clock::now() - t_load).count()) << std::endl;
		mode = settings.force_phased ? TWK_HIP_MODE_PHASED : (settings.forced_unphased ? TWK_HIP_MODE_UNPHASED : TWK_HIP_MODE_AUTO);
		f = twk_hip_filters{settings.minR2, settings.maxR2, settings.minDprime, settings.maxDprime, settings.minP};
		options = (settings.window ? TWK_HIP_OPT_WINDOW : 0) | (ref_compat() ? TWK_HIP_OPT_REF_COMPAT : 0);
		return ready;
	}
	// The selection's pairs as the geometry of one engine call (`ldscore`, `lddecay`, `ldaggregate`): the whole triangle if the selection
	// is diagonal, else left x right.  pairs false: the selection holds no pair and the command makes no engine call
	struct Geometry { bool pairs; uint32_t a0, nA, b0, nB; int32_t triangle; };
	Geometry geometry() const {
		if (S.bal.diag) return Geometry{M > 1, 0, M, 0, M, 1};
		return Geometry{S.nL && S.nR, 0, (uint32_t)S.nL, (uint32_t)S.nL, (uint32_t)S.nR, 0};
	}
	// The one engine call, timed: -> its seconds, or a negative number after the error message.  np: where the call leaves the pairs it
	// compared, kept as the object's result (null: the call compares none)
	template <class Call>
	double call(const char* what, Call&& engine, const uint64_t* np) {
		const auto t0 = clock::now();
		if (!hip_ok(ctx, engine(), what)) return -1;
		if (np) n_pairs = *np;
		return std::chrono::duration<double>(clock::now() - t0).count();
	}
	// An output file, announced; -> false after an error message
	static bool open(std::ofstream& f, const std::string& path, std::ios::openmode mode = std::ios::out) {
		opening(path);
		f.open(path, std::ios::out | std::ios::trunc | mode);
		return opened(f.good(), path);
	}
	bool to_stdout() const { return settings.out.empty() || settings.out == "-"; }
	// The text output: -o, or stdout.  -> null after an error message
	std::ostream* open_text() {
		if (to_stdout()) return &std::cout;
		return open(file, settings.out) ? &file : nullptr;
	}
	// The `##` lines every command's text begins with (name: "ldscore", "prune", ...); the command's own lines follow
	void header(std::ostream& os, const char* name) const {
		os << "##tomahawk_" << name << "Version=" << TWK_AMD_VERSION << "\n"
		   << "##tomahawk_" << name << "Command=" << command_line() << "; Date=" << datetime() << "\n"
		   << "##mode=" << (mode == TWK_HIP_MODE_PHASED ? "phased" : mode == TWK_HIP_MODE_UNPHASED ? "unphased" : "per-pair (unphased where either variant has missing genotypes)") << "\n";
		char line[256];
		snprintf(line, sizeof(line), "##filters=minR2=%.17g,maxR2=%.17g,minDprime=%.17g,maxDprime=%.17g,minP=%.17g\n", f.minR2, f.maxR2, f.minDprime, f.maxDprime, f.minP);
		os << line << "##window=" << (settings.window ? std::to_string(settings.l_window) + " bases" : std::string("none")) << "\n";
	}
	// Contig and position of variant v as `view` prints them for a record's A side: the contig's name, a tab, the 1-based position
	void place(std::string& text, uint32_t v) const {
		if (rid[v] < S.reader.hdr.contigs.size()) text += S.reader.hdr.contigs[rid[v]].name; else text += '.';
		text += '\t'; text += std::to_string(pos[v] + 1);
	}
	// (a variant's line is complete: the text goes out a megabyte at a time)
	static void spill(std::ostream& os, std::string& text) { if (text.size() > (1u << 20)) { os << text; text.clear(); } }
	// The rest of the text; -> false after "Failed to write <what>..."
	static bool finish(std::ostream& os, std::string& text, const char* what) {
		os << text;
		os.flush();
		if (!os.good()) { std::cerr << stamp("ERROR", "WRITER") << "Failed to write " << what << "..." << std::endl; return false; }
		return true;
	}
	// A dense n x n matrix as text, a row per line: `digits` significant digits, `sep` between two values; plain_nan: every NaN is spelled
	// nan (else as printf spells it, sign included).  -> finish()
	template <class T>
	static bool dense_text(std::ostream& os, const T* m, uint32_t n, char sep, int digits, bool plain_nan) {
		std::string text;
		char num[40];
		for (uint32_t a = 0; a < n; ++a) {
			for (uint32_t b = 0; b < n; ++b) {
				const double v = (double)m[(size_t)a * n + b];
				if (b) text += sep;
				if (plain_nan && v != v) text += "nan";
				else { snprintf(num, sizeof(num), "%.*g", digits, v); text += num; }
			}
			text += '\n';
			spill(os, text);
		}
		return finish(os, text, "the matrix");
	}
	// An array as a NumPy file, format 1.0: magic, version, a little-endian uint16 header length, the dictionary padded with
	// spaces and ended by a newline so that the data begins on a multiple of 64 bytes; C order (the hosts this runs on are little-endian).
	// descr: "<f4", "<f8", "<i4", "<i8".  rows x cols: a dense matrix, shape (rows, cols); cols == 0: a 1-D array, shape (rows,).
	// -> finish()
	static bool npy(std::ostream& os, const char* descr, uint64_t rows, uint64_t cols, const void* data, size_t bytes) {
		std::string dict = std::string("{'descr': '") + descr + "', 'fortran_order': False, 'shape': (" + std::to_string(rows) + "," + (cols ? " " + std::to_string(cols) : std::string()) + "), }";
		const size_t fixed = 6 + 2 + 2;
		const size_t total = (fixed + dict.size() + 1 + 63) / 64 * 64;
		dict.append(total - fixed - dict.size() - 1, ' ');
		dict += '\n';
		const char head[fixed] = {'\x93', 'N', 'U', 'M', 'P', 'Y', 1, 0, (char)(dict.size() & 0xFF), (char)(dict.size() >> 8 & 0xFF)};
		os.write(head, fixed);
		os.write(dict.data(), (std::streamsize)dict.size());
		os.write(static_cast<const char*>(data), (std::streamsize)bytes);
		std::string nothing;
		return finish(os, nothing, "the matrix");
	}
	// The band writer: 1-D arrays as NumPy files PREFIX<suffix>, and the rows' variants as PREFIX.variants.tsv ("contig <TAB> pos").
	struct NpyArray { const char* suffix; const char* descr; uint64_t items; const void* data; size_t bytes; };
	bool npy_files(const std::string& prefix, std::initializer_list<NpyArray> arrays) {
		std::ofstream out;
		for (const NpyArray& a : arrays) {
			if (!open(out, prefix + a.suffix, std::ios::binary)) return false;
			if (!npy(out, a.descr, a.items, 0, a.data, a.bytes)) return false;
			out.close();
		}
		return true;
	}
	bool variant_list(const std::string& prefix) {
		std::ofstream vfile;
		if (!open(vfile, prefix + ".variants.tsv")) return false;
		std::string text;
		for (uint32_t v = 0; v < M; ++v) {
			place(text, v);
			text += '\n';
			spill(vfile, text);
		}
		return finish(vfile, text, "the variant list");
	}
	void all_done() const {
		std::cerr << stamp("LOG", "PROGRESS") << "All done..." << elapsed_string(std::chrono::duration<double>(clock::now() - t_load).count()) << "!" << std::endl;
	}
};
}  // namespace

// `tomahawk ldscore`: per variant of the selection the number of records Compute would write with the variant at either end and the
// sum of their R2 (twk_hip_ld_score: reduced on the GPU, no record is formed), as text.  The input is loaded exactly as Compute loads
// it; one GPU.  Not in the reference.
bool twk_ld::Score(const twk_ld_settings& s) { return Score(s, twk_score_settings()); }

// The annotation file of `tomahawk ldscore --annot` (include/twk_ld.h): the categories' names and (contig name, 1-based position) -> a row of
// numbers.  -> false after an error message with file and line: unreadable, no header, no or too many columns, a name twice, a row of
// another length, a position or a number that is none, not finite or beyond 65536 in magnitude, the same key twice.
namespace {
struct AnnotFile {
	std::vector<std::string> names;
	std::map<std::pair<std::string, uint64_t>, size_t> row;      // -> the row's first number in `values`
	std::vector<double> values;
	std::vector<bool> used;
};
bool read_annot(const std::string& path, AnnotFile& out) {
	std::ifstream in(path);
	if (!in.good()) { std::cerr << stamp("ERROR") << "Failed to open the annotation file: " << path << "..." << std::endl; return false; }
	std::string text;
	size_t skip = 0, C = 0;               // the SNP and CM columns of an LDSC .annot; the categories
	bool have_header = false;
	for (uint64_t n_line = 1; std::getline(in, text); ++n_line) {
		if (!text.empty() && text.back() == '\r') text.pop_back();
		if (text.compare(0, 2, "##") == 0) continue;
		std::vector<std::string> col;
		for (size_t at = 0; at < text.size();) {
			const size_t from = text.find_first_not_of(" \t", at);
			if (from == std::string::npos) break;
			const size_t to = text.find_first_of(" \t", from);
			col.push_back(text.substr(from, to == std::string::npos ? std::string::npos : to - from));
			at = to == std::string::npos ? text.size() : to;
		}
		if (col.empty()) continue;
		const auto bad = [&]() -> std::ostream& { return std::cerr << stamp("ERROR") << path << ":" << n_line << ": "; };
		if (!have_header) {
			have_header = true;
			if (col[0] == "#" && col.size() > 1) col.erase(col.begin());      // ("# contig pos ...")
			if (col.size() >= 4 && col[2] == "SNP" && col[3] == "CM") skip = 2;
			if (col.size() < 2 + skip + 1 || col.size() - 2 - skip > TWK_HIP_ANNOT_MAX_CATEGORIES) {
				bad() << "the number of annotation columns must be between 1 and " << TWK_HIP_ANNOT_MAX_CATEGORIES << ", not " << (col.size() < 2 + skip ? 0 : col.size() - 2 - skip) << "..." << std::endl;
				return false;
			}
			out.names.assign(col.begin() + 2 + skip, col.end());
			C = out.names.size();
			std::set<std::string> seen;
			for (const std::string& name : out.names)
				if (!seen.insert(name).second) { bad() << "the annotation " << name << " is named twice..." << std::endl; return false; }
			continue;
		}
		if (col.size() != 2 + skip + C) { bad() << "expected " << 2 + skip + C << " columns, found " << col.size() << "..." << std::endl; return false; }
		char* end = nullptr;
		const unsigned long long pos = strtoull(col[1].c_str(), &end, 10);
		if (*end || col[1][0] == '-' || pos == 0) { bad() << "not a 1-based position: " << col[1] << std::endl; return false; }
		if (!out.row.emplace(std::make_pair(col[0], (uint64_t)pos), out.values.size()).second) { bad() << col[0] << ":" << pos << " is named twice..." << std::endl; return false; }
		for (size_t k = 0; k < C; ++k) {
			const std::string& word = col[2 + skip + k];
			const double a = strtod(word.c_str(), &end);
			if (end == word.c_str() || *end || !(a >= -TWK_HIP_ANNOT_MAX_ABS && a <= TWK_HIP_ANNOT_MAX_ABS)) {
				bad() << "not a finite annotation of at most " << (long long)TWK_HIP_ANNOT_MAX_ABS << " in magnitude: " << word << std::endl;
				return false;
			}
			out.values.push_back(a);
		}
	}
	if (!have_header) { std::cerr << stamp("ERROR") << path << ": no header line (contig pos name1 ...)..." << std::endl; return false; }
	out.used.assign(out.row.size(), false);
	return true;
}
}  // namespace

// ... and with ss.annot partitioned LD scores (twk_hip_ld_score_annot): per variant and annotation column the sum over the variant's
// partners of annotation * R2, summed exactly on the GPU.  The annotation file is read and checked before the input is opened or a
// device touched, as Clump reads its association file.
bool twk_ld::Score(const twk_ld_settings& s, const twk_score_settings& ss) {
	ReduceCommand cmd(settings, *mImpl);
	if (!cmd.begin(s, "A score sums over every record", nullptr)) return false;
	const bool annotated = !ss.annot.empty();
	if (ss.top < 0 || ss.top > TWK_HIP_TOPK_MAX) { std::cerr << stamp("ERROR") << "The number of partners to list (--top) must be between 1 and " << TWK_HIP_TOPK_MAX << "..." << std::endl; return false; }
	const int32_t top_stat = ss.top_stat < 0 ? (int32_t)TWK_HIP_STAT_R2 : ss.top_stat;
	if (ss.top > 0 && (annotated || !LD_STATS.valid(top_stat))) { std::cerr << stamp("ERROR") << "--top lists partners by one of " << LD_STATS.list() << " and takes no annotation file..." << std::endl; return false; }
	if (ss.self && !annotated) { std::cerr << stamp("ERROR") << "--self adds a variant's own annotation to its partitioned scores: it needs an annotation file (--annot)..." << std::endl; return false; }
	AnnotFile af;
	std::vector<twk_hip_variant_meta> meta;
	if (annotated) {
		if (!read_annot(ss.annot, af)) return false;
		cmd.meta = &meta;
	}
	if (const auto l = cmd.load(); l != cmd.ready) return l == cmd.empty;
	const uint32_t M = cmd.M;
	if (annotated) {
		const size_t C = af.names.size();
		// every variant of the selection at a (contig, position) the file names gets that row; the others zeros
		const auto& contigs = cmd.S.reader.hdr.contigs;
		std::vector<double> annot((size_t)M * C, 0.0);
		uint64_t n_named = 0;
		for (uint32_t v = 0; v < M; ++v) {
			const uint32_t rid = mImpl->rid[v];
			if (rid >= contigs.size()) continue;
			const auto it = af.row.find(std::make_pair(contigs[rid].name, (uint64_t)mImpl->pos[v] + 1));
			if (it == af.row.end()) continue;
			af.used[it->second / C] = true;
			std::copy(af.values.begin() + it->second, af.values.begin() + it->second + C, annot.begin() + (size_t)v * C);
			++n_named;
		}
		const uint64_t n_unmatched = (uint64_t)std::count(af.used.begin(), af.used.end(), false);
		std::cerr << stamp("LOG") << "Annotation file: " << pretty(C) << " categories, " << pretty(af.row.size()) << " rows, " << pretty(n_unmatched) << " name no selected variant; "
		          << pretty(n_named) << " of " << pretty(M) << " variants are annotated." << std::endl;
		// the regression's M and M_5_50: the categories' sums over the selection, and over its variants with a minor allele frequency above 0.05
		std::vector<double> sum_all(C, 0.0), sum_common(C, 0.0);
		for (uint32_t v = 0; v < M; ++v) {
			const int64_t called = 2 * (int64_t)cmd.S.n_samples - (int64_t)meta[v].an, ac = meta[v].ac;
			const bool common = called > 0 && (double)std::min(ac, called - ac) / (double)called > 0.05;
			for (size_t k = 0; k < C; ++k) {
				sum_all[k] += annot[(size_t)v * C + k];
				if (common) sum_common[k] += annot[(size_t)v * C + k];
			}
		}
		std::vector<uint64_t> n_partners(M, 0);
		std::vector<double> score((size_t)M * C, 0.0);
		uint64_t np = 0;
		const auto g = cmd.geometry();
		const double sec = cmd.call("twk_hip_ld_score_annot", [&] {
			return !g.pairs ? TWK_HIP_OK : twk_hip_ld_score_annot(cmd.ctx, cmd.mode, &cmd.f, g.a0, g.nA, g.b0, g.nB, g.triangle, 0, 1, 0, cmd.options, (uint32_t)settings.l_window,
			                                                       annot.data(), (uint32_t)C, C, n_partners.data(), score.data(), &np);
		}, &np);
		if (sec < 0) return false;
		if (ss.self) for (size_t k = 0; k < score.size(); ++k) score[k] += annot[k];      // (LDSC's convention: r2(v, v) = 1)

		std::ostream* const os = cmd.open_text();
		if (!os) return false;
		cmd.header(*os, "ldscore");
		std::string text = "##annotations=" + std::to_string(C) + "\n";
		char num[64];
		for (const auto* sums : {&sum_all, &sum_common}) {
			text += sums == &sum_all ? "##M=" : "##M_5_50=";
			for (size_t k = 0; k < C; ++k) { snprintf(num, sizeof(num), k ? ",%.17g" : "%.17g", (*sums)[k]); text += num; }
			text += '\n';
		}
		if (ss.self) text += "##self=1\n";
		text += "#contig\tpos\tn_partners";
		for (const std::string& name : af.names) { text += '\t'; text += name; }
		text += '\n';
		for (uint32_t v = 0; v < M; ++v) {
			cmd.place(text, v);
			snprintf(num, sizeof(num), "\t%llu", (unsigned long long)n_partners[v]); text += num;
			for (size_t k = 0; k < C; ++k) { snprintf(num, sizeof(num), "\t%.17g", score[(size_t)v * C + k]); text += num; }
			text += '\n';
			cmd.spill(*os, text);
		}
		if (!cmd.finish(*os, text, "the scores")) return false;
		std::cerr << stamp("LOG") << "Scored " << pretty(M) << " variants in " << pretty(C) << " categories over " << pretty(np) << " variant comparisons. " << elapsed_string(sec) << std::endl;
		cmd.all_done();
		return true;
	}
	if (ss.top > 0) {
		// the k strongest partners of every variant (twk_hip_ld_topk): selected on the GPU, one line per variant and rank
		const uint32_t K = (uint32_t)ss.top;
		std::vector<uint32_t> idx((size_t)M * K, TWK_HIP_NO_PARTNER);
		std::vector<float> val((size_t)M * K, 0.0f);
		uint64_t np = 0;
		const auto g = cmd.geometry();
		const double sec = cmd.call("twk_hip_ld_topk", [&] {
			return !g.pairs ? TWK_HIP_OK : twk_hip_ld_topk(cmd.ctx, cmd.mode, &cmd.f, g.a0, g.nA, g.b0, g.nB, g.triangle, 0, 1, 0, cmd.options, (uint32_t)settings.l_window,
			                                                top_stat, K, idx.data(), val.data(), &np);
		}, &np);
		if (sec < 0) return false;
		std::ostream* const os = cmd.open_text();
		if (!os) return false;
		cmd.header(*os, "ldscore");
		std::string text = "##top=" + std::to_string(K) + "\n##stat=" + LD_STATS.name(top_stat) + "\n";
		if (settings.n_chunks != 1)
			text += "##shard=" + std::to_string(settings.c_chunk + 1) + "/" + std::to_string(settings.n_chunks) + ": the lists hold the partners among this part's pairs only; the parts' lists merge into the whole's\n";
		text += "#contig\tpos\trank\tpartner_contig\tpartner_pos\tvalue\n";
		char num[64];
		uint64_t n_listed = 0;
		for (uint32_t v = 0; v < M; ++v)
			for (uint32_t r = 0; r < K && idx[(size_t)v * K + r] != TWK_HIP_NO_PARTNER; ++r, ++n_listed) {
				cmd.place(text, v);
				snprintf(num, sizeof(num), "\t%u\t", r + 1); text += num;
				cmd.place(text, idx[(size_t)v * K + r]);
				snprintf(num, sizeof(num), "\t%.9g\n", (double)val[(size_t)v * K + r]); text += num;
				cmd.spill(*os, text);
			}
		if (!cmd.finish(*os, text, "the partner lists")) return false;
		std::cerr << stamp("LOG") << "Listed " << pretty(n_listed) << " partners of " << pretty(M) << " variants over " << pretty(np) << " variant comparisons. " << elapsed_string(sec) << std::endl;
		cmd.all_done();
		return true;
	}
	std::vector<uint64_t> n_partners(M, 0);
	std::vector<double> sum_r2(M, 0.0);
	uint64_t np = 0;
	const auto g = cmd.geometry();
	const double sec = cmd.call("twk_hip_ld_score", [&] {
		return !g.pairs ? TWK_HIP_OK : twk_hip_ld_score(cmd.ctx, cmd.mode, &cmd.f, g.a0, g.nA, g.b0, g.nB, g.triangle, 0, 1, 0, cmd.options, (uint32_t)settings.l_window, n_partners.data(), sum_r2.data(), &np);
	}, &np);
	if (sec < 0) return false;

	std::ostream* const os = cmd.open_text();
	if (!os) return false;
	cmd.header(*os, "ldscore");
	*os << "#contig\tpos\tn_partners\tsum_r2\n";
	std::string text;
	char line[256];
	for (uint32_t v = 0; v < M; ++v) {
		cmd.place(text, v);
		snprintf(line, sizeof(line), "\t%llu\t%.17g\n", (unsigned long long)n_partners[v], sum_r2[v]);
		text += line;
		cmd.spill(*os, text);
	}
	if (!cmd.finish(*os, text, "the scores")) return false;
	std::cerr << stamp("LOG") << "Scored " << pretty(M) << " variants over " << pretty(np) << " variant comparisons. " << elapsed_string(sec) << std::endl;
	cmd.all_done();
	return true;
}

// `tomahawk lddecay`: r2 by the distance between two variants, over the records Compute would write (twk_hip_ld_decay: binned and summed
// exactly on the GPU, no record is formed), as text: one line per bin.  The input is loaded exactly as Compute loads it; one GPU.  The
// reference's two_reader::Decay bins the records of a .two file; its columns are kept and `Sum` is added.
bool twk_ld::Decay(const twk_ld_settings& s, const twk_decay_settings& ds) {
	ReduceCommand cmd(settings, *mImpl);
	if (!cmd.begin(s, "A decay curve averages over every record", nullptr)) return false;
	if (ds.n_bins < 1 || ds.n_bins > MAX_BINS) { std::cerr << stamp("ERROR") << "The number of bins must be between 1 and " << MAX_BINS << "..." << std::endl; return false; }
	if (ds.range_bp < ds.n_bins || ds.range_bp > MAX_RANGE_BP) { std::cerr << stamp("ERROR") << "The range in bases must be at least the number of bins and below 2^32..." << std::endl; return false; }
	if (const auto l = cmd.load(); l != cmd.ready) return l == cmd.empty;
	const uint32_t B = (uint32_t)ds.n_bins, range = (uint32_t)ds.range_bp;
	std::vector<uint64_t> n(B, 0);
	std::vector<double> sum_r2(B, 0.0);
	uint64_t np = 0;
	const auto g = cmd.geometry();
	const double sec = cmd.call("twk_hip_ld_decay", [&] {
		return !g.pairs ? TWK_HIP_OK : twk_hip_ld_decay(cmd.ctx, cmd.mode, &cmd.f, g.a0, g.nA, g.b0, g.nB, g.triangle, 0, 1, 0, cmd.options, (uint32_t)settings.l_window, range, B, n.data(), sum_r2.data(), &np);
	}, &np);
	if (sec < 0) return false;

	std::ostream* const os = cmd.open_text();
	if (!os) return false;
	cmd.header(*os, "lddecay");
	const uint32_t width = range / B;
	uint64_t counted = 0;
	for (uint32_t b = 0; b < B; ++b) counted += n[b];
	*os << "##range=" << range << ",bins=" << B << ",width=" << width << ",pairs=" << counted << "\n"
	    << "From\tTo\tMean\tFrequency\tSum\n";
	std::string text;
	char line[256];
	for (uint32_t b = 0; b < B; ++b) {
		snprintf(line, sizeof(line), "%llu\t%llu\t%.17g\t%llu\t%.17g\n", (unsigned long long)b * width, (unsigned long long)(b + 1) * width,
		         n[b] ? sum_r2[b] / (double)n[b] : 0.0, (unsigned long long)n[b], sum_r2[b]);
		text += line;
		cmd.spill(*os, text);
	}
	if (!cmd.finish(*os, text, "the decay table")) return false;
	std::cerr << stamp("LOG") << "Binned " << pretty(counted) << " records of " << pretty(np) << " variant comparisons into " << pretty(B) << " bins. " << elapsed_string(sec) << std::endl;
	cmd.all_done();
	return true;
}

// `tomahawk ldaggregate`: the statistic of every record Compute would write, rasterised into x-by-y cells of the landscape the loaded
// variants span (twk_hip_ld_aggregate: binned and summed exactly on the GPU, no record is formed), as text: one line per x bin.  The
// input is loaded exactly as Compute loads it; one GPU.  The reference's two_reader::Aggregate rasterises the records of a .two file
// into a binary .twa; its coordinate rule is kept (twk_aggregate_landscape.h), its file format is not provided.
bool twk_ld::Aggregate(const twk_ld_settings& s, const twk_aggregate_settings& as) {
	ReduceCommand cmd(settings, *mImpl);
	if (!cmd.begin(s, "An aggregate takes in every record", nullptr)) return false;
	if (as.x_bins < 1 || as.x_bins > MAX_BINS || as.y_bins < 1 || as.y_bins > MAX_BINS) { std::cerr << stamp("ERROR") << "The number of bins per axis must be between 1 and " << MAX_BINS << "..." << std::endl; return false; }
	if (!LD_STATS.valid(as.stat)) { std::cerr << stamp("ERROR") << "Unknown statistic..." << std::endl; return false; }
	if (!AGGREGATE_REDUCTIONS.valid(as.reduce) || as.min_count < 0) { std::cerr << stamp("ERROR") << "Unknown reduction or a negative minimum count..." << std::endl; return false; }
	if (const auto l = cmd.load(); l != cmd.ready) return l == cmd.empty;
	const Selection& S = cmd.S;
	const uint32_t M = cmd.M, X = (uint32_t)as.x_bins, Y = (uint32_t)as.y_bins;
	std::vector<int64_t> contig_bases;
	for (const auto& ctg : S.reader.hdr.contigs) contig_bases.push_back(ctg.n_bases);
	twk_aggregate_landscape land;
	std::vector<uint16_t> bin_x, bin_y;
	if (!agl_build(mImpl->rid.data(), mImpl->pos.data(), M, contig_bases, X, Y, land, bin_x, bin_y)) {
		std::cerr << stamp("ERROR") << "Cannot lay out the landscape: a variant on a contig the header does not have, or a range of 0 or of 2^32 bases and more..." << std::endl;
		return false;
	}
	const size_t cells = (size_t)X * Y;
	std::vector<uint64_t> n(cells, 0);
	std::vector<double> sum(cells, 0.0), sum_sq(cells, 0.0), mn(cells, 0.0), mx(cells, 0.0);
	uint64_t np = 0;
	const auto g = cmd.geometry();
	const double sec = cmd.call("twk_hip_ld_aggregate", [&] {
		return !g.pairs ? TWK_HIP_OK : twk_hip_ld_aggregate(cmd.ctx, cmd.mode, &cmd.f, g.a0, g.nA, g.b0, g.nB, g.triangle, 0, 1, 0, cmd.options, (uint32_t)settings.l_window, as.stat, bin_x.data(), bin_y.data(), X, Y, n.data(), sum.data(), sum_sq.data(), mn.data(), mx.data(), &np);
	}, &np);
	if (sec < 0) return false;

	std::ostream* const os = cmd.open_text();
	if (!os) return false;
	cmd.header(*os, "ldaggregate");
	uint64_t contributions = 0;
	for (size_t k = 0; k < cells; ++k) contributions += n[k];
	*os << "#x=" << X << ",y=" << Y << ",bpx=" << land.bpx << ",bpy=" << land.bpy << ",range=" << land.range
	    << ",stat=" << LD_STATS.name(as.stat) << ",reduce=" << AGGREGATE_REDUCTIONS.name(as.reduce) << ",min_count=" << as.min_count << ",contributions=" << contributions << "\n";
	if (land.single) *os << "#landscape=one contig,min_pos=" << land.min_pos << "\n";
	else *os << "#landscape=whole contigs\n";
	for (size_t k = 0; k < contig_bases.size(); ++k)
		if (land.present[k]) *os << "#contig=" << S.reader.hdr.contigs[k].name << ",rid=" << k << ",offset=" << (land.single ? 0 : land.offset[k]) << "\n";
	std::string text;
	char cell[64];
	for (uint32_t x = 0; x < X; ++x) {
		for (uint32_t y = 0; y < Y; ++y) {
			const size_t k = (size_t)x * Y + y;
			double v = 0.0;
			if (n[k] && n[k] >= (uint64_t)as.min_count) {
				const double cnt = (double)n[k], mean = sum[k] / cnt;
				switch (as.reduce) {
				case TWK_AGGREGATE_MEAN: v = mean; break;
				case TWK_AGGREGATE_COUNT: v = cnt; break;
				case TWK_AGGREGATE_MIN: v = mn[k]; break;
				case TWK_AGGREGATE_MAX: v = mx[k]; break;
				case TWK_AGGREGATE_SD: { const double var = sum_sq[k] / cnt - mean * mean; v = var > 0 ? sqrt(var) : 0.0; break; }
				default: v = sum[k]; break;      // TWK_AGGREGATE_TOTAL
				}
			}
			snprintf(cell, sizeof(cell), y ? "\t%.17g" : "%.17g", v);
			text += cell;
		}
		text += '\n';
		cmd.spill(*os, text);
	}
	if (!cmd.finish(*os, text, "the aggregate")) return false;
	std::cerr << stamp("LOG") << "Aggregated " << pretty(contributions) << " contributions of " << pretty(np) << " variant comparisons into " << pretty(cells) << " cells. " << elapsed_string(sec) << std::endl;
	cmd.all_done();
	return true;
}

// `tomahawk prune`: greedy LD pruning of the selection in file order (twk_hip_ld_prune: the edges are the records Compute would write,
// decided and walked on the GPU, no record is formed), as text: one line per variant with its keep flag.  The input is loaded exactly
// as Compute loads it; one GPU; the whole triangle (the walk needs every pair: no -c / -C).  Not in the reference.
bool twk_ld::Prune(const twk_ld_settings& s) { return Prune(s, twk_prune_settings()); }
bool twk_ld::Prune(const twk_ld_settings& s, const twk_prune_settings& ps) {
	ReduceCommand cmd(settings, *mImpl);
	if (!cmd.begin(s, "Pruning looks at every record", "Cannot prune a part of the pair space: the walk needs every pair")) return false;
	if (const auto l = cmd.load(); l != cmd.ready) return l == cmd.empty;
	const uint32_t M = cmd.M;
	std::vector<uint8_t> keep(M, 0);
	uint64_t np = 0, n_kept = 0, n_edges = 0;
	const double sec = cmd.call("twk_hip_ld_prune", [&] { return twk_hip_ld_prune(cmd.ctx, cmd.mode, &cmd.f, 0, M, 0, cmd.options, (uint32_t)settings.l_window, keep.data(), &n_kept, &n_edges, &np); }, &np);
	if (sec < 0) return false;

	std::ostream* const os = cmd.open_text();
	if (!os) return false;
	cmd.header(*os, "prune");
	char line[256];
	snprintf(line, sizeof(line), "##kept=%llu,total=%u,edges=%llu\n", (unsigned long long)n_kept, M, (unsigned long long)n_edges);
	*os << line << "#contig\tpos\tkeep\n";
	std::string text;
	for (uint32_t v = 0; v < M; ++v) {
		if (ps.kept_only && !keep[v]) continue;
		cmd.place(text, v);
		text += keep[v] ? "\t1\n" : "\t0\n";
		cmd.spill(*os, text);
	}
	if (!cmd.finish(*os, text, "the keep flags")) return false;
	std::cerr << stamp("LOG") << "Pruned: kept " << pretty(n_kept) << " of " << pretty(M) << " variants; " << pretty(n_edges) << " pairs in LD among "
	          << pretty(np) << " variant comparisons. " << elapsed_string(sec) << std::endl;
	cmd.all_done();
	return true;
}

// The association file of `tomahawk clump` (include/twk_ld.h): (contig name, 1-based position) -> P, NaN for "no P value".  -> false
// after an error message: unreadable, a malformed line, a P outside [0, 1], the same key twice.
namespace {
struct AssocEntry { double p; bool used; };
using AssocMap = std::map<std::pair<std::string, uint64_t>, AssocEntry>;
bool read_assoc(const std::string& path, AssocMap& out) {
	std::ifstream in(path);
	if (!in.good()) { std::cerr << stamp("ERROR") << "Failed to open the association file: " << path << "..." << std::endl; return false; }
	std::string text;
	for (uint64_t n_line = 1; std::getline(in, text); ++n_line) {
		if (!text.empty() && text.back() == '\r') text.pop_back();
		if (text.empty() || text[0] == '#') continue;
		std::vector<std::string> col;
		for (size_t at = 0; at < text.size() && col.size() < 3;) {
			const size_t from = text.find_first_not_of(" \t", at);
			if (from == std::string::npos) break;
			const size_t to = text.find_first_of(" \t", from);
			col.push_back(text.substr(from, to == std::string::npos ? std::string::npos : to - from));
			at = to == std::string::npos ? text.size() : to;
		}
		if (col.empty()) continue;
		if (col.size() < 3) { std::cerr << stamp("ERROR") << path << ":" << n_line << ": expected contig, position and P..." << std::endl; return false; }
		char* end = nullptr;
		const unsigned long long pos = strtoull(col[1].c_str(), &end, 10);
		if (col[1].empty() || *end || col[1][0] == '-' || pos == 0) { std::cerr << stamp("ERROR") << path << ":" << n_line << ": not a 1-based position: " << col[1] << std::endl; return false; }
		std::string low = col[2];
		for (char& ch : low) ch = (char)tolower((unsigned char)ch);
		double pv = std::numeric_limits<double>::quiet_NaN();
		if (low != "na" && low != "nan" && low != ".") {
			pv = strtod(col[2].c_str(), &end);
			if (*end || !(pv >= 0.0 && pv <= 1.0)) { std::cerr << stamp("ERROR") << path << ":" << n_line << ": not a P value in [0, 1]: " << col[2] << std::endl; return false; }
		}
		if (!out.emplace(std::make_pair(col[0], (uint64_t)pos), AssocEntry{pv, false}).second) {
			std::cerr << stamp("ERROR") << path << ":" << n_line << ": " << col[0] << ":" << pos << " is named twice..." << std::endl; return false;
		}
	}
	return true;
}
}  // namespace

// `tomahawk clump`: LD clumping of the selection (twk_hip_ld_clump: the edges are the records Compute would write, seen from both ends,
// decided on the GPU and walked there in P order, no record is formed), as text: one line per variant with its index variant.  The
// association file is read and checked before the input is opened or a device touched; the input is then loaded exactly as Prune
// loads it; one GPU; the whole triangle (no -c / -C).  Not in the reference.
bool twk_ld::Clump(const twk_ld_settings& s, const twk_clump_settings& cs) {
	ReduceCommand cmd(settings, *mImpl);
	if (!cmd.begin(s, "Clumping looks at every record", "Cannot clump a part of the pair space: the walk needs every pair")) return false;
	if (!(cs.p1 >= 0 && cs.p1 <= cs.p2 && cs.p2 <= 1)) { std::cerr << stamp("ERROR") << "The clumping thresholds must satisfy 0 <= p1 <= p2 <= 1..." << std::endl; return false; }
	if (cs.assoc.empty()) { std::cerr << stamp("ERROR") << "No association file provided..." << std::endl; return false; }
	AssocMap assoc;
	if (!read_assoc(cs.assoc, assoc)) return false;
	if (const auto l = cmd.load(); l != cmd.ready) return l == cmd.empty;
	const uint32_t M = cmd.M;

	// every variant of the selection at a (contig, position) the file names gets that P
	const auto& contigs = cmd.S.reader.hdr.contigs;
	std::vector<double> p(M, std::numeric_limits<double>::quiet_NaN());
	uint64_t n_with_p = 0;
	for (uint32_t v = 0; v < M; ++v) {
		const uint32_t rid = mImpl->rid[v];
		if (rid >= contigs.size()) continue;
		const auto it = assoc.find(std::make_pair(contigs[rid].name, (uint64_t)mImpl->pos[v] + 1));
		if (it == assoc.end()) continue;
		it->second.used = true;
		p[v] = it->second.p;
		if (p[v] == p[v]) ++n_with_p;
	}
	uint64_t n_unmatched = 0;
	for (const auto& kv : assoc) if (!kv.second.used) ++n_unmatched;
	std::cerr << stamp("LOG") << "Association file: " << pretty(assoc.size()) << " lines, " << pretty(n_unmatched) << " name no selected variant; "
	          << pretty(n_with_p) << " of " << pretty(M) << " variants have a P value." << std::endl;

	std::vector<uint32_t> index_of(M, TWK_HIP_NO_CLUMP);
	uint64_t np = 0, n_clumps = 0, n_members = 0, n_edges = 0;
	const double sec = cmd.call("twk_hip_ld_clump", [&] {
		return twk_hip_ld_clump(cmd.ctx, cmd.mode, &cmd.f, 0, M, 0, cmd.options, (uint32_t)settings.l_window, p.data(), cs.p1, cs.p2, index_of.data(), &n_clumps, &n_members, &n_edges, &np);
	}, &np);
	if (sec < 0) return false;

	std::ostream* const os = cmd.open_text();
	if (!os) return false;
	cmd.header(*os, "clump");
	char line[256];
	snprintf(line, sizeof(line), "##thresholds=p1=%.17g,p2=%.17g\n", cs.p1, cs.p2);
	*os << line;
	snprintf(line, sizeof(line), "##clumps=%llu,members=%llu,total=%u,edges=%llu\n", (unsigned long long)n_clumps, (unsigned long long)n_members, M, (unsigned long long)n_edges);
	*os << line << "#contig\tpos\tP\tindex_contig\tindex_pos\n";
	std::string text;
	for (uint32_t v = 0; v < M; ++v) {
		cmd.place(text, v);
		if (p[v] == p[v]) { snprintf(line, sizeof(line), "\t%.17g\t", p[v]); text += line; }
		else text += "\tNA\t";
		const uint32_t ix = index_of[v];
		if (ix < M) { cmd.place(text, ix); text += '\n'; }
		else text += ".\t.\n";
		cmd.spill(*os, text);
	}
	if (!cmd.finish(*os, text, "the clumps")) return false;
	std::cerr << stamp("LOG") << "Clumped: " << pretty(n_clumps) << " index variants claimed " << pretty(n_members) << " of " << pretty(M) << " variants; " << pretty(n_edges)
	          << " pairs in LD among " << pretty(np) << " variant comparisons. " << elapsed_string(sec) << std::endl;
	cmd.all_done();
	return true;
}

// `tomahawk ldmatrix`: the dense LD matrix of the selection (twk_hip_ld_matrix: one statistic of every record Compute would write, stored
// on the GPU at (u, v) and (v, u), no record is formed), as a NumPy file or as text, with the rows' variants next to it.  The input is
// loaded exactly as Prune loads it; one GPU; the whole triangle (no -c / -C).  Not in the reference.
bool twk_ld::Matrix(const twk_ld_settings& s, const twk_matrix_settings& ms) {
	ReduceCommand cmd(settings, *mImpl);
	if (!cmd.begin(s, "The matrix holds every record", "Cannot fill a part of the pair space: the matrix needs every pair")) return false;
	if (!LD_STATS.valid(ms.stat)) { std::cerr << stamp("ERROR") << "Unknown statistic: one of " << LD_STATS.list() << "..." << std::endl; return false; }
	if (cmd.to_stdout()) { std::cerr << stamp("ERROR") << "No output prefix provided: the matrix and its variant list are files..." << std::endl; return false; }
	if (ms.band && !settings.window) { std::cerr << stamp("ERROR") << "A banded matrix stores the columns inside the window: it needs one (-w)..." << std::endl; return false; }
	if (ms.band && ms.text) { std::cerr << stamp("ERROR") << "A banded matrix has no text form..." << std::endl; return false; }
	if (const auto l = cmd.load(); l != cmd.ready) return l == cmd.empty;
	const uint32_t M = cmd.M;
	uint64_t np = 0, n_recs = 0, nnz = 0;
	double sec = 0;
	std::ofstream file;
	if (ms.band) {
		// the band: its layout first, which sizes the values; then the three arrays of a CSR matrix, each a NumPy file
		if (M > 0x7FFFFFFFu) { std::cerr << stamp("ERROR") << "Too many variants for PREFIX.first.npy (int32)..." << std::endl; return false; }
		std::vector<uint32_t> first(M);
		std::vector<uint64_t> indptr((size_t)M + 1);
		if (!hip_ok(cmd.ctx, twk_hip_bandmat_layout(cmd.ctx, 0, M, (uint32_t)settings.l_window, first.data(), indptr.data()), "twk_hip_bandmat_layout")) return false;
		nnz = indptr[M];
		std::vector<float> values((size_t)nnz);
		sec = cmd.call("twk_hip_ld_matrix_band", [&] {
			return twk_hip_ld_matrix_band(cmd.ctx, cmd.mode, &cmd.f, 0, M, 0, cmd.options, (uint32_t)settings.l_window, ms.stat, ms.fill, values.data(), nnz, first.data(), indptr.data(), &n_recs, &np);
		}, &np);
		if (sec < 0) return false;
		if (!cmd.npy_files(settings.out, {
			{".values.npy", "<f4", nnz, values.data(), values.size() * sizeof(float)},
			{".indptr.npy", "<i8", (uint64_t)M + 1, indptr.data(), indptr.size() * sizeof(uint64_t)},      // (below 2^63: the same bits)
			{".first.npy", "<i4", M, first.data(), first.size() * sizeof(uint32_t)}})) return false;        // (below 2^31)
	} else {
		std::vector<float> m((size_t)M * M);
		sec = cmd.call("twk_hip_ld_matrix", [&] { return twk_hip_ld_matrix(cmd.ctx, cmd.mode, &cmd.f, 0, M, 0, cmd.options, (uint32_t)settings.l_window, ms.stat, ms.fill, m.data(), M, &n_recs, &np); }, &np);
		if (sec < 0) return false;
		if (!cmd.open(file, settings.out + (ms.text ? ".ld" : ".npy"), std::ios::binary)) return false;
		if (!(ms.text ? cmd.dense_text(file, m.data(), M, ' ', 9, false) : cmd.npy(file, "<f4", M, M, m.data(), m.size() * sizeof(float)))) return false;
		file.close();
	}
	mImpl->n_records = n_recs;
	if (!cmd.variant_list(settings.out)) return false;
	std::cerr << stamp("LOG") << "Matrix of " << LD_STATS.name(ms.stat) << ": " << pretty(M) << " x " << pretty(M) << (ms.band ? ", a band of " + pretty(nnz) + " entries" : std::string()) << ", " << pretty(n_recs) << " pairs with a value among "
	          << pretty(np) << " variant comparisons. " << elapsed_string(sec) << std::endl;
	cmd.all_done();
	return true;
}

// `tomahawk blocks`: haplotype blocks of the selection by the rule of Gabriel et al. (twk_hip_ld_blocks: the D' confidence bounds of the
// records Compute would write, in band storage, and the blocks selected from them, all on the GPU), as text: one line per block.  With
// bs.ci_out the bounds themselves are written through the band writer (twk_hip_ld_dprime_ci_band: a second engine call with the same
// arguments, the same bytes).  The input is loaded exactly as Prune loads it; one GPU; the whole triangle (no -c / -C); the window is
// always on.  Not in the reference.
bool twk_ld::Blocks(const twk_ld_settings& s, const twk_block_settings& bs) {
	ReduceCommand cmd(settings, *mImpl);
	if (!cmd.begin(s, "Blocks look at every record", "Cannot find the blocks of a part of the pair space: a block needs every pair inside it")) return false;
	if (!settings.window) { settings.window = true; settings.l_window = 200000; }
	const twk_hip_block_params par{bs.strong_lo, bs.strong_hi, bs.recomb_hi, bs.strong_lo_2, bs.strong_lo_34, bs.inform_permille, bs.max_span_2, bs.max_span_3};
	if (par.strong_lo > 100 || par.strong_hi > 100 || par.recomb_hi > 100 || par.strong_lo_2 > 100 || par.strong_lo_34 > 100 || par.recomb_hi > par.strong_hi || par.inform_permille > 1000) {
		std::cerr << stamp("ERROR") << "The block thresholds are percentages up to 100 with recomb-hi <= strong-hi, and a fraction in permille up to 1000..." << std::endl;
		return false;
	}
	if (settings.l_window <= 0) { std::cerr << stamp("ERROR") << "Blocks need a window of at least one base (-w): it is the longest block..." << std::endl; return false; }
	if (const auto l = cmd.load(); l != cmd.ready) return l == cmd.empty;
	const uint32_t M = cmd.M;
	if (M > 0x7FFFFFFFu) { std::cerr << stamp("ERROR") << "Too many variants..." << std::endl; return false; }
	std::vector<uint32_t> block_of(M, TWK_HIP_NO_BLOCK), first(M / 2 + 1), last(M / 2 + 1), n_strong(M / 2 + 1), n_recomb(M / 2 + 1);
	uint64_t np = 0, n_blocks = 0, n_cand = 0, n_inf = 0;
	const double sec = cmd.call("twk_hip_ld_blocks", [&] {
		return twk_hip_ld_blocks(cmd.ctx, cmd.mode, &cmd.f, 0, M, 0, (uint32_t)settings.l_window, &par, block_of.data(), first.data(), last.data(), n_strong.data(), n_recomb.data(),
		                         &n_blocks, &n_cand, &n_inf, &np);
	}, &np);
	if (sec < 0) return false;
	mImpl->n_records = n_inf;
	if (!bs.ci_out.empty()) {
		std::vector<uint32_t> bfirst(M);
		std::vector<uint64_t> indptr((size_t)M + 1);
		if (!hip_ok(cmd.ctx, twk_hip_bandmat_layout(cmd.ctx, 0, M, (uint32_t)settings.l_window, bfirst.data(), indptr.data()), "twk_hip_bandmat_layout")) return false;
		const uint64_t nnz = indptr[M];
		std::vector<uint8_t> lo((size_t)nnz), hi((size_t)nnz);
		uint64_t n_recs = 0, np2 = 0;
		if (cmd.call("twk_hip_ld_dprime_ci_band", [&] {
			return twk_hip_ld_dprime_ci_band(cmd.ctx, cmd.mode, &cmd.f, 0, M, 0, (uint32_t)settings.l_window, lo.data(), hi.data(), nnz, bfirst.data(), indptr.data(), &n_recs, &np2);
		}, nullptr) < 0) return false;
		if (!cmd.npy_files(bs.ci_out, {
			{".lo.npy", "|u1", nnz, lo.data(), lo.size()},
			{".hi.npy", "|u1", nnz, hi.data(), hi.size()},
			{".indptr.npy", "<i8", (uint64_t)M + 1, indptr.data(), indptr.size() * sizeof(uint64_t)},      // (below 2^63: the same bits)
			{".first.npy", "<i4", M, bfirst.data(), bfirst.size() * sizeof(uint32_t)}})) return false;     // (below 2^31)
		if (!cmd.variant_list(bs.ci_out)) return false;
	}
	std::ostream* const os = cmd.open_text();
	if (!os) return false;
	cmd.header(*os, "blocks");
	char line[256];
	snprintf(line, sizeof(line), "##thresholds=strong_lo=%u,strong_hi=%u,recomb_hi=%u,strong_lo_2=%u,strong_lo_34=%u,inform_permille=%u,max_span_2=%u,max_span_3=%u\n",
	         par.strong_lo, par.strong_hi, par.recomb_hi, par.strong_lo_2, par.strong_lo_34, par.inform_permille, par.max_span_2, par.max_span_3);
	*os << line;
	snprintf(line, sizeof(line), "##blocks=%llu,candidates=%llu,informative=%llu,total=%u\n", (unsigned long long)n_blocks, (unsigned long long)n_cand, (unsigned long long)n_inf, M);
	*os << line << "#contig\tfirst_pos\tlast_pos\tspan\tvariants\tstrong\trecombinant\n";
	std::string text;
	for (uint64_t k = 0; k < n_blocks; ++k) {
		const uint32_t a = first[k], b = last[k];
		cmd.place(text, a);
		snprintf(line, sizeof(line), "\t%u\t%u\t%u\t%u\t%u\n", mImpl->pos[b] + 1, mImpl->pos[b] - mImpl->pos[a], b - a + 1, n_strong[k], n_recomb[k]);
		text += line;
		cmd.spill(*os, text);
	}
	if (!cmd.finish(*os, text, "the blocks")) return false;
	std::cerr << stamp("LOG") << "Blocks: " << pretty(n_blocks) << " among " << pretty(M) << " variants, from " << pretty(n_cand) << " candidate pairs of " << pretty(n_inf)
	          << " informative ones among " << pretty(np) << " variant comparisons. " << elapsed_string(sec) << std::endl;
	cmd.all_done();
	return true;
}

// `tomahawk ldsplit`: every contig of the selection split into K near-independent LD blocks for every K up to ss.max_blocks
// (twk_hip_ld_split: the banded r2 matrix kept on the GPU, the dynamic programme solved there), one engine call a contig.  The input is
// loaded exactly as Prune loads it; one GPU; the whole triangle (no -c / -C); the window is required.  Not in the reference.
bool twk_ld::Split(const twk_ld_settings& s, const twk_split_settings& ss) {
	ReduceCommand cmd(settings, *mImpl);
	if (!cmd.begin(s, "A split looks at every record", "Cannot split a part of the pair space: a block sum needs every pair inside the block")) return false;
	if (!settings.window || settings.l_window <= 0) { std::cerr << stamp("ERROR") << "A split needs a window in bases (-w): it bounds the band of r2 that is kept..." << std::endl; return false; }
	if (ss.min_size == 0 || ss.min_size > ss.max_size || ss.max_size > 65535 || ss.max_blocks == 0 || ss.max_blocks > 1024) {
		std::cerr << stamp("ERROR") << "A split needs 1 <= --min-size <= --max-size <= 65535 and 1 <= --max-blocks <= 1024..." << std::endl;
		return false;
	}
	if (ss.blocks > ss.max_blocks) { std::cerr << stamp("ERROR") << "Cannot write a partition of more blocks (-B) than --max-blocks..." << std::endl; return false; }
	if (cmd.to_stdout()) { std::cerr << stamp("ERROR") << "A split writes PREFIX.costs.tsv and PREFIX.blocks.tsv: -o wants a prefix..." << std::endl; return false; }
	if (const auto l = cmd.load(); l != cmd.ready) return l == cmd.empty;
	const uint32_t M = cmd.M, k_max = ss.max_blocks;
	struct Contig { uint32_t a0, n; uint64_t total; std::vector<uint8_t> feasible; std::vector<uint64_t> cost; std::vector<uint32_t> cuts; };
	std::vector<Contig> contigs;
	for (uint32_t a = 0; a < M;) {
		uint32_t b = a + 1;
		while (b < M && mImpl->rid[b] == mImpl->rid[a]) ++b;
		contigs.push_back(Contig{a, b - a, 0, std::vector<uint8_t>(k_max, 0), std::vector<uint64_t>(k_max, 0), std::vector<uint32_t>((size_t)k_max * (k_max + 1), 0)});
		a = b;
	}
	uint64_t pairs = 0, records = 0;
	double sec = 0;
	for (Contig& c : contigs) {
		if ((uint64_t)c.n * ss.max_size >= (1ull << 32)) {
			std::cerr << stamp("ERROR") << "Cannot split a contig of " << pretty(c.n) << " variants into blocks of up to " << ss.max_size << ": variants x --max-size must stay below 2^32..." << std::endl;
			return false;
		}
		uint64_t np = 0, nr = 0;
		const double one = cmd.call("twk_hip_ld_split", [&] {
			return twk_hip_ld_split(cmd.ctx, cmd.mode, &cmd.f, c.a0, c.n, 0, (uint32_t)settings.l_window, ss.min_size, ss.max_size, k_max, &c.total, c.feasible.data(), c.cost.data(), c.cuts.data(), &nr, &np);
		}, nullptr);
		if (one < 0) return false;
		sec += one; pairs += np; records += nr;
	}
	mImpl->n_pairs = pairs;
	mImpl->n_records = records;
	auto cut = [&](const Contig& c, uint32_t K, uint32_t i) { return c.cuts[(size_t)(K - 1) * (k_max + 1) + i]; };
	if (ss.blocks)
		for (const Contig& c : contigs)
			if (!c.feasible[ss.blocks - 1]) {
				std::string where;
				cmd.place(where, c.a0);
				std::cerr << stamp("ERROR") << "Cannot split the contig of " << where.substr(0, where.find('\t')) << " (" << pretty(c.n) << " variants) into " << ss.blocks << " blocks of " << ss.min_size << " to "
				          << ss.max_size << " variants..." << std::endl;
				return false;
			}
	std::ofstream out;
	if (!cmd.open(out, settings.out + ".costs.tsv")) return false;
	cmd.header(out, "ldsplit");
	char line[256];
	snprintf(line, sizeof(line), "##sizes=min_size=%u,max_size=%u,max_blocks=%u\n", ss.min_size, ss.max_size, k_max);
	out << line << "#contig\tK\tcost\tcost_fraction\tsum_squared_sizes\n";
	std::string text;
	uint64_t rows = 0;
	for (const Contig& c : contigs) {
		std::string where;
		cmd.place(where, c.a0);
		where.resize(where.find('\t'));
		for (uint32_t K = 1; K <= k_max; ++K) {
			if (!c.feasible[K - 1]) continue;
			uint64_t squares = 0;
			for (uint32_t i = 1; i <= K; ++i) { const uint64_t size = cut(c, K, i) - cut(c, K, i - 1); squares += size * size; }
			const double cost = (double)c.cost[K - 1];
			snprintf(line, sizeof(line), "\t%u\t%.17g\t%.17g\t%llu\n", K, cost / 4294967296.0, c.total ? cost / (double)c.total : 0.0, (unsigned long long)squares);
			text += where; text += line;
			cmd.spill(out, text);
			++rows;
		}
	}
	if (!cmd.finish(out, text, "the costs")) return false;
	out.close();
	text.clear();
	if (ss.blocks) {
		if (!cmd.open(out, settings.out + ".blocks.tsv")) return false;
		cmd.header(out, "ldsplit");
		snprintf(line, sizeof(line), "##sizes=min_size=%u,max_size=%u,max_blocks=%u,blocks=%u\n", ss.min_size, ss.max_size, k_max, ss.blocks);
		out << line << "#contig\tblock\tfirst_pos\tlast_pos\tvariants\n";
		for (const Contig& c : contigs)
			for (uint32_t i = 1; i <= ss.blocks; ++i) {
				const uint32_t a = c.a0 + cut(c, ss.blocks, i - 1), b = c.a0 + cut(c, ss.blocks, i) - 1;
				cmd.place(text, a);
				snprintf(line, sizeof(line), "\t%u\t%u\n", mImpl->pos[b] + 1, b - a + 1);
				// (contig <TAB> first pos came from place(): the block's number goes between them)
				const size_t tab = text.rfind('\t');
				text.insert(tab, "\t" + std::to_string(i));
				text += line;
				cmd.spill(out, text);
			}
		if (!cmd.finish(out, text, "the blocks")) return false;
		out.close();
	}
	std::cerr << stamp("LOG") << "Split: " << pretty(contigs.size()) << " contigs of " << pretty(M) << " variants, " << pretty(rows) << " feasible (contig, K) among K <= " << k_max << ", " << pretty(records)
	          << " pairs with a value among " << pretty(pairs) << " variant comparisons. " << elapsed_string(sec) << std::endl;
	cmd.all_done();
	return true;
}

// `tomahawk relationship`: the sample-by-sample matrix over the variants of the selection (twk_hip_relationship: transposed, contracted and
// divided on the GPU), as text on stdout or as a NumPy file or text file with the samples' names next to it.  The input is loaded exactly as
// Prune loads it; one GPU.  The reference's command of the same name is not reproduced (include/twk_hip.h says why).
bool twk_ld::Relationship(const twk_ld_settings& s, const twk_relationship_settings& rs) {
	ReduceCommand cmd(settings, *mImpl);
	if (!cmd.begin(s, "The matrix is counted, not tested", "Cannot relate over a part of the pair space: the samples are compared over every selected variant")) return false;
	if (!REL_STATS.valid(rs.stat)) { std::cerr << stamp("ERROR") << "Unknown statistic: one of " << REL_STATS.list() << "..." << std::endl; return false; }
	if (const auto l = cmd.load(); l != cmd.ready) return l == cmd.empty;
	const uint32_t n = cmd.S.n_samples;
	std::vector<double> m((size_t)n * n);
	uint64_t np = 0;
	const double sec = cmd.call("twk_hip_relationship", [&] { return twk_hip_relationship(cmd.ctx, nullptr, 0, 0, n, 0, n, rs.stat, rs.fill, m.data(), n, nullptr, 0, &np); }, nullptr);
	if (sec < 0) return false;

	// as text: one row per sample, tab-separated, 17 significant digits (a NaN prints as nan whatever its bits: the .npy keeps them)
	if (cmd.to_stdout()) {
		if (!cmd.dense_text(std::cout, m.data(), n, '\t', 17, true)) return false;
	} else {
		std::ofstream file, sfile;
		if (!cmd.open(file, settings.out + (rs.text ? ".tsv" : ".npy"), std::ios::binary)) return false;
		if (!(rs.text ? cmd.dense_text(file, m.data(), n, '\t', 17, true) : cmd.npy(file, "<f8", n, n, m.data(), m.size() * sizeof(double)))) return false;
		file.close();
		if (!cmd.open(sfile, settings.out + ".samples.tsv")) return false;
		std::string text;
		for (const std::string& name : cmd.S.reader.hdr.samples) { text += name; text += '\n'; }
		if (!cmd.finish(sfile, text, "the sample list")) return false;
	}
	std::cerr << stamp("LOG") << "Relationship (" << REL_STATS.name(rs.stat) << "): " << pretty(n) << " x " << pretty(n) << " samples over " << pretty(cmd.M) << " variants, "
	          << pretty(np) << " sample pairs. " << elapsed_string(sec) << std::endl;
	cmd.all_done();
	return true;
}

// scalc: one target site against its neighbourhood (ld.cpp:673-876, LoadTargetSingle :123-255,
// CalculateSingle ld_engine.cpp:2226-2332).
bool twk_ld::ComputeSingle(bool verbose, bool) {
	mImpl->n_pairs = mImpl->n_records = 0;
	if (settings.in.empty()) { std::cerr << stamp("ERROR") << "No file-name provided..." << std::endl; return false; }
	if (settings.n_chunks != 1) { std::cerr << stamp("ERROR") << "Cannot use chunking in single mode!" << std::endl; return false; }
	if (settings.window) { std::cerr << stamp("ERROR") << "Cannot use window mode when running in single mode!" << std::endl; return false; }
	if (settings.ival_strings.size() != 1) { std::cerr << stamp("ERROR") << "Single mode requires exactly one target interval (-I)..." << std::endl; return false; }
	settings.single = true;
	TwkReader reader;
	if (!open_input(reader, settings.in, verbose)) return false;
	const uint32_t n_samples = (uint32_t)reader.hdr.samples.size();      // (of the input: what is uploaded)
	std::vector<uint32_t> keep;
	if (!select_samples(settings, reader.hdr, keep)) return false;
	VariantLists lists;
	if (!read_variant_lists(settings, lists)) return false;
	Interval tgt;
	if (!parse_interval(settings.ival_strings[0], reader.hdr, tgt)) return false;
	// Flanks (ld.cpp:145-153), 1-based inclusive matching of pos+1 (ld.cpp:192):
	//   left  [max(from - l_surrounding, 0), max(from - 1, 0)]    right [to, to + l_surrounding]
	const uint32_t L = (uint32_t)std::max(0, settings.l_surrounding);
	const uint32_t left_lo = tgt.from > L ? tgt.from - L : 0, left_hi = tgt.from > 0 ? tgt.from - 1 : 0;
	const uint32_t right_lo = tgt.to, right_hi = tgt.to + L;
	std::vector<uint32_t> blocks;
	overlapping_blocks(reader.index, Interval{tgt.rid, left_lo, right_hi}, blocks);
	if (blocks.empty()) { std::cerr << stamp("ERROR", "INTERVAL") << "Found no blocks overlapping the provided range(s)..." << std::endl; return false; }

	// Neighbourhoods are small: read the overlapping blocks whole, keep targets first then the rest.
	std::vector<Variant> targets, others;
	for (uint32_t b : blocks) {
		Block blk;
		if (!reader.read_block(b, blk)) { std::cerr << stamp("ERROR") << "Failed to load block " << b << "..." << std::endl; return false; }
		for (auto& v : blk.rcds) {
			if ((int32_t)v.rid != tgt.rid) continue;
			const uint32_t p1 = v.pos + 1;
			if (p1 >= tgt.from && p1 <= tgt.to) targets.push_back(std::move(v));
			else if ((p1 >= left_lo && p1 <= left_hi) || (p1 >= right_lo && p1 <= right_hi)) others.push_back(std::move(v));
		}
	}
	if (targets.empty()) { std::cerr << "no data found for reference" << std::endl; return false; }
	if (ref_compat()) others.resize(others.size() / 100 * 100);      // the reference keeps the neighbours in full groups of 100 only (ld.cpp:203-205, 239-244)
	if (others.empty()) { std::cerr << "no surrounding variants" << std::endl; return false; }
	uint32_t nT = (uint32_t)targets.size(), nO = (uint32_t)others.size();
	const uint32_t M = nT + nO;
	if (verbose) std::cerr << stamp("LOG") << pretty(nT) << " target and " << pretty(nO) << " surrounding variants..." << std::endl;

	DeviceCtxs dc;
	if (!create_devices(dc, 1, mImpl->engine_options)) return false;
	twk_hip_ctx* ctx = dc.ctx[0];
	if (!hip_ok(ctx, twk_hip_set_problem(ctx, n_samples, M), "twk_hip_set_problem")) return false;
	const size_t w64 = ((size_t)2 * n_samples + 63) / 64;
	std::vector<uint64_t> data((size_t)M * w64), mask;
	std::vector<twk_hip_variant_meta> meta(M);
	bool any_mask = false;
	for (uint32_t i = 0; i < M; ++i) any_mask |= (i < nT ? targets[i] : others[i - nT]).gt_missing;
	if (any_mask) mask.assign((size_t)M * w64, 0);
	mImpl->rid.assign(M, 0); mImpl->pos.assign(M, 0);
	for (uint32_t i = 0; i < M; ++i) {
		const Variant& v = i < nT ? targets[i] : others[i - nT];
		if (!v.build_bitvector(n_samples, &data[(size_t)i * w64], (any_mask && v.gt_missing) ? &mask[(size_t)i * w64] : nullptr)) {
			std::cerr << stamp("ERROR") << "Corrupt genotype runs!" << std::endl; return false;
		}
		twk_hip_variant_meta& mm = meta[i];
		mm.ac = v.ac; mm.an = v.an; mm.pos = v.pos; mm.rid = v.rid; mm.missing = v.gt_missing ? 1 : 0; mm._pad = 0; mm.hwe = v.hwe;
		mImpl->rid[i] = v.rid; mImpl->pos[i] = v.pos;
	}
	if (!hip_ok(ctx, twk_hip_upload_bitvectors(ctx, 0, M, data.data(), any_mask ? mask.data() : nullptr, w64, meta.data()),
	            "twk_hip_upload_bitvectors")) return false;
	if (!apply_sample_selection(ctx, keep, M, (uint32_t)std::max(1, std::min(settings.n_threads, util::usable_cpus())), nullptr)) return false;
	if (!apply_variant_selection(dc.ctx, settings, lists, reader.hdr, mImpl->rid, mImpl->pos, nT, nO, nullptr)) return false;      // (targets first, then the neighbours: the order is kept)
	if (nT == 0) { std::cerr << "no data found for reference" << std::endl; return false; }
	if (nO == 0) { std::cerr << "no surrounding variants" << std::endl; return false; }
	RunSpec spec;
	spec.nA = nT; spec.nB = nO; spec.triangleA = true; spec.rectAB = true;
	spec.options = TWK_HIP_OPT_KEEP_LOW_AC | (ref_compat() ? TWK_HIP_OPT_REF_COMPAT : 0);      // the skip is commented out in CalculateSingle (:2267-2269)
	return mImpl->run(settings, reader.hdr, dc.ctx, (uint32_t)reader.hdr.samples.size(), &spec);
}

}  // namespace tomahawk
