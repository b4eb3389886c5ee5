// Ownership harness for the engine's buffer types (csrc/hip/twk_buffers.h) with the runtime's allocator stubbed: `make buffers-check`
// builds this file with plain g++ and runs it.  The stub keeps the set of live pointers: releasing a pointer that is not live (a double
// free, a free through the wrong call) fails the run at once, and so does a case that ends with a pointer still live (a leak).  The cases
// walk what the engine does with its buffers: growing, parking, flushing, freeing at once, running out of memory with and without
// something to reclaim, groups that share a capacity, moves, holders that are assigned over and destroyed; and a call's memory
// (CallMemory): takes released once with the owner, a take that fails in the middle, its bytes(), a scratch buffer taken again.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>

#include "../hip/twk_buffers.h"

struct StubOps {
	typedef int error;
	static constexpr int ok = 0, out_of_memory = 2, broken = 1;
	static std::map<void*, bool> live;        // pointer -> page-locked?
	static long n_alloc, n_release;
	static long fail_at;                      // the n-th allocation from now fails (0: none) ...
	static int fail_with;                     // ... with this
	static size_t budget;                     // bytes that may be live at a time (0: no limit): beyond it an allocation is out of memory
	static size_t live_bytes;
	static std::map<void*, size_t> bytes_of;

	static int alloc(void** p, size_t bytes, bool pinned) {
		++n_alloc;
		if (fail_at && --fail_at == 0) return fail_with;
		if (budget && live_bytes + bytes > budget) return out_of_memory;
		*p = std::malloc(bytes ? bytes : 1);
		if (!*p) { std::fprintf(stderr, "the host is out of memory\n"); std::exit(2); }
		live[*p] = pinned; bytes_of[*p] = bytes; live_bytes += bytes;
		return ok;
	}
	static void release(void* p, bool pinned) {
		++n_release;
		auto it = live.find(p);
		if (it == live.end()) { std::fprintf(stderr, "FAIL: release of %p, which is not live\n", p); std::exit(1); }
		if (it->second != pinned) { std::fprintf(stderr, "FAIL: %p released through the wrong call\n", p); std::exit(1); }
		live_bytes -= bytes_of[p]; bytes_of.erase(p); live.erase(it);
		std::free(p);
	}
	static int device_alloc(void** p, size_t bytes) { return alloc(p, bytes, false); }
	static void device_free(void* p) { release(p, false); }
	static int host_alloc(void** p, size_t bytes) { return alloc(p, bytes, true); }
	static void host_free(void* p) { release(p, true); }
};
std::map<void*, bool> StubOps::live;
std::map<void*, size_t> StubOps::bytes_of;
long StubOps::n_alloc = 0, StubOps::n_release = 0, StubOps::fail_at = 0;
int StubOps::fail_with = StubOps::out_of_memory;
size_t StubOps::budget = 0, StubOps::live_bytes = 0;

template <class T> using Dev = twk::Buffer<T, StubOps>;
template <class T> using Pinned = twk::Buffer<T, StubOps, true>;
typedef twk::Graveyard<StubOps> Yard;
typedef twk::CallMemory<StubOps> Call;

static int n_cases = 0, n_bad = 0;
static const char* current = "";
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "FAIL [%s] %s:%d: %s\n", current, __FILE__, __LINE__, #cond); ++n_bad; } } while (0)
template <class F> static void run(const char* name, F body) {
	current = name; ++n_cases;
	StubOps::fail_at = 0; StubOps::fail_with = StubOps::out_of_memory; StubOps::budget = 0;
	body();
	if (!StubOps::live.empty()) { std::fprintf(stderr, "FAIL [%s]: %zu pointers still live at the end\n", name, StubOps::live.size()); ++n_bad; }
	for (auto& kv : StubOps::live) std::free(kv.first);
	StubOps::live.clear(); StubOps::bytes_of.clear(); StubOps::live_bytes = 0;
}
static bool is_live(const void* p) { return StubOps::live.count(const_cast<void*>(p)) != 0; }

// a holder in the manner of the engine's plane sets: some owners, some plain fields
struct Holder { Dev<int> a; Dev<double> b; Pinned<int> h; int* alias = nullptr; int n = 0; };

int main() {
	run("grow from empty, grow again, grow to less", [] {
		Yard yard; Dev<int> b;
		CHECK(b.get() == nullptr && b.capacity() == 0);
		CHECK(b.reserve(0, 0, &yard) == StubOps::ok && !b.get());                  // nothing wanted, nothing allocated
		CHECK(b.reserve(100, 125, &yard) == StubOps::ok);
		CHECK(b.get() && b.capacity() == 125 && yard.empty());
		int* first = b.get();
		CHECK(b.reserve(120, 150, &yard) == StubOps::ok && b.get() == first);      // room for 120: nothing happens
		const long releases = StubOps::n_release;
		CHECK(b.reserve(200, 250, &yard) == StubOps::ok);
		CHECK(b.get() != first && b.capacity() == 250);
		CHECK(is_live(first) && !yard.empty() && StubOps::n_release == releases);   // parked, not released
		CHECK(b.reserve(10, 10, &yard) == StubOps::ok && b.capacity() == 250);
		yard.flush();
		CHECK(!is_live(first) && yard.empty() && StubOps::n_release == releases + 1);
		yard.flush();                                                               // (once: a second flush has nothing to release)
		CHECK(StubOps::n_release == releases + 1 && is_live(b.get()));
	});
	run("freed at once", [] {
		Pinned<char> b;
		CHECK(b.reserve(10, 10, nullptr) == StubOps::ok);
		char* first = b.get();
		CHECK(StubOps::live[first] == true);                                        // page-locked memory through the host calls
		const long releases = StubOps::n_release;
		CHECK(b.reserve(20, 20, nullptr) == StubOps::ok);
		CHECK(StubOps::n_release == releases + 1 && StubOps::live.size() == 1 && is_live(b.get()) && b.capacity() == 20);      // (its address may be the old one again)
		b.reset();
		CHECK(!b.get() && b.capacity() == 0);
		b.reset();
	});
	run("an allocation fails: old self or empty, a later grow succeeds", [] {
		Yard yard; Dev<int> b;
		CHECK(b.reserve(10, 10, &yard) == StubOps::ok);
		int* first = b.get();
		StubOps::fail_at = 1; StubOps::fail_with = StubOps::broken;                 // not out of memory: nothing is parked, nothing retried
		CHECK(b.reserve(20, 20, &yard) == StubOps::broken);
		CHECK(b.get() == first && b.capacity() == 10 && yard.empty());
		StubOps::fail_at = 1; StubOps::fail_with = StubOps::out_of_memory;          // out of memory, no reclaim to ask: parked, empty
		CHECK(b.reserve(20, 20, &yard) == StubOps::out_of_memory);
		CHECK(!b.get() && b.capacity() == 0 && is_live(first) && !yard.empty());
		CHECK(b.reserve(20, 20, &yard) == StubOps::ok && b.capacity() == 20);
		Dev<int> at_once;
		CHECK(at_once.reserve(5, 5, nullptr) == StubOps::ok);
		StubOps::fail_at = 1;
		CHECK(at_once.reserve(50, 50, nullptr) == StubOps::out_of_memory);
		CHECK(!at_once.get() && at_once.capacity() == 0);
		CHECK(at_once.reserve(1, 1, nullptr) == StubOps::ok && at_once.capacity() == 1);      // (a fallback that needs far less)
	});
	run("out of memory with a reclaim hook: the retry succeeds", [] {
		Yard yard; Dev<char> b, other;
		int asked = 0;
		yard.reclaim = [&] { ++asked; const bool any = !yard.empty(); yard.flush(); return any; };
		StubOps::budget = 1000;
		CHECK(b.reserve(600, 600, &yard) == StubOps::ok);
		CHECK(b.reserve(700, 700, &yard) == StubOps::ok);       // 600 parked + 700 > 1000: the old buffer is given back, then there is room
		CHECK(asked == 1 && b.capacity() == 700 && yard.empty() && StubOps::live_bytes == 700);
		CHECK(other.reserve(200, 200, &yard) == StubOps::ok);
		CHECK(other.reserve(400, 400, &yard) == StubOps::out_of_memory);      // 700 + 400: what can be given back (its own 200) is not enough
		CHECK(asked == 2 && !other.get() && other.capacity() == 0 && b.capacity() == 700);
		CHECK(other.reserve(300, 300, &yard) == StubOps::ok);
		const long allocs = StubOps::n_alloc;
		Dev<char> third;
		CHECK(third.reserve(100, 100, &yard) == StubOps::out_of_memory);      // nothing to give back: not tried again
		CHECK(asked == 3 && StubOps::n_alloc == allocs + 1);
	});
	run("a group with one capacity: the second allocation fails", [] {
		Yard yard; Dev<double> recs; Dev<long> keys; Dev<int> vals;
		CHECK(twk::reserve_together(10, 10, &yard, recs, keys, vals) == StubOps::ok);
		CHECK(twk::shared_capacity(recs, keys, vals) == 10);
		StubOps::fail_at = 2;
		CHECK(twk::reserve_together(40, 50, &yard, recs, keys, vals) == StubOps::out_of_memory);
		CHECK(twk::shared_capacity(recs, keys, vals) < 40);                     // not the new capacity
		CHECK(recs.capacity() == 50 && keys.capacity() == 0 && vals.capacity() == 10);
		const long allocs = StubOps::n_alloc;
		CHECK(twk::reserve_together(40, 50, &yard, recs, keys, vals) == StubOps::ok);      // the ones that are behind catch up
		CHECK(twk::shared_capacity(recs, keys, vals) == 50 && StubOps::n_alloc == allocs + 2);
		Pinned<int> h; Dev<int> d;                                              // page-locked and device memory side by side
		CHECK(twk::reserve_together(8, 16, &yard, h, d) == StubOps::ok && twk::shared_capacity(h, d) == 16);
		CHECK(twk::reserve_together(32, 32, &yard, h, d) == StubOps::ok);
	});
	run("move assignment over a buffer in use", [] {
		Dev<int> keep, fresh;
		CHECK(keep.reserve(10, 10, nullptr) == StubOps::ok && fresh.reserve(30, 30, nullptr) == StubOps::ok);
		int* old = keep.get(); int* taken = fresh.get();
		const long releases = StubOps::n_release;
		keep = std::move(fresh);
		CHECK(!is_live(old) && StubOps::n_release == releases + 1);
		CHECK(keep.get() == taken && keep.capacity() == 30 && !fresh.get() && fresh.capacity() == 0);
		Dev<int> built(std::move(keep));
		CHECK(built.get() == taken && !keep.get() && StubOps::n_release == releases + 1);
	});
	run("a holder assigned from a fresh one; destruction with buffers parked", [] {
		Holder h;
		{
			Yard yard;
			CHECK(h.a.reserve(4, 4, &yard) == StubOps::ok && h.b.reserve(4, 4, nullptr) == StubOps::ok && h.h.reserve(4, 4, &yard) == StubOps::ok);
			CHECK(h.a.reserve(8, 8, &yard) == StubOps::ok && h.h.reserve(8, 8, &yard) == StubOps::ok);      // two parked
			h.alias = h.a.get(); h.n = 3;
			CHECK(StubOps::live.size() == 5);
			h = Holder();
			CHECK(StubOps::live.size() == 2 && !h.a.get() && !h.b.get() && !h.h.get() && !h.alias && h.n == 0);
		}      // the graveyard goes with two buffers still parked
		CHECK(StubOps::live.empty());
	});
	run("call memory: every take released once, when the owner dies", [] {
		const long allocs = StubOps::n_alloc, releases = StubOps::n_release;
		{
			Call mem;
			int e = StubOps::broken;
			int* a = mem.take<int>(10, &e);
			CHECK(e == StubOps::ok && is_live(a) && StubOps::bytes_of[a] == 40);
			double* b = mem.take<double>(7, &e);
			CHECK(e == StubOps::ok && is_live(b) && StubOps::bytes_of[b] == 56);
			char* z = mem.take<char>(0, &e);                                       // as reserve(0, 0): nothing wanted, nothing allocated
			CHECK(e == StubOps::ok && !z && StubOps::n_alloc == allocs + 2);
			Dev<char> plain;
			CHECK(plain.reserve(0, 0, nullptr) == StubOps::ok && !plain.get() && StubOps::n_alloc == allocs + 2);
			short* s = mem.take<short>(3, &e);
			CHECK(e == StubOps::ok && is_live(s) && is_live(a) && is_live(b));      // (the owner's bookkeeping grew: what it handed out stays put)
			CHECK(mem.bytes() == 40 + 56 + 0 + 6 && StubOps::live_bytes == mem.bytes());
			CHECK(StubOps::n_alloc == allocs + 3 && StubOps::n_release == releases && StubOps::live.size() == 3);
		}
		CHECK(StubOps::live.empty() && StubOps::n_release == releases + 3);
	});
	for (const int verdict : {StubOps::out_of_memory, StubOps::broken})
		for (int k = 1; k <= 4; ++k) run("call memory: the k-th take fails, the earlier ones stay held", [=] {
			const long releases = StubOps::n_release;
			{
				Call mem;
				void* got[4] = {nullptr, nullptr, nullptr, nullptr};
				size_t want = 0;
				StubOps::fail_at = k; StubOps::fail_with = verdict;
				for (int t = 1; t <= 4; ++t) {
					int e = StubOps::ok;
					got[t - 1] = mem.take<long>(100 * t, &e);
					if (t == k) { CHECK(e == verdict && !got[t - 1]); break; }
					CHECK(e == StubOps::ok && got[t - 1]);
					want += 100 * t * sizeof(long);
				}
				for (int t = 1; t < k; ++t) CHECK(is_live(got[t - 1]));
				CHECK(StubOps::live.size() == (size_t)(k - 1) && StubOps::n_release == releases && mem.bytes() == want);
				int e = StubOps::broken;                                                // the owner is still good for a request that can be met
				CHECK(mem.take<char>(5, &e) && e == StubOps::ok && mem.bytes() == want + 5);
			}
			CHECK(StubOps::live.empty() && StubOps::n_release == releases + k);
		});
	// twk_hip_ld_blocks as the source before CallMemory allocated (twk_hip.hip, `hold_for_call` lines of that entry point): ten buffers in
	// front of the launches - two prefix-count bands, counts3, blk, pos, flat, off, block_of, used, the scan's scratch -, the bounds' three
	// (band map, upper, lower), six for the candidates (keys, keys_out, vals, vals_out, cs, cr), and the scratch once more where the sort
	// needs more of it than the scan did: 20 allocations (the outgrown scratch freed at once, so 19 live), 19 where it does not
	for (const bool sort_needs_more : {true, false}) run("call memory: a blocks-like call, scan scratch then sort scratch", [=] {
		const long allocs = StubOps::n_alloc, releases = StubOps::n_release;
		{
			Call mem;
			int e = StubOps::ok;
			const size_t n = 300, cells = 9000, M = 400, q = 1234, scan_tmp = 2048, sort_tmp = sort_needs_more ? 40000 : 1024;
			for (int t = 0; t < 2; ++t) CHECK(mem.take<unsigned>(cells, &e) && e == StubOps::ok);
			for (int t = 0; t < 2; ++t) CHECK(mem.take<unsigned>(n * 3, &e) && e == StubOps::ok);
			for (int t = 0; t < 3; ++t) CHECK(mem.take<unsigned>(n, &e) && e == StubOps::ok);
			CHECK(mem.take<unsigned>(M, &e) && e == StubOps::ok);
			CHECK(mem.take<unsigned long long>((n + 63) / 64, &e) && e == StubOps::ok);
			char* tmp = mem.take<char>(scan_tmp, &e);
			CHECK(tmp && e == StubOps::ok && StubOps::n_alloc == allocs + 10);
			CHECK(mem.take<long>(n, &e) && e == StubOps::ok);                       // the band map (a BandRow is 16 bytes; the size is not the point)
			for (int t = 0; t < 2; ++t) CHECK(mem.take<unsigned char>(cells, &e) && e == StubOps::ok);
			for (int t = 0; t < 2; ++t) CHECK(mem.take<unsigned long long>(q, &e) && e == StubOps::ok);
			for (int t = 0; t < 4; ++t) CHECK(mem.take<unsigned>(q, &e) && e == StubOps::ok);
			const size_t before = mem.bytes();
			char* tmp2 = mem.retake(tmp, std::max(scan_tmp, sort_tmp), &e);
			CHECK(tmp2 && e == StubOps::ok && is_live(tmp2));
			if (sort_needs_more) CHECK(StubOps::bytes_of[tmp2] == sort_tmp && mem.bytes() == before + sort_tmp - scan_tmp && StubOps::n_release == releases + 1);
			else CHECK(tmp2 == tmp && mem.bytes() == before && StubOps::n_release == releases);
			CHECK(StubOps::n_alloc == allocs + (sort_needs_more ? 20 : 19) && StubOps::live.size() == 19 && StubOps::live_bytes == mem.bytes());
		}
		CHECK(StubOps::live.empty() && StubOps::n_release == releases + (sort_needs_more ? 20 : 19));
	});
	run("call memory: a retake that fails leaves its buffer empty and the others held", [] {
		Call mem;
		int e = StubOps::ok;
		int* a = mem.take<int>(4, &e); char* tmp = mem.take<char>(100, &e);
		StubOps::fail_at = 1;
		CHECK(!mem.retake(tmp, (size_t)500, &e) && e == StubOps::out_of_memory);
		CHECK(is_live(a) && StubOps::live.size() == 1 && mem.bytes() == 16);
	});
	// twk_hip_ld_split: bytes() of its takes against the closed form twk_hip_split_last has reported since the call exists
	run("call memory: a split-like call's bytes() is the closed form", [] {
		Call mem;
		int e = StubOps::ok;
		const size_t n = 300, cells = 9000, widest = 17, min_size = 5, max_size = 40, k_max = 12, n1 = n + 1;
		const size_t rp = widest * n, w = (max_size - min_size + 1) * n1, d = k_max * n1, cut = k_max * (k_max + 1);
		mem.take<long long>(rp, &e); mem.take<long long>(w, &e); mem.take<unsigned short>(d, &e); mem.take<long long>(2 * n1, &e);
		mem.take<long long>(n, &e); mem.take<unsigned>(n, &e); mem.take<long long>(k_max + 1, &e); mem.take<unsigned long long>(k_max, &e);
		mem.take<unsigned>(cut, &e); mem.take<unsigned char>(k_max, &e); mem.take<unsigned long long>(1, &e); mem.take<unsigned>(1, &e);
		mem.take<float>(cells, &e);
		struct Row16 { unsigned long long base; unsigned first, len; };
		mem.take<Row16>(n, &e);
		CHECK(e == StubOps::ok);
		CHECK(mem.bytes() == cells * 4 + n * 16 + (rp + w + 2 * n1 + n + k_max + 1) * 8 + d * 2 + n * 4 + k_max * 9 + cut * 4 + 12);
	});
	std::printf("%d cases, %d bad\n", n_cases, n_bad);
	return n_bad ? 1 : 0;
}
