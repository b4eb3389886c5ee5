// The engine's device and page-locked host buffers (twk_hip.hip): each is owned by one object that frees it, and all of them grow
// through one step, Buffer::reserve.
//
// Freeing device memory waits for the whole device, every stream, and in the middle of a region's launch pipeline that was a stall of
// 50-250 ms a time (profiles/r05_delivery_thread.txt).  So a buffer that is outgrown while launches may still read it is not freed but
// parked in the call's Graveyard, which frees what it holds when it is flushed - by the engine once nothing is in flight any more: when
// the call ends, or with the context.  A buffer that nothing can still be reading is grown without a graveyard: freed at once, before its
// successor is allocated.
// Out of memory is handled here and nowhere else: the old buffer is parked too, the graveyard's owner is asked to give back what it can
// (Graveyard::reclaim - the engine hands over what the delivery queue holds idle, waits for the device and flushes the graveyard) and the
// allocation is tried once more before the call fails.
//
// Backend-free, like twk_delivery.h: the four runtime calls come in through Ops, so that ownership can be checked on the CPU with stub
// operations that keep the set of live pointers (csrc/tools/buffers_check.cpp, `make buffers-check`).  Ops provides, all static,
//     typedef ... error;   error ok, out_of_memory
//     error device_alloc(void** p, size_t bytes)     void device_free(void* p)
//     error host_alloc(void** p, size_t bytes)       void host_free(void* p)         (page-locked)
#pragma once
#include <algorithm>
#include <cstddef>
#include <functional>
#include <utility>
#include <vector>

namespace twk {

template <class Ops>
class Graveyard {
public:
	std::function<bool()> reclaim;      // out of memory: give back what can be given back, what is parked here included -> true when anything was

	Graveyard() = default;
	~Graveyard() { flush(); }
	Graveyard(const Graveyard&) = delete;
	Graveyard& operator=(const Graveyard&) = delete;

	bool empty() const { return parked.empty(); }
	void park(void* p, bool pinned) { if (p) parked.emplace_back(p, pinned); }
	void flush() {                      // (the caller has made sure that nothing reads them any more)
		for (const auto& b : parked) b.second ? Ops::host_free(b.first) : Ops::device_free(b.first);
		parked.clear();
	}

private:
	std::vector<std::pair<void*, bool>> parked;
};

// `capacity()` items of T in device memory, or (Pinned) in page-locked host memory.  Reads like the pointer it holds.
template <class T, class Ops, bool Pinned = false>
class Buffer {
public:
	Buffer() = default;
	~Buffer() { reset(); }
	Buffer(Buffer&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
	Buffer& operator=(Buffer&& o) noexcept {
		if (this != &o) { reset(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
		return *this;
	}

	T* get() const { return p; }
	operator T*() const { return p; }
	size_t capacity() const { return cap; }
	void reset() {
		if (p) Pinned ? Ops::host_free(p) : Ops::device_free(p);
		p = nullptr; cap = 0;
	}

	// Room for `need` items: nothing happens while there is; otherwise the buffer is replaced by one of `want` (>= need) items - the
	// slack is the caller's rule.  Contents are not kept.  park: where the old buffer waits while launches may still read it (null: it
	// is freed at once).  After a failure the buffer is its old self, or empty.
	typename Ops::error reserve(size_t need, size_t want, Graveyard<Ops>* park) {
		if (cap >= need) return Ops::ok;
		if (!park) reset();
		const size_t bytes = std::max(need, want) * sizeof(T);
		void* q = nullptr;
		typename Ops::error e = alloc(&q, bytes);
		if (e == Ops::out_of_memory && park) {
			park->park(p, Pinned); p = nullptr; cap = 0;
			if (park->reclaim && park->reclaim()) e = alloc(&q, bytes);
		}
		if (e != Ops::ok) return e;
		if (park) park->park(p, Pinned);
		p = static_cast<T*>(q); cap = std::max(need, want);
		return Ops::ok;
	}

private:
	static typename Ops::error alloc(void** q, size_t bytes) { return Pinned ? Ops::host_alloc(q, bytes) : Ops::device_alloc(q, bytes); }
	T* p = nullptr;
	size_t cap = 0;
};

// Buffers that share one capacity (a survivor, its sort key, its position) grow through one call.  What they share is the smallest of
// theirs: when an allocation in the middle fails, the group still has its old capacity, and the next call grows the ones that are behind.
template <class Ops, class... B>
typename Ops::error reserve_together(size_t need, size_t want, Graveyard<Ops>* park, B&... b) {
	typename Ops::error e = Ops::ok;
	(void)(((e = b.reserve(need, want, park)) == Ops::ok) && ...);
	return e;
}
template <class... B>
size_t shared_capacity(const B&... b) { return std::min({b.capacity()...}); }

// The device buffers that live exactly as long as one call: each request is an allocation of its own (Buffer::reserve, freed at once -
// no graveyard: nothing reads a buffer that has not been handed out yet), all of them are released together when the owner dies, and a
// request that fails leaves the earlier ones held until then.  The owner's place decides when that is: a member of the object whose
// destructor waits for the device is released behind that wait.
template <class Ops>
class CallMemory {
public:
	CallMemory() = default;
	CallMemory(const CallMemory&) = delete;
	CallMemory& operator=(const CallMemory&) = delete;

	// `items` of T, or null with the allocator's verdict in *e.  (No item: null and ok, as reserve(0, 0) - nothing is allocated.)
	template <class T>
	T* take(size_t items, typename Ops::error* e) {
		held.emplace_back();
		return grow<T>(held.back(), items, e);
	}
	// Room for `items` in the buffer take() returned as `p`: it stays where it is while it has the room and is replaced - freed, then
	// allocated - when not (a scratch buffer that a later step of the call needs larger).  Contents are not kept; after a failure that
	// buffer is empty.
	template <class T>
	T* retake(T* p, size_t items, typename Ops::error* e) {
		for (Buffer<char, Ops>& b : held)
			if (p && b.get() == reinterpret_cast<char*>(p)) return grow<T>(b, items, e);
		return take<T>(items, e);
	}
	// What the requests that succeeded asked for, in bytes.
	size_t bytes() const { return total; }

private:
	template <class T>
	T* grow(Buffer<char, Ops>& b, size_t items, typename Ops::error* e) {
		total -= b.capacity();
		*e = b.reserve(items * sizeof(T), items * sizeof(T), nullptr);
		total += b.capacity();
		return *e == Ops::ok ? reinterpret_cast<T*>(b.get()) : nullptr;
	}
	std::vector<Buffer<char, Ops>> held;      // (each as many bytes as its request)
	size_t total = 0;
};

}  // namespace twk
