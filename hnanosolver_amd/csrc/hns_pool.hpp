// hns_pool.hpp -- what a piece of host code that needs device memory reaches for: the owner of one block of the pool (hns_arena.hip), the one way to lay slices
// over a block, the blocks of one call, and a private stream for a build. Host code only; hns_internal.hpp includes it in front of the structs that own blocks.
#pragma once

#include <type_traits>
#include <utility>
#include <vector>

// implemented in hns_arena.hip: the process-wide pool of device allocations. hns_arena_put waits for the whole device (unless p is null: then it does nothing).
// It is a weak reference: the host-only files of the library (hns_topology.cpp, hns_nanovdb.cpp, hns_leafio.cpp) destroy grids, whose owners name it, and still link
// into a program without the pool (tests/cpp/host_sanitize.cpp). Such a program never draws a block, and an owner without a block never calls it.
extern "C" __attribute__((visibility("hidden"))) int hns_arena_get(size_t need, int device, void** p, size_t* bytes);
extern "C" __attribute__((visibility("hidden"), weak)) void hns_arena_put(void* p, size_t bytes, int device);

namespace hns {

inline size_t pad256(size_t b) { return (b + 255) & ~(size_t)255; }

// One block of the pool, given back when its owner goes. Move-only; an empty owner never calls the pool. No zeroing, no streams: what the block holds and who may
// still be reading it is its user's business (release() and the destructor wait for the device inside hns_arena_put).
struct Pooled {
	void* p = nullptr;
	size_t bytes = 0;  // of the block: at least what was asked for
	int device = -1;
	Pooled() = default;
	Pooled(const Pooled&) = delete;
	Pooled& operator=(const Pooled&) = delete;
	Pooled(Pooled&& o) noexcept : p(o.p), bytes(o.bytes), device(o.device) { o.p = nullptr, o.bytes = 0; }
	Pooled& operator=(Pooled&& o) noexcept {
		if (this != &o) {
			release();
			p = o.p, bytes = o.bytes, device = o.device;
			o.p = nullptr, o.bytes = 0;
		}
		return *this;
	}
	~Pooled() { release(); }
	void release() {
		if (p) hns_arena_put(p, bytes, device);
		p = nullptr, bytes = 0;
	}
	int get(size_t need, int dev) {  // a block of at least `need` bytes on `dev` (what the owner held goes back first); empty when the pool fails
		release();
		device = dev;
		const int rc = hns_arena_get(need, dev, &p, &bytes);
		if (rc != HNS_OK) p = nullptr, bytes = 0;
		return rc;
	}
	int reserve(size_t need, int dev) { return p && bytes >= need ? (int)HNS_OK : get(need, dev); }  // keeps a block that is large enough; the contents are not carried over
	explicit operator bool() const { return p != nullptr; }
	template <class T = void>
	T* as() const { return (T*)p; }
};

// Slices of one allocation, 256-byte aligned, stated once: `slices(slice)` names every slice in order, as slice(pointer, bytes) -- pad256(bytes) of room -- or
// slice(pointer, k, unit) -- k units of `unit` bytes, unit a multiple of 256. carve walks the list twice: first to add up the room, then (base not null) to point
// every pointer at its slice; it returns the room. On the second walk slice(...) is true, so a list may upload behind it. Any memory, pooled or not.
struct Slice {
	char* base;  // null: the sizing walk
	size_t* at;
	template <class T>
	bool operator()(T*& ptr, size_t bytes) const { return (*this)(ptr, pad256(bytes), 1); }
	template <class T>
	bool operator()(T*& ptr, size_t k, size_t unit) const {
		if (base) ptr = (T*)(base + *at);
		*at += k * unit;
		return base != nullptr;
	}
};
template <class F>
size_t carve(void* base, F&& slices) {
	size_t room = 0, at = 0;
	slices(Slice{nullptr, &room});
	if (base) slices(Slice{(char*)base, &at});
	return room;
}
// ... over a block drawn for it
template <class F>
int carve(Pooled& block, int device, F&& slices) {
	HNS_TRY(block.get(carve(nullptr, slices), device));
	carve(block.p, slices);
	return HNS_OK;
}

// The device allocations of one call, back in the pool however it ends. A block the call's result keeps is moved (or swapped) out of `held`.
struct Scratch {
	std::vector<Pooled> held;
	int device;
	explicit Scratch(int dev) : device(dev) {}
	int get(size_t bytes, void** p) {  // the new block is held.back()
		Pooled b;
		HNS_TRY(b.get(bytes, device));
		*p = b.p;
		held.push_back(std::move(b));
		return HNS_OK;
	}
	template <class F>
	int carve(F&& slices) {
		Pooled b;
		HNS_TRY(hns::carve(b, device, slices));
		held.push_back(std::move(b));
		return HNS_OK;
	}
};

// A non-blocking stream of a build's own, destroyed on every way out of the scope.
struct PrivateStream {
	hipStream_t st = nullptr;
	PrivateStream() = default;
	PrivateStream(const PrivateStream&) = delete;
	PrivateStream& operator=(const PrivateStream&) = delete;
	int create() {
		HNS_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
		return HNS_OK;
	}
	~PrivateStream() {
		if (st) (void)hipStreamDestroy(st);
	}
};

}  // namespace hns
