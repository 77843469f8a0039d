// hns_seed.hpp -- the seeds of a point set (include/hns.h: hns_point_leaves states the definition once): which points seed, the leaves under their eight taps and the tap
// bits, shared by the host mirror (hns_leafio.cpp), the device kernels (hns_seed.hip) and the seeded regrid (hns_regrid.hip); and the pooled device scratch of a call that
// the regrid and the seed kernels both draw from.
#pragma once

#include <type_traits>
#include <utility>
#include <vector>

#include "hns_internal.hpp"

namespace hns {

constexpr uint64_t kMaxSeedPoints = 0x7fffffffull;
constexpr uint64_t kMaxSeedLeaves = uint64_t(1) << 23;  // distinct leaves of a point set: the candidate-hash bound of the regrid

// does a coordinate seed? (NaN and +-inf fail; inside, a float32 floor is exact and a leaf coordinate of a tap fits 21 bits)
__host__ __device__ inline bool seeds_f(float c) { return -8388608.0f <= c && c < 8388607.0f; }

inline size_t pad256(size_t b) { return (b + 255) & ~(size_t)255; }

// device allocations of one call, returned to the pool however it ends (hns_arena_put waits for the device first)
struct Scratch {
	std::vector<std::pair<void*, size_t>> held;
	int device;
	explicit Scratch(int dev) : device(dev) {}
	Scratch(const Scratch&) = delete;
	Scratch& operator=(const Scratch&) = delete;
	int get(size_t bytes, void** p) {
		size_t got = 0;
		const int rc = hns_arena_get(bytes, device, p, &got);
		if (rc == HNS_OK) held.emplace_back(*p, got);
		return rc;
	}
	// One allocation in 256-byte aligned slices: `slices(slice)` calls slice(pointer, bytes) once per slice, first to size the allocation, then
	// to point every pointer at its slice, so the sizes and the carve come from the same list.
	template <class F>
	int carve(F slices) {
		size_t total = 0;
		slices([&](auto*&, size_t bytes) { total += pad256(bytes); });
		void* p = nullptr;
		HNS_TRY(get(total, &p));
		char* q = (char*)p;
		slices([&](auto*& ptr, size_t bytes) {
			ptr = reinterpret_cast<std::remove_reference_t<decltype(ptr)>>(q);
			q += pad256(bytes);
		});
		return HNS_OK;
	}
	size_t keep(void* p) {  // ownership passes to the caller: returns the allocation's size
		size_t bytes = 0;
		for (size_t i = 0; i < held.size(); ++i)
			if (held[i].first == p) bytes = held[i].second, held.erase(held.begin() + (long)i);
		return bytes;
	}
	~Scratch() {
		for (auto& h : held) hns_arena_put(h.first, h.second, device);
	}
};

// The seed set S of n device-resident points, on the device: its leaves in no particular order and their masks (64 bytes each, exactly the tap bits).
struct SeedSet {
	int4* origins = nullptr;
	unsigned char* masks = nullptr;
	uint64_t n_leaves = 0;
	uint64_t skipped = 0;  // points that do not seed
};

// hns_seed.hip: builds S in `scratch` on `st`. Waits once, for the leaf count (the masks cannot be sized without it); k_seed_masks is left running on `st`.
// HNS_ERR_TOPOLOGY under `who` when the points hold more than kMaxSeedLeaves distinct leaves.
int seed_leaves(Scratch& scratch, const float* d_xyz, uint64_t n, hipStream_t st, const char* who, SeedSet* out);

// hns_leafio.cpp: perm[r] = the position in xyz of the leaf that comes r-th in OpenVDB leaf order (sort_leaf_origins' order)
void leaf_order(const int32_t* xyz, size_t n, std::vector<uint32_t>* perm);

// n int4 origins on the device, as xyz on the host: what sort_leaf_origins and leaf_order take. Waits for `st`.
inline int download_origins(const int4* d_origins, size_t n, hipStream_t st, std::vector<int32_t>* xyz) {
	std::vector<int32_t> o4(n * 4);
	HNS_HIP(hipMemcpyAsync(o4.data(), d_origins, 16 * n, hipMemcpyDeviceToHost, st));
	HNS_HIP(hipStreamSynchronize(st));
	xyz->resize(n * 3);
	for (size_t i = 0; i < n; ++i)
		for (int a = 0; a < 3; ++a) (*xyz)[3 * i + a] = o4[4 * i + a];
	return HNS_OK;
}

}  // namespace hns
