// hns_seed.hpp -- the seeds of a point set (include/hns.h: hns_point_leaves states the definition once): which points seed, the leaves under their eight taps and the tap
// bits, shared by the host mirror (hns_leafio.cpp), the device kernels (hns_seed.hip) and the seeded regrid (hns_regrid.hip). (The pooled device scratch of a call that
// the regrid and the seed kernels both draw from: hns::Scratch, hns_pool.hpp.)
#pragma once

#include <vector>

#include "hns_internal.hpp"

namespace hns {

constexpr uint64_t kMaxSeedPoints = 0x7fffffffull;
constexpr uint64_t kMaxSeedLeaves = uint64_t(1) << 23;  // distinct leaves of a point set: the candidate-hash bound of the regrid

// does a coordinate seed? (NaN and +-inf fail; inside, a float32 floor is exact and a leaf coordinate of a tap fits 21 bits)
__host__ __device__ inline bool seeds_f(float c) { return -8388608.0f <= c && c < 8388607.0f; }

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
