// hns_stats.hpp -- the one reduction behind hns_stats (include/hns.h: "The reduction"), stated once for the host mirror (hns_leafio.cpp: hns_leaf_stats) and the
// device (hns_diagnostics.hip). A record is combined from per-voxel terms in ONE fixed order, so that the two agree in every byte:
//   inside a leaf   lane L (0..63) adds the terms of voxels 64k + L for k = 0..7 ascending, then the 64 lane sums go through an xor butterfly over lanes 1, 2, 4, 8, 16, 32
//                   (fp addition commutes, so every lane ends with the sum of the balanced tree over lane index);
//   over leaves     a balanced tree over leaf index, padded with empty records up to the next power of two: level s adds entry i + s to entry i for i a multiple of 2s.
// count, nan_count, min, max and max_abs do not depend on any order; they ride along.
#pragma once

#include <cstdint>
#include <cstring>

#include "hns.h"

namespace hns {

// f32 -> u32 whose unsigned order is the order of the floats with -0 < +0 (NaN never gets here)
__host__ __device__ inline uint32_t stats_key(float x) {
	uint32_t b;
	memcpy(&b, &x, 4);
	return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__host__ __device__ inline float stats_unkey(uint32_t k) {
	const uint32_t b = k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu);
	float x;
	memcpy(&x, &b, 4);
	return x;
}
constexpr uint32_t kStatsKeyPosInf = 0xFF800000u, kStatsKeyNegInf = 0x007FFFFFu;  // stats_key(+inf), stats_key(-inf)

// the record of no voxel at all: what pads the tree over leaves
__host__ __device__ inline hns_stats stats_empty() {
	hns_stats e;
	e.count = e.nan_count = 0;
	e.min = stats_unkey(kStatsKeyPosInf), e.max = stats_unkey(kStatsKeyNegInf), e.max_abs = 0.0f;
	e.reserved = 0;
	e.sum = e.sum_sq = 0.0;
	return e;
}

// a += b: one node of either tree
__host__ __device__ inline void stats_combine(hns_stats& a, const hns_stats& b) {
	a.count += b.count, a.nan_count += b.nan_count;
	if (stats_key(b.min) < stats_key(a.min)) a.min = b.min;
	if (stats_key(b.max) > stats_key(a.max)) a.max = b.max;
	if (b.max_abs > a.max_abs) a.max_abs = b.max_abs;
	a.sum = a.sum + b.sum, a.sum_sq = a.sum_sq + b.sum_sq;
}

// The last step: +inf and -inf in one sum make a NaN whose sign and payload the adder chooses (x86 and gfx950 choose differently): stored as 0x7FF8000000000000.
__host__ __device__ inline void stats_finish(hns_stats& a) {
	const uint64_t qnan = 0x7FF8000000000000ull;
	if (a.sum != a.sum) memcpy(&a.sum, &qnan, 8);
	if (a.sum_sq != a.sum_sq) memcpy(&a.sum_sq, &qnan, 8);
}

// the tree over leaves, in place over n >= 1 records (the host's form; the device's k_stats_fold walks the same levels with a workgroup)
inline void stats_fold(hns_stats* t, uint64_t n) {
	for (uint64_t s = 1; s < n; s *= 2)
		for (uint64_t i = 0; i < n; i += 2 * s) stats_combine(t[i], i + s < n ? t[i + s] : stats_empty());
}

}  // namespace hns
