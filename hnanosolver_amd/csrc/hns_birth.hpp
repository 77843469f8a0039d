// hns_birth.hpp -- points born from a field (include/hns.h: "BIRTH AND DEATH OF POINTS" states the rule): the hash, the draws, the count of a voxel and the position of a
// birth, stated once for the kernels of hns_population.hip and the host mirror hns_grid_birth_points (hns_leafio.cpp), so that the two cannot drift. Every line is one
// rounded float32 operation (-ffp-contract=off); the integer arithmetic is uint32, wrapping.
#pragma once

#include <cmath>

#include "hns_internal.hpp"

namespace hns {

constexpr uint32_t kBirthMaxPerVoxel = 16;
constexpr uint32_t kBirthNaN = 0x7FC00000u, kBirthNoVoxel = 0xFFFFFFFFu;  // what a filled row of xyz / of voxel holds

// H
HNS_HD uint32_t birth_hash(uint32_t x) {
	x ^= x >> 16;
	x *= 0x7feb352du;
	x ^= x >> 15;
	x *= 0x846ca68bu;
	x ^= x >> 16;
	return x;
}

// h of the voxel (i, j, k): its global coordinates and the seed only
HNS_HD uint32_t birth_voxel_hash(uint32_t seed, int i, int j, int k) {
	return birth_hash(birth_hash(birth_hash(birth_hash(seed ^ 0x9E3779B9u) ^ (uint32_t)i) ^ (uint32_t)j) ^ (uint32_t)k);
}

// U(d): a multiple of 2^-24 in [0, 1), exact
HNS_HD float birth_uniform(uint32_t h, uint32_t d) { return (float)(birth_hash(h + d) >> 8) * 0x1p-24f; }

// may a voxel with this coordinate bear points? (every birth then meets the seeds' condition: its position is below c + 1 <= 8388607)
HNS_HD bool birth_coordinate(int c) { return -8388608 <= c && c <= 8388606; }

// the spec's refusals, for the device call and the mirror alike: null, or what is wrong
inline const char* birth_spec_refusal(const hns_birth_spec* sp) {
	if (!sp) return "null spec";
	if (sp->max_per_voxel < 1 || sp->max_per_voxel > kBirthMaxPerVoxel) return "max_per_voxel is outside 1 .. 16";
	if (!std::isfinite(sp->threshold)) return "threshold is not finite";
	if (!std::isfinite(sp->rate) || !(sp->rate > 0.0f)) return "rate is not a positive finite number";
	return nullptr;
}

// c of the voxel (i, j, k) holding v; unmasked: no masks, or the voxel's bit is set. *h: the voxel's hash, for its positions (set where c > 0)
HNS_HD uint32_t birth_count(float v, bool unmasked, int i, int j, int k, const hns_birth_spec& sp, uint32_t* h) {
	if (!(unmasked && v > sp.threshold && birth_coordinate(i) && birth_coordinate(j) && birth_coordinate(k))) return 0;
	*h = birth_voxel_hash(sp.seed, i, j, k);
	const float scaled = v * sp.rate;
	const float m = fmaxf(0.0f, fminf(scaled, (float)sp.max_per_voxel));
	const uint32_t b = (uint32_t)m;
	const float f = m - (float)b;
	return b + (birth_uniform(*h, 0) < f ? 1u : 0u);
}

// nextafterf(top, -inf) of a finite top
HNS_HD float birth_below(float top) {
	uint32_t u;
	__builtin_memcpy(&u, &top, 4);
	u = top > 0.0f ? u - 1u : (top < 0.0f ? u + 1u : 0x80000001u);
	float r;
	__builtin_memcpy(&r, &u, 4);
	return r;
}

// coordinate a of birth q of a voxel whose coordinate along that axis is i: Floor of it is i
HNS_HD float birth_position(int i, uint32_t h, uint32_t q, int a) {
	const float top = (float)(i + 1);
	const float p = (float)i + birth_uniform(h, 1u + 3u * q + (uint32_t)a);
	return p < top ? p : birth_below(top);
}

}  // namespace hns
