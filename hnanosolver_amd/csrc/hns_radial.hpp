// hns_radial.hpp -- the weight of the radial footprint and the fixed-point total, the two pieces of the splat's arithmetic (hns_points.hpp states the rest) that host code
// compiled without hipcc shares with the kernels: hns_points.hpp includes this file for the kernel files, hns_neighbours.hpp for hns_leafio.cpp. -ffp-contract=off: every
// line is one rounded operation; include/hns.h states them in words (hns_splat_spec: "Weight", hns_dev_splat_points: "Finish").
#pragma once

#include "hns_internal.hpp"

namespace hns {

__host__ __device__ inline float radial_inv(float r) {
	const float r2 = r * r;
	return 1.0f / r2;
}
// the weight of the candidate (dx, dy, dz) away from the point; false: it is not in the footprint
__host__ __device__ inline bool radial_weight(float dx, float dy, float dz, float inv, float* w) {
	const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
	const float xy = xx + yy;
	const float d2 = xy + zz;
	const float q = d2 * inv;
	if (!(q < 1.0f)) return false;
	const float a = 1.0f - q;
	*w = a * a;
	return true;
}

// what a non-zero accumulator adds to its voxel: quantum = 2^Q
__host__ __device__ inline float splat_total(unsigned long long a, double quantum) { return (float)((double)(long long)a * quantum); }

}  // namespace hns
