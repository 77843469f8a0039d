// hns_neighbours.hpp -- the arithmetic of a point's neighbourhood (include/hns.h: "POINT NEIGHBOURHOODS THROUGH A LEAF ORDER" states it in words), stated once for the
// kernels of hns_neighbours.hip and the host mirror hns_grid_point_neighbours (hns_leafio.cpp): the box of cells a point looks into, the term of one pair, the finish.
// The weight is the radial splat's (hns_radial.hpp: radial_inv, radial_weight), the sums are its int64 multiples of 2^-32 and the finish its splat_total, so that a
// result depends neither on the order pairs are met in nor on how they are split over lanes. -ffp-contract=off: every line is one rounded operation.
#pragma once

#include <cmath>

#include "hns_radial.hpp"

namespace hns {

constexpr float kNeighbourMaxRadius = 2.0f;
constexpr double kNeighbourScale = 0x1p32, kNeighbourQuantum = 0x1p-32;
// cells of a box along one axis: 5 by the real numbers (h <= 2); 6 where x + h rounds up to the next integer. Never more than two leaves
constexpr int kNeighbourMaxExtent = 6;

// is h a radius the query takes? (a NaN fails)
__host__ __device__ inline bool neighbour_radius(float h) { return 0.0f < h && h <= kNeighbourMaxRadius; }

// the box along one axis of a point that takes part (its coordinate seeds: both floors are exact and fit an int): cells lo .. hi
__host__ __device__ inline void neighbour_box(float c, float h, int* lo, int* hi) {
	const float low = c - h, high = c + h;
	*lo = (int)floorf(low);
	*hi = (int)floorf(high);
}

// a term as a multiple of 2^-32, ties to even: |t| is about 1 at most, so nothing is refused
__host__ __device__ inline long long neighbour_term(float t) {
	const double x = (double)t * kNeighbourScale;  // (exact: a power of two)
#ifdef __HIP_DEVICE_COMPILE__
	return __double2ll_rn(x);
#else
	return (long long)std::nearbyint(x);  // (the default rounding mode)
#endif
}

// what one point gathers from its neighbours: a count and four sums modulo 2^64
struct NeighbourSums {
	unsigned count = 0;
	unsigned long long w = 0, px = 0, py = 0, pz = 0;
};

// the pair (i, j), j a candidate from i's box: d = x_i - x_j per axis. A coincident pair (d2 == 0) counts with w = 1 and pushes nowhere
__host__ __device__ inline void neighbour_pair(float xi, float yi, float zi, float xj, float yj, float zj, float inv, NeighbourSums& s) {
	const float dx = xi - xj, dy = yi - yj, dz = zi - zj;
	float w;
	if (!radial_weight(dx, dy, dz, inv, &w)) return;
	++s.count;
	s.w += (unsigned long long)neighbour_term(w);
	const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
	const float xy = xx + yy;
	const float d2 = xy + zz;  // (radial_weight's own d2)
	if (!(d2 > 0.0f)) return;
	const float d = sqrtf(d2);
	const float g = w / d;
	const float tx = dx * g, ty = dy * g, tz = dz * g;
	s.px += (unsigned long long)neighbour_term(tx);
	s.py += (unsigned long long)neighbour_term(ty);
	s.pz += (unsigned long long)neighbour_term(tz);
}

// the finish of one sum: +0.0f for an empty one
__host__ __device__ inline float neighbour_total(unsigned long long a) { return splat_total(a, kNeighbourQuantum); }

}  // namespace hns
