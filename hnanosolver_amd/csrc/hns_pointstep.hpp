// hns_pointstep.hpp -- what the three kernels that move points through a sim share, each stated once: hns_points.hip (k_trace_points: points traced through the velocity),
// hns_points_collide.hip (k_trace_points_collide: the same against a collision SDF) and hns_point_motion.hip (k_move_points: points with a velocity of their own). The
// Runge-Kutta step, the push out of the collider along the SDF's normal, the status rule, the hit bits, the block size and the refusals of the numbers the launchers share.
// No other file includes it: the splat, rasterise, order and neighbour files do not depend on a line here.
#pragma once

#include <cmath>
#include <type_traits>

#include "hns_points.hpp"

namespace hns {

constexpr int kPointBlock = 256;

// what hit holds (include/hns.h); hns_point_motion.hip calls bit 1 "bounced" and adds a bit 16 of its own
constexpr unsigned kHitPushed = 1, kHitReverted = 2, kHitKilled = 4, kHitStartInside = 8;

// One step x' = x + s U(x) at ORDER: 1 forward Euler, 2 the midpoint rule, 4 the classical Runge-Kutta step. U is the Vec3f sampler, s = dt * inv_dx, h = 0.5f * s,
// s6 = s * 0.16666667f. Every a + c*b is a multiply, then an add.
template <int ORDER, class Sampler>
__device__ __forceinline__ f3 rk_step(Sampler& U, const f3 x, const float s, const float h, const float s6) {
	const f3 k1 = U(x.x, x.y, x.z);
	if (ORDER == 1) return f3{x.x + s * k1.x, x.y + s * k1.y, x.z + s * k1.z};
	const f3 k2 = U(x.x + h * k1.x, x.y + h * k1.y, x.z + h * k1.z);
	if (ORDER == 2) return f3{x.x + s * k2.x, x.y + s * k2.y, x.z + s * k2.z};
	f3 sum = {k1.x + 2.0f * k2.x, k1.y + 2.0f * k2.y, k1.z + 2.0f * k2.z};
	const f3 k3 = U(x.x + h * k2.x, x.y + h * k2.y, x.z + h * k2.z);
	sum = f3{sum.x + 2.0f * k3.x, sum.y + 2.0f * k3.y, sum.z + 2.0f * k3.z};
	const f3 k4 = U(x.x + s * k3.x, x.y + s * k3.y, x.z + s * k3.z);
	sum = f3{sum.x + k4.x, sum.y + k4.y, sum.z + k4.z};
	return f3{x.x + s6 * sum.x, x.y + s6 * sum.y, x.z + s6 * sum.z};
}

// The push of a position x1 with d = S(x1) < threshold out of the collider: up to `iterations` times, while d < threshold, the SDF's normal from six samples one voxel
// either side, a move of (threshold - d) * inv_dx + skin along it, and d again. first(nrm) runs on iteration 0 only (k_move_points reflects its velocity there). The six
// samples run through ONE rolled sampler body with the results selected into registers: unrolled, the compiler issues all 48 taps together and a kernel needs about 150
// registers (three waves per SIMD) whatever share of the points ever pushes.
template <class Sampler, class First>
__device__ __forceinline__ void push_out(Sampler& S, f3& x1, float& d, const float threshold, const float skin, const float inv_dx, const int iterations, First first) {
#pragma unroll 1
	for (int it = 0; it < iterations && d < threshold; ++it) {
		float nb[6] = {};
#pragma unroll 1
		for (int q = 0; q < 6; ++q) {  // -x, +x, -y, +y, -z, +z: one sample's taps in flight (x + -1.0f is x - 1.0f)
			const float off = (q & 1) ? 1.0f : -1.0f;
			const int axis = q >> 1;
			const float v = S(axis == 0 ? x1.x + off : x1.x, axis == 1 ? x1.y + off : x1.y, axis == 2 ? x1.z + off : x1.z);
#pragma unroll
			for (int e = 0; e < 6; ++e) nb[e] = q == e ? v : nb[e];  // (selects: nb stays in registers)
		}
		const f3 nrm = sdf_normal_of(nb, inv_dx);
		if (it == 0) first(nrm);
		float a = (threshold - d) * inv_dx;
		a = a + skin;
		x1 = f3{x1.x + a * nrm.x, x1.y + a * nrm.y, x1.z + a * nrm.z};
		d = S(x1.x, x1.y, x1.z);
	}
}

// status: is a point that is `alive` by its kernel's own rule at a finite position whose cell's leaf exists?
template <bool CURSOR>
__device__ __forceinline__ bool in_a_leaf(const GridDev& g, Cursor& cur, const f3 x, const bool alive) {
	// (&, on ints: one test; with && and a branch per term k_move_points<false> takes three more registers)
	bool in = (int)alive & (int)finite_f(x.x) & (int)finite_f(x.y) & (int)finite_f(x.z);
	if (in) {
		int L[8];
		const int i = __float2int_rd(x.x), j = __float2int_rd(x.y), k = __float2int_rd(x.z);
		cell_leaves<CURSOR>(g, cur, i & ~7, j & ~7, k & ~7, L);  // (the leaf's own corner: one lookup)
		in = L[0] >= 0;
	}
	return in;
}

// ---- launcher plumbing ----

inline dim3 point_blocks(uint64_t n) { return dim3((unsigned)((n + kPointBlock - 1) / kPointBlock)); }

// a run-time order (1, 2 or 4: check_step_numbers) as a template argument: launch(std::integral_constant<int, ORDER>)
template <class Launch>
inline void with_order(int order, Launch launch) {
	switch (order) {
	case 1: launch(std::integral_constant<int, 1>{}); break;
	case 2: launch(std::integral_constant<int, 2>{}); break;
	default: launch(std::integral_constant<int, 4>{}); break;
	}
}

// the numbers of a trace. dx_name: what the caller calls inv_dx
inline int check_step_numbers(const char* who, const char* dx_name, int order, int steps, float dt, float inv_dx) {
	if (order != 1 && order != 2 && order != 4) return refuse(who, "order must be 1, 2 or 4");
	if (steps < 1) return refuse(who, "steps must be at least 1");
	if (std::isnan(dt)) return refuse(who, "dt is NaN");
	if (!(inv_dx > 0.0f) || std::isinf(inv_dx)) {
		set_error("%s: %s must be a positive finite number", who, dx_name);
		return HNS_ERR_INVALID_ARGUMENT;
	}
	return HNS_OK;
}

// the numbers of a push
inline int check_push_numbers(const char* who, float threshold, float skin, int iterations) {
	if (!std::isfinite(threshold)) return refuse(who, "threshold must be finite");
	if (!std::isfinite(skin) || skin < 0.0f) return refuse(who, "skin must be finite and not negative");
	if (iterations < 1 || iterations > 8) return refuse(who, "iterations must be 1 .. 8");
	return HNS_OK;
}

// a sim call's voxel_size as the kernels' inv_dx
inline int inv_voxel_size(const char* who, float voxel_size, float* inv_dx) {
	if (!(voxel_size > 0.0f) || std::isinf(voxel_size)) return refuse(who, "voxel_size must be a positive finite number");
	*inv_dx = 1.0f / voxel_size;
	return HNS_OK;
}

}  // namespace hns
