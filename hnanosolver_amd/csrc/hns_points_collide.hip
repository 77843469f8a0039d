// hns_points_collide.hip -- points traced through the velocity that honour a collision SDF: after every step of k_trace_points' arithmetic the SDF is sampled at the new
// position (IndexSampler<float,1>, the sampler of hns_dev_sample_points), and a point that landed in the collider is put back (STOP: the reference's rule for a back-trace
// that ends in the collider, Kernel.cu:144-147), pushed out along the SDF's normal (PUSH) or frozen and marked dead (KILL). One thread per point, the leaf cursor of
// hns_points.hpp on, no LDS, no atomics; include/hns.h states the arithmetic line by line. -ffp-contract=off.
#include "hns_points.hpp"

#include <cmath>

using namespace hns;

namespace {

constexpr int kCollideBlock = 256;

// what hit holds (include/hns.h)
constexpr unsigned kHitPushed = 1, kHitReverted = 2, kHitKilled = 4, kHitStartInside = 8;

struct CollideDev {
	int mode;  // wave-uniform: the branch on it costs no divergence
	float threshold, skin;
	int iterations;
};

// One step of k_trace_points (hns_points.hip) at ORDER, with exactly its operations: U is its sampler, s = dt * inv_dx, h = 0.5f * s, s6 = s * 0.16666667f.
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

// `steps` steps of a point; after each, d = S(x1) decides: !(d < threshold) -- a NaN included -- takes the step. The push branch holds one float sample at a time (eight
// taps; a stage of the RK step holds 24), so the kernel's register count is the RK step's plus x0, d and the flags. A killed point leaves the loop: its lanes idle until
// the wave's last point is through.
template <int ORDER>
__global__ __launch_bounds__(kCollideBlock) void k_trace_points_collide(const GridDev g, const float* __restrict__ u, const float* __restrict__ sdf, float* __restrict__ xyz,
                                                                          const unsigned n, const float s, const float inv_dx, const int steps, const CollideDev c,
                                                                          unsigned char* __restrict__ status, unsigned char* __restrict__ hit) {
	const unsigned p = blockIdx.x * (unsigned)kCollideBlock + threadIdx.x;
	if (p >= n) return;
	f3 x = ld3(xyz, (int)p);
	const float h = 0.5f * s, s6 = s * 0.16666667f;
	Cursor cur{-1, 0, 0, 0};
	auto U = [&](float a, float b, float e) { return sample_v(u, point_cell<true>(g, cur, a, b, e)); };
	auto S = [&](float a, float b, float e) { return sample_f(sdf, point_cell<true>(g, cur, a, b, e)); };
	unsigned flags = S(x.x, x.y, x.z) < c.threshold ? kHitStartInside : 0u;
	bool dead = false;
	for (int step = 0; step < steps; ++step) {
		f3 x1 = rk_step<ORDER>(U, x, s, h, s6);
		float d = S(x1.x, x1.y, x1.z);
		if (d < c.threshold) {
			if (c.mode == HNS_COLLIDE_KILL) {
				flags |= kHitKilled;
				dead = true;
				x = x1;
				break;
			}
			if (c.mode == HNS_COLLIDE_PUSH) {
				flags |= kHitPushed;
#pragma unroll 1
				for (int it = 0; it < c.iterations && d < c.threshold; ++it) {
					float nb[6] = {};
#pragma unroll 1
					for (int q = 0; q < 6; ++q) {  // -x, +x, -y, +y, -z, +z: ONE sampler body in the code, one sample's taps in flight (x + -1.0f is x - 1.0f)
						const float off = (q & 1) ? 1.0f : -1.0f;
						const int axis = q >> 1;
						const float v = S(axis == 0 ? x1.x + off : x1.x, axis == 1 ? x1.y + off : x1.y, axis == 2 ? x1.z + off : x1.z);
#pragma unroll
						for (int e = 0; e < 6; ++e) nb[e] = q == e ? v : nb[e];  // (selects: nb stays in registers)
					}
					const f3 nrm = sdf_normal_of(nb, inv_dx);
					float a = (c.threshold - d) * inv_dx;
					a = a + c.skin;
					x1 = f3{x1.x + a * nrm.x, x1.y + a * nrm.y, x1.z + a * nrm.z};
					d = S(x1.x, x1.y, x1.z);
				}
			}
			if (d < c.threshold) {  // STOP, or a push that did not get out
				flags |= kHitReverted;
				x1 = x;
			}
		}
		x = x1;
	}
	st3(xyz, (int)p, x);
	if (hit) hit[p] = (unsigned char)flags;
	if (status) {
		int L[8];
		const int i = __float2int_rd(x.x), j = __float2int_rd(x.y), k = __float2int_rd(x.z);
		bool in = !dead && finite_f(x.x) && finite_f(x.y) && finite_f(x.z);
		if (in) {
			cell_leaves<true>(g, cur, i & ~7, j & ~7, k & ~7, L);  // (the leaf's own corner: one lookup)
			in = L[0] >= 0;
		}
		status[p] = in ? 1 : 0;
	}
}

// Every refusal comes before the first launch, and every refusal of an argument before the grid's device tables are looked at. dx_name: what the caller calls inv_dx.
int trace_points_collide(const char* who, const char* dx_name, hns_grid* g, const float* vel3, const float* sdf, float* xyz, uint64_t n, float dt, float inv_dx, int order,
                         int steps, const hns_point_collision* c, unsigned char* status, unsigned char* hit, void* stream) {
	if (!g) return refuse(who, "null grid");
	if (order != 1 && order != 2 && order != 4) return refuse(who, "order must be 1, 2 or 4");
	if (steps < 1) return refuse(who, "steps must be at least 1");
	if (std::isnan(dt)) return refuse(who, "dt is NaN");
	if (!(inv_dx > 0.0f) || std::isinf(inv_dx)) {
		set_error("%s: %s must be a positive finite number", who, dx_name);
		return HNS_ERR_INVALID_ARGUMENT;
	}
	if (!c) return refuse(who, "the collision spec is null");
	if (c->mode < HNS_COLLIDE_STOP || c->mode > HNS_COLLIDE_KILL) return refuse(who, "mode must be 1 (stop), 2 (push) or 3 (kill)");
	if (!std::isfinite(c->threshold)) return refuse(who, "threshold must be finite");
	if (!std::isfinite(c->skin) || c->skin < 0.0f) return refuse(who, "skin must be finite and not negative");
	if (c->iterations < 1 || c->iterations > 8) return refuse(who, "iterations must be 1 .. 8");
	if (n > kMaxPoints) return refuse(who, "n is above 2^31 - 1");
	if (n == 0) return HNS_OK;  // (no point, no device pointer looked at; the numbers and the spec, a host struct, are checked whatever n, as hns_dev_trace_points checks order and steps)
	if (!xyz) return refuse(who, "xyz is null");
	if (!vel3) return refuse(who, "vel3 is null");
	if (!sdf) return refuse(who, "sdf is null");
	const void* buf[5] = {xyz, vel3, sdf, status, hit};
	const char* name[5] = {"xyz", "vel3", "sdf", "status", "hit"};
	for (int a = 1; a < 5; ++a)
		for (int b = 0; b < a; ++b)
			if (buf[a] && buf[a] == buf[b]) {
				set_error("%s: %s is %s (xyz, vel3, sdf, status and hit must be different buffers)", who, name[a], name[b]);
				return HNS_ERR_INVALID_ARGUMENT;
			}
	if (int rc = check_grid(g, who)) return rc;
	if (g->topo.n_leaves == 0) {  // no leaf: U = 0 and S = 0 everywhere, nothing moves, nothing is inside
		if (status) HNS_HIP(hipMemsetAsync(status, 0, n, (hipStream_t)stream));
		if (hit) HNS_HIP(hipMemsetAsync(hit, 0, n, (hipStream_t)stream));
		return HNS_OK;
	}
	const float s = dt * inv_dx;
	const CollideDev d{c->mode, c->threshold, c->skin, c->iterations};
	const dim3 grid((unsigned)((n + kCollideBlock - 1) / kCollideBlock)), block(kCollideBlock);
	switch (order) {
	case 1: hipLaunchKernelGGL(k_trace_points_collide<1>, grid, block, 0, (hipStream_t)stream, g->dev(), vel3, sdf, xyz, (unsigned)n, s, inv_dx, steps, d, status, hit); break;
	case 2: hipLaunchKernelGGL(k_trace_points_collide<2>, grid, block, 0, (hipStream_t)stream, g->dev(), vel3, sdf, xyz, (unsigned)n, s, inv_dx, steps, d, status, hit); break;
	default: hipLaunchKernelGGL(k_trace_points_collide<4>, grid, block, 0, (hipStream_t)stream, g->dev(), vel3, sdf, xyz, (unsigned)n, s, inv_dx, steps, d, status, hit); break;
	}
	return launch_status(who);
}

}  // namespace

extern "C" {

int hns_dev_trace_points_collide(hns_grid* g, const float* vel3, const float* sdf, float* xyz, uint64_t n, float dt, float inv_dx, int order, int steps,
                                 const hns_point_collision* c, unsigned char* status, unsigned char* hit, void* stream) {
	return trace_points_collide("hns_dev_trace_points_collide", "inv_dx", g, vel3, sdf, xyz, n, dt, inv_dx, order, steps, c, status, hit, stream);
}

// Reads the sim's current velocity and collision_sdf and nothing else of it: the look-ahead memo, the masks, the feedback signatures and the solve report stay as they are.
int hns_sim_trace_points_collide(hns_sim* s, float* xyz, uint64_t n, float dt, float voxel_size, int order, int steps, const hns_point_collision* c, unsigned char* status,
                                 unsigned char* hit, void* stream) {
	const char* who = "hns_sim_trace_points_collide";
	if (int rc = check_sim(s, who)) return rc;
	if (!(voxel_size > 0.0f) || std::isinf(voxel_size)) return refuse(who, "voxel_size must be a positive finite number");
	const int k = s->find("collision_sdf");
	if (k < 0) return refuse(who, "no float field named 'collision_sdf' in this sim");
	return trace_points_collide(who, "1 / voxel_size", s->grid, s->vel, s->cur[k], xyz, n, dt, 1.0f / voxel_size, order, steps, c, status, hit, stream);
}

}  // extern "C"
