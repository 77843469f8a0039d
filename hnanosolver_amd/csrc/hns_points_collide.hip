// hns_points_collide.hip -- points traced through the velocity that honour a collision SDF: after every step of k_trace_points (rk_step, hns_pointstep.hpp) the SDF is
// sampled at the new position (IndexSampler<float,1>, the sampler of hns_dev_sample_points), and a point that landed in the collider is put back (STOP: the reference's
// rule for a back-trace that ends in the collider, Kernel.cu:144-147), pushed out along the SDF's normal (PUSH: push_out, hns_pointstep.hpp) or frozen and marked dead
// (KILL). One thread per point, the leaf cursor of hns_points.hpp on, no LDS, no atomics; include/hns.h states the arithmetic line by line. -ffp-contract=off.
#include "hns_pointstep.hpp"

using namespace hns;

namespace {

struct CollideDev {
	int mode;  // wave-uniform: the branch on it costs no divergence
	float threshold, skin;
	int iterations;
};

// `steps` steps of a point; after each, d = S(x1) decides: !(d < threshold) -- a NaN included -- takes the step. The push branch holds one float sample at a time (eight
// taps; a stage of the RK step holds 24), so the kernel's register count is the RK step's plus x0, d and the flags. A killed point leaves the loop: its lanes idle until
// the wave's last point is through.
template <int ORDER>
__global__ __launch_bounds__(kPointBlock) void k_trace_points_collide(const GridDev g, const float* __restrict__ u, const float* __restrict__ sdf, float* __restrict__ xyz,
                                                                          const unsigned n, const float s, const float inv_dx, const int steps, const CollideDev c,
                                                                          unsigned char* __restrict__ status, unsigned char* __restrict__ hit) {
	const unsigned p = blockIdx.x * (unsigned)kPointBlock + threadIdx.x;
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
				push_out(S, x1, d, c.threshold, c.skin, inv_dx, c.iterations, [](const f3&) {});
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
	if (status) status[p] = in_a_leaf<true>(g, cur, x, !dead) ? 1 : 0;
}

// Every refusal comes before the first launch, and every refusal of an argument before the grid's device tables are looked at. dx_name: what the caller calls inv_dx.
int trace_points_collide(const char* who, const char* dx_name, hns_grid* g, const float* vel3, const float* sdf, float* xyz, uint64_t n, float dt, float inv_dx, int order,
                         int steps, const hns_point_collision* c, unsigned char* status, unsigned char* hit, void* stream) {
	if (!g) return refuse(who, "null grid");
	if (int rc = check_step_numbers(who, dx_name, order, steps, dt, inv_dx)) return rc;
	if (!c) return refuse(who, "the collision spec is null");
	if (c->mode < HNS_COLLIDE_STOP || c->mode > HNS_COLLIDE_KILL) return refuse(who, "mode must be 1 (stop), 2 (push) or 3 (kill)");
	if (int rc = check_push_numbers(who, c->threshold, c->skin, c->iterations)) return rc;
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
	with_order(order, [&](auto o) {
		hipLaunchKernelGGL(k_trace_points_collide<decltype(o)::value>, point_blocks(n), dim3(kPointBlock), 0, (hipStream_t)stream, g->dev(), vel3, sdf, xyz, (unsigned)n, s, inv_dx, steps, d, status, hit);
	});
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
	float inv_dx;
	if (int rc = inv_voxel_size(who, voxel_size, &inv_dx)) return rc;
	const int k = s->find("collision_sdf");
	if (k < 0) return refuse(who, "no float field named 'collision_sdf' in this sim");
	return trace_points_collide(who, "1 / voxel_size", s->grid, s->vel, s->cur[k], xyz, n, dt, inv_dx, order, steps, c, status, hit, stream);
}

}  // extern "C"
