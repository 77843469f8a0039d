// hns_point_motion.hip -- points with a velocity of their own: an object that owns the per-point state (position, velocity, age, status, hit; one block of the pool) and
// the kernel that steps it through a sim's fluid: drag towards the gas (implicit Euler), gravity, the move, and the collision SDF's answer to a step that lands in the
// collider -- stick, bounce (reflect the velocity about the SDF's normal, then the collision trace's push) or kill. The samplers and the leaf cursor are those of
// hns_points.hpp; the push (push_out, which hands the reflection its normal), the status rule and the hit bits those of hns_pointstep.hpp, as k_trace_points_collide
// (hns_points_collide.hip) uses them; include/hns.h states the arithmetic line by line. One thread per point, no LDS, no atomics. -ffp-contract=off.
#include "hns_pointstep.hpp"

using namespace hns;

namespace {

// what hit holds beside the bits of hns_pointstep.hpp (include/hns.h)
constexpr unsigned kHitBounced = kHitPushed, kHitReflected = 16;

// the host's constants of one call (include/hns.h: "Host constants"), by value: wave-uniform, so the branches on mode and empty cost no divergence
struct MotionDev {
	int mode, iterations;
	int empty;  // the grid has no leaves: U = 0 and S = 0 everywhere, no leaf exists
	float inv_dx, s, k, r, dt, gdx, gdy, gdz, restitution, ft, max_age, threshold, skin;
};

// `steps` steps of a point. COLLIDE = false is mode FREE: S is not in the kernel at all. The bounce holds one float sample at a time (the rolled sampler body of
// push_out); x, v and age are written once, behind the last step. A killed point leaves the loop.
template <bool COLLIDE>
__global__ __launch_bounds__(kPointBlock) void k_move_points(const GridDev g, const float* __restrict__ u, const float* __restrict__ sdf, float* __restrict__ xyz,
                                                               float* __restrict__ vel, float* __restrict__ age, const unsigned n, const int steps, const MotionDev c,
                                                               unsigned char* __restrict__ status, unsigned char* __restrict__ hit) {
	const unsigned p = blockIdx.x * (unsigned)kPointBlock + threadIdx.x;
	if (p >= n) return;
	f3 x = ld3(xyz, (int)p);
	if (!(finite_f(x.x) && finite_f(x.y) && finite_f(x.z))) {  // a row that holds no point (PointPopulation's rows beyond the live count): every bit stays
		status[p] = 0;
		hit[p] = 0;
		return;
	}
	f3 v = ld3(vel, (int)p);
	float a = age[p];
	Cursor cur{-1, 0, 0, 0};
	auto U = [&](float q, float b, float e) { return c.empty ? f3{0.0f, 0.0f, 0.0f} : sample_v(u, point_cell<true>(g, cur, q, b, e)); };
	auto S = [&](float q, float b, float e) { return c.empty ? 0.0f : sample_f(sdf, point_cell<true>(g, cur, q, b, e)); };
	unsigned flags = 0;
	if (COLLIDE) flags = S(x.x, x.y, x.z) < c.threshold ? kHitStartInside : 0u;
	bool dead = false;
	for (int step = 0; step < steps; ++step) {
		const f3 w = U(x.x, x.y, x.z);
		f3 t = {c.k * w.x, c.k * w.y, c.k * w.z};  // drag, implicit Euler
		t = f3{v.x + t.x, v.y + t.y, v.z + t.z};
		v = f3{t.x * c.r, t.y * c.r, t.z * c.r};
		v = f3{v.x + c.gdx, v.y + c.gdy, v.z + c.gdz};  // gravity
		const f3 m = {c.s * v.x, c.s * v.y, c.s * v.z};  // the move
		f3 x1 = {x.x + m.x, x.y + m.y, x.z + m.z};
		a = a + c.dt;
		if (COLLIDE) {
			float d = S(x1.x, x1.y, x1.z);
			if (d < c.threshold) {
				if (c.mode == HNS_MOTION_KILL) {
					flags |= kHitKilled;
					dead = true;
					x = x1;
					break;
				}
				if (c.mode == HNS_MOTION_STICK) {
					flags |= kHitReverted;
					v = f3{0.0f, 0.0f, 0.0f};
					x1 = x;
				} else {
					flags |= kHitBounced;
					push_out(S, x1, d, c.threshold, c.skin, c.inv_dx, c.iterations, [&](const f3& nrm) {  // reflect the velocity, once a step
						const float vn = (v.x * nrm.x + v.y * nrm.y) + v.z * nrm.z;
						if (vn < 0.0f) {
							const f3 wn = {vn * nrm.x, vn * nrm.y, vn * nrm.z};
							const f3 vt = {v.x - wn.x, v.y - wn.y, v.z - wn.z};
							const float b = c.restitution * vn;
							const f3 pt = {c.ft * vt.x, c.ft * vt.y, c.ft * vt.z};
							const f3 qn = {b * nrm.x, b * nrm.y, b * nrm.z};
							v = f3{pt.x - qn.x, pt.y - qn.y, pt.z - qn.z};
							flags |= kHitReflected;
						}
					});
					if (d < c.threshold) {  // a push that did not get out: the reflected velocity stays
						flags |= kHitReverted;
						x1 = x;
					}
				}
			}
		}
		x = x1;
	}
	st3(xyz, (int)p, x);
	st3(vel, (int)p, v);
	age[p] = a;
	hit[p] = (unsigned char)flags;
	status[p] = in_a_leaf<true>(g, cur, x, !dead && a < c.max_age && !c.empty) ? 1 : 0;
}

}  // namespace

struct hns_point_motion {
	int device = -1;
	uint64_t capacity = 0;
	hipStream_t stream = nullptr;
	// one pooled allocation: the five per-point arrays
	Pooled arena;
	float *xyz = nullptr, *vel = nullptr, *age = nullptr;
	unsigned char *status = nullptr, *hit = nullptr;
};

extern "C" {

hns_point_motion* hns_point_motion_create(uint64_t capacity, int* err) {
	return make_object<hns_point_motion>("hns_point_motion_create", err, false, nullptr, capacity, "", [&](hns_point_motion* o) {
		o->capacity = capacity;
		const size_t cap = (size_t)std::max<uint64_t>(capacity, 1);
		return carve(o->arena, o->device, [&](const Slice& slice) {
			slice(o->xyz, 12 * cap), slice(o->vel, 12 * cap), slice(o->age, 4 * cap), slice(o->status, cap), slice(o->hit, cap);
		});
	});
}

void hns_point_motion_destroy(hns_point_motion* o) {
	if (!o) return;
	delete o;  // (its block goes back to the pool, which waits for the device first)
}

int hns_point_motion_set_stream(hns_point_motion* o, void* hip_stream) { return set_object_stream(o, hip_stream, "hns_point_motion_set_stream", "null point motion"); }

int hns_point_motion_get(hns_point_motion* o, hns_point_motion_info* info) {
	if (!o) return refuse("hns_point_motion_get", "null point motion");
	if (!info) return refuse("hns_point_motion_get", "null info");
	*info = hns_point_motion_info{o->capacity, o->xyz, o->vel, o->age, o->status, o->hit};
	return HNS_OK;
}

// Reads the sim's current velocity and collision_sdf and nothing else of it: the look-ahead memo, the masks, the feedback signatures and the solve report stay as they are.
int hns_point_motion_step(hns_point_motion* o, hns_sim* s, uint64_t n, float dt, float voxel_size, int steps, const hns_point_motion_spec* sp) {
	const char* who = "hns_point_motion_step";
	// the numbers and the spec, a host struct, first: they are refused whatever the objects are, a machine without a device included
	if (!sp) return refuse(who, "the spec is null");
	if (n > kMaxPoints) return refuse(who, "n is above 2^31 - 1");
	if (steps < 1) return refuse(who, "steps must be at least 1");
	if (std::isnan(dt)) return refuse(who, "dt is NaN");
	float inv_dx;
	if (int rc = inv_voxel_size(who, voxel_size, &inv_dx)) return rc;
	if (sp->mode < HNS_MOTION_FREE || sp->mode > HNS_MOTION_KILL) return refuse(who, "mode must be 0 (free), 1 (stick), 2 (bounce) or 3 (kill)");
	for (int a = 0; a < 3; ++a)
		if (!std::isfinite(sp->gravity[a])) return refuse(who, "gravity must be finite");
	if (!std::isfinite(sp->drag) || sp->drag < 0.0f) return refuse(who, "drag must be finite and not negative");
	if (!(sp->restitution >= 0.0f && sp->restitution <= 1.0f)) return refuse(who, "restitution must be in [0, 1]");
	if (!(sp->friction >= 0.0f && sp->friction <= 1.0f)) return refuse(who, "friction must be in [0, 1]");
	if (!(sp->max_age > 0.0f)) return refuse(who, "max_age must be positive (+inf: no point expires)");
	if (int rc = check_push_numbers(who, sp->threshold, sp->skin, sp->iterations)) return rc;
	if (!o) return refuse(who, "null point motion");
	HNS_TRY(check_capacity(who, n, o->capacity));
	if (int rc = check_sim(s, who)) return rc;
	const int f = sp->mode == HNS_MOTION_FREE ? -1 : s->find("collision_sdf");
	if (sp->mode != HNS_MOTION_FREE && f < 0) return refuse(who, "no float field named 'collision_sdf' in this sim (mode free needs none)");
	if (n == 0) return HNS_OK;
	hns_grid* g;
	HNS_TRY(sim_grid(who, s, o->device, "point motion", false, &g));  // (not sized: the kernel addresses the sim's buffers through the grid's tables, point by point)
	MotionDev d;
	d.mode = sp->mode, d.iterations = sp->iterations, d.empty = g->topo.n_leaves == 0;
	d.inv_dx = inv_dx;
	d.s = dt * d.inv_dx;
	d.k = sp->drag * dt;
	d.r = 1.0f / (1.0f + d.k);
	d.dt = dt;
	d.gdx = dt * sp->gravity[0], d.gdy = dt * sp->gravity[1], d.gdz = dt * sp->gravity[2];
	d.restitution = sp->restitution;
	d.ft = 1.0f - sp->friction;
	d.max_age = sp->max_age, d.threshold = sp->threshold, d.skin = sp->skin;
	const dim3 grid = point_blocks(n), block(kPointBlock);
	if (sp->mode == HNS_MOTION_FREE)
		hipLaunchKernelGGL(k_move_points<false>, grid, block, 0, o->stream, g->dev(), (const float*)s->vel, (const float*)nullptr, o->xyz, o->vel, o->age, (unsigned)n, steps, d,
		                   o->status, o->hit);
	else
		hipLaunchKernelGGL(k_move_points<true>, grid, block, 0, o->stream, g->dev(), (const float*)s->vel, (const float*)s->cur[(size_t)f], o->xyz, o->vel, o->age, (unsigned)n,
		                   steps, d, o->status, o->hit);
	return launch_status(who);
}

}  // extern "C"
