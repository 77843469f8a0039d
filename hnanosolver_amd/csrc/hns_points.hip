// hns_points.hip -- fields sampled at arbitrary positions and points traced through the velocity: the reference's samplers IndexSampler<float,1> /
// IndexSampler<Vec3f,1> (src/Utils/Stencils.hpp:96-173) behind its Floor (Stencils.hpp:25-43), at positions that are no voxel centres. One thread per point, plain
// 64-bit addressed loads (a point's taps may lie anywhere: the leaf-sized buffer descriptors of hns_advect.hip do not apply), no LDS. Positions are INDEX-SPACE
// float triples, AoS n x 3, as the samplers and the advection kernels' back-traced `pos` have them. Arithmetic keeps the reference's association; -ffp-contract=off.
// The trace's RK step, its status rule, the block size and the refusals of its numbers: hns_pointstep.hpp, shared with hns_points_collide.hip and hns_point_motion.hip.
#include "hns_pointstep.hpp"

using namespace hns;

namespace {

constexpr int kMaxPointFields = 8;  // fields that share one launch of k_sample_points

struct PointFields {
	const float* in[kMaxPointFields];
	float* out[kMaxPointFields];
	int n;
	unsigned vec3;  // bit q: field q is Vec3f AoS
};

// the cell under a position, its tap indices and fractions (Cell, Cursor, point_cell): hns_points.hpp, shared with hns_splat.hip

// (ldz, sample_f, sample_v -- the two samplers over a Cell: hns_points.hpp, shared with hns_points_collide.hip)

// Up to eight fields, float or Vec3f, at n positions: one Floor, one set of tap indices and fractions for all of them. Output q is what a launch with field q alone gives.
__global__ __launch_bounds__(kPointBlock) void k_sample_points(const GridDev g, const PointFields P, const float* __restrict__ xyz, const unsigned n) {
	const unsigned p = blockIdx.x * (unsigned)kPointBlock + threadIdx.x;
	if (p >= n) return;
	const f3 pos = ld3(xyz, (int)p);
	Cursor none{-1, 0, 0, 0};
	const Cell C = point_cell<false>(g, none, pos.x, pos.y, pos.z);
#pragma unroll
	for (int q = 0; q < kMaxPointFields; ++q) {
		if (q >= P.n) break;
		if ((P.vec3 >> q) & 1u)
			st3(P.out[q], (int)p, sample_v(P.in[q], C));
		else
			P.out[q][p] = sample_f(P.in[q], C);
	}
}

// `steps` steps of a point through the velocity u in registers, x' = x + s U(x) with U the Vec3f sampler above and s = dt / dx (negative: a back-trace), each step
// rk_step<ORDER>. A point with no leaf under any tap samples U = 0 and stays where it is. status (or null): 1 iff the final position is finite in all three components
// and the leaf of its cell exists.
template <int ORDER, bool CURSOR>
__global__ __launch_bounds__(kPointBlock) __attribute__((amdgpu_waves_per_eu(7, 8))) void k_trace_points(const GridDev g, const float* __restrict__ u, float* __restrict__ xyz, const unsigned n, const float s,
                                                              const int steps, unsigned char* __restrict__ status) {
	const unsigned p = blockIdx.x * (unsigned)kPointBlock + threadIdx.x;
	if (p >= n) return;
	f3 x = ld3(xyz, (int)p);
	const float h = 0.5f * s, s6 = s * 0.16666667f;
	Cursor cur{-1, 0, 0, 0};
	auto U = [&](float a, float b, float c) { return sample_v(u, point_cell<CURSOR>(g, cur, a, b, c)); };
	for (int step = 0; step < steps; ++step) x = rk_step<ORDER>(U, x, s, h, s6);
	st3(xyz, (int)p, x);
	if (status) status[p] = in_a_leaf<CURSOR>(g, cur, x, true) ? 1 : 0;
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------------------------------------------

// (refuse, kMaxPoints, check_sim: hns_points.hpp)

// fields / ncomp / out: HOST arrays of n_fields entries. Every refusal comes before the first launch.
int sample_points(const char* who, hns_grid* g, const float* const* fields, const int* ncomp, int n_fields, const float* xyz, uint64_t n, float* const* out, void* stream) {
	if (int rc = check_grid(g, who)) return rc;
	if (n_fields < 1) return refuse(who, "n_fields must be at least 1");
	if (!fields || !ncomp || !out) return refuse(who, "null list (fields, ncomp or out)");
	for (int i = 0; i < n_fields; ++i)
		if (ncomp[i] != 1 && ncomp[i] != 3) {
			set_error("%s: ncomp[%d] is %d (must be 1 or 3)", who, i, ncomp[i]);
			return HNS_ERR_INVALID_ARGUMENT;
		}
	if (n > kMaxPoints) return refuse(who, "n is above 2^31 - 1");
	if (n == 0) return HNS_OK;  // (no point, no device pointer looked at: an empty array's may well be null)
	if (!xyz) return refuse(who, "xyz is null");
	for (int i = 0; i < n_fields; ++i) {
		if (!fields[i] || !out[i]) {
			set_error("%s: %s[%d] is null", who, fields[i] ? "out" : "fields", i);
			return HNS_ERR_INVALID_ARGUMENT;
		}
		if (out[i] == xyz) {
			set_error("%s: out[%d] is xyz", who, i);
			return HNS_ERR_INVALID_ARGUMENT;
		}
		for (int j = 0; j < n_fields; ++j) {
			if (out[i] == fields[j]) {
				set_error("%s: out[%d] is fields[%d]", who, i, j);
				return HNS_ERR_INVALID_ARGUMENT;
			}
			if (j < i && out[i] == out[j]) {
				set_error("%s: out[%d] is out[%d]", who, i, j);
				return HNS_ERR_INVALID_ARGUMENT;
			}
		}
	}
	if (g->topo.n_leaves == 0) {  // no leaf, no field element: every tap is outside and reads 0
		for (int i = 0; i < n_fields; ++i) HNS_HIP(hipMemsetAsync(out[i], 0, sizeof(float) * ncomp[i] * n, (hipStream_t)stream));
		return HNS_OK;
	}
	const dim3 grid((unsigned)((n + kPointBlock - 1) / kPointBlock)), block(kPointBlock);
	for (int base = 0; base < n_fields; base += kMaxPointFields) {  // (the cell does not depend on the fields: more launches change nothing numerically)
		PointFields P{};
		P.n = n_fields - base < kMaxPointFields ? n_fields - base : kMaxPointFields;
		for (int q = 0; q < P.n; ++q) {
			P.in[q] = fields[base + q], P.out[q] = out[base + q];
			P.vec3 |= (ncomp[base + q] == 3 ? 1u : 0u) << q;
		}
		hipLaunchKernelGGL(k_sample_points, grid, block, 0, (hipStream_t)stream, g->dev(), P, xyz, (unsigned)n);
	}
	return launch_status(who);
}

int trace_points(const char* who, const char* dx_name, hns_grid* g, const float* vel3, float* xyz, uint64_t n, float dt, float inv_dx, int order, int steps,
                 unsigned char* status, void* stream) {
	if (int rc = check_grid(g, who)) return rc;
	if (int rc = check_step_numbers(who, dx_name, order, steps, dt, inv_dx)) return rc;
	if (n > kMaxPoints) return refuse(who, "n is above 2^31 - 1");
	if (n == 0) return HNS_OK;  // (as above)
	if (!xyz) return refuse(who, "xyz is null");
	if (!vel3) return refuse(who, "vel3 is null");
	if ((const void*)xyz == (const void*)vel3 || (status && ((const void*)status == (const void*)xyz || (const void*)status == (const void*)vel3)))
		return refuse(who, "xyz, status and vel3 must be three different buffers");
	if (g->topo.n_leaves == 0) {  // U = 0 everywhere: no point moves, none is inside
		if (status) HNS_HIP(hipMemsetAsync(status, 0, n, (hipStream_t)stream));
		return HNS_OK;
	}
	const float s = dt * inv_dx;
	// The leaf cursor (cell_leaves) stays on: at 256^3 it takes 0.61-0.70 of the hash form's time on points in leaf order at order 4 and 1.08 on randomly permuted ones
	// (profiles/points_ab.txt; the hash form is profiles/micro/exp/points_hash_form.patch). The same words either way.
	constexpr bool cursor = true;
	with_order(order, [&](auto o) {
		hipLaunchKernelGGL((k_trace_points<decltype(o)::value, cursor>), point_blocks(n), dim3(kPointBlock), 0, (hipStream_t)stream, g->dev(), vel3, xyz, (unsigned)n, s, steps, status);
	});
	return launch_status(who);
}

}  // namespace

extern "C" {

int hns_dev_sample_points(hns_grid* g, const float* const* fields, const int* ncomp, int n_fields, const float* xyz, uint64_t n, float* const* out, void* stream) {
	return sample_points("hns_dev_sample_points", g, fields, ncomp, n_fields, xyz, n, out, stream);
}

int hns_dev_trace_points(hns_grid* g, const float* vel3, float* xyz, uint64_t n, float dt, float inv_dx, int order, int steps, unsigned char* status, void* stream) {
	return trace_points("hns_dev_trace_points", "inv_dx", g, vel3, xyz, n, dt, inv_dx, order, steps, status, stream);
}

// Reads the sim's current buffers and nothing else of it: the look-ahead memo, the masks, the feedback signatures and the solve report stay as they are.
int hns_sim_sample_points(hns_sim* s, const char* const* names, int n_names, int with_velocity, const float* xyz, uint64_t n, float* const* out, void* stream) {
	const char* who = "hns_sim_sample_points";
	if (int rc = check_sim(s, who)) return rc;
	std::vector<const float*> fields;
	std::vector<int> ncomp, which;
	HNS_TRY(sim_fields(who, "names", s, n_names, names_at(names), nullptr, true, which));
	for (int k : which) fields.push_back(s->cur[k]), ncomp.push_back(1);
	if (with_velocity) fields.push_back(s->vel), ncomp.push_back(3);
	if (fields.empty()) return refuse(who, "no field to sample (no names and with_velocity = 0)");
	return sample_points(who, s->grid, fields.data(), ncomp.data(), (int)fields.size(), xyz, n, out, stream);
}

int hns_sim_trace_points(hns_sim* s, float* xyz, uint64_t n, float dt, float voxel_size, int order, int steps, unsigned char* status, void* stream) {
	const char* who = "hns_sim_trace_points";
	if (int rc = check_sim(s, who)) return rc;
	float inv_dx;
	if (int rc = inv_voxel_size(who, voxel_size, &inv_dx)) return rc;
	return trace_points(who, "1 / voxel_size", s->grid, s->vel, xyz, n, dt, inv_dx, order, steps, status, stream);
}

}  // extern "C"
