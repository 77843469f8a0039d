// hns_diffusion.hip -- implicit diffusion of float fields and viscosity of the velocity on a device-resident sim: per listed field (I - a L) x = b over the sim's unknowns,
// by Jacobi or Chebyshev-accelerated Jacobi iterations (include/hns.h: "DIFFUSING A SIM" states the arithmetic line by line). The reference carries an explicit form that
// it never launches (reference src/Cuda/Kernel.cu:873-920); nothing of it is kept. Two kernels, one workgroup of 512 threads per leaf, one thread per voxel:
//   k_diffuse_faces   once per call: the class of every voxel of the leaf and of the six face layers of its neighbours (masks, collision_sdf) into LDS, then per voxel one
//                     byte {unknown, six open faces} and one byte {six wall faces}. The iterations read those and never the masks or the SDF again.
//   k_diffuse<C, V>   one iteration of every listed field (and of the velocity, V) per launch: per field the leaf's 512 values of the previous iterate and the 384 of its
//                     neighbours' face layers go into an LDS tile (hns_device.hpp: kTile, halo_entry, tile_nbr), double-buffered so that a field costs one barrier; the code
//                     bytes, the tile entries of the six neighbours and the halo duty are formed once per thread, not once per field. C: the Chebyshev step (k >= 2).
// The iterates ping-pong between two scratch arrays per field; the first iteration reads the field itself (x^0 = b) and the last writes into it -- its thread reads b and
// x^(k-2) of its own voxel only, and the neighbours come from the scratch --, so there is no copy except for iterations == 1 (k_diffuse_copy: one iteration cannot read its
// neighbours out of the array it writes). No atomics, no scratch memory, no division, nothing waits on another workgroup. -ffp-contract=off.
#include <cstring>

#include "hns_device.hpp"
#include "hns_points.hpp"

using namespace hns;

namespace {

constexpr int kDiffMaxTerms = 8;
constexpr int kDiffMaxIterations = 256;
constexpr unsigned kDiffUnknown = 64u;  // bit of the low code byte; bits 0..5: the face is open, in the order +x, -x, +y, -y, +z, -z; the high byte: the face is a wall

// one field of one launch: b (the field as it stood at the call), the previous iterate, x^(k-2) (Chebyshev) and the iterate to write, with the host's constants
struct DiffTerm {
	const float* b;
	const float* in;
	const float* prev;
	float* out;
	float a, w;
	float r[7];
};
struct DiffDev {
	const unsigned char* lo;
	const unsigned char* hi;
	int n_terms;
	DiffTerm term[kDiffMaxTerms];
	DiffTerm vel;  // (V only; 12-byte AoS elements)
};

// 0: neither, 1: an unknown, 2: solid (include/hns.h: "Voxel classes"; a NaN is not solid)
__device__ __forceinline__ unsigned diffuse_class(const unsigned char* __restrict__ masks, const float* __restrict__ sdf, float threshold, int leaf, int v) {
	const bool solid = sdf && sdf[(size_t)leaf * 512 + v] < threshold;
	return solid ? 2u : (is_unknown(masks, leaf, v) ? 1u : 0u);
}

// the tile entries of the six face neighbours of own voxel n, in the header's order
__device__ __forceinline__ void diffuse_entries(int n, int (&e)[6]) {
	e[0] = tile_nbr<0, 1>(n), e[1] = tile_nbr<0, -1>(n), e[2] = tile_nbr<1, 1>(n), e[3] = tile_nbr<1, -1>(n), e[4] = tile_nbr<2, 1>(n), e[5] = tile_nbr<2, -1>(n);
}

__global__ __launch_bounds__(512) void k_diffuse_faces(const GridDev g, const unsigned char* __restrict__ masks, const float* __restrict__ sdf, const float threshold,
                                                       unsigned char* __restrict__ lo, unsigned char* __restrict__ hi) {
	__shared__ unsigned char s_c[kTile];
	__shared__ int s_nbr[27];
	const LeafCtx L = stage_leaf(g, s_nbr, blockIdx.x);
	const int n = threadIdx.x;
	s_c[n] = (unsigned char)diffuse_class(masks, sdf, threshold, L.leaf, n);
	if (n < 384) {
		int slot, local;
		halo_entry(n, slot, local);
		const int nl = s_nbr[slot];
		s_c[512 + n] = nl < 0 ? 0 : (unsigned char)diffuse_class(masks, sdf, threshold, nl, local);  // an absent leaf: closed
	}
	__syncthreads();
	int e[6];
	diffuse_entries(n, e);
	unsigned open = 0, wall = 0;
#pragma unroll
	for (int f = 0; f < 6; ++f) {
		const unsigned k = s_c[e[f]];
		open |= (k == 1u ? 1u : 0u) << f;
		wall |= (k == 2u ? 1u : 0u) << f;
	}
	const bool me = s_c[n] == 1;
	const int idx = L.leaf * 512 + n;
	lo[idx] = (unsigned char)(me ? (kDiffUnknown | open) : 0u);
	hi[idx] = (unsigned char)(me ? wall : 0u);
}

__device__ __forceinline__ float pick_r(const float (&r)[7], int m) {
	float v = r[0];
#pragma unroll
	for (int k = 1; k < 7; ++k) v = m == k ? r[k] : v;
	return v;
}

// One component of one field for thread n: stage the previous iterate (own value x, and as halo thread the value `halo`) into tile T, then the header's lines.
template <bool CHEB>
__device__ __forceinline__ float diffuse_value(float* T, int n, const int (&e)[6], unsigned open, float x, float halo, float b, float prev, float a, float r, float w) {
	T[n] = x;
	if (n < 384) T[512 + n] = halo;
	__syncthreads();
	float S = 0.0f;
#pragma unroll
	for (int f = 0; f < 6; ++f) {
		const float v = T[e[f]];
		S = (open >> f) & 1u ? S + v : S;
	}
	float t = a * S;
	t = b + t;
	const float j = t * r;
	if (!CHEB) return j;
	float d = j - prev;
	d = w * d;
	return prev + d;
}

template <bool CHEB, bool VEL>
__global__ __launch_bounds__(512) void k_diffuse(const GridDev g, const DiffDev c) {
	__shared__ float s_x[2][kTile];  // double-buffered: the barrier of one component also ends the reads of the one before the last
	__shared__ int s_nbr[27];
	const LeafCtx L = stage_leaf(g, s_nbr, blockIdx.x);
	const int n = threadIdx.x;
	const int idx = L.leaf * 512 + n;
	const unsigned lo = c.lo[idx];
	const unsigned open = lo & 63u;
	const bool unknown = (lo & kDiffUnknown) != 0;
	int e[6];
	diffuse_entries(n, e);
	int slot, local;
	halo_entry(n < 384 ? n : 0, slot, local);
	const int hl = n < 384 ? s_nbr[slot] : -1;
	const int hidx = hl < 0 ? 0 : hl * 512 + local;  // (a value read for an absent leaf, or from scratch that no iteration wrote, is never taken: its face is not open)
	int buf = 0;
	if (VEL) {
		const DiffTerm& q = c.vel;
		const int m = __popc(open) + __popc((unsigned)c.hi[idx]);
		const float r = pick_r(q.r, m);
		const f3 x = ld3(q.in, idx), b = ld3(q.b, idx), h = ld3(q.in, hidx);
		f3 p = {0.0f, 0.0f, 0.0f};
		if (CHEB) p = ld3(q.prev, idx);
		f3 o;
		o.x = diffuse_value<CHEB>(s_x[0], n, e, open, x.x, h.x, b.x, p.x, q.a, r, q.w);
		o.y = diffuse_value<CHEB>(s_x[1], n, e, open, x.y, h.y, b.y, p.y, q.a, r, q.w);
		o.z = diffuse_value<CHEB>(s_x[0], n, e, open, x.z, h.z, b.z, p.z, q.a, r, q.w);
		if (unknown) st3(q.out, idx, o);
		buf = 1;
	}
	const int m = __popc(open);
	for (int d = 0; d < c.n_terms; ++d) {
		const DiffTerm& q = c.term[d];
		const float r = pick_r(q.r, m);
		const float x = q.in[idx], b = q.b[idx], h = q.in[hidx];
		const float p = CHEB ? q.prev[idx] : 0.0f;
		const float o = diffuse_value<CHEB>(s_x[buf], n, e, open, x, h, b, p, q.a, r, q.w);
		if (unknown) q.out[idx] = o;
		buf ^= 1;
	}
}

// iterations == 1 only: the one iterate from the scratch into the unknowns of the field
__global__ __launch_bounds__(512) void k_diffuse_copy(const GridDev g, const DiffDev c, const int has_vel) {
	const int leaf = g.sched ? g.sched[blockIdx.x] : g.first + (int)blockIdx.x;
	const int idx = leaf * 512 + (int)threadIdx.x;
	if (!(c.lo[idx] & kDiffUnknown)) return;
	if (has_vel) st3(c.vel.out, idx, ld3(c.vel.in, idx));
	for (int d = 0; d < c.n_terms; ++d) c.term[d].out[idx] = c.term[d].in[idx];
}

// the host constants of one coefficient (include/hns.h: "Host constants"): one rounded float32 operation per statement
void diffusion_schedule(float coefficient, float dt, float voxel_size, int iterations, hns_diffusion_schedule* o) {
	const float h2 = voxel_size * voxel_size;
	float a = coefficient * dt;
	a = a / h2;
	o->a = a;
	for (int m = 0; m < 7; ++m) {
		const float e = a * (float)m;
		const float den = 1.0f + e;
		o->r[m] = 1.0f / den;
	}
	const float s = 6.0f * a;
	const float den = 1.0f + s;
	const float rho = s / den;
	const float q = rho * rho;
	o->rho = rho;
	for (int k = 0; k < kDiffMaxIterations; ++k) o->omega[k] = 0.0f;
	o->omega[0] = 1.0f;
	if (iterations >= 2) {
		const float h = q * 0.5f;
		const float d = 1.0f - h;
		o->omega[1] = 1.0f / d;
	}
	const float c = q * 0.25f;
	for (int k = 2; k < iterations; ++k) {  // w_(k+1) from w_k
		const float e = c * o->omega[k - 1];
		const float d = 1.0f - e;
		o->omega[k] = 1.0f / d;
	}
}

// coefficient, dt and voxel size as one term's a: is it a number the iteration can run with?
const char* diffusion_a_refusal(float coefficient, float dt, float voxel_size) {
	const float h2 = voxel_size * voxel_size;
	float a = coefficient * dt;
	a = a / h2;
	const float s = 6.0f * a;
	return std::isfinite(a) && std::isfinite(s) ? nullptr : "a = coefficient * dt / voxel_size^2, or 6 a, is not finite";
}

int check_diffusion_scalars(const char* who, float dt, float voxel_size, int iterations) {
	if (!std::isfinite(dt) || dt < 0.0f) return refuse(who, "dt is NaN, infinite or negative");
	if (!std::isfinite(voxel_size) || !(voxel_size > 0.0f)) return refuse(who, "voxel_size is not finite and > 0");
	if (iterations < 1 || iterations > kDiffMaxIterations) return refuse(who, "iterations is outside 1 .. 256");
	return HNS_OK;
}

int check_diffusion_numbers(const char* who, float dt, float voxel_size, const hns_diffusion_spec* sp, const hns_diffusion_term* terms, int n_terms) {
	if (!sp) return refuse(who, "null spec");
	if (int rc = check_diffusion_scalars(who, dt, voxel_size, sp->iterations)) return rc;
	if (sp->method < 0 || sp->method > 1) return refuse(who, "method is outside 0 .. 1");
	if (!std::isfinite(sp->viscosity) || sp->viscosity < 0.0f) return refuse(who, "viscosity is NaN, infinite or negative");
	if (diffusion_a_refusal(sp->viscosity, dt, voxel_size)) return refuse(who, "viscosity: a = coefficient * dt / voxel_size^2, or 6 a, is not finite");
	if (sp->collide && !std::isfinite(sp->threshold)) return refuse(who, "threshold is not finite");
	if (n_terms < 0 || n_terms > kDiffMaxTerms) return refuse(who, "n_terms is outside 0 .. 8");
	if (n_terms > 0 && !terms) return refuse(who, "terms is null with n_terms > 0");
	for (int k = 0; k < n_terms; ++k) {
		if (!terms[k].name) return refuse(who, "a term has a null name");
		if (!std::isfinite(terms[k].coefficient) || terms[k].coefficient < 0.0f) return refuse(who, "a term's coefficient is NaN, infinite or negative");
		if (diffusion_a_refusal(terms[k].coefficient, dt, voxel_size)) return refuse(who, "a term's coefficient: a = coefficient * dt / voxel_size^2, or 6 a, is not finite");
	}
	return HNS_OK;
}

}  // namespace

struct hns_diffusion {
	int device = -1;
	hipStream_t stream = nullptr;
	hns::Pooled block;  // the two code bytes per voxel and the second iterate of every written float field of the largest call so far
};

extern "C" {

hns_diffusion* hns_diffusion_create(int* err) {
	return make_object<hns_diffusion>("hns_diffusion_create", err, false, nullptr, 0, "", [](hns_diffusion*) { return (int)HNS_OK; });
}

void hns_diffusion_destroy(hns_diffusion* o) { delete o; }

int hns_diffusion_set_stream(hns_diffusion* o, void* hip_stream) { return set_object_stream(o, hip_stream, "hns_diffusion_set_stream", "null diffusion"); }

int hns_diffusion_schedule_host(float coefficient, float dt, float voxel_size, int iterations, hns_diffusion_schedule* out) {
	const char* who = "hns_diffusion_schedule_host";
	if (!out) return refuse(who, "null out");
	if (int rc = check_diffusion_scalars(who, dt, voxel_size, iterations)) return rc;
	if (!std::isfinite(coefficient) || coefficient < 0.0f) return refuse(who, "coefficient is NaN, infinite or negative");
	if (const char* bad = diffusion_a_refusal(coefficient, dt, voxel_size)) return refuse(who, bad);
	diffusion_schedule(coefficient, dt, voxel_size, iterations, out);
	return HNS_OK;
}

int hns_diffusion_apply(hns_diffusion* o, hns_sim* s, float dt, float voxel_size, const hns_diffusion_spec* sp, const hns_diffusion_term* terms, int n_terms) {
	const char* who = "hns_diffusion_apply";
	// the numbers and the host structs first: they are refused whatever the objects are, a machine without a device included
	if (int rc = check_diffusion_numbers(who, dt, voxel_size, sp, terms, n_terms)) return rc;
	if (!o) return refuse(who, "null diffusion");
	if (int rc = check_sim(s, who)) return rc;
	std::vector<int> field;
	HNS_TRY(sim_fields(who, "terms", s, n_terms, [&](int k) { return terms[k].name; }, "decides what is solid and is not diffused", false, field));
	const int i_sdf = sp->collide ? s->find("collision_sdf") : -1;
	if (sp->collide && i_sdf < 0) return refuse(who, "collide: no float field named 'collision_sdf' in this sim");
	// the terms that run: a == +0 (coefficient 0 or dt 0) is skipped, neither read nor written
	std::vector<hns_diffusion_schedule> sched;
	std::vector<int> which;  // float field index, kVelocity for the velocity
	auto add = [&](float coefficient, int k) {
		hns_diffusion_schedule c;
		diffusion_schedule(coefficient, dt, voxel_size, sp->iterations, &c);
		if (c.a != 0.0f) sched.push_back(c), which.push_back(k);
	};
	add(sp->viscosity, hns_sim::kVelocity);
	const bool has_vel = !which.empty();
	for (int k = 0; k < n_terms; ++k) add(terms[k].coefficient, field[k]);
	if (which.empty()) return HNS_OK;
	hns_grid* g;
	HNS_TRY(sim_grid(who, s, o->device, "diffusion object", true, &g));
	if (g->first_active != 0 || g->n_active != (uint64_t)g->topo.n_leaves) return refuse(who, "the grid's launch range is not the whole grid");
	if (g->n_active == 0) return HNS_OK;
	// scratch: of the velocity adv and tmp (the look-ahead memo in adv goes with the forget below), of a float field its own nxt and one pooled array
	const size_t n_float = which.size() - (has_vel ? 1 : 0), unit = sim_unit(s->n);
	unsigned char *lo = nullptr, *hi = nullptr;
	float* second = nullptr;
	auto slices = [&](const Slice& slice) { slice(lo, (size_t)s->n), slice(hi, (size_t)s->n), slice(second, n_float ? n_float : 1, unit); };
	HNS_TRY(o->block.reserve(carve(nullptr, slices), o->device));
	carve(o->block.p, slices);
	const GridDev gd = g->dev();
	const dim3 grid((unsigned)g->n_active), block(512);
	hipLaunchKernelGGL(k_diffuse_faces, grid, block, 0, o->stream, gd, s->d_masks.as<unsigned char>(), i_sdf >= 0 ? s->cur[(size_t)i_sdf] : nullptr, sp->threshold, lo, hi);
	const int K = sp->iterations;
	DiffDev d = {};
	d.lo = lo, d.hi = hi, d.n_terms = (int)n_float;
	for (int k = 1; k <= K; ++k) {
		const bool cheb = sp->method == 1 && k >= 2;
		size_t nf = 0;
		for (size_t t = 0; t < which.size(); ++t) {
			const bool v = which[t] == hns_sim::kVelocity;
			float* cur = v ? s->vel : s->cur[(size_t)which[t]];
			float* X[2] = {v ? s->adv : s->nxt[(size_t)which[t]], v ? s->tmp : (float*)((char*)second + nf * unit)};
			DiffTerm& q = v ? d.vel : d.term[nf];
			q.b = cur;
			q.in = k == 1 ? cur : X[(k - 1) & 1];
			q.prev = k == 2 ? cur : X[k & 1];  // x^(k-2); read by the Chebyshev step alone
			q.out = k == K && K >= 2 ? cur : X[k & 1];
			q.a = sched[t].a, q.w = sched[t].omega[k - 1];
			for (int m = 0; m < 7; ++m) q.r[m] = sched[t].r[m];
			if (!v) ++nf;
		}
		if (cheb && has_vel)
			hipLaunchKernelGGL((k_diffuse<true, true>), grid, block, 0, o->stream, gd, d);
		else if (cheb)
			hipLaunchKernelGGL((k_diffuse<true, false>), grid, block, 0, o->stream, gd, d);
		else if (has_vel)
			hipLaunchKernelGGL((k_diffuse<false, true>), grid, block, 0, o->stream, gd, d);
		else
			hipLaunchKernelGGL((k_diffuse<false, false>), grid, block, 0, o->stream, gd, d);
	}
	if (K == 1) {  // the one iterate lies in the scratch
		size_t nf = 0;
		for (size_t t = 0; t < which.size(); ++t) {
			const bool v = which[t] == hns_sim::kVelocity;
			DiffTerm& q = v ? d.vel : d.term[nf];
			q.in = q.out, q.out = v ? s->vel : s->cur[(size_t)which[t]];
			if (!v) ++nf;
		}
		hipLaunchKernelGGL(k_diffuse_copy, grid, block, 0, o->stream, gd, d, has_vel ? 1 : 0);
	}
	if (has_vel) s->forget(hns_sim::kVelocity);
	for (size_t t = 0; t < which.size(); ++t)
		if (which[t] != hns_sim::kVelocity) s->wrote_field(which[t]);
	return launch_status(who);
}

}  // extern "C"
