// hns_shaping.hip -- shaping a device-resident sim in place: divergence-free curl-noise turbulence on the velocity, optionally weighted by a control field, and implicit
// decay of float fields towards a target, in ONE launch over the leaves of the grid's launch range (include/hns.h: "SHAPING A SIM" states the arithmetic line by line;
// hns_noise.hpp states the noise once for this kernel and for hns_shaping_curl_host). One workgroup of 512 threads per leaf, one thread per voxel. The kernel is
// VALU-bound; every thread hashes its own eight lattice corners, 14 H per octave (the chain's shared links once). A form that hashed an octave's corner box of the leaf once
// into LDS and let the threads read their corners from it was built and measured: it lost at every frequency (profiles/shaping_time_256.jsonl) and
// is gone. The gradient table lies in LDS as floats. No atomics, no scratch, nothing waits on another workgroup. -ffp-contract=off.
#include <cstring>

#include "hns_device.hpp"
#include "hns_noise.hpp"
#include "hns_points.hpp"

using namespace hns;

namespace {

constexpr int kShapeMaxDecays = 8;

// the host's constants of one call (include/hns.h: "Host constants"), by value
struct ShapeDev {
	NoiseOctave oct[kNoiseMaxOctaves];
	int octaves;
	float off[3];
	float kA;
	float lo, inv;
	int n_decays;
	float r[kShapeMaxDecays], target[kShapeMaxDecays];
	float* vel;
	const float* control;  // null: w = 1. It may be one of `decay`: the thread reads it before it writes any field
	float* decay[kShapeMaxDecays];
};

template <bool TURBULENCE>
__global__ __launch_bounds__(512) void k_shape(const GridDev g, const ShapeDev c) {
	__shared__ float s_tab[64];
	const int leaf = g.sched ? g.sched[blockIdx.x] : g.first + (int)blockIdx.x;
	const int n = threadIdx.x;
	const int idx = leaf * 512 + n;
	if (TURBULENCE) {
		const int4 org = g.origins[leaf];
		if (n < 64) s_tab[n] = noise_table_word(n);
		__syncthreads();
		const float w_in = c.control ? c.control[idx] : 0.0f;
		const int ijk[3] = {org.x + (n >> 6), org.y + ((n >> 3) & 7), org.z + (n & 7)};
		float C[3];
		noise_sum(c.oct, c.octaves, c.off, ijk, s_tab, [&](int o, const int (&I)[3], uint32_t (&h)[8]) { noise_cell_hashes(c.oct[o].s, I, h); }, C);
		float k = c.kA;
		if (c.control) {
			float w = w_in - c.lo;
			w = w * c.inv;
			w = w > 0.0f ? w : 0.0f;  // (a NaN and -0 give +0)
			w = w < 1.0f ? w : 1.0f;
			k = c.kA * w;
		}
		const f3 v = ld3(c.vel, idx);
		const f3 m = {k * C[0], k * C[1], k * C[2]};
		st3(c.vel, idx, f3{v.x + m.x, v.y + m.y, v.z + m.z});
	}
	for (int d = 0; d < c.n_decays; ++d) {
		float t = c.decay[d][idx] - c.target[d];
		t = t * c.r[d];
		c.decay[d][idx] = c.target[d] + t;
	}
}

// the checks of the turbulence spec's numbers (null: none is asked for) and of the decay list, the objects not looked at
int check_shaping_numbers(const char* who, float dt, const hns_turbulence_spec* tb, const hns_decay_spec* decays, int n_decays) {
	if (!std::isfinite(dt) || dt < 0.0f) return refuse(who, "dt is NaN, infinite or negative");
	if (tb) {
		if (const char* bad = noise_spec_refusal(tb)) return refuse(who, bad);
		if (tb->control && !(std::isfinite(tb->control_lo) && std::isfinite(tb->control_hi) && tb->control_lo < tb->control_hi))
			return refuse(who, "control_lo and control_hi must be finite with control_lo < control_hi");
	}
	if (n_decays < 0 || n_decays > kShapeMaxDecays) return refuse(who, "n_decays is outside 0 .. 8");
	if (n_decays > 0 && !decays) return refuse(who, "decays is null with n_decays > 0");
	for (int d = 0; d < n_decays; ++d) {
		if (!decays[d].name) return refuse(who, "a decay has a null name");
		if (!std::isfinite(decays[d].rate) || decays[d].rate < 0.0f) return refuse(who, "a decay's rate is NaN, infinite or negative");
		if (!std::isfinite(decays[d].target)) return refuse(who, "a decay's target is not finite");
	}
	return HNS_OK;
}

}  // namespace

struct hns_shaping {
	int device = -1;
	hipStream_t stream = nullptr;
};

extern "C" {

hns_shaping* hns_shaping_create(int* err) {
	return make_object<hns_shaping>("hns_shaping_create", err, false, nullptr, 0, "", [](hns_shaping*) { return (int)HNS_OK; });
}

void hns_shaping_destroy(hns_shaping* o) { delete o; }

int hns_shaping_set_stream(hns_shaping* o, void* hip_stream) { return set_object_stream(o, hip_stream, "hns_shaping_set_stream", "null shaping"); }

int hns_shaping_apply(hns_shaping* o, hns_sim* s, float dt, const hns_turbulence_spec* tb, const hns_decay_spec* decays, int n_decays) {
	const char* who = "hns_shaping_apply";
	// the numbers and the specs, host structs, first: they are refused whatever the objects are, a machine without a device included
	if (int rc = check_shaping_numbers(who, dt, tb, decays, n_decays)) return rc;
	if (!o) return refuse(who, "null shaping");
	if (int rc = check_sim(s, who)) return rc;
	ShapeDev d = {};
	int control = -1;
	if (tb && tb->control) {
		control = s->find(tb->control);
		if (control < 0) {
			set_error("%s: control: no float field named '%s' in this sim", who, tb->control);
			return HNS_ERR_INVALID_ARGUMENT;
		}
	}
	std::vector<int> field;
	HNS_TRY(sim_fields(who, "decays", s, n_decays, [&](int k) { return decays[k].name; }, "may be the control, not a decayed field", false, field));
	const bool turbulent = tb && tb->amplitude != 0.0f;
	if (!turbulent && n_decays == 0) return HNS_OK;
	hns_grid* g;
	HNS_TRY(sim_grid(who, s, o->device, "shaping object", true, &g));
	if (g->n_active == 0) return HNS_OK;
	if (turbulent) {
		noise_octaves(*tb, d.oct);
		d.octaves = tb->octaves;
		for (int a = 0; a < 3; ++a) d.off[a] = tb->offset[a];
		d.kA = tb->amplitude * dt;
		d.vel = s->vel;
		if (control >= 0) {
			d.control = s->cur[(size_t)control];
			d.lo = tb->control_lo;
			d.inv = 1.0f / (tb->control_hi - tb->control_lo);
		}
	}
	d.n_decays = n_decays;
	for (int k = 0; k < n_decays; ++k) {
		d.decay[k] = s->cur[(size_t)field[k]];
		d.r[k] = 1.0f / (1.0f + decays[k].rate * dt);
		d.target[k] = decays[k].target;
	}
	const dim3 grid((unsigned)g->n_active), block(512);
	if (turbulent)
		hipLaunchKernelGGL(k_shape<true>, grid, block, 0, o->stream, g->dev(), d);
	else
		hipLaunchKernelGGL(k_shape<false>, grid, block, 0, o->stream, g->dev(), d);
	// what the sim knew of the buffers just written, as hns_sim_splat_points forgets it: the velocity's signature and the look-ahead memo, which is a function of the
	// velocity (and of collision_sdf, which is why that field is no decay name); of a decayed field its signature alone
	if (turbulent) s->forget(hns_sim::kVelocity);
	for (int k = 0; k < n_decays; ++k) s->wrote_field(field[k]);
	return launch_status(who);
}

int hns_shaping_curl_host(const hns_turbulence_spec* tb, int i, int j, int k, hns_shaping_curl* out) {
	const char* who = "hns_shaping_curl_host";
	if (!tb) return refuse(who, "null spec");
	if (!out) return refuse(who, "null out");
	if (const char* bad = noise_spec_refusal(tb)) return refuse(who, bad);
	float tab[64];
	for (int w = 0; w < 64; ++w) tab[w] = noise_table_word(w);
	NoiseOctave oct[kNoiseMaxOctaves];
	noise_octaves(*tb, oct);
	const int ijk[3] = {i, j, k};
	float C[3];
	noise_sum(oct, tb->octaves, tb->offset, ijk, tab, [&](int o, const int (&I)[3], uint32_t (&h)[8]) { noise_cell_hashes(oct[o].s, I, h); }, C);
	out->c[0] = C[0], out->c[1] = C[1], out->c[2] = C[2];
	return HNS_OK;
}

}  // extern "C"
