// hns_api.hip -- host code only: the device-resident simulation state (hns_sim_*), its substep (Substep: core and full), the cook cache (make_sim) and the drop-in
// operators of include/hns.h with the resident-feedback cook (Cook). The launch orders follow the reference's host drivers (reference src/Cuda/HNanoSolver.cu:150-356,
// src/Cuda/PressureProjection.cu:43-66, src/Cuda/Advection.cu:76-91,148-155); what differs is that fields can stay
// resident across substeps and that nothing is allocated inside a substep. The pool the memory comes from: hns_arena.hip.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "hns_internal.hpp"
#include "hns_digest.hpp"
#include "hns_device.hpp"  // check_grid, which hns_simcall.hpp builds on
#include "hns_simcall.hpp"

using namespace hns;

// ---------------------------------------------------------------------------------------------------------------
// grid: device tables
// ---------------------------------------------------------------------------------------------------------------

GridDev hns_grid::dev() const {
	GridDev d;
	d.origins = (const int4*)d_origins;
	d.nbr27 = (const int*)d_nbr27;
	d.hash = (const int*)d_hash;
	d.sched = (const int*)d_sched;
	d.sched_seg = sched_seg, d.sched_pre = sched_pre;
	d.blk = (const int*)d_blk;
	d.hash_mask = topo.hash_mask;
	d.n_leaves = (int)topo.n_leaves;
	d.n_active = (int)n_active;
	d.first = (int)first_active;
	d.oob = (int)outside_element;
	d.rev = 0;
	d.far_flag = far_flag;
	return d;
}

extern "C" int hns_device_count(void) {
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) return 0;
	return n;
}

// ---------------------------------------------------------------------------------------------------------------
// device-resident simulation state
// ---------------------------------------------------------------------------------------------------------------

// (struct hns_sim: hns_internal.hpp -- hns_regrid.hip moves a sim onto a new grid)

extern "C" void hns_sim_destroy(hns_sim* s) {
	if (!s) return;
	s->solve_ev.destroy();
	s->stage_ev.destroy();
	for (hipEvent_t e : s->xev)
		if (e) (void)hipEventDestroy(e);
	for (hipEvent_t e : s->rev)
		if (e) (void)hipEventDestroy(e);
	if (s->xfer) (void)hipStreamDestroy(s->xfer);
	if (s->h_dig) (void)hipHostFree(s->h_dig);
	hns_sim_free_diagnostics(s);
	hns_sim_free_multigrid(s);
	delete s;  // (its pooled blocks go back with their owners)
}

// Frees the device-resident state operator calls left with the grid (see make_sim below) and the accumulator of hns_dev_splat_points.
extern "C" int hns_grid_release_cache(hns_grid* g) {
	if (!g) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_grid_release_cache: null grid");
	std::vector<hns_sim*> drop;
	{
		std::lock_guard<std::mutex> lock(g->host_mutex);
		for (size_t i = 0; i < g->sim_cache.size();) {
			if (g->sim_cache[i]->in_use) {
				++i;
				continue;
			}
			drop.push_back(g->sim_cache[i]);
			g->sim_cache.erase(g->sim_cache.begin() + (long)i);
		}
	}
	for (hns_sim* s : drop) {
		s->cached = false;
		hns_sim_destroy(s);
	}
	hns_grid_free_splat(g);
	return HNS_OK;
}

// (the sim's buffers over its arena: hns_sim_arena_need / hns_sim_layout, hns_internal.hpp)

// zero: clear the arena (what hns_sim_create promises); the operator path skips it when every buffer is written before it is read
static hns_sim* sim_create(hns_grid* g, const char* const* float_names, int n_float, bool zero, void* stream, int* rc_out) {
	hns_sim* s = new hns_sim;
	s->grid = g;
	s->n = hns_grid_voxel_count(g);
	s->device = g->device;
	int rc = HNS_OK;
	for (int i = 0; i < n_float && rc == HNS_OK; ++i) {
		if (!float_names[i]) {
			rc = fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_create: null field name");
		} else if (s->find(float_names[i]) >= 0) {
			set_error("hns_sim_create: duplicate field name '%s'", float_names[i]);
			rc = HNS_ERR_INVALID_ARGUMENT;
		} else {
			s->names.push_back(float_names[i]);
		}
	}
	s->handed_cur.resize(s->names.size());
	if (rc == HNS_OK) rc = s->arena.get(hns_sim_arena_need(s, s->n), s->device);
	if (rc == HNS_OK) {
		hns_sim_layout(s, s->arena.p, s->n);
		if (zero && hipMemsetAsync(s->arena.p, 0, (char*)s->d_dig - s->arena.as<char>(), (hipStream_t)stream) != hipSuccess) rc = fail(HNS_ERR_HIP, "hns_sim_create: clearing the field memory failed");
	}
	if (rc != HNS_OK) {
		hns_sim_destroy(s);
		s = nullptr;
	}
	*rc_out = rc;
	return s;
}

extern "C" hns_sim* hns_sim_create(hns_grid* g, const char* const* float_names, int n_float, int* err) {
	int rc = HNS_OK;
	if (!g || n_float < 0 || (n_float > 0 && !float_names)) {
		rc = fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_create: bad arguments");
	} else if (!g->on_device) {
		rc = fail(HNS_ERR_NO_DEVICE, "hns_sim_create: grid has no device tables (there is no CPU fallback)");
	}
	if (rc != HNS_OK) {
		if (err) *err = rc;
		return nullptr;
	}
	hns_sim* s = sim_create(g, float_names, n_float, true, nullptr, &rc);
	// the clear ran on the null stream: finish it, so that the caller may use any stream (also a non-blocking one) afterwards
	if (s && hipStreamSynchronize(nullptr) != hipSuccess) {
		rc = fail(HNS_ERR_HIP, "hns_sim_create: clearing the field memory failed");
		hns_sim_destroy(s);
		s = nullptr;
	}
	if (err) *err = rc;
	return s;
}

// The device buffer behind a field of hns_sim_upload / hns_sim_download, and its index for hns_sim::forget: ncomp 3 is the velocity, 1 a float field looked up by name.
static int sim_field(hns_sim* s, const hns_field& f, const char* who, int* k, float** buf) {
	if (f.ncomp == 3) {
		*k = hns_sim::kVelocity, *buf = s->vel;
		return HNS_OK;
	}
	if (f.ncomp != 1) {
		set_error("%s: ncomp must be 1 or 3", who);
		return HNS_ERR_INVALID_ARGUMENT;
	}
	*k = f.name ? s->find(f.name) : -1;
	if (*k < 0) {
		set_error("%s: no float field named '%s' in this sim", who, f.name ? f.name : "?");
		return HNS_ERR_RUNTIME;
	}
	*buf = s->cur[*k];
	return HNS_OK;
}

extern "C" int hns_sim_upload(hns_sim* s, const hns_field* fields, int n_fields, void* stream) {
	if (!s || (n_fields > 0 && !fields)) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_upload: null argument");
	for (int i = 0; i < n_fields; ++i) {
		const hns_field& f = fields[i];
		if (!f.host) {
			set_error("hns_sim_upload: host pointer is null for block: %s", f.name ? f.name : "?");
			return HNS_ERR_RUNTIME;
		}
		int k;
		float* buf;
		HNS_TRY(sim_field(s, f, "hns_sim_upload", &k, &buf));
		s->forget(k);
		HNS_HIP(hipMemcpyAsync(buf, f.host, sizeof(float) * (size_t)f.ncomp * (size_t)s->n, hipMemcpyHostToDevice, (hipStream_t)stream));
	}
	return HNS_OK;
}

extern "C" int hns_sim_download(hns_sim* s, hns_field* fields, int n_fields, void* stream) {
	if (!s || (n_fields > 0 && !fields)) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_download: null argument");
	for (int i = 0; i < n_fields; ++i) {
		hns_field& f = fields[i];
		if (!f.host) return fail(HNS_ERR_RUNTIME, "hns_sim_download: null host pointer");
		int k;
		float* buf;
		HNS_TRY(sim_field(s, f, "hns_sim_download", &k, &buf));
		HNS_HIP(hipMemcpyAsync(f.host, buf, sizeof(float) * (size_t)f.ncomp * (size_t)s->n, hipMemcpyDeviceToHost, (hipStream_t)stream));
	}
	HNS_HIP(hipStreamSynchronize((hipStream_t)stream));
	return HNS_OK;
}

extern "C" float* hns_sim_velocity_ptr(hns_sim* s) {
	if (!s) return nullptr;
	s->ahead_off = true;  // a writable pointer the library cannot watch: this sim never looks ahead again (include/hns.h)
	s->drop_ahead();
	return s->vel;
}
// How often a substep of this sim launched the look-ahead form of advect_scalars, and how often one skipped its advect_vector launch for it (tests, profiles).
extern "C" int hns_sim_lookahead_counts(hns_sim* s, long long* produced, long long* consumed) {
	if (!s || !produced || !consumed) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_lookahead_counts: null argument");
	*produced = s->ahead_produced, *consumed = s->ahead_consumed;
	return HNS_OK;
}
extern "C" float* hns_sim_field_ptr(hns_sim* s, const char* name) {
	if (!s || !name) return nullptr;
	const int k = s->find(name);
	return k < 0 ? nullptr : s->cur[k];
}
extern "C" float* hns_sim_divergence_ptr(hns_sim* s) { return s ? s->div : nullptr; }
extern "C" float* hns_sim_pressure_ptr(hns_sim* s) { return s ? s->p_result : nullptr; }

static int validate_step(float voxel_size, float dt, int64_t iterations, bool need_iter) {
	if (voxel_size <= 0.0f) return fail(HNS_ERR_INVALID_ARGUMENT, "voxelSize must be positive.");                          // HNanoSolver.cu:12-14
	if (dt < 0.0f) return fail(HNS_ERR_INVALID_ARGUMENT, "dt (time step) cannot be negative.");                           // :15-17
	if (need_iter && iterations <= 0) return fail(HNS_ERR_INVALID_ARGUMENT, "Number of pressure iterations must be positive.");  // :18-20
	return HNS_OK;
}

namespace hns {  // (declared in hns_dist.hpp: the partitioned substep uses the same omega)
float omega_compute(float vs) { return 2.0f / (1.0f + sinf(static_cast<float>(3.14159) * vs)); }          // HNanoSolver.cu:257
}  // namespace hns
static float omega_project(float vs) { return (float)(2.0f / (1.0f + sin(3.14159 * (double)vs))); }             // PressureProjection.cu:53

extern "C" int hns_sim_pressure_solve(hns_sim* s, int iterations, float voxel_size, void* stream) {
	if (!s) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_pressure_solve: null sim");
	HNS_TRY(validate_step(voxel_size, 0.0f, iterations, true));
	HNS_TRY(hns_solve_preflight(s, stream, "hns_sim_pressure_solve"));
	return hns_sim_solve(s, iterations, voxel_size, omega_compute(voxel_size), stream);
}

// Bracket every following pressure loop (up to max_solves of them) with a hipEvent pair on its launch stream.
extern "C" int hns_sim_timing(hns_sim* s, int max_solves) {
	if (!s || max_solves < 0) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_timing: bad arguments");
	s->timed_launches = 0;
	return s->solve_ev.reset(max_solves);
}

// Bracket the five stages of the next max_substeps substeps (six events per substep: a few microseconds
// each on the launch stream, which is why this is a switch of its own and not part of hns_sim_timing).
extern "C" int hns_sim_stage_timing(hns_sim* s, int max_substeps) {
	if (!s || max_substeps < 0) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_stage_timing: bad arguments");
	return s->stage_ev.reset(max_substeps);
}

// Per-stage device time of the substeps run since hns_sim_stage_timing(): ms5 = {advect_vector, divergence, pressure loop,
// gradient subtraction, advect_scalars} (what the full substep adds to each: Substep), summed over `*substeps` substeps; events sit on the launch stream.
extern "C" int hns_sim_stage_times(hns_sim* s, float* ms5, long long* substeps) {
	if (!s || !ms5 || !substeps) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_stage_times: null argument");
	double tot[5];
	HNS_TRY(s->stage_ev.elapsed(tot));
	for (int k = 0; k < 5; ++k) ms5[k] = (float)tot[k];
	*substeps = (long long)s->stage_ev.used;
	return HNS_OK;
}

// Sum of the bracketed pressure-loop times since hns_sim_timing() and the number of fused-iteration launches inside.
extern "C" int hns_sim_pressure_time(hns_sim* s, float* total_ms, long long* launches) {
	if (!s || !total_ms || !launches) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_pressure_time: null argument");
	double tot;
	HNS_TRY(s->solve_ev.elapsed(&tot));
	*total_ms = (float)tot;
	*launches = s->timed_launches;
	return HNS_OK;
}

// can the advect_scalars launch of a substep over `fields` float fields also leave advect_vector in s->adv?
static bool sim_ahead_applies(const hns_sim* s, bool coll, size_t fields) { return !coll && fields > 0 && fields <= 8 && hns_advect_ahead_ok(s->grid); }

// *ahead (in): also leave advect_vector(s->vel, dt) in s->adv, where one launch can (out: it was done)
static int sim_advect_scalars(hns_sim* s, const float* sdf, bool coll, float dt, float inv_dx, void* stream, bool* ahead) {
	std::vector<const float*> ins;
	std::vector<float*> outs;
	std::vector<int> which;
	for (size_t i = 0; i < s->names.size(); ++i) {
		if (s->names[i] == "collision_sdf") continue;  // HNanoSolver.cu:327
		ins.push_back(s->cur[i]);
		outs.push_back(s->nxt[i]);
		which.push_back((int)i);
	}
	*ahead = *ahead && sim_ahead_applies(s, coll, ins.size());
	if (*ahead)
		HNS_TRY(hns_dev_advect_scalars_ahead(s->grid, s->vel, ins.data(), outs.data(), (int)ins.size(), s->adv, dt, inv_dx, stream));
	else
		HNS_TRY(hns_dev_advect_scalars(s->grid, s->vel, ins.data(), outs.data(), (int)ins.size(), sdf, coll, dt, inv_dx, stream));
	for (int i : which) std::swap(s->cur[i], s->nxt[i]);
	return HNS_OK;
}

// One substep in the order of reference HNanoSolver.cu:150-356, cut at the two points where it starts to need more input
// fields, so that the operator path can enqueue each part as soon as its inputs are on the device:
//   part A  needs velocity (+ collision_sdf)      collision, advect_vector, vorticity
//   part B  needs fuel/waste/temperature/flame     divergence, combustion, buoyancy, pressure solve, gradient subtraction, collision
//   part C  needs every advected float field       advect_scalars
// The core substep (hns_sim_core_substep; `params` null) is the same sequence without its optional parts -- no collision, no vorticity, no combustion and buoyancy, never
// fused -- as Step::full() tells the two apart in the partitioned substep (hns_dist_substep.hip). It asks nothing of the sim's float fields.
// Round 6: without a collision field (and while a 16-byte-per-voxel array stays 32-bit addressable) part B opens with ONE launch for divergence + combustion +
// buoyancy (hns_divergence_combust_buoyancy: 60 B/voxel instead of 16 + 40 + 28) that leaves the four combustion fields as one 16-byte element per voxel in s->q4, and
// part C gathers those four from there (hns_advect_scalars_q4: a corner tap of the four is one gather, not four). Same expressions in the same order per voxel:
// bit-identical to the separate launches, which remain the path of the hns_dev_* entry points. With a collision field the same (the fused launch reads no SDF; part C
// launches the q4 form with its collision branch) unless option "collide" = generic, which keeps the separate launches and the 64-bit addressed advection kernels.
// Look-ahead (option "lookahead"): advect_scalars of substep n and advect_vector of substep n + 1 read the same velocity -- s->vel after the gradient subtraction -- with the same
// dt, and make the same backtrace: own velocity, neighbour tables, back position, eight tap offsets, eight 12-byte gathers. Where part C runs the float-only 32-bit form in one
// launch and there is no collision field it launches the look-ahead form (hns_dev_advect_scalars_ahead), which leaves advect_vector(s->vel, dt) in s->adv (dead since the
// gradient kernel read it) and notes what that memo is valid for; the next part A, called with exactly these arguments, skips its advect_vector launch. Bit-identical, one
// stream, 28 launches per core substep in steady state instead of 29. Every other writer of vel or adv drops the memo (hns_sim::drop_ahead).
namespace {
uint32_t float_bits(float x) {
	uint32_t b;
	memcpy(&b, &x, 4);
	return b;
}
struct Substep {
	hns_sim* s;
	int iterations;
	float dt, voxel_size, inv_dx;
	const hns_combustion_params* params;  // null: the core substep
	int ci[4];
	bool coll = false, fused = false;
	bool ahead_live = false;  // this substep may consume and produce the look-ahead memo
	const float* sdf = nullptr;
	void* stream;
	hipEvent_t* stage_events = nullptr;  // six events of hns_sim_stage_timing, or null
	bool full() const { return params != nullptr; }
	int mark(int k) {
		if (stage_events) HNS_HIP(hipEventRecord(stage_events[k], (hipStream_t)stream));
		return HNS_OK;
	}

	// What a substep with these arguments does, decided from the sim as it stands; changes nothing (hns_sim_substep_plan stops here). `capturing`: its stream is being captured.
	int decide(hns_sim* sim, int iters, float dt_, float vs, const hns_combustion_params* prm, int has_collision, void* st, bool capturing) {
		s = sim;
		iterations = iters;
		dt = dt_;
		voxel_size = vs;
		inv_dx = 1.0f / vs;
		params = prm;
		stream = st;
		ahead_live = !capturing && !s->ahead_off && options().lookahead.load() != kLookaheadOff;
		if (!full()) return HNS_OK;
		if (s->names.empty()) return fail(HNS_ERR_RUNTIME, "No float blocks found in input data.");  // :61-63
		for (int c = 0; c < 4; ++c) {                                                                 // :193-201
			ci[c] = s->find(kCombustionFields[c]);
			if (ci[c] < 0) {
				set_error("Missing required input field for combustion: %s", kCombustionFields[c]);
				return HNS_ERR_RUNTIME;
			}
		}
		const int i_sdf = has_collision ? s->find("collision_sdf") : -1;  // :66-75
		coll = i_sdf >= 0;
		sdf = coll ? s->cur[i_sdf] : nullptr;
		size_t advected = 0;
		for (const std::string& n : s->names) advected += n != "collision_sdf";
		// (every leaf active: the pointwise kernels of the separate path run over ALL voxels, read-only ghost leaves included, and advection taps read them there)
		fused = !(coll && options().collide_generic.load()) && s->q4 && s->grid->d_blk && s->grid->n_active == (uint64_t)s->grid->topo.n_leaves && !options().stencil_block.load() && hns_advect_q4_ok(s->grid) &&
		        advected - 4 <= 8 && options().fuse_pointwise.load();
		return HNS_OK;
	}
	// decide(), and what the decision does to the sim before the first launch
	int prepare(hns_sim* sim, int iters, float dt_, float vs, const hns_combustion_params* prm, int has_collision, void* st) {
		bool capturing = false;
		if (!sim->ahead_off && options().lookahead.load() != kLookaheadOff) {  // neither produce nor consume while the stream is captured: a replayed graph writes vel and adv unseen, so such a sim stops looking ahead for good
			if (stream_is_capturing(st)) capturing = true, sim->ahead_off = true;
		}
		const int rc = decide(sim, iters, dt_, vs, prm, has_collision, st, capturing);
		if (!ahead_live) s->drop_ahead();
		return rc;
	}
	// what part A, part C and hns_sim_substep_plan decide alike
	bool memo() const {  // s->adv holds advect_vector(s->vel, dt) already (with a collider part A rewrites the velocity first: never)
		const hns_grid* g = s->grid;
		const hns_sim::Ahead& m = s->ahead;
		return ahead_live && !coll && m.valid && m.grid == g && m.first == g->first_active && m.n_active == g->n_active && m.dt_bits == float_bits(dt) &&
		       m.vs_bits == float_bits(voxel_size);
	}
	bool vorticity() const { return full() && (int)params->factorScale != 0; }
	// speculate? lookahead = 1: always; auto: when the previous substep call on this sim had this dt and voxel size (a lone substep, or a changing dt, pays nothing)
	bool speculate() const {
		return ahead_live && !fused && (options().lookahead.load() == kLookaheadOn || (s->have_last && s->last_dt_bits == float_bits(dt) && s->last_vs_bits == float_bits(voxel_size)));
	}
	int part_a() {
		hns_grid* g = s->grid;
		HNS_TRY(mark(0));
		const bool memo = this->memo();
		s->drop_ahead();  // (from here on the substep overwrites adv, then vel)
		if (coll) HNS_TRY(hns_dev_enforce_collision_boundaries(g, s->vel, sdf, voxel_size, stream));  // :153-157
		if (memo)
			++s->ahead_consumed;  // s->adv holds advect_vector(s->vel, dt) already: the previous substep's part C
		else
			HNS_TRY(hns_dev_advect_vector(g, s->vel, s->adv, sdf, coll, dt, inv_dx, stream));  // :162-170
		if (vorticity()) {  // :172-176. With (int)factorScale == 0 every vorticity-magnitude tap collapses onto the centre, the
			// gradient is 0, N = 0/(0+1e-5) = 0 and the kernel writes u + dt*(scale*0) = u: a bit-exact copy, skipped.
			HNS_TRY(hns_dev_vorticity_confinement(g, s->adv, s->tmp, dt, inv_dx,
			                                      params->vorticityScale, params->factorScale, stream));
			std::swap(s->adv, s->tmp);
		}
		return HNS_OK;
	}
	int part_b() {
		hns_grid* g = s->grid;
		HNS_TRY(mark(1));
		if (fused) {  // :181-234 in one launch; the four fields' new values live in s->q4 until part C (cur[] / nxt[] of those four are not touched here)
			HNS_TRY(hns_divergence_combust_buoyancy(g, s->adv, s->div, inv_dx, s->cur[ci[0]], s->cur[ci[1]], s->cur[ci[2]], s->cur[ci[3]], s->q4, s->tmp,
			                                        params->temperatureRelease, params->expansionRate, dt, params->ambientTemp, params->buoyancyStrength, stream));
			std::swap(s->adv, s->tmp);
		} else {
			HNS_TRY(hns_dev_divergence(g, s->adv, s->div, inv_dx, stream));  // :181-188
			if (full()) {
				HNS_TRY(hns_dev_combustion_oxygen(s->cur[ci[0]], s->cur[ci[1]], s->cur[ci[2]], s->div, s->cur[ci[3]], s->nxt[ci[0]], s->nxt[ci[1]],
				                                  s->nxt[ci[2]], s->nxt[ci[3]], params->temperatureRelease, params->expansionRate, s->n, stream));  // :211-221
				HNS_TRY(hns_dev_temperature_buoyancy(s->adv, s->nxt[ci[2]], s->adv, dt, params->ambientTemp, params->buoyancyStrength, s->n,
				                                     stream));  // :226-234 (temperature AFTER combustion)
				for (int c = 0; c < 4; ++c) std::swap(s->cur[ci[c]], s->nxt[ci[c]]);  // :239-246
			}
		}
		HNS_TRY(mark(2));
		HNS_TRY(hns_sim_solve(s, iterations, voxel_size, omega_compute(voxel_size), stream));  // :256-272
		HNS_TRY(mark(3));
		HNS_TRY(hns_dev_subtract_pressure_gradient(g, s->adv, s->p_result, s->vel, sdf, coll,
		                                           inv_dx, stream));  // :278-289
		if (coll) HNS_TRY(hns_dev_enforce_collision_boundaries(g, s->vel, sdf, voxel_size, stream));  // :292-296
		return HNS_OK;
	}
	int part_c() {  // :321-356
		HNS_TRY(mark(4));
		const uint32_t dtb = float_bits(dt), vsb = float_bits(voxel_size);
		bool ahead = speculate();
		s->have_last = true, s->last_dt_bits = dtb, s->last_vs_bits = vsb, s->last_iterations = iterations;
		if (!fused) {
			HNS_TRY(sim_advect_scalars(s, sdf, coll, dt, inv_dx, stream, &ahead));
			if (ahead) {
				s->ahead = hns_sim::Ahead{true, s->grid, s->grid->first_active, s->grid->n_active, dtb, vsb};
				++s->ahead_produced;
			}
			return HNS_OK;
		}
		std::vector<const float*> ins;
		std::vector<float*> outs;
		float* q4_out[4];
		for (int c = 0; c < 4; ++c) q4_out[c] = s->nxt[ci[c]];
		for (size_t i = 0; i < s->names.size(); ++i) {
			if (s->names[i] == "collision_sdf" || (int)i == ci[0] || (int)i == ci[1] || (int)i == ci[2] || (int)i == ci[3]) continue;  // :327
			ins.push_back(s->cur[i]);
			outs.push_back(s->nxt[i]);
		}
		HNS_TRY(hns_advect_scalars_q4(s->grid, s->vel, s->q4, q4_out, ins.data(), outs.data(), (int)ins.size(), sdf, dt, inv_dx, stream));
		for (size_t i = 0; i < s->names.size(); ++i)
			if (s->names[i] != "collision_sdf") std::swap(s->cur[i], s->nxt[i]);
		return HNS_OK;
	}
	// The whole substep on one stream. hns_sim_stage_timing brackets five stages, the same for the core and the full substep -- {collision + advect_vector + vorticity,
	// divergence + combustion + buoyancy (one launch when fused), pressure loop, gradient subtraction + collision, advect_scalars}: mark(0..4) open them, mark(5) closes the last.
	// hns_sim_substep_plan: the kernel each stage of run() launches, `stage=kernel` words; what decides is the code the parts run
	std::string describe() const {
		const hns_grid* g = s->grid;
		size_t advected = 0;
		for (const std::string& n : s->names) advected += n != "collision_sdf";
		char sor[256];
		if (hns_grid_rbgs_plan(s->grid, iterations, sor, sizeof(sor), nullptr, nullptr) != HNS_OK) sor[0] = 0;
		std::string pressure = s->mg ? hns_mg_plan(s) : std::string(sor, strcspn(sor, ":"));
		std::string out = std::string("collision=") + (coll ? "k_enforce_collision" : "-");
		out += std::string(" advect_vector=") + (memo() ? "memo" : hns_advect_vector_kernel(g, sdf, coll));
		out += std::string(" vorticity=") + (vorticity() ? "k_vorticity" : "-");
		out += std::string(" divergence=") + hns_divergence_kernel(g, fused) + (!fused && full() ? "+k_combustion_oxygen+k_temperature_buoyancy" : "");
		out += " pressure=" + (pressure.empty() ? std::string("-") : pressure);
		out += std::string(" gradient=") + hns_subtract_gradient_kernel(g, sdf, coll);
		out += " advect_scalars=";
		if (fused)
			out += hns_advect_scalars_q4_kernel(sdf);
		else if (advected == 0)
			out += "-";
		else
			out += speculate() && sim_ahead_applies(s, coll, advected) ? hns_advect_scalars_ahead_kernel() : hns_advect_scalars_kernel(g, sdf, coll);
		return out;
	}
	int run() {
		stage_events = s->stage_ev.current();
		HNS_TRY(part_a());
		HNS_TRY(part_b());
		HNS_TRY(part_c());
		HNS_TRY(mark(5));
		if (stage_events) s->stage_ev.advance();
		return HNS_OK;
	}
};

// hns_sim_substep, and with `params` null hns_sim_core_substep
int sim_substep(hns_sim* s, int iterations, float dt, float voxel_size, const hns_combustion_params* params, int has_collision, void* stream) {
	HNS_TRY(validate_step(voxel_size, dt, iterations, true));
	if (s->n == 0) return HNS_OK;  // HNanoSolver.cu:26-28
	HNS_TRY(hns_solve_preflight(s, stream, params ? "hns_sim_substep" : "hns_sim_core_substep"));  // (before anything is launched)
	Substep step;
	HNS_TRY(step.prepare(s, iterations, dt, voxel_size, params, has_collision, stream));
	return step.run();
}
}  // namespace

extern "C" int hns_sim_substep(hns_sim* s, int iterations, float dt, float voxel_size, const hns_combustion_params* params, int has_collision,
                               void* stream) {
	if (!s || !params) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_substep: null argument");
	return sim_substep(s, iterations, dt, voxel_size, params, has_collision, stream);
}

// Which kernel each stage of the next hns_sim_substep (params null: hns_sim_core_substep) with these arguments launches, as `stage=kernel` words; launches nothing and
// leaves the sim as it is (Substep::decide, not prepare). The time step, the voxel size and the iteration count are taken to be those of the previous substep call on the sim
// (the first two decide whether the look-ahead memo is consumed and produced; before the first call: one iteration, which a substep needs at the least), the stream to be
// one that is not being captured (a captured substep neither consumes nor produces the memo).
extern "C" int hns_sim_substep_plan(hns_sim* s, const hns_combustion_params* params, int has_collision, char* description, uint64_t description_bytes) {
	if (!s) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_substep_plan: null sim");
	float dt = 0.0f, vs = 0.0f;
	if (s->have_last) memcpy(&dt, &s->last_dt_bits, 4), memcpy(&vs, &s->last_vs_bits, 4);
	Substep step;
	HNS_TRY(step.decide(s, s->have_last ? s->last_iterations : 1, dt, vs, params, params ? has_collision : 0, nullptr, false));
	if (description && description_bytes) snprintf(description, description_bytes, "%s", s->n == 0 ? "" : step.describe().c_str());
	return HNS_OK;
}

extern "C" int hns_sim_core_substep(hns_sim* s, int iterations, float dt, float voxel_size, void* stream) {
	if (!s) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_core_substep: null sim");
	return sim_substep(s, iterations, dt, voxel_size, nullptr, 0, stream);
}

// AdvectIndexGrid over the named float fields (n_names -1: all of them), then AdvectIndexGridVelocity, on the sim's buffers (Advection.cu:76-91,148-155): the fields read the
// velocity before its self-advection. Every check comes before the first launch.
extern "C" int hns_sim_advect(hns_sim* s, const char* const* names, int n_names, int advect_velocity, float dt, float voxel_size, void* stream) {
	const char* who = "hns_sim_advect";
	HNS_TRY(check_sim(s, who));
	HNS_TRY(validate_step(voxel_size, dt, 0, false));
	std::vector<int> which;
	HNS_TRY(sim_fields(who, "names", s, n_names, names_at(names), nullptr, true, which));
	if (s->n == 0) return HNS_OK;
	const float inv_dx = 1.0f / voxel_size;
	std::vector<const float*> ins;
	std::vector<float*> outs;
	for (int k : which) ins.push_back(s->cur[k]), outs.push_back(s->nxt[k]);
	HNS_TRY(hns_dev_advect_scalar_multi(s->grid, s->vel, ins.data(), outs.data(), (int)ins.size(), nullptr, 0, dt, inv_dx, stream));
	for (int k : which) {
		s->forget(k);
		std::swap(s->cur[k], s->nxt[k]);
	}
	if (advect_velocity) {
		s->forget(hns_sim::kVelocity);  // (drops the look-ahead memo: adv is overwritten, then becomes vel)
		HNS_TRY(hns_dev_advect_vector(s->grid, s->vel, s->adv, nullptr, 0, dt, inv_dx, stream));
		std::swap(s->vel, s->adv);
	}
	return HNS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// drop-in operators (host pointers, synchronous, in place)
// ---------------------------------------------------------------------------------------------------------------

namespace {
struct FieldSplit {
	hns_field* velocity = nullptr;
	int n_vec3 = 0;
	std::vector<hns_field*> floats;
};

int split_fields(hns_field* fields, int n_fields, FieldSplit& out, const char* who) {
	if (n_fields < 0 || (n_fields > 0 && !fields)) {
		set_error("%s: null field array", who);
		return HNS_ERR_INVALID_ARGUMENT;
	}
	for (int i = 0; i < n_fields; ++i) {
		if (fields[i].ncomp == 3) {
			if (!out.velocity) out.velocity = &fields[i];
			++out.n_vec3;
		} else if (fields[i].ncomp == 1) {
			out.floats.push_back(&fields[i]);
		} else {
			set_error("%s: field %d has ncomp %d (must be 1 or 3)", who, i, fields[i].ncomp);
			return HNS_ERR_INVALID_ARGUMENT;
		}
		if (!fields[i].name) {
			set_error("%s: field %d has no name", who, i);
			return HNS_ERR_INVALID_ARGUMENT;
		}
	}
	return HNS_OK;
}

// Persistent state across cooks (the reference's cook cache is an empty struct, SOP_HNanoSolver.hpp:60-64,
// and every cook pays cudaMallocAsync x 15+ and the matching frees, HNanoSolver.cu:87-133). An operator call borrows a
// device-resident hns_sim for its field-name list from the grid and returns it afterwards; the buffers live until the
// grid is destroyed or hns_grid_release_cache() is called. Two entries cover the usual "full solver + one single-field
// operator" pattern; a call that finds its entry lent out (concurrent cooks on one grid) works on a private sim.
// Option "cook_cache" = 0 disables the cache.
struct SimGuard {
	hns_sim* s = nullptr;
	~SimGuard() {
		if (!s) return;
		if (!s->cached) {
			hns_sim_destroy(s);
			return;
		}
		std::lock_guard<std::mutex> lock(s->grid->host_mutex);
		s->in_use = false;
	}
};

int make_sim(hns_grid* g, const std::vector<hns_field*>& floats, SimGuard& guard, void* stream) {
	std::vector<const char*> names;
	for (hns_field* f : floats) names.push_back(f->name);
	const bool use_cache = options().cook_cache.load() != 0;
	if (use_cache) {
		std::lock_guard<std::mutex> lock(g->host_mutex);
		for (hns_sim* c : g->sim_cache) {
			if (c->in_use || c->names.size() != names.size()) continue;
			bool same = true;
			for (size_t i = 0; i < names.size() && same; ++i) same = c->names[i] == names[i];
			if (!same) continue;
			c->in_use = true;
			guard.s = c;
			break;
		}
	}
	if (guard.s) {
		guard.s->ahead_off = true, guard.s->drop_ahead();  // (operator calls upload a velocity per call and write vel / adv themselves: nothing to look ahead for)
		// A fresh sim starts zeroed and a substep only writes the active leaves; with an active prefix
		// (hns_grid_set_active_leaves) restore that guarantee for everything a kernel may read across a leaf face.
		if (g->n_active != (uint64_t)g->topo.n_leaves) {
			hns_sim* s = guard.s;
			const size_t bytes = sizeof(float) * (size_t)s->n;
			hipStream_t st = (hipStream_t)stream;
			HNS_HIP(hipMemsetAsync(s->div, 0, bytes, st));
			HNS_HIP(hipMemsetAsync(s->p_a, 0, bytes, st));
			HNS_HIP(hipMemsetAsync(s->p_b, 0, bytes, st));
			HNS_HIP(hipMemsetAsync(s->adv, 0, 3 * bytes, st));
			HNS_HIP(hipMemsetAsync(s->tmp, 0, 3 * bytes, st));
			for (float* q : s->nxt) HNS_HIP(hipMemsetAsync(q, 0, bytes, st));
		}
		return HNS_OK;
	}
	int err = HNS_OK;
	// every operator writes each buffer before it reads it when all leaves are active, so the new memory is not cleared
	guard.s = sim_create(g, names.data(), (int)names.size(), g->n_active != (uint64_t)g->topo.n_leaves, stream, &err);
	if (guard.s) guard.s->ahead_off = true;
	if (err != HNS_OK || !use_cache) return err;
	std::lock_guard<std::mutex> lock(g->host_mutex);
	if (g->sim_cache.size() >= 2) {  // evict the oldest entry that is not lent out
		for (size_t i = 0; i < g->sim_cache.size(); ++i)
			if (!g->sim_cache[i]->in_use) {
				g->sim_cache[i]->cached = false;
				hns_sim_destroy(g->sim_cache[i]);
				g->sim_cache.erase(g->sim_cache.begin() + (long)i);
				break;
			}
	}
	if (g->sim_cache.size() < 2) {
		guard.s->cached = guard.s->in_use = true;
		g->sim_cache.push_back(guard.s);
	}
	return HNS_OK;
}

// How the four velocity-driven operators open: the grid, the field list, exactly one Vec3f block. What only one of them checks follows in that operator.
int operator_fields(hns_grid* g, hns_field* fields, int n_fields, const char* who, FieldSplit& fs) {
	if (!g) {
		set_error("%s: null grid", who);
		return HNS_ERR_INVALID_ARGUMENT;
	}
	HNS_TRY(split_fields(fields, n_fields, fs, who));
	if (fs.n_vec3 != 1) return fail(HNS_ERR_RUNTIME, "Expected exactly one Vec3f block (velocity)");  // Advection.cu:19-21,119-121, PressureProjection.cu:14-17,85-88
	return HNS_OK;
}

// ... and how they get to the device once their checks have passed: a sim borrowed for the float blocks `floats` (none: the velocity alone), with `up` uploaded. An empty
// grid leaves guard.s null: the operator has nothing to do.
int operator_sim(hns_grid* g, const char* who, const std::vector<hns_field*>& floats, const hns_field* up, int n_up, SimGuard& guard, void* stream) {
	if (hns_grid_voxel_count(g) == 0) return HNS_OK;
	if (!g->on_device) {
		set_error("%s: grid has no device tables (there is no CPU fallback)", who);
		return HNS_ERR_NO_DEVICE;
	}
	HNS_TRY(make_sim(g, floats, guard, stream));
	return hns_sim_upload(guard.s, up, n_up, stream);
}
}  // namespace

// hns_compute_sim's data movement. The reference uploads everything, runs, downloads everything (HNanoSolver.cu:87-133,
// 361-371). Here the fields go up in the order the substep consumes them, on a transfer stream of the sim's own, and each
// part of the substep is enqueued on the caller's stream as soon as its inputs are queued: advect_vector runs under the
// upload of the four combustion fields, the pressure solve under the upload of every other field (Substep::part_b),
// and advect_scalars under the download of the final velocity. Same kernels, same order per buffer; only the overlap
// differs. Option "cook_pipeline" = 0 falls back to upload-all / run / download-all.
// What a host array and the device buffer it was downloaded from have in common afterwards. Two strengths (hns_compute_sim_resident):
//  * the SAMPLE signature: element count and 4,096 evenly spread elements, hashed (FNV-1a over their bits). 16 KB read out of 67 - 201 MB: a tripwire
//    against handing in a different array, NOT a check of the promise -- an edit that misses the samples (an emitter added to a few leaves) passes.
//    resident[i] = 1 ("vouched") relies on the caller knowing what it changed, as the reference's SOP does (it adds its sources itself,
//    SOP_HNanoSolver.cpp:159-179, and must not flag a field it sourced into);
//  * the FULL digest (hns_digest.hpp): every element, an order-independent sum over 16-byte pieces -- taken on the DEVICE when a field is handed back (beside the
//    downloads) and on up to 8 HOST threads when the array comes in again (~5.5 ms for the 537 MB of a 256^3 cook, partly under the first kernels).
//    resident[i] = 2 ("checked"): an edit goes unnoticed only if the 64-bit digests collide (probability ~2^-64 for an edit that is not crafted against the digest); 14.8 ms per cook at 256^3 against 19.8 plain and 11.9 vouched.
// Neither is ever 0.
static uint64_t host_signature(const float* a, size_t count) {
	uint64_t h = 1469598103934665603ull ^ (uint64_t)count;
	const size_t samples = count < 4096 ? count : 4096;
	for (size_t i = 0; i < samples; ++i) {
		uint32_t bits;
		memcpy(&bits, a + (samples == count ? i : (size_t)(((unsigned __int128)i * count) / samples)), 4);
		h = (h ^ bits) * 1099511628211ull;
	}
	return h ? h : 1;
}
static uint64_t host_digest(const float* a, size_t count) {  // hns_digest.hpp: the number k_field_digest takes of the device copy of the same bits
	const size_t n_pieces = count / 4;
	constexpr size_t kChunk = (size_t)1 << 14;  // pieces per chunk (256 KiB)
	const size_t n_chunks = (n_pieces + kChunk - 1) / kChunk;
	std::vector<uint64_t> part(std::max<size_t>(1, n_chunks), 0);
	auto work = [&](size_t c0, size_t c1) {
		for (size_t c = c0; c < c1; ++c) {
			const size_t lo = c * kChunk, hi = std::min(n_pieces, lo + kChunk);
			uint64_t s0 = 0, s1 = 0;
			size_t i = lo;
			for (; i + 2 <= hi; i += 2) {  // two independent accumulators
				uint64_t w[4];
				memcpy(w, a + 4 * i, 32);
				s0 += hns_digest_piece(i, w[0], w[1]);
				s1 += hns_digest_piece(i + 1, w[2], w[3]);
			}
			for (; i < hi; ++i) {
				uint64_t w[2];
				memcpy(w, a + 4 * i, 16);
				s0 += hns_digest_piece(i, w[0], w[1]);
			}
			part[c] = s0 + s1;
		}
	};
	const size_t n_threads = std::min<size_t>(8, std::max<size_t>(1, n_chunks / 8));  // (2 MiB and more per thread: a thread costs ~30 us to start)
	if (n_threads <= 1) work(0, n_chunks);
	else {
		std::vector<std::thread> th;
		for (size_t t = 1; t < n_threads; ++t) th.emplace_back(work, n_chunks * t / n_threads, n_chunks * (t + 1) / n_threads);
		work(0, n_chunks / n_threads);
		for (auto& t : th) t.join();
	}
	uint64_t sum = 0;
	for (uint64_t p : part) sum += p;
	if (count & 3) {  // a zero-padded last piece
		uint32_t w[4] = {0, 0, 0, 0};
		memcpy(w, a + 4 * n_pieces, 4 * (count & 3));
		sum += hns_digest_piece(n_pieces, (uint64_t)w[0] | (uint64_t)w[1] << 32, (uint64_t)w[2] | (uint64_t)w[3] << 32);
	}
	return hns_digest_finish(sum, count);
}

// `resident` (hns_compute_sim_resident): per field of `fields` (by position), non-zero = the caller vouches that the host array still
// holds what the previous hns_compute_sim on this grid handed back for the block of that name. The field is then not uploaded -- if
// the device state lent to this call is the one that produced it and the array's signature still matches; uploaded as usual otherwise.
namespace {
struct Cook {
	hns_sim* s;
	const hns_field* fields;  // the caller's array: fs points into it, `resident` runs beside it
	int n_fields;
	FieldSplit& fs;
	const unsigned char* resident;
	int* skipped;
	int iterations;
	float dt, voxel_size;
	const hns_combustion_params* params;
	int has_collision;
	hipStream_t st;
	std::vector<std::pair<uint64_t*, size_t>> dig_slots = {};  // (where the digest goes, its element count), in the order of s->d_dig

	size_t count() const { return (size_t)s->n; }
	int level_of(const hns_field* f) const { return resident ? resident[f - fields] : 0; }
	static bool is_sdf(const hns_field* f) { return !strcmp(f->name, "collision_sdf"); }
	static bool is_combustion_field(const hns_field* f) {
		return std::any_of(kCombustionFields, kCombustionFields + 4, [f](const char* n) { return !strcmp(f->name, n); });
	}

	bool stays(const hns_field* f) {
		const int level = level_of(f);
		if (!level) return false;
		hns_sim::Handed have;
		const size_t n = (size_t)f->ncomp * count();
		if (f->ncomp == 3) have = s->handed_vel;
		else if (const int k = s->find(f->name); k >= 0) have = s->handed_cur[(size_t)k];
		if (!have.sig || have.sig != host_signature(f->host, n)) return false;
		if (level >= 2 && (!have.dig || have.dig != host_digest(f->host, n))) return false;  // (no digest taken last cook: nothing to check against -> upload)
		if (skipped) ++*skipped;
		return true;
	}
	int upload(hns_field* f, hipStream_t on) { return stays(f) ? (int)HNS_OK : hns_sim_upload(s, f, 1, on); }

	// the full digest of a CHECKED field is taken ON THE DEVICE, of the buffer the host array is downloaded from (the same bits), behind the last kernel of the
	// substep and beside the downloads: one pass at memory speed instead of a second host pass over every array
	int digest_on_device(hipStream_t on) {
		std::vector<const float*> bufs;
		if (level_of(fs.velocity) >= 2) bufs.push_back(s->vel), dig_slots.emplace_back(&s->handed_vel.dig, 3 * count());
		for (hns_field* f : fs.floats) {
			const int k = s->find(f->name);
			if (k >= 0 && !is_sdf(f) && level_of(f) >= 2) bufs.push_back(s->cur[(size_t)k]), dig_slots.emplace_back(&s->handed_cur[(size_t)k].dig, count());
		}
		if (bufs.empty()) return HNS_OK;
		if (!s->h_dig) HNS_HIP(hipHostMalloc((void**)&s->h_dig, sizeof(unsigned long long) * 16, hipHostMallocDefault));  // (host memory: no device synchronisation)
		HNS_HIP(hipMemsetAsync(s->d_dig, 0, sizeof(unsigned long long) * 16, on));
		for (size_t i = 0; i < bufs.size(); ++i) HNS_TRY(hns_field_digest(bufs[i], dig_slots[i].second, s->d_dig + i, on));
		HNS_HIP(hipMemcpyAsync(s->h_dig, s->d_dig, sizeof(unsigned long long) * 16, hipMemcpyDeviceToHost, on));  // (on the cook's own stream, in front of its final synchronise: ADVICE r5)
		return HNS_OK;
	}
	int sign() {  // (the downloads and the digest kernels have completed: what the host arrays hold now is what vel / cur[] hold)
		s->handed_vel = {host_signature(fs.velocity->host, 3 * count()), 0};
		for (hns_field* f : fs.floats) {
			const int k = s->find(f->name);
			if (k >= 0) s->handed_cur[(size_t)k] = {is_sdf(f) ? 0 : host_signature(f->host, count()), 0};  // (the SDF comes back zeroed, the device keeps it)
		}
		for (size_t i = 0; i < dig_slots.size(); ++i) *dig_slots[i].first = hns_digest_finish(s->h_dig[i], dig_slots[i].second);  // (the stream the copy ran on has been synchronised)
		return HNS_OK;
	}

	// option "cook_pipeline" = 0: upload all / run / download all, on the caller's stream
	int plain() {
		std::vector<hns_field> all;
		HNS_TRY(upload(fs.velocity, st));
		all.push_back(*fs.velocity);
		for (hns_field* f : fs.floats) {
			HNS_TRY(upload(f, st));
			all.push_back(*f);
		}
		HNS_TRY(hns_sim_substep(s, iterations, dt, voxel_size, params, has_collision, st));
		HNS_TRY(digest_on_device(st));
		HNS_TRY(hns_sim_download(s, all.data(), (int)all.size(), st));
		return sign();
	}

	static int handoff(hipEvent_t e, hipStream_t from, hipStream_t to) {
		HNS_HIP(hipEventRecord(e, from));
		HNS_HIP(hipStreamWaitEvent(to, e, 0));
		return HNS_OK;
	}
	int pipelined() {
		if (!s->xfer) {
			HNS_HIP(hipStreamCreateWithFlags(&s->xfer, hipStreamNonBlocking));
			for (hipEvent_t& e : s->xev) HNS_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
		}
		hipStream_t xf = s->xfer;
		Substep step;
		HNS_TRY(step.prepare(s, iterations, dt, voxel_size, params, has_collision, st));
		HNS_TRY(handoff(s->xev[0], st, xf));  // transfers start after whatever the caller's stream holds
		if (step.coll)
			for (hns_field* f : fs.floats)
				if (is_sdf(f)) HNS_TRY(hns_sim_upload(s, f, 1, xf));
		HNS_TRY(upload(fs.velocity, xf));
		HNS_TRY(handoff(s->xev[1], xf, st));
		HNS_TRY(step.part_a());
		for (hns_field* f : fs.floats)
			if (is_combustion_field(f)) HNS_TRY(upload(f, xf));
		HNS_TRY(handoff(s->xev[2], xf, st));
		HNS_TRY(step.part_b());  // the solve runs while every remaining field is still on its way
		HNS_HIP(hipEventRecord(s->xev[3], st));  // s->vel is final here
		for (hns_field* f : fs.floats)  // "collision_sdf" went up first if this call uses it; if not, nothing reads it and it returns zeroed
			if (!is_combustion_field(f) && !is_sdf(f)) HNS_TRY(upload(f, xf));
		HNS_TRY(handoff(s->xev[4], xf, st));
		HNS_TRY(step.part_c());
		HNS_TRY(digest_on_device(st));  // (every field is final on the device here; the kernels run beside the downloads)
		HNS_HIP(hipStreamWaitEvent(xf, s->xev[3], 0));
		HNS_HIP(hipMemcpyAsync(fs.velocity->host, s->vel, sizeof(float) * 3 * count(), hipMemcpyDeviceToHost, xf));
		HNS_TRY(handoff(s->xev[0], st, xf));  // (xev[0] again: its first use is long past)
		std::vector<hns_field> outs;
		for (hns_field* f : fs.floats)
			if (!is_sdf(f)) outs.push_back(*f);  // the caller's SDF array comes back zeroed (hns_compute_sim): no bytes to fetch
		HNS_TRY(hns_sim_download(s, outs.data(), (int)outs.size(), xf));  // synchronises xf
		HNS_HIP(hipStreamSynchronize(st));
		return sign();
	}

	int run() {
		int checked = 0;  // (refused before anything is enqueued: the digest kernels have 16 accumulators)
		for (int i = 0; resident && i < n_fields; ++i) checked += resident[i] >= 2 ? 1 : 0;
		if (checked > 16) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_compute_sim_resident: more than 16 CHECKED fields");
		return options().cook_pipeline.load() ? pipelined() : plain();
	}
};
}  // namespace

extern "C" int hns_compute_sim(hns_grid* g, hns_field* fields, int n_fields, int iterations, float dt, float voxel_size,
                               const hns_combustion_params* params, int has_collision, void* stream) {
	return hns_compute_sim_resident(g, fields, n_fields, nullptr, nullptr, iterations, dt, voxel_size, params, has_collision, stream);
}

extern "C" int hns_compute_sim_resident(hns_grid* g, hns_field* fields, int n_fields, const unsigned char* resident, int* uploads_skipped, int iterations, float dt,
                                        float voxel_size, const hns_combustion_params* params, int has_collision, void* stream) {
	if (uploads_skipped) *uploads_skipped = 0;
	HNS_TRY(validate_step(voxel_size, dt, iterations, true));
	if (!g) return fail(HNS_ERR_INVALID_ARGUMENT, "Invalid grid handle provided (null grid).");  // HNanoSolver.cu:21-23
	if (!params) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_compute_sim: null combustion params");
	if (hns_grid_voxel_count(g) == 0) return HNS_OK;  // :26-28
	FieldSplit fs;
	HNS_TRY(split_fields(fields, n_fields, fs, "hns_compute_sim"));
	if (fs.n_vec3 != 1) {  // :42-45
		set_error("Expected exactly one Vec3f block (velocity), found %d", fs.n_vec3);
		return HNS_ERR_RUNTIME;
	}
	if (!fs.velocity->host) return fail(HNS_ERR_RUNTIME, "Host velocity data pointer is null");  // :48-51
	if (fs.floats.empty()) return fail(HNS_ERR_RUNTIME, "No float blocks found in input data.");  // :61-63
	for (hns_field* f : fs.floats)
		if (!f->host) {
			set_error("Host float data pointer is null for block: %s", f->name);  // :80-82
			return HNS_ERR_RUNTIME;
		}
	if (!g->on_device) return fail(HNS_ERR_NO_DEVICE, "hns_compute_sim: grid has no device tables (there is no CPU fallback)");
	SimGuard guard;
	HNS_TRY(make_sim(g, fs.floats, guard, stream));
	Cook cook{guard.s, fields, n_fields, fs, resident, uploads_skipped, iterations, dt, voxel_size, params, has_collision, (hipStream_t)stream};
	if (int rc = cook.run()) {
		guard.s->forget();  // whatever the buffers hold now, nobody was handed it
		// copies on the transfer stream and kernels on the caller's may still be queued: let them finish before the
		// guard hands the buffers on (and before the caller reuses its host arrays)
		if (guard.s->xfer) (void)hipStreamSynchronize(guard.s->xfer);
		(void)hipStreamSynchronize((hipStream_t)stream);
		return rc;
	}
	// The reference copies every float block back from its OUTPUT buffer; "collision_sdf" is never advected, so its
	// output buffer is still the memset zeros and the caller's SDF array comes back zeroed (HNanoSolver.cu:115-117,327,364-369).
	for (hns_field* f : fs.floats)
		if (strcmp(f->name, "collision_sdf") == 0) memset(f->host, 0, sizeof(float) * (size_t)hns_grid_voxel_count(g));
	return HNS_OK;
}

extern "C" int hns_advect_index_grid(hns_grid* g, hns_field* fields, int n_fields, float dt, float voxel_size, void* stream) {
	FieldSplit fs;
	HNS_TRY(operator_fields(g, fields, n_fields, "hns_advect_index_grid", fs));
	if (fs.floats.empty()) return fail(HNS_ERR_RUNTIME, "No float blocks found");                     // Advection.cu:27-29
	if (!fs.velocity->host) return fail(HNS_ERR_RUNTIME, "Velocity data not found");                  // :32-34
	for (hns_field* f : fs.floats)
		if (!f->host) {
			set_error("Block '%s' not found or type mismatch", f->name);  // :46-48
			return HNS_ERR_RUNTIME;
		}
	SimGuard guard;
	HNS_TRY(operator_sim(g, "hns_advect_index_grid", fs.floats, fields, n_fields, guard, stream));
	hns_sim* s = guard.s;
	if (!s) return HNS_OK;
	const float inv_dx = 1.0f / voxel_size;
	// advect_scalar of every float block (Advection.cu:88-91: one launch per block), here with one back-trace for all of them: the same bits
	HNS_TRY(hns_dev_advect_scalar_multi(g, s->vel, s->cur.data(), s->nxt.data(), (int)s->names.size(), nullptr, 0, dt, inv_dx, stream));
	for (size_t i = 0; i < s->names.size(); ++i) std::swap(s->cur[i], s->nxt[i]);
	std::vector<hns_field> outs;
	for (hns_field* f : fs.floats) outs.push_back(*f);  // velocity is not copied back (Advection.cu:94-96)
	return hns_sim_download(s, outs.data(), (int)outs.size(), stream);
}

extern "C" int hns_advect_index_grid_velocity(hns_grid* g, hns_field* fields, int n_fields, float dt, float voxel_size, void* stream) {
	FieldSplit fs;
	HNS_TRY(operator_fields(g, fields, n_fields, "hns_advect_index_grid_velocity", fs));
	if (!fs.velocity->host) return fail(HNS_ERR_RUNTIME, "Velocity data not found");
	SimGuard guard;
	HNS_TRY(operator_sim(g, "hns_advect_index_grid_velocity", {}, fs.velocity, 1, guard, stream));
	hns_sim* s = guard.s;
	if (!s) return HNS_OK;
	HNS_TRY(hns_dev_advect_vector(g, s->vel, s->adv, nullptr, 0, dt, 1.0f / voxel_size, stream));
	std::swap(s->vel, s->adv);
	return hns_sim_download(s, fs.velocity, 1, stream);
}

extern "C" int hns_project_non_divergent(hns_grid* g, hns_field* fields, int n_fields, uint64_t iterations, float voxel_size, void* stream) {
	FieldSplit fs;
	HNS_TRY(operator_fields(g, fields, n_fields, "hns_project_non_divergent", fs));
	if (!fs.velocity->host) return fail(HNS_ERR_RUNTIME, "Velocity data not found");
	if (voxel_size <= 0.0f) return fail(HNS_ERR_INVALID_ARGUMENT, "voxelSize must be positive.");
	if (iterations > 0x7fffffffull) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_project_non_divergent: iteration count too large");
	SimGuard guard;
	HNS_TRY(operator_sim(g, "hns_project_non_divergent", {}, fs.velocity, 1, guard, stream));
	hns_sim* s = guard.s;
	if (!s) return HNS_OK;
	const float inv_dx = 1.0f / voxel_size;
	HNS_TRY(hns_dev_divergence(g, s->vel, s->div, inv_dx, stream));              // PressureProjection.cu:48
	HNS_TRY(hns_sim_solve(s, (int)iterations, voxel_size, omega_project(voxel_size), stream));            // :51-60 (0 iterations leaves p = 0)
	HNS_TRY(hns_dev_subtract_pressure_gradient(g, s->vel, s->p_result, s->vel, nullptr, 0,
	                                           inv_dx, stream));  // :64, in place
	return hns_sim_download(s, fs.velocity, 1, stream);
}

extern "C" int hns_divergence(hns_grid* g, hns_field* fields, int n_fields, float voxel_size, void* stream) {
	FieldSplit fs;
	HNS_TRY(operator_fields(g, fields, n_fields, "hns_divergence", fs));
	if (!fs.velocity->host) return fail(HNS_ERR_RUNTIME, "Velocity data not found");
	hns_field* out = nullptr;
	for (hns_field* f : fs.floats)
		if (strcmp(f->name, "divergence") == 0) out = f;  // PressureProjection.cu:91
	if (!out || !out->host) return fail(HNS_ERR_RUNTIME, "hns_divergence: no float block named 'divergence' to receive the result");
	if (voxel_size <= 0.0f) return fail(HNS_ERR_INVALID_ARGUMENT, "voxelSize must be positive.");
	SimGuard guard;
	HNS_TRY(operator_sim(g, "hns_divergence", {}, fs.velocity, 1, guard, stream));
	hns_sim* s = guard.s;
	if (!s) return HNS_OK;
	HNS_TRY(hns_dev_divergence(g, s->vel, s->div, 1.0f / voxel_size, stream));
	HNS_HIP(hipMemcpyAsync(out->host, s->div, sizeof(float) * (size_t)s->n, hipMemcpyDeviceToHost, (hipStream_t)stream));
	HNS_HIP(hipStreamSynchronize((hipStream_t)stream));
	return HNS_OK;
}
