// hns_diagnostics.hip -- what a device-resident sim can say about itself without a download (include/hns.h: "Diagnostics"): statistics of its fields, the residual
// of its pressure solve, and what a solve control adds to the solve's driver so that it stops on that residual (hns_pressure.hip: hns_sim_solve). Hand-written HIP for gfx950 / CDNA4, wave64.
//
// Everything ends in hns_stats records, and every record comes out of ONE reduction (hns_stats.hpp; the host mirror hns_leaf_stats walks the same trees):
//   a wave turns one leaf of one component into a partial record (leaf_record: per-lane sums over voxels 64k + lane, then an xor butterfly) and writes it into a table,
//   one row of n_leaves records per component; a second small launch (k_stats_fold: one workgroup per row) folds each row through the balanced tree over leaf index.
// No float or double atomics, no order that depends on where a workgroup ran: two calls give the same bytes.
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "hns_device.hpp"
#include "hns_stats.hpp"

namespace hns {
namespace {

// ---------------------------------------------------------------------------------------------------------------
// the reduction inside a leaf
// ---------------------------------------------------------------------------------------------------------------

// x[k]: the value of voxel 64k + lane; act[k] (wave-uniform): the voxels of round k that take part. Every lane returns the leaf's record.
__device__ __forceinline__ hns_stats leaf_record(const float (&x)[8], const uint64_t (&act)[8], const int lane) {
	double sum = 0.0, sq = 0.0;
	uint32_t kmin = kStatsKeyPosInf, kmax = kStatsKeyNegInf, kabs = 0;
	unsigned count = 0, nans = 0;
#pragma unroll
	for (int k = 0; k < 8; ++k) {
		const bool on = (act[k] >> lane) & 1;
		const bool nan = x[k] != x[k];
		count += (unsigned)__popcll(act[k]);
		nans += (unsigned)__popcll(__ballot(on && nan));
		const bool use = on && !nan;
		const double t = use ? (double)x[k] : 0.0;
		sum = k ? sum + t : t;
		sq = k ? sq + t * t : t * t;
		const uint32_t key = stats_key(x[k]);
		kmin = use && key < kmin ? key : kmin;
		kmax = use && key > kmax ? key : kmax;
		const uint32_t mag = __float_as_uint(x[k]) & 0x7FFFFFFFu;
		kabs = use && mag > kabs ? mag : kabs;
	}
#pragma unroll
	for (int m = 1; m < 64; m *= 2) {
		sum = sum + __shfl_xor(sum, m);
		sq = sq + __shfl_xor(sq, m);
		kmin = min(kmin, (uint32_t)__shfl_xor((int)kmin, m));
		kmax = max(kmax, (uint32_t)__shfl_xor((int)kmax, m));
		kabs = max(kabs, (uint32_t)__shfl_xor((int)kabs, m));
	}
	hns_stats r;
	r.count = count, r.nan_count = nans;
	r.min = stats_unkey(kmin), r.max = stats_unkey(kmax), r.max_abs = __uint_as_float(kabs);
	r.reserved = 0;
	r.sum = sum, r.sum_sq = sq;
	return r;
}

// ---------------------------------------------------------------------------------------------------------------
// field statistics: one wave per leaf, four leaves per workgroup (the shape of k_deactivate, hns_regrid.hip)
// ---------------------------------------------------------------------------------------------------------------

struct StatRow {
	const float* p;
	int ncomp;
	int first;  // the table row of its first component
};
constexpr int kStatRows = 16;  // fields per launch (they travel as the kernel argument)
struct StatRows {
	StatRow f[kStatRows];
	int n;
};

// masks null: every voxel. Reads only: eight raw buffer loads in flight per field, a round without an active voxel loads nothing.
// WORDS: the masks are 8-byte aligned (the library's own always are) and lane k < 8 loads the 64-bit word of round k. Else they are a caller's byte array, which may start at
// any byte (include/hns.h: an unsigned char* needs no alignment): lane k puts the word together from its eight bytes, lowest first -- the same value.
template <bool WORDS>
__device__ __forceinline__ void field_stats(const StatRows& rows, const unsigned char* __restrict__ masks, const uint64_t n_leaves, hns_stats* __restrict__ table) {
	const uint64_t leaf = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
	if (leaf >= n_leaves) return;  // (whole waves)
	const int lane = (int)(threadIdx.x & 63);
	uint64_t word = ~0ull;
	if (masks && lane < 8) {
		const unsigned char* b = masks + 64 * leaf + 8 * (uint64_t)lane;
		if (WORDS) {
			word = *reinterpret_cast<const uint64_t*>(b);
		} else {
			word = 0;
#pragma unroll
			for (int k = 0; k < 8; ++k) word |= (uint64_t)b[k] << (8 * k);
		}
	}
	uint64_t act[8];
#pragma unroll
	for (int k = 0; k < 8; ++k) act[k] = readlane64(word, k);
	for (int f = 0; f < rows.n; ++f) {
		const StatRow e = rows.f[f];
		hns_stats* out = table + (uint64_t)e.first * n_leaves + leaf;
		if (e.ncomp == 1) {
			const v4i r = field_rsrc(e.p + 512 * leaf, 2048u);
			float x[8];
#pragma unroll
			for (int k = 0; k < 8; ++k) x[k] = hns_buffer_load_f32(r, act[k] ? 4 * (64 * k + lane) : kActSkip, 0, 0);
			const hns_stats rec = leaf_record(x, act, lane);
			if (lane == 0) out[0] = rec;
		} else {
			const v4i r = field_rsrc(e.p + 1536 * leaf, 6144u);
			v3f x[8];
#pragma unroll
			for (int k = 0; k < 8; ++k) x[k] = hns_buffer_load_v3f32(r, act[k] ? 12 * (64 * k + lane) : kActSkip, 0, 0);
			float c[8];
#pragma unroll
			for (int k = 0; k < 8; ++k) c[k] = x[k].x;
			const hns_stats r0 = leaf_record(c, act, lane);
#pragma unroll
			for (int k = 0; k < 8; ++k) c[k] = x[k].y;
			const hns_stats r1 = leaf_record(c, act, lane);
#pragma unroll
			for (int k = 0; k < 8; ++k) c[k] = x[k].z;
			const hns_stats r2 = leaf_record(c, act, lane);
			if (lane == 0) out[0] = r0, out[n_leaves] = r1, out[2 * n_leaves] = r2;
		}
	}
}

__global__ __launch_bounds__(256) void k_field_stats(const StatRows rows, const unsigned char* __restrict__ masks, const uint64_t n_leaves, hns_stats* __restrict__ table) {
	field_stats<true>(rows, masks, n_leaves, table);
}
__global__ __launch_bounds__(256) void k_field_stats_bytes(const StatRows rows, const unsigned char* __restrict__ masks, const uint64_t n_leaves, hns_stats* __restrict__ table) {
	field_stats<false>(rows, masks, n_leaves, table);
}

// The tree over leaves (hns_stats.hpp: stats_fold), in place: workgroup b folds row b of the table (n records) and writes out[b]. n = 0: the record of nothing.
__global__ __launch_bounds__(1024) void k_stats_fold(hns_stats* __restrict__ table, const uint64_t n, hns_stats* __restrict__ out) {
	hns_stats* t = table + (uint64_t)blockIdx.x * n;
	for (uint64_t s = 1; s < n; s *= 2) {
		for (uint64_t i = 2 * s * threadIdx.x; i < n; i += 2 * s * 1024u) {
			hns_stats a = t[i];
			stats_combine(a, i + s < n ? t[i + s] : stats_empty());
			t[i] = a;
		}
		__syncthreads();
	}
	if (threadIdx.x == 0) {
		hns_stats r = n ? t[0] : stats_empty();
		stats_finish(r);
		out[blockIdx.x] = r;
	}
}

// ---------------------------------------------------------------------------------------------------------------
// the pressure residual: one wave per leaf
// ---------------------------------------------------------------------------------------------------------------

// c = gs_value(six neighbours of p, div, dx2) - p over every voxel of the leaves of the launch range. The tile of p is staged as the gradient subtraction stages it
// (stage_tile_wave); the divergence streams through as two 16-byte pieces per lane, lane l holding voxels 4(l + 64j) .. + 3 -- through a per-leaf buffer descriptor, 32-bit
// offsets, bounds tested by the hardware. The reduction wants voxel 64k + lane in round k, so c crosses LDS once (2 KiB, conflict-free either way). 8 B/voxel.
__global__ __launch_bounds__(64) void k_residual(const GridDev g, const float* __restrict__ div, const float* __restrict__ p, const float dx2, float* c_out,
                                                 hns_stats* __restrict__ table) {
	__shared__ __attribute__((aligned(16))) float P[kTile];
	__shared__ __attribute__((aligned(16))) float Cs[512];
	const int l = threadIdx.x;
	const int* __restrict__ rec = g.blk + (size_t)launch_pos(g, blockIdx.x) * 28;
	const int leaf = __builtin_amdgcn_readfirstlane(rec[0]);
	const v4i rd = field_rsrc(div + (size_t)leaf * 512, 2048u);
	v4f32 d[2];
#pragma unroll
	for (int j = 0; j < 2; ++j) d[j] = hns_buffer_load_v4f32(rd, 16 * (l + 64 * j), 0, 0);
	stage_tile_wave(P, p, rec, leaf, l);
	__syncthreads();
	const v4i rc = field_rsrc(c_out + (size_t)leaf * 512, c_out ? 2048u : 0u);  // (no c_out: an empty descriptor, the stores are dropped)
#pragma unroll
	for (int j = 0; j < 2; ++j) {
		v4f32 c;
#pragma unroll
		for (int e = 0; e < 4; ++e) {
			const int v = 4 * (l + 64 * j) + e;
			c[e] = gs_value(P[tile_nbr<0, 1>(v)], P[tile_nbr<0, -1>(v)], P[tile_nbr<1, 1>(v)], P[tile_nbr<1, -1>(v)], P[tile_nbr<2, 1>(v)], P[tile_nbr<2, -1>(v)], d[j][e], dx2) - P[v];
		}
		*reinterpret_cast<v4f32*>(&Cs[4 * (l + 64 * j)]) = c;
		hns_buffer_store_v4f32(c, rc, 16 * (l + 64 * j), 0, 0);
	}
	__syncthreads();
	float x[8];
	uint64_t all[8];
#pragma unroll
	for (int k = 0; k < 8; ++k) x[k] = Cs[64 * k + l], all[k] = ~0ull;
	const hns_stats r = leaf_record(x, all, l);
	if (l == 0) table[leaf - g.first] = r;
}

// ---------------------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------------------

constexpr size_t kRecordBytes = 4096;  // head of a sim's diagnostics allocation: the records its calls leave (85 of them)
constexpr size_t kRecordsMax = kRecordBytes / sizeof(hns_stats);

// rows of fields over n_leaves leaves -> n_records records at d_out; table: n_records x n_leaves partial records
int launch_stats(const std::vector<StatRow>& rows, int n_records, const unsigned char* masks, uint64_t n_leaves, hns_stats* table, hns_stats* d_out, hipStream_t st,
                 const char* who) {
	for (size_t i0 = 0; i0 < rows.size() && n_leaves; i0 += kStatRows) {
		StatRows a{};
		a.n = (int)std::min<size_t>(kStatRows, rows.size() - i0);
		for (int j = 0; j < a.n; ++j) a.f[j] = rows[i0 + (size_t)j];
		if (((uintptr_t)masks & 7) == 0)
			k_field_stats<<<(unsigned)((n_leaves + 3) / 4), 256, 0, st>>>(a, masks, n_leaves, table);
		else
			k_field_stats_bytes<<<(unsigned)((n_leaves + 3) / 4), 256, 0, st>>>(a, masks, n_leaves, table);
	}
	k_stats_fold<<<(unsigned)n_records, 1024, 0, st>>>(table, n_leaves, d_out);
	return launch_status(who);
}

// hns_dev_residual without its argument checks; table: n_active partial records
int launch_residual(hns_grid* g, const float* div, const float* p, float dx, float* c_out, hns_stats* table, hns_stats* d_out, hipStream_t st, const char* who) {
	if (g->n_active) {
		if (!g->d_blk) {
			set_error("%s: the grid has no launch tables", who);
			return HNS_ERR_RUNTIME;
		}
		k_residual<<<(unsigned)g->n_active, 64, 0, st>>>(g->dev(), div, p, dx * dx, c_out, table);  // (dx * dx in f32: Kernel.cu:608, as the sweeps)
	}
	k_stats_fold<<<1, 1024, 0, st>>>(table, g->n_active, d_out);
	return launch_status(who);
}

int grid_table(hns_grid* g, size_t records, hns_stats** table) {
	std::lock_guard<std::mutex> lock(g->build_mutex);
	HNS_TRY(g->d_diag.reserve(sizeof(hns_stats) * std::max<size_t>(records, 1), g->device));  // (a put waits for the device: nothing still reads the old table)
	*table = g->d_diag.as<hns_stats>();
	return HNS_OK;
}

// a sim's diagnostics memory: device records | partial table for `rows` table rows; pinned host records
int sim_diag(hns_sim* s, size_t rows, hns_stats** d_rec, hns_stats** table) {
	const uint64_t n_leaves = s->n / 512u;
	HNS_TRY(s->d_diag.reserve(kRecordBytes + sizeof(hns_stats) * std::max<uint64_t>(rows * n_leaves, 1), s->device));
	if (!s->h_diag) HNS_HIP(hipHostMalloc((void**)&s->h_diag, kRecordBytes, hipHostMallocDefault));
	*d_rec = s->d_diag.as<hns_stats>();
	*table = (hns_stats*)(s->d_diag.as<char>() + kRecordBytes);
	return HNS_OK;
}

int fetch(hns_sim* s, const hns_stats* d_rec, int first, int n, hipStream_t st) {  // records [first, first + n) into s->h_diag, waited for
	HNS_HIP(hipMemcpyAsync(s->h_diag + first, d_rec + first, sizeof(hns_stats) * (size_t)n, hipMemcpyDeviceToHost, st));
	HNS_HIP(hipStreamSynchronize(st));
	return HNS_OK;
}

}  // namespace
}  // namespace hns

using namespace hns;

void hns_sim_free_diagnostics(hns_sim* s) {
	if (s->h_diag) (void)hipHostFree(s->h_diag);
	s->d_diag.release();
	delete s->control;
	s->h_diag = nullptr, s->control = nullptr;
}

// The control's part of a solve (include/hns.h: hns_solve_control). The driver, hns_sim_solve (hns_pressure.hip), cuts the loop into pieces of check_every iterations
// (V-cycles under hns_sim_set_solve_method) with hns_control_check behind each.
// before the solve's bracket opens: the diagnostics memory, an empty report
int hns_control_begin(hns_sim* s) {
	hns_stats *d_rec, *table;
	HNS_TRY(sim_diag(s, 1, &d_rec, &table));
	*s->control = hns_sim::Control{s->control->c, hns_solve_report{}, {}, false};
	return HNS_OK;
}
// p null: `initial`, the residual at p = 0 (the solve never warm-starts: p_a is zeroed for it), into record 0. Else, behind a piece that brought the solve to `done`
// iterations: the residual of p into record 1, the history and the report; *met: the stop rule holds. The one wait of a check is the fetch.
int hns_control_check(hns_sim* s, const float* p, int done, float voxel_size, void* stream, bool* met) {
	const char* who = "hns_sim_pressure_solve (controlled)";
	hns_sim::Control& ctl = *s->control;
	const hipStream_t st = (hipStream_t)stream;
	hns_stats *d_rec, *table;
	HNS_TRY(sim_diag(s, 1, &d_rec, &table));
	if (!p) {
		HNS_HIP(hipMemsetAsync(s->p_a, 0, sizeof(float) * 512 * (size_t)s->grid->topo.n_leaves, st));
		return launch_residual(s->grid, s->div, s->p_a, voxel_size, nullptr, table, d_rec, st, who);
	}
	HNS_TRY(launch_residual(s->grid, s->div, p, voxel_size, nullptr, table, d_rec + 1, st, who));
	HNS_TRY(fetch(s, d_rec, ctl.history.empty() ? 0 : 1, ctl.history.empty() ? 2 : 1, st));
	const hns_stats& r = s->h_diag[1];
	ctl.history.push_back(r);
	const bool monitor_only = ctl.c.rel_tol == 0.0f && ctl.c.abs_tol == 0.0f;
	*met = !monitor_only && r.nan_count == 0 && r.max_abs <= std::max(ctl.c.abs_tol, ctl.c.rel_tol * s->h_diag[0].max_abs);
	ctl.report = hns_solve_report{};
	ctl.report.converged = *met, ctl.report.iterations = done, ctl.report.checks = (int)ctl.history.size();
	ctl.report.initial = s->h_diag[0], ctl.report.final = r;
	ctl.ran = true;
	return HNS_OK;
}

extern "C" {

int hns_sim_set_solve_control(hns_sim* s, const hns_solve_control* c) {
	if (!s) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_set_solve_control: null sim");
	if (s->cached) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_set_solve_control: the sim belongs to a grid's cook cache");
	if (!c) {
		delete s->control;
		s->control = nullptr;
		return HNS_OK;
	}
	if (!(c->rel_tol >= 0.0f) || !(c->abs_tol >= 0.0f)) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_set_solve_control: a tolerance is negative or NaN");
	if (c->check_every < 1) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_set_solve_control: check_every must be at least 1");
	if (!s->control) s->control = new (std::nothrow) hns_sim::Control{};
	if (!s->control) return fail(HNS_ERR_RUNTIME, "hns_sim_set_solve_control: out of memory");
	s->control->c = *c;
	return HNS_OK;
}

int hns_sim_solve_report(hns_sim* s, hns_solve_report* report, hns_stats* history, int capacity, int* n_history) {
	if (!s || !report || capacity < 0 || (capacity > 0 && !history)) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_solve_report: bad arguments");
	if (!s->control || !s->control->ran) return fail(HNS_ERR_RUNTIME, "hns_sim_solve_report: no controlled solve has run on this sim");
	const hns_sim::Control& ctl = *s->control;
	*report = ctl.report;
	const size_t n = std::min<size_t>((size_t)capacity, ctl.history.size());
	if (n) memcpy(history, ctl.history.data(), sizeof(hns_stats) * n);
	if (n_history) *n_history = (int)ctl.history.size();
	return HNS_OK;
}

int hns_sim_stats(hns_sim* s, const hns_stats_field* names, int n_fields, int use_masks, hns_stats* out, void* stream) {
	const char* who = "hns_sim_stats";
	if (!s || !s->grid || !out) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_stats: null argument");
	if (s->cached) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_stats: the sim belongs to a grid's cook cache");
	if (n_fields < 1 || !names) {
		set_error("%s: bad field list (%d fields%s)", who, n_fields, names ? "" : ", NULL list");
		return HNS_ERR_INVALID_ARGUMENT;
	}
	std::vector<StatRow> rows;
	int n_records = 0;
	bool velocity = false;
	for (int i = 0; i < n_fields; ++i) {
		const hns_stats_field& q = names[i];
		const char* nm = q.name ? q.name : "(null)";
		const int f = q.name ? s->find(q.name) : -1;
		if (q.ncomp != 1 && q.ncomp != 3) {
			set_error("%s: field %d ('%s'): ncomp %d (1 or 3)", who, i, nm, q.ncomp);
			return HNS_ERR_INVALID_ARGUMENT;
		}
		if (q.ncomp == 1 && f < 0) {
			set_error("%s: field %d: the sim has no float field '%s'", who, i, nm);
			return HNS_ERR_INVALID_ARGUMENT;
		}
		if (q.ncomp == 3 && f >= 0) {
			set_error("%s: field %d: ncomp 3 under the float field name '%s'", who, i, nm);
			return HNS_ERR_INVALID_ARGUMENT;
		}
		bool twice = q.ncomp == 3 && velocity;
		for (int j = 0; j < i && q.ncomp == 1; ++j) twice = twice || (names[j].ncomp == 1 && names[j].name && !strcmp(names[j].name, q.name));
		if (twice) {
			set_error("%s: field %d: a second entry for %s%s", who, i, q.ncomp == 3 ? "the velocity" : "", q.ncomp == 3 ? "" : nm);
			return HNS_ERR_INVALID_ARGUMENT;
		}
		velocity = velocity || q.ncomp == 3;
		rows.push_back(StatRow{q.ncomp == 3 ? s->vel : s->cur[(size_t)f], q.ncomp, n_records});
		n_records += q.ncomp;
	}
	if ((size_t)n_records > kRecordsMax) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_stats: too many fields in one call");
	DeviceScope on(s->device);
	const hipStream_t st = (hipStream_t)stream;
	hns_stats *d_rec, *table;
	HNS_TRY(sim_diag(s, (size_t)n_records, &d_rec, &table));
	HNS_TRY(launch_stats(rows, n_records, use_masks ? s->d_masks.as<unsigned char>() : nullptr, s->n / 512u, table, d_rec, st, who));
	HNS_TRY(fetch(s, d_rec, 0, n_records, st));
	memcpy(out, s->h_diag, sizeof(hns_stats) * (size_t)n_records);
	return HNS_OK;
}

int hns_sim_residual(hns_sim* s, float voxel_size, hns_stats* out, void* stream) {
	const char* who = "hns_sim_residual";
	if (!s || !s->grid || !out) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_residual: null argument");
	if (s->cached) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_residual: the sim belongs to a grid's cook cache");
	if (!(voxel_size > 0.0f)) return fail(HNS_ERR_INVALID_ARGUMENT, "voxelSize must be positive.");
	if (!s->solved) return fail(HNS_ERR_RUNTIME, "hns_sim_residual: no pressure solve has run on this sim's grid");
	DeviceScope on(s->device);
	const hipStream_t st = (hipStream_t)stream;
	hns_stats *d_rec, *table;
	HNS_TRY(sim_diag(s, 1, &d_rec, &table));
	HNS_TRY(launch_residual(s->grid, s->div, s->p_result, voxel_size, nullptr, table, d_rec, st, who));
	HNS_TRY(fetch(s, d_rec, 0, 1, st));
	*out = s->h_diag[0];
	return HNS_OK;
}

int hns_dev_field_stats(hns_grid* g, const float* values, int ncomp, const unsigned char* masks, hns_stats* d_out, void* stream) {
	if (int rc = check_grid(g, "hns_dev_field_stats")) return rc;
	NULLCHK(!values || !d_out, "hns_dev_field_stats");
	if (ncomp != 1 && ncomp != 3) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_dev_field_stats: ncomp must be 1 or 3");
	const uint64_t n_leaves = (uint64_t)g->topo.n_leaves;
	hns_stats* table;
	HNS_TRY(grid_table(g, (size_t)ncomp * n_leaves, &table));
	return launch_stats({StatRow{values, ncomp, 0}}, ncomp, masks, n_leaves, table, d_out, (hipStream_t)stream, "hns_dev_field_stats");
}

int hns_dev_residual(hns_grid* g, const float* div, const float* p, float dx, float* c_out, hns_stats* d_out, void* stream) {
	if (int rc = check_grid(g, "hns_dev_residual")) return rc;
	NULLCHK(!div || !p || !d_out, "hns_dev_residual");
	hns_stats* table;
	HNS_TRY(grid_table(g, (size_t)g->topo.n_leaves, &table));
	return launch_residual(g, div, p, dx, c_out, table, d_out, (hipStream_t)stream, "hns_dev_residual");
}

}  // extern "C"
