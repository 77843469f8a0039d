// hns_internal.hpp -- shared declarations of libhns.so (not part of the public ABI; see include/hns.h).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <mutex>
#include <string>
#include <vector>

#include "hns.h"

// a function the host and the device both compile (hns_originhash.hpp, hns_dilate.hpp)
#define HNS_HD __host__ __device__ __forceinline__

namespace hns {

// ---- error plumbing -------------------------------------------------------------------------------------------
void set_error(const char* fmt, ...);
inline int fail(int code, const char* msg) {
	set_error("%s", msg);
	return code;
}
// The test behind every "must not alias" of include/hns.h, stated once: the byte ranges [a, a + a_bytes) and [b, b + b_bytes) share a byte, or the pointers are equal (so
// that two empty ranges at one address still count). A partial overlap -- an output that starts one leaf into its input -- is refused like identical pointers.
inline bool ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
	const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
	return x == y || (x < y + b_bytes && y < x + a_bytes);
}

#define HNS_TRY(call)                    \
	do {                                 \
		int rc__ = (call);               \
		if (rc__ != HNS_OK) return rc__; \
	} while (0)

#define HNS_HIP(call)                                                                                   \
	do {                                                                                                \
		hipError_t e__ = (call);                                                                        \
		if (e__ != hipSuccess) {                                                                        \
			hns::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__, __LINE__); \
			return HNS_ERR_HIP;                                                                         \
		}                                                                                               \
	} while (0)

// the four float fields combustion reads and writes, in the order the kernels take them (reference HNanoSolver.cu:193-201)
constexpr const char* kCombustionFields[4] = {"fuel", "waste", "temperature", "flame"};

// hipEvents that bracket stretches of a stream, in groups of `per`: 2 for a pressure loop (start, stop), 6 for the boundaries of a substep's five stages. Whoever is
// timed records into current() -- null when timing is off or every group is used -- and calls advance() behind the group's last record; the group may be opened in
// one function and closed in another (the partitioned pressure loop: its first block and its gradient phase).
struct EventGroups {
	size_t per;
	std::vector<hipEvent_t> ev;
	size_t used = 0;  // groups
	bool on = false;
	explicit EventGroups(size_t per_) : per(per_) {}
	int reset(int groups) {  // room for `groups` groups (events are kept, never given back), none of them used; 0 = timing off
		while (ev.size() < (size_t)groups * per) {
			hipEvent_t e;
			HNS_HIP(hipEventCreate(&e));
			ev.push_back(e);
		}
		on = groups > 0;
		used = 0;
		return HNS_OK;
	}
	hipEvent_t* current() { return on && (used + 1) * per <= ev.size() ? &ev[used * per] : nullptr; }
	void advance() { ++used; }
	int elapsed(double* ms) {  // ms[per - 1]: the time from each event of a group to the next, summed over the used groups (waits for their last events)
		std::fill(ms, ms + per - 1, 0.0);
		for (size_t g = 0; g < used; ++g) {
			const hipEvent_t* e = &ev[g * per];
			HNS_HIP(hipEventSynchronize(e[per - 1]));
			for (size_t k = 0; k + 1 < per; ++k) {
				float t = 0.0f;
				HNS_HIP(hipEventElapsedTime(&t, e[k], e[k + 1]));
				ms[k] += t;
			}
		}
		return HNS_OK;
	}
	void destroy() {
		for (hipEvent_t e : ev) (void)hipEventDestroy(e);
		ev.clear();
	}
};

// Is `stream` being captured into a graph? A query that fails counts as yes, and its error is cleared.
inline bool stream_is_capturing(void* stream) {
	hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
	if (hipStreamIsCapturing((hipStream_t)stream, &cs) != hipSuccess) {
		(void)hipGetLastError();
		return true;
	}
	return cs != hipStreamCaptureStatusNone;
}

// ---- the pressure loop's launch schedule ----------------------------------------------------------------------------
// What one solve of `iterations` (red, black) iterations launches, as a value: hns_rbgs_iterate walks it, hns_grid_rbgs_plan describes it, the partitioned substep
// queries it. lb = 0 is the colour form (copy, then one k_rbgs_color launch per colour, in place): every iteration is one ping-pong step and two kernel launches.
// lb = 1 / 2 is the temporally blocked form on blocks of lb^3 leaves (hns_sorblock.hip): every step is one launch -- n4 of four iterations while k_max = 4 and four are
// left, then n2 of two, then n1 = 1 for an odd iteration left over (the two-iteration kernel with two colour sweeps instead of four), in that order.
struct SorSchedule {
	int lb = 0, k_max = 0;
	int n4 = 0, n2 = 0, n1 = 0;
	int iterations() const { return 4 * n4 + 2 * n2 + n1; }
	int steps() const { return n4 + n2 + n1; }                          // src -> dst ping-pong steps: their parity is result_in_b
	int step(int i) const { return i < n4 ? 4 : (i < n4 + n2 ? 2 : 1); }  // iterations of step i
	int launches() const { return lb ? steps() : 2 * steps(); }         // kernel launches
	int iterations_per_launch() const { return lb && iterations() >= 2 ? k_max : 1; }
	bool one_blocked_launch() const { return lb && steps() == 1; }
};
inline SorSchedule sor_schedule(int lb, int k_max, int iterations) {
	SorSchedule s;
	if (iterations < 1) return s;
	if (!lb) {
		s.n1 = iterations;
		return s;
	}
	s.lb = lb, s.k_max = k_max;
	s.n4 = k_max >= 4 ? iterations / 4 : 0;
	s.n2 = (iterations - 4 * s.n4) / 2;
	s.n1 = iterations & 1;
	return s;
}

// makes `device` current for the scope (allocations, frees and synchronisation of pooled memory belong to ITS device,
// whatever the calling thread has current)
struct DeviceScope {
	int prev = -1;
	bool switched = false;
	explicit DeviceScope(int device) {
		if (device >= 0 && hipGetDevice(&prev) == hipSuccess && prev != device) switched = hipSetDevice(device) == hipSuccess;
	}
	~DeviceScope() {
		if (switched) (void)hipSetDevice(prev);
	}
};

// ---- options (hns_set_option) -------------------------------------------------------------------------------------
// Alternative kernel forms and data-movement strategies kept for A/B measurement and as cross-checks of the default one.
// Every entry point reads the current value when it is called, so a test or benchmark can switch forms between calls.
enum { kRbgsAuto = 0, kRbgsColor = 1 };
enum { kScheduleAuto = 0, kScheduleLinear = 1 };
enum { kLookaheadAuto = 0, kLookaheadOff = 1, kLookaheadOn = 2 };
struct Options {
	std::atomic<int> rbgs{kRbgsAuto};          // "rbgs": auto | color (the reference's two launches per iteration: the independent cross-check)
	std::atomic<int> advect_generic{0};        // "advect": auto | generic (64-bit addressed kernels)
	std::atomic<int> collide_generic{0};       // "collide": auto | generic -- with a collision SDF advect_vector / advect_scalars run the 64-bit addressed kernels and hns_sim_substep does not fuse (the dispatch before the 32-bit collision forms: cross-check, A/B)
	std::atomic<int> stencil_block{0};         // "stencil": auto | block (512-thread divergence / gradient)
	std::atomic<int> schedule{kScheduleAuto};  // "schedule": auto | linear (read when launch tables are built)
	std::atomic<int> cook_cache{1};            // "cook_cache": operator calls keep their device buffers with the grid
	std::atomic<int> cook_pipeline{1};         // "cook_pipeline": hns_compute_sim overlaps transfers with the substep
	std::atomic<int> divergence_form{0};       // "divergence": 0 auto (by size) | 1 row | 2 coalesced (own leaf fetched in memory order, handed to the row owners through LDS) | 3 zpair (coalesced, two z-adjacent leaves per workgroup)
	std::atomic<int> fuse_pointwise{1};        // "fuse": hns_sim_substep / hns_compute_sim without a collision field run divergence + combustion + buoyancy as one launch and advect the four combustion fields out of one 16-byte-per-voxel array
	std::atomic<int> lookahead{kLookaheadAuto};  // "lookahead": auto | 0 | 1 -- a substep's advect_scalars also computes the NEXT substep's advect_vector (hns_api.hip: Substep); auto: only when the previous substep on the sim had the same dt and voxel size
	std::atomic<int> sor_block_lb{0};          // "sor_block_lb": block edge of the temporally blocked SOR in leaves, 0 = by size | 1 | 2 (the tests' way to every kernel on every grid)
	std::atomic<int> dist_wire_us{0};          // "dist_wire_us": loopback transport only, emulated time on the wire per exchange
	std::atomic<int> dist_mirror{1};           // "dist_mirror": 1 | 0 | guarded -- over the ipc / local transports a rank of 16^3 blocks with sweeps_per_exchange = 2 runs the CHAINED substep (every kernel delivers its own halo); 0 = the exchanged substep (what RCCL ranks run)
	std::atomic<int> arena_fill{-1};           // "arena_fill": off | 0 .. 255 -- a TEST switch: every block the pool (hns_arena.hip) hands out is filled with that byte first, so that a result which depends on what pooled memory held shows up; a device-wide wait per block, never on while a stream captures
	std::atomic<int> dist_unsplit{1};          // "dist_unsplit": small ranks of the exchanged substep run their short phases as ONE launch over the owned leaves with the exchange behind it on the compute stream; 0 = boundary / interior split on two streams at every size
};
Options& options();

// ---- host topology ----------------------------------------------------------------------------------------------
// Replaces the NanoGrid<ValueOnIndex> tree walk (reference Stencils.hpp:51-71 -> NanoVDB.h:5549) with flat tables:
//   origins[l]      leaf origin (8-aligned), l = position of the leaf in the caller's coordinate array
//   nbr27[l][27]    leaf index of the 27 surrounding leaves ((dx+1)*9+(dy+1)*3+(dz+1)), -1 = absent
//   hash            open-addressing map origin -> leaf for taps further than one leaf away
struct Topology {
	std::vector<int32_t> origins;  // n_leaves * 4 (x, y, z, pad) -- int4 on the device
	std::vector<int32_t> nbr27;    // n_leaves * 27
	std::vector<int32_t> hash;     // table_size entries, -1 = empty
	uint32_t hash_mask = 0;
	int64_t n_leaves = 0;
	bool have_tables = false;  // nbr27 / hash present on the host (device-built grids fetch them on first host query)

	// Both return HNS_OK or HNS_ERR_TOPOLOGY (message set).
	int prepare(const int32_t* leaf_origins_xyz, int64_t n_leaves);  // origins + hash size; checks alignment and the leaf limit
	int build_tables();                                             // host build of hash + nbr27; detects duplicate origins
	int64_t find_leaf(int32_t ox, int32_t oy, int32_t oz) const;
	uint64_t offset(int32_t i, int32_t j, int32_t k) const;  // 1-based, 0 = outside
};

void sort_leaf_origins(int32_t* xyz, size_t n);  // OpenVDB leaf order, in place (hns_leafio.cpp)

// Device view handed to every kernel by value.
struct GridDev {
	const int4* origins;
	const int* nbr27;
	const int* hash;
	const int* sched;  // block -> leaf order (XCD-chunked), n_active entries
	int sched_seg;     // >= 0: the order is the closed form sched_leaf(pos, n_active, sched_seg, sched_pre) (hns_device.hpp) -- one chunk per XCD (0) or
	int sched_pre;     // plain order (1): a few scalar instructions instead of a dependent load at the head of every workgroup; -1: look `sched` up
	const int* blk;    // per block, in launch order: {leaf, nbr27[27]} (28 ints)
	uint32_t hash_mask;
	int n_leaves;
	int n_active;
	int first;  // first active leaf: kernels update leaves [first, first + n_active)
	int oob;  // element read by advect_scalars for out-of-domain taps (0 on an unpartitioned grid)
	int rev;  // 1: walk the launch order backwards (rows of eight workgroups reversed: a kernel starts on the cached tail of what its predecessor wrote)
	int* far_flag;  // null, or (the local grid of a multi-GPU rank) a word the advection kernels raise when a tap leaves the 27-leaf neighbourhood of its
	                // leaf: the rank holds one layer of ghost leaves, further away it cannot tell "outside the domain" from "on another rank"
};

// workgroup -> position in the launch-order tables, honouring GridDev::rev
__device__ __forceinline__ unsigned launch_pos(const GridDev& g, unsigned b) {
	if (!g.rev) return b;
	const unsigned rows = (unsigned)g.n_active >> 3;
	return (b >> 3) < rows ? (((rows - 1u - (b >> 3)) << 3) | (b & 7u)) : b;
}

// the leaf workgroup b works on (kernels with one workgroup per leaf). One chunk per XCD (sched_seg 0: every grid up to 40k leaves) is
// closed form -- block b = 8 i + x is leaf x * (n / 8) + min(x, n % 8) + i of the range -- and costs a few scalar instructions; reading
// it from the table put a dependent load in front of everything a workgroup does (the advection kernels are bound by the length of
// that chain: profiles/r04_advect_notes.txt).
__device__ __forceinline__ int launch_leaf(const GridDev& g, unsigned b) {
	const int pos = (int)launch_pos(g, b);
	if (g.sched_seg == 0 && g.sched_pre == 0) {
		const int base = g.n_active >> 3, rem = g.n_active & 7, x = pos & 7, i = pos >> 3;
		return g.first + x * base + (x < rem ? x : rem) + i;
	}
	return g.sched ? g.sched[pos] : g.first + pos;
}

}  // namespace hns

#include "hns_pool.hpp"  // hns::Pooled, hns::carve, hns::Scratch: every block of pooled device memory below has one owner

struct hns_sim;

struct hns_grid {
	hns::Topology topo;
	float voxel_size = 1.0f;
	uint64_t n_active = 0;      // kernels update leaves [first_active, first_active + n_active) and only read the others
	uint64_t first_active = 0;
	uint64_t outside_element = 0;
	int* far_flag = nullptr;    // see GridDev::far_flag (set by hns_dist; not owned)
	bool on_device = false;
	int device = -1;
	// device copies
	void* d_origins = nullptr;
	void* d_nbr27 = nullptr;
	void* d_hash = nullptr;
	void* d_sched = nullptr;
	void* d_blk = nullptr;
	int sched_seg = -1, sched_pre = 0;  // parameters of the current launch order (hns_grid_upload_schedule), for GridDev
	uint64_t chain_boundary = 0;  // leaves at the head of the active range that are a multi-GPU rank's BOUNDARY leaves (hns_dist: the range its chained sweeps run over); correctness, not speed
	uint64_t sched_prefix = 0;    // leaves at the head of the active range that the launch order deals out to all XCDs first (hns_dist: boundary leaves)
	void* d_sched_mem = nullptr;  // storage of d_sched (d_sched itself is null under the linear schedule)
	void* d_scratch = nullptr;    // scratch of the block-record build (hns_grid_build_blocks)
	hns::Pooled d_arena;          // the one device allocation all of the above are slices of (hns::grid_slices below)
	// temporally blocked SOR kernel (hns_sorblock.hip): records of the 16^3-voxel blocks in launch order (64 leaves under each tile),
	// built on first use into an arena allocation of their own
	hns::Pooled d_sb_tab;
	uint64_t n_sb = 0;
	bool sb_built = false;
	int sb_seg = 0;
	uint64_t sb_first = 0, sb_count = 0;                  // the launch range the records were built for
	std::vector<hns::Pooled> sb_retired;                  // superseded tables: back to the pool when the grid goes, or -- beyond four of them -- behind a device synchronise
	// hns_dev_field_stats / hns_dev_residual (hns_diagnostics.hip): the table of per-leaf partial records, an arena allocation of its own made on first use
	hns::Pooled d_diag;
	// hns_dev_splat_points (hns_splat.hip): the fixed-point accumulator -- splat_channels int64 channels per voxel, then one touched word per leaf --, an arena allocation of
	// its own made on first use and all zero between calls; splat_dirty: it must be cleared before its next use (fresh from the pool, or a call failed half way)
	hns::Pooled d_splat;
	int splat_channels = 0;
	bool splat_dirty = false;
	hns_splat_spec splat_spec = {0, 0, 0.0f, nullptr, 0.0f};  // hns_grid_set_splat_spec: what hns_dev_splat_points on this grid reads (the default: today's cell, a sum)
	std::mutex build_mutex;              // guards the tables built on first use (block records): cooks from several host threads may share a grid
	std::mutex host_mutex;               // guards the lazy host copy of the device-built tables and sim_cache
	std::vector<hns_sim*> sim_cache;     // device-resident state kept between operator calls (hns_api.hip: make_sim)
	hns::GridDev dev() const;
};

// Device-resident simulation state (include/hns.h: hns_sim_*). Lives in hns_api.hip; hns_regrid.hip moves one onto a new grid.
struct hns_sim {
	hns_grid* grid = nullptr;
	uint64_t n = 0;  // voxels
	std::vector<std::string> names;
	std::vector<float*> cur;  // current value of each float field (the reference's d_inputs)
	std::vector<float*> nxt;  // scratch / next value        (the reference's d_outputs)
	float* vel = nullptr;  // d_velocity      (Vec3f AoS, 3n floats: the host/reference layout, so H2D/D2H are plain copies)
	float* adv = nullptr;  // d_advectedVel
	float* tmp = nullptr;  // out-of-place vorticity target; the buoyed u* of the fused divergence / combustion / buoyancy launch
	float* q4 = nullptr;   // {fuel, waste, temperature, flame} as one 16-byte element per voxel between that launch and advect_scalars (sims that hold those four fields)
	float* div = nullptr;
	float* p_a = nullptr;
	float* p_b = nullptr;
	float* p_result = nullptr;  // whichever of p_a/p_b holds the last solve
	// optional hipEvent bracketing of the pressure hot loop (hns_sim_timing), on the stream the kernels run on
	hns::EventGroups solve_ev{2};  // start/stop pairs
	long long timed_launches = 0;
	int solve_begin(void* stream) {  // the bracket round one solve (hns_pressure.hip: hns_sim_solve)
		if (hipEvent_t* timed = solve_ev.current()) HNS_HIP(hipEventRecord(timed[0], (hipStream_t)stream));
		return HNS_OK;
	}
	int solve_end(void* stream, int iterations) {
		if (hipEvent_t* timed = solve_ev.current()) {
			HNS_HIP(hipEventRecord(timed[1], (hipStream_t)stream));
			solve_ev.advance();
			timed_launches += iterations;
		}
		return HNS_OK;
	}
	hns::EventGroups stage_ev{6};  // hns_sim_stage_timing: also bracket the five stages of hns_sim_substep / hns_sim_core_substep (six boundaries per substep)
	hipStream_t xfer = nullptr;  // transfer stream + hand-off events of the pipelined operator path (hns_api.hip: Cook)
	hipEvent_t xev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
	bool cached = false, in_use = false;  // owned by the grid's cook cache / currently lent to an operator call
	// Device-resident feedback across cooks (hns_compute_sim_resident): a signature of what the last hns_compute_sim on this state handed
	// back for the velocity and for float field i -- those bytes are still in `vel` / cur[i]. 0 = nothing to vouch for (any upload clears it).
	struct Handed { uint64_t sig = 0, dig = 0; };  // (sig: sample signature; dig: full digest, 0 = not taken)
	Handed handed_vel;
	std::vector<Handed> handed_cur;  // one per float field (sized where `names` is fixed: sim_create)
	static constexpr int kVelocity = -1, kEverything = -2;
	// Look-ahead (hns_api.hip: Substep): `adv` as a memo of advect_vector(vel, dt), filled by a substep's advect_scalars launch and consumed by the next substep in place of
	// its advect_vector launch. Valid for exactly one grid, dt and voxel size (compared by their bits), and only until something other than the substep writes vel or adv.
	struct Ahead {
		bool valid = false;
		const hns_grid* grid = nullptr;
		uint64_t first = 0, n_active = 0;  // the grid's launch range
		uint32_t dt_bits = 0, vs_bits = 0;
	};
	Ahead ahead;
	bool ahead_off = false;     // for good: the velocity pointer was handed out, the sim is lent to operator calls, or a substep was captured into a graph
	bool have_last = false;     // option lookahead = auto: dt and voxel size of the previous substep call
	uint32_t last_dt_bits = 0, last_vs_bits = 0;
	int last_iterations = 0;    // (hns_sim_substep_plan: the pressure stage of the previous call)
	long long ahead_produced = 0, ahead_consumed = 0;  // hns_sim_lookahead_counts
	void drop_ahead() { ahead.valid = false; }
	void forget(int k = kEverything) {  // float field k, the velocity or everything: the buffer no longer holds what the caller was handed
		drop_ahead();
		if (k == kEverything || k == kVelocity) handed_vel = Handed{};
		for (size_t i = 0; i < handed_cur.size(); ++i)
			if (k == kEverything || k == (int)i) handed_cur[i] = Handed{};
	}
	void wrote_field(int k) { handed_cur[(size_t)k] = Handed{}; }  // float field k was written in place by a call that left the velocity alone: its signature goes, the look-ahead memo (a function of the velocity and collision_sdf) stays
	unsigned long long* d_dig = nullptr;  // 16 accumulators of the digest kernels (hns_digest.hpp): a slice of the arena
	unsigned long long* h_dig = nullptr;  // pinned host copy of them (read asynchronously on the cook's own stream)
	hns::Pooled arena;  // every field above is a slice of this one allocation (hns::sim_slices below)
	// active voxel masks of the leaves (hns_sim_set_active_masks / hns_sim_regrid): leaf_count x 64 bytes, byte x*8+y, bit z; null = every voxel active.
	// An allocation of their own from the arena pool, made on first use: nothing else reads them.
	hns::Pooled d_masks;
	hipEvent_t rev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // phase boundaries of the last hns_sim_regrid (hns_sim_regrid_times)
	bool regrid_timed = false;
	// hns_sim_deactivate's device table (its counts, then one row per listed field), made on first use from the arena pool, written by a kernel
	hns::Pooled d_act;
	// Diagnostics (hns_diagnostics.hip). d_diag: the records a call leaves, then the table of per-leaf partial records -- an arena allocation of its own, made on first
	// use; h_diag: pinned host memory the records are read into. solved: p_result holds a solve on the current grid (hns_sim_residual).
	hns::Pooled d_diag;
	hns_stats* h_diag = nullptr;
	bool solved = false;
	// hns_sim_set_solve_control: null = off, and then hns_sim_solve (hns_pressure.hip) is the uncontrolled loop after one pointer test
	struct Control {
		hns_solve_control c;
		hns_solve_report report;
		std::vector<hns_stats> history;
		bool ran = false;
	};
	Control* control = nullptr;
	// hns_sim_set_solve_method: null = SOR, and then hns_sim_solve (hns_pressure.hip) is the plain loop after one more pointer test; else the V-cycle's parameters and its
	// hierarchy of coarse grids, masks, tables and buffers (hns_multigrid.hip)
	struct Multigrid;
	Multigrid* mg = nullptr;
	hns_splat_spec splat_spec = {0, 0, 0.0f, nullptr, 0.0f};  // hns_sim_set_splat_spec: what hns_sim_splat_points reads; the sim's own, so a regrid's new grid changes nothing
	int device = -1;
	int find(const char* name) const {
		for (size_t i = 0; i < names.size(); ++i)
			if (names[i] == name) return (int)i;
		return -1;
	}
};

// A field list of hns_sim_deactivate (s: its sim) or hns_deactivate_leaf_masks (s null), checked (hns_leafio.cpp): HNS_OK, or HNS_ERR_INVALID_ARGUMENT
// with the message under `who`. field_of (or null) receives each entry's float field index in s, -1 for the velocity.
namespace hns { int check_activity_fields(const hns_sim* s, const hns_activity_field* fields, int n_fields, const char* who, std::vector<int>* field_of); }

// hns_pressure.hip: the one driver of a sim's pressure solve -- SOR sweeps or V-cycles, whole or in a control's pieces -- and the checks in front of its first launch
int hns_sim_solve(hns_sim* s, int iterations, float voxel_size, float omega, void* stream);
int hns_solve_preflight(hns_sim* s, void* stream, const char* who);
// hns_diagnostics.hip: what a control adds to hns_sim_solve -- before its bracket opens; the residual at p = 0 (p null) and behind each piece
int hns_control_begin(hns_sim* s);
int hns_control_check(hns_sim* s, const float* p, int done, float voxel_size, void* stream, bool* met);
void hns_sim_free_diagnostics(hns_sim* s);  // (hns_sim_destroy)

// hns_multigrid.hip: the V-cycle solve of a sim with a method set (include/hns.h: hns_solve_method)
int hns_mg_ready(hns_sim* s, void* stream, const char* who);  // the hierarchy of the sim's current grid is there afterwards: built here when a regrid dropped it (refused on a capturing stream), before anything is launched
int hns_mg_cycles(hns_sim* s, float** cur, float** other, float dx, int cycles, bool first, void* stream);  // `cycles` V-cycles on *cur (first: from p = 0, whatever *cur holds); *cur / *other are swapped as the fine sweeps ping-pong
std::string hns_mg_plan(hns_sim* s);  // the pressure stage's word of hns_sim_substep_plan
void hns_sim_drop_hierarchy(hns_sim* s);   // the sim has moved onto another grid (hns_regrid.hip): the next solve builds the hierarchy again
void hns_sim_free_multigrid(hns_sim* s);   // (hns_sim_destroy)
void hns_grid_free_splat(hns_grid* g);       // hns_splat.hip: the grid's accumulator back to the pool (hns_grid_release_cache, and through it hns_grid_destroy)

// The two layouts that lie under every kernel, each stated once as a list for hns::carve (plain host arithmetic: tests/cpp/pool_owner.cpp pins their offsets).
namespace hns {
// A sim's buffers for n voxels over one arena, in units of one 256-byte aligned float field: vel, adv, tmp | div, p_a, p_b | cur, nxt per field | q4 (sims that hold the four
// combustion fields) | the 16 digest accumulators of hns_compute_sim_resident. s.cur / s.nxt hold one entry per name.
inline size_t sim_unit(uint64_t n) { return pad256(sizeof(float) * (size_t)(n ? n : 1)); }
inline bool sim_combust(const hns_sim& s) { return std::all_of(kCombustionFields, kCombustionFields + 4, [&s](const char* n) { return s.find(n) >= 0; }); }
inline void sim_slices(hns_sim& s, uint64_t n, const Slice& slice) {
	const size_t unit = sim_unit(n);
	slice(s.vel, 3, unit), slice(s.adv, 3, unit), slice(s.tmp, 3, unit);
	slice(s.div, 1, unit), slice(s.p_a, 1, unit), slice(s.p_b, 1, unit);
	for (size_t i = 0; i < s.names.size(); ++i) slice(s.cur[i], 1, unit), slice(s.nxt[i], 1, unit);
	if (sim_combust(s)) slice(s.q4, 4, unit);
	slice(s.d_dig, 16 * sizeof(unsigned long long));
}
// A grid's device tables over one allocation (hns_grid_upload), sized for n_active = n_leaves.
inline void grid_slices(hns_grid& g, const Slice& slice) {
	const size_t nl = (size_t)(g.topo.n_leaves > 0 ? g.topo.n_leaves : 1), hash_size = (size_t)g.topo.hash_mask + 1;
	slice(g.d_origins, 16 * nl);             // int4
	slice(g.d_nbr27, 4 * 27 * nl);
	slice(g.d_hash, 4 * (hash_size + 1));    // + the duplicate-origin status word
	slice(g.d_sched_mem, 4 * nl);
	slice(g.d_blk, 4 * 28 * nl);             // block records
	slice(g.d_scratch, 4 * (2 * nl + 2));    // of the block-record build on first use (hns_grid_build_blocks: flag[n] | leaders[n] | total[2])
}
}  // namespace hns
// bytes an arena needs for n voxels of s's fields, and the slices of `arena` for them (sets n, every buffer pointer, d_dig, p_result). Neither owns anything: a sim whose
// `arena` owner is empty may be laid over any memory (hns_regrid.hip: the new layout before the sim moves onto it).
inline void hns_sim_layout(hns_sim* s, void* arena, uint64_t n) {
	s->n = n;
	s->cur.assign(s->names.size(), nullptr), s->nxt.assign(s->names.size(), nullptr);
	s->q4 = nullptr;
	hns::carve(arena, [&](const hns::Slice& slice) { hns::sim_slices(*s, n, slice); });
	s->p_result = s->p_a;
}
inline size_t hns_sim_arena_need(const hns_sim* s, uint64_t n) {
	hns_sim shell;  // (the list wants somewhere to point: a layout-only object with the same names)
	shell.names = s->names;
	shell.cur.resize(s->names.size()), shell.nxt.resize(s->names.size());
	return hns::carve(nullptr, [&](const hns::Slice& slice) { hns::sim_slices(shell, n, slice); });
}

// implemented in hns_pressure.hip: hns_dev_rbgs_iterate with the option of starting from p = 0 without reading (or clearing) p_a
extern "C" __attribute__((visibility("hidden"))) int hns_rbgs_iterate(hns_grid* g, const float* div, float* p_a, float* p_b, float dx, float omega, int iterations, int* result_in_b,
                                void* stream, bool from_zero);

// the sweeps of a multi-GPU rank (hns_flags.hpp: PhaseMirror, PackMirror)
namespace hns { struct PhaseMirror; struct PackMirror; }
extern "C" __attribute__((visibility("hidden"))) int hns_rbgs_block_pack_launch(hns_grid* g, const float* div, const float* src, float* dst, float dx, float omega, bool src_is_zero,
                                                                                 const hns::PackMirror* m, void* stream, bool* done, int iterations);  // hns_sorblock.hip: the sweep (one or two iterations) that packs its own messages
extern "C" __attribute__((visibility("hidden"))) bool hns_rbgs_block_packable(hns_grid* g);  // hns_sorblock.hip: would hns_rbgs_block_pack_launch launch on this grid's range?
extern "C" __attribute__((visibility("hidden"))) int hns_rbgs_block_mirror_launch(hns_grid* g, const float* div, const float* src, float* dst, float dx, float omega, bool src_is_zero,
                                                                                   const hns::PhaseMirror* m, void* stream, int iterations);  // hns_sorblock.hip: one or two iterations per chained launch
extern "C" __attribute__((visibility("hidden"))) int hns_chain_divergence(hns_grid* g, const float* vel3, float* div, float inv_dx, const hns::PhaseMirror* m, void* stream);
extern "C" __attribute__((visibility("hidden"))) int hns_chain_subtract_pressure_gradient(hns_grid* g, const float* vel3, const float* p, float* out3, float inv_dx,
                                                                                          const hns::PhaseMirror* m, void* stream);

// the fused middle of hns_sim_substep (round 6): divergence + combustion_oxygen + temperature_buoyancy in one launch (hns_pressure.hip), leaving {fuel, waste, temperature,
// flame} as one 16-byte element per voxel, and the advect_scalars launch that gathers its taps from that array (hns_advect.hip)
extern "C" __attribute__((visibility("hidden"))) int hns_divergence_combust_buoyancy(hns_grid* g, const float* vel3, float* div, float inv_dx, const float* fuel, const float* waste,
                                                                                      const float* temperature, const float* flame, float* q4, float* vel3_out, float temp_gain,
                                                                                      float expansion, float dt, float ambient, float strength, void* stream);
extern "C" __attribute__((visibility("hidden"))) int hns_advect_scalars_q4(hns_grid* g, const float* vel3, const float* q4, float* const* q4_out, const float* const* in,
                                                                            float* const* out, int n, const float* sdf /* null: no collider */, float dt, float inv_dx, void* stream);
// which kernel a launcher picks for these arguments, by the code that picks it for the launch (hns_sim_substep_plan)
extern "C" __attribute__((visibility("hidden"))) const char* hns_advect_vector_kernel(const hns_grid* g, const float* sdf, int has_collision);
extern "C" __attribute__((visibility("hidden"))) const char* hns_advect_scalars_kernel(const hns_grid* g, const float* sdf, int has_collision);
extern "C" __attribute__((visibility("hidden"))) const char* hns_advect_scalars_q4_kernel(const float* sdf);
extern "C" __attribute__((visibility("hidden"))) const char* hns_advect_scalars_ahead_kernel(void);
extern "C" __attribute__((visibility("hidden"))) const char* hns_divergence_kernel(const hns_grid* g, bool fused);
extern "C" __attribute__((visibility("hidden"))) const char* hns_subtract_gradient_kernel(const hns_grid* g, const float* sdf, int has_collision);
extern "C" __attribute__((visibility("hidden"))) bool hns_advect_q4_ok(const hns_grid* g);
extern "C" __attribute__((visibility("hidden"))) bool hns_advect_ahead_ok(const hns_grid* g);  // hns_advect.hip: does hns_dev_advect_scalars_ahead apply to this grid?

// implemented in hns_pointwise.hip: combustion_oxygen split into its divergence update (needs fuel, waste) and the rest (hns_dist_*.hip: the boundary leaves' divergence first)
extern "C" __attribute__((visibility("hidden"))) int hns_combustion_div(const float* fuel, const float* waste, float* divergence, float expansion, uint64_t n,
                                                                        void* stream);
extern "C" __attribute__((visibility("hidden"))) int hns_combustion_fields(const float* fuel, const float* waste, const float* temperature, const float* flame,
                                                                           float* out_fuel, float* out_waste, float* out_temperature, float* out_flame,
                                                                           float temp_gain, uint64_t n, void* stream);

// implemented in hns_gridbuild.hip
int hns_grid_upload(hns_grid* g);           // device build of every table from topo.origins
void hns_grid_free_device(hns_grid* g);
int hns_grid_upload_schedule(hns_grid* g);  // launch-order tables for the current n_active
// implemented in hns_sorblock.hip: the temporally blocked SOR form (k iterations per launch)
int hns_grid_build_blocks(hns_grid* g);     // records of the 16^3-voxel blocks of the grid's launch range
void hns_grid_retire_blocks(hns_grid* g);   // superseded records back to the pool (grid destruction / rebuild only)
hns::SorSchedule hns_rbgs_schedule(hns_grid* g, int iterations);  // what hns_rbgs_iterate launches for `iterations` over the grid's launch range under the current options (may build the block records)
int hns_rbgs_block_launch(hns_grid* g, int lb, int k, bool src_is_zero, const float* div, const float* src, float* dst, float dx2, float omega, void* stream);
int hns_grid_host_tables(const hns_grid* g);  // make topo.nbr27 / topo.hash valid on the host
