// hns_multigrid.hip -- the second solve method of a device-resident sim (include/hns.h: hns_solve_method): geometric multigrid V-cycles on the leaf-sparse grid.
// Hand-written HIP for gfx950 / CDNA4, wave64. The fine level is swept by the temporally blocked SOR kernels as they are (hns_rbgs_iterate); this file holds
// the hierarchy (coarse grids, EXACT masks, child / parent tables, buffers) and the four kernels of the coarse levels:
//   k_mg_masks     a coarse voxel is an unknown iff one of its eight children is an unknown of the level below (integer ORs only)
//   k_mg_color     one colour of the red-black sweep in place, on unknowns only (the masked form of k_rbgs_color)
//   k_mg_restrict  residual + restriction in one launch: one workgroup per coarse leaf, one wave per child leaf, c never written to memory
//   k_mg_prolong   cell-centred trilinear prolongation + add: one wave per fine leaf, the parent's octant and its one-voxel rim (6^3) in LDS
// Why exact masks: with plain coarse leaf grids the coarse problem lives on a larger domain than the fine one and the cycle DIVERGES on ragged leaf sets
// (DESIGN_HISTORY.md: "Multigrid"). A voxel that is not an unknown holds +0 on every level, always: it is zeroed with its leaf and never updated.
#include <array>
#include <cstring>
#include <map>
#include <new>
#include <string>

#include "hns_device.hpp"

namespace hns {
namespace {

// One wave per coarse leaf, lane = mask byte x*8+y. child: the <= 8 child leaves of each coarse leaf (octant ox*4+oy*2+oz, -1 = absent); the children of coarse voxel
// (x, y, z) are the voxels (2(x&3)+dx, 2(y&3)+dy, 2(z&3)+dz) of the child leaf in octant (x>>2, y>>2, z>>2): four bytes of its mask, two bits of each.
__global__ __launch_bounds__(64) void k_mg_masks(const int* __restrict__ child, const unsigned char* __restrict__ fine_masks, unsigned char* __restrict__ coarse_masks) {
	const int leaf = blockIdx.x, l = threadIdx.x, x = l >> 3, y = l & 7;
	unsigned out = 0;
#pragma unroll
	for (int oz = 0; oz < 2; ++oz) {
		const int c = child[(size_t)leaf * 8 + (x >> 2) * 4 + (y >> 2) * 2 + oz];
		unsigned m = 0;
		if (c >= 0) {
#pragma unroll
			for (int d = 0; d < 4; ++d) {
				const int fx = 2 * (x & 3) + (d >> 1), fy = 2 * (y & 3) + (d & 1);
				m |= fine_masks ? (unsigned)fine_masks[(size_t)c * 64 + fx * 8 + fy] : 0xFFu;
			}
		}
#pragma unroll
		for (int zz = 0; zz < 4; ++zz) out |= ((m >> (2 * zz)) & 3u) ? 1u << (4 * oz + zz) : 0u;
	}
	coarse_masks[(size_t)leaf * 64 + l] = (unsigned char)out;
}

// One colour of one iteration in place on unknowns only: the masked instance of the sweep k_rbgs_color is the other instance of (hns_device.hpp: color_sweep)
__global__ __launch_bounds__(256) void k_mg_color(const GridDev g, const unsigned char* __restrict__ masks, const float* __restrict__ rhs, float* p, const float dx2,
                                                  const float omega, const int color) {
	__shared__ int s_nbr[27];
	color_sweep<true>(g, s_nbr, masks, rhs, p, dx2, omega, color);
}

// Residual + restriction (include/hns.h: "Restriction"). One workgroup per coarse leaf; wave w has the child leaf of octant w and stages its tile of p as k_residual
// stages its own (stage_tile_wave: the tile is the wave's, so a wave-level barrier is all it needs, and a wave without a child skips it). Lane (lx, ly, lz) of the wave
// forms coarse voxel (4ox + lx, 4oy + ly, 4oz + lz): the correction c of its eight children in registers -- +0 at a child that is not an unknown --, their sum in the
// stated association, times k. It also zeroes the coarse level's p for the solve from e = 0 that follows: every voxel of rhs_c and p_c is written in every cycle.
__global__ __launch_bounds__(512) void k_mg_restrict(const GridDev gf, const unsigned char* __restrict__ fmasks, const float* __restrict__ rhs_f, const float* __restrict__ p_f,
                                                     const float dx2, const float k, const int* __restrict__ child, float* __restrict__ rhs_c, float* __restrict__ p_c) {
	__shared__ __attribute__((aligned(16))) float Ps[8][kTile];
	const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), l = threadIdx.x & 63;
	const int leaf = __builtin_amdgcn_readfirstlane(child[(size_t)blockIdx.x * 8 + w]);
	const int lx = l >> 4, ly = (l >> 2) & 3, lz = l & 3;
	float sum = 0.0f;  // (an absent child leaf reads +0)
	if (leaf >= 0) {   // (wave-uniform)
		float* P = Ps[w];
		stage_tile_wave(P, p_f, gf.nbr27 + (size_t)leaf * 27 - 1, leaf, l);  // (rec[1 + j] = neighbour j, as in the launch-order records)
		wave_sync();
		float c[8];
#pragma unroll
		for (int d = 0; d < 8; ++d) {
			const int v = ((2 * lx + (d >> 2)) << 6) | ((2 * ly + ((d >> 1) & 1)) << 3) | (2 * lz + (d & 1));
			const float cv = gs_value(P[tile_nbr<0, 1>(v)], P[tile_nbr<0, -1>(v)], P[tile_nbr<1, 1>(v)], P[tile_nbr<1, -1>(v)], P[tile_nbr<2, 1>(v)], P[tile_nbr<2, -1>(v)],
			                          rhs_f[(size_t)leaf * 512 + v], dx2) - P[v];
			c[d] = is_unknown(fmasks, leaf, v) ? cv : 0.0f;
		}
		sum = ((c[0] + c[1]) + (c[2] + c[3])) + ((c[4] + c[5]) + (c[6] + c[7]));
	}
	const size_t at = (size_t)blockIdx.x * 512 + (((4 * (w >> 2) + lx) << 6) | ((4 * ((w >> 1) & 1) + ly) << 3) | (4 * (w & 1) + lz));
	rhs_c[at] = sum * k;
	p_c[at] = 0.0f;
}

// Prolongation + add (include/hns.h: "Prolongation"). One wave per fine leaf. parent: {coarse leaf, octant} of each fine leaf. The 6^3 coarse voxels around the
// leaf's octant -- local coordinates 4o - 1 .. 4o + 4 per axis, through the coarse grid's 27-neighbour table where they leave the parent, 0 where that leaf is absent;
// a masked coarse voxel holds 0 -- go into LDS; lane l then holds fine voxels 4(l + 64j) .. + 3, j = 0, 1: 16-byte loads and stores.
__global__ __launch_bounds__(64) void k_mg_prolong(const GridDev gc, const int2* __restrict__ parent, const float* __restrict__ e, const unsigned char* __restrict__ fmasks,
                                                   float* __restrict__ p_f) {
	__shared__ float E[216];
	const int leaf = blockIdx.x, l = threadIdx.x;
	const int2 po = parent[leaf];
	const int pl = __builtin_amdgcn_readfirstlane(po.x), oct = __builtin_amdgcn_readfirstlane(po.y);
	const int bx = 4 * (oct >> 2) - 1, by = 4 * ((oct >> 1) & 1) - 1, bz = 4 * (oct & 1) - 1;
	for (int i = l; i < 216; i += 64) {
		const int a = i / 36, b = (i / 6) % 6, c = i % 6;
		const int X = bx + a, Y = by + b, Z = bz + c;  // -1 .. 8
		const int sx = X < 0 ? 0 : (X > 7 ? 2 : 1), sy = Y < 0 ? 0 : (Y > 7 ? 2 : 1), sz = Z < 0 ? 0 : (Z > 7 ? 2 : 1);
		const int nl = gc.nbr27[(size_t)pl * 27 + sx * 9 + sy * 3 + sz];
		const float v = e[(size_t)(nl < 0 ? 0 : nl) * 512 + (((X & 7) << 6) | ((Y & 7) << 3) | (Z & 7))];
		E[i] = nl < 0 ? 0.0f : v;
	}
	wave_sync();
	const v4i rp = field_rsrc(p_f + (size_t)leaf * 512, 2048u);
#pragma unroll
	for (int j = 0; j < 2; ++j) {
		v4f32 pv = hns_buffer_load_v4f32(rp, 16 * (l + 64 * j), 0, 0);
#pragma unroll
		for (int q = 0; q < 4; ++q) {
			const int v = 4 * (l + 64 * j) + q;
			const int x = v >> 6, y = (v >> 3) & 7, z = v & 7;
			// box coordinates of the coarse voxel I = i >> 1 and of the second one, I + ((i & 1) ? 1 : -1)
			const int ax = (x >> 1) + 1, ay = (y >> 1) + 1, az = (z >> 1) + 1;
			const int ox = ax + ((x & 1) ? 1 : -1), oy = ay + ((y & 1) ? 1 : -1), oz = az + ((z & 1) ? 1 : -1);
			// z, then y, then x (tri_nest's order): each 0.75f * a + 0.25f * b is two multiplies, then an add
			const float z00 = 0.75f * E[ax * 36 + ay * 6 + az] + 0.25f * E[ax * 36 + ay * 6 + oz];
			const float z01 = 0.75f * E[ax * 36 + oy * 6 + az] + 0.25f * E[ax * 36 + oy * 6 + oz];
			const float z10 = 0.75f * E[ox * 36 + ay * 6 + az] + 0.25f * E[ox * 36 + ay * 6 + oz];
			const float z11 = 0.75f * E[ox * 36 + oy * 6 + az] + 0.25f * E[ox * 36 + oy * 6 + oz];
			const float y0 = 0.75f * z00 + 0.25f * z01, y1 = 0.75f * z10 + 0.25f * z11;
			const float val = 0.75f * y0 + 0.25f * y1;
			pv[q] = is_unknown(fmasks, leaf, v) ? pv[q] + val : pv[q];
		}
		hns_buffer_store_v4f32(pv, rp, 16 * (l + 64 * j), 0, 0);
	}
}

}  // namespace
}  // namespace hns

using namespace hns;

// ---------------------------------------------------------------------------------------------------------------
// the hierarchy
// ---------------------------------------------------------------------------------------------------------------

namespace {
struct Level {  // level >= 1
	hns_grid* grid = nullptr;
	uint64_t n = 0;                 // leaves
	unsigned char* masks = nullptr;  // n x 64 bytes
	int* child = nullptr;            // n x 8: the leaves of the level below, -1 = absent
	int2* parent = nullptr;          // per leaf of the level BELOW: {leaf of this level, octant}
	float *p = nullptr, *rhs = nullptr;
};
}  // namespace

struct hns_sim::Multigrid {
	hns_solve_method m{};
	bool built = false;
	std::vector<Level> levels;       // levels[i] is level i + 1
	std::vector<uint64_t> leaves;    // per level, level 0 included
	Pooled mem;                      // masks, tables and buffers of every level: one pooled allocation kept with the sim
	void drop_grids() {
		for (Level& L : levels) hns_grid_destroy(L.grid);
		levels.clear();
		leaves.clear();
		built = false;
	}
};

// Level l + 1 from level l on the host (include/hns.h: "The hierarchy"): the distinct floor(origin / 16) * 8, each fine leaf's parent and octant, each coarse leaf's
// children. fine: n x 4 ints (x, y, z, pad: Topology::origins). -> coarse origins (m x 3, lexicographic), parent (n x 2), child (m x 8)
static void coarsen(const int32_t* fine, size_t n, std::vector<int32_t>& coarse, std::vector<int>& parent, std::vector<int>& child) {
	typedef std::array<int32_t, 3> Key;
	std::map<Key, int> index;
	for (size_t i = 0; i < n; ++i) index.emplace(Key{(fine[4 * i] >> 4) * 8, (fine[4 * i + 1] >> 4) * 8, (fine[4 * i + 2] >> 4) * 8}, 0);  // (>> of a negative int: floor)
	coarse.clear();
	for (auto& kv : index) {
		kv.second = (int)(coarse.size() / 3);
		coarse.insert(coarse.end(), kv.first.begin(), kv.first.end());
	}
	parent.assign(2 * n, 0);
	child.assign(8 * index.size(), -1);
	for (size_t i = 0; i < n; ++i) {
		const int32_t* o = fine + 4 * i;
		const int pl = index[Key{(o[0] >> 4) * 8, (o[1] >> 4) * 8, (o[2] >> 4) * 8}];
		const int oct = ((o[0] >> 3) & 1) * 4 + ((o[1] >> 3) & 1) * 2 + ((o[2] >> 3) & 1);
		parent[2 * i] = pl, parent[2 * i + 1] = oct;
		child[(size_t)pl * 8 + oct] = (int)i;
	}
}

// Builds the hierarchy of the sim's current grid: coarse grids through the existing device builder, tables by copies and masks by k_mg_masks on a private stream that is
// waited for. Synchronous; never called on a capturing stream (hns_mg_ready).
static int build_hierarchy(hns_sim* s, const char* who) {
	hns_sim::Multigrid& mg = *s->mg;
	hns_grid* g0 = s->grid;
	if (g0->first_active != 0 || g0->n_active != (uint64_t)g0->topo.n_leaves) {
		set_error("%s: a solve method is set and the grid's launch range is not the whole grid", who);
		return HNS_ERR_INVALID_ARGUMENT;
	}
	DeviceScope on(s->device);
	mg.drop_grids();
	struct Host {
		std::vector<int> parent, child;
	};
	std::vector<Host> host;
	mg.leaves.push_back((uint64_t)g0->topo.n_leaves);
	const hns_grid* below = g0;
	// levels end at one leaf, at max_levels, or where a coarser level would have no fewer leaves than the one below it (leaves either side of coordinate 0 never merge)
	while (mg.leaves.back() > 1 && (mg.m.max_levels == 0 || (int)mg.leaves.size() < mg.m.max_levels)) {
		std::vector<int32_t> origins;
		Host h;
		coarsen(below->topo.origins.data(), (size_t)below->topo.n_leaves, origins, h.parent, h.child);
		if (origins.size() / 3 >= (size_t)below->topo.n_leaves) break;
		int rc = HNS_OK;
		Level L;
		L.n = origins.size() / 3;
		L.grid = hns_grid_create_from_leaves(origins.data(), L.n, 2.0f * below->voxel_size, HNS_GRID_DEFAULT, &rc);
		if (!L.grid) {
			mg.drop_grids();
			return rc;
		}
		mg.levels.push_back(L);
		mg.leaves.push_back(L.n);
		host.push_back(std::move(h));
		below = L.grid;
	}
	// one allocation: per level p | rhs | masks | child | parent (and 256 bytes to spare behind them)
	auto slices = [&](const Slice& slice) {
		for (size_t i = 0; i < mg.levels.size(); ++i) {
			Level& L = mg.levels[i];
			slice(L.p, 2048 * L.n), slice(L.rhs, 2048 * L.n), slice(L.masks, 64 * L.n), slice(L.child, 32 * L.n), slice(L.parent, 8 * mg.leaves[i]);
		}
	};
	const size_t need = 256 + carve(nullptr, slices);
	if (int rc = mg.mem.reserve(need, s->device)) {  // (a put waits for the device: nothing still reads the old block)
		mg.drop_grids();
		return rc;
	}
	PrivateStream own;
	HNS_TRY(own.create());
	const hipStream_t st = own.st;
	HNS_HIP(hipMemsetAsync(mg.mem.p, 0, need, st));  // (zeroed when drawn; every cycle writes what it reads all the same: tests/test_multigrid_pool_gpu.py)
	carve(mg.mem.p, slices);
	for (size_t i = 0; i < mg.levels.size(); ++i) {
		Level& L = mg.levels[i];
		HNS_HIP(hipMemcpyAsync(L.child, host[i].child.data(), 32 * L.n, hipMemcpyHostToDevice, st));
		HNS_HIP(hipMemcpyAsync(L.parent, host[i].parent.data(), 8 * mg.leaves[i], hipMemcpyHostToDevice, st));
		k_mg_masks<<<(unsigned)L.n, 64, 0, st>>>(L.child, i ? mg.levels[i - 1].masks : nullptr, L.masks);
	}
	HNS_TRY(launch_status(who));
	HNS_HIP(hipStreamSynchronize(st));  // (the host tables above live until here)
	mg.built = true;
	return HNS_OK;
}

int hns_mg_ready(hns_sim* s, void* stream, const char* who) {
	if (s->mg->built) return HNS_OK;
	if (stream_is_capturing(stream)) {
		set_error("%s: a solve method is set, the hierarchy of this grid is not built yet (the host derives its coarse leaves) and the stream is capturing", who);
		return HNS_ERR_INVALID_ARGUMENT;
	}
	return build_hierarchy(s, who);
}

void hns_sim_drop_hierarchy(hns_sim* s) {
	if (s->mg) s->mg->drop_grids();
}

void hns_sim_free_multigrid(hns_sim* s) {
	if (!s->mg) return;
	s->mg->drop_grids();
	delete s->mg;  // (mem goes back to the pool with it)
	s->mg = nullptr;
}

// ---------------------------------------------------------------------------------------------------------------
// the cycle
// ---------------------------------------------------------------------------------------------------------------

namespace {
struct Cycle {
	hns_sim* s;
	hns_sim::Multigrid& mg;
	float **cur, **other;  // level 0's p and its ping-pong twin
	hipStream_t st;
	void* stream;

	const unsigned char* masks(size_t l) const { return l ? mg.levels[l - 1].masks : nullptr; }
	hns_grid* grid(size_t l) const { return l ? mg.levels[l - 1].grid : s->grid; }
	float* p(size_t l) const { return l ? mg.levels[l - 1].p : *cur; }
	const float* rhs(size_t l) const { return l ? mg.levels[l - 1].rhs : s->div; }

	int smooth(size_t l, int iterations, float dx, bool from_zero) {
		if (l == 0) {  // the temporally blocked SOR kernels, as the SOR method runs them
			int in_b = 0;
			HNS_TRY(hns_rbgs_iterate(s->grid, s->div, *cur, *other, dx, mg.m.omega, iterations, &in_b, stream, from_zero));
			if (in_b) std::swap(*cur, *other);
			return HNS_OK;
		}
		const Level& L = mg.levels[l - 1];
		const GridDev gd = L.grid->dev();
		for (int i = 0; i < 2 * iterations; ++i) k_mg_color<<<(unsigned)L.n, 256, 0, st>>>(gd, L.masks, L.rhs, L.p, dx * dx, mg.m.omega, i & 1);
		return HNS_OK;
	}
	// one cycle on level l (include/hns.h: "One cycle on level l"); dx: this level's voxel size. from_zero: level 0 of a solve's first cycle
	int run(size_t l, float dx, bool from_zero) {
		if (l == mg.levels.size()) return smooth(l, mg.m.coarse_iterations, dx, from_zero);
		HNS_TRY(smooth(l, mg.m.pre, dx, from_zero));
		const Level& C = mg.levels[l];
		const float dx2 = dx * dx;
		k_mg_restrict<<<(unsigned)C.n, 512, 0, st>>>(grid(l)->dev(), masks(l), rhs(l), p(l), dx2, -0.75f / dx2, C.child, C.rhs, C.p);
		HNS_TRY(run(l + 1, 2.0f * dx, false));  // (from e = 0: k_mg_restrict has just zeroed it)
		k_mg_prolong<<<(unsigned)mg.leaves[l], 64, 0, st>>>(C.grid->dev(), C.parent, C.p, masks(l), p(l));
		return smooth(l, mg.m.post, dx, false);
	}
};
}  // namespace

int hns_mg_cycles(hns_sim* s, float** cur, float** other, float dx, int cycles, bool first, void* stream) {
	Cycle c{s, *s->mg, cur, other, (hipStream_t)stream, stream};
	for (int i = 0; i < cycles; ++i) HNS_TRY(c.run(0, dx, first && i == 0));
	return launch_status("hns_sim_pressure_solve (V-cycle)");
}

// `pressure=` of hns_sim_substep_plan under method 1: vcycle<pre,post,coarse_iterations>/L<levels>: the fine sweeps' kernel + the three coarse-level kernels
std::string hns_mg_plan(hns_sim* s) {
	const hns_sim::Multigrid& mg = *s->mg;
	char sor[256];
	if (hns_grid_rbgs_plan(s->grid, std::max(mg.m.pre, mg.m.post), sor, sizeof(sor), nullptr, nullptr) != HNS_OK) sor[0] = 0;
	std::string out = "vcycle<" + std::to_string(mg.m.pre) + "," + std::to_string(mg.m.post) + "," + std::to_string(mg.m.coarse_iterations) + ">";
	out += mg.built ? "/L" + std::to_string(mg.leaves.size()) : std::string("/L?");  // (?: a regrid dropped the hierarchy; the next solve builds it)
	out += ":" + std::string(sor, strcspn(sor, ":"));
	if (!mg.built || mg.leaves.size() > 1) out += "+k_mg_restrict+k_mg_color+k_mg_prolong";
	return out;
}

extern "C" {

int hns_sim_set_solve_method(hns_sim* s, const hns_solve_method* m) {
	const char* who = "hns_sim_set_solve_method";
	if (!s) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_set_solve_method: null sim");
	if (s->cached) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_set_solve_method: the sim belongs to a grid's cook cache");
	if (m && m->method != 0 && m->method != 1) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_set_solve_method: method must be 0 (SOR) or 1 (V-cycle)");
	if (!m || m->method == 0) {  // back to SOR (the other members of a method-0 struct are not looked at)
		hns_sim_free_multigrid(s);
		return HNS_OK;
	}
	if (m->pre < 0 || m->post < 0 || m->pre + (long long)m->post < 1) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_set_solve_method: pre and post must be >= 0 and not both 0");
	if (m->coarse_iterations < 1) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_set_solve_method: coarse_iterations must be at least 1");
	if (m->max_levels < 0) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_set_solve_method: max_levels must be 0 (down to one leaf) or positive");
	if (!(m->omega > 0.0f && m->omega < 2.0f)) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_set_solve_method: omega must lie strictly between 0 and 2");
	if (!s->grid || !s->grid->on_device) return fail(HNS_ERR_NO_DEVICE, "hns_sim_set_solve_method: the sim's grid has no device tables");
	if (s->grid->first_active != 0 || s->grid->n_active != (uint64_t)s->grid->topo.n_leaves)
		return fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_set_solve_method: the grid's launch range is not the whole grid");
	const bool fresh = !s->mg;
	if (fresh) s->mg = new (std::nothrow) hns_sim::Multigrid{};
	if (!s->mg) return fail(HNS_ERR_RUNTIME, "hns_sim_set_solve_method: out of memory");
	const hns_solve_method before = s->mg->m;
	const bool rebuild = !s->mg->built || before.max_levels != m->max_levels;
	s->mg->m = *m;
	if (rebuild) {
		const int rc = build_hierarchy(s, who);
		if (rc != HNS_OK) {  // sim unchanged
			if (fresh)
				hns_sim_free_multigrid(s);
			else
				s->mg->m = before;
			return rc;
		}
	}
	return HNS_OK;
}

int hns_sim_solve_levels(hns_sim* s, int* n_levels, uint64_t* leaves_per_level, int capacity) {
	if (!s || !n_levels || capacity < 0) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_sim_solve_levels: bad arguments");
	if (!s->mg) return fail(HNS_ERR_RUNTIME, "hns_sim_solve_levels: no solve method is set on this sim");
	HNS_TRY(hns_mg_ready(s, nullptr, "hns_sim_solve_levels"));
	*n_levels = (int)s->mg->leaves.size();
	for (int i = 0; leaves_per_level && i < std::min(capacity, *n_levels); ++i) leaves_per_level[i] = s->mg->leaves[(size_t)i];
	return HNS_OK;
}

}  // extern "C"
