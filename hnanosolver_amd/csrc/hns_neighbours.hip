// hns_neighbours.hip -- point neighbourhoods through a leaf order (include/hns.h: "POINT NEIGHBOURHOODS THROUGH A LEAF ORDER" states the definition): the cell table of a
// voxel-level sort -- the ranks of every voxel as one range -- and the query that reads it: for every point the count of the points around it, a density and a push, summed
// over pairs. The second reader of the order's ranges, next to the binned splat (hns_splat_binned.hip). The pair arithmetic is hns_neighbours.hpp's.
//   k_cell_table     one workgroup per leaf: a histogram of the leaf's ranks over 512 LDS counters (the ranks are sorted: a wave adds each run of equal keys once), an
//                    exclusive scan (hns_blockscan.hpp) on top of leaf_start[leaf], plain stores; the last leaf's first thread writes the closing entry
//   k_neighbours     work goes by RANK, so the lanes of a wave hold points of one voxel or of adjacent ones. G lanes share a point and split the (x, y) columns of its
//                    box; a column's z-run is one contiguous rank range per leaf under it (z is the low bits of the voxel key), read from two entries of the table. The
//                    int64 partial sums of a group are combined with cross-lane integer adds, which makes the split free. Ranks that take no part write their zeros here.
// No kernel waits on another workgroup, no float atomics, no scratch. Addresses: a leaf comes from the origin hash, by coordinates, never from a key; the table's entries
// are ranks <= leaf_start[L] <= n and perm's are rows < n, both the object's own buffers.
#include "hns_blockscan.hpp"
#include "hns_neighbours.hpp"
#include "hns_points.hpp"

namespace hns {
namespace {

constexpr int kCellBlock = kBlockScanThreads;  // k_cell_table: two voxels per thread
constexpr int kNbrBlock = 256;
static_assert(2 * kCellBlock == 512, "k_cell_table gives every thread two voxels of a leaf");

__global__ __launch_bounds__(kCellBlock) void k_cell_table(const unsigned* __restrict__ keys, const unsigned* __restrict__ leaf_start, const unsigned n_leaves,
                                                           unsigned* __restrict__ cell_start) {
	__shared__ unsigned s_cnt[512];
	__shared__ unsigned s_wave[kBlockScanWaves];
	const unsigned leaf = blockIdx.x, t = threadIdx.x, lane = t & 63u;
	s_cnt[t] = 0, s_cnt[t + kCellBlock] = 0;
	__syncthreads();
	const unsigned r0 = leaf_start[leaf], r1 = leaf_start[leaf + 1];
	for (unsigned base = r0; base < r1; base += (unsigned)kCellBlock) {  // (the same trips in every lane: the ballot sees whole waves)
		const unsigned r = base + t;
		const bool valid = r < r1;
		const unsigned v = valid ? keys[r] & 511u : ~0u;
		const unsigned before = (unsigned)__shfl_up((int)v, 1);
		const bool head = valid && (lane == 0 || before != v);
		// a run of equal keys ends where the next one starts or the valid lanes end
		const unsigned long long ends = __ballot(head || !valid);
		const unsigned long long above = lane == 63u ? 0ull : ends >> (lane + 1u);
		const unsigned len = above ? (unsigned)__ffsll((long long)above) : 64u - lane;
		if (head) atomicAdd(&s_cnt[v], len);
	}
	__syncthreads();
	const unsigned a0 = s_cnt[2 * t], a1 = s_cnt[2 * t + 1];
	unsigned sum;
	const unsigned at = r0 + block_scan(a0 + a1, s_wave, sum);
	cell_start[(size_t)leaf * 512u + 2u * t] = at;
	cell_start[(size_t)leaf * 512u + 2u * t + 1u] = at + a0;
	if (leaf == n_leaves - 1u && t == 0) cell_start[(size_t)n_leaves * 512u] = leaf_start[n_leaves];
}

// one of the (up to) eight leaves under a box, c = di*4 + dj*2 + dk with dk fixed by the caller: selects, so that the ids stay in registers
__device__ __forceinline__ int pick_leaf(const int (&L)[8], int cxy, int dk) { return cxy == 0 ? L[dk] : cxy == 2 ? L[2 | dk] : cxy == 4 ? L[4 | dk] : L[6 | dk]; }

template <typename T>
__device__ __forceinline__ T group_sum(T v, int G) {
	for (int m = 1; m < G; m *= 2) v += __shfl_xor(v, m);
	return v;
}

// RANKED: row r of xyz and of the outputs belongs to rank r; else row perm[r]
template <int G, bool RANKED>
__global__ __launch_bounds__(kNbrBlock) void k_neighbours(const GridDev g, const unsigned* __restrict__ perm, const unsigned* __restrict__ leaf_start,
                                                          const unsigned* __restrict__ cell_start, const float* __restrict__ xyz, const unsigned n, const float h,
                                                          unsigned* __restrict__ count, float* __restrict__ density, float* __restrict__ push) {
	static_assert(G == 4 || G == 16 || G == 32, "G is 4, 16 or 32");
	const unsigned r = blockIdx.x * (unsigned)(kNbrBlock / G) + threadIdx.x / (unsigned)G;
	const int lane = (int)(threadIdx.x & 63u), t = (int)(threadIdx.x % (unsigned)G);
	const unsigned inside = leaf_start[g.n_leaves];
	unsigned row = 0;
	f3 x = {0.0f, 0.0f, 0.0f};
	bool ok = false;
	if (r < n) {
		row = RANKED ? r : perm[r];
		x = ld3(xyz, (int)row);
		ok = r < inside && seeds_f(x.x) && seeds_f(x.y) && seeds_f(x.z);  // (a rank below `inside` seeds, by the contract; other positions must not widen the box)
	}
	int ilo = 0, ihi = -1, jlo = 0, jhi = -1, klo = 0, khi = -1;
	if (ok) neighbour_box(x.x, h, &ilo, &ihi), neighbour_box(x.y, h, &jlo, &jhi), neighbour_box(x.z, h, &klo, &khi);
	const int Ex = min(ihi - ilo + 1, kNeighbourMaxExtent), Ey = min(jhi - jlo + 1, kNeighbourMaxExtent);
	khi = min(khi, klo + kNeighbourMaxExtent - 1);
	const float inv = radial_inv(h);
	const int ox = ilo & ~7, oy = jlo & ~7, oz = klo & ~7;
	const bool cx = ((ilo + Ex - 1) & ~7) != ox, cy = ((jlo + Ey - 1) & ~7) != oy, cz = (khi & ~7) != oz;  // the box reaches into the next leaf (at most one)

	// the leaves under the box, leaf c = di*4 + dj*2 + dk: one lookup per leaf and point, handed round the group
	constexpr int NL = G >= 8 ? 1 : 8 / G;
	int mine[NL];
#pragma unroll
	for (int a = 0; a < NL; ++a) {
		const int c = t + a * G;
		const bool need = ok && c < 8 && (!(c & 4) || cx) && (!(c & 2) || cy) && (!(c & 1) || cz);
		mine[a] = need ? d_find_leaf(g, (c & 4) ? plus8(ox) : ox, (c & 2) ? plus8(oy) : oy, (c & 1) ? plus8(oz) : oz) : -1;
	}
	int L[8];
	const int first = lane & ~(G - 1);
#pragma unroll
	for (int c = 0; c < 8; ++c) L[c] = __shfl(mine[c / G], first + c % G);

	NeighbourSums s;
	const int columns = Ex * Ey;  // 0 for a point that takes no part
	for (int col = t; col < columns; col += G) {
		const int a = col / Ey, i = ilo + a, j = jlo + (col - a * Ey);
		const int cxy = ((i & ~7) != ox ? 4 : 0) | ((j & ~7) != oy ? 2 : 0);
		const unsigned local = ((unsigned)i & 7u) << 6 | ((unsigned)j & 7u) << 3;
#pragma unroll
		for (int dk = 0; dk < 2; ++dk) {  // the z-run below and above the leaf face
			const int leaf = pick_leaf(L, cxy, dk);
			const int k0 = dk ? oz + 8 : klo, k1 = dk ? khi : min(khi, oz + 7);
			if (leaf < 0 || k0 > k1) continue;
			const unsigned v = (unsigned)leaf * 512u + local;
			const unsigned q0 = cell_start[v + ((unsigned)k0 & 7u)], q1 = cell_start[v + ((unsigned)k1 & 7u) + 1u];
			for (unsigned q = q0; q < q1; ++q) {
				if (q == r) continue;
				const f3 y = ld3(xyz, (int)(RANKED ? q : perm[q]));
				neighbour_pair(x.x, x.y, x.z, y.x, y.y, y.z, inv, s);
			}
		}
	}
	s.count = group_sum(s.count, G);
	s.w = group_sum(s.w, G), s.px = group_sum(s.px, G), s.py = group_sum(s.py, G), s.pz = group_sum(s.pz, G);
	if (r < n && t == 0) {
		if (count) count[row] = s.count;
		if (density) density[row] = neighbour_total(s.w);
		if (push) {
			float* __restrict__ p = push + (size_t)row * 3u;
			p[0] = neighbour_total(s.px), p[1] = neighbour_total(s.py), p[2] = neighbour_total(s.pz);
		}
	}
}

// lanes that share a point: the columns of the largest box of this radius, ceil(2 h) + 1 cells an axis, rounded up to a group the wave divides into
int neighbour_group(float h) {
	const int e = radial_extent(h) + 1;
	return e <= 2 ? 4 : e <= 4 ? 16 : 32;
}

template <int G>
void launch_neighbours(const hns_point_order* o, const float* xyz, int rows, float h, unsigned* count, float* density, float* push) {
	const unsigned n = (unsigned)o->n, per_block = (unsigned)(kNbrBlock / G);
	const dim3 grid((n + per_block - 1u) / per_block), block(kNbrBlock);
	if (rows)
		hipLaunchKernelGGL((k_neighbours<G, true>), grid, block, 0, o->stream, o->grid->dev(), (const unsigned*)o->perm, (const unsigned*)o->leaf_start,
		                   o->cell_start.as<const unsigned>(), xyz, n, h, count, density, push);
	else
		hipLaunchKernelGGL((k_neighbours<G, false>), grid, block, 0, o->stream, o->grid->dev(), (const unsigned*)o->perm, (const unsigned*)o->leaf_start,
		                   o->cell_start.as<const unsigned>(), xyz, n, h, count, density, push);
}

// what the cell calls refuse about the object's sort
int check_voxel_sort(const hns_point_order* o, const char* who) {
	if (!o->sorted) return refuse(who, "no sort has run on this object");
	if (o->level != 1) return refuse(who, "the last sort is at level 0 (by leaf): the cell table needs a sort at level 1 (by voxel)");
	return HNS_OK;
}

// the table of the last sort, on the object's stream: drawn from the pool once, rebuilt by the first call behind every sort
int ensure_cells(hns_point_order* o, const char* who) {
	const size_t L = (size_t)o->n_leaves, bytes = 4 * (512 * L + 1);
	HNS_TRY(o->cell_start.reserve(bytes, o->device));
	if (o->cells_fresh) return HNS_OK;
	if (!o->n || !L) {
		HNS_HIP(hipMemsetAsync(o->cell_start.p, 0, bytes, o->stream));
	} else {
		hipLaunchKernelGGL(k_cell_table, dim3((unsigned)L), dim3(kCellBlock), 0, o->stream, (const unsigned*)o->keys, (const unsigned*)o->leaf_start, (unsigned)L,
		                   o->cell_start.as<unsigned>());
		HNS_TRY(launch_status(who));
	}
	o->cells_fresh = true;
	return HNS_OK;
}

}  // namespace
}  // namespace hns

using namespace hns;

extern "C" {

int hns_point_order_cells(hns_point_order* o, const uint32_t** d_cell_start) {
	const char* who = "hns_point_order_cells";
	HNS_TRY(check_order(o, who));
	HNS_TRY(check_voxel_sort(o, who));
	if (!d_cell_start) return refuse(who, "null d_cell_start");
	HNS_TRY(ensure_cells(o, who));
	*d_cell_start = o->cell_start.as<uint32_t>();
	return HNS_OK;
}

int hns_point_order_neighbours(hns_point_order* o, const float* d_xyz, int rows, float radius, uint32_t* d_count, float* d_density, float* d_push) {
	const char* who = "hns_point_order_neighbours";
	HNS_TRY(check_order(o, who));
	HNS_TRY(check_voxel_sort(o, who));
	if (rows != 0 && rows != 1) {
		set_error("%s: rows is %d (0: the arrays the sort saw, 1: their gather)", who, rows);
		return HNS_ERR_INVALID_ARGUMENT;
	}
	if (!neighbour_radius(radius)) {
		set_error("%s: radius %g (0 < radius <= 2)", who, (double)radius);
		return HNS_ERR_INVALID_ARGUMENT;
	}
	if (o->n && !d_xyz) return refuse(who, "d_xyz is null");
	if (!d_count && !d_density && !d_push) return refuse(who, "d_count, d_density and d_push are all null");
	const void* out[3] = {d_count, d_density, d_push};
	const char* names[3] = {"d_count", "d_density", "d_push"};
	for (int a = 0; a < 3; ++a) {
		if (!out[a]) continue;
		if (out[a] == (const void*)d_xyz) {
			set_error("%s: %s is d_xyz", who, names[a]);
			return HNS_ERR_INVALID_ARGUMENT;
		}
		for (int b = 0; b < a; ++b)
			if (out[a] == out[b]) {
				set_error("%s: %s and %s are the same buffer", who, names[b], names[a]);
				return HNS_ERR_INVALID_ARGUMENT;
			}
	}
	if (!o->n) return HNS_OK;
	HNS_TRY(ensure_cells(o, who));
	switch (neighbour_group(radius)) {
	case 4: launch_neighbours<4>(o, d_xyz, rows, radius, d_count, d_density, d_push); break;
	case 16: launch_neighbours<16>(o, d_xyz, rows, radius, d_count, d_density, d_push); break;
	default: launch_neighbours<32>(o, d_xyz, rows, radius, d_count, d_density, d_push); break;
	}
	return launch_status(who);
}

}  // extern "C"
