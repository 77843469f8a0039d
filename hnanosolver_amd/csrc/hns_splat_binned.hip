// hns_splat_binned.hip -- point values added into fields THROUGH A LEAF ORDER (include/hns.h: hns_point_order_splat): the arithmetic, the accumulator and the passes of
// hns_splat.hip, the sums of a leaf's voxels kept in LDS by the one workgroup that owns the leaf, the fields written with plain stores. The atomic path of hns_splat.hip /
// hns_rasterize.hip is bound by the rate of global 64-bit atomic requests; here the only global atomics are those of the tail.
//   k_binned_points  the tail: ranks leaf_start[L] .. n -- points whose cell's leaf is absent and points that do not sort --, whose taps may still land. One thread per point,
//                    a fixed grid striding over the range it reads on the device, integer atomics into the grid's accumulator and its touched words: what k_splat_points
//                    and k_splat_radial do. Where status is asked for it walks every rank (status depends on positions only) and adds for the tail ranks alone.
//   k_binned_leaf    one workgroup per leaf Q: the ranks of every source leaf whose points can reach Q (Q's nbr27 row), each point's candidates recomputed with the shared
//                    functions and clipped to Q, splat_term's integers added into LDS (ds_add_u64); then Q's piece of the global accumulator -- what the tail left there --
//                    is added in and zeroed, and the shared finish rule writes the fields. So a voxel reached by a tail point and a binned point gets one sum and one
//                    rounded add: the tail kernel runs first for that reason alone.
// Every (point, tap, channel) term is evaluated by exactly one workgroup: the tail kernel for a tail rank, else the workgroup of the leaf the tap lies in. No kernel waits
// on another workgroup; every dependence is a launch boundary. No float atomics, no scratch. Every per-point row index is a rank below n or perm[rank], which the sort left
// below n; every field, mask and accumulator index is a voxel of an existing leaf: the leaf kernel clips to its own leaf whatever the positions hold.
// Known limit: one workgroup per destination leaf, so a point set concentrated in a few leaves is summed by a few workgroups.
#include "hns_points.hpp"

#include <cmath>

using namespace hns;

namespace {

constexpr int kBinnedBlock = 256;
constexpr int kTailBlocks = 512;  // k_binned_points: a fixed grid, since the host never learns how long the tail is

// LDS per kernel, stated and held
constexpr int kLdsLeaf = 512 * kSplatChannels * 8 + 64 + 2 * 27 * 4;  // k_binned_leaf: the sums, the mask copy, the source ranges: 16,664 bytes and padding, nine workgroups a CU
static_assert(kLdsLeaf <= 17 * 1024, "k_binned_leaf: LDS per workgroup");

// Radial: a point of leaf P has Floor(x) in P, lo = Floor(x - r) + 1 >= Floor(x) - (ceil(r) + 1) and lo + E - 1 <= Floor(x) + floor(r) + 3 (one rounding of x - r included).
// With r <= 4 that is at most 8 voxels out on either side: the box lies under P + {-1, 0, 1}^3, so the 27 leaves of Q's nbr27 row hold every point that can reach Q.
constexpr float kBinnedMaxRadius = 4.0f;  // (check_splat_spec: radius in (0, 4])
static_assert((int)kBinnedMaxRadius + 1 + 1 <= 8 && (int)kBinnedMaxRadius + 3 <= 8, "a radial box reaches beyond the 27 neighbours");

// the order as the kernels read it. rows: 0 -- per-point row perm[r] belongs to rank r; 1 -- row r does
struct OrderDev {
	const unsigned *perm, *leaf_start;
	unsigned n;
	int rows;
};

__device__ __forceinline__ unsigned row_of(const OrderDev& o, unsigned r) { return o.rows ? r : o.perm[r]; }  // (< n: the sort's permutation of 0 .. n - 1)

// the point values of row `row`: a channel without values is the weight channel of an average (1.0f)
__device__ __forceinline__ void load_values(const SplatChannels& ch, unsigned row, float (&v)[kSplatChannels]) {
#pragma unroll
	for (int q = 0; q < kSplatChannels; ++q) v[q] = q < ch.n ? (ch.c[q].val ? ch.c[q].val[(size_t)row * (unsigned)ch.c[q].stride + (unsigned)ch.c[q].off] : 1.0f) : 0.0f;
}

// one add per wave that has something to report (whole waves get here)
__device__ __forceinline__ void report_rejected(unsigned rej, unsigned long long* __restrict__ rejected) {
	if (!rejected) return;
#pragma unroll
	for (int m = 1; m < 64; m *= 2) rej += (unsigned)__shfl_xor((int)rej, m);
	if ((threadIdx.x & 63u) == 0 && rej) atomicAdd(rejected, (unsigned long long)rej);
}

// ---- the tail --------------------------------------------------------------------------------------------------------------------------------------------------------------

// The terms of one landed tap (flat voxel t, weight w) of the point in row `row` into the global accumulator, as k_splat_points adds them. The channels are walked by a
// loop that is not unrolled and the value is loaded per term: the tail is short, and the channel table stays in the kernel's arguments instead of sixteen scalar registers.
__device__ __forceinline__ void tail_tap(const SplatChannels& ch, unsigned row, int t, float w, double scale, unsigned long long* __restrict__ acc, int S,
                                         int* __restrict__ touched, unsigned* __restrict__ masks, unsigned& rej) {
	touched[t >> 9] = 1;
	if (masks && w > 0.0f) atomicOr(masks + ((unsigned)t >> 5), 1u << ((unsigned)t & 31u));
#pragma unroll 1
	for (int q = 0; q < ch.n; ++q) {
		const float v = ch.c[q].val ? ch.c[q].val[(size_t)row * (unsigned)ch.c[q].stride + (unsigned)ch.c[q].off] : 1.0f;  // (no values: the weight channel of an average)
		long long k;
		if (!splat_term(w * v, scale, &k))
			++rej;
		else if (k)
			atomicAdd(acc + (size_t)t * (unsigned)S + (unsigned)q, (unsigned long long)k);
	}
}

// Ranks first .. n - 1, first = 0 where status is asked for, else leaf_start[L]: status for every rank, terms for the tail ranks. RADIAL: the box of hns_rasterize.hip walked
// by one thread (one lookup for each of the up to eight leaves under it, then its candidates one by one); else the cell of point_cell.
template <bool RADIAL>
__global__ __launch_bounds__(kBinnedBlock) void k_binned_points(const GridDev g, const SplatChannels ch, const OrderDev o, const float* __restrict__ xyz,
                                                                 const float* __restrict__ radii, const float bound, const double scale, unsigned long long* __restrict__ acc,
                                                                 const int S, int* __restrict__ touched, unsigned* __restrict__ masks, unsigned char* __restrict__ status,
                                                                 unsigned long long* __restrict__ rejected) {
	const unsigned tail = o.leaf_start[g.n_leaves];  // (<= n)
	unsigned rej = 0;
	for (unsigned r = (status ? 0u : tail) + blockIdx.x * (unsigned)kBinnedBlock + threadIdx.x; r < o.n; r += (unsigned)(kTailBlocks * kBinnedBlock)) {
		const unsigned row = row_of(o, r);
		const bool add = r >= tail;
		const f3 pos = ld3(xyz, (int)row);
		if (RADIAL) {
			const float rad = radii ? radii[row] : bound;
			int in_footprint = 0, landed = 0;
			if (radial_point(pos.x, pos.y, pos.z, rad, bound)) {
				const int E = radial_extent(rad), i0 = radial_lo(pos.x, rad), j0 = radial_lo(pos.y, rad), k0 = radial_lo(pos.z, rad);
				const float inv = radial_inv(rad);
				const int ox = i0 & ~7, oy = j0 & ~7, oz = k0 & ~7;
				const bool cx = ((i0 + E - 1) & ~7) != ox, cy = ((j0 + E - 1) & ~7) != oy, cz = ((k0 + E - 1) & ~7) != oz;  // the box reaches into the next leaf (E <= 8: at most one)
				int L[8];  // leaf c = di*4 + dj*2 + dk under the box: one lookup per leaf (L is indexed by constants only: registers)
#pragma unroll
				for (int c = 0; c < 8; ++c) {
					const bool need = (!(c & 4) || cx) && (!(c & 2) || cy) && (!(c & 1) || cz);
					L[c] = need ? d_find_leaf(g, (c & 4) ? plus8(ox) : ox, (c & 2) ? plus8(oy) : oy, (c & 1) ? plus8(oz) : oz) : -1;
				}
				int i = i0, j = j0, k = k0;
				for (int m = 0; m < E * E * E; ++m) {  // the candidates, z fastest
					const int c = ((i & ~7) != ox ? 4 : 0) | ((j & ~7) != oy ? 2 : 0) | ((k & ~7) != oz ? 1 : 0);
					int leaf = L[0];
#pragma unroll
					for (int a = 1; a < 8; ++a) leaf = c == a ? L[a] : leaf;
					float w = 0.0f;
					const bool in = radial_weight((float)i - pos.x, (float)j - pos.y, (float)k - pos.z, inv, &w), land = in && leaf >= 0;
					in_footprint += in, landed += land;
					if (land && add) tail_tap(ch, row, leaf * 512 + (int)(((unsigned)i & 7u) << 6 | ((unsigned)j & 7u) << 3 | ((unsigned)k & 7u)), w, scale, acc, S, touched, masks, rej);
					if (++k == k0 + E) {
						k = k0;
						if (++j == j0 + E) j = j0, ++i;
					}
				}
			}
			if (status) status[row] = (unsigned char)(in_footprint > 0 && landed == in_footprint ? 2 : landed > 0 ? 1 : 0);
		} else {
			int landed = 0;
			if (finite_f(pos.x) && finite_f(pos.y) && finite_f(pos.z)) {  // (any other point lands nowhere)
				Cursor none{-1, 0, 0, 0};
				const Cell C = point_cell<false>(g, none, pos.x, pos.y, pos.z);
				float w[8];
				splat_weights(C.fx, C.fy, C.fz, w);
#pragma unroll
				for (int c = 0; c < 8; ++c) {
					if (C.t[c] < 0) continue;
					++landed;
					if (add) tail_tap(ch, row, C.t[c], w[c], scale, acc, S, touched, masks, rej);
				}
			}
			if (status) status[row] = (unsigned char)landed;
		}
	}
	report_rejected(rej, rejected);
}

// ---- one workgroup per leaf ------------------------------------------------------------------------------------------------------------------------------------------------

// the terms of one candidate inside Q (local voxel vox, weight w) into the workgroup's sums
__device__ __forceinline__ void leaf_tap(const SplatChannels& ch, const float (&v)[kSplatChannels], unsigned vox, float w, double scale, unsigned long long* s_sum, int S,
                                         unsigned* s_mask, bool masks, unsigned& rej) {
	if (masks && w > 0.0f) atomicOr(&s_mask[vox >> 5], 1u << (vox & 31u));
#pragma unroll
	for (int q = 0; q < kSplatChannels; ++q) {
		if (q >= ch.n) break;
		long long k;
		if (!splat_term(w * v[q], scale, &k))
			++rej;
		else if (k)
			atomicAdd(&s_sum[vox * (unsigned)S + (unsigned)q], (unsigned long long)k);
	}
}

// G = 0: trilinear, one point per thread. G = 1, 4, 16, 64: radial, G = EB^2 lanes per point as in k_splat_radial -- lane t of a group is column (y, z) = (t / EB, t % EB) of
// the point's box and walks it along x. Source leaves: slot s of Q's nbr27 row, s = (dx+1)*9 + (dy+1)*3 + (dz+1); trilinear points reach one voxel up, so only the eight
// slots with every d in {-1, 0} count; radial: all 27 (above). At level 1 the keys are voxel keys, and keys[r] & 511 could reject a
// trilinear neighbour's point without its position being loaded; measured, that filter LOSES where the points are spread over the leaves (one float 0.40 against 0.31 ms at 256^3,
// 2^22 points: on ranked rows the position is a coalesced load, and the key is one more load in front of it), so it is not built: both levels run the same code.
template <int G>
__global__ __launch_bounds__(kBinnedBlock) void k_binned_leaf(const GridDev g, const SplatChannels ch, const OrderDev o, const float* __restrict__ xyz,
                                                               const float* __restrict__ radii, const float bound, const double scale, const double quantum,
                                                               unsigned long long* __restrict__ acc, const int S, int* __restrict__ touched, unsigned* __restrict__ masks,
                                                               unsigned long long* __restrict__ rejected) {
	constexpr int EB = G <= 1 ? 1 : G == 4 ? 2 : G == 16 ? 4 : 8, PG = G ? G : 1;
	static_assert(G == 0 || EB * EB == G, "G is 0, 1, 4, 16 or 64");
	__shared__ unsigned long long s_sum[512 * kSplatChannels];
	__shared__ unsigned s_mask[16];
	__shared__ unsigned s_lo[27], s_hi[27];
	static_assert(sizeof(s_sum) + sizeof(s_mask) + sizeof(s_lo) + sizeof(s_hi) == kLdsLeaf, "k_binned_leaf: LDS");
	const unsigned Q = blockIdx.x, tid = threadIdx.x;  // (the launch has one workgroup per leaf of the grid, ghost leaves included)

	if (tid < 27u) {
		const bool source = G != 0 || (tid / 9u <= 1u && (tid / 3u) % 3u <= 1u && tid % 3u <= 1u);
		const int P = source ? g.nbr27[Q * 27u + tid] : -1;
		s_lo[tid] = P >= 0 ? o.leaf_start[P] : 0u, s_hi[tid] = P >= 0 ? o.leaf_start[P + 1] : 0u;
	}
	const bool merge = touched[Q] != 0;  // the tail landed here
	__syncthreads();
	bool live = merge;
#pragma unroll
	for (int s = 0; s < 27; ++s) live |= s_lo[s] < s_hi[s];
	if (!live) return;  // (the same answer in every thread) nothing arrives: nothing is zeroed, nothing written

	for (unsigned e = tid; e < 512u * (unsigned)S; e += (unsigned)kBinnedBlock) s_sum[e] = 0ull;
	if (masks && tid < 16u) s_mask[tid] = masks[Q * 16u + tid];
	__syncthreads();

	const int4 qo = g.origins[Q];
	unsigned rej = 0;
	const int t = (int)(tid % (unsigned)PG), ly = t / EB, lz = t % EB;
	for (int s = 0; s < 27; ++s) {
		const unsigned hi = s_hi[s];
		for (unsigned r = s_lo[s] + tid / (unsigned)PG; r < hi; r += (unsigned)(kBinnedBlock / PG)) {
			const unsigned row = row_of(o, r);
			const f3 pos = ld3(xyz, (int)row);
			float v[kSplatChannels];
			if (G == 0) {
				if (!(finite_f(pos.x) && finite_f(pos.y) && finite_f(pos.z))) continue;
				const int i = __float2int_rd(pos.x), j = __float2int_rd(pos.y), k = __float2int_rd(pos.z);  // the cell and the corners of point_cell
				float w[8];
				splat_weights(pos.x - (float)i, pos.y - (float)j, pos.z - (float)k, w);
				load_values(ch, row, v);
#pragma unroll
				for (int c = 0; c < 8; ++c) {
					const int ci = (int)((unsigned)i + (unsigned)(c >> 2)), cj = (int)((unsigned)j + (unsigned)((c >> 1) & 1)), ck = (int)((unsigned)k + (unsigned)(c & 1));
					if ((ci & ~7) != qo.x || (cj & ~7) != qo.y || (ck & ~7) != qo.z) continue;  // another leaf's
					leaf_tap(ch, v, ((unsigned)ci & 7u) << 6 | ((unsigned)cj & 7u) << 3 | ((unsigned)ck & 7u), w[c], scale, s_sum, S, s_mask, masks != nullptr, rej);
				}
			} else {
				const float rad = radii ? radii[row] : bound;
				if (!radial_point(pos.x, pos.y, pos.z, rad, bound)) continue;
				const int E = radial_extent(rad), i0 = radial_lo(pos.x, rad), j = radial_lo(pos.y, rad) + ly, k = radial_lo(pos.z, rad) + lz;
				if (ly >= E || lz >= E || (j & ~7) != qo.y || (k & ~7) != qo.z) continue;  // no column of the box, or another leaf's
				const float inv = radial_inv(rad);
				load_values(ch, row, v);
#pragma unroll
				for (int dx = 0; dx < EB; ++dx) {
					const int i = i0 + dx;
					float w;
					if (dx >= E || (i & ~7) != qo.x || !radial_weight((float)i - pos.x, (float)j - pos.y, (float)k - pos.z, inv, &w)) continue;
					leaf_tap(ch, v, ((unsigned)i & 7u) << 6 | ((unsigned)j & 7u) << 3 | ((unsigned)k & 7u), w, scale, s_sum, S, s_mask, masks != nullptr, rej);
				}
			}
		}
	}
	report_rejected(rej, rejected);
	__syncthreads();

	if (masks && tid < 16u) masks[Q * 16u + tid] = s_mask[tid];
	if (merge) {  // (the same answer in every thread) Q's piece of the global accumulator joins the sums and is left zero
		unsigned long long* __restrict__ piece = acc + (size_t)Q * 512u * (unsigned)S;
		for (unsigned e = tid; e < 512u * (unsigned)S; e += (unsigned)kBinnedBlock) {
			s_sum[e] += piece[e];
			piece[e] = 0ull;
		}
		if (tid == 0) touched[Q] = 0;
		__syncthreads();
	}
#pragma unroll
	for (int h = 0; h < 512 / kBinnedBlock; ++h) {
		const unsigned vox = (unsigned)(h * kBinnedBlock) + tid;
#pragma unroll
		for (int q = 0; q < kSplatChannels; ++q) {
			if (q >= ch.n) break;
			if (ch.average && q == 0) continue;  // W has no field
			const SplatChannel e = ch.c[q];
			splat_finish(ch.average, s_sum[vox * (unsigned)S + (unsigned)q], s_sum[vox * (unsigned)S], quantum, ch.min_weight,
			             e.field + ((size_t)Q * 512u + vox) * (unsigned)e.stride + (unsigned)e.off);
		}
	}
}

template <int G>
void launch_leaf(hipStream_t st, unsigned n_leaves, const GridDev& g, const SplatChannels& ch, const OrderDev& o, const float* xyz, const float* radii, float bound,
                 double scale, double quantum, unsigned long long* acc, int S, int* touched, unsigned* masks, unsigned long long* rejected) {
	hipLaunchKernelGGL(k_binned_leaf<G>, dim3(n_leaves), dim3(kBinnedBlock), 0, st, g, ch, o, xyz, radii, bound, scale, quantum, acc, S, touched, masks, rejected);
}

// ---- launcher --------------------------------------------------------------------------------------------------------------------------------------------------------------

// splat_points of hns_splat.hip through the order `o`, on its stream; g is o's grid. Every refusal comes before the first launch.
int splat_ordered(const char* who, const hns_point_order* o, const hns_splat_spec& sp, float* const* fields, const int* ncomp, int n_fields, const float* xyz,
                  const float* const* values, int rows, int log2_quantum, unsigned char* masks, unsigned char* status, uint64_t* d_rejected) {
	if (!o->sorted) return refuse(who, "no sort has run on this object");
	if (rows != 0 && rows != 1) {
		set_error("%s: rows is %d (0: the arrays the sort saw, 1: their gather)", who, rows);
		return HNS_ERR_INVALID_ARGUMENT;
	}
	const uint64_t n = o->n;
	HNS_TRY(check_splat_lists(who, fields, ncomp, n_fields, values, n, log2_quantum));
	if (n == 0) return HNS_OK;
	HNS_TRY(check_splat_pointers(who, fields, n_fields, xyz, values, status, d_rejected));
	hns_grid* g = o->grid;
	const hipStream_t st = o->stream;
	if (g->topo.n_leaves == 0) {  // no leaf: nothing lands
		if (status) HNS_HIP(hipMemsetAsync(status, 0, n, st));
		return HNS_OK;
	}
	std::vector<SplatChannel> all;
	for (int i = 0; i < n_fields; ++i)
		for (int c = 0; c < ncomp[i]; ++c) all.push_back(SplatChannel{values[i], fields[i], ncomp[i], c, 0});
	HNS_TRY(splat_accumulator(g, std::min<int>(kSplatChannels, (int)all.size() + (sp.mode ? 1 : 0)), st));
	const int S = g->splat_channels;
	unsigned long long* acc = g->d_splat.as<unsigned long long>();
	int* touched = (int*)(g->d_splat.as<char>() + splat_acc_bytes(g, S));
	const double scale = std::ldexp(1.0, -log2_quantum), quantum = std::ldexp(1.0, log2_quantum);
	const unsigned n_leaves = (unsigned)g->topo.n_leaves;
	const OrderDev od{o->perm, o->leaf_start, (unsigned)n, rows};
	const GridDev gd = g->dev();
	unsigned long long* rej = (unsigned long long*)d_rejected;
	bool first = true;
	for (const SplatChannels& ch : splat_passes(all, sp)) {  // status and masks: positions only, written by the first pass
		unsigned* m = first ? (unsigned*)masks : nullptr;
		unsigned char* stat = first ? status : nullptr;
		first = false;
		if (sp.kernel) {
			hipLaunchKernelGGL(k_binned_points<true>, dim3(kTailBlocks), dim3(kBinnedBlock), 0, st, gd, ch, od, xyz, sp.d_radius, sp.radius, scale, acc, S, touched, m, stat, rej);
			switch (splat_radial_group(sp.radius)) {
			case 1: launch_leaf<1>(st, n_leaves, gd, ch, od, xyz, sp.d_radius, sp.radius, scale, quantum, acc, S, touched, m, rej); break;
			case 4: launch_leaf<4>(st, n_leaves, gd, ch, od, xyz, sp.d_radius, sp.radius, scale, quantum, acc, S, touched, m, rej); break;
			case 16: launch_leaf<16>(st, n_leaves, gd, ch, od, xyz, sp.d_radius, sp.radius, scale, quantum, acc, S, touched, m, rej); break;
			default: launch_leaf<64>(st, n_leaves, gd, ch, od, xyz, sp.d_radius, sp.radius, scale, quantum, acc, S, touched, m, rej); break;
			}
		} else {
			hipLaunchKernelGGL(k_binned_points<false>, dim3(kTailBlocks), dim3(kBinnedBlock), 0, st, gd, ch, od, xyz, nullptr, 0.0f, scale, acc, S, touched, m, stat, rej);
			launch_leaf<0>(st, n_leaves, gd, ch, od, xyz, nullptr, 0.0f, scale, quantum, acc, S, touched, m, rej);
		}
		if (int rc = launch_status(who)) {
			g->splat_dirty = true;  // whatever ran may have left sums behind: the next call clears first
			return rc;
		}
	}
	return HNS_OK;
}

}  // namespace

extern "C" {

int hns_point_order_splat(const hns_point_order* o, float* const* fields, const int* ncomp, int n_fields, const float* d_xyz, const float* const* values, int rows,
                          int log2_quantum, unsigned char* status, uint64_t* d_rejected) {
	const char* who = "hns_point_order_splat";
	HNS_TRY(check_order(o, who));
	return splat_ordered(who, o, o->grid->splat_spec, fields, ncomp, n_fields, d_xyz, values, rows, log2_quantum, nullptr, status, d_rejected);
}

int hns_point_order_splat_sim(const hns_point_order* o, hns_sim* s, const char* const* names, int n_names, const float* velocity_values, const float* d_xyz,
                              const float* const* values, int rows, int log2_quantum, int activate, unsigned char* status, uint64_t* d_rejected) {
	const char* who = "hns_point_order_splat_sim";
	HNS_TRY(check_order(o, who));
	if (int rc = check_sim(s, who)) return rc;
	if (s->grid != o->grid) return refuse(who, "the sim's grid is not the grid of the point order");
	std::vector<float*> fields;
	std::vector<const float*> vals;
	std::vector<int> ncomp, which;
	HNS_TRY(sim_splat_fields(who, s, names, n_names, velocity_values, values, fields, vals, ncomp, which));
	HNS_TRY(splat_ordered(who, o, s->splat_spec, fields.data(), ncomp.data(), (int)fields.size(), d_xyz, vals.data(), rows, log2_quantum, activate ? s->d_masks.as<unsigned char>() : nullptr, status,
	                      d_rejected));
	if (o->n) sim_splat_wrote(s, which, velocity_values != nullptr);
	return HNS_OK;
}

}  // extern "C"
