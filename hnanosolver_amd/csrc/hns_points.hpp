// hns_points.hpp -- the trilinear cell under an index-space position, shared by the kernel files that work at points: hns_points.hip (fields read at points, points
// traced through the velocity), hns_points_collide.hip (the same against a collision SDF), hns_splat.hip (point values added into fields), hns_rasterize.hip (the same with a radius) and hns_splat_binned.hip (the same through a leaf order). One statement of Floor, the tap indices and
// the fractions for both directions, and one of the splat's arithmetic -- weights, footprint, term, total, average -- for the kernels and the host mirror.
#pragma once

#include <cmath>

#include "hns_device.hpp"
#include "hns_radial.hpp"
#include "hns_seed.hpp"
#include "hns_simcall.hpp"  // refuse, check_sim, kMaxPoints and the rest of a call's host preamble

namespace hns {

// the trilinear cell under a position: flat voxel index of corner (di,dj,dk) at t[di*4+dj*2+dk] (-1: its leaf is absent) and the fractions
struct Cell {
	int t[8];
	float fx, fy, fz;
};

// The last leaf a thread of k_trace_points found and its origin (k_sample_points takes one sample per point and has none: CURSOR = false). The successive samples of one point (RK stages, steps) mostly land in that leaf or one of its 26 neighbours, whose
// ids are one row of nbr27: one load in place of a walk through the origin hash (hash slot, then the candidate's origin, then perhaps the next slot: dependent
// loads, one walk per distinct leaf under the cell). nbr27 is built from the same hash, so the answer is the hash's.
struct Cursor {
	int leaf, ox, oy, oz;  // leaf < 0: nothing found yet
};

__device__ __forceinline__ int plus8(int a) { return (int)((unsigned)a + 8u); }  // (wraps at the end of the int32 range, where no leaf lies beyond)

// is leaf offset d (a multiple of 8 voxels; 64-bit: the difference of two int32 origins) one of {-8, 0, 8}, and with `crosses` (the cell reaches into the next leaf) one of {-8, 0}?
__device__ __forceinline__ bool near_axis(long long d, bool crosses) { return (unsigned long long)(d + 8) <= (crosses ? 8ull : 16ull); }

// leaf ids under the cell with lower corner (i, j, k), L[di*4+dj*2+dk]: one lookup per DISTINCT leaf (1, 2, 4 or 8: the lower corner on local index 7 along one, two
// or three axes), as far_cell_taps (hns_device.hpp) takes its hash walks
template <bool CURSOR>
__device__ __forceinline__ void cell_leaves(const GridDev& g, Cursor& cur, int i, int j, int k, int (&L)[8]) {
	const int i0 = i & ~7, j0 = j & ~7, k0 = k & ~7;
	const bool cx = (i & 7) == 7, cy = (j & 7) == 7, cz = (k & 7) == 7;
	bool near = false;
	if (CURSOR && cur.leaf >= 0) near = near_axis((long long)i0 - cur.ox, cx) && near_axis((long long)j0 - cur.oy, cy) && near_axis((long long)k0 - cur.oz, cz);
	// near: every leaf under the cell is the cursor's leaf or one of its 26 neighbours. Slot of the lower corner's leaf in the cursor's nbr27 row (13: the cursor's leaf itself)
	const int slot = near ? (((i0 - cur.ox) >> 3) + 1) * 9 + (((j0 - cur.oy) >> 3) + 1) * 3 + ((k0 - cur.oz) >> 3) + 1 : 0;
	const int* __restrict__ row = g.nbr27 + (near ? cur.leaf : 0) * 27;
	// the leaf (a, b, c) leaves up from the lower corner's: the cursor's own id without a load, one load from its row, or a walk through the origin hash
	auto leaf_at = [&](int a, int b, int c) -> int {
		if (near) {
			const int s = slot + a * 9 + b * 3 + c;
			return s == 13 ? cur.leaf : row[s];
		}
		return d_find_leaf(g, a ? plus8(i0) : i0, b ? plus8(j0) : j0, c ? plus8(k0) : k0);
	};
	L[0] = leaf_at(0, 0, 0);
	L[1] = cz ? leaf_at(0, 0, 1) : L[0];
	L[2] = cy ? leaf_at(0, 1, 0) : L[0];
	L[3] = cy ? (cz ? leaf_at(0, 1, 1) : L[2]) : L[1];
	if (cx) {
		L[4] = leaf_at(1, 0, 0);
		L[5] = cz ? leaf_at(1, 0, 1) : L[4];
		L[6] = cy ? leaf_at(1, 1, 0) : L[4];
		L[7] = cy ? (cz ? leaf_at(1, 1, 1) : L[6]) : L[5];
	} else {
		L[4] = L[0], L[5] = L[1], L[6] = L[2], L[7] = L[3];
	}
	if (CURSOR && L[0] >= 0) cur = Cursor{L[0], i0, j0, k0};
}

// Floor (Stencils.hpp:25-43: __float2int_rd -- saturating, NaN -> 0 --, then xyz -= float(ijk)) and the eight corners of TrilinearSampler::stencil (Stencils.hpp:104-114)
template <bool CURSOR>
__device__ __forceinline__ Cell point_cell(const GridDev& g, Cursor& cur, float x, float y, float z) {
	Cell C;
	const int i = __float2int_rd(x), j = __float2int_rd(y), k = __float2int_rd(z);
	C.fx = x - (float)i;
	C.fy = y - (float)j;
	C.fz = z - (float)k;
	int L[8];
	cell_leaves<CURSOR>(g, cur, i, j, k, L);
	const unsigned lx[2] = {((unsigned)i & 7u) << 6, (((unsigned)i + 1u) & 7u) << 6}, ly[2] = {((unsigned)j & 7u) << 3, (((unsigned)j + 1u) & 7u) << 3},
	               lz[2] = {(unsigned)k & 7u, ((unsigned)k + 1u) & 7u};
#pragma unroll
	for (int c = 0; c < 8; ++c) C.t[c] = L[c] < 0 ? -1 : L[c] * 512 + (int)(lx[c >> 2] | ly[(c >> 1) & 1] | lz[c & 1]);
	return C;
}

__device__ __forceinline__ bool finite_f(float a) { return (__float_as_uint(a) & 0x7fffffffu) < 0x7f800000u; }

// ---- the samplers over a Cell: what hns_points.hip and hns_points_collide.hip share ------------------------------------------------------------------------------------

// value or 0 outside the domain (IndexSampler<float,0>, Stencils.hpp:81-89) without a branch: the eight taps of a sample are issued together. (Reads element 0 for an
// absent leaf: the launchers keep empty grids away from the kernels.)
__device__ __forceinline__ float ldz(const float* __restrict__ f, int idx) {
	const float v = f[idx < 0 ? 0 : idx];
	return idx < 0 ? 0.0f : v;
}

// IndexSampler<float,1>: the nest z, y, x with the unfused lerp
__device__ __forceinline__ float sample_f(const float* __restrict__ f, const Cell& C) {
	float c[8];
#pragma unroll
	for (int q = 0; q < 8; ++q) c[q] = ldz(f, C.t[q]);
	return tri_nest(c, C.fx, C.fy, C.fz, lerp_f);
}

// IndexSampler<Vec3f,1> on the device branch (Stencils.hpp:131-135): the same nest per component with fmaf(w, b - a, a); eight 12-byte taps
__device__ __forceinline__ f3 sample_v(const float* __restrict__ u, const Cell& C) {
	float x[8], y[8], z[8];
#pragma unroll
	for (int q = 0; q < 8; ++q) {
		const f3 c = ld3z(u, C.t[q]);
		x[q] = c.x, y[q] = c.y, z[q] = c.z;
	}
	return f3{tri_nest(x, C.fx, C.fy, C.fz, lerp_c), tri_nest(y, C.fx, C.fy, C.fz, lerp_c), tri_nest(z, C.fx, C.fy, C.fz, lerp_c)};
}

// ---- point values into fields: what hns_splat.hip and hns_rasterize.hip share ----------------------------------------------------------------------------------------

constexpr int kSplatChannels = 4;   // channels one launch accumulates: the channels of a voxel's piece of the accumulator (32 bytes: one L2 sector pair)
constexpr int kSplatBlock = 256;

// one component of a field and of its point values: element e of either is at [e * stride + off] (a float field: 1, 0; component c of a Vec3f AoS field: 3, c).
// val null: the weight channel W of an average (every point's value is 1.0f, no field)
struct SplatChannel {
	const float* val;
	float* field;
	int stride, off;
	int wide;  // finish: the field is a 16-byte aligned float array, four voxels per access
};
// the channels of one pass. average: channel 0 is W and the finish divides channels 1 .. n - 1 by it
struct SplatChannels {
	SplatChannel c[kSplatChannels];
	int n;
	int average;
	float min_weight;
};

// The arithmetic, stated once for the kernels and the host mirror (-ffp-contract=off: every line is one rounded operation; include/hns.h states it in words).

// trilinear: w[di*4+dj*2+dk] = (wx[di] * wy[dj]) * wz[dk]
__host__ __device__ inline void splat_weights(float fx, float fy, float fz, float (&w)[8]) {
	const float wx[2] = {1.0f - fx, fx}, wy[2] = {1.0f - fy, fy}, wz[2] = {1.0f - fz, fz};
	for (int c = 0; c < 8; ++c) w[c] = (wx[c >> 2] * wy[(c >> 1) & 1]) * wz[c & 1];
}

// radial: does a point with radius r rasterise under the spec's bound? (a NaN fails every comparison)
__host__ __device__ inline bool radial_point(float x, float y, float z, float r, float bound) { return seeds_f(x) && seeds_f(y) && seeds_f(z) && 0.0f < r && r <= bound; }
// the box of candidates along one axis: lo .. lo + E - 1 (a rasterising point: the floor is exact and fits an int; r <= 4: E <= 8)
__host__ __device__ inline int radial_extent(float r) { return (int)ceilf(2.0f * r); }
__host__ __device__ inline int radial_lo(float c, float r) {
	const float low = c - r;
	return (int)floorf(low) + 1;
}
// (radial_inv and radial_weight, the footprint's weight: hns_radial.hpp)

// Is the term t accepted, and as which multiple of the quantum? scale = 2^-Q: the product is exact in f64 (a power of two, |t| < 2^128, scale <= 2^40), so the test is the
// header's "t finite and |t| * 2^-Q < 2^62" (a NaN and an inf fail the comparison), and k = rint of it, ties to even.
__host__ __device__ inline bool splat_term(float t, double scale, long long* k) {
	const double x = (double)t * scale;
	if (!(fabs(x) < 0x1p62)) return false;
#ifdef __HIP_DEVICE_COMPILE__
	*k = __double2ll_rn(x);
#else
	*k = (long long)std::nearbyint(x);  // (the default rounding mode: to nearest, ties to even)
#endif
	return true;
}

// (splat_total, what a non-zero accumulator adds to its voxel: hns_radial.hpp)

// average: what a voxel with the non-zero weight accumulator a_w becomes
__host__ __device__ inline float splat_average(unsigned long long a_v, unsigned long long a_w, double quantum, float min_weight) {
	const float wsum = splat_total(a_w, quantum), vsum = splat_total(a_v, quantum);
	const float den = fmaxf(wsum, min_weight);
	return vsum / den;
}

// The finish rule, stated once for k_splat_finish, the leaf kernel of hns_splat_binned.hip and the host mirror. a_v: the channel's accumulator of a voxel; a_w: the weight
// channel's (read in average mode only). The gate says whether the voxel changes at all: the channel's own accumulator, or W.
__host__ __device__ inline unsigned long long splat_gate(int average, unsigned long long a_v, unsigned long long a_w) { return average ? a_w : a_v; }
// what a voxel whose gate is non-zero becomes, `old` being what it holds
__host__ __device__ inline float splat_finished(int average, float old, unsigned long long a_v, unsigned long long a_w, double quantum, float min_weight) {
	return average ? splat_average(a_v, a_w, quantum, min_weight) : old + splat_total(a_v, quantum);
}
// one voxel of one channel: *f changes iff the gate is non-zero (every other voxel keeps its bytes: -0.0f stays)
__host__ __device__ inline void splat_finish(int average, unsigned long long a_v, unsigned long long a_w, double quantum, float min_weight, float* f) {
	if (splat_gate(average, a_v, a_w)) *f = splat_finished(average, *f, a_v, a_w, quantum, min_weight);
}

// hns_rasterize.hip: lanes of a group that share one point (1, 4, 16 or 64, from the spec's radius), and the radial kernel's launch in place of k_splat_points'
int splat_radial_group(float radius);
void launch_splat_radial(hipStream_t st, const GridDev& g, const SplatChannels& ch, const float* xyz, const float* radii, float bound, unsigned n, double scale,
                         unsigned long long* acc, int S, int* touched, unsigned* masks, unsigned char* status, unsigned long long* rejected);

// hns_splat.hip: what its launcher shares with the ordered one of hns_splat_binned.hip -- the grid's pooled accumulator (int64 channels over all voxels, then a touched
// word per leaf: all zero between calls), the refusals, the passes of a call and the field lists of a sim call
size_t splat_acc_bytes(const hns_grid* g, int channels);
int splat_accumulator(hns_grid* g, int channels, hipStream_t st);
int check_splat_lists(const char* who, const void* fields, const int* ncomp, int n_fields, const void* values, uint64_t n, int log2_quantum);
int check_splat_pointers(const char* who, float* const* fields, int n_fields, const float* xyz, const float* const* values, const void* status, const void* rejected);
std::vector<SplatChannels> splat_passes(const std::vector<SplatChannel>& all, const hns_splat_spec& sp);
int sim_splat_fields(const char* who, const hns_sim* s, const char* const* names, int n_names, const float* velocity_values, const float* const* values,
                     std::vector<float*>& fields, std::vector<const float*>& vals, std::vector<int>& ncomp, std::vector<int>& which);
void sim_splat_wrote(hns_sim* s, const std::vector<int>& which, bool velocity);

}  // namespace hns

// The leaf order of a point set (hns_pointorder.hip makes it; hns_splat_binned.hip and hns_neighbours.hip read perm, keys and leaf_start)
struct hns_point_order {
	hns_grid* grid = nullptr;
	int device = -1;
	uint64_t capacity = 0, n_leaves = 0;
	hipStream_t stream = nullptr;
	// one pooled allocation: the results, the (key, index) ping-pong -- the keys of k_order_keys lie in kb: by the time a pass writes kb they are spent --, and the tables
	hns::Pooled arena;
	uint32_t *perm = nullptr, *keys = nullptr, *ka = nullptr, *ia = nullptr, *kb = nullptr, *ib = nullptr, *leaf_start = nullptr;
	uint32_t *hist = nullptr, *total = nullptr;  // of the running pass: the [digit][tile] table and its row sums
	uint64_t n = 0;
	int level = -1;
	bool sorted = false;
	// the cell table of a voxel-level sort (hns_neighbours.hip): a pooled allocation of its own, drawn by the first call that needs it; stale after every sort
	hns::Pooled cell_start;
	bool cells_fresh = false;
};

namespace hns {

inline int check_order(const hns_point_order* o, const char* who) {
	if (!o) return refuse(who, "null point order");
	return check_grid(o->grid, who);
}

}  // namespace hns
