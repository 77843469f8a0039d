// hns_points.hpp -- the trilinear cell under an index-space position, shared by the kernel files that work at points: hns_points.hip (fields read at points, points
// traced through the velocity) and hns_splat.hip (point values added into fields). One statement of Floor, the tap indices and the fractions for both directions.
#pragma once

#include "hns_device.hpp"

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

// ---- launcher plumbing of the point calls ----

inline int refuse(const char* who, const char* what) {
	set_error("%s: %s", who, what);
	return HNS_ERR_INVALID_ARGUMENT;
}

constexpr uint64_t kMaxPoints = 0x7fffffffull;

// a sim the point calls may use: not null (without a device there is none to pass: hns_sim_create refused, and the caller learns why here too), not lent to a cook cache
inline int check_sim(const hns_sim* s, const char* who) {
	if (!s) {
		if (hns_device_count() == 0) {
			set_error("%s: no HIP device (there is no CPU fallback)", who);
			return HNS_ERR_NO_DEVICE;
		}
		return refuse(who, "null sim");
	}
	if (s->cached || s->in_use) return refuse(who, "the sim belongs to a grid's cook cache");
	return HNS_OK;
}

}  // namespace hns
