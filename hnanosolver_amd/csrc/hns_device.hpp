// hns_device.hpp -- device-side helpers shared by the kernel files: topology access (replaces the NanoVDB accessor walk
// of reference src/Utils/Stencils.hpp:51-71), the samplers of Stencils.hpp:74-173, and the collision helpers of
// reference src/Cuda/Kernel.cu:8-74. Arithmetic keeps the reference's association; build with -ffp-contract=off.
#pragma once

#include "hns_originhash.hpp"

namespace hns {

// ---------------------------------------------------------------------------------------------------------------
// topology access on the device
// ---------------------------------------------------------------------------------------------------------------

// the leaf with origin (ox, oy, oz), -1 = none (hns_originhash.hpp)
__device__ __forceinline__ int d_find_leaf(const GridDev& g, int ox, int oy, int oz) { return find_origin(OriginIndex{g.origins, g.hash, g.hash_mask}, ox, oy, oz); }

// Flat index of global voxel (i,j,k), or -1 when its leaf is absent. `org` is the workgroup's leaf origin and s_nbr its
// 27-neighbour table (LDS). Replaces IndexOffsetSampler<0>::offset (reference Stencils.hpp:59-61), minus the +1.
__device__ __forceinline__ int tap_index(const GridDev& g, const int* s_nbr, const int4 org, int i, int j, int k) {
	const int dx = (i >> 3) - (org.x >> 3), dy = (j >> 3) - (org.y >> 3), dz = (k >> 3) - (org.z >> 3);
	int leaf;
	if ((unsigned)(dx + 1) <= 2u && (unsigned)(dy + 1) <= 2u && (unsigned)(dz + 1) <= 2u)
		leaf = s_nbr[(dx + 1) * 9 + (dy + 1) * 3 + (dz + 1)];
	else
		leaf = d_find_leaf(g, i & ~7, j & ~7, k & ~7);
	return leaf < 0 ? -1 : leaf * 512 + (((i & 7) << 6) | ((j & 7) << 3) | (k & 7));
}

// The eight corners of a trilinear cell whose lower corner (i, j, k) lies beyond the 27-leaf neighbourhood of the workgroup's leaf (origin `org`, neighbours `s_nbr` in LDS): a
// back-trace of more than a leaf, |u| dt / dx > 8. Same leaf ids, same indices as eight calls of tap_index; t[di*4 + dj*2 + dk].
// Round 6: up to two leaves away (|u| dt / dx < 16: where a fast plume's back-traces land) the leaf comes out of the neighbour tables in TWO HOPS -- the workgroup's own neighbour
// towards it (LDS), then that neighbour's row of nbr27 (one 4-byte load) -- instead of a walk through the origin hash (hash slot, then the candidate's origin, then the next
// slot: dependent loads, one walk after the other for the 1, 2, 4 or 8 leaves under the cell). The eight table loads are independent and issued together: one round trip. nbr27 rows
// are built from the same hash, so the answer is the hash's; the hash is still asked where the intermediate leaf is absent or the cell lies farther out.
__device__ __forceinline__ void far_cell_taps(const GridDev& g, const int* s_nbr, const int4 org, int i, int j, int k, int (&t)[8]) {
	const int i0 = i & ~7, j0 = j & ~7, k0 = k & ~7;
	// leaf offsets, relative to the workgroup's leaf, of the leaf under the lower corner and (where the cell crosses a leaf face: lower corner on the last voxel) the one above it
	const int ax[2] = {(i0 - org.x) >> 3, ((i0 - org.x) >> 3) + ((i & 7) == 7)}, ay[2] = {(j0 - org.y) >> 3, ((j0 - org.y) >> 3) + ((j & 7) == 7)},
	          az[2] = {(k0 - org.z) >> 3, ((k0 - org.z) >> 3) + ((k & 7) == 7)};
	int L[8];
#pragma unroll
	for (int c = 0; c < 8; ++c) {
		const int a = ax[c >> 2], b = ay[(c >> 1) & 1], d = az[c & 1];
		const int a1 = max(-1, min(1, a)), b1 = max(-1, min(1, b)), d1 = max(-1, min(1, d));
		const bool two = max(max(abs(a), abs(b)), abs(d)) <= 2;
		const int n1 = two ? s_nbr[(a1 + 1) * 9 + (b1 + 1) * 3 + (d1 + 1)] : -1;
		L[c] = n1 >= 0 ? g.nbr27[n1 * 27 + (a - a1 + 1) * 9 + (b - b1 + 1) * 3 + (d - d1 + 1)] : -2;  // (-2: not in the tables' reach)
	}
	bool hash = false;
#pragma unroll
	for (int c = 0; c < 8; ++c) hash |= L[c] == -2;
	if (hash) {  // one walk per DISTINCT leaf under the cell: in two cells out of three all eight corners share one leaf
		const bool cx = (i & 7) == 7, cy = (j & 7) == 7, cz = (k & 7) == 7;
		L[0] = d_find_leaf(g, i0, j0, k0);
		L[1] = cz ? d_find_leaf(g, i0, j0, k0 + 8) : L[0];
		L[2] = cy ? d_find_leaf(g, i0, j0 + 8, k0) : L[0];
		L[3] = cy ? (cz ? d_find_leaf(g, i0, j0 + 8, k0 + 8) : L[2]) : L[1];
		if (cx) {
			L[4] = d_find_leaf(g, i0 + 8, j0, k0);
			L[5] = cz ? d_find_leaf(g, i0 + 8, j0, k0 + 8) : L[4];
			L[6] = cy ? d_find_leaf(g, i0 + 8, j0 + 8, k0) : L[4];
			L[7] = cy ? (cz ? d_find_leaf(g, i0 + 8, j0 + 8, k0 + 8) : L[6]) : L[5];
		} else {
			L[4] = L[0], L[5] = L[1], L[6] = L[2], L[7] = L[3];
		}
	}
#pragma unroll
	for (int c = 0; c < 8; ++c) {
		const int di = c >> 2, dj = (c >> 1) & 1, dk = c & 1;
		const int leaf = L[c];  // (corner c lies in the leaf of the same index: where an axis does not cross, L[] repeats the lower leaf)
		t[c] = leaf < 0 ? -1 : leaf * 512 + ((((i + di) & 7) << 6) | (((j + dj) & 7) << 3) | ((k + dk) & 7));
	}
}

// IndexSampler<float,0> (Stencils.hpp:81-89): value, or 0 outside the domain
__device__ __forceinline__ float ld0(const float* __restrict__ f, int idx) { return idx < 0 ? 0.0f : f[idx]; }

struct f3 {
	float x, y, z;
};

// float lerp of TrilinearSampler (Stencils.hpp:140): a + w*(b-a), unfused
__device__ __forceinline__ float lerp_f(float a, float b, float w) { return a + w * (b - a); }
// Vec3f lerp on the device branch (Stencils.hpp:131-135): fmaf(w, b-a, a)
__device__ __forceinline__ float lerp_c(float a, float b, float w) { return __fmaf_rn(w, b - a, a); }

// TrilinearSampler's nest, z then y then x (Stencils.hpp:140-152), over the corners c[di*4+dj*2+dk] with one of the three lerps: lerp_f (IndexSampler<float,1>: unfused
// a + w*(b-a)), lerp_c (IndexSampler<Vec3f,1> on the device branch: per component fmaf(w, b-a, a), Stencils.hpp:131-135) or hns_advect.hip's lerp_v3 (the same on a register pair)
template <class T, class Lerp>
__device__ __forceinline__ T tri_nest_yx(const T (&z)[4], float fx, float fy, Lerp lerp) {  // (from the four z columns on: the look-ahead kernel forms those as its taps arrive)
	const T y0 = lerp(z[0], z[1], fy), y1 = lerp(z[2], z[3], fy);
	return lerp(y0, y1, fx);
}
template <class T, class Lerp>
__device__ __forceinline__ T tri_nest(const T (&c)[8], float fx, float fy, float fz, Lerp lerp) {
	const T z[4] = {lerp(c[0], c[1], fz), lerp(c[2], c[3], fz), lerp(c[4], c[5], fz), lerp(c[6], c[7], fz)};
	return tri_nest_yx(z, fx, fy, lerp);
}

// ---- raw buffer access ---------------------------------------------------------------------------------------------
// A buffer descriptor over a field takes a 32-bit byte offset, and the hardware bounds-checks it: a load at or past the
// descriptor's end returns 0 without touching memory and a store there is dropped. hns_advect.hip (which see: "32-bit addressed
// field access"), hns_sorblock.hip and hns_regrid.hip build on that.
typedef float v2f32 __attribute__((ext_vector_type(2)));
typedef float v3f __attribute__((ext_vector_type(3)));
typedef float v4f32 __attribute__((ext_vector_type(4)));
typedef int v4i __attribute__((ext_vector_type(4)));
// through the LLVM intrinsics (this toolchain's __builtin_amdgcn_raw_buffer_load_b96 returns one dword)
__device__ float hns_buffer_load_f32(v4i rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.load.f32");
__device__ v2f32 hns_buffer_load_v2f32(v4i rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.load.v2f32");
__device__ v3f hns_buffer_load_v3f32(v4i rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.load.v3f32");
__device__ v4f32 hns_buffer_load_v4f32(v4i rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.load.v4f32");
__device__ void hns_buffer_store_v4f32(v4f32 data, v4i rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.store.v4f32");

__device__ __forceinline__ v4i field_rsrc(const float* p, unsigned bytes) {
	const unsigned long long a = (unsigned long long)p;
	v4i r;
	r.x = __builtin_amdgcn_readfirstlane((int)(unsigned)a);
	r.y = __builtin_amdgcn_readfirstlane((int)((unsigned)(a >> 32) & 0xffffu));  // stride 0: raw buffer
	r.z = __builtin_amdgcn_readfirstlane((int)bytes);                            // num_records in bytes: offsets at or past it read 0 / are not stored
	r.w = 0x00020000;                                                            // 32-bit float data format
	return r;
}

// One wave over one leaf of a field, voxel 64k + lane in round k (hns_regrid.hip: k_deactivate; hns_diagnostics.hip: k_field_stats). The descriptor covers the leaf alone
// (as in hns_advect.hip): a round to skip gets an offset past the descriptor's end, for which the hardware returns 0 without touching memory. So the eight rounds'
// loads are issued back to back with no branch (a branch per round makes the compiler wait for each load before the next). A leaf's 64 mask bytes are eight 64-bit
// words, word k = voxels 64k .. 64k + 63, loaded by lanes 0..7 and handed to the wave through readlane.
constexpr int kActSkip = 0x40000000;  // a byte offset past any leaf

__device__ __forceinline__ uint64_t readlane64(uint64_t v, int lane) {
	const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
	return (uint64_t)hi << 32 | lo;
}

// OR of `bits` over the lanes for which `take` holds, in every lane (two 32-bit butterflies)
__device__ __forceinline__ uint64_t wave_or64(uint64_t bits, bool take) {
	uint32_t lo = take ? (uint32_t)bits : 0u, hi = take ? (uint32_t)(bits >> 32) : 0u;
#pragma unroll
	for (int w = 32; w >= 1; w >>= 1) {
		lo |= (uint32_t)__shfl_xor((int)lo, w);
		hi |= (uint32_t)__shfl_xor((int)hi, w);
	}
	return (uint64_t)hi << 32 | lo;
}

// ---- launch order ------------------------------------------------------------------------------------------------
// Block -> leaf order. The dispatcher places workgroup b on XCD b % 8 (observed, not contractual), each XCD has a
// private 4 MiB L2, and a leaf's halo is its neighbours' payload: every XCD gets one contiguous chunk of the leaf
// list (sizes differ by at most one leaf), so halo reads hit the L2 that already holds those leaves. Speed only; any
// order is correct. Option "schedule" = linear disables it.
// `seg`: leaves per contiguous segment; consecutive segments go to consecutive XCDs. seg = 1 is plain leaf order, seg <= 0
// (or >= n/8) one chunk per XCD; in between, the eight XCDs walk through neighbouring stretches of memory together (DRAM
// pages, Infinity Cache) while a leaf's z / y neighbours still sit in its own L2.
__host__ __device__ inline int sched_leaf(int b, int n, int seg) {
	if (seg == 1) return b;
	int body = 0;
	if (seg > 1) {
		const int rows = n / (8 * seg);
		body = rows * 8 * seg;
		if (b < body) {
			const int x = b & 7, i = b >> 3;
			return ((i / seg) * 8 + x) * seg + i % seg;
		}
		b -= body, n -= body;
	}
	const int base = n >> 3, rem = n & 7;
	const int x = b & 7, i = b >> 3;  // rows i < base hold all eight XCDs; the last row only x < rem, and b - 8*base == x there
	return body + x * base + (x < rem ? x : rem) + i;
}

// `pre` (a multiple of 8, 0 = none): the first `pre` leaves are dealt out first, an equal contiguous piece to every XCD, the rest
// as above behind them -- a multi-GPU rank's boundary leaves (first in its leaf order) then run on all eight XCDs instead of
// filling the head of XCD 0's chunk (hns_dist_*.hip: their waves poll and signal, and are slower than the others).
__host__ __device__ inline int sched_leaf(int b, int n, int seg, int pre) {
	if (pre <= 0) return sched_leaf(b, n, seg);
	if (b < pre) return (b & 7) * (pre >> 3) + (b >> 3);
	return pre + sched_leaf(b - pre, n - pre, seg);
}


// ---- face-neighbour values through LDS ------------------------------------------------------------------------------
// Kernels that need the six face neighbours of every voxel of a leaf (BFECC clamps, pressure gradient) would issue six
// wave-wide loads per thread, and on gfx950 the L1 charges a load instruction 16 cycles per wave whatever it touches. A
// 512-thread workgroup instead stages a tile: its own 512 values plus the six 8x8 face layers of the neighbouring
// leaves (384 values, one per thread of the first six waves), and every thread reads its neighbours from LDS, branch-free.
// Tile entry e: [0,512) own voxel n; 512 + 64*f + (a*8+b): face layer f (-x,+x,-y,+y,-z,+z) of the neighbouring leaf,
// (a,b) = the two other coordinates in x,y,z order.
constexpr int kTile = 512 + 6 * 64;

// halo entry h in [0,384): slot of the neighbour leaf in the 27-table and the voxel of that leaf to fetch
__device__ __forceinline__ void halo_entry(int h, int& slot, int& local) {
	const int f = h >> 6, a = (h >> 3) & 7, b = h & 7;
	const int axis = f >> 1, dir = (f & 1) ? 1 : -1;
	const int c = dir > 0 ? 0 : 7;  // the layer of the neighbour that touches our face
	slot = 13 + dir * (axis == 0 ? 9 : (axis == 1 ? 3 : 1));
	local = axis == 0 ? ((c << 6) | (a << 3) | b) : (axis == 1 ? ((a << 6) | (c << 3) | b) : ((a << 6) | (b << 3) | c));
}

template <int AXIS, int DIR>
__device__ __forceinline__ int tile_nbr(int n) {  // tile entry of the face neighbour of own voxel n
	constexpr int shift = AXIS == 0 ? 6 : (AXIS == 1 ? 3 : 0);
	constexpr int f = 2 * AXIS + (DIR > 0 ? 1 : 0);
	const int c = (n >> shift) & 7;
	const bool inside = DIR > 0 ? c != 7 : c != 0;
	const int x = n >> 6, y = (n >> 3) & 7, z = n & 7;
	const int ab = AXIS == 0 ? ((y << 3) | z) : (AXIS == 1 ? ((x << 3) | z) : ((x << 3) | y));
	return inside ? n + DIR * (1 << shift) : 512 + 64 * f + ab;
}

// The Gauss-Seidel value of a voxel in the reference's association (Kernel.cu:621) with the product divVal * dx2 passed in: the temporally blocked sweeps carry
// it already multiplied (hns_sorblock.hip: sb_update)
__device__ __forceinline__ float gs_value_of(float pxp, float pxm, float pyp, float pym, float pzp, float pzm, float div_dx2) {
	constexpr float inv6 = 0.166666667f;  // Kernel.cu:609
	return ((pxp + pxm + pyp + pym + pzp + pzm) - div_dx2) * inv6;
}
// The same from divVal and dx2: what the sweep relaxes p towards (sor_update below), what the residual measures p against (hns_diagnostics.hip: k_residual) and
// what the V-cycle restricts (hns_multigrid.hip: k_mg_restrict)
__device__ __forceinline__ float gs_value(float pxp, float pxm, float pyp, float pym, float pzp, float pzm, float divVal, float dx2) { return gs_value_of(pxp, pxm, pyp, pym, pzp, pzm, divVal * dx2); }

// One relaxed Gauss-Seidel update (Kernel.cu:621-622): every sweep of hns_pressure.hip and hns_multigrid.hip
__device__ __forceinline__ float sor_update(float pxp, float pxm, float pyp, float pym, float pzp, float pzm, float divVal, float pOld, float dx2, float omega) {
	const float pGS = gs_value(pxp, pxm, pyp, pym, pzp, pzm, divVal, dx2);  // Kernel.cu:621
	return pOld + omega * (pGS - pOld);                                      // Kernel.cu:622
}

// One wave stages a whole tile of float field p for the leaf of launch record `rec` ({leaf, nbr27[27]}: GridDev::blk): its own values as two 16-byte
// loads per lane, each face layer as one value per lane, 0 where the neighbour leaf is absent. The caller synchronises before it reads P.
// (k_subtract_gradient_s and k_residual)
__device__ __forceinline__ void stage_tile_wave(float* P, const float* __restrict__ p, const int* __restrict__ rec, int leaf, int l) {
	{
		const float4* q = reinterpret_cast<const float4*>(p + (size_t)leaf * 512 + l * 8);
		const float4 a = q[0], b = q[1];
		*reinterpret_cast<float4*>(&P[l * 8]) = a;
		*reinterpret_cast<float4*>(&P[l * 8 + 4]) = b;
	}
#pragma unroll
	for (int f = 0; f < 6; ++f) {  // face f: -x,+x,-y,+y,-z,+z; its 64 entries are one per lane
		int slot, local;
		halo_entry(f * 64 + l, slot, local);
		const int nb = __builtin_amdgcn_readfirstlane(rec[1 + slot]);
		const float v = p[(size_t)(nb < 0 ? 0 : nb) * 512 + local];
		P[512 + f * 64 + l] = nb < 0 ? 0.0f : v;
	}
}

// Stage the workgroup's leaf id, origin and 27-neighbour table. Returns false for an out-of-range block.
struct LeafCtx {
	int leaf;
	int4 org;
};

__device__ __forceinline__ LeafCtx stage_leaf(const GridDev& g, int* s_nbr, int block) {
	LeafCtx c;
	c.leaf = g.sched ? g.sched[block] : g.first + block;
	c.org = g.origins[c.leaf];
	if (threadIdx.x < 27) s_nbr[threadIdx.x] = g.nbr27[c.leaf * 27 + threadIdx.x];
	__syncthreads();
	return c;
}

// ---------------------------------------------------------------------------------------------------------------
// collision helpers (reference Kernel.cu:8-74)
// ---------------------------------------------------------------------------------------------------------------

// the normalised central-difference gradient of the SDF from the six face neighbours' values nb[-x,+x,-y,+y,-z,+z] (0 outside the domain); eps = 1 / voxel size
__device__ __forceinline__ f3 sdf_normal_of(const float (&nb)[6], float eps) {
	const float s = 0.5f * eps;
	f3 gr = {s * (nb[1] - nb[0]), s * (nb[3] - nb[2]), s * (nb[5] - nb[4])};
	const float len = sqrtf(gr.x * gr.x + gr.y * gr.y + gr.z * gr.z);
	if (len > 1e-6f) {
		const float inv = 1.0f / len;
		gr.x = inv * gr.x;
		gr.y = inv * gr.y;
		gr.z = inv * gr.z;
	} else {
		gr.x = gr.y = gr.z = 0.0f;
	}
	return gr;
}

__device__ __forceinline__ f3 sdf_normal(const GridDev& g, const int* s_nbr, const int4 org, const float* __restrict__ sdf, int i, int j, int k,
                                         float eps) {
	const float right = ld0(sdf, tap_index(g, s_nbr, org, i + 1, j, k));
	const float left = ld0(sdf, tap_index(g, s_nbr, org, i - 1, j, k));
	const float top = ld0(sdf, tap_index(g, s_nbr, org, i, j + 1, k));
	const float bottom = ld0(sdf, tap_index(g, s_nbr, org, i, j - 1, k));
	const float front = ld0(sdf, tap_index(g, s_nbr, org, i, j, k + 1));
	const float back = ld0(sdf, tap_index(g, s_nbr, org, i, j, k - 1));
	const float nb[6] = {left, right, bottom, top, back, front};
	return sdf_normal_of(nb, eps);
}

__device__ __forceinline__ f3 no_slip_blend(f3 v, f3 n, float blend) {
	// applyNoSlipBoundary (Kernel.cu:57-74) then v*(1-blend) + no_slip*blend (Kernel.cu:114,448,824)
	const float vdotn = v.x * n.x + v.y * n.y + v.z * n.z;
	const f3 t = {v.x - vdotn * n.x, v.y - vdotn * n.y, v.z - vdotn * n.z};
	const float a = 1.0f - blend;
	f3 r = {a * v.x + blend * t.x, a * v.y + blend * t.y, a * v.z + blend * t.z};
	return r;
}


// ---------------------------------------------------------------------------------------------------------------
// 6-neighbour access of a leaf-dense float field for thread n of the leaf's workgroup
// ---------------------------------------------------------------------------------------------------------------

// value at (x+dx, y+dy, z+dz) for a unit step along one axis; faces resolve through the neighbour table
template <int AXIS, int DIR>
__device__ __forceinline__ float nbr_val(const float* __restrict__ f, const int* s_nbr, int leaf, int n) {
	constexpr int shift = AXIS == 0 ? 6 : (AXIS == 1 ? 3 : 0);
	constexpr int stride = 1 << shift;
	const int c = (n >> shift) & 7;
	if (DIR > 0) {
		if (c != 7) return f[leaf * 512 + n + stride];
		const int nl = s_nbr[13 + (AXIS == 0 ? 9 : (AXIS == 1 ? 3 : 1))];
		return nl < 0 ? 0.0f : f[nl * 512 + n - 7 * stride];
	} else {
		if (c != 0) return f[leaf * 512 + n - stride];
		const int nl = s_nbr[13 - (AXIS == 0 ? 9 : (AXIS == 1 ? 3 : 1))];
		return nl < 0 ? 0.0f : f[nl * 512 + n + 7 * stride];
	}
}


// Vec3f element idx of an AoS velocity array (12-byte stride, exactly the reference's nanovdb::Vec3f[]): one 12-byte access
__device__ __forceinline__ f3 ld3(const float* u, int idx) {
	const float3 v = *reinterpret_cast<const float3*>(u + 3 * (size_t)idx);
	f3 r = {v.x, v.y, v.z};
	return r;
}
__device__ __forceinline__ f3 ld3z(const float* u, int idx) {  // zero outside the domain (IndexSampler<Vec3f,0>)
	const f3 v = ld3(u, idx < 0 ? 0 : idx);
	f3 r = {idx < 0 ? 0.0f : v.x, idx < 0 ? 0.0f : v.y, idx < 0 ? 0.0f : v.z};
	return r;
}
__device__ __forceinline__ void st3(float* u, int idx, f3 v) { *reinterpret_cast<float3*>(u + 3 * (size_t)idx) = make_float3(v.x, v.y, v.z); }

// component COMP of the velocity at the face neighbour of voxel n along AXIS (0 outside the domain)
template <int AXIS, int DIR, int COMP>
__device__ __forceinline__ float nbr_val3(const float* __restrict__ u, const int* s_nbr, int leaf, int n) {
	constexpr int shift = AXIS == 0 ? 6 : (AXIS == 1 ? 3 : 0);
	constexpr int stride = 1 << shift;
	const int c = (n >> shift) & 7;
	if (DIR > 0) {
		if (c != 7) return u[3 * (size_t)(leaf * 512 + n + stride) + COMP];
		const int nl = s_nbr[13 + (AXIS == 0 ? 9 : (AXIS == 1 ? 3 : 1))];
		return nl < 0 ? 0.0f : u[3 * (size_t)(nl * 512 + n - 7 * stride) + COMP];
	} else {
		if (c != 0) return u[3 * (size_t)(leaf * 512 + n - stride) + COMP];
		const int nl = s_nbr[13 - (AXIS == 0 ? 9 : (AXIS == 1 ? 3 : 1))];
		return nl < 0 ? 0.0f : u[3 * (size_t)(nl * 512 + n + 7 * stride) + COMP];
	}
}

// ---------------------------------------------------------------------------------------------------------------
// the projection's reference expressions, each stated once (hns_pressure.hip, hns_pointwise.hip, hns_multigrid.hip)
// ---------------------------------------------------------------------------------------------------------------

// LDS written by this wave is visible to this wave
__device__ __forceinline__ void wave_sync() {
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// divergence of one voxel (Kernel.cu:499-519) from its centre velocity c and the six face values: u.x at +-x, u.y at +-y, u.z at +-z (0 outside the domain)
__device__ __forceinline__ float divergence_of(f3 c, float uxp, float uxm, float uyp, float uym, float uzp, float uzm, float inv_dx) {
	const float xp = (c.x + uxp) * 0.5f, xm = (c.x + uxm) * 0.5f;
	const float yp = (c.y + uyp) * 0.5f, ym = (c.y + uym) * 0.5f;
	const float zp = (c.z + uzp) * 0.5f, zm = (c.z + uzm) * 0.5f;
	return (xp - xm + yp - ym + zp - zm) * inv_dx;
}

// one component of the central pressure gradient (Kernel.cu:795-801)
__device__ __forceinline__ float central_gradient(float p_plus, float p_minus, float inv_dx) { return ((p_plus - p_minus) * 0.5f) * inv_dx; }

// combustion_oxygen of one voxel (Kernel.cu:923-966): the four new fields, the burn amount and whether the voxel burns at all (no oxygen left: it passes through, and
// `burn` is not to be used). Branch-free -- selects between bit-exact alternatives -- as the fused divergence launch needs it (hns_pressure.hip: fused_epilogue).
struct Burnt { float fuel, waste, temperature, flame, burn; bool burns; };
__device__ __forceinline__ Burnt combust_voxel(float fuel, float waste, float temperature, float flame, float temp_gain) {
	const float fu = fuel < 0.001f ? 0.0f : fuel;  // :936-938
	const float oxy = 1.0f - fu - waste;           // :941
	const bool burns = !(oxy < 0.0f);              // :942-949
	const float burn = fminf(oxy, fu);             // :952
	const float te = burns ? temperature + burn * temp_gain : temperature;
	return {burns ? fu - burn : fu, burns ? waste + burn * 2.0f : waste, te, burns ? fmaxf(flame, fminf(1.0f, burn * 10.0f)) : flame, burn, burns};
}
// what combustion leaves of a divergence d (Kernel.cu:964)
__device__ __forceinline__ float combust_divergence(const Burnt& b, float d, float expansion) { return b.burns ? d + b.burn * expansion : d; }

// temperature_buoyancy of one voxel (Kernel.cu:831-847): vel + (0, max(0, (T - Tamb) * k), 0) * dt where T > Tamb. The x and z results are vel + 0 * dt; they go
// through the same add so that the stored bits equal the reference's (-0 + 0 = +0). Branch-free, as combust_voxel.
__device__ __forceinline__ f3 buoyancy_voxel(f3 v, float t, float dt, float ambient, float strength) {
	const bool hot = !(t <= ambient);
	const float tempDiff = t - ambient;
	const float bx = v.x + dt * 0.0f, by = v.y + dt * fmaxf(0.0f, tempDiff * strength), bz = v.z + dt * 0.0f;
	return {hot ? bx : v.x, hot ? by : v.y, hot ? bz : v.z};
}

// is voxel v of leaf `leaf` an unknown? masks: 64 bytes per leaf, byte x*8+y, bit z; null = every voxel (hns_multigrid.hip)
__device__ __forceinline__ bool is_unknown(const unsigned char* __restrict__ masks, int leaf, int v) { return !masks || ((masks[(size_t)leaf * 64 + (v >> 3)] >> (v & 7)) & 1); }

// One colour of one red-black iteration in place (Kernel.cu:591-623 / :521-588), a 256-thread workgroup per leaf, one thread per voxel of the colour.
// MASKED: on unknowns only -- a voxel whose mask bit is clear keeps its 0 (k_mg_color); else every voxel (k_rbgs_color).
template <bool MASKED>
__device__ __forceinline__ void color_sweep(const GridDev& g, int* s_nbr, const unsigned char* __restrict__ masks, const float* __restrict__ div, float* p, float dx2,
                                            float omega, int color) {
	const LeafCtx L = stage_leaf(g, s_nbr, blockIdx.x);
	const int t = threadIdx.x, x = t >> 5, y = (t >> 2) & 7;
	const int z = 2 * (t & 3) + ((x + y + color) & 1);  // origins are 8-aligned, so global parity == local parity
	const int n = (x << 6) | (y << 3) | z;
	if (MASKED && !is_unknown(masks, L.leaf, n)) return;
	const int idx = L.leaf * 512 + n;
	const float pxp = nbr_val<0, 1>(p, s_nbr, L.leaf, n), pxm = nbr_val<0, -1>(p, s_nbr, L.leaf, n);
	const float pyp = nbr_val<1, 1>(p, s_nbr, L.leaf, n), pym = nbr_val<1, -1>(p, s_nbr, L.leaf, n);
	const float pzp = nbr_val<2, 1>(p, s_nbr, L.leaf, n), pzm = nbr_val<2, -1>(p, s_nbr, L.leaf, n);
	p[idx] = sor_update(pxp, pxm, pyp, pym, pzp, pzm, div[idx], p[idx], dx2, omega);
}

}  // namespace hns

// ---- launcher plumbing shared by the kernel files ----

inline int check_grid(const hns_grid* g, const char* who) {
	if (!g) {
		hns::set_error("%s: null grid", who);
		return HNS_ERR_INVALID_ARGUMENT;
	}
	if (!g->on_device) {
		hns::set_error("%s: grid has no device tables (host-only grid or no HIP device); there is no CPU fallback", who);
		return HNS_ERR_NO_DEVICE;
	}
	int cur = -1;
	if (hipGetDevice(&cur) != hipSuccess || cur != g->device) {  // launches go to the CURRENT device; the grid's tables live on g->device
		hns::set_error("%s: the grid lives on HIP device %d but device %d is current in this thread", who, g->device, cur);
		return HNS_ERR_INVALID_ARGUMENT;
	}
	return HNS_OK;
}

inline int launch_status(const char* who) {
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) {
		hns::set_error("%s: kernel launch failed: %s", who, hipGetErrorString(e));
		return HNS_ERR_HIP;
	}
	return HNS_OK;
}

inline unsigned ew_blocks(uint64_t n) {
	uint64_t b = (n + 255) / 256;
	return (unsigned)(b < 1 ? 1 : (b > 16384 ? 16384 : b));
}

#define NULLCHK(cond, who)                                \
	if (cond) {                                           \
		hns::set_error("%s: null device pointer", who);        \
		return HNS_ERR_INVALID_ARGUMENT;                  \
	}

